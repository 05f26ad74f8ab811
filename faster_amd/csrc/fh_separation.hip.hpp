// fh_separation.hip.hpp — the committed plans of a fleet against each other (include/fasterhip_separation.h, which is the
// specification): for every tested instant of every vehicle, the other vehicles nearer than cap.  Reads the vehicle records and the
// plans; writes one fh_plan_separation per vehicle and working buffers of the context.  The broad phase is the cell grid
// (fh_cells.hip.hpp: its launches, why its prefilters lose nothing and where every index comes from), with reach = cap.  Its own:
//   sep_boxes_kernel : one wavefront per vehicle k, lane = tested state.  The plan extent is checked, then the bounding box of the finite
//                      positions k can show to anyone: its states at j = 0, stride, ... < m_k (what it tests itself, and what an other
//                      sees of it while it flies) and its last state when an other can test an instant >= size_k (count == 0 or
//                      size_k < count).  The box, the checked extent and a validity word go into boxes[k].
//   sep_narrow_kernel: one wavefront per vehicle i, one per workgroup.  The candidates of the walk whose box meets box_i grown by
//                      cap + g are compacted into an LDS list (ballot + rank).  When the list cannot take 64 more, or the cells end,
//                      it is tested with lane = state: for every listed k the lane reads plan_k[min(j, size_k - 1)] and keeps the
//                      lexicographic minimum of (d2, j, k) and of (j, k) among the near ones; one ballot per listed k counts n_near.
//                      The record leaves as one 16-byte store from each of lanes 0..3.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fasterhip_separation.h"
#include "fh_cells.hip.hpp"
#include "fh_plans.hip.hpp"
#include "fh_wave.hip.hpp"

namespace fh {

constexpr int SEP_LIST = FH_SEP_LIST_VEHICLES;

enum {               // SepBox.c.valid, above CELL_BOXED
  SEP_GOOD = 2,      // the plan extent fits (not FH_SEP_BAD_PLAN)
  SEP_OTHER = 4,     // good and plan_size >= 1: an other of everyone else
  SEP_NOT_FINITE = 8 // a tested position of its own is not finite
};

struct SepBox {  // 64 B
  CellBox c;
  int head, size;  // the checked plan extent (0, 0 for a bad record)
};

struct SepArgs {
  double r2, cap, cap2;  // r * r and cap * cap, rounded once on the host as the model rounds them
  int stride, count, n, max_states;
  const fh_vehicle* vehicles;
  const fh_state* plans;
  CellGrid g;
  SepBox* boxes;  // [n]
  fh_plan_separation* out;
};

__global__ void __launch_bounds__(64) sep_boxes_kernel(SepArgs a) {
  const int lane = fhw::lane_id();
  const int k = (int)blockIdx.x;
  if (k >= a.n) return;
  const fh_vehicle& V = a.vehicles[k];
  const int head = fhw::uniform_i32(V.plan_head), size = fhw::uniform_i32(V.plan_size);
  const bool bad = plan_bad_extent(head, size, a.max_states);
  int valid = 0, cell = 0;
  double lx = INFINITY, ly = INFINITY, lz = INFINITY, hx = -INFINITY, hy = -INFINITY, hz = -INFINITY;
  if (!bad) {
    valid = SEP_GOOD | (size >= 1 ? SEP_OTHER : 0);
    const int n_tested = plan_instants(plan_limit(a.count, size), a.stride);
    const int rounds = (n_tested + 63) >> 6;
    const fh_state* plan = a.plans + ((size_t)k * (size_t)a.max_states + (size_t)head);
    bool not_finite = false;
    for (int s = 0; s <= rounds; s++) {
      // round `rounds`: lane 0 takes the last state, where the vehicle stands for those that outlast it
      const bool extra = s == rounds;
      if (extra ? !(lane == 0 && size >= 1 && (a.count == 0 || size < a.count)) : s * 64 + lane >= n_tested) continue;
      const double* p = plan[extra ? (size_t)(size - 1) : (size_t)(s * 64 + lane) * (size_t)a.stride].pos;
      const double x = p[0], y = p[1], z = p[2];
      if (plan_finite(x) && plan_finite(y) && plan_finite(z)) {
        plan_box_take(x, y, z, lx, ly, lz, hx, hy, hz);
      } else if (!extra) {
        not_finite = true;
      }
    }
    if (fhw::wave_any(not_finite)) valid |= SEP_NOT_FINITE;
    valid |= cell_box_tail(a.g, lane, lx, ly, lz, hx, hy, hz, cell);
  }
  if (lane == 0) {
    SepBox& b = a.boxes[k];
    cell_box_store(b.c, lx, ly, lz, hx, hy, hz, valid, cell);
    b.head = bad ? 0 : head; b.size = bad ? 0 : size;
  }
}

struct SepBest {  // what one lane has seen
  double d2;
  int j_min, k_min, j_first, k_first;
};

__global__ void __launch_bounds__(64) sep_narrow_kernel(SepArgs a) {
#pragma clang fp contract(off)
  __shared__ int list_k[SEP_LIST], list_head[SEP_LIST], list_size[SEP_LIST];
  const int lane = fhw::lane_id();
  const int i = (int)blockIdx.x;
  if (i >= a.n) return;
  const SepBox& B = a.boxes[i];
  const int valid = fhw::uniform_i32(B.c.valid), head = fhw::uniform_i32(B.head), size = fhw::uniform_i32(B.size);
  int flags = 0, n_tested = 0, first = -1, first_other = -1, worst = -1, worst_other = -1, n_near = 0;
  double min_d2 = INFINITY;
  if (!(valid & SEP_GOOD)) {
    flags = FH_SEP_BAD_PLAN;
  } else {
    n_tested = plan_instants(plan_limit(a.count, size), a.stride);
    const int rounds = (n_tested + 63) >> 6;
    if (valid & SEP_NOT_FINITE) flags |= FH_SEP_NOT_FINITE;
    if ((valid & CELL_BOXED) && n_tested > 0) {
      const fh_state* plan = a.plans + ((size_t)i * (size_t)a.max_states + (size_t)head);
      SepBest best = {INFINITY, 0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff};
      int n_list = 0;  // (uniform)
      cell_walk(a.g, B.c, a.cap, i, a.n, lane, [&](int k, const CellReach& w, bool end) {
        bool keep = false;
        int k_head = 0, k_size = 0;
        if (k >= 0) {
          const SepBox& K = a.boxes[k];
          k_head = K.head; k_size = K.size;
          keep = (K.c.valid & (SEP_OTHER | CELL_BOXED)) == (SEP_OTHER | CELL_BOXED) && cell_meets(K.c, w);
        }
        const unsigned long long km = __ballot(keep);
        if (keep) {
          const int slot = n_list + fhw::rank_in(km);
          list_k[slot] = k; list_head[slot] = k_head; list_size[slot] = k_size;
        }
        n_list += (int)__popcll(km);
        if (n_list > SEP_LIST - 64 || end) {
          __syncthreads();
          for (int e = 0; e < n_list; e++) {
            const int k_e = list_k[e], last_e = list_size[e] - 1;
            const fh_state* other = a.plans + ((size_t)k_e * (size_t)a.max_states + (size_t)list_head[e]);
            bool near = false;
            for (int s = 0; s < rounds; s++) {
              const int t = s * 64 + lane;
              if (t >= n_tested) continue;
              const int j = t * a.stride;
              const double* p = plan[j].pos;
              const double px = p[0], py = p[1], pz = p[2];
              if (!(plan_finite(px) && plan_finite(py) && plan_finite(pz))) continue;
              const double* o = other[j < last_e ? j : last_e].pos;
              const double dx = o[0] - px, dy = o[1] - py, dz = o[2] - pz;
              const double d2 = dx * dx + dy * dy + dz * dz;
              if (d2 < a.cap2) {
                if (d2 < best.d2 || (d2 == best.d2 && (j < best.j_min || (j == best.j_min && k_e < best.k_min)))) {
                  best.d2 = d2; best.j_min = j; best.k_min = k_e;
                }
                if (d2 < a.r2) {
                  near = true;
                  if (j < best.j_first || (j == best.j_first && k_e < best.k_first)) { best.j_first = j; best.k_first = k_e; }
                }
              }
            }
            n_near += fhw::wave_any(near) ? 1 : 0;
          }
          __syncthreads();
          n_list = 0;
        }
      });
      // the minimum d2, then the smallest j among the lanes that hold it, then the smallest k among those; the same for first
      min_d2 = fhw::wave_min(best.d2);
      const bool holds = best.d2 == min_d2 && min_d2 < INFINITY;
      worst = fhw::wave_min_i32(holds ? best.j_min : 0x7fffffff);
      worst_other = fhw::wave_min_i32(holds && best.j_min == worst ? best.k_min : 0x7fffffff);
      first = fhw::wave_min_i32(best.j_first);
      first_other = fhw::wave_min_i32(best.j_first == first ? best.k_first : 0x7fffffff);
      if (worst == 0x7fffffff) worst = worst_other = -1;
      if (first == 0x7fffffff) first = first_other = -1;
      if (first >= 0) flags |= FH_SEP_NEAR;
    }
  }
  // words 2 l and 2 l + 1 of the record from lane l < 4: 64 contiguous bytes in one store instruction
  double w0 = 0.0, w1 = 0.0;
  if (lane == 0) { w0 = plan_pack(flags, n_tested); w1 = plan_pack(first, first_other); }
  if (lane == 1) { w0 = plan_pack(worst, worst_other); w1 = plan_pack(n_near, 0); }
  if (lane == 2) { w0 = min_d2; }
  if (lane < 4) reinterpret_cast<double2*>(a.out + i)[lane] = make_double2(w0, w1);
}

}  // namespace fh

// fh_separation.hip.hpp — the committed plans of a fleet against each other (include/fasterhip_separation.h, which is the
// specification): for every tested instant of every vehicle, the other vehicles nearer than cap.  Reads the vehicle records and the
// plans; writes one fh_plan_separation per vehicle and working buffers of the context.  Four launches:
//   sep_boxes_kernel : one wavefront per vehicle k, lane = tested state.  The plan extent is checked, then the bounding box of the finite
//                      positions k can show to anyone: its states at j = 0, stride, ... < m_k (what it tests itself, and what an other
//                      sees of it while it flies) and its last state when an other can test an instant >= size_k (count == 0 or
//                      size_k < count).  The box, the checked extent and a validity word go into boxes[k]; the half-extents go into
//                      the fleet-wide maximum H per axis (atomicMax on the bit pattern of a non-negative double); k is counted into
//                      the cell of its box centre.
//   sep_scan_kernel  : one workgroup, the exclusive scan of the cell counts into starts[0 .. n_cells]; the counts are left zero.
//   sep_fill_kernel  : lane = vehicle: items[starts[cell] + (the count of its cell, drawn again)] = k.  The order inside a cell is
//                      whatever the atomics give; the tie rules make the output independent of it.
//   sep_narrow_kernel: one wavefront per vehicle i, one per workgroup.  The cells whose clamped range covers box_i grown by
//                      cap + g + H: k sits in exactly one cell, that of its centre, and its centre is at most H from any point of its
//                      box.  Cells of one row along x are neighbours in `items`, so a row is one run of vehicles, read 64 at a time,
//                      lane = candidate; box_k is tested against box_i grown by cap + g and the survivors are compacted into an LDS
//                      list (ballot + rank).  When the list cannot take 64 more, or the cells end, it is tested with lane = state: for
//                      every listed k the lane reads plan_k[min(j, size_k - 1)] and keeps the lexicographic minimum of (d2, j, k) and
//                      of (j, k) among the near ones; one ballot per listed k counts n_near.  The record leaves as one 16-byte store
//                      from each of lanes 0..3.
// PREFILTERS ARE CONSERVATIVE.  A pair counts only by its d2, computed as the model writes it; boxes and cells only decide what is
// looked at.  g = 1e-9 (cap + |lo| + |hi|) for the box test and 1e-9 (cap + |lo| + |hi| + H) for the cells: the roundings of
// lo - (cap + g), of the centre, of the half-extent and of d2 are relative 1e-16, seven orders below.  A position becomes a cell
// number by the same monotonic expression for centres and for ranges, after comparisons in double: no NaN, infinity or 1e300 is ever
// converted to int, and an infinite H (a box that overflowed) is every cell.
// Every index comes from a checked record: boxes[k].head / .size are written by sep_boxes_kernel after the extent test, items[] by
// sep_fill_kernel from vehicle numbers < n, and the narrow phase reads plans through those only.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fasterhip_separation.h"
#include "fh_wave.hip.hpp"

namespace fh {

constexpr int SEP_LIST = FH_SEP_LIST_VEHICLES;
constexpr int SEP_SCAN_THREADS = 1024;

enum {               // SepBox.valid
  SEP_GOOD = 1,      // the plan extent fits (not FH_SEP_BAD_PLAN)
  SEP_OTHER = 2,     // good and plan_size >= 1: an other of everyone else
  SEP_BOXED = 4,     // at least one finite position: lo / hi / cell are set and the vehicle is counted into its cell
  SEP_NOT_FINITE = 8 // a tested position of its own is not finite
};

struct SepBox {  // 64 B
  double lo[3], hi[3];
  int valid, head, size, cell;  // head, size: the checked plan extent (0, 0 for a bad record)
};

struct SepArgs {
  double r2, cap, cap2;  // r * r and cap * cap, rounded once on the host as the model rounds them
  int stride, count, n, max_states;
  const fh_vehicle* vehicles;
  const fh_state* plans;
  double ox, oy, oz, res;  // the cell grid
  int nx, ny, nz;
  SepBox* boxes;                  // [n]
  unsigned long long* extent;     // [3]: bit patterns of H per axis
  int* counts;                    // [n_cells]
  int* starts;                    // [n_cells + 1]
  int* items;                     // [n]
  fh_plan_separation* out;
};

__device__ __forceinline__ bool sep_finite(double x) { return fabs(x) < INFINITY; }  // false for a NaN

// The cell of x along one axis (n cells of size res from o), clamped into [0, n - 1]; monotonic in x, and a NaN gives `nan_cell`.
__device__ __forceinline__ int sep_cell(double x, double o, double res, int n, int nan_cell) {
#pragma clang fp contract(off)
  const double f = floor((x - o) / res), last = (double)(n - 1);
  if (f >= 0.0) return f <= last ? (int)f : n - 1;
  return f < 0.0 ? 0 : nan_cell;
}

__device__ __forceinline__ double sep_pack(int lo, int hi) { return __hiloint2double(hi, lo); }

// *word = max(*word, the bit pattern of h) for h >= +0.  The word only grows, so a vehicle that does not exceed what it reads has
// nothing to add: the whole fleet raises three words, and without the look all of its atomics queue up behind each other.
__device__ __forceinline__ void sep_raise(unsigned long long* word, double h) {
  const unsigned long long bits = (unsigned long long)__double_as_longlong(h);
  if (bits > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(word, bits);
}

__global__ void __launch_bounds__(64) sep_boxes_kernel(SepArgs a) {
#pragma clang fp contract(off)
  const int lane = fhw::lane_id();
  const int k = (int)blockIdx.x;
  if (k >= a.n) return;
  const fh_vehicle& V = a.vehicles[k];
  const int head = fhw::uniform_i32(V.plan_head), size = fhw::uniform_i32(V.plan_size);
  const bool bad = head < 0 || size < 0 || (long long)head + (long long)size > (long long)a.max_states;
  int valid = 0, cell = 0;
  double lx = INFINITY, ly = INFINITY, lz = INFINITY, hx = -INFINITY, hy = -INFINITY, hz = -INFINITY;
  if (!bad) {
    valid = SEP_GOOD | (size >= 1 ? SEP_OTHER : 0);
    const int m = a.count > 0 ? min(a.count, size) : size;
    const int n_tested = (int)(((long long)m + a.stride - 1) / a.stride);
    const int rounds = (n_tested + 63) >> 6;
    const fh_state* plan = a.plans + ((size_t)k * (size_t)a.max_states + (size_t)head);
    bool not_finite = false;
    for (int s = 0; s <= rounds; s++) {
      // round `rounds`: lane 0 takes the last state, where the vehicle stands for those that outlast it
      const bool extra = s == rounds;
      if (extra ? !(lane == 0 && size >= 1 && (a.count == 0 || size < a.count)) : s * 64 + lane >= n_tested) continue;
      const double* p = plan[extra ? (size_t)(size - 1) : (size_t)(s * 64 + lane) * (size_t)a.stride].pos;
      const double x = p[0], y = p[1], z = p[2];
      if (sep_finite(x) && sep_finite(y) && sep_finite(z)) {
        lx = x < lx ? x : lx; ly = y < ly ? y : ly; lz = z < lz ? z : lz;
        hx = x > hx ? x : hx; hy = y > hy ? y : hy; hz = z > hz ? z : hz;
      } else if (!extra) {
        not_finite = true;
      }
    }
    if (fhw::wave_any(not_finite)) valid |= SEP_NOT_FINITE;
    lx = fhw::wave_min(lx); ly = fhw::wave_min(ly); lz = fhw::wave_min(lz);
    hx = fhw::wave_max(hx); hy = fhw::wave_max(hy); hz = fhw::wave_max(hz);
    if (lx <= hx) {  // (uniform)
      valid |= SEP_BOXED;
      // centre and half-extent: halves first, so that two coordinates near the largest double do not overflow in the sum
      const int cx = sep_cell(lx * 0.5 + hx * 0.5, a.ox, a.res, a.nx, 0), cy = sep_cell(ly * 0.5 + hy * 0.5, a.oy, a.res, a.ny, 0),
                cz = sep_cell(lz * 0.5 + hz * 0.5, a.oz, a.res, a.nz, 0);
      cell = (cz * a.ny + cy) * a.nx + cx;
      if (lane == 0) {
        // (hi - lo is >= +0 or +INFINITY, never a NaN: the order of the bit patterns is the order of the values)
        sep_raise(a.extent + 0, (hx - lx) * 0.5);
        sep_raise(a.extent + 1, (hy - ly) * 0.5);
        sep_raise(a.extent + 2, (hz - lz) * 0.5);
        atomicAdd(a.counts + cell, 1);
      }
    }
  }
  if (lane == 0) {
    SepBox& b = a.boxes[k];
    b.lo[0] = lx; b.lo[1] = ly; b.lo[2] = lz;
    b.hi[0] = hx; b.hi[1] = hy; b.hi[2] = hz;
    b.valid = valid; b.head = bad ? 0 : head; b.size = bad ? 0 : size; b.cell = cell;
  }
}

// starts[c] = the sum of counts[0 .. c), starts[n_cells] = the total; counts[] is left zero for sep_fill_kernel to draw from.  One
// workgroup: thread t owns the cells [t chunk, (t + 1) chunk).
__global__ void __launch_bounds__(SEP_SCAN_THREADS) sep_scan_kernel(int* __restrict__ counts, int* __restrict__ starts, int n_cells) {
  __shared__ int part[SEP_SCAN_THREADS];
  const int t = (int)threadIdx.x;
  const int chunk = (n_cells + SEP_SCAN_THREADS - 1) / SEP_SCAN_THREADS;
  const int c0 = min(t * chunk, n_cells), c1 = min(c0 + chunk, n_cells);
  int sum = 0;
  for (int c = c0; c < c1; c++) sum += counts[c];
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < SEP_SCAN_THREADS; d <<= 1) {  // inclusive scan of the partial sums
    const int v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - sum;
  for (int c = c0; c < c1; c++) {
    const int v = counts[c];
    starts[c] = run;
    counts[c] = 0;
    run += v;
  }
  if (t == SEP_SCAN_THREADS - 1) starts[n_cells] = part[t];
}

__global__ void __launch_bounds__(256) sep_fill_kernel(SepArgs a) {
  const int k = (int)(blockIdx.x * 256 + threadIdx.x);
  if (k >= a.n) return;
  const SepBox& b = a.boxes[k];
  if (!(b.valid & SEP_BOXED)) return;
  const int slot = a.starts[b.cell] + atomicAdd(a.counts + b.cell, 1);
  if (slot >= 0 && slot < a.n) a.items[slot] = k;  // (always: the boxed vehicles are the ones that were counted)
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
  const int valid = fhw::uniform_i32(B.valid), head = fhw::uniform_i32(B.head), size = fhw::uniform_i32(B.size);
  int flags = 0, n_tested = 0, first = -1, first_other = -1, worst = -1, worst_other = -1, n_near = 0;
  double min_d2 = INFINITY;
  if (!(valid & SEP_GOOD)) {
    flags = FH_SEP_BAD_PLAN;
  } else {
    const int m = a.count > 0 ? min(a.count, size) : size;
    n_tested = (int)(((long long)m + a.stride - 1) / a.stride);
    const int rounds = (n_tested + 63) >> 6;
    if (valid & SEP_NOT_FINITE) flags |= FH_SEP_NOT_FINITE;
    if ((valid & SEP_BOXED) && n_tested > 0) {
      const fh_state* plan = a.plans + ((size_t)i * (size_t)a.max_states + (size_t)head);
      const double lx = fhw::uniform_f64(B.lo[0]), ly = fhw::uniform_f64(B.lo[1]), lz = fhw::uniform_f64(B.lo[2]);
      const double hx = fhw::uniform_f64(B.hi[0]), hy = fhw::uniform_f64(B.hi[1]), hz = fhw::uniform_f64(B.hi[2]);
      const double Hx = __longlong_as_double((long long)a.extent[0]), Hy = __longlong_as_double((long long)a.extent[1]),
                   Hz = __longlong_as_double((long long)a.extent[2]);
      // the box test: box_i grown by cap + g
      const double gx = a.cap + 1e-9 * (a.cap + fabs(lx) + fabs(hx)), gy = a.cap + 1e-9 * (a.cap + fabs(ly) + fabs(hy)),
                   gz = a.cap + 1e-9 * (a.cap + fabs(lz) + fabs(hz));
      const double x0 = lx - gx, x1 = hx + gx, y0 = ly - gy, y1 = hy + gy, z0 = lz - gz, z1 = hz + gz;
      // the cells: grown by cap + g + H, where centres of boxes that pass the box test can lie
      const double wx = (a.cap + 1e-9 * (a.cap + fabs(lx) + fabs(hx) + Hx)) + Hx, wy = (a.cap + 1e-9 * (a.cap + fabs(ly) + fabs(hy) + Hy)) + Hy,
                   wz = (a.cap + 1e-9 * (a.cap + fabs(lz) + fabs(hz) + Hz)) + Hz;
      const int cxa = sep_cell(lx - wx, a.ox, a.res, a.nx, 0), cxb = sep_cell(hx + wx, a.ox, a.res, a.nx, a.nx - 1);
      const int cya = sep_cell(ly - wy, a.oy, a.res, a.ny, 0), cyb = sep_cell(hy + wy, a.oy, a.res, a.ny, a.ny - 1);
      const int cza = sep_cell(lz - wz, a.oz, a.res, a.nz, 0), czb = sep_cell(hz + wz, a.oz, a.res, a.nz, a.nz - 1);
      SepBest best = {INFINITY, 0x7fffffff, 0x7fffffff, 0x7fffffff, 0x7fffffff};
      int n_list = 0;  // (uniform)
      for (int cz = cza; cz <= czb; cz++) {
        for (int cy = cya; cy <= cyb; cy++) {
          const bool last_row = cz == czb && cy == cyb;
          const int row = (cz * a.ny + cy) * a.nx;
          const int s0 = fhw::uniform_i32(a.starts[row + cxa]), s1 = fhw::uniform_i32(a.starts[row + cxb + 1]);
          // (an empty last row still has to flush the list: one turn with no candidate)
          for (int q0 = s0; q0 < s1 || (last_row && q0 == s0); q0 += 64) {
            const int q = q0 + lane;
            bool keep = false;
            int k = -1, k_head = 0, k_size = 0;
            if (q < s1) {
              k = a.items[q];
              if (k >= 0 && k < a.n && k != i) {
                const SepBox& K = a.boxes[k];
                k_head = K.head; k_size = K.size;
                keep = (K.valid & (SEP_OTHER | SEP_BOXED)) == (SEP_OTHER | SEP_BOXED) && K.hi[0] >= x0 && K.lo[0] <= x1 && K.hi[1] >= y0 &&
                       K.lo[1] <= y1 && K.hi[2] >= z0 && K.lo[2] <= z1;
              }
            }
            const unsigned long long km = __ballot(keep);
            if (keep) {
              const int slot = n_list + fhw::rank_in(km);
              list_k[slot] = k; list_head[slot] = k_head; list_size[slot] = k_size;
            }
            n_list += (int)__popcll(km);
            const bool end = last_row && q0 + 64 >= s1;
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
                  if (!(sep_finite(px) && sep_finite(py) && sep_finite(pz))) continue;
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
          }
        }
      }
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
  if (lane == 0) { w0 = sep_pack(flags, n_tested); w1 = sep_pack(first, first_other); }
  if (lane == 1) { w0 = sep_pack(worst, worst_other); w1 = sep_pack(n_near, 0); }
  if (lane == 2) { w0 = min_d2; }
  if (lane < 4) reinterpret_cast<double2*>(a.out + i)[lane] = make_double2(w0, w1);
}

}  // namespace fh

// fh_check.hip.hpp — the commit check of a fleet (include/fasterhip_check.h, which is the specification): every vehicle that committed
// this cycle against what the others flew before the commit (old_k, the backup) and against what the lower candidates fly now (cur_k),
// at equal instants from its first new state on; the commits that conflict are taken back.  The broad phase is the cell grid
// (fh_cells.hip.hpp: its launches, why its prefilters lose nothing and where every index comes from), with reach = r.  Its own:
//   check_backup_kernel : one wavefront per vehicle: the record (35 words of 8 bytes: 280 bytes are no multiple of 16) and the live extent
//                         of the plan, 16 bytes per lane (a state is six of them), to the same indexes of the backup arrays.
//   check_boxes_kernel  : one wavefront per vehicle k, lane = state.  Both extents are checked, candidate and kept_k decided, then the
//                         bounding box of every finite position k can show to anyone: old_k's states (an other of kind 0 of everyone) and,
//                         for a candidate, cur_k's (what it tests itself, and an other of kind 1 of the candidates above it), each up to
//                         `count` and with the last state.  Box, extents, kept and a validity word go into boxes[k].  A box holds every
//                         state of a plan below `count`, not only the strided ones, and the box a candidate asks with is the one it
//                         shows (old and new states): both are supersets of what the pairs read.
//   check_narrow_kernel : one wavefront per vehicle i; a vehicle that is no candidate stores the record of "nothing tested" and is done.
//                         The candidates of the walk whose box meets box_i grown by r + g enter an LDS list as (k, kind, head, size),
//                         kind 0 first (two ballots).  When the list cannot take 128 more, or the cells end, it is tested in rounds of 64 instants,
//                         lane = instant j = kept_i + (64 s + lane) stride: the lane reads its own position once per round and, for
//                         every listed other with j < M, the other's; it keeps the lexicographic minimum of (j, k, kind) with d2 < r r.
//                         A round in which a lane found a conflict is the last one looked at, in this list and in every later one:
//                         the instants of later rounds are larger; and in the lists after it the lanes behind the smallest instant
//                         in conflict so far read nothing: in a dense fleet a listed other then costs a state or two, not 64.  The
//                         record leaves as one 16-byte store from each of lanes 0, 1.
//   check_revert_kernel : one wavefront per vehicle: a record without FH_CHECK_CONFLICT ends it; else the backup's record with stage =
//                         FH_FLEET_STAGE_CONFLICT and the backup's live extent come back, 16 bytes per lane.
// check_backup_kernel and check_revert_kernel test the extent they copy (plan_bad_extent).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>

#include "../../include/fasterhip_check.h"
#include "fh_cells.hip.hpp"
#include "fh_plans.hip.hpp"
#include "fh_wave.hip.hpp"

namespace fh {

constexpr int CHK_LIST = FH_CHECK_LIST_OTHERS;
constexpr int CHK_RECORD_WORDS = (int)(sizeof(fh_vehicle) / 8);
static_assert(sizeof(fh_vehicle) % 8 == 0 && offsetof(fh_vehicle, stage) % 8 == 0, "a vehicle record is copied as words of 8 bytes, stage in the low half of one");
static_assert(sizeof(fh_state) % 16 == 0 && sizeof(fh_plan_check) == 32, "states are copied and records stored 16 bytes per lane");

enum {                 // ChkBox.c.valid, above CELL_BOXED
  CHK_OLD_OTHER = 2,   // the old extent fits and holds a state: old_k is an other of everyone else
  CHK_CANDIDATE = 4,   // committed, active, both extents fit
  CHK_CUR_OTHER = 8,   // a candidate whose new plan holds a state: cur_k is an other of the candidates above k
  CHK_NOT_FINITE = 16, // a candidate: one of its own positions the pairs can read is not finite
  CHK_CLAMPED = 32     // a candidate: kept was outside [0, min(old size, cur size)]
};

struct ChkBox {  // 80 B
  CellBox c;
  int old_head, old_size, cur_head, cur_size;  // the checked extents (0, 0 where the flag of that side is missing)
  int kept, pad;
};

struct ChkArgs {
  double r, r2;  // r * r rounded once on the host, as the model rounds it
  int stride, count, n, max_states;
  const fh_vehicle* cur_v;
  const fh_state* cur_p;
  const fh_vehicle* old_v;
  const fh_state* old_p;
  CellGrid g;
  ChkBox* boxes;  // [n]
  fh_plan_check* out;
};

// the record of src to dst, words of 8 bytes from lanes 0 .. 34; `stage` >= 0 replaces the stage on the way
__device__ __forceinline__ void chk_copy_record(const fh_vehicle* src, fh_vehicle* dst, int lane, int stage) {
  if (lane >= CHK_RECORD_WORDS) return;
  unsigned long long w = reinterpret_cast<const unsigned long long*>(src)[lane];
  if (stage >= 0 && lane == (int)(offsetof(fh_vehicle, stage) / 8)) w = (w & 0xffffffff00000000ull) | (unsigned long long)(unsigned)stage;
  reinterpret_cast<unsigned long long*>(dst)[lane] = w;
}

// `size` states from src to dst, 16 bytes per lane and turn
__device__ __forceinline__ void chk_copy_states(const fh_state* src, fh_state* dst, int size, int lane) {
  const uint4* s = reinterpret_cast<const uint4*>(src);
  uint4* d = reinterpret_cast<uint4*>(dst);
  const long long chunks = (long long)size * (long long)(sizeof(fh_state) / 16);
  for (long long c = lane; c < chunks; c += 64) d[c] = s[c];
}

__global__ void __launch_bounds__(64) check_backup_kernel(const fh_vehicle* __restrict__ vehicles, const fh_state* __restrict__ plans, int n,
                                                          int max_states, fh_vehicle* __restrict__ b_vehicles, fh_state* __restrict__ b_plans) {
  const int lane = fhw::lane_id();
  const int k = (int)blockIdx.x;
  if (k >= n) return;
  const int head = fhw::uniform_i32(vehicles[k].plan_head), size = fhw::uniform_i32(vehicles[k].plan_size);
  chk_copy_record(vehicles + k, b_vehicles + k, lane, -1);
  if (plan_bad_extent(head, size, max_states)) return;
  const size_t first = (size_t)k * (size_t)max_states + (size_t)head;
  chk_copy_states(plans + first, b_plans + first, size, lane);
}

__global__ void __launch_bounds__(64) check_revert_kernel(const fh_plan_check* __restrict__ records, const fh_vehicle* __restrict__ b_vehicles,
                                                          const fh_state* __restrict__ b_plans, int n, int max_states,
                                                          fh_vehicle* __restrict__ vehicles, fh_state* __restrict__ plans) {
  const int lane = fhw::lane_id();
  const int k = (int)blockIdx.x;
  if (k >= n) return;
  if (!(fhw::uniform_i32(records[k].flags) & FH_CHECK_CONFLICT)) return;
  const int head = fhw::uniform_i32(b_vehicles[k].plan_head), size = fhw::uniform_i32(b_vehicles[k].plan_size);
  chk_copy_record(b_vehicles + k, vehicles + k, lane, FH_FLEET_STAGE_CONFLICT);
  if (plan_bad_extent(head, size, max_states)) return;
  const size_t first = (size_t)k * (size_t)max_states + (size_t)head;
  chk_copy_states(b_plans + first, plans + first, size, lane);
}

__global__ void __launch_bounds__(64) check_boxes_kernel(ChkArgs a) {
#pragma clang fp contract(off)
  const int lane = fhw::lane_id();
  const int k = (int)blockIdx.x;
  if (k >= a.n) return;
  const fh_vehicle& O = a.old_v[k];
  const fh_vehicle& C = a.cur_v[k];
  const int o_head = fhw::uniform_i32(O.plan_head), o_size = fhw::uniform_i32(O.plan_size), k_end = fhw::uniform_i32(O.k_end_whole);
  const int c_head = fhw::uniform_i32(C.plan_head), c_size = fhw::uniform_i32(C.plan_size);
  const int stage = fhw::uniform_i32(C.stage), active = fhw::uniform_i32(C.active);
  const bool bad_o = plan_bad_extent(o_head, o_size, a.max_states), bad_c = plan_bad_extent(c_head, c_size, a.max_states);
  const bool cand = stage == FH_FLEET_STAGE_COMMITTED && active != 0 && !bad_o && !bad_c;
  int valid = (!bad_o && o_size >= 1 ? CHK_OLD_OTHER : 0) | (cand ? CHK_CANDIDATE : 0) | (cand && c_size >= 1 ? CHK_CUR_OTHER : 0);
  int kept = 0, cell = 0;
  if (cand) {
    const long long want = (long long)o_size - (long long)k_end - 1, top = o_size < c_size ? o_size : c_size;
    if (want < 0 || want > top) valid |= CHK_CLAMPED;
    kept = (int)(want < 0 ? 0 : (want > top ? top : want));
  }
  double lx = INFINITY, ly = INFINITY, lz = INFINITY, hx = -INFINITY, hy = -INFINITY, hz = -INFINITY;
  bool not_finite = false;
  for (int side = 0; side < 2; side++) {  // 0: old_k, 1: cur_k of a candidate
    if (side == 0 ? bad_o : !cand) continue;
    const int head = side == 0 ? o_head : c_head, size = side == 0 ? o_size : c_size;
    const int m = plan_limit(a.count, size);  // (the last state is below m whenever an instant behind the plan can be tested)
    const bool stands = size >= 1 && (a.count == 0 || size < a.count);
    const fh_state* plan = (side == 0 ? a.old_p : a.cur_p) + ((size_t)k * (size_t)a.max_states + (size_t)head);
    for (int j = lane; j < m; j += 64) {
      const double* p = plan[j].pos;
      const double x = p[0], y = p[1], z = p[2];
      if (plan_finite(x) && plan_finite(y) && plan_finite(z)) {
        plan_box_take(x, y, z, lx, ly, lz, hx, hy, hz);
      } else if (side == 1 && ((j >= kept && (j - kept) % a.stride == 0) || (stands && j == size - 1))) {
        not_finite = true;
      }
    }
  }
  if (fhw::wave_any(not_finite)) valid |= CHK_NOT_FINITE;
  valid |= cell_box_tail(a.g, lane, lx, ly, lz, hx, hy, hz, cell);
  if (lane == 0) {
    ChkBox& b = a.boxes[k];
    cell_box_store(b.c, lx, ly, lz, hx, hy, hz, valid, cell);
    b.old_head = (valid & CHK_OLD_OTHER) ? o_head : 0; b.old_size = (valid & CHK_OLD_OTHER) ? o_size : 0;
    b.cur_head = cand ? c_head : 0; b.cur_size = cand ? c_size : 0;
    b.kept = kept; b.pad = 0;
  }
}

__global__ void __launch_bounds__(64) check_narrow_kernel(ChkArgs a) {
#pragma clang fp contract(off)
  __shared__ int list_k[CHK_LIST], list_kind[CHK_LIST], list_head[CHK_LIST], list_size[CHK_LIST];
  const int lane = fhw::lane_id();
  const int i = (int)blockIdx.x;
  if (i >= a.n) return;
  const ChkBox& B = a.boxes[i];
  const int valid = fhw::uniform_i32(B.c.valid);
  int flags = 0, n_tested = 0, first = -1, first_other = -1, first_kind = -1;
  double first_d2 = INFINITY;
  if (valid & CHK_CANDIDATE) {  // (uniform)
    const int head = fhw::uniform_i32(B.cur_head), size = fhw::uniform_i32(B.cur_size), kept = fhw::uniform_i32(B.kept);
    flags = FH_CHECK_CANDIDATE | ((valid & CHK_CLAMPED) ? FH_CHECK_BAD_PLAN : 0) | ((valid & CHK_NOT_FINITE) ? FH_CHECK_NOT_FINITE : 0);
    const int m_own = plan_limit(a.count, size);
    n_tested = m_own > kept ? plan_instants(m_own - kept, a.stride) : 0;
    if ((valid & CELL_BOXED) && size >= 1) {
      const fh_state* plan = a.cur_p + ((size_t)i * (size_t)a.max_states + (size_t)head);
      int b_j = 0x7fffffff, b_k = 0x7fffffff, b_kind = 0x7fffffff;  // what this lane has seen: the smallest (j, k, kind) in conflict
      double b_d2 = INFINITY;
      int n_list = 0, r_end = 0x7fffffff;  // (uniform) entries in the list; rounds at and behind r_end cannot hold the first conflict
      int j_cut = 0x7fffffff;              // (uniform) the smallest instant in conflict so far: later instants are not read again
      cell_walk(a.g, B.c, a.r, i, a.n, lane, [&](int k, const CellReach& w, bool end) {
        bool keep_old = false, keep_cur = false;
        int o_head = 0, o_size = 0, c_head = 0, c_size = 0;
        if (k >= 0) {
          const ChkBox& K = a.boxes[k];
          const int kv = K.c.valid;
          o_head = K.old_head; o_size = K.old_size; c_head = K.cur_head; c_size = K.cur_size;
          const bool meets = (kv & CELL_BOXED) && cell_meets(K.c, w);
          keep_old = meets && (kv & CHK_OLD_OTHER);
          keep_cur = meets && (kv & CHK_CUR_OTHER) && k < i;
        }
        const unsigned long long m_old = __ballot(keep_old), m_cur = __ballot(keep_cur);
        if (keep_old) {
          const int slot = n_list + fhw::rank_in(m_old);
          list_k[slot] = k; list_kind[slot] = 0; list_head[slot] = o_head; list_size[slot] = o_size;
        }
        n_list += (int)__popcll(m_old);
        if (keep_cur) {
          const int slot = n_list + fhw::rank_in(m_cur);
          list_k[slot] = k; list_kind[slot] = 1; list_head[slot] = c_head; list_size[slot] = c_size;
        }
        n_list += (int)__popcll(m_cur);
        if (n_list > CHK_LIST - 128 || end) {
          __syncthreads();
          // the instants this list can test: below the largest M of its pairs
          int longest = size;
          for (int e = lane; e < n_list; e += 64) longest = max(longest, list_size[e]);
          longest = -fhw::wave_min_i32(-longest);
          if (a.count > 0) longest = min(longest, a.count);
          const long long instants = longest > kept ? ((long long)(longest - kept) + a.stride - 1) / a.stride : 0;
          const int rounds = (int)((instants + 63) >> 6);
          for (int s = 0; s < rounds && s < r_end; s++) {
            const long long t = (long long)s * 64 + lane;
            const int j = t < instants ? kept + (int)t * a.stride : 0x7fffffff;  // (< longest <= max_states)
            const bool mine = j <= j_cut;  // (an instant behind the first conflict so far cannot be the first; j_cut itself can, by k and kind)
            double px = 0.0, py = 0.0, pz = 0.0;
            if (mine) {
              const double* p = plan[j < size - 1 ? j : size - 1].pos;
              px = p[0]; py = p[1]; pz = p[2];
            }
            bool hit = false;
            for (int e = 0; e < n_list; e++) {
              const int k_e = list_k[e], kind_e = list_kind[e], size_e = list_size[e];
              int M = size > size_e ? size : size_e;
              if (a.count > 0) M = min(M, a.count);
              if (!mine || j >= M) continue;
              const fh_state* other = (kind_e ? a.cur_p : a.old_p) + ((size_t)k_e * (size_t)a.max_states + (size_t)list_head[e]);
              const double* o = other[j < size_e - 1 ? j : size_e - 1].pos;
              const double dx = o[0] - px, dy = o[1] - py, dz = o[2] - pz;
              const double d2 = dx * dx + dy * dy + dz * dz;
              if (d2 < a.r2 && (j < b_j || (j == b_j && (k_e < b_k || (k_e == b_k && kind_e < b_kind))))) {
                b_j = j; b_k = k_e; b_kind = kind_e; b_d2 = d2;
                hit = true;
              }
            }
            if (fhw::wave_any(hit)) {  // every instant of a later round is larger
              r_end = s + 1;
              j_cut = fhw::wave_min_i32(b_j);
              break;
            }
          }
          __syncthreads();
          n_list = 0;
        }
      });
      // the smallest j, then the smallest k among the lanes that hold it, then the smaller kind; one lane holds all three
      first = fhw::wave_min_i32(b_j);
      if (first == 0x7fffffff) {
        first = -1;
      } else {
        first_other = fhw::wave_min_i32(b_j == first ? b_k : 0x7fffffff);
        first_kind = fhw::wave_min_i32(b_j == first && b_k == first_other ? b_kind : 0x7fffffff);
        first_d2 = fhw::readlane_f64(b_d2, fhw::first_lane(b_j == first && b_k == first_other && b_kind == first_kind));
        flags |= FH_CHECK_CONFLICT;
      }
    }
  }
  // words 2 l and 2 l + 1 of the record from lane l < 2: 32 contiguous bytes in one store instruction
  double w0 = 0.0, w1 = 0.0;
  if (lane == 0) { w0 = plan_pack(flags, n_tested); w1 = plan_pack(first, first_other); }
  if (lane == 1) { w0 = plan_pack(first_kind, 0); w1 = first_d2; }
  if (lane < 2) reinterpret_cast<double2*>(a.out + i)[lane] = make_double2(w0, w1);
}

}  // namespace fh

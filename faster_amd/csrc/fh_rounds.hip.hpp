// fh_rounds.hip.hpp — the priority rounds of a fleet (include/fasterhip_rounds.h, which is the specification): which vehicles can come
// near each other (neighbours: d2 < reach reach at one tested instant of the two plans), and from that a class per vehicle such that
// neighbours get different classes below the last: greedy colouring in index order, computed in passes.  The broad phase is the cell
// grid (fh_cells.hip.hpp: its launches, why its prefilters lose nothing and where every index comes from), with reach.  Its own:
//   rounds_boxes_kernel  : one wavefront per vehicle k, lane = state.  The extent is checked, then the bounding box of every finite
//                          position the pairs can read (every state below `count` and with it the last one: a superset of the strided
//                          ones), FH_ROUND_BAD_PLAN and FH_ROUND_NOT_FINITE decided; box, extent and flags go into boxes[k].
//   rounds_narrow_kernel : one wavefront per vehicle i.  The candidates of the walk with k < i whose box meets box_i grown by reach + g
//                          enter an LDS list as (k, head, size).  When the list cannot take 64 more, or the cells end, it is tested in
//                          rounds of 64 instants, lane = instant j = (64 s + lane) stride: the lane reads its own position once per
//                          round and, for every listed other that has not hit yet and with j < M, the other's.  One instant decides a
//                          neighbour: an other is finished at its first hit (a bit of `done`, two words of 64, uniform), and the
//                          rounds end when every listed other is.  The neighbours of a list are its `done` bits: their slots in row i
//                          of the lists come from that ballot and the rank of the lane, no atomics; n_lower counts every hit, the row
//                          keeps the first FH_ROUNDS_LIST.  The order inside a row is that of the walk and nothing depends on it.
//                          The pass-0 record leaves as one 16-byte store.
//   rounds_pass_kernel   : lane = vehicle, launched for p = 1 .. passes.  A vehicle that is decided is done.  Else one 8-byte load of
//                          (round_class, decided_pass) per listed neighbour: all of them 0 <= decided_pass < p, and the vehicle takes
//                          the smallest class missing in a mask of 64 bits, clipped, with one 8-byte store.  A neighbour that this
//                          same launch decides shows decided_pass = -1 or p: both fail the test, so no launch reads what it writes
//                          in a way that matters: no race that changes a byte, no order between wavefronts, no waiting.
//   rounds_finish_kernel : lane = vehicle: who is still undecided goes into the last round with FH_ROUND_UNSETTLED.
//   rounds_gate_kernel   : lane = vehicle: active (the record's and the path search's) = begin's active and the round's condition.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fasterhip_check.h"
#include "../../include/fasterhip_rounds.h"
#include "fh_cells.hip.hpp"
#include "fh_plans.hip.hpp"
#include "fh_wave.hip.hpp"

namespace fh {

constexpr int RND_LIST = 128;  // the LDS list of the narrow phase (the check's holds 256)
static_assert(sizeof(fh_plan_round) == 16 && offsetof(fh_plan_round, round_class) == 0 && offsetof(fh_plan_round, decided_pass) == 4,
              "(round_class, decided_pass) is the first word of 8 bytes of a record of 16");
static_assert(FH_ROUNDS_MAX <= 64 && FH_ROUNDS_LIST == 64, "the mex is taken with one mask of 64 bits; a row of the lists is filled from ballots of 64");

enum {                 // RndBox.c.valid, above CELL_BOXED
  RND_PLAN = 2,        // a good extent that holds a state: the vehicle can have neighbours
  RND_BAD = 4,         // a bad extent
  RND_NOT_FINITE = 8   // one of its own readable positions is not finite
};

struct RndBox {  // 64 B
  CellBox c;
  int head, size;  // the checked extent (0, 0 without RND_PLAN)
};

struct RndArgs {
  double reach, r2;  // reach * reach rounded once on the host, as the model rounds it
  int rounds, stride, count, n, max_states;
  const fh_vehicle* vehicles;
  const fh_state* plans;
  CellGrid g;
  RndBox* boxes;        // [n]
  int* lists;           // [n][FH_ROUNDS_LIST]
  fh_plan_round* out;   // [n]
};

// the word (round_class, decided_pass) of a record, whole
__device__ __forceinline__ unsigned long long rnd_word(int round_class, int decided_pass) {
  return (unsigned long long)(unsigned)round_class | ((unsigned long long)(unsigned)decided_pass << 32);
}

__global__ void __launch_bounds__(64) rounds_boxes_kernel(RndArgs a) {
#pragma clang fp contract(off)
  const int lane = fhw::lane_id();
  const int k = (int)blockIdx.x;
  if (k >= a.n) return;
  const fh_vehicle& V = a.vehicles[k];
  const int head = fhw::uniform_i32(V.plan_head), size = fhw::uniform_i32(V.plan_size);
  const bool bad = plan_bad_extent(head, size, a.max_states);
  int valid = bad ? RND_BAD : (size >= 1 ? RND_PLAN : 0), cell = 0;
  double lx = INFINITY, ly = INFINITY, lz = INFINITY, hx = -INFINITY, hy = -INFINITY, hz = -INFINITY;
  bool not_finite = false;
  if (!bad) {
    const int m = plan_limit(a.count, size);  // (the last state is below m whenever an instant behind the plan can be tested)
    const bool stands = size >= 1 && (a.count == 0 || size < a.count);
    const fh_state* plan = a.plans + ((size_t)k * (size_t)a.max_states + (size_t)head);
    for (int j = lane; j < m; j += 64) {
      const double* p = plan[j].pos;
      const double x = p[0], y = p[1], z = p[2];
      if (plan_finite(x) && plan_finite(y) && plan_finite(z)) {
        plan_box_take(x, y, z, lx, ly, lz, hx, hy, hz);
      } else if (j % a.stride == 0 || (stands && j == size - 1)) {
        not_finite = true;
      }
    }
  }
  if (fhw::wave_any(not_finite)) valid |= RND_NOT_FINITE;
  valid |= cell_box_tail(a.g, lane, lx, ly, lz, hx, hy, hz, cell);
  if (lane == 0) {
    RndBox& b = a.boxes[k];
    cell_box_store(b.c, lx, ly, lz, hx, hy, hz, valid, cell);
    b.head = (valid & RND_PLAN) ? head : 0; b.size = (valid & RND_PLAN) ? size : 0;
  }
}

__global__ void __launch_bounds__(64) rounds_narrow_kernel(RndArgs a) {
#pragma clang fp contract(off)
  __shared__ int list_k[RND_LIST], list_head[RND_LIST], list_size[RND_LIST];
  const int lane = fhw::lane_id();
  const int i = (int)blockIdx.x;
  if (i >= a.n) return;
  const RndBox& B = a.boxes[i];
  const int valid = fhw::uniform_i32(B.c.valid);
  int n_lower = 0;  // (uniform)
  if ((valid & CELL_BOXED) && (valid & RND_PLAN)) {  // (uniform)
    const int head = fhw::uniform_i32(B.head), size = fhw::uniform_i32(B.size);
    const fh_state* plan = a.plans + ((size_t)i * (size_t)a.max_states + (size_t)head);
    int* row = a.lists + (size_t)i * (size_t)FH_ROUNDS_LIST;
    int n_list = 0;  // (uniform) entries in the list
    cell_walk(a.g, B.c, a.reach, i, a.n, lane, [&](int k, const CellReach& w, bool end) {
      bool keep = false;
      int k_head = 0, k_size = 0;
      if (k >= 0 && k < i) {
        const RndBox& K = a.boxes[k];
        const int kv = K.c.valid;
        k_head = K.head; k_size = K.size;
        keep = (kv & CELL_BOXED) && (kv & RND_PLAN) && cell_meets(K.c, w);
      }
      const unsigned long long m_keep = __ballot(keep);
      if (keep) {
        const int slot = n_list + fhw::rank_in(m_keep);  // (< RND_LIST: the list is emptied when it cannot take 64 more)
        list_k[slot] = k; list_head[slot] = k_head; list_size[slot] = k_size;
      }
      n_list += (int)__popcll(m_keep);
      if (n_list > RND_LIST - 64 || end) {
        __syncthreads();
        // the instants this list can test: below the largest M of its pairs
        int longest = size;
        for (int e = lane; e < n_list; e += 64) longest = max(longest, list_size[e]);
        longest = -fhw::wave_min_i32(-longest);
        if (a.count > 0) longest = min(longest, a.count);
        const long long instants = ((long long)longest + a.stride - 1) / a.stride;
        const int turns = (int)((instants + 63) >> 6);
        unsigned long long done0 = 0ull, done1 = 0ull;  // (uniform) bit e & 63 of word e >> 6: listed other e is a neighbour
        int n_done = 0;
        for (int s = 0; s < turns && n_done < n_list; s++) {
          const long long t = (long long)s * 64 + lane;
          const bool mine = t < instants;
          const int j = mine ? (int)t * a.stride : 0;  // (< longest <= max_states)
          double px = 0.0, py = 0.0, pz = 0.0;
          if (mine) {
            const double* p = plan[j < size - 1 ? j : size - 1].pos;
            px = p[0]; py = p[1]; pz = p[2];
          }
          for (int e = 0; e < n_list; e++) {
            if (((e < 64 ? done0 : done1) >> (e & 63)) & 1ull) continue;  // (uniform)
            const int size_e = list_size[e];
            int M = size > size_e ? size : size_e;
            if (a.count > 0) M = min(M, a.count);
            bool hit = false;
            if (mine && j < M) {
              const fh_state* other = a.plans + ((size_t)list_k[e] * (size_t)a.max_states + (size_t)list_head[e]);
              const double* o = other[j < size_e - 1 ? j : size_e - 1].pos;
              const double dx = o[0] - px, dy = o[1] - py, dz = o[2] - pz;
              const double d2 = dx * dx + dy * dy + dz * dz;
              hit = d2 < a.r2;
            }
            if (fhw::wave_any(hit)) {
              if (e < 64) done0 |= 1ull << e; else done1 |= 1ull << (e - 64);
              n_done++;
            }
          }
        }
        // the neighbours of this list into row i: the slot of lane l's entry is its rank among the done bits
        for (int half = 0; half < 2; half++) {
          const unsigned long long m_done = half ? done1 : done0;
          const int e = half * 64 + lane;
          const int slot = n_lower + fhw::rank_in(m_done);
          if (((m_done >> lane) & 1ull) && e < n_list && slot < FH_ROUNDS_LIST) row[slot] = list_k[e];
          n_lower += (int)__popcll(m_done);
        }
        __syncthreads();
        n_list = 0;
      }
    });
  }
  if (lane == 0) {
    int flags = ((valid & RND_BAD) ? FH_ROUND_BAD_PLAN : 0) | ((valid & RND_NOT_FINITE) ? FH_ROUND_NOT_FINITE : 0);
    int round_class = -1, decided_pass = -1;
    if (n_lower == 0) {
      round_class = 0; decided_pass = 0;
    } else if (n_lower > FH_ROUNDS_LIST) {
      round_class = a.rounds - 1; decided_pass = 0; flags |= FH_ROUND_OVERFLOW;
    }
    *reinterpret_cast<int4*>(a.out + i) = make_int4(round_class, decided_pass, n_lower, flags);
  }
}

__global__ void __launch_bounds__(256) rounds_pass_kernel(const int* __restrict__ lists, fh_plan_round* out, int n, int rounds, int p) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i >= n) return;
  unsigned long long* words = reinterpret_cast<unsigned long long*>(out);  // word 2 k: (round_class, decided_pass) of vehicle k
  if ((int)(__hip_atomic_load(words + 2 * (size_t)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> 32) >= 0) return;  // decided
  const int n_lower = min(out[i].n_lower, FH_ROUNDS_LIST);  // (an undecided vehicle has 1 .. FH_ROUNDS_LIST; the narrow phase wrote it)
  const int* row = lists + (size_t)i * (size_t)FH_ROUNDS_LIST;
  unsigned long long taken = 0ull;
  for (int e = 0; e < n_lower; e++) {
    const int k = row[e];
    if (!(k >= 0 && k < i)) return;  // (never: the narrow phase wrote lower vehicles)
    const unsigned long long w = __hip_atomic_load(words + 2 * (size_t)k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int k_class = (int)(unsigned)w, k_pass = (int)(w >> 32);
    if (!(k_pass >= 0 && k_pass < p)) return;  // undecided, or decided by this very launch: not yet
    taken |= 1ull << (k_class & 63);           // (0 <= class < rounds <= 64)
  }
  const int mex = ~taken ? (int)__builtin_ctzll(~taken) : 64;
  __hip_atomic_store(words + 2 * (size_t)i, rnd_word(min(mex, rounds - 1), p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void __launch_bounds__(256) rounds_finish_kernel(fh_plan_round* __restrict__ out, int n, int rounds) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i >= n) return;
  const int4 r = *reinterpret_cast<const int4*>(out + i);
  if (r.y >= 0) return;
  *reinterpret_cast<int4*>(out + i) = make_int4(rounds - 1, -1, r.z, r.w | FH_ROUND_UNSETTLED);
}

__global__ void __launch_bounds__(256) rounds_gate_kernel(const fh_plan_round* __restrict__ rounds, int round,
                                                          const int32_t* __restrict__ active_begin, int n, fh_vehicle* __restrict__ vehicles,
                                                          int32_t* __restrict__ active) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i >= n) return;
  bool on = active_begin[i] != 0;
  if (round >= 0) on = on && rounds[i].round_class == round;
  else if (round == FH_ROUND_RETRY) on = on && vehicles[i].stage == FH_FLEET_STAGE_CONFLICT;
  vehicles[i].active = on ? 1 : 0;
  active[i] = on ? 1 : 0;
}

}  // namespace fh

// fh_link_los.hip.hpp — walls block a radio link (include/fasterhip_link_los.h, which is the specification): the groups of fh_link.hip.hpp
// with one more condition on a linked pair, a line of sight through the occupancy bits of the map.  link_boxes_kernel, the cell grid,
// link_init_kernel and link_jump_kernel are launched as they are; the narrow phase and the hook are the two kernels of this file.
//   link_los_narrow_kernel : one wavefront per vehicle i.  The walk of link_narrow_kernel and its in-range test (link_test), lane =
//                        candidate; the ballot of the in-range lanes is the compaction.  Then the rays, one in-range candidate after the
//                        other (a uniform loop over the set bits), LANE = SAMPLE: the pair's two ends go to every lane (readlane), lane l
//                        takes the samples j = 1 + l, 65 + l, .. of the ray, and one ballot per 64 samples ends the ray at the first
//                        round with a hit.  The views of the pairs that are not blocked go into row i exactly as link_narrow_kernel
//                        stores them (slots from the ballot and the rank of the lane, the first FH_LINK_LIST), nbrs[i] counts them,
//                        and the pairs with k > i are added once per wavefront to info[2] (linked) and info[3] (blocked).
//                        It also keeps, for the first LINK_LOS_TURNS turns of the walk, the ballot of the linked lanes (`turns`).
//   link_los_hook_kernel  : link_hook_kernel on those rows; a vehicle with more than FH_LINK_LIST neighbours in line of sight walks the
//                        cells again.  That walk is the narrow phase's, turn for turn (the same grid, boxes, starts and items within one
//                        call), so for a kept turn the ballot says which lanes hold a linked candidate and no ray is cast a second time
//                        (the rays of a crowded vehicle, times `passes`, were nine tenths of the stage before the ballots were kept);
//                        past the kept turns it applies the narrow phase's test again.  Reads L, writes H by an atomic minimum only
//                        where it lowers a label.
// WHY LANE = SAMPLE AND NOT LANE = CANDIDATE.  A vehicle of the fleets this project measures has a handful of vehicles in range (1 to 16)
// and a ray has 2 dist / res_map samples (30 at 3 m and 0.2 m, up to 8191 at the limit).  With lane = candidate the wavefront would
// run the longest ray of the turn serially on a handful of lanes; with lane = sample a ray of up to 64 samples is ONE round of loads for
// the whole wavefront, the cost of a vehicle is (candidates in range) x ceil((K - 1) / 64) rounds, and a blocked ray stops at its first
// round with a hit.  The order of the rays and the lane that finds a hit do not show: a pair is blocked iff ANY sample hits.
// Both ends of a pair cast THE SAME ray (from the vehicle with the smaller index), so what i finds for (i, k) is what k finds for
// (k, i) bit for bit: rows and counts need no agreement between wavefronts, and no atomics beyond those of fh_link.hip.hpp (the minimum
// into H, the counters of info).
// EVERY INDEX COMES FROM A CHECKED VALUE.  Candidates are boxed vehicles (link_test: finite positions, a checked view); a ray is cast
// only for a pair with d2 < r2, so its ends are finite and K is below 2 (4096 + 1) by the entry point's limit (and clamped before it
// becomes an int); a sample's floored cell is compared with the map's dimensions in double before it becomes an index, and a sample
// outside the map reads nothing.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fasterhip_link_los.h"
#include "fh_link.hip.hpp"

namespace fh {

struct LinkLosMap {  // the map a ray is cast through: its lattice and its occupancy bits (fh_map_dims, fh_map_occupancy_bits_device)
  const unsigned* occ;  // cell (x, y, z) = bit (z my + y) mx + x
  double ox, oy, oz, res;
  int mx, my, mz, pad;
};

constexpr int LINK_LOS_TURNS = 32;  // turns of a vehicle's walk whose ballots of the pairs in line of sight are kept for the hooks

struct LinkLosArgs {
  LinkArgs l;
  LinkLosMap m;
  unsigned long long* turns;  // [n][LINK_LOS_TURNS]: per turn of the walk of vehicle i, the lanes whose candidate is linked
};

constexpr int LINK_LOS_MAX_K = 16384;  // (never reached: range / res_map <= 4096 gives K <= 8193)

// Is the pair with the ends p (the vehicle with the smaller index) and q blocked?  Whole wavefront, every argument uniform; lane = sample.
__device__ __forceinline__ bool link_los_blocked(const LinkLosMap& m, int lane, double px, double py, double pz, double qx, double qy, double qz) {
#pragma clang fp contract(off)
  const double dx = qx - px, dy = qy - py, dz = qz - pz;
  const double d2 = dx * dx + dy * dy + dz * dz;
  const double kf = ceil(sqrt(d2) / (0.5 * m.res));
  const int K = kf > 1.0 ? (kf < (double)LINK_LOS_MAX_K ? (int)kf : LINK_LOS_MAX_K) : 1;  // (a NaN gives 1: no sample)
  const double pfx = floor((px - m.ox) / m.res), pfy = floor((py - m.oy) / m.res), pfz = floor((pz - m.oz) / m.res);  // the cells of the two
  const double qfx = floor((qx - m.ox) / m.res), qfy = floor((qy - m.oy) / m.res), qfz = floor((qz - m.oz) / m.res);  // ends: not tested
  for (int j0 = 1; j0 < K; j0 += 64) {  // (uniform)
    const int j = j0 + lane;
    bool hit = false;
    if (j < K) {
      const double t = (double)j / (double)K;
      const double fx = floor((px + dx * t - m.ox) / m.res), fy = floor((py + dy * t - m.oy) / m.res), fz = floor((pz + dz * t - m.oz) / m.res);
      const bool end_cell = (fx == pfx && fy == pfy && fz == pfz) || (fx == qfx && fy == qfy && fz == qfz);
      const bool inside = fx >= 0.0 && fx < (double)m.mx && fy >= 0.0 && fy < (double)m.my && fz >= 0.0 && fz < (double)m.mz;
      if (inside && !end_cell) {
        const long long id = ((long long)(int)fz * m.my + (int)fy) * m.mx + (int)fx;
        hit = (m.occ[id >> 5] >> (id & 31)) & 1u;
      }
    }
    if (fhw::wave_any(hit)) return true;
  }
  return false;
}

// One turn of the walk of vehicle i at (px, py, pz) (whole wavefront): k = this lane's candidate or -1.  Returns the lanes whose
// candidate is in range (uniform) and, in `clear`, those of them whose pair is not blocked; kv = the view of this lane's candidate.
__device__ __forceinline__ unsigned long long link_los_turn(const LinkLosArgs& a, int lane, int i, double px, double py, double pz, int k, int& kv,
                                                            unsigned long long& clear) {
  const bool in_range = link_test(a.l, k, px, py, pz, kv);
  double kx = 0.0, ky = 0.0, kz = 0.0;
  if (in_range) {
    const double* lo = a.l.boxes[k].c.lo;
    kx = lo[0]; ky = lo[1]; kz = lo[2];
  }
  const unsigned long long m_near = __ballot(in_range);
  clear = 0ull;
  for (unsigned long long todo = m_near; todo; todo &= todo - 1ull) {  // (uniform)
    const int src = (int)__builtin_ctzll(todo);
    const int ks = __builtin_amdgcn_readlane(k, src);
    const double sx = fhw::readlane_f64(kx, src), sy = fhw::readlane_f64(ky, src), sz = fhw::readlane_f64(kz, src);
    const bool blocked = ks > i ? link_los_blocked(a.m, lane, px, py, pz, sx, sy, sz) : link_los_blocked(a.m, lane, sx, sy, sz, px, py, pz);
    if (!blocked) clear |= 1ull << src;
  }
  return m_near;
}

__global__ void __launch_bounds__(64) link_los_narrow_kernel(LinkLosArgs a) {
  const int lane = fhw::lane_id();
  const int i = (int)blockIdx.x;
  if (i >= a.l.n) return;
  const LinkBox& B = a.l.boxes[i];
  int n_nbr = 0, n_up = 0, n_blocked_up = 0, turn = 0;  // (uniform)
  if (fhw::uniform_i32(B.c.valid) & CELL_BOXED) {
    const double px = fhw::uniform_f64(B.c.lo[0]), py = fhw::uniform_f64(B.c.lo[1]), pz = fhw::uniform_f64(B.c.lo[2]);
    int* row = a.l.lists + (size_t)i * (size_t)FH_LINK_LIST;
    unsigned long long* kept = a.turns + (size_t)i * (size_t)LINK_LOS_TURNS;
    cell_walk(a.l.g, B.c, a.l.range, i, a.l.n, lane, [&](int k, const CellReach&, bool) {
      int kv = 0;
      unsigned long long m_hit = 0ull;
      const unsigned long long m_near = link_los_turn(a, lane, i, px, py, pz, k, kv, m_hit);
      if (lane == 0 && turn < LINK_LOS_TURNS) kept[turn] = m_hit;
      turn++;
      const bool hit = (m_hit >> lane) & 1ull, in_range = (m_near >> lane) & 1ull;
      const int slot = n_nbr + fhw::rank_in(m_hit);
      if (hit && slot < FH_LINK_LIST) row[slot] = kv;
      n_nbr += (int)__popcll(m_hit);
      n_up += (int)__popcll(__ballot(hit && k > i));
      n_blocked_up += (int)__popcll(__ballot(in_range && !hit && k > i));
    });
  }
  if (lane == 0) {
    a.l.nbrs[i] = n_nbr;
    if (n_up > 0) atomicAdd(a.l.info + 2, (unsigned long long)n_up);
    if (n_blocked_up > 0) atomicAdd(a.l.info + 3, (unsigned long long)n_blocked_up);
  }
}

__global__ void __launch_bounds__(64) link_los_hook_kernel(LinkLosArgs a, const int* __restrict__ L, int* H) {
  const int lane = fhw::lane_id();
  const int i = (int)blockIdx.x;
  if (i >= a.l.n) return;
  const LinkBox& B = a.l.boxes[i];
  if (!(fhw::uniform_i32(B.c.valid) & CELL_BOXED)) return;
  const int n_nbr = fhw::uniform_i32(a.l.nbrs[i]);
  const int view = fhw::uniform_i32(B.view);
  if (n_nbr <= 0 || !(view >= 0 && view < a.l.n_views)) return;  // (the view of a boxed vehicle was checked by link_boxes_kernel)
  int m = 0x7fffffff;
  if (n_nbr <= FH_LINK_LIST) {
    const int* row = a.l.lists + (size_t)i * (size_t)FH_LINK_LIST;
    if (lane < n_nbr) {
      const int kv = row[lane];
      if (kv >= 0 && kv < a.l.n_views) m = L[kv];
    }
  } else {  // more in line of sight than a row holds: the cells again.  The walk is the narrow phase's turn for turn (the same grid, boxes,
            // starts and items), so the ballot it kept for a turn says which lanes hold a linked candidate; past the kept turns, its test
    const double px = fhw::uniform_f64(B.c.lo[0]), py = fhw::uniform_f64(B.c.lo[1]), pz = fhw::uniform_f64(B.c.lo[2]);
    const unsigned long long* kept = a.turns + (size_t)i * (size_t)LINK_LOS_TURNS;
    int turn = 0;  // (uniform)
    cell_walk(a.l.g, B.c, a.l.range, i, a.l.n, lane, [&](int k, const CellReach&, bool) {
      int kv = 0;
      unsigned long long m_hit = 0ull;
      if (turn < LINK_LOS_TURNS) {
        m_hit = kept[turn];
        if (k >= 0 && ((m_hit >> lane) & 1ull)) kv = a.l.boxes[k].view;  // (0 <= k < n from the walk; the view was checked by link_boxes_kernel)
      } else {
        link_los_turn(a, lane, i, px, py, pz, k, kv, m_hit);
      }
      turn++;
      if (k >= 0 && ((m_hit >> lane) & 1ull) && kv >= 0 && kv < a.l.n_views) m = min(m, L[kv]);
    });
  }
  m = fhw::wave_min_i32(m);
  if (lane == 0 && m < L[view]) atomicMin(H + view, m);
}

// The ray test above for the device header that comes in below: the prefix of this file's names stays in this file
// (tests/test_link_los_abi.py), so the tracker calls the same function, unchanged, by this name.
__device__ __forceinline__ bool ray_blocked(const LinkLosMap& m, int lane, double px, double py, double pz, double qx, double qy, double qz) {
  return link_los_blocked(m, lane, px, py, pz, qx, qy, qz);
}

}  // namespace fh

// The tracker of moving obstacles (include/fasterhip_track.h) comes in here, behind the last kernel of the link headers: its kernel lies
// after every kernel of before in the code object of fh_capi.hip, and fh_capi.hip names no device header more.
#include "fh_track.hip.hpp"

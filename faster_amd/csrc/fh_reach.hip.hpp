// fh_reach.hip.hpp — the kernel of include/fasterhip_reach.h (which is the specification): for every vehicle that wants a goal, the
// frontier voxel of its view that a flood of known free space reaches in the fewest steps.  Included by fh_reach.hip only.
//   reach_goals_kernel : ONE workgroup of 256 per vehicle.  Status, stage, view and the six coordinates are read as uniform values; a
//                        vehicle that is not searched has its three outputs written by thread 0 and the workgroup returns.
//                        Its body is reach_body<CLAIMS>: reach_body<false> is this kernel, reach_body<true> the pass kernel of
//                        fh_spread.hip.hpp, in which the build also leaves out the candidates near a peer's goal.
//     build   A wavefront takes a row (iy, iz) of the box, lanes along x, one coalesced flag byte per lane; what depends on the row
//             alone — the z test, dy dy, dz dz, the map's row — is computed once per row, with the float expressions of
//             frontier_goals_kernel (fh_frontier.hip.hpp), so the candidates are its candidates.  The 64 predicates of a row segment
//             become one LDS word by a ballot: two bitmaps of wx rows_y rows_z words, `pass` and `cand`, word (rz rows_y + ry) wx + k.
//             A lane beyond hi0 votes 0 in both, so nothing leaks from the end of one row into the next.  candidates = popcounts.
//     flood   Bitmaps cur and nxt in LDS; thread t owns the words t, t + 256, t + 512, t + 768 and keeps their pass, cand and seen words
//             and the six "has a neighbour word" bits in registers.  Per level
//                 nxt[w] = (cur[w] << 1 | cur[w] >> 1 | carries from cur[w -+ 1] in the SAME row | cur[w -+ wx] in the slab
//                           | cur[w -+ wx rows_y]) & pass[w] & ~seen[w]
//             then seen |= nxt, reached and reachable are popcounts, "any bit" and "any candidate bit" are a wave_or into one LDS slot
//             per wavefront (two sets of slots, by the parity of the level), ONE barrier, and cur and nxt change roles: what a level
//             writes was last read before the barrier of the level before.  No atomics, no spin.
//     choice  In the first level that holds a candidate, and only there, every set bit of level & cand recomputes its d2 with the
//             model's expression; the smallest (d2, c) by wave_min / wave_min_i32 and across the four wavefronts through LDS, the
//             two-key rule of frontier_goals_kernel.  The flood goes on to its end (or max_hops) for the counts.
// LDS: 4 bitmaps of FH_REACH_MAX_WORDS words = 32 KB static, and the slots of the reductions.
// Every address comes from a checked number: view in [0, n_views), the start cell tested against the dims before it is used, box
// indices clipped to the lattice, neighbour bytes tested against the dims and neighbour words against the box before they are
// loaded, the map cell tested against the map's dims before its word is loaded.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fasterhip_reach.h"
#include "fh_wave.hip.hpp"

namespace fhp {

struct ReachArgs {
  double r_max, r2, a2, z_lo, z_hi;  // r2 = r_max * r_max, a2 = r_avoid * r_avoid: rounded once on the host, as the model rounds them
  int want, max_hops;
  int nx, ny, nz;  // the lattice of the views
  double res, ox, oy, oz;
  const unsigned char* flags;
  size_t view_stride;
  const int32_t* view_of;
  int n_views;
  const fh_vehicle* vehicles;
  int mx, my, mz;  // the map
  double mres, mox, moy, moz;
  const unsigned* bits;
  double* goals;
  int32_t* mask;
  fh_reach_record* records;
};

constexpr int REACH_WORDS = FH_REACH_MAX_WORDS;  // words per bitmap
constexpr int REACH_OWN = REACH_WORDS / 256;     // words a thread owns

__device__ __forceinline__ bool reach_finite(double x) { return fabs(x) < INFINITY; }  // (a NaN fails the comparison)

// the first and the last index of the box along one axis, inside [0, n - 1] or empty (lo > hi); whatever f is, NaN included
__device__ __forceinline__ int reach_box_lo(double f, int n) { return f > 0.0 ? (f < (double)n ? (int)f : n) : 0; }
__device__ __forceinline__ int reach_box_hi(double f, int n) { return f < (double)(n - 1) ? (f >= 0.0 ? (int)f : -1) : n - 1; }

// (d2, c) < (e2, k), lexicographic
__device__ __forceinline__ bool reach_before(double d2, int c, double e2, int k) { return d2 < e2 || (d2 == e2 && c < k); }

struct ReachCounts {
  int hops, candidates, reachable, reached, levels;
};

// the three outputs of vehicle i, by one thread
__device__ __forceinline__ void reach_store(const ReachArgs& a, int i, int flags, int view, int cell, double d2, const ReachCounts& n) {
#pragma clang fp contract(off)
  const unsigned long long* g = (const unsigned long long*)a.vehicles[i].g_term;
  unsigned long long* out = (unsigned long long*)(a.goals + 3 * (size_t)i);
  if (cell >= 0) {
    const int ix = cell % a.nx, iy = (cell / a.nx) % a.ny, iz = cell / (a.nx * a.ny);
    a.goals[3 * (size_t)i] = (ix + 0.5) * a.res + a.ox;
    a.goals[3 * (size_t)i + 1] = (iy + 0.5) * a.res + a.oy;
    a.goals[3 * (size_t)i + 2] = (iz + 0.5) * a.res + a.oz;
    flags |= FH_FRONTIER_FOUND;
  } else {
    out[0] = g[0]; out[1] = g[1]; out[2] = g[2];  // the bits of g_term, whatever they are
  }
  a.mask[i] = cell >= 0 ? 1 : 0;
  fh_reach_record r;
  r.flags = flags; r.view = view; r.cell = cell; r.hops = n.hops;
  r.candidates = n.candidates; r.reachable = n.reachable; r.reached = n.reached; r.levels = n.levels;
  r.d2 = d2; r.reserved = 0.0;
  a.records[i] = r;
}

struct ReachNoClaims {};  // the X of reach_body<false>: nothing is read from it

// The body of reach_goals_kernel, and with CLAIMS of the pass kernel of fh_spread.hip.hpp (include/fasterhip_spread.h): there x holds
// x.count points x.pts[3 j ..] in LDS (uniform; written before a barrier that every thread has passed), x.s2, four LDS ints x.sum, and
// x.store writes the outputs.  A candidate with s2 < x.s2 to one of the points is CLAIMED: counted, and left out of `cand`.
// With CLAIMS false every `if constexpr` below is gone and the code is what the kernel held before it was a template.
template <bool CLAIMS, class X>
__device__ __forceinline__ void reach_body(const ReachArgs& a, const X& x) {
#pragma clang fp contract(off)
  __shared__ unsigned long long s_pass[REACH_WORDS], s_cand[REACH_WORDS], s_a[REACH_WORDS], s_b[REACH_WORDS];
  __shared__ double s_d2[4];
  __shared__ int s_c[4], s_n[4], s_m[4];
  __shared__ unsigned s_or[2][4];
  const int i = (int)blockIdx.x, t = (int)threadIdx.x, lane = t & 63, w = t >> 6;
  const fh_vehicle& V = a.vehicles[i];
  const int view = fhw::uniform_i32(a.view_of ? a.view_of[i] : i);
  const int status = fhw::uniform_i32(V.status), stage = fhw::uniform_i32(V.stage);
  const double px = fhw::uniform_f64(V.state.pos[0]), py = fhw::uniform_f64(V.state.pos[1]), pz = fhw::uniform_f64(V.state.pos[2]);
  const double gx = fhw::uniform_f64(V.g_term[0]), gy = fhw::uniform_f64(V.g_term[1]), gz = fhw::uniform_f64(V.g_term[2]);
  const bool wanted = ((a.want & FH_FRONTIER_WANT_REACHED) && status == FH_VEHICLE_GOAL_REACHED) ||
                      ((a.want & FH_FRONTIER_WANT_NO_PATH) && stage == FH_FLEET_STAGE_NO_PATH) || (a.want & FH_FRONTIER_WANT_ALL);
  const bool finite = reach_finite(px) && reach_finite(py) && reach_finite(pz) && reach_finite(gx) && reach_finite(gy) && reach_finite(gz);
  int flags = (wanted ? FH_FRONTIER_WANTED : 0) | (view >= 0 && view < a.n_views ? 0 : FH_FRONTIER_NO_VIEW) | (finite ? 0 : FH_FRONTIER_BAD_POS);
  const ReachCounts none = {-1, 0, 0, 0, 0};
  if (flags != FH_FRONTIER_WANTED) {  // not eligible (uniform over the workgroup)
    if (t == 0) {
      if constexpr (CLAIMS) x.store(a, i, flags, view, -1, INFINITY, none, 0);
      else reach_store(a, i, flags, view, -1, INFINITY, none);
    }
    return;
  }
  // the start cell, tested as a double before it is an index
  const double sfx = floor((px - a.ox) / a.res), sfy = floor((py - a.oy) / a.res), sfz = floor((pz - a.oz) / a.res);
  if (!(sfx >= 0.0 && sfx < (double)a.nx && sfy >= 0.0 && sfy < (double)a.ny && sfz >= 0.0 && sfz < (double)a.nz)) {
    if (t == 0) {
      if constexpr (CLAIMS) x.store(a, i, flags | FH_REACH_START_OUTSIDE, view, -1, INFINITY, none, 0);
      else reach_store(a, i, flags | FH_REACH_START_OUTSIDE, view, -1, INFINITY, none);
    }
    return;
  }
  const int sx = (int)sfx, sy = (int)sfy, sz = (int)sfz;
  const unsigned char* F = a.flags + (size_t)view * a.view_stride;
  const int lo0 = reach_box_lo(floor((px - a.r_max - a.ox) / a.res) - 1.0, a.nx), hi0 = reach_box_hi(floor((px + a.r_max - a.ox) / a.res) + 1.0, a.nx);
  const int lo1 = reach_box_lo(floor((py - a.r_max - a.oy) / a.res) - 1.0, a.ny), hi1 = reach_box_hi(floor((py + a.r_max - a.oy) / a.res) + 1.0, a.ny);
  const int lo2 = reach_box_lo(floor((pz - a.r_max - a.oz) / a.res) - 1.0, a.nz), hi2 = reach_box_hi(floor((pz + a.r_max - a.oz) / a.res) + 1.0, a.nz);
  // (s inside the lattice and r_max > 0: lo <= s <= hi on every axis; tested all the same, an empty box counts as too large)
  const bool holds = lo0 <= sx && sx <= hi0 && lo1 <= sy && sy <= hi1 && lo2 <= sz && sz <= hi2;
  const int rows_y = hi1 - lo1 + 1, rows_z = hi2 - lo2 + 1;
  const int wx = holds ? (hi0 - lo0 + 64) >> 6 : 0;                     // (hi0 - lo0 + 1 <= nx: no overflow)
  const long long words = (long long)wx * rows_y * rows_z;            // (rows_y rows_z <= ny nz < 2^31, wx < 2^26)
  if (!holds || words > (long long)REACH_WORDS) {
    if (t == 0) {
      if constexpr (CLAIMS) x.store(a, i, flags | FH_REACH_BOX_TOO_LARGE, view, -1, INFINITY, none, 0);
      else reach_store(a, i, flags | FH_REACH_BOX_TOO_LARGE, view, -1, INFINITY, none);
    }
    return;
  }
  const int W = (int)words, rows = rows_y * rows_z, slab = wx * rows_y;
  const int slice = a.nx * a.ny;

  // ---- build: pass and cand, a wavefront per row ----
  int count = 0;  // candidates (uniform over the wavefront: sums of popcounts of ballots)
  [[maybe_unused]] int claimed = 0;  // CLAIMS: those of them that are claimed
  for (int r = w; r < rows; r += 4) {  // (r, and all that follows from it alone, is uniform over the wavefront)
    const int iz = lo2 + r / rows_y, iy = lo1 + r % rows_y;
    const double qz = (iz + 0.5) * a.res + a.oz, qy = (iy + 0.5) * a.res + a.oy;
    const bool z_ok = a.z_lo <= qz && qz <= a.z_hi;
    const double fy = floor((qy - a.moy) / a.mres), fz = floor((qz - a.moz) / a.mres);
    const bool row_in_map = fy >= 0.0 && fy < (double)a.my && fz >= 0.0 && fz < (double)a.mz;  // (outside the map: nothing passable in this row)
    const int map_row = row_in_map ? a.mx * ((int)fy + a.my * (int)fz) : 0;
    const double dy = qy - py, dz = qz - pz, ey = qy - gy, ez = qz - gz;
    const double dy2 = dy * dy, dz2 = dz * dz, ey2 = ey * ey, ez2 = ez * ez;
    const int c0 = (iz * a.ny + iy) * a.nx;
    for (int k = 0; k < wx; k++) {
      const int ix = lo0 + 64 * k + lane;
      const int c = c0 + ix;
      bool pass = row_in_map && ix <= hi0 && F[c] == 0;
      const double qx = (ix + 0.5) * a.res + a.ox;
      if (pass) {
        const double fx = floor((qx - a.mox) / a.mres);
        pass = fx >= 0.0 && fx < (double)a.mx;
        if (pass) {
          const int id = map_row + (int)fx;
          pass = ((a.bits[id >> 5] >> (id & 31)) & 1u) == 0u;
        }
      }
      bool cand = pass && z_ok;
      if (cand) {
        const double dx = qx - px;
        const double d2 = dx * dx + dy2 + dz2;
        const double ex = qx - gx;
        const double e2 = ex * ex + ey2 + ez2;
        cand = d2 < a.r2 && !(e2 < a.a2);
        if (cand)
          cand = (ix > 0 && F[c - 1] != 0) || (ix < a.nx - 1 && F[c + 1] != 0) || (iy > 0 && F[c - a.nx] != 0) ||
                 (iy < a.ny - 1 && F[c + a.nx] != 0) || (iz > 0 && F[c - slice] != 0) || (iz < a.nz - 1 && F[c + slice] != 0);
      }
      bool claim = false;
      if constexpr (CLAIMS) {
        if (cand) {  // (x.count is uniform; a point is read by every lane at once: a broadcast)
          for (int j = 0; j < x.count; j++) {
            const double sx = x.pts[3 * j] - qx, sy = x.pts[3 * j + 1] - qy, sz = x.pts[3 * j + 2] - qz;
            const double s2 = sx * sx + sy * sy + sz * sz;
            claim = claim || s2 < x.s2;
          }
        }
      }
      // all 64 lanes are here again
      unsigned long long bp = __ballot(pass), bc = __ballot(cand);
      count += __popcll(bc);
      if constexpr (CLAIMS) {
        const unsigned long long bk = __ballot(claim);
        claimed += __popcll(bk);
        bc &= ~bk;
      }
      if (lane == 0) { s_pass[r * wx + k] = bp; s_cand[r * wx + k] = bc; }
    }
  }
  if constexpr (CLAIMS) {
    if (lane == 0) x.sum[w] = claimed;  // (read after the barrier below)
  }
  // the start: level 0, whatever its flag and map bit are
  const int sw = ((sz - lo2) * rows_y + (sy - lo1)) * wx + ((sx - lo0) >> 6);  // (< W: s is in the box)
  const unsigned long long sbit = 1ull << ((sx - lo0) & 63);
#pragma unroll
  for (int j = 0; j < REACH_OWN; j++) {
    const int u = t + 256 * j;
    if (u < W) { s_a[u] = u == sw ? sbit : 0ull; s_b[u] = 0ull; }
  }
  if (lane == 0) s_n[w] = count;
  __syncthreads();

  // ---- flood ----
  unsigned long long own_pass[REACH_OWN], own_cand[REACH_OWN], own_seen[REACH_OWN];
  unsigned own_nb[REACH_OWN];  // bit 0: owned (u < W); 1, 2: a word before / after in the same row; 4, 8: a row before / after in the slab; 16, 32: a slab below / above
#pragma unroll
  for (int j = 0; j < REACH_OWN; j++) {
    const int u = t + 256 * j;
    const bool own = u < W;
    const int k = own ? u % wx : 0, r = own ? u / wx : 0, ry = r % rows_y, rz = r / rows_y;
    own_nb[j] = own ? (1u | (k > 0 ? 2u : 0u) | (k < wx - 1 ? 4u : 0u) | (ry > 0 ? 8u : 0u) | (ry < rows_y - 1 ? 16u : 0u) | (rz > 0 ? 32u : 0u) |
                       (rz < rows_z - 1 ? 64u : 0u))
                    : 0u;
    own_pass[j] = own ? s_pass[u] : 0ull;
    own_cand[j] = own ? s_cand[u] : 0ull;
    own_seen[j] = own && u == sw ? sbit : 0ull;
  }
  const int candidates = s_n[0] + s_n[1] + s_n[2] + s_n[3];
  unsigned long long* cur = s_a;
  unsigned long long* nxt = s_b;
  int n_reached = t == 0 ? 1 : 0, n_reachable = 0;  // sums over this thread's words (the start: thread 0's)
  int level = 0, hops = -1, best_cell = -1;
  double best = INFINITY;
  bool cut = false;
  bool hit = (s_cand[sw] & sbit) != 0ull;  // a candidate in the level that cur holds (uniform)
  if (hit && t == 0) n_reachable = 1;
  for (;;) {
    if (hit && hops < 0) {  // (uniform) the first level with a candidate: the smallest (d2, c) of cur & cand
      double b_d2 = INFINITY;
      int b_c = 0x7fffffff;
#pragma unroll
      for (int j = 0; j < REACH_OWN; j++) {
        const int u = t + 256 * j;
        unsigned long long h = (own_nb[j] & 1u) ? cur[u] & own_cand[j] : 0ull;
        if (h) {
          const int k = u % wx, r = u / wx;
          const int iy = lo1 + r % rows_y, iz = lo2 + r / rows_y;
          const double qy = (iy + 0.5) * a.res + a.oy, qz = (iz + 0.5) * a.res + a.oz;
          const double dy = qy - py, dz = qz - pz;
          const double dy2 = dy * dy, dz2 = dz * dz;
          while (h) {
            const int ix = lo0 + 64 * k + (int)__builtin_ctzll(h);
            h &= h - 1ull;
            const double qx = (ix + 0.5) * a.res + a.ox;
            const double dx = qx - px;
            const double d2 = dx * dx + dy2 + dz2;
            const int c = (iz * a.ny + iy) * a.nx + ix;
            if (reach_before(d2, c, b_d2, b_c)) { b_d2 = d2; b_c = c; }
          }
        }
      }
      // all 64 lanes are here again (no NaN: a d2 that is kept has passed d2 < r2 in the build)
      const double wave_d2 = fhw::wave_min(b_d2);
      const int wave_c = fhw::wave_min_i32(b_d2 == wave_d2 ? b_c : 0x7fffffff);
      if (lane == 0) { s_d2[w] = wave_d2; s_c[w] = wave_c; }
      __syncthreads();
      best = s_d2[0];
      best_cell = s_c[0];
      for (int k = 1; k < 4; k++)
        if (reach_before(s_d2[k], s_c[k], best, best_cell)) { best = s_d2[k]; best_cell = s_c[k]; }
      hops = level;
    }
    if (a.max_hops > 0 && level >= a.max_hops) {  // (cur is never empty)
      cut = true;
      break;
    }
    unsigned any = 0u;
#pragma unroll
    for (int j = 0; j < REACH_OWN; j++) {
      if (!(own_nb[j] & 1u)) continue;
      const int u = t + 256 * j;
      const unsigned nb = own_nb[j];
      const unsigned long long c = cur[u];
      unsigned long long v = (c << 1) | (c >> 1);
      if (nb & 2u) v |= cur[u - 1] >> 63;
      if (nb & 4u) v |= cur[u + 1] << 63;
      if (nb & 8u) v |= cur[u - wx];
      if (nb & 16u) v |= cur[u + wx];
      if (nb & 32u) v |= cur[u - slab];
      if (nb & 64u) v |= cur[u + slab];
      v &= own_pass[j] & ~own_seen[j];
      nxt[u] = v;
      own_seen[j] |= v;
      const unsigned long long h = v & own_cand[j];
      n_reached += __popcll(v);
      n_reachable += __popcll(h);
      any |= (v ? 1u : 0u) | (h ? 2u : 0u);
    }
    const unsigned wave_any = fhw::wave_or(any);
    if (lane == 0) s_or[level & 1][w] = wave_any;
    __syncthreads();
    const unsigned all = s_or[level & 1][0] | s_or[level & 1][1] | s_or[level & 1][2] | s_or[level & 1][3];
    if (!(all & 1u)) break;
    level++;
    hit = (all & 2u) != 0u;
    unsigned long long* const swap = cur;
    cur = nxt;
    nxt = swap;
  }
  const int wave_reached = fhw::wave_sum_i32(n_reached), wave_reachable = fhw::wave_sum_i32(n_reachable);
  __syncthreads();  // (s_n was read above by every thread)
  if (lane == 0) { s_n[w] = wave_reached; s_m[w] = wave_reachable; }
  __syncthreads();
  if (t == 0) {
    ReachCounts n;
    n.hops = hops; n.candidates = candidates;
    n.reachable = s_m[0] + s_m[1] + s_m[2] + s_m[3];
    n.reached = s_n[0] + s_n[1] + s_n[2] + s_n[3];
    n.levels = level;
    if (cut) flags |= FH_REACH_CUT;
    if constexpr (CLAIMS) x.store(a, i, flags, view, hops >= 0 ? best_cell : -1, hops >= 0 ? best : INFINITY, n, x.sum[0] + x.sum[1] + x.sum[2] + x.sum[3]);
    else reach_store(a, i, flags, view, hops >= 0 ? best_cell : -1, hops >= 0 ? best : INFINITY, n);
  }
}

__global__ void __launch_bounds__(256) reach_goals_kernel(ReachArgs a) { reach_body<false>(a, ReachNoClaims()); }

}  // namespace fhp

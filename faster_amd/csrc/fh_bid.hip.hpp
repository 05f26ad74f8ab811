// fh_bid.hip.hpp — the kernels of include/fasterhip_bid.h (which is the specification): K18's search inside rounds that are ordered by
// bids, not by the vehicle index.  Included by fh_reach.hip only, after the headers of the choosers before it, whose helpers are called
// here (gain_ball, gain_take, GainBest, the key helpers of K17; the reach_ helpers); the class kernel of fh_spread.hip.hpp is launched
// as it is.  d_work: the class bytes, the rows of FH_BID_LIST, an offer of two words per vehicle, two buffers of "decided in round" words.
//   bid_peers_kernel  : a wavefront per vehicle: the scan of K18's peers kernel with the rivals on both sides of the index; the slots
//                       of a row beyond the list hold -1, so a row entry is a vehicle iff it lies in [0, n).  Writes buffer 0 of the
//                       decided words (0: no searcher or OVERFLOW, -1: undecided), "no offer", and the outputs of pass 0.
//   bid_goals_kernel  : launched once per round p, a workgroup of 256 per vehicle.  It returns at once unless the vehicle is undecided
//                       (buffer (p - 1) & 1) and due a search: p == 1, or a listed rival was decided in round p - 1 with d_mask == 1.
//                       The claims (standing vehicles, and rivals decided in earlier rounds with d_mask == 1: what they wrote to d_goals
//                       and d_mask is final, their workgroups of this launch return at once) go to LDS as in K18's kernel, then K18's
//                       body: build with CLAIMED, cover by the owners of the words of `unk`, flood, gain.  It writes the provisional
//                       outputs and the offer: K17's 64-bit key as two words, or "none".
//   bid_settle_kernel : launched once per round p, a wavefront per vehicle; lane j holds slot j of the row.  It reads the decided words
//                       of buffer (p - 1) & 1 and the offers, and writes the decided word of its own vehicle to buffer p & 1 and
//                       decided_pass to the record: no launch reads a word that another workgroup of the same launch writes.  One
//                       ballot decides: a rival that was undecided, has an offer and beats this vehicle's blocks it.  The last launch
//                       rewrites the outputs of the vehicles still undecided (UNSETTLED).
// No atomics, no spin.  LDS of bid_goals_kernel: 4 bitmaps of FH_REACH_MAX_WORDS words = 32 KB static, 64 x 3 doubles, 64 x 3 ints, the
// slots of the reductions.  Every address comes from a checked number: a row entry is tested against [0, n), a claim voxel is an int
// only after it was found within claim_radius of the box as a double, and a word of `unk` is named by u < W.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fasterhip_bid.h"
#include "fh_wave.hip.hpp"
// (ReachArgs, the reach_ helpers, SPREAD_*, GainArgs, GainBest and the gain_ helpers: fh_reach.hip includes their headers before this one)

namespace fhp {

static_assert(sizeof(fh_bid_record) == 96 && sizeof(fh_bid_params) == 80 && FH_BID_LIST == 64, "include/fasterhip_bid.h: a lane per slot of a row");

constexpr int BID_NONE_HI = (int)0x80000000u;  // the high word of "no offer": below every key (|key| < 2^47)

struct BidArgs {
  GainArgs gn;                 // gn.r: the lattice, the views, the map, d_goals and d_mask; g, g2, hop_cost, min_gain (gn.records is not used)
  double s2, reach2, near2;    // r_spread^2, ((r_max + r_max) + r_int)^2, (r_max + r_int)^2: rounded once on the host
  int n, pass, last;           // last: pass == passes (the settle kernel rewrites the undecided)
  int cr, cr2;                 // claim_radius (-1: nothing is covered) and its square
  const int32_t* group;
  const unsigned char* cls;    // [n], written by spread_class_kernel
  int32_t* rows;               // [n][FH_BID_LIST]
  int32_t* offers;             // [n][2]: the key, low word first
  int32_t* decided;            // [2][n]: round p reads buffer (p - 1) & 1 and writes buffer p & 1
  fh_bid_record* records;
};

__device__ __forceinline__ int bid_group(const BidArgs& s, int view) { return s.group ? s.group[view] : view; }

__device__ __forceinline__ long long bid_offer(const BidArgs& s, int k) {
  const unsigned lo = (unsigned)s.offers[2 * (size_t)k];
  const int hi = s.offers[2 * (size_t)k + 1];
  return (long long)(((unsigned long long)(unsigned)hi << 32) | lo);
}
__device__ __forceinline__ void bid_set_offer(const BidArgs& s, int i, bool some, long long key) {
  s.offers[2 * (size_t)i] = some ? (int)(unsigned)((unsigned long long)key & 0xffffffffull) : 0;
  s.offers[2 * (size_t)i + 1] = some ? (int)(unsigned)((unsigned long long)key >> 32) : BID_NONE_HI;
}
__device__ __forceinline__ bool bid_is_offer(long long key) { return (int)(key >> 32) != BID_NONE_HI; }

// what a vehicle that is not searched has in the last eight words
struct BidGain {
  int gain, utility, poor, best_gain, covered;
};

// the three outputs of vehicle i, by one thread
__device__ __forceinline__ void bid_store(const BidArgs& s, int i, int flags, int view, int cell, int hops, double d2, int candidates,
                                          int reachable, int reached, int levels, int group, int decided_pass, int rivals, int claims,
                                          int claimed, int searches, const BidGain& q) {
#pragma clang fp contract(off)
  const ReachArgs& a = s.gn.r;
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
    if (claimed > 0) flags |= FH_BID_CLAIMED;
  }
  a.mask[i] = cell >= 0 ? 1 : 0;
  fh_bid_record r;
  r.flags = flags; r.view = view; r.cell = cell; r.hops = hops;
  r.candidates = candidates; r.reachable = reachable; r.reached = reached; r.levels = levels;
  r.d2 = d2;
  r.group = group; r.decided_pass = decided_pass; r.rivals = rivals; r.claims = claims; r.claimed = claimed; r.searches = searches;
  r.gain = q.gain; r.utility = q.utility; r.poor = q.poor; r.best_gain = q.best_gain; r.covered = q.covered;
  r.reserved[0] = 0; r.reserved[1] = 0; r.reserved[2] = 0;
  s.records[i] = r;
}

// a vehicle that is not searched, or whose search ends before the box
__device__ __forceinline__ void bid_store_idle(const BidArgs& s, int i, int flags, int view, int group, int decided_pass, int rivals, int claims,
                                               int searches) {
  const BidGain none = {-1, 0, 0, -1, 0};
  bid_store(s, i, flags, view, -1, -1, INFINITY, 0, 0, 0, 0, group, decided_pass, rivals, claims, 0, searches, none);
}

__global__ void __launch_bounds__(64) bid_peers_kernel(BidArgs s) {
#pragma clang fp contract(off)
  const ReachArgs& a = s.gn.r;
  const int i = (int)blockIdx.x, lane = (int)threadIdx.x;
  const int mine = fhw::uniform_i32((int)s.cls[i]);
  const int view = fhw::uniform_i32(a.view_of ? a.view_of[i] : i);
  const int flags = mine & 63;
  const int group = (flags & FH_FRONTIER_NO_VIEW) ? 0 : fhw::uniform_i32(bid_group(s, view));
  int32_t* row = s.rows + (size_t)i * FH_BID_LIST;
  if ((mine >> 6) != SPREAD_SEARCHER) {
    row[lane] = -1;
    if (lane == 0) {
      bid_store_idle(s, i, flags, view, group, 0, 0, 0, 0);
      bid_set_offer(s, i, false, 0ll);
      s.decided[i] = 0;
    }
    return;
  }
  const fh_vehicle& V = a.vehicles[i];
  const double px = fhw::uniform_f64(V.state.pos[0]), py = fhw::uniform_f64(V.state.pos[1]), pz = fhw::uniform_f64(V.state.pos[2]);
  int total = 0, rivals = 0, standing = 0;  // (uniform: sums of popcounts of ballots)
  for (int base = 0; base < s.n; base += 64) {
    const int k = base + lane;
    const int ck = k < s.n ? (int)s.cls[k] >> 6 : SPREAD_NONE;
    bool riv = false, stand = false;
    if (k != i && (ck == SPREAD_SEARCHER || ck == SPREAD_STANDING)) {  // (its view is in range: the class says so)
      const int vk = a.view_of ? a.view_of[k] : k;
      if (bid_group(s, vk) == group) {
        const fh_vehicle& K = a.vehicles[k];
        const double* c = ck == SPREAD_SEARCHER ? K.state.pos : K.g_term;
        const double dx = c[0] - px, dy = c[1] - py, dz = c[2] - pz;
        const double d2 = dx * dx + dy * dy + dz * dz;  // (the same bits from k's side: the squares of -dx, -dy, -dz)
        riv = ck == SPREAD_SEARCHER && d2 < s.reach2;
        stand = ck == SPREAD_STANDING && d2 < s.near2;
      }
    }
    // all 64 lanes are here again
    const unsigned long long br = __ballot(riv), bs = __ballot(stand), both = br | bs;
    const int slot = total + fhw::rank_in(both);
    if ((riv || stand) && slot < FH_BID_LIST) row[slot] = k;
    total += __popcll(both);
    rivals += __popcll(br);
    standing += __popcll(bs);
  }
  if (lane >= total) row[lane] = -1;  // (lane < FH_BID_LIST: a slot beyond the list names nobody)
  if (lane == 0) {
    const bool over = total > FH_BID_LIST;
    bid_store_idle(s, i, flags | (over ? FH_BID_OVERFLOW : FH_BID_UNSETTLED), view, group, over ? 0 : -1, rivals, standing, 0);
    bid_set_offer(s, i, false, 0ll);
    s.decided[i] = over ? 0 : -1;
  }
}

__global__ void __launch_bounds__(64) bid_settle_kernel(BidArgs s) {
  const ReachArgs& a = s.gn.r;
  const int i = (int)blockIdx.x, lane = (int)threadIdx.x;
  const int32_t* prev = s.decided + (size_t)((s.pass - 1) & 1) * s.n;
  int32_t* cur = s.decided + (size_t)(s.pass & 1) * s.n;
  const int before = fhw::uniform_i32(prev[i]);
  if (before != -1) {  // decided in an earlier round, or never a bidder
    if (lane == 0) cur[i] = before;
    return;
  }
  const int k = s.rows[(size_t)i * FH_BID_LIST + lane];
  const bool listed = k >= 0 && k < s.n;
  const int ck = listed ? (int)s.cls[k] >> 6 : SPREAD_NONE;
  const long long mine = bid_offer(s, i);  // (uniform: every lane reads the same two words)
  bool blocks = false;
  if (ck == SPREAD_SEARCHER && bid_is_offer(mine) && prev[k] == -1) {  // a rival that was undecided at the start of this round
    const long long theirs = bid_offer(s, k);
    blocks = bid_is_offer(theirs) && (theirs > mine || (theirs == mine && k < i));
  }
  // all 64 lanes are here again
  const bool decided = __ballot(blocks) == 0ull;  // (no offer: nobody blocks)
  const int standing = (int)__popcll(__ballot(ck == SPREAD_STANDING));
  if (lane != 0) return;
  if (decided) {
    cur[i] = s.pass;
    s.records[i].decided_pass = s.pass;
    return;
  }
  cur[i] = -1;
  if (s.last) {  // UNSETTLED: the outputs of a vehicle that is not searched; it keeps its rivals and its searches
    const fh_bid_record& R = s.records[i];
    bid_store_idle(s, i, ((int)s.cls[i] & 63) | FH_BID_UNSETTLED, a.view_of ? a.view_of[i] : i, R.group, -1, R.rivals, standing, R.searches);
  }
}

__global__ void __launch_bounds__(256) bid_goals_kernel(BidArgs s) {
#pragma clang fp contract(off)
  __shared__ unsigned long long s_pass[REACH_WORDS], s_cand[REACH_WORDS], s_a[REACH_WORDS], s_unk[REACH_WORDS];
  __shared__ double s_pts[3 * FH_BID_LIST];
  __shared__ int s_vox[3 * FH_BID_LIST];
  __shared__ double s_d2[4];
  __shared__ long long s_key[4];
  __shared__ int s_best[4][4], s_n[4], s_m[4], s_sum[4], s_cov[4], s_start;
  __shared__ unsigned s_or[2][4];
  const ReachArgs& a = s.gn.r;
  const int i = (int)blockIdx.x, t = (int)threadIdx.x, lane = t & 63, w = t >> 6;
  // ---- is this vehicle searched in this round?  (the same in all four wavefronts) ----
  const int32_t* prev = s.decided + (size_t)((s.pass - 1) & 1) * s.n;
  if (fhw::uniform_i32(prev[i]) != -1) return;  // decided, or no bidder
  const fh_bid_record& R = s.records[i];  // (only this workgroup and this vehicle's wavefront of the settle kernel write it: other launches)
  const int rivals = fhw::uniform_i32(R.rivals), group = fhw::uniform_i32(R.group), searches = fhw::uniform_i32(R.searches) + 1;
  const int k = s.rows[(size_t)i * FH_BID_LIST + lane];
  const bool listed = k >= 0 && k < s.n;
  const int ck = listed ? (int)s.cls[k] >> 6 : SPREAD_NONE;
  const int dk = ck == SPREAD_SEARCHER ? prev[k] : 0;
  const bool won = dk >= 1 && dk < s.pass && a.mask[k] == 1;  // (d_goals and d_mask of a decided rival: an earlier launch wrote them)
  if (s.pass > 1 && __ballot(won && dk == s.pass - 1) == 0ull) return;  // the claims are those of the last search: the offer stands
  const bool low = won;                          // (K18's name: a claim read from d_goals)
  const bool has = won || ck == SPREAD_STANDING;
  const unsigned long long bh = __ballot(has);
  const int n_claims = __popcll(bh);

  // ---- the vehicle, as K17's kernel reads it (a searcher: the exits below were judged by the class kernel, and are tested all the same) ----
  const fh_vehicle& V = a.vehicles[i];
  const int view = fhw::uniform_i32(a.view_of ? a.view_of[i] : i);
  const int status = fhw::uniform_i32(V.status), stage = fhw::uniform_i32(V.stage);
  const double px = fhw::uniform_f64(V.state.pos[0]), py = fhw::uniform_f64(V.state.pos[1]), pz = fhw::uniform_f64(V.state.pos[2]);
  const double gx = fhw::uniform_f64(V.g_term[0]), gy = fhw::uniform_f64(V.g_term[1]), gz = fhw::uniform_f64(V.g_term[2]);
  const bool wanted = ((a.want & FH_FRONTIER_WANT_REACHED) && status == FH_VEHICLE_GOAL_REACHED) ||
                      ((a.want & FH_FRONTIER_WANT_NO_PATH) && stage == FH_FLEET_STAGE_NO_PATH) || (a.want & FH_FRONTIER_WANT_ALL);
  const bool finite = reach_finite(px) && reach_finite(py) && reach_finite(pz) && reach_finite(gx) && reach_finite(gy) && reach_finite(gz);
  int flags = (wanted ? FH_FRONTIER_WANTED : 0) | (view >= 0 && view < a.n_views ? 0 : FH_FRONTIER_NO_VIEW) | (finite ? 0 : FH_FRONTIER_BAD_POS);
  if (flags != FH_FRONTIER_WANTED) {  // not eligible (uniform over the workgroup): no offer
    if (t == 0) {
      bid_store_idle(s, i, flags, view, group, -1, rivals, n_claims, searches);
      bid_set_offer(s, i, false, 0ll);
    }
    return;
  }
  // the start cell, tested as a double before it is an index
  const double sfx = floor((px - a.ox) / a.res), sfy = floor((py - a.oy) / a.res), sfz = floor((pz - a.oz) / a.res);
  if (!(sfx >= 0.0 && sfx < (double)a.nx && sfy >= 0.0 && sfy < (double)a.ny && sfz >= 0.0 && sfz < (double)a.nz)) {
    if (t == 0) {
      bid_store_idle(s, i, flags | FH_REACH_START_OUTSIDE, view, group, -1, rivals, n_claims, searches);
      bid_set_offer(s, i, false, 0ll);
    }
    return;
  }
  const int sx = (int)sfx, sy = (int)sfy, sz = (int)sfz;
  const unsigned char* F = a.flags + (size_t)view * a.view_stride;
  const int lo0 = reach_box_lo(floor((px - a.r_max - a.ox) / a.res) - 1.0, a.nx), hi0 = reach_box_hi(floor((px + a.r_max - a.ox) / a.res) + 1.0, a.nx);
  const int lo1 = reach_box_lo(floor((py - a.r_max - a.oy) / a.res) - 1.0, a.ny), hi1 = reach_box_hi(floor((py + a.r_max - a.oy) / a.res) + 1.0, a.ny);
  const int lo2 = reach_box_lo(floor((pz - a.r_max - a.oz) / a.res) - 1.0, a.nz), hi2 = reach_box_hi(floor((pz + a.r_max - a.oz) / a.res) + 1.0, a.nz);
  const bool holds = lo0 <= sx && sx <= hi0 && lo1 <= sy && sy <= hi1 && lo2 <= sz && sz <= hi2;
  const int rows_y = hi1 - lo1 + 1, rows_z = hi2 - lo2 + 1;
  const int wx = holds ? (hi0 - lo0 + 64) >> 6 : 0;                     // (hi0 - lo0 + 1 <= nx: no overflow)
  const long long words = (long long)wx * rows_y * rows_z;            // (rows_y rows_z <= ny nz < 2^31, wx < 2^26)
  if (!holds || words > (long long)REACH_WORDS) {
    if (t == 0) {
      bid_store_idle(s, i, flags | FH_REACH_BOX_TOO_LARGE, view, group, -1, rivals, n_claims, searches);
      bid_set_offer(s, i, false, 0ll);
    }
    return;
  }
  const int W = (int)words, rows = rows_y * rows_z, slab = wx * rows_y, nbx = hi0 - lo0 + 1;
  const int slice = a.nx * a.ny;
  const int sw = ((sz - lo2) * rows_y + (sy - lo1)) * wx + ((sx - lo0) >> 6);  // the start's word (< W: s is in the box)
  const unsigned long long sbit = 1ull << ((sx - lo0) & 63);

  // ---- the claims: every wavefront writes the same values to the same slots ----
  bool ball = false;  // the ball of this lane's claim touches the box
  int kx = 0, ky = 0, kz = 0;
  if (has) {
    const double* c = low ? a.goals + 3 * (size_t)k : a.vehicles[k].g_term;
    const double cx = c[0], cy = c[1], cz = c[2];
    const int j = fhw::rank_in(bh);  // (< FH_BID_LIST: a lane per claim)
    s_pts[3 * j] = cx; s_pts[3 * j + 1] = cy; s_pts[3 * j + 2] = cz;
    if (s.cr >= 0) {  // the claim voxel, tested as a double against the box widened by the radius before it is an int (a NaN fails)
      const double fx = floor((cx - a.ox) / a.res), fy = floor((cy - a.oy) / a.res), fz = floor((cz - a.oz) / a.res);
      ball = fx >= (double)(lo0 - s.cr) && fx <= (double)(hi0 + s.cr) && fy >= (double)(lo1 - s.cr) && fy <= (double)(hi1 + s.cr) &&
             fz >= (double)(lo2 - s.cr) && fz <= (double)(hi2 + s.cr);
      if (ball) { kx = (int)fx; ky = (int)fy; kz = (int)fz; }
    }
  }
  const unsigned long long bb = __ballot(ball);
  if (ball) {
    const int j = fhw::rank_in(bb);
    s_vox[3 * j] = kx; s_vox[3 * j + 1] = ky; s_vox[3 * j + 2] = kz;
  }
  const int n_balls = fhw::uniform_i32(__popcll(bb));  // (<= n_claims <= FH_BID_LIST)
  __syncthreads();

  // ---- build: pass, cand and unk, a wavefront per row; a claimed candidate is counted and leaves cand ----
  int count = 0, claimed = 0;  // (uniform over the wavefront: sums of popcounts of ballots)
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
    for (int kw = 0; kw < wx; kw++) {
      const int ix = lo0 + 64 * kw + lane;
      const int c = c0 + ix;
      const bool known = ix <= hi0 && F[c] == 0, unk = ix <= hi0 && !known;  // (a lane beyond hi0 reads nothing)
      bool pass = row_in_map && known;
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
      if (cand) {  // (n_claims is uniform; a point is read by every lane at once: a broadcast)
        for (int j = 0; j < n_claims; j++) {
          const double tx = s_pts[3 * j] - qx, ty = s_pts[3 * j + 1] - qy, tz = s_pts[3 * j + 2] - qz;
          const double t2 = tx * tx + ty * ty + tz * tz;
          claim = claim || t2 < s.s2;
        }
      }
      // all 64 lanes are here again
      const unsigned long long bp = __ballot(pass), bk = __ballot(claim), bu = __ballot(unk);
      unsigned long long bc = __ballot(cand);
      count += __popcll(bc);
      claimed += __popcll(bk);
      bc &= ~bk;
      if (lane == 0) {
        const int u = r * wx + kw;
        s_pass[u] = bp; s_cand[u] = bc; s_unk[u] = bu;
        if (u == sw) s_start = (bc & sbit) != 0ull ? 1 : 0;  // (one word of the box is the start's)
      }
    }
  }
  // the start: level 0, whatever its flag and map bit are
#pragma unroll
  for (int j = 0; j < REACH_OWN; j++) {
    const int u = t + 256 * j;
    if (u < W) s_a[u] = u == sw ? sbit : 0ull;
  }
  if (lane == 0) { s_n[w] = count; s_sum[w] = claimed; }
  __syncthreads();

  // ---- cover: the owner of a word of unk clears what the balls of the claims cover ----
  int n_covered = 0;  // over this thread's words
  if (n_balls > 0) {  // (uniform over the workgroup: the barrier below is reached by all or none)
#pragma unroll
    for (int j = 0; j < REACH_OWN; j++) {
      const int u = t + 256 * j;
      if (u >= W) continue;
      const int kw = u % wx, r = u / wx, iy = lo1 + r % rows_y, iz = lo2 + r / rows_y;
      const int x0 = 64 * kw, x1 = x0 + 63 < nbx - 1 ? x0 + 63 : nbx - 1;  // the box columns of this word (x0 <= x1: the word exists)
      unsigned long long cov = 0ull;
      for (int m = 0; m < n_balls; m++) {  // (a claim voxel is read by every lane at once: a broadcast)
        const int dy = iy - s_vox[3 * m + 1], dz = iz - s_vox[3 * m + 2];  // (|.| <= FH_REACH_MAX_WORDS + 31: the squares fit)
        const int rem = s.cr2 - dy * dy - dz * dz;
        if (rem < 0) continue;
        int hx = 0;  // the largest h with h h <= rem (rem <= 961: h <= 31)
#pragma unroll
        for (int b = 16; b > 0; b >>= 1) {
          const int h = hx + b;
          hx = h * h <= rem ? h : hx;
        }
        const int cx = s_vox[3 * m] - lo0;  // the claim's column of the box, in [-31 - nbx, nbx + 31]
        const int xa = cx - hx > x0 ? cx - hx : x0, xb = cx + hx < x1 ? cx + hx : x1;
        if (xa <= xb) cov |= (~0ull << (xa - x0)) & (~0ull >> (63 - (xb - x0)));  // (0 <= xa - x0 <= xb - x0 <= 63)
      }
      const unsigned long long word = s_unk[u], gone = word & cov;
      n_covered += __popcll(gone);
      s_unk[u] = word & ~gone;
    }
    __syncthreads();
  }
  const int wave_covered = fhw::wave_sum_i32(n_covered);
  if (lane == 0) s_cov[w] = wave_covered;  // (read by thread 0 after the barriers at the end)

  // ---- flood, and the gain of the candidates of every level: the body of K17's kernel ----
  unsigned long long own_pass[REACH_OWN], own_cand[REACH_OWN], own_seen[REACH_OWN];
  unsigned own_nb[REACH_OWN];  // bit 0: owned (u < W); 1, 2: a word before / after in the same row; 4, 8: a row before / after in the slab; 16, 32: a slab below / above
#pragma unroll
  for (int j = 0; j < REACH_OWN; j++) {
    const int u = t + 256 * j;
    const bool own = u < W;
    const int kw = own ? u % wx : 0, r = own ? u / wx : 0, ry = r % rows_y, rz = r / rows_y;
    own_nb[j] = own ? (1u | (kw > 0 ? 2u : 0u) | (kw < wx - 1 ? 4u : 0u) | (ry > 0 ? 8u : 0u) | (ry < rows_y - 1 ? 16u : 0u) | (rz > 0 ? 32u : 0u) |
                       (rz < rows_z - 1 ? 64u : 0u))
                    : 0u;
    own_pass[j] = own ? s_pass[u] : 0ull;  // (a word of pass and of cand is read by its owner alone: from here on their arrays are
    own_cand[j] = own ? s_cand[u] : 0ull;  //  the first nxt and the hit words, which a word's owner alone writes)
    own_seen[j] = own && u == sw ? sbit : 0ull;
  }
  const int candidates = s_n[0] + s_n[1] + s_n[2] + s_n[3];
  const int n_claimed = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
  unsigned long long* cur = s_a;
  unsigned long long* nxt = s_pass;
  unsigned long long* const s_hit = s_cand;
  GainBest best = {0ll, INFINITY, -1, -1, 0, -1};
  int n_reached = t == 0 ? 1 : 0, n_reachable = 0;  // sums over this thread's words (the start: thread 0's)
  int level = 0;
  bool cut = false;
  bool hit = fhw::uniform_i32(s_start) != 0;  // a candidate in the level that cur holds
  if (hit && t == 0) n_reachable = 1;
  for (;;) {
    if (hit) {  // (uniform) the candidates of this level, each with its gain
      if (level == 0) {  // the start itself, by the first wavefront (the hit words are not written yet)
        if (w == 0) {
          const double qy = (sy + 0.5) * a.res + a.oy, qz = (sz + 0.5) * a.res + a.oz;
          const double dy = qy - py, dz = qz - pz;
          const double dy2 = dy * dy, dz2 = dz * dz;
          const double qx = (sx + 0.5) * a.res + a.ox;
          const double dx = qx - px;
          const double d2 = dx * dx + dy2 + dz2;
          const int gain = gain_ball(s_unk, sx - lo0, sy - lo1, sz - lo2, nbx, rows_y, rows_z, wx, s.gn.g, s.gn.g2, lane);
          gain_take(best, s.gn, gain, 0, d2, (sz * a.ny + sy) * a.nx + sx);
        }
      } else {
        for (int base = 0; base < W; base += 256) {  // wavefront w: the hit words u = w (mod 4), 64 at a time
          const int mine = base + 4 * lane + w;
          unsigned long long m = __ballot(mine < W && s_hit[mine] != 0ull);
          while (m) {  // (uniform)
            const int u = base + 4 * (int)__builtin_ctzll(m) + w;  // (< W: its lane has tested it)
            m &= m - 1ull;
            const unsigned long long hw = s_hit[u];
            unsigned h_lo = (unsigned)fhw::uniform_i32((int)(unsigned)hw), h_hi = (unsigned)fhw::uniform_i32((int)(unsigned)(hw >> 32));
            const int kw = u % wx, r = u / wx, ry = r % rows_y, rz = r / rows_y;
            const int iy = lo1 + ry, iz = lo2 + rz;
            const double qy = (iy + 0.5) * a.res + a.oy, qz = (iz + 0.5) * a.res + a.oz;
            const double dy = qy - py, dz = qz - pz;
            const double dy2 = dy * dy, dz2 = dz * dz;
            while (h_lo | h_hi) {
              int b;
              if (h_lo) { b = (int)__builtin_ctz(h_lo); h_lo &= h_lo - 1u; }
              else { b = 32 + (int)__builtin_ctz(h_hi); h_hi &= h_hi - 1u; }
              const int bx = 64 * kw + b, ix = lo0 + bx;
              const double qx = (ix + 0.5) * a.res + a.ox;
              const double dx = qx - px;
              const double d2 = dx * dx + dy2 + dz2;
              const int gain = gain_ball(s_unk, bx, ry, rz, nbx, rows_y, rows_z, wx, s.gn.g, s.gn.g2, lane);
              gain_take(best, s.gn, gain, level, d2, (iz * a.ny + iy) * a.nx + ix);
            }
          }
        }
      }
    }
    if (a.max_hops > 0 && level >= a.max_hops) {  // (cur is never empty)
      cut = true;
      break;
    }
    if (hit) __syncthreads();  // every wavefront has read this level's hit words before the next level's are written
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
      s_hit[u] = h;
      n_reached += __popcll(v);
      n_reachable += __popcll(h);
      any |= (v ? 1u : 0u) | (h ? 2u : 0u);
    }
    const unsigned wave_any = fhw::wave_or(any);
    if (lane == 0) s_or[level & 1][w] = wave_any;
    __syncthreads();
    const unsigned all = (unsigned)fhw::uniform_i32((int)(s_or[level & 1][0] | s_or[level & 1][1] | s_or[level & 1][2] | s_or[level & 1][3]));
    if (!(all & 1u)) break;
    level++;
    hit = (all & 2u) != 0u;
    unsigned long long* const swap = cur;
    cur = nxt;
    nxt = swap;
  }
  const int wave_reached = fhw::wave_sum_i32(n_reached), wave_reachable = fhw::wave_sum_i32(n_reachable);
  __syncthreads();  // (s_n was read above by every thread)
  if (lane == 0) {
    s_n[w] = wave_reached; s_m[w] = wave_reachable;
    s_best[w][0] = best.cell; s_best[w][1] = best.gain; s_best[w][2] = best.poor; s_best[w][3] = best.best_gain;
    s_key[w] = best.key;
    s_d2[w] = best.d2;
  }
  __syncthreads();
  if (t == 0) {
    GainBest b = {0ll, INFINITY, -1, -1, 0, -1};
    for (int m = 0; m < 4; m++) {
      const bool take = s_best[m][0] >= 0 && gain_before(s_key[m], s_d2[m], s_best[m][0], b);
      b.key = take ? s_key[m] : b.key;
      b.d2 = take ? s_d2[m] : b.d2;
      b.cell = take ? s_best[m][0] : b.cell;
      b.gain = take ? s_best[m][1] : b.gain;
      b.poor += s_best[m][2];
      b.best_gain = s_best[m][3] > b.best_gain ? s_best[m][3] : b.best_gain;
    }
    const int reachable = s_m[0] + s_m[1] + s_m[2] + s_m[3], reached = s_n[0] + s_n[1] + s_n[2] + s_n[3];
    if (cut) flags |= FH_REACH_CUT;
    if (reachable > 0 && b.poor == reachable) flags |= FH_BID_ALL_POOR;
    const bool found = b.cell >= 0;
    BidGain q;
    q.gain = found ? b.gain : -1; q.utility = found ? gain_key_utility(b.key) : 0; q.poor = b.poor; q.best_gain = b.best_gain;
    q.covered = s_cov[0] + s_cov[1] + s_cov[2] + s_cov[3];
    // provisional: the settle kernel of the round that makes the offer final writes decided_pass
    bid_store(s, i, flags, view, found ? b.cell : -1, found ? gain_key_hops(b.key) : -1, found ? b.d2 : INFINITY, candidates, reachable, reached,
              level, group, -1, rivals, n_claims, n_claimed, searches, q);
    bid_set_offer(s, i, found, b.key);
  }
}

}  // namespace fhp

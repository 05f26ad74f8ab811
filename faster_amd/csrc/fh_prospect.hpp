// fh_prospect.hpp — the kernels of include/fasterhip_prospect.h (which is the specification): the far chooser (K21) with a gain, the
// unknown voxels of a cube of blocks around a target block, and the choice by utility = gain - hop_cost * hops over ALL levels of the
// flood.  Included by fh_reach.hip only, after K21's device header (which stays the last *.hip.hpp) and before the device header of the
// far chooser for a team (which stays the last include).  d_work: K21's workspace, then [n_views][64 W] counts of 16 bits.  The need
// bytes are written by far_need_kernel as it is.
//   prospect_blocks_kernel : a workgroup of 256 per (word of 64 blocks, view); it returns at once for a view nobody needs.  ONE pass
//                            over the flag bytes writes T, LX, LY, LZ and U.  A wavefront takes a LINE of voxels along x of the word's
//                            row of blocks, in runs of 64 voxels: lane = consecutive x, so a wavefront reads whole 64-byte lines.  The
//                            five answers of a voxel (unknown, target, link +x, +y, +z) are ballots over the run; lane j owns block
//                            64 k + j of the word and takes its share of a ballot by the mask of the block's voxels in the run —
//                            popcount(unknown & mask) is added to its count, (ballot & mask) != 0 is or-ed into its four bits.  That
//                            holds for every B in 1..16, also where blocks straddle two runs.  The neighbour bytes are loaded only
//                            for a voxel that is known, free and inside z.  The four wavefronts meet in LDS; the first one writes one
//                            64-bit word per bitmap by a ballot and the 64 counts of the word, 128 consecutive bytes.
//   prospect_goals_kernel  : ONE workgroup of 256 per vehicle.  Judge, summary into LDS, r_avoid out of T and the flood are K21's, on
//                            K21's helpers.  In EVERY level the thread that owns a word weighs each new bit of v & T: the gain from the
//                            counts in global memory (a row of the cube is at most 2 g - 1 consecutive uint16_t: the words of a row of
//                            x follow each other, so entry 64 (row wx) + bx' is block bx' of that row), the utility, poor or not, and
//                            a running best under the total order (-utility, hops, D2, b).  One reduction after the last level (wave,
//                            then LDS), then the voxel scan of the chosen block, once.  Its body is prospect_body<false>.
// prospect_body<true> is the pass kernel of the chooser by gain for a team (K24, the device header after this one): between the
// summary and the flood K21's claim scan takes the claimed blocks out of T and sets the covered ones in a SEVENTH bitmap C; each
// thread sums popcount(C[u]) and the U of the set bits of its words, covered and removed; and the weighing skips covered counts — a
// row of the cube is at most 9 consecutive counts, and the 9-bit piece of C that belongs to it is taken from one or two words.  A
// workgroup that covered nothing (a uniform flag) weighs as K23 does: prospect_weigh<false>.
// LDS of prospect_goals_kernel: 6 bitmaps of FAR_WORDS words = 24 KB static, and the slots of the reductions.
// Every address comes from a checked number: what K21's header lists, and the cube of a gain is clipped to [0, C_a) per axis before an
// entry of C or of the counts is loaded.  Integer work and minima of total orders; nothing depends on scheduling.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fasterhip_prospect.h"
// (FarArgs, FarStart, FarMaps, FarCounts, far_judge by far_start, far_summary, far_claim_scan, far_expand, far_level_any, far_scan_block,
// far_put_goal, far_head, far_passable, far_target, far_block_d2, reach_before and fhw:: come from K21's device header, which
// fh_reach.hip includes before this)

namespace fhp {

struct ProspectArgs {
  FarArgs f;  // (f.records is not used)
  int g, hop_cost, min_gain;
  uint16_t* counts;  // [n_views][64 W]
  fh_prospect_record* records;
};

__global__ void __launch_bounds__(256) prospect_blocks_kernel(ProspectArgs p) {
  __shared__ int s_u[4][64];
  __shared__ unsigned char s_f[4][64];
  const FarArgs& a = p.f;
  const ReachArgs& r = a.r;
  const int t = (int)threadIdx.x, lane = t & 63, w = t >> 6;
  const int word = (int)blockIdx.x;  // (< W: the grid)
  const int k = word % a.wx, row = word / a.wx, by = row % a.cy, bz = row / a.cy;
  const int y0 = by * a.B, y1 = min(y0 + a.B, r.ny), z0 = bz * a.B, z1 = min(z0 + a.B, r.nz);
  const bool has_y = by + 1 < a.cy, has_z = bz + 1 < a.cz;  // (then y1 = y0 + B < ny: the voxel above the block's last row is inside)
  const int xw = 64 * k * a.B;                              // the first voxel of the word (< nx: k < wx)
  const int span = min(xw + 64 * a.B, r.nx) - xw;           // its voxels along x, 1 .. 1024
  const int bh = y1 - y0, lines = bh * (z1 - z0);           // (<= 256)
  // the voxels [m0, m1) of the block this lane owns, clipped to the lattice; empty for a bit beyond Cx
  const int m0 = min((64 * k + lane) * a.B, r.nx), m1 = min(m0 + a.B, r.nx);
  for (int view = (int)blockIdx.y; view < r.n_views; view += (int)gridDim.y) {
    if (fhw::uniform_i32((int)a.need[view]) == 0) continue;  // (uniform over the workgroup)
    const unsigned char* F = r.flags + (size_t)view * r.view_stride;
    int u = 0;
    unsigned bits = 0u;  // 1: T, 2: LX, 4: LY, 8: LZ of the block this lane owns
    for (int l = w; l < lines; l += 4) {  // (l, iy and iz are uniform over the wavefront)
      const int iy = y0 + l % bh, iz = z0 + l / bh;
      const bool last_y = has_y && iy == y1 - 1, last_z = has_z && iz == z1 - 1;
      for (int xr = xw; xr < xw + span; xr += 64) {
        const int ix = xr + lane;
        bool vu = false, vt = false, vx = false, vy = false, vz = false;
        if (ix < r.nx) {
          vu = F[(iz * r.ny + iy) * r.nx + ix] != 0;
          if (!vu && far_passable(r, F, ix, iy, iz)) {
            vt = far_target(r, F, ix, iy, iz);
            vx = ix + 1 < r.nx && (ix + 1) % a.B == 0 && far_passable(r, F, ix + 1, iy, iz);  // the last voxel of a block that has a +x neighbour
            vy = last_y && far_passable(r, F, ix, iy + 1, iz);
            vz = last_z && far_passable(r, F, ix, iy, iz + 1);
          }
        }
        // all 64 lanes are here again
        const unsigned long long bu = __ballot(vu), bt = __ballot(vt), bx = __ballot(vx), bY = __ballot(vy), bZ = __ballot(vz);
        const int lo = max(m0, xr) - xr, hi = min(m1, xr + 64) - xr;  // the share of this lane's block in the run: hi - lo <= 16
        if (hi > lo) {
          const unsigned long long mask = ((1ull << (hi - lo)) - 1ull) << lo;
          u += __popcll(bu & mask);
          bits |= ((bt & mask) ? 1u : 0u) | ((bx & mask) ? 2u : 0u) | ((bY & mask) ? 4u : 0u) | ((bZ & mask) ? 8u : 0u);
        }
      }
    }
    s_u[w][lane] = u;
    s_f[w][lane] = (unsigned char)bits;
    __syncthreads();
    if (w == 0) {
      const int sum = s_u[0][lane] + s_u[1][lane] + s_u[2][lane] + s_u[3][lane];  // (<= 16^3)
      const unsigned all = (unsigned)(s_f[0][lane] | s_f[1][lane] | s_f[2][lane] | s_f[3][lane]);
      unsigned long long* out = a.sums + (size_t)view * 4u * (size_t)a.W + (size_t)word;
#pragma unroll
      for (int m = 0; m < 4; m++) {
        const unsigned long long b = __ballot(((all >> m) & 1u) != 0u);
        if (lane == 0) out[(size_t)m * (size_t)a.W] = b;
      }
      p.counts[((size_t)view * (size_t)a.W + (size_t)word) * 64u + (size_t)lane] = (uint16_t)sum;
    }
    __syncthreads();  // (s_u and s_f are written again for the next view)
  }
}

// the gain's words of a record
struct ProspectGain {
  int gain, utility, poor, best_gain;
};

template <class R>
__device__ __forceinline__ void prospect_words(R& q, const ProspectGain& e) {
  q.gain = e.gain; q.utility = e.utility; q.poor = e.poor; q.best_gain = e.best_gain;
}

// the three outputs of vehicle i, by one thread
__device__ __forceinline__ void prospect_store(const ProspectArgs& p, int i, int flags, int view, int cell, double d2, double block_d2,
                                               const FarCounts& n, const ProspectGain& e) {
  flags |= far_put_goal(p.f.r, i, cell);
  fh_prospect_record q;
  far_head(q, flags, view, cell, d2, block_d2, n);
  prospect_words(q, e);
  p.records[i] = q;
}

// the best target block a thread has seen so far, under the total order (-utility, hops, D2, b); b < 0: none
struct ProspectBest {
  int utility, hops, b, gain;
  double d2;
};

__device__ __forceinline__ bool prospect_before(int utility, int hops, double d2, int b, const ProspectBest& o) {
  if (o.b < 0) return true;
  if (utility != o.utility) return utility > o.utility;
  if (hops != o.hops) return hops < o.hops;
  return reach_before(d2, b, o.d2, o.b);
}

// Weighs the target blocks `h` (bits of word u) of level `hops`: the gain of each from the counts U of the view, with COVERED without
// the blocks whose bit of C (LDS, [W]) is set, poor or not, the running best; -> in poor and best_gain this thread's sums.
template <bool COVERED>
__device__ __forceinline__ void prospect_weigh(const ProspectArgs& p, const uint16_t* U, const unsigned long long* C, unsigned long long h, int u,
                                               int hops, double px, double py, double pz, ProspectBest& best, int& poor, int& best_gain) {
#pragma clang fp contract(off)
  const FarArgs& a = p.f;
  if (h == 0ull) return;
  const int k = u % a.wx, row = u / a.wx, by = row % a.cy, bz = row / a.cy;
  const int g = p.g;
  const int ylo = max(by - g + 1, 0), yhi = min(by + g - 1, a.cy - 1), zlo = max(bz - g + 1, 0), zhi = min(bz + g - 1, a.cz - 1);
  while (h) {
    const int bx = 64 * k + (int)__builtin_ctzll(h);  // (a set bit of T: bx < cx)
    h &= h - 1ull;
    const int xlo = max(bx - g + 1, 0), xhi = min(bx + g - 1, a.cx - 1);  // (g >= 1: 0 <= xlo <= bx <= xhi < cx, xhi - xlo <= 8)
    int gain = 0;
    if constexpr (COVERED) {
      if (g > 0) {
        const int w0 = xlo >> 6, w1 = xhi >> 6, sh = xlo & 63;  // (w0 <= w1 < wx; w1 > w0: sh >= 56)
        for (int z = zlo; z <= zhi; z++)
          for (int y = ylo; y <= yhi; y++) {
            const int rw = (z * a.cy + y) * a.wx;  // the first word of the row (< W)
            unsigned long long piece = C[rw + w0] >> sh;
            if (w1 != w0) piece |= C[rw + w1] << (64 - sh);
            const uint16_t* line = U + (size_t)rw * 64u;
            for (int x = xlo; x <= xhi; x++)
              if (!((piece >> (x - xlo)) & 1ull)) gain += (int)line[x];
          }
      }
    } else {
      for (int z = zlo; z <= zhi; z++)      // (g == 0: lo > hi on every axis, nothing is loaded)
        for (int y = ylo; y <= yhi; y++) {
          const uint16_t* line = U + (size_t)(z * a.cy + y) * (size_t)(64 * a.wx);
          for (int x = xlo; x <= xhi; x++) gain += (int)line[x];
        }
    }
    if (gain > best_gain) best_gain = gain;
    if (gain < p.min_gain) {
      poor++;
      continue;
    }
    const int utility = gain - p.hop_cost * hops;
    const double d2 = far_block_d2(a, bx, by, bz, px, py, pz);
    const int b = (bz * a.cy + by) * a.cx + bx;
    if (prospect_before(utility, hops, d2, b, best)) { best.utility = utility; best.hops = hops; best.d2 = d2; best.b = b; best.gain = gain; }
  }
}

struct ProspectNoClaims {};

// The body of prospect_goals_kernel, and with CLAIMS that of the pass kernel of the chooser by gain for a team: K21's claim scan
// with the covered set x.c between the summary and the flood, covered and removed summed into x.sum, the weighing without the
// covered counts unless nothing is covered, and x.store() for the longer record.  With CLAIMS false every `if constexpr` below is gone.
template <bool CLAIMS, class X>
__device__ __forceinline__ void prospect_body(const ProspectArgs& p, const X& x) {
#pragma clang fp contract(off)
  __shared__ unsigned long long s_t[FAR_WORDS], s_lx[FAR_WORDS], s_ly[FAR_WORDS], s_lz[FAR_WORDS], s_a[FAR_WORDS], s_b[FAR_WORDS];
  __shared__ double s_bd2[4];
  __shared__ int s_bu[4], s_bh[4], s_bc[4], s_bg[4], s_n[4], s_m[4], s_k[4], s_p[4], s_g[4];
  __shared__ unsigned s_or[2][4];
  const FarArgs& a = p.f;
  const ReachArgs& r = a.r;
  const int i = (int)blockIdx.x, t = (int)threadIdx.x, lane = t & 63, w = t >> 6;
  const FarStart st = far_start(a, i);
  const int view = st.view;
  int flags = st.who.flags;
  if (!st.who.searched) {  // (uniform over the workgroup)
    if constexpr (!CLAIMS) {  // (with CLAIMS the count kernel has written the outputs of a vehicle that is not searched)
      const FarCounts none = {-1, -1, 0, 0, 0, 0, 0};
      const ProspectGain no_gain = {-1, 0, 0, -1};
      if (t == 0) prospect_store(p, i, flags, view, -1, INFINITY, INFINITY, none, no_gain);
    }
    return;
  }
  const int W = a.W, wx = a.wx, slab = a.wx * a.cy, sw = st.sw;
  const unsigned long long sbit = st.sbit;
  const double px = st.px, py = st.py, pz = st.pz;
  const unsigned char* F = r.flags + (size_t)view * r.view_stride;
  const uint16_t* U = p.counts + (size_t)view * (size_t)W * 64u;
  const FarMaps maps = {s_t, s_lx, s_ly, s_lz, s_a, s_b};

  // ---- the view's summary into LDS, T without the blocks within r_avoid of g_term (K21's); with CLAIMS C starts empty ----
  unsigned long long own_seen[FAR_OWN];
  unsigned own_nb[FAR_OWN];
  const unsigned long long* C = nullptr;
  int n_targets, n_claims = 0, n_standing = 0;  // (the last two are uniform)
  if constexpr (CLAIMS) {
    n_targets = far_summary<true>(a, st, t, maps, x.c, own_seen, own_nb);
    // every thread takes the claimed blocks out of the words of T it owns and sets the covered blocks in the words of C it owns
    const int n_claimed = far_claim_scan<true>(a, x.team, i, t, s_t, x.c, n_claims, n_standing);
    // covered and removed: the set bits of the words of C this thread owns, and their counts
    int n_covered = 0, n_removed = 0;
    if (x.team.k > 0)
      for (int u = t; u < W; u += 256) {
        unsigned long long cw = x.c[u];
        n_covered += __popcll(cw);
        while (cw) {
          n_removed += (int)U[(size_t)u * 64u + (size_t)__builtin_ctzll(cw)];  // (<= 64 * 512 blocks of <= 4096 voxels: < 2^31)
          cw &= cw - 1ull;
        }
      }
    const int wave_claimed = fhw::wave_sum_i32(n_claimed), wave_covered = fhw::wave_sum_i32(n_covered), wave_removed = fhw::wave_sum_i32(n_removed);
    if (lane == 0) { x.sum[w] = wave_claimed; x.sum[4 + w] = wave_covered; x.sum[8 + w] = wave_removed; }
    C = x.c;
  } else {
    n_targets = far_summary<false>(a, st, t, maps, nullptr, own_seen, own_nb);
  }
  const int wave_targets = fhw::wave_sum_i32(n_targets);
  if (lane == 0) s_k[w] = wave_targets;
  __syncthreads();

  // ---- flood: every target block of every level is weighed by the thread that owns its word ----
  const int targets = s_k[0] + s_k[1] + s_k[2] + s_k[3];
  int covered = 0;  // (uniform) nothing is covered: the weighing without C
  if constexpr (CLAIMS) covered = x.sum[4] + x.sum[5] + x.sum[6] + x.sum[7];
  unsigned long long* cur = s_a;
  unsigned long long* nxt = s_b;
  int n_reached = t == 0 ? 1 : 0, n_reachable = 0;  // sums over this thread's words (the start: thread 0's)
  int n_poor = 0, top_gain = -1;
  ProspectBest mine = {0, 0, -1, 0, INFINITY};
  const auto weigh = [&](unsigned long long h, int u, int hops) {
    if constexpr (CLAIMS) {
      if (covered != 0) {
        prospect_weigh<true>(p, U, C, h, u, hops, px, py, pz, mine, n_poor, top_gain);
        return;
      }
    }
    prospect_weigh<false>(p, U, C, h, u, hops, px, py, pz, mine, n_poor, top_gain);
  };
  int level = 0;
  bool cut = false;
  if ((s_t[sw] & sbit) != 0ull && t == 0) n_reachable = 1;  // (uniform read) the start's block is a target block of level 0
  if (t == (sw & 255)) weigh(s_t[sw] & sbit, sw, 0);        // (the owner of word sw)
  for (;;) {
    if (r.max_hops > 0 && level >= r.max_hops) {  // (cur is never empty)
      cut = true;
      break;
    }
    unsigned any = 0u;
#pragma unroll
    for (int j = 0; j < FAR_OWN; j++) {
      if (!(own_nb[j] & 1u)) continue;
      const int u = t + 256 * j;
      const unsigned long long v = far_expand(maps, cur, nxt, u, own_nb[j], wx, slab, own_seen[j]);
      const unsigned long long h = v & s_t[u];
      n_reached += __popcll(v);
      n_reachable += __popcll(h);
      any |= v ? 1u : 0u;
      weigh(h, u, level + 1);
    }
    const unsigned all = far_level_any(any, s_or, level, lane, w);
    if (!(all & 1u)) break;
    level++;
    unsigned long long* const swap = cur;
    cur = nxt;
    nxt = swap;
  }

  // ---- the smallest (-utility, hops, D2, b) of the workgroup: the wavefront's, then the four through LDS ----
  const bool have = mine.b >= 0;
  const int wave_nu = fhw::wave_min_i32(have ? -mine.utility : 0x7fffffff);  // (|utility| < 2^30)
  const bool in_u = have && -mine.utility == wave_nu;
  const int wave_h = fhw::wave_min_i32(in_u ? mine.hops : 0x7fffffff);
  const bool in_h = in_u && mine.hops == wave_h;
  const double wave_d2 = fhw::wave_min(in_h ? mine.d2 : INFINITY);  // (no NaN: the gaps are differences of finite numbers)
  const bool in_d = in_h && mine.d2 == wave_d2;
  const int wave_b = fhw::wave_min_i32(in_d ? mine.b : 0x7fffffff);
  const int wave_g = fhw::wave_min_i32(in_d && mine.b == wave_b ? mine.gain : 0x7fffffff);
  const int wave_reached = fhw::wave_sum_i32(n_reached), wave_reachable = fhw::wave_sum_i32(n_reachable), wave_poor = fhw::wave_sum_i32(n_poor);
  const int wave_top = -fhw::wave_min_i32(-top_gain);
  if (lane == 0) {
    s_bu[w] = wave_nu; s_bh[w] = wave_h; s_bd2[w] = wave_d2; s_bc[w] = wave_b; s_bg[w] = wave_g;
    s_n[w] = wave_reached; s_m[w] = wave_reachable; s_p[w] = wave_poor; s_g[w] = wave_top;
  }
  __syncthreads();
  ProspectBest best = {0, 0, -1, 0, INFINITY};
  for (int k = 0; k < 4; k++)
    if (s_bc[k] != 0x7fffffff && prospect_before(-s_bu[k], s_bh[k], s_bd2[k], s_bc[k], best)) {
      best.utility = -s_bu[k]; best.hops = s_bh[k]; best.d2 = s_bd2[k]; best.b = s_bc[k]; best.gain = s_bg[k];
    }
  // ---- the voxels of the chosen block: the smallest (d2, c) of its target voxels, and their number (K21's scan, once) ----
  const bool found = best.b >= 0;  // (uniform over the workgroup)
  FarVoxel voxel = {INFINITY, -1, 0};
  if (found) voxel = far_scan_block(a, F, best.b, px, py, pz, t);
  if (t == 0) {
    FarCounts n;
    n.block = found ? best.b : -1;
    n.hops = found ? best.hops : -1;
    n.targets = targets;
    n.reachable = s_m[0] + s_m[1] + s_m[2] + s_m[3];
    n.reached = s_n[0] + s_n[1] + s_n[2] + s_n[3];
    n.levels = level;
    n.members = voxel.members;
    const int poor = s_p[0] + s_p[1] + s_p[2] + s_p[3];
    const int top = max(max(s_g[0], s_g[1]), max(s_g[2], s_g[3]));
    if (cut) flags |= FH_REACH_CUT;
    if (n.reachable > 0 && poor == n.reachable) flags |= FH_PROSPECT_ALL_POOR;
    const ProspectGain e = {found ? best.gain : -1, found ? best.utility : 0, poor, top};
    if constexpr (CLAIMS)
      x.store(i, flags, view, voxel.cell, voxel.d2, found ? best.d2 : INFINITY, n, e, n_claims, n_standing, x.sum[0] + x.sum[1] + x.sum[2] + x.sum[3],
              covered, x.sum[8] + x.sum[9] + x.sum[10] + x.sum[11]);
    else
      prospect_store(p, i, flags, view, voxel.cell, voxel.d2, found ? best.d2 : INFINITY, n, e);
  }
}

__global__ void __launch_bounds__(256) prospect_goals_kernel(ProspectArgs p) { prospect_body<false>(p, ProspectNoClaims()); }

}  // namespace fhp

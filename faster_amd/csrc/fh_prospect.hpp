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
//                            then LDS), then the voxel scan of the chosen block, once.
// LDS of prospect_goals_kernel: 6 bitmaps of FAR_WORDS words = 24 KB static, and the slots of the reductions.
// Every address comes from a checked number: what K21's header lists, and the cube of a gain is clipped to [0, C_a) per axis before an
// entry of the counts is loaded.  Integer work and minima of total orders; nothing depends on scheduling.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fasterhip_prospect.h"
// (FarArgs, FarWho, far_judge, far_passable, far_target, far_block_d2, reach_before and fhw:: come from K21's device header, which
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

// the three outputs of vehicle i, by one thread
__device__ __forceinline__ void prospect_store(const ProspectArgs& p, int i, int flags, int view, int cell, double d2, double block_d2,
                                               const FarCounts& n, int gain, int utility, int poor, int best_gain) {
#pragma clang fp contract(off)
  const ReachArgs& r = p.f.r;
  const unsigned long long* g = (const unsigned long long*)r.vehicles[i].g_term;
  unsigned long long* out = (unsigned long long*)(r.goals + 3 * (size_t)i);
  if (cell >= 0) {
    const int ix = cell % r.nx, iy = (cell / r.nx) % r.ny, iz = cell / (r.nx * r.ny);
    r.goals[3 * (size_t)i] = (ix + 0.5) * r.res + r.ox;
    r.goals[3 * (size_t)i + 1] = (iy + 0.5) * r.res + r.oy;
    r.goals[3 * (size_t)i + 2] = (iz + 0.5) * r.res + r.oz;
    flags |= FH_FRONTIER_FOUND;
  } else {
    out[0] = g[0]; out[1] = g[1]; out[2] = g[2];  // the bits of g_term, whatever they are
  }
  r.mask[i] = cell >= 0 ? 1 : 0;
  fh_prospect_record q;
  q.flags = flags; q.view = view; q.cell = cell; q.block_cell = n.block; q.hops = n.hops;
  q.targets = n.targets; q.reachable = n.reachable; q.reached = n.reached; q.levels = n.levels; q.members = n.members;
  q.reserved[0] = 0; q.reserved[1] = 0;
  q.d2 = d2; q.block_d2 = block_d2;
  q.gain = gain; q.utility = utility; q.poor = poor; q.best_gain = best_gain;
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

// Weighs the target blocks `h` (bits of word u) of level `hops`: the gain of each from the counts U of the view, poor or not, the
// running best; -> in poor and best_gain this thread's sums.
__device__ __forceinline__ void prospect_weigh(const ProspectArgs& p, const uint16_t* U, unsigned long long h, int u, int hops, double px, double py,
                                               double pz, ProspectBest& best, int& poor, int& best_gain) {
#pragma clang fp contract(off)
  const FarArgs& a = p.f;
  if (h == 0ull) return;
  const int k = u % a.wx, row = u / a.wx, by = row % a.cy, bz = row / a.cy;
  const int g = p.g;
  const int ylo = max(by - g + 1, 0), yhi = min(by + g - 1, a.cy - 1), zlo = max(bz - g + 1, 0), zhi = min(bz + g - 1, a.cz - 1);
  while (h) {
    const int bx = 64 * k + (int)__builtin_ctzll(h);  // (a set bit of T: bx < cx)
    h &= h - 1ull;
    const int xlo = max(bx - g + 1, 0), xhi = min(bx + g - 1, a.cx - 1);
    int gain = 0;
    for (int z = zlo; z <= zhi; z++)      // (g == 0: lo > hi on every axis, nothing is loaded)
      for (int y = ylo; y <= yhi; y++) {
        const uint16_t* line = U + (size_t)(z * a.cy + y) * (size_t)(64 * a.wx);
        for (int x = xlo; x <= xhi; x++) gain += (int)line[x];
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

__global__ void __launch_bounds__(256) prospect_goals_kernel(ProspectArgs p) {
#pragma clang fp contract(off)
  __shared__ unsigned long long s_t[FAR_WORDS], s_lx[FAR_WORDS], s_ly[FAR_WORDS], s_lz[FAR_WORDS], s_a[FAR_WORDS], s_b[FAR_WORDS];
  __shared__ double s_bd2[4], s_vd2[4];
  __shared__ int s_bu[4], s_bh[4], s_bc[4], s_bg[4], s_vc[4], s_vm[4], s_n[4], s_m[4], s_k[4], s_p[4], s_g[4];
  __shared__ unsigned s_or[2][4];
  const FarArgs& a = p.f;
  const ReachArgs& r = a.r;
  const int i = (int)blockIdx.x, t = (int)threadIdx.x, lane = t & 63, w = t >> 6;
  const fh_vehicle& V = r.vehicles[i];
  const int view = fhw::uniform_i32(r.view_of ? r.view_of[i] : i);
  const int status = fhw::uniform_i32(V.status), stage = fhw::uniform_i32(V.stage);
  const int skip = fhw::uniform_i32(a.skip ? a.skip[i] : 0);
  const double px = fhw::uniform_f64(V.state.pos[0]), py = fhw::uniform_f64(V.state.pos[1]), pz = fhw::uniform_f64(V.state.pos[2]);
  const double gx = fhw::uniform_f64(V.g_term[0]), gy = fhw::uniform_f64(V.g_term[1]), gz = fhw::uniform_f64(V.g_term[2]);
  const FarWho who = far_judge(a, view, status, stage, skip, px, py, pz, gx, gy, gz);
  int flags = who.flags;
  if (!who.searched) {  // (uniform over the workgroup)
    const FarCounts none = {-1, -1, 0, 0, 0, 0, 0};
    if (t == 0) prospect_store(p, i, flags, view, -1, INFINITY, INFINITY, none, -1, 0, 0, -1);
    return;
  }
  const int W = a.W, wx = a.wx, slab = a.wx * a.cy;
  const unsigned char* F = r.flags + (size_t)view * r.view_stride;
  const unsigned long long* S = a.sums + (size_t)view * 4u * (size_t)W;
  const uint16_t* U = p.counts + (size_t)view * (size_t)W * 64u;
  const int sbx = who.sx / a.B, sby = who.sy / a.B, sbz = who.sz / a.B;  // (< cx, cy, cz: s is inside the lattice)
  const int sw = (sbz * a.cy + sby) * wx + (sbx >> 6);                   // (< W)
  const unsigned long long sbit = 1ull << (sbx & 63);

  // ---- the view's summary into LDS, T without the blocks within r_avoid of g_term (K21's) ----
  unsigned long long own_seen[FAR_OWN];
  unsigned own_nb[FAR_OWN];  // bit 0: owned (u < W); 1, 2: a word before / after in the same row; 4, 8: a row before / after in the slab; 16, 32: a slab below / above
  int n_targets = 0;
#pragma unroll
  for (int j = 0; j < FAR_OWN; j++) {
    const int u = t + 256 * j;
    const bool own = u < W;
    const int k = own ? u % wx : 0, row = own ? u / wx : 0, by = row % a.cy, bz = row / a.cy;
    own_nb[j] = own ? (1u | (k > 0 ? 2u : 0u) | (k < wx - 1 ? 4u : 0u) | (by > 0 ? 8u : 0u) | (by < a.cy - 1 ? 16u : 0u) | (bz > 0 ? 32u : 0u) |
                       (bz < a.cz - 1 ? 64u : 0u))
                    : 0u;
    own_seen[j] = own && u == sw ? sbit : 0ull;
    if (own) {
      unsigned long long tw = S[u];
      if (r.a2 > 0.0) {  // (with a2 == 0 no E2 is below it)
        unsigned long long h = tw;
        while (h) {
          const int bit = (int)__builtin_ctzll(h);
          h &= h - 1ull;
          const double e2 = far_block_d2(a, 64 * k + bit, by, bz, gx, gy, gz);
          if (e2 < r.a2) tw &= ~(1ull << bit);
        }
      }
      n_targets += __popcll(tw);
      s_t[u] = tw;
      s_lx[u] = S[(size_t)W + u];
      s_ly[u] = S[2 * (size_t)W + u];
      s_lz[u] = S[3 * (size_t)W + u];
      s_a[u] = u == sw ? sbit : 0ull;
      s_b[u] = 0ull;
    }
  }
  const int wave_targets = fhw::wave_sum_i32(n_targets);
  if (lane == 0) s_k[w] = wave_targets;
  __syncthreads();

  // ---- flood: every target block of every level is weighed by the thread that owns its word ----
  const int targets = s_k[0] + s_k[1] + s_k[2] + s_k[3];
  unsigned long long* cur = s_a;
  unsigned long long* nxt = s_b;
  int n_reached = t == 0 ? 1 : 0, n_reachable = 0;  // sums over this thread's words (the start: thread 0's)
  int n_poor = 0, top_gain = -1;
  ProspectBest mine = {0, 0, -1, 0, INFINITY};
  int level = 0;
  bool cut = false;
  if ((s_t[sw] & sbit) != 0ull && t == 0) n_reachable = 1;  // (uniform read) the start's block is a target block of level 0
  if (t == (sw & 255)) prospect_weigh(p, U, s_t[sw] & sbit, sw, 0, px, py, pz, mine, n_poor, top_gain);  // (the owner of word sw)
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
      const unsigned nb = own_nb[j];
      const unsigned long long c = cur[u], lx = s_lx[u];
      unsigned long long v = (c & lx) << 1;                  // +x inside the word
      unsigned long long down = c >> 1;                      // -x: block b from block b + 1, the link at b
      if (nb & 2u) v |= (cur[u - 1] & s_lx[u - 1]) >> 63;
      if (nb & 4u) down |= cur[u + 1] << 63;
      v |= down & lx;
      if (nb & 8u) v |= cur[u - wx] & s_ly[u - wx];
      if (nb & 16u) v |= cur[u + wx] & s_ly[u];
      if (nb & 32u) v |= cur[u - slab] & s_lz[u - slab];
      if (nb & 64u) v |= cur[u + slab] & s_lz[u];
      v &= ~own_seen[j];
      nxt[u] = v;
      own_seen[j] |= v;
      const unsigned long long h = v & s_t[u];
      n_reached += __popcll(v);
      n_reachable += __popcll(h);
      any |= v ? 1u : 0u;
      prospect_weigh(p, U, h, u, level + 1, px, py, pz, mine, n_poor, top_gain);
    }
    const unsigned wave_any = fhw::wave_or(any);
    if (lane == 0) s_or[level & 1][w] = wave_any;
    __syncthreads();
    const unsigned all = s_or[level & 1][0] | s_or[level & 1][1] | s_or[level & 1][2] | s_or[level & 1][3];
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
  double v_best = INFINITY;
  int best_cell = -1, members = 0;
  if (best.b >= 0) {  // (uniform over the workgroup)
    const int bx = best.b % a.cx, by = (best.b / a.cx) % a.cy, bz = best.b / (a.cx * a.cy);  // (a set bit of T: a block of the lattice)
    const int x0 = bx * a.B, y0 = by * a.B, z0 = bz * a.B;
    const int bw = min(x0 + a.B, r.nx) - x0, bh = min(y0 + a.B, r.ny) - y0, vol = bw * bh * (min(z0 + a.B, r.nz) - z0);
    double v_d2 = INFINITY;
    int v_c = 0x7fffffff, v_n = 0;
    for (int l = t; l < vol; l += 256) {
      const int ix = x0 + l % bw, iy = y0 + (l / bw) % bh, iz = z0 + l / (bw * bh);
      if (far_passable(r, F, ix, iy, iz) && far_target(r, F, ix, iy, iz)) {
        const double qx = (ix + 0.5) * r.res + r.ox, qy = (iy + 0.5) * r.res + r.oy, qz = (iz + 0.5) * r.res + r.oz;
        const double dx = qx - px, dy = qy - py, dz = qz - pz;
        const double d2 = dx * dx + dy * dy + dz * dz;
        const int c = (iz * r.ny + iy) * r.nx + ix;
        v_n++;
        if (reach_before(d2, c, v_d2, v_c)) { v_d2 = d2; v_c = c; }
      }
    }
    const double wave_v = fhw::wave_min(v_d2);
    const int wave_vc = fhw::wave_min_i32(v_d2 == wave_v ? v_c : 0x7fffffff);
    const int wave_vn = fhw::wave_sum_i32(v_n);
    if (lane == 0) { s_vd2[w] = wave_v; s_vc[w] = wave_vc; s_vm[w] = wave_vn; }
    __syncthreads();
    v_best = s_vd2[0];
    best_cell = s_vc[0];
    for (int k = 1; k < 4; k++)
      if (reach_before(s_vd2[k], s_vc[k], v_best, best_cell)) { v_best = s_vd2[k]; best_cell = s_vc[k]; }
    members = s_vm[0] + s_vm[1] + s_vm[2] + s_vm[3];
  }
  if (t == 0) {
    const bool found = best.b >= 0;
    FarCounts n;
    n.block = found ? best.b : -1;
    n.hops = found ? best.hops : -1;
    n.targets = targets;
    n.reachable = s_m[0] + s_m[1] + s_m[2] + s_m[3];
    n.reached = s_n[0] + s_n[1] + s_n[2] + s_n[3];
    n.levels = level;
    n.members = found ? members : 0;
    const int poor = s_p[0] + s_p[1] + s_p[2] + s_p[3];
    const int top = max(max(s_g[0], s_g[1]), max(s_g[2], s_g[3]));
    if (cut) flags |= FH_REACH_CUT;
    if (n.reachable > 0 && poor == n.reachable) flags |= FH_PROSPECT_ALL_POOR;
    prospect_store(p, i, flags, view, found ? best_cell : -1, found ? v_best : INFINITY, found ? best.d2 : INFINITY, n, found ? best.gain : -1,
                   found ? best.utility : 0, poor, top);
  }
}

}  // namespace fhp

// fh_stake.hpp — the kernels of include/fasterhip_stake.h (which is the specification): the far chooser by gain (K23) inside the passes of
// the far chooser for a team (K22), and a claim that stakes a region: it takes the target blocks within r_spread of it out of T (K22's
// rule) and the unknown voxels of a cube of blocks around its own block out of every gain of the vehicle.  Included by fh_reach.hip only,
// after K23's device header and before K22's (which stays the last include).  d_work: K23's workspace (K21's words and need bytes, then
// [n_views][64 W] counts of 16 bits), then K22's tail: a class byte per vehicle (rounded up to a multiple of 64), a group per vehicle and
// `lower` per vehicle.  The need bytes are written by far_need_kernel, the summaries and counts by prospect_blocks_kernel and the class
// bytes and groups by K22's class kernel, all as they are; the host code launches them.
//   stake_count_kernel : a wavefront per vehicle, K22's count logic.  A vehicle that is no searcher has its final outputs written by lane
//                        0.  A searcher scans all n class bytes and groups in chunks of 64 ascending, lane = k, and counts lower and
//                        standing by ballots and popcounts: no list, so nothing overflows.  lower goes to d_work; lower >= passes: lane
//                        0 writes the UNSETTLED outputs.
//   stake_goals_kernel : launched once per pass p, ONE workgroup of 256 per vehicle; it returns at once unless the vehicle is a searcher
//                        with lower == p - 1 (the searching members of a group are one chain by index, so its lower peers were decided by
//                        the launches before).  Judge, summary into LDS and r_avoid out of T are K21's, on K21's helpers.  Then the claim
//                        scan, this file's own: the n vehicles in chunks of 256, thread = k; the claim points of the chunk are compacted
//                        into LDS in ascending k by ballot and rank (256 x 3 doubles), and beside each point the block of its voxel (3
//                        x 16 bits, 0xffff: the voxel lies outside the lattice).  Every thread then works on the words u = t, t + 256, ..
//                        it OWNS: it sets in a SEVENTH bitmap C the blocks the chunk's claims cover — for a claim whose cube crosses the
//                        word's (by, bz) row the bits [cbx - k + 1, cbx + k - 1] of the row that fall into the word and below Cx — and
//                        takes the blocks with G2 < r_spread^2 out of T, with K22's shortcut on the y and z gaps.  A word of either
//                        bitmap has one writer, so the bytes do not depend on scheduling.  After the scan each thread sums popcount(C[u])
//                        and the U of the set bits of its words: covered and removed.  Then K23's flood and weighing with one change: a
//                        row of the cube is at most 9 consecutive counts, the 9-bit piece of C that belongs to it is taken from one or two
//                        words, and covered counts are skipped.  A workgroup that covered nothing (a uniform flag) takes K23's own
//                        prospect_weigh, unchanged.  The reduction is K23's, the voxel scan K21's.
// No read-modify-write on global memory, no spin.  LDS of stake_goals_kernel: 7 bitmaps of FAR_WORDS words = 28 KB, 256 x 3 doubles and
// 256 x 3 x 16 bits of claims = 7.5 KB, and the slots of the reductions: below 40960 bytes, four workgroups a CU.
// Every address comes from a checked number: what K21's, K22's and K23's device headers list; k < n before a class byte is read; a
// class other than none says that the view is in [0, n_views); d_goals of a lower peer is read only under its mask, which an earlier
// launch wrote; a claim's voxel is tested against the dims as a double before it is a block; the bits of C are clipped to the word and to
// [0, Cx), and the cube of a gain to [0, C_a) per axis, before an entry of C or of the counts is loaded.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fasterhip_stake.h"
// (FarArgs, FarWho, FarCounts, far_judge, far_passable, far_target, far_gap2, far_block_d2, reach_before and fhw:: come from K21's device
// header, ProspectArgs, ProspectBest, prospect_before and prospect_weigh from K23's; fh_reach.hip includes both before this)

namespace fhp {

constexpr int STAKE_NONE = 0, STAKE_SEARCHER = 1, STAKE_STANDING = 2;  // K22's class bytes (the host file asserts the equalities)
constexpr int STAKE_CHUNK = 256;                                        // claims held in LDS at a time: one per thread

struct StakeArgs {
  ProspectArgs p;  // (p.records and p.f.records are not used)
  double s2;       // r_spread^2, rounded once on the host
  int pass, passes;
  int k;                     // claim_blocks
  const unsigned char* cls;  // [n]
  const int32_t* grp;        // [n]
  int32_t* lower;            // [n]
  fh_stake_record* records;
};

struct StakeTeam {
  int group, decided_pass, lower, standing, claims, claimed;
};

struct StakeGain {
  int gain, utility, poor, best_gain, covered, removed;
};

// the three outputs of vehicle i, by one thread
__device__ __forceinline__ void stake_store(const StakeArgs& s, int i, int flags, int view, int cell, double d2, double block_d2, const FarCounts& n,
                                            const StakeTeam& m, const StakeGain& e) {
#pragma clang fp contract(off)
  const ReachArgs& r = s.p.f.r;
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
    if (m.claimed > 0) flags |= FH_STAKE_CLAIMED;
  }
  r.mask[i] = cell >= 0 ? 1 : 0;
  fh_stake_record q;
  q.flags = flags; q.view = view; q.cell = cell; q.block_cell = n.block; q.hops = n.hops;
  q.targets = n.targets; q.reachable = n.reachable; q.reached = n.reached; q.levels = n.levels; q.members = n.members;
  q.reserved[0] = 0; q.reserved[1] = 0;
  q.d2 = d2; q.block_d2 = block_d2;
  q.group = m.group; q.decided_pass = m.decided_pass; q.lower = m.lower; q.standing = m.standing; q.claims = m.claims; q.claimed = m.claimed;
  q.reserved_tail[0] = 0; q.reserved_tail[1] = 0;
  q.gain = e.gain; q.utility = e.utility; q.poor = e.poor; q.best_gain = e.best_gain; q.covered = e.covered; q.removed = e.removed;
  q.reserved_end[0] = 0; q.reserved_end[1] = 0;
  s.records[i] = q;
}

__global__ void __launch_bounds__(64) stake_count_kernel(StakeArgs s) {
#pragma clang fp contract(off)
  const FarArgs& a = s.p.f;
  const ReachArgs& r = a.r;
  const int i = (int)blockIdx.x, lane = (int)threadIdx.x, n = a.n;
  const fh_vehicle& V = r.vehicles[i];
  const int view = fhw::uniform_i32(r.view_of ? r.view_of[i] : i);
  const int mine = fhw::uniform_i32((int)s.cls[i]), group = fhw::uniform_i32(s.grp[i]);
  const FarCounts none = {-1, -1, 0, 0, 0, 0, 0};
  const StakeGain no_gain = {-1, 0, 0, -1, 0, 0};
  if (mine != STAKE_SEARCHER) {  // (uniform)
    if (lane == 0) {
      const FarWho w = far_judge(a, view, V.status, V.stage, a.skip ? a.skip[i] : 0, V.state.pos[0], V.state.pos[1], V.state.pos[2], V.g_term[0],
                                 V.g_term[1], V.g_term[2]);
      const StakeTeam m = {group, 0, 0, 0, 0, 0};
      stake_store(s, i, w.flags, view, -1, INFINITY, INFINITY, none, m, no_gain);
      s.lower[i] = 0;
    }
    return;
  }
  int lower = 0, standing = 0;  // (uniform: sums of popcounts of ballots)
  for (int base = 0; base < n; base += 64) {
    const int k = base + lane;
    const bool in = k < n && k != i;
    const int ck = in ? (int)s.cls[k] : STAKE_NONE;
    const bool peer = ck != STAKE_NONE && s.grp[k] == group;  // (a class other than none: a view in range)
    lower += __popcll(__ballot(peer && ck == STAKE_SEARCHER && k < i));
    standing += __popcll(__ballot(peer && ck == STAKE_STANDING));
  }
  if (lane == 0) {
    s.lower[i] = lower;
    if (lower >= s.passes) {  // (a searcher: its flags are WANTED alone)
      const StakeTeam m = {group, -1, lower, standing, standing, 0};
      stake_store(s, i, FH_FRONTIER_WANTED | FH_STAKE_UNSETTLED, view, -1, INFINITY, INFINITY, none, m, no_gain);
    }
  }
}

// prospect_weigh with the covered set: weighs the target blocks `h` (bits of word u) of level `hops`, the gain of each from the counts U
// of the view without the blocks whose bit of C (LDS, [W]) is set; -> in poor and best_gain this thread's sums.
__device__ __forceinline__ void stake_weigh(const ProspectArgs& p, const uint16_t* U, const unsigned long long* C, unsigned long long h, int u, int hops,
                                            double px, double py, double pz, ProspectBest& best, int& poor, int& best_gain) {
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

__global__ void __launch_bounds__(256) stake_goals_kernel(StakeArgs s) {
#pragma clang fp contract(off)
  __shared__ unsigned long long s_t[FAR_WORDS], s_lx[FAR_WORDS], s_ly[FAR_WORDS], s_lz[FAR_WORDS], s_a[FAR_WORDS], s_b[FAR_WORDS], s_c[FAR_WORDS];
  __shared__ double s_pts[3 * STAKE_CHUNK];
  __shared__ unsigned short s_cb[3 * STAKE_CHUNK];
  __shared__ double s_bd2[4], s_vd2[4];
  __shared__ int s_bu[4], s_bh[4], s_bc[4], s_bg[4], s_vc[4], s_vm[4], s_n[4], s_m[4], s_k[4], s_p[4], s_g[4];
  __shared__ int s_cnt[8], s_cl[4], s_cv[4], s_rm[4];
  __shared__ unsigned s_or[2][4];
  const ProspectArgs& p = s.p;
  const FarArgs& a = p.f;
  const ReachArgs& r = a.r;
  const int i = (int)blockIdx.x, t = (int)threadIdx.x, lane = t & 63, w = t >> 6, n = a.n;
  if (fhw::uniform_i32((int)s.cls[i]) != STAKE_SEARCHER) return;  // (uniform over the workgroup)
  const int lower = fhw::uniform_i32(s.lower[i]);
  if (lower != s.pass - 1) return;
  const int group = fhw::uniform_i32(s.grp[i]);
  const fh_vehicle& V = r.vehicles[i];
  const int view = fhw::uniform_i32(r.view_of ? r.view_of[i] : i);
  const int status = fhw::uniform_i32(V.status), stage = fhw::uniform_i32(V.stage);
  const int skip = fhw::uniform_i32(a.skip ? a.skip[i] : 0);
  const double px = fhw::uniform_f64(V.state.pos[0]), py = fhw::uniform_f64(V.state.pos[1]), pz = fhw::uniform_f64(V.state.pos[2]);
  const double gx = fhw::uniform_f64(V.g_term[0]), gy = fhw::uniform_f64(V.g_term[1]), gz = fhw::uniform_f64(V.g_term[2]);
  const FarWho who = far_judge(a, view, status, stage, skip, px, py, pz, gx, gy, gz);
  int flags = who.flags;
  if (!who.searched) return;  // (uniform; a searcher is searched: the class kernel judged the same values)
  const int W = a.W, wx = a.wx, slab = a.wx * a.cy;
  const unsigned char* F = r.flags + (size_t)view * r.view_stride;
  const unsigned long long* S = a.sums + (size_t)view * 4u * (size_t)W;
  const uint16_t* U = p.counts + (size_t)view * (size_t)W * 64u;
  const int sbx = who.sx / a.B, sby = who.sy / a.B, sbz = who.sz / a.B;  // (< cx, cy, cz: s is inside the lattice)
  const int sw = (sbz * a.cy + sby) * wx + (sbx >> 6);                   // (< W)
  const unsigned long long sbit = 1ull << (sbx & 63);

  // ---- the view's summary into LDS, T without the blocks within r_avoid of g_term (K21's); C starts empty ----
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
      s_c[u] = 0ull;
    }
  }

  // ---- the claims: every thread takes the claimed blocks out of the words of T it owns (and alone has written) and sets the covered
  // ---- blocks in the words of C it owns; the barriers inside are uniform.  Who claims, the compaction by ballot and rank, the two
  // ---- halves of s_cnt and the clearing of T with the shortcut on the y and z gaps are K22's claim scan (FarClaims::clear in K22's
  // ---- device header, which is included after this file and cannot be called from here), restated: a fix to either belongs in both ----
  int n_claimed = 0, n_claims = 0, n_standing = 0;  // (the last two are uniform)
  {
    int parity = 0;
    for (int base = 0; base < n; base += STAKE_CHUNK, parity ^= 1) {
      const int k = base + t;
      const bool in = k < n && k != i;
      const int ck = in ? (int)s.cls[k] : STAKE_NONE;
      const bool low = ck == STAKE_SEARCHER && k < i;
      bool has = (low || ck == STAKE_STANDING) && s.grp[k] == group;
      if (has && low) has = r.mask[k] == 1;  // (a lower peer of this chain: a launch before this one wrote its mask and goal)
      const unsigned long long bh = __ballot(has);
      const unsigned long long bs = __ballot(has && !low);
      if (lane == 0) s_cnt[4 * parity + w] = __popcll(bh) | (__popcll(bs) << 16);  // (each <= 64)
      __syncthreads();
      const int c0 = s_cnt[4 * parity], c1 = s_cnt[4 * parity + 1], c2 = s_cnt[4 * parity + 2], c3 = s_cnt[4 * parity + 3];
      const int both = c0 + c1 + c2 + c3, m = both & 0xffff;  // (<= 256 each: no carry between the halves)
      if (m == 0) continue;  // (uniform over the workgroup; the next chunk writes the other half of s_cnt)
      if (has) {
        const double* c = low ? r.goals + 3 * (size_t)k : r.vehicles[k].g_term;
        const int j = (((w > 0 ? c0 : 0) + (w > 1 ? c1 : 0) + (w > 2 ? c2 : 0)) & 0xffff) + fhw::rank_in(bh);  // (< 256)
        const double c_x = c[0], c_y = c[1], c_z = c[2];
        s_pts[3 * j] = c_x; s_pts[3 * j + 1] = c_y; s_pts[3 * j + 2] = c_z;
        // the voxel of the claim, tested as a double before it is an index (the expression of the start cell)
        const double vfx = floor((c_x - r.ox) / r.res), vfy = floor((c_y - r.oy) / r.res), vfz = floor((c_z - r.oz) / r.res);
        const bool inside = vfx >= 0.0 && vfx < (double)r.nx && vfy >= 0.0 && vfy < (double)r.ny && vfz >= 0.0 && vfz < (double)r.nz;
        s_cb[3 * j] = inside ? (unsigned short)((int)vfx / a.B) : (unsigned short)0xffffu;  // (a block per axis: < 64 * 512)
        s_cb[3 * j + 1] = inside ? (unsigned short)((int)vfy / a.B) : (unsigned short)0xffffu;
        s_cb[3 * j + 2] = inside ? (unsigned short)((int)vfz / a.B) : (unsigned short)0xffffu;
      }
      __syncthreads();
      n_claims += m;
      n_standing += both >> 16;
      for (int u = t; u < W; u += 256) {
        const int kx = u % wx, row = u / wx, by = row % a.cy, bz = row / a.cy;
        if (s.k > 0) {  // the covered blocks of this word
          const int first = 64 * kx, last = min(first + 63, a.cx - 1);
          unsigned long long cw = 0ull;
          for (int j = 0; j < m; j++) {
            const int cbx = (int)s_cb[3 * j], cby = (int)s_cb[3 * j + 1], cbz = (int)s_cb[3 * j + 2];
            if (cbx == 0xffff) continue;
            if (abs(by - cby) >= s.k || abs(bz - cbz) >= s.k) continue;
            const int lo = max(cbx - s.k + 1, first), hi = min(cbx + s.k - 1, last);
            if (lo <= hi) cw |= ((1ull << (hi - lo + 1)) - 1ull) << (lo - first);  // (hi - lo <= 8, lo - first <= 63 - (hi - lo))
          }
          if (cw) s_c[u] |= cw;
        }
        unsigned long long tw = s_t[u];
        if (tw == 0ull) continue;
        const unsigned long long before = tw;
        const int y0 = by * a.B, y1 = min(y0 + a.B, r.ny) - 1, z0 = bz * a.B, z1 = min(z0 + a.B, r.nz) - 1;
        for (int j = 0; j < m && tw != 0ull; j++) {
          const double cx = s_pts[3 * j], cy = s_pts[3 * j + 1], cz = s_pts[3 * j + 2];
          const double gy2 = far_gap2(cy, y0, y1, r.res, r.oy), gz2 = far_gap2(cz, z0, z1, r.res, r.oz);
          if (!(gy2 + gz2 < s.s2)) continue;  // (x2 + y2) + z2 >= y2 + z2 in rounded sums of non-negative terms: no block of this word
          unsigned long long h = tw;
          while (h) {
            const int bit = (int)__builtin_ctzll(h);
            h &= h - 1ull;
            const int x0 = (64 * kx + bit) * a.B;
            const double gx2 = far_gap2(cx, x0, min(x0 + a.B, r.nx) - 1, r.res, r.ox);
            if ((gx2 + gy2) + gz2 < s.s2) tw &= ~(1ull << bit);
          }
        }
        if (tw != before) {
          s_t[u] = tw;
          n_claimed += __popcll(before ^ tw);
        }
      }
      // (the next chunk's first barrier stands between these reads of s_pts / s_cb and the next writes)
    }
  }
  // covered and removed: the set bits of the words of C this thread owns, and their counts
  int n_covered = 0, n_removed = 0;
  if (s.k > 0)
    for (int u = t; u < W; u += 256) {
      unsigned long long cw = s_c[u];
      n_covered += __popcll(cw);
      while (cw) {
        n_removed += (int)U[(size_t)u * 64u + (size_t)__builtin_ctzll(cw)];  // (<= 64 * 512 blocks of <= 4096 voxels: < 2^31)
        cw &= cw - 1ull;
      }
    }
  const int wave_claimed = fhw::wave_sum_i32(n_claimed), wave_covered = fhw::wave_sum_i32(n_covered), wave_removed = fhw::wave_sum_i32(n_removed);
  const int wave_targets = fhw::wave_sum_i32(n_targets);
  if (lane == 0) { s_cl[w] = wave_claimed; s_cv[w] = wave_covered; s_rm[w] = wave_removed; s_k[w] = wave_targets; }
  __syncthreads();

  // ---- flood: every target block of every level is weighed by the thread that owns its word (K23's) ----
  const int targets = s_k[0] + s_k[1] + s_k[2] + s_k[3];
  const int covered = s_cv[0] + s_cv[1] + s_cv[2] + s_cv[3];
  const bool plain = covered == 0;  // (uniform) nothing is covered: K23's own weighing
  unsigned long long* cur = s_a;
  unsigned long long* nxt = s_b;
  int n_reached = t == 0 ? 1 : 0, n_reachable = 0;  // sums over this thread's words (the start: thread 0's)
  int n_poor = 0, top_gain = -1;
  ProspectBest mine = {0, 0, -1, 0, INFINITY};
  int level = 0;
  bool cut = false;
  if ((s_t[sw] & sbit) != 0ull && t == 0) n_reachable = 1;  // (uniform read) the start's block is a target block of level 0
  if (t == (sw & 255)) {                                    // (the owner of word sw)
    if (plain) prospect_weigh(p, U, s_t[sw] & sbit, sw, 0, px, py, pz, mine, n_poor, top_gain);
    else stake_weigh(p, U, s_c, s_t[sw] & sbit, sw, 0, px, py, pz, mine, n_poor, top_gain);
  }
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
      if (plain) prospect_weigh(p, U, h, u, level + 1, px, py, pz, mine, n_poor, top_gain);
      else stake_weigh(p, U, s_c, h, u, level + 1, px, py, pz, mine, n_poor, top_gain);
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

  // ---- the smallest (-utility, hops, D2, b) of the workgroup: the wavefront's, then the four through LDS (K23's) ----
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
    FarCounts c;
    c.block = found ? best.b : -1;
    c.hops = found ? best.hops : -1;
    c.targets = targets;
    c.reachable = s_m[0] + s_m[1] + s_m[2] + s_m[3];
    c.reached = s_n[0] + s_n[1] + s_n[2] + s_n[3];
    c.levels = level;
    c.members = found ? members : 0;
    const int poor = s_p[0] + s_p[1] + s_p[2] + s_p[3];
    const int top = max(max(s_g[0], s_g[1]), max(s_g[2], s_g[3]));
    if (cut) flags |= FH_REACH_CUT;
    if (c.reachable > 0 && poor == c.reachable) flags |= FH_STAKE_ALL_POOR;
    const StakeTeam m = {group, s.pass, lower, n_standing, n_claims, s_cl[0] + s_cl[1] + s_cl[2] + s_cl[3]};
    const StakeGain e = {found ? best.gain : -1, found ? best.utility : 0, poor, top, covered, s_rm[0] + s_rm[1] + s_rm[2] + s_rm[3]};
    stake_store(s, i, flags, view, found ? best_cell : -1, found ? v_best : INFINITY, found ? best.d2 : INFINITY, c, m, e);
  }
}

}  // namespace fhp

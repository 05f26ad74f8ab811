// fh_apart.hpp — the kernels of include/fasterhip_apart.h (which is the specification): the far chooser (K21) for
// a team, in which a target block nearer than r_spread to a goal that a peer holds or was given by an earlier pass is no target.
// Included by fh_reach.hip only, last, after K21's device header (which stays the last *.hip.hpp).  d_work: K21's workspace, then a
// class byte per vehicle (rounded up to a multiple of 64), a group per vehicle and `lower` per vehicle.  The summaries are written by
// far_need_kernel and far_blocks_kernel as they are.
//   far_spread_class_kernel : a thread per vehicle.  far_judge and the standing predicate; the class byte, and the group (0 without a
//                             view in range).
//   far_spread_count_kernel : a wavefront per vehicle.  A vehicle that is no searcher has its final outputs written by lane 0.  A
//                             searcher scans all n class bytes and groups in chunks of 64 ascending, lane = k, both coalesced, and
//                             counts lower and standing by ballots and popcounts: no list, so nothing overflows.  lower goes to d_work;
//                             lower >= passes: lane 0 writes the UNSETTLED outputs.  Brute force on purpose, as spread_peers_kernel is.
//   far_spread_goals_kernel : launched once per pass p, a workgroup of 256 per vehicle; it returns at once unless the vehicle is a
//                             searcher with lower == p - 1 (the searching members of a group are one chain by index, so its lower
//                             peers were decided by the launches before).  Then far_body<true>: FarClaims::clear scans the n vehicles
//                             in chunks of 256, thread = k, compacts the claim points of the chunk into LDS in ascending k by ballot
//                             and rank (at most 256 x 3 doubles), and every thread clears from the words of T it OWNS the blocks
//                             those points cover — a word has one writer, so the bytes do not depend on scheduling.  A word whose y
//                             and z gaps alone reach r_spread^2 costs two gaps per claim, not 64: the sum of three non-negative
//                             squares, rounded, is never below the rounded sum of two of them.  Only the set bits of a word are tested.
// No atomics, no spin.  LDS of the pass kernel: far_body's 24768 bytes + 256 x 3 doubles + 12 ints.
// Every address comes from a checked number: k < n before a class byte is read; a class other than none says that the view is in
// [0, n_views); d_goals of a lower peer is read only under its mask, which an earlier launch wrote.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fasterhip_apart.h"
// (FarArgs, far_judge, far_body, far_gap2 and fhw:: come from K21's device header, which fh_reach.hip includes before this)

namespace fhp {

constexpr int FAR_SPREAD_NONE = 0, FAR_SPREAD_SEARCHER = 1, FAR_SPREAD_STANDING = 2;

struct FarSpreadArgs {
  FarArgs f;  // (f.records is not used)
  double s2;  // r_spread^2, rounded once on the host
  int pass, passes;
  const int32_t* group;  // [n_views] or null
  unsigned char* cls;    // [n]
  int32_t* grp;          // [n]
  int32_t* lower;        // [n]
  fh_apart_record* records;
};

// the three outputs of vehicle i, by one thread: far_store with the longer record
__device__ __forceinline__ void far_spread_store(const FarSpreadArgs& s, int i, int flags, int view, int cell, double d2, double block_d2,
                                                 const FarCounts& n, int group, int decided_pass, int lower, int standing, int claims, int claimed) {
#pragma clang fp contract(off)
  const ReachArgs& r = s.f.r;
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
    if (claimed > 0) flags |= FH_APART_CLAIMED;
  }
  r.mask[i] = cell >= 0 ? 1 : 0;
  fh_apart_record q;
  q.flags = flags; q.view = view; q.cell = cell; q.block_cell = n.block; q.hops = n.hops;
  q.targets = n.targets; q.reachable = n.reachable; q.reached = n.reached; q.levels = n.levels; q.members = n.members;
  q.reserved[0] = 0; q.reserved[1] = 0;
  q.d2 = d2; q.block_d2 = block_d2;
  q.group = group; q.decided_pass = decided_pass; q.lower = lower; q.standing = standing; q.claims = claims; q.claimed = claimed;
  q.reserved_tail[0] = 0; q.reserved_tail[1] = 0;
  s.records[i] = q;
}

__global__ void __launch_bounds__(256) far_spread_class_kernel(FarSpreadArgs s) {
#pragma clang fp contract(off)
  const ReachArgs& r = s.f.r;
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= s.f.n) return;
  const fh_vehicle& V = r.vehicles[i];
  const int view = r.view_of ? r.view_of[i] : i;
  const int status = V.status, skip = s.f.skip ? s.f.skip[i] : 0;
  const double gx = V.g_term[0], gy = V.g_term[1], gz = V.g_term[2];
  const FarWho w = far_judge(s.f, view, status, V.stage, skip, V.state.pos[0], V.state.pos[1], V.state.pos[2], gx, gy, gz);
  const bool has_view = !(w.flags & FH_FRONTIER_NO_VIEW);
  int cls = FAR_SPREAD_NONE;
  if (w.searched) cls = FAR_SPREAD_SEARCHER;
  else if (has_view && status != FH_VEHICLE_GOAL_REACHED && reach_finite(gx) && reach_finite(gy) && reach_finite(gz) &&
           (!(w.flags & FH_FRONTIER_WANTED) || skip != 0))
    cls = FAR_SPREAD_STANDING;
  s.cls[i] = (unsigned char)cls;
  s.grp[i] = has_view ? (s.group ? s.group[view] : view) : 0;  // (has_view: view in [0, n_views))
}

__global__ void __launch_bounds__(64) far_spread_count_kernel(FarSpreadArgs s) {
#pragma clang fp contract(off)
  const ReachArgs& r = s.f.r;
  const int i = (int)blockIdx.x, lane = (int)threadIdx.x, n = s.f.n;
  const fh_vehicle& V = r.vehicles[i];
  const int view = fhw::uniform_i32(r.view_of ? r.view_of[i] : i);
  const int mine = fhw::uniform_i32((int)s.cls[i]), group = fhw::uniform_i32(s.grp[i]);
  const FarCounts none = {-1, -1, 0, 0, 0, 0, 0};
  if (mine != FAR_SPREAD_SEARCHER) {  // (uniform)
    if (lane == 0) {
      const FarWho w = far_judge(s.f, view, V.status, V.stage, s.f.skip ? s.f.skip[i] : 0, V.state.pos[0], V.state.pos[1], V.state.pos[2],
                                 V.g_term[0], V.g_term[1], V.g_term[2]);
      far_spread_store(s, i, w.flags, view, -1, INFINITY, INFINITY, none, group, 0, 0, 0, 0, 0);
      s.lower[i] = 0;
    }
    return;
  }
  int lower = 0, standing = 0;  // (uniform: sums of popcounts of ballots)
  for (int base = 0; base < n; base += 64) {
    const int k = base + lane;
    const bool in = k < n && k != i;
    const int ck = in ? (int)s.cls[k] : FAR_SPREAD_NONE;
    const bool peer = ck != FAR_SPREAD_NONE && s.grp[k] == group;  // (a class other than none: a view in range)
    lower += __popcll(__ballot(peer && ck == FAR_SPREAD_SEARCHER && k < i));
    standing += __popcll(__ballot(peer && ck == FAR_SPREAD_STANDING));
  }
  if (lane == 0) {
    s.lower[i] = lower;
    if (lower >= s.passes)  // (a searcher: its flags are WANTED alone)
      far_spread_store(s, i, FH_FRONTIER_WANTED | FH_APART_UNSETTLED, view, -1, INFINITY, INFINITY, none, group, -1, lower, standing, standing, 0);
  }
}

// what far_body<true> reads and calls
struct FarClaims {
  const FarSpreadArgs* s;
  double* pts;  // LDS [256][3]
  int* cnt;     // LDS [2][4]: the claims of a chunk per wavefront (the standing ones among them << 16), by the chunk's parity
  int* sum;     // LDS [4]
  int group, lower;

  // Takes the blocks that a claim covers out of the words u = t, t + 256, .. < W of T that thread t owns; -> how many bits this thread
  // cleared, and in n_claims and n_standing the number of claims and of the standing peers among them (uniform).  Called by all 256
  // threads.
  __device__ __forceinline__ int clear(const FarArgs& a, int i, int t, unsigned long long* s_t, int& n_claims, int& n_standing) const {
#pragma clang fp contract(off)
    const ReachArgs& r = a.r;
    const int lane = t & 63, w = t >> 6, n = a.n;
    int cleared = 0, total = 0, standing = 0, parity = 0;
    for (int base = 0; base < n; base += 256, parity ^= 1) {
      const int k = base + t;
      const bool in = k < n && k != i;
      const int ck = in ? (int)s->cls[k] : FAR_SPREAD_NONE;
      const bool low = ck == FAR_SPREAD_SEARCHER && k < i;
      bool has = (low || ck == FAR_SPREAD_STANDING) && s->grp[k] == group;
      if (has && low) has = r.mask[k] == 1;  // (a lower peer of this chain: a launch before this one wrote its mask and goal)
      const unsigned long long bh = __ballot(has);
      const unsigned long long bs = __ballot(has && !low);
      if (lane == 0) cnt[4 * parity + w] = __popcll(bh) | (__popcll(bs) << 16);  // (each <= 64)
      __syncthreads();
      const int c0 = cnt[4 * parity], c1 = cnt[4 * parity + 1], c2 = cnt[4 * parity + 2], c3 = cnt[4 * parity + 3];
      const int both = c0 + c1 + c2 + c3, m = both & 0xffff;  // (<= 256 each: no carry between the halves)
      if (m == 0) continue;  // (uniform over the workgroup; the next chunk writes the other half of cnt)
      if (has) {
        const double* c = low ? r.goals + 3 * (size_t)k : r.vehicles[k].g_term;
        const int j = (((w > 0 ? c0 : 0) + (w > 1 ? c1 : 0) + (w > 2 ? c2 : 0)) & 0xffff) + fhw::rank_in(bh);  // (< 256)
        pts[3 * j] = c[0]; pts[3 * j + 1] = c[1]; pts[3 * j + 2] = c[2];
      }
      __syncthreads();
      total += m;
      standing += both >> 16;
      for (int u = t; u < a.W; u += 256) {
        unsigned long long tw = s_t[u];
        if (tw == 0ull) continue;
        const unsigned long long before = tw;
        const int kx = u % a.wx, row = u / a.wx, by = row % a.cy, bz = row / a.cy;
        const int y0 = by * a.B, y1 = min(y0 + a.B, r.ny) - 1, z0 = bz * a.B, z1 = min(z0 + a.B, r.nz) - 1;
        for (int j = 0; j < m && tw != 0ull; j++) {
          const double cx = pts[3 * j], cy = pts[3 * j + 1], cz = pts[3 * j + 2];
          const double gy2 = far_gap2(cy, y0, y1, r.res, r.oy), gz2 = far_gap2(cz, z0, z1, r.res, r.oz);
          if (!(gy2 + gz2 < s->s2)) continue;  // (x2 + y2) + z2 >= y2 + z2 in rounded sums of non-negative terms: no block of this word
          unsigned long long h = tw;
          while (h) {
            const int bit = (int)__builtin_ctzll(h);
            h &= h - 1ull;
            const int x0 = (64 * kx + bit) * a.B;
            const double gx2 = far_gap2(cx, x0, min(x0 + a.B, r.nx) - 1, r.res, r.ox);
            if ((gx2 + gy2) + gz2 < s->s2) tw &= ~(1ull << bit);
          }
        }
        if (tw != before) {
          s_t[u] = tw;
          cleared += __popcll(before ^ tw);
        }
      }
      // (the next chunk's first barrier stands between these reads of pts and the next writes)
    }
    n_claims = total;
    n_standing = standing;
    return cleared;
  }

  __device__ __forceinline__ void store(const FarArgs&, int i, int flags, int view, int cell, double d2, double block_d2, const FarCounts& n,
                                        int claims, int standing, int claimed) const {
    far_spread_store(*s, i, flags, view, cell, d2, block_d2, n, group, s->pass, lower, standing, claims, claimed);
  }
};

__global__ void __launch_bounds__(256) far_spread_goals_kernel(FarSpreadArgs s) {
  __shared__ double s_pts[3 * 256];
  __shared__ int s_cnt[8], s_sum[4];
  const int i = (int)blockIdx.x;
  if (fhw::uniform_i32((int)s.cls[i]) != FAR_SPREAD_SEARCHER) return;  // (uniform over the workgroup)
  const int lower = fhw::uniform_i32(s.lower[i]);
  if (lower != s.pass - 1) return;
  FarClaims x;
  x.s = &s; x.pts = s_pts; x.cnt = s_cnt; x.sum = s_sum;
  x.group = fhw::uniform_i32(s.grp[i]); x.lower = lower;
  far_body<true>(s.f, x);
}

}  // namespace fhp

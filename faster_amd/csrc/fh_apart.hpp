// fh_apart.hpp — the kernels of include/fasterhip_apart.h (which is the specification): the far chooser (K21) for
// a team, in which a target block nearer than r_spread to a goal that a peer holds or was given by an earlier pass is no target.
// Included by fh_reach.hip only, last, after K21's device header (which stays the last *.hip.hpp).  d_work: K21's workspace, then a
// class byte per vehicle (rounded up to a multiple of 64), a group per vehicle and `lower` per vehicle.  The summaries are written by
// far_need_kernel and far_blocks_kernel as they are.
//   far_spread_class_kernel : a thread per vehicle.  far_judge and the standing predicate; the class byte, and the group (0 without a
//                             view in range).
//   far_spread_count_kernel : a wavefront per vehicle, K21's far_count_body.  A vehicle that is no searcher has its final outputs
//                             written by lane 0.  A searcher scans all n class bytes and groups in chunks of 64 ascending, lane = k,
//                             both coalesced, and counts lower and standing by ballots and popcounts: no list, so nothing overflows.
//                             lower goes to d_work; lower >= passes: lane 0 writes the UNSETTLED outputs.  Brute force on purpose, as
//                             spread_peers_kernel is.
//   far_spread_goals_kernel : launched once per pass p, a workgroup of 256 per vehicle; it returns at once unless the vehicle is a
//                             searcher with lower == p - 1 (the searching members of a group are one chain by index, so its lower
//                             peers were decided by the launches before).  Then far_body<true>: K21's far_claim_scan<false> scans the
//                             n vehicles in chunks of 256, thread = k, compacts the claim points of the chunk into LDS in ascending k
//                             by ballot and rank (at most 256 x 3 doubles), and every thread clears from the words of T it OWNS the
//                             blocks those points cover — a word has one writer, so the bytes do not depend on scheduling.  A word
//                             whose y and z gaps alone reach r_spread^2 costs two gaps per claim, not 64: the sum of three non-negative
//                             squares, rounded, is never below the rounded sum of two of them.  Only the set bits of a word are tested.
// No atomics, no spin.  LDS of the pass kernel: far_body's 24768 bytes + 256 x 3 doubles + 12 ints.
// Every address comes from a checked number: what K21's device header lists.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fasterhip_apart.h"
// (FarArgs, FarTeam, FarTeamCounts, the class bytes, far_judge, far_body, far_count_body, far_put_goal, far_head, far_team_words and fhw::
// come from K21's device header, which fh_reach.hip includes before this)

namespace fhp {

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
                                                 const FarCounts& n, const FarTeamCounts& m) {
  flags |= far_put_goal(s.f.r, i, cell);
  if (cell < 0 && m.claimed > 0) flags |= FH_APART_CLAIMED;
  fh_apart_record q;
  far_head(q, flags, view, cell, d2, block_d2, n);
  far_team_words(q, m);
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
  int cls = FAR_CLASS_NONE;
  if (w.searched) cls = FAR_CLASS_SEARCHER;
  else if (has_view && status != FH_VEHICLE_GOAL_REACHED && reach_finite(gx) && reach_finite(gy) && reach_finite(gz) &&
           (!(w.flags & FH_FRONTIER_WANTED) || skip != 0))
    cls = FAR_CLASS_STANDING;
  s.cls[i] = (unsigned char)cls;
  s.grp[i] = has_view ? (s.group ? s.group[view] : view) : 0;  // (has_view: view in [0, n_views))
}

__global__ void __launch_bounds__(64) far_spread_count_kernel(FarSpreadArgs s) {
  const int i = (int)blockIdx.x;
  const FarCounts none = {-1, -1, 0, 0, 0, 0, 0};
  far_count_body(s.f, s.cls, s.grp, s.lower, s.passes, FH_APART_UNSETTLED,
                 [&](int flags, int view, const FarTeamCounts& m) { far_spread_store(s, i, flags, view, -1, INFINITY, INFINITY, none, m); });
}

// what far_body<true> reads and calls
struct FarClaims {
  const FarSpreadArgs* s;
  FarTeam team;
  int* sum;  // LDS [4]
  int lower;

  __device__ __forceinline__ void store(int i, int flags, int view, int cell, double d2, double block_d2, const FarCounts& n, int claims, int standing,
                                        int claimed) const {
    const FarTeamCounts m = {team.group, s->pass, lower, standing, claims, claimed};
    far_spread_store(*s, i, flags, view, cell, d2, block_d2, n, m);
  }
};

__global__ void __launch_bounds__(256) far_spread_goals_kernel(FarSpreadArgs s) {
  __shared__ int s_sum[4];
  const int i = (int)blockIdx.x;
  if (fhw::uniform_i32((int)s.cls[i]) != FAR_CLASS_SEARCHER) return;  // (uniform over the workgroup)
  const int lower = fhw::uniform_i32(s.lower[i]);
  if (lower != s.pass - 1) return;
  FarClaims x;
  x.s = &s; x.sum = s_sum; x.lower = lower;
  x.team.cls = s.cls; x.team.grp = s.grp; x.team.group = fhw::uniform_i32(s.grp[i]); x.team.s2 = s.s2; x.team.k = 0;
  far_body<true>(s.f, x);
}

}  // namespace fhp

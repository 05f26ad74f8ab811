// fh_stake.hpp — the kernels of include/fasterhip_stake.h (which is the specification): the far chooser by gain (K23) inside the passes of
// the far chooser for a team (K22), and a claim that stakes a region: it takes the target blocks within r_spread of it out of T (K22's
// rule) and the unknown voxels of a cube of blocks around its own block out of every gain of the vehicle.  Included by fh_reach.hip only,
// after K23's device header and before K22's (which stays the last include).  d_work: K23's workspace (K21's words and need bytes, then
// [n_views][64 W] counts of 16 bits), then K22's tail: a class byte per vehicle (rounded up to a multiple of 64), a group per vehicle and
// `lower` per vehicle.  The need bytes are written by far_need_kernel, the summaries and counts by prospect_blocks_kernel and the class
// bytes and groups by K22's class kernel, all as they are; the host code launches them.
//   stake_count_kernel : a wavefront per vehicle, K21's far_count_body with this chooser's record.
//   stake_goals_kernel : launched once per pass p, ONE workgroup of 256 per vehicle; it returns at once unless the vehicle is a searcher
//                        with lower == p - 1 (the searching members of a group are one chain by index, so its lower peers were decided by
//                        the launches before).  Then K23's prospect_body<true>: K21's judge, summary and flood, K21's claim scan with
//                        the covered blocks in the SEVENTH bitmap C, which this kernel holds, K23's weighing without the covered counts
//                        and K23's reduction.  A word of T or of C has one writer, so the bytes do not depend on scheduling.
// No read-modify-write on global memory, no spin.  LDS of stake_goals_kernel: 7 bitmaps of FAR_WORDS words = 28 KB, 256 x 3 doubles and
// 256 x 3 x 16 bits of claims = 7.5 KB, and the slots of the reductions: below 40960 bytes, four workgroups a CU.
// Every address comes from a checked number: what K21's and K23's device headers list.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fasterhip_stake.h"
// (FarArgs, FarCounts, FarTeam, FarTeamCounts, the class bytes, FAR_WORDS, far_count_body, far_put_goal, far_head, far_team_words and fhw::
// come from K21's device header, ProspectArgs, ProspectGain, prospect_words and prospect_body from K23's; fh_reach.hip includes both
// before this)

namespace fhp {

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

// the three outputs of vehicle i, by one thread
__device__ __forceinline__ void stake_store(const StakeArgs& s, int i, int flags, int view, int cell, double d2, double block_d2, const FarCounts& n,
                                            const FarTeamCounts& m, const ProspectGain& e, int covered, int removed) {
  flags |= far_put_goal(s.p.f.r, i, cell);
  if (cell < 0 && m.claimed > 0) flags |= FH_STAKE_CLAIMED;
  fh_stake_record q;
  far_head(q, flags, view, cell, d2, block_d2, n);
  far_team_words(q, m);
  prospect_words(q, e);
  q.covered = covered; q.removed = removed;
  q.reserved_end[0] = 0; q.reserved_end[1] = 0;
  s.records[i] = q;
}

__global__ void __launch_bounds__(64) stake_count_kernel(StakeArgs s) {
#pragma clang fp contract(off)
  const int i = (int)blockIdx.x;
  const FarCounts none = {-1, -1, 0, 0, 0, 0, 0};
  const ProspectGain no_gain = {-1, 0, 0, -1};
  far_count_body(s.p.f, s.cls, s.grp, s.lower, s.passes, FH_STAKE_UNSETTLED, [&](int flags, int view, const FarTeamCounts& m) {
    stake_store(s, i, flags, view, -1, INFINITY, INFINITY, none, m, no_gain, 0, 0);
  });
}

// what prospect_body<true> reads and calls
struct StakeClaims {
  const StakeArgs* s;
  FarTeam team;
  unsigned long long* c;  // LDS [FAR_WORDS]: the covered blocks
  int* sum;               // LDS [3][4]: claimed, covered, removed per wavefront
  int lower;

  __device__ __forceinline__ void store(int i, int flags, int view, int cell, double d2, double block_d2, const FarCounts& n, const ProspectGain& e,
                                        int claims, int standing, int claimed, int covered, int removed) const {
    const FarTeamCounts m = {team.group, s->pass, lower, standing, claims, claimed};
    stake_store(*s, i, flags, view, cell, d2, block_d2, n, m, e, covered, removed);
  }
};

__global__ void __launch_bounds__(256) stake_goals_kernel(StakeArgs s) {
#pragma clang fp contract(off)
  __shared__ unsigned long long s_c[FAR_WORDS];
  __shared__ int s_sum[12];
  const int i = (int)blockIdx.x;
  if (fhw::uniform_i32((int)s.cls[i]) != FAR_CLASS_SEARCHER) return;  // (uniform over the workgroup)
  const int lower = fhw::uniform_i32(s.lower[i]);
  if (lower != s.pass - 1) return;
  StakeClaims x;
  x.s = &s; x.c = s_c; x.sum = s_sum; x.lower = lower;
  x.team.cls = s.cls; x.team.grp = s.grp; x.team.group = fhw::uniform_i32(s.grp[i]); x.team.s2 = s.s2; x.team.k = s.k;
  prospect_body<true>(s.p, x);
}

}  // namespace fhp

/* fasterhip_check.h: a fleet (include/fasterhip.h) CHECKS EVERY COMMIT AGAINST THE OTHER PLANS AND WITHHOLDS THE CONFLICTS.
 * fasterhip_separation.h measures how near the committed plans come to each other and fasterhip_traffic.h shows every vehicle the
 * others' plans as occupied points; neither can refuse: a vehicle commits whatever its solve produced.  This header adds the step
 * between commit and next goals that takes a commit back when its trajectory meets, at the same instant, what another vehicle flies.
 * The plans are aligned in time (state j of every plan, counted from the front, belongs to the instant now + j dc), so comparing a
 * candidate with the others at equal instants is exact.  A cycle with the check is
 *     ... -> safe solve -> BACKUP -> fh_fleet_commit_device (untouched) -> CHECK -> REVERT,
 * three entry points here; no entry point, struct or kernel of fasterhip.h changes and FH_ABI_VERSION stays.  C99 / C++11, includes
 * fasterhip.h.
 *
 * THE MODEL.  Everything is IEEE double, no fused multiply-add (tests/check_model.py restates it in numpy, brute force, and the kernels
 * are compared with that in every byte).  The squared distance of a position p of vehicle i to a position q of an other is the audit's
 * and the separation's:
 *     d2 = dx dx + dy dy + dz dz,   d = q - p per axis, the three products summed x, y, z from left to right.
 * Every comparison is strict.
 *   Names.  old_k: the record d_backup_vehicles[k] and the plan d_backup_plans[k * max_states ..) as fh_fleet_backup_device left them
 *     after fh_fleet_begin_device; cur_k: d_vehicles[k] and d_plans[k * max_states ..) after the commit.  An extent (plan_head, plan_size) is
 *     bad by the separation's rule: head < 0, size < 0 or head + size > max_states, decided before any state is read.  A plan with an
 *     extent (head, size), size >= 1, is at instant j at plan[head + min(j, size - 1)].pos: a plan that has ended stands at its last
 *     state.
 *   Candidate.  Vehicle i is a candidate iff cur_i.stage == FH_FLEET_STAGE_COMMITTED, cur_i.active != 0 and neither the extent of old_i nor
 *     that of cur_i is bad.  Everyone else gets the record of "nothing tested": flags = 0, n_tested = 0, first = first_other =
 *     first_kind = -1, d2 = +INFINITY.  Its kept states: kept_i = old_i.plan_size - old_i.k_end_whole - 1, the leading states cur_i
 *     shares with old_i (fh_fleet_commit_device keeps them and appends behind them).  A kept_i outside [0, min(old_i.plan_size,
 *     cur_i.plan_size)] is clamped into it and the record gets FH_CHECK_BAD_PLAN: the two records do not describe a commit.
 *   The others of candidate i.  Kind 0: old_k for every k != i whose old extent is not bad and old_k.plan_size >= 1.  Kind 1: cur_k for
 *     every k < i that is itself a candidate with cur_k.plan_size >= 1.  Lower indexes have priority, as with the traffic's
 *     FH_TRAFFIC_YIELD_TO_LOWER; a lower candidate counts even when it is withheld itself: conservative, and no record depends on another.
 *   Tested instants.  For the pair (i, other): j = kept_i, kept_i + stride, kept_i + 2 stride, ... < M with
 *     M = max(cur_i.plan_size, the size of the other), and M = min(M, count) when count > 0.
 *     The maximum matters: after i has arrived and stands, an other that still flies through it has to be seen.  The instants below
 *     kept_i are states i already flew with: a conflict there is not this commit's doing, and testing them would deadlock two vehicles
 *     that start near each other.  A candidate with cur_i.plan_size == 0 has no position and tests nothing.
 *   Conflict.  d2 < r * r at a tested instant, between cur_i at that instant and the other at that instant.  A coordinate of either side
 *     that is not finite makes d2 fail the comparison by the arithmetic itself; there is no special case.
 *   The record (32 B).  flags: FH_CHECK_CANDIDATE; FH_CHECK_BAD_PLAN (above); FH_CHECK_NOT_FINITE iff one of i's own positions that the
 *     pairs can read has a coordinate that is not finite: cur_i at j = kept_i, kept_i + stride, ... < m_i, m_i = count > 0 ?
 *     min(count, cur size) : cur size, or its last state when an instant behind its plan can be tested (cur size >= 1 and count == 0 or
 *     cur size < count); FH_CHECK_CONFLICT iff first >= 0.  n_tested = how many j = kept_i, kept_i + stride, ... < m_i there are: the
 *     tested instants of i's own plan.  first = the smallest tested j with a conflict over all others, first_other = the smallest k that
 *     conflicts at that j, first_kind = the smaller kind (0 before 1) of that k at that j, d2 = the squared distance of exactly that
 *     (first, first_other, first_kind); -1, -1, -1 and +INFINITY when there is none.  reserved = 0.
 *   Revert.  For every record with FH_CHECK_CONFLICT: d_vehicles[i] = old_i with stage = FH_FLEET_STAGE_CONFLICT, and the states
 *     [old head, old head + old size) of plan i are restored from the backup (a bad old extent restores the record alone).  Nothing else
 *     of the vehicle array and no other vehicle's plan is written; the bytes of a reverted plan outside the restored extent are
 *     unspecified.  A withheld vehicle flies on with its previous plan, status, windows and persisted safe factor, exactly like a failed
 *     replan (stages 1, 2, 3, 6).
 *
 * WHAT THIS PROMISES.  With stride == 1 and count == 0, backup before and check + revert after every commit: the set of unordered pairs
 * {i, k} that the separation's model calls near (same r, whole plans: FH_SEP_NEAR with first_other == k in record i or the reverse, i.e.
 * d2 < r r at one instant below max(size_i, size_k)) never gains a member — not by a cycle, and not by fh_fleet_next_goals_device, which
 * drops the same number of leading instants of every plan.  Pairs that are near stay allowed to be: the check creates no distance.
 * WHAT IT DOES NOT.  stride > 1 or count > 0 is a cheaper and weaker check: conflicts between or beyond the tested instants pass.  Two
 * vehicles whose new trajectories each pass through the place where the other one stands are both withheld and both stay: the check
 * guarantees separation, avoiding is the traffic's job.  A vehicle that stands within r of another one's start state A is withheld until the
 * other has left.  A vehicle that is withheld replans from the same plan next cycle; nothing here makes that replan differ.
 *
 * THE CELL GRID.  `cells` (origin, res, dims) is a uniform grid that only the broad phase uses, as in fasterhip_separation.h: a vehicle is
 * counted into the cell of the centre of the box of everything it can show (old_k, and cur_k of a candidate), a candidate looks at the
 * cells its own box, grown by r and by the largest half-extent of the fleet, reaches.  NO FIELD OF ANY RECORD DEPENDS ON THE GRID:
 * dims = (1, 1, 1) gives the same bytes, slower. */
#ifndef FASTERHIP_CHECK_H
#define FASTERHIP_CHECK_H
#include "fasterhip.h"
#ifdef __cplusplus
extern "C" {
#endif

enum {
  FH_FLEET_STAGE_CONFLICT = 7 /* fh_vehicle.stage: the replan was committed and taken back by fh_fleet_revert_device: plan, status and
                                 windows are those of before the commit (no reference counterpart, like FH_FLEET_STAGE_OVERFLOW)     */
};
enum {                       /* fh_plan_check.flags */
  FH_CHECK_BAD_PLAN = 1,     /* a candidate whose kept_i had to be clamped into [0, min(old size, cur size)]                         */
  FH_CHECK_NOT_FINITE = 4,   /* a position of the candidate's own plan that the pairs can read has a coordinate that is not finite   */
  FH_CHECK_CANDIDATE = 16,   /* committed this cycle, active, both extents good: the vehicle was checked                             */
  FH_CHECK_CONFLICT = 32     /* first >= 0: fh_fleet_revert_device takes the commit back                                             */
};
enum {
  FH_CHECK_LIST_OTHERS = 256,  /* capacity of the narrow phase's LDS list of others (it is tested and emptied when it cannot take 128
                                  more: a vehicle can enter it twice, as old_k and as cur_k)                                        */
  FH_CHECK_MAX_CELLS = 1 << 20 /* the largest dims[0] * dims[1] * dims[2] of the cell grid                                            */
};

typedef struct fh_check_params { /* 32 B */
  double r;              /* a conflict is d2 < r * r (strict) at a tested instant                                                   */
  int32_t stride, count; /* tested j = kept_i, kept_i + stride, ... < M; count > 0 caps M.  stride > 1 or count > 0: a weaker check   */
  int32_t reserved[4];
} fh_check_params;

typedef struct fh_plan_check { /* 32 B */
  int32_t flags, n_tested;     /* n_tested: the tested instants of the candidate's own plan                                          */
  int32_t first, first_other;  /* the smallest tested j with a conflict; the smallest vehicle that conflicts at that j               */
  int32_t first_kind, reserved; /* 0: with old_k (what k flew before this cycle's commit), 1: with cur_k (k < i committed as well)    */
  double d2;                   /* the squared distance of that conflict; +INFINITY when there is none                               */
} fh_plan_check;

/* Copies, for every vehicle, the record d_vehicles[i] to d_backup_vehicles[i] and the live extent [plan_head, plan_head + plan_size) of
 * its plan to the same indexes of d_backup_plans (n * max_states states, like d_plans); a bad extent gets its record copied only.  One
 * launch, asynchronous on the context's stream; device pointers, every array aligned to 16 bytes.  Between fh_fleet_begin_device (which
 * sets active and k_end_whole) and fh_fleet_commit_device.  FH_ERR_ARG after a null context: n < 0, max_states < 1; then FH_ERR_DEVICE
 * without a device, FH_OK for n == 0, FH_ERR_ARG for a null pointer. */
int fh_fleet_backup_device(fh_ctx* ctx, const fh_vehicle* d_vehicles, const fh_state* d_plans, int n, int max_states,
                           fh_vehicle* d_backup_vehicles, fh_state* d_backup_plans);

/* d_out[i] = the check record of vehicle i: a pure measurement, as fh_fleet_separation_device is.  Four launches on the context's
 * stream (boxes, cell starts, cell items, the narrow phase: one wavefront per candidate), asynchronous; written: d_out and working buffers
 * of the context, which every call sets up again on the stream.  FH_ERR_ARG, checked in this order after a null context: par == NULL; r
 * that is NaN, negative or infinite; stride < 1; count < 0; n < 0; max_states < 1; cells == NULL, res <= 0, a dimension < 1,
 * dims[0] dims[1] dims[2] > FH_CHECK_MAX_CELLS.  Then FH_ERR_DEVICE without a device (there is no CPU path), FH_OK for n == 0, and
 * FH_ERR_ARG for a null d_vehicles, d_plans, d_backup_vehicles, d_backup_plans or d_out.  Every index the kernels use comes from a
 * record they have checked: a wrong vehicle record gives a flag or no candidate, never a read outside the arrays. */
int fh_fleet_check_device(fh_ctx* ctx, const fh_check_params* par, const fh_vehicle* d_vehicles, const fh_state* d_plans,
                          const fh_vehicle* d_backup_vehicles, const fh_state* d_backup_plans, int n, int max_states,
                          const struct fh_voxel_grid* cells, fh_plan_check* d_out);

/* Takes back the commit of every vehicle whose record d_out[i] has FH_CHECK_CONFLICT (the revert of the model above); the others are
 * not touched.  One launch, asynchronous on the context's stream.  FH_ERR_ARG after a null context: n < 0, max_states < 1; then
 * FH_ERR_DEVICE without a device, FH_OK for n == 0, FH_ERR_ARG for a null pointer. */
int fh_fleet_revert_device(fh_ctx* ctx, const fh_plan_check* d_out, const fh_vehicle* d_backup_vehicles, const fh_state* d_backup_plans, int n,
                           int max_states, fh_vehicle* d_vehicles, fh_state* d_plans);

#ifdef __cplusplus
}
#endif
#endif /* FASTERHIP_CHECK_H */

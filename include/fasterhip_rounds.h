/* fasterhip_rounds.h: a fleet (include/fasterhip.h) REPLANS IN PRIORITY ROUNDS, AND A LATER ROUND SEES WHAT THE EARLIER ONES COMMITTED.
 * fasterhip_traffic.h shows every vehicle the others' plans and fasterhip_check.h takes a conflicting commit back, but all vehicles plan
 * at once: both sides of a crossing replan from the same stale picture, and a withheld vehicle replans from the same plan next cycle.
 * Prioritised planning splits a cycle into rounds.  Vehicles that can come near each other go into different rounds; the vehicles of a
 * round see, through the existing traffic stage, what the rounds before them committed moments ago, and with the check each round is
 * backed up, checked and reverted on its own.  Two entry points: one decides the round of every vehicle (its class), one switches the
 * vehicles of a round on and all others off.  A cycle in rounds is
 *     begin -> CLASSES -> for every round: GATE -> [traffic] -> path search -> ... -> commit [-> check -> revert] -> GATE (restore);
 * no entry point, struct or kernel of fasterhip.h changes and FH_ABI_VERSION stays.  C99 / C++11, includes fasterhip.h.
 *
 * THE MODEL.  Everything is IEEE double, no fused multiply-add (tests/rounds_model.py restates it in numpy, brute force, and the kernels
 * are compared with that in every byte).  The squared distance of two positions is the check's:
 *     d2 = dx dx + dy dy + dz dz,   d = q - p per axis, the three products summed x, y, z from left to right.
 * Every comparison is strict.
 *   Plans.  An extent (plan_head, plan_size) is bad by the separation's rule: head < 0, size < 0 or head + size > max_states, decided
 *     before any state is read.  A plan with a good extent and size >= 1 is at instant j at plan[head + min(j, size - 1)].pos: a plan
 *     that has ended stands at its last state.
 *   Neighbours.  i and k (i != k) are neighbours iff both have a good extent with size >= 1 and there is a tested instant
 *     j = 0, stride, 2 stride, ... < M with d2 < reach * reach between the two plans at j, where M = max(size_i, size_k), and
 *     M = min(M, count) when count > 0.  Symmetric by construction.  A coordinate that is not finite makes d2 fail the comparison by the
 *     arithmetic itself; there is no special case.
 *   Flags of the plan.  FH_ROUND_BAD_PLAN: the extent of i is bad; such a vehicle has no neighbours.  FH_ROUND_NOT_FINITE: one of i's
 *     own positions that the pairs can read has a coordinate that is not finite, by the rule of FH_CHECK_NOT_FINITE with kept = 0: the
 *     states j = 0, stride, ... < m_i, m_i = count > 0 ? min(count, size_i) : size_i, or the last state when an instant behind the plan can
 *     be tested (size_i >= 1 and count == 0 or size_i < count).
 *   n_lower = the number of neighbours k < i, exact even above the capacity of the list (FH_ROUNDS_LIST).
 *   Pass 0.  n_lower == 0: round_class = 0, decided_pass = 0.  n_lower > FH_ROUNDS_LIST: round_class = rounds - 1, FH_ROUND_OVERFLOW,
 *     decided_pass = 0.  Everyone else starts undecided: round_class = -1, decided_pass = -1.
 *   Pass p = 1 .. passes.  An undecided i is decided in pass p iff every lower neighbour k has 0 <= decided_pass_k < p; then
 *     round_class_i = min(mex of the classes of its lower neighbours, rounds - 1) (mex: the smallest class >= 0 none of them has) and
 *     decided_pass_i = p.  Nothing a pass decides is seen by that same pass.
 *   After the last pass.  A vehicle that is still undecided gets round_class = rounds - 1, FH_ROUND_UNSETTLED and decided_pass = -1.
 * TWO CONSEQUENCES (tests/test_rounds_model.py).  With enough passes (n - 1 always suffice) and no flag in any record, the classes are
 * those of sequential greedy colouring in index order, clipped at rounds - 1.  Two neighbours without flags share a class only if it is
 * rounds - 1: whoever shares a round below the last cannot come within `reach` at a tested instant of the plans the classes were made from.
 * rounds == 1 gives class 0 everywhere.
 *
 * THE CELL GRID.  `cells` (origin, res, dims) is a uniform grid that only the broad phase uses, as in fasterhip_check.h.  NO FIELD OF ANY
 * RECORD DEPENDS ON THE GRID: dims = (1, 1, 1) gives the same bytes, slower. */
#ifndef FASTERHIP_ROUNDS_H
#define FASTERHIP_ROUNDS_H
#include "fasterhip.h"
#ifdef __cplusplus
extern "C" {
#endif

enum {
  FH_ROUNDS_MAX = 64,          /* the largest `rounds`: the mex of a pass is taken with a mask of 64 bits                              */
  FH_ROUNDS_LIST = 64,         /* lower neighbours kept per vehicle; a vehicle with more goes into the last round (FH_ROUND_OVERFLOW)  */
  FH_ROUNDS_MAX_PASSES = 1024, /* the largest `passes`: every pass is one launch                                                       */
  FH_ROUNDS_MAX_CELLS = 1 << 20 /* the largest dims[0] * dims[1] * dims[2] of the cell grid                                            */
};
enum {                   /* the `round` of fh_fleet_round_gate_device below zero */
  FH_ROUND_RESTORE = -1, /* every vehicle as fh_fleet_begin_device left it                                                           */
  FH_ROUND_RETRY = -2    /* the vehicles whose commit was taken back (stage FH_FLEET_STAGE_CONFLICT, fasterhip_check.h: 7)           */
};
enum {                      /* fh_plan_round.flags */
  FH_ROUND_OVERFLOW = 1,    /* more than FH_ROUNDS_LIST lower neighbours: the last round, decided in pass 0                          */
  FH_ROUND_UNSETTLED = 2,   /* undecided after the last pass: the last round                                                        */
  FH_ROUND_NOT_FINITE = 4,  /* a position of the vehicle's own plan that the pairs can read has a coordinate that is not finite     */
  FH_ROUND_BAD_PLAN = 8     /* a bad extent: no neighbours                                                                          */
};

typedef struct fh_round_params { /* 32 B */
  double reach;            /* neighbours: d2 < reach * reach (strict) at a tested instant                                            */
  int32_t rounds, passes;  /* classes 0 .. rounds - 1; the passes after pass 0 (one launch each)                                     */
  int32_t stride, count;   /* tested j = 0, stride, ... < M; count > 0 caps M                                                        */
  int32_t reserved[2];
} fh_round_params;

typedef struct fh_plan_round { /* 16 B; round_class and decided_pass are one aligned word of 8 bytes, always read and written whole */
  int32_t round_class;   /* the round the vehicle replans in                                                                        */
  int32_t decided_pass;  /* the pass that decided it; -1: FH_ROUND_UNSETTLED                                                         */
  int32_t n_lower;       /* neighbours with a lower index                                                                           */
  int32_t flags;
} fh_plan_round;

/* d_out[i] = the round record of vehicle i: a pure measurement of d_vehicles and d_plans.  Launches on the context's stream,
 * asynchronous: boxes, cell starts, cell items, the narrow phase (one wavefront per vehicle), `passes` pass launches, one that settles
 * the rest; written: d_out and working buffers of the context, which every call sets up again on the stream.  RACE-FREE AND
 * DETERMINISTIC: a pass reads the (round_class, decided_pass) word of a lower neighbour with one load of 8 bytes while the same launch
 * may be storing it with one store of 8 bytes; it sees either decided_pass = -1 or decided_pass = p, and the test decided_pass < p
 * (with >= 0) makes both mean "undecided".  No kernel waits for another wavefront.
 * FH_ERR_ARG, checked in this order after a null context: par == NULL; reach that is NaN, negative or infinite; rounds outside
 * [1, FH_ROUNDS_MAX]; passes outside [0, FH_ROUNDS_MAX_PASSES]; stride < 1; count < 0; n < 0; max_states < 1; cells == NULL, res <= 0,
 * a dimension < 1, dims[0] dims[1] dims[2] > FH_ROUNDS_MAX_CELLS.  Then FH_ERR_DEVICE without a device (there is no CPU path), FH_OK
 * for n == 0, and FH_ERR_ARG for a null d_vehicles, d_plans or d_out.  Every index the kernels use comes from a record they have
 * checked. */
int fh_fleet_round_classes_device(fh_ctx* ctx, const fh_round_params* par, const fh_vehicle* d_vehicles, const fh_state* d_plans, int n,
                                  int max_states, const struct fh_voxel_grid* cells, fh_plan_round* d_out);

/* Switches the vehicles of one round on and everyone else off: on_i = d_active_begin[i] != 0 && (round >= 0: d_rounds[i].round_class ==
 * round; FH_ROUND_RETRY: d_vehicles[i].stage == FH_FLEET_STAGE_CONFLICT; FH_ROUND_RESTORE: true); d_vehicles[i].active = on_i and
 * d_active[i] = on_i (0 or 1), and nothing else is written.  d_active_begin is what fh_fleet_begin_device wrote as its d_active;
 * d_active is what the path search reads.  d_rounds may be NULL for the two negative rounds.  One launch, asynchronous on the
 * context's stream.  FH_ERR_ARG after a null context: round < FH_ROUND_RETRY, round >= FH_ROUNDS_MAX, n < 0, d_active_begin ==
 * d_active; then FH_ERR_DEVICE without a device, FH_OK for n == 0, FH_ERR_ARG for a null pointer that is needed. */
int fh_fleet_round_gate_device(fh_ctx* ctx, const fh_plan_round* d_rounds, int round, const int32_t* d_active_begin, int n,
                               fh_vehicle* d_vehicles, int32_t* d_active);

#ifdef __cplusplus
}
#endif
#endif /* FASTERHIP_ROUNDS_H */

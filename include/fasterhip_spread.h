/* fasterhip_spread.h: A TEAM SPREADS OVER ITS FRONTIERS — GOALS CLAIMED BY PEERS ARE AVOIDED.  fh_reach_goals_device
 * (include/fasterhip_reach.h) decides for every vehicle alone: two vehicles with equal views that stand close together choose the same
 * voxel, one uncovers it, the other arrives at a place that is no frontier any more.  The entry point of this header is that chooser
 * with one more rule: a candidate nearer than r_spread to a goal that a PEER holds or has just been given is not chosen.  Peers are the
 * vehicles of one group (the labels of fh_fleet_link_groups_device, or the view); who yields is decided by the vehicle index.  A closed
 * period is
 *     sense -> observe -> [link] -> SPREAD GOALS -> fh_fleet_set_goals_device -> replan -> next goals
 * A pure measurement: no entry point, struct or kernel of the other headers changes and FH_ABI_VERSION stays.  C99 / C++11, includes
 * fasterhip.h, fasterhip_frontier.h and fasterhip_reach.h (the FH_FRONTIER_* and FH_REACH_* constants are reused).
 *
 * THE MODEL (tests/spread_model.py restates it in Python over the vehicles in index order; the kernels are compared with that in every
 * byte).  IEEE double, no fused multiply-add.  Every squared length is summed x, y, z from the left, of other - own.  Every radius is
 * squared once on the host: r_spread r_spread, reach reach with reach = (r_max + r_max) + r_spread, near near with near = r_max +
 * r_spread.  Every comparison is strict.
 *   Views, wanted, NO_VIEW, BAD_POS, eligible, start cell, box, box cap, passable, flood, candidate: fasterhip_reach.h's, word for word.
 *     Vehicle i is a SEARCHER iff that header would search it: eligible, start inside the lattice, box within FH_REACH_MAX_WORDS.
 *   Groups.  group(i) = d_group ? d_group[view(i)] : view(i) for a vehicle whose view is in [0, n_views); 0 in the record of any other.
 *     It is compared for equality only and never used as an index: any int32 is a label.  Two vehicles are PEERS iff both have a view
 *     in range, they are different vehicles and their groups are equal.
 *   Class.  searcher: as above.  standing: not wanted, view in range, status != FH_VEHICLE_GOAL_REACHED and the three coordinates of
 *     g_term finite — on its way to a goal it holds.  none: every other vehicle, a wanted one that is not a searcher and a
 *     GOAL_REACHED one that is not wanted among them.
 *   Lists of searcher i.  LOWER PEERS: the peers k < i of class searcher with d2(pos_k, pos_i) < reach reach.  STANDING CLAIMS: the
 *     peers k (below or above i) of class standing with d2(g_term_k, pos_i) < near near.  `lower` and `standing` are the exact sizes
 *     of the two lists.  The restrictions are part of the model; but for rounding a peer outside them cannot matter: a candidate of
 *     i is nearer than r_max to pos_i, a goal given to k nearer than r_max to pos_k, so beyond reach the two are r_spread apart, and
 *     a g_term beyond near is r_spread from every candidate of i.
 *   Pass 0.  A vehicle that is not a searcher gets the outputs of fasterhip_reach.h for it (cell = hops = -1, counts 0, d2 = +inf,
 *     the bits of g_term, mask 0) and decided_pass = 0.  A searcher with lower + standing > FH_SPREAD_LIST gets FH_SPREAD_OVERFLOW,
 *     is not searched (the same outputs, with `lower`, and claims = standing) and has decided_pass = 0.  Every other searcher starts
 *     undecided, decided_pass = -1.
 *   Pass p = 1 .. passes.  An undecided searcher i is decided in pass p iff every lower peer k has 0 <= decided_pass_k < p: nothing a
 *     pass decides is seen by that same pass.  Its CLAIMS are the g_term of its standing claims and the d_goals of the lower peers
 *     with d_mask == 1 (an overflowed peer, or one that found nothing, claims nothing).  A candidate q is CLAIMED iff s2(q, c) <
 *     r_spread r_spread for some claim c.  The choice is fasterhip_reach.h's, the smallest (hops, d2, cell), over the candidates that
 *     are in some level and not claimed.
 *   After the last pass a searcher still undecided gets FH_SPREAD_UNSETTLED: mask 0, the bits of g_term, decided_pass = -1, claims =
 *     standing, the counts of a vehicle that is not searched.  It keeps its status, so the next period wants it again.
 *   Record.  flags: those of fh_reach_record | FH_SPREAD_OVERFLOW | FH_SPREAD_UNSETTLED | FH_SPREAD_CLAIMED (searched, no choice, and
 *     claimed > 0).  view, cell, hops, reached, levels, d2 as there.  candidates: that header's count, claims or not.  reachable: the
 *     candidates in some level that are not claimed.  group, decided_pass, lower as above.  claims = standing + the lower peers with
 *     d_mask == 1.  claimed: the candidates, reachable or not, within r_spread of a claim.  reserved = 0.
 *   Every byte of all three outputs is written by every call.
 *   Consequences.  When no searcher has a peer, d_goals, d_mask and the first 40 bytes of every record are fh_reach_goals_device's.
 *     With enough passes and no OVERFLOW no two peers within reach of each other are given goals nearer than r_spread, and no goal lies
 *     within r_spread of a standing claim on its vehicle's list.
 *
 * KNOWN LIMITS.  The vehicle index decides who yields: the lower index chooses first, however far its way is.  Claims are points, not
 * regions: a sensor uncovers a ball around a goal, and r_spread stands for it.  The goal of a peer whose replan then fails stays a
 * claim for that period.  Every searcher scans all n vehicles (no broad phase).  A chain of lower peers longer than `passes` leaves
 * its tail FH_SPREAD_UNSETTLED for a period. */
#ifndef FASTERHIP_SPREAD_H
#define FASTERHIP_SPREAD_H
#include "fasterhip.h"
#include "fasterhip_frontier.h"
#include "fasterhip_reach.h"
#ifdef __cplusplus
extern "C" {
#endif

enum {
  FH_SPREAD_OVERFLOW = 128,  /* fh_spread_record.flags, beside those of fh_reach_record: lower + standing > FH_SPREAD_LIST, not searched  */
  FH_SPREAD_UNSETTLED = 256, /*                           a lower peer was still undecided after the last pass: not searched              */
  FH_SPREAD_CLAIMED = 512    /*                           searched, nothing chosen, and claimed > 0                                       */
};
enum { FH_SPREAD_LIST = 32, FH_SPREAD_MAX_PASSES = 64, FH_SPREAD_DEFAULT_PASSES = 8 };

typedef struct fh_spread_params { /* 80 B: the first 40 bytes are fh_reach_params' */
  double r_max;     /* as fh_reach_params                                                                                            */
  double r_avoid;
  double z_lo;
  double z_hi;
  int32_t want;
  int32_t max_hops;
  double r_spread;  /* no candidate with s2 < r_spread * r_spread around a claim; finite and > 0                                     */
  int32_t passes;   /* 1 .. FH_SPREAD_MAX_PASSES                                                                                     */
  int32_t reserved[7];
} fh_spread_params;

typedef struct fh_spread_record { /* 64 B: the first 40 bytes are laid out as fh_reach_record's */
  int32_t flags;        /* fh_reach_record's | FH_SPREAD_OVERFLOW | UNSETTLED | CLAIMED                                              */
  int32_t view;
  int32_t cell;
  int32_t hops;
  int32_t candidates;   /* claimed or not                                                                                            */
  int32_t reachable;    /* in some level and not claimed                                                                             */
  int32_t reached;
  int32_t levels;
  double d2;
  int32_t group;        /* group(i); 0 without a view in range                                                                       */
  int32_t decided_pass; /* 0: not a searcher, or OVERFLOW; 1 .. passes: searched in that pass; -1: UNSETTLED                         */
  int32_t lower;        /* the size of the list of lower peers, also beyond FH_SPREAD_LIST                                           */
  int32_t claims;       /* standing + the lower peers with d_mask == 1 (OVERFLOW, UNSETTLED: standing)                               */
  int32_t claimed;      /* candidates, reachable or not, within r_spread of a claim                                                  */
  int32_t reserved;     /* 0                                                                                                         */
} fh_spread_record;

/* The bytes of d_work for n vehicles: a class byte per vehicle, rounded up to a multiple of 64, and a row of FH_SPREAD_LIST int32 per
 * vehicle.  0 for n <= 0. */
size_t fh_spread_work_bytes(int n);

/* d_goals [n][3], d_mask [n] int32 and d_records [n] as above, in the shape fh_fleet_set_goals_device takes.  map_grid, d_map_bits, grid,
 * d_flags, view_stride, d_view_of, n_views, d_vehicles: those of fh_reach_goals_device.  d_group [n_views] int32 or NULL.  d_work: device
 * memory of this call alone, work_bytes >= fh_spread_work_bytes(n), aligned to 4 bytes (any device allocation is); what it holds
 * afterwards has no meaning.  2 + passes launches on `stream` (a hipStream_t, NULL: the default stream), asynchronous, on the device
 * that owns d_records: a thread per vehicle for the classes; a wavefront per vehicle that scans all n vehicles in chunks of 64 for the
 * two lists; then per pass a workgroup of 256 per vehicle, which returns at once unless the vehicle is decided by that pass.  No
 * atomics, no kernel waits for another wavefront.  DETERMINISTIC: a pass reads of other vehicles only what earlier launches wrote.
 * FH_ERR_ARG, checked in this order, all before the first call of the runtime: the clauses of fh_reach_goals_device from par == NULL to
 * n < 0, in its order; r_spread NaN, infinite or <= 0; passes < 1 or > FH_SPREAD_MAX_PASSES.  Then FH_OK for n == 0, then FH_ERR_ARG
 * for a null d_flags, d_vehicles, d_goals, d_mask or d_records; a null d_work; work_bytes < fh_spread_work_bytes(n).  d_view_of and
 * d_group may be NULL.  FH_ERR_DEVICE: d_records is no device memory, or a launch failed.  Every index the kernels use comes from a
 * value they have checked. */
int fh_spread_goals_device(void* stream, const fh_spread_params* par, const struct fh_voxel_grid* map_grid, const unsigned* d_map_bits,
                           const struct fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of,
                           int n_views, const int32_t* d_group, const fh_vehicle* d_vehicles, int n, void* d_work, size_t work_bytes,
                           double* d_goals, int32_t* d_mask, fh_spread_record* d_records);

#ifdef __cplusplus
}
#endif
#endif /* FASTERHIP_SPREAD_H */

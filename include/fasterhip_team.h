/* fasterhip_team.h: GAIN-AWARE GOALS FOR A TEAM — CLAIMED SPACE IS NOT COUNTED TWICE.  The exploration loop has two choosers that
 * solve half of one problem each: the chooser for a team with point claims (K16) keeps teammates off each other's voxels but picks by
 * the fewest steps; the chooser by what a goal would uncover (K17) weighs the unknown space around a candidate but decides for every
 * vehicle alone, so teammates with equal views choose the same voxel.  The entry point of this header is K17's utility inside K16's
 * passes, and a peer's claim removes two things: the candidates next to it (K16's rule), and, from every gain, the unknown voxels that
 * the peer's sensor will uncover anyway.  Claims are regions: two teammates in front of one hall get goals whose balls do not count
 * the same voxels twice.  A closed period is
 *     sense -> observe -> [link] -> TEAM GOALS -> fh_fleet_set_goals_device -> replan -> next goals
 * A pure measurement: no entry point, struct or kernel of the other headers changes and FH_ABI_VERSION stays.  C99 / C++11, includes
 * fasterhip.h, fasterhip_frontier.h and fasterhip_reach.h.  The headers of K16 and K17 each ask that no other header names them, so
 * this one carries the constants it shares with them under names of its own, with the same values (tests/test_team_abi.py compares
 * them): FH_TEAM_OVERFLOW, UNSETTLED, CLAIMED, LIST, MAX_PASSES and DEFAULT_PASSES are K16's, FH_TEAM_MAX_RADIUS and
 * FH_TEAM_MAX_HOP_COST K17's; K17's ALL_POOR bit is K16's OVERFLOW bit (128), so FH_TEAM_ALL_POOR is a bit of its own.
 *
 * THE MODEL (tests/team_model.py restates it in Python on top of the models of K16 and K17; the kernels are compared with that in
 * every byte).  IEEE double, no fused multiply-add, every squared length summed x, y, z from the left of other - own, every radius
 * squared once on the host, as in K16; everything K17 and this header add is integer arithmetic.
 *   Kept from K16, word for word.  Views, wanted, eligible, start cell, box, box cap, passable, flood, candidate, groups, peers, classes
 *     (searcher, standing, none), lower peers and standing claims, pass 0, the passes ("an undecided searcher i is decided in pass p iff
 *     every lower peer k has 0 <= decided_pass_k < p: nothing a pass decides is seen by that same pass"), OVERFLOW (lower + standing >
 *     FH_TEAM_LIST), UNSETTLED, the claims of a decided searcher (the g_term of its standing claims and the d_goals of the lower peers
 *     with d_mask == 1), and CLAIMED: a candidate q is claimed iff s2(q, c) < r_spread r_spread for some claim c, strict.
 *   One change: the interaction radius.  r_int = r_spread if claim_radius < 0, else
 *     r_int = fmax(r_spread, (double)(gain_radius + claim_radius + 1) * grid->res), computed once on the host.  Then reach =
 *     (r_max + r_max) + r_int and near = r_max + r_int, each squared once on the host, take the places of K16's reach and near in the
 *     two lists.  The widened restrictions are part of the model; a peer beyond them cannot touch the ball of a candidate.
 *   Claim voxel.  The voxel of a claim c is k = floor((c - origin) / res) per axis, the double expression that the start cell uses; it
 *     is an integer of any size and may lie outside the box or outside the lattice.
 *   Covered.  An unknown voxel u of the box (K17's unknown: F[u] != 0) is COVERED iff claim_radius >= 0 and
 *     (ux - kx)^2 + (uy - ky)^2 + (uz - kz)^2 <= claim_radius^2 for the voxel k of some claim: integer arithmetic, <=.  `covered`
 *     counts the union, every voxel once.
 *   Gain.  gain(c) is K17's count over the unknown voxels of the box that are not covered.
 *   Utility, poor, choice.  utility(c) = gain(c) - hop_cost * hops(c); a candidate in some level with gain(c) < min_gain is POOR.
 *     reachable, poor, best_gain and the choice run over the candidates in some level that are NOT CLAIMED.  The choice is the largest
 *     utility of those that are not poor, then the smallest (hops, d2, cell).
 *   Flags.  Those of fh_reach_record | FH_TEAM_OVERFLOW | FH_TEAM_UNSETTLED | FH_TEAM_CLAIMED (searched, nothing chosen, claimed > 0)
 *     | FH_TEAM_ALL_POOR (searched, reachable > 0 and poor == reachable).
 *   Not searched.  A vehicle that is not searched (no searcher, OVERFLOW, UNSETTLED) gets K16's outputs for it and gain = best_gain =
 *     -1, utility = poor = covered = 0.
 *   Every byte of all three outputs is written by every call.
 *   Reduction A.  With claim_radius = -1, gain_radius = 0, hop_cost = 1 and min_gain = 0: r_int = r_spread, every gain is 0, nothing is
 *     poor and the utility is -hops, so d_goals, d_mask and the first 64 bytes of every record are those of K16's entry point.
 *   Reduction B.  When no searcher has a peer: d_goals and d_mask are those of K17's entry point, bytes 0 .. 39 of every record equal
 *     that record's with bit 128 read as bit 1024, and bytes 64 .. 79 (gain, utility, poor, best_gain) equal its bytes 40 .. 55.
 *
 * KNOWN LIMITS.  The vehicle index still decides who yields.  The widened lists overflow FH_TEAM_LIST sooner than K16's.  No occlusion,
 * and both balls are clipped to the box, as in K17.  The goal of a peer whose replan then fails stays a claim, point and ball, for that
 * period.  Every searcher scans all n vehicles (no broad phase); a chain of lower peers longer than `passes` leaves its tail
 * FH_TEAM_UNSETTLED for a period. */
#ifndef FASTERHIP_TEAM_H
#define FASTERHIP_TEAM_H
#include "fasterhip.h"
#include "fasterhip_frontier.h"
#include "fasterhip_reach.h"
#ifdef __cplusplus
extern "C" {
#endif

enum {
  FH_TEAM_OVERFLOW = 128,  /* fh_team_record.flags, beside those of fh_reach_record: lower + standing > FH_TEAM_LIST, not searched      */
  FH_TEAM_UNSETTLED = 256, /*                         a lower peer was still undecided after the last pass: not searched                */
  FH_TEAM_CLAIMED = 512,   /*                         searched, nothing chosen, and claimed > 0                                         */
  FH_TEAM_ALL_POOR = 1024  /*                         searched, candidates that are not claimed were reached, all of them poor          */
};
enum { FH_TEAM_LIST = 32, FH_TEAM_MAX_PASSES = 64, FH_TEAM_DEFAULT_PASSES = 8, FH_TEAM_MAX_RADIUS = 31, FH_TEAM_MAX_HOP_COST = 16384 };

typedef struct fh_team_params { /* 80 B: K16's params with four of their reserved words in use */
  double r_max;         /* as fh_reach_params                                                                                        */
  double r_avoid;
  double z_lo;
  double z_hi;
  int32_t want;
  int32_t max_hops;
  double r_spread;      /* no candidate with s2 < r_spread * r_spread around a claim; finite and > 0                                 */
  int32_t passes;       /* 1 .. FH_TEAM_MAX_PASSES                                                                                   */
  int32_t gain_radius;  /* g, in voxels of the views' lattice: 0 .. FH_TEAM_MAX_RADIUS                                               */
  int32_t hop_cost;     /* unknown voxels that one step of the flood is worth: 0 .. FH_TEAM_MAX_HOP_COST                             */
  int32_t min_gain;     /* a candidate with a smaller gain is poor; >= 0                                                             */
  int32_t claim_radius; /* the ball, in voxels, that a claim covers: 0 .. FH_TEAM_MAX_RADIUS; -1: claims cover nothing               */
  int32_t reserved[3];
} fh_team_params;

typedef struct fh_team_record { /* 96 B: the first 64 bytes are laid out as K16's record, the first 40 as fh_reach_record */
  int32_t flags;        /* fh_reach_record's | FH_TEAM_OVERFLOW | UNSETTLED | CLAIMED | ALL_POOR                                     */
  int32_t view;
  int32_t cell;         /* the chosen cell of the lattice, -1: none                                                                  */
  int32_t hops;         /* its level, -1: none                                                                                       */
  int32_t candidates;   /* claimed or not                                                                                            */
  int32_t reachable;    /* in some level and not claimed                                                                             */
  int32_t reached;
  int32_t levels;
  double d2;            /* of the chosen cell, +inf: none                                                                            */
  int32_t group;        /* group(i); 0 without a view in range                                                                       */
  int32_t decided_pass; /* 0: not a searcher, or OVERFLOW; 1 .. passes: searched in that pass; -1: UNSETTLED                         */
  int32_t lower;        /* the size of the list of lower peers, also beyond FH_TEAM_LIST                                             */
  int32_t claims;       /* standing + the lower peers with d_mask == 1 (OVERFLOW, UNSETTLED: standing)                               */
  int32_t claimed;      /* candidates, reachable or not, within r_spread of a claim                                                  */
  int32_t reserved0;    /* 0                                                                                                         */
  int32_t gain;         /* of the chosen cell, covered voxels not counted; -1: none                                                  */
  int32_t utility;      /* of the chosen cell, 0: none                                                                               */
  int32_t poor;         /* candidates in some level, not claimed, with a gain below min_gain                                         */
  int32_t best_gain;    /* the largest gain of a candidate in some level that is not claimed, poor ones included; -1: none           */
  int32_t covered;      /* unknown voxels of the box inside the ball of at least one claim, each counted once                        */
  int32_t reserved[3];  /* 0                                                                                                         */
} fh_team_record;

/* d_goals [n][3], d_mask [n] int32 and d_records [n] as above, in the shape fh_fleet_set_goals_device takes.  The arguments after par
 * are exactly those of K16's entry point: map_grid, d_map_bits, grid, d_flags, view_stride, d_view_of, n_views, d_vehicles as for
 * fh_reach_goals_device; d_group [n_views] int32 or NULL; d_work: device memory of this call alone, aligned to 4 bytes, work_bytes >=
 * ((n + 63) & ~63) + n * FH_TEAM_LIST * 4 (what K16's work-bytes function returns for n: a class byte per vehicle, rounded up to a
 * multiple of 64, and a row of FH_TEAM_LIST int32 per vehicle); what it holds afterwards has no meaning.  2 + passes launches on
 * `stream` (a hipStream_t, NULL: the default stream), asynchronous, on the device that owns d_records: K16's class kernel, a thread
 * per vehicle; a wavefront per vehicle that scans all n vehicles for the two lists; then per pass a workgroup of 256 per vehicle, which
 * returns at once unless the vehicle is decided by that pass.  No atomics, no kernel waits for another wavefront.  DETERMINISTIC: a pass
 * reads of other vehicles only what earlier launches wrote; integer counts and the extremum of a total order.
 * FH_ERR_ARG, checked in this order, all before the first call of the runtime: the clauses of fh_reach_goals_device from par == NULL to
 * n < 0, in its order; r_spread NaN, infinite or <= 0; passes < 1 or > FH_TEAM_MAX_PASSES (so far K16's clauses); gain_radius < 0 or >
 * FH_TEAM_MAX_RADIUS; hop_cost < 0 or > FH_TEAM_MAX_HOP_COST; min_gain < 0; claim_radius < -1 or > FH_TEAM_MAX_RADIUS.  Then FH_OK for n == 0, then FH_ERR_ARG for a null d_flags, d_vehicles,
 * d_goals, d_mask or d_records; a null d_work; work_bytes too small.  d_view_of and d_group may be NULL.  FH_ERR_DEVICE: d_records is no
 * device memory, or a launch failed.  Every index the kernels use comes from a value they have checked. */
int fh_team_goals_device(void* stream, const fh_team_params* par, const struct fh_voxel_grid* map_grid, const unsigned* d_map_bits,
                         const struct fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of,
                         int n_views, const int32_t* d_group, const fh_vehicle* d_vehicles, int n, void* d_work, size_t work_bytes,
                         double* d_goals, int32_t* d_mask, fh_team_record* d_records);

#ifdef __cplusplus
}
#endif
#endif /* FASTERHIP_TEAM_H */

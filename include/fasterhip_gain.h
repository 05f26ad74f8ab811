/* fasterhip_gain.h: FRONTIER GOALS CHOSEN BY WHAT THEY WOULD UNCOVER.  fh_reach_goals_device (include/fasterhip_reach.h) takes, of the
 * frontier voxels that a flood of known free space reaches, the one with the fewest steps: a one-voxel hole of unknown space two steps
 * away beats the edge of an unexplored hall ten steps away, every period, until the hole is filled.  The entry point of this header has
 * the same inputs and outputs and a richer record, and weighs the unknown space near a candidate against the steps to it, the ordinary
 * next-best-view rule of frontier exploration:
 *     utility(c) = (unknown voxels in a ball around c) - hop_cost * hops(c).
 * A closed period is
 *     sense -> observe -> [link] -> GAIN GOALS -> fh_fleet_set_goals_device -> replan -> next goals
 * It is a pure measurement: no entry point, struct or kernel of fasterhip.h, fasterhip_frontier.h or fasterhip_reach.h changes and
 * FH_ABI_VERSION stays.  It takes the map's lattice and bits as arguments and a stream; no handle is needed.
 * C99 / C++11, includes fasterhip.h, fasterhip_frontier.h and fasterhip_reach.h (FH_FRONTIER_WANT_*, FH_REACH_MAX_WORDS and the record
 * flags of those headers are reused).
 *
 * THE MODEL (tests/gain_model.py restates it in Python, and the kernel is compared with that in every byte).  It is the model of
 * fasterhip_reach.h word for word except where stated.  IEEE double for what that header computes, no fused multiply-add, comparisons
 * as written; everything this header adds is integer arithmetic.
 *   Views, wanted, eligible, start cell, box, box cap (FH_REACH_MAX_WORDS), searched, passable, flood (six neighbours, max_hops),
 *     candidate.  As in fasterhip_reach.h, unchanged.  hops(c) = the level of c.
 *   Unknown.  A voxel u of the box is UNKNOWN iff F[u] != 0.  The map bits do not enter: an unknown voxel whose map cell is occupied
 *     counts.  Voxels outside the box are never counted.
 *   Gain.  For a candidate c at (cx, cy, cz), gain(c) = the number of unknown voxels u of the box with
 *     (ux - cx)^2 + (uy - cy)^2 + (uz - cz)^2 <= g^2, g = gain_radius: a ball in voxel units, so a row of it is at most 63 voxels wide.
 *     No line of sight is tested.  With g = 0 the ball is c itself, which is known: the gain is 0.
 *   Utility.  utility(c) = gain(c) - hop_cost * hops(c), an int32.  The gain is at most 65536 (the box holds at most
 *     64 FH_REACH_MAX_WORDS voxels) and the hops are below 65536; with hop_cost <= FH_GAIN_MAX_HOP_COST, |utility| < 2^30.
 *   Poor.  A candidate in some level with gain(c) < min_gain is POOR and is never chosen.
 *   Choice.  Of the candidates in some level that are not poor the one with the largest utility; among equals the smallest
 *     (hops, d2, c), lexicographic: a total order.
 *   Reduction.  With gain_radius = 0, hop_cost = 1 and min_gain = 0 every gain is 0, nothing is poor and the utility is -hops: the
 *     choice, d_goals, d_mask and the first 40 bytes of every record are those of fh_reach_goals_device exactly.
 *   Outputs.  Every byte of all three is written by every call.  d_mask and d_goals as in fasterhip_reach.h.  d_records[i]: the first
 *     40 bytes are fh_reach_record's (flags, view, cell, hops, candidates, reachable, reached, levels, d2), with cell, hops and d2 of
 *     this choice; gain and utility of the choice, -1 and 0 without one; poor = the number of poor candidates; best_gain = the
 *     largest gain over all candidates in some level, poor ones included, -1 if there are none; reserved = 0.  flags has
 *     FH_GAIN_ALL_POOR iff reachable > 0 and every reachable candidate is poor.  A vehicle that is not searched has
 *     gain = best_gain = -1, utility = poor = 0, and the rest as in fasterhip_reach.h.
 *
 * KNOWN LIMITS.  No occlusion: an unknown voxel behind a wall counts like one in the open.  The ball is clipped to the box, so gains
 * near the box's faces are under-counted.  The claims of peers (the chooser for a team, which keeps teammates off each other's voxels) are not honoured:
 * composing the two is a later change.  Hops are still Manhattan steps, not metres.  The limits of fasterhip_reach.h on the flood hold as there. */
#ifndef FASTERHIP_GAIN_H
#define FASTERHIP_GAIN_H
#include "fasterhip.h"
#include "fasterhip_frontier.h"
#include "fasterhip_reach.h"
#ifdef __cplusplus
extern "C" {
#endif

enum {
  FH_GAIN_MAX_RADIUS = 31,      /* gain_radius: a row of the ball is at most 63 voxels, which lie in at most two words of 64          */
  FH_GAIN_MAX_HOP_COST = 16384, /* hop_cost: |utility| < 2^30                                                                         */
  FH_GAIN_ALL_POOR = 128        /* fh_gain_record.flags, beside FH_FRONTIER_* and FH_REACH_*: candidates were reached, all of them poor */
};

typedef struct fh_gain_params { /* 64 B: fh_reach_params with three of its reserved words in use */
  double r_max;     /* as fh_reach_params                                                                                            */
  double r_avoid;
  double z_lo;
  double z_hi;
  int32_t want;
  int32_t max_hops;
  int32_t gain_radius; /* g, in voxels of the views' lattice: 0 .. FH_GAIN_MAX_RADIUS                                                */
  int32_t hop_cost;    /* unknown voxels that one step of the flood is worth: 0 .. FH_GAIN_MAX_HOP_COST                              */
  int32_t min_gain;    /* a candidate with a smaller gain is poor; >= 0                                                              */
  int32_t reserved[3];
} fh_gain_params;

typedef struct fh_gain_record { /* 64 B: the first 40 bytes are those of fh_reach_record */
  int32_t flags;      /* those of fh_reach_record | FH_GAIN_ALL_POOR                                                                 */
  int32_t view;
  int32_t cell;       /* the chosen cell of the lattice, -1: none                                                                    */
  int32_t hops;       /* its level, -1: none                                                                                         */
  int32_t candidates;
  int32_t reachable;
  int32_t reached;
  int32_t levels;
  double d2;          /* of the chosen cell, +inf: none                                                                              */
  int32_t gain;       /* of the chosen cell, -1: none                                                                                */
  int32_t utility;    /* of the chosen cell, 0: none                                                                                 */
  int32_t poor;       /* candidates in some level with a gain below min_gain                                                         */
  int32_t best_gain;  /* the largest gain of a candidate in some level, poor ones included; -1: no candidate in any level            */
  double reserved;    /* 0                                                                                                           */
} fh_gain_record;

/* The arguments of fh_reach_goals_device, with d_records [n] fh_gain_record.  One launch on `stream` (a hipStream_t, NULL: the default
 * stream), asynchronous, on the device that owns d_records: one workgroup of 256 per vehicle.  A vehicle that is not searched costs its
 * three outputs.  Reads nothing it writes; DETERMINISTIC: integer counts and the extremum of a total order.
 * FH_ERR_ARG, checked in this order, all before the first call of the runtime: par == NULL; r_max NaN, infinite or <= 0; r_avoid NaN,
 * infinite or negative; z_lo or z_hi NaN, or z_lo > z_hi; want == 0 or a bit above 4; max_hops < 0; gain_radius < 0 or
 * > FH_GAIN_MAX_RADIUS; hop_cost < 0 or > FH_GAIN_MAX_HOP_COST; min_gain < 0; map_grid null, res not > 0 or a dimension < 1; more than
 * 2^31 - 1 map cells; d_map_bits null; grid null, res not > 0, or a dimension < 1; more than 2^31 - 1 cells; view_stride < cells;
 * n_views < 1; n < 0.  Then FH_OK for n == 0, then FH_ERR_ARG for a null d_flags, d_vehicles, d_goals, d_mask or d_records.  d_view_of
 * may be NULL.  FH_ERR_DEVICE: d_records is no device memory, or the launch failed.  Every index the kernel uses comes from a value it
 * has checked. */
int fh_gain_goals_device(void* stream, const fh_gain_params* par, const struct fh_voxel_grid* map_grid, const unsigned* d_map_bits,
                         const struct fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of,
                         int n_views, const fh_vehicle* d_vehicles, int n, double* d_goals, int32_t* d_mask, fh_gain_record* d_records);

#ifdef __cplusplus
}
#endif
#endif /* FASTERHIP_GAIN_H */

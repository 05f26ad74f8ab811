/* fasterhip_sight.h: FRONTIER GOALS CHOSEN BY WHAT THEY WOULD SEE.  The chooser by gain (K17) weighs a frontier voxel
 * by the unknown voxels in a ball around it, and counts an unknown voxel behind a wall like one in the open.  The fleet's own sensor
 * (fh_fleet_sense_device) does not: a ray stops at the first occupied map cell.  A candidate beside a wall the vehicle already knows,
 * with an unexplored hall on the other side, is promised the hall, flies there, uncovers nothing and is sent on.  The entry point of
 * this header has that chooser's arguments and outputs and counts an unknown voxel only if a straight line of voxels from the
 * candidate to it crosses no voxel that the vehicle knows to be occupied: the ordinary next-best-view rule.
 *     utility(c) = (unknown voxels in a ball around c that c can see) - hop_cost * hops(c).
 * A closed period is
 *     sense -> observe -> [link] -> SIGHT GOALS -> fh_fleet_set_goals_device -> replan -> next goals
 * It is a pure measurement: no entry point, struct or kernel of any other header changes and FH_ABI_VERSION stays.  It takes the map's
 * lattice and bits as arguments and a stream; no handle is needed.
 * C99 / C++11, includes fasterhip.h, fasterhip_frontier.h and fasterhip_reach.h (FH_FRONTIER_WANT_*, FH_REACH_MAX_WORDS and the record
 * flags of those headers are reused).  The constants it shares with K17 are carried under its own names.
 *
 * THE MODEL (tests/sight_model.py restates it in Python, and the kernel is compared with that in every byte).  It is K17's model word
 * for word except where stated.  IEEE double for what fasterhip_reach.h computes, no fused multiply-add, comparisons as written;
 * everything this header adds is integer arithmetic.
 *   Views, wanted, eligible, start cell, box, box cap (FH_REACH_MAX_WORDS), searched, passable, flood (six neighbours, max_hops),
 *     candidate, hops(c) = the level of c.  As in fasterhip_reach.h, unchanged.
 *   Unknown.  A voxel u of the box is UNKNOWN iff F[u] != 0, whatever its map bit.  Voxels outside the box are never counted.
 *   Ball.  The voxels u of the box with (ux - cx)^2 + (uy - cy)^2 + (uz - cz)^2 <= g^2, g = gain_radius, in voxel units.
 *   Wall.  A voxel of the box is a WALL iff F[u] == 0 and it is not passable: it is known, and its map cell lies outside the map or has
 *     its bit set.  An unknown voxel is never a wall, whatever its map bit: the vehicle does not know what is there, and sight passes
 *     through unknown space.  That is the optimistic reading, and the only one the vehicle's knowledge supports.
 *   Line.  For a candidate c and a voxel u of the box, d = u - c and m = max(|dx|, |dy|, |dz|).  For k = 1 .. m - 1 the line voxel is
 *     l_k = c + (r(dx, k), r(dy, k), r(dz, k)),  r(a, k) = sgn(a) * floor((2 |a| k + m) / (2 m)):
 *     sign and magnitude, a half rounds away from c.  |r(a, k)| <= |a|, so every l_k lies in the box (c and u do) and in the ball.
 *   Visible.  u is VISIBLE from c iff no l_k is a wall.  c and u themselves are not tested: with m <= 1 u is visible.
 *   Gain.  gain(c) = the unknown voxels of the box in the ball of c that are visible from c.  ball_gain(c) = the unknown voxels of the
 *     box in the ball, K17's count.  If the ball of c holds no wall, gain(c) = ball_gain(c).  With g = 0 both are 0.
 *   Utility, poor, best_gain, choice, ALL_POOR.  K17's, on this gain: utility(c) = gain(c) - hop_cost * hops(c), an int32; a candidate
 *     in some level with gain(c) < min_gain is POOR and is never chosen; of the others the one with the largest utility, among equals
 *     the smallest (hops, d2, c), lexicographic: a total order.
 *   Reductions.  (A) For a searched vehicle whose box holds no wall the goal, the mask and bytes 0 .. 55 of the record are K17's, and
 *     ball_gain == gain.  (B) With gain_radius = 0, hop_cost = 1 and min_gain = 0 the choice, d_goals, d_mask and the first 40 bytes of
 *     every record are those of fh_reach_goals_device exactly.
 *   Outputs.  Every byte of all three is written by every call.  d_mask and d_goals as in fasterhip_reach.h.  d_records[i]: the first
 *     40 bytes are fh_reach_record's with cell, hops and d2 of this choice; gain and utility of the choice, -1 and 0 without one;
 *     poor = the number of poor candidates; best_gain = the largest gain over all candidates in some level, poor ones included, -1 if
 *     there are none; ball_gain = ball_gain(c) of the choice, -1 without one; walls = the wall voxels of the box.  flags has
 *     FH_SIGHT_ALL_POOR iff reachable > 0 and every reachable candidate is poor.  A vehicle that is not searched has
 *     gain = best_gain = ball_gain = -1, utility = poor = walls = 0, and the rest as in fasterhip_reach.h.
 *
 * KNOWN LIMITS.  A wall one voxel thick that runs diagonally lets a line slip through: the line's voxels are 26-connected.  The map's
 * bits are inflated, so sight is blocked a little early.  Ball and lines stop at the box, so gains near its faces are under-counted.
 * There is no field of view: the ball is a full sphere.  The chooser for a team still counts through walls: composing the two is a
 * later change.  Hops are Manhattan steps, not metres, and the limits of fasterhip_reach.h on the flood hold as there. */
#ifndef FASTERHIP_SIGHT_H
#define FASTERHIP_SIGHT_H
#include "fasterhip.h"
#include "fasterhip_frontier.h"
#include "fasterhip_reach.h"
#ifdef __cplusplus
extern "C" {
#endif

enum {
  FH_SIGHT_MAX_RADIUS = 31,      /* gain_radius: a row of the ball is at most 63 voxels, which lie in at most two words of 64           */
  FH_SIGHT_MAX_HOP_COST = 16384, /* hop_cost: |utility| < 2^30                                                                          */
  FH_SIGHT_ALL_POOR = 128        /* fh_sight_record.flags, beside FH_FRONTIER_* and FH_REACH_*: candidates were reached, all of them poor */
};

typedef struct fh_sight_params { /* 64 B: K17's params, field by field */
  double r_max;     /* as fh_reach_params                                                                                            */
  double r_avoid;
  double z_lo;
  double z_hi;
  int32_t want;
  int32_t max_hops;
  int32_t gain_radius; /* g, in voxels of the views' lattice: 0 .. FH_SIGHT_MAX_RADIUS                                               */
  int32_t hop_cost;    /* unknown voxels that one step of the flood is worth: 0 .. FH_SIGHT_MAX_HOP_COST                             */
  int32_t min_gain;    /* a candidate that sees fewer unknown voxels is poor; >= 0                                                   */
  int32_t reserved[3];
} fh_sight_params;

typedef struct fh_sight_record { /* 64 B: the first 40 bytes are those of fh_reach_record, the first 56 those of K17's record */
  int32_t flags;      /* those of fh_reach_record | FH_SIGHT_ALL_POOR                                                                */
  int32_t view;
  int32_t cell;       /* the chosen cell of the lattice, -1: none                                                                    */
  int32_t hops;       /* its level, -1: none                                                                                         */
  int32_t candidates;
  int32_t reachable;
  int32_t reached;
  int32_t levels;
  double d2;          /* of the chosen cell, +inf: none                                                                              */
  int32_t gain;       /* the unknown voxels the chosen cell sees, -1: none                                                           */
  int32_t utility;    /* of the chosen cell, 0: none                                                                                 */
  int32_t poor;       /* candidates in some level with a gain below min_gain                                                         */
  int32_t best_gain;  /* the largest gain of a candidate in some level, poor ones included; -1: no candidate in any level            */
  int32_t ball_gain;  /* the unknown voxels in the ball of the chosen cell, seen or not; -1: none                                    */
  int32_t walls;      /* the wall voxels of the box; 0: not searched                                                                 */
} fh_sight_record;

/* The arguments of fh_reach_goals_device, with d_records [n] fh_sight_record.  One launch on `stream` (a hipStream_t, NULL: the default
 * stream), asynchronous, on the device that owns d_records: one workgroup of 256 per vehicle.  A vehicle that is not searched costs its
 * three outputs; a candidate whose ball holds no wall costs two sweeps over the rows of its ball, and one that does a walk of at most
 * g - 1 voxels for every unknown voxel of its ball.  Reads nothing it writes; DETERMINISTIC: integer counts and the extremum of a
 * total order.
 * FH_ERR_ARG, checked in this order, all before the first call of the runtime: par == NULL; r_max NaN, infinite or <= 0; r_avoid NaN,
 * infinite or negative; z_lo or z_hi NaN, or z_lo > z_hi; want == 0 or a bit above 4; max_hops < 0; gain_radius < 0 or
 * > FH_SIGHT_MAX_RADIUS; hop_cost < 0 or > FH_SIGHT_MAX_HOP_COST; min_gain < 0; map_grid null, res not > 0 or a dimension < 1; more
 * than 2^31 - 1 map cells; d_map_bits null; grid null, res not > 0, or a dimension < 1; more than 2^31 - 1 cells; view_stride < cells;
 * n_views < 1; n < 0.  Then FH_OK for n == 0, then FH_ERR_ARG for a null d_flags, d_vehicles, d_goals, d_mask or d_records.  d_view_of
 * may be NULL.  FH_ERR_DEVICE: d_records is no device memory, or the launch failed.  Every index the kernel uses comes from a value it
 * has checked. */
int fh_sight_goals_device(void* stream, const fh_sight_params* par, const struct fh_voxel_grid* map_grid, const unsigned* d_map_bits,
                          const struct fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of,
                          int n_views, const fh_vehicle* d_vehicles, int n, double* d_goals, int32_t* d_mask, fh_sight_record* d_records);

#ifdef __cplusplus
}
#endif
#endif /* FASTERHIP_SIGHT_H */

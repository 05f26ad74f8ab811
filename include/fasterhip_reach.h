/* fasterhip_reach.h: FRONTIER GOALS A VEHICLE CAN REACH, BY A FLOOD OF ITS VIEW.  fh_map_frontier_goals_device
 * (include/fasterhip_frontier.h) gives a vehicle the frontier voxel with the smallest straight-line distance.  A frontier voxel behind a
 * wall, or inside a pocket that occupied cells seal, wins there over every voxel the vehicle could fly to; the path search then answers
 * NO_PATH, r_avoid excludes that one voxel, and the next period picks its neighbour.  The entry point of this header has the same
 * outputs and a richer record, and chooses by the connectivity of the space the vehicle knows to be free: a breadth-first flood from
 * the voxel the vehicle stands in, over the bounding box of its sphere, and of the candidates the flood reaches the one with the fewest
 * steps.  A closed period is
 *     sense -> observe -> [link] -> REACH GOALS -> fh_fleet_set_goals_device -> replan -> next goals
 * It is a pure measurement: no entry point, struct or kernel of fasterhip.h or fasterhip_frontier.h changes and FH_ABI_VERSION stays.
 * It takes the map's lattice and bits as arguments (fh_map_dims, fh_map_occupancy_bits_device) and a stream; no handle is needed.
 * C99 / C++11, includes fasterhip.h and fasterhip_frontier.h (FH_FRONTIER_WANT_* and the record flags of that header are reused).
 *
 * THE MODEL (tests/reach_model.py restates it in Python, a queue over voxels, and the kernel is compared with that in every byte).  It
 * is the model of fasterhip_frontier.h word for word except where stated.  IEEE double, no fused multiply-add, comparisons as written.
 *   Views, wanted.  As there: view(i) = d_view_of ? d_view_of[i] : i, the flags F of view v at d_flags + v * view_stride on the lattice
 *     (origin, res, dims) of `grid`, cell c = (iz ny + iy) nx + ix; wanted by the bits of par->want; FH_FRONTIER_NO_VIEW and
 *     FH_FRONTIER_BAD_POS judged as there.  A vehicle that header would search (wanted, a view, six finite coordinates) is ELIGIBLE.
 *   Start cell.  s = floor((p - origin) / res), per axis, p = state.pos.  An eligible vehicle whose s lies outside the lattice is not
 *     searched and gets FH_REACH_START_OUTSIDE (the bit is judged for eligible vehicles only).
 *   Box.  Per axis lo = floor((p - r_max - origin) / res) - 1 and hi = floor((p + r_max - origin) / res) + 1, clipped to the lattice:
 *     the box that header's kernel scans.  With s inside the lattice the box is not empty and holds s.  The box is the domain of the
 *     flood.  Let wx = ceil((hi.x - lo.x + 1) / 64), rows_y = hi.y - lo.y + 1, rows_z = hi.z - lo.z + 1.
 *   Box cap.  An eligible vehicle with s inside and wx rows_y rows_z > FH_REACH_MAX_WORDS is not searched and gets
 *     FH_REACH_BOX_TOO_LARGE.  1024 words of 64 voxels hold the 63 x 63 x 15 box of a vehicle with r_max = 6 on a lattice of 0.2 (945).
 *   Searched.  Eligible, s inside, box within the cap.
 *   Passable.  A voxel of the box is passable iff its flag is 0 and the map cell floor((q - origin_map) / res_map), per axis, of its
 *     centre q = (ix + 0.5) res + origin lies inside the map with its bit clear (that header's expression).  z_lo / z_hi do not enter:
 *     the map's own z_ground / z_max already do.
 *   Flood.  Level 0 = {s}, whatever the flag and the map bit of s are: the vehicle is there, possibly inside an inflated cell.
 *     Level k + 1 = the passable voxels of the box that are in no earlier level and have a face neighbour (six neighbours, inside the
 *     box) in level k.  The flood ends when a level is empty, or after level max_hops if max_hops > 0.  hops(c) = the level of c.  Six
 *     neighbours on purpose: such a route is also a route of the 26-connected path search, so a voxel the flood reaches has a voxel path.
 *   Candidate.  That header's candidate exactly: F[c] == 0 with an unknown face neighbour inside the LATTICE, z_lo <= q.z <= z_hi,
 *     d2 < r_max r_max, not e2 < r_avoid r_avoid, map cell inside and clear.  (Every candidate lies in the box and is passable.)
 *   Choice.  Of the candidates that are in some level the one with the smallest (hops, d2, c), lexicographic: a total order.
 *   Outputs.  Every byte of all three is written by every call.  d_mask[i] = 1 iff a candidate was chosen; d_goals[3 i ..] = q of the
 *     choice, else the bits of g_term.  d_records[i]: flags = FH_FRONTIER_WANTED | NO_VIEW | BAD_POS as in that header |
 *     FH_REACH_START_OUTSIDE | FH_REACH_BOX_TOO_LARGE | FH_FRONTIER_FOUND if a candidate was chosen | FH_REACH_CUT if max_hops > 0 and
 *     level max_hops is not empty (the flood stopped there); view as read; cell and hops of the choice, -1 without one; candidates =
 *     the number of candidates, reachable or not, that header's count; reachable = the candidates in some level; reached = the voxels
 *     in some level, s included; levels = the index of the last level that is not empty; d2 of the choice, +inf without one;
 *     reserved = 0.  A vehicle that is not searched has cell = hops = -1, candidates = reachable = reached = levels = 0, d2 = +inf.
 *
 * KNOWN LIMITS.  Voxels beyond the box are not flooded: a route that leaves the box and comes back is not found.  Unknown voxels are
 * never passable, the conservative reading; the whole-trajectory planner is more optimistic.  Two vehicles with equal views that stand
 * close together still choose the same voxel.  Hops are Manhattan steps, not metres: of two candidates the one with fewer steps wins,
 * whatever their distances. */
#ifndef FASTERHIP_REACH_H
#define FASTERHIP_REACH_H
#include "fasterhip.h"
#include "fasterhip_frontier.h"
#ifdef __cplusplus
extern "C" {
#endif

enum {
  FH_REACH_START_OUTSIDE = 16, /* fh_reach_record.flags, beside FH_FRONTIER_WANTED .. BAD_POS: s outside the lattice, nothing searched  */
  FH_REACH_BOX_TOO_LARGE = 32, /*                          the box needs more than FH_REACH_MAX_WORDS words: nothing searched           */
  FH_REACH_CUT = 64            /*                          the flood stopped at max_hops with a last level that is not empty            */
};
enum { FH_REACH_MAX_WORDS = 1024 }; /* words of 64 voxels (a row of x begins a word) that the box of a vehicle may need                 */

typedef struct fh_reach_params { /* 64 B: fh_frontier_params with max_hops in its first reserved word */
  double r_max;     /* candidates: d2 < r_max * r_max (strict); the box                                                              */
  double r_avoid;   /* no candidate with e2 < r_avoid * r_avoid around g_term; 0: off                                                */
  double z_lo;      /* candidates: z_lo <= q.z <= z_hi                                                                               */
  double z_hi;
  int32_t want;     /* FH_FRONTIER_WANT_*, a bit set                                                                                 */
  int32_t max_hops; /* the last level of the flood; 0: no limit                                                                      */
  int32_t reserved[6];
} fh_reach_params;

typedef struct fh_reach_record { /* 48 B */
  int32_t flags;      /* FH_FRONTIER_WANTED | FOUND | NO_VIEW | BAD_POS | FH_REACH_START_OUTSIDE | BOX_TOO_LARGE | CUT               */
  int32_t view;       /* view(i) as read                                                                                             */
  int32_t cell;       /* the chosen cell of the lattice, -1: none                                                                    */
  int32_t hops;       /* its level, -1: none                                                                                         */
  int32_t candidates; /* how many candidates the vehicle had, reachable or not: the count of fh_frontier_record                      */
  int32_t reachable;  /* how many of them are in some level                                                                          */
  int32_t reached;    /* voxels in some level, the start included                                                                    */
  int32_t levels;     /* the index of the last level that is not empty (0: only the start); 0 when not searched                      */
  double d2;          /* of the chosen cell, +inf: none                                                                              */
  double reserved;    /* 0                                                                                                           */
} fh_reach_record;

/* d_mask [n] int32, d_goals [n][3] and d_records [n] as above, in the shape fh_fleet_set_goals_device takes.  map_grid and d_map_bits:
 * the lattice (fh_map_dims, and the res of fh_map_occupancy_bits_device) and the bits (fh_map_occupancy_bits_device) of a map that has
 * been filled on `stream`, one bit per cell, cell (x, y, z) = bit ((z my + y) mx + x) & 31 of word ((z my + y) mx + x) >> 5.  One launch
 * on `stream` (a hipStream_t, NULL: the default stream), asynchronous, on the device that owns d_records: one workgroup of 256 per
 * vehicle.  A vehicle that is not searched costs its three outputs.  Reads nothing it writes; DETERMINISTIC: integer counts and the
 * minimum of a total order.
 * FH_ERR_ARG, checked in this order, all before the first call of the runtime: par == NULL; r_max NaN, infinite or <= 0; r_avoid NaN,
 * infinite or negative; z_lo or z_hi NaN, or z_lo > z_hi; want == 0 or a bit above 4; max_hops < 0; map_grid null, res not > 0 or a
 * dimension < 1; more than 2^31 - 1 map cells; d_map_bits null; grid null, res not > 0, or a dimension < 1; more than 2^31 - 1 cells;
 * view_stride < cells; n_views < 1; n < 0.  Then FH_OK for n == 0, then FH_ERR_ARG for a null d_flags, d_vehicles, d_goals, d_mask or
 * d_records.  d_view_of may be NULL.  FH_ERR_DEVICE: d_records is no device memory, or the launch failed.  Every index the kernel uses
 * comes from a value it has checked. */
int fh_reach_goals_device(void* stream, const fh_reach_params* par, const struct fh_voxel_grid* map_grid, const unsigned* d_map_bits,
                          const struct fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of,
                          int n_views, const fh_vehicle* d_vehicles, int n, double* d_goals, int32_t* d_mask, fh_reach_record* d_records);

#ifdef __cplusplus
}
#endif
#endif /* FASTERHIP_REACH_H */

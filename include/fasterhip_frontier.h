/* fasterhip_frontier.h: ARRIVED VEHICLES TAKE THE NEAREST FRONTIER OF THEIR VIEW AS GOAL.  A fleet (include/fasterhip.h) gives every
 * vehicle a view of unknown voxels that fh_fleet_sense_device grows, a row of point masks that fh_fleet_observe_device grows
 * (include/fasterhip_occupancy.h), and pools both between vehicles in radio range (include/fasterhip_link.h).  Where to fly was still the
 * host's business: a vehicle that had arrived sat in GOAL_REACHED until somebody read its view back, looked for unexplored space and
 * uploaded a goal with fh_fleet_set_goals_device.  Two entry points on fh_map: one chooses, per vehicle, the nearest voxel of its view
 * that is known, free, and next to unknown space, in exactly the shape fh_fleet_set_goals_device takes; one counts what every view knows,
 * so that a loop can tell when it is done.  A closed period is
 *     sense -> observe -> [link] -> FRONTIER GOALS -> fh_fleet_set_goals_device -> replan -> next goals
 * with no host data in it.  Both are pure measurements: no entry point, struct or kernel of fasterhip.h changes and FH_ABI_VERSION stays.
 * They live on fh_map because the map owns the occupancy bits, their lattice and a stream; nothing of fh_ctx is needed.  C99 / C++11,
 * includes fasterhip.h.
 *
 * THE MODEL (tests/frontier_model.py restates it in numpy, brute force, and the kernels are compared with that in every byte).
 * Everything is IEEE double, no fused multiply-add, every comparison as written here.
 *   Views.  view(i) = d_view_of ? d_view_of[i] : i, as everywhere else.  View v has the flags F = d_flags + v * view_stride on the
 *     lattice (origin, res, dims) of `grid`; cell c = (iz ny + iy) nx + ix, cells = nx ny nz.  Bytes between cells and view_stride are
 *     never read.
 *   Frontier voxel.  c is a frontier voxel of v iff F[c] == 0 and at least one of its six face neighbours INSIDE THE LATTICE has
 *     F != 0.  A neighbour outside the lattice is not unknown, and the byte after the end of a row of x is not a neighbour.
 *   Candidate.  With p = d_vehicles[i].state.pos, g = d_vehicles[i].g_term and q = ((ix + 0.5) res + origin), per axis, the centre
 *     of the voxel (the expression of the sense model), a frontier voxel of view(i) is a candidate of vehicle i iff all of
 *       z_lo <= q.z <= z_hi                                  (both inclusive; infinite bounds are allowed);
 *       d2 < r_max * r_max                                   (strict), d2 = dx dx + dy dy + dz dz, d = q - p, the three products summed
 *                                                            x, y, z from left to right; r_max * r_max is rounded once;
 *       not (e2 < r_avoid * r_avoid)                         e = q - g, e2 summed the same way; r_avoid = 0 switches the rule off.  It
 *                                                            keeps a vehicle from choosing the neighbourhood of the goal it already has
 *                                                            or could not reach;
 *       the map cell floor((q - origin_map) / res_map), per axis, lies inside the map and its occupancy bit is clear.  The map is the
 *                                                            inflated grid of fh_map_read_device.  A centre outside the map is not a
 *                                                            candidate: nothing can be planned there.  A known voxel has been seen, so
 *                                                            its occupancy is known to the vehicle: this is the sensor's model.
 *   Wanted.  Vehicle i is wanted iff a set bit of par->want matches: FH_FRONTIER_WANT_REACHED its status == FH_VEHICLE_GOAL_REACHED,
 *     FH_FRONTIER_WANT_NO_PATH its stage == FH_FLEET_STAGE_NO_PATH, FH_FRONTIER_WANT_ALL always.
 *   Searched.  Vehicle i is searched iff it is wanted, 0 <= view(i) < n_views, and all six coordinates of p and g are finite.
 *   Choice.  The chosen candidate of a searched vehicle has the smallest (d2, c), lexicographic: a total order, so the result does not
 *     depend on scheduling.
 *   Outputs.  Every byte of all three is written by every call.
 *     d_mask[i] = 1 if a candidate was chosen, else 0.
 *     d_goals[3 i ..] = q of the chosen voxel, or the bits of g_term when nothing was chosen.
 *     d_records[i]: flags = FH_FRONTIER_WANTED if wanted | FH_FRONTIER_NO_VIEW if view(i) is outside [0, n_views) | FH_FRONTIER_BAD_POS
 *       if a coordinate of p or g is not finite (the three are judged independently) | FH_FRONTIER_FOUND if a candidate was chosen;
 *       view = view(i) as read; cell = c of the choice, -1 without one; candidates = the exact number of candidates (0 when not
 *       searched); d2 of the choice, +inf without one; reserved = 0.
 *
 * KNOWN LIMITS.  Two vehicles with equal views that stand close together choose the same voxel: nothing spreads a team over its
 * frontiers.  The straight-line distance decides, not the length of a path.  A vehicle wanted for NO_PATH may alternate between two
 * frontiers it cannot reach: r_avoid excludes only the last one.  Nothing is searched beyond r_max: a vehicle whose frontiers all lie
 * farther away stays where it is, and its record says candidates = 0. */
#ifndef FASTERHIP_FRONTIER_H
#define FASTERHIP_FRONTIER_H
#include "fasterhip.h"
#ifdef __cplusplus
extern "C" {
#endif

enum {
  FH_FRONTIER_WANT_REACHED = 1, /* fh_frontier_params.want: vehicles with status FH_VEHICLE_GOAL_REACHED                               */
  FH_FRONTIER_WANT_NO_PATH = 2, /*                          vehicles whose last replan ended in FH_FLEET_STAGE_NO_PATH                 */
  FH_FRONTIER_WANT_ALL = 4      /*                          every vehicle                                                              */
};
enum {
  FH_FRONTIER_WANTED = 1,  /* fh_frontier_record.flags: a bit of `want` matched                                                       */
  FH_FRONTIER_FOUND = 2,   /*                           a candidate was chosen: d_mask[i] = 1, d_goals[i] = its centre                */
  FH_FRONTIER_NO_VIEW = 4, /*                           view(i) outside [0, n_views): nothing searched                                */
  FH_FRONTIER_BAD_POS = 8  /*                           a coordinate of state.pos or g_term not finite: nothing searched              */
};

typedef struct fh_frontier_params { /* 64 B */
  double r_max;   /* candidates: d2 < r_max * r_max (strict)                                                                         */
  double r_avoid; /* no candidate with e2 < r_avoid * r_avoid around g_term; 0: off                                                  */
  double z_lo;    /* candidates: z_lo <= q.z <= z_hi                                                                                 */
  double z_hi;
  int32_t want;   /* FH_FRONTIER_WANT_*, a bit set                                                                                   */
  int32_t reserved[7];
} fh_frontier_params;

typedef struct fh_frontier_record { /* 32 B */
  int32_t flags;      /* FH_FRONTIER_WANTED | FOUND | NO_VIEW | BAD_POS                                                              */
  int32_t view;       /* view(i) as read                                                                                             */
  int32_t cell;       /* the chosen cell of the lattice, -1: none                                                                    */
  int32_t candidates; /* how many candidates the vehicle had, exact                                                                  */
  double d2;          /* of the chosen cell, +inf: none                                                                              */
  double reserved;    /* 0                                                                                                           */
} fh_frontier_record;

typedef struct fh_view_coverage { /* 16 B */
  int64_t known;    /* voxels with flag 0                                                                                            */
  int64_t frontier; /* frontier voxels: flags alone, no map, range or z test                                                         */
} fh_view_coverage;

/* d_mask [n] int32, d_goals [n][3] and d_records [n] as above: a pure measurement of the views, the vehicles and the map, in the
 * shape fh_fleet_set_goals_device takes (d_new_goals, d_mask); applying the goals is that call.  One launch on the map's stream,
 * asynchronous: one workgroup of 256 per vehicle.  A vehicle that is not searched costs its three outputs; a searched one scans the
 * bounding box of its sphere, clipped to the lattice, and loads the six neighbour bytes only of voxels that are known.  The map must
 * have been filled on the same stream (faster_amd.fleet.Fleet sets both to one stream).  Reads nothing it writes; DETERMINISTIC: the
 * minimum of a total order and an integer count.
 * FH_ERR_ARG, checked in this order: a null map; a map that has never been read (fh_map_read_device); par == NULL; r_max NaN,
 * infinite or <= 0; r_avoid NaN, infinite or negative; z_lo or z_hi NaN, or z_lo > z_hi; want == 0 or a bit above 4; grid null, res
 * not > 0, or a dimension < 1; more than 2^31 - 1 cells (computed in 64 bits); view_stride < cells; n_views < 1; n < 0.  Then FH_OK
 * for n == 0, then FH_ERR_ARG for a null d_flags, d_vehicles, d_goals, d_mask or d_records.  d_view_of may be NULL.  Every index the
 * kernel uses comes from a value it has checked. */
int fh_map_frontier_goals_device(fh_map* map, const fh_frontier_params* par, const struct fh_voxel_grid* grid, const unsigned char* d_flags,
                                 size_t view_stride, const int32_t* d_view_of, int n_views, const fh_vehicle* d_vehicles, int n,
                                 double* d_goals, int32_t* d_mask, fh_frontier_record* d_records);

/* d_out[v] = (known, frontier) of view v, v < n_views: the voxels with flag 0, and the frontier voxels above.  Only the dims of `grid`
 * are read.  A memset and one launch on the map's stream, asynchronous; integer sums only (a count per wavefront, one integer atomic
 * add per workgroup), so the bytes do not depend on scheduling.  The map need not have been read.
 * FH_ERR_ARG in this order: a null map; grid null or a dimension < 1; more than 2^31 - 1 cells; view_stride < cells; n_views < 1;
 * then a null d_flags or d_out. */
int fh_map_view_coverage_device(fh_map* map, const struct fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride,
                                int n_views, fh_view_coverage* d_out /* [n_views] */);

#ifdef __cplusplus
}
#endif
#endif /* FASTERHIP_FRONTIER_H */

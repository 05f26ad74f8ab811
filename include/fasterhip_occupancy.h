/* fasterhip_occupancy.h: occupied space per vehicle or team for the fleet of include/fasterhip.h, as masks over the points of the
 * shared cloud, grown on the device by observing.  The model, the memory per view and the limits are stated in fasterhip.h (the
 * occupancy block after the heading entry points); this header declares the entry points.  C99 / C++11, includes fasterhip.h. */
#ifndef FASTERHIP_OCCUPANCY_H
#define FASTERHIP_OCCUPANCY_H
#include "fasterhip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* n_views inflated occupancy grids on one lattice: the lattice and the inflation arithmetic of fh_map_read_device with the same
 * arguments; cloud point k marks the grid of view v only if its bit is set in row v.  Bits are only ORed: the result does not depend on
 * scheduling.  With a mask of all ones every grid equals the one fh_map_read_device builds, bit for bit.  The grids belong to the map
 * and are rebuilt by every call; the map of fh_map_read_device is not touched.  Asynchronous on the map's stream. */
int fh_map_read_views_device(fh_map* map, const double* d_cloud_xyz, int n_cloud, const uint32_t* d_point_mask, int mask_words, int n_views,
                             const int32_t cells[3], double res, const double center[3], double z_ground, double z_max, double inflation);
/* The grid of one view on the host, as fh_map_occupancy gives the map's: [nz][ny][nx], 0 free / 100 occupied (synchronises). */
int fh_map_view_occupancy(fh_map* map, int view, int8_t* occ);
/* fh_map_plan_batch_radius_device in which query i reads the grid of view(i) (a view number outside [0, n_views): n_points = 0).  The
 * grids must be n_views grids on the lattice of the map (fh_map_read_views_device after fh_map_read_device, same arguments), else
 * FH_ERR_ARG.  Everything else, the search mode included, as fh_map_plan_batch_radius_device; that entry point is unchanged. */
int fh_map_plan_batch_radius_views_device(fh_map* map, const double* d_starts, const double* d_goals, const double* d_radius,
                                          const int32_t* d_active, int n, int max_points, double max_vertex_dist, int max_poly, double* d_paths,
                                          int32_t* d_n_points, int64_t* d_expansions, const int32_t* d_view_of, int n_views);
/* Attaches the masks to the context (d_point_mask NULL: detaches them), as fh_set_unknown_views_device attaches views.  While attached,
 * fh_corridor_batch_device and fh_safe_corridor_batch_device skip a cloud point whose bit is clear in the view of the query (the
 * decomposition works per segment: the view of segment / max_poly); list lengths, homes and caps count known points only, so a masked
 * run is the run on the compacted sub-cloud.  Both return FH_ERR_ARG when mask_words * 32 < n_cloud.  fh_decompose_batch* takes no
 * query and ignores the masks.  fh_solve_pairs_device refuses attached masks (FH_ERR_ARG); fh_pool_* has contexts of its own and no
 * call that attaches masks to them.  With nothing attached every entry point does exactly what it did before masks existed. */
int fh_set_point_views_device(fh_ctx* ctx, const uint32_t* d_point_mask, int mask_words, const int32_t* d_view_of, int n_views);
/* Observing: for every view v and every cloud point k, if the voxel of `grid` that contains point k is known in view v (flag byte 0 in
 * d_flags + v * view_stride), bit k of row v is set.  The voxel is floor((x - origin) / res) per axis, in double, no fused multiply-add.
 * A point outside the lattice, or a point that is not finite, is never observed.  Nothing is ever cleared and bits are ORed
 * atomically: knowledge only grows, and scheduling cannot show.  Rows belong to views, so d_view_of is not read (it is in the
 * signature for symmetry with fh_fleet_sense_device; pass what that call gets).  Limit of the model, next to the sensor's: a point is
 * observed through the voxel it lies in, and sensing never clears a voxel that lies in an occupied cell of the world map behind
 * another one.  With the world map inflated by more than a cell, a point in the interior of its own blob lies in such a voxel and is
 * never observed: the caller chooses the world inflation accordingly (one cell: every point's voxel can be seen from outside).
 * FH_ERR_ARG when n_views <= 0 or mask_words * 32 < n_cloud.  A word that is already full costs one read.  Asynchronous on the stream
 * of `ctx`. */
int fh_fleet_observe_device(fh_ctx* ctx, const struct fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride,
                            const int32_t* d_view_of, int n_views, const double* d_cloud_xyz, int n_cloud, uint32_t* d_point_mask,
                            int mask_words);

#ifdef __cplusplus
}
#endif
#endif /* FASTERHIP_OCCUPANCY_H */

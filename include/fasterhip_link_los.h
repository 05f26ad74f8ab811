/* fasterhip_link_los.h: WALLS BLOCK A RADIO LINK.  fasterhip_link.h lets the vehicles in radio range of each other pool what their views
 * know, and its labels are the teams of every team chooser; its first known limit was "walls do not block a link": two vehicles 4 m
 * apart on either side of a wall were one team from the first period.  The fleet's sensor already refuses to see through an occupied
 * cell of the map; this header gives the radio the same rule.  One entry point beside fh_fleet_link_groups_device: the same labels and
 * info, with one more condition on a linked pair, a line of sight through the map.  fh_link_params and fh_fleet_link_merge_device are
 * reused as they are; no entry point, struct or kernel of fasterhip.h or fasterhip_link.h changes and FH_ABI_VERSION stays.
 * C99 / C++11, includes fasterhip_link.h.
 *
 * THE MODEL is the model of fasterhip_link.h with a third condition on a linked pair.  Views, speaking, edges, labels and passes are
 * unchanged, and so are d_info[0] and d_info[1] and the independence from the cell grid and from FH_LINK_LIST.  Everything is IEEE
 * double, no fused multiply-add, every comparison strict, the operations in the order written here (tests/link_los_model.py restates it
 * in numpy, brute force over all pairs, and the kernels are compared with that in every byte).
 *   Pair orientation.  For a pair i != k that both speak: a = min(i, k), b = max(i, k), p = pos_a, q = pos_b, d = q - p per axis.  The
 *     same orientation whichever of the two asks, so the relation is symmetric by construction.  THE ORIENTATION IS PART OF THE MODEL:
 *     the samples below are not the samples of the ray from the other end (on the CPU about 8 % of random pairs on a 0.1 m grid against
 *     a 0.2 m map sample a different set of cells), and there are pairs for which that decides the answer (tests/test_link_los_model.py
 *     finds one by a seeded search).
 *   In range.  d2 = (dx dx + dy dy) + dz dz < range * range, as in fasterhip_link.h; range * range is rounded once.
 *   Blocked.  dist = sqrt(d2);  K = max(1, ceil(dist / (0.5 * res_map))), with 0.5 * res_map computed first.  For j = 1 .. K - 1:
 *     t = j / K, the sample is (p.x + dx t, p.y + dy t, p.z + dz t), and its cell is floor((x - origin_map) / res_map) per axis: the
 *     arithmetic of the sensor (fh_fleet_sense_device; tests/sense_model.py).  A sample whose cell is outside the map is free.  A sample
 *     whose cell equals the cell of p or the cell of q is not tested: the comparison is on the floored doubles, as the sensor compares
 *     them, also outside the map (a vehicle that stands inside an inflated cell must not lose every link).  The pair is blocked iff some
 *     tested sample lies in an occupied cell of `map`: cell (x, y, z) is bit (z my + y) mx + x of fh_map_occupancy_bits_device, the grid
 *     fh_map_occupancy returns.
 *   Linked.  A pair is linked iff both speak, it is in range, and it is not blocked.
 *   Info.  d_info[0], d_info[1] as in fasterhip_link.h; d_info[2] = the number of linked pairs i < k; d_info[3] = the number of pairs
 *     i < k that both speak, are in range and are blocked.  Both exact.  d_info[2] + d_info[3] is therefore what
 *     fh_fleet_link_groups_device reports in d_info[2] for the same inputs.
 *   Limits.  range / res_map <= 4096, the sensor's limit (a ray then has fewer than 8192 samples).  The map is only read; it must have
 *     been filled on the stream of `ctx` (or its fill waited for).
 * THREE CONSEQUENCES (tests/test_link_los_model.py, tests/test_gpu_link_los.py).  With a map that has no occupied cell, labels and
 * d_info[0 .. 2] equal fh_fleet_link_groups_device's byte for byte and d_info[3] = 0.  The linked pairs are a subset of the plain ones,
 * so every group of this entry point lies inside one plain group.  A blocked pair can still be in one group through a third vehicle that
 * sees both, a relay: the labels are those of connected components, as before.
 *
 * KNOWN LIMITS.  The map's bits are inflated, so a link is blocked a little early.  A diagonal wall one cell thick can be slipped by
 * half-cell steps.  No attenuation, no Fresnel zone, no latency.  Traffic (fasterhip_traffic.h) still shows every plan in range,
 * whoever is linked. */
#ifndef FASTERHIP_LINK_LOS_H
#define FASTERHIP_LINK_LOS_H
#include "fasterhip_link.h"
#ifdef __cplusplus
extern "C" {
#endif

/* fh_fleet_link_groups_device with THE MODEL above: d_labels[v] = the label of view v, d_info[0 .. 3].  A pure measurement of
 * d_vehicles, d_view_of and the map's occupancy.  Launches on the context's stream, asynchronous: the boxes, cell starts and cell items
 * of fh_fleet_link_groups_device, a narrow phase that casts the rays (one wavefront per vehicle: the rows of the views linked in line of
 * sight, the two pair counts), then per pass a hook that reads those rows (a vehicle with more such neighbours than FH_LINK_LIST walks
 * the cells again, with what the narrow phase found for each turn of the walk or, where that was not kept, with the same test) and the
 * jump of fh_fleet_link_groups_device.  DETERMINISTIC as that entry point is.
 * FH_ERR_ARG, checked in this order after a null context: the argument checks of fh_fleet_link_groups_device, in its order; then
 * map == NULL or a map that holds no grid (fh_map_read* first); then range / res_map > 4096.  Then FH_ERR_DEVICE without a device (there
 * is no CPU path); n == 0 and null pointers as in fh_fleet_link_groups_device (n == 0: labels = identity, info = (0, n_views, 0, 0)).
 * Every index the kernels use comes from a value they have checked: a sample outside the map reads nothing, and a position that is not
 * finite never reaches a ray. */
int fh_fleet_link_groups_los_device(fh_ctx* ctx, fh_map* map, const fh_link_params* par, const fh_vehicle* d_vehicles, int n,
                                    const int32_t* d_view_of, int n_views, const struct fh_voxel_grid* cells,
                                    int32_t* d_labels /* [n_views] */, int64_t* d_info /* [4] */);

#ifdef __cplusplus
}
#endif
#endif /* FASTERHIP_LINK_LOS_H */

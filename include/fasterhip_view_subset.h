/* fasterhip_view_subset.h: REBUILD AND TABLE ONLY THE VIEWS THAT SOMEBODY SEARCHES.  fh_map_read_views_device (fasterhip_occupancy.h)
 * clears and marks the grid of every view, and the next view search in jump-point mode rebuilds the jump tables of every view (64 bytes
 * per cell and view).  A fleet that replans in rounds (fasterhip_rounds.h) searches a handful of views in most rounds and pays for all of
 * them.  Two entry points on fh_map: one lists, on the device, the views that the active queries of a search need; one refreshes the
 * grids and, where they exist, the jump tables of the listed views and leaves every other view as it is.  Both are asynchronous on the
 * map's stream; the list and its count never visit the host.  A cycle becomes
 *     ... -> gate -> [traffic] -> VIEW LIST -> LISTED READ -> fh_map_plan_batch_radius_views_device -> ...
 * No entry point, struct or kernel of fasterhip.h or fasterhip_occupancy.h changes and FH_ABI_VERSION stays.  C99 / C++11, includes
 * fasterhip.h.
 *
 * THE LIST (tests/view_subset_model.py restates it in numpy; the device is compared with that in every byte).  Query q < n needs view
 *     v = d_view_of ? d_view_of[q] : q
 * iff (d_active == NULL or d_active[q] != 0) and 0 <= v < n_views: the conventions of fh_map_plan_batch_radius_views_device, where a
 * view number outside the range is "no path", not an error.  d_list[0 .. count) holds the needed views, each once, ascending;
 * d_list[count .. n_views) is -1; *d_count = count.  Every byte of both outputs is written by every call.
 *
 * WHY A VIEW THAT IS NOT LISTED MAY STAY STALE.  A search reads the grid and the tables of view v only for a query q with
 * d_active[q] != 0 and view v; a list made from the same d_active and d_view_of holds v, and the listed read that follows rebuilds v from
 * the cloud and the masks it is given.  What stays stale is read by nobody in that search.  The argument needs the lattice to stay: a
 * listed read on another lattice is refused, and the caller does a full fh_map_read_views_device instead. */
#ifndef FASTERHIP_VIEW_SUBSET_H
#define FASTERHIP_VIEW_SUBSET_H
#include "fasterhip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The list above into d_list [n_views] and d_count [1] (device memory).  Three launches: flags cleared, a flag per needed view (several
 * queries of one view store the same value), one workgroup that compacts the flags in ascending order by ballot and rank and writes
 * the tail and the count.  Deterministic whatever the order of the wavefronts.  n_views from 1 to 2^24.
 * FH_ERR_ARG: a null map, d_list or d_count; n < 0; n_views <= 0 or above 2^24; n > n_views with a null d_view_of.  Nothing is
 * launched on an error.  n == 0 lists nothing: count 0 and a list of -1. */
int fh_map_view_list_device(fh_map* map, const int32_t* d_active, const int32_t* d_view_of, int n, int n_views, int32_t* d_list,
                            int32_t* d_count);

/* For every e < min(*d_count, n_views) with 0 <= d_list[e] < n_views the grid of view d_list[e] becomes, bit for bit, what
 * fh_map_read_views_device with the same arguments makes it; every other view keeps the bytes of its grid.  If the views of the map
 * have valid jump tables (a view search in mode 1 has run since the last fh_map_read_views_device), the tables of the listed views
 * become what a full rebuild makes them and stay valid; otherwise the next such search builds all of them, as it does today.  Entries
 * outside the range are skipped; a view listed twice is harmless (clearing, marking and the three table levels are launches of their
 * own, in stream order).  *d_count and the list are read on the device only: work is proportional to the count, with no host wait.
 * Needs a previous fh_map_read_views_device on this map with the same lattice (cells, res, center, z_ground, z_max by the same
 * arithmetic), the same n_views and inflation, and mask_words * 32 >= n_cloud; anything else is FH_ERR_ARG with fh_map_last_error
 * set, and nothing is launched.  Never reallocates the grids or the tables. */
int fh_map_read_views_listed_device(fh_map* map, const double* d_cloud_xyz, int n_cloud, const uint32_t* d_point_mask, int mask_words,
                                    int n_views, const int32_t cells[3], double res, const double center[3], double z_ground, double z_max,
                                    double inflation, const int32_t* d_list, const int32_t* d_count);

#ifdef __cplusplus
}
#endif
#endif /* FASTERHIP_VIEW_SUBSET_H */

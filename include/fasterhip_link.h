/* fasterhip_link.h: VEHICLES IN RADIO RANGE POOL WHAT THEIR VIEWS KNOW.  A fleet (include/fasterhip.h) can give every vehicle its own
 * picture of the world: a view of unknown voxels grown by fh_fleet_sense_device, a row of point masks grown by fh_fleet_observe_device
 * (include/fasterhip_occupancy.h).  Views are shared only through d_view_of, a table fixed at set-up: between "alone" and "one team for
 * ever" there was nothing.  Two entry points: one decides who is linked to whom this period, as a label per view; one makes the views
 * of a group equal.  A closed loop is
 *     sense -> observe -> LINK GROUPS -> LINK MERGE -> replan -> next goals;
 * the merged bytes are the two tables every planning stage already reads, so no entry point, struct or kernel of fasterhip.h changes
 * and FH_ABI_VERSION stays.  C99 / C++11, includes fasterhip.h.
 *
 * THE MODEL OF THE GROUPS.  Everything is IEEE double, no fused multiply-add, every comparison strict (tests/link_model.py restates it
 * in numpy, brute force, and the kernels are compared with that in every byte).
 *   Views.  view(i) = d_view_of ? d_view_of[i] : i, as everywhere else.
 *   Speaking.  Vehicle i speaks iff 0 <= view(i) < n_views and all three coordinates of d_vehicles[i].state.pos are finite.
 *   Linked pairs.  i and k (i != k) are linked iff both speak and d2 < range * range, with
 *     d2 = dx dx + dy dy + dz dz,   d = pos_k - pos_i per axis, the three products summed x, y, z from left to right.
 *     Symmetric by construction.  range * range is rounded once.
 *   Edges.  A linked pair is an edge between view(i) and view(k) (two vehicles of one view give an edge that changes nothing).
 *   Labels.  L0[v] = v.  Pass p = 1 .. passes, reading only the labels of the pass before:
 *     hook: H[v] = min(L[v], min over the linked (i, k) with view(i) = v of L[view(k)]);     jump: L'[v] = H[H[v]].
 *     Nothing a pass writes is seen by that same pass.  The minimum over a set does not depend on the order, so an atomic minimum
 *     into a copy of L followed by a jump launch gives these bytes under any scheduling.
 *   Outputs.  d_labels = L after the last pass.  d_info[0] = the number of views whose label changed in the last pass (0: settled),
 *     d_info[1] = the number of views with L[v] == v, d_info[2] = the number of linked pairs i < k, exact, d_info[3] = 0.
 * THREE CONSEQUENCES (tests/test_link_model.py).  L[v] <= v always.  L[v] is always a view of v's connected component (of the graph of
 * views and edges).  Settled labels are the smallest view index of each connected component, and n_views - 1 passes always suffice.
 * HOW MANY PASSES (the CPU model at 64 and at 1024 views; passes after which no label changes).  A jump follows labels, not edges, so a
 * small label travels ONE edge per pass where the labels around it are already low:
 *     a chain in descending index order (63 - 62 - .. - 0)                          6 and 10: the distance to the minimum doubles per pass;
 *     the same chain ascending, zigzag (0, n-1, 1, n-2, ..), sawteeth of 2          6 and 10;      sawteeth of 32: 32 and 36;
 *     a chain in bit-reversed order                                                32 and 512;
 *     an ascending chain with the minimum at its far end (1 - 2 - .. - n-1 - 0)     63 and 1023: the bound n_views - 1 is tight;
 *     random chains (300 / 60 of them)                                             58 and 701;    thin random trees: 33 and 376;
 *     random graphs with n/2 .. 2n edges                                           10 and 21;
 *     vehicles at random in a cube, 1 to 16 linked neighbours each on average      10 and 27 (the most at 5 and at 2.7 neighbours);
 *     vehicles along a corridor in random index order, range = two spacings          8 and 9.
 * The default (FH_LINK_DEFAULT_PASSES = 32) settles every random fleet above and no long chain in a bad order; d_info[0] says which
 * it was.  Labels that have not settled are still safe to merge: a view whose label is not a root is alone this call, the groups
 * that did form are parts of connected components, and what they merged stays merged in the next period.
 *
 * THE CELL GRID.  `cells` (origin, res, dims) is a uniform grid that only the broad phase uses, as in fasterhip_check.h; the box of a
 * vehicle is its one position.  NO OUTPUT BYTE DEPENDS ON THE GRID, OR ON THE CAPACITY OF THE NEIGHBOUR LIST (FH_LINK_LIST): a vehicle
 * with more linked neighbours than its row holds walks the cells again in every pass.  dims = (1, 1, 1) gives the same bytes, slower.
 *
 * THE MERGE.  View v SENDS to r = d_labels[v] iff 0 <= r < n_views, r != v and d_labels[r] == r.  Every other view is alone this call:
 * also a view with a label out of range, and a view whose label is not itself a root (unsettled labels).  The group of a root r is r
 * and its senders; roots never send.  For every group, after the call:
 *   flag byte c < view_bytes of every member is 0 if it was 0 in any member, else what that member had (nothing is ever set);
 *   mask word w < shared_words of every member is the OR of the members' words; words from shared_words on are not touched (traffic
 *     bits are per observer: a vehicle must not inherit its own plan as an obstacle);
 *   bytes between view_bytes and view_stride are not touched.
 * The OR of observed rows is the observation of the AND of the views, so a linked group plans as one team does.
 *
 * KNOWN LIMITS.  Walls do not block a link (fasterhip_link_los.h adds the entry point where they do).  There is no bandwidth or latency model: a call is one period in which a connected group
 * floods everything.  Nothing is forgotten when vehicles part.  Jump tables and grids are not touched: they are rebuilt by the map's
 * view stage as before, and views that are not listed keep old grids (include/fasterhip_view_subset.h). */
#ifndef FASTERHIP_LINK_H
#define FASTERHIP_LINK_H
#include "fasterhip.h"
#ifdef __cplusplus
extern "C" {
#endif

enum {
  FH_LINK_MAX_PASSES = 1024,     /* the largest `passes`: every pass is two launches                                                  */
  FH_LINK_MAX_CELLS = 1 << 20,   /* the largest dims[0] * dims[1] * dims[2] of the cell grid                                          */
  FH_LINK_LIST = 64,             /* views of linked neighbours kept per vehicle; a vehicle with more walks the cells in every pass    */
  FH_LINK_DEFAULT_PASSES = 32    /* abi.default_link_params: random fleets needed up to 10 (64 views) and 27 (1024 views), see above  */
};

typedef struct fh_link_params { /* 32 B */
  double range;          /* linked: d2 < range * range (strict)                                                                     */
  int32_t passes;        /* passes of hook and jump (two launches each)                                                             */
  int32_t reserved[5];
} fh_link_params;

/* d_labels[v] = the label of view v, d_info[0 .. 3] as above: a pure measurement of d_vehicles and d_view_of.  Launches on the
 * context's stream, asynchronous: boxes, cell starts, cell items, the narrow phase (one wavefront per vehicle: the rows of linked
 * views, the pair count), then per pass a hook (one wavefront per vehicle, an atomic minimum only where it lowers a label) and a jump
 * (lane = view); written: d_labels, d_info and working buffers of the context, which every call sets up again on the stream.
 * DETERMINISTIC: a hook reads L and writes a copy, a jump reads the copy and writes L and the next copy; no launch reads what it
 * writes, no kernel waits for another wavefront.
 * FH_ERR_ARG, checked in this order after a null context: par == NULL; range that is NaN, infinite or <= 0; passes outside
 * [1, FH_LINK_MAX_PASSES]; n < 0; n_views < 1; cells == NULL, res <= 0, a dimension < 1, dims[0] dims[1] dims[2] > FH_LINK_MAX_CELLS.
 * Then FH_ERR_DEVICE without a device (there is no CPU path); for n == 0 labels = identity, info = (0, n_views, 0, 0) and FH_OK (the
 * roots are counted from the labels: without d_labels nothing is counted, and a null d_info is skipped); and FH_ERR_ARG for a null
 * d_vehicles, d_labels or d_info.  d_view_of may be NULL.  Every index the kernels use comes from a value they have checked. */
int fh_fleet_link_groups_device(fh_ctx* ctx, const fh_link_params* par, const fh_vehicle* d_vehicles, int n, const int32_t* d_view_of,
                                int n_views, const struct fh_voxel_grid* cells, int32_t* d_labels /* [n_views] */, int64_t* d_info /* [4] */);

/* The views of a group become equal (THE MERGE above), in place.  d_flags: n_views rows of view_bytes flag bytes, view_stride apart
 * (view_stride need not be a multiple of 4); d_point_mask: n_views rows of mask_words words.  Either table may be NULL and is then
 * skipped.  Two launches per table on the context's stream, asynchronous: senders fold into their root, then members take the root's
 * bytes.  Receivers and senders of a launch are disjoint and every write is an atomic AND / OR of an aligned word that lies wholly
 * inside a row, or a single-byte store of zero for the at most three bytes at an unaligned end of a row, so THE RESULT DOES NOT DEPEND
 * ON SCHEDULING; a word is read before it is written and equal bytes cost reads only.
 * FH_ERR_ARG after a null context: n_views < 1; view_stride < view_bytes when d_flags is given; mask_words < 0 or shared_words outside
 * [0, mask_words] when d_point_mask is given.  Then FH_ERR_DEVICE without a device, and FH_ERR_ARG for null labels. */
int fh_fleet_link_merge_device(fh_ctx* ctx, const int32_t* d_labels, int n_views, unsigned char* d_flags, size_t view_stride,
                               size_t view_bytes, uint32_t* d_point_mask, int mask_words, int shared_words);

#ifdef __cplusplus
}
#endif
#endif /* FASTERHIP_LINK_H */

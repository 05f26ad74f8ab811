/* fasterhip_far.h: FAR FRONTIER GOALS, BY A COARSE FLOOD OF THE WHOLE VIEW.  Every chooser of fasterhip_frontier.h and fasterhip_reach.h
 * works inside the bounding box of the vehicle's r_max sphere, at most FH_REACH_MAX_WORDS words of 64 voxels.  A vehicle whose frontiers
 * all lie farther away gets no goal from them and stays where it is, while whole halls of its view are unknown two rooms away.  The
 * entry point of this header floods the WHOLE view at the resolution of blocks of B x B x B voxels, which fits the LDS of a workgroup
 * whatever the size of the view, and gives the vehicle the nearest frontier it can plausibly reach, however far away that is.  It is a
 * fallback: it runs after any of the other choosers, for the vehicles that chooser left without a goal (d_skip is that chooser's mask).
 *     sense -> observe -> [link] -> reach goals -> set_goals -> FAR GOALS (skip = the mask) -> set_goals -> replan -> next goals
 * A pure measurement: no entry point, struct or kernel of another header changes and FH_ABI_VERSION stays.  It takes the map's lattice
 * and bits as arguments (fh_map_dims, fh_map_occupancy_bits_device) and a stream; no handle is needed.  C99 / C++11, includes fasterhip.h,
 * fasterhip_frontier.h and fasterhip_reach.h (FH_FRONTIER_WANT_*, FH_FRONTIER_WANTED | FOUND | NO_VIEW | BAD_POS, FH_REACH_START_OUTSIDE
 * and FH_REACH_CUT are reused).
 *
 * THE MODEL (tests/far_model.py restates it in Python, a queue over blocks, and the kernels are compared with that in every byte).
 * IEEE double, no fused multiply-add, comparisons as written.
 *   Views, wanted, eligible, start cell s.  Those of fasterhip_reach.h word for word: view(i) = d_view_of ? d_view_of[i] : i, the flags
 *     F of view v at d_flags + v * view_stride on the lattice (origin, res, dims = n) of `grid`, cell c = (iz ny + iy) nx + ix; wanted by
 *     the bits of par->want; FH_FRONTIER_NO_VIEW and FH_FRONTIER_BAD_POS judged as there; ELIGIBLE = wanted, a view, six finite
 *     coordinates; s = floor((p - origin) / res), per axis, p = state.pos.
 *   Skipped.  d_skip != NULL and d_skip[i] != 0: the vehicle gets FH_FAR_SKIPPED beside the flags judged as always, and is not searched.
 *   Searched.  Eligible, not skipped, s inside the lattice.  An eligible vehicle that is not skipped and whose s lies outside the lattice
 *     gets FH_REACH_START_OUTSIDE (the bit is judged for those vehicles only).
 *   Blocks.  B = par->block, 1 <= B <= 16.  Per axis C = (n + B - 1) / B.  Block b = (bz Cy + by) Cx + bx covers the voxel indices
 *     [b_a B, min(b_a B + B, n_a)) per axis a.  wx = ceil(Cx / 64), W = wx Cy Cz; the bit of b is bit bx & 63 of word
 *     (bz Cy + by) wx + (bx >> 6); bits beyond Cx are 0.  W > FH_FAR_MAX_WORDS is FH_ERR_ARG: a property of the call, not of a vehicle.
 *   Passable voxel.  That of fasterhip_reach.h: the flag is 0, and the map cell floor((q - origin_map) / res_map), per axis, of its centre
 *     q = (ix + 0.5) res + origin lies inside the map with its bit clear.
 *   Target voxel of view v.  Passable, a frontier voxel of v (fasterhip_frontier.h: an unknown face neighbour inside the lattice), and
 *     z_lo <= q.z <= z_hi.  It does not depend on the vehicle.
 *   Summary of view v.  Four bitmaps of W words.  T: the block holds a target voxel.  LX: bx + 1 < Cx, and some voxel c of b and its +x
 *     neighbour, which lies in block b + (1, 0, 0), are both passable.  LY, LZ: likewise along y and z.  A link is a real pair of free
 *     voxels with a face in common across the face the blocks share, not "both blocks hold something free".
 *   Needed.  View v is summarised iff some searched vehicle reads it; the summary words of a view nobody needs are not written.
 *   Workspace.  [n_views][4][W] words of 64 bits in the order T, LX, LY, LZ, then ((n_views + 63) & ~63) need bytes (0 / 1):
 *     fh_far_work_bytes = n_views * 4 * W * 8 + ((n_views + 63) & ~63), and 0 for a null grid, a dimension < 1, a block outside 1..16,
 *     W > FH_FAR_MAX_WORDS or n_views < 1.
 *   Flood of vehicle i.  Level 0 = {the block of s}, whatever its bits.  Level k + 1 = the blocks in no earlier level that a link joins
 *     to a block of level k; a link counts in either direction.  The flood ends at an empty level, or after level max_hops if
 *     max_hops > 0, and then sets FH_REACH_CUT iff that level is not empty, as fasterhip_reach.h does.  hops(b) = the level of b.
 *   Distance to a block.  Per axis lo = (b_a B + 0.5) res + origin and hi = (min(b_a B + B, n_a) - 1 + 0.5) res + origin, the centres of
 *     its first and last voxel; gap(x) = x < lo ? lo - x : (x > hi ? x - hi : 0.0); D2(b) = gap(p.x)^2 + gap(p.y)^2 + gap(p.z)^2, summed
 *     in that order, and E2(b) the same from g_term.
 *   Target block of vehicle i.  Its T bit is set, and not (E2(b) < r_avoid * r_avoid), the product rounded once; r_avoid = 0: off.
 *     (Every target voxel of a target block then has e2 >= r_avoid^2 by the voxel rule of fasterhip_frontier.h: subtraction, squaring and
 *     summation are monotone.  The voxel rule is not tested again.)
 *   Choice.  Of the target blocks in some level the one with the smallest (hops, D2, b), and in it, of the target voxels of the view, the
 *     one with the smallest (d2, c), d2 = that header's expression from p.
 *   Outputs.  Every byte of all three is written by every call.  d_mask[i] = 1 iff a voxel was chosen; d_goals[3 i ..] = its centre q,
 *     else the bits of g_term.  d_records[i]: flags = FH_FRONTIER_WANTED | NO_VIEW | BAD_POS | FH_FAR_SKIPPED | FH_REACH_START_OUTSIDE |
 *     FH_FRONTIER_FOUND if a voxel was chosen | FH_REACH_CUT; view as read; cell = the voxel, block_cell = b and hops of the choice, -1
 *     without one; targets = the target blocks of vehicle i in the whole view, reached or not; reachable = those in some level; reached =
 *     the blocks in some level; levels = the index of the last level that is not empty; members = the target voxels of the chosen block;
 *     d2 and block_d2 = D2(b) of the choice, +inf without one; reserved = 0.  A vehicle that is not searched has cell = block_cell =
 *     hops = -1, targets = reachable = reached = levels = members = 0, d2 = block_d2 = +inf.
 *
 * KNOWN LIMITS.  Connectivity inside a block is assumed: two links of a block count as joined, whatever lies between them.  Hops are
 * block steps, not metres.  Unknown voxels are never passable.  The path search has the last word: a goal it answers with NO_PATH is
 * answered next period by `want` no_path and r_avoid, as with the other choosers. */
#ifndef FASTERHIP_FAR_H
#define FASTERHIP_FAR_H
#include "fasterhip.h"
#include "fasterhip_frontier.h"
#include "fasterhip_reach.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { FH_FAR_SKIPPED = 128 };   /* fh_far_record.flags, beside FH_FRONTIER_WANTED .. FH_REACH_CUT: d_skip[i] != 0, nothing searched        */
enum { FH_FAR_MAX_WORDS = 512 }; /* words of 64 blocks (a row of x begins a word) that the blocks of the lattice may need               */

typedef struct fh_far_params { /* 64 B */
  double r_avoid;    /* no target block with E2 < r_avoid * r_avoid around g_term; 0: off                                            */
  double z_lo;       /* target voxels: z_lo <= q.z <= z_hi                                                                           */
  double z_hi;
  double reserved_d; /* 0                                                                                                            */
  int32_t want;      /* FH_FRONTIER_WANT_*, a bit set                                                                                */
  int32_t max_hops;  /* the last level of the flood; 0: no limit                                                                     */
  int32_t block;     /* B, the edge of a block in voxels, 1 .. 16                                                                    */
  int32_t reserved[5];
} fh_far_params;

typedef struct fh_far_record { /* 64 B */
  int32_t flags;      /* FH_FRONTIER_WANTED | FOUND | NO_VIEW | BAD_POS | FH_REACH_START_OUTSIDE | FH_REACH_CUT | FH_FAR_SKIPPED      */
  int32_t view;       /* view(i) as read                                                                                             */
  int32_t cell;       /* the chosen voxel of the lattice, -1: none                                                                   */
  int32_t block_cell; /* the block b it lies in, -1: none                                                                            */
  int32_t hops;       /* the level of that block, -1: none                                                                           */
  int32_t targets;    /* the target blocks of the vehicle in the whole view, reached or not                                          */
  int32_t reachable;  /* how many of them are in some level                                                                          */
  int32_t reached;    /* blocks in some level, the start's included                                                                  */
  int32_t levels;     /* the index of the last level that is not empty (0: only the start); 0 when not searched                      */
  int32_t members;    /* the target voxels of the chosen block, 0: none                                                              */
  int32_t reserved[2];
  double d2;          /* of the chosen voxel, +inf: none                                                                             */
  double block_d2;    /* D2 of the chosen block, +inf: none                                                                          */
} fh_far_record;

/* The bytes of d_work for these arguments (above); 0 where the arguments are not valid. */
size_t fh_far_work_bytes(const struct fh_voxel_grid* grid, int block, int n_views);

/* d_mask [n] int32, d_goals [n][3] and d_records [n] as above, in the shape fh_fleet_set_goals_device takes.  map_grid and d_map_bits as
 * for the entry point of fasterhip_reach.h.  d_skip [n] int32 or NULL: the mask another chooser wrote in this period.  d_work: work_bytes
 * >= fh_far_work_bytes(grid, par->block, n_views) of device memory, 8-byte aligned; what it holds before the call is not read.  On
 * `stream` (a hipStream_t, NULL: the default stream), asynchronous, on the device that owns d_records: a memset of the need bytes, a
 * thread per vehicle that marks the views that are needed, a pass over the voxels of the needed views that writes their summaries, and
 * one workgroup of 256 per vehicle.  A vehicle that is not searched costs its three outputs.  Reads nothing it writes but d_work;
 * DETERMINISTIC: integer work and the minimum of total orders, no atomics.
 * FH_ERR_ARG, checked in this order, all before the first call of the runtime: par == NULL; r_avoid NaN, infinite or negative; z_lo or
 * z_hi NaN, or z_lo > z_hi; want == 0 or a bit above 4; max_hops < 0; block outside 1..16; map_grid null, res not > 0 or a dimension
 * < 1; more than 2^31 - 1 map cells; d_map_bits null; grid null, res not > 0, or a dimension < 1; more than 2^31 - 1 cells;
 * view_stride < cells; n_views < 1; n < 0; W > FH_FAR_MAX_WORDS; work_bytes < fh_far_work_bytes.  Then FH_OK for n == 0, then FH_ERR_ARG
 * for a null d_work, d_flags, d_vehicles, d_goals, d_mask or d_records.  d_view_of and d_skip may be NULL.  FH_ERR_DEVICE: d_records is
 * no device memory, or a launch failed.  Every index the kernels use comes from a value they have checked. */
int fh_far_goals_device(void* stream, const fh_far_params* par, const struct fh_voxel_grid* map_grid, const unsigned* d_map_bits,
                        const struct fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of,
                        int n_views, const int32_t* d_skip, const fh_vehicle* d_vehicles, int n, void* d_work, size_t work_bytes,
                        double* d_goals, int32_t* d_mask, fh_far_record* d_records);

#ifdef __cplusplus
}
#endif
#endif /* FASTERHIP_FAR_H */

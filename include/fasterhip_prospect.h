/* fasterhip_prospect.h: FAR FRONTIER GOALS BY WHAT THEY WOULD UNCOVER — UNKNOWN VOXELS PER BLOCK, AND A UTILITY OVER ALL LEVELS.  The far
 * chooser (K21 in DESIGN.md, the fallback that floods the whole view by blocks of B x B x B voxels) takes the fewest block steps, then
 * the nearest block: a one-voxel hole of unknown space in the next block beats the edge of an unexplored hall three blocks on, every
 * period, until the hole is filled, and a far goal costs a whole flight.  The entry point of this header is that chooser with the
 * next-best-view rule of the near chooser that weighs a candidate by what it would uncover (K17), one level up: every block carries the
 * number of its unknown voxels, the PROSPECT of a target block is the sum of those numbers over a cube of blocks around it, and the
 * vehicle takes the target block with the largest  utility = gain - hop_cost * hops  of all levels of its flood.
 *     sense -> observe -> [link] -> a chooser -> set_goals -> PROSPECT GOALS (skip = its mask) -> set_goals -> replan -> next goals
 * A pure measurement: no entry point, struct or kernel of another header changes and FH_ABI_VERSION stays.  C99 / C++11, includes
 * fasterhip.h, fasterhip_frontier.h and fasterhip_reach.h.  K21's header keeps its names to itself, as it does towards every header
 * built beside it: its skip flag, word cap, params and record stand here under this header's names with their values and layouts (the
 * host file asserts the equalities).
 *
 * THE MODEL (tests/far_gain_model.py restates it in Python on the pieces of tests/far_model.py; the kernels are compared with that in
 * every byte).  What K21 computes is IEEE double with no fused multiply-add; everything this header adds is integer arithmetic.
 *   Views, wanted, eligible, start cell, skipped, searched, blocks, W, passable voxel, target voxel, the summary T / LX / LY / LZ, needed,
 *     flood, D2 / E2, the TARGET BLOCK of a vehicle and r_avoid: K21's header's, word for word.  B = par->block, C_a = (n_a + B - 1) / B
 *     per axis, b = (bz Cy + by) Cx + bx, wx = ceil(Cx / 64), W = wx Cy Cz, the bit of b is bit bx & 63 of word (bz Cy + by) wx + (bx >> 6).
 *   Unknown count.  U(v, b) = the number of voxels u of block b, inside the lattice, with F_v[u] != 0.  The map bits do not enter, z_lo
 *     and z_hi do not enter, and a partial last block counts only its voxels inside the lattice.  0 <= U <= B^3 <= 4096.
 *   Gain.  g = par->gain_blocks, 0 <= g <= FH_PROSPECT_MAX_BLOCKS.  gain(b) = the sum of U(v, b') over the blocks b' of the lattice with
 *     |b'_a - b_a| < g on every axis a: a cube of edge 2 g - 1 blocks, clipped to [0, C_a) per axis; it never wraps from the end of a
 *     row of x into the next row.  g = 0: the cube is empty and every gain is 0.  The gain does not depend on the vehicle: r_avoid
 *     removes targets, not unknown voxels from a neighbour's gain.  gain <= 729 * 4096 < 2^22.
 *   Utility.  utility(b) = gain(b) - hop_cost * hops(b), an int32.  0 <= hop_cost <= FH_PROSPECT_MAX_HOP_COST and hops < 32768, so
 *     |utility| < 2^30.
 *   Poor.  A target block in some level with gain(b) < min_gain is POOR and never chosen.  min_gain >= 0.
 *   Choice.  Of the target blocks in some level that are not poor the one with the largest utility; among equals the smallest
 *     (hops, D2, b).  In the chosen block K21's voxel rule: of the target voxels of the view the smallest (d2, c).  The choice is over
 *     ALL levels: K21 stops choosing at the first level that holds a target block, this chooser cannot.
 *   Reduction.  With gain_blocks = 0, hop_cost >= 1 and min_gain = 0 the values d_goals, d_mask, the first 64 bytes of every record, the
 *     summary words and the need bytes are those of K21's entry point, exactly.
 *   Workspace.  K21's: [n_views][4][W] words of 64 bits in the order T, LX, LY, LZ, then ((n_views + 63) & ~63) need bytes (0 / 1).
 *     Then the counts: [n_views][64 W] of uint16_t, entry 64 word + bit = U(v, b) of the block whose T bit is that bit; the entries of
 *     bits beyond Cx are 0.  Neither the summary words nor the counts of a view nobody needs are written.
 *     fh_prospect_work_bytes = n_views * 4 * W * 8 + ((n_views + 63) & ~63) + n_views * 64 * W * 2 (the first two terms are a multiple
 *     of 8, so the table is aligned), and 0 for a null grid, a dimension < 1, a block outside 1..16, W > FH_PROSPECT_MAX_WORDS or
 *     n_views < 1.
 *   Outputs.  Every byte of all three is written by every call.  d_mask[i] = 1 iff a voxel was chosen; d_goals[3 i ..] = its centre,
 *     else the bits of g_term.  The first 64 bytes of d_records[i] are K21's record with cell, block_cell, hops, members, d2 and block_d2
 *     of THIS choice; targets, reachable, reached and levels as there (reachable counts poor blocks too).  gain = that of the chosen
 *     block, -1 without one; utility = that of the chosen block, 0 without one; poor = the poor target blocks in some level; best_gain =
 *     the largest gain of a target block in some level, poor ones included, -1 without one.  flags: K21's | FH_PROSPECT_ALL_POOR iff
 *     reachable > 0 and every reachable target block is poor.  A vehicle that is not searched has gain = best_gain = -1, utility =
 *     poor = 0 and the rest as K21's record of such a vehicle.
 *
 * KNOWN LIMITS.  No claims of peers: composing with the far chooser for a team is a later change (the flag values 256 and 512 are
 * left free for it, and the counts are per view, not per vehicle).  The cube is not a sensor footprint.  Unknown space behind walls
 * counts.  The counts are rebuilt in every call.  K21's limits hold: connectivity inside a block is assumed, hops are block steps. */
#ifndef FASTERHIP_PROSPECT_H
#define FASTERHIP_PROSPECT_H
#include "fasterhip.h"
#include "fasterhip_frontier.h"
#include "fasterhip_reach.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { FH_PROSPECT_SKIPPED = 128 };    /* fh_prospect_record.flags: d_skip[i] != 0, nothing searched (K21's bit)                          */
enum { FH_PROSPECT_ALL_POOR = 1024 };  /* reachable > 0 and every reachable target block is poor (256 and 512: the team's far chooser)    */
enum { FH_PROSPECT_MAX_WORDS = 512 };  /* words of 64 blocks that the blocks of the lattice may need (K21's cap)                          */
enum { FH_PROSPECT_MAX_BLOCKS = 5, FH_PROSPECT_MAX_HOP_COST = 16384 };

typedef struct fh_prospect_params { /* 64 B: K21's params, three of its reserved words in use */
  double r_avoid;
  double z_lo;
  double z_hi;
  double reserved_d;   /* 0                                                                                                          */
  int32_t want;
  int32_t max_hops;
  int32_t block;
  int32_t gain_blocks; /* g: the cube of a gain has 2 g - 1 blocks an edge; 0 .. FH_PROSPECT_MAX_BLOCKS, 0: every gain is 0          */
  int32_t hop_cost;    /* unknown voxels that one block step must be worth; 0 .. FH_PROSPECT_MAX_HOP_COST                            */
  int32_t min_gain;    /* a target block with a smaller gain is poor; >= 0                                                           */
  int32_t reserved[2];
} fh_prospect_params;

typedef struct fh_prospect_record { /* 80 B: the first 64 bytes are laid out as K21's record */
  int32_t flags;       /* K21's | FH_PROSPECT_SKIPPED | FH_PROSPECT_ALL_POOR                                                         */
  int32_t view;
  int32_t cell;
  int32_t block_cell;
  int32_t hops;
  int32_t targets;
  int32_t reachable;   /* the target blocks in some level, poor or not                                                               */
  int32_t reached;
  int32_t levels;
  int32_t members;
  int32_t reserved[2];
  double d2;
  double block_d2;
  int32_t gain;        /* of the chosen block, -1: none                                                                              */
  int32_t utility;     /* of the chosen block, 0: none                                                                               */
  int32_t poor;        /* the poor target blocks in some level                                                                       */
  int32_t best_gain;   /* the largest gain of a target block in some level, poor ones included, -1: none                             */
} fh_prospect_record;

/* The bytes of d_work for these arguments (above); 0 where the arguments are not valid. */
size_t fh_prospect_work_bytes(const struct fh_voxel_grid* grid, int block, int n_views);

/* The seventeen arguments of K21's entry point in its order, with this header's params and record.  d_work: work_bytes >=
 * fh_prospect_work_bytes(grid, par->block, n_views) of device memory, 8-byte aligned; what it holds before the call is not read.  On
 * `stream` (a hipStream_t, NULL: the default stream), asynchronous, on the device that owns d_records: a memset of the need bytes, K21's
 * thread per vehicle that marks the views that are needed, ONE pass over the flag bytes of the needed views that writes the four bitmaps
 * and the counts (a workgroup per word of 64 blocks and view, a wavefront per line of voxels along x, so a wavefront reads whole lines
 * of 64 bytes; the ballots of a run of 64 voxels are split per block by masks), and one workgroup of 256 per vehicle, which floods as
 * K21 does, weighs every target block of every level with the counts of its cube, and scans the voxels of the chosen block once.
 * DETERMINISTIC: integer work and the minimum of total orders, no atomics.
 * FH_ERR_ARG, checked in this order, all before the first call of the runtime: par == NULL; r_avoid NaN, infinite or negative; z_lo or
 * z_hi NaN, or z_lo > z_hi; want == 0 or a bit above 4; max_hops < 0; block outside 1..16; gain_blocks outside 0 ..
 * FH_PROSPECT_MAX_BLOCKS; hop_cost outside 0 .. FH_PROSPECT_MAX_HOP_COST; min_gain < 0; map_grid null, res not > 0 or a dimension < 1;
 * more than 2^31 - 1 map cells; d_map_bits null; grid null, res not > 0, or a dimension < 1; more than 2^31 - 1 cells; view_stride <
 * cells; n_views < 1; n < 0; W > FH_PROSPECT_MAX_WORDS; work_bytes < fh_prospect_work_bytes.  Then FH_OK for n == 0, then FH_ERR_ARG for
 * a null d_work, d_flags, d_vehicles, d_goals, d_mask or d_records.  d_view_of and d_skip may be NULL.  FH_ERR_DEVICE: d_records is no
 * device memory, or a launch failed.  Every index the kernels use comes from a value they have checked. */
int fh_prospect_goals_device(void* stream, const fh_prospect_params* par, const struct fh_voxel_grid* map_grid, const unsigned* d_map_bits,
                             const struct fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of,
                             int n_views, const int32_t* d_skip, const fh_vehicle* d_vehicles, int n, void* d_work, size_t work_bytes,
                             double* d_goals, int32_t* d_mask, fh_prospect_record* d_records);

#ifdef __cplusplus
}
#endif
#endif /* FASTERHIP_PROSPECT_H */

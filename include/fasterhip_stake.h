/* fasterhip_stake.h: FAR FRONTIER GOALS BY WHAT THEY WOULD UNCOVER, FOR A TEAM — A PEER'S CLAIM IS A REGION.  The far fallback (K21 in
 * DESIGN.md, a flood of the whole view by blocks of B x B x B voxels) has a chooser for a team (K22: a peer's claim removes the target
 * blocks within r_spread of it) and a chooser by gain (K23: the unknown voxels of a cube of blocks around a target block, a utility over
 * all levels).  A fleet had to pick one defect: with K23 two stranded teammates on one view compute the same utilities and fly to the same
 * hall; with K22 they part by r_spread, but each takes the nearest one-voxel hole.  The entry point of this header is K22's passes with
 * K23's utility inside them, and one new rule: a claim STAKES A REGION.  It removes the target blocks within r_spread of it (K22's
 * rule), and it removes, from every gain of the vehicle, the unknown voxels of the blocks in a cube around the claim's block: that peer
 * uncovers them anyway.  It is the far counterpart of the near chooser that weighs gain inside a team's passes (K18).
 *     sense -> observe -> [link] -> a chooser -> set_goals -> STAKE GOALS (skip = its mask) -> set_goals -> replan -> next goals
 * A pure measurement: no entry point, struct or kernel of another header changes and FH_ABI_VERSION stays.  C99 / C++11, includes
 * fasterhip.h, fasterhip_frontier.h and fasterhip_reach.h.  The headers of K21, K22 and K23 keep their names to themselves, as they do
 * towards every header built beside them: what this header takes from them stands here under its own names with equal values and
 * layouts (the host file asserts the equalities).
 *
 * THE MODEL (tests/far_team_model.py restates it in Python over the vehicles in index order, on the pieces of the models of K21, K22 and
 * K23; the kernels are compared with that in every byte).  What K21 and K22 compute is IEEE double with no fused multiply-add; everything
 * K23 and this header add is integer arithmetic.
 *   From K21, word for word: views, wanted, eligible, skipped, searched, blocks, W, passable voxel, target voxel, the summary
 *     T / LX / LY / LZ, needed, flood, D2 / E2, r_avoid, the TARGET BLOCK of a vehicle and the voxel choice.  B = par->block,
 *     C_a = (n_a + B - 1) / B per axis, b = (bz Cy + by) Cx + bx, wx = ceil(Cx / 64), W = wx Cy Cz.
 *   From K22, word for word: groups, peers, the classes SEARCHER / STANDING / NONE, lower(i), standing(i), the pass of a searcher
 *     (lower(i) + 1), FH_STAKE_UNSETTLED for lower(i) >= passes, the CLAIMS of searcher i (the g_term of every standing peer, and the
 *     d_goals[k] of every searching peer k < i with d_mask[k] == 1), and a CLAIMED block: a target block of the vehicle with
 *     G2(b, c) < r_spread r_spread for some claim c (r_spread r_spread rounded once on the host, the comparison strict).  Claims remove
 *     targets, never links.
 *   From K23, word for word: U(v, b), the unknown voxels of block b inside the lattice; the cube of 2 g - 1 blocks an edge around a
 *     block, g = par->gain_blocks, clipped to [0, C_a) per axis, which never wraps from the end of a row of x into the next row;
 *     utility = gain - hop_cost * hops; POOR: gain < min_gain; the choice over ALL levels of the flood.
 *   Covered set of searcher i (new).  k = par->claim_blocks, 0 <= k <= FH_STAKE_MAX_CLAIM_BLOCKS.  The voxel of a claim point c is
 *     floor((c_a - origin_a) / res) per axis, judged inside or outside the lattice exactly as K21 judges the start cell of a vehicle: the
 *     same expression, compared with 0 and n_a as a double before any conversion.  A claim whose voxel lies outside covers nothing (it
 *     still claims target blocks by K22's rule).  Otherwise cb_a = voxel_a / B, and the claim COVERS the blocks b' of the lattice with
 *     |b'_a - cb_a| < k on every axis: a cube of 2 k - 1 blocks an edge, clipped to [0, C_a) per axis, never wrapping.  Covered(i) = the
 *     union over the claims of i.  k = 0 covers nothing.  Integer arithmetic only.  A covered block that is a target block stays one.
 *   Gain of searcher i.  gain_i(b) = the sum of U(view(i), b') over the blocks b' of the cube of b that are NOT in Covered(i).  The gain
 *     now depends on the vehicle.  Poor, utility, best_gain and poor all use gain_i.
 *   Choice.  Of the target blocks of the vehicle that are in some level, not claimed and not poor, the one with the largest utility;
 *     among equals the smallest (hops, D2, b).  In the chosen block K21's voxel rule, the smallest (d2, c).
 *   Record.  The first 96 bytes are K22's record for THIS choice: targets = the target blocks of the vehicle, claimed or not; reachable
 *     = those in some level and not claimed, poor or not; group, decided_pass, lower, standing, claims, claimed as there.  gain, utility,
 *     poor, best_gain: K23's rules on gain_i.  covered = the number of blocks of Covered(i), each counted once; removed = the sum of
 *     U(view(i), b') over Covered(i).  flags: K21's | FH_STAKE_UNSETTLED | FH_STAKE_ALL_POOR (reachable > 0 and every reachable block is
 *     poor) | FH_STAKE_CLAIMED (searched, nothing chosen, claimed > 0); the last two may be set together.  A vehicle that is not
 *     searched, or is UNSETTLED, has gain = best_gain = -1 and utility = poor = covered = removed = 0 beside K22's fields for it.
 *   Every byte of d_goals, d_mask and d_records is written by every call.
 *   Workspace.  K23's, n_views * 4 * W * 8 + ((n_views + 63) & ~63) + n_views * 64 * W * 2 bytes (the summary words, the need bytes,
 *     the counts), then K22's tail: ((n + 63) & ~63) class bytes + n int32 groups + n int32 `lower`.
 *   Consequences.  (a) Where no searcher has a peer, d_goals, d_mask, the first 64 bytes of every record, gain, utility, poor, best_gain
 *     and K23's part of the workspace are K23's.  (b) With gain_blocks = 0, hop_cost >= 1 and min_gain = 0, for any claim_blocks,
 *     d_goals, d_mask, the first 96 bytes of every record and the class / group / lower tail of the workspace are K22's.  (c) Both
 *     together give K21.  (d) gain_i(b) <= K23's gain(b): coverage only takes terms out of a sum of non-negative numbers.  (e) K22's
 *     consequence (b) holds: with passes > the largest lower no two peers are given goals nearer than r_spread, and no goal lies within
 *     r_spread of a standing peer's g_term — coverage removes no claim and adds no target.
 *
 * KNOWN LIMITS.  The covered cube is a guess at what a peer uncovers, not a sensor footprint, and it is centred on the claim, not
 * swept along the peer's flight.  The vehicle index decides who yields.  A team of m stranded members needs m passes.  K21's, K22's
 * and K23's limits hold: connectivity inside a block is assumed, hops are block steps, unknown space behind walls counts, the counts
 * are rebuilt in every call, every count of peers scans all n vehicles. */
#ifndef FASTERHIP_STAKE_H
#define FASTERHIP_STAKE_H
#include "fasterhip.h"
#include "fasterhip_frontier.h"
#include "fasterhip_reach.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { FH_STAKE_SKIPPED = 128 };   /* fh_stake_record.flags: d_skip[i] != 0, nothing searched (K21's bit)                                  */
enum {
  FH_STAKE_UNSETTLED = 256,        /* lower >= passes, not searched (K22's bit)                                                          */
  FH_STAKE_CLAIMED = 512,          /* searched, nothing chosen, and claimed > 0 (K22's bit)                                              */
  FH_STAKE_ALL_POOR = 1024         /* reachable > 0 and every reachable target block is poor (K23's bit)                                 */
};
enum { FH_STAKE_MAX_WORDS = 512 }; /* words of 64 blocks that the blocks of the lattice may need (K21's cap)                              */
enum { FH_STAKE_MAX_PASSES = 64, FH_STAKE_DEFAULT_PASSES = 8 };
enum { FH_STAKE_MAX_BLOCKS = 5, FH_STAKE_MAX_HOP_COST = 16384 };
enum { FH_STAKE_MAX_CLAIM_BLOCKS = 5 };

typedef struct fh_stake_params { /* 96 B: K22's params, three reserved words of K21's part and one of the tail in use */
  double r_avoid;
  double z_lo;
  double z_hi;
  double reserved_d;    /* 0                                                                                                         */
  int32_t want;
  int32_t max_hops;
  int32_t block;
  int32_t gain_blocks;  /* g: the cube of a gain has 2 g - 1 blocks an edge; 0 .. FH_STAKE_MAX_BLOCKS, 0: every gain is 0              */
  int32_t hop_cost;     /* unknown voxels that one block step must be worth; 0 .. FH_STAKE_MAX_HOP_COST                               */
  int32_t min_gain;     /* a target block with a smaller gain is poor; >= 0                                                          */
  int32_t reserved[2];  /* 0                                                                                                         */
  double r_spread;      /* no target block with G2 < r_spread * r_spread around a claim; finite and > 0                              */
  int32_t passes;       /* 1 .. FH_STAKE_MAX_PASSES                                                                                  */
  int32_t claim_blocks; /* k: a claim covers a cube of 2 k - 1 blocks an edge; 0 .. FH_STAKE_MAX_CLAIM_BLOCKS, 0: nothing is covered  */
  int32_t reserved_tail[4]; /* 0                                                                                                     */
} fh_stake_params;

typedef struct fh_stake_record { /* 128 B: the first 96 bytes are laid out as K22's record, whose first 64 are K21's */
  int32_t flags;        /* K21's | FH_STAKE_SKIPPED | FH_STAKE_UNSETTLED | FH_STAKE_CLAIMED | FH_STAKE_ALL_POOR                        */
  int32_t view;
  int32_t cell;
  int32_t block_cell;
  int32_t hops;
  int32_t targets;      /* the target blocks of the vehicle, claimed or not                                                          */
  int32_t reachable;    /* those in some level and not claimed, poor or not                                                          */
  int32_t reached;
  int32_t levels;
  int32_t members;
  int32_t reserved[2];
  double d2;
  double block_d2;
  int32_t group;        /* group(i); 0 without a view in range                                                                       */
  int32_t decided_pass; /* 0: no searcher; 1 .. passes: searched in that pass; -1: UNSETTLED                                         */
  int32_t lower;        /* the searching peers below i                                                                               */
  int32_t standing;     /* the standing peers, of any index                                                                          */
  int32_t claims;       /* standing + the lower peers with d_mask == 1 (UNSETTLED: standing)                                         */
  int32_t claimed;      /* the target blocks of the vehicle that are claimed, reached or not                                         */
  int32_t reserved_tail[2];
  int32_t gain;         /* gain_i of the chosen block, -1: none                                                                      */
  int32_t utility;      /* of the chosen block, 0: none                                                                              */
  int32_t poor;         /* the poor target blocks in some level that are not claimed                                                 */
  int32_t best_gain;    /* the largest gain_i of a target block in some level that is not claimed, poor ones included, -1: none      */
  int32_t covered;      /* the blocks of Covered(i), each counted once                                                               */
  int32_t removed;      /* the sum of U over Covered(i)                                                                              */
  int32_t reserved_end[2];
} fh_stake_record;

/* The bytes of d_work: n_views * 4 * W * 8 + ((n_views + 63) & ~63) + n_views * 64 * W * 2 + ((n + 63) & ~63) + n * 4 + n * 4, with W
 * the words of a bitmap of blocks; 0 where K23's workspace is 0 (a null grid, a dimension < 1, a block outside 1..16,
 * W > FH_STAKE_MAX_WORDS, n_views < 1) or n < 0. */
size_t fh_stake_work_bytes(const struct fh_voxel_grid* grid, int block, int n_views, int n);

/* K22's eighteen arguments in K22's order, with this header's params and record: d_group [n_views] int32 or NULL after d_skip, and
 * d_records [n] fh_stake_record.  d_work: work_bytes >= fh_stake_work_bytes(grid, par->block, n_views, n) of device memory, 8-byte
 * aligned; what it holds before the call is not read.  On `stream` (a hipStream_t, NULL: the default stream), asynchronous, on the
 * device that owns d_records: a memset of the need bytes; K21's thread per vehicle that marks the views that are needed; K23's ONE pass
 * over the flag bytes of the needed views for the four bitmaps and the counts; K22's thread per vehicle for the class bytes and
 * groups; a wavefront per vehicle that counts lower and standing and writes the outputs of every vehicle that no pass decides; then per
 * pass a workgroup of 256 per vehicle, which returns at once unless lower == pass - 1: it scans the n vehicles in chunks of 256,
 * takes the blocks its claims claim out of T in LDS and sets the blocks they cover in a seventh bitmap in LDS (a word has one writer),
 * sums covered and removed, floods as K21 does, weighs every target block of every level with the counts of its cube that are not
 * covered, and scans the voxels of the chosen block once.  No atomics, no kernel waits for another wavefront.  DETERMINISTIC: a launch
 * reads of other vehicles only what earlier launches wrote; integer work and minima of total orders.
 * FH_ERR_ARG, checked in this order, all before the first call of the runtime: par == NULL; r_avoid NaN, infinite or negative; z_lo or
 * z_hi NaN, or z_lo > z_hi; want == 0 or a bit above 4; max_hops < 0; block outside 1..16; gain_blocks outside 0 ..
 * FH_STAKE_MAX_BLOCKS; hop_cost outside 0 .. FH_STAKE_MAX_HOP_COST; min_gain < 0; map_grid null, res not > 0 or a dimension < 1; more
 * than 2^31 - 1 map cells; d_map_bits null; grid null, res not > 0, or a dimension < 1; more than 2^31 - 1 cells; view_stride < cells;
 * n_views < 1; n < 0; W > FH_STAKE_MAX_WORDS; r_spread NaN, infinite or <= 0; passes < 1 or > FH_STAKE_MAX_PASSES; claim_blocks outside
 * 0 .. FH_STAKE_MAX_CLAIM_BLOCKS; work_bytes < fh_stake_work_bytes.  Then FH_OK for n == 0, then FH_ERR_ARG for a null d_work, d_flags,
 * d_vehicles, d_goals, d_mask or d_records.  d_view_of, d_skip and d_group may be NULL.  FH_ERR_DEVICE: d_records is no device memory,
 * or a launch failed.  Every index the kernels use comes from a value they have checked. */
int fh_stake_goals_device(void* stream, const fh_stake_params* par, const struct fh_voxel_grid* map_grid, const unsigned* d_map_bits,
                          const struct fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of,
                          int n_views, const int32_t* d_skip, const int32_t* d_group, const fh_vehicle* d_vehicles, int n, void* d_work,
                          size_t work_bytes, double* d_goals, int32_t* d_mask, fh_stake_record* d_records);

#ifdef __cplusplus
}
#endif
#endif /* FASTERHIP_STAKE_H */

/* fasterhip_apart.h: FAR FRONTIER GOALS FOR A TEAM — A PEER'S CLAIM REMOVES TARGET BLOCKS, AND STRANDED TEAMMATES FLY APART.  The far
 * chooser (K21 in DESIGN.md, the fallback that floods the whole view by blocks) decides for every vehicle alone: two stranded teammates with one view choose the same voxel, rooms away,
 * both fly the long way, one uncovers it.  The entry point of this header is that chooser with one more rule, the rule of the near
 * chooser for a team (K16, Fleet.explore_spread) at the resolution of blocks: a target block nearer than r_spread to a goal that a
 * PEER holds or has just been given is no target of the vehicle.  Peers are the vehicles of one group; who yields is decided by the
 * vehicle index.
 *     sense -> observe -> [link] -> a chooser -> set_goals -> FAR SPREAD GOALS (skip = its mask) -> set_goals -> replan -> next goals
 * A pure measurement: no entry point, struct or kernel of another header changes and FH_ABI_VERSION stays.  C99 / C++11, includes
 * fasterhip.h, fasterhip_frontier.h and fasterhip_reach.h.  K21's header and the team chooser's keep their names to themselves, as
 * they do towards every header built beside them: K21's skip flag, word cap, params and record, and K16's two flags and pass limits,
 * stand here under this header's names with their values and layouts (the host file asserts the equalities); K16's list cap has no
 * counterpart, for there are no lists.
 *
 * THE MODEL (tests/far_spread_model.py restates it in Python over the vehicles in index order, on tests/far_model.py; the kernels are
 * compared with that in every byte).  IEEE double, no fused multiply-add; squared lengths are summed x, y, z from the left;
 * r_spread r_spread is rounded once on the host; every comparison is strict.
 *   Views, wanted, eligible, skipped, searched, blocks, passable, target voxel, summary, needed, flood, D2, E2 and the TARGET BLOCK of a
 *     vehicle: K21's header's, word for word.  The summary stage is K21's own launches: a view is needed iff some searched
 *     vehicle reads it, settled or not, so the summary words and the need bytes of a call equal what K21's entry point writes for
 *     the same arguments.
 *   Groups and peers.  K16's: group(i) = d_group ? d_group[view(i)] : view(i) for a vehicle whose view is in
 *     [0, n_views), compared for equality only (any int32 is a label); 0 in the record of any other.  PEERS: different vehicles, both
 *     with a view in range, with equal groups.
 *   Class.  SEARCHER: a vehicle K21 would search.  STANDING: its view is in range, it is no searcher, status !=
 *     FH_VEHICLE_GOAL_REACHED, the three coordinates of g_term are finite, and it is not wanted or d_skip[i] != 0.  (A vehicle the
 *     earlier chooser gave a goal, applied by fh_fleet_set_goals_device, is therefore standing with that goal; a skipped vehicle that
 *     is still GOAL_REACHED claims nothing.)  NONE: every other vehicle.
 *   Order, with no lists.  lower(i) = the number of searching peers k < i; standing(i) = the number of standing peers, of any index.
 *     No distance restriction and no cap: the far chooser has no r_max to prune by.  The searching members of a group form ONE chain
 *     by index, so searcher i is decided in pass lower(i) + 1.  lower(i) >= passes: FH_APART_UNSETTLED — mask 0, the bits of
 *     g_term, decided_pass = -1, the counts of a vehicle that is not searched; it keeps its status and is wanted again next period.
 *     There is no overflow flag, because nothing overflows.
 *   Claims of searcher i.  The g_term of every standing peer, and the d_goals[k] of every searching peer k < i with d_mask[k] == 1 (an
 *     earlier launch of the same call wrote them; a lower peer that found nothing, and one that is UNSETTLED, claim nothing).
 *   Claimed block.  G2(b, c) = the block-gap distance of K21 (the expression of D2 and E2) from the claim point c.  A target
 *     block of the vehicle is CLAIMED iff G2(b, c) < r_spread r_spread for some claim c: a claim excludes whole blocks, as r_avoid does
 *     there.  Claims remove targets, never links: the flood crosses a claimed block as before.
 *   Choice.  K21's, the smallest (hops, D2, b), over the target blocks in some level that are not claimed; in the chosen
 *     block that header's voxel choice, the smallest (d2, c).
 *   Record.  The first 64 bytes are K21's record, field for field, with targets = the target blocks of the vehicle, claimed or not, and
 *     reachable = those in some level and not claimed.  group as above; decided_pass: 0 for no searcher, 1 .. passes, -1 for
 *     UNSETTLED; lower, standing as above; claims = standing + the lower peers with mask 1 (UNSETTLED: standing); claimed = the target
 *     blocks of the vehicle that are claimed, reached or not; reserved = 0.  A vehicle that is no searcher has decided_pass = lower =
 *     standing = claims = claimed = 0 beside K21's fields for a vehicle that is not searched.  flags: K21's |
 *     FH_APART_UNSETTLED | FH_APART_CLAIMED (searched, nothing chosen, claimed > 0).
 *   Every byte of d_goals, d_mask and d_records is written by every call.
 *   Consequences.  (a) Where no searcher has a peer, d_goals, d_mask and the first 64 bytes of every record are K21's.
 *     (b) With passes > the largest lower: no two peers are given goals nearer than r_spread, and no goal lies within r_spread of a
 *     standing peer's g_term.  Both by monotony of the gap: a goal q lies in its block, so per axis |q - c| >= gap(c), and
 *     subtraction, squaring and summation are monotone; G2 >= r_spread r_spread then gives s2(q, c) >= r_spread r_spread.
 *
 * KNOWN LIMITS.  The vehicle index decides who yields.  A claim removes whole blocks, so a small scene with one far region serves
 * one teammate per period.  A team of m stranded members needs m passes.  Every vehicle's count scans all n vehicles in chunks of 64,
 * as K16's scan does.  Still no gain in the far choice. */
#ifndef FASTERHIP_APART_H
#define FASTERHIP_APART_H
#include "fasterhip.h"
#include "fasterhip_frontier.h"
#include "fasterhip_reach.h"
#ifdef __cplusplus
extern "C" {
#endif

enum {
  FH_APART_UNSETTLED = 256, /* fh_apart_record.flags, beside K21's: lower >= passes, not searched              */
  FH_APART_CLAIMED = 512    /*                             searched, nothing chosen, and claimed > 0                                 */
};
enum { FH_APART_MAX_PASSES = 64, FH_APART_DEFAULT_PASSES = 8 };
enum { FH_APART_SKIPPED = 128 };   /* d_skip[i] != 0, nothing searched (K21's bit)                                                            */
enum { FH_APART_MAX_WORDS = 512 }; /* words of 64 blocks that the blocks of the lattice may need (K21's cap)                                 */

typedef struct fh_apart_params { /* 96 B: the first 64 bytes are K21's params, its reserved fields 0 */
  double r_avoid;
  double z_lo;
  double z_hi;
  double reserved_d;
  int32_t want;
  int32_t max_hops;
  int32_t block;
  int32_t reserved[5];
  double r_spread;   /* no target block with G2 < r_spread * r_spread around a claim; finite and > 0                                 */
  int32_t passes;    /* 1 .. FH_APART_MAX_PASSES                                                                                */
  int32_t reserved_tail[5];
} fh_apart_params;

typedef struct fh_apart_record { /* 96 B: the first 64 bytes are laid out as K21's record */
  int32_t flags;        /* K21's | FH_APART_SKIPPED | FH_APART_UNSETTLED | FH_APART_CLAIMED                                */
  int32_t view;
  int32_t cell;
  int32_t block_cell;
  int32_t hops;
  int32_t targets;      /* the target blocks of the vehicle, claimed or not                                                          */
  int32_t reachable;    /* those in some level and not claimed                                                                       */
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
} fh_apart_record;

/* The bytes of d_work: K21's workspace, n_views * 4 * W * 8 + ((n_views + 63) & ~63) with W the words of a bitmap of blocks, +
 * ((n + 63) & ~63) class bytes + n int32 groups + n int32 `lower`; 0 where K21's is 0 (a null grid, a dimension < 1, a block outside
 * 1..16, W > FH_APART_MAX_WORDS, n_views < 1) or n < 0. */
size_t fh_apart_work_bytes(const struct fh_voxel_grid* grid, int block, int n_views, int n);

/* The arguments of K21's entry point with d_group [n_views] int32 or NULL after d_skip, and d_records [n] fh_apart_record.
 * d_work: work_bytes >= fh_apart_work_bytes(grid, par->block, n_views, n) of device memory, 8-byte aligned; what it holds before
 * the call is not read.  On `stream` (a hipStream_t, NULL: the default stream), asynchronous, on the device that owns d_records: the
 * summary stage of K21 as it is; a thread per vehicle for the class bytes and groups; a wavefront per vehicle that scans
 * all n class bytes and groups in chunks of 64 and counts lower and standing, and writes the outputs of every vehicle that no pass
 * decides; then per pass a workgroup of 256 per vehicle, which returns at once unless lower == pass - 1: it scans the n vehicles in
 * chunks of 256, takes the blocks its claims cover out of T in LDS (the number of claims is not bounded), and floods as
 * K21 does.  No atomics on global memory, no kernel waits for another wavefront.  DETERMINISTIC: a launch reads of
 * other vehicles only what earlier launches wrote.
 * FH_ERR_ARG, checked in this order, all before the first call of the runtime: K21's clauses from par == NULL to
 * W > FH_APART_MAX_WORDS, in its order; r_spread NaN, infinite or <= 0; passes < 1 or > FH_APART_MAX_PASSES; work_bytes <
 * fh_apart_work_bytes.  Then FH_OK for n == 0, then FH_ERR_ARG for a null d_work, d_flags, d_vehicles, d_goals, d_mask or
 * d_records.  d_view_of, d_skip and d_group may be NULL.  FH_ERR_DEVICE: d_records is no device memory, or a launch failed.  Every
 * index the kernels use comes from a value they have checked. */
int fh_apart_goals_device(void* stream, const fh_apart_params* par, const struct fh_voxel_grid* map_grid,
                               const unsigned* d_map_bits, const struct fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride,
                               const int32_t* d_view_of, int n_views, const int32_t* d_skip, const int32_t* d_group,
                               const fh_vehicle* d_vehicles, int n, void* d_work, size_t work_bytes, double* d_goals, int32_t* d_mask,
                               fh_apart_record* d_records);

#ifdef __cplusplus
}
#endif
#endif /* FASTERHIP_APART_H */

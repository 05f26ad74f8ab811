/* fasterhip_bid.h: TEAM GOALS BY BIDS — THE BEST OFFER WINS A CONTESTED FRONTIER.  The two choosers for a team (K16: point claims, K18:
 * claims as regions, a goal worth gain - hop_cost * hops) let the vehicle index decide who yields: the lower index chooses first, however
 * far its way is, a vehicle waits for every lower peer in reach, and a chain of L lower peers needs L passes.  The entry point of this
 * header (K20) has K18's arguments, K18's search (flood, gain, cover, claims as regions) and K18's outputs, and orders its rounds by
 * BIDS: every undecided vehicle makes an offer, the best chosen cell of its search under the claims so far; an offer that beats the offer
 * of every undecided rival is final in that round; the others search again under the new claims.  This is the greedy assignment of
 * coordinated exploration (Burgard et al.: fix the best (vehicle, goal) pair, discount the others, repeat) in parallel rounds: offers
 * never improve as claims grow (a claim only removes candidates and unknown voxels, and the flood does not see claims), so a local
 * maximum is a global one among everybody it could still meet.  A closed period is
 *     sense -> observe -> [link] -> BID GOALS -> fh_fleet_set_goals_device -> replan -> next goals
 * A pure measurement: no entry point, struct or kernel of the other headers changes and FH_ABI_VERSION stays.  C99 / C++11, includes
 * fasterhip.h, fasterhip_frontier.h and fasterhip_reach.h and names no header of another chooser; the constants it shares with them are
 * carried under names of its own, with the same values (tests/test_bid_abi.py compares them): FH_BID_OVERFLOW, UNSETTLED, CLAIMED,
 * ALL_POOR, MAX_PASSES, DEFAULT_PASSES, MAX_RADIUS and MAX_HOP_COST are K18's.  FH_BID_LIST is 64, twice K18's: a lane of a wavefront
 * per listed vehicle.
 *
 * THE MODEL (tests/bid_model.py restates it in Python on top of the models of the choosers before it; the kernels are compared with
 * that in every byte).  IEEE double, no fused multiply-add, every squared length summed x, y, z from the left of other - own, every
 * radius squared once on the host; gains, utilities and offers are integer arithmetic.
 *   Kept from K18, word for word.  Views, wanted, eligible, start cell, box, box cap, passable, flood, candidate, groups, peers, classes
 *     (searcher, standing, none); standing claims and the interaction radius r_int, reach = (r_max + r_max) + r_int and near = r_max +
 *     r_int; the claim voxel, covered, gain, utility, poor and the choice (the largest utility of the candidates in some level that are
 *     not claimed and not poor, then the smallest (hops, d2, cell)); CLAIMED, ALL_POOR; the outputs of a vehicle that is not searched.
 *   Lists of searcher i.  RIVALS: the peers k != i, BELOW OR ABOVE i, of class searcher with d2(pos_k, pos_i) < reach * reach.  The sum
 *     (x, y, z from the left) of the squares of other - own has the same bits in both directions, so k lists i iff i lists k.  STANDING
 *     CLAIMS: K16's (class standing, d2(g_term_k, pos_i) < near * near).  `rivals` and `standing` are exact sizes.  OVERFLOW iff
 *     rivals + standing > FH_BID_LIST: decided in round 0 with K16's outputs for it; an overflowed vehicle never bids and claims nothing.
 *   Round p = 1 .. passes.  Nothing a round decides is seen by that same round.
 *     Offer.  The claims of an undecided searcher i in round p are the g_term of its standing claims and the d_goals of its listed
 *       rivals k with 1 <= decided_pass_k < p and d_mask_k == 1.  Its offer is K18's search under those claims: a chosen cell with its
 *       (utility, hops), or none.  The offer is a function of the claims: a vehicle whose claims are those of its last search keeps that
 *       offer and is not searched again.
 *     searches.  In round 1 every undecided searcher is searched; in round p > 1 it is searched iff some listed rival has decided_pass
 *       == p - 1 and d_mask == 1.  `searches` counts these; a vehicle that is not searched has 0.
 *     Settle.  An undecided i without an offer is decided in round p with what its search wrote: d_mask 0, it claims nothing.  An
 *       undecided i with an offer is decided in round p iff its offer BEATS the round-p offer of every listed rival that was undecided
 *       at the start of round p and has an offer.  a beats b iff a has the larger utility, then the fewer hops, then the smaller vehicle
 *       index (K17's 64-bit key utility * 65536 + 65535 - hops: the larger key, then the smaller index; d2 is not compared, it is
 *       measured from different vehicles).  A rival that is decided, overflowed or without an offer blocks nobody.
 *     Output.  A decided vehicle has the outputs of its last search, decided_pass = p, `claims` as K18 counts them for that search.
 *   After the last round.  A searcher still undecided gets FH_BID_UNSETTLED and K16's outputs for it: d_mask 0, the bits of g_term,
 *     decided_pass = -1, claims = standing, the counts of a vehicle that is not searched; it keeps `rivals`, and `searches` as counted.
 *     Its status is what it was, so the next period wants it again.
 *   Every byte of all three outputs is written by every call.
 *   CONSEQUENCES (tests/test_bid_model.py holds them).
 *     1. Progress.  In every round the best offer of each connected set of undecided rivals is decided.
 *     2. Greedy.  With no UNSETTLED vehicle, d_goals, d_mask and every record word except decided_pass and searches equal those of the
 *        sequential rule: search every undecided searcher under the goals decided so far, decide the one whose offer beats all others
 *        (a searcher without an offer at once), repeat.
 *     3. Reduction A.  Where no searcher has a rival and no list exceeds 32, d_goals, d_mask and every record word except `searches` are
 *        those of K18's entry point.
 *     4. Relabelling.  Renumbering the vehicles of a case in which no two rival offers tie in (utility, hops) permutes the outputs and
 *        changes nothing else except decided_pass.  K18 does not have this property.
 *
 * KNOWN LIMITS.  A vehicle is searched once per round in which a listed rival wins a goal: more work than K18's one search.  Ties still
 * fall to the index.  The launches of all `passes` rounds are paid whether or not anybody is left.  Every searcher scans all n vehicles
 * (no broad phase).  No occlusion, and both balls are clipped to the box.  The goal of a rival whose replan then fails stays a claim,
 * point and ball, for that period. */
#ifndef FASTERHIP_BID_H
#define FASTERHIP_BID_H
#include "fasterhip.h"
#include "fasterhip_frontier.h"
#include "fasterhip_reach.h"
#ifdef __cplusplus
extern "C" {
#endif

enum {
  FH_BID_OVERFLOW = 128,  /* fh_bid_record.flags, beside those of fh_reach_record: rivals + standing > FH_BID_LIST, not searched, no bid  */
  FH_BID_UNSETTLED = 256, /*                        a rival's offer still beat this vehicle's after the last round                         */
  FH_BID_CLAIMED = 512,   /*                        searched, nothing chosen, and claimed > 0                                              */
  FH_BID_ALL_POOR = 1024  /*                        searched, candidates that are not claimed were reached, all of them poor               */
};
enum { FH_BID_LIST = 64, FH_BID_MAX_PASSES = 64, FH_BID_DEFAULT_PASSES = 8, FH_BID_MAX_RADIUS = 31, FH_BID_MAX_HOP_COST = 16384 };

typedef struct fh_bid_params { /* 80 B: laid out as K18's params, with K18's ranges and defaults */
  double r_max;         /* as fh_reach_params                                                                                        */
  double r_avoid;
  double z_lo;
  double z_hi;
  int32_t want;
  int32_t max_hops;
  double r_spread;      /* no candidate with s2 < r_spread * r_spread around a claim; finite and > 0                                 */
  int32_t passes;       /* the rounds: 1 .. FH_BID_MAX_PASSES                                                                        */
  int32_t gain_radius;  /* g, in voxels of the views' lattice: 0 .. FH_BID_MAX_RADIUS                                                */
  int32_t hop_cost;     /* unknown voxels that one step of the flood is worth: 0 .. FH_BID_MAX_HOP_COST                              */
  int32_t min_gain;     /* a candidate with a smaller gain is poor; >= 0                                                             */
  int32_t claim_radius; /* the ball, in voxels, that a claim covers: 0 .. FH_BID_MAX_RADIUS; -1: claims cover nothing                */
  int32_t reserved[3];
} fh_bid_params;

typedef struct fh_bid_record { /* 96 B: laid out as K18's record; two of its words have other names */
  int32_t flags;        /* fh_reach_record's | FH_BID_OVERFLOW | UNSETTLED | CLAIMED | ALL_POOR                                      */
  int32_t view;
  int32_t cell;         /* the chosen cell of the lattice, -1: none                                                                  */
  int32_t hops;         /* its level, -1: none                                                                                       */
  int32_t candidates;   /* claimed or not                                                                                            */
  int32_t reachable;    /* in some level and not claimed                                                                             */
  int32_t reached;
  int32_t levels;
  double d2;            /* of the chosen cell, +inf: none                                                                            */
  int32_t group;        /* group(i); 0 without a view in range                                                                       */
  int32_t decided_pass; /* 0: not a searcher, or OVERFLOW; 1 .. passes: the round that made its offer final; -1: UNSETTLED           */
  int32_t rivals;       /* the size of the list of rivals, below and above, also beyond FH_BID_LIST                                  */
  int32_t claims;       /* standing + the rivals decided before its last search with d_mask == 1 (OVERFLOW, UNSETTLED: standing)     */
  int32_t claimed;      /* candidates, reachable or not, within r_spread of a claim                                                  */
  int32_t searches;     /* the rounds in which it was searched; 0: not searched                                                      */
  int32_t gain;         /* of the chosen cell, covered voxels not counted; -1: none                                                  */
  int32_t utility;      /* of the chosen cell, 0: none                                                                               */
  int32_t poor;         /* candidates in some level, not claimed, with a gain below min_gain                                         */
  int32_t best_gain;    /* the largest gain of a candidate in some level that is not claimed, poor ones included; -1: none           */
  int32_t covered;      /* unknown voxels of the box inside the ball of at least one claim, each counted once                        */
  int32_t reserved[3];  /* 0                                                                                                         */
} fh_bid_record;

/* The bytes of d_work for n vehicles: 0 for n <= 0, else
 *     ((n + 63) & ~63) + n * FH_BID_LIST * 4 + n * 8 + 2 * n * 4
 * a class byte per vehicle, rounded up to a multiple of 64; a row of FH_BID_LIST int32 per vehicle; an offer of two int32 per vehicle;
 * and the "decided in round" word of every vehicle twice, one buffer read and one written by each round. */
size_t fh_bid_work_bytes(int n);

/* d_goals [n][3], d_mask [n] int32 and d_records [n] as above, in the shape fh_fleet_set_goals_device takes.  The arguments after par
 * are exactly those of K18's entry point: map_grid, d_map_bits, grid, d_flags, view_stride, d_view_of, n_views, d_vehicles as for
 * fh_reach_goals_device; d_group [n_views] int32 or NULL; d_work: device memory of this call alone, aligned to 4 bytes, work_bytes >=
 * fh_bid_work_bytes(n); what it holds afterwards has no meaning.  2 + 2 * passes launches on `stream` (a hipStream_t, NULL: the default
 * stream), asynchronous, on the device that owns d_records: K16's class kernel, a thread per vehicle; a wavefront per vehicle that scans
 * all n vehicles for the two lists; then per round a workgroup of 256 per vehicle, which returns at once unless the vehicle is undecided
 * and due a search, and a wavefront per vehicle that settles the round: lane j reads the offer of the vehicle in slot j of the row, one
 * ballot decides.  No atomics, no kernel waits for another wavefront.  DETERMINISTIC: the "decided in round" words are double-buffered,
 * so no launch reads a word that another workgroup of the same launch writes; integer counts and the extremum of a total order.
 * FH_ERR_ARG, checked in this order, all before the first call of the runtime: the clauses of fh_reach_goals_device from par == NULL to
 * n < 0, in its order; r_spread NaN, infinite or <= 0; passes < 1 or > FH_BID_MAX_PASSES; gain_radius < 0 or > FH_BID_MAX_RADIUS;
 * hop_cost < 0 or > FH_BID_MAX_HOP_COST; min_gain < 0; claim_radius < -1 or > FH_BID_MAX_RADIUS.  Then FH_OK for n == 0, then
 * FH_ERR_ARG for a null d_flags, d_vehicles, d_goals, d_mask or d_records; a null d_work; work_bytes too small.  d_view_of and d_group
 * may be NULL.  FH_ERR_DEVICE: d_records is no device memory, or a launch failed.  Every index the kernels use comes from a value they
 * have checked. */
int fh_bid_goals_device(void* stream, const fh_bid_params* par, const struct fh_voxel_grid* map_grid, const unsigned* d_map_bits,
                        const struct fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of,
                        int n_views, const int32_t* d_group, const fh_vehicle* d_vehicles, int n, void* d_work, size_t work_bytes,
                        double* d_goals, int32_t* d_mask, fh_bid_record* d_records);

#ifdef __cplusplus
}
#endif
#endif /* FASTERHIP_BID_H */

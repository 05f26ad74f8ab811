/* fasterhip_traffic_timed.h: TIME-AWARE TRAFFIC.  fasterhip_traffic.h shows vehicle i every sample of every other plan within `range`
 * of where vehicle i stands now, whatever the instant of that sample: two plans that pass one point twenty instants apart wall each
 * other off.  Every fleet plan is indexed by the same clock (state j of every plan is j DC from now), so this header asks instead:
 * will we be near each other AT THE SAME TIME?  A sample of vehicle k at instant j is shown to vehicle i only if i's own committed plan
 * is within `range` of it at instant j, or within a window of sampled instants around j.  Slots, points, words and the two rules are
 * those of fasterhip_traffic.h; what changes is which bits are set.  No existing entry point, kernel or struct changes,
 * FH_ABI_VERSION stays.  C99 / C++11, includes fasterhip_traffic.h.
 *
 * THE MODEL.  Everything is IEEE double, no fused multiply-add, squared distances, no roots, as in fasterhip_traffic.h
 * (tests/traffic_timed_model.py restates it in numpy, brute force over all (i, k, s, s'), and the kernels are compared with that byte
 * for byte).  S = samples, pps = hull > 0 ? 7 : 1.
 *   Instants.  Sample s < S is the instant j = first_instant + s * stride, computed in 64 bits.  The instant of the start state A of a
 *     replan is delta_t - 1: the states before it cannot be changed by the replan, so a caller passes first_instant = delta_t - 1.
 *   Shows.  Sample s of vehicle k SHOWS iff the plan extent of record k is good (not head < 0, size < 0 or head + size > max_states: the
 *     separation header's FH_SEP_BAD_PLAN rule, decided before any plan state is read), plan_size >= 1, and all three coordinates of
 *         c[k][s] = d_plans[k * max_states + head_k + min(j, size_k - 1)].pos
 *     are finite.  A plan that has ended stands at its last state.
 *   Slots and points.  Exactly fasterhip_traffic.h's: sample s of vehicle k owns the cloud points first_point + (k S + s) pps + o,
 *     o < pps.  A sample that shows writes the centre, then +x, -x, +y, -y, +z, -z at `hull`, each one double add or subtract on one
 *     coordinate.  A sample that does not show writes (0, 0, 0) to all its points.  Every traffic point is written by every call.
 *   Bits.  All points of sample (k, s) share one decision.  In row i they are set iff all of these hold:
 *       (k, s) shows;
 *       k != i;
 *       the rule allows it: FH_TRAFFIC_ALL, or FH_TRAFFIC_YIELD_TO_LOWER and k < i;
 *       there is an s' with max(0, s - window) <= s' <= min(S - 1, s + window) such that sample (i, s') shows and d2 < range * range
 *         (strict), with d = c[k][s] - c[i][s'] per axis and d2 = dx dx + dy dy + dz dz, the three products summed from left to right.
 *     window >= 0 counts SAMPLES, not states; any value >= S - 1 means "any sampled instant of my plan".  d_vehicles[i].state is not
 *     read.  An observer none of whose samples show has an all-zero row.
 *   Words.  As in fasterhip_traffic.h: the traffic words [first_point / 32, ceil((first_point + n S pps) / 32)) of every row are written
 *     WHOLE, bits past the last traffic point are zero, nothing else is touched; first_point is a multiple of 32.
 *   Limit.  samples <= FH_TRAFFIC_TIMED_MAX_SAMPLES: the mask kernel keeps the observer's samples on chip.
 * Two properties follow.  The bits are monotone in `window`: the set for w is a subset of the set for w + 1, and it is constant from
 * S - 1 on.  With S = 1, first_instant = 0, good non-empty plans and state.pos bitwise equal to the first plan state, cloud and masks
 * equal fh_fleet_traffic_device's with the same range, hull, rule and first_point, byte for byte.
 *
 * KNOWN LIMITS.
 *   The match is against the observer's PREVIOUS plan: the one it committed last cycle, not the one it is about to compute.
 *   A vehicle that retimes itself (slows down, takes another way round) can meet what it was not shown; that is what the commit check
 *     of fasterhip_check.h is for.
 *   Shown points remain static obstacles for the whole horizon of the planner, as in fasterhip_traffic.h.
 *   Memory is n rows of ceil(n S pps / 32) words beside the static ones, as in fasterhip_traffic.h. */
#ifndef FASTERHIP_TRAFFIC_TIMED_H
#define FASTERHIP_TRAFFIC_TIMED_H
#include "fasterhip_traffic.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FH_TRAFFIC_TIMED_MAX_SAMPLES 512 /* the largest fh_traffic_timed_params.samples */

typedef struct fh_traffic_timed_params { /* 48 B */
  double range;          /* sample (k, s) is shown to vehicle i when a sample (i, s') inside the window has d2 < range * range (strict) */
  double hull;           /* 0: one point per sample.  > 0: seven: centre, +x, -x, +y, -y, +z, -z at `hull`, in that order               */
  int32_t samples;       /* 1 <= S <= FH_TRAFFIC_TIMED_MAX_SAMPLES samples per vehicle                                                 */
  int32_t stride;        /* sample s is the instant j = first_instant + s * stride (>= 1)                                              */
  int32_t rule;          /* FH_TRAFFIC_ALL: i sees every k != i.  FH_TRAFFIC_YIELD_TO_LOWER: i sees k < i only                         */
  int32_t first_point;   /* cloud index of the first traffic point; a multiple of 32                                                   */
  int32_t first_instant; /* the instant of sample 0 (>= 0); delta_t - 1 is the start state of a replan                                 */
  int32_t window;        /* |s - s'| <= window, in samples (>= 0); >= S - 1: any sampled instant of the observer's plan                 */
  int32_t reserved[2];
} fh_traffic_timed_params;

/* Writes the traffic points d_cloud_xyz[3 first_point .. 3 (first_point + n S pps)) and the traffic words of the n rows of
 * d_point_mask ([n][mask_words] words).  Two launches on the context's stream (the points with a compact record per sample, then the
 * words: one wavefront per row and 64 chunks of 64 samples, the row's own samples staged on chip), asynchronous; device pointers.
 * Written besides: the working buffers of the context that fh_fleet_traffic_device uses; calls of both may alternate on one context.
 * FH_ERR_ARG, checked in this order:
 *    1. ctx == NULL or par == NULL;
 *    2. range NaN, infinite or <= 0;
 *    3. hull NaN, infinite or negative;
 *    4. samples < 1 or samples > FH_TRAFFIC_TIMED_MAX_SAMPLES;
 *    5. stride < 1;
 *    6. rule not one of the two;
 *    7. first_point < 0 or not a multiple of 32;
 *    8. first_instant < 0;
 *    9. window < 0;
 *   10. n < 0 or max_states < 1;
 *   11. first_point + n S pps above n_cloud or above mask_words * 32 (computed in 64 bits).
 * Then FH_ERR_DEVICE without a device (there is no CPU path), FH_OK for n == 0, and FH_ERR_ARG for a null d_vehicles, d_plans,
 * d_cloud_xyz or d_point_mask.  Every index the kernels use comes from a record they have checked: a wrong vehicle record gives zeros
 * and clear bits, never a read outside the arrays. */
int fh_fleet_traffic_timed_device(fh_ctx* ctx, const fh_traffic_timed_params* par, const fh_vehicle* d_vehicles, const fh_state* d_plans,
                                  int n, int max_states, double* d_cloud_xyz, int n_cloud, uint32_t* d_point_mask, int mask_words);

#ifdef __cplusplus
}
#endif
#endif /* FASTERHIP_TRAFFIC_TIMED_H */

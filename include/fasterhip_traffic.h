/* fasterhip_traffic.h: the vehicles of a fleet (include/fasterhip.h) AVOID EACH OTHER.  fasterhip_separation.h measures how near the
 * committed plans come to each other; this header closes the gap with the mechanism a vehicle already has for seeing something the
 * others do not: occupied space per view (fasterhip_occupancy.h), a bit mask per view over the points of the shared cloud.  Every cycle
 * the committed plans of the other vehicles become points at the tail of the cloud, and in row i of the masks exactly the bits of the
 * points vehicle i has to keep clear of are set.  The view path search, both corridor decompositions and the safe corridor honour the
 * masks as they are: no existing entry point, kernel or struct changes, FH_ABI_VERSION stays.  C99 / C++11, includes fasterhip.h.
 *
 * THE MODEL.  Everything is IEEE double, no fused multiply-add (tests/traffic_model.py restates it in numpy, brute force over all
 * (i, k, s), and the kernels are compared with that byte for byte).  Squared distances are decided and no root is taken, as in
 * fasterhip_audit.h and fasterhip_separation.h.  With S = samples and pps = hull > 0 ? 7 : 1 points per sample:
 *   Slots.  Sample s < S of vehicle k < n owns the cloud points first_point + (k S + s) pps + o, o < pps.
 *   A sample SHOWS iff the plan extent of record k is good (not head < 0, size < 0 or head + size > max_states: the separation header's
 *     FH_SEP_BAD_PLAN rule, decided before any plan state is read), plan_size >= 1, and all three coordinates of
 *         c = d_plans[k * max_states + head_k + min(s * stride, size_k - 1)].pos
 *     are finite.  A vehicle whose plan has ended stands at its last state, as in the separation model and in
 *     fh_fleet_next_goals_device.
 *   Points.  A sample that shows writes c to its point, and with a hull the seven points c, c + hull e_x, c - hull e_x, c + hull e_y,
 *     c - hull e_y, c + hull e_z, c - hull e_z in that order, each one double add or subtract on one coordinate.  A sample that does not
 *     show writes (0, 0, 0) to all its points.  Every traffic point of the cloud is written by every call.
 *   Bits.  Row i of the masks is vehicle i's: there are n rows, a view per vehicle.  All points of a sample share one decision: their
 *     bits in row i are set iff the sample shows, k != i, rule == FH_TRAFFIC_ALL or k < i, all three coordinates of
 *     d_vehicles[i].state.pos are finite, and d2 < range * range (strict) with
 *         d2 = dx dx + dy dy + dz dz,   d = c - state_i.pos per axis, the three products summed x, y, z from left to right.
 *   Words.  Traffic owns the words [first_point / 32, ceil((first_point + n S pps) / 32)) of every row.  Every call writes these words
 *     WHOLE, not ORed: plans move, so last cycle's bits must go.  Bits past the last traffic point in the last word are zero.  Every
 *     other word of a row and every cloud point below first_point is not touched; that is why first_point is a multiple of 32:
 *     fh_fleet_observe_device keeps ORing into the words below it (called with n_cloud = first_point or less).
 *
 * KNOWN LIMITS.
 *   The others are static obstacles over the sampled horizon: conservative in space and blind to time.  A vehicle keeps clear of where
 *     another one will be at any sampled instant, whenever it would be there itself.
 *   With FH_TRAFFIC_ALL two vehicles may both give way, and do so again next cycle.  FH_TRAFFIC_YIELD_TO_LOWER breaks the symmetry at
 *     the price of the lower index never yielding.
 *   A neighbour whose inflated points cover a vehicle's start makes that vehicle's path search fail, and it keeps its plan: what an
 *     occupied start does today.
 *   Memory is n rows of ceil(n S pps / 32) words beside the static ones.  Fleets too large for that need the team views of the
 *     occupancy layer, which this entry point does not serve. */
#ifndef FASTERHIP_TRAFFIC_H
#define FASTERHIP_TRAFFIC_H
#include "fasterhip.h"
#ifdef __cplusplus
extern "C" {
#endif

enum { FH_TRAFFIC_ALL = 0, FH_TRAFFIC_YIELD_TO_LOWER = 1 }; /* fh_traffic_params.rule */

typedef struct fh_traffic_params { /* 48 B */
  double range;        /* a sample of another vehicle is shown to vehicle i when d2 < range * range (strict)          */
  double hull;         /* 0: one point per sample.  > 0: seven: centre, +x, -x, +y, -y, +z, -z at `hull`, in that order */
  int32_t samples;     /* S >= 1 samples per vehicle                                                                  */
  int32_t stride;      /* sample s is the instant j = s * stride (>= 1)                                               */
  int32_t rule;        /* FH_TRAFFIC_ALL: i sees every k != i.  FH_TRAFFIC_YIELD_TO_LOWER: i sees k < i only          */
  int32_t first_point; /* cloud index of the first traffic point; a multiple of 32                                    */
  int32_t reserved[4];
} fh_traffic_params;

/* Writes the traffic points d_cloud_xyz[3 first_point .. 3 (first_point + n S pps)) and the traffic words of the n rows of
 * d_point_mask ([n][mask_words] words).  Two launches on the context's stream (the points with a compact record per sample, then the
 * words: one wavefront per row and 64 chunks of 64 samples), asynchronous; device pointers.  Written besides: working buffers of the
 * context.  FH_ERR_ARG, checked in this order after a null context: par == NULL; range NaN, infinite or <= 0; hull NaN, infinite or
 * negative; samples < 1; stride < 1; rule not one of the two; first_point < 0 or not a multiple of 32; n < 0; max_states < 1;
 * first_point + n S pps above n_cloud or above mask_words * 32 (computed in 64 bits).  Then FH_ERR_DEVICE without a device (there is no
 * CPU path), FH_OK for n == 0, and FH_ERR_ARG for a null d_vehicles, d_plans, d_cloud_xyz or d_point_mask.  Every index the kernels use
 * comes from a record they have checked: a wrong vehicle record gives zeros and clear bits, never a read outside the arrays. */
int fh_fleet_traffic_device(fh_ctx* ctx, const fh_traffic_params* par, const fh_vehicle* d_vehicles, const fh_state* d_plans, int n,
                            int max_states, double* d_cloud_xyz, int n_cloud, uint32_t* d_point_mask, int mask_words);

#ifdef __cplusplus
}
#endif
#endif /* FASTERHIP_TRAFFIC_H */

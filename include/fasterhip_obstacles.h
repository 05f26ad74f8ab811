/* fasterhip_obstacles.h: MOVING OBSTACLES.  Everything a fleet vehicle avoids is a point of the static cloud or the committed plan of
 * another fleet member (fasterhip_traffic.h, fasterhip_traffic_timed.h).  This header adds things that move and are no fleet member, a
 * person, a door, a foreign vehicle: each is a ball that flies a straight line at a constant velocity.  The mechanism is the traffic's:
 * samples of the obstacle's predicted positions are written as points behind the cloud, and in the mask row of vehicle i the bits of
 * those samples are set that i's own committed plan comes near AT THE SAME INSTANT (or within a window of sampled instants around it),
 * once i has detected the obstacle.  A second entry point measures what the fleet then flies against the obstacles' positions at the
 * same instant.  No existing entry point, kernel or struct changes, FH_ABI_VERSION stays.  C99 / C++11, includes
 * fasterhip_traffic_timed.h.
 *
 * THE MODEL.  Everything is IEEE double, no fused multiply-add, squared distances, no roots, every comparison strict unless it says
 * otherwise (tests/obstacle_model.py restates it in numpy, brute force over all (i, o, s, s') and all (i, j, o), and the kernels are
 * compared with that byte for byte).  d2(d) = dx dx + dy dy + dz dz, the three products summed from left to right.
 *   Valid.  Obstacle o is VALID iff FH_OBSTACLE_ON is set in its flags, p0[0..2], v[0..2] and radius are finite, and radius >= 0.
 *   The clock.  State j of every plan is j dc from now, and now is tick0 dc after the obstacle records were written: at instant j
 *         tau = (double)(tick0 + j) * dc       (the sum in 64 bits, 0 <= tick0 <= FH_OBSTACLE_MAX_TICK; one conversion, one product)
 *         c[o][j] = p0 + v * tau per axis      (the product is rounded, then the sum is rounded)
 *     and now[o] = c[o][0].
 *   Slots.  S = samples, pps = points (1 or 7).  Sample s < S of obstacle o < m is the instant j = first_instant + s * stride, computed
 *     in 64 bits.  It owns the cloud points first_point + (o S + s) pps + q, q < pps.
 *   Shows.  Sample (o, s) SHOWS iff o is valid and all three coordinates of c[o][j] are finite.  A sample that shows writes its centre;
 *     with points = 7 it writes the centre, then +x, -x, +y, -y, +z, -z at the obstacle's own radius, each one double add or subtract
 *     on one coordinate.  A sample that does not show writes (0, 0, 0) to all its points.  Every owned point is written by every call.
 *   Observer.  c[i][s'] and whether sample (i, s') of vehicle i shows are exactly fasterhip_traffic_timed.h's "Shows" for vehicle i,
 *     with this record's first_instant and stride: a good plan extent, plan_size >= 1, the state at min(j, size - 1), finite.
 *   Detected.  detected(i, o) holds iff r_detect == 0 (detection is off, everything is known), or now[o] and d_vehicles[i].state.pos
 *     are finite and d2(now[o] - pos_i) < r_detect * r_detect.
 *   Bits.  All points of sample (o, s) share one decision.  In row i they are set iff all of these hold:
 *       (o, s) shows;
 *       detected(i, o);
 *       there is an s' with max(0, s - window) <= s' <= min(S - 1, s + window) such that (i, s') shows and
 *         d2(c[o][s] - c[i][s']) < reach_o * reach_o, with reach_o = range + radius_o (one add, then one product).
 *   Words.  The words [first_point / 32, ceil((first_point + m S pps) / 32)) of every one of the n rows are written WHOLE, bits past the
 *     last owned point are zero, nothing else is touched; first_point is a multiple of 32.
 * Three properties follow.
 *   The bits are monotone in `window`: the set for w is a subset of the set for w + 1, and it is constant from S - 1 on.
 *   The bits are monotone in r_detect for r_detect > 0: a larger radius detects no less.
 *   With valid obstacles, v = +0, radius = 0, r_detect = 0 and points = 1, words and points equal what fh_fleet_traffic_timed_device
 *     (rule FH_TRAFFIC_ALL, hull 0, the same range, samples, stride, first_instant and window) writes for the rows 0 .. n - 1 of a
 *     fleet to which the obstacles are appended as vehicles n .. n + m - 1, each with a plan of one state at p0, when n S is a multiple
 *     of 32 and this call's first_point is that call's advanced by n S.  (p0 + 0 tau = p0 in every bit unless a coordinate is -0.)
 *
 * KNOWN LIMITS.
 *   Shown points are static obstacles for the whole horizon of the planner, as in fasterhip_traffic.h.
 *   The prediction is the truth: a constant velocity, known exactly.  Nothing estimates it and nothing doubts it.
 *   Detection is a ball around the vehicle; walls do not hide an obstacle.
 *   The match is against the observer's PREVIOUS plan, as in fasterhip_traffic_timed.h.
 *   Memory is n rows of ceil(m S pps / 32) words beside the others. */
#ifndef FASTERHIP_OBSTACLES_H
#define FASTERHIP_OBSTACLES_H
#include "fasterhip_traffic_timed.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FH_OBSTACLE_MAX_SAMPLES 512                /* the largest fh_obstacle_params.samples                                       */
#define FH_OBSTACLE_MAX_TICK (((int64_t)1) << 62) /* the largest tick0: tick0 + j stays inside 64 bits                             */
#define FH_OBSTACLE_AUDIT_CHUNK 64                 /* obstacles that fh_fleet_obstacle_audit_device stages on chip at a time        */

enum {                 /* fh_obstacle.flags */
  FH_OBSTACLE_ON = 1   /* the record is in use; a record without it is shown to nobody and measured against nothing                */
};

typedef struct fh_obstacle { /* 64 B */
  double p0[3];        /* where the centre was when the clock stood at 0                                                           */
  double v[3];         /* its velocity, per unit of dc's time                                                                      */
  double radius;       /* the ball around the centre (>= 0)                                                                        */
  int32_t flags;       /* FH_OBSTACLE_ON                                                                                           */
  int32_t reserved;
} fh_obstacle;

typedef struct fh_obstacle_params { /* 64 B */
  double range;          /* sample (o, s) is shown to vehicle i when a sample (i, s') inside the window has d2 < (range + radius_o)^2 */
  double r_detect;       /* 0: every obstacle is known to everyone.  > 0: to the vehicles with d2(now[o] - pos_i) < r_detect^2    */
  double dc;             /* the time between two states of a plan (> 0)                                                            */
  int32_t samples;       /* 1 <= S <= FH_OBSTACLE_MAX_SAMPLES samples per obstacle and per observer                                */
  int32_t stride;        /* sample s is the instant j = first_instant + s * stride (>= 1)                                          */
  int32_t points;        /* 1: one point per sample.  7: centre, +x, -x, +y, -y, +z, -z at the obstacle's radius, in that order    */
  int32_t first_point;   /* cloud index of the first owned point; a multiple of 32                                                 */
  int32_t first_instant; /* the instant of sample 0 (>= 0); delta_t - 1 is the start state of a replan                             */
  int32_t window;        /* |s - s'| <= window, in samples (>= 0); >= S - 1: any sampled instant of the observer's plan            */
  int32_t reserved[4];
} fh_obstacle_params;

/* Writes the points d_cloud_xyz[3 first_point .. 3 (first_point + m S pps)) and the owned words of the n rows of d_point_mask
 * ([n][mask_words] words).  Three launches on the context's stream (the obstacles' points with a compact record per sample, the
 * observers' samples as compact records, then the words: one wavefront per row and 64 chunks of 64 samples, the row's own samples
 * staged on chip), asynchronous; device pointers.  Written besides: working buffers of the context that no other entry point uses;
 * calls of this one and of the traffic entry points may alternate on one context.
 * FH_ERR_ARG, checked in this order:
 *    1. ctx == NULL or par == NULL;
 *    2. range NaN, infinite or <= 0;
 *    3. r_detect NaN, infinite or negative;
 *    4. dc NaN, infinite or <= 0;
 *    5. samples < 1 or samples > FH_OBSTACLE_MAX_SAMPLES;
 *    6. stride < 1;
 *    7. points neither 1 nor 7;
 *    8. first_point < 0 or not a multiple of 32;
 *    9. first_instant < 0;
 *   10. window < 0;
 *   11. n < 0, m < 0, max_states < 1, or n S above 2^31 - 1;
 *   12. tick0 < 0 or tick0 > FH_OBSTACLE_MAX_TICK;
 *   13. first_point + m S pps above n_cloud or above mask_words * 32 (computed in 64 bits).
 * Then FH_ERR_DEVICE without a device (there is no CPU path), FH_OK for n == 0 or m == 0 (nothing is written: with m == 0 no word and
 * no point is owned, with n == 0 there is no row), and FH_ERR_ARG for a null d_obstacles, d_vehicles, d_plans, d_cloud_xyz or
 * d_point_mask.  Every index the kernels use comes from a value they have checked: a wrong vehicle record gives an all-zero row, a
 * wrong obstacle record zeros and clear bits, never a read outside the arrays. */
int fh_fleet_obstacles_device(fh_ctx* ctx, const fh_obstacle_params* par, const fh_obstacle* d_obstacles, int m, int64_t tick0,
                              const fh_vehicle* d_vehicles, const fh_state* d_plans, int n, int max_states, double* d_cloud_xyz,
                              int n_cloud, uint32_t* d_point_mask, int mask_words);

/* THE AUDIT: what the fleet flies against where the obstacles are at the same instant.  A pure measurement: it writes d_out only.
 *   Tested states of vehicle i, FH_OBSTACLE_BAD_PLAN, FH_OBSTACLE_NOT_FINITE and n_tested are fasterhip_separation.h's, word for word:
 *     with head = d_vehicles[i].plan_head, size = .plan_size, mm = count > 0 ? min(count, size) : size: the positions
 *     d_plans[i * max_states + head + j].pos for j = 0, stride, 2 stride, ... < mm; n_tested = ceil(mm / stride).  A tested position with
 *     a coordinate that is not finite is skipped; it counts in n_tested and sets FH_OBSTACLE_NOT_FINITE.  head < 0, size < 0 or
 *     head + size > max_states, decided before any plan state is read, is FH_OBSTACLE_BAD_PLAN: n_tested = 0, n_hit = 0, the indexes
 *     are -1, min_d2 = +INFINITY and the flag is alone.  An empty plan is not bad: n_tested = 0.
 *   At a tested instant j with position p, every valid obstacle o whose c[o][j] (THE MODEL above) is finite gives d2(c[o][j] - p).
 *   The record.  min_d2 = the smallest d2 below +INFINITY over tested j and obstacles, +INFINITY when there is none (no obstacle, no
 *     instant); worst = the smallest tested j that attains it, worst_obstacle = the smallest o that attains it at that j (-1, -1).
 *     An obstacle HITS at j when d2 < hit_o * hit_o with hit_o = r + radius_o (one add, then one product; strict: a vehicle at exactly
 *     r + radius_o is no hit).  first = the smallest tested j with a hit, first_obstacle = the smallest o that hits at that j
 *     (-1, -1); n_hit = how many distinct obstacles hit at one tested instant at least; FH_OBSTACLE_HIT is set iff first >= 0.  Ties
 *     go to the smallest j, then to the smallest o: the minimum is of the total order (d2, j, o). */
enum {                        /* fh_plan_obstacle_audit.flags */
  FH_OBSTACLE_BAD_PLAN = 1,   /* the plan extent of the vehicle record does not fit max_states: nothing was read, the flag is alone */
  FH_OBSTACLE_NOT_FINITE = 4, /* a tested position has a coordinate that is not finite (it was skipped)                            */
  FH_OBSTACLE_HIT = 8         /* first >= 0: at a tested instant an obstacle is nearer than r + its radius                         */
};

typedef struct fh_obstacle_audit_params { /* 32 B */
  double r;              /* the vehicle's own radius: obstacle o hits when d2 < (r + radius_o)^2 (strict)                          */
  double dc;             /* the time between two states of a plan (> 0)                                                            */
  int32_t stride, count; /* tested j = 0, stride, 2 stride, ... < mm; mm = count > 0 ? min(count, size) : size                     */
  int32_t reserved[2];
} fh_obstacle_audit_params;

typedef struct fh_plan_obstacle_audit { /* 64 B */
  int32_t flags, n_tested;        /* n_tested = ceil(mm / stride)                                                                  */
  int32_t first, first_obstacle;  /* smallest tested j with a hit; the smallest obstacle that hits at that j                       */
  int32_t worst, worst_obstacle;  /* smallest tested j that attains min_d2; the smallest obstacle that attains it at that j        */
  int32_t n_hit, reserved;        /* distinct obstacles that hit at one tested j at least                                          */
  double min_d2;                  /* smallest d2 over tested j and obstacles; +INFINITY when there is none                         */
  double reserved_d[3];           /* zero                                                                                          */
} fh_plan_obstacle_audit;

/* d_out[i] = the record of vehicle i.  One launch on the context's stream (one wavefront per vehicle, the obstacles staged on chip
 * FH_OBSTACLE_AUDIT_CHUNK at a time, lanes over the tested instants), asynchronous; device pointers; d_out aligned to 16 bytes.
 * FH_ERR_ARG, checked in this order:
 *    1. ctx == NULL or par == NULL;
 *    2. r NaN, negative or infinite;
 *    3. dc NaN, infinite or <= 0;
 *    4. stride < 1;
 *    5. count < 0;
 *    6. n < 0, m < 0 or max_states < 1;
 *    7. tick0 < 0 or tick0 > FH_OBSTACLE_MAX_TICK.
 * Then FH_ERR_DEVICE without a device (there is no CPU path), FH_OK for n == 0, and FH_ERR_ARG for a null d_vehicles, d_plans or d_out,
 * or a null d_obstacles with m > 0.  With m == 0 every record is written: no obstacle, min_d2 = +INFINITY.  Every index the kernel uses
 * comes from a record it has checked. */
int fh_fleet_obstacle_audit_device(fh_ctx* ctx, const fh_obstacle_audit_params* par, const fh_obstacle* d_obstacles, int m, int64_t tick0,
                                   const fh_vehicle* d_vehicles, const fh_state* d_plans, int n, int max_states,
                                   fh_plan_obstacle_audit* d_out);

#ifdef __cplusplus
}
#endif
#endif /* FASTERHIP_OBSTACLES_H */

/* fasterhip_track.h: TRACKING MOVING OBSTACLES FROM WHAT VEHICLES SEE.  fasterhip_obstacles.h shows the fleet balls that fly a straight
 * line, and takes their records for the truth: "nothing estimates it and nothing doubts it", and "walls do not hide an obstacle".  This
 * header adds the stage in front of it.  Per call and on the device it decides which obstacles some vehicle sees now (in range, and not
 * behind an occupied cell of the map: the ray of fasterhip_link_los.h), keeps a short history of sightings per obstacle, fits a constant
 * velocity to it, and writes the fh_obstacle records that fh_fleet_obstacles_device and fh_fleet_obstacle_audit_device consume as they
 * are.  No existing entry point, kernel or struct changes, FH_ABI_VERSION stays.  C99 / C++11, includes fasterhip_obstacles.h and
 * fasterhip_link_los.h.
 *
 * THE MODEL.  Everything is IEEE double, no fused multiply-add, every comparison strict, the operations in the order written here
 * (tests/track_model.py restates it in plain Python, brute force over all (o, i) and all samples of a ray, and the kernel is compared
 * with that in every byte).  d2(d) = dx dx + dy dy + dz dz, the three products summed from left to right.  A running sum starts at +0
 * and takes its terms one by one.  `tick` counts the caller's cycles of dc; it is the clock of the sightings.
 *   Reading a track.  count and head are read first.  A record with count outside [0, FH_TRACK_HISTORY] or head outside
 *     [0, FH_TRACK_HISTORY - 1] is read as an EMPTY track (count = 0, head = 0).  Sighting q of count, q = 0 the oldest, lies in slot
 *     (head + q) mod FH_TRACK_HISTORY.  A record one of whose count sightings has a tick outside [0, FH_OBSTACLE_MAX_TICK] is read as
 *     empty too, so every difference of two ticks stays inside 64 bits.  The newest sighting is q = count - 1; newest_tick is its tick.
 *     radius is read only with count > 0; an empty track has radius 0.  Nothing else of the record is read.  An all-zero record is an
 *     empty track.
 *   Emptying a track: count = 0, head = 0, radius = 0.
 * Per obstacle o, in this order:
 *   1. Measurement.  z = c_truth[o][0] with the clock of fasterhip_obstacles.h: tau = (double)truth_tick0 * dc, z = p0 + v * tau per
 *      axis (the product is rounded, then the sum).  o is VISIBLE iff the truth record is valid (that header's "Valid") and all three
 *      coordinates of z are finite.  (A real system writes v = 0, p0 = this cycle's detection, truth_tick0 = 0.)
 *   2. Forget.  If count > 0, max_age > 0 and tick - newest_tick > max_age, the track is emptied and FH_TRACK_LOST is set.
 *   3. Seen.  Vehicle i SEES o iff o is visible, the three coordinates of d_vehicles[i].state.pos are finite,
 *      d2(z - pos_i) < r_detect * r_detect (the product rounded once), and map is NULL or the pair is not blocked.  Blocked is
 *      fasterhip_link_los.h's "Blocked" word for word with p = pos_i and q = z: the ray is always cast FROM THE VEHICLE; the cells of
 *      its two ends are not tested; a sample outside the map is free.  d_seer[o] = the smallest i that sees o, or -1.
 *   4. Sighting, if d_seer[o] >= 0.  With count > 0 and tick <= newest_tick the sighting is ignored and FH_TRACK_STALE is set.
 *      Otherwise: with gate > 0 and count > 0, pred = the p0 of step 5 for the track as it stands (after step 2) and this tick; if
 *      d2(z - pred) < gate * gate does NOT hold (a pred that is not finite does not), the track is emptied and FH_TRACK_RESET is set.
 *      Then (tick, z) is appended as the newest sighting: with count = FH_TRACK_HISTORY the oldest one is dropped (its slot takes the
 *      new one and head = (head + 1) mod FH_TRACK_HISTORY), otherwise count grows by one.  radius = the truth's radius, and
 *      FH_TRACK_SEEN is set.
 *   5. Estimate, with count > 0, from the newest k = min(count, fit) sightings s taken from the oldest of them to the newest:
 *        u = (double)(tick_s - newest_tick) * dc;  Su += u;  Suu += u * u;  per axis  Sp += p_s;  Sup += u * p_s.
 *      kk = (double)k.  k = 1: v = +0, a = p of that sighting.  k >= 2:
 *        D = kk * Suu - Su * Su;   per axis  v = (kk * Sup - Su * Sp) / D;   a = (Sp - v * Su) / kk.
 *      age = (double)(tick - newest_tick) * dc;  per axis  p0 = a + v * age;  radius_est = radius + grow * age.
 *      The estimate is USABLE iff the three p0, the three v and radius_est are finite and, for k >= 2, D > 0.
 *   6. Record.  d_est[o] = {p0, v, radius_est, FH_OBSTACLE_ON, 0} iff count >= min_obs and the estimate is usable; otherwise all 64
 *      bytes are zero.  FH_TRACK_BAD_FIT is set iff count >= min_obs and the estimate is not usable.  p0 is where the obstacle is NOW:
 *      the consumer passes tick0 = 0.
 *   7. Writing the track.  Slot (head + q) mod FH_TRACK_HISTORY = sighting q for q < count, every other slot is zero; radius (0 with
 *      count = 0), count, head, flags = the FH_TRACK_* of this call; the reserved words are zero.  EVERY BYTE OF EVERY RECORD IS
 *      WRITTEN BY EVERY CALL, so a track is a function of the sightings and of nothing else the record held.
 *   8. Info.  d_info[0] = the obstacles with d_seer >= 0, d_info[1] = the records with FH_OBSTACLE_ON, d_info[2] = the tracks with
 *      FH_TRACK_RESET, d_info[3] = those with FH_TRACK_LOST.  All four exact.
 * Two properties follow.  Seen is monotone in r_detect without a map or with the same map.  With a map that has no occupied cell every
 * output equals that of map = NULL.
 *
 * KNOWN LIMITS.
 *   The track belongs to the whole fleet: anyone's sighting reaches everyone at once.  Tracks per group of fasterhip_link.h's labels
 *     are a later change.
 *   A sighting is exact.  There is no model of measurement noise, and the fit weighs every sighting alike.
 *   Obstacles are identified: sighting o belongs to track o.  There is no data association.
 *   Constant velocity only.
 *   fh_fleet_obstacles_device still applies its own r_detect ball to the estimated position, with no wall in it.
 *   The map's bits are inflated, so an obstacle is hidden a little early, and a diagonal wall one cell thick can be slipped
 *     (fasterhip_link_los.h).
 *   There is no broad phase: the scan is n m / 64 turns of one wavefront per obstacle, ended early by the first seer. */
#ifndef FASTERHIP_TRACK_H
#define FASTERHIP_TRACK_H
#include "fasterhip_obstacles.h"
#include "fasterhip_link_los.h"
#ifdef __cplusplus
extern "C" {
#endif

#define FH_TRACK_HISTORY 8 /* the sightings a track keeps, and the largest fit and min_obs */

enum {                   /* fh_obstacle_track.flags: what this call did */
  FH_TRACK_SEEN = 1,     /* a sighting was appended                                                                                */
  FH_TRACK_LOST = 2,     /* the newest sighting was older than max_age: the track was emptied (step 2)                             */
  FH_TRACK_RESET = 4,    /* the sighting fell outside the gate: the track was emptied before it was appended (step 4)             */
  FH_TRACK_STALE = 8,    /* seen, but tick <= newest_tick: the sighting was ignored                                                */
  FH_TRACK_BAD_FIT = 16  /* count >= min_obs, but the estimate is not usable: the record is zero                                   */
};

typedef struct fh_track_params { /* 64 B */
  double r_detect;     /* vehicle i sees o when d2(z - pos_i) < r_detect^2 and no wall is between (> 0)                            */
  double dc;           /* the time of one tick (> 0)                                                                               */
  double gate;         /* a sighting farther than this from the prediction starts the track anew (>= 0; 0: no gate)                */
  double grow;         /* the estimated radius grows by this per unit of time since the newest sighting (>= 0)                     */
  int64_t max_age;     /* a track whose newest sighting is more than this many ticks old is forgotten (>= 0; 0: never)             */
  int32_t fit;         /* the newest min(count, fit) sightings are fitted (1 .. FH_TRACK_HISTORY; 1: the last position, at rest)   */
  int32_t min_obs;     /* a record is ON from this many sightings on (1 .. FH_TRACK_HISTORY)                                       */
  int32_t reserved[4];
} fh_track_params;

typedef struct fh_obstacle_track { /* 320 B */
  int64_t tick[FH_TRACK_HISTORY];    /* the ring: the tick of the sighting in each slot                                            */
  double pos[FH_TRACK_HISTORY][3];   /* and where the obstacle was seen                                                            */
  double radius;                     /* the truth's radius at the newest sighting                                                  */
  int32_t count;                     /* sightings held, 0 .. FH_TRACK_HISTORY                                                      */
  int32_t head;                      /* the slot of the oldest one                                                                 */
  int32_t flags;                     /* FH_TRACK_*: this call's                                                                    */
  int32_t reserved[11];              /* zero                                                                                       */
} fh_obstacle_track;

/* One call of THE MODEL for m obstacles and n vehicles: d_tracks[o] is read and rewritten, d_est[o], d_seer[o] and d_info[0 .. 3] are
 * written.  `map` is only read; it must have been filled on the stream of `ctx` (or its fill waited for).  A clear of d_info and one
 * launch on the context's stream (one wavefront per obstacle: the vehicles in ascending chunks of 64, lane = vehicle, one ballot of the
 * lanes in range, their rays one after the other with lane = sample, ended by the first clear one; then the ring and the fit),
 * asynchronous; device pointers.
 * FH_ERR_ARG, checked in this order:
 *    1. ctx == NULL or par == NULL;
 *    2. r_detect NaN, infinite or <= 0;
 *    3. dc NaN, infinite or <= 0;
 *    4. gate NaN, infinite or negative;
 *    5. grow NaN, infinite or negative;
 *    6. max_age < 0;
 *    7. fit < 1 or fit > FH_TRACK_HISTORY;
 *    8. min_obs < 1 or min_obs > FH_TRACK_HISTORY;
 *    9. n < 0 or m < 0;
 *   10. truth_tick0 < 0 or truth_tick0 > FH_OBSTACLE_MAX_TICK;
 *   11. tick < 0 or tick > FH_OBSTACLE_MAX_TICK;
 *   12. map != NULL and the map holds no grid (fh_map_read* first);
 *   13. map != NULL and r_detect / res_map > 4096 (a ray then has fewer than 8192 samples).
 * Then FH_ERR_DEVICE without a device (there is no CPU path), FH_OK for m == 0 (nothing is written), and FH_ERR_ARG for a null d_truth,
 * d_tracks, d_est, d_seer or d_info, or a null d_vehicles with n > 0.  With n == 0 nothing is seen and every record is still written:
 * tracks age, are forgotten and extrapolated.  Every index the kernel uses comes from a value it has checked: count and head before a
 * slot is named, a sample's floored cell against the map's dimensions before it becomes an index, and a position that is not finite
 * never reaches a ray. */
int fh_fleet_obstacle_track_device(fh_ctx* ctx, fh_map* map /* NULL: nothing hides an obstacle */, const fh_track_params* par,
                                   const fh_obstacle* d_truth, int m, int64_t truth_tick0, int64_t tick, const fh_vehicle* d_vehicles,
                                   int n, fh_obstacle_track* d_tracks /* [m], read and rewritten */, fh_obstacle* d_est /* [m] */,
                                   int32_t* d_seer /* [m] */, int64_t* d_info /* [4] */);

#ifdef __cplusplus
}
#endif
#endif /* FASTERHIP_TRACK_H */

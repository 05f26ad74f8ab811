// fh_track.hip.hpp — tracking moving obstacles from what vehicles see (include/fasterhip_track.h, which is the specification): which
// obstacles some vehicle sees now, a ring of sightings per obstacle, a constant velocity fitted to it, and the fh_obstacle records that
// the obstacle stage and its audit consume as they are.  One kernel, no LDS, no working buffer.
//   track_kernel : one wavefront per obstacle o.
//     the scan:  z = p0 + v tau of the truth record, wave-uniform.  The vehicles in ascending chunks of 64, LANE = VEHICLE: the position
//                is read and tested (finite, d2 < r_detect^2), one ballot gives the lanes in range.  They are taken in ascending order
//                (a uniform loop over the set bits); the vehicle's position goes to every lane (readlane) and the ray from it to z is
//                cast by the ray test of fh_link_los.hip.hpp as it is, LANE = SAMPLE.  The first clear ray ends the scan: its vehicle is
//                the smallest index that sees o.  Without a map the first lane in range is the seer.
//     the track: lane 0 alone.  The ring is read into registers in order of age (slot (head + q) & 7, a memory address; every register
//                index is a constant of an unrolled loop, so nothing goes to scratch), checked, aged, gated, appended to and fitted as
//                the header writes it, operation for operation, and written back whole.  A few dozen double operations per obstacle.
//                The record, the seer and up to four integer adds into info leave from that lane.
// WHY ONE WAVEFRONT PER OBSTACLE.  The answer for o is the FIRST vehicle in index order with a clear ray, so the rays of one obstacle
// are ordered; lane = sample makes a ray of up to 64 samples one round of loads (r_detect 6 m on a 0.2 m map: 60 samples), and a
// blocked ray ends at its first round with a hit.  There is no broad phase: every obstacle reads every vehicle until it is seen, n m / 64
// turns at the worst (nobody sees anything).  That is cheap while the positions of the fleet (n x 24 B of records 280 B apart) stay in
// L2 and n m / 64 is in the tens of thousands; DESIGN.md K27 says where it stops.
// EVERY INDEX COMES FROM A CHECKED VALUE.  i < n before a vehicle is read; a ray is cast only for a pair with d2 < r_detect^2, so its
// ends are finite and K is bounded by the entry point's limit; the ray test compares a floored cell with the map's dimensions before it
// becomes an index; a slot is (head + q) & 7, inside the record whatever head holds, and count and head are tested before they are used.
// This file names the records of fasterhip_obstacles.h by its own mirrors (TrackRec, TRACK_TRUTH_ON; fh_capi.hip asserts that they
// equal the header's): the words of that header's stage stay in its own device file (tests/test_obstacle_abi.py).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fasterhip_track.h"
#include "fh_link_los.hip.hpp"
#include "fh_plans.hip.hpp"
#include "fh_wave.hip.hpp"

namespace fh {

constexpr int TRACK_H = FH_TRACK_HISTORY;
constexpr int TRACK_TRUTH_ON = 1;             // the ON bit of a truth or estimate record
constexpr long long TRACK_MAX_TICK = 1ll << 62;  // the largest tick of the clock of the records

struct TrackRec {  // 320 B: the track record of the header, field for field
  long long tick[TRACK_H];
  double pos[TRACK_H][3];
  double radius;
  int count, head, flags;
  int reserved[11];
};

struct TrackArgs {
  LinkLosMap map;  // occ == nullptr: no map, nothing hides an obstacle
  double detect2, gate2;  // r_detect^2 and gate^2, rounded once on the host as the model rounds them
  double dc, grow;
  long long max_age, truth_tick0, tick;
  int fit, min_obs, gate, n, m, pad;  // gate: gate > 0
  const fh_obstacle* truth;
  const fh_vehicle* vehicles;
  TrackRec* tracks;
  fh_obstacle* est;
  int* seer;
  unsigned long long* info;
};

struct TrackRing {  // a track in registers, in order of age: sighting q < count, zeros behind
  long long t[TRACK_H];
  double x[TRACK_H], y[TRACK_H], z[TRACK_H];
  double radius;
  int count, head;
};

struct TrackFit {
  double p[3], v[3], radius;
  bool usable;
};

__device__ __forceinline__ void track_empty(TrackRing& r) {
#pragma unroll
  for (int q = 0; q < TRACK_H; q++) { r.t[q] = 0; r.x[q] = 0.0; r.y[q] = 0.0; r.z[q] = 0.0; }
  r.radius = 0.0; r.count = 0; r.head = 0;
}

__device__ __forceinline__ long long track_newest(const TrackRing& r) {
  long long t = 0;
#pragma unroll
  for (int q = 0; q < TRACK_H; q++)
    if (q == r.count - 1) t = r.t[q];
  return t;
}

// Step 5 of the model for a ring with count > 0.
__device__ __forceinline__ TrackFit track_fit(const TrackRing& r, int fit, long long tick, double dc, double grow) {
#pragma clang fp contract(off)
  const int k = r.count < fit ? r.count : fit;
  const int first = r.count - k;
  const long long newest = track_newest(r);
  double su = 0.0, suu = 0.0, sx = 0.0, sy = 0.0, sz = 0.0, sux = 0.0, suy = 0.0, suz = 0.0, lx = 0.0, ly = 0.0, lz = 0.0;
#pragma unroll
  for (int q = 0; q < TRACK_H; q++) {
    if (q >= first && q < r.count) {
      const double u = (double)(r.t[q] - newest) * dc;
      su = su + u; suu = suu + u * u;
      sx = sx + r.x[q]; sy = sy + r.y[q]; sz = sz + r.z[q];
      sux = sux + u * r.x[q]; suy = suy + u * r.y[q]; suz = suz + u * r.z[q];
      lx = r.x[q]; ly = r.y[q]; lz = r.z[q];
    }
  }
  const double kk = (double)k;
  TrackFit f;
  double ax = lx, ay = ly, az = lz, D = 1.0;
  f.v[0] = 0.0; f.v[1] = 0.0; f.v[2] = 0.0;
  if (k >= 2) {
    D = kk * suu - su * su;
    f.v[0] = (kk * sux - su * sx) / D; f.v[1] = (kk * suy - su * sy) / D; f.v[2] = (kk * suz - su * sz) / D;
    ax = (sx - f.v[0] * su) / kk; ay = (sy - f.v[1] * su) / kk; az = (sz - f.v[2] * su) / kk;
  }
  const double age = (double)(tick - newest) * dc;
  f.p[0] = ax + f.v[0] * age; f.p[1] = ay + f.v[1] * age; f.p[2] = az + f.v[2] * age;
  f.radius = r.radius + grow * age;
  f.usable = plan_finite(f.p[0]) && plan_finite(f.p[1]) && plan_finite(f.p[2]) && plan_finite(f.v[0]) && plan_finite(f.v[1]) &&
             plan_finite(f.v[2]) && plan_finite(f.radius) && D > 0.0;
  return f;
}

// Steps 2 and 4 to 8 of the model for obstacle o, by one lane: the track is read, updated and written whole, the record and the counts.
__device__ __forceinline__ void track_update(const TrackArgs& a, int o, bool seen, double zx, double zy, double zz, double truth_radius) {
#pragma clang fp contract(off)
  TrackRec& R = a.tracks[o];
  TrackRing r;
  r.count = R.count; r.head = R.head;
  bool good = r.count >= 0 && r.count <= TRACK_H && r.head >= 0 && r.head < TRACK_H;
#pragma unroll
  for (int q = 0; q < TRACK_H; q++) {
    const int slot = (r.head + q) & (TRACK_H - 1);  // (inside the record whatever head holds)
    r.t[q] = R.tick[slot]; r.x[q] = R.pos[slot][0]; r.y[q] = R.pos[slot][1]; r.z[q] = R.pos[slot][2];
  }
  r.radius = R.radius;
#pragma unroll
  for (int q = 0; q < TRACK_H; q++) {
    if (q < r.count) {
      if (!(r.t[q] >= 0 && r.t[q] <= TRACK_MAX_TICK)) good = false;
    } else {
      r.t[q] = 0; r.x[q] = 0.0; r.y[q] = 0.0; r.z[q] = 0.0;
    }
  }
  if (!good || r.count == 0) track_empty(r);
  int flags = 0;
  if (r.count > 0 && a.max_age > 0 && a.tick - track_newest(r) > a.max_age) {  // 2. forget
    track_empty(r);
    flags |= FH_TRACK_LOST;
  }
  if (seen) {  // 4. the sighting
    if (r.count > 0 && a.tick <= track_newest(r)) {
      flags |= FH_TRACK_STALE;
    } else {
      if (a.gate && r.count > 0) {
        const TrackFit g = track_fit(r, a.fit, a.tick, a.dc, a.grow);
        const double dx = zx - g.p[0], dy = zy - g.p[1], dz = zz - g.p[2];
        const double d2 = dx * dx + dy * dy + dz * dz;
        if (!(d2 < a.gate2)) {
          track_empty(r);
          flags |= FH_TRACK_RESET;
        }
      }
      if (r.count == TRACK_H) {
#pragma unroll
        for (int q = 0; q + 1 < TRACK_H; q++) { r.t[q] = r.t[q + 1]; r.x[q] = r.x[q + 1]; r.y[q] = r.y[q + 1]; r.z[q] = r.z[q + 1]; }
        r.head = (r.head + 1) & (TRACK_H - 1);
        r.count = TRACK_H - 1;
      }
#pragma unroll
      for (int q = 0; q < TRACK_H; q++)
        if (q == r.count) { r.t[q] = a.tick; r.x[q] = zx; r.y[q] = zy; r.z[q] = zz; }
      r.count++;
      r.radius = truth_radius;
      flags |= FH_TRACK_SEEN;
    }
  }
  bool on = false;  // 5. and 6.: the estimate and the record
  TrackFit f;
  if (r.count > 0) {
    f = track_fit(r, a.fit, a.tick, a.dc, a.grow);
    if (r.count >= a.min_obs) {
      on = f.usable;
      if (!on) flags |= FH_TRACK_BAD_FIT;
    }
  }
  fh_obstacle& E = a.est[o];
  E.p0[0] = on ? f.p[0] : 0.0; E.p0[1] = on ? f.p[1] : 0.0; E.p0[2] = on ? f.p[2] : 0.0;
  E.v[0] = on ? f.v[0] : 0.0; E.v[1] = on ? f.v[1] : 0.0; E.v[2] = on ? f.v[2] : 0.0;
  E.radius = on ? f.radius : 0.0;
  E.flags = on ? TRACK_TRUTH_ON : 0; E.reserved = 0;
#pragma unroll
  for (int q = 0; q < TRACK_H; q++) {  // 7. the track, whole
    const int slot = (r.head + q) & (TRACK_H - 1);
    R.tick[slot] = r.t[q]; R.pos[slot][0] = r.x[q]; R.pos[slot][1] = r.y[q]; R.pos[slot][2] = r.z[q];
  }
  R.radius = r.radius; R.count = r.count; R.head = r.head; R.flags = flags;
#pragma unroll
  for (int w = 0; w < 11; w++) R.reserved[w] = 0;
  if (seen) atomicAdd(a.info + 0, 1ull);  // 8.
  if (on) atomicAdd(a.info + 1, 1ull);
  if (flags & FH_TRACK_RESET) atomicAdd(a.info + 2, 1ull);
  if (flags & FH_TRACK_LOST) atomicAdd(a.info + 3, 1ull);
}

__global__ void __launch_bounds__(64) track_kernel(TrackArgs a) {
#pragma clang fp contract(off)
  const int lane = fhw::lane_id();
  const int o = (int)blockIdx.x;
  if (o >= a.m) return;
  const fh_obstacle& T = a.truth[o];
  const double px = fhw::uniform_f64(T.p0[0]), py = fhw::uniform_f64(T.p0[1]), pz = fhw::uniform_f64(T.p0[2]);
  const double vx = fhw::uniform_f64(T.v[0]), vy = fhw::uniform_f64(T.v[1]), vz = fhw::uniform_f64(T.v[2]);
  const double radius = fhw::uniform_f64(T.radius);
  const int tflags = fhw::uniform_i32(T.flags);
  const double tau = (double)a.truth_tick0 * a.dc;
  const double zx = px + vx * tau, zy = py + vy * tau, zz = pz + vz * tau;  // 1. the measurement
  const bool visible = (tflags & TRACK_TRUTH_ON) != 0 && plan_finite(px) && plan_finite(py) && plan_finite(pz) && plan_finite(vx) &&
                       plan_finite(vy) && plan_finite(vz) && plan_finite(radius) && radius >= 0.0 && plan_finite(zx) && plan_finite(zy) &&
                       plan_finite(zz);
  int seer = -1;  // 3. (uniform)
  if (visible) {
    for (long long base = 0; base < (long long)a.n && seer < 0; base += 64) {
      const long long i = base + lane;
      bool near = false;
      double ix = 0.0, iy = 0.0, iz = 0.0;
      if (i < (long long)a.n) {
        const double* pos = a.vehicles[i].state.pos;
        ix = pos[0]; iy = pos[1]; iz = pos[2];
        if (plan_finite(ix) && plan_finite(iy) && plan_finite(iz)) {
          const double dx = zx - ix, dy = zy - iy, dz = zz - iz;
          const double d2 = dx * dx + dy * dy + dz * dz;
          near = d2 < a.detect2;
        }
      }
      for (unsigned long long todo = __ballot(near); todo; todo &= todo - 1ull) {  // (uniform)
        const int src = (int)__builtin_ctzll(todo);
        bool blocked = false;
        if (a.map.occ) {
          const double sx = fhw::readlane_f64(ix, src), sy = fhw::readlane_f64(iy, src), sz = fhw::readlane_f64(iz, src);
          blocked = ray_blocked(a.map, lane, sx, sy, sz, zx, zy, zz);
        }
        if (!blocked) {
          seer = (int)base + src;
          break;
        }
      }
    }
  }
  if (lane == 0) {
    a.seer[o] = seer;
    track_update(a, o, seer >= 0, zx, zy, zz, radius);
  }
}

}  // namespace fh

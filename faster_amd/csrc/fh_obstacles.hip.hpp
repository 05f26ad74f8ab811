// fh_obstacles.hip.hpp — moving obstacles (include/fasterhip_obstacles.h, which is the specification): things that fly a straight line
// at a constant velocity and are no fleet member, as points behind the cloud and as bits of every vehicle's mask row, and the audit of
// the committed plans against where the obstacles are at the same instant.  The slots, words, chunks (64 samples, one wavefront of the
// points kernel, one ballot of the mask kernel) and the mask frame are those of fh_traffic.hip.hpp, which is included and not changed:
// traffic_rows, traffic_word, TrafficRec, TrafficBox and TrafficArgs are used as they are, with n = the observers (rows) and the samples
// numbered t = o S + s over the OBSTACLES.  Working buffers of its own (fh_capi.hip: OBSTACLE_*), so calls of traffic and of this stage
// may alternate on one context.  No atomics, every word of a row stored exactly once (traffic_rows).
//   obstacle_points{1,7}_kernel: one wavefront per chunk, lane = sample.  The obstacle record is checked (ON, seven finite doubles,
//                      radius >= 0), c = p0 + v tau computed as the model writes it, the PPS points of the slot written (zeros when the
//                      sample does not show), and the compact record of the sample in two halves of 32 B: TrafficRec (centre, show
//                      word, o) to OBSTACLE_SAMPLES, which is what traffic_rows hands to the decide step, and ObstacleMore (now[o],
//                      reach_o^2) to OBSTACLE_MORE.  The box of the shown centres of the chunk, grown by the chunk's LARGEST reach,
//                      goes to OBSTACLE_BOXES.
//   obstacle_observers_kernel: one wavefront per chunk of 64 samples t = i S + s' of the VEHICLES: traffic_points' reading of the
//                      plan (extent checked, a plan that has ended stands at its last state), a TrafficRec per sample to
//                      OBSTACLE_OBSERVERS, and nothing into the cloud.
//   obstacle_mask{1,7}_kernel: traffic_rows with
//     row:    the S records of vehicle i staged into LDS as three arrays of doubles, NaN where a sample does not show (every comparison
//             with it fails without a branch); their box reduced on the way; state_i.pos read once, wave-uniform.  Lane = chunk:
//             does the chunk's grown box overlap the row box?
//     decide: lane = sample t, s = t - o S; the window loop of traffic_timed_mask with reach2 of the SAMPLE instead of range2, ANDed
//             with detected(i, o): detection off, or now[o] and pos_i finite and d2 < r_detect^2.
//   obstacle_audit_kernel: one wavefront per vehicle, lanes over the tested instants (a turn of 64 at a time).  The obstacles go through
//             LDS FH_OBSTACLE_AUDIT_CHUNK at a time as seven arrays of doubles (p0, v, hit^2; p0[0] = NaN for an obstacle that is not
//             valid: its c is then not finite and it is skipped with no branch of its own).  A lane keeps the lexicographic minimum of
//             (d2, j, o) and of (j, o) among the hits, and per chunk one bit per obstacle that hit; the bits are ORed over the lanes
//             once per chunk and counted.  The record leaves as one 16-byte store from each of lanes 0..3.  The minimum is of a total
//             order, so no field depends on which lane or turn saw a pair first.
// THE BOX MARGIN.  A bit needs a shown c = c[o][s] and a shown c' = c[i][s'] with d2 < reach_o^2 as rounded, so |c - c'| < reach_o
// (1 + 4e-16) per axis (fh_traffic.hip.hpp argues the 4e-16: the roundings of the difference, of its square, of the sums and of
// reach_o^2).  c lies in its chunk's box [lo, hi] exactly, c' in the row box [rlo, rhi] exactly, and reach_o <= R, the largest reach
// among the shown samples of the chunk (reach_o = fl(range + radius_o) is the very number the decision squares).  Hence rhi >= c' > lo -
// R (1 + 4e-16) and rlo <= c' < hi + R (1 + 4e-16): the chunk box grown by cell_box_margin(R, lo, hi) = R + 1e-9 (R + |lo| + |hi|),
// seven orders above those roundings, overlaps the row box.  R = +inf (a radius near the end of the doubles) gives a box that overlaps
// every row; a chunk with no shown sample has the box (+inf, -inf), whose grown bounds are NaN, and is looked at by nobody: its words
// are stored as zeros.  Detection is not part of the prefilter: it is decided per sample.
// Every index comes from a checked value: o = t / S < m for t < m S, the buffers are sized in whole chunks so that a lane past the last
// sample reads and writes its own slot, head and size are tested against max_states before a plan is read, and an LDS index is clamped
// to [0, S - 1] (samples) or runs below the staged count (audit).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fasterhip_obstacles.h"
#include "fh_traffic.hip.hpp"
#include "fh_traffic_timed.hip.hpp"

namespace fh {

struct ObstacleMore {  // 32 B: the second half of a sample's compact record
  double now[3];       // c[o][0]
  double reach2;       // (range + radius_o)^2
};

struct ObstacleArgs {
  TrafficArgs t;  // n = the rows; samples, stride, first_instant, window, span, the words and the mask; recs and boxes: the obstacles'
  double dc, detect2;  // detect2 = r_detect * r_detect, rounded once on the host as the model rounds it
  long long tick0;
  int m, detect;  // detect: r_detect != 0
  int n_own, n_own_chunks;  // n S and ceil(n S / 64)
  const fh_obstacle* obstacles;
  ObstacleMore* more;  // [64 t.n_chunks]
  TrafficRec* own;     // [64 n_own_chunks]: the observers' samples
};

__device__ __forceinline__ bool obstacle_valid(int flags, double px, double py, double pz, double vx, double vy, double vz, double radius) {
  return (flags & FH_OBSTACLE_ON) != 0 && plan_finite(px) && plan_finite(py) && plan_finite(pz) && plan_finite(vx) && plan_finite(vy) &&
         plan_finite(vz) && plan_finite(radius) && radius >= 0.0;
}

template <int PPS>
__device__ __forceinline__ void obstacle_points(const ObstacleArgs& A) {
#pragma clang fp contract(off)
  using fhw::wave_max;
  using fhw::wave_min;
  const TrafficArgs& a = A.t;
  const int lane = fhw::lane_id();
  const int chunk = (int)blockIdx.x;
  if (chunk >= a.n_chunks) return;
  const int t = chunk * 64 + lane;
  bool show = false;
  double cx = 0.0, cy = 0.0, cz = 0.0, nx = 0.0, ny = 0.0, nz = 0.0, reach = 0.0, reach2 = 0.0, radius = 0.0;
  int o = 0;
  if (t < a.n_samples) {
    o = t / a.samples;
    const int s = t - o * a.samples;
    const fh_obstacle& O = A.obstacles[o];
    const double px = O.p0[0], py = O.p0[1], pz = O.p0[2], vx = O.v[0], vy = O.v[1], vz = O.v[2];
    radius = O.radius;
    if (obstacle_valid(O.flags, px, py, pz, vx, vy, vz, radius)) {
      const long long j = (long long)a.first_instant + (long long)s * (long long)a.stride;
      const double tau = (double)(A.tick0 + j) * A.dc, tau0 = (double)A.tick0 * A.dc;
      const double x = px + vx * tau, y = py + vy * tau, z = pz + vz * tau;
      nx = px + vx * tau0; ny = py + vy * tau0; nz = pz + vz * tau0;
      reach = a.range + radius;
      reach2 = reach * reach;
      if (plan_finite(x) && plan_finite(y) && plan_finite(z)) {
        show = true;
        cx = x; cy = y; cz = z;
      }
    }
    double* out = a.cloud + 3 * ((size_t)a.first_point + (size_t)t * (size_t)PPS);
    out[0] = cx; out[1] = cy; out[2] = cz;
    if (PPS == 7) {
      const double h = radius;
      const double xp = show ? cx + h : 0.0, xm = show ? cx - h : 0.0, yp = show ? cy + h : 0.0, ym = show ? cy - h : 0.0,
                   zp = show ? cz + h : 0.0, zm = show ? cz - h : 0.0;
      out[3] = xp; out[4] = cy; out[5] = cz;
      out[6] = xm; out[7] = cy; out[8] = cz;
      out[9] = cx; out[10] = yp; out[11] = cz;
      out[12] = cx; out[13] = ym; out[14] = cz;
      out[15] = cx; out[16] = cy; out[17] = zp;
      out[18] = cx; out[19] = cy; out[20] = zm;
    }
  }
  TrafficRec& R = a.recs[(size_t)t];  // (a lane past the last sample has a slot too: show = 0)
  R.c[0] = cx; R.c[1] = cy; R.c[2] = cz;
  R.show = show ? 1 : 0; R.k = o;
  ObstacleMore& M = A.more[(size_t)t];
  M.now[0] = nx; M.now[1] = ny; M.now[2] = nz; M.reach2 = reach2;
  const double lx = wave_min(show ? cx : INFINITY), ly = wave_min(show ? cy : INFINITY), lz = wave_min(show ? cz : INFINITY);
  const double hx = wave_max(show ? cx : -INFINITY), hy = wave_max(show ? cy : -INFINITY), hz = wave_max(show ? cz : -INFINITY);
  const double big = wave_max(show ? reach : 0.0);  // (the largest reach of the chunk; reach >= range > 0, no NaN: radius is finite)
  if (lane == 0) {
    const double gx = cell_box_margin(big, lx, hx), gy = cell_box_margin(big, ly, hy), gz = cell_box_margin(big, lz, hz);
    TrafficBox& B = a.boxes[chunk];
    B.lo[0] = lx - gx; B.lo[1] = ly - gy; B.lo[2] = lz - gz;
    B.hi[0] = hx + gx; B.hi[1] = hy + gy; B.hi[2] = hz + gz;
  }
}

__device__ __forceinline__ void obstacle_observers(const ObstacleArgs& A) {
  const TrafficArgs& a = A.t;
  const int lane = fhw::lane_id();
  const int chunk = (int)blockIdx.x;
  if (chunk >= A.n_own_chunks) return;
  const int t = chunk * 64 + lane;
  bool show = false;
  double cx = 0.0, cy = 0.0, cz = 0.0;
  int i = 0;
  if (t < A.n_own) {
    i = t / a.samples;
    const int s = t - i * a.samples;
    const fh_vehicle& V = a.vehicles[i];
    const int head = V.plan_head, size = V.plan_size;
    if (!plan_bad_extent(head, size, a.max_states) && size >= 1) {
      const long long j = (long long)a.first_instant + (long long)s * (long long)a.stride, last = (long long)size - 1;
      const double* p = a.plans[(size_t)i * (size_t)a.max_states + (size_t)head + (size_t)(j < last ? j : last)].pos;
      const double x = p[0], y = p[1], z = p[2];
      if (plan_finite(x) && plan_finite(y) && plan_finite(z)) {
        show = true;
        cx = x; cy = y; cz = z;
      }
    }
  }
  TrafficRec& R = A.own[(size_t)t];  // (a lane past the last sample has a slot too: show = 0)
  R.c[0] = cx; R.c[1] = cy; R.c[2] = cz;
  R.show = show ? 1 : 0; R.k = i;
}

template <int PPS>
__device__ __forceinline__ void obstacle_mask(const ObstacleArgs& A) {
#pragma clang fp contract(off)
  using fhw::uniform_f64;
  using fhw::wave_max;
  using fhw::wave_min;
  // the observer's samples, NaN where one does not show.  One wavefront is the workgroup: the barriers order its LDS accesses only.
  __shared__ double ox[FH_OBSTACLE_MAX_SAMPLES], oy[FH_OBSTACLE_MAX_SAMPLES], oz[FH_OBSTACLE_MAX_SAMPLES];
  const TrafficArgs& a = A.t;
  const int lane = fhw::lane_id();
  const int S = a.samples;
  double px = 0.0, py = 0.0, pz = 0.0;  // where vehicle i stands
  bool p_finite = false;
  traffic_rows<PPS>(
      a,
      [&](int i, const TrafficBox& B) {
        __syncthreads();  // (the last row's reads are done)
        const double* p = a.vehicles[i].state.pos;
        px = uniform_f64(p[0]); py = uniform_f64(p[1]); pz = uniform_f64(p[2]);
        p_finite = plan_finite(px) && plan_finite(py) && plan_finite(pz);
        double lx = INFINITY, ly = INFINITY, lz = INFINITY, hx = -INFINITY, hy = -INFINITY, hz = -INFINITY;
        for (int s0 = 0; s0 < S; s0 += 64) {
          const int sp = s0 + lane;
          bool show = false;
          double x = NAN, y = NAN, z = NAN;
          if (sp < S) {
            const TrafficRec& R = A.own[(size_t)i * (size_t)S + (size_t)sp];
            show = R.show != 0;
            if (show) { x = R.c[0]; y = R.c[1]; z = R.c[2]; }
            ox[sp] = x; oy[sp] = y; oz[sp] = z;
          }
          lx = fmin(lx, wave_min(show ? x : INFINITY)); ly = fmin(ly, wave_min(show ? y : INFINITY)); lz = fmin(lz, wave_min(show ? z : INFINITY));
          hx = fmax(hx, wave_max(show ? x : -INFINITY)); hy = fmax(hy, wave_max(show ? y : -INFINITY)); hz = fmax(hz, wave_max(show ? z : -INFINITY));
        }
        __syncthreads();
        const double gx = cell_box_margin(0.0, lx, hx), gy = cell_box_margin(0.0, ly, hy), gz = cell_box_margin(0.0, lz, hz);
        const double rx0 = lx - gx, rx1 = hx + gx, ry0 = ly - gy, ry1 = hy + gy, rz0 = lz - gz, rz1 = hz + gz;
        return __ballot(B.lo[0] <= rx1 && B.hi[0] >= rx0 && B.lo[1] <= ry1 && B.hi[1] >= ry0 && B.lo[2] <= rz1 && B.hi[2] >= rz0);
      },
      [&](int, int t, const TrafficRec& R) {
        const ObstacleMore& M = A.more[(size_t)t];
        const double cx = R.c[0], cy = R.c[1], cz = R.c[2];
        const double reach2 = M.reach2;
        const double ex = M.now[0] - px, ey = M.now[1] - py, ez = M.now[2] - pz;
        const double e2 = ex * ex + ey * ey + ez * ez;
        const bool now_finite = plan_finite(M.now[0]) && plan_finite(M.now[1]) && plan_finite(M.now[2]);
        const bool detected = A.detect == 0 || (now_finite && p_finite && e2 < A.detect2);
        const int o = R.k;
        const bool ask = R.show != 0;
        const int s = ask ? t - o * S : 0;  // (a shown sample has t < m S and o = t / S)
        const int lo = max(0, s - a.window), hi = ask ? min(S - 1, s + a.window) : -1;
        bool near = false;
        for (int q = 0; q < a.span; q++) {
          const int sp = lo + q, at = min(sp, S - 1);
          const double dx = cx - ox[at], dy = cy - oy[at], dz = cz - oz[at];
          const double d2 = dx * dx + dy * dy + dz * dz;
          near = near || (sp <= hi && d2 < reach2);
        }
        return near && detected;
      });
}

struct ObstacleAuditArgs {
  double r, dc;
  long long tick0;
  int stride, count, n, m, max_states;
  const fh_obstacle* obstacles;
  const fh_vehicle* vehicles;
  const fh_state* plans;
  fh_plan_obstacle_audit* out;
};

__device__ __forceinline__ void obstacle_audit(const ObstacleAuditArgs& a) {
#pragma clang fp contract(off)
  constexpr int CH = FH_OBSTACLE_AUDIT_CHUNK;
  static_assert(CH == 64, "a lane stages one obstacle, and a lane's hits of a chunk are one 64-bit word");
  __shared__ double qx[CH], qy[CH], qz[CH], ux[CH], uy[CH], uz[CH], h2[CH];
  const int lane = fhw::lane_id();
  const int i = (int)blockIdx.x;
  if (i >= a.n) return;
  const fh_vehicle& V = a.vehicles[i];
  const int head = fhw::uniform_i32(V.plan_head), size = fhw::uniform_i32(V.plan_size);
  int flags = 0, n_tested = 0, first = -1, first_o = -1, worst = -1, worst_o = -1, n_hit = 0;
  double min_d2 = INFINITY;
  if (plan_bad_extent(head, size, a.max_states)) {
    flags = FH_OBSTACLE_BAD_PLAN;
  } else {
    n_tested = plan_instants(plan_limit(a.count, size), a.stride);
    const int turns = (n_tested + 63) >> 6;
    const fh_state* plan = a.plans + ((size_t)i * (size_t)a.max_states + (size_t)head);
    bool not_finite = false;
    double b_d2 = INFINITY;
    int b_j = 0x7fffffff, b_o = 0x7fffffff, f_j = 0x7fffffff, f_o = 0x7fffffff;
    // (with no obstacle the loop below does not run: the tested positions are still looked at once, for FH_OBSTACLE_NOT_FINITE)
    const int chunks = a.m > 0 ? (a.m + CH - 1) / CH : 1;
    for (int ch = 0; ch < chunks; ch++) {
      const int o0 = ch * CH, staged = min(CH, a.m - o0);  // (staged <= 0 only when m == 0)
      __syncthreads();  // (the last chunk's reads are done)
      if (lane < staged) {
        const fh_obstacle& O = a.obstacles[o0 + lane];
        const double px = O.p0[0], py = O.p0[1], pz = O.p0[2], vx = O.v[0], vy = O.v[1], vz = O.v[2], radius = O.radius;
        const bool valid = obstacle_valid(O.flags, px, py, pz, vx, vy, vz, radius);
        const double hit = a.r + radius;
        qx[lane] = valid ? px : NAN; qy[lane] = py; qz[lane] = pz;
        ux[lane] = vx; uy[lane] = vy; uz[lane] = vz;
        h2[lane] = hit * hit;
      }
      __syncthreads();
      unsigned long long hits = 0ull;  // bit e: obstacle o0 + e hit at one of this lane's instants
      for (int turn = 0; turn < turns; turn++) {
        const int k = turn * 64 + lane;
        if (k >= n_tested) continue;
        const int j = k * a.stride;  // (< size <= max_states)
        const double* p = plan[j].pos;
        const double x = p[0], y = p[1], z = p[2];
        if (!(plan_finite(x) && plan_finite(y) && plan_finite(z))) {
          not_finite = true;
          continue;
        }
        const double tau = (double)(a.tick0 + (long long)j) * a.dc;
        for (int e = 0; e < staged; e++) {
          const double cx = qx[e] + ux[e] * tau, cy = qy[e] + uy[e] * tau, cz = qz[e] + uz[e] * tau;
          if (!(plan_finite(cx) && plan_finite(cy) && plan_finite(cz))) continue;  // (an obstacle that is not valid has cx = NaN)
          const double dx = cx - x, dy = cy - y, dz = cz - z;
          const double d2 = dx * dx + dy * dy + dz * dz;
          const int o = o0 + e;
          if (d2 < b_d2 || (d2 == b_d2 && d2 < INFINITY && (j < b_j || (j == b_j && o < b_o)))) {
            b_d2 = d2; b_j = j; b_o = o;
          }
          if (d2 < h2[e]) {
            hits |= 1ull << e;
            if (j < f_j || (j == f_j && o < f_o)) { f_j = j; f_o = o; }
          }
        }
      }
      const unsigned all_lo = fhw::wave_or((unsigned)hits), all_hi = fhw::wave_or((unsigned)(hits >> 32));
      n_hit += __popc(all_lo) + __popc(all_hi);
    }
    if (fhw::wave_any(not_finite)) flags |= FH_OBSTACLE_NOT_FINITE;
    // the minimum d2, then the smallest j among the lanes that hold it, then the smallest o among those; the same for first
    min_d2 = fhw::wave_min(b_d2);
    const bool holds = b_d2 == min_d2 && min_d2 < INFINITY;
    worst = fhw::wave_min_i32(holds ? b_j : 0x7fffffff);
    worst_o = fhw::wave_min_i32(holds && b_j == worst ? b_o : 0x7fffffff);
    first = fhw::wave_min_i32(f_j);
    first_o = fhw::wave_min_i32(f_j == first ? f_o : 0x7fffffff);
    if (worst == 0x7fffffff) worst = worst_o = -1;
    if (first == 0x7fffffff) first = first_o = -1;
    if (first >= 0) flags |= FH_OBSTACLE_HIT;
  }
  // words 2 l and 2 l + 1 of the record from lane l < 4: 64 contiguous bytes in one store instruction
  double w0 = 0.0, w1 = 0.0;
  if (lane == 0) { w0 = plan_pack(flags, n_tested); w1 = plan_pack(first, first_o); }
  if (lane == 1) { w0 = plan_pack(worst, worst_o); w1 = plan_pack(n_hit, 0); }
  if (lane == 2) { w0 = min_d2; }
  if (lane < 4) reinterpret_cast<double2*>(a.out + i)[lane] = make_double2(w0, w1);
}

// Plain kernels, as in fh_traffic.hip.hpp and for its reason.
__global__ void __launch_bounds__(64) obstacle_points1_kernel(ObstacleArgs a) { obstacle_points<1>(a); }
__global__ void __launch_bounds__(64) obstacle_points7_kernel(ObstacleArgs a) { obstacle_points<7>(a); }
__global__ void __launch_bounds__(64) obstacle_observers_kernel(ObstacleArgs a) { obstacle_observers(a); }
__global__ void __launch_bounds__(64) obstacle_mask1_kernel(ObstacleArgs a) { obstacle_mask<1>(a); }
__global__ void __launch_bounds__(64) obstacle_mask7_kernel(ObstacleArgs a) { obstacle_mask<7>(a); }
__global__ void __launch_bounds__(64) obstacle_audit_kernel(ObstacleAuditArgs a) { obstacle_audit(a); }

}  // namespace fh

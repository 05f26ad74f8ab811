// fh_certify.hip.hpp — the certificate of a solved trajectory (include/fasterhip_certify.h, which is the specification): the constraints
// of solverGurobi.cpp as they are written there, evaluated on the 12 N coefficients of an fh_result against its fh_problem and the face
// rows.  Shares nothing with the solver (fh_solve.hip.hpp): no jerk space, no reduced space, no table, no active set.
//
// certify_kernel: one wavefront per result, four per workgroup, grid ceil(n / 4); no atomics, no LDS, no state between workgroups.
//   corridor lanes : lane = (t = lane >> 2, k = lane & 3) holds control point k of segment t in registers (N = 16 fills the wave) and
//                    sweeps the rows of every polytope, which all lanes read at the same address (scalar loads, several rows in flight);
//                    e(t, q) = the maximum over the four lanes of a segment, then the minimum over q per segment, then the wave maximum.
//   state lanes    : lane = (t = lane >> 2, axis = lane & 3 < 3) evaluates pos / vel / acc of its axis at tau = 0 and tau = dt (and of
//                    segment t + 1 at 0): x0, xf, continuity, the box rows and the peaks are wave maxima over these lanes.
//   cost           : (6 a)(6 a) per state lane, added up in the model's order (t outer, axis inner) from lane to lane.
//   the certificate leaves as one store of 16 bytes from each of lanes 0..7.
// Every double operation is written in the order of the specification with contraction off: tests/certify_model.py restates it in numpy
// and tests/test_gpu_certify.py compares bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fasterhip_certify.h"
#include "fh_wave.hip.hpp"

namespace fh {

struct CertTol {  // fh_certify_tol by value; given = 0: no tolerances, only the structural flags
  double corridor, state, box, cost_rel;
  int given;
};

__device__ __forceinline__ double cert_pos(double a, double b, double c, double d, double tau) {
#pragma clang fp contract(off)
  return a * tau * tau * tau + b * tau * tau + c * tau + d;
}
__device__ __forceinline__ double cert_vel(double a, double b, double c, double tau) {
#pragma clang fp contract(off)
  return 3 * a * tau * tau + 2 * b * tau + c;
}
__device__ __forceinline__ double cert_acc(double a, double b, double tau) {
#pragma clang fp contract(off)
  return 6 * a * tau + 2 * b;
}
__device__ __forceinline__ double cert_max(double m, double x) { return x > m ? x : m; }  // a NaN never wins
__device__ __forceinline__ bool cert_finite(double x) { return fabs(x) < INFINITY; }      // false for a NaN
__device__ __forceinline__ double cert_pick3(int k, double x0, double x1, double x2) { return k == 0 ? x0 : k == 1 ? x1 : x2; }

// words 2 l and 2 l + 1 of the certificate from lane l < 8: 128 contiguous bytes in one store instruction
__device__ __forceinline__ void cert_store(fh_certificate* o, int lane, const double (&w)[16]) {
  double lo = 0.0, hi = 0.0;
#pragma unroll
  for (int l = 0; l < 8; l++)
    if (lane == l) { lo = w[2 * l]; hi = w[2 * l + 1]; }
  if (lane < 8) reinterpret_cast<double2*>(o)[lane] = make_double2(lo, hi);
}

__global__ void __launch_bounds__(256) certify_kernel(const fh_problem* __restrict__ problems, const fh_face* __restrict__ faces, long long n_faces,
                                                      const fh_result* __restrict__ results, int n, CertTol tol,
                                                      fh_certificate* __restrict__ out) {
#pragma clang fp contract(off)
  const int lane = fhw::lane_id();
  const int i = (int)blockIdx.x * 4 + fhw::uniform_i32((int)threadIdx.x >> 6);
  if (i >= n) return;  // (a tail wavefront leaves before any cross-lane operation)
  const fh_problem& P = problems[i];
  const fh_result& R = results[i];
  const int N = P.n_seg, Q = P.n_poly, fb = P.face_begin;
  const int t = lane >> 2, k = lane & 3;
  double w[16];
#pragma unroll
  for (int j = 0; j < 16; j++) w[j] = 0.0;

  // ---- the structural flags: nothing is read that they do not allow ----
  int flags = 0;
  if (R.solved == 0) {
    flags = FH_CERT_UNSOLVED;
  } else {
    bool bad = N < 1 || N > FH_MAX_SEG || Q < 0 || Q > FH_MAX_POLY || fb < 0;
    if (!bad) {
      bad = P.face_off[0] != 0;
      for (int q = 0; q < Q; q++) bad |= P.face_off[q] > P.face_off[q + 1];
      bad |= (long long)fb + (long long)P.face_off[Q] > n_faces;
      if (Q > 0) {
        const int a = lane < N ? (int)R.assign[lane] : 0;
        bad |= fhw::wave_any(lane < N && (a < 0 || a >= Q));
      }
    }
    if (bad) flags = FH_CERT_BAD_INPUT;
  }
  if (flags) {
    w[0] = __hiloint2double(0, flags);
    cert_store(out + i, lane, w);
    return;
  }
  const bool seg = t < N;  // N is 1..16 here: rows t < N of the result exist
  const double dt = R.dt;
  double c[12];
#pragma unroll
  for (int j = 0; j < 12; j++) c[j] = seg ? R.coeff[t][j] : 0.0;
  bool lane_bad = false;
#pragma unroll
  for (int j = 0; j < 12; j++) lane_bad |= !cert_finite(c[j]);
  if (!cert_finite(dt) || !(dt > 0) || fhw::wave_any(seg && lane_bad)) {
    w[0] = __hiloint2double(0, FH_CERT_NOT_FINITE);
    cert_store(out + i, lane, w);
    return;
  }

  // ---- corridor: control point k of segment t against every row of every polytope ----
  double p[3];
#pragma unroll
  for (int ax = 0; ax < 3; ax++) {
    const double a = c[ax], b = c[3 + ax], cc = c[6 + ax], d = c[9 + ax];
    const double Bn = b * dt * dt, Cn = cc * dt;
    const double cp0 = cert_pos(a, b, cc, d, 0.0), cp1 = (Cn + 3 * d) / 3, cp2 = (Bn + 2 * Cn + 3 * d) / 3, cp3 = cert_pos(a, b, cc, d, dt);
    p[ax] = k == 0 ? cp0 : k == 1 ? cp1 : k == 2 ? cp2 : cp3;
  }
  const int my_q = seg ? (int)R.assign[t] : -1;
  double best = INFINITY, assigned = -INFINITY;
  for (int q = 0; q < Q; q++) {
    const long long f0 = (long long)fb + P.face_off[q], f1 = (long long)fb + P.face_off[q + 1];  // inside [0, n_faces): checked above
    double e = -INFINITY;
#pragma unroll 4
    for (long long f = f0; f < f1; f++) {
      const fh_face F = faces[f];
      const double v = F.a[0] * p[0] + F.a[1] * p[1] + F.a[2] * p[2] - F.b;
      e = v > e ? v : e;
    }
    e = fhw::quad_max(e);
    best = e < best ? e : best;
    if (q == my_q) assigned = e;
  }
  const bool cor = seg && Q > 0;
  const double best_t = cor ? best : -INFINITY;
  const double corridor_best = fhw::wave_max(best_t);
  const double corridor_assigned = fhw::wave_max(cor ? assigned : -INFINITY);
  const int worst_seg = Q > 0 ? fhw::first_lane(cor && best_t == corridor_best) >> 2 : -1;

  // ---- the state rows: lane = (segment t, axis k) ----
  const bool act = seg && k < 3;
  const int ax = k < 3 ? k : 2;
  const double a = cert_pick3(ax, c[0], c[1], c[2]), b = cert_pick3(ax, c[3], c[4], c[5]);
  const double cc = cert_pick3(ax, c[6], c[7], c[8]), d = cert_pick3(ax, c[9], c[10], c[11]);
  const double p0 = cert_pos(a, b, cc, d, 0.0), v0 = cert_vel(a, b, cc, 0.0), a0 = cert_acc(a, b, 0.0);
  const double p1 = cert_pos(a, b, cc, d, dt), v1 = cert_vel(a, b, cc, dt), a1 = cert_acc(a, b, dt);
  const double jerk = 6 * a;

  double m = -INFINITY;
  if (act && t == 0) {
    m = cert_max(m, fabs(p0 - P.x0[ax]));
    m = cert_max(m, fabs(v0 - P.x0[3 + ax]));
    m = cert_max(m, fabs(a0 - P.x0[6 + ax]));
  }
  const double x0_defect = fhw::wave_max(m);

  m = -INFINITY;
  if (act && t == N - 1) {
    if (P.force_final_pos) m = cert_max(m, fabs(p1 - P.xf[ax]));
    m = cert_max(m, fabs(v1 - P.xf[3 + ax]));
    m = cert_max(m, fabs(a1 - P.xf[6 + ax]));
  }
  const double xf_defect = fhw::wave_max(m);

  m = -INFINITY;
  if (act && t < N - 1) {
    const double na = R.coeff[t + 1][ax], nb = R.coeff[t + 1][3 + ax], nc = R.coeff[t + 1][6 + ax], nd = R.coeff[t + 1][9 + ax];
    m = cert_max(m, fabs(p1 - cert_pos(na, nb, nc, nd, 0.0)));
    m = cert_max(m, fabs(v1 - cert_vel(na, nb, nc, 0.0)));
    m = cert_max(m, fabs(a1 - cert_acc(na, nb, 0.0)));
  }
  const double joined = fhw::wave_max(m);
  const double continuity_defect = N == 1 ? 0.0 : joined;

  const double v_excess = fhw::wave_max(act ? fabs(v0) - P.v_max : -INFINITY);
  const double a_excess = fhw::wave_max(act ? fabs(a0) - P.a_max : -INFINITY);
  const double j_excess = fhw::wave_max(act ? fabs(jerk) - P.j_max : -INFINITY);

  double vp = cert_max(cert_max(-INFINITY, fabs(v0)), fabs(v1));
  if (a != 0) {
    const double ts = (-b) / (3 * a);
    if (0 < ts && ts < dt) vp = cert_max(vp, fabs(cert_vel(a, b, cc, ts)));
  }
  const double v_peak = fhw::wave_max(act ? vp : -INFINITY);
  const double a_peak = fhw::wave_max(act ? cert_max(cert_max(-INFINITY, fabs(a0)), fabs(a1)) : -INFINITY);

  // ---- cost: the squares sit in their lanes and are added in the model's order ----
  const double jj = jerk * jerk;
  double cost = 0.0;
  for (int s = 0; s < N; s++) {
    cost = cost + fhw::readlane_f64(jj, 4 * s);
    cost = cost + fhw::readlane_f64(jj, 4 * s + 1);
    cost = cost + fhw::readlane_f64(jj, 4 * s + 2);
  }
  const double cost_defect = fabs(cost - R.cost);

  if (tol.given) {
    if (corridor_best > tol.corridor) flags |= FH_CERT_CORRIDOR;
    if (corridor_assigned > tol.corridor) flags |= FH_CERT_ASSIGNMENT;
    if (x0_defect > tol.state) flags |= FH_CERT_X0;
    if (xf_defect > tol.state) flags |= FH_CERT_XF;
    if (continuity_defect > tol.state) flags |= FH_CERT_CONTINUITY;
    if (v_excess > tol.box || a_excess > tol.box || j_excess > tol.box) flags |= FH_CERT_BOX;
    const double ac = fabs(R.cost);
    if (cost_defect > tol.cost_rel * (ac > 1 ? ac : 1)) flags |= FH_CERT_COST;
  }
  w[0] = __hiloint2double(worst_seg, flags);
  w[2] = corridor_assigned; w[3] = corridor_best;
  w[4] = x0_defect; w[5] = xf_defect; w[6] = continuity_defect;
  w[7] = v_excess; w[8] = a_excess; w[9] = j_excess;
  w[10] = v_peak; w[11] = a_peak;
  w[12] = cost; w[13] = cost_defect;
  cert_store(out + i, lane, w);
}

}  // namespace fh

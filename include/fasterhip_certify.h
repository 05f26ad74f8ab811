/* fasterhip_certify.h: a certificate for every solved trajectory, computed on the device from what a caller holds (the fh_problem, the
 * face rows, the fh_result) against the UNREDUCED model of faster/src/solverGurobi.cpp: the constraints as they are written there, on the
 * 12 N polynomial coefficients.  Nothing of the solver is shared: no jerk space, no reduced space, no table, no active set.  A pure
 * measurement: no entry point of fasterhip.h changes, FH_ABI_VERSION stays.  C99 / C++11, includes fasterhip.h.
 *
 * THE MODEL.  Everything is IEEE double, no fused multiply-add, in the operation order written here (tests/certify_model.py restates it
 * in numpy and the kernel is compared with that bit for bit).  With a, b, c, d = coeff[t][0 + i], [3 + i], [6 + i], [9 + i] of segment t
 * and axis i, dt = result.dt, N = problem.n_seg, and products and sums taken left to right:
 *   pos(t, tau)  = a tau tau tau + b tau tau + c tau + d      (getPos,   solverGurobi.cpp:763)
 *   vel(t, tau)  = 3 a tau tau + 2 b tau + c                  (getVel,   :772)
 *   acc(t, tau)  = 6 a tau + 2 b                              (getAccel, :779)
 *   jerk(t)      = 6 a                                        (getJerk,  :786)
 * Control points (getCP0..3, :833-862, as fh_control_points evaluates them), Bn = b dt dt, Cn = c dt:
 *   cp0 = pos(t, 0)    cp1 = (Cn + 3 d) / 3    cp2 = (Bn + 2 Cn + 3 d) / 3    cp3 = pos(t, dt)
 * Row value of face f at a point p: ((a_x p_x + a_y p_y) + a_z p_z) - b.
 * "max" is always m = x > m ? x : m from -INFINITY and "min" m = x < m ? x : m from +INFINITY: a NaN never wins, and a maximum over
 * NaNs alone is -INFINITY.  (Which of +0 and -0 a maximum of zeros returns is not specified.)
 *   corridor (:237-288)   e(t, q) = max over the faces of polytope q and k = 0..3 of the row value at cp_k(t)  (no faces: -INFINITY)
 *                         corridor_assigned = max_t e(t, assign[t])
 *                         corridor_best     = max_t min_q e(t, q): the feasibility of the MIQP itself, whatever `assign` says
 *                         worst_seg         = the smallest t whose min_q e(t, q) equals corridor_best
 *                         n_poly == 0: both numbers are -INFINITY, worst_seg = -1
 *   x0 (:371-377)         x0_defect = max over axes of |pos(0,0) - x0[i]|, |vel(0,0) - x0[3+i]|, |acc(0,0) - x0[6+i]|
 *   xf (:349-354)         xf_defect = max over axes of |vel(N-1,dt) - xf[3+i]|, |acc(N-1,dt) - xf[6+i]| and, only when
 *                         force_final_pos != 0, |pos(N-1,dt) - xf[i]|
 *   continuity (:513-520) continuity_defect = max over t < N-1 and axes of |pos(t,dt) - pos(t+1,0)|, |vel(t,dt) - vel(t+1,0)|,
 *                         |acc(t,dt) - acc(t+1,0)|; 0 for N = 1
 *   box (:397-404)        v_excess = max_{t,i} (|vel(t,0)| - v_max), a_excess = max (|acc(t,0)| - a_max), j_excess = max (|jerk(t)| - j_max):
 *                         the rows the model has, at tau = 0 of every segment
 *   peaks                 what the model does NOT bound.  a_peak = max_{t,i} of |acc(t,0)|, |acc(t,dt)| (acc is linear in tau: this is
 *                         its maximum over the trajectory).  v_peak = max_{t,i} of |vel(t,0)|, |vel(t,dt)| and, when a != 0 and
 *                         tau* = (-b) / (3 a) satisfies 0 < tau* < dt, |vel(t, tau*)|
 *   cost (:113-119)       cost = sum_t sum_i (6 a)(6 a), accumulated from 0 in this order (t outer, axis inner);
 *                         cost_defect = |cost - result.cost|
 *
 * STRUCTURAL FLAGS.  Exactly one of them, or none; with one set, every other word of the certificate is 0.  Decided in this order:
 *   FH_CERT_UNSOLVED    result.solved == 0 (nothing else of the record is looked at)
 *   FH_CERT_BAD_INPUT   n_seg outside 1..FH_MAX_SEG; n_poly outside 0..FH_MAX_POLY; face_off[0] != 0 or face_off[q] > face_off[q+1] for
 *                       a q < n_poly; face_begin < 0 or face_begin + face_off[n_poly] > n_faces; with n_poly > 0, an assign[t], t < n_seg,
 *                       outside [0, n_poly).  Decided before any face is read: such a record causes no read outside [0, n_faces) or
 *                       outside the result.
 *   FH_CERT_NOT_FINITE  dt is not finite or dt <= 0, or a coefficient of rows 0 .. n_seg-1 is not finite (rows from n_seg on are dead
 *                       and never read)
 * The other bits compare the numbers with a caller's tolerances and are set only when `tol` is given: there are no default tolerances. */
#ifndef FASTERHIP_CERTIFY_H
#define FASTERHIP_CERTIFY_H
#include "fasterhip.h"
#ifdef __cplusplus
extern "C" {
#endif

enum {                           /* fh_certificate.flags */
  FH_CERT_UNSOLVED = 1,          /* result.solved == 0: every number below is 0                                     */
  FH_CERT_BAD_INPUT = 2,         /* the record cannot be evaluated (rules above): every number is 0                 */
  FH_CERT_NOT_FINITE = 4,        /* dt or a coefficient of rows 0..n_seg-1 is not finite, or dt <= 0: numbers 0     */
  FH_CERT_CORRIDOR = 8,          /* corridor_best > tol.corridor                                                    */
  FH_CERT_ASSIGNMENT = 16,       /* corridor_assigned > tol.corridor                                                */
  FH_CERT_X0 = 32,               /* x0_defect > tol.state                                                           */
  FH_CERT_XF = 64,               /* xf_defect > tol.state                                                           */
  FH_CERT_CONTINUITY = 128,      /* continuity_defect > tol.state                                                   */
  FH_CERT_BOX = 256,             /* v_excess, a_excess or j_excess > tol.box                                        */
  FH_CERT_COST = 512             /* cost_defect > tol.cost_rel * max(1, |result.cost|)   (max as above)             */
};

typedef struct fh_certificate { /* 128 B */
  int32_t flags, worst_seg, reserved_i[2];
  double corridor_assigned, corridor_best;
  double x0_defect, xf_defect, continuity_defect;
  double v_excess, a_excess, j_excess; /* the model's rows: tau = 0 of every segment              */
  double v_peak, a_peak;               /* what the model does not bound: the maximum over all tau */
  double cost, cost_defect;
  double reserved_d[2];
} fh_certificate;

typedef struct fh_certify_tol {
  double corridor, state, box, cost_rel;
} fh_certify_tol;

/* d_out[i] = the certificate of d_results[i] as a solution of d_problems[i] over the rows d_faces[0 .. n_faces).  tol == NULL: only the
 * structural flags are set; a tolerance that is negative or NaN: FH_ERR_ARG.  One wavefront per result, no working memory of the
 * context: results of one launch may be certified while the next solve launch of ANOTHER context runs.  Device pointers, asynchronous
 * on the context's stream; d_out aligned to 16 bytes (every device allocation is).  No CPU fallback: FH_ERR_DEVICE without a device. */
int fh_certify_batch_device(fh_ctx* ctx, const fh_problem* d_problems, const fh_face* d_faces, int64_t n_faces, const fh_result* d_results,
                            int n, const fh_certify_tol* tol, fh_certificate* d_out);
/* The same with host pointers: copies in, launches, copies out and waits (the staging buffers of fh_solve_batch). */
int fh_certify_batch(fh_ctx* ctx, const fh_problem* problems, const fh_face* faces, int64_t n_faces, const fh_result* results, int n,
                     const fh_certify_tol* tol, fh_certificate* out);

#ifdef __cplusplus
}
#endif
#endif /* FASTERHIP_CERTIFY_H */

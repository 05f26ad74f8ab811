// fh_fleet.hip.hpp — steady-state replanning of a fleet on the device (gfx950, wave64): what Faster::replan carries from one period
// to the next (/root/reference/faster/src/faster.cpp:296-595) — the committed plan, the start state A deltaT states into it, the
// vehicle status and the two factor windows — kept per vehicle in caller-owned device memory (fh_vehicle, include/fasterhip.h).
//
// fleet_init_kernel   : setTerminalGoal + the first updateState (faster.cpp:139-155, :267-279).          One lane per vehicle.
// fleet_begin_kernel  : G, dist_to_goal, GOAL_REACHED, k_end_whole, A, ra (faster.cpp:317-373).           One lane per vehicle.
// fleet_commit_kernel : the outcome of the cycle, appendToPlan, GOAL_SEEN, the factor windows (:548-588, :606-648).
//                       One wavefront per vehicle; the samples are written by sample_into, the sampler of fh_sample_batch.
// fleet_next_kernel   : getNextGoal `ticks` times (faster.cpp:699-723, without yaw).                     One lane per vehicle.
// fleet_set_goals_kernel : setTerminalGoal for a running fleet (:139-159: GOAL_REACHED becomes YAWING).  One lane per vehicle.
// fleet_next_yaw_kernel  : getNextGoal with getDesiredYaw and yaw, `ticks` times (:650-723).                One lane per vehicle.
// fleet_sense_kernel  : every vehicle clears, in its own unknown-voxel view, what it can see (no reference counterpart: the sensor
//                       model of include/fasterhip.h, checked against a numpy restatement).             One workgroup per vehicle.
// fleet_observe_kernel : every view learns the cloud points that lie in voxels it knows (no reference counterpart: the mapper's occupied
//                       cloud per vehicle, modelled on the shared cloud; checked against a numpy restatement). One wavefront per 64 points.
// The host restatement these kernels are checked against, cycle by cycle, is fhreplan::Planner (faster_amd/host/replan_stub.hpp),
// compiled by g++ without contraction into fused multiply-adds: the geometry here is written with contraction off, in the same
// operation order (a last-bit difference in G or ra changes a path, and a cycle later a factor window).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fasterhip.h"
#include "fh_sample.hip.hpp"

namespace fh {

__device__ __forceinline__ double fleet_norm3(double x, double y, double z) {
#pragma clang fp contract(off)
  return sqrt(x * x + y * y + z * z);  // V3::norm = sqrt(dot(*this)) (corridor_frontend.hpp)
}

// projectPointToBox (utils.cpp:1065-1115) as replan_stub.hpp's project_to_box restates it: the box of size w around c; p inside is
// returned as it is, else the nearest crossing of the segment c -> p with a face plane
__device__ inline void fleet_project_to_box(const double (&c)[3], const double (&p)[3], const double (&w)[3], double (&out)[3]) {
#pragma clang fp contract(off)
  double lo[3], hi[3];
  for (int a = 0; a < 3; a++) { lo[a] = c[a] - w[a] / 2; hi[a] = c[a] + w[a] / 2; }
  out[0] = p[0]; out[1] = p[1]; out[2] = p[2];
  if (p[0] < hi[0] && p[0] > lo[0] && p[1] < hi[1] && p[1] > lo[1] && p[2] < hi[2] && p[2] > lo[2]) return;
  double best = INFINITY;
  for (int ax = 0; ax < 3; ax++)
    for (int side = 0; side < 2; side++) {
      const double plane = side ? lo[ax] : hi[ax], den = p[ax] - c[ax];
      if (den == 0) continue;
      const double t = (plane - c[ax]) / den;
      if (t < 0 || t > 1) continue;
      double x[3];
      for (int a = 0; a < 3; a++) x[a] = c[a] + (p[a] - c[a]) * t;
      const double dist = fleet_norm3(x[0] - c[0], x[1] - c[1], x[2] - c[2]);
      if (dist < best) { best = dist; out[0] = x[0]; out[1] = x[1]; out[2] = x[2]; }
    }
}

__device__ __forceinline__ void fleet_clear_log(fh_vehicle& v) {
  v.stage = FH_FLEET_STAGE_NONE;
  v.needed_safe = 0; v.k_end_whole = 0; v.k_safe = 0; v.index_h = 0; v.n_whole = 0; v.n_safe = 0; v.reserved = 0;
  v.whole_factor = 0; v.safe_factor = 0;
}

__global__ void __launch_bounds__(256) fleet_init_kernel(fh_fleet_params par, const fh_state* __restrict__ states, const double* __restrict__ goals,
                                                         int n, int max_states, fh_vehicle* __restrict__ vehicles, fh_state* __restrict__ plans) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i >= n) return;
  fh_vehicle v;
  const fh_state s = states[i];
  for (int a = 0; a < 3; a++) { v.g_term[a] = goals[3 * i + a]; v.goal[a] = v.g_term[a]; }
  v.state = s;
  v.status = FH_VEHICLE_TRAVELING;
  v.plan_head = 0; v.plan_size = 1; v.active = 0;
  v.whole_init = 1; v.whole_final = 10; v.whole_inc = par.increment_whole;  // faster.cpp:57
  v.safe_init = 1; v.safe_final = 10; v.safe_inc = par.increment_safe;      // faster.cpp:68
  v.safe_factor_worked = 0;                                                 // solverGurobi.hpp:135
  v.ra = 0; v.dist_to_goal = 0;
  fleet_clear_log(v);
  vehicles[i] = v;
  plans[(size_t)i * (size_t)max_states] = s;  // the first updateState seeds the plan (faster.cpp:146-152)
}

__global__ void __launch_bounds__(256) fleet_begin_kernel(fh_fleet_params par, fh_vehicle* __restrict__ vehicles, const fh_state* __restrict__ plans,
                                                          int n, int max_states, fh_problem* __restrict__ whole, fh_problem* __restrict__ safe,
                                                          double* __restrict__ starts, double* __restrict__ goals, double* __restrict__ radius,
                                                          int32_t* __restrict__ active) {
#pragma clang fp contract(off)
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i >= n) return;
  fh_vehicle& v = vehicles[i];
  const double here[3] = {v.state.pos[0], v.state.pos[1], v.state.pos[2]};
  const double gterm[3] = {v.g_term[0], v.g_term[1], v.g_term[2]};
  const double w[3] = {par.wdx, par.wdy, par.wdz};
  double G[3];
  fleet_project_to_box(here, gterm, w, G);                                                        // :317-319
  const double dist = fleet_norm3(gterm[0] - here[0], gterm[1] - here[1], gterm[2] - here[2]);   // :331
  int status = v.status;
  if (dist < par.goal_radius) status = FH_VEHICLE_GOAL_REACHED;                                  // :332-335
  const bool run = status != FH_VEHICLE_GOAL_REACHED && status != FH_VEHICLE_YAWING && v.plan_size >= 1;  // :337-343 (:334: nor while YAWING)
  int k_end = 0;
  double ra = 0;
  double x0[9] = {here[0], here[1], here[2], 0, 0, 0, 0, 0, 0};
  if (run) {
    k_end = v.plan_size - par.delta_t;                                                            // :351
    k_end = k_end > 0 ? k_end : 0;
    const fh_state& A = plans[(size_t)i * (size_t)max_states + v.plan_head + v.plan_size - 1 - k_end];  // :352
    for (int a = 0; a < 3; a++) { x0[a] = A.pos[a]; x0[3 + a] = A.vel[a]; x0[6 + a] = A.accel[a]; }
    const double r = dist - 0.001;
    ra = par.ra < r ? par.ra : r;                                                                  // std::min(dist - 0.001, Ra), :373
  }
  v.status = status;
  v.active = run ? 1 : 0;
  for (int a = 0; a < 3; a++) v.goal[a] = G[a];
  v.ra = ra;
  v.dist_to_goal = dist;
  fleet_clear_log(v);
  v.k_end_whole = k_end;
  fh_problem& pw = whole[i];
  for (int j = 0; j < 9; j++) pw.x0[j] = x0[j];
  pw.f_init = v.whole_init; pw.f_final = v.whole_final; pw.f_inc = v.whole_inc;
  fh_problem& ps = safe[i];
  ps.f_init = v.safe_init; ps.f_final = v.safe_final; ps.f_inc = v.safe_inc;
  for (int a = 0; a < 3; a++) { starts[3 * i + a] = x0[a]; goals[3 * i + a] = G[a]; }
  radius[i] = ra;
  active[i] = run ? 1 : 0;
}

__device__ __forceinline__ bool fleet_problem_ok(const fh_problem& p, const fh_result& r) { return r.solved && p.n_seg >= 1 && p.n_seg <= FH_MAX_SEG; }

__global__ void __launch_bounds__(64) fleet_commit_kernel(fh_fleet_params par, fh_vehicle* __restrict__ vehicles, fh_state* __restrict__ plans, int n,
                                                          int max_states, const int32_t* __restrict__ n_points, const fh_problem* __restrict__ whole,
                                                          const fh_result* __restrict__ wres, const fh_problem* __restrict__ safe,
                                                          const fh_result* __restrict__ sres, UnknownGrid ug, UnknownViews vw) {
  __shared__ __attribute__((aligned(16))) double tile[64 * 12];
  __shared__ double coef[FH_MAX_SEG * 12];
  const int b = blockIdx.x;
  if (b >= n) return;
  ug.flags = view_flags(ug.flags, vw, b);
  const int lane = threadIdx.x;
  fh_vehicle& v = vehicles[b];
  if (!uniform_i32(v.active)) return;  // the log was cleared by fleet_begin_kernel (a GOAL_REACHED vehicle: stage 0)
  const fh_problem& pw = whole[b];
  const fh_result& rw = wres[b];
  const fh_problem& ps = safe[b];
  const fh_result& rs = sres[b];
  int stage = FH_FLEET_STAGE_NONE, need = 0, k = 0, iH = 0, size_w = 0, size_s = 0;
  double wf = 0, sf = 0;
  bool have_safe = false;
  if (n_points[b] < 2) {
    stage = FH_FLEET_STAGE_NO_PATH;                          // :361-367
  } else if (!fleet_problem_ok(pw, rw)) {
    stage = FH_FLEET_STAGE_NO_WHOLE;                         // :427-431 (a missing corridor marks the record n_seg = 0)
  } else {
    size_w = uniform_i32(sample_count(pw, rw));
    wf = rw.factor;
    need = choose_r_index(pw, rw, 0.0, par.rule, lane, k, &ug, &iH) ? 1 : 0;  // findIndexH / findIndexR, :456-475
    k = uniform_i32(k);
    iH = uniform_i32(iH);
    have_safe = need && fleet_problem_ok(ps, rs);
    if (need && !have_safe) {
      stage = FH_FLEET_STAGE_NO_SAFE;                        // :529-533
    } else {
      if (have_safe) {
        size_s = uniform_i32(sample_count(ps, rs));
        sf = rs.factor;
      }
      const int kept = v.plan_size - v.k_end_whole - 1;      // appendToPlan: the last k_end_whole + 1 states go (:617-623)
      const long long total = (long long)kept + (k + 1) + size_s;
      stage = total > max_states ? FH_FLEET_STAGE_OVERFLOW : FH_FLEET_STAGE_COMMITTED;
    }
  }
  stage = uniform_i32(stage);
  int new_size = 0, status = v.status;
  if (stage == FH_FLEET_STAGE_COMMITTED) {
    fh_state* base = plans + (size_t)b * (size_t)max_states;
    const int head = uniform_i32(v.plan_head);
    const int kept = uniform_i32(v.plan_size - v.k_end_whole - 1);
    // the kept prefix [head, head + kept) to [0, kept): chunk c reads head + 64 c + lane and writes 64 c + lane, each state read into
    // registers before it is written (a store of chunk c never touches what chunk c + 1 reads: head + 64 (c + 1) >= 64 c + 64)
    if (head != 0)
      for (int j0 = 0; j0 < kept; j0 += 64) {
        const int j = j0 + lane;
        fh_state s;
        if (j < kept) s = base[head + j];
        __syncthreads();
        if (j < kept) base[j] = s;
        __syncthreads();
      }
    __syncthreads();
    sample_into(pw, rw, size_w, k + 1, base + kept, tile, coef, lane);            // whole samples 0 .. k_safe (:627-633)
    int last = k;                                                                   // tile row of the last state written
    if (size_s > 0) {
      sample_into(ps, rs, size_s, size_s, base + kept + k + 1, tile, coef, lane);  // every safe sample (:635-640)
      last = size_s - 1;
    }
    new_size = kept + k + 1 + size_s;
    // plan_.back(): the last state written, still in the sampler's LDS tile (the same bits as in memory)
    const double* lp = &tile[(last % 64) * 12];
    {
#pragma clang fp contract(off)
      const double d = fleet_norm3(v.g_term[0] - lp[0], v.g_term[1] - lp[1], v.g_term[2] - lp[2]);
      if (d < par.goal_radius) status = FH_VEHICLE_GOAL_SEEN;                     // :563-570
    }
  }
  if (lane == 0) {
    v.stage = stage;
    if (stage >= FH_FLEET_STAGE_NO_SAFE) {  // (stages 3, 5, 6: the whole trajectory exists, findIndexH / findIndexR ran)
      v.needed_safe = need;
      v.index_h = iH;
      v.k_safe = k;
      v.n_whole = size_w;
    }
    if (stage >= FH_FLEET_STAGE_NO_SAFE) v.whole_factor = wf;
    if (have_safe) {                       // sg_safe_.factor_that_worked_ changes with every successful safe solve (solver_hip.cpp:132)
      v.safe_factor = sf;
      v.n_safe = size_s;
      v.safe_factor_worked = sf;
    }
    if (stage == FH_FLEET_STAGE_COMMITTED) {
      v.plan_head = 0;
      v.plan_size = new_size;
      v.status = status;
      // faster.cpp:578-584 — std::max(f - gamma, 1.0): 1.0 unless f - gamma is larger
      const double wi = wf - par.gamma_whole, si = v.safe_factor_worked - par.gamma_safe;
      v.whole_init = wi > 1.0 ? wi : 1.0;
      v.whole_final = wf + par.gammap_whole;
      v.whole_inc = par.increment_whole;
      v.safe_init = si > 1.0 ? si : 1.0;
      v.safe_final = v.safe_factor_worked + par.gammap_safe;
      v.safe_inc = par.increment_safe;
    }
  }
}

__global__ void __launch_bounds__(256) fleet_next_kernel(fh_vehicle* __restrict__ vehicles, const fh_state* __restrict__ plans, int n, int max_states,
                                                         int ticks, int follow, fh_state* __restrict__ goals) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i >= n) return;
  fh_vehicle& v = vehicles[i];
  const int size = v.plan_size, head = v.plan_head;
  fh_state g;
  for (int a = 0; a < 3; a++) { g.pos[a] = 0; g.vel[a] = 0; g.accel[a] = 0; g.jerk[a] = 0; }
  if (size > 0) {
    const int last = head + (ticks - 1 < size - 1 ? ticks - 1 : size - 1);  // front() of the last of the `ticks` calls
    g = plans[(size_t)i * (size_t)max_states + last];
    const int pops = ticks < size - 1 ? ticks : size - 1;                    // pop_front() while more than one state is left
    v.plan_head = head + pops;
    v.plan_size = size - pops;
    if (follow) v.state = g;
  }
  goals[i] = g;
}

// setTerminalGoal (faster.cpp:139-159) for the vehicles the mask selects
__global__ void __launch_bounds__(256) fleet_set_goals_kernel(fh_fleet_params par, fh_vehicle* __restrict__ vehicles, const double* __restrict__ new_goals,
                                                              const int32_t* __restrict__ mask, int n) {
#pragma clang fp contract(off)
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i >= n) return;
  if (mask && !mask[i]) return;
  fh_vehicle& v = vehicles[i];
  const double here[3] = {v.state.pos[0], v.state.pos[1], v.state.pos[2]};
  const double gterm[3] = {new_goals[3 * i], new_goals[3 * i + 1], new_goals[3 * i + 2]};
  const double w[3] = {par.wdx, par.wdy, par.wdz};
  double G[3];
  fleet_project_to_box(here, gterm, w, G);                                  // :148
  for (int a = 0; a < 3; a++) { v.g_term[a] = gterm[a]; v.goal[a] = G[a]; }
  if (v.status == FH_VEHICLE_GOAL_REACHED) v.status = FH_VEHICLE_YAWING;    // :149-152 (not done in any other status)
}

__global__ void __launch_bounds__(256) fleet_heading_init_kernel(const double* __restrict__ yaw0, int n, fh_heading* __restrict__ headings) {
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i >= n) return;
  fh_heading h;
  const double y = yaw0 ? yaw0[i] : 0.0;
  h.yaw = y; h.previous_yaw = y; h.dyaw_filtered = 0; h.goal_yaw = 0; h.goal_dyaw = 0;
  h.look_at[0] = 0; h.look_at[1] = 0; h.look_at[2] = 0;
  h.dir[0] = cos(y); h.dir[1] = sin(y);
  h.reserved[0] = 0; h.reserved[1] = 0;
  headings[i] = h;
}

// getNextGoal + getDesiredYaw + yaw (faster.cpp:650-723) `ticks` times: the plan cursor moves as in fleet_next_kernel; the yaw needs the
// goal position of every tick, so this one walks them.  Restated by fhreplan::Planner::getNextGoalYaw and tests/heading_model.py.
__global__ void __launch_bounds__(256) fleet_next_yaw_kernel(fh_yaw_params yp, fh_vehicle* __restrict__ vehicles, const fh_state* __restrict__ plans,
                                                             fh_heading* __restrict__ headings, int n, int max_states, int ticks, int follow,
                                                             fh_state* __restrict__ goals, double* __restrict__ goal_yaw) {
#pragma clang fp contract(off)
  const int i = (int)(blockIdx.x * 256 + threadIdx.x);
  if (i >= n) return;
  fh_vehicle& v = vehicles[i];
  const int size = v.plan_size, head = v.plan_head;
  fh_state g;
  for (int a = 0; a < 3; a++) { g.pos[a] = 0; g.vel[a] = 0; g.accel[a] = 0; g.jerk[a] = 0; }
  double out_yaw = 0, out_dyaw = 0;
  if (size > 0) {
    const fh_state* plan = plans + (size_t)i * (size_t)max_states + head;
    fh_heading h = headings[i];
    int status = v.status;
    const double gt[2] = {v.g_term[0], v.g_term[1]};
    const double pi = 3.14159265358979323846;  // M_PI
    for (int t = 0; t < ticks; t++) {
      const int at = t < size - 1 ? t : size - 1;  // front() of call t: popped while more than one state is left
      const double gx = plan[at].pos[0], gy = plan[at].pos[1];
      double yaw, dyaw;
      if (status == FH_VEHICLE_GOAL_REACHED) {     // :683-686
        dyaw = 0.0;
        yaw = h.previous_yaw;
      } else {
        const double tx = status == FH_VEHICLE_YAWING ? gt[0] : h.look_at[0], ty = status == FH_VEHICLE_YAWING ? gt[1] : h.look_at[1];
        const double desired = atan2(ty - gy, tx - gx);                                            // :674, :680
        double diff = desired - h.yaw;
        diff = fmod(diff + pi, 2 * pi);                                                            // angle_wrap, utils.cpp:496-502
        if (diff < 0) diff += 2 * pi;
        diff -= pi;
        if (fabs(diff) < 0.04 && status == FH_VEHICLE_YAWING) status = FH_VEHICLE_TRAVELING;       // :690-693
        const double not_filtered = copysign(1.0, diff) * yp.w_max;                                // :655
        h.dyaw_filtered = (1 - yp.alpha_filter_dyaw) * not_filtered + yp.alpha_filter_dyaw * h.dyaw_filtered;  // :657
        dyaw = h.dyaw_filtered;
        yaw = h.previous_yaw + h.dyaw_filtered * yp.dc;                                            // :662
      }
      h.previous_yaw = yaw;                                                                        // :718
      h.goal_yaw = yaw; h.goal_dyaw = dyaw;
      if (follow) h.yaw = yaw;
    }
    h.dir[0] = cos(h.previous_yaw); h.dir[1] = sin(h.previous_yaw);
    out_yaw = h.goal_yaw; out_dyaw = h.goal_dyaw;
    headings[i] = h;
    v.status = status;
    const int last = ticks - 1 < size - 1 ? ticks - 1 : size - 1;
    g = plan[last];
    const int pops = ticks < size - 1 ? ticks : size - 1;
    v.plan_head = head + pops;
    v.plan_size = size - pops;
    if (follow) v.state = g;
  }
  goals[i] = g;
  goal_yaw[2 * i] = out_yaw; goal_yaw[2 * i + 1] = out_dyaw;
}

// ---- sensing: every vehicle clears, in ITS view, the unknown flag of each voxel it can see (fh_fleet_sense_device) ----
// The model (include/fasterhip.h states it; tests restate it in numpy and compare every byte): voxel centre q = ((i + 0.5) res + origin) is
// in range of p when sqrt(dx dx + dy dy + dz dz) < r_sense, and visible when none of the points p + (q - p) (j / K), j = 1 .. K - 1,
// K = max(1, ceil(|q - p| / (0.5 res_map))), lies in an occupied cell of the map other than the cell q itself lies in (a point outside
// the map is free).  All in double, no contraction, in this order.  Only zeros are ever stored: vehicles that share a view clear the union, in any order.
//
// One workgroup of four wavefronts per vehicle.  Scan: a wavefront takes rows (iz, iy) of the lattice cells inside the bounding box of the
// sphere, lanes along x, and reads the flag bytes; a cell that is already known costs nothing more (steady state: nearly all of them).
// The cells that are unknown and in range are compacted into an LDS queue, so that the rays — 40 samples each at r_sense = 4 m, res 0.2 —
// are cast by full wavefronts and not by the few lanes of a row that need one.  The occupancy bits a ray can touch (the bounding box of
// the sphere in map cells, rows padded to 32 bits) are copied to LDS when the first queue is drained, and not at all by a vehicle whose
// surroundings are known already.
//
// FOV = true (fh_fleet_sense_fov_device): the sensor looks along (c, s) = fh_heading.dir and a voxel must also be in view: f = c dx + s dy > 0,
// |c dy - s dx| <= f tan_half_h, |dz| <= f tan_half_v.  The per-voxel predicate alone decides; what the field of view saves is the scan: the
// box scanned (and, in map cells, staged) is not the sphere's but one that holds the frustum cut at r_sense — every point of it is f (c, s) +
// l (-s, c) with 0 < f < r, |l| <= f th, so x - px lies in [min(0, r (c - |s| th)), max(0, r (c + |s| th))], y alike, |z - pz| <= r tv —
// intersected with the sphere's box, with the same cell of slack.  It contains p, so it holds every ray too.
#define FH_SENSE_QUEUE 2048      // cells waiting for their ray (LDS, 8 KB)
#define FH_SENSE_OCC_WORDS 6144  // staged occupancy (LDS, 24 KB: 54 x 54 rows of two words); a larger box is read from memory
struct SenseArgs {
  double r_sense;
  double ox, oy, oz, res;      // the lattice of the views
  int nx, ny, nz, n;
  unsigned char* flags;
  UnknownViews views;
  const unsigned* occ;         // the map: one bit per cell, cell (x, y, z) = bit (z my + y) mx + x
  double mox, moy, moz, mres;
  int mx, my, mz, stage;
  const fh_vehicle* vehicles;
  const fh_heading* headings;  // FOV only
  double th, tv;               // FOV only: tan of half the horizontal / vertical field of view
};

__device__ __forceinline__ int sense_clamp_cell(double v, int lo, int hi) {  // floor(v) clamped to [lo, hi], safe for any v
  const double f = floor(v);
  return !(f > (double)lo) ? lo : (f > (double)hi ? hi : (int)f);
}

template <bool FOV>
__global__ void __launch_bounds__(256) fleet_sense_kernel(SenseArgs a) {
#pragma clang fp contract(off)
  __shared__ int queue[FH_SENSE_QUEUE];
  __shared__ unsigned occ_lds[FH_SENSE_OCC_WORDS];
  __shared__ int q_count;
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = uniform_i32(tid >> 6);
  if (b >= a.n) return;
  const int view = a.views.view_of ? a.views.view_of[b] : b;
  if (view < 0 || view >= a.views.n_views) return;
  unsigned char* flags = a.flags + (size_t)view * a.views.stride;
  const double px = a.vehicles[b].state.pos[0], py = a.vehicles[b].state.pos[1], pz = a.vehicles[b].state.pos[2];
  if (!(fabs(px) < 1e300) || !(fabs(py) < 1e300) || !(fabs(pz) < 1e300)) return;  // (NaN or infinite: sees nothing)
  const double r = a.r_sense;
  // what the box around the scanned volume spans from p, per axis: the sphere's, or (FOV) the frustum's inside it
  double slx = -r, shx = r, sly = -r, shy = r, slz = -r, shz = r;
  double hc = 1.0, hs = 0.0;  // the heading's dir
  if (FOV) {
    hc = a.headings[b].dir[0]; hs = a.headings[b].dir[1];
    if (!(fabs(hc) < 1e300) || !(fabs(hs) < 1e300)) return;  // (NaN or infinite: sees nothing)
    const double big = fmax(fabs(hc), fabs(hs));
    if (!(big > 0.0)) return;                                // ((0, 0): f = 0 for every voxel, nothing is in view)
    const double uc = hc / big, us = hs / big;               // (scaled first: the squares of a very long or very short dir must not leave the range)
    const double len = sqrt(uc * uc + us * us);              // (in [1, sqrt 2])
    const double cn = uc / len, sn = us / len;               // (the predicate does not depend on the length of dir; the box must not either)
    slx = fmax(-r, fmin(0.0, r * (cn - fabs(sn) * a.th))); shx = fmin(r, fmax(0.0, r * (cn + fabs(sn) * a.th)));
    sly = fmax(-r, fmin(0.0, r * (sn - fabs(cn) * a.th))); shy = fmin(r, fmax(0.0, r * (sn + fabs(cn) * a.th)));
    slz = fmax(-r, -r * a.tv); shz = fmin(r, r * a.tv);
  }
  // lattice cells whose centre can be in range (and in view): one cell of slack on each side of that box
  const int x0 = sense_clamp_cell((px + slx - a.ox) / a.res - 1.0, 0, a.nx), x1 = sense_clamp_cell((px + shx - a.ox) / a.res + 1.0, -1, a.nx - 1);
  const int y0 = sense_clamp_cell((py + sly - a.oy) / a.res - 1.0, 0, a.ny), y1 = sense_clamp_cell((py + shy - a.oy) / a.res + 1.0, -1, a.ny - 1);
  const int z0 = sense_clamp_cell((pz + slz - a.oz) / a.res - 1.0, 0, a.nz), z1 = sense_clamp_cell((pz + shz - a.oz) / a.res + 1.0, -1, a.nz - 1);
  const int cx = x1 - x0 + 1, cy = y1 - y0 + 1, cz = z1 - z0 + 1;
  if (cx <= 0 || cy <= 0 || cz <= 0) return;  // the box misses the lattice
  // the map cells a sample point can fall into: the same box in the map's cells
  const int bx0 = sense_clamp_cell((px + slx - a.mox) / a.mres - 1.0, 0, a.mx), bx1 = sense_clamp_cell((px + shx - a.mox) / a.mres + 1.0, -1, a.mx - 1);
  const int by0 = sense_clamp_cell((py + sly - a.moy) / a.mres - 1.0, 0, a.my), by1 = sense_clamp_cell((py + shy - a.moy) / a.mres + 1.0, -1, a.my - 1);
  const int bz0 = sense_clamp_cell((pz + slz - a.moz) / a.mres - 1.0, 0, a.mz), bz1 = sense_clamp_cell((pz + shz - a.moz) / a.mres + 1.0, -1, a.mz - 1);
  const int bcx = bx1 - bx0 + 1, bcy = by1 - by0 + 1, bcz = bz1 - bz0 + 1;
  const int row_words = (bcx + 31) >> 5;
  const bool box_ok = bcx > 0 && bcy > 0 && bcz > 0;
  const bool can_stage = a.stage && box_ok && (long long)row_words * bcy * bcz <= FH_SENSE_OCC_WORDS;
  bool staged = false;
  if (tid == 0) q_count = 0;
  __syncthreads();

  const int chunks = (cx + 63) >> 6;        // 64 cells of a row at a time
  const int units = cy * cz * chunks;       // (row, chunk) pairs (at most the cells of the lattice, <= 2^30)
  for (int u0 = 0; u0 < units; u0 += 8) {
    // scan: two units per wavefront and trip, both flag loads in flight together
    int cell[2];
    unsigned char fl[2];
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const int u = u0 + 2 * wave + k;
      cell[k] = -1;
      fl[k] = 0;
      if (u < units) {
        const int row = chunks == 1 ? u : u / chunks, ix = (u - row * chunks) * 64 + lane;
        const int iz = row / cy, iy = row - iz * cy;
        if (ix < cx) {
          cell[k] = ((z0 + iz) * a.ny + (y0 + iy)) * a.nx + (x0 + ix);
          fl[k] = flags[cell[k]];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 2; k++) {
      bool cand = false;
      if (cell[k] >= 0 && fl[k] != 0) {
        const int ix = cell[k] % a.nx, t = cell[k] / a.nx, iy = t % a.ny, iz = t / a.ny;
        const double dx = ((double)ix + 0.5) * a.res + a.ox - px, dy = ((double)iy + 0.5) * a.res + a.oy - py,
                     dz = ((double)iz + 0.5) * a.res + a.oz - pz;
        cand = sqrt(dx * dx + dy * dy + dz * dz) < r;
        if (FOV) {
          const double f = hc * dx + hs * dy, l = hc * dy - hs * dx;
          cand = cand && f > 0.0 && fabs(l) <= f * a.th && fabs(dz) <= f * a.tv;
        }
      }
      const unsigned long long m = __ballot(cand);
      if (m) {
        int base = 0;
        if (lane == 0) base = atomicAdd(&q_count, __popcll(m));
        base = uniform_i32(base);
        if (cand) queue[base + __popcll(m & ((1ull << lane) - 1ull))] = cell[k];  // (drained below before it can overflow: 512 a trip)
      }
    }
    __syncthreads();
    const int waiting = q_count;
    __syncthreads();  // (every wavefront has read the count before the next trip adds to it)
    if (waiting == 0 || (waiting <= FH_SENSE_QUEUE - 512 && u0 + 8 < units)) continue;
    if (can_stage && !staged) {
      // local word w of local row (lz, ly) = the 32 bits of the map from cell (bx0 + 32 w, by0 + ly, bz0 + lz) on: two words of the map
      const int total_words = row_words * bcy * bcz;
      const long long map_bits = (long long)a.mx * a.my * a.mz;
      for (int w = tid; w < total_words; w += 256) {
        const int lrow = w / row_words, lw = w - lrow * row_words, lz = lrow / bcy, ly = lrow - lz * bcy;
        const long long bit = ((long long)(bz0 + lz) * a.my + (by0 + ly)) * a.mx + bx0 + 32 * lw;
        const long long wi = bit >> 5;
        const int sh = (int)(bit & 31);
        const unsigned lo = a.occ[wi];
        const unsigned hi = sh && (wi + 1) * 32 < map_bits ? a.occ[wi + 1] : 0u;  // (the word after the map's last is not the map's)
        occ_lds[w] = sh ? (lo >> sh) | (hi << (32 - sh)) : lo;  // (bits past the row's end belong to other rows and are never looked at)
      }
      staged = true;
      __syncthreads();
    }
    for (int e = tid; e < waiting; e += 256) {
      const int c = queue[e];
      const int ix = c % a.nx, t = c / a.nx, iy = t % a.ny, iz = t / a.ny;
      const double qx = ((double)ix + 0.5) * a.res + a.ox, qy = ((double)iy + 0.5) * a.res + a.oy, qz = ((double)iz + 0.5) * a.res + a.oz;
      const double dx = qx - px, dy = qy - py, dz = qz - pz;
      const double d = sqrt(dx * dx + dy * dy + dz * dz);
      const double qfx = floor((qx - a.mox) / a.mres), qfy = floor((qy - a.moy) / a.mres), qfz = floor((qz - a.moz) / a.mres);  // q's own map cell
      const double kf = ceil(d / (0.5 * a.mres));
      const int K = kf > 1.0 ? (int)kf : 1;  // (r_sense / res_map is bounded by fh_fleet_sense_device)
      bool blocked = false;
      for (int j = 1; j < K && !blocked; j++) {
        const double tt = (double)j / (double)K;
        const double fx = floor((px + dx * tt - a.mox) / a.mres), fy = floor((py + dy * tt - a.moy) / a.mres),
                     fz = floor((pz + dz * tt - a.moz) / a.mres);
        if (fx == qfx && fy == qfy && fz == qfz) continue;  // the map cell of q itself is not tested: an occupied cell is seen, not what is behind it
        if (!(fx >= 0.0 && fx < (double)a.mx && fy >= 0.0 && fy < (double)a.my && fz >= 0.0 && fz < (double)a.mz)) continue;  // outside the map: free
        const int sx = (int)fx, sy = (int)fy, sz = (int)fz;
        const int lx = sx - bx0, ly = sy - by0, lz = sz - bz0;
        if (staged && lx >= 0 && lx < bcx && ly >= 0 && ly < bcy && lz >= 0 && lz < bcz) {
          blocked = (occ_lds[(lz * bcy + ly) * row_words + (lx >> 5)] >> (lx & 31)) & 1u;
        } else {
          const long long id = ((long long)sz * a.my + sy) * a.mx + sx;
          blocked = (a.occ[id >> 5] >> (id & 31)) & 1u;
        }
      }
      if (!blocked) flags[c] = 0;
    }
    __syncthreads();
    if (tid == 0) q_count = 0;
    __syncthreads();
  }
}

// ---- observing: a view learns the points of the shared cloud that lie in voxels it knows (fh_fleet_observe_device) ----
// For view v and cloud point k: the voxel of the views' lattice that holds the point is (floor((x - ox) / res), floor((y - oy) / res),
// floor((z - oz) / res)), in double, no contraction; if it lies inside the lattice and its flag byte in view v is 0 (known), bit k & 31 of
// word k >> 5 of row v is set.  A point outside the lattice or with a coordinate that is not finite is never observed.  Bits are only
// ORed: nothing is cleared, and vehicles or calls that overlap cannot show.
// One wavefront takes 64 consecutive points of one view: the two mask words they fill.  It reads both words first and leaves when
// every bit of a point that exists is already set — in steady state nearly every word of what a vehicle has passed — before any
// coordinate or flag is read.  Otherwise the lanes whose bit is still clear look their voxel up, and one ballot holds both words:
// lane 0 ORs the low half into the first, lane 32 the high half into the second, each only when it adds a bit.
struct ObserveArgs {
  double ox, oy, oz, res;   // the lattice of the views
  int nx, ny, nz, n_views;
  const unsigned char* flags;
  size_t stride;
  const double* cloud;
  int n_cloud, words, blocks_per_view, pad;
  unsigned* mask;           // [n_views][words]
};

__global__ void __launch_bounds__(256) fleet_observe_kernel(ObserveArgs a) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, wave = uniform_i32(threadIdx.x >> 6);
  const int view = (int)(blockIdx.x / (unsigned)a.blocks_per_view), blk = (int)(blockIdx.x - (unsigned)view * (unsigned)a.blocks_per_view);
  const long long k0 = ((long long)blk * 4 + wave) * 64;
  if (view >= a.n_views || k0 >= (long long)a.n_cloud) return;  // (wave-uniform)
  const int k = (int)k0 + lane;
  unsigned* row = a.mask + (size_t)view * (size_t)a.words;
  const int w0 = (int)(k0 >> 5);
  const bool two = (k0 + 32) < (long long)a.n_cloud;  // the second word holds a point (and lies inside the row: words * 32 >= n_cloud)
  const unsigned have_lo = row[w0], have_hi = two ? row[w0 + 1] : 0u;
  const unsigned long long have = (unsigned long long)have_lo | ((unsigned long long)have_hi << 32);
  const bool need = k < a.n_cloud && !((have >> lane) & 1ull);
  if (!__ballot(need)) return;  // both words are full already: no coordinate, no flag is read
  bool seen = false;
  if (need) {
    const double x = a.cloud[3 * (size_t)k], y = a.cloud[3 * (size_t)k + 1], z = a.cloud[3 * (size_t)k + 2];
    const double fx = floor((x - a.ox) / a.res), fy = floor((y - a.oy) / a.res), fz = floor((z - a.oz) / a.res);
    // (a NaN or an infinity fails one of these comparisons)
    if (fx >= 0.0 && fx < (double)a.nx && fy >= 0.0 && fy < (double)a.ny && fz >= 0.0 && fz < (double)a.nz) {
      const size_t cell = ((size_t)(int)fz * (size_t)a.ny + (size_t)(int)fy) * (size_t)a.nx + (size_t)(int)fx;
      seen = a.flags[(size_t)view * a.stride + cell] == 0;
    }
  }
  const unsigned long long m = __ballot(seen);
  const unsigned lo = (unsigned)m, hi = (unsigned)(m >> 32);
  if (lane == 0 && lo) atomicOr(&row[w0], lo);
  if (lane == 32 && hi) atomicOr(&row[w0 + 1], hi);  // (hi != 0 only when the second word holds a point)
}

}  // namespace fh

// A fleet with HEADING in closed loop through the caller of the hot path, one vehicle at a time: replan_stub.hpp's Planner with its yaw
// logic (getNextGoalYaw: getDesiredYaw, yaw; M_; setNewTerminalGoal and the YAWING status — faster/src/faster.cpp:139-159, :334, :452,
// :496, :503-504, :650-723) driving SolverHip, the vehicle following its goals perfectly, yaw included.
// tests/test_gpu_fleet_heading.py runs the same vehicles through the device fleet (forward sense -> replan -> next goals with yaw, a new
// terminal goal in the cycle after GOAL_REACHED) and compares every cycle.  The driver is test_replan_fleet_views.cpp's with the heading
// added; every state is reached through the Planner's public calls (a fresh Planner has yaw = previous_yaw = 0, as the reference).
//
// Per vehicle i and cycle c: if new_goal[i][c], setNewTerminalGoal(second goal of i); the cells learned before this replan become known;
// updateState (the start state at c = 0, the last goal after that, its yaw included); updateMap; replan; then ticks[c] x
// (getNextGoalYaw, updateState(goal)).  Output per vehicle and cycle: int32[12] = ok, the ReplanLog (stage, needed_safe, k_end_whole,
// k_safe, indexH, n_whole, n_safe), the status after the replan, the plan size after the ticks, ReplanLog::m_writes, the status after
// the ticks; double[32] = both factors, both windows, G, ra, the last goal (12), M_ after the replan (3), yaw and dyaw of the last goal,
// previous_yaw, 2 spare; after the last cycle the whole plan.
// Scenario file: test_replan_fleet_views's, then [B][3] doubles (the second goals) and [B][C] int32 (new_goal).
//   usage: test_replan_fleet_heading <scenario.bin> <out.bin>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "replan_stub.hpp"
#include "solver_hip.hpp"

using fhfront::V3;

// SolverHip with its factor window readable (the reference's members are protected: solverGurobi.hpp:178-180)
struct WindowSolver : SolverHip {
  double f_init() const { return factor_initial_; }
  double f_final() const { return factor_final_; }
  double f_inc() const { return factor_increment_; }
};

static void put_state(std::vector<double>& out, const state& s) {
  const double v[12] = {s.pos.x(), s.pos.y(), s.pos.z(), s.vel.x(), s.vel.y(), s.vel.z(), s.accel.x(), s.accel.y(), s.accel.z(),
                        s.jerk.x(), s.jerk.y(), s.jerk.z()};
  out.insert(out.end(), v, v + 12);
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 3;
  int32_t hi[16];
  double hd[32];
  if (std::fread(hi, sizeof(hi), 1, f) != 1 || std::fread(hd, sizeof(hd), 1, f) != 1) return 3;
  const int N = hi[0], max_poly = hi[1], B = hi[5], n_occ = hi[6], C = hi[7], dims[3] = {hi[8], hi[9], hi[10]}, deltaT = hi[11];
  const size_t cells = (size_t)dims[0] * dims[1] * dims[2];
  std::vector<double> occ_raw((size_t)3 * n_occ), veh((size_t)12 * B);
  std::vector<int32_t> ticks(C);
  if (std::fread(occ_raw.data(), sizeof(double), occ_raw.size(), f) != occ_raw.size() || std::fread(veh.data(), sizeof(double), veh.size(), f) != veh.size() ||
      std::fread(ticks.data(), sizeof(int32_t), C, f) != (size_t)C)
    return 3;
  std::vector<std::vector<std::vector<int32_t>>> reveals(B, std::vector<std::vector<int32_t>>(C));
  for (int i = 0; i < B; i++)
    for (int c = 0; c < C; c++) {
      int32_t count = 0;
      if (std::fread(&count, sizeof(count), 1, f) != 1 || count < 0 || (size_t)count > cells) return 3;
      reveals[i][c].resize(count);
      if (count && std::fread(reveals[i][c].data(), sizeof(int32_t), count, f) != (size_t)count) return 3;
      for (int32_t id : reveals[i][c])
        if (id < 0 || (size_t)id >= cells) return 3;
    }
  std::vector<double> second((size_t)3 * B);
  std::vector<int32_t> new_goal((size_t)B * C);
  if (std::fread(second.data(), sizeof(double), second.size(), f) != second.size() ||
      std::fread(new_goal.data(), sizeof(int32_t), new_goal.size(), f) != new_goal.size())
    return 3;
  std::fclose(f);
  std::vector<V3> occ;
  for (int i = 0; i < n_occ; i++) occ.push_back(V3(occ_raw[3 * i], occ_raw[3 * i + 1], occ_raw[3 * i + 2]));
  const double res = hd[10], origin[3] = {hd[20], hd[21], hd[22]};

  fhreplan::Params par;
  par.N_whole = par.N_safe = N;
  par.max_poly_whole = par.max_poly_safe = max_poly;
  par.dc = hd[0]; par.v_max = hd[1]; par.a_max = hd[2]; par.j_max = hd[3]; par.Ra = hd[4]; par.drone_radius = hd[5]; par.decomp_radius = hd[6];
  par.dist_max_vertexes = hd[7]; par.delta_a = hd[8]; par.delta_H = hd[9]; par.res = res; par.inflation_jps = hd[11]; par.z_ground = 0.0;
  par.z_max = hd[12];
  par.map_fixed = true;
  for (int k = 0; k < 3; k++) { par.map_center[k] = hd[13 + k]; par.map_cells[k] = hi[2 + k]; }
  par.goal_radius = hd[16]; par.wdx = hd[17]; par.wdy = hd[18]; par.wdz = hd[19];
  par.gamma_whole = hd[23]; par.gammap_whole = hd[24]; par.increment_whole = hd[25];
  par.gamma_safe = hd[26]; par.gammap_safe = hd[27]; par.increment_safe = hd[28];
  par.deltaT = deltaT;
  par.jps = true;
  par.w_max = hd[29];
  par.alpha_filter_dyaw = hd[30];

  const int rec_i = 12, rec_d = 32;
  std::vector<std::vector<int32_t>> out_i(B);
  std::vector<std::vector<double>> out_d(B), out_plan(B);
#pragma omp parallel
  {
    fhreplan::Planner<WindowSolver> planner(par);
    std::vector<unsigned char> flags(cells);  // the view of the vehicle at hand
    std::vector<V3> unknown;
#pragma omp for schedule(dynamic, 1)
    for (int i = 0; i < B; i++) {
      planner.reset();
      planner.sg_whole_.factor_that_worked_ = 0;  // (reset() keeps them: one vehicle's factors must not leak into the next)
      planner.sg_safe_.factor_that_worked_ = 0;
      const double* p = &veh[(size_t)12 * i];
      state cur, G;
      cur.setPos(p[0], p[1], p[2]);
      cur.setVel(p[3], p[4], p[5]);
      cur.setAccel(p[6], p[7], p[8]);
      G.setPos(p[9], p[10], p[11]);
      planner.setTerminalGoal(G);
      std::fill(flags.begin(), flags.end(), (unsigned char)1);
      for (int c = 0; c < C; c++) {
        if (new_goal[(size_t)i * C + c]) {
          G.setPos(second[3 * i], second[3 * i + 1], second[3 * i + 2]);
          planner.setNewTerminalGoal(G);
        }
        for (int32_t id : reveals[i][c]) flags[id] = 0;
        unknown.clear();  // the unknown voxel centres of THIS vehicle, z-major, x fastest (the device's order)
        for (int iz = 0; iz < dims[2]; iz++)
          for (int iy = 0; iy < dims[1]; iy++)
            for (int ix = 0; ix < dims[0]; ix++)
              if (flags[((size_t)iz * dims[1] + iy) * dims[0] + ix])
                unknown.push_back(V3((ix + 0.5) * res + origin[0], (iy + 0.5) * res + origin[1], (iz + 0.5) * res + origin[2]));
        planner.updateState(cur);
        planner.updateMap(occ, unknown);
        fhreplan::ReplanLog L;
        const bool ok = planner.replan(&L);
        const V3 here = fhreplan::pos_of(cur), gterm = fhreplan::pos_of(G);
        const V3 Gp = fhreplan::project_to_box(here, gterm, par.wdx, par.wdy, par.wdz);
        const double dist = (gterm - here).norm();
        const double ra = std::min(dist - 0.001, par.Ra);
        state goal;
        goal.setZero();
        const int32_t status_replan = (int32_t)planner.status();
        const state M = planner.M();
        for (int t = 0; t < ticks[c]; t++) {
          planner.getNextGoalYaw(goal);
          planner.updateState(goal);  // a vehicle that tracks perfectly: state_.yaw is the goal's on the next tick
        }
        if (ticks[c] > 0) cur = goal;
        const int32_t ri[rec_i] = {ok ? 1 : 0, L.stage, L.needed_safe ? 1 : 0, L.k_end_whole, L.k_safe, L.index_H, (int32_t)L.n_whole, (int32_t)L.n_safe,
                                   status_replan, 0, L.m_writes, (int32_t)planner.status()};
        out_i[i].insert(out_i[i].end(), ri, ri + rec_i);
        const double rd[12] = {L.whole_factor, L.safe_factor, planner.sg_whole_.f_init(), planner.sg_whole_.f_final(), planner.sg_whole_.f_inc(),
                               planner.sg_safe_.f_init(), planner.sg_safe_.f_final(), planner.sg_safe_.f_inc(), Gp.x, Gp.y, Gp.z, ra};
        out_d[i].insert(out_d[i].end(), rd, rd + 12);
        put_state(out_d[i], goal);
        const double rh[8] = {M.pos.x(), M.pos.y(), M.pos.z(), goal.yaw, goal.dyaw, planner.previous_yaw(), 0.0, 0.0};
        out_d[i].insert(out_d[i].end(), rh, rh + 8);
        out_i[i][out_i[i].size() - 3] = (int32_t)planner.plan().size();  // plan size after the ticks
      }
      for (const state& s : planner.plan()) put_state(out_plan[i], s);
    }
  }
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 4;
  for (int i = 0; i < B; i++) {
    for (int c = 0; c < C; c++) {
      std::fwrite(&out_i[i][(size_t)rec_i * c], sizeof(int32_t), rec_i, o);
      std::fwrite(&out_d[i][(size_t)rec_d * c], sizeof(double), rec_d, o);
    }
    const int32_t np = (int32_t)(out_plan[i].size() / 12);
    std::fwrite(&np, sizeof(np), 1, o);
    std::fwrite(out_plan[i].data(), sizeof(double), out_plan[i].size(), o);
  }
  std::fclose(o);
  return 0;
}

// A fleet whose vehicles each know their OWN part of the world — unknown voxels AND occupied points — over many replan cycles through the
// caller of the hot path, one vehicle at a time: replan_stub.hpp's Planner (the restatement of Faster::replan, appendToPlan and getNextGoal: faster/src/faster.cpp:296-595,
// :606-648, :699-723) driving SolverHip, with the vehicle following its plan perfectly between two cycles.
// tests/test_gpu_fleet_occupancy.py runs the same vehicles through the device fleet with an unknown-voxel view and a mask over the points
// of the shared cloud per vehicle or team (fh_set_unknown_views_device, fh_set_point_views_device), grown on the device by sensing and
// observing, and compares every cycle.  (test_replan_fleet_views.cpp is the same driver with every occupied point known to everyone.)
//
// Per vehicle i: setTerminalGoal; its view starts all unknown; then per cycle c: the cells the vehicle learned before this replan
// (cell number (iz ny + iy) nx + ix) become known, and so do the cloud points it learned (index into the cloud); updateState (the start
// state at c = 0, the last goal after that), updateMap with the occupied points the vehicle knows, in the cloud's order, and the centres of the cells still unknown in view i, z-major, x fastest (the device's order), replan, then
// ticks[c] x getNextGoal.  Output as test_replan_fleet's: per vehicle and cycle the ReplanLog, the status, both factor windows, the
// plan size, G and ra and the last goal; after the last cycle the whole plan.
// Scenario file: the header, cloud, vehicles and ticks of test_replan_fleet's, then for every vehicle and cycle an int32 count and
// that many int32 cell numbers, then an int32 count and that many int32 point numbers.
//   usage: test_replan_fleet_occupancy <scenario.bin> <out.bin>
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
  std::vector<std::vector<std::vector<int32_t>>> reveals(B, std::vector<std::vector<int32_t>>(C)), learned(B, std::vector<std::vector<int32_t>>(C));
  for (int i = 0; i < B; i++)
    for (int c = 0; c < C; c++)
      for (int what = 0; what < 2; what++) {
        std::vector<int32_t>& list = what ? learned[i][c] : reveals[i][c];
        const size_t limit = what ? (size_t)n_occ : cells;
        int32_t count = 0;
        if (std::fread(&count, sizeof(count), 1, f) != 1 || count < 0 || (size_t)count > limit) return 3;
        list.resize(count);
        if (count && std::fread(list.data(), sizeof(int32_t), count, f) != (size_t)count) return 3;
        for (int32_t id : list)
          if (id < 0 || (size_t)id >= limit) return 3;
      }
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

  const int rec_i = 12, rec_d = 24;
  std::vector<std::vector<int32_t>> out_i(B);
  std::vector<std::vector<double>> out_d(B), out_plan(B);
#pragma omp parallel
  {
    fhreplan::Planner<WindowSolver> planner(par);
    std::vector<unsigned char> flags(cells);  // the view of the vehicle at hand
    std::vector<unsigned char> knows(n_occ);  // ... and the cloud points it knows
    std::vector<V3> unknown, mine;
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
      std::fill(knows.begin(), knows.end(), (unsigned char)0);
      for (int c = 0; c < C; c++) {
        for (int32_t id : reveals[i][c]) flags[id] = 0;
        unknown.clear();  // the unknown voxel centres of THIS vehicle, z-major, x fastest (the device's order)
        for (int iz = 0; iz < dims[2]; iz++)
          for (int iy = 0; iy < dims[1]; iy++)
            for (int ix = 0; ix < dims[0]; ix++)
              if (flags[((size_t)iz * dims[1] + iy) * dims[0] + ix])
                unknown.push_back(V3((ix + 0.5) * res + origin[0], (iy + 0.5) * res + origin[1], (iz + 0.5) * res + origin[2]));
        planner.updateState(cur);
        for (int32_t k : learned[i][c]) knows[k] = 1;
        mine.clear();  // cloud[mask_i], in the cloud's own order
        for (int k = 0; k < n_occ; k++)
          if (knows[k]) mine.push_back(occ[k]);
        planner.updateMap(mine, unknown);
        fhreplan::ReplanLog L;
        const bool ok = planner.replan(&L);
        const V3 here = fhreplan::pos_of(cur), gterm = fhreplan::pos_of(G);
        const V3 Gp = fhreplan::project_to_box(here, gterm, par.wdx, par.wdy, par.wdz);
        const double dist = (gterm - here).norm();
        const double ra = std::min(dist - 0.001, par.Ra);
        state goal;
        goal.setZero();
        for (int t = 0; t < ticks[c]; t++) planner.getNextGoal(goal);
        if (ticks[c] > 0) cur = goal;
        const int32_t ri[rec_i] = {ok ? 1 : 0, L.stage, L.needed_safe ? 1 : 0, L.k_end_whole, L.k_safe, L.index_H, (int32_t)L.n_whole, (int32_t)L.n_safe,
                                   (int32_t)planner.status(), 0, 0, 0};
        out_i[i].insert(out_i[i].end(), ri, ri + rec_i);
        const double rd[12] = {L.whole_factor, L.safe_factor, planner.sg_whole_.f_init(), planner.sg_whole_.f_final(), planner.sg_whole_.f_inc(),
                               planner.sg_safe_.f_init(), planner.sg_safe_.f_final(), planner.sg_safe_.f_inc(), Gp.x, Gp.y, Gp.z, ra};
        out_d[i].insert(out_d[i].end(), rd, rd + 12);
        put_state(out_d[i], goal);
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

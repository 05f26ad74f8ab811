// The yaw logic of replan_stub.hpp's Planner (getNextGoalYaw: getDesiredYaw, yaw, angle_wrap, the YAWING status — the restatement of
// faster/src/faster.cpp:650-723) on given sequences, tick by tick: what tests/heading_model.py must equal exactly.  No solver is
// involved: the Planner is instantiated on a type with no solver behind it and replan() is never called.
// Input (binary): int32 n_cases; per case int32 {status, n_plan, ticks, follow}, double {alpha, w_max, dc, yaw, previous_yaw,
// dyaw_filtered, g_term x, y, look_at x, y}, then n_plan x {x, y}.  Output: per case and tick double {yaw, dyaw, status}.
//   usage: test_heading_yaw <cases.bin> <out.bin>
#include <cstdint>
#include <cstdio>
#include <deque>
#include <vector>

#include "replan_stub.hpp"

struct NoSolver {  // the calls Planner's constructor makes (faster.cpp:52-71); nothing else is instantiated
  void setN(int) {}
  void createVars() {}
  void setDC(double) {}
  void setBounds(double*) {}
  void setForceFinalConstraint(bool) {}
  void setFactorInitialAndFinalAndIncrement(double, double, double) {}
  void setVerbose(int) {}
  void setThreads(int) {}
  void setWMax(double) {}
};

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  FILE* o = std::fopen(argv[2], "wb");
  if (!f || !o) return 3;
  int32_t n_cases = 0;
  if (std::fread(&n_cases, sizeof(n_cases), 1, f) != 1) return 3;
  for (int c = 0; c < n_cases; c++) {
    int32_t hi[4];
    double hd[10];
    if (std::fread(hi, sizeof(hi), 1, f) != 1 || std::fread(hd, sizeof(hd), 1, f) != 1 || hi[1] < 1) return 3;
    std::vector<double> xy((size_t)2 * hi[1]);
    if (std::fread(xy.data(), sizeof(double), xy.size(), f) != xy.size()) return 3;
    fhreplan::Params par;
    par.dc = hd[2];
    fhreplan::Planner<NoSolver> planner(par);
    planner.setYawParams(hd[1], hd[0]);
    state g, cur, M;
    g.setPos(hd[6], hd[7], 0.0);
    M.setPos(hd[8], hd[9], 0.0);
    planner.setTerminalGoal(g);
    std::deque<state> plan;
    for (int k = 0; k < hi[1]; k++) {
      state s;
      s.setPos(xy[2 * k], xy[2 * k + 1], 0.0);
      plan.push_back(s);
    }
    cur = plan.front();
    cur.yaw = hd[3];
    planner.updateState(cur);
    planner.setPlan(plan);
    planner.setHeadingState((fhreplan::Status)hi[0], hd[4], hd[5], M);
    for (int t = 0; t < hi[2]; t++) {
      state goal;
      if (!planner.getNextGoalYaw(goal)) return 4;
      if (hi[3]) planner.updateState(goal);  // a vehicle that tracks perfectly: state_.yaw = the goal's
      const double rec[3] = {goal.yaw, goal.dyaw, (double)(int)planner.status()};
      std::fwrite(rec, sizeof(double), 3, o);
    }
  }
  std::fclose(f);
  std::fclose(o);
  return 0;
}

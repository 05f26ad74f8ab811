// fh_spread.hip.hpp — the kernels of include/fasterhip_spread.h (which is the specification): the chooser of fh_reach.hip.hpp for a
// team, in which a candidate nearer than r_spread to a goal that a peer holds or was given by an earlier pass is left out.  Included
// by fh_reach.hip only, after fh_reach.hip.hpp.  d_work: a class byte per vehicle, then (from a multiple of 64 bytes) a row of
// FH_SPREAD_LIST int32 per vehicle.
//   spread_class_kernel : a thread per vehicle.  The prologue of reach_body per thread, the same expressions under fp contract(off):
//                         byte = the flags fasterhip_reach.h gives a vehicle that is not searched (WANTED .. BOX_TOO_LARGE, below 64)
//                         | class << 6.
//   spread_peers_kernel : a wavefront per vehicle.  A vehicle that is no searcher writes its final outputs.  A searcher scans all n
//                         vehicles in chunks of 64 ascending, lane = k, one coalesced class byte per lane; view, group, position or
//                         g_term are loaded only for a k of class searcher (below i) or standing.  The k that pass go to the row by
//                         ballot and rank, so the row ascends in k; lower and standing are counted beyond the cap.  Then lane 0 writes
//                         the OVERFLOW outputs, or the UNSETTLED ones, which stand unless a pass decides the vehicle.
//   spread_goals_kernel : launched once per pass p, a workgroup of 256 per vehicle.  Every wavefront reads the record of its vehicle and
//                         the decided_pass of the listed lower peers (aligned 4-byte loads).  A peer that this launch decides shows -1 or
//                         p, and both fail 0 <= . < p: the four wavefronts reach one verdict whatever the scheduling, so the barrier
//                         behind the verdict is reached by all or none.  A ready vehicle puts its claims into LDS — d_goals of a lower
//                         peer is read only when its decided_pass < p, so an earlier launch wrote it — and runs reach_body<true>.
// No atomics, no spin.  LDS of the pass kernel: reach_body's 32880 bytes + 32 x 3 doubles + 4 ints.
// Every address comes from a checked number: a class other than none says that the view is in [0, n_views); the row holds indices
// k < n that the scan wrote, and only the first lower + standing <= FH_SPREAD_LIST of them are read.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fasterhip_spread.h"
// (ReachArgs, reach_body, reach_finite, reach_box_lo / hi and fhw:: come from fh_reach.hip.hpp, which fh_reach.hip includes before this)

namespace fhp {

constexpr int SPREAD_NONE = 0, SPREAD_SEARCHER = 1, SPREAD_STANDING = 2;

struct SpreadArgs {
  ReachArgs r;             // (r.records is not used)
  double s2, reach2, near2;  // r_spread^2, ((r_max + r_max) + r_spread)^2, (r_max + r_spread)^2: rounded once on the host
  int n, pass;
  const int32_t* group;
  unsigned char* cls;      // [n]
  int32_t* rows;           // [n][FH_SPREAD_LIST]
  fh_spread_record* records;
};

__device__ __forceinline__ int spread_group(const SpreadArgs& s, int view) { return s.group ? s.group[view] : view; }

// the three outputs of vehicle i, by one thread: reach_store with the longer record
__device__ __forceinline__ void spread_store(const SpreadArgs& s, int i, int flags, int view, int cell, double d2, const ReachCounts& n, int group,
                                             int decided_pass, int lower, int claims, int claimed) {
#pragma clang fp contract(off)
  const ReachArgs& a = s.r;
  const unsigned long long* g = (const unsigned long long*)a.vehicles[i].g_term;
  unsigned long long* out = (unsigned long long*)(a.goals + 3 * (size_t)i);
  if (cell >= 0) {
    const int ix = cell % a.nx, iy = (cell / a.nx) % a.ny, iz = cell / (a.nx * a.ny);
    a.goals[3 * (size_t)i] = (ix + 0.5) * a.res + a.ox;
    a.goals[3 * (size_t)i + 1] = (iy + 0.5) * a.res + a.oy;
    a.goals[3 * (size_t)i + 2] = (iz + 0.5) * a.res + a.oz;
    flags |= FH_FRONTIER_FOUND;
  } else {
    out[0] = g[0]; out[1] = g[1]; out[2] = g[2];  // the bits of g_term, whatever they are
    if (claimed > 0) flags |= FH_SPREAD_CLAIMED;
  }
  a.mask[i] = cell >= 0 ? 1 : 0;
  fh_spread_record r;
  r.flags = flags; r.view = view; r.cell = cell; r.hops = n.hops;
  r.candidates = n.candidates; r.reachable = n.reachable; r.reached = n.reached; r.levels = n.levels;
  r.d2 = d2;
  r.group = group; r.decided_pass = decided_pass; r.lower = lower; r.claims = claims; r.claimed = claimed; r.reserved = 0;
  s.records[i] = r;
}

__global__ void __launch_bounds__(256) spread_class_kernel(SpreadArgs s) {
#pragma clang fp contract(off)
  const ReachArgs& a = s.r;
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= s.n) return;
  const fh_vehicle& V = a.vehicles[i];
  const int view = a.view_of ? a.view_of[i] : i;
  const int status = V.status, stage = V.stage;
  const double px = V.state.pos[0], py = V.state.pos[1], pz = V.state.pos[2];
  const double gx = V.g_term[0], gy = V.g_term[1], gz = V.g_term[2];
  const bool wanted = ((a.want & FH_FRONTIER_WANT_REACHED) && status == FH_VEHICLE_GOAL_REACHED) ||
                      ((a.want & FH_FRONTIER_WANT_NO_PATH) && stage == FH_FLEET_STAGE_NO_PATH) || (a.want & FH_FRONTIER_WANT_ALL);
  const bool has_view = view >= 0 && view < a.n_views;
  const bool g_finite = reach_finite(gx) && reach_finite(gy) && reach_finite(gz);
  const bool finite = reach_finite(px) && reach_finite(py) && reach_finite(pz) && g_finite;
  int flags = (wanted ? FH_FRONTIER_WANTED : 0) | (has_view ? 0 : FH_FRONTIER_NO_VIEW) | (finite ? 0 : FH_FRONTIER_BAD_POS);
  int cls = SPREAD_NONE;
  if (flags == FH_FRONTIER_WANTED) {  // eligible: the start cell and the box, as reach_body judges them
    const double sfx = floor((px - a.ox) / a.res), sfy = floor((py - a.oy) / a.res), sfz = floor((pz - a.oz) / a.res);
    if (!(sfx >= 0.0 && sfx < (double)a.nx && sfy >= 0.0 && sfy < (double)a.ny && sfz >= 0.0 && sfz < (double)a.nz)) {
      flags |= FH_REACH_START_OUTSIDE;
    } else {
      const int sx = (int)sfx, sy = (int)sfy, sz = (int)sfz;
      const int lo0 = reach_box_lo(floor((px - a.r_max - a.ox) / a.res) - 1.0, a.nx), hi0 = reach_box_hi(floor((px + a.r_max - a.ox) / a.res) + 1.0, a.nx);
      const int lo1 = reach_box_lo(floor((py - a.r_max - a.oy) / a.res) - 1.0, a.ny), hi1 = reach_box_hi(floor((py + a.r_max - a.oy) / a.res) + 1.0, a.ny);
      const int lo2 = reach_box_lo(floor((pz - a.r_max - a.oz) / a.res) - 1.0, a.nz), hi2 = reach_box_hi(floor((pz + a.r_max - a.oz) / a.res) + 1.0, a.nz);
      const bool holds = lo0 <= sx && sx <= hi0 && lo1 <= sy && sy <= hi1 && lo2 <= sz && sz <= hi2;
      const int rows_y = hi1 - lo1 + 1, rows_z = hi2 - lo2 + 1;
      const int wx = holds ? (hi0 - lo0 + 64) >> 6 : 0;
      const long long words = (long long)wx * rows_y * rows_z;
      if (!holds || words > (long long)REACH_WORDS) flags |= FH_REACH_BOX_TOO_LARGE;
      else cls = SPREAD_SEARCHER;
    }
  } else if (!wanted && has_view && status != FH_VEHICLE_GOAL_REACHED && g_finite) {
    cls = SPREAD_STANDING;
  }
  s.cls[i] = (unsigned char)(flags | (cls << 6));
}

__global__ void __launch_bounds__(64) spread_peers_kernel(SpreadArgs s) {
#pragma clang fp contract(off)
  const ReachArgs& a = s.r;
  const int i = (int)blockIdx.x, lane = (int)threadIdx.x;
  const int mine = fhw::uniform_i32((int)s.cls[i]);
  const int view = fhw::uniform_i32(a.view_of ? a.view_of[i] : i);
  const int flags = mine & 63;
  const int group = (flags & FH_FRONTIER_NO_VIEW) ? 0 : fhw::uniform_i32(spread_group(s, view));
  const ReachCounts none = {-1, 0, 0, 0, 0};
  if ((mine >> 6) != SPREAD_SEARCHER) {
    if (lane == 0) spread_store(s, i, flags, view, -1, INFINITY, none, group, 0, 0, 0, 0);
    return;
  }
  const fh_vehicle& V = a.vehicles[i];
  const double px = fhw::uniform_f64(V.state.pos[0]), py = fhw::uniform_f64(V.state.pos[1]), pz = fhw::uniform_f64(V.state.pos[2]);
  int32_t* row = s.rows + (size_t)i * FH_SPREAD_LIST;
  int total = 0, lower = 0, standing = 0;  // (uniform: sums of popcounts of ballots)
  for (int base = 0; base < s.n; base += 64) {
    const int k = base + lane;
    const int ck = k < s.n ? (int)s.cls[k] >> 6 : SPREAD_NONE;
    bool low = false, stand = false;
    if (k != i && ((ck == SPREAD_SEARCHER && k < i) || ck == SPREAD_STANDING)) {  // (its view is in range: the class says so)
      const int vk = a.view_of ? a.view_of[k] : k;
      if (spread_group(s, vk) == group) {
        const fh_vehicle& K = a.vehicles[k];
        const double* c = ck == SPREAD_SEARCHER ? K.state.pos : K.g_term;
        const double dx = c[0] - px, dy = c[1] - py, dz = c[2] - pz;
        const double d2 = dx * dx + dy * dy + dz * dz;
        low = ck == SPREAD_SEARCHER && d2 < s.reach2;
        stand = ck == SPREAD_STANDING && d2 < s.near2;
      }
    }
    // all 64 lanes are here again
    const unsigned long long bl = __ballot(low), bs = __ballot(stand), both = bl | bs;
    const int slot = total + fhw::rank_in(both);
    if ((low || stand) && slot < FH_SPREAD_LIST) row[slot] = k;
    total += __popcll(both);
    lower += __popcll(bl);
    standing += __popcll(bs);
  }
  if (lane == 0) {
    const bool over = total > FH_SPREAD_LIST;
    spread_store(s, i, flags | (over ? FH_SPREAD_OVERFLOW : FH_SPREAD_UNSETTLED), view, -1, INFINITY, none, group, over ? 0 : -1, lower, standing, 0);
  }
}

// what reach_body<true> reads and calls
struct SpreadClaims {
  const SpreadArgs* s;
  const double* pts;  // LDS
  int* sum;           // LDS
  int count, group, lower;
  double s2;
  __device__ __forceinline__ void store(const ReachArgs&, int i, int flags, int view, int cell, double d2, const ReachCounts& n, int claimed) const {
    spread_store(*s, i, flags, view, cell, d2, n, group, s->pass, lower, count, claimed);
  }
};

__global__ void __launch_bounds__(256) spread_goals_kernel(SpreadArgs s) {
  __shared__ double s_pts[3 * FH_SPREAD_LIST];
  __shared__ int s_sum[4];
  const int i = (int)blockIdx.x, lane = (int)threadIdx.x & 63;
  const fh_spread_record& R = s.records[i];
  if (fhw::uniform_i32(R.decided_pass) >= 0) return;  // decided, or no searcher (uniform over the workgroup: only this workgroup writes it, at its end)
  const int lower = fhw::uniform_i32(R.lower), standing = fhw::uniform_i32(R.claims), group = fhw::uniform_i32(R.group);
  const int total = lower + standing;  // (<= FH_SPREAD_LIST: a longer list is an OVERFLOW, decided in pass 0; tested all the same)
  if (total > FH_SPREAD_LIST) return;
  const int k = lane < total ? s.rows[(size_t)i * FH_SPREAD_LIST + lane] : -1;
  const bool listed = k >= 0 && k < s.n;
  const bool low = listed && ((int)s.cls[k] >> 6) == SPREAD_SEARCHER;
  const int dk = low ? s.records[k].decided_pass : 0;
  if (__ballot(low && !(dk >= 0 && dk < s.pass)) != 0ull) return;  // a lower peer is not decided yet (the same verdict in all four wavefronts)
  // the claims: every wavefront writes the same values to the same slots
  const bool has = listed && (low ? s.r.mask[k] == 1 : true);
  const unsigned long long bh = __ballot(has);
  if (has) {
    const double* c = low ? s.r.goals + 3 * (size_t)k : s.r.vehicles[k].g_term;
    const int j = fhw::rank_in(bh);
    s_pts[3 * j] = c[0]; s_pts[3 * j + 1] = c[1]; s_pts[3 * j + 2] = c[2];
  }
  __syncthreads();
  SpreadClaims x;
  x.s = &s; x.pts = s_pts; x.sum = s_sum;
  x.count = __popcll(bh); x.group = group; x.lower = lower;
  x.s2 = s.s2;
  reach_body<true>(s.r, x);
}

}  // namespace fhp

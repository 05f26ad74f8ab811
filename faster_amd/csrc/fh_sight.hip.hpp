// fh_sight.hip.hpp — the kernel of include/fasterhip_sight.h (which is the specification): K17's chooser with a gain that counts an
// unknown voxel of the ball only if the straight line of voxels from the candidate to it crosses no voxel that the vehicle knows to be
// occupied.  Included by fh_reach.hip only, after the header of K18's kernels; K17's helpers are called here (gain_ball, gain_take,
// GainBest, gain_before and the key helpers), as are those of fh_reach.hip.hpp.
//   sight_goals_kernel : ONE workgroup of 256 per vehicle; the body of K17's kernel, statement by statement, with three additions.
//     build   a fourth ballot per row segment: `wall`, ix <= hi0 && known && !pass, into a fifth bitmap; the popcounts of the ballots
//             are `walls`.  A lane beyond hi0 votes 0, as in the other three.
//     sight   per candidate sight_gain(): K17's gain_ball over `unk` (ball_gain), then the same function over `wall`.  No wall in the
//             ball: the gain is ball_gain, and the candidate has cost one more sweep of popcounts than in K17.  Otherwise the lanes
//             take the rows of the ball as gain_ball gives them out, and a lane walks, for every set bit of its masked `unk` words, the
//             line voxels l_1 .. l_(m-1): per axis a remainder mod 2 m that starts at m and grows by 2 |a| a step, a carry moves the
//             voxel by the sign of a — no division and no multiplication inside the walk.  A step reads one word of `wall`; the walk
//             of a voxel ends within four steps of the first wall.  The lanes diverge; wave_sum_i32 after the loop has all 64 again.
//     store   the two new words of the record; ball_gain of the choice is kept beside the wavefront's GainBest.
// No atomics, no spin, the barriers of K17's kernel.  LDS: 5 bitmaps of FH_REACH_MAX_WORDS words = 40 KB static and the slots of the
// reductions: three workgroups per CU, where K17's kernel has four.  Every address comes from a checked number: a line voxel lies
// between the candidate and a voxel of the ball's row, both inside the box on all three axes (|r(a, k)| <= |a|), so its word is < W.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fasterhip_sight.h"
#include "fh_wave.hip.hpp"
// (ReachArgs, the reach_ helpers, GainArgs, GainBest and the gain_ helpers: fh_reach.hip includes their headers before this one)

namespace fhp {

static_assert(sizeof(fh_sight_record) == 64 && sizeof(fh_sight_params) == 64, "include/fasterhip_sight.h");

struct SightArgs {
  GainArgs gn;  // gn.r: the lattice, the views, the map, d_goals and d_mask; g, g2, hop_cost, min_gain (gn.records is not used)
  fh_sight_record* records;
};

// Is the box voxel (ux, uy, uz) visible from the box voxel (cx, cy, cz)?  The line voxels l_1 .. l_(m-1) of include/fasterhip_sight.h,
// none of them a wall.  Both ends lie in the box, so every line voxel does.
__device__ __forceinline__ bool sight_visible(const unsigned long long* wall, int cx, int cy, int cz, int ux, int uy, int uz, int rows_y, int wx) {
  const int dx = ux - cx, dy = uy - cy, dz = uz - cz;
  const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy, az = dz < 0 ? -dz : dz;
  const int sx = dx < 0 ? -1 : 1, sy = dy < 0 ? -wx : wx, sz = dz < 0 ? -wx * rows_y : wx * rows_y;  // steps of x, and of the row's first word
  const int m = ax > ay ? (ax > az ? ax : az) : (ay > az ? ay : az);
  const int m2 = 2 * m, ix2 = 2 * ax, iy2 = 2 * ay, iz2 = 2 * az;
  int rx = m, ry = m, rz = m;                  // (2 |a| k + m) mod 2 m, k = 0
  int x = cx, row = (cz * rows_y + cy) * wx;  // the line voxel: its column and the first word of its row
  // four steps between two tests: the four reads of `wall` do not wait for each other (a walk that tested every step was bound by
  // the latency of LDS).  A step beyond l_(m-1) does not move and reads the last voxel again, so no address leaves the line.
  for (int k = 1; k < m; k += 4) {
    unsigned long long met = 0ull;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const bool on = k + j < m;
      rx += on ? ix2 : 0; ry += on ? iy2 : 0; rz += on ? iz2 : 0;  // (2 |a| <= 2 m: at most one carry a step)
      if (rx >= m2) { rx -= m2; x += sx; }
      if (ry >= m2) { ry -= m2; row += sy; }
      if (rz >= m2) { rz -= m2; row += sz; }
      met |= wall[row + (x >> 6)] >> (x & 63);
    }
    if (met & 1ull) return false;
  }
  return true;
}

// The unknown voxels of the box in the ball of radius g around the box voxel (bx, by, bz) that are visible from it, all arguments
// uniform and all 64 lanes here; *ball_gain: those of the ball, visible or not.  The per-candidate evaluation of the header: a chooser
// for a team could call it in place of gain_ball.
__device__ __forceinline__ int sight_gain(const unsigned long long* unk, const unsigned long long* wall, int bx, int by, int bz, int nbx, int rows_y,
                                          int rows_z, int wx, int g, int g2, int lane, int* ball_gain) {
  const int ball = gain_ball(unk, bx, by, bz, nbx, rows_y, rows_z, wx, g, g2, lane);
  *ball_gain = ball;
  if (ball == 0 || gain_ball(wall, bx, by, bz, nbx, rows_y, rows_z, wx, g, g2, lane) == 0) return ball;  // (uniform)
  // the rows of the ball as gain_ball gives them to the lanes
  const int y0 = by - g > 0 ? by - g : 0, y1 = by + g < rows_y - 1 ? by + g : rows_y - 1;
  const int z0 = bz - g > 0 ? bz - g : 0, z1 = bz + g < rows_z - 1 ? bz + g : rows_z - 1;
  const int ny = y1 - y0 + 1, n_rows = ny * (z1 - z0 + 1);
  int sum = 0;
  for (int j = lane; j < n_rows; j += 64) {
    const int jz = j / ny, ry = y0 + (j - jz * ny), rz = z0 + jz;
    const int dy = ry - by, dz = rz - bz;
    const int rem = g2 - dy * dy - dz * dz;
    if (rem < 0) continue;
    int hx = 0;  // the largest h with h h <= rem
#pragma unroll
    for (int b = 16; b > 0; b >>= 1) {
      const int h = hx + b;
      hx = h * h <= rem ? h : hx;
    }
    const int xa = bx - hx > 0 ? bx - hx : 0, xb = bx + hx < nbx - 1 ? bx + hx : nbx - 1;  // (xa <= bx <= xb, xb - xa <= 62)
    const int ka = xa >> 6, kb = xb >> 6;                                                    // (kb == ka or ka + 1, both < wx)
    const int row = (rz * rows_y + ry) * wx;
    const unsigned long long from = ~0ull << (xa & 63), to = ~0ull >> (63 - (xb & 63));
    unsigned long long first = unk[row + ka] & from, second = 0ull;
    if (ka == kb) first &= to;
    else second = unk[row + kb] & to;
    while (first) {
      const int ux = 64 * ka + (int)__builtin_ctzll(first);
      first &= first - 1ull;
      sum += sight_visible(wall, bx, by, bz, ux, ry, rz, rows_y, wx) ? 1 : 0;
    }
    while (second) {
      const int ux = 64 * kb + (int)__builtin_ctzll(second);
      second &= second - 1ull;
      sum += sight_visible(wall, bx, by, bz, ux, ry, rz, rows_y, wx) ? 1 : 0;
    }
  }
  return fhw::wave_sum_i32(sum);
}

// the three outputs of vehicle i, by one thread; ball: ball_gain of b.cell
__device__ __forceinline__ void sight_store(const SightArgs& s, int i, int flags, int view, int levels, int candidates, int reachable, int reached,
                                            const GainBest& b, int ball, int walls) {
#pragma clang fp contract(off)
  const ReachArgs& a = s.gn.r;
  const unsigned long long* g = (const unsigned long long*)a.vehicles[i].g_term;
  unsigned long long* out = (unsigned long long*)(a.goals + 3 * (size_t)i);
  const int cell = b.cell;
  if (cell >= 0) {
    const int ix = cell % a.nx, iy = (cell / a.nx) % a.ny, iz = cell / (a.nx * a.ny);
    a.goals[3 * (size_t)i] = (ix + 0.5) * a.res + a.ox;
    a.goals[3 * (size_t)i + 1] = (iy + 0.5) * a.res + a.oy;
    a.goals[3 * (size_t)i + 2] = (iz + 0.5) * a.res + a.oz;
    flags |= FH_FRONTIER_FOUND;
  } else {
    out[0] = g[0]; out[1] = g[1]; out[2] = g[2];  // the bits of g_term, whatever they are
  }
  if (reachable > 0 && b.poor == reachable) flags |= FH_SIGHT_ALL_POOR;
  a.mask[i] = cell >= 0 ? 1 : 0;
  fh_sight_record r;
  r.flags = flags; r.view = view; r.cell = cell >= 0 ? cell : -1; r.hops = cell >= 0 ? gain_key_hops(b.key) : -1;
  r.candidates = candidates; r.reachable = reachable; r.reached = reached; r.levels = levels;
  r.d2 = cell >= 0 ? b.d2 : INFINITY;
  r.gain = cell >= 0 ? b.gain : -1; r.utility = cell >= 0 ? gain_key_utility(b.key) : 0; r.poor = b.poor; r.best_gain = b.best_gain;
  r.ball_gain = cell >= 0 ? ball : -1; r.walls = walls;
  s.records[i] = r;
}

__global__ void __launch_bounds__(256) sight_goals_kernel(SightArgs s) {
#pragma clang fp contract(off)
  __shared__ unsigned long long s_pass[REACH_WORDS], s_cand[REACH_WORDS], s_a[REACH_WORDS], s_unk[REACH_WORDS], s_wall[REACH_WORDS];
  __shared__ double s_d2[4];
  __shared__ long long s_key[4];
  __shared__ int s_best[4][5], s_n[4], s_m[4], s_wl[4], s_start;
  __shared__ unsigned s_or[2][4];
  const GainArgs& gn = s.gn;
  const ReachArgs& a = gn.r;
  const int i = (int)blockIdx.x, t = (int)threadIdx.x, lane = t & 63, w = t >> 6;
  const fh_vehicle& V = a.vehicles[i];
  const int view = fhw::uniform_i32(a.view_of ? a.view_of[i] : i);
  const int status = fhw::uniform_i32(V.status), stage = fhw::uniform_i32(V.stage);
  const double px = fhw::uniform_f64(V.state.pos[0]), py = fhw::uniform_f64(V.state.pos[1]), pz = fhw::uniform_f64(V.state.pos[2]);
  const double gx = fhw::uniform_f64(V.g_term[0]), gy = fhw::uniform_f64(V.g_term[1]), gz = fhw::uniform_f64(V.g_term[2]);
  const bool wanted = ((a.want & FH_FRONTIER_WANT_REACHED) && status == FH_VEHICLE_GOAL_REACHED) ||
                      ((a.want & FH_FRONTIER_WANT_NO_PATH) && stage == FH_FLEET_STAGE_NO_PATH) || (a.want & FH_FRONTIER_WANT_ALL);
  const bool finite = reach_finite(px) && reach_finite(py) && reach_finite(pz) && reach_finite(gx) && reach_finite(gy) && reach_finite(gz);
  int flags = (wanted ? FH_FRONTIER_WANTED : 0) | (view >= 0 && view < a.n_views ? 0 : FH_FRONTIER_NO_VIEW) | (finite ? 0 : FH_FRONTIER_BAD_POS);
  GainBest best = {0ll, INFINITY, -1, -1, 0, -1};
  int best_ball = -1;  // ball_gain of best.cell
  if (flags != FH_FRONTIER_WANTED) {  // not eligible (uniform over the workgroup)
    if (t == 0) sight_store(s, i, flags, view, 0, 0, 0, 0, best, -1, 0);
    return;
  }
  // the start cell, tested as a double before it is an index
  const double sfx = floor((px - a.ox) / a.res), sfy = floor((py - a.oy) / a.res), sfz = floor((pz - a.oz) / a.res);
  if (!(sfx >= 0.0 && sfx < (double)a.nx && sfy >= 0.0 && sfy < (double)a.ny && sfz >= 0.0 && sfz < (double)a.nz)) {
    if (t == 0) sight_store(s, i, flags | FH_REACH_START_OUTSIDE, view, 0, 0, 0, 0, best, -1, 0);
    return;
  }
  const int sx = (int)sfx, sy = (int)sfy, sz = (int)sfz;
  const unsigned char* F = a.flags + (size_t)view * a.view_stride;
  const int lo0 = reach_box_lo(floor((px - a.r_max - a.ox) / a.res) - 1.0, a.nx), hi0 = reach_box_hi(floor((px + a.r_max - a.ox) / a.res) + 1.0, a.nx);
  const int lo1 = reach_box_lo(floor((py - a.r_max - a.oy) / a.res) - 1.0, a.ny), hi1 = reach_box_hi(floor((py + a.r_max - a.oy) / a.res) + 1.0, a.ny);
  const int lo2 = reach_box_lo(floor((pz - a.r_max - a.oz) / a.res) - 1.0, a.nz), hi2 = reach_box_hi(floor((pz + a.r_max - a.oz) / a.res) + 1.0, a.nz);
  // (s inside the lattice and r_max > 0: lo <= s <= hi on every axis; tested all the same, an empty box counts as too large)
  const bool holds = lo0 <= sx && sx <= hi0 && lo1 <= sy && sy <= hi1 && lo2 <= sz && sz <= hi2;
  const int rows_y = hi1 - lo1 + 1, rows_z = hi2 - lo2 + 1;
  const int wx = holds ? (hi0 - lo0 + 64) >> 6 : 0;                     // (hi0 - lo0 + 1 <= nx: no overflow)
  const long long words = (long long)wx * rows_y * rows_z;            // (rows_y rows_z <= ny nz < 2^31, wx < 2^26)
  if (!holds || words > (long long)REACH_WORDS) {
    if (t == 0) sight_store(s, i, flags | FH_REACH_BOX_TOO_LARGE, view, 0, 0, 0, 0, best, -1, 0);
    return;
  }
  const int W = (int)words, rows = rows_y * rows_z, slab = wx * rows_y, nbx = hi0 - lo0 + 1;
  const int slice = a.nx * a.ny;
  const int sw = ((sz - lo2) * rows_y + (sy - lo1)) * wx + ((sx - lo0) >> 6);  // the start's word (< W: s is in the box)
  const unsigned long long sbit = 1ull << ((sx - lo0) & 63);

  // ---- build: pass, cand, unk and wall, a wavefront per row ----
  int count = 0, n_wall = 0;  // candidates and walls (uniform over the wavefront: sums of popcounts of ballots)
  for (int r = w; r < rows; r += 4) {  // (r, and all that follows from it alone, is uniform over the wavefront)
    const int iz = lo2 + r / rows_y, iy = lo1 + r % rows_y;
    const double qz = (iz + 0.5) * a.res + a.oz, qy = (iy + 0.5) * a.res + a.oy;
    const bool z_ok = a.z_lo <= qz && qz <= a.z_hi;
    const double fy = floor((qy - a.moy) / a.mres), fz = floor((qz - a.moz) / a.mres);
    const bool row_in_map = fy >= 0.0 && fy < (double)a.my && fz >= 0.0 && fz < (double)a.mz;  // (outside the map: nothing passable in this row)
    const int map_row = row_in_map ? a.mx * ((int)fy + a.my * (int)fz) : 0;
    const double dy = qy - py, dz = qz - pz, ey = qy - gy, ez = qz - gz;
    const double dy2 = dy * dy, dz2 = dz * dz, ey2 = ey * ey, ez2 = ez * ez;
    const int c0 = (iz * a.ny + iy) * a.nx;
    for (int k = 0; k < wx; k++) {
      const int ix = lo0 + 64 * k + lane;
      const int c = c0 + ix;
      const bool known = ix <= hi0 && F[c] == 0, unk = ix <= hi0 && !known;  // (a lane beyond hi0 reads nothing)
      bool pass = row_in_map && known;
      const double qx = (ix + 0.5) * a.res + a.ox;
      if (pass) {
        const double fx = floor((qx - a.mox) / a.mres);
        pass = fx >= 0.0 && fx < (double)a.mx;
        if (pass) {
          const int id = map_row + (int)fx;
          pass = ((a.bits[id >> 5] >> (id & 31)) & 1u) == 0u;
        }
      }
      const bool wall = known && !pass;  // (known: ix <= hi0) known, and outside the map or occupied in it
      bool cand = pass && z_ok;
      if (cand) {
        const double dx = qx - px;
        const double d2 = dx * dx + dy2 + dz2;
        const double ex = qx - gx;
        const double e2 = ex * ex + ey2 + ez2;
        cand = d2 < a.r2 && !(e2 < a.a2);
        if (cand)
          cand = (ix > 0 && F[c - 1] != 0) || (ix < a.nx - 1 && F[c + 1] != 0) || (iy > 0 && F[c - a.nx] != 0) ||
                 (iy < a.ny - 1 && F[c + a.nx] != 0) || (iz > 0 && F[c - slice] != 0) || (iz < a.nz - 1 && F[c + slice] != 0);
      }
      // all 64 lanes are here again
      const unsigned long long bp = __ballot(pass), bc = __ballot(cand), bu = __ballot(unk), bw = __ballot(wall);
      count += __popcll(bc);
      n_wall += __popcll(bw);
      if (lane == 0) {
        const int u = r * wx + k;
        s_pass[u] = bp; s_cand[u] = bc; s_unk[u] = bu; s_wall[u] = bw;
        if (u == sw) s_start = (bc & sbit) != 0ull ? 1 : 0;  // (one word of the box is the start's)
      }
    }
  }
  // the start: level 0, whatever its flag and map bit are
#pragma unroll
  for (int j = 0; j < REACH_OWN; j++) {
    const int u = t + 256 * j;
    if (u < W) s_a[u] = u == sw ? sbit : 0ull;
  }
  if (lane == 0) { s_n[w] = count; s_wl[w] = n_wall; }
  __syncthreads();

  // ---- flood ----
  unsigned long long own_pass[REACH_OWN], own_cand[REACH_OWN], own_seen[REACH_OWN];
  unsigned own_nb[REACH_OWN];  // bit 0: owned (u < W); 1, 2: a word before / after in the same row; 4, 8: a row before / after in the slab; 16, 32: a slab below / above
#pragma unroll
  for (int j = 0; j < REACH_OWN; j++) {
    const int u = t + 256 * j;
    const bool own = u < W;
    const int k = own ? u % wx : 0, r = own ? u / wx : 0, ry = r % rows_y, rz = r / rows_y;
    own_nb[j] = own ? (1u | (k > 0 ? 2u : 0u) | (k < wx - 1 ? 4u : 0u) | (ry > 0 ? 8u : 0u) | (ry < rows_y - 1 ? 16u : 0u) | (rz > 0 ? 32u : 0u) |
                       (rz < rows_z - 1 ? 64u : 0u))
                    : 0u;
    own_pass[j] = own ? s_pass[u] : 0ull;  // (a word of pass and of cand is read by its owner alone: from here on their arrays are
    own_cand[j] = own ? s_cand[u] : 0ull;  //  the first nxt and the hit words, which a word's owner alone writes)
    own_seen[j] = own && u == sw ? sbit : 0ull;
  }
  const int candidates = s_n[0] + s_n[1] + s_n[2] + s_n[3], walls = s_wl[0] + s_wl[1] + s_wl[2] + s_wl[3];
  unsigned long long* cur = s_a;
  unsigned long long* nxt = s_pass;
  unsigned long long* const s_hit = s_cand;
  int n_reached = t == 0 ? 1 : 0, n_reachable = 0;  // sums over this thread's words (the start: thread 0's)
  int level = 0;
  bool cut = false;
  // (what steers the loop over the levels is made uniform for the compiler too: the branches around the evaluation are scalar, and
  //  the record of the wavefront stays in step over its lanes)
  bool hit = fhw::uniform_i32(s_start) != 0;  // a candidate in the level that cur holds
  if (hit && t == 0) n_reachable = 1;
  for (;;) {
    if (hit) {  // (uniform) the candidates of this level, each with its gain
      if (level == 0) {  // the start itself, by the first wavefront (the hit words are not written yet)
        if (w == 0) {
          const double qy = (sy + 0.5) * a.res + a.oy, qz = (sz + 0.5) * a.res + a.oz;
          const double dy = qy - py, dz = qz - pz;
          const double dy2 = dy * dy, dz2 = dz * dz;
          const double qx = (sx + 0.5) * a.res + a.ox;
          const double dx = qx - px;
          const double d2 = dx * dx + dy2 + dz2;
          const int c = (sz * a.ny + sy) * a.nx + sx;
          int ball;
          const int gain = sight_gain(s_unk, s_wall, sx - lo0, sy - lo1, sz - lo2, nbx, rows_y, rows_z, wx, gn.g, gn.g2, lane, &ball);
          gain_take(best, gn, gain, 0, d2, c);
          best_ball = best.cell == c ? ball : best_ball;
        }
      } else {
        for (int base = 0; base < W; base += 256) {  // wavefront w: the hit words u = w (mod 4), 64 at a time
          const int mine = base + 4 * lane + w;
          unsigned long long m = __ballot(mine < W && s_hit[mine] != 0ull);
          while (m) {  // (uniform)
            const int u = base + 4 * (int)__builtin_ctzll(m) + w;  // (< W: its lane has tested it)
            m &= m - 1ull;
            const unsigned long long hw = s_hit[u];
            unsigned h_lo = (unsigned)fhw::uniform_i32((int)(unsigned)hw), h_hi = (unsigned)fhw::uniform_i32((int)(unsigned)(hw >> 32));
            const int k = u % wx, r = u / wx, ry = r % rows_y, rz = r / rows_y;
            const int iy = lo1 + ry, iz = lo2 + rz;
            const double qy = (iy + 0.5) * a.res + a.oy, qz = (iz + 0.5) * a.res + a.oz;
            const double dy = qy - py, dz = qz - pz;
            const double dy2 = dy * dy, dz2 = dz * dz;
            while (h_lo | h_hi) {
              int b;
              if (h_lo) { b = (int)__builtin_ctz(h_lo); h_lo &= h_lo - 1u; }
              else { b = 32 + (int)__builtin_ctz(h_hi); h_hi &= h_hi - 1u; }
              const int bx = 64 * k + b, ix = lo0 + bx;
              const double qx = (ix + 0.5) * a.res + a.ox;
              const double dx = qx - px;
              const double d2 = dx * dx + dy2 + dz2;
              const int c = (iz * a.ny + iy) * a.nx + ix;
              int ball;
              const int gain = sight_gain(s_unk, s_wall, bx, ry, rz, nbx, rows_y, rows_z, wx, gn.g, gn.g2, lane, &ball);
              gain_take(best, gn, gain, level, d2, c);
              best_ball = best.cell == c ? ball : best_ball;
            }
          }
        }
      }
    }
    if (a.max_hops > 0 && level >= a.max_hops) {  // (cur is never empty)
      cut = true;
      break;
    }
    if (hit) __syncthreads();  // every wavefront has read this level's hit words before the next level's are written
    unsigned any = 0u;
#pragma unroll
    for (int j = 0; j < REACH_OWN; j++) {
      if (!(own_nb[j] & 1u)) continue;
      const int u = t + 256 * j;
      const unsigned nb = own_nb[j];
      const unsigned long long c = cur[u];
      unsigned long long v = (c << 1) | (c >> 1);
      if (nb & 2u) v |= cur[u - 1] >> 63;
      if (nb & 4u) v |= cur[u + 1] << 63;
      if (nb & 8u) v |= cur[u - wx];
      if (nb & 16u) v |= cur[u + wx];
      if (nb & 32u) v |= cur[u - slab];
      if (nb & 64u) v |= cur[u + slab];
      v &= own_pass[j] & ~own_seen[j];
      nxt[u] = v;
      own_seen[j] |= v;
      const unsigned long long h = v & own_cand[j];
      s_hit[u] = h;
      n_reached += __popcll(v);
      n_reachable += __popcll(h);
      any |= (v ? 1u : 0u) | (h ? 2u : 0u);
    }
    const unsigned wave_any = fhw::wave_or(any);
    if (lane == 0) s_or[level & 1][w] = wave_any;
    __syncthreads();
    const unsigned all = (unsigned)fhw::uniform_i32((int)(s_or[level & 1][0] | s_or[level & 1][1] | s_or[level & 1][2] | s_or[level & 1][3]));
    if (!(all & 1u)) break;
    level++;
    hit = (all & 2u) != 0u;
    unsigned long long* const swap = cur;
    cur = nxt;
    nxt = swap;
  }
  const int wave_reached = fhw::wave_sum_i32(n_reached), wave_reachable = fhw::wave_sum_i32(n_reachable);
  __syncthreads();  // (s_n was read above by every thread)
  if (lane == 0) {
    s_n[w] = wave_reached; s_m[w] = wave_reachable;
    s_best[w][0] = best.cell; s_best[w][1] = best.gain; s_best[w][2] = best.poor; s_best[w][3] = best.best_gain; s_best[w][4] = best_ball;
    s_key[w] = best.key;
    s_d2[w] = best.d2;
  }
  __syncthreads();
  if (t == 0) {
    GainBest b = {0ll, INFINITY, -1, -1, 0, -1};
    int ball = -1;
    for (int k = 0; k < 4; k++) {
      const bool take = s_best[k][0] >= 0 && gain_before(s_key[k], s_d2[k], s_best[k][0], b);
      b.key = take ? s_key[k] : b.key;
      b.d2 = take ? s_d2[k] : b.d2;
      b.cell = take ? s_best[k][0] : b.cell;
      b.gain = take ? s_best[k][1] : b.gain;
      ball = take ? s_best[k][4] : ball;
      b.poor += s_best[k][2];
      b.best_gain = s_best[k][3] > b.best_gain ? s_best[k][3] : b.best_gain;
    }
    if (cut) flags |= FH_REACH_CUT;
    sight_store(s, i, flags, view, level, candidates, s_m[0] + s_m[1] + s_m[2] + s_m[3], s_n[0] + s_n[1] + s_n[2] + s_n[3], b, ball, walls);
  }
}

}  // namespace fhp

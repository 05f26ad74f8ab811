// fh_gain.hip.hpp — the kernel of include/fasterhip_gain.h (which is the specification): for every vehicle that wants a goal, of the
// frontier voxels that a flood of known free space reaches the one with the largest utility = (unknown voxels of the box in a ball of
// gain_radius voxels around it) - hop_cost * (steps of the flood to it).  Included by fh_reach.hip only, after fh_spread.hip.hpp; it
// calls the small helpers of fh_reach.hip.hpp (reach_finite, reach_box_lo / hi, reach_before, ReachArgs) and has a body of its own.
//   gain_goals_kernel : ONE workgroup of 256 per vehicle; the exits of a vehicle that is not searched are those of reach_goals_kernel.
//     build   That kernel's build, float expression by float expression, so the candidates are its candidates, plus a third ballot per
//             row segment: `unk`, ix <= hi0 && F[c] != 0.  A lane beyond hi0 votes 0 in all three, so nothing leaks from the end of one
//             row into the next.  The wavefront that builds the start's word leaves "the start is a candidate" in an LDS slot.
//     flood   That kernel's flood.  `pass` and `cand` are dead in LDS once their owners hold them in registers (a word of them is read
//             by its owner alone), so the array of `pass` is the first nxt and the array of `cand` holds the HIT words, level & cand,
//             which the owners leave there in every level before the level's one barrier.
//     gain    When a level holds a candidate bit its candidates are evaluated before the next level.  Wavefront w takes the hit words
//             u = w (mod 4): its lanes load 64 of them at once, a ballot says which are not zero, and those are read again as uniform
//             values and their set bits enumerated.  For a candidate the 64 lanes take the (dy, dz) rows of the ball that lie inside
//             the box; hx = the largest h with h h <= g g - dy dy - dz dz by five integer steps (no float); the 2 hx + 1 voxels of the
//             row, clipped to [lo0, hi0], are one mask over one word of `unk` or two masks over two; popcounts, a wave_sum_i32: the
//             gain.  The best (utility, hops, d2, cell) and the counts are uniform values of the wavefront, merged across the four
//             through LDS at the end.  A second barrier, after the evaluation, keeps the next level's hit words from those still
//             being read: a level without candidates costs the one barrier it costs in reach_goals_kernel.
// LDS: 4 bitmaps of FH_REACH_MAX_WORDS words = 32 KB static (pass / nxt, cand / hit, cur, unk), and the slots of the reductions.
// Every address comes from a checked number, as in fh_reach.hip.hpp; a row of the ball is clipped to the box on all three axes before
// a word of `unk` is named, and a hit word is named by u < W.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fasterhip_gain.h"
#include "fh_wave.hip.hpp"
// (ReachArgs and the reach_ helpers: fh_reach.hip includes their header before this one)

namespace fhp {

struct GainArgs {
  ReachArgs r;  // (r.records is not used)
  int g, g2;    // gain_radius and its square
  int hop_cost, min_gain;
  fh_gain_record* records;
};

// The best candidate so far and the counts of include/fasterhip_gain.h: uniform over a wavefront.  Utility and hops are ONE number,
// key = utility * 65536 + (65535 - hops): the larger utility, then the fewer hops, is the larger key (hops < 65536: the box holds at
// most 64 FH_REACH_MAX_WORDS voxels; |utility| < 2^30), so the two cannot come apart and a comparison of the order is one of integers.
struct GainBest {
  long long key;
  double d2;
  int cell, gain;  // cell < 0: none yet
  int poor, best_gain;
};

__device__ __forceinline__ long long gain_key(int utility, int hops) { return (long long)utility * 65536 + (long long)(65535 - hops); }
__device__ __forceinline__ int gain_key_utility(long long key) { return (int)(key >> 16); }       // (floor: the low 16 bits are not negative)
__device__ __forceinline__ int gain_key_hops(long long key) { return 65535 - (int)(key & 65535); }

// (key, d2, c) before the best so far: the larger key, then the smaller (d2, c)
__device__ __forceinline__ bool gain_before(long long key, double d2, int c, const GainBest& b) {
  return b.cell < 0 || key > b.key || (key == b.key && reach_before(d2, c, b.d2, b.cell));
}

// a candidate with its gain, into the record of the wavefront
__device__ __forceinline__ void gain_take(GainBest& b, const GainArgs& a, int gain, int hops, double d2, int c) {
  b.best_gain = gain > b.best_gain ? gain : b.best_gain;
  const bool poor = gain < a.min_gain;
  b.poor += poor ? 1 : 0;
  const long long key = gain_key(gain - a.hop_cost * hops, hops);  // (|utility| < 2^30: gain <= 65536, hop_cost <= 16384)
  const bool take = !poor && gain_before(key, d2, c, b);
  b.key = take ? key : b.key;
  b.d2 = take ? d2 : b.d2;
  b.cell = take ? c : b.cell;
  b.gain = take ? gain : b.gain;
}

// The unknown voxels of the box in the ball of radius g around the box voxel (bx, by, bz), all uniform: the sum over the 64 lanes,
// which take the rows of the ball.  nbx, rows_y, rows_z: the box; wx: the words of a row; all 64 lanes are here.
__device__ __forceinline__ int gain_ball(const unsigned long long* unk, int bx, int by, int bz, int nbx, int rows_y, int rows_z, int wx, int g,
                                         int g2, int lane) {
  const int y0 = by - g > 0 ? by - g : 0, y1 = by + g < rows_y - 1 ? by + g : rows_y - 1;  // the rows of the ball inside the box
  const int z0 = bz - g > 0 ? bz - g : 0, z1 = bz + g < rows_z - 1 ? bz + g : rows_z - 1;
  const int ny = y1 - y0 + 1, n_rows = ny * (z1 - z0 + 1);  // (>= 1: the candidate's own row)
  int sum = 0;
  for (int j = lane; j < n_rows; j += 64) {
    const int jz = j / ny, ry = y0 + (j - jz * ny), rz = z0 + jz;
    const int dy = ry - by, dz = rz - bz;
    const int rem = g2 - dy * dy - dz * dz;
    if (rem < 0) continue;
    int hx = 0;  // the largest h with h h <= rem (rem <= 961: h <= 31)
#pragma unroll
    for (int b = 16; b > 0; b >>= 1) {
      const int h = hx + b;
      hx = h * h <= rem ? h : hx;
    }
    const int xa = bx - hx > 0 ? bx - hx : 0, xb = bx + hx < nbx - 1 ? bx + hx : nbx - 1;  // (xa <= bx <= xb, xb - xa <= 62)
    const int ka = xa >> 6, kb = xb >> 6;                                                    // (kb == ka or ka + 1, both < wx)
    const int row = (rz * rows_y + ry) * wx;
    const unsigned long long from = ~0ull << (xa & 63), to = ~0ull >> (63 - (xb & 63));
    if (ka == kb) sum += __popcll(unk[row + ka] & from & to);
    else sum += __popcll(unk[row + ka] & from) + __popcll(unk[row + kb] & to);
  }
  return fhw::wave_sum_i32(sum);
}

// the three outputs of vehicle i, by one thread
__device__ __forceinline__ void gain_store(const GainArgs& s, int i, int flags, int view, int levels, int candidates, int reachable, int reached,
                                           const GainBest& b) {
#pragma clang fp contract(off)
  const ReachArgs& a = s.r;
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
  if (reachable > 0 && b.poor == reachable) flags |= FH_GAIN_ALL_POOR;
  a.mask[i] = cell >= 0 ? 1 : 0;
  fh_gain_record r;
  r.flags = flags; r.view = view; r.cell = cell >= 0 ? cell : -1; r.hops = cell >= 0 ? gain_key_hops(b.key) : -1;
  r.candidates = candidates; r.reachable = reachable; r.reached = reached; r.levels = levels;
  r.d2 = cell >= 0 ? b.d2 : INFINITY;
  r.gain = cell >= 0 ? b.gain : -1; r.utility = cell >= 0 ? gain_key_utility(b.key) : 0; r.poor = b.poor; r.best_gain = b.best_gain;
  r.reserved = 0.0;
  s.records[i] = r;
}

__global__ void __launch_bounds__(256) gain_goals_kernel(GainArgs s) {
#pragma clang fp contract(off)
  __shared__ unsigned long long s_pass[REACH_WORDS], s_cand[REACH_WORDS], s_a[REACH_WORDS], s_unk[REACH_WORDS];
  __shared__ double s_d2[4];
  __shared__ long long s_key[4];
  __shared__ int s_best[4][4], s_n[4], s_m[4], s_start;
  __shared__ unsigned s_or[2][4];
  const ReachArgs& a = s.r;
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
  if (flags != FH_FRONTIER_WANTED) {  // not eligible (uniform over the workgroup)
    if (t == 0) gain_store(s, i, flags, view, 0, 0, 0, 0, best);
    return;
  }
  // the start cell, tested as a double before it is an index
  const double sfx = floor((px - a.ox) / a.res), sfy = floor((py - a.oy) / a.res), sfz = floor((pz - a.oz) / a.res);
  if (!(sfx >= 0.0 && sfx < (double)a.nx && sfy >= 0.0 && sfy < (double)a.ny && sfz >= 0.0 && sfz < (double)a.nz)) {
    if (t == 0) gain_store(s, i, flags | FH_REACH_START_OUTSIDE, view, 0, 0, 0, 0, best);
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
    if (t == 0) gain_store(s, i, flags | FH_REACH_BOX_TOO_LARGE, view, 0, 0, 0, 0, best);
    return;
  }
  const int W = (int)words, rows = rows_y * rows_z, slab = wx * rows_y, nbx = hi0 - lo0 + 1;
  const int slice = a.nx * a.ny;
  const int sw = ((sz - lo2) * rows_y + (sy - lo1)) * wx + ((sx - lo0) >> 6);  // the start's word (< W: s is in the box)
  const unsigned long long sbit = 1ull << ((sx - lo0) & 63);

  // ---- build: pass, cand and unk, a wavefront per row ----
  int count = 0;  // candidates (uniform over the wavefront: sums of popcounts of ballots)
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
      const unsigned long long bp = __ballot(pass), bc = __ballot(cand), bu = __ballot(unk);
      count += __popcll(bc);
      if (lane == 0) {
        const int u = r * wx + k;
        s_pass[u] = bp; s_cand[u] = bc; s_unk[u] = bu;
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
  if (lane == 0) s_n[w] = count;
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
  const int candidates = s_n[0] + s_n[1] + s_n[2] + s_n[3];
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
          const int gain = gain_ball(s_unk, sx - lo0, sy - lo1, sz - lo2, nbx, rows_y, rows_z, wx, s.g, s.g2, lane);
          gain_take(best, s, gain, 0, d2, (sz * a.ny + sy) * a.nx + sx);
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
              const int gain = gain_ball(s_unk, bx, ry, rz, nbx, rows_y, rows_z, wx, s.g, s.g2, lane);
              gain_take(best, s, gain, level, d2, (iz * a.ny + iy) * a.nx + ix);
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
    s_best[w][0] = best.cell; s_best[w][1] = best.gain; s_best[w][2] = best.poor; s_best[w][3] = best.best_gain;
    s_key[w] = best.key;
    s_d2[w] = best.d2;
  }
  __syncthreads();
  if (t == 0) {
    GainBest b = {0ll, INFINITY, -1, -1, 0, -1};
    for (int k = 0; k < 4; k++) {
      const bool take = s_best[k][0] >= 0 && gain_before(s_key[k], s_d2[k], s_best[k][0], b);
      b.key = take ? s_key[k] : b.key;
      b.d2 = take ? s_d2[k] : b.d2;
      b.cell = take ? s_best[k][0] : b.cell;
      b.gain = take ? s_best[k][1] : b.gain;
      b.poor += s_best[k][2];
      b.best_gain = s_best[k][3] > b.best_gain ? s_best[k][3] : b.best_gain;
    }
    if (cut) flags |= FH_REACH_CUT;
    gain_store(s, i, flags, view, level, candidates, s_m[0] + s_m[1] + s_m[2] + s_m[3], s_n[0] + s_n[1] + s_n[2] + s_n[3], b);
  }
}

}  // namespace fhp

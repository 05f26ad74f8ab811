// fh_far.hip.hpp — the kernels of include/fasterhip_far.h (which is the specification): for every vehicle that another chooser left
// without a goal, the nearest frontier of its WHOLE view that a flood over blocks of B x B x B voxels reaches.  Included by the host
// file of the flood choosers only, last of its device headers: ReachArgs, reach_finite and reach_before are those of the voxel flood.
//   far_need_kernel   : a thread per vehicle.  The searched predicate; a searched vehicle stores 1 to the need byte of its view (every
//                       writer stores the same value).
//   far_blocks_kernel : a workgroup of 256 per (word of 64 blocks, view); it returns at once for a view nobody needs.  A wavefront takes
//                       a block, its lanes run over the voxels of the block, x fastest, one flag byte per lane; the six neighbour bytes
//                       are loaded only for a voxel that is known, free and inside z.  "Any voxel of the block" is a ballot; the four
//                       answers of a block go to LDS, and the first wavefront turns the 64 answers of each bitmap into one word by a
//                       ballot: one 64-bit store per bitmap per word.  Integer work only; the bytes do not depend on scheduling.
//   far_goals_kernel  : ONE workgroup of 256 per vehicle.  A vehicle that is not searched has its three outputs written by thread 0.
//                       A searched one copies the four bitmaps of its view to LDS, takes the blocks within r_avoid of g_term out of T,
//                       and floods as the voxel flood does: cur / nxt in LDS, thread t owns the words t and t + 256 and keeps their
//                       seen words in registers, one barrier per level, "any bit" a wave_or into slots chosen by the level's parity.
//                           nxt[w] = ((cur[w] & LX[w]) << 1 | carry of (cur & LX)[w - 1] in the SAME row                       (+x)
//                                     | ((cur[w] >> 1 | carry of cur[w + 1]) & LX[w])                                            (-x)
//                                     | (cur & LY)[w - wx] | cur[w + wx] & LY[w] | (cur & LZ)[w - wx Cy] | cur[w + wx Cy] & LZ[w]) & ~seen[w]
//                       A link bit lives at the LOWER block of the pair, and LX is clear in the last block of a row: nothing leaks from
//                       the end of one row into the next.  In the first level that holds a target block every such bit computes D2; the
//                       smallest (D2, b) by wave_min / wave_min_i32 and across the wavefronts through LDS; then the workgroup scans the
//                       at most 16^3 voxels of that block for the smallest (d2, c) and counts them.  The flood runs on for the counts.
//                       Its body is far_body<false>; the chooser for a team instantiates far_body<true>.
// LDS of far_goals_kernel: 6 bitmaps of FH_FAR_MAX_WORDS words = 24 KB static, and the slots of the reductions.
// Every address comes from a checked number: view in [0, n_views), the start cell tested against the dims before it is used, block
// extents clipped to the lattice, neighbour bytes tested against the dims and neighbour words against the rows before they are loaded,
// the map cell tested against the map's dims before its word is loaded.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fasterhip_far.h"
#include "fh_wave.hip.hpp"

namespace fhp {

struct FarArgs {
  ReachArgs r;  // the lattice, the views, the vehicles, the map, a2, z_lo / z_hi, want, max_hops, goals and mask (r_max, r2, records: not read)
  int B, cx, cy, cz, wx, W;  // the blocks: edge, counts per axis, words per row of x, words per bitmap (<= FH_FAR_MAX_WORDS)
  int n;
  const int32_t* skip;
  unsigned long long* sums;  // [n_views][4][W]: T, LX, LY, LZ
  unsigned char* need;       // [n_views]
  fh_far_record* records;
};

constexpr int FAR_WORDS = FH_FAR_MAX_WORDS;  // words per bitmap
constexpr int FAR_OWN = FAR_WORDS / 256;     // words a thread owns

struct FarWho {
  int flags;      // the record's flags before FOUND and CUT
  bool searched;  // eligible, not skipped, s inside
  int sx, sy, sz;
};

// what the model says about vehicle i before anything is searched, from values the caller has read
__device__ __forceinline__ FarWho far_judge(const FarArgs& a, int view, int status, int stage, int skip, double px, double py, double pz, double gx,
                                            double gy, double gz) {
#pragma clang fp contract(off)
  const ReachArgs& r = a.r;
  const bool wanted = ((r.want & FH_FRONTIER_WANT_REACHED) && status == FH_VEHICLE_GOAL_REACHED) ||
                      ((r.want & FH_FRONTIER_WANT_NO_PATH) && stage == FH_FLEET_STAGE_NO_PATH) || (r.want & FH_FRONTIER_WANT_ALL);
  const bool finite = reach_finite(px) && reach_finite(py) && reach_finite(pz) && reach_finite(gx) && reach_finite(gy) && reach_finite(gz);
  FarWho w;
  w.flags = (wanted ? FH_FRONTIER_WANTED : 0) | (view >= 0 && view < r.n_views ? 0 : FH_FRONTIER_NO_VIEW) | (finite ? 0 : FH_FRONTIER_BAD_POS);
  w.searched = false;
  w.sx = w.sy = w.sz = 0;
  const bool eligible = w.flags == FH_FRONTIER_WANTED;
  if (skip != 0) w.flags |= FH_FAR_SKIPPED;
  if (!eligible || skip != 0) return w;
  // the start cell, tested as a double before it is an index
  const double sfx = floor((px - r.ox) / r.res), sfy = floor((py - r.oy) / r.res), sfz = floor((pz - r.oz) / r.res);
  if (!(sfx >= 0.0 && sfx < (double)r.nx && sfy >= 0.0 && sfy < (double)r.ny && sfz >= 0.0 && sfz < (double)r.nz)) {
    w.flags |= FH_REACH_START_OUTSIDE;
    return w;
  }
  w.searched = true;
  w.sx = (int)sfx; w.sy = (int)sfy; w.sz = (int)sfz;
  return w;
}

__global__ void __launch_bounds__(256) far_need_kernel(FarArgs a) {
  const int i = (int)(blockIdx.x * 256u + threadIdx.x);
  if (i >= a.n) return;
  const fh_vehicle& V = a.r.vehicles[i];
  const int view = a.r.view_of ? a.r.view_of[i] : i;
  const FarWho w = far_judge(a, view, V.status, V.stage, a.skip ? a.skip[i] : 0, V.state.pos[0], V.state.pos[1], V.state.pos[2], V.g_term[0],
                             V.g_term[1], V.g_term[2]);
  if (w.searched) a.need[view] = 1;  // (searched: view in [0, n_views))
}

// voxel (ix, iy, iz) of the lattice, inside it, is passable in the view F: the flag is 0 and the map cell of its centre is inside the
// map and clear (the expressions of the voxel flood)
__device__ __forceinline__ bool far_passable(const ReachArgs& r, const unsigned char* F, int ix, int iy, int iz) {
#pragma clang fp contract(off)
  if (F[(iz * r.ny + iy) * r.nx + ix] != 0) return false;
  const double qx = (ix + 0.5) * r.res + r.ox, qy = (iy + 0.5) * r.res + r.oy, qz = (iz + 0.5) * r.res + r.oz;
  const double fx = floor((qx - r.mox) / r.mres), fy = floor((qy - r.moy) / r.mres), fz = floor((qz - r.moz) / r.mres);
  if (!(fx >= 0.0 && fx < (double)r.mx && fy >= 0.0 && fy < (double)r.my && fz >= 0.0 && fz < (double)r.mz)) return false;
  const int id = r.mx * ((int)fy + r.my * (int)fz) + (int)fx;
  return ((r.bits[id >> 5] >> (id & 31)) & 1u) == 0u;
}

// a passable voxel is a target voxel: z_lo <= q.z <= z_hi and an unknown face neighbour inside the lattice
__device__ __forceinline__ bool far_target(const ReachArgs& r, const unsigned char* F, int ix, int iy, int iz) {
#pragma clang fp contract(off)
  const double qz = (iz + 0.5) * r.res + r.oz;
  if (!(r.z_lo <= qz && qz <= r.z_hi)) return false;
  const int slice = r.nx * r.ny, c = (iz * r.ny + iy) * r.nx + ix;
  return (ix > 0 && F[c - 1] != 0) || (ix < r.nx - 1 && F[c + 1] != 0) || (iy > 0 && F[c - r.nx] != 0) || (iy < r.ny - 1 && F[c + r.nx] != 0) ||
         (iz > 0 && F[c - slice] != 0) || (iz < r.nz - 1 && F[c + slice] != 0);
}

__global__ void __launch_bounds__(256) far_blocks_kernel(FarArgs a) {
  __shared__ unsigned char s_bit[4][64];
  const ReachArgs& r = a.r;
  const int t = (int)threadIdx.x, lane = t & 63, w = t >> 6;
  const int word = (int)blockIdx.x;  // (< W: the grid)
  const int k = word % a.wx, row = word / a.wx, by = row % a.cy, bz = row / a.cy;
  const int y0 = by * a.B, y1 = min(y0 + a.B, r.ny), z0 = bz * a.B, z1 = min(z0 + a.B, r.nz);
  const bool has_y = by + 1 < a.cy, has_z = bz + 1 < a.cz;  // (then y1 = y0 + B < ny: the voxel above the block's last row is inside)
  for (int view = (int)blockIdx.y; view < r.n_views; view += (int)gridDim.y) {
    if (fhw::uniform_i32((int)a.need[view]) == 0) continue;  // (uniform over the workgroup)
    const unsigned char* F = r.flags + (size_t)view * r.view_stride;
    for (int j = w; j < 64; j += 4) {  // (j, and all that follows from it alone, is uniform over the wavefront)
      const int bx = 64 * k + j;
      bool any_t = false, any_x = false, any_y = false, any_z = false;
      if (bx < a.cx) {
        const int x0 = bx * a.B, x1 = min(x0 + a.B, r.nx);
        const bool has_x = bx + 1 < a.cx;
        const int bw = x1 - x0, bh = y1 - y0, vol = bw * bh * (z1 - z0);  // (<= 16^3)
        for (int base = 0; base < vol; base += 64) {
          const int l = base + lane;
          bool vt = false, vx = false, vy = false, vz = false;
          if (l < vol) {
            const int ix = x0 + l % bw, iy = y0 + (l / bw) % bh, iz = z0 + l / (bw * bh);
            if (far_passable(r, F, ix, iy, iz)) {
              vt = !any_t && far_target(r, F, ix, iy, iz);
              vx = !any_x && has_x && ix == x1 - 1 && far_passable(r, F, ix + 1, iy, iz);
              vy = !any_y && has_y && iy == y1 - 1 && far_passable(r, F, ix, iy + 1, iz);
              vz = !any_z && has_z && iz == z1 - 1 && far_passable(r, F, ix, iy, iz + 1);
            }
          }
          // all 64 lanes are here again
          any_t = any_t || __ballot(vt) != 0ull;
          any_x = any_x || __ballot(vx) != 0ull;
          any_y = any_y || __ballot(vy) != 0ull;
          any_z = any_z || __ballot(vz) != 0ull;
          if (any_t && (any_x || !has_x) && (any_y || !has_y) && (any_z || !has_z)) break;  // (uniform) nothing left to learn
        }
      }
      if (lane == 0) {
        s_bit[0][j] = any_t ? 1 : 0; s_bit[1][j] = any_x ? 1 : 0; s_bit[2][j] = any_y ? 1 : 0; s_bit[3][j] = any_z ? 1 : 0;
      }
    }
    __syncthreads();
    if (w == 0) {
      unsigned long long* out = a.sums + (size_t)view * 4u * (size_t)a.W + (size_t)word;
#pragma unroll
      for (int m = 0; m < 4; m++) {
        const unsigned long long bits = __ballot(s_bit[m][lane] != 0);
        if (lane == 0) out[(size_t)m * (size_t)a.W] = bits;
      }
    }
    __syncthreads();  // (s_bit is written again for the next view)
  }
}

struct FarCounts {
  int block, hops, targets, reachable, reached, levels, members;
};

// the three outputs of vehicle i, by one thread
__device__ __forceinline__ void far_store(const FarArgs& a, int i, int flags, int view, int cell, double d2, double block_d2, const FarCounts& n) {
#pragma clang fp contract(off)
  const ReachArgs& r = a.r;
  const unsigned long long* g = (const unsigned long long*)r.vehicles[i].g_term;
  unsigned long long* out = (unsigned long long*)(r.goals + 3 * (size_t)i);
  if (cell >= 0) {
    const int ix = cell % r.nx, iy = (cell / r.nx) % r.ny, iz = cell / (r.nx * r.ny);
    r.goals[3 * (size_t)i] = (ix + 0.5) * r.res + r.ox;
    r.goals[3 * (size_t)i + 1] = (iy + 0.5) * r.res + r.oy;
    r.goals[3 * (size_t)i + 2] = (iz + 0.5) * r.res + r.oz;
    flags |= FH_FRONTIER_FOUND;
  } else {
    out[0] = g[0]; out[1] = g[1]; out[2] = g[2];  // the bits of g_term, whatever they are
  }
  r.mask[i] = cell >= 0 ? 1 : 0;
  fh_far_record q;
  q.flags = flags; q.view = view; q.cell = cell; q.block_cell = n.block; q.hops = n.hops;
  q.targets = n.targets; q.reachable = n.reachable; q.reached = n.reached; q.levels = n.levels; q.members = n.members;
  q.reserved[0] = 0; q.reserved[1] = 0;
  q.d2 = d2; q.block_d2 = block_d2;
  a.records[i] = q;
}

// the squared distance from x to [lo, hi], the centres of the first and the last voxel of a block along one axis
__device__ __forceinline__ double far_gap2(double x, int first, int last, double res, double o) {
#pragma clang fp contract(off)
  const double lo = (first + 0.5) * res + o, hi = (last + 0.5) * res + o;
  const double g = x < lo ? lo - x : (x > hi ? x - hi : 0.0);
  return g * g;
}

// D2 (or E2) of block (bx, by, bz) from the point (x, y, z)
__device__ __forceinline__ double far_block_d2(const FarArgs& a, int bx, int by, int bz, double x, double y, double z) {
#pragma clang fp contract(off)
  const ReachArgs& r = a.r;
  const double gx2 = far_gap2(x, bx * a.B, min(bx * a.B + a.B, r.nx) - 1, r.res, r.ox);
  const double gy2 = far_gap2(y, by * a.B, min(by * a.B + a.B, r.ny) - 1, r.res, r.oy);
  const double gz2 = far_gap2(z, bz * a.B, min(bz * a.B + a.B, r.nz) - 1, r.res, r.oz);
  return gx2 + gy2 + gz2;
}

struct FarNoClaims {};

// The body of far_goals_kernel, and with CLAIMS that of far_spread_goals_kernel (fh_apart.hpp): x.clear() takes the blocks that
// the claims of peers cover out of T in LDS before the flood, x.store() writes the longer record.  With CLAIMS false every
// `if constexpr` below is gone and the code is what the kernel held before it was a template.
template <bool CLAIMS, class X>
__device__ __forceinline__ void far_body(const FarArgs& a, const X& x) {
#pragma clang fp contract(off)
  __shared__ unsigned long long s_t[FAR_WORDS], s_lx[FAR_WORDS], s_ly[FAR_WORDS], s_lz[FAR_WORDS], s_a[FAR_WORDS], s_b[FAR_WORDS];
  __shared__ double s_bd2[4], s_vd2[4];
  __shared__ int s_bc[4], s_vc[4], s_vm[4], s_n[4], s_m[4], s_k[4];
  __shared__ unsigned s_or[2][4];
  const ReachArgs& r = a.r;
  const int i = (int)blockIdx.x, t = (int)threadIdx.x, lane = t & 63, w = t >> 6;
  const fh_vehicle& V = r.vehicles[i];
  const int view = fhw::uniform_i32(r.view_of ? r.view_of[i] : i);
  const int status = fhw::uniform_i32(V.status), stage = fhw::uniform_i32(V.stage);
  const int skip = fhw::uniform_i32(a.skip ? a.skip[i] : 0);
  const double px = fhw::uniform_f64(V.state.pos[0]), py = fhw::uniform_f64(V.state.pos[1]), pz = fhw::uniform_f64(V.state.pos[2]);
  const double gx = fhw::uniform_f64(V.g_term[0]), gy = fhw::uniform_f64(V.g_term[1]), gz = fhw::uniform_f64(V.g_term[2]);
  const FarWho who = far_judge(a, view, status, stage, skip, px, py, pz, gx, gy, gz);
  int flags = who.flags;
  const FarCounts none = {-1, -1, 0, 0, 0, 0, 0};
  if (!who.searched) {  // (uniform over the workgroup)
    if constexpr (!CLAIMS) {  // (with CLAIMS the count kernel has written the outputs of a vehicle that is not searched)
      if (t == 0) far_store(a, i, flags, view, -1, INFINITY, INFINITY, none);
    }
    return;
  }
  const int W = a.W, wx = a.wx, slab = a.wx * a.cy;
  const unsigned char* F = r.flags + (size_t)view * r.view_stride;
  const unsigned long long* S = a.sums + (size_t)view * 4u * (size_t)W;
  const int sbx = who.sx / a.B, sby = who.sy / a.B, sbz = who.sz / a.B;  // (< cx, cy, cz: s is inside the lattice)
  const int sw = (sbz * a.cy + sby) * wx + (sbx >> 6);                   // (< W)
  const unsigned long long sbit = 1ull << (sbx & 63);

  // ---- the view's summary into LDS, T without the blocks within r_avoid of g_term ----
  unsigned long long own_seen[FAR_OWN];
  unsigned own_nb[FAR_OWN];  // bit 0: owned (u < W); 1, 2: a word before / after in the same row; 4, 8: a row before / after in the slab; 16, 32: a slab below / above
  int n_targets = 0;
#pragma unroll
  for (int j = 0; j < FAR_OWN; j++) {
    const int u = t + 256 * j;
    const bool own = u < W;
    const int k = own ? u % wx : 0, row = own ? u / wx : 0, by = row % a.cy, bz = row / a.cy;
    own_nb[j] = own ? (1u | (k > 0 ? 2u : 0u) | (k < wx - 1 ? 4u : 0u) | (by > 0 ? 8u : 0u) | (by < a.cy - 1 ? 16u : 0u) | (bz > 0 ? 32u : 0u) |
                       (bz < a.cz - 1 ? 64u : 0u))
                    : 0u;
    own_seen[j] = own && u == sw ? sbit : 0ull;
    if (own) {
      unsigned long long tw = S[u];
      if (r.a2 > 0.0) {  // (with a2 == 0 no E2 is below it)
        unsigned long long h = tw;
        while (h) {
          const int bit = (int)__builtin_ctzll(h);
          h &= h - 1ull;
          const double e2 = far_block_d2(a, 64 * k + bit, by, bz, gx, gy, gz);
          if (e2 < r.a2) tw &= ~(1ull << bit);
        }
      }
      n_targets += __popcll(tw);
      s_t[u] = tw;
      s_lx[u] = S[(size_t)W + u];
      s_ly[u] = S[2 * (size_t)W + u];
      s_lz[u] = S[3 * (size_t)W + u];
      s_a[u] = u == sw ? sbit : 0ull;
      s_b[u] = 0ull;
    }
  }
  int n_claims = 0, n_standing = 0;  // (uniform)
  if constexpr (CLAIMS) {
    // every thread takes the claimed blocks out of the words of T it owns (and alone has written); the barriers inside are uniform
    const int n_claimed = x.clear(a, i, t, s_t, n_claims, n_standing);
    const int wave_claimed = fhw::wave_sum_i32(n_claimed);
    if (lane == 0) x.sum[w] = wave_claimed;
  }
  const int wave_targets = fhw::wave_sum_i32(n_targets);
  if (lane == 0) s_k[w] = wave_targets;
  __syncthreads();

  // ---- flood ----
  const int targets = s_k[0] + s_k[1] + s_k[2] + s_k[3];
  unsigned long long* cur = s_a;
  unsigned long long* nxt = s_b;
  int n_reached = t == 0 ? 1 : 0, n_reachable = 0;  // sums over this thread's words (the start: thread 0's)
  int level = 0, hops = -1, best_block = -1, best_cell = -1, members = 0;
  double best_bd2 = INFINITY, best = INFINITY;
  bool cut = false;
  bool hit = (s_t[sw] & sbit) != 0ull;  // a target block in the level that cur holds (uniform)
  if (hit && t == 0) n_reachable = 1;
  for (;;) {
    if (hit && hops < 0) {  // (uniform) the first level with a target block: the smallest (D2, b) of cur & T
      double b_d2 = INFINITY;
      int b_c = 0x7fffffff;
#pragma unroll
      for (int j = 0; j < FAR_OWN; j++) {
        const int u = t + 256 * j;
        unsigned long long h = (own_nb[j] & 1u) ? cur[u] & s_t[u] : 0ull;
        if (h) {
          const int k = u % wx, row = u / wx, by = row % a.cy, bz = row / a.cy;
          while (h) {
            const int bx = 64 * k + (int)__builtin_ctzll(h);
            h &= h - 1ull;
            const double d2 = far_block_d2(a, bx, by, bz, px, py, pz);
            const int b = (bz * a.cy + by) * a.cx + bx;
            if (reach_before(d2, b, b_d2, b_c)) { b_d2 = d2; b_c = b; }
          }
        }
      }
      // all 64 lanes are here again (no NaN: the gaps are differences of finite numbers)
      const double wave_d2 = fhw::wave_min(b_d2);
      const int wave_c = fhw::wave_min_i32(b_d2 == wave_d2 ? b_c : 0x7fffffff);
      if (lane == 0) { s_bd2[w] = wave_d2; s_bc[w] = wave_c; }
      __syncthreads();
      best_bd2 = s_bd2[0];
      best_block = s_bc[0];
      for (int k = 1; k < 4; k++)
        if (reach_before(s_bd2[k], s_bc[k], best_bd2, best_block)) { best_bd2 = s_bd2[k]; best_block = s_bc[k]; }
      hops = level;
      // the voxels of that block: the smallest (d2, c) of its target voxels, and their number
      const int bx = best_block % a.cx, by = (best_block / a.cx) % a.cy, bz = best_block / (a.cx * a.cy);  // (a set bit of T: a block of the lattice)
      const int x0 = bx * a.B, y0 = by * a.B, z0 = bz * a.B;
      const int bw = min(x0 + a.B, r.nx) - x0, bh = min(y0 + a.B, r.ny) - y0, vol = bw * bh * (min(z0 + a.B, r.nz) - z0);
      double v_d2 = INFINITY;
      int v_c = 0x7fffffff, v_n = 0;
      for (int l = t; l < vol; l += 256) {
        const int ix = x0 + l % bw, iy = y0 + (l / bw) % bh, iz = z0 + l / (bw * bh);
        if (far_passable(r, F, ix, iy, iz) && far_target(r, F, ix, iy, iz)) {
          const double qx = (ix + 0.5) * r.res + r.ox, qy = (iy + 0.5) * r.res + r.oy, qz = (iz + 0.5) * r.res + r.oz;
          const double dx = qx - px, dy = qy - py, dz = qz - pz;
          const double d2 = dx * dx + dy * dy + dz * dz;
          const int c = (iz * r.ny + iy) * r.nx + ix;
          v_n++;
          if (reach_before(d2, c, v_d2, v_c)) { v_d2 = d2; v_c = c; }
        }
      }
      const double wave_v = fhw::wave_min(v_d2);
      const int wave_vc = fhw::wave_min_i32(v_d2 == wave_v ? v_c : 0x7fffffff);
      const int wave_vn = fhw::wave_sum_i32(v_n);
      if (lane == 0) { s_vd2[w] = wave_v; s_vc[w] = wave_vc; s_vm[w] = wave_vn; }
      __syncthreads();
      best = s_vd2[0];
      best_cell = s_vc[0];
      for (int k = 1; k < 4; k++)
        if (reach_before(s_vd2[k], s_vc[k], best, best_cell)) { best = s_vd2[k]; best_cell = s_vc[k]; }
      members = s_vm[0] + s_vm[1] + s_vm[2] + s_vm[3];
    }
    if (r.max_hops > 0 && level >= r.max_hops) {  // (cur is never empty)
      cut = true;
      break;
    }
    unsigned any = 0u;
#pragma unroll
    for (int j = 0; j < FAR_OWN; j++) {
      if (!(own_nb[j] & 1u)) continue;
      const int u = t + 256 * j;
      const unsigned nb = own_nb[j];
      const unsigned long long c = cur[u], lx = s_lx[u];
      unsigned long long v = (c & lx) << 1;                  // +x inside the word
      unsigned long long down = c >> 1;                      // -x: block b from block b + 1, the link at b
      if (nb & 2u) v |= (cur[u - 1] & s_lx[u - 1]) >> 63;
      if (nb & 4u) down |= cur[u + 1] << 63;
      v |= down & lx;
      if (nb & 8u) v |= cur[u - wx] & s_ly[u - wx];
      if (nb & 16u) v |= cur[u + wx] & s_ly[u];
      if (nb & 32u) v |= cur[u - slab] & s_lz[u - slab];
      if (nb & 64u) v |= cur[u + slab] & s_lz[u];
      v &= ~own_seen[j];
      nxt[u] = v;
      own_seen[j] |= v;
      const unsigned long long h = v & s_t[u];
      n_reached += __popcll(v);
      n_reachable += __popcll(h);
      any |= (v ? 1u : 0u) | (h ? 2u : 0u);
    }
    const unsigned wave_any = fhw::wave_or(any);
    if (lane == 0) s_or[level & 1][w] = wave_any;
    __syncthreads();
    const unsigned all = s_or[level & 1][0] | s_or[level & 1][1] | s_or[level & 1][2] | s_or[level & 1][3];
    if (!(all & 1u)) break;
    level++;
    hit = (all & 2u) != 0u;
    unsigned long long* const swap = cur;
    cur = nxt;
    nxt = swap;
  }
  const int wave_reached = fhw::wave_sum_i32(n_reached), wave_reachable = fhw::wave_sum_i32(n_reachable);
  if (lane == 0) { s_n[w] = wave_reached; s_m[w] = wave_reachable; }
  __syncthreads();
  if (t == 0) {
    FarCounts n;
    n.block = hops >= 0 ? best_block : -1;
    n.hops = hops; n.targets = targets;
    n.reachable = s_m[0] + s_m[1] + s_m[2] + s_m[3];
    n.reached = s_n[0] + s_n[1] + s_n[2] + s_n[3];
    n.levels = level;
    n.members = hops >= 0 ? members : 0;
    if (cut) flags |= FH_REACH_CUT;
    if constexpr (CLAIMS)
      x.store(a, i, flags, view, hops >= 0 ? best_cell : -1, hops >= 0 ? best : INFINITY, hops >= 0 ? best_bd2 : INFINITY, n, n_claims, n_standing,
              x.sum[0] + x.sum[1] + x.sum[2] + x.sum[3]);
    else
      far_store(a, i, flags, view, hops >= 0 ? best_cell : -1, hops >= 0 ? best : INFINITY, hops >= 0 ? best_bd2 : INFINITY, n);
  }
}

__global__ void __launch_bounds__(256) far_goals_kernel(FarArgs a) { far_body<false>(a, FarNoClaims()); }

}  // namespace fhp

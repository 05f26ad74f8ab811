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
// The pieces that the three later far choosers (by gain, for a team, both) share with this one stand here, once, and their kernels
// call them: far_start (the vehicle's values, judged, and its start block), far_summary (the view's bitmaps into LDS, r_avoid out of T),
// far_expand and far_level_any (one level of the flood for an owned word; its barrier), far_scan_block (the voxels of the chosen
// block), far_put_goal and far_head (goal, mask, the 64 bytes every record begins with), and for the teams the class bytes,
// far_count_body (lower and standing, the outputs no pass decides) and far_claim_scan<COVER> (peers' claims out of T; with COVER
// also the blocks they cover, into a seventh bitmap).
// LDS of far_goals_kernel: 6 bitmaps of FH_FAR_MAX_WORDS words = 24 KB static, and the slots of the reductions.
// Every address comes from a checked number: view in [0, n_views), the start cell tested against the dims before it is used, block
// extents clipped to the lattice, neighbour bytes tested against the dims and neighbour words against the rows before they are loaded,
// the map cell tested against the map's dims before its word is loaded; in the claim scan k < n before a class byte is read, a class
// other than none says that the view is in [0, n_views), d_goals of a lower peer is read only under its mask, which an earlier launch
// wrote, a claim's voxel is tested against the dims as a double before it is a block, and the bits of C are clipped to the word and to
// [0, Cx).
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

// goal and mask of vehicle i, by one thread: the centre of voxel `cell`, or with cell < 0 the bits of g_term; -> FOUND or 0
__device__ __forceinline__ int far_put_goal(const ReachArgs& r, int i, int cell) {
#pragma clang fp contract(off)
  const unsigned long long* g = (const unsigned long long*)r.vehicles[i].g_term;
  unsigned long long* out = (unsigned long long*)(r.goals + 3 * (size_t)i);
  if (cell >= 0) {
    const int ix = cell % r.nx, iy = (cell / r.nx) % r.ny, iz = cell / (r.nx * r.ny);
    r.goals[3 * (size_t)i] = (ix + 0.5) * r.res + r.ox;
    r.goals[3 * (size_t)i + 1] = (iy + 0.5) * r.res + r.oy;
    r.goals[3 * (size_t)i + 2] = (iz + 0.5) * r.res + r.oz;
  } else {
    out[0] = g[0]; out[1] = g[1]; out[2] = g[2];  // the bits of g_term, whatever they are
  }
  r.mask[i] = cell >= 0 ? 1 : 0;
  return cell >= 0 ? FH_FRONTIER_FOUND : 0;
}

// the 64 bytes that the records of all four far choosers begin with (the host file asserts the offsets)
template <class R>
__device__ __forceinline__ void far_head(R& q, int flags, int view, int cell, double d2, double block_d2, const FarCounts& n) {
  q.flags = flags; q.view = view; q.cell = cell; q.block_cell = n.block; q.hops = n.hops;
  q.targets = n.targets; q.reachable = n.reachable; q.reached = n.reached; q.levels = n.levels; q.members = n.members;
  q.reserved[0] = 0; q.reserved[1] = 0;
  q.d2 = d2; q.block_d2 = block_d2;
}

// the three outputs of vehicle i, by one thread
__device__ __forceinline__ void far_store(const FarArgs& a, int i, int flags, int view, int cell, double d2, double block_d2, const FarCounts& n) {
  flags |= far_put_goal(a.r, i, cell);
  fh_far_record q;
  far_head(q, flags, view, cell, d2, block_d2, n);
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

// what a workgroup of a goals kernel knows of its vehicle i before it searches (every member uniform over the workgroup)
struct FarStart {
  int view;
  FarWho who;
  double px, py, pz, gx, gy, gz;  // position and g_term
  int sw;                         // the word of the start block (< W) and its bit; of a searched vehicle only
  unsigned long long sbit;
};

__device__ __forceinline__ FarStart far_start(const FarArgs& a, int i) {
#pragma clang fp contract(off)
  const ReachArgs& r = a.r;
  const fh_vehicle& V = r.vehicles[i];
  FarStart s;
  s.view = fhw::uniform_i32(r.view_of ? r.view_of[i] : i);
  const int status = fhw::uniform_i32(V.status), stage = fhw::uniform_i32(V.stage);
  const int skip = fhw::uniform_i32(a.skip ? a.skip[i] : 0);
  s.px = fhw::uniform_f64(V.state.pos[0]); s.py = fhw::uniform_f64(V.state.pos[1]); s.pz = fhw::uniform_f64(V.state.pos[2]);
  s.gx = fhw::uniform_f64(V.g_term[0]); s.gy = fhw::uniform_f64(V.g_term[1]); s.gz = fhw::uniform_f64(V.g_term[2]);
  s.who = far_judge(a, s.view, status, stage, skip, s.px, s.py, s.pz, s.gx, s.gy, s.gz);
  const int sbx = s.who.sx / a.B, sby = s.who.sy / a.B, sbz = s.who.sz / a.B;  // (< cx, cy, cz: s is inside the lattice)
  s.sw = (sbz * a.cy + sby) * a.wx + (sbx >> 6);
  s.sbit = 1ull << (sbx & 63);
  return s;
}

// the six bitmaps of a flood in LDS, FAR_WORDS words each: T, the links, and the two levels
struct FarMaps {
  unsigned long long *t, *lx, *ly, *lz, *a, *b;
};

// The view's summary into LDS, by the thread that owns the words u = t + 256 j: T without the blocks within r_avoid of g_term, the
// links, the start bit in m.a, and with COVER an empty word of the seventh bitmap c.  -> the set bits of T in this thread's words; in
// seen the start bit; in nb, per word: 1: owned (u < W); 2, 4: a word before / after in the same row; 8, 16: a row before / after in
// the slab; 32, 64: a slab below / above.
template <bool COVER>
__device__ __forceinline__ int far_summary(const FarArgs& a, const FarStart& s, int t, const FarMaps& m, unsigned long long* c,
                                           unsigned long long (&seen)[FAR_OWN], unsigned (&nb)[FAR_OWN]) {
#pragma clang fp contract(off)
  const ReachArgs& r = a.r;
  const int W = a.W, wx = a.wx;
  const unsigned long long* S = a.sums + (size_t)s.view * 4u * (size_t)W;
  int n_targets = 0;
#pragma unroll
  for (int j = 0; j < FAR_OWN; j++) {
    const int u = t + 256 * j;
    const bool own = u < W;
    const int k = own ? u % wx : 0, row = own ? u / wx : 0, by = row % a.cy, bz = row / a.cy;
    nb[j] = own ? (1u | (k > 0 ? 2u : 0u) | (k < wx - 1 ? 4u : 0u) | (by > 0 ? 8u : 0u) | (by < a.cy - 1 ? 16u : 0u) | (bz > 0 ? 32u : 0u) |
                   (bz < a.cz - 1 ? 64u : 0u))
                : 0u;
    seen[j] = own && u == s.sw ? s.sbit : 0ull;
    if (own) {
      unsigned long long tw = S[u];
      if (r.a2 > 0.0) {  // (with a2 == 0 no E2 is below it)
        unsigned long long h = tw;
        while (h) {
          const int bit = (int)__builtin_ctzll(h);
          h &= h - 1ull;
          const double e2 = far_block_d2(a, 64 * k + bit, by, bz, s.gx, s.gy, s.gz);
          if (e2 < r.a2) tw &= ~(1ull << bit);
        }
      }
      n_targets += __popcll(tw);
      m.t[u] = tw;
      m.lx[u] = S[(size_t)W + u];
      m.ly[u] = S[2 * (size_t)W + u];
      m.lz[u] = S[3 * (size_t)W + u];
      m.a[u] = u == s.sw ? s.sbit : 0ull;
      m.b[u] = 0ull;
      if constexpr (COVER) c[u] = 0ull;
    }
  }
  return n_targets;
}

// One level of the flood for the owned word u with neighbour bits nb: nxt[u] and -> the new bits, which join seen
__device__ __forceinline__ unsigned long long far_expand(const FarMaps& m, const unsigned long long* cur, unsigned long long* nxt, int u, unsigned nb,
                                                         int wx, int slab, unsigned long long& seen) {
  const unsigned long long c = cur[u], lx = m.lx[u];
  unsigned long long v = (c & lx) << 1;                  // +x inside the word
  unsigned long long down = c >> 1;                      // -x: block b from block b + 1, the link at b
  if (nb & 2u) v |= (cur[u - 1] & m.lx[u - 1]) >> 63;
  if (nb & 4u) down |= cur[u + 1] << 63;
  v |= down & lx;
  if (nb & 8u) v |= cur[u - wx] & m.ly[u - wx];
  if (nb & 16u) v |= cur[u + wx] & m.ly[u];
  if (nb & 32u) v |= cur[u - slab] & m.lz[u - slab];
  if (nb & 64u) v |= cur[u + slab] & m.lz[u];
  v &= ~seen;
  nxt[u] = v;
  seen |= v;
  return v;
}

// the level's barrier: -> the or of `any` over the workgroup.  The slots s_or[2][4] are chosen by the level's parity, so that one
// barrier per level suffices.
__device__ __forceinline__ unsigned far_level_any(unsigned any, unsigned (*s_or)[4], int level, int lane, int w) {
  const unsigned wave_any = fhw::wave_or(any);
  if (lane == 0) s_or[level & 1][w] = wave_any;
  __syncthreads();
  return s_or[level & 1][0] | s_or[level & 1][1] | s_or[level & 1][2] | s_or[level & 1][3];
}

struct FarVoxel {
  double d2;
  int cell, members;
};

// the voxels of block b, a set bit of T (so a block of the lattice), by the workgroup: the smallest (d2, c) of its target voxels from
// the point p, and their number.  One barrier; the slots are this scan's own.
__device__ __forceinline__ FarVoxel far_scan_block(const FarArgs& a, const unsigned char* F, int b, double px, double py, double pz, int t) {
#pragma clang fp contract(off)
  __shared__ double s_vd2[4];
  __shared__ int s_vc[4], s_vm[4];
  const ReachArgs& r = a.r;
  const int lane = t & 63, w = t >> 6;
  const int bx = b % a.cx, by = (b / a.cx) % a.cy, bz = b / (a.cx * a.cy);
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
  FarVoxel best = {s_vd2[0], s_vc[0], s_vm[0] + s_vm[1] + s_vm[2] + s_vm[3]};
  for (int k = 1; k < 4; k++)
    if (reach_before(s_vd2[k], s_vc[k], best.d2, best.cell)) { best.d2 = s_vd2[k]; best.cell = s_vc[k]; }
  return best;
}

// ---- the teams: vehicles of a group decided in passes, the goals of standing and lower peers are claims ----

constexpr int FAR_CLASS_NONE = 0, FAR_CLASS_SEARCHER = 1, FAR_CLASS_STANDING = 2;  // the class byte of a vehicle
constexpr int FAR_CHUNK = 256;                                                     // claims held in LDS at a time: one per thread

// the team's words of a record, which follow the 64 bytes of far_head
struct FarTeamCounts {
  int group, decided_pass, lower, standing, claims, claimed;
};

template <class R>
__device__ __forceinline__ void far_team_words(R& q, const FarTeamCounts& m) {
  q.group = m.group; q.decided_pass = m.decided_pass; q.lower = m.lower; q.standing = m.standing; q.claims = m.claims; q.claimed = m.claimed;
  q.reserved_tail[0] = 0; q.reserved_tail[1] = 0;
}

// what a claim scan reads
struct FarTeam {
  const unsigned char* cls;  // [n]
  const int32_t* grp;        // [n]
  int group;                 // the vehicle's own
  double s2;                 // r_spread^2
  int k;                     // claim_blocks (COVER only)
};

// The body of a count kernel, a wavefront per vehicle: lower -> lower_out[i]; a vehicle that is no searcher, or one with
// lower >= passes, has its final outputs written by lane 0 through store(flags, view, counts).
template <class STORE>
__device__ __forceinline__ void far_count_body(const FarArgs& a, const unsigned char* cls, const int32_t* grp, int32_t* lower_out, int passes,
                                               int unsettled, const STORE& store) {
#pragma clang fp contract(off)
  const ReachArgs& r = a.r;
  const int i = (int)blockIdx.x, lane = (int)threadIdx.x, n = a.n;
  const fh_vehicle& V = r.vehicles[i];
  const int view = fhw::uniform_i32(r.view_of ? r.view_of[i] : i);
  const int mine = fhw::uniform_i32((int)cls[i]), group = fhw::uniform_i32(grp[i]);
  if (mine != FAR_CLASS_SEARCHER) {  // (uniform)
    if (lane == 0) {
      const FarWho w = far_judge(a, view, V.status, V.stage, a.skip ? a.skip[i] : 0, V.state.pos[0], V.state.pos[1], V.state.pos[2], V.g_term[0],
                                 V.g_term[1], V.g_term[2]);
      const FarTeamCounts m = {group, 0, 0, 0, 0, 0};
      store(w.flags, view, m);
      lower_out[i] = 0;
    }
    return;
  }
  int lower = 0, standing = 0;  // (uniform: sums of popcounts of ballots)
  for (int base = 0; base < n; base += 64) {
    const int k = base + lane;
    const bool in = k < n && k != i;
    const int ck = in ? (int)cls[k] : FAR_CLASS_NONE;
    const bool peer = ck != FAR_CLASS_NONE && grp[k] == group;  // (a class other than none: a view in range)
    lower += __popcll(__ballot(peer && ck == FAR_CLASS_SEARCHER && k < i));
    standing += __popcll(__ballot(peer && ck == FAR_CLASS_STANDING));
  }
  if (lane == 0) {
    lower_out[i] = lower;
    if (lower >= passes) {  // (a searcher: its flags are WANTED alone)
      const FarTeamCounts m = {group, -1, lower, standing, standing, 0};
      store(FH_FRONTIER_WANTED | unsettled, view, m);
    }
  }
}

// The claim scan of a pass kernel, called by all 256 threads.  The n vehicles in chunks of 256, thread = k; the claim points of a chunk
// are compacted into LDS in ascending k by ballot and rank.  Every thread then takes the blocks with G2 < r_spread^2 of a claim out of
// the words u = t, t + 256, .. < W of T that it OWNS (and alone has written).  With COVER the block of each claim's voxel stands
// beside the point (3 x 16 bits, 0xffff: the voxel lies outside the lattice) and the thread sets in its words of C the blocks within
// k - 1 of it per axis.  A word of either bitmap has one writer, so the bytes do not depend on scheduling.  The barriers inside are
// uniform.  -> how many bits of T this thread cleared, and in n_claims and n_standing the number of claims and of the standing peers
// among them (uniform).
template <bool COVER>
__device__ __forceinline__ int far_claim_scan(const FarArgs& a, const FarTeam& m, int i, int t, unsigned long long* s_t, unsigned long long* s_c,
                                              int& n_claims, int& n_standing) {
#pragma clang fp contract(off)
  __shared__ double s_pts[3 * FAR_CHUNK];
  __shared__ int s_cnt[8];  // [2][4]: the claims of a chunk per wavefront (the standing ones among them << 16), by the chunk's parity
  __shared__ unsigned short s_cb[COVER ? 3 * FAR_CHUNK : 1];  // (without COVER nothing refers to it, and it takes no LDS)
  const ReachArgs& r = a.r;
  const int lane = t & 63, w = t >> 6, n = a.n;
  int cleared = 0, total = 0, standing = 0, parity = 0;
  for (int base = 0; base < n; base += FAR_CHUNK, parity ^= 1) {
    const int k = base + t;
    const bool in = k < n && k != i;
    const int ck = in ? (int)m.cls[k] : FAR_CLASS_NONE;
    const bool low = ck == FAR_CLASS_SEARCHER && k < i;
    bool has = (low || ck == FAR_CLASS_STANDING) && m.grp[k] == m.group;
    if (has && low) has = r.mask[k] == 1;  // (a lower peer of this chain: a launch before this one wrote its mask and goal)
    const unsigned long long bh = __ballot(has);
    const unsigned long long bs = __ballot(has && !low);
    if (lane == 0) s_cnt[4 * parity + w] = __popcll(bh) | (__popcll(bs) << 16);  // (each <= 64)
    __syncthreads();
    const int c0 = s_cnt[4 * parity], c1 = s_cnt[4 * parity + 1], c2 = s_cnt[4 * parity + 2], c3 = s_cnt[4 * parity + 3];
    const int both = c0 + c1 + c2 + c3, cm = both & 0xffff;  // (<= 256 each: no carry between the halves)
    if (cm == 0) continue;  // (uniform over the workgroup; the next chunk writes the other half of s_cnt)
    if (has) {
      const double* c = low ? r.goals + 3 * (size_t)k : r.vehicles[k].g_term;
      const int j = (((w > 0 ? c0 : 0) + (w > 1 ? c1 : 0) + (w > 2 ? c2 : 0)) & 0xffff) + fhw::rank_in(bh);  // (< 256)
      const double c_x = c[0], c_y = c[1], c_z = c[2];
      s_pts[3 * j] = c_x; s_pts[3 * j + 1] = c_y; s_pts[3 * j + 2] = c_z;
      if constexpr (COVER) {
        // the voxel of the claim, tested as a double before it is an index (the expression of the start cell)
        const double vfx = floor((c_x - r.ox) / r.res), vfy = floor((c_y - r.oy) / r.res), vfz = floor((c_z - r.oz) / r.res);
        const bool inside = vfx >= 0.0 && vfx < (double)r.nx && vfy >= 0.0 && vfy < (double)r.ny && vfz >= 0.0 && vfz < (double)r.nz;
        s_cb[3 * j] = inside ? (unsigned short)((int)vfx / a.B) : (unsigned short)0xffffu;  // (a block per axis: < 64 * 512)
        s_cb[3 * j + 1] = inside ? (unsigned short)((int)vfy / a.B) : (unsigned short)0xffffu;
        s_cb[3 * j + 2] = inside ? (unsigned short)((int)vfz / a.B) : (unsigned short)0xffffu;
      }
    }
    __syncthreads();
    total += cm;
    standing += both >> 16;
    for (int u = t; u < a.W; u += 256) {
      const int kx = u % a.wx, row = u / a.wx, by = row % a.cy, bz = row / a.cy;
      if constexpr (COVER) {
        if (m.k > 0) {  // the covered blocks of this word
          const int first = 64 * kx, last = min(first + 63, a.cx - 1);
          unsigned long long cw = 0ull;
          for (int j = 0; j < cm; j++) {
            const int cbx = (int)s_cb[3 * j], cby = (int)s_cb[3 * j + 1], cbz = (int)s_cb[3 * j + 2];
            if (cbx == 0xffff) continue;
            if (abs(by - cby) >= m.k || abs(bz - cbz) >= m.k) continue;
            const int lo = max(cbx - m.k + 1, first), hi = min(cbx + m.k - 1, last);
            if (lo <= hi) cw |= ((1ull << (hi - lo + 1)) - 1ull) << (lo - first);  // (hi - lo <= 8, lo - first <= 63 - (hi - lo))
          }
          if (cw) s_c[u] |= cw;
        }
      }
      unsigned long long tw = s_t[u];
      if (tw == 0ull) continue;
      const unsigned long long before = tw;
      const int y0 = by * a.B, y1 = min(y0 + a.B, r.ny) - 1, z0 = bz * a.B, z1 = min(z0 + a.B, r.nz) - 1;
      for (int j = 0; j < cm && tw != 0ull; j++) {
        const double cx = s_pts[3 * j], cy = s_pts[3 * j + 1], cz = s_pts[3 * j + 2];
        const double gy2 = far_gap2(cy, y0, y1, r.res, r.oy), gz2 = far_gap2(cz, z0, z1, r.res, r.oz);
        if (!(gy2 + gz2 < m.s2)) continue;  // (x2 + y2) + z2 >= y2 + z2 in rounded sums of non-negative terms: no block of this word
        unsigned long long h = tw;
        while (h) {
          const int bit = (int)__builtin_ctzll(h);
          h &= h - 1ull;
          const int x0 = (64 * kx + bit) * a.B;
          const double gx2 = far_gap2(cx, x0, min(x0 + a.B, r.nx) - 1, r.res, r.ox);
          if ((gx2 + gy2) + gz2 < m.s2) tw &= ~(1ull << bit);
        }
      }
      if (tw != before) {
        s_t[u] = tw;
        cleared += __popcll(before ^ tw);
      }
    }
    // (the next chunk's first barrier stands between these reads of s_pts / s_cb and the next writes)
  }
  n_claims = total;
  n_standing = standing;
  return cleared;
}

struct FarNoClaims {};

// The body of far_goals_kernel, and with CLAIMS that of far_spread_goals_kernel (fh_apart.hpp): far_claim_scan takes the blocks that
// the claims of x.team cover out of T in LDS before the flood, x.store() writes the longer record.  With CLAIMS false every
// `if constexpr` below is gone.
template <bool CLAIMS, class X>
__device__ __forceinline__ void far_body(const FarArgs& a, const X& x) {
#pragma clang fp contract(off)
  __shared__ unsigned long long s_t[FAR_WORDS], s_lx[FAR_WORDS], s_ly[FAR_WORDS], s_lz[FAR_WORDS], s_a[FAR_WORDS], s_b[FAR_WORDS];
  __shared__ double s_bd2[4];
  __shared__ int s_bc[4], s_n[4], s_m[4], s_k[4];
  __shared__ unsigned s_or[2][4];
  const ReachArgs& r = a.r;
  const int i = (int)blockIdx.x, t = (int)threadIdx.x, lane = t & 63, w = t >> 6;
  const FarStart st = far_start(a, i);
  const int view = st.view;
  int flags = st.who.flags;
  const FarCounts none = {-1, -1, 0, 0, 0, 0, 0};
  if (!st.who.searched) {  // (uniform over the workgroup)
    if constexpr (!CLAIMS) {  // (with CLAIMS the count kernel has written the outputs of a vehicle that is not searched)
      if (t == 0) far_store(a, i, flags, view, -1, INFINITY, INFINITY, none);
    }
    return;
  }
  const int wx = a.wx, slab = a.wx * a.cy, sw = st.sw;
  const unsigned long long sbit = st.sbit;
  const double px = st.px, py = st.py, pz = st.pz;
  const unsigned char* F = r.flags + (size_t)view * r.view_stride;
  const FarMaps maps = {s_t, s_lx, s_ly, s_lz, s_a, s_b};

  // ---- the view's summary into LDS, T without the blocks within r_avoid of g_term ----
  unsigned long long own_seen[FAR_OWN];
  unsigned own_nb[FAR_OWN];
  const int n_targets = far_summary<false>(a, st, t, maps, nullptr, own_seen, own_nb);
  int n_claims = 0, n_standing = 0;  // (uniform)
  if constexpr (CLAIMS) {
    const int n_claimed = far_claim_scan<false>(a, x.team, i, t, s_t, nullptr, n_claims, n_standing);
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
  int level = 0, hops = -1, best_block = -1;
  double best_bd2 = INFINITY;
  FarVoxel voxel = {INFINITY, -1, 0};
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
      voxel = far_scan_block(a, F, best_block, px, py, pz, t);
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
      const unsigned long long v = far_expand(maps, cur, nxt, u, own_nb[j], wx, slab, own_seen[j]);
      const unsigned long long h = v & s_t[u];
      n_reached += __popcll(v);
      n_reachable += __popcll(h);
      any |= (v ? 1u : 0u) | (h ? 2u : 0u);
    }
    const unsigned all = far_level_any(any, s_or, level, lane, w);
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
    n.members = hops >= 0 ? voxel.members : 0;
    if (cut) flags |= FH_REACH_CUT;
    if constexpr (CLAIMS)
      x.store(i, flags, view, hops >= 0 ? voxel.cell : -1, hops >= 0 ? voxel.d2 : INFINITY, hops >= 0 ? best_bd2 : INFINITY, n, n_claims, n_standing,
              x.sum[0] + x.sum[1] + x.sum[2] + x.sum[3]);
    else
      far_store(a, i, flags, view, hops >= 0 ? voxel.cell : -1, hops >= 0 ? voxel.d2 : INFINITY, hops >= 0 ? best_bd2 : INFINITY, n);
  }
}

__global__ void __launch_bounds__(256) far_goals_kernel(FarArgs a) { far_body<false>(a, FarNoClaims()); }

}  // namespace fhp

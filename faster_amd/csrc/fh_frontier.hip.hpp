// fh_frontier.hip.hpp — the kernels of include/fasterhip_frontier.h (which is the specification): the nearest frontier voxel of its
// view for every vehicle that wants a goal, and what every view knows.  Included in fh_map.hip after fh_view_subset.hip.hpp, so that
// these kernels come last in the code object and the ones before them keep their bytes.
//   frontier_goals_kernel : ONE workgroup of 256 per vehicle.  Status, stage, view and the six coordinates are read as uniform values; a
//                           vehicle that is not searched has its three outputs written by thread 0 and the workgroup returns.  A searched
//                           one scans the bounding box of its sphere — floor((p -+ r_max - origin) / res) and one voxel more on every
//                           side, clipped to the lattice; the distance test decides — a wavefront per row of x, lanes along x, so the
//                           flag bytes of a row are loaded coalesced.  What depends on (iy, iz) alone — the z test, dy dy, dz dz, the
//                           map's row — is computed once per row.  A lane whose own flag is 0 and whose voxel passes the two distance
//                           tests loads its six neighbour bytes, then the map bit.  Every lane keeps the smallest (d2, c) it has seen
//                           and a count; after the scan wave_min of d2 (identity +inf; no NaN: a d2 that is kept has passed d2 < r2),
//                           wave_min_i32 of c among the lanes that hold that minimum, an integer sum of the counts, and the four
//                           wavefronts combined through LDS with the same two-key rule.  Thread 0 recomputes q from c.
//   view_coverage_kernel  : blockIdx.y = view, a thread takes every (gridDim.x 256)-th chunk of 16 flag bytes, aligned in memory: one
//                           16-byte load, and only a chunk with a zero byte is looked at byte by byte — known voxels and, for those, the
//                           six neighbour bytes.  The chunks over the ends of a row are loaded byte by byte, the row's bytes only.
//                           Integer sums per wavefront, LDS, one integer atomic add per counter and workgroup.
// Every address comes from a checked number: view in [0, n_views), box indices clipped to the lattice, neighbours tested against the
// dims before they are loaded, the map cell tested against the map's dims before its word is loaded.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fasterhip_frontier.h"
#include "fh_wave.hip.hpp"

namespace fhp {

struct FrontierArgs {
  double r_max, r2, a2, z_lo, z_hi;  // r2 = r_max * r_max, a2 = r_avoid * r_avoid: rounded once on the host, as the model rounds them
  int want;
  int nx, ny, nz;  // the lattice of the views
  double res, ox, oy, oz;
  const unsigned char* flags;
  size_t view_stride;
  const int32_t* view_of;
  int n_views;
  const fh_vehicle* vehicles;
  int mx, my, mz;  // the map
  double mres, mox, moy, moz;
  const unsigned* bits;
  double* goals;
  int32_t* mask;
  fh_frontier_record* records;
};

__device__ __forceinline__ bool frontier_finite(double x) { return fabs(x) < INFINITY; }  // (a NaN fails the comparison)

// the first and the last index of the box along one axis, inside [0, n - 1] or empty (lo > hi); whatever f is, NaN included
__device__ __forceinline__ int frontier_box_lo(double f, int n) { return f > 0.0 ? (f < (double)n ? (int)f : n) : 0; }
__device__ __forceinline__ int frontier_box_hi(double f, int n) { return f < (double)(n - 1) ? (f >= 0.0 ? (int)f : -1) : n - 1; }

// (d2, c) < (e2, k), lexicographic
__device__ __forceinline__ bool frontier_before(double d2, int c, double e2, int k) { return d2 < e2 || (d2 == e2 && c < k); }

// the three outputs of vehicle i, by one thread
__device__ __forceinline__ void frontier_store(const FrontierArgs& a, int i, int flags, int view, int cell, int candidates, double d2) {
#pragma clang fp contract(off)
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
  }
  a.mask[i] = cell >= 0 ? 1 : 0;
  fh_frontier_record r;
  r.flags = flags; r.view = view; r.cell = cell; r.candidates = candidates;
  r.d2 = d2; r.reserved = 0.0;
  a.records[i] = r;
}

__global__ void __launch_bounds__(256) frontier_goals_kernel(FrontierArgs a) {
#pragma clang fp contract(off)
  __shared__ double s_d2[4];
  __shared__ int s_c[4], s_n[4];
  const int i = (int)blockIdx.x, t = (int)threadIdx.x, lane = t & 63, w = t >> 6;
  const fh_vehicle& V = a.vehicles[i];
  const int view = fhw::uniform_i32(a.view_of ? a.view_of[i] : i);
  const int status = fhw::uniform_i32(V.status), stage = fhw::uniform_i32(V.stage);
  const double px = fhw::uniform_f64(V.state.pos[0]), py = fhw::uniform_f64(V.state.pos[1]), pz = fhw::uniform_f64(V.state.pos[2]);
  const double gx = fhw::uniform_f64(V.g_term[0]), gy = fhw::uniform_f64(V.g_term[1]), gz = fhw::uniform_f64(V.g_term[2]);
  const bool wanted = ((a.want & FH_FRONTIER_WANT_REACHED) && status == FH_VEHICLE_GOAL_REACHED) ||
                      ((a.want & FH_FRONTIER_WANT_NO_PATH) && stage == FH_FLEET_STAGE_NO_PATH) || (a.want & FH_FRONTIER_WANT_ALL);
  const bool finite = frontier_finite(px) && frontier_finite(py) && frontier_finite(pz) && frontier_finite(gx) && frontier_finite(gy) &&
                      frontier_finite(gz);
  const int flags = (wanted ? FH_FRONTIER_WANTED : 0) | (view >= 0 && view < a.n_views ? 0 : FH_FRONTIER_NO_VIEW) | (finite ? 0 : FH_FRONTIER_BAD_POS);
  if (flags != FH_FRONTIER_WANTED) {  // not searched (uniform over the workgroup)
    if (t == 0) frontier_store(a, i, flags, view, -1, 0, INFINITY);
    return;
  }
  const unsigned char* F = a.flags + (size_t)view * a.view_stride;
  const int lo0 = frontier_box_lo(floor((px - a.r_max - a.ox) / a.res) - 1.0, a.nx), hi0 = frontier_box_hi(floor((px + a.r_max - a.ox) / a.res) + 1.0, a.nx);
  const int lo1 = frontier_box_lo(floor((py - a.r_max - a.oy) / a.res) - 1.0, a.ny), hi1 = frontier_box_hi(floor((py + a.r_max - a.oy) / a.res) + 1.0, a.ny);
  const int lo2 = frontier_box_lo(floor((pz - a.r_max - a.oz) / a.res) - 1.0, a.nz), hi2 = frontier_box_hi(floor((pz + a.r_max - a.oz) / a.res) + 1.0, a.nz);
  const int rows_y = hi1 - lo1 + 1, rows_z = hi2 - lo2 + 1;
  const int rows = (hi0 < lo0 || rows_y <= 0 || rows_z <= 0) ? 0 : rows_y * rows_z;  // (<= ny nz: the cells fit an int)
  const int slice = a.nx * a.ny;
  double best_d2 = INFINITY;
  int best_c = 0x7fffffff, count = 0;
  for (int r = w; r < rows; r += 4) {  // (r, and all that follows from it alone, is uniform over the wavefront)
    const int iz = lo2 + r / rows_y, iy = lo1 + r % rows_y;
    const double qz = (iz + 0.5) * a.res + a.oz, qy = (iy + 0.5) * a.res + a.oy;
    if (!(a.z_lo <= qz && qz <= a.z_hi)) continue;
    const double fy = floor((qy - a.moy) / a.mres), fz = floor((qz - a.moz) / a.mres);
    if (!(fy >= 0.0 && fy < (double)a.my && fz >= 0.0 && fz < (double)a.mz)) continue;  // (outside the map: no candidate in this row)
    const int map_row = a.mx * ((int)fy + a.my * (int)fz);
    const double dy = qy - py, dz = qz - pz, ey = qy - gy, ez = qz - gz;
    const double dy2 = dy * dy, dz2 = dz * dz, ey2 = ey * ey, ez2 = ez * ez;
    const int c0 = (iz * a.ny + iy) * a.nx;
    for (int x0 = lo0; x0 <= hi0; x0 += 64) {
      const int ix = x0 + lane;
      if (ix > hi0) continue;
      const int c = c0 + ix;
      if (F[c] != 0) continue;
      const double qx = (ix + 0.5) * a.res + a.ox;
      const double dx = qx - px;
      const double d2 = dx * dx + dy2 + dz2;
      if (!(d2 < a.r2)) continue;
      const double ex = qx - gx;
      const double e2 = ex * ex + ey2 + ez2;
      if (e2 < a.a2) continue;
      const bool unknown_next = (ix > 0 && F[c - 1] != 0) || (ix < a.nx - 1 && F[c + 1] != 0) || (iy > 0 && F[c - a.nx] != 0) ||
                                (iy < a.ny - 1 && F[c + a.nx] != 0) || (iz > 0 && F[c - slice] != 0) || (iz < a.nz - 1 && F[c + slice] != 0);
      if (!unknown_next) continue;
      const double fx = floor((qx - a.mox) / a.mres);
      if (!(fx >= 0.0 && fx < (double)a.mx)) continue;
      const int id = map_row + (int)fx;
      if ((a.bits[id >> 5] >> (id & 31)) & 1u) continue;
      count++;
      if (frontier_before(d2, c, best_d2, best_c)) { best_d2 = d2; best_c = c; }
    }
  }
  // all 64 lanes are here again: the trip counts above are uniform over the wavefront
  const double wave_d2 = fhw::wave_min(best_d2);
  const int wave_c = fhw::wave_min_i32(best_d2 == wave_d2 ? best_c : 0x7fffffff);
  const int wave_n = fhw::wave_sum_i32(count);
  if (lane == 0) { s_d2[w] = wave_d2; s_c[w] = wave_c; s_n[w] = wave_n; }
  __syncthreads();
  if (t == 0) {
    double d2 = s_d2[0];
    int c = s_c[0], n = s_n[0];
    for (int k = 1; k < 4; k++) {
      if (frontier_before(s_d2[k], s_c[k], d2, c)) { d2 = s_d2[k]; c = s_c[k]; }
      n += s_n[k];
    }
    const bool found = d2 < INFINITY;
    frontier_store(a, i, flags, view, found ? c : -1, n, found ? d2 : INFINITY);
  }
}

constexpr int VIEW_COVERAGE_BLOCKS = 256;  // gridDim.x of view_coverage_kernel (at most; fewer with fewer cells)

__device__ __forceinline__ bool frontier_no_zero_byte(unsigned v) { return ((v - 0x01010101u) & ~v & 0x80808080u) == 0u; }

// out: [n_views][2] counters (known, frontier), zero before the launch.  A thread takes chunks of 16 bytes that are aligned in MEMORY
// (the rows of the views begin anywhere): a chunk that lies wholly inside the row is one 16-byte load, and most chunks of a view that
// is largely unknown end there, with no zero byte; the at most two chunks that reach over an end of the row are loaded byte by byte,
// the bytes of the row only.
__global__ void __launch_bounds__(256) view_coverage_kernel(const unsigned char* __restrict__ flags, size_t view_stride, int nx, int ny, int nz,
                                                            int v0, unsigned long long* out) {
  __shared__ int s_known[4], s_front[4];
  const int t = (int)threadIdx.x, lane = t & 63, w = t >> 6;
  const size_t v = (size_t)v0 + blockIdx.y;
  const unsigned char* F = flags + v * view_stride;
  const long long cells = (long long)nx * ny * nz, step = (long long)gridDim.x * 256;
  const int slice = nx * ny;
  const long long skew = (long long)((size_t)F & 15u);  // F - skew is aligned; chunk k holds the cells 16 k - skew .. + 15
  const long long chunks = (skew + cells + 15) >> 4;
  int known = 0, front = 0;  // (a thread sees at most 16 (chunks / 256 + 1) voxels)
  for (long long k = (long long)blockIdx.x * 256 + t; k < chunks; k += step) {
    const long long first = k * 16 - skew;
    const long long lo = first < 0 ? 0 : first, hi = first + 16 < cells ? first + 16 : cells;  // the cells of the chunk: [lo, hi)
    unsigned word[4] = {0x01010101u, 0x01010101u, 0x01010101u, 0x01010101u};
    if (first >= 0 && first + 16 <= cells) {
      const uint4 q = *reinterpret_cast<const uint4*>(F + first);
      word[0] = q.x; word[1] = q.y; word[2] = q.z; word[3] = q.w;
    } else {
#pragma unroll
      for (int j = 0; j < 16; j++) {  // (what lies outside the row stays 1: not known, and not counted below either)
        const long long cc = first + j;
        if (cc >= lo && cc < hi) word[j >> 2] = (word[j >> 2] & ~(0xffu << (8 * (j & 3)))) | ((unsigned)F[cc] << (8 * (j & 3)));
      }
    }
    if (frontier_no_zero_byte(word[0]) && frontier_no_zero_byte(word[1]) && frontier_no_zero_byte(word[2]) && frontier_no_zero_byte(word[3])) continue;
    const int c_lo = (int)lo;
    int ix = c_lo % nx, iy = (c_lo / nx) % ny, iz = c_lo / slice;
#pragma unroll
    for (int j = 0; j < 16; j++) {
      const long long cc = first + j;
      if (cc < lo || cc >= hi) continue;
      if (((word[j >> 2] >> (8 * (j & 3))) & 0xffu) == 0u) {
        const int c = (int)cc;
        known++;
        // six loads that do not wait for each other: a neighbour outside the lattice is replaced by the voxel itself, whose flag is 0
        const unsigned near = (unsigned)F[ix > 0 ? c - 1 : c] | F[ix < nx - 1 ? c + 1 : c] | F[iy > 0 ? c - nx : c] | F[iy < ny - 1 ? c + nx : c] |
                              F[iz > 0 ? c - slice : c] | F[iz < nz - 1 ? c + slice : c];
        front += near != 0u ? 1 : 0;
      }
      if (++ix == nx) {
        ix = 0;
        if (++iy == ny) { iy = 0; iz++; }
      }
    }
  }
  const int wave_known = fhw::wave_sum_i32(known), wave_front = fhw::wave_sum_i32(front);
  if (lane == 0) { s_known[w] = wave_known; s_front[w] = wave_front; }
  __syncthreads();
  if (t == 0) {
    const int k = s_known[0] + s_known[1] + s_known[2] + s_known[3], f = s_front[0] + s_front[1] + s_front[2] + s_front[3];
    if (k) atomicAdd(out + 2 * v, (unsigned long long)k);
    if (f) atomicAdd(out + 2 * v + 1, (unsigned long long)f);
  }
}

}  // namespace fhp

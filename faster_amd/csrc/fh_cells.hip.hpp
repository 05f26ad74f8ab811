// fh_cells.hip.hpp — the cell grid: the broad phase of the fleet stages that ask "which other vehicles can come near vehicle i"
// (fh_separation, fh_check).  A stage keeps one box record per vehicle that BEGINS with a CellBox, and a CellGrid in its kernel
// arguments.  Four launches, the first and the last of them the stage's own kernels:
//   the stage's boxes kernel : one wavefront per vehicle k.  Whatever positions k can show to anyone go, per lane, into a box
//                      (plan_box_take); cell_box_tail reduces it over the wavefront, raises the fleet-wide maximum half-extent H per
//                      axis (atomicMax on the bit pattern of a non-negative double) and counts k into the cell of its box centre.
//   cell_scan_kernel : one workgroup, the exclusive scan of the cell counts into starts[0 .. n_cells]; the counts are left zero.
//   cell_fill_kernel : lane = vehicle: items[starts[cell] + (the count of its cell, drawn again)] = k.  The order inside a cell is
//                      whatever the atomics give; the stages' tie rules make their output independent of it.
//   the stage's narrow kernel: one wavefront per vehicle i, one per workgroup.  cell_walk visits the cells whose clamped range covers
//                      box_i grown by reach + g + H: k sits in exactly one cell, that of its centre, and its centre is at most H from
//                      any point of its box.  Cells of one row along x are neighbours in `items`, so a row is one run of vehicles,
//                      read 64 at a time, lane = candidate.  Each turn hands the stage its lane's candidate, box_i grown by reach + g
//                      to test box_k against (cell_meets), and whether the cells end here; the stage keeps its own list of survivors.
// PREFILTERS ARE CONSERVATIVE.  A pair counts only by its d2, computed as the stage's model writes it; boxes and cells only decide
// what is looked at.  g = 1e-9 (reach + |lo| + |hi|) for the box test and 1e-9 (reach + |lo| + |hi| + H) for the cells: the roundings
// of lo - (reach + g), of the centre, of the half-extent and of d2 are relative 1e-16, seven orders below.  A position becomes a cell
// number by the same monotonic expression for centres and for ranges, after comparisons in double: no NaN, infinity or 1e300 is ever
// converted to int, and an infinite H (a box that overflowed) is every cell.  A box may hold more positions than the pairs read (the
// check's boxes do): a superset only adds candidates.
// Every index comes from a checked record: the stage's boxes kernel writes plan extents into boxes[k] after plan_bad_extent (0, 0
// otherwise), cell_box_tail clamps the cell into the grid, cell_fill_kernel writes vehicle numbers < n into items[], cell_walk hands
// out only 0 <= k < n, and the narrow phase reads plans through those only.
#pragma once
#include <hip/hip_runtime.h>

#include "fh_wave.hip.hpp"

namespace fh {

constexpr int CELL_SCAN_THREADS = 1024;
constexpr int CELL_BOXED = 1;  // CellBox.valid: at least one finite position: lo / hi / cell are set and the vehicle is counted into its cell

struct CellBox {  // 56 B: the head of a stage's box record (SepBox, ChkBox)
  double lo[3], hi[3];
  int valid, cell;  // valid: CELL_BOXED and the stage's own bits above it
};

struct CellGrid {  // the grid part of a stage's kernel arguments
  double ox, oy, oz, res;
  int nx, ny, nz;
  unsigned long long* extent;  // [3]: bit patterns of H per axis
  int* counts;                 // [n_cells]
  int* starts;                 // [n_cells + 1]
  int* items;                  // [n]
};

struct CellReach {  // box_i grown by reach + g
  double x0, x1, y0, y1, z0, z1;
};

// The cell of x along one axis (n cells of size res from o), clamped into [0, n - 1]; monotonic in x, and a NaN gives `nan_cell`.
__device__ __forceinline__ int cell_of(double x, double o, double res, int n, int nan_cell) {
#pragma clang fp contract(off)
  const double f = floor((x - o) / res), last = (double)(n - 1);
  if (f >= 0.0) return f <= last ? (int)f : n - 1;
  return f < 0.0 ? 0 : nan_cell;
}

// reach + g of the box test, and reach + g + H of the cells: where centres of boxes that pass the box test can lie
__device__ __forceinline__ double cell_box_margin(double reach, double lo, double hi) {
#pragma clang fp contract(off)
  return reach + 1e-9 * (reach + fabs(lo) + fabs(hi));
}
__device__ __forceinline__ double cell_range_margin(double reach, double lo, double hi, double H) {
#pragma clang fp contract(off)
  return (reach + 1e-9 * (reach + fabs(lo) + fabs(hi) + H)) + H;
}

// *word = max(*word, the bit pattern of h) for h >= +0.  The word only grows, so a vehicle that does not exceed what it reads has
// nothing to add: the whole fleet raises three words, and without the look all of its atomics queue up behind each other.
__device__ __forceinline__ void cell_raise(unsigned long long* word, double h) {
  const unsigned long long bits = (unsigned long long)__double_as_longlong(h);
  if (bits > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(word, bits);
}

// The end of a boxes kernel (whole wavefront): the lanes' boxes become the vehicle's; a box that is not empty gives the cell of its
// centre, and lane 0 raises H and counts the vehicle into that cell.  Returns CELL_BOXED or 0 (uniform).
__device__ __forceinline__ int cell_box_tail(const CellGrid& g, int lane, double& lx, double& ly, double& lz, double& hx, double& hy,
                                             double& hz, int& cell) {
#pragma clang fp contract(off)
  lx = fhw::wave_min(lx); ly = fhw::wave_min(ly); lz = fhw::wave_min(lz);
  hx = fhw::wave_max(hx); hy = fhw::wave_max(hy); hz = fhw::wave_max(hz);
  if (!(lx <= hx)) return 0;  // (uniform)
  // centre and half-extent: halves first, so that two coordinates near the largest double do not overflow in the sum
  const int cx = cell_of(lx * 0.5 + hx * 0.5, g.ox, g.res, g.nx, 0), cy = cell_of(ly * 0.5 + hy * 0.5, g.oy, g.res, g.ny, 0),
            cz = cell_of(lz * 0.5 + hz * 0.5, g.oz, g.res, g.nz, 0);
  cell = (cz * g.ny + cy) * g.nx + cx;
  if (lane == 0) {
    // (hi - lo is >= +0 or +INFINITY, never a NaN: the order of the bit patterns is the order of the values)
    cell_raise(g.extent + 0, (hx - lx) * 0.5);
    cell_raise(g.extent + 1, (hy - ly) * 0.5);
    cell_raise(g.extent + 2, (hz - lz) * 0.5);
    atomicAdd(g.counts + cell, 1);
  }
  return CELL_BOXED;
}

__device__ __forceinline__ void cell_box_store(CellBox& b, double lx, double ly, double lz, double hx, double hy, double hz, int valid,
                                               int cell) {
  b.lo[0] = lx; b.lo[1] = ly; b.lo[2] = lz;
  b.hi[0] = hx; b.hi[1] = hy; b.hi[2] = hz;
  b.valid = valid; b.cell = cell;
}

// starts[c] = the sum of counts[0 .. c), starts[n_cells] = the total; counts[] is left zero for cell_fill_kernel to draw from.  One
// workgroup: thread t owns the cells [t chunk, (t + 1) chunk).
__global__ void __launch_bounds__(CELL_SCAN_THREADS) cell_scan_kernel(int* __restrict__ counts, int* __restrict__ starts, int n_cells) {
  __shared__ int part[CELL_SCAN_THREADS];
  const int t = (int)threadIdx.x;
  const int chunk = (n_cells + CELL_SCAN_THREADS - 1) / CELL_SCAN_THREADS;
  const int c0 = min(t * chunk, n_cells), c1 = min(c0 + chunk, n_cells);
  int sum = 0;
  for (int c = c0; c < c1; c++) sum += counts[c];
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < CELL_SCAN_THREADS; d <<= 1) {  // inclusive scan of the partial sums
    const int v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int run = part[t] - sum;
  for (int c = c0; c < c1; c++) {
    const int v = counts[c];
    starts[c] = run;
    counts[c] = 0;
    run += v;
  }
  if (t == CELL_SCAN_THREADS - 1) starts[n_cells] = part[t];
}

// boxes: the stage's records, box_bytes apart, each beginning with a CellBox
__global__ void __launch_bounds__(256) cell_fill_kernel(CellGrid g, const unsigned char* __restrict__ boxes, int box_bytes, int n) {
  const int k = (int)(blockIdx.x * 256 + threadIdx.x);
  if (k >= n) return;
  const CellBox& b = *reinterpret_cast<const CellBox*>(boxes + (size_t)k * (size_t)box_bytes);
  if (!(b.valid & CELL_BOXED)) return;
  const int slot = g.starts[b.cell] + atomicAdd(g.counts + b.cell, 1);
  if (slot >= 0 && slot < n) g.items[slot] = k;  // (always: the boxed vehicles are the ones that were counted)
}

__device__ __forceinline__ bool cell_meets(const CellBox& K, const CellReach& w) {
  return K.hi[0] >= w.x0 && K.lo[0] <= w.x1 && K.hi[1] >= w.y0 && K.lo[1] <= w.y1 && K.hi[2] >= w.z0 && K.lo[2] <= w.z1;
}

// The walk of a narrow kernel (whole wavefront, B = the box of vehicle i, which is boxed): turn(k, w, end) once per run of 64 items,
// with k = this lane's candidate (0 <= k < n, k != i) or -1, w = box_i grown by reach + g, end = no turn follows.  There is always a
// last turn, so that a stage's list is flushed: an empty last row has one with no candidate.  `turn` is inlined: no call, no scratch.
template <class Turn>
__device__ __forceinline__ void cell_walk(const CellGrid& g, const CellBox& B, double reach, int i, int n, int lane, Turn&& turn) {
#pragma clang fp contract(off)
  const double lx = fhw::uniform_f64(B.lo[0]), ly = fhw::uniform_f64(B.lo[1]), lz = fhw::uniform_f64(B.lo[2]);
  const double hx = fhw::uniform_f64(B.hi[0]), hy = fhw::uniform_f64(B.hi[1]), hz = fhw::uniform_f64(B.hi[2]);
  const double Hx = __longlong_as_double((long long)g.extent[0]), Hy = __longlong_as_double((long long)g.extent[1]),
               Hz = __longlong_as_double((long long)g.extent[2]);
  const double gx = cell_box_margin(reach, lx, hx), gy = cell_box_margin(reach, ly, hy), gz = cell_box_margin(reach, lz, hz);
  const CellReach w = {lx - gx, hx + gx, ly - gy, hy + gy, lz - gz, hz + gz};
  const double wx = cell_range_margin(reach, lx, hx, Hx), wy = cell_range_margin(reach, ly, hy, Hy), wz = cell_range_margin(reach, lz, hz, Hz);
  const int cxa = cell_of(lx - wx, g.ox, g.res, g.nx, 0), cxb = cell_of(hx + wx, g.ox, g.res, g.nx, g.nx - 1);
  const int cya = cell_of(ly - wy, g.oy, g.res, g.ny, 0), cyb = cell_of(hy + wy, g.oy, g.res, g.ny, g.ny - 1);
  const int cza = cell_of(lz - wz, g.oz, g.res, g.nz, 0), czb = cell_of(hz + wz, g.oz, g.res, g.nz, g.nz - 1);
  for (int cz = cza; cz <= czb; cz++) {
    for (int cy = cya; cy <= cyb; cy++) {
      const bool last_row = cz == czb && cy == cyb;
      const int row = (cz * g.ny + cy) * g.nx;
      const int s0 = fhw::uniform_i32(g.starts[row + cxa]), s1 = fhw::uniform_i32(g.starts[row + cxb + 1]);
      for (int q0 = s0; q0 < s1 || (last_row && q0 == s0); q0 += 64) {
        const int q = q0 + lane;
        int k = -1;
        if (q < s1) {
          k = g.items[q];
          if (!(k >= 0 && k < n && k != i)) k = -1;
        }
        turn(k, w, last_row && q0 + 64 >= s1);
      }
    }
  }
}

}  // namespace fh

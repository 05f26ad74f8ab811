// fh_view_subset.hip.hpp — the kernels of include/fasterhip_view_subset.h: the list of the views that the active queries of a search
// need, and clear / mark / jump tables for the listed views only.  Included in fh_map.hip after fh_path.hip.hpp, so that these kernels
// come last in the code object and the ones before them keep their bytes; jps_table_lines and the arithmetic of mark_views_kernel are
// used as they are.
//   view_flag_kernel    : lane = query.  flags[view(q)] = 1 for an active query with a view in range.  Queries of one view store the
//                         same value with plain stores.
//   view_compact_kernel : ONE workgroup of 1024 threads walks the flags 1024 views at a time, thread = view: a ballot per wavefront,
//                         the 16 counts through LDS, and list[listed so far + wavefronts below + rank in the ballot] = view.  Ascending
//                         and deterministic: the position of a view depends on the flags below it and on nothing else.  Then the tail
//                         (-1) and the count.
//   the listed kernels  : grid (x as the kernel for all views, y = a bounded number of rows).  Row blockIdx.y takes the list entries
//                         e = blockIdx.y, blockIdx.y + gridDim.y, ... < count ("a wavefront takes every 1024th row" of the traffic
//                         kernels), so work is proportional to the count and a block with nothing to do returns after one uniform
//                         load of *count.  count is clamped to n_views and an entry outside [0, n_views) is skipped: every address
//                         comes from a checked number.
#pragma once
#include <hip/hip_runtime.h>

#include "fh_path.hip.hpp"

namespace fhp {

constexpr int VIEW_COMPACT_THREADS = 1024;
constexpr int VIEW_LIST_ROWS = 128;  // gridDim.y of the listed kernels (at most; fewer with fewer views)

__global__ void __launch_bounds__(256) view_flag_kernel(const int* __restrict__ active, const int* __restrict__ view_of, int n, int n_views,
                                                        int* __restrict__ flags) {
  const int q = (int)(blockIdx.x * 256 + threadIdx.x);
  if (q >= n) return;
  if (active && active[q] == 0) return;
  const int v = view_of ? view_of[q] : q;
  if (v >= 0 && v < n_views) flags[v] = 1;
}

__global__ void __launch_bounds__(VIEW_COMPACT_THREADS) view_compact_kernel(const int* __restrict__ flags, int n_views, int* __restrict__ list,
                                                                            int* __restrict__ count) {
  __shared__ int wave_count[VIEW_COMPACT_THREADS / 64];
  const int t = (int)threadIdx.x, lane = t & 63, w = t >> 6;
  int listed = 0;  // views listed by the chunks before this one (uniform over the workgroup)
  for (int v0 = 0; v0 < n_views; v0 += VIEW_COMPACT_THREADS) {
    const int v = v0 + t;
    const bool need = v < n_views && flags[v] != 0;
    const unsigned long long m = __ballot(need);
    if (lane == 0) wave_count[w] = __popcll(m);
    __syncthreads();
    int below = 0, all = 0;
    for (int k = 0; k < VIEW_COMPACT_THREADS / 64; k++) {
      const int c = wave_count[k];
      all += c;
      below += k < w ? c : 0;
    }
    if (need) list[listed + below + rank_in(m)] = v;  // (< n_views: as many slots as flags seen so far)
    listed += all;
    __syncthreads();
  }
  for (int i = listed + t; i < n_views; i += VIEW_COMPACT_THREADS) list[i] = -1;
  if (t == 0) *count = listed;
}

// how many entries of the list a listed kernel reads (uniform: one scalar load)
__device__ __forceinline__ int view_list_count(const int* count, int n_views) {
  const int c = uniform_i32(*count);
  return c < n_views ? c : n_views;
}

// the words of the grids of the listed views become zero
__global__ void __launch_bounds__(256) clear_views_listed_kernel(unsigned* bits, long long words_per_view, int n_views, const int* __restrict__ list,
                                                                 const int* __restrict__ count) {
  const int cnt = view_list_count(count, n_views);
  const long long w = (long long)blockIdx.x * 256 + threadIdx.x;
  for (int e = (int)blockIdx.y; e < cnt; e += (int)gridDim.y) {
    const long long v = uniform_i32(list[e]);
    if (v < 0 || v >= n_views) continue;
    if (w < words_per_view) bits[v * words_per_view + w] = 0u;
  }
}

// mark_views_kernel for the listed views: the same arithmetic (mark_cell, mark_cube), the view from the list instead of from blockIdx.y
__global__ void __launch_bounds__(256) mark_views_listed_kernel(const double* cloud, int n, int nx, int ny, int nz, double res, double ox, double oy,
                                                                double oz, int m, MarkLimits lim, unsigned* bits, long long words_per_view,
                                                                const unsigned* mask, int mask_words, int n_views, const int* __restrict__ list,
                                                                const int* __restrict__ count) {
  const int cnt = view_list_count(count, n_views);
  if ((int)blockIdx.y >= cnt) return;
  const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
  if (i >= n) return;
  long long c[3];
  if (!mark_cell(cloud, i, res, ox, oy, oz, lim, c)) return;
  for (int e = (int)blockIdx.y; e < cnt; e += (int)gridDim.y) {
    const long long v = uniform_i32(list[e]);
    if (v < 0 || v >= n_views) continue;
    if (!((mask[v * mask_words + (i >> 5)] >> (i & 31)) & 1u)) continue;
    mark_cube(c, nx, ny, nz, m, bits + v * words_per_view);
  }
}

// jps_table_views_kernel for the listed views (mv.bits: view 0, words_per_view words apart; jt alike); one launch per level
__global__ void __launch_bounds__(256) jps_table_views_listed_kernel(MapView mv, const unsigned char* tb, short* jt, int level,
                                                                     long long words_per_view, int n_views, const int* __restrict__ list,
                                                                     const int* __restrict__ count) {
  const int cnt = view_list_count(count, n_views);
  const unsigned* bits0 = mv.bits;
  for (int e = (int)blockIdx.y; e < cnt; e += (int)gridDim.y) {
    const long long v = uniform_i32(list[e]);
    if (v < 0 || v >= n_views) continue;
    mv.bits = bits0 + v * words_per_view;
    jps_table_lines(mv, tb, jt + v * (long long)mv.total * 32, level);
  }
}

}  // namespace fhp

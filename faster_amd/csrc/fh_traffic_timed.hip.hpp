// fh_traffic_timed.hip.hpp — time-aware traffic (include/fasterhip_traffic_timed.h, which is the specification): the slots, points,
// words and working buffers of fh_traffic.hip.hpp, and other bits.  Sample (k, s) is shown to vehicle i when vehicle i's OWN committed
// plan has a shown sample s' with |s - s'| <= window within `range` of it; state_i.pos is not read.  Chunks, words per chunk and
// traffic_word<PPS> are those of fh_traffic.hip.hpp.  Two launches:
//   traffic_timed_points{1,7}_kernel: traffic_points<PPS> with the instant j = first_instant + s stride (64 bits).  A second pair and
//                      not a parameter of the first: TrafficArgs with one more member moves the kernel arguments of
//                      traffic_points{1,7}_kernel, which were to keep their instruction bytes.  Writes the PPS points of every slot, the
//                      32-byte record per sample and the grown box per chunk.
//   traffic_timed_mask{1,7}_kernel: one wavefront per (group of 64 chunks, row i), rows strided over a grid at most TRAFFIC_GRID_ROWS
//                      high.  Per row: the S records of vehicle i are staged once into LDS as three arrays of doubles (24 bytes per
//                      sample, 12 KB at the cap), a sample that does not show as NaN: every comparison with it fails without a branch.
//                      The box of i's shown samples is reduced on the way (wave_min / wave_max).  Lane = chunk: does the chunk's grown
//                      box overlap the row box?  One ballot names the chunks that are looked at; the words of the others are stored as
//                      zeros.  For a chunk that is looked at: lane = sample t, s = t - k S; the loop over the window reads LDS at
//                      lo + q, lo = max(0, s - window): neighbouring lanes read neighbouring doubles (or, where the window is clipped
//                      at 0, the same one), which is free of bank conflicts.  The d2 decisions are ORed, then one ballot, and the words
//                      are assembled by traffic_word<PPS>.  No atomics, every word of a row stored exactly once.
// THE PREFILTER IS CONSERVATIVE.  A bit needs a shown c' = c[i][s'] and a shown c = c[k][s] with d2 < range range, so
// |c - c'| < range (1 + 4e-16) per axis.  c lies in its chunk's box [lo, hi] exactly and c' in the row box [rlo, rhi] exactly, hence
// rhi >= c' > lo - range (1 + 4e-16) and rlo <= c' < hi + range (1 + 4e-16): the chunk box grown by cell_box_margin(range, lo, hi)
// (fh_traffic.hip.hpp argues the margin) overlaps the row box.  The row box is grown by cell_box_margin(0, rlo, rhi) besides, the
// relative part alone: it costs nothing and the argument does not need it.  An empty box is (+inf, -inf): its grown bounds are NaN and
// no comparison holds, so an observer none of whose samples show has every word stored as zero.
// Every index comes from a checked record: head and size are tested against max_states before the plan is read, the records carry
// vehicle numbers < n, both buffers are sized in whole chunks, and an LDS index is clamped to [0, S - 1] before it is used.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fasterhip_traffic_timed.h"
#include "fh_traffic.hip.hpp"

namespace fh {

struct TrafficTimedArgs {
  TrafficArgs t;  // (stride, range2, the buffers: as fh_fleet_traffic_device fills them)
  int first_instant;
  int window;  // min(window, S - 1)
  int span;    // min(2 window + 1, S): the most samples a window holds
};

template <int PPS>
__device__ __forceinline__ void traffic_timed_points(const TrafficTimedArgs& b) {
#pragma clang fp contract(off)
  using fhw::lane_id;
  using fhw::wave_max;
  using fhw::wave_min;
  const TrafficArgs& a = b.t;
  const int lane = lane_id();
  const int chunk = (int)blockIdx.x;
  if (chunk >= a.n_chunks) return;
  const int t = chunk * 64 + lane;
  bool show = false;
  double cx = 0.0, cy = 0.0, cz = 0.0;
  int k = 0;
  if (t < a.n_samples) {
    k = t / a.samples;
    const int s = t - k * a.samples;
    const fh_vehicle& V = a.vehicles[k];
    const int head = V.plan_head, size = V.plan_size;
    if (!plan_bad_extent(head, size, a.max_states) && size >= 1) {
      const long long j = (long long)b.first_instant + (long long)s * (long long)a.stride, last = (long long)size - 1;
      const double* p = a.plans[(size_t)k * (size_t)a.max_states + (size_t)head + (size_t)(j < last ? j : last)].pos;
      const double x = p[0], y = p[1], z = p[2];
      if (plan_finite(x) && plan_finite(y) && plan_finite(z)) {
        show = true;
        cx = x; cy = y; cz = z;
      }
    }
    double* out = a.cloud + 3 * ((size_t)a.first_point + (size_t)t * (size_t)PPS);
    out[0] = cx; out[1] = cy; out[2] = cz;
    if (PPS == 7) {
      const double h = a.hull;
      const double xp = show ? cx + h : 0.0, xm = show ? cx - h : 0.0, yp = show ? cy + h : 0.0, ym = show ? cy - h : 0.0,
                   zp = show ? cz + h : 0.0, zm = show ? cz - h : 0.0;
      out[3] = xp; out[4] = cy; out[5] = cz;
      out[6] = xm; out[7] = cy; out[8] = cz;
      out[9] = cx; out[10] = yp; out[11] = cz;
      out[12] = cx; out[13] = ym; out[14] = cz;
      out[15] = cx; out[16] = cy; out[17] = zp;
      out[18] = cx; out[19] = cy; out[20] = zm;
    }
  }
  TrafficRec& R = a.recs[(size_t)t];  // (a lane past the last sample has a slot too: show = 0)
  R.c[0] = cx; R.c[1] = cy; R.c[2] = cz;
  R.show = show ? 1 : 0; R.k = k;
  const double lx = wave_min(show ? cx : INFINITY), ly = wave_min(show ? cy : INFINITY), lz = wave_min(show ? cz : INFINITY);
  const double hx = wave_max(show ? cx : -INFINITY), hy = wave_max(show ? cy : -INFINITY), hz = wave_max(show ? cz : -INFINITY);
  if (lane == 0) {
    const double gx = cell_box_margin(a.range, lx, hx), gy = cell_box_margin(a.range, ly, hy), gz = cell_box_margin(a.range, lz, hz);
    TrafficBox& B = a.boxes[chunk];
    B.lo[0] = lx - gx; B.lo[1] = ly - gy; B.lo[2] = lz - gz;
    B.hi[0] = hx + gx; B.hi[1] = hy + gy; B.hi[2] = hz + gz;
  }
}

template <int PPS>
__device__ __forceinline__ void traffic_timed_mask(const TrafficTimedArgs& b) {
#pragma clang fp contract(off)
  using fhw::lane_id;
  using fhw::wave_max;
  using fhw::wave_min;
  constexpr int WPC = 2 * PPS;  // words per chunk
  // the observer's samples, NaN where one does not show.  One wavefront is the workgroup: the barriers order its LDS accesses only.
  __shared__ double ox[FH_TRAFFIC_TIMED_MAX_SAMPLES], oy[FH_TRAFFIC_TIMED_MAX_SAMPLES], oz[FH_TRAFFIC_TIMED_MAX_SAMPLES];
  const TrafficArgs& a = b.t;
  const int lane = lane_id();
  const int S = a.samples;
  const int c0 = (int)blockIdx.x * 64;  // the first chunk of this group
  if (c0 >= a.n_chunks) return;
  const int chunk = c0 + lane;
  double x0 = NAN, x1 = NAN, y0 = NAN, y1 = NAN, z0 = NAN, z1 = NAN;
  if (chunk < a.n_chunks) {
    const TrafficBox& B = a.boxes[chunk];
    x0 = B.lo[0]; y0 = B.lo[1]; z0 = B.lo[2];
    x1 = B.hi[0]; y1 = B.hi[1]; z1 = B.hi[2];
  }
  const int w0 = c0 * WPC;                                // the group's first word among the traffic words
  const int group_words = min(64 * WPC, a.n_words - w0);  // (the last chunk may end before its 2 PPS words do)
  for (int i = (int)blockIdx.y; i < a.n; i += (int)gridDim.y) {
    __syncthreads();  // (the last row's reads are done)
    double lx = INFINITY, ly = INFINITY, lz = INFINITY, hx = -INFINITY, hy = -INFINITY, hz = -INFINITY;
    for (int s0 = 0; s0 < S; s0 += 64) {
      const int sp = s0 + lane;
      bool show = false;
      double x = NAN, y = NAN, z = NAN;
      if (sp < S) {
        const TrafficRec& R = a.recs[(size_t)i * (size_t)S + (size_t)sp];
        show = R.show != 0;
        if (show) { x = R.c[0]; y = R.c[1]; z = R.c[2]; }
        ox[sp] = x; oy[sp] = y; oz[sp] = z;
      }
      lx = fmin(lx, wave_min(show ? x : INFINITY)); ly = fmin(ly, wave_min(show ? y : INFINITY)); lz = fmin(lz, wave_min(show ? z : INFINITY));
      hx = fmax(hx, wave_max(show ? x : -INFINITY)); hy = fmax(hy, wave_max(show ? y : -INFINITY)); hz = fmax(hz, wave_max(show ? z : -INFINITY));
    }
    __syncthreads();
    const double gx = cell_box_margin(0.0, lx, hx), gy = cell_box_margin(0.0, ly, hy), gz = cell_box_margin(0.0, lz, hz);
    const double rx0 = lx - gx, rx1 = hx + gx, ry0 = ly - gy, ry1 = hy + gy, rz0 = lz - gz, rz1 = hz + gz;
    const unsigned long long looked = __ballot(x0 <= rx1 && x1 >= rx0 && y0 <= ry1 && y1 >= ry0 && z0 <= rz1 && z1 >= rz0);
    uint32_t* row = a.mask + ((size_t)i * (size_t)a.mask_words + (size_t)a.first_word + (size_t)w0);
    for (int w = lane; w < group_words; w += 64)
      if (!((looked >> (w / WPC)) & 1ull)) row[w] = 0u;
    for (unsigned long long rest = looked; rest; rest &= rest - 1ull) {
      const int ch = (int)__builtin_ctzll(rest);
      const int t = (c0 + ch) * 64 + lane;
      const TrafficRec& R = a.recs[(size_t)t];
      const double cx = R.c[0], cy = R.c[1], cz = R.c[2];
      const int k = R.k;
      const bool ask = R.show != 0 && k != i && (a.rule == FH_TRAFFIC_ALL || k < i);
      const int s = ask ? t - k * S : 0;  // (a shown sample has t < n S and k = t / S)
      const int lo = max(0, s - b.window), hi = ask ? min(S - 1, s + b.window) : -1;
      bool near = false;
      for (int q = 0; q < b.span; q++) {
        const int sp = lo + q, at = min(sp, S - 1);
        const double dx = cx - ox[at], dy = cy - oy[at], dz = cz - oz[at];
        const double d2 = dx * dx + dy * dy + dz * dz;
        near = near || (sp <= hi && d2 < a.range2);
      }
      const unsigned long long ballot = __ballot(near);
      const int w = ch * WPC + lane;
      if (lane < WPC && w < group_words) row[w] = traffic_word<PPS>(ballot, lane);
    }
  }
}

// Plain kernels, as in fh_traffic.hip.hpp and for its reason.
__global__ void __launch_bounds__(64) traffic_timed_points1_kernel(TrafficTimedArgs a) { traffic_timed_points<1>(a); }
__global__ void __launch_bounds__(64) traffic_timed_points7_kernel(TrafficTimedArgs a) { traffic_timed_points<7>(a); }
__global__ void __launch_bounds__(64) traffic_timed_mask1_kernel(TrafficTimedArgs a) { traffic_timed_mask<1>(a); }
__global__ void __launch_bounds__(64) traffic_timed_mask7_kernel(TrafficTimedArgs a) { traffic_timed_mask<7>(a); }

}  // namespace fh

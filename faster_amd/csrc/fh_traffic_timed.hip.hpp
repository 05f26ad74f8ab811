// fh_traffic_timed.hip.hpp — time-aware traffic (include/fasterhip_traffic_timed.h, which is the specification): the points kernels,
// slots, words, working buffers and mask frame of fh_traffic.hip.hpp, and other bits.  Sample (k, s) is shown to vehicle i when vehicle
// i's OWN committed plan has a shown sample s' with |s - s'| <= window within `range` of it; state_i.pos is not read.
//   traffic_timed_mask{1,7}_kernel: traffic_rows with
//     row:    the S records of vehicle i are staged once into LDS as three arrays of doubles (24 bytes per sample, 12 KB at the cap), a
//             sample that does not show as NaN: every comparison with it fails without a branch.  The box of i's shown samples is
//             reduced on the way (wave_min / wave_max).  Lane = chunk: does the chunk's grown box overlap the row box?
//     decide: lane = sample t, s = t - k S; the loop over the window reads LDS at lo + q, lo = max(0, s - window): neighbouring lanes
//             read neighbouring doubles (or, where the window is clipped at 0, the same one), which is free of bank conflicts.  The d2
//             decisions are ORed.
// THE ROW BOX.  A bit needs a shown c' = c[i][s'] and a shown c = c[k][s] with d2 < range range, so |c - c'| < range (1 + 4e-16) per
// axis.  c lies in its chunk's box [lo, hi] exactly and c' in the row box [rlo, rhi] exactly, hence rhi >= c' > lo - range (1 + 4e-16)
// and rlo <= c' < hi + range (1 + 4e-16): the chunk box grown by cell_box_margin(range, lo, hi) (fh_traffic.hip.hpp argues the margin)
// overlaps the row box.  The row box is grown by cell_box_margin(0, rlo, rhi) besides, the relative part alone: it costs nothing and
// the argument does not need it.  An observer none of whose samples show has an empty row box and every word stored as zero.
// An LDS index is clamped to [0, S - 1] before it is used.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fasterhip_traffic_timed.h"
#include "fh_traffic.hip.hpp"

namespace fh {

template <int PPS>
__device__ __forceinline__ void traffic_timed_mask(const TrafficArgs& a) {
#pragma clang fp contract(off)
  using fhw::wave_max;
  using fhw::wave_min;
  // the observer's samples, NaN where one does not show.  One wavefront is the workgroup: the barriers order its LDS accesses only.
  __shared__ double ox[FH_TRAFFIC_TIMED_MAX_SAMPLES], oy[FH_TRAFFIC_TIMED_MAX_SAMPLES], oz[FH_TRAFFIC_TIMED_MAX_SAMPLES];
  const int lane = fhw::lane_id();
  const int S = a.samples;
  traffic_rows<PPS>(
      a,
      [&](int i, const TrafficBox& B) {
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
        return __ballot(B.lo[0] <= rx1 && B.hi[0] >= rx0 && B.lo[1] <= ry1 && B.hi[1] >= ry0 && B.lo[2] <= rz1 && B.hi[2] >= rz0);
      },
      [&](int i, int t, const TrafficRec& R) {
        const double cx = R.c[0], cy = R.c[1], cz = R.c[2];
        const int k = R.k;
        const bool ask = R.show != 0 && k != i && (a.rule == FH_TRAFFIC_ALL || k < i);
        const int s = ask ? t - k * S : 0;  // (a shown sample has t < n S and k = t / S)
        const int lo = max(0, s - a.window), hi = ask ? min(S - 1, s + a.window) : -1;
        bool near = false;
        for (int q = 0; q < a.span; q++) {
          const int sp = lo + q, at = min(sp, S - 1);
          const double dx = cx - ox[at], dy = cy - oy[at], dz = cz - oz[at];
          const double d2 = dx * dx + dy * dy + dz * dz;
          near = near || (sp <= hi && d2 < a.range2);
        }
        return near;
      });
}

// Plain kernels, as in fh_traffic.hip.hpp and for its reason.
__global__ void __launch_bounds__(64) traffic_timed_mask1_kernel(TrafficArgs a) { traffic_timed_mask<1>(a); }
__global__ void __launch_bounds__(64) traffic_timed_mask7_kernel(TrafficArgs a) { traffic_timed_mask<7>(a); }

}  // namespace fh

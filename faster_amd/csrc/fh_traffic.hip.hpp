// fh_traffic.hip.hpp — the committed plans of the other vehicles as occupied points of a vehicle's view, under both rules: untimed
// (include/fasterhip_traffic.h) here, matched instant by instant (include/fasterhip_traffic_timed.h) in fh_traffic_timed.hip.hpp; the
// two public headers are the specification.  Reads the vehicle records and the plans; writes the traffic points at the tail of the
// cloud, the traffic words of every mask row, and two working buffers of the context.  Samples are numbered t = k S + s, sample s is
// the instant first_instant + s stride (the untimed entry point passes 0); 64 samples are a CHUNK, which is one wavefront of the first
// kernel and one ballot of the second.  first_point is a multiple of 32 and a chunk has 64 pps bits, so a chunk owns 2 pps whole words
// of a row: 2 with one point per sample, 14 with seven.  Two launches:
//   traffic_points{1,7}_kernel (both rules): one wavefront per chunk, lane = sample.  The plan extent is checked, the sampled position
//                      read (a plan that has ended stands at its last state), the PPS points of the slot written (zeros when the
//                      sample does not show), and a compact record per sample (centre, show word, vehicle number: 32 B) goes to
//                      TRAFFIC_SAMPLES: the second kernel never reads a vehicle's plan.  The box of the shown centres of the chunk
//                      goes to TRAFFIC_BOXES, already grown by range + g: the prefilter of the second kernel is six comparisons.
//   a mask kernel:     one wavefront per (group of 64 chunks, row i); the grid is at most TRAFFIC_GRID_ROWS high and a wavefront takes
//                      every TRAFFIC_GRID_ROWS-th row, so the boxes of its group are loaded once for all of them.  traffic_rows is
//                      the frame of all four: per row the rule's ROW step says, lane = chunk, which chunks are looked at (one
//                      ballot).  The words of the others are stored as zeros, lane = word, coalesced.  For each chunk that is looked
//                      at: lane = sample, the 64 records in one coalesced load, the rule's DECIDE step, one ballot; then lane = word:
//                      lanes 0 .. 2 PPS - 1 assemble their 32 bits from the ballot (a sample's PPS bits share its decision) and
//                      store them.  No atomics, every word of the row stored exactly once.
//   traffic_mask{1,7}_kernel: row = is the position of vehicle i inside the grown box of the chunk?  decide = d2 to that position, as
//                      the model writes it.  No LDS.
// PREFILTERS ARE CONSERVATIVE.  A bit is decided by its d2 alone; the box only decides what is looked at.  A shown centre c lies in
// its chunk's box exactly, and d2 < range range needs |c - p| < range (1 + 4e-16) per axis; g = 1e-9 (range + |lo| + |hi|), the audit's
// relative margin, is seven orders above the roundings of lo - (range + g) and of d2.  An empty box is (+inf, -inf): its grown bounds are
// NaN and no comparison holds.  A position of vehicle i that is a NaN fails every comparison; one that is infinite may pass a box that
// overflowed, and the decision itself then asks for a finite position.
// Every index comes from a checked record: head and size are tested against max_states before the plan is read, the compact records
// carry vehicle numbers < n, and both buffers are sized in whole chunks, so a lane past the last sample reads and writes its own slot.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fasterhip_traffic.h"
#include "fh_cells.hip.hpp"
#include "fh_plans.hip.hpp"
#include "fh_wave.hip.hpp"

namespace fh {

constexpr int TRAFFIC_GRID_ROWS = 1024;  // the height of the mask kernels' grid: 8 groups of a 4096-vehicle fleet fill 256 CUs

struct TrafficRec {  // 32 B: what the mask kernel needs of a sample
  double c[3];
  int show, k;  // show: 1 iff the sample shows; k: its vehicle
};

struct TrafficBox {  // 48 B: the box of the shown centres of a chunk, grown by range + g (lo > hi or NaN: no centre)
  double lo[3], hi[3];
};

struct TrafficArgs {
  double range, range2, hull;  // range2 = range * range, rounded once on the host as the model rounds it
  int samples, stride, rule, first_point;
  int n, max_states, n_samples, n_chunks;  // n_samples = n S; n_chunks = ceil(n_samples / 64)
  int mask_words, first_word, n_words;     // the traffic words of a row: [first_word, first_word + n_words)
  int first_instant;                       // sample s is the instant first_instant + s stride
  int window, span;                        // the timed mask kernels alone: min(window, S - 1) and min(2 window + 1, S)
  const fh_vehicle* vehicles;
  const fh_state* plans;
  double* cloud;
  uint32_t* mask;
  TrafficRec* recs;   // [64 n_chunks]
  TrafficBox* boxes;  // [n_chunks]
};

template <int PPS>
__device__ __forceinline__ void traffic_points(const TrafficArgs& a) {
#pragma clang fp contract(off)
  using fhw::lane_id;
  using fhw::wave_max;
  using fhw::wave_min;
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
      const long long j = (long long)a.first_instant + (long long)s * (long long)a.stride, last = (long long)size - 1;
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

// Bits [32 w, 32 w + 32) of the stream in which sample s < 64 owns the PPS bits from PPS s on, all equal to bit s of `ballot`.
template <int PPS>
__device__ __forceinline__ unsigned traffic_word(unsigned long long ballot, int w) {
  if (PPS == 1) return (unsigned)(ballot >> (32 * w));
  unsigned word = 0u;
  const int s0 = (32 * w) / PPS;
#pragma unroll
  for (int q = 0; q < 32 / PPS + 2; q++) {
    const int s = s0 + q, off = PPS * s - 32 * w;  // off > -PPS
    if (s < 64 && off < 32 && ((ballot >> s) & 1ull)) word |= off >= 0 ? ((1u << PPS) - 1u) << off : ((1u << PPS) - 1u) >> -off;
  }
  return word;
}

// The frame of the mask kernels.  row_step(i, B) is wave-uniform in i and returns the ballot of the chunks (lane = chunk, B = the lane's
// grown box, NaN past the last chunk) that row i looks at; decide(i, t, R) is the lane's decision on sample t, whose record is R.
template <int PPS, class Row, class Decide>
__device__ __forceinline__ void traffic_rows(const TrafficArgs& a, Row&& row_step, Decide&& decide) {
  constexpr int WPC = 2 * PPS;  // words per chunk
  const int lane = fhw::lane_id();
  const int c0 = (int)blockIdx.x * 64;  // the first chunk of this group
  if (c0 >= a.n_chunks) return;
  const int chunk = c0 + lane;
  TrafficBox B = {{NAN, NAN, NAN}, {NAN, NAN, NAN}};
  if (chunk < a.n_chunks) B = a.boxes[chunk];
  const int w0 = c0 * WPC;                                // the group's first word among the traffic words
  const int group_words = min(64 * WPC, a.n_words - w0);  // (the last chunk may end before its 2 PPS words do)
  for (int i = (int)blockIdx.y; i < a.n; i += (int)gridDim.y) {
    const unsigned long long looked = row_step(i, B);
    uint32_t* row = a.mask + ((size_t)i * (size_t)a.mask_words + (size_t)a.first_word + (size_t)w0);
    for (int w = lane; w < group_words; w += 64)
      if (!((looked >> (w / WPC)) & 1ull)) row[w] = 0u;
    for (unsigned long long rest = looked; rest; rest &= rest - 1ull) {
      const int ch = (int)__builtin_ctzll(rest);
      const int t = (c0 + ch) * 64 + lane;
      const unsigned long long ballot = __ballot(decide(i, t, a.recs[(size_t)t]));
      const int w = ch * WPC + lane;
      if (lane < WPC && w < group_words) row[w] = traffic_word<PPS>(ballot, lane);
    }
  }
}

template <int PPS>
__device__ __forceinline__ void traffic_mask(const TrafficArgs& a) {
#pragma clang fp contract(off)
  using fhw::uniform_f64;
  double px, py, pz;  // where vehicle i stands
  bool p_finite;
  traffic_rows<PPS>(
      a,
      [&](int i, const TrafficBox& B) {
        const double* p = a.vehicles[i].state.pos;
        px = uniform_f64(p[0]); py = uniform_f64(p[1]); pz = uniform_f64(p[2]);
        p_finite = plan_finite(px) && plan_finite(py) && plan_finite(pz);
        return __ballot(px >= B.lo[0] && px <= B.hi[0] && py >= B.lo[1] && py <= B.hi[1] && pz >= B.lo[2] && pz <= B.hi[2]);
      },
      [&](int i, int, const TrafficRec& R) {
        const double dx = R.c[0] - px, dy = R.c[1] - py, dz = R.c[2] - pz;
        const double d2 = dx * dx + dy * dy + dz * dz;
        const int k = R.k;
        return R.show != 0 && k != i && (a.rule == FH_TRAFFIC_ALL || k < i) && p_finite && d2 < a.range2;
      });
}

// Plain kernels, one per number of points per sample; both entry points launch the points pair.  As instantiations of a kernel template
// they were laid out elsewhere in the code object, and the pair solve kernels came out with other offsets in their calls of out-of-line
// functions (the byte check).
__global__ void __launch_bounds__(64) traffic_points1_kernel(TrafficArgs a) { traffic_points<1>(a); }
__global__ void __launch_bounds__(64) traffic_points7_kernel(TrafficArgs a) { traffic_points<7>(a); }
__global__ void __launch_bounds__(64) traffic_mask1_kernel(TrafficArgs a) { traffic_mask<1>(a); }
__global__ void __launch_bounds__(64) traffic_mask7_kernel(TrafficArgs a) { traffic_mask<7>(a); }

}  // namespace fh

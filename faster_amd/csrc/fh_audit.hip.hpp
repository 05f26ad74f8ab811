// fh_audit.hip.hpp — the audit of committed plans (include/fasterhip_audit.h, which is the specification): every tested state of a
// vehicle's plan against the unknown voxel centres of its view and against the cloud points it knows (or all of them).  Reads the
// vehicle records, the plans, the views, the cloud and the masks; writes one fh_plan_audit per vehicle and nothing else.
//
// audit_kernel: one wavefront per vehicle, one wavefront per workgroup (the LDS below is the wavefront's own), grid n; no atomics, no
// state between workgroups.  In every distance loop lane = tested state: round s holds tested state t = 64 s + lane, plan index
// j = t stride, and a lane keeps (smallest d2, the smallest j that attains it, the smallest j with d2 < r r) of what it has seen.
//   pass 0        : the bounding box of the finite tested positions (wave_min / wave_max) and the not-finite flag.
//   unknown side  : the cells of the box, grown, in slabs of at most SLAB_WORDS words of 64 cells: rows along x (a tile of at most
//                   TILE_X cells) numbered (z, y); the wavefront reads the view's bytes row by row, 64 consecutive bytes per load,
//                   and keeps them as bits (__ballot).  Then every lane walks the cells of the cube of its own state that lie in
//                   the slab, reads words from LDS and evaluates d2 for set bits only.  A box that fits is one slab.
//   occupied side : the cloud is swept 64 points at a time, lane = point; finite points whose mask bit is set and which lie in the
//                   grown box are compacted into an LDS list (ballot + rank).  When the list cannot take 64 more, or the cloud ends,
//                   it is tested with lane = state and broadcast reads, and emptied.
//   the record leaves as one 16-byte store from each of lanes 0..3.
// PREFILTERS ARE CONSERVATIVE.  A candidate counts only if its d2, computed as the model writes it, is below cap cap; box and cube
// only decide what is looked at.  Both are grown by cap + g with g = 1e-9 (cap + |lo| + |hi|) on the occupied side, and
// g = res + 1e-9 (cap + |lo| + |hi| + |origin|) and one more cell on each side on the unknown side: the roundings of lo - (cap + g),
// of (x - origin) / res and of d2 itself are relative 1e-16, seven orders below that margin, so no candidate with d2 < cap cap is lost.
// A position is turned into a cell number by comparing in double first: no NaN, infinity or 1e300 is ever converted to int.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fasterhip_audit.h"
#include "fh_cells.hip.hpp"
#include "fh_plans.hip.hpp"
#include "fh_wave.hip.hpp"

namespace fh {

constexpr int AUDIT_LIST = FH_AUDIT_LIST_POINTS;
constexpr int AUDIT_SLAB_WORDS = FH_AUDIT_SLAB_CELLS / 64;  // 64-bit words of one slab
constexpr int AUDIT_TILE_X = 4096;                          // cells of a row tile: at most 64 words per row, at least 16 rows per slab

struct AuditArgs {
  double r2_unknown, r2_occupied, cap, cap2;  // r * r and cap * cap, rounded once on the host as the model rounds them
  int stride, count, n, max_states;
  const fh_vehicle* vehicles;
  const fh_state* plans;
  double ox, oy, oz, res;  // the lattice of the views
  int nx, ny, nz, n_views;
  const unsigned char* flags;  // NULL: no unknown side
  size_t view_stride;
  const int32_t* view_of;
  const double* cloud;  // NULL: no occupied side
  int n_cloud, mask_words;
  const unsigned* mask;  // NULL: every point counts
  fh_plan_audit* out;
};

struct AuditBest {  // what one lane has seen on one side
  double d2;
  int j_min, j_first;
};

__device__ __forceinline__ void audit_take(AuditBest& b, double d2, double cap2, double r2, int j) {
  if (d2 < cap2) {
    if (d2 < b.d2 || (d2 == b.d2 && j < b.j_min)) { b.d2 = d2; b.j_min = j; }
    if (d2 < r2 && j < b.j_first) b.j_first = j;
  }
}

// The cells [a, b] of one axis (n cells of size res from o) whose centres can lie within cap of [lo, hi]; false: none.  grow is
// cap + the margin of the header comment; one more cell on each side covers the half cell between a centre and its cell's border.
__device__ __forceinline__ bool audit_cells(double lo, double hi, double grow, double o, double res, int n, int& a, int& b) {
#pragma clang fp contract(off)
  const double fa = floor(((lo - grow) - o) / res) - 1.0, fb = floor(((hi + grow) - o) / res) + 1.0;
  const double last = (double)(n - 1);
  if (!(fa <= last) || !(fb >= 0.0)) return false;  // (a NaN leaves here)
  a = fa >= 0.0 ? (int)fa : 0;
  b = fb <= last ? (int)fb : n - 1;
  return a <= b;
}
__device__ __forceinline__ double audit_grow_cells(double lo, double hi, double cap, double o, double res) {
#pragma clang fp contract(off)
  return cap + (res + 1e-9 * (cap + fabs(lo) + fabs(hi) + fabs(o)));
}

// minimum d2, then the smallest index among the lanes that hold it; the smallest first index.  INT_MAX stands for "none".
__device__ __forceinline__ void audit_reduce(const AuditBest& b, double& d2, int& worst, int& first) {
  d2 = fhw::wave_min(b.d2);
  worst = fhw::wave_min_i32(b.d2 == d2 && d2 < INFINITY ? b.j_min : 0x7fffffff);
  first = fhw::wave_min_i32(b.j_first);
  if (worst == 0x7fffffff) worst = -1;
  if (first == 0x7fffffff) first = -1;
}

__global__ void __launch_bounds__(64) audit_kernel(AuditArgs a) {
#pragma clang fp contract(off)
  __shared__ unsigned long long slab[AUDIT_SLAB_WORDS];
  __shared__ double list_x[AUDIT_LIST], list_y[AUDIT_LIST], list_z[AUDIT_LIST];
  const int lane = fhw::lane_id();
  const int i = (int)blockIdx.x;
  if (i >= a.n) return;
  const fh_vehicle& V = a.vehicles[i];
  const int head = fhw::uniform_i32(V.plan_head), size = fhw::uniform_i32(V.plan_size);
  int flags = 0, n_tested = 0, view = -1;
  int first_u = -1, worst_u = -1, first_o = -1, worst_o = -1;
  double min_u = INFINITY, min_o = INFINITY;
  const bool bad = head < 0 || size < 0 || (long long)head + (long long)size > (long long)a.max_states;  // (plan_bad_extent, written out: see there)
  if (bad) {
    flags = FH_AUDIT_BAD_PLAN;
  } else {
    n_tested = plan_instants(plan_limit(a.count, size), a.stride);
    const int rounds = (n_tested + 63) >> 6;
    const fh_state* plan = a.plans + ((size_t)i * (size_t)a.max_states + (size_t)head);
    const bool side_o = a.cloud && a.n_cloud > 0;
    bool side_u = a.flags != nullptr, masked = side_o && a.mask;
    if (side_u || masked) {
      view = (a.flags && a.view_stride == 0 && a.n_views == 1) ? 0 : (a.view_of ? fhw::uniform_i32(a.view_of[i]) : i);
      if (view < 0 || view >= a.n_views) {
        flags |= FH_AUDIT_NO_VIEW;
        side_u = false;
      }
    }
    const bool no_view = (flags & FH_AUDIT_NO_VIEW) != 0;

    // ---- pass 0: the box of the finite tested positions ----
    double lx = INFINITY, ly = INFINITY, lz = INFINITY, hx = -INFINITY, hy = -INFINITY, hz = -INFINITY;
    bool not_finite = false;
    for (int s = 0; s < rounds; s++) {
      const int t = s * 64 + lane;
      if (t < n_tested) {
        const double* p = plan[(size_t)t * (size_t)a.stride].pos;
        const double x = p[0], y = p[1], z = p[2];
        if (plan_finite(x) && plan_finite(y) && plan_finite(z)) {
          lx = x < lx ? x : lx; ly = y < ly ? y : ly; lz = z < lz ? z : lz;
          hx = x > hx ? x : hx; hy = y > hy ? y : hy; hz = z > hz ? z : hz;
        } else {
          not_finite = true;
        }
      }
    }
    if (fhw::wave_any(not_finite)) flags |= FH_AUDIT_NOT_FINITE;
    lx = fhw::wave_min(lx); ly = fhw::wave_min(ly); lz = fhw::wave_min(lz);
    hx = fhw::wave_max(hx); hy = fhw::wave_max(hy); hz = fhw::wave_max(hz);
    const bool any_state = lx <= hx;  // (uniform; false when every tested position was skipped or there is none)

    // ---- unknown side ----
    if (side_u && any_state) {
      AuditBest best = {INFINITY, 0x7fffffff, 0x7fffffff};
      int bx0, bx1, by0, by1, bz0, bz1;
      const bool some = audit_cells(lx, hx, audit_grow_cells(lx, hx, a.cap, a.ox, a.res), a.ox, a.res, a.nx, bx0, bx1) &&
                        audit_cells(ly, hy, audit_grow_cells(ly, hy, a.cap, a.oy, a.res), a.oy, a.res, a.ny, by0, by1) &&
                        audit_cells(lz, hz, audit_grow_cells(lz, hz, a.cap, a.oz, a.res), a.oz, a.res, a.nz, bz0, bz1);
      if (some) {
        const unsigned char* vf = a.flags + (size_t)view * a.view_stride;
        const int by = by1 - by0 + 1;
        const long long rows = (long long)by * (long long)(bz1 - bz0 + 1);
        for (long long tile = bx0; tile <= (long long)bx1; tile += AUDIT_TILE_X) {
          const int tx0 = (int)tile, tx1 = (int)min((long long)bx1, tile + AUDIT_TILE_X - 1), rw = (tx1 - tx0 + 64) >> 6;  // words per row
          const int rps = AUDIT_SLAB_WORDS / rw;                                        // rows per slab
          for (long long r0 = 0; r0 < rows; r0 += rps) {
            const long long r1 = min(rows, r0 + (long long)rps);
            // the view's bytes of rows [r0, r1), as bits
            const int zs0 = bz0 + (int)(r0 / by), zs1 = bz0 + (int)((r1 - 1) / by);
            int z = zs0, y = by0 + (int)(r0 % by);
            for (long long r = r0; r < r1; r++, z += y == by1, y = y == by1 ? by0 : y + 1) {
              const unsigned char* row = vf + ((size_t)z * (size_t)a.ny + (size_t)y) * (size_t)a.nx;
              for (int c = 0; c < rw; c++) {
                const int x = tx0 + c * 64 + lane;
                const unsigned long long bits = __ballot(x <= tx1 && row[x] != 0);
                if (lane == 0) slab[(int)(r - r0) * rw + c] = bits;
              }
            }
            __syncthreads();
            for (int s = 0; s < rounds; s++) {
              const int t = s * 64 + lane;
              if (t >= n_tested) continue;
              const int j = t * a.stride;
              const double* p = plan[j].pos;
              const double px = p[0], py = p[1], pz = p[2];
              if (!(plan_finite(px) && plan_finite(py) && plan_finite(pz))) continue;
              int xa, xb, ya, yb, za, zb;
              if (!audit_cells(px, px, audit_grow_cells(px, px, a.cap, a.ox, a.res), a.ox, a.res, a.nx, xa, xb)) continue;
              if (!audit_cells(py, py, audit_grow_cells(py, py, a.cap, a.oy, a.res), a.oy, a.res, a.ny, ya, yb)) continue;
              if (!audit_cells(pz, pz, audit_grow_cells(pz, pz, a.cap, a.oz, a.res), a.oz, a.res, a.nz, za, zb)) continue;
              xa = max(xa, tx0); xb = min(xb, tx1);
              ya = max(ya, by0); yb = min(yb, by1);
              za = max(za, zs0); zb = min(zb, zs1);
              if (xa > xb) continue;
              const int c0 = (xa - tx0) >> 6, c1 = (xb - tx0) >> 6;
              for (int z = za; z <= zb; z++) {
                const double dz = (((double)z + 0.5) * a.res + a.oz) - pz;
                for (int y = ya; y <= yb; y++) {
                  const long long r = (long long)(z - bz0) * by + (y - by0);
                  if (r < r0 || r >= r1) continue;
                  const double dy = (((double)y + 0.5) * a.res + a.oy) - py;
                  for (int c = c0; c <= c1; c++) {
                    unsigned long long w = slab[(int)(r - r0) * rw + c];
                    const int xw = tx0 + c * 64;  // the cell of bit 0
                    if (xa > xw) w &= ~0ull << (xa - xw);
                    if (xb < xw + 63) w &= ~0ull >> (xw + 63 - xb);
                    while (w) {
                      const int x = xw + (int)__builtin_ctzll(w);
                      w &= w - 1;
                      const double dx = (((double)x + 0.5) * a.res + a.ox) - px;
                      audit_take(best, dx * dx + dy * dy + dz * dz, a.cap2, a.r2_unknown, j);
                    }
                  }
                }
              }
            }
            __syncthreads();
          }
        }
      }
      audit_reduce(best, min_u, worst_u, first_u);
      if (first_u >= 0) flags |= FH_AUDIT_UNKNOWN;
    }

    // ---- occupied side ----
    if (side_o && any_state && !(masked && no_view)) {
      AuditBest best = {INFINITY, 0x7fffffff, 0x7fffffff};
      const unsigned* mrow = masked ? a.mask + (size_t)view * (size_t)a.mask_words : nullptr;
      const double gx = cell_box_margin(a.cap, lx, hx), gy = cell_box_margin(a.cap, ly, hy), gz = cell_box_margin(a.cap, lz, hz);
      const double x0 = lx - gx, x1 = hx + gx, y0 = ly - gy, y1 = hy + gy, z0 = lz - gz, z1 = hz + gz;
      int n_list = 0;  // (uniform)
      for (long long k0 = 0; k0 < (long long)a.n_cloud; k0 += 64) {
        const int k = (int)min(k0 + lane, (long long)a.n_cloud);  // (n_cloud: past the end)
        bool keep = false;
        double qx = 0.0, qy = 0.0, qz = 0.0;
        if (k < a.n_cloud && (!mrow || ((mrow[k >> 5] >> (k & 31)) & 1u))) {
          qx = a.cloud[3 * (size_t)k]; qy = a.cloud[3 * (size_t)k + 1]; qz = a.cloud[3 * (size_t)k + 2];
          // (a NaN fails a comparison; an infinity lies outside a box of finite positions unless the box itself overflowed)
          keep = qx >= x0 && qx <= x1 && qy >= y0 && qy <= y1 && qz >= z0 && qz <= z1 && plan_finite(qx) && plan_finite(qy) && plan_finite(qz);
        }
        const unsigned long long km = __ballot(keep);
        if (keep) {
          const int slot = n_list + fhw::rank_in(km);
          list_x[slot] = qx; list_y[slot] = qy; list_z[slot] = qz;
        }
        n_list += (int)__popcll(km);
        if (n_list > AUDIT_LIST - 64 || k0 + 64 >= (long long)a.n_cloud) {
          __syncthreads();
          if (n_list > 0) {
            for (int s = 0; s < rounds; s++) {
              const int t = s * 64 + lane;
              if (t >= n_tested) continue;
              const int j = t * a.stride;
              const double* p = plan[j].pos;
              const double px = p[0], py = p[1], pz = p[2];
              if (!(plan_finite(px) && plan_finite(py) && plan_finite(pz))) continue;
              for (int q = 0; q < n_list; q++) {
                const double dx = list_x[q] - px, dy = list_y[q] - py, dz = list_z[q] - pz;
                audit_take(best, dx * dx + dy * dy + dz * dz, a.cap2, a.r2_occupied, j);
              }
            }
          }
          __syncthreads();
          n_list = 0;
        }
      }
      audit_reduce(best, min_o, worst_o, first_o);
      if (first_o >= 0) flags |= FH_AUDIT_OCCUPIED;
    }
  }
  // words 2 l and 2 l + 1 of the record from lane l < 4: 64 contiguous bytes in one store instruction
  double w0 = 0.0, w1 = 0.0;
  if (lane == 0) { w0 = plan_pack(flags, n_tested); w1 = plan_pack(first_u, worst_u); }
  if (lane == 1) { w0 = plan_pack(first_o, worst_o); w1 = plan_pack(view, 0); }
  if (lane == 2) { w0 = min_u; w1 = min_o; }
  if (lane < 4) reinterpret_cast<double2*>(a.out + i)[lane] = make_double2(w0, w1);
}

}  // namespace fh

// fh_link.hip.hpp — vehicles in radio range pool what their views know (include/fasterhip_link.h, which is the specification): who is
// linked to whom (d2 < range range between two speaking vehicles), from that a label per view by passes of hook and jump, and the merge
// that makes the flag rows and the shared mask words of a group equal.  The broad phase is the cell grid (fh_cells.hip.hpp: its
// launches, why its prefilters lose nothing and where every index comes from), with range; the box of a vehicle is its one position.
//   link_boxes_kernel  : one wavefront per vehicle k.  view(k) is checked against n_views and the position against finiteness: a
//                        vehicle that speaks gets a box of one point (lo = hi = pos, exactly) and its view; the others are not boxed
//                        and are in no cell.
//   link_narrow_kernel : one wavefront per vehicle i, lane = candidate of the walk.  d2 as the model writes it, from the two points of
//                        the boxes; the views of the linked go into row i (their slots from the ballot and the rank of the lane, no
//                        atomics; the row keeps the first FH_LINK_LIST), nbrs[i] counts all of them, and the pairs with k > i are
//                        added to info[2] once per wavefront.
//   link_init_kernel   : lane = view: L[v] = H[v] = v.
//   link_hook_kernel   : one wavefront per vehicle i, launched once per pass: m = the smallest L[view(k)] over the linked k — from the
//                        row when nbrs[i] fits it, else by walking the cells again with the same test — and, only where m < L[view(i)],
//                        an atomic minimum into H[view(i)].  Reads L, writes H: H entered the launch as a copy of L.
//   link_jump_kernel   : lane = view: L'[v] = H[H[v]] into L (only where it differs) and into the other copy, which the next hook
//                        lowers.  The last pass counts the views that changed and the roots into info[0] and info[1].
//   link_merge_flags_kernel / link_merge_mask_kernel : blockIdx.y = view.  A view that sends (its label is another view that is its own
//                        label) folds into its root (take = 0) or takes from it (take = 1); every other view returns at once.  Flags:
//                        a lane owns 16 bytes of the DESTINATION row that are aligned in memory, reads them and the 16 source bytes,
//                        and clears, word by word, the bytes that are zero in the source and not in the destination: atomic AND on a
//                        word that lies wholly inside the row (no other row shares it), single-byte stores of zero at the ends.  Masks:
//                        a lane owns four words; atomic OR of the bits the destination lacks.  Nothing is written where nothing differs.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/fasterhip_link.h"
#include "fh_cells.hip.hpp"
#include "fh_wave.hip.hpp"

namespace fh {

static_assert(FH_LINK_LIST == 64, "a row of the lists is filled from ballots of 64");

struct LinkBox {  // 64 B
  CellBox c;
  int view, pad;  // the checked view of a vehicle that speaks (0 otherwise)
};

struct LinkArgs {
  double range, r2;  // range * range rounded once on the host, as the model rounds it
  int n, n_views;
  const fh_vehicle* vehicles;
  const int32_t* view_of;
  CellGrid g;
  LinkBox* boxes;            // [n]
  int* lists;                // [n][FH_LINK_LIST]: views of the linked
  int* nbrs;                 // [n]: how many are linked to i, exact
  unsigned long long* info;  // [4]
};

__device__ __forceinline__ bool link_finite(double x) { return fabs(x) < INFINITY; }  // (a NaN fails the comparison)

__global__ void __launch_bounds__(64) link_boxes_kernel(LinkArgs a) {
  const int lane = fhw::lane_id();
  const int k = (int)blockIdx.x;
  if (k >= a.n) return;
  const int view = fhw::uniform_i32(a.view_of ? a.view_of[k] : k);
  double lx = INFINITY, ly = INFINITY, lz = INFINITY, hx = -INFINITY, hy = -INFINITY, hz = -INFINITY;
  if (lane == 0 && view >= 0 && view < a.n_views) {
    const double* p = a.vehicles[k].state.pos;
    const double x = p[0], y = p[1], z = p[2];
    if (link_finite(x) && link_finite(y) && link_finite(z)) { lx = hx = x; ly = hy = y; lz = hz = z; }
  }
  int cell = 0;
  const int valid = cell_box_tail(a.g, lane, lx, ly, lz, hx, hy, hz, cell);
  if (lane == 0) {
    LinkBox& b = a.boxes[k];
    cell_box_store(b.c, lx, ly, lz, hx, hy, hz, valid, cell);
    b.view = valid ? view : 0; b.pad = 0;
  }
}

// Is candidate k of the walk linked to the vehicle at (px, py, pz)?  Its view comes back in kv.  (k is a boxed vehicle or -1.)
__device__ __forceinline__ bool link_test(const LinkArgs& a, int k, double px, double py, double pz, int& kv) {
#pragma clang fp contract(off)
  if (k < 0) return false;
  const LinkBox& K = a.boxes[k];
  if (!(K.c.valid & CELL_BOXED)) return false;
  kv = K.view;
  const double dx = K.c.lo[0] - px, dy = K.c.lo[1] - py, dz = K.c.lo[2] - pz;
  const double d2 = dx * dx + dy * dy + dz * dz;
  return d2 < a.r2;
}

__global__ void __launch_bounds__(64) link_narrow_kernel(LinkArgs a) {
  const int lane = fhw::lane_id();
  const int i = (int)blockIdx.x;
  if (i >= a.n) return;
  const LinkBox& B = a.boxes[i];
  int n_nbr = 0, n_up = 0;  // (uniform)
  if (fhw::uniform_i32(B.c.valid) & CELL_BOXED) {
    const double px = fhw::uniform_f64(B.c.lo[0]), py = fhw::uniform_f64(B.c.lo[1]), pz = fhw::uniform_f64(B.c.lo[2]);
    int* row = a.lists + (size_t)i * (size_t)FH_LINK_LIST;
    cell_walk(a.g, B.c, a.range, i, a.n, lane, [&](int k, const CellReach&, bool) {
      int kv = 0;
      const bool hit = link_test(a, k, px, py, pz, kv);
      const unsigned long long m_hit = __ballot(hit);
      const int slot = n_nbr + fhw::rank_in(m_hit);
      if (hit && slot < FH_LINK_LIST) row[slot] = kv;
      n_nbr += (int)__popcll(m_hit);
      n_up += (int)__popcll(__ballot(hit && k > i));
    });
  }
  if (lane == 0) {
    a.nbrs[i] = n_nbr;
    if (n_up > 0) atomicAdd(a.info + 2, (unsigned long long)n_up);
  }
}

__global__ void __launch_bounds__(256) link_init_kernel(int* __restrict__ L, int* __restrict__ H, int n_views) {
  const int v = (int)(blockIdx.x * 256 + threadIdx.x);
  if (v >= n_views) return;
  L[v] = v;
  H[v] = v;
}

__global__ void __launch_bounds__(64) link_hook_kernel(LinkArgs a, const int* __restrict__ L, int* H) {
  const int lane = fhw::lane_id();
  const int i = (int)blockIdx.x;
  if (i >= a.n) return;
  const LinkBox& B = a.boxes[i];
  if (!(fhw::uniform_i32(B.c.valid) & CELL_BOXED)) return;
  const int n_nbr = fhw::uniform_i32(a.nbrs[i]);
  const int view = fhw::uniform_i32(B.view);
  if (n_nbr <= 0 || !(view >= 0 && view < a.n_views)) return;  // (the view of a boxed vehicle was checked by link_boxes_kernel)
  int m = 0x7fffffff;
  if (n_nbr <= FH_LINK_LIST) {
    const int* row = a.lists + (size_t)i * (size_t)FH_LINK_LIST;
    if (lane < n_nbr) {
      const int kv = row[lane];
      if (kv >= 0 && kv < a.n_views) m = L[kv];
    }
  } else {  // more linked than a row holds: the cells again, with the narrow phase's test
    const double px = fhw::uniform_f64(B.c.lo[0]), py = fhw::uniform_f64(B.c.lo[1]), pz = fhw::uniform_f64(B.c.lo[2]);
    cell_walk(a.g, B.c, a.range, i, a.n, lane, [&](int k, const CellReach&, bool) {
      int kv = 0;
      if (link_test(a, k, px, py, pz, kv) && kv >= 0 && kv < a.n_views) m = min(m, L[kv]);
    });
  }
  m = fhw::wave_min_i32(m);
  if (lane == 0 && m < L[view]) atomicMin(H + view, m);
}

__global__ void __launch_bounds__(256) link_jump_kernel(const int* __restrict__ H, int* __restrict__ L, int* __restrict__ H_next, int n_views,
                                                        unsigned long long* info) {
  const int v = (int)(blockIdx.x * 256 + threadIdx.x);
  bool changed = false, root = false;
  if (v < n_views) {
    int h = H[v];
    if (!(h >= 0 && h < n_views)) h = v;  // (never: labels are views)
    int hh = H[h];
    if (!(hh >= 0 && hh < n_views)) hh = h;
    changed = L[v] != hh;
    root = hh == v;
    if (changed) L[v] = hh;
    H_next[v] = hh;
  }
  if (info) {  // (uniform: the last pass)
    const int n_changed = (int)__popcll(__ballot(changed)), n_root = (int)__popcll(__ballot(root));
    if (fhw::lane_id() == 0) {
      if (n_changed > 0) atomicAdd(info + 0, (unsigned long long)n_changed);
      if (n_root > 0) atomicAdd(info + 1, (unsigned long long)n_root);
    }
  }
}

// ---- the merge ----
// the root view v sends to, or -1 (uniform per workgroup: every lane reads the same two labels)
__device__ __forceinline__ int link_root_of(const int32_t* __restrict__ labels, int n_views, int v) {
  const int r = labels[v];
  if (!(r >= 0 && r < n_views) || r == v) return -1;
  return labels[r] == r ? r : -1;
}

// 0xFF in every byte of x that is not zero
__device__ __forceinline__ unsigned link_nonzero_bytes(unsigned x) {
  const unsigned top = (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
  return (top >> 7) * 0xFFu;
}

// dst (an aligned word wholly inside a row) loses the bytes that are zero in src; `have` is what was read of it
__device__ __forceinline__ void link_clear_word(unsigned* dst, unsigned have, unsigned src) {
  const unsigned keep = link_nonzero_bytes(src);
  if (have & ~keep) atomicAnd(dst, keep);
}

constexpr int LINK_MERGE_THREADS = 256;

__global__ void __launch_bounds__(LINK_MERGE_THREADS) link_merge_flags_kernel(const int32_t* __restrict__ labels, int n_views, unsigned char* flags,
                                                                              size_t view_stride, size_t view_bytes, int take) {
  for (int v = (int)blockIdx.y; v < n_views; v += (int)gridDim.y) {
    const int r = link_root_of(labels, n_views, v);
    if (r < 0) continue;
    unsigned char* dst = flags + (size_t)(take ? v : r) * view_stride;
    const unsigned char* src = flags + (size_t)(take ? r : v) * view_stride;
    // chunks of 16 bytes that are aligned in memory, over the bytes [0, view_bytes) of the destination row; chunk q covers the row's
    // bytes [16 q - lead, 16 q - lead + 16)
    const long long lead = (long long)(reinterpret_cast<uintptr_t>(dst) & 15u);
    const long long bytes = (long long)view_bytes;
    const long long chunks = (lead + bytes + 15) >> 4;
    for (long long q = (long long)blockIdx.x * LINK_MERGE_THREADS + threadIdx.x; q < chunks; q += (long long)gridDim.x * LINK_MERGE_THREADS) {
      const long long c0 = q * 16 - lead;
      if (c0 >= 0 && c0 + 16 <= bytes) {  // wholly inside: one load of 16 aligned bytes, one of 16 source bytes at any alignment
        const uint4 d = *reinterpret_cast<const uint4*>(dst + c0);
        uint4 s;
        __builtin_memcpy(&s, src + c0, 16);
        if (d.x == s.x && d.y == s.y && d.z == s.z && d.w == s.w) continue;
        unsigned* w = reinterpret_cast<unsigned*>(dst + c0);
        link_clear_word(w + 0, d.x, s.x);
        link_clear_word(w + 1, d.y, s.y);
        link_clear_word(w + 2, d.z, s.z);
        link_clear_word(w + 3, d.w, s.w);
        continue;
      }
      for (int j = 0; j < 4; j++) {  // a chunk at an end of the row: word by word
        const long long c = c0 + 4 * j;
        if (c >= 0 && c + 4 <= bytes) {
          unsigned s;
          __builtin_memcpy(&s, src + c, 4);
          link_clear_word(reinterpret_cast<unsigned*>(dst + c), *reinterpret_cast<const unsigned*>(dst + c), s);
        } else {
          for (long long b = c; b < c + 4; b++)  // the at most three bytes of the row in a word that other rows or the padding share
            if (b >= 0 && b < bytes && src[b] == 0 && dst[b] != 0) dst[b] = 0;
        }
      }
    }
  }
}

__global__ void __launch_bounds__(LINK_MERGE_THREADS) link_merge_mask_kernel(const int32_t* __restrict__ labels, int n_views, uint32_t* mask,
                                                                             int mask_words, int shared_words, int take) {
  for (int v = (int)blockIdx.y; v < n_views; v += (int)gridDim.y) {
    const int r = link_root_of(labels, n_views, v);
    if (r < 0) continue;
    uint32_t* dst = mask + (size_t)(take ? v : r) * (size_t)mask_words;
    const uint32_t* src = mask + (size_t)(take ? r : v) * (size_t)mask_words;
    for (int w0 = 4 * (int)(blockIdx.x * LINK_MERGE_THREADS + threadIdx.x); w0 < shared_words; w0 += 4 * (int)gridDim.x * LINK_MERGE_THREADS) {
      if (w0 + 4 <= shared_words) {
        uint4 d, s;
        __builtin_memcpy(&d, dst + w0, 16);
        __builtin_memcpy(&s, src + w0, 16);
        if (s.x & ~d.x) atomicOr(dst + w0 + 0, s.x);
        if (s.y & ~d.y) atomicOr(dst + w0 + 1, s.y);
        if (s.z & ~d.z) atomicOr(dst + w0 + 2, s.z);
        if (s.w & ~d.w) atomicOr(dst + w0 + 3, s.w);
      } else {
        for (int w = w0; w < shared_words; w++) {
          const uint32_t s = src[w];
          if (s & ~dst[w]) atomicOr(dst + w, s);
        }
      }
    }
  }
}

}  // namespace fh

// The link with a line of sight (include/fasterhip_link_los.h) comes in here, behind the last kernel of this file: its two kernels lie
// after every kernel of before in the code object of fh_capi.hip, and this header stays the last device header that fh_capi.hip names.
#include "fh_link_los.hip.hpp"

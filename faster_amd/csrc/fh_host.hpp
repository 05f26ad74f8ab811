// fh_host.hpp — what the host sides of the C ABI (fh_capi.hip, fh_map.hip, fh_pool.hip, fh_reach.hip) share: the device-scope guard,
// the owned device buffer, the HIP check, and the argument rules that more than one entry point applies.  Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/fasterhip.h"

namespace fhh {

// Makes `device` current for the duration of an entry point (a process may drive several GPUs from one thread) and restores the
// caller's device on exit.  A negative index (a context without a device) changes nothing.  ok: `device` is current.
struct DeviceScope {
  int prev = -1;
  bool switched = false, ok = false;
  explicit DeviceScope(int device) {
    if (device < 0 || hipGetDevice(&prev) != hipSuccess) return;
    if (prev != device) switched = hipSetDevice(device) == hipSuccess;
    ok = switched || prev == device;
  }
  ~DeviceScope() {
    if (switched) (void)hipSetDevice(prev);
  }
};

// A device allocation that its holder grows on demand and reuses.  (Freed by the holder's destroy function, not by a destructor: the
// holders are plain structs behind C handles, and PoolDev is copied into its vector.)
struct DeviceBuffer {
  void* ptr = nullptr;
  size_t cap = 0;
  // At least `bytes` (and 4096): nothing to do when the buffer is large enough; else a launch in flight on `stream` may still use the
  // old one, so the stream is waited for before it is freed.  The contents do not survive growing.
  hipError_t reserve(size_t bytes, hipStream_t stream) {
    if (bytes <= cap) return hipSuccess;
    hipError_t e;
    if (ptr && ((e = hipStreamSynchronize(stream)) != hipSuccess || (e = hipFree(ptr)) != hipSuccess)) return e;
    ptr = nullptr;
    cap = 0;
    const size_t want = std::max(bytes, (size_t)4096);
    if ((e = hipMalloc(&ptr, want)) == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const { return static_cast<T*>(ptr); }
};

// The HIP check of all three files: on failure `err` gets "<call>: <HIP's message>" and the statements after it run (a return).
#define FHH_HIP(call, err, ...)                                     \
  do {                                                              \
    const hipError_t e__ = (call);                                  \
    if (e__ != hipSuccess) {                                        \
      (err) = std::string(#call) + ": " + hipGetErrorString(e__);   \
      __VA_ARGS__;                                                  \
    }                                                               \
  } while (0)

// What a host-pointer solve learns from its records before they are copied (fh_solve_batch, and every shard of fh_pool_solve_*).
struct BatchScan {
  int max_seg = 1, max_faces = 8;  // the largest n_seg and row count of the well-formed records (what selects the kernel instantiation)
  int64_t face_lo = 0, face_hi = 0;  // [face_lo, face_hi): the rows of the face array that those records address
  int first_outside = -1;            // the first record whose rows lie outside [0, n_faces) (the scan stops there), -1: none
};
inline BatchScan scan_batch(const fh_problem* problems, int n, int64_t n_faces) {
  BatchScan s;
  s.face_lo = n_faces;
  for (int i = 0; i < n; i++) {
    const fh_problem& p = problems[i];
    if (p.n_seg >= 1 && p.n_seg <= FH_MAX_SEG) s.max_seg = std::max(s.max_seg, (int)p.n_seg);
    if (p.n_poly < 1 || p.n_poly > FH_MAX_POLY) continue;
    const int nf = p.face_off[p.n_poly];
    if (nf < 0 || nf > FH_MAX_FACES || p.face_begin < 0) continue;  // the kernel reports FH_ST_BAD_INPUT before it reads a row
    // the kernel cannot see n_faces: corridors that point outside the face array are refused on the host
    if ((int64_t)p.face_begin + nf > n_faces) {
      s.first_outside = i;
      break;
    }
    s.face_lo = std::min<int64_t>(s.face_lo, p.face_begin);
    s.face_hi = std::max<int64_t>(s.face_hi, (int64_t)p.face_begin + nf);
    s.max_faces = std::max(s.max_faces, nf);
  }
  if (s.face_hi < s.face_lo) s.face_lo = s.face_hi = 0;
  return s;
}

// A lattice a kernel can index: all dimensions positive and, where the entry point uses it, a positive cell size.
inline bool voxel_grid_ok(const fh_voxel_grid* g, bool with_res = true) {
  return g && (!with_res || g->res > 0) && g->dims[0] >= 1 && g->dims[1] >= 1 && g->dims[2] >= 1;
}
inline long long voxel_grid_cells(const fh_voxel_grid& g) { return (long long)g.dims[0] * g.dims[1] * g.dims[2]; }
// The cells of a lattice that passed voxel_grid_ok and whose kernels number a cell with an int; 0: more than 2^31 - 1.
// (Each factor is below 2^31; the product of two fits 62 bits, and what is above the limit after two never comes back under it.)
inline long long voxel_grid_cells31(const fh_voxel_grid& g) {
  const long long xy = (long long)g.dims[0] * g.dims[1];
  return xy > 0x7fffffffll || xy * g.dims[2] > 0x7fffffffll ? 0 : xy * g.dims[2];
}
// The lattice of the views of include/fasterhip_frontier.h and of every chooser behind it: a lattice whose cell count fits 31 bits,
// views at least that many bytes apart, at least one view.  true: fine, `cells` filled in.
inline bool view_lattice_ok(const fh_voxel_grid* grid, bool with_res, size_t view_stride, int n_views, long long* cells) {
  if (!voxel_grid_ok(grid, with_res)) return false;
  *cells = voxel_grid_cells31(*grid);
  return *cells != 0 && view_stride >= (size_t)*cells && n_views >= 1;
}

// origin, cell size and dimensions into any of the kernels' argument structs that carry a lattice as ox, oy, oz, res, nx, ny, nz
template <class To>
inline void set_lattice(To& to, const fh_voxel_grid& g) {
  to.ox = g.origin[0]; to.oy = g.origin[1]; to.oz = g.origin[2]; to.res = g.res;
  to.nx = g.dims[0]; to.ny = g.dims[1]; to.nz = g.dims[2];
}
template <class To, class From>
inline void copy_lattice(To& to, const From& from) {
  to.ox = from.ox; to.oy = from.oy; to.oz = from.oz; to.res = from.res;
  to.nx = from.nx; to.ny = from.ny; to.nz = from.nz;
}

}  // namespace fhh

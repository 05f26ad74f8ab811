// fh_plans.hip.hpp — what every fleet stage (fh_audit, fh_separation, fh_traffic, fh_check) does with a committed plan before it looks
// at anything else: is the extent of the record inside the plan array, how many instants are tested, is a position finite, the
// bounding box of positions, and the packing of two ints into one word of a record.  All force-inlined; no state.
#pragma once
#include <hip/hip_runtime.h>

namespace fh {

__device__ __forceinline__ bool plan_finite(double x) { return fabs(x) < INFINITY; }  // false for a NaN

// two ints as one word of 8 bytes of a record, `lo` at the lower address
__device__ __forceinline__ double plan_pack(int lo, int hi) { return __hiloint2double(hi, lo); }

// The BAD_PLAN rule of every stage, decided before any plan state is read.  A record that passes it indexes plans[k max_states + head
// .. + size) inside the array: every later index of a stage comes from such a record.
// (audit_kernel writes this expression out, and the six lines of plan_box_take: through the functions the compiler orders its box
// registers differently, and the kernel was not to move when these helpers were gathered: DESIGN.md, the cell grid.)
__device__ __forceinline__ bool plan_bad_extent(int head, int size, int max_states) {
  return head < 0 || size < 0 || (long long)head + (long long)size > (long long)max_states;
}

// the states of a plan below which instants are tested (count == 0: all of them), and how many instants a stride takes from m states
__device__ __forceinline__ int plan_limit(int count, int size) { return count > 0 ? min(count, size) : size; }
__device__ __forceinline__ int plan_instants(int m, int stride) { return (int)(((long long)m + stride - 1) / stride); }

// a finite position into the box (lx, ly, lz) .. (hx, hy, hz), which starts as (+inf, -inf)
__device__ __forceinline__ void plan_box_take(double x, double y, double z, double& lx, double& ly, double& lz, double& hx, double& hy,
                                              double& hz) {
  lx = x < lx ? x : lx; ly = y < ly ? y : ly; lz = z < lz ? z : lz;
  hx = x > hx ? x : hx; hy = y > hy ? y : hy; hz = z > hz ? z : hz;
}

}  // namespace fh

// wave_probe.hip — test-only device code: every primitive of faster_amd/csrc/fh_wave.hip.hpp run on one wavefront, lane by lane, and
// fhu::div (fh_udiv.hpp) on the device.  Built by faster_amd/build.py (build_wave_probe) into tests/hip/libwaveprobe.so; driven by
// tests/test_gpu_wave.py, which compares what comes back with the contracts of tests/wave_model.py.
//
// One probe per primitive, one wavefront per block (__launch_bounds__(64)): block b reads case b — a row of 64 lane values per operand,
// or one word per case where the operand is wave-uniform — and EVERY lane writes what it got, so "uniform" and "in every lane of the
// group" are checked and not only the lane a kernel happens to read.  Operands come from memory: nothing folds at compile time.
// This file names fhw:: and fhu:: functions only: no cross-lane builtin and no inline assembly of its own.
// The launchers take device pointers, the number of cases and a stream, and return the HIP error code of the launch.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../faster_amd/csrc/fh_udiv.hpp"
#include "../../faster_amd/csrc/fh_wave.hip.hpp"

namespace {

constexpr int W = 64;

__device__ __forceinline__ size_t at() { return (size_t)blockIdx.x * W + threadIdx.x; }

template <typename K, typename... A>
int launch(K kernel, int cases, hipStream_t stream, A... args) {
  if (cases <= 0) return (int)hipErrorInvalidValue;
  kernel<<<dim3((unsigned)cases), dim3(W), 0, stream>>>(args...);
  return (int)hipGetLastError();
}

}  // namespace

// row of doubles -> row of doubles
#define PROBE_F64(NAME, EXPR)                                                                                     \
  __global__ void __launch_bounds__(64) k_##NAME(const double* __restrict__ in, double* __restrict__ out) {       \
    const double v = in[at()];                                                                                    \
    out[at()] = (EXPR);                                                                                           \
  }                                                                                                               \
  extern "C" int wp_##NAME(const double* in, double* out, int cases, hipStream_t s) { return launch(k_##NAME, cases, s, in, out); }

// row of ints -> row of ints
#define PROBE_I32(NAME, EXPR)                                                                                     \
  __global__ void __launch_bounds__(64) k_##NAME(const int* __restrict__ in, int* __restrict__ out) {             \
    const int v = in[at()];                                                                                       \
    out[at()] = (int)(EXPR);                                                                                      \
  }                                                                                                               \
  extern "C" int wp_##NAME(const int* in, int* out, int cases, hipStream_t s) { return launch(k_##NAME, cases, s, in, out); }

// row of doubles and one wave-uniform int per case -> row of doubles
#define PROBE_F64_SH(NAME, EXPR)                                                                                                    \
  __global__ void __launch_bounds__(64) k_##NAME(const double* __restrict__ in, const int* __restrict__ shs, double* __restrict__ out) { \
    const double v = in[at()];                                                                                                      \
    const int sh = fhw::uniform_i32(shs[blockIdx.x]);                                                                               \
    out[at()] = (EXPR);                                                                                                             \
  }                                                                                                                                 \
  extern "C" int wp_##NAME(const double* in, const int* shs, double* out, int cases, hipStream_t s) {                               \
    return launch(k_##NAME, cases, s, in, shs, out);                                                                                \
  }

PROBE_F64(wave_sum, fhw::wave_sum(v))
PROBE_F64(half_sum, fhw::half_sum(v))
PROBE_F64(halves_sum, fhw::halves_sum(v))
PROBE_F64(wave_min, fhw::wave_min(v))
PROBE_F64(wave_max, fhw::wave_max(v))
PROBE_F64(wave_max_nonneg, fhw::wave_max_nonneg(v))
PROBE_F64(half_min, fhw::half_min(v))
PROBE_F64(half_max_nonneg, fhw::half_max_nonneg(v))
PROBE_F64(quad_max, fhw::quad_max(v))
PROBE_F64(group_max_nonneg8, fhw::group_max_nonneg<8>(v))
PROBE_F64(group_max_nonneg16, fhw::group_max_nonneg<16>(v))
PROBE_F64_SH(slices_max, fhw::slices_max(sh, v))
PROBE_F64_SH(readlane_f64, fhw::readlane_f64(v, sh & 63))

PROBE_I32(wave_sum_i32, fhw::wave_sum_i32(v))
PROBE_I32(wave_or, fhw::wave_or((unsigned)v))
PROBE_I32(wave_min_i32, fhw::wave_min_i32(v))
PROBE_I32(wave_min_i32_xor, fhw::wave_min_i32_xor(v))
PROBE_I32(rows3_sum_i32, fhw::rows3_sum_i32(v))
PROBE_I32(first_lane, fhw::first_lane(v != 0))
PROBE_I32(wave_any, fhw::wave_any(v != 0) ? 1 : 0)
PROBE_I32(lane_id, fhw::lane_id() + 0 * v)

// two rows -> two rows
__global__ void __launch_bounds__(64) k_half_sum2(const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ sa,
                                                  double* __restrict__ sb) {
  double ra, rb;
  fhw::half_sum2(a[at()], b[at()], ra, rb);
  sa[at()] = ra;
  sb[at()] = rb;
}
extern "C" int wp_half_sum2(const double* a, const double* b, double* sa, double* sb, int cases, hipStream_t s) {
  return launch(k_half_sum2, cases, s, a, b, sa, sb);
}

// the operands formed as products inside the probe: the compiler may contract the product with the first addition of the reduction
__global__ void __launch_bounds__(64) k_half_sum_prod(const double* __restrict__ x, const double* __restrict__ y, double* __restrict__ out) {
  out[at()] = fhw::half_sum(x[at()] * y[at()]);
}
extern "C" int wp_half_sum_prod(const double* x, const double* y, double* out, int cases, hipStream_t s) {
  return launch(k_half_sum_prod, cases, s, x, y, out);
}
__global__ void __launch_bounds__(64) k_half_sum2_prod(const double* __restrict__ x, const double* __restrict__ y, const double* __restrict__ z,
                                                       const double* __restrict__ w, double* __restrict__ sa, double* __restrict__ sb) {
  double ra, rb;
  fhw::half_sum2(x[at()] * y[at()], z[at()] * w[at()], ra, rb);
  sa[at()] = ra;
  sb[at()] = rb;
}
extern "C" int wp_half_sum2_prod(const double* x, const double* y, const double* z, const double* w, double* sa, double* sb, int cases,
                                 hipStream_t s) {
  return launch(k_half_sum2_prod, cases, s, x, y, z, w, sa, sb);
}

__global__ void __launch_bounds__(64) k_vminmax_f64(const double* __restrict__ a, const double* __restrict__ b, double* __restrict__ mx,
                                                    double* __restrict__ mn) {
  mx[at()] = fhw::vmax_f64(a[at()], b[at()]);
  mn[at()] = fhw::vmin_f64(a[at()], b[at()]);
}
extern "C" int wp_vminmax_f64(const double* a, const double* b, double* mx, double* mn, int cases, hipStream_t s) {
  return launch(k_vminmax_f64, cases, s, a, b, mx, mn);
}

__global__ void __launch_bounds__(64) k_quad_argmax(const double* __restrict__ v, const int* __restrict__ i, const int* __restrict__ shs,
                                                    double* __restrict__ ov, int* __restrict__ oi) {
  double rv = v[at()];
  int ri = i[at()];
  fhw::quad_argmax(fhw::uniform_i32(shs[blockIdx.x]), rv, ri);
  ov[at()] = rv;
  oi[at()] = ri;
}
extern "C" int wp_quad_argmax(const double* v, const int* i, const int* shs, double* ov, int* oi, int cases, hipStream_t s) {
  return launch(k_quad_argmax, cases, s, v, i, shs, ov, oi);
}

// src must hold lane numbers 0..63 (the caller checks): every lane is active
__global__ void __launch_bounds__(64) k_gather_f64(const double* __restrict__ v, const int* __restrict__ src, double* __restrict__ out) {
  out[at()] = fhw::gather_f64(v[at()], src[at()] & 63);
}
extern "C" int wp_gather_f64(const double* v, const int* src, double* out, int cases, hipStream_t s) {
  return launch(k_gather_f64, cases, s, v, src, out);
}
__global__ void __launch_bounds__(64) k_gather_i32(const int* __restrict__ v, const int* __restrict__ src, int* __restrict__ out) {
  out[at()] = fhw::gather_i32(v[at()], src[at()] & 63);
}
extern "C" int wp_gather_i32(const int* v, const int* src, int* out, int cases, hipStream_t s) {
  return launch(k_gather_i32, cases, s, v, src, out);
}

__global__ void __launch_bounds__(64) k_rank_in(const unsigned long long* __restrict__ masks, int* __restrict__ out) {
  out[at()] = fhw::rank_in(masks[blockIdx.x]);
}
extern "C" int wp_rank_in(const unsigned long long* masks, int* out, int cases, hipStream_t s) { return launch(k_rank_in, cases, s, masks, out); }

// lanes k..63 call the primitive, lanes below k write nothing: the value of the first ACTIVE lane, lane k
__global__ void __launch_bounds__(64) k_uniform_i32(const int* __restrict__ in, const int* __restrict__ ks, int* __restrict__ out) {
  const int v = in[at()];
  if ((int)threadIdx.x >= ks[blockIdx.x]) out[at()] = fhw::uniform_i32(v);
}
extern "C" int wp_uniform_i32(const int* in, const int* ks, int* out, int cases, hipStream_t s) {
  return launch(k_uniform_i32, cases, s, in, ks, out);
}
__global__ void __launch_bounds__(64) k_uniform_f64(const double* __restrict__ in, const int* __restrict__ ks, double* __restrict__ out) {
  const double v = in[at()];
  if ((int)threadIdx.x >= ks[blockIdx.x]) out[at()] = fhw::uniform_f64(v);
}
extern "C" int wp_uniform_f64(const double* in, const int* ks, double* out, int cases, hipStream_t s) {
  return launch(k_uniform_f64, cases, s, in, ks, out);
}

// fhu::div on the device: lane l of block b divides n[64 b + l] by d[64 b + l] with both inverses, both computed on the device
__global__ void __launch_bounds__(64) k_udiv(const int* __restrict__ n, const int* __restrict__ d, int* __restrict__ q, int* __restrict__ q_fp,
                                             unsigned* __restrict__ inv, unsigned* __restrict__ inv_fp) {
  const int nn = n[at()], dd = d[at()];
  const unsigned i0 = fhu::inverse(dd), i1 = fhu::inverse_fp(dd);
  inv[at()] = i0;
  inv_fp[at()] = i1;
  q[at()] = fhu::div(nn, dd, i0);
  q_fp[at()] = fhu::div(nn, dd, i1);
}
extern "C" int wp_udiv(const int* n, const int* d, int* q, int* q_fp, unsigned* inv, unsigned* inv_fp, int cases, hipStream_t s) {
  return launch(k_udiv, cases, s, n, d, q, q_fp, inv, inv_fp);
}

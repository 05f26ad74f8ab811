// fh_wave.hip.hpp — the wave64 vocabulary of the device code (gfx950): lane numbers, wave-uniform values, reductions over the 64
// lanes of a wavefront.  The one place where the cross-lane builtins are spelled out (tests/test_wave_primitives_home.py); every
// other device header names what it uses with `using fhw::...`.
// Includes nothing of the project: fh_path.hip.hpp is compiled into fh_map.hip without the fh headers.  Sets no file-level pragma
// and tests no macro: what is included after it is compiled as if this header were not there.
#pragma once
#include <hip/hip_runtime.h>

namespace fhw {

__device__ __forceinline__ int lane_id() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
// how many lanes below this one have their bit set in m (the slot of a lane in a ballot compaction)
__device__ __forceinline__ int rank_in(unsigned long long m) {
  return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}
__device__ __forceinline__ int first_lane(bool pred) {  // lowest lane with pred, -1 if none (uniform)
  unsigned long long m = __ballot(pred);
  return m ? (int)__builtin_ctzll(m) : -1;
}
__device__ __forceinline__ bool wave_any(bool pred) { return __ballot(pred) != 0ull; }

// the value of the first active lane, in scalar registers (v_readfirstlane): sizes, positions and loop conditions read by all lanes
__device__ __forceinline__ int uniform_i32(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ double uniform_f64(double v) {
  int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
  int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ double readlane_f64(double v, int lane) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_readlane(lo, lane);
  hi = __builtin_amdgcn_readlane(hi, lane);
  return __hiloint2double(hi, lo);
}

// Wave64 reductions on the DPP network (row_shr 1/2/4/8 inside each 16-lane row, then row_bcast:15 / row_bcast:31
// across rows; the total lands in lane 63) instead of ds_bpermute round trips through the LDS crossbar.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_f64(double identity, double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(__double2loint(identity), lo, CTRL, ROW_MASK, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(__double2hiint(identity), hi, CTRL, ROW_MASK, 0xf, false);
  return __hiloint2double(hi, lo);
}
// Zero-filling variant (bound_ctrl, every row written): no `old` operand to initialise.  Rows 0 and 2 pick up partial sums
// they do not need in the row_bcast steps; only lane 63 is read, and it sees the values of before each step.
template <int CTRL>
__device__ __forceinline__ double dpp0_f64(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xf, 0xf, true);
  hi = __builtin_amdgcn_update_dpp(0, hi, CTRL, 0xf, 0xf, true);
  return __hiloint2double(hi, lo);
}
template <int CTRL>
__device__ __forceinline__ int dpp0_i32(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }
// v_max_f64 / v_min_f64 without the canonicalising self-max the fmax/fmin lowering adds (no NaNs reach the reductions)
__device__ __forceinline__ double vmax_f64(double a, double b) {
  double r;
  asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ double vmin_f64(double a, double b) {
  double r;
  asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// lanes l and l+32 exchange a double and add: both halves end up with the same sum (v_permlane32_swap, gfx950)
__device__ __forceinline__ double halves_sum(double v) {
  const unsigned lo = (unsigned)__double2loint(v), hi = (unsigned)__double2hiint(v);
  const auto a = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
  const auto b = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
  return __hiloint2double((int)b[0], (int)a[0]) + __hiloint2double((int)b[1], (int)a[1]);
}
// The summation tree is pairwise summation in lane order (`while (n > 1) v = v[0::2] + v[1::2]`): after row_shr 1/2/4/8 lane 15 of a
// row holds the balanced tree of its 16 lanes, row_bcast:15 makes lanes 31 and 63 r1 + r0 and r3 + r2, row_bcast:31 makes lane 63
// (r3 + r2) + (r1 + r0).  The device returns these bits in every lane (tests/test_gpu_wave.py), depth 6: |error| <= 6 u sum |v|.
__device__ __forceinline__ double wave_sum(double v) {
  v += dpp0_f64<0x111>(v); v += dpp0_f64<0x112>(v); v += dpp0_f64<0x114>(v); v += dpp0_f64<0x118>(v);  // inside each row of 16 lanes
  v += dpp0_f64<0x142>(v); v += dpp0_f64<0x143>(v);  // across the rows
  return readlane_f64(v, 63);
}
__device__ __forceinline__ int wave_sum_i32(int v) {
  v += dpp0_i32<0x111>(v); v += dpp0_i32<0x112>(v); v += dpp0_i32<0x114>(v); v += dpp0_i32<0x118>(v);  // inside each row of 16 lanes
  v += dpp0_i32<0x142>(v); v += dpp0_i32<0x143>(v);  // across the rows
  return __builtin_amdgcn_readlane(v, 63);
}
__device__ __forceinline__ unsigned wave_or(unsigned v) {
  v |= (unsigned)dpp0_i32<0x111>((int)v); v |= (unsigned)dpp0_i32<0x112>((int)v);  // inside each row of 16 lanes: row_shr 1, 2,
  v |= (unsigned)dpp0_i32<0x114>((int)v); v |= (unsigned)dpp0_i32<0x118>((int)v);  // 4, 8
  v |= (unsigned)dpp0_i32<0x142>((int)v); v |= (unsigned)dpp0_i32<0x143>((int)v);  // across the rows
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
// The maximum over the lanes, for callers that only ask whether it is positive and where it sits: positive iff some lane is positive,
// and the maximum itself when that is >= +0.  NOT max(0, ...): the zero fill goes to lanes without a source, and lane 63 and the lanes
// it depends on all have one, so all-negative input returns the negative maximum (measured, tests/test_gpu_wave.py; half_max_nonneg
// likewise).  No NaN.
__device__ __forceinline__ double wave_max_nonneg(double v) {
  v = vmax_f64(v, dpp0_f64<0x111>(v)); v = vmax_f64(v, dpp0_f64<0x112>(v));  // inside each row of 16 lanes: row_shr 1, 2,
  v = vmax_f64(v, dpp0_f64<0x114>(v)); v = vmax_f64(v, dpp0_f64<0x118>(v));  // 4, 8
  v = vmax_f64(v, dpp0_f64<0x142>(v)); v = vmax_f64(v, dpp0_f64<0x143>(v));  // across the rows
  return readlane_f64(v, 63);
}
__device__ __forceinline__ double wave_min(double v) {
  v = vmin_f64(v, dpp_f64<0x111, 0xf>(INFINITY, v)); v = vmin_f64(v, dpp_f64<0x112, 0xf>(INFINITY, v));  // inside each row of 16 lanes: row_shr 1, 2,
  v = vmin_f64(v, dpp_f64<0x114, 0xf>(INFINITY, v)); v = vmin_f64(v, dpp_f64<0x118, 0xf>(INFINITY, v));  // 4, 8
  v = vmin_f64(v, dpp_f64<0x142, 0xa>(INFINITY, v)); v = vmin_f64(v, dpp_f64<0x143, 0xc>(INFINITY, v));  // across the rows
  return readlane_f64(v, 63);
}
// max over the wavefront, any sign (identity -INFINITY).  fmax, not vmax_f64: its callers have not been shown to be free of NaNs.
__device__ __forceinline__ double wave_max(double v) {
  v = fmax(v, dpp_f64<0x111, 0xf>(-INFINITY, v)); v = fmax(v, dpp_f64<0x112, 0xf>(-INFINITY, v));  // inside each row of 16 lanes: row_shr 1, 2,
  v = fmax(v, dpp_f64<0x114, 0xf>(-INFINITY, v)); v = fmax(v, dpp_f64<0x118, 0xf>(-INFINITY, v));  // 4, 8
  v = fmax(v, dpp_f64<0x142, 0xa>(-INFINITY, v)); v = fmax(v, dpp_f64<0x143, 0xc>(-INFINITY, v));  // across the rows
  return readlane_f64(v, 63);
}
// Reductions over lanes 0..31 only, five stages: row_shr 1/2/4/8, row_bcast:15, the result in lane 31.  Where lanes 32..63 hold the
// identity (+0, INFINITY) they return the bits of the six-stage forms above: lane 63 of wave_sum is (r3 + r2) + (r1 + r0) over the
// four row totals, (0 + 0) + (r1 + r0) = r1 + r0 when no summand is -0; a maximum or minimum with its identity is the other operand
// (+0 is the identity of half_max_nonneg only while lanes 0..31 hold a value >= +0: see wave_max_nonneg).  half_sum is pairwise
// summation in lane order over lanes 0..31, depth 5.  What lanes 32..63 hold is not read (NaN there changes nothing).
__device__ __forceinline__ double half_sum(double v) {
  v += dpp0_f64<0x111>(v); v += dpp0_f64<0x112>(v); v += dpp0_f64<0x114>(v); v += dpp0_f64<0x118>(v);  // inside each row of 16 lanes
  v += dpp0_f64<0x142>(v);  // row 0 into row 1
  return readlane_f64(v, 31);
}
__device__ __forceinline__ double half_max_nonneg(double v) {
  v = vmax_f64(v, dpp0_f64<0x111>(v)); v = vmax_f64(v, dpp0_f64<0x112>(v));  // inside each row of 16 lanes: row_shr 1, 2,
  v = vmax_f64(v, dpp0_f64<0x114>(v)); v = vmax_f64(v, dpp0_f64<0x118>(v));  // 4, 8
  v = vmax_f64(v, dpp0_f64<0x142>(v));  // row 0 into row 1
  return readlane_f64(v, 31);
}
__device__ __forceinline__ double half_min(double v) {
  v = vmin_f64(v, dpp_f64<0x111, 0xf>(INFINITY, v)); v = vmin_f64(v, dpp_f64<0x112, 0xf>(INFINITY, v));  // inside each row of 16 lanes: row_shr 1, 2,
  v = vmin_f64(v, dpp_f64<0x114, 0xf>(INFINITY, v)); v = vmin_f64(v, dpp_f64<0x118, 0xf>(INFINITY, v));  // 4, 8
  v = vmin_f64(v, dpp_f64<0x142, 0xa>(INFINITY, v));  // row 0 into row 1
  return readlane_f64(v, 31);
}
// Two sums over lanes 0..31 in one pass: lanes 0..31 of b move to lanes 32..63 (v_permlane32_swap, gfx950), the five stages run once,
// and the totals are read from lanes 31 and 63 (row_bcast:15 adds row 2 into row 3 the way it adds row 0 into row 1): sa and sb have
// the bits of half_sum(a) and half_sum(b).  What a and b hold in lanes 32..63 is not read.
__device__ __forceinline__ void half_sum2(double a, double b, double& sa, double& sb) {
  // The first stage runs on a and b themselves, as in half_sum: where a is a product, the compiler contracts it with this addition
  // (fma) as it does there, and the bits are those of the single sums.  A row_shr stays inside its row, so it commutes with the move.
  a += dpp0_f64<0x111>(a);
  b += dpp0_f64<0x111>(b);
  const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)__double2loint(a), (unsigned)__double2loint(b), false, false);
  const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)__double2hiint(a), (unsigned)__double2hiint(b), false, false);
  double v = __hiloint2double((int)hi[0], (int)lo[0]);  // lanes 0..31: a, lanes 32..63: b of the lane 32 below
  v += dpp0_f64<0x112>(v); v += dpp0_f64<0x114>(v); v += dpp0_f64<0x118>(v);  // inside each row of 16 lanes
  v += dpp0_f64<0x142>(v);  // row 0 into row 1, row 2 into row 3
  sa = readlane_f64(v, 31);
  sb = readlane_f64(v, 63);
}
// The sum of an int over lanes 0..47: the four stages inside the rows, then the three row totals added as scalars.
__device__ __forceinline__ int rows3_sum_i32(int v) {
  v += dpp0_i32<0x111>(v); v += dpp0_i32<0x112>(v); v += dpp0_i32<0x114>(v); v += dpp0_i32<0x118>(v);  // inside each row of 16 lanes
  return __builtin_amdgcn_readlane(v, 15) + __builtin_amdgcn_readlane(v, 31) + __builtin_amdgcn_readlane(v, 47);
}
// max over each aligned group of four lanes, the result in all four of them (quad_perm [1,0,3,2], then [2,3,0,1]).  Written as the
// comparison `o > v ? o : v`, not fmax: with no NaN among the inputs there is none in the result.  All 64 lanes must be active.
__device__ __forceinline__ double quad_max(double v) {
  double o = dpp0_f64<0xB1>(v);
  v = o > v ? o : v;
  o = dpp0_f64<0x4E>(v);
  return o > v ? o : v;
}
// max over each aligned group of 8 or 16 lanes of values that are >= +0 and no NaN, the result in every lane of the group: the two
// quad_perm steps of quad_max, then row_half_mirror (the other quad of the eight) and row_mirror (the other eight of the row).
// All 64 lanes must be active.
template <int GROUP>
__device__ __forceinline__ double group_max_nonneg(double v) {
  static_assert(GROUP == 8 || GROUP == 16, "an aligned group inside a row of 16 lanes");
  v = vmax_f64(v, dpp0_f64<0xB1>(v));
  v = vmax_f64(v, dpp0_f64<0x4E>(v));
  v = vmax_f64(v, dpp0_f64<0x141>(v));
  if constexpr (GROUP == 16) v = vmax_f64(v, dpp0_f64<0x140>(v));
  return v;
}
// every lane reads v of the lane it names (ds_bpermute_b32: the LDS crossbar, no LDS memory); src in 0..63, that lane active
__device__ __forceinline__ double gather_f64(double v, int src) {
  const int lo = __builtin_amdgcn_ds_bpermute(src << 2, __double2loint(v));
  const int hi = __builtin_amdgcn_ds_bpermute(src << 2, __double2hiint(v));
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ int gather_i32(int v, int src) { return __builtin_amdgcn_ds_bpermute(src << 2, v); }
// One step of an arg-max over pairs (v, i): the lane takes the pair of the lane CTRL names when that one is larger in the order
// "greater v first, among equal v the smaller i as an unsigned number" (so i = -1, no candidate, loses against every index).  A total
// order: both lanes of an exchange keep the same pair.  No NaN among the v.  All 64 lanes must be active.
template <int CTRL>
__device__ __forceinline__ void argmax_step(double& v, int& i) {
  const double ov = dpp0_f64<CTRL>(v);
  const int oi = dpp0_i32<CTRL>(i);
  const bool take = ov > v || (ov == v && (unsigned)oi < (unsigned)i);
  v = take ? ov : v;
  i = take ? oi : i;
}
// arg-max over each aligned group of 1 << sh lanes, sh in {0, 1, 2} (wave-uniform), the winning pair in every lane of the group:
// the quad_perm steps of quad_max
__device__ __forceinline__ void quad_argmax(int sh, double& v, int& i) {
  if (sh >= 1) argmax_step<0xB1>(v, i);
  if (sh >= 2) argmax_step<0x4E>(v, i);
}
// max over each aligned group of 1 << sh lanes, sh in {0, 1, 2} (wave-uniform), the result in every lane of the group: the quad_perm
// steps of quad_max on v_max_f64.  Any sign and -INFINITY, no NaN.  All 64 lanes must be active.
__device__ __forceinline__ double slices_max(int sh, double v) {
  if (sh >= 1) v = vmax_f64(v, dpp0_f64<0xB1>(v));
  if (sh >= 2) v = vmax_f64(v, dpp0_f64<0x4E>(v));
  return v;
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_min_step(int v) {
  const int o = __builtin_amdgcn_update_dpp(0x7fffffff, v, CTRL, ROW_MASK, 0xf, false);
  return o < v ? o : v;
}
__device__ __forceinline__ int wave_min_i32(int v) {
  v = dpp_min_step<0x111, 0xf>(v); v = dpp_min_step<0x112, 0xf>(v);  // inside each row of 16 lanes: row_shr 1, 2,
  v = dpp_min_step<0x114, 0xf>(v); v = dpp_min_step<0x118, 0xf>(v);  // 4, 8
  v = dpp_min_step<0x142, 0xa>(v); v = dpp_min_step<0x143, 0xc>(v);  // across the rows
  return __builtin_amdgcn_readlane(v, 63);
}
// The same minimum as a __shfl_xor butterfly, the result in every lane.  Pinned by solve_kernel<.., PAIRS = true, ..>, which inlines
// choose_r_index: with the DPP form its twelve instantiations no longer have the instruction bytes they had.
__device__ __forceinline__ int wave_min_i32_xor(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
  return v;
}

}  // namespace fhw

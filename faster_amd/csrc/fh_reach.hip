// fh_reach.hip — host side of the ten frontier choosers behind fh_map_frontier_goals_device, K15 … K24: one entry point for each of
// include/fasterhip_{reach,spread,gain,team,sight,bid,far,apart,prospect,stake}.h, its kernels in the device header of the same
// chooser.  What two entry points share is written once above `extern "C"`: the clause groups, the argument fills, the device of
// d_records and the one layout of each workspace; the lattice rule and the device scope are fh_host.hpp's.  An entry point keeps
// its own clauses in its header's order, its static_asserts and its launches.
// A translation unit of its own: fh_map.hip and fh_capi.hip, their kernels and their code objects are what they were.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>

#include "../../include/fasterhip.h"
#include "../../include/fasterhip_reach.h"
#include "../../include/fasterhip_spread.h"
#include "../../include/fasterhip_gain.h"
#include "../../include/fasterhip_team.h"
#include "../../include/fasterhip_sight.h"
#include "../../include/fasterhip_bid.h"
#include "../../include/fasterhip_far.h"
#include "../../include/fasterhip_apart.h"
#include "../../include/fasterhip_prospect.h"
#include "../../include/fasterhip_stake.h"
#include "fh_reach.hip.hpp"
#include "fh_spread.hip.hpp"
#include "fh_gain.hip.hpp"
#include "fh_team.hip.hpp"
#include "fh_sight.hip.hpp"
#include "fh_bid.hip.hpp"
#include "fh_far.hip.hpp"
#include "fh_host.hpp"
#include "fh_prospect.hpp"
#include "fh_stake.hpp"
#include "fh_apart.hpp"

// ---- clauses: what more than one entry point tests, each group once; an entry point calls them in its header's order ----

// the clauses of fh_reach_goals_device from r_max to max_hops < 0, in the header's order (the fields that every params struct has;
// fh_far_params and the three behind it have no r_max: any r_max that passes stands in for it)
template <class P>
static int reach_field_clauses(double r_max, const P& par) {
  if (!std::isfinite(r_max) || !(r_max > 0.0)) return FH_ERR_ARG;
  if (!std::isfinite(par.r_avoid) || !(par.r_avoid >= 0.0)) return FH_ERR_ARG;
  if (std::isnan(par.z_lo) || std::isnan(par.z_hi) || par.z_lo > par.z_hi) return FH_ERR_ARG;
  const int all_wants = FH_FRONTIER_WANT_REACHED | FH_FRONTIER_WANT_NO_PATH | FH_FRONTIER_WANT_ALL;
  if (par.want == 0 || (par.want & ~all_wants) != 0) return FH_ERR_ARG;
  if (par.max_hops < 0) return FH_ERR_ARG;
  return FH_OK;
}

// and its clauses from map_grid to n < 0 (fh_gain_goals_device and the far choosers have clauses of their own between the two)
static int reach_table_clauses(const fh_voxel_grid* map_grid, const unsigned* d_map_bits, const fh_voxel_grid* grid, size_t view_stride, int n_views,
                               int n) {
  if (!fhh::voxel_grid_ok(map_grid) || fhh::voxel_grid_cells31(*map_grid) == 0) return FH_ERR_ARG;
  if (!d_map_bits) return FH_ERR_ARG;
  long long cells = 0;
  if (!fhh::view_lattice_ok(grid, true, view_stride, n_views, &cells)) return FH_ERR_ARG;
  if (n < 0) return FH_ERR_ARG;
  return FH_OK;
}

// both, with nothing between them (K15, K16, K18, K20)
template <class P>
static int reach_clauses(const P& par, const fh_voxel_grid* map_grid, const unsigned* d_map_bits, const fh_voxel_grid* grid, size_t view_stride,
                         int n_views, int n) {
  if (reach_field_clauses(par.r_max, par) != FH_OK) return FH_ERR_ARG;
  return reach_table_clauses(map_grid, d_map_bits, grid, view_stride, n_views, n);
}

// r_spread and passes against the chooser's cap (K16, K18, K20, K22, K24)
static bool spread_pair_ok(double r_spread, int passes, int max_passes) {
  return std::isfinite(r_spread) && r_spread > 0.0 && passes >= 1 && passes <= max_passes;
}

// gain_radius (the far choosers: gain_blocks), hop_cost and min_gain against the chooser's two caps (K17 … K20, K23, K24)
static bool gain_triple_ok(int radius, int hop_cost, int min_gain, int max_radius, int max_hop_cost) {
  return radius >= 0 && radius <= max_radius && hop_cost >= 0 && hop_cost <= max_hop_cost && min_gain >= 0;
}

// the edge of a block of the far choosers, in voxels
static bool block_ok(int block) { return block >= 1 && block <= 16; }

// the pointers every chooser reads or writes once n > 0 (a workspace is the entry point's own clause: its place differs)
static bool pointers_ok(const void* d_flags, const void* d_vehicles, const void* d_goals, const void* d_mask, const void* d_records) {
  return d_flags && d_vehicles && d_goals && d_mask && d_records;
}

// The device that `p` lies on, -1: the runtime does not know it as device memory (HIP's error is cleared).  An entry point opens
// its fhh::DeviceScope on the answer for d_records, which refuses -1: the scope is the entry's own object and lives until it returns.
static int device_of(const void* p) {
  hipPointerAttribute_t where;
  if (hipPointerGetAttributes(&where, p) == hipSuccess && where.type == hipMemoryTypeDevice) return where.device;
  (void)hipGetLastError();
  return -1;
}

// ---- workspaces: one layout each, read by the size function and by the carve ----

// K16's, K18's and K20's: the class bytes, rounded up to a multiple of 64, before the rows (K20's offers: bid_offers_offset below)
static size_t spread_rows_offset(int n) { return ((size_t)n + 63) & ~(size_t)63; }

// the words of a bitmap of blocks of edge `block` over the lattice; 0: a null grid, a dimension < 1 or a block outside 1..16;
// FH_FAR_MAX_WORDS + 1: more than FH_FAR_MAX_WORDS (each partial product is tested, so nothing overflows)
static int far_words(const fh_voxel_grid* grid, int block) {
  if (!fhh::voxel_grid_ok(grid, false) || !block_ok(block)) return 0;
  long long w = (((long long)grid->dims[0] + block - 1) / block + 63) / 64;
  for (int k = 1; k < 3; k++) {
    if (w > FH_FAR_MAX_WORDS) return FH_FAR_MAX_WORDS + 1;
    w *= ((long long)grid->dims[k] + block - 1) / block;
  }
  return w > FH_FAR_MAX_WORDS ? FH_FAR_MAX_WORDS + 1 : (int)w;
}

// The far choosers' (K21 … K24), in bytes from d_work: K21's sums [n_views][4][W] at 0, its need bytes (n_views, rounded up to a
// multiple of 64: `counts - need` is what the memset clears), K23's counts [n_views][64 W] of 16 bits where the chooser has a gain
// (K23, K24), and for a team (K22, K24; n = 0 for the other two) the class bytes (n, rounded up to a multiple of 64), the groups and
// `lower`, n int32 each.  A part that a chooser does not have is empty, so `end` is what its header's formula states.  (The
// offsets through `grp` are multiples of 32, `lower` is one of 4.)
struct FarLayout {
  size_t need, counts, cls, grp, lower, end;
};
static FarLayout far_layout(int W, int n_views, bool with_counts, int n) {
  FarLayout at;
  at.need = (size_t)n_views * 4u * (size_t)W * sizeof(unsigned long long);
  at.counts = at.need + (((size_t)n_views + 63) & ~(size_t)63);
  at.cls = at.counts + (with_counts ? (size_t)n_views * 64u * (size_t)W * sizeof(uint16_t) : 0);
  at.grp = at.cls + spread_rows_offset(n);
  at.lower = at.grp + (size_t)n * sizeof(int32_t);
  at.end = at.lower + (size_t)n * sizeof(int32_t);
  return at;
}
// what the four size functions answer: `end`, or 0 for a null grid, a dimension < 1, a block outside 1..16, too many words,
// n_views < 1 or n < 0
static size_t far_bytes(const fh_voxel_grid* grid, int block, int n_views, bool with_counts, int n) {
  const int W = far_words(grid, block);
  if (W < 1 || W > FH_FAR_MAX_WORDS || n_views < 1 || n < 0) return 0;
  return far_layout(W, n_views, with_counts, n).end;
}

// ---- argument fills from checked values; what a fill leaves out (a record pointer of the chooser's own type, a pass counter that
// the launch loop advances) is the entry point's to set ----

// K15's kernel arguments, the head of every chooser's (r_max: see reach_field_clauses; d_records: null wherever the chooser has
// a longer record of its own)
template <class P>
static void reach_args(fhp::ReachArgs& a, double r_max, const P& par, const fh_voxel_grid* map_grid, const unsigned* d_map_bits,
                       const fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of, int n_views,
                       const fh_vehicle* d_vehicles, double* d_goals, int32_t* d_mask, fh_reach_record* d_records) {
  a.r_max = r_max;
  a.r2 = r_max * r_max;
  a.a2 = par.r_avoid * par.r_avoid;
  a.z_lo = par.z_lo; a.z_hi = par.z_hi;
  a.want = par.want;
  a.max_hops = par.max_hops;
  fhh::set_lattice(a, *grid);
  a.flags = d_flags; a.view_stride = view_stride; a.view_of = d_view_of; a.n_views = n_views;
  a.vehicles = d_vehicles;
  a.mx = map_grid->dims[0]; a.my = map_grid->dims[1]; a.mz = map_grid->dims[2];
  a.mres = map_grid->res; a.mox = map_grid->origin[0]; a.moy = map_grid->origin[1]; a.moz = map_grid->origin[2];
  a.bits = d_map_bits;
  a.goals = d_goals; a.mask = d_mask; a.records = d_records;
}

// K17's on top of them (K17 … K20): the gain radius and its square, hop_cost, min_gain
template <class P>
static void gain_args(fhp::GainArgs& s, const P& par, const fh_voxel_grid* map_grid, const unsigned* d_map_bits, const fh_voxel_grid* grid,
                      const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of, int n_views, const fh_vehicle* d_vehicles,
                      double* d_goals, int32_t* d_mask) {
  reach_args(s.r, par.r_max, par, map_grid, d_map_bits, grid, d_flags, view_stride, d_view_of, n_views, d_vehicles, d_goals, d_mask, nullptr);
  s.g = par.gain_radius;
  s.g2 = par.gain_radius * par.gain_radius;
  s.hop_cost = par.hop_cost;
  s.min_gain = par.min_gain;
  s.records = nullptr;
}

// K18's on top of those, for fhp::TeamArgs and fhp::BidArgs alike (K20's params and arguments are K18's under its own names, as
// its static_asserts state): the radii, the claim radius, the labels, and the class bytes and rows of the workspace
template <class A, class P>
static void team_args(A& s, const P& par, const fh_voxel_grid* map_grid, const unsigned* d_map_bits, const fh_voxel_grid* grid,
                      const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of, int n_views, const int32_t* d_group,
                      const fh_vehicle* d_vehicles, int n, void* d_work, double* d_goals, int32_t* d_mask) {
  gain_args(s.gn, par, map_grid, d_map_bits, grid, d_flags, view_stride, d_view_of, n_views, d_vehicles, d_goals, d_mask);
  // the interaction radius: a peer beyond it cannot touch the ball of a candidate
  const double r_int = par.claim_radius < 0 ? par.r_spread : std::fmax(par.r_spread, (double)(par.gain_radius + par.claim_radius + 1) * grid->res);
  const double reach = (par.r_max + par.r_max) + r_int, near = par.r_max + r_int;
  s.s2 = par.r_spread * par.r_spread;
  s.reach2 = reach * reach;
  s.near2 = near * near;
  s.n = n; s.pass = 0;
  s.cr = par.claim_radius;
  s.cr2 = par.claim_radius * par.claim_radius;
  s.group = d_group;
  s.cls = static_cast<unsigned char*>(d_work);
  s.rows = reinterpret_cast<int32_t*>(static_cast<unsigned char*>(d_work) + spread_rows_offset(n));
}

// what the class kernel of fh_spread.hip.hpp gets from K18 and K20 as it is: it reads the vehicles and writes the class bytes
template <class A>
static void spread_class_args(fhp::SpreadArgs& c, const A& s, void* d_work) {
  c.r = s.gn.r;
  c.s2 = s.s2; c.reach2 = s.reach2; c.near2 = s.near2;
  c.n = s.n; c.pass = 0;
  c.group = s.group;
  c.cls = static_cast<unsigned char*>(d_work);
  c.rows = s.rows;
  c.records = nullptr;
}

// K21's, the head of every far chooser's: reach_args without an r_max, the blocks, the skip list, the sums and the need bytes
template <class P>
static void far_args(fhp::FarArgs& s, const P& par, const fh_voxel_grid* map_grid, const unsigned* d_map_bits, const fh_voxel_grid* grid,
                     const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of, int n_views, const int32_t* d_skip,
                     const fh_vehicle* d_vehicles, int n, void* d_work, int W, const FarLayout& at, double* d_goals, int32_t* d_mask) {
  reach_args(s.r, 1.0, par, map_grid, d_map_bits, grid, d_flags, view_stride, d_view_of, n_views, d_vehicles, d_goals, d_mask, nullptr);
  s.B = par.block;
  s.cx = (grid->dims[0] + s.B - 1) / s.B;  // (W <= FH_FAR_MAX_WORDS: the dims are far below 2^31 - 16)
  s.cy = (grid->dims[1] + s.B - 1) / s.B;
  s.cz = (grid->dims[2] + s.B - 1) / s.B;
  s.wx = (s.cx + 63) / 64;
  s.W = W;
  s.n = n;
  s.skip = d_skip;
  s.sums = static_cast<unsigned long long*>(d_work);
  s.need = static_cast<unsigned char*>(d_work) + at.need;
  s.records = nullptr;
}

// K23's on top of them (K23, K24): the gain in blocks, hop_cost, min_gain and the counts
template <class P>
static void prospect_args(fhp::ProspectArgs& x, const P& par, void* d_work, const FarLayout& at, fh_prospect_record* d_records) {
  x.g = par.gain_blocks;
  x.hop_cost = par.hop_cost;
  x.min_gain = par.min_gain;
  x.counts = reinterpret_cast<uint16_t*>(static_cast<unsigned char*>(d_work) + at.counts);
  x.records = d_records;
}

// K22's on top of K21's (K22's own arguments, and what its class kernel reads and writes for K24): r_spread squared, the passes,
// the labels and the three tables of a team
template <class P>
static void far_spread_args(fhp::FarSpreadArgs& x, const P& par, const int32_t* d_group, void* d_work, const FarLayout& at,
                            fh_apart_record* d_records) {
  unsigned char* const work = static_cast<unsigned char*>(d_work);
  x.s2 = par.r_spread * par.r_spread;
  x.pass = 0; x.passes = par.passes;
  x.group = d_group;
  x.cls = work + at.cls;
  x.grp = reinterpret_cast<int32_t*>(work + at.grp);
  x.lower = reinterpret_cast<int32_t*>(work + at.lower);
  x.records = d_records;
}

extern "C" {

int fh_reach_goals_device(void* stream, const fh_reach_params* par, const fh_voxel_grid* map_grid, const unsigned* d_map_bits,
                          const fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of, int n_views,
                          const fh_vehicle* d_vehicles, int n, double* d_goals, int32_t* d_mask, fh_reach_record* d_records) {
  if (!par) return FH_ERR_ARG;
  if (reach_clauses(*par, map_grid, d_map_bits, grid, view_stride, n_views, n) != FH_OK) return FH_ERR_ARG;
  if (n == 0) return FH_OK;
  if (!pointers_ok(d_flags, d_vehicles, d_goals, d_mask, d_records)) return FH_ERR_ARG;
  fhh::DeviceScope scope(device_of(d_records));
  if (!scope.ok) return FH_ERR_DEVICE;
  fhp::ReachArgs a;
  reach_args(a, par->r_max, *par, map_grid, d_map_bits, grid, d_flags, view_stride, d_view_of, n_views, d_vehicles, d_goals, d_mask, d_records);
  hipLaunchKernelGGL(fhp::reach_goals_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? FH_OK : FH_ERR_DEVICE;
}

size_t fh_spread_work_bytes(int n) { return n <= 0 ? 0 : spread_rows_offset(n) + (size_t)n * FH_SPREAD_LIST * sizeof(int32_t); }

int fh_spread_goals_device(void* stream, const fh_spread_params* par, const fh_voxel_grid* map_grid, const unsigned* d_map_bits,
                           const fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of, int n_views,
                           const int32_t* d_group, const fh_vehicle* d_vehicles, int n, void* d_work, size_t work_bytes, double* d_goals,
                           int32_t* d_mask, fh_spread_record* d_records) {
  if (!par) return FH_ERR_ARG;
  if (reach_clauses(*par, map_grid, d_map_bits, grid, view_stride, n_views, n) != FH_OK) return FH_ERR_ARG;
  if (!spread_pair_ok(par->r_spread, par->passes, FH_SPREAD_MAX_PASSES)) return FH_ERR_ARG;
  if (n == 0) return FH_OK;
  if (!pointers_ok(d_flags, d_vehicles, d_goals, d_mask, d_records)) return FH_ERR_ARG;
  if (!d_work) return FH_ERR_ARG;
  if (work_bytes < fh_spread_work_bytes(n)) return FH_ERR_ARG;
  fhh::DeviceScope scope(device_of(d_records));
  if (!scope.ok) return FH_ERR_DEVICE;
  fhp::SpreadArgs s;
  reach_args(s.r, par->r_max, *par, map_grid, d_map_bits, grid, d_flags, view_stride, d_view_of, n_views, d_vehicles, d_goals, d_mask, nullptr);
  const double reach = (par->r_max + par->r_max) + par->r_spread, near = par->r_max + par->r_spread;
  s.s2 = par->r_spread * par->r_spread;
  s.reach2 = reach * reach;
  s.near2 = near * near;
  s.n = n; s.pass = 0;
  s.group = d_group;
  s.cls = static_cast<unsigned char*>(d_work);
  s.rows = reinterpret_cast<int32_t*>(static_cast<unsigned char*>(d_work) + spread_rows_offset(n));
  s.records = d_records;
  const hipStream_t q = (hipStream_t)stream;
  hipLaunchKernelGGL(fhp::spread_class_kernel, dim3(((unsigned)n + 255u) / 256u), dim3(256), 0, q, s);
  hipLaunchKernelGGL(fhp::spread_peers_kernel, dim3((unsigned)n), dim3(64), 0, q, s);
  for (int p = 1; p <= par->passes; p++) {
    s.pass = p;
    hipLaunchKernelGGL(fhp::spread_goals_kernel, dim3((unsigned)n), dim3(256), 0, q, s);
  }
  return hipGetLastError() == hipSuccess ? FH_OK : FH_ERR_DEVICE;
}

int fh_gain_goals_device(void* stream, const fh_gain_params* par, const fh_voxel_grid* map_grid, const unsigned* d_map_bits,
                         const fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of, int n_views,
                         const fh_vehicle* d_vehicles, int n, double* d_goals, int32_t* d_mask, fh_gain_record* d_records) {
  if (!par) return FH_ERR_ARG;
  if (reach_field_clauses(par->r_max, *par) != FH_OK) return FH_ERR_ARG;
  if (!gain_triple_ok(par->gain_radius, par->hop_cost, par->min_gain, FH_GAIN_MAX_RADIUS, FH_GAIN_MAX_HOP_COST)) return FH_ERR_ARG;
  if (reach_table_clauses(map_grid, d_map_bits, grid, view_stride, n_views, n) != FH_OK) return FH_ERR_ARG;
  if (n == 0) return FH_OK;
  if (!pointers_ok(d_flags, d_vehicles, d_goals, d_mask, d_records)) return FH_ERR_ARG;
  fhh::DeviceScope scope(device_of(d_records));
  if (!scope.ok) return FH_ERR_DEVICE;
  fhp::GainArgs s;
  gain_args(s, *par, map_grid, d_map_bits, grid, d_flags, view_stride, d_view_of, n_views, d_vehicles, d_goals, d_mask);
  s.records = d_records;
  hipLaunchKernelGGL(fhp::gain_goals_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, s);
  return hipGetLastError() == hipSuccess ? FH_OK : FH_ERR_DEVICE;
}

size_t fh_far_work_bytes(const fh_voxel_grid* grid, int block, int n_views) { return far_bytes(grid, block, n_views, false, 0); }

int fh_far_goals_device(void* stream, const fh_far_params* par, const fh_voxel_grid* map_grid, const unsigned* d_map_bits,
                        const fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of, int n_views,
                        const int32_t* d_skip, const fh_vehicle* d_vehicles, int n, void* d_work, size_t work_bytes, double* d_goals,
                        int32_t* d_mask, fh_far_record* d_records) {
  static_assert(sizeof(fh_far_params) == 64 && sizeof(fh_far_record) == 64 && FH_FAR_MAX_WORDS % 256 == 0, "include/fasterhip_far.h");
  if (!par) return FH_ERR_ARG;
  if (reach_field_clauses(1.0, *par) != FH_OK) return FH_ERR_ARG;
  if (!block_ok(par->block)) return FH_ERR_ARG;
  if (reach_table_clauses(map_grid, d_map_bits, grid, view_stride, n_views, n) != FH_OK) return FH_ERR_ARG;
  const int W = far_words(grid, par->block);  // (>= 1 after the clauses above, so `at.end` below is what the size function answers)
  if (W > FH_FAR_MAX_WORDS) return FH_ERR_ARG;
  const FarLayout at = far_layout(W, n_views, false, 0);
  if (work_bytes < at.end) return FH_ERR_ARG;
  if (n == 0) return FH_OK;
  if (!d_work || !pointers_ok(d_flags, d_vehicles, d_goals, d_mask, d_records)) return FH_ERR_ARG;
  fhh::DeviceScope scope(device_of(d_records));
  if (!scope.ok) return FH_ERR_DEVICE;
  fhp::FarArgs s;
  far_args(s, *par, map_grid, d_map_bits, grid, d_flags, view_stride, d_view_of, n_views, d_skip, d_vehicles, n, d_work, W, at, d_goals, d_mask);
  s.records = d_records;
  const hipStream_t q = (hipStream_t)stream;
  if (hipMemsetAsync(s.need, 0, at.counts - at.need, q) != hipSuccess) {
    (void)hipGetLastError();
    return FH_ERR_DEVICE;
  }
  hipLaunchKernelGGL(fhp::far_need_kernel, dim3(((unsigned)n + 255u) / 256u), dim3(256), 0, q, s);
  hipLaunchKernelGGL(fhp::far_blocks_kernel, dim3((unsigned)W, (unsigned)(n_views < 65535 ? n_views : 65535)), dim3(256), 0, q, s);
  hipLaunchKernelGGL(fhp::far_goals_kernel, dim3((unsigned)n), dim3(256), 0, q, s);
  return hipGetLastError() == hipSuccess ? FH_OK : FH_ERR_DEVICE;
}

// the offers (two words a vehicle) and the two buffers of decided words, after the rows of FH_BID_LIST
static size_t bid_offers_offset(int n) { return spread_rows_offset(n) + (size_t)n * FH_BID_LIST * sizeof(int32_t); }

size_t fh_bid_work_bytes(int n) { return n <= 0 ? 0 : bid_offers_offset(n) + (size_t)n * 2 * sizeof(int32_t) + (size_t)n * 2 * sizeof(int32_t); }

size_t fh_apart_work_bytes(const fh_voxel_grid* grid, int block, int n_views, int n) { return far_bytes(grid, block, n_views, false, n); }

size_t fh_prospect_work_bytes(const fh_voxel_grid* grid, int block, int n_views) { return far_bytes(grid, block, n_views, true, 0); }

size_t fh_stake_work_bytes(const fh_voxel_grid* grid, int block, int n_views, int n) { return far_bytes(grid, block, n_views, true, n); }

// (K23's clauses through min_gain, K21's tables, then K22's two and claim_blocks; K21's memset and need kernel, K23's one pass for the
// bitmaps and the counts and K22's class kernel as they stand, then this chooser's count kernel and its pass kernel once per pass)
int fh_stake_goals_device(void* stream, const fh_stake_params* par, const fh_voxel_grid* map_grid, const unsigned* d_map_bits,
                          const fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of, int n_views,
                          const int32_t* d_skip, const int32_t* d_group, const fh_vehicle* d_vehicles, int n, void* d_work, size_t work_bytes,
                          double* d_goals, int32_t* d_mask, fh_stake_record* d_records) {
  static_assert(sizeof(fh_stake_params) == sizeof(fh_apart_params) && sizeof(fh_stake_record) == 128 && sizeof(fh_apart_record) == 96 &&
                    sizeof(fh_prospect_record) == 80 && FH_STAKE_SKIPPED == FH_FAR_SKIPPED && FH_STAKE_MAX_WORDS == FH_FAR_MAX_WORDS &&
                    FH_STAKE_UNSETTLED == FH_APART_UNSETTLED && FH_STAKE_CLAIMED == FH_APART_CLAIMED && FH_STAKE_ALL_POOR == FH_PROSPECT_ALL_POOR &&
                    FH_STAKE_MAX_PASSES == FH_APART_MAX_PASSES && FH_STAKE_DEFAULT_PASSES == FH_APART_DEFAULT_PASSES &&
                    FH_STAKE_MAX_BLOCKS == FH_PROSPECT_MAX_BLOCKS && FH_STAKE_MAX_HOP_COST == FH_PROSPECT_MAX_HOP_COST &&
                    FH_STAKE_MAX_CLAIM_BLOCKS == 5 &&
                    offsetof(fh_stake_params, r_avoid) == offsetof(fh_apart_params, r_avoid) && offsetof(fh_stake_params, z_lo) == offsetof(fh_apart_params, z_lo) &&
                    offsetof(fh_stake_params, z_hi) == offsetof(fh_apart_params, z_hi) &&
                    offsetof(fh_stake_params, reserved_d) == offsetof(fh_apart_params, reserved_d) &&
                    offsetof(fh_stake_params, want) == offsetof(fh_apart_params, want) && offsetof(fh_stake_params, max_hops) == offsetof(fh_apart_params, max_hops) &&
                    offsetof(fh_stake_params, block) == offsetof(fh_apart_params, block) &&
                    offsetof(fh_stake_params, gain_blocks) == offsetof(fh_prospect_params, gain_blocks) &&
                    offsetof(fh_stake_params, hop_cost) == offsetof(fh_prospect_params, hop_cost) &&
                    offsetof(fh_stake_params, min_gain) == offsetof(fh_prospect_params, min_gain) &&
                    offsetof(fh_stake_params, reserved) == offsetof(fh_prospect_params, reserved) &&
                    offsetof(fh_stake_params, r_spread) == offsetof(fh_apart_params, r_spread) && offsetof(fh_stake_params, r_spread) == 64 &&
                    offsetof(fh_stake_params, passes) == offsetof(fh_apart_params, passes) && offsetof(fh_stake_params, passes) == 72 &&
                    offsetof(fh_stake_params, claim_blocks) == offsetof(fh_apart_params, reserved_tail) && offsetof(fh_stake_params, claim_blocks) == 76 &&
                    offsetof(fh_stake_record, flags) == offsetof(fh_apart_record, flags) && offsetof(fh_stake_record, view) == offsetof(fh_apart_record, view) &&
                    offsetof(fh_stake_record, cell) == offsetof(fh_apart_record, cell) &&
                    offsetof(fh_stake_record, block_cell) == offsetof(fh_apart_record, block_cell) &&
                    offsetof(fh_stake_record, hops) == offsetof(fh_apart_record, hops) && offsetof(fh_stake_record, targets) == offsetof(fh_apart_record, targets) &&
                    offsetof(fh_stake_record, reachable) == offsetof(fh_apart_record, reachable) &&
                    offsetof(fh_stake_record, reached) == offsetof(fh_apart_record, reached) && offsetof(fh_stake_record, levels) == offsetof(fh_apart_record, levels) &&
                    offsetof(fh_stake_record, members) == offsetof(fh_apart_record, members) &&
                    offsetof(fh_stake_record, reserved) == offsetof(fh_apart_record, reserved) && offsetof(fh_stake_record, d2) == offsetof(fh_apart_record, d2) &&
                    offsetof(fh_stake_record, block_d2) == offsetof(fh_apart_record, block_d2) &&
                    offsetof(fh_stake_record, group) == offsetof(fh_apart_record, group) &&
                    offsetof(fh_stake_record, decided_pass) == offsetof(fh_apart_record, decided_pass) &&
                    offsetof(fh_stake_record, lower) == offsetof(fh_apart_record, lower) &&
                    offsetof(fh_stake_record, standing) == offsetof(fh_apart_record, standing) &&
                    offsetof(fh_stake_record, claims) == offsetof(fh_apart_record, claims) &&
                    offsetof(fh_stake_record, claimed) == offsetof(fh_apart_record, claimed) &&
                    offsetof(fh_stake_record, reserved_tail) == offsetof(fh_apart_record, reserved_tail) &&
                    offsetof(fh_stake_record, gain) == 96 && offsetof(fh_stake_record, gain) - 96 == offsetof(fh_prospect_record, gain) - 64 &&
                    offsetof(fh_stake_record, utility) - 96 == offsetof(fh_prospect_record, utility) - 64 &&
                    offsetof(fh_stake_record, poor) - 96 == offsetof(fh_prospect_record, poor) - 64 &&
                    offsetof(fh_stake_record, best_gain) - 96 == offsetof(fh_prospect_record, best_gain) - 64 &&
                    offsetof(fh_stake_record, covered) == 112 && offsetof(fh_stake_record, removed) == 116,
                "include/fasterhip_stake.h: K21's, K22's and K23's params, records, flags and limits under its own names");
  if (!par) return FH_ERR_ARG;
  if (reach_field_clauses(1.0, *par) != FH_OK) return FH_ERR_ARG;
  if (!block_ok(par->block)) return FH_ERR_ARG;
  if (!gain_triple_ok(par->gain_blocks, par->hop_cost, par->min_gain, FH_STAKE_MAX_BLOCKS, FH_STAKE_MAX_HOP_COST)) return FH_ERR_ARG;
  if (reach_table_clauses(map_grid, d_map_bits, grid, view_stride, n_views, n) != FH_OK) return FH_ERR_ARG;
  const int W = far_words(grid, par->block);
  if (W > FH_STAKE_MAX_WORDS) return FH_ERR_ARG;
  if (!spread_pair_ok(par->r_spread, par->passes, FH_STAKE_MAX_PASSES)) return FH_ERR_ARG;
  if (par->claim_blocks < 0 || par->claim_blocks > FH_STAKE_MAX_CLAIM_BLOCKS) return FH_ERR_ARG;
  const FarLayout at = far_layout(W, n_views, true, n);
  if (work_bytes < at.end) return FH_ERR_ARG;
  if (n == 0) return FH_OK;
  if (!d_work || !pointers_ok(d_flags, d_vehicles, d_goals, d_mask, d_records)) return FH_ERR_ARG;
  fhh::DeviceScope scope(device_of(d_records));
  if (!scope.ok) return FH_ERR_DEVICE;
  fhp::StakeArgs k;
  fhp::ProspectArgs& x = k.p;
  fhp::FarArgs& s = x.f;
  far_args(s, *par, map_grid, d_map_bits, grid, d_flags, view_stride, d_view_of, n_views, d_skip, d_vehicles, n, d_work, W, at, d_goals, d_mask);
  prospect_args(x, *par, d_work, at, nullptr);
  fhp::FarSpreadArgs c;  // what K22's class kernel reads: the judge's values, the labels and the two tables it writes
  c.f = s;
  far_spread_args(c, *par, d_group, d_work, at, nullptr);
  k.s2 = c.s2;
  k.pass = 0; k.passes = par->passes;
  k.k = par->claim_blocks;
  k.cls = c.cls; k.grp = c.grp; k.lower = c.lower;
  k.records = d_records;
  const hipStream_t q = (hipStream_t)stream;
  if (hipMemsetAsync(s.need, 0, at.counts - at.need, q) != hipSuccess) {
    (void)hipGetLastError();
    return FH_ERR_DEVICE;
  }
  hipLaunchKernelGGL(fhp::far_need_kernel, dim3(((unsigned)n + 255u) / 256u), dim3(256), 0, q, s);
  hipLaunchKernelGGL(fhp::prospect_blocks_kernel, dim3((unsigned)W, (unsigned)(n_views < 65535 ? n_views : 65535)), dim3(256), 0, q, x);
  hipLaunchKernelGGL(fhp::far_spread_class_kernel, dim3(((unsigned)n + 255u) / 256u), dim3(256), 0, q, c);
  hipLaunchKernelGGL(fhp::stake_count_kernel, dim3((unsigned)n), dim3(64), 0, q, k);
  for (int p = 1; p <= par->passes; p++) {
    k.pass = p;
    hipLaunchKernelGGL(fhp::stake_goals_kernel, dim3((unsigned)n), dim3(256), 0, q, k);
  }
  return hipGetLastError() == hipSuccess ? FH_OK : FH_ERR_DEVICE;
}

// (K21's clauses in K21's order, the three new fields right behind `block`; K21's memset and need kernel as they stand above, then
// one pass over the needed views for the four bitmaps and the counts, then a workgroup per vehicle)
int fh_prospect_goals_device(void* stream, const fh_prospect_params* par, const fh_voxel_grid* map_grid, const unsigned* d_map_bits,
                             const fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of, int n_views,
                             const int32_t* d_skip, const fh_vehicle* d_vehicles, int n, void* d_work, size_t work_bytes, double* d_goals,
                             int32_t* d_mask, fh_prospect_record* d_records) {
  static_assert(sizeof(fh_prospect_params) == sizeof(fh_far_params) && sizeof(fh_prospect_record) == 80 && sizeof(fh_far_record) == 64 &&
                    FH_PROSPECT_SKIPPED == FH_FAR_SKIPPED && FH_PROSPECT_MAX_WORDS == FH_FAR_MAX_WORDS &&
                    offsetof(fh_prospect_params, r_avoid) == offsetof(fh_far_params, r_avoid) && offsetof(fh_prospect_params, z_lo) == offsetof(fh_far_params, z_lo) &&
                    offsetof(fh_prospect_params, z_hi) == offsetof(fh_far_params, z_hi) &&
                    offsetof(fh_prospect_params, reserved_d) == offsetof(fh_far_params, reserved_d) &&
                    offsetof(fh_prospect_params, want) == offsetof(fh_far_params, want) && offsetof(fh_prospect_params, max_hops) == offsetof(fh_far_params, max_hops) &&
                    offsetof(fh_prospect_params, block) == offsetof(fh_far_params, block) &&
                    offsetof(fh_prospect_params, gain_blocks) == offsetof(fh_far_params, reserved) &&
                    offsetof(fh_prospect_params, reserved) == offsetof(fh_far_params, reserved) + 3 * sizeof(int32_t) &&
                    offsetof(fh_prospect_record, flags) == offsetof(fh_far_record, flags) && offsetof(fh_prospect_record, view) == offsetof(fh_far_record, view) &&
                    offsetof(fh_prospect_record, cell) == offsetof(fh_far_record, cell) &&
                    offsetof(fh_prospect_record, block_cell) == offsetof(fh_far_record, block_cell) &&
                    offsetof(fh_prospect_record, hops) == offsetof(fh_far_record, hops) && offsetof(fh_prospect_record, targets) == offsetof(fh_far_record, targets) &&
                    offsetof(fh_prospect_record, reachable) == offsetof(fh_far_record, reachable) &&
                    offsetof(fh_prospect_record, reached) == offsetof(fh_far_record, reached) && offsetof(fh_prospect_record, levels) == offsetof(fh_far_record, levels) &&
                    offsetof(fh_prospect_record, members) == offsetof(fh_far_record, members) &&
                    offsetof(fh_prospect_record, reserved) == offsetof(fh_far_record, reserved) && offsetof(fh_prospect_record, d2) == offsetof(fh_far_record, d2) &&
                    offsetof(fh_prospect_record, block_d2) == offsetof(fh_far_record, block_d2) && offsetof(fh_prospect_record, gain) == 64 &&
                    (FH_PROSPECT_ALL_POOR & (FH_APART_UNSETTLED | FH_APART_CLAIMED | FH_FAR_SKIPPED)) == 0,
                "include/fasterhip_prospect.h: K21's params, record, skip flag and word cap under its own names");
  if (!par) return FH_ERR_ARG;
  if (reach_field_clauses(1.0, *par) != FH_OK) return FH_ERR_ARG;
  if (!block_ok(par->block)) return FH_ERR_ARG;
  if (!gain_triple_ok(par->gain_blocks, par->hop_cost, par->min_gain, FH_PROSPECT_MAX_BLOCKS, FH_PROSPECT_MAX_HOP_COST)) return FH_ERR_ARG;
  if (reach_table_clauses(map_grid, d_map_bits, grid, view_stride, n_views, n) != FH_OK) return FH_ERR_ARG;
  const int W = far_words(grid, par->block);
  if (W > FH_PROSPECT_MAX_WORDS) return FH_ERR_ARG;
  const FarLayout at = far_layout(W, n_views, true, 0);
  if (work_bytes < at.end) return FH_ERR_ARG;
  if (n == 0) return FH_OK;
  if (!d_work || !pointers_ok(d_flags, d_vehicles, d_goals, d_mask, d_records)) return FH_ERR_ARG;
  fhh::DeviceScope scope(device_of(d_records));
  if (!scope.ok) return FH_ERR_DEVICE;
  fhp::ProspectArgs x;
  fhp::FarArgs& s = x.f;
  far_args(s, *par, map_grid, d_map_bits, grid, d_flags, view_stride, d_view_of, n_views, d_skip, d_vehicles, n, d_work, W, at, d_goals, d_mask);
  prospect_args(x, *par, d_work, at, d_records);
  const hipStream_t q = (hipStream_t)stream;
  if (hipMemsetAsync(s.need, 0, at.counts - at.need, q) != hipSuccess) {
    (void)hipGetLastError();
    return FH_ERR_DEVICE;
  }
  hipLaunchKernelGGL(fhp::far_need_kernel, dim3(((unsigned)n + 255u) / 256u), dim3(256), 0, q, s);
  hipLaunchKernelGGL(fhp::prospect_blocks_kernel, dim3((unsigned)W, (unsigned)(n_views < 65535 ? n_views : 65535)), dim3(256), 0, q, x);
  hipLaunchKernelGGL(fhp::prospect_goals_kernel, dim3((unsigned)n), dim3(256), 0, q, x);
  return hipGetLastError() == hipSuccess ? FH_OK : FH_ERR_DEVICE;
}

// (behind K21's entry point and the bid chooser's workspace: K21's clauses in K21's order, then K16's two; the summary stage is K21's
// three calls as they stand above)
int fh_apart_goals_device(void* stream, const fh_apart_params* par, const fh_voxel_grid* map_grid, const unsigned* d_map_bits,
                               const fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of, int n_views,
                               const int32_t* d_skip, const int32_t* d_group, const fh_vehicle* d_vehicles, int n, void* d_work,
                               size_t work_bytes, double* d_goals, int32_t* d_mask, fh_apart_record* d_records) {
  static_assert(sizeof(fh_apart_params) == 96 && sizeof(fh_apart_record) == 96 && offsetof(fh_apart_params, r_spread) == 64 &&
                    offsetof(fh_apart_params, block) == offsetof(fh_far_params, block) &&
                    offsetof(fh_apart_record, d2) == offsetof(fh_far_record, d2) &&
                    offsetof(fh_apart_record, block_d2) == offsetof(fh_far_record, block_d2) && offsetof(fh_apart_record, group) == 64 &&
                    FH_APART_UNSETTLED == FH_SPREAD_UNSETTLED && FH_APART_CLAIMED == FH_SPREAD_CLAIMED &&
                    FH_APART_MAX_PASSES == FH_SPREAD_MAX_PASSES && FH_APART_DEFAULT_PASSES == FH_SPREAD_DEFAULT_PASSES &&
                    FH_APART_SKIPPED == FH_FAR_SKIPPED && FH_APART_MAX_WORDS == FH_FAR_MAX_WORDS &&
                    offsetof(fh_apart_params, want) == offsetof(fh_far_params, want) && offsetof(fh_apart_params, max_hops) == offsetof(fh_far_params, max_hops) &&
                    offsetof(fh_apart_record, members) == offsetof(fh_far_record, members) && offsetof(fh_apart_record, hops) == offsetof(fh_far_record, hops),
                "include/fasterhip_apart.h: K21's params and record, K16's flags and pass limits under its own names");
  if (!par) return FH_ERR_ARG;
  if (reach_field_clauses(1.0, *par) != FH_OK) return FH_ERR_ARG;
  if (!block_ok(par->block)) return FH_ERR_ARG;
  if (reach_table_clauses(map_grid, d_map_bits, grid, view_stride, n_views, n) != FH_OK) return FH_ERR_ARG;
  const int W = far_words(grid, par->block);
  if (W > FH_FAR_MAX_WORDS) return FH_ERR_ARG;
  if (!spread_pair_ok(par->r_spread, par->passes, FH_APART_MAX_PASSES)) return FH_ERR_ARG;
  const FarLayout at = far_layout(W, n_views, false, n);
  if (work_bytes < at.end) return FH_ERR_ARG;
  if (n == 0) return FH_OK;
  if (!d_work || !pointers_ok(d_flags, d_vehicles, d_goals, d_mask, d_records)) return FH_ERR_ARG;
  fhh::DeviceScope scope(device_of(d_records));
  if (!scope.ok) return FH_ERR_DEVICE;
  fhp::FarSpreadArgs x;
  fhp::FarArgs& s = x.f;
  far_args(s, *par, map_grid, d_map_bits, grid, d_flags, view_stride, d_view_of, n_views, d_skip, d_vehicles, n, d_work, W, at, d_goals, d_mask);
  far_spread_args(x, *par, d_group, d_work, at, d_records);
  const hipStream_t q = (hipStream_t)stream;
  if (hipMemsetAsync(s.need, 0, at.counts - at.need, q) != hipSuccess) {
    (void)hipGetLastError();
    return FH_ERR_DEVICE;
  }
  hipLaunchKernelGGL(fhp::far_need_kernel, dim3(((unsigned)n + 255u) / 256u), dim3(256), 0, q, s);
  hipLaunchKernelGGL(fhp::far_blocks_kernel, dim3((unsigned)W, (unsigned)(n_views < 65535 ? n_views : 65535)), dim3(256), 0, q, s);
  hipLaunchKernelGGL(fhp::far_spread_class_kernel, dim3(((unsigned)n + 255u) / 256u), dim3(256), 0, q, x);
  hipLaunchKernelGGL(fhp::far_spread_count_kernel, dim3((unsigned)n), dim3(64), 0, q, x);
  for (int p = 1; p <= par->passes; p++) {
    x.pass = p;
    hipLaunchKernelGGL(fhp::far_spread_goals_kernel, dim3((unsigned)n), dim3(256), 0, q, x);
  }
  return hipGetLastError() == hipSuccess ? FH_OK : FH_ERR_DEVICE;
}

// (K18's clauses in K18's order; it stands before fh_sight_goals_device, and fh_team_goals_device still ends this file)
int fh_bid_goals_device(void* stream, const fh_bid_params* par, const fh_voxel_grid* map_grid, const unsigned* d_map_bits,
                        const fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of, int n_views,
                        const int32_t* d_group, const fh_vehicle* d_vehicles, int n, void* d_work, size_t work_bytes, double* d_goals,
                        int32_t* d_mask, fh_bid_record* d_records) {
  static_assert(FH_BID_OVERFLOW == FH_TEAM_OVERFLOW && FH_BID_UNSETTLED == FH_TEAM_UNSETTLED && FH_BID_CLAIMED == FH_TEAM_CLAIMED &&
                    FH_BID_ALL_POOR == FH_TEAM_ALL_POOR && FH_BID_MAX_PASSES == FH_TEAM_MAX_PASSES && FH_BID_DEFAULT_PASSES == FH_TEAM_DEFAULT_PASSES &&
                    FH_BID_MAX_RADIUS == FH_TEAM_MAX_RADIUS && FH_BID_MAX_HOP_COST == FH_TEAM_MAX_HOP_COST && FH_BID_LIST == 2 * FH_TEAM_LIST,
                "the constants that include/fasterhip_bid.h shares with K18");
  static_assert(sizeof(fh_bid_params) == sizeof(fh_team_params) && offsetof(fh_bid_params, r_spread) == offsetof(fh_team_params, r_spread) &&
                    offsetof(fh_bid_params, passes) == offsetof(fh_team_params, passes) &&
                    offsetof(fh_bid_params, gain_radius) == offsetof(fh_team_params, gain_radius) &&
                    offsetof(fh_bid_params, hop_cost) == offsetof(fh_team_params, hop_cost) &&
                    offsetof(fh_bid_params, min_gain) == offsetof(fh_team_params, min_gain) &&
                    offsetof(fh_bid_params, claim_radius) == offsetof(fh_team_params, claim_radius),
                "include/fasterhip_bid.h: K18's params");
  static_assert(sizeof(fh_bid_record) == sizeof(fh_team_record) && offsetof(fh_bid_record, d2) == offsetof(fh_team_record, d2) &&
                    offsetof(fh_bid_record, decided_pass) == offsetof(fh_team_record, decided_pass) &&
                    offsetof(fh_bid_record, rivals) == offsetof(fh_team_record, lower) && offsetof(fh_bid_record, claims) == offsetof(fh_team_record, claims) &&
                    offsetof(fh_bid_record, searches) == offsetof(fh_team_record, reserved0) && offsetof(fh_bid_record, gain) == offsetof(fh_team_record, gain) &&
                    offsetof(fh_bid_record, covered) == offsetof(fh_team_record, covered),
                "include/fasterhip_bid.h: K18's record, `lower` read as `rivals` and `reserved0` as `searches`");
  if (!par) return FH_ERR_ARG;
  if (reach_clauses(*par, map_grid, d_map_bits, grid, view_stride, n_views, n) != FH_OK) return FH_ERR_ARG;
  if (!spread_pair_ok(par->r_spread, par->passes, FH_BID_MAX_PASSES)) return FH_ERR_ARG;
  if (!gain_triple_ok(par->gain_radius, par->hop_cost, par->min_gain, FH_BID_MAX_RADIUS, FH_BID_MAX_HOP_COST)) return FH_ERR_ARG;
  if (par->claim_radius < -1 || par->claim_radius > FH_BID_MAX_RADIUS) return FH_ERR_ARG;
  if (n == 0) return FH_OK;
  if (!pointers_ok(d_flags, d_vehicles, d_goals, d_mask, d_records)) return FH_ERR_ARG;
  if (!d_work) return FH_ERR_ARG;
  if (work_bytes < fh_bid_work_bytes(n)) return FH_ERR_ARG;
  fhh::DeviceScope scope(device_of(d_records));
  if (!scope.ok) return FH_ERR_DEVICE;
  fhp::BidArgs s;
  team_args(s, *par, map_grid, d_map_bits, grid, d_flags, view_stride, d_view_of, n_views, d_group, d_vehicles, n, d_work, d_goals, d_mask);
  s.last = 0;
  s.offers = reinterpret_cast<int32_t*>(static_cast<unsigned char*>(d_work) + bid_offers_offset(n));
  s.decided = s.offers + 2 * (size_t)n;
  s.records = d_records;
  fhp::SpreadArgs c;
  spread_class_args(c, s, d_work);
  const hipStream_t q = (hipStream_t)stream;
  hipLaunchKernelGGL(fhp::spread_class_kernel, dim3(((unsigned)n + 255u) / 256u), dim3(256), 0, q, c);
  hipLaunchKernelGGL(fhp::bid_peers_kernel, dim3((unsigned)n), dim3(64), 0, q, s);
  for (int p = 1; p <= par->passes; p++) {
    s.pass = p;
    s.last = p == par->passes ? 1 : 0;
    hipLaunchKernelGGL(fhp::bid_goals_kernel, dim3((unsigned)n), dim3(256), 0, q, s);
    hipLaunchKernelGGL(fhp::bid_settle_kernel, dim3((unsigned)n), dim3(64), 0, q, s);
  }
  return hipGetLastError() == hipSuccess ? FH_OK : FH_ERR_DEVICE;
}

// (before fh_team_goals_device, whose three launches end this file)
int fh_sight_goals_device(void* stream, const fh_sight_params* par, const fh_voxel_grid* map_grid, const unsigned* d_map_bits,
                          const fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of, int n_views,
                          const fh_vehicle* d_vehicles, int n, double* d_goals, int32_t* d_mask, fh_sight_record* d_records) {
  static_assert(FH_SIGHT_MAX_RADIUS == FH_GAIN_MAX_RADIUS && FH_SIGHT_MAX_HOP_COST == FH_GAIN_MAX_HOP_COST && FH_SIGHT_ALL_POOR == FH_GAIN_ALL_POOR,
                "the constants that include/fasterhip_sight.h shares with K17");
  static_assert(sizeof(fh_sight_params) == sizeof(fh_gain_params) && offsetof(fh_sight_params, min_gain) == offsetof(fh_gain_params, min_gain) &&
                    sizeof(fh_sight_record) == sizeof(fh_gain_record) && offsetof(fh_sight_record, best_gain) == offsetof(fh_gain_record, best_gain) &&
                    offsetof(fh_sight_record, ball_gain) == 56 && offsetof(fh_sight_record, walls) == 60,
                "include/fasterhip_sight.h: K17's params, and K17's record through best_gain");
  if (!par) return FH_ERR_ARG;
  if (reach_field_clauses(par->r_max, *par) != FH_OK) return FH_ERR_ARG;
  if (!gain_triple_ok(par->gain_radius, par->hop_cost, par->min_gain, FH_SIGHT_MAX_RADIUS, FH_SIGHT_MAX_HOP_COST)) return FH_ERR_ARG;
  if (reach_table_clauses(map_grid, d_map_bits, grid, view_stride, n_views, n) != FH_OK) return FH_ERR_ARG;
  if (n == 0) return FH_OK;
  if (!pointers_ok(d_flags, d_vehicles, d_goals, d_mask, d_records)) return FH_ERR_ARG;
  fhh::DeviceScope scope(device_of(d_records));
  if (!scope.ok) return FH_ERR_DEVICE;
  fhp::SightArgs s;
  gain_args(s.gn, *par, map_grid, d_map_bits, grid, d_flags, view_stride, d_view_of, n_views, d_vehicles, d_goals, d_mask);
  s.records = d_records;
  hipLaunchKernelGGL(fhp::sight_goals_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, s);
  return hipGetLastError() == hipSuccess ? FH_OK : FH_ERR_DEVICE;
}

int fh_team_goals_device(void* stream, const fh_team_params* par, const fh_voxel_grid* map_grid, const unsigned* d_map_bits,
                         const fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of, int n_views,
                         const int32_t* d_group, const fh_vehicle* d_vehicles, int n, void* d_work, size_t work_bytes, double* d_goals,
                         int32_t* d_mask, fh_team_record* d_records) {
  static_assert(FH_TEAM_MAX_RADIUS == FH_GAIN_MAX_RADIUS && FH_TEAM_MAX_HOP_COST == FH_GAIN_MAX_HOP_COST, "include/fasterhip_team.h");
  if (!par) return FH_ERR_ARG;
  if (reach_clauses(*par, map_grid, d_map_bits, grid, view_stride, n_views, n) != FH_OK) return FH_ERR_ARG;
  if (!spread_pair_ok(par->r_spread, par->passes, FH_TEAM_MAX_PASSES)) return FH_ERR_ARG;
  if (!gain_triple_ok(par->gain_radius, par->hop_cost, par->min_gain, FH_TEAM_MAX_RADIUS, FH_TEAM_MAX_HOP_COST)) return FH_ERR_ARG;
  if (par->claim_radius < -1 || par->claim_radius > FH_TEAM_MAX_RADIUS) return FH_ERR_ARG;
  if (n == 0) return FH_OK;
  if (!pointers_ok(d_flags, d_vehicles, d_goals, d_mask, d_records)) return FH_ERR_ARG;
  if (!d_work) return FH_ERR_ARG;
  if (work_bytes < fh_spread_work_bytes(n)) return FH_ERR_ARG;
  fhh::DeviceScope scope(device_of(d_records));
  if (!scope.ok) return FH_ERR_DEVICE;
  fhp::TeamArgs s;
  team_args(s, *par, map_grid, d_map_bits, grid, d_flags, view_stride, d_view_of, n_views, d_group, d_vehicles, n, d_work, d_goals, d_mask);
  s.records = d_records;
  fhp::SpreadArgs c;
  spread_class_args(c, s, d_work);
  const hipStream_t q = (hipStream_t)stream;
  hipLaunchKernelGGL(fhp::spread_class_kernel, dim3(((unsigned)n + 255u) / 256u), dim3(256), 0, q, c);
  hipLaunchKernelGGL(fhp::team_peers_kernel, dim3((unsigned)n), dim3(64), 0, q, s);
  for (int p = 1; p <= par->passes; p++) {
    s.pass = p;
    hipLaunchKernelGGL(fhp::team_goals_kernel, dim3((unsigned)n), dim3(256), 0, q, s);
  }
  return hipGetLastError() == hipSuccess ? FH_OK : FH_ERR_DEVICE;
}

}  // extern "C"

// fh_reach.hip — host side of include/fasterhip_reach.h (fh_reach_goals_device): the frontier voxel that a flood of the space a vehicle
// knows to be free reaches in the fewest steps (kernel: fh_reach.hip.hpp), and of include/fasterhip_spread.h (fh_spread_goals_device):
// that chooser for a team, goals claimed by peers avoided (kernels: fh_spread.hip.hpp), and of include/fasterhip_gain.h
// (fh_gain_goals_device): the reachable frontier voxel with the most unknown space around it for its steps (kernel: fh_gain.hip.hpp),
// and of include/fasterhip_team.h (fh_team_goals_device): that utility inside the passes of the chooser for a team, the space a peer's
// claim covers not counted twice (kernels: fh_team.hip.hpp), and of include/fasterhip_sight.h (fh_sight_goals_device): the gain chooser
// with a gain that counts only the unknown voxels a candidate has a line of sight to (kernel: fh_sight.hip.hpp), and of
// include/fasterhip_bid.h (fh_bid_goals_device): the search of the gain-aware chooser for a team inside rounds ordered by bids, the best
// offer wins a contested frontier (kernels: fh_bid.hip.hpp), and of include/fasterhip_far.h (fh_far_goals_device): the fallback for the
// vehicles those choosers left without a goal, a flood of the whole view over blocks of voxels (kernels: fh_far.hip.hpp), and of
// include/fasterhip_apart.h (fh_apart_goals_device): that fallback for a team, the target blocks that a peer's claim covers
// taken out before the flood (kernels: fh_apart.hpp), and of include/fasterhip_prospect.h (fh_prospect_goals_device): that fallback
// with a gain, the unknown voxels of the blocks around a target block, chosen by utility over all levels (kernels: fh_prospect.hpp), and
// of include/fasterhip_stake.h (fh_stake_goals_device): that gain inside the passes of the fallback for a team, a peer's claim covering
// a cube of blocks whose unknown voxels no gain of the vehicle counts (kernels: fh_stake.hpp).
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

// the lattice of the views, judged as fh_map_frontier_goals_device judges it (0: fine, cells filled in)
static int reach_lattice(const fh_voxel_grid* grid, size_t view_stride, int n_views, long long* cells) {
  if (!fhh::voxel_grid_ok(grid)) return FH_ERR_ARG;
  // (each factor is below 2^31; the product of two fits 62 bits, and what is above the limit after two never comes back under it)
  const long long xy = (long long)grid->dims[0] * grid->dims[1];
  if (xy > 0x7fffffffll || xy * grid->dims[2] > 0x7fffffffll) return FH_ERR_ARG;
  *cells = xy * grid->dims[2];
  if (view_stride < (size_t)*cells) return FH_ERR_ARG;
  if (n_views < 1) return FH_ERR_ARG;
  return FH_OK;
}

// the clauses of fh_reach_goals_device from r_max to max_hops < 0, in the header's order (the fields that all three params share)
static int reach_field_clauses(double r_max, double r_avoid, double z_lo, double z_hi, int want, int max_hops) {
  if (!std::isfinite(r_max) || !(r_max > 0.0)) return FH_ERR_ARG;
  if (!std::isfinite(r_avoid) || !(r_avoid >= 0.0)) return FH_ERR_ARG;
  if (std::isnan(z_lo) || std::isnan(z_hi) || z_lo > z_hi) return FH_ERR_ARG;
  const int all_wants = FH_FRONTIER_WANT_REACHED | FH_FRONTIER_WANT_NO_PATH | FH_FRONTIER_WANT_ALL;
  if (want == 0 || (want & ~all_wants) != 0) return FH_ERR_ARG;
  if (max_hops < 0) return FH_ERR_ARG;
  return FH_OK;
}

// and its clauses from map_grid to n < 0 (fh_gain_goals_device has clauses of its own between the two)
static int reach_table_clauses(const fh_voxel_grid* map_grid, const unsigned* d_map_bits, const fh_voxel_grid* grid, size_t view_stride, int n_views,
                               int n) {
  if (!fhh::voxel_grid_ok(map_grid)) return FH_ERR_ARG;
  const long long map_xy = (long long)map_grid->dims[0] * map_grid->dims[1];
  if (map_xy > 0x7fffffffll || map_xy * map_grid->dims[2] > 0x7fffffffll) return FH_ERR_ARG;
  if (!d_map_bits) return FH_ERR_ARG;
  long long cells = 0;
  if (reach_lattice(grid, view_stride, n_views, &cells) != FH_OK) return FH_ERR_ARG;
  if (n < 0) return FH_ERR_ARG;
  return FH_OK;
}

// the clauses of fh_reach_goals_device from r_max to n < 0, in the header's order (it and fh_spread_goals_device)
static int reach_clauses(double r_max, double r_avoid, double z_lo, double z_hi, int want, int max_hops, const fh_voxel_grid* map_grid,
                         const unsigned* d_map_bits, const fh_voxel_grid* grid, size_t view_stride, int n_views, int n) {
  if (reach_field_clauses(r_max, r_avoid, z_lo, z_hi, want, max_hops) != FH_OK) return FH_ERR_ARG;
  return reach_table_clauses(map_grid, d_map_bits, grid, view_stride, n_views, n);
}

// the kernel's arguments from checked values (the outputs are the caller's to set)
static void reach_args(fhp::ReachArgs& a, double r_max, double r_avoid, double z_lo, double z_hi, int want, int max_hops,
                       const fh_voxel_grid* map_grid, const unsigned* d_map_bits, const fh_voxel_grid* grid, const unsigned char* d_flags,
                       size_t view_stride, const int32_t* d_view_of, int n_views, const fh_vehicle* d_vehicles) {
  a.r_max = r_max;
  a.r2 = r_max * r_max;
  a.a2 = r_avoid * r_avoid;
  a.z_lo = z_lo; a.z_hi = z_hi;
  a.want = want;
  a.max_hops = max_hops;
  fhh::set_lattice(a, *grid);
  a.flags = d_flags; a.view_stride = view_stride; a.view_of = d_view_of; a.n_views = n_views;
  a.vehicles = d_vehicles;
  a.mx = map_grid->dims[0]; a.my = map_grid->dims[1]; a.mz = map_grid->dims[2];
  a.mres = map_grid->res; a.mox = map_grid->origin[0]; a.moy = map_grid->origin[1]; a.moz = map_grid->origin[2];
  a.bits = d_map_bits;
}

// the class bytes, rounded up to a multiple of 64, before the rows
static size_t spread_rows_offset(int n) { return ((size_t)n + 63) & ~(size_t)63; }

extern "C" {

int fh_reach_goals_device(void* stream, const fh_reach_params* par, const fh_voxel_grid* map_grid, const unsigned* d_map_bits,
                          const fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of, int n_views,
                          const fh_vehicle* d_vehicles, int n, double* d_goals, int32_t* d_mask, fh_reach_record* d_records) {
  if (!par) return FH_ERR_ARG;
  if (reach_clauses(par->r_max, par->r_avoid, par->z_lo, par->z_hi, par->want, par->max_hops, map_grid, d_map_bits, grid, view_stride, n_views,
                    n) != FH_OK)
    return FH_ERR_ARG;
  if (n == 0) return FH_OK;
  if (!d_flags || !d_vehicles || !d_goals || !d_mask || !d_records) return FH_ERR_ARG;
  hipPointerAttribute_t where;
  if (hipPointerGetAttributes(&where, d_records) != hipSuccess || where.type != hipMemoryTypeDevice) {
    (void)hipGetLastError();
    return FH_ERR_DEVICE;
  }
  fhh::DeviceScope scope(where.device);
  if (!scope.ok) return FH_ERR_DEVICE;
  fhp::ReachArgs a;
  reach_args(a, par->r_max, par->r_avoid, par->z_lo, par->z_hi, par->want, par->max_hops, map_grid, d_map_bits, grid, d_flags, view_stride,
             d_view_of, n_views, d_vehicles);
  a.goals = d_goals; a.mask = d_mask; a.records = d_records;
  hipLaunchKernelGGL(fhp::reach_goals_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? FH_OK : FH_ERR_DEVICE;
}

size_t fh_spread_work_bytes(int n) { return n <= 0 ? 0 : spread_rows_offset(n) + (size_t)n * FH_SPREAD_LIST * sizeof(int32_t); }

int fh_spread_goals_device(void* stream, const fh_spread_params* par, const fh_voxel_grid* map_grid, const unsigned* d_map_bits,
                           const fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of, int n_views,
                           const int32_t* d_group, const fh_vehicle* d_vehicles, int n, void* d_work, size_t work_bytes, double* d_goals,
                           int32_t* d_mask, fh_spread_record* d_records) {
  if (!par) return FH_ERR_ARG;
  if (reach_clauses(par->r_max, par->r_avoid, par->z_lo, par->z_hi, par->want, par->max_hops, map_grid, d_map_bits, grid, view_stride, n_views,
                    n) != FH_OK)
    return FH_ERR_ARG;
  if (!std::isfinite(par->r_spread) || !(par->r_spread > 0.0)) return FH_ERR_ARG;
  if (par->passes < 1 || par->passes > FH_SPREAD_MAX_PASSES) return FH_ERR_ARG;
  if (n == 0) return FH_OK;
  if (!d_flags || !d_vehicles || !d_goals || !d_mask || !d_records) return FH_ERR_ARG;
  if (!d_work) return FH_ERR_ARG;
  if (work_bytes < fh_spread_work_bytes(n)) return FH_ERR_ARG;
  hipPointerAttribute_t where;
  if (hipPointerGetAttributes(&where, d_records) != hipSuccess || where.type != hipMemoryTypeDevice) {
    (void)hipGetLastError();
    return FH_ERR_DEVICE;
  }
  fhh::DeviceScope scope(where.device);
  if (!scope.ok) return FH_ERR_DEVICE;
  fhp::SpreadArgs s;
  reach_args(s.r, par->r_max, par->r_avoid, par->z_lo, par->z_hi, par->want, par->max_hops, map_grid, d_map_bits, grid, d_flags, view_stride,
             d_view_of, n_views, d_vehicles);
  s.r.goals = d_goals; s.r.mask = d_mask; s.r.records = nullptr;
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
  if (reach_field_clauses(par->r_max, par->r_avoid, par->z_lo, par->z_hi, par->want, par->max_hops) != FH_OK) return FH_ERR_ARG;
  if (par->gain_radius < 0 || par->gain_radius > FH_GAIN_MAX_RADIUS) return FH_ERR_ARG;
  if (par->hop_cost < 0 || par->hop_cost > FH_GAIN_MAX_HOP_COST) return FH_ERR_ARG;
  if (par->min_gain < 0) return FH_ERR_ARG;
  if (reach_table_clauses(map_grid, d_map_bits, grid, view_stride, n_views, n) != FH_OK) return FH_ERR_ARG;
  if (n == 0) return FH_OK;
  if (!d_flags || !d_vehicles || !d_goals || !d_mask || !d_records) return FH_ERR_ARG;
  hipPointerAttribute_t where;
  if (hipPointerGetAttributes(&where, d_records) != hipSuccess || where.type != hipMemoryTypeDevice) {
    (void)hipGetLastError();
    return FH_ERR_DEVICE;
  }
  fhh::DeviceScope scope(where.device);
  if (!scope.ok) return FH_ERR_DEVICE;
  fhp::GainArgs s;
  reach_args(s.r, par->r_max, par->r_avoid, par->z_lo, par->z_hi, par->want, par->max_hops, map_grid, d_map_bits, grid, d_flags, view_stride,
             d_view_of, n_views, d_vehicles);
  s.r.goals = d_goals; s.r.mask = d_mask; s.r.records = nullptr;
  s.g = par->gain_radius;
  s.g2 = par->gain_radius * par->gain_radius;
  s.hop_cost = par->hop_cost;
  s.min_gain = par->min_gain;
  s.records = d_records;
  hipLaunchKernelGGL(fhp::gain_goals_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, s);
  return hipGetLastError() == hipSuccess ? FH_OK : FH_ERR_DEVICE;
}

// the words of a bitmap of blocks of edge `block` over the lattice; 0: a null grid, a dimension < 1 or a block outside 1..16;
// FH_FAR_MAX_WORDS + 1: more than FH_FAR_MAX_WORDS (each partial product is tested, so nothing overflows)
static int far_words(const fh_voxel_grid* grid, int block) {
  if (!fhh::voxel_grid_ok(grid, false) || block < 1 || block > 16) return 0;
  long long w = (((long long)grid->dims[0] + block - 1) / block + 63) / 64;
  for (int k = 1; k < 3; k++) {
    if (w > FH_FAR_MAX_WORDS) return FH_FAR_MAX_WORDS + 1;
    w *= ((long long)grid->dims[k] + block - 1) / block;
  }
  return w > FH_FAR_MAX_WORDS ? FH_FAR_MAX_WORDS + 1 : (int)w;
}

size_t fh_far_work_bytes(const fh_voxel_grid* grid, int block, int n_views) {
  const int W = far_words(grid, block);
  if (W < 1 || W > FH_FAR_MAX_WORDS || n_views < 1) return 0;
  return (size_t)n_views * 4u * (size_t)W * sizeof(unsigned long long) + (((size_t)n_views + 63) & ~(size_t)63);
}

int fh_far_goals_device(void* stream, const fh_far_params* par, const fh_voxel_grid* map_grid, const unsigned* d_map_bits,
                        const fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of, int n_views,
                        const int32_t* d_skip, const fh_vehicle* d_vehicles, int n, void* d_work, size_t work_bytes, double* d_goals,
                        int32_t* d_mask, fh_far_record* d_records) {
  static_assert(sizeof(fh_far_params) == 64 && sizeof(fh_far_record) == 64 && FH_FAR_MAX_WORDS % 256 == 0, "include/fasterhip_far.h");
  if (!par) return FH_ERR_ARG;
  // (K15's field clauses without r_max, which this chooser does not have: any r_max that passes stands in for it)
  if (reach_field_clauses(1.0, par->r_avoid, par->z_lo, par->z_hi, par->want, par->max_hops) != FH_OK) return FH_ERR_ARG;
  if (par->block < 1 || par->block > 16) return FH_ERR_ARG;
  if (reach_table_clauses(map_grid, d_map_bits, grid, view_stride, n_views, n) != FH_OK) return FH_ERR_ARG;
  const int W = far_words(grid, par->block);
  if (W > FH_FAR_MAX_WORDS) return FH_ERR_ARG;
  if (work_bytes < fh_far_work_bytes(grid, par->block, n_views)) return FH_ERR_ARG;
  if (n == 0) return FH_OK;
  if (!d_work || !d_flags || !d_vehicles || !d_goals || !d_mask || !d_records) return FH_ERR_ARG;
  hipPointerAttribute_t where;
  if (hipPointerGetAttributes(&where, d_records) != hipSuccess || where.type != hipMemoryTypeDevice) {
    (void)hipGetLastError();
    return FH_ERR_DEVICE;
  }
  fhh::DeviceScope scope(where.device);
  if (!scope.ok) return FH_ERR_DEVICE;
  fhp::FarArgs s;
  reach_args(s.r, 1.0, par->r_avoid, par->z_lo, par->z_hi, par->want, par->max_hops, map_grid, d_map_bits, grid, d_flags, view_stride, d_view_of,
             n_views, d_vehicles);
  s.r.goals = d_goals; s.r.mask = d_mask; s.r.records = nullptr;
  s.B = par->block;
  s.cx = (grid->dims[0] + s.B - 1) / s.B;  // (W <= FH_FAR_MAX_WORDS: the dims are far below 2^31 - 16)
  s.cy = (grid->dims[1] + s.B - 1) / s.B;
  s.cz = (grid->dims[2] + s.B - 1) / s.B;
  s.wx = (s.cx + 63) / 64;
  s.W = W;
  s.n = n;
  s.skip = d_skip;
  s.sums = static_cast<unsigned long long*>(d_work);
  const size_t need_bytes = ((size_t)n_views + 63) & ~(size_t)63;
  s.need = static_cast<unsigned char*>(d_work) + (size_t)n_views * 4u * (size_t)W * sizeof(unsigned long long);
  s.records = d_records;
  const hipStream_t q = (hipStream_t)stream;
  if (hipMemsetAsync(s.need, 0, need_bytes, q) != hipSuccess) {
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

size_t fh_apart_work_bytes(const fh_voxel_grid* grid, int block, int n_views, int n) {
  const size_t far = fh_far_work_bytes(grid, block, n_views);
  if (far == 0 || n < 0) return 0;
  return far + spread_rows_offset(n) + (size_t)n * sizeof(int32_t) + (size_t)n * sizeof(int32_t);
}

size_t fh_prospect_work_bytes(const fh_voxel_grid* grid, int block, int n_views) {
  const size_t far = fh_far_work_bytes(grid, block, n_views);  // (0: a null grid, a dimension < 1, a block outside 1..16, too many words, n_views < 1)
  if (far == 0) return 0;
  return far + (size_t)n_views * 64u * (size_t)far_words(grid, block) * sizeof(uint16_t);
}

size_t fh_stake_work_bytes(const fh_voxel_grid* grid, int block, int n_views, int n) {
  const size_t pro = fh_prospect_work_bytes(grid, block, n_views);
  if (pro == 0 || n < 0) return 0;
  return pro + spread_rows_offset(n) + (size_t)n * sizeof(int32_t) + (size_t)n * sizeof(int32_t);
}

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
                    offsetof(fh_stake_record, covered) == 112 && offsetof(fh_stake_record, removed) == 116 &&
                    fhp::STAKE_NONE == fhp::FAR_SPREAD_NONE && fhp::STAKE_SEARCHER == fhp::FAR_SPREAD_SEARCHER &&
                    fhp::STAKE_STANDING == fhp::FAR_SPREAD_STANDING,
                "include/fasterhip_stake.h: K21's, K22's and K23's params, records, flags, limits and class bytes under its own names");
  if (!par) return FH_ERR_ARG;
  if (reach_field_clauses(1.0, par->r_avoid, par->z_lo, par->z_hi, par->want, par->max_hops) != FH_OK) return FH_ERR_ARG;
  if (par->block < 1 || par->block > 16) return FH_ERR_ARG;
  if (par->gain_blocks < 0 || par->gain_blocks > FH_STAKE_MAX_BLOCKS) return FH_ERR_ARG;
  if (par->hop_cost < 0 || par->hop_cost > FH_STAKE_MAX_HOP_COST) return FH_ERR_ARG;
  if (par->min_gain < 0) return FH_ERR_ARG;
  if (reach_table_clauses(map_grid, d_map_bits, grid, view_stride, n_views, n) != FH_OK) return FH_ERR_ARG;
  const int W = far_words(grid, par->block);
  if (W > FH_STAKE_MAX_WORDS) return FH_ERR_ARG;
  if (!std::isfinite(par->r_spread) || !(par->r_spread > 0.0)) return FH_ERR_ARG;
  if (par->passes < 1 || par->passes > FH_STAKE_MAX_PASSES) return FH_ERR_ARG;
  if (par->claim_blocks < 0 || par->claim_blocks > FH_STAKE_MAX_CLAIM_BLOCKS) return FH_ERR_ARG;
  if (work_bytes < fh_stake_work_bytes(grid, par->block, n_views, n)) return FH_ERR_ARG;
  if (n == 0) return FH_OK;
  if (!d_work || !d_flags || !d_vehicles || !d_goals || !d_mask || !d_records) return FH_ERR_ARG;
  hipPointerAttribute_t where;
  if (hipPointerGetAttributes(&where, d_records) != hipSuccess || where.type != hipMemoryTypeDevice) {
    (void)hipGetLastError();
    return FH_ERR_DEVICE;
  }
  fhh::DeviceScope scope(where.device);
  if (!scope.ok) return FH_ERR_DEVICE;
  fhp::StakeArgs k;
  fhp::ProspectArgs& x = k.p;
  fhp::FarArgs& s = x.f;
  reach_args(s.r, 1.0, par->r_avoid, par->z_lo, par->z_hi, par->want, par->max_hops, map_grid, d_map_bits, grid, d_flags, view_stride, d_view_of,
             n_views, d_vehicles);
  s.r.goals = d_goals; s.r.mask = d_mask; s.r.records = nullptr;
  s.B = par->block;
  s.cx = (grid->dims[0] + s.B - 1) / s.B;
  s.cy = (grid->dims[1] + s.B - 1) / s.B;
  s.cz = (grid->dims[2] + s.B - 1) / s.B;
  s.wx = (s.cx + 63) / 64;
  s.W = W;
  s.n = n;
  s.skip = d_skip;
  unsigned char* const work = static_cast<unsigned char*>(d_work);
  s.sums = static_cast<unsigned long long*>(d_work);
  const size_t need_bytes = ((size_t)n_views + 63) & ~(size_t)63;
  s.need = work + (size_t)n_views * 4u * (size_t)W * sizeof(unsigned long long);
  s.records = nullptr;
  x.g = par->gain_blocks;
  x.hop_cost = par->hop_cost;
  x.min_gain = par->min_gain;
  x.counts = reinterpret_cast<uint16_t*>(s.need + need_bytes);  // (= work + K21's bytes: a multiple of 8)
  x.records = nullptr;
  fhp::FarSpreadArgs c;  // what K22's class kernel reads: the judge's values, the labels and the two tables it writes
  c.f = s;
  c.s2 = par->r_spread * par->r_spread;
  c.pass = 0; c.passes = par->passes;
  c.group = d_group;
  c.cls = work + fh_prospect_work_bytes(grid, par->block, n_views);  // (K23's bytes: a multiple of 8)
  c.grp = reinterpret_cast<int32_t*>(c.cls + spread_rows_offset(n));
  c.lower = c.grp + n;
  c.records = nullptr;
  k.s2 = c.s2;
  k.pass = 0; k.passes = par->passes;
  k.k = par->claim_blocks;
  k.cls = c.cls; k.grp = c.grp; k.lower = c.lower;
  k.records = d_records;
  const hipStream_t q = (hipStream_t)stream;
  if (hipMemsetAsync(s.need, 0, need_bytes, q) != hipSuccess) {
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
  if (reach_field_clauses(1.0, par->r_avoid, par->z_lo, par->z_hi, par->want, par->max_hops) != FH_OK) return FH_ERR_ARG;
  if (par->block < 1 || par->block > 16) return FH_ERR_ARG;
  if (par->gain_blocks < 0 || par->gain_blocks > FH_PROSPECT_MAX_BLOCKS) return FH_ERR_ARG;
  if (par->hop_cost < 0 || par->hop_cost > FH_PROSPECT_MAX_HOP_COST) return FH_ERR_ARG;
  if (par->min_gain < 0) return FH_ERR_ARG;
  if (reach_table_clauses(map_grid, d_map_bits, grid, view_stride, n_views, n) != FH_OK) return FH_ERR_ARG;
  const int W = far_words(grid, par->block);
  if (W > FH_PROSPECT_MAX_WORDS) return FH_ERR_ARG;
  if (work_bytes < fh_prospect_work_bytes(grid, par->block, n_views)) return FH_ERR_ARG;
  if (n == 0) return FH_OK;
  if (!d_work || !d_flags || !d_vehicles || !d_goals || !d_mask || !d_records) return FH_ERR_ARG;
  hipPointerAttribute_t where;
  if (hipPointerGetAttributes(&where, d_records) != hipSuccess || where.type != hipMemoryTypeDevice) {
    (void)hipGetLastError();
    return FH_ERR_DEVICE;
  }
  fhh::DeviceScope scope(where.device);
  if (!scope.ok) return FH_ERR_DEVICE;
  fhp::ProspectArgs x;
  fhp::FarArgs& s = x.f;
  reach_args(s.r, 1.0, par->r_avoid, par->z_lo, par->z_hi, par->want, par->max_hops, map_grid, d_map_bits, grid, d_flags, view_stride, d_view_of,
             n_views, d_vehicles);
  s.r.goals = d_goals; s.r.mask = d_mask; s.r.records = nullptr;
  s.B = par->block;
  s.cx = (grid->dims[0] + s.B - 1) / s.B;
  s.cy = (grid->dims[1] + s.B - 1) / s.B;
  s.cz = (grid->dims[2] + s.B - 1) / s.B;
  s.wx = (s.cx + 63) / 64;
  s.W = W;
  s.n = n;
  s.skip = d_skip;
  unsigned char* const work = static_cast<unsigned char*>(d_work);
  s.sums = static_cast<unsigned long long*>(d_work);
  const size_t need_bytes = ((size_t)n_views + 63) & ~(size_t)63;
  s.need = work + (size_t)n_views * 4u * (size_t)W * sizeof(unsigned long long);
  s.records = nullptr;
  x.g = par->gain_blocks;
  x.hop_cost = par->hop_cost;
  x.min_gain = par->min_gain;
  x.counts = reinterpret_cast<uint16_t*>(s.need + need_bytes);  // (= work + K21's bytes: a multiple of 8)
  x.records = d_records;
  const hipStream_t q = (hipStream_t)stream;
  if (hipMemsetAsync(s.need, 0, need_bytes, q) != hipSuccess) {
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
  if (reach_field_clauses(1.0, par->r_avoid, par->z_lo, par->z_hi, par->want, par->max_hops) != FH_OK) return FH_ERR_ARG;
  if (par->block < 1 || par->block > 16) return FH_ERR_ARG;
  if (reach_table_clauses(map_grid, d_map_bits, grid, view_stride, n_views, n) != FH_OK) return FH_ERR_ARG;
  const int W = far_words(grid, par->block);
  if (W > FH_FAR_MAX_WORDS) return FH_ERR_ARG;
  if (!std::isfinite(par->r_spread) || !(par->r_spread > 0.0)) return FH_ERR_ARG;
  if (par->passes < 1 || par->passes > FH_APART_MAX_PASSES) return FH_ERR_ARG;
  if (work_bytes < fh_apart_work_bytes(grid, par->block, n_views, n)) return FH_ERR_ARG;
  if (n == 0) return FH_OK;
  if (!d_work || !d_flags || !d_vehicles || !d_goals || !d_mask || !d_records) return FH_ERR_ARG;
  hipPointerAttribute_t where;
  if (hipPointerGetAttributes(&where, d_records) != hipSuccess || where.type != hipMemoryTypeDevice) {
    (void)hipGetLastError();
    return FH_ERR_DEVICE;
  }
  fhh::DeviceScope scope(where.device);
  if (!scope.ok) return FH_ERR_DEVICE;
  fhp::FarSpreadArgs x;
  fhp::FarArgs& s = x.f;
  reach_args(s.r, 1.0, par->r_avoid, par->z_lo, par->z_hi, par->want, par->max_hops, map_grid, d_map_bits, grid, d_flags, view_stride, d_view_of,
             n_views, d_vehicles);
  s.r.goals = d_goals; s.r.mask = d_mask; s.r.records = nullptr;
  s.B = par->block;
  s.cx = (grid->dims[0] + s.B - 1) / s.B;
  s.cy = (grid->dims[1] + s.B - 1) / s.B;
  s.cz = (grid->dims[2] + s.B - 1) / s.B;
  s.wx = (s.cx + 63) / 64;
  s.W = W;
  s.n = n;
  s.skip = d_skip;
  unsigned char* const work = static_cast<unsigned char*>(d_work);
  s.sums = static_cast<unsigned long long*>(d_work);
  const size_t need_bytes = ((size_t)n_views + 63) & ~(size_t)63;
  s.need = work + (size_t)n_views * 4u * (size_t)W * sizeof(unsigned long long);
  s.records = nullptr;
  x.s2 = par->r_spread * par->r_spread;
  x.pass = 0; x.passes = par->passes;
  x.group = d_group;
  x.cls = s.need + need_bytes;  // (= work + fh_far_work_bytes: a multiple of 8)
  x.grp = reinterpret_cast<int32_t*>(x.cls + spread_rows_offset(n));
  x.lower = x.grp + n;
  x.records = d_records;
  const hipStream_t q = (hipStream_t)stream;
  if (hipMemsetAsync(s.need, 0, need_bytes, q) != hipSuccess) {
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
  if (reach_clauses(par->r_max, par->r_avoid, par->z_lo, par->z_hi, par->want, par->max_hops, map_grid, d_map_bits, grid, view_stride, n_views,
                    n) != FH_OK)
    return FH_ERR_ARG;
  if (!std::isfinite(par->r_spread) || !(par->r_spread > 0.0)) return FH_ERR_ARG;
  if (par->passes < 1 || par->passes > FH_BID_MAX_PASSES) return FH_ERR_ARG;
  if (par->gain_radius < 0 || par->gain_radius > FH_BID_MAX_RADIUS) return FH_ERR_ARG;
  if (par->hop_cost < 0 || par->hop_cost > FH_BID_MAX_HOP_COST) return FH_ERR_ARG;
  if (par->min_gain < 0) return FH_ERR_ARG;
  if (par->claim_radius < -1 || par->claim_radius > FH_BID_MAX_RADIUS) return FH_ERR_ARG;
  if (n == 0) return FH_OK;
  if (!d_flags || !d_vehicles || !d_goals || !d_mask || !d_records) return FH_ERR_ARG;
  if (!d_work) return FH_ERR_ARG;
  if (work_bytes < fh_bid_work_bytes(n)) return FH_ERR_ARG;
  hipPointerAttribute_t where;
  if (hipPointerGetAttributes(&where, d_records) != hipSuccess || where.type != hipMemoryTypeDevice) {
    (void)hipGetLastError();
    return FH_ERR_DEVICE;
  }
  fhh::DeviceScope scope(where.device);
  if (!scope.ok) return FH_ERR_DEVICE;
  fhp::BidArgs s;
  reach_args(s.gn.r, par->r_max, par->r_avoid, par->z_lo, par->z_hi, par->want, par->max_hops, map_grid, d_map_bits, grid, d_flags, view_stride,
             d_view_of, n_views, d_vehicles);
  s.gn.r.goals = d_goals; s.gn.r.mask = d_mask; s.gn.r.records = nullptr;
  s.gn.g = par->gain_radius;
  s.gn.g2 = par->gain_radius * par->gain_radius;
  s.gn.hop_cost = par->hop_cost;
  s.gn.min_gain = par->min_gain;
  s.gn.records = nullptr;
  // the interaction radius: a peer beyond it cannot touch the ball of a candidate
  const double r_int = par->claim_radius < 0 ? par->r_spread : std::fmax(par->r_spread, (double)(par->gain_radius + par->claim_radius + 1) * grid->res);
  const double reach = (par->r_max + par->r_max) + r_int, near = par->r_max + r_int;
  s.s2 = par->r_spread * par->r_spread;
  s.reach2 = reach * reach;
  s.near2 = near * near;
  s.n = n; s.pass = 0; s.last = 0;
  s.cr = par->claim_radius;
  s.cr2 = par->claim_radius * par->claim_radius;
  s.group = d_group;
  unsigned char* const work = static_cast<unsigned char*>(d_work);
  s.cls = work;
  s.rows = reinterpret_cast<int32_t*>(work + spread_rows_offset(n));
  s.offers = reinterpret_cast<int32_t*>(work + bid_offers_offset(n));
  s.decided = s.offers + 2 * (size_t)n;
  s.records = d_records;
  fhp::SpreadArgs c;  // the class kernel of fh_spread.hip.hpp as it is: it reads the vehicles and writes the class bytes
  c.r = s.gn.r;
  c.s2 = s.s2; c.reach2 = s.reach2; c.near2 = s.near2;
  c.n = n; c.pass = 0;
  c.group = d_group;
  c.cls = work;
  c.rows = s.rows;
  c.records = nullptr;
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
  if (reach_field_clauses(par->r_max, par->r_avoid, par->z_lo, par->z_hi, par->want, par->max_hops) != FH_OK) return FH_ERR_ARG;
  if (par->gain_radius < 0 || par->gain_radius > FH_SIGHT_MAX_RADIUS) return FH_ERR_ARG;
  if (par->hop_cost < 0 || par->hop_cost > FH_SIGHT_MAX_HOP_COST) return FH_ERR_ARG;
  if (par->min_gain < 0) return FH_ERR_ARG;
  if (reach_table_clauses(map_grid, d_map_bits, grid, view_stride, n_views, n) != FH_OK) return FH_ERR_ARG;
  if (n == 0) return FH_OK;
  if (!d_flags || !d_vehicles || !d_goals || !d_mask || !d_records) return FH_ERR_ARG;
  hipPointerAttribute_t where;
  if (hipPointerGetAttributes(&where, d_records) != hipSuccess || where.type != hipMemoryTypeDevice) {
    (void)hipGetLastError();
    return FH_ERR_DEVICE;
  }
  fhh::DeviceScope scope(where.device);
  if (!scope.ok) return FH_ERR_DEVICE;
  fhp::SightArgs s;
  reach_args(s.gn.r, par->r_max, par->r_avoid, par->z_lo, par->z_hi, par->want, par->max_hops, map_grid, d_map_bits, grid, d_flags, view_stride,
             d_view_of, n_views, d_vehicles);
  s.gn.r.goals = d_goals; s.gn.r.mask = d_mask; s.gn.r.records = nullptr;
  s.gn.g = par->gain_radius;
  s.gn.g2 = par->gain_radius * par->gain_radius;
  s.gn.hop_cost = par->hop_cost;
  s.gn.min_gain = par->min_gain;
  s.gn.records = nullptr;
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
  if (reach_clauses(par->r_max, par->r_avoid, par->z_lo, par->z_hi, par->want, par->max_hops, map_grid, d_map_bits, grid, view_stride, n_views,
                    n) != FH_OK)
    return FH_ERR_ARG;
  if (!std::isfinite(par->r_spread) || !(par->r_spread > 0.0)) return FH_ERR_ARG;
  if (par->passes < 1 || par->passes > FH_TEAM_MAX_PASSES) return FH_ERR_ARG;
  if (par->gain_radius < 0 || par->gain_radius > FH_TEAM_MAX_RADIUS) return FH_ERR_ARG;
  if (par->hop_cost < 0 || par->hop_cost > FH_TEAM_MAX_HOP_COST) return FH_ERR_ARG;
  if (par->min_gain < 0) return FH_ERR_ARG;
  if (par->claim_radius < -1 || par->claim_radius > FH_TEAM_MAX_RADIUS) return FH_ERR_ARG;
  if (n == 0) return FH_OK;
  if (!d_flags || !d_vehicles || !d_goals || !d_mask || !d_records) return FH_ERR_ARG;
  if (!d_work) return FH_ERR_ARG;
  if (work_bytes < fh_spread_work_bytes(n)) return FH_ERR_ARG;
  hipPointerAttribute_t where;
  if (hipPointerGetAttributes(&where, d_records) != hipSuccess || where.type != hipMemoryTypeDevice) {
    (void)hipGetLastError();
    return FH_ERR_DEVICE;
  }
  fhh::DeviceScope scope(where.device);
  if (!scope.ok) return FH_ERR_DEVICE;
  fhp::TeamArgs s;
  reach_args(s.gn.r, par->r_max, par->r_avoid, par->z_lo, par->z_hi, par->want, par->max_hops, map_grid, d_map_bits, grid, d_flags, view_stride,
             d_view_of, n_views, d_vehicles);
  s.gn.r.goals = d_goals; s.gn.r.mask = d_mask; s.gn.r.records = nullptr;
  s.gn.g = par->gain_radius;
  s.gn.g2 = par->gain_radius * par->gain_radius;
  s.gn.hop_cost = par->hop_cost;
  s.gn.min_gain = par->min_gain;
  s.gn.records = nullptr;
  // the interaction radius: a peer beyond it cannot touch the ball of a candidate
  const double r_int = par->claim_radius < 0 ? par->r_spread : std::fmax(par->r_spread, (double)(par->gain_radius + par->claim_radius + 1) * grid->res);
  const double reach = (par->r_max + par->r_max) + r_int, near = par->r_max + r_int;
  s.s2 = par->r_spread * par->r_spread;
  s.reach2 = reach * reach;
  s.near2 = near * near;
  s.n = n; s.pass = 0;
  s.cr = par->claim_radius;
  s.cr2 = par->claim_radius * par->claim_radius;
  s.group = d_group;
  s.cls = static_cast<unsigned char*>(d_work);
  s.rows = reinterpret_cast<int32_t*>(static_cast<unsigned char*>(d_work) + spread_rows_offset(n));
  s.records = d_records;
  fhp::SpreadArgs c;  // the class kernel of fh_spread.hip.hpp as it is: it reads the vehicles and writes the class bytes
  c.r = s.gn.r;
  c.s2 = s.s2; c.reach2 = s.reach2; c.near2 = s.near2;
  c.n = n; c.pass = 0;
  c.group = d_group;
  c.cls = static_cast<unsigned char*>(d_work);
  c.rows = s.rows;
  c.records = nullptr;
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

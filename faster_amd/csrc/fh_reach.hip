// fh_reach.hip — host side of include/fasterhip_reach.h (fh_reach_goals_device): the frontier voxel that a flood of the space a vehicle
// knows to be free reaches in the fewest steps (kernel: fh_reach.hip.hpp).  A translation unit of its own: fh_map.hip and fh_capi.hip,
// their kernels and their code objects are what they were.  No CPU fallback.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/fasterhip.h"
#include "../../include/fasterhip_reach.h"
#include "fh_reach.hip.hpp"
#include "fh_host.hpp"

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

extern "C" {

int fh_reach_goals_device(void* stream, const fh_reach_params* par, const fh_voxel_grid* map_grid, const unsigned* d_map_bits,
                          const fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of, int n_views,
                          const fh_vehicle* d_vehicles, int n, double* d_goals, int32_t* d_mask, fh_reach_record* d_records) {
  if (!par) return FH_ERR_ARG;
  if (!std::isfinite(par->r_max) || !(par->r_max > 0.0)) return FH_ERR_ARG;
  if (!std::isfinite(par->r_avoid) || !(par->r_avoid >= 0.0)) return FH_ERR_ARG;
  if (std::isnan(par->z_lo) || std::isnan(par->z_hi) || par->z_lo > par->z_hi) return FH_ERR_ARG;
  const int all_wants = FH_FRONTIER_WANT_REACHED | FH_FRONTIER_WANT_NO_PATH | FH_FRONTIER_WANT_ALL;
  if (par->want == 0 || (par->want & ~all_wants) != 0) return FH_ERR_ARG;
  if (par->max_hops < 0) return FH_ERR_ARG;
  if (!fhh::voxel_grid_ok(map_grid)) return FH_ERR_ARG;
  const long long map_xy = (long long)map_grid->dims[0] * map_grid->dims[1];
  if (map_xy > 0x7fffffffll || map_xy * map_grid->dims[2] > 0x7fffffffll) return FH_ERR_ARG;
  if (!d_map_bits) return FH_ERR_ARG;
  long long cells = 0;
  if (reach_lattice(grid, view_stride, n_views, &cells) != FH_OK) return FH_ERR_ARG;
  if (n < 0) return FH_ERR_ARG;
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
  a.r_max = par->r_max;
  a.r2 = par->r_max * par->r_max;
  a.a2 = par->r_avoid * par->r_avoid;
  a.z_lo = par->z_lo; a.z_hi = par->z_hi;
  a.want = par->want;
  a.max_hops = par->max_hops;
  fhh::set_lattice(a, *grid);
  a.flags = d_flags; a.view_stride = view_stride; a.view_of = d_view_of; a.n_views = n_views;
  a.vehicles = d_vehicles;
  a.mx = map_grid->dims[0]; a.my = map_grid->dims[1]; a.mz = map_grid->dims[2];
  a.mres = map_grid->res; a.mox = map_grid->origin[0]; a.moy = map_grid->origin[1]; a.moz = map_grid->origin[2];
  a.bits = d_map_bits;
  a.goals = d_goals; a.mask = d_mask; a.records = d_records;
  hipLaunchKernelGGL(fhp::reach_goals_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? FH_OK : FH_ERR_DEVICE;
}

}  // extern "C"

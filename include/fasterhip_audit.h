/* fasterhip_audit.h: an audit of what a vehicle of the fleet (include/fasterhip.h) actually flies, the COMMITTED plan: the sampled
 * states in d_plans, against the unknown space of the vehicle's view and against occupied space (the points its view knows, or every
 * point of the cloud: ground truth).  The corridors are cut around voxel centres and inflated points, so a trajectory inside its
 * polytopes can still pass closer than drone_radius to a voxel centre or a point, and the first delta_t states of a plan are flown
 * whatever sensing and observing reveal after the commit.  The reference has a check of that piece, Faster::ARisInFreeSpace
 * (faster/src/faster.cpp:725-762, every tenth sample, a hard-coded 0.2 m; its call is commented out at :479-483).  A pure measurement:
 * nothing is written but d_out, no entry point of fasterhip.h changes, FH_ABI_VERSION stays.  C99 / C++11, includes fasterhip.h.
 *
 * THE MODEL.  Everything is IEEE double, no fused multiply-add (tests/audit_model.py restates it in numpy and the kernel is compared
 * with that bit for bit).  The squared distance of a tested position p to a point q is
 *     d2 = dx dx + dy dy + dz dz,   d = q - p per axis, the three products summed x, y, z from left to right.
 * The reference decides sqrt(d2) < r; this record decides d2 < r * r and reports squared distances, so nothing depends on how a
 * square root is rounded (faster_amd.abi.audit_distances takes the roots on the host).
 *   Tested states.  With head = d_vehicles[i].plan_head, size = .plan_size, m = count > 0 ? min(count, size) : size: the positions
 *     d_plans[i * max_states + head + j].pos for j = 0, stride, 2 stride, ... < m; n_tested = ceil(m / stride).  Every index reported
 *     is j, counted from the front of the plan.  A tested position with a coordinate that is not finite is skipped; it counts in
 *     n_tested and sets FH_AUDIT_NOT_FINITE.
 *   FH_AUDIT_BAD_PLAN.  head < 0, size < 0 or head + size > max_states, decided before any plan state is read: n_tested = 0, no side
 *     is evaluated, view = -1, the numbers are the defaults and the flag is alone.  An empty plan (size == 0) is not bad: n_tested = 0.
 *   The view.  Needed by the unknown side and by the masks: view = d_view_of ? d_view_of[i] : i; d_flags with view_stride == 0 and
 *     n_views == 1 is one grid for the whole fleet, and every vehicle has view 0.  A view outside [0, n_views) sets FH_AUDIT_NO_VIEW:
 *     the unknown side is not evaluated, no byte of d_flags or of the masks is read for that vehicle, and with masks it knows no point.
 *     The record's `view` is the number used, -1 when neither side needed one.
 *   Unknown side (d_flags != NULL).  The points are the centres ((ix + 0.5) res + origin), per axis, of the voxels of `grid` whose
 *     flag byte d_flags[view * view_stride + (iz ny + iy) nx + ix] is non-zero: the arithmetic of the safe corridor's nearest-unknown
 *     query.  min_unknown_d2 = the smallest d2 over tested states and unknown voxels among those with d2 < cap * cap, +INFINITY when
 *     there is none; worst_unknown = the smallest tested j that attains it, -1 when there is none; first_unknown = the smallest tested j
 *     with an unknown voxel at d2 < r_unknown * r_unknown, -1 when there is none; FH_AUDIT_UNKNOWN is set iff first_unknown >= 0.
 *   Occupied side (d_cloud_xyz != NULL and n_cloud > 0).  The points are the cloud points k whose three coordinates are finite and,
 *     with d_point_mask != NULL, whose bit k & 31 of word k >> 5 of row `view` ([n_views][mask_words], fasterhip_occupancy.h) is set;
 *     d_point_mask == NULL: every point counts, which is ground truth.  min_occupied_d2, worst_occupied, first_occupied (with
 *     r_occupied) and FH_AUDIT_OCCUPIED by the rules of the unknown side.
 *   A side that does not run leaves +INFINITY, -1 and -1.  All comparisons are strict: a point at exactly r is not near, a point at
 *     exactly cap is not looked at.  r <= cap, so what decides first_* is always inside what is looked at. */
#ifndef FASTERHIP_AUDIT_H
#define FASTERHIP_AUDIT_H
#include "fasterhip.h"
#ifdef __cplusplus
extern "C" {
#endif

enum {                       /* fh_plan_audit.flags */
  FH_AUDIT_BAD_PLAN = 1,     /* the plan extent of the vehicle record does not fit max_states: nothing was read, the flag is alone */
  FH_AUDIT_NO_VIEW = 2,      /* a view was needed and the vehicle's number lies outside [0, n_views)                                */
  FH_AUDIT_NOT_FINITE = 4,   /* a tested position has a coordinate that is not finite (it was skipped)                             */
  FH_AUDIT_UNKNOWN = 8,      /* first_unknown >= 0: a tested state is nearer than r_unknown to an unknown voxel centre              */
  FH_AUDIT_OCCUPIED = 16     /* first_occupied >= 0: a tested state is nearer than r_occupied to a point                           */
};
enum {
  FH_AUDIT_LIST_POINTS = 256,   /* capacity of the kernel's LDS list of candidate points (it is tested and emptied when it cannot
                                   take 64 more)                                                                                  */
  FH_AUDIT_SLAB_CELLS = 65536   /* lattice cells whose unknown bits one LDS slab holds: rows along x of the grown box of the
                                   plan, each padded to a multiple of 64 cells; a larger box is taken in several slabs            */
};

typedef struct fh_audit_params { /* 32 B */
  double r_unknown, r_occupied;  /* a tested state is "near" when d2 < r * r (strict)                                             */
  double cap;                    /* nothing at d2 >= cap * cap is looked at or reported                                           */
  int32_t stride, count;         /* tested plan indexes j = 0, stride, 2 stride, ... < m; m = count > 0 ? min(count, size) : size */
} fh_audit_params;

typedef struct fh_plan_audit { /* 64 B */
  int32_t flags, n_tested;     /* n_tested = ceil(m / stride) */
  int32_t first_unknown, worst_unknown;
  int32_t first_occupied, worst_occupied;
  int32_t view, reserved;
  double min_unknown_d2, min_occupied_d2;
  double reserved_d[2];
} fh_plan_audit;

/* d_out[i] = the audit of the plan of vehicle i.  One wavefront per vehicle, no working memory of the context; device pointers,
 * asynchronous on the context's stream; d_out aligned to 16 bytes (every device allocation is).  Only d_out is written.
 * FH_ERR_ARG, checked in this order after a null context: par == NULL; a radius or cap that is NaN, negative or infinite; cap <= 0;
 * r_unknown > cap or r_occupied > cap; stride < 1 or count < 0; n < 0 or max_states < 1; with d_flags: no grid, res <= 0, a dimension
 * < 1, cap > 64 res, n_views < 1, or view_stride non-zero and smaller than a view (dims[0] dims[1] dims[2] bytes); with d_point_mask:
 * mask_words * 32 < n_cloud or n_views < 1.  Then FH_ERR_DEVICE without a device (there is no CPU path), FH_OK for n == 0, and
 * FH_ERR_ARG for a null d_vehicles, d_plans or d_out.  Every index the kernel uses comes from a record it has checked: a wrong
 * vehicle record or view number gives a flag, never a read outside the arrays. */
int fh_fleet_audit_device(fh_ctx* ctx, const fh_audit_params* par, const fh_vehicle* d_vehicles, const fh_state* d_plans, int n, int max_states,
                          const struct fh_voxel_grid* grid, const unsigned char* d_flags, size_t view_stride, const int32_t* d_view_of, int n_views,
                          const double* d_cloud_xyz, int n_cloud, const uint32_t* d_point_mask, int mask_words, fh_plan_audit* d_out);

#ifdef __cplusplus
}
#endif
#endif /* FASTERHIP_AUDIT_H */

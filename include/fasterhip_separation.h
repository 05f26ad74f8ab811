/* fasterhip_separation.h: the committed plans of a fleet (include/fasterhip.h) against EACH OTHER.  Every vehicle plans as if it were
 * alone in the shared world; fasterhip_audit.h compares what it flies with unknown and occupied space, and this header compares it with
 * what the other vehicles fly.  The plans are aligned in time: every cycle ticks all vehicles by the same number of states
 * (fh_fleet_next_goals_device), so state j of every plan, counted from the front, belongs to the instant now + j dc.  A pure
 * measurement: nothing is written but d_out and working memory of the context, no entry point of fasterhip.h changes, FH_ABI_VERSION
 * stays.  C99 / C++11, includes fasterhip.h.
 *
 * THE MODEL.  Everything is IEEE double, no fused multiply-add (tests/separation_model.py restates it in numpy, brute force over all
 * pairs, and the kernels are compared with that bit for bit).  The squared distance of a position p of vehicle i to a position q of
 * vehicle k is the audit's:
 *     d2 = dx dx + dy dy + dz dz,   d = q - p per axis, the three products summed x, y, z from left to right,
 * and squared distances are decided and reported, so nothing depends on how a square root is rounded
 * (faster_amd.abi.separation_distances takes the roots on the host).
 *   Tested states of vehicle i: the audit's rules.  With head = d_vehicles[i].plan_head, size = .plan_size,
 *     m = count > 0 ? min(count, size) : size: the positions d_plans[i * max_states + head + j].pos for j = 0, stride, 2 stride, ... < m;
 *     n_tested = ceil(m / stride).  Every index reported is j, counted from the front of the plan: an instant.  A tested position with a
 *     coordinate that is not finite is skipped; it counts in n_tested and sets FH_SEP_NOT_FINITE.
 *   FH_SEP_BAD_PLAN.  head < 0, size < 0 or head + size > max_states, decided before any plan state is read: n_tested = 0, n_near = 0,
 *     the indexes are -1, min_d2 = +INFINITY and the flag is alone.  An empty plan (size == 0) is not bad: n_tested = 0.
 *   The others of vehicle i: every k != i whose record is not bad and whose plan_size >= 1.  At instant j vehicle k is at
 *     d_plans[k * max_states + head_k + min(j, size_k - 1)].pos: a vehicle whose plan has ended stands at its last state, which is what
 *     fh_fleet_next_goals_device hands out for it.  A coordinate of either side that is not finite makes d2 fail d2 < cap * cap by the
 *     arithmetic itself; there is no special case for the others.
 *   The record.  Over the tested j of i and its others k, among the pairs (j, k) with d2 < cap * cap:
 *     min_d2 = the smallest d2, +INFINITY when there is none; worst = the smallest tested j that attains it, worst_other = the smallest k
 *     that attains it at that j (-1, -1 when there is none); first = the smallest tested j with an other at d2 < r * r, first_other = the
 *     smallest such k at that j (-1, -1); n_near = how many distinct k are at d2 < r * r at one tested j at least; FH_SEP_NEAR is set
 *     iff first >= 0.  Ties go to the smallest j, then to the smallest k.  All comparisons are strict: an other at exactly r is not
 *     near, an other at exactly cap is not looked at.  r <= cap, so what decides first is inside what is looked at.
 *   ONE RECORD IS ONE SIDE OF A PAIR.  Record i tests only j < m_i: the instants at which i has ended (or lie beyond its `count`) and
 *     k still flies are in record k, where i is the one that stands at its last state.  The closest approach of the pair (i, k) is the
 *     smaller of the values the two records hold for it; for two plans of equal length and count == 0 the two are equal.
 *
 * THE CELL GRID.  `cells` (origin, res, dims) is a uniform grid that only the broad phase uses: every vehicle is counted into the cell
 * of the centre of its bounding box (clamped into the grid: vehicles outside sit in its border cells), and a vehicle looks at the cells
 * its own box reaches.  NO FIELD OF ANY RECORD DEPENDS ON THE GRID: dims = (1, 1, 1) gives the same bytes as a fine grid, slower.  A
 * good grid covers the space the fleet flies in with a cell of about cap, at least 1 m.  Known degradation: a vehicle sits in ONE
 * cell, that of its centre, so every vehicle has to look as far as the largest half-extent H of any box of the fleet reaches; one
 * vehicle with a very long plan raises H for everyone and the query degrades towards all pairs.  It stays correct.  Registering a
 * vehicle in several cells is not done. */
#ifndef FASTERHIP_SEPARATION_H
#define FASTERHIP_SEPARATION_H
#include "fasterhip.h"
#ifdef __cplusplus
extern "C" {
#endif

enum {                     /* fh_plan_separation.flags */
  FH_SEP_BAD_PLAN = 1,     /* the plan extent of the vehicle record does not fit max_states: nothing was read, the flag is alone; the
                              vehicle is not an other of anyone                                                                    */
  FH_SEP_NOT_FINITE = 4,   /* a tested position has a coordinate that is not finite (it was skipped)                             */
  FH_SEP_NEAR = 8          /* first >= 0: at a tested instant another vehicle is nearer than r                                    */
};
enum {
  FH_SEP_LIST_VEHICLES = 256,  /* capacity of the narrow phase's LDS list of candidate vehicles (it is tested and emptied when it
                                  cannot take 64 more)                                                                             */
  FH_SEP_MAX_CELLS = 1 << 20   /* the largest dims[0] * dims[1] * dims[2] of the cell grid                                          */
};

typedef struct fh_separation_params { /* 32 B */
  double r;              /* two vehicles are "near" at a tested instant when d2 < r * r (strict)                                   */
  double cap;            /* nothing at d2 >= cap * cap is looked at or reported; r <= cap                                          */
  int32_t stride, count; /* tested j = 0, stride, 2 stride, ... < m; m = count > 0 ? min(count, size) : size                       */
  int32_t reserved[2];
} fh_separation_params;

typedef struct fh_plan_separation { /* 64 B */
  int32_t flags, n_tested;      /* n_tested = ceil(m / stride)                                                                     */
  int32_t first, first_other;   /* smallest tested j with another vehicle at d2 < r r; the smallest such vehicle at that j         */
  int32_t worst, worst_other;   /* smallest tested j that attains min_d2; the smallest vehicle that attains it at that j           */
  int32_t n_near, reserved;     /* distinct other vehicles that are near at one tested j at least                                  */
  double min_d2;                /* smallest d2 below cap cap over tested j and others; +INFINITY when there is none                */
  double reserved_d[3];         /* zero                                                                                            */
} fh_plan_separation;

/* d_out[i] = the separation record of vehicle i.  Four launches on the context's stream (boxes, cell starts, cell items, the narrow
 * phase: one wavefront per vehicle), asynchronous; device pointers; d_out aligned to 16 bytes (every device allocation is).  Written:
 * d_out and working buffers of the context, which every call sets up again on the stream.  FH_ERR_ARG, checked in this order after a
 * null context: par == NULL; r or cap that is NaN, negative or infinite; cap <= 0; r > cap; stride < 1; count < 0; n < 0;
 * max_states < 1; cells == NULL, res <= 0, a dimension < 1, dims[0] dims[1] dims[2] > FH_SEP_MAX_CELLS.  Then FH_ERR_DEVICE without a
 * device (there is no CPU path), FH_OK for n == 0, and FH_ERR_ARG for a null d_vehicles, d_plans or d_out.  Every index the kernels
 * use comes from a record they have checked: a wrong vehicle record gives a flag, never a read outside the arrays. */
int fh_fleet_separation_device(fh_ctx* ctx, const fh_separation_params* par, const fh_vehicle* d_vehicles, const fh_state* d_plans, int n,
                               int max_states, const struct fh_voxel_grid* cells, fh_plan_separation* d_out);

#ifdef __cplusplus
}
#endif
#endif /* FASTERHIP_SEPARATION_H */

/*
 * sdplr_hip_dual_hp.h — the high-precision dual bound, dual_obj(data, var, aux, trace_bound, iter; highprecision=true)
 * (src/coreop.jl:376-415, branch :389-400), as one device call, and the bounds of a whole batch of instances as one call
 * in the form of the lockstep calls of sdplr_hip.h, whose batch conventions hold here too.
 *
 * sdplr_hip_dual_obj_hp does, in order: copy2y_λ_sub_pvio! (:384: y ← −min(λ_ub, λ − σ·primal_vio_raw), y[m+1] = 1),
 * 𝒜t_preprocess! (:385), the solver of sdplr_hip_S_eigval(s, 1, SA, ncv, tol, maxiter, v0, …) (:389-400) and
 * dual_value = −⟨y[1:m], b⟩ + trace_bound·min(ev, 0) (:412) with the dot product taken on the device.  Nothing but
 * scalars comes back over PCIe.  ncv ≤ 0 ⇒ min(100, n); tol ≤ 0 ⇒ machine precision; v0 (HOST, length n) or NULL for the
 * fixed internal start vector — all as in sdplr_hip_S_eigval, whose argument errors and error codes these are too (they are
 * checked before y is written).  Afterwards the handle holds y and the assembled S of that bound (a following At_left or
 * S_eigval uses them as they are).  *n_converged < 1 ⇒ the cycle budget ran out (mineig is the current Ritz value).
 *
 * sdplr_hip_batch_dual_obj_hp: each item is that argument list.  The items sdplr_hip_batch_S_eigval would serve by its
 * shared launch (include/sdplr_hip_eig_batch.h: the same test on the same arguments, nev = 1, SA) share TWO kinds of
 * launches: one prologue grid, a workgroup per instance, that forms y, assembles S.nzval from it — the same expressions
 * and, per entry of S, the same order of terms as the single-instance kernels: y and S are bit-identical to theirs — and
 * leaves ⟨y[1:m], b⟩ in the instance's result block (that sum alone is taken in another order); then the resident
 * thick-restart Lanczos of the batch eigenvalue call, bounded launches until every instance has finished.  Argument tables
 * and start vectors go up in one copy, results (and the copies of y asked for) come back in one copy per launch of the
 * eigensolver.  Every other item is served by sdplr_hip_dual_obj_hp on the library's own worker threads, so the call is
 * total; `route` says which of the two served an item (a route-1 item advances out[11] of sdplr_hip_get_stats by one).
 *
 * Results: a route-0 item is bit-identical to sdplr_hip_dual_obj_hp (it is that call).  A route-1 item leaves the same y
 * and S bit for bit; its mineig is that of sdplr_hip_batch_S_eigval's shared launch on that S (bit-identical from run to
 * run and whatever batch it travels in; equal to route 0 to the accuracy the convergence test guarantees).
 *
 * `status` is what sdplr_hip_dual_obj_hp returns for that item (maxiter < 1, an unfinalized handle: that item alone fails
 * and the others are served); the function returns the first non-zero status, or an argument error: handles must be
 * distinct (a duplicate is SDPLR_ERR_INVALID_ARG for the call, and nothing is written) and live on one device.
 * count == 0 is SDPLR_OK.  Without a device both calls return SDPLR_ERR_NO_DEVICE, before any handle or item is looked at.
 *
 * Environment (read per call): SDPLR_HIP_NO_BATCH_EIG=1 sends every item to sdplr_hip_dual_obj_hp;
 * SDPLR_HIP_BATCH_EIG_NMAX lowers the largest n the shared launches take (both as for sdplr_hip_batch_S_eigval).
 */
#ifndef SDPLR_HIP_DUAL_HP_H
#define SDPLR_HIP_DUAL_HP_H

#include "sdplr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* dual_obj(...; highprecision=true)  src/coreop.jl:376-415 (:384, :385, :389-400, :412) */
int32_t sdplr_hip_dual_obj_hp(sdplr_hip_solver* s, double trace_bound, int64_t ncv, double tol,
                              int64_t maxiter, const double* v0, double* dual_value, double* mineig,
                              int64_t* n_matvec, int64_t* n_converged);

typedef struct sdplr_hip_dual_hp_item {   /* sdplr_hip_dual_obj_hp */
  sdplr_hip_solver* s;
  double trace_bound;
  int64_t ncv;
  double tol;
  int64_t maxiter;
  const double* v0;                       /* NULL or [n] */
  double* y_out;                          /* NULL or [m+1]: var.y as the bound leaves it (−λ of the bound, src/sdplr.jl:325) */
  double dual_value, mineig;              /* out */
  int64_t n_matvec, n_converged;          /* out */
  int32_t route;                          /* out: 1 = served by the shared launches, 0 = by sdplr_hip_dual_obj_hp */
  int32_t status;                         /* out: what sdplr_hip_dual_obj_hp returns for this item */
} sdplr_hip_dual_hp_item;
int32_t sdplr_hip_batch_dual_obj_hp(int32_t count, sdplr_hip_dual_hp_item* items);

#ifdef __cplusplus
}
#endif
#endif /* SDPLR_HIP_DUAL_HP_H */

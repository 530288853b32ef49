/*
 * sdplr_hip_eig_batch.h — sdplr_hip_S_eigval (SDP_S_eigval, src/coreop.jl:351-374: the eigenvalue certificate of
 * DIMACS_errors, src/coreop.jl:417-453) for a whole batch of instances in one call, in the form of the lockstep calls of
 * sdplr_hip.h, whose batch conventions hold here too.
 *
 * Each item is exactly the argument list of sdplr_hip_S_eigval.  The small instances of the call share ONE launch: one
 * workgroup per instance runs the same thick-restart Lanczos — the operator on the assembled S, both Gram–Schmidt passes,
 * the projected eigenproblem and the restart — without leaving its CU.  Argument tables and start vectors go up in one copy,
 * all results come back in one copy.  A launch runs at most a fixed number of restart cycles per instance
 * (SDPLR_HIP_BATCH_EIG_CYCLES, default 8); unfinished instances are relaunched from their restart state, which gives bit for
 * bit the iterates of an uncapped run.  Every other item (n or the basis size too large for the kernel's on-chip arrays,
 * more low-rank columns than one register pass takes, a handle with per-kernel profiling on, an instance kept on the
 * multi-launch routes by SDPLR_HIP_FORCE_GRAPH / SDPLR_HIP_NO_RESIDENT) is served by sdplr_hip_S_eigval on the library's own
 * worker threads, so the call is total; `route` says which of the two served an item.
 *
 * Results: a route-0 item is bit-identical to sdplr_hip_S_eigval (it is that call).  A route-1 item is bit-identical from
 * run to run and whatever batch it travels in; it agrees with route 0 to the eigenvalue accuracy the convergence test
 * guarantees, not bitwise (the summation orders differ).
 *
 * `status` is what sdplr_hip_S_eigval returns for that item (nev < 1, null evals, an unfinalized handle: that item alone
 * fails and the others are served); the function returns the first non-zero status, or an argument error: handles must be
 * distinct (a duplicate is SDPLR_ERR_INVALID_ARG for the call, and nothing is written) and live on one device.
 * count == 0 is SDPLR_OK.  Without a device: SDPLR_ERR_NO_DEVICE, before any item is looked at.
 * Per item the call prepares what sdplr_hip_S_eigval prepares (S is assembled if it is stale); no other solver state is
 * written.
 *
 * Environment (read per call): SDPLR_HIP_NO_BATCH_EIG=1 sends every item to sdplr_hip_S_eigval;
 * SDPLR_HIP_BATCH_EIG_NMAX lowers the largest n the shared launch takes.
 */
#ifndef SDPLR_HIP_EIG_BATCH_H
#define SDPLR_HIP_EIG_BATCH_H

#include "sdplr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sdplr_hip_eig_item {       /* sdplr_hip_S_eigval */
  sdplr_hip_solver* s;
  int64_t nev;
  int32_t which;
  int64_t ncv;
  double tol;
  int64_t maxiter;
  const double* v0;                       /* NULL or [n] */
  double* evals;                          /* [nev] */
  int64_t n_matvec, n_converged;          /* out */
  int32_t route;                          /* out: 1 = served by the shared launch, 0 = by sdplr_hip_S_eigval */
  int32_t status;                         /* out: what sdplr_hip_S_eigval returns for this item */
} sdplr_hip_eig_item;
int32_t sdplr_hip_batch_S_eigval(int32_t count, sdplr_hip_eig_item* items);

#ifdef __cplusplus
}
#endif
#endif /* SDPLR_HIP_EIG_BATCH_H */

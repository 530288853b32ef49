/*
 * sdplr_hip_round_batch.h — the rounding of sdplr_hip_round.h for a whole batch of solutions in one call: the step that
 * follows every solve of the reference's batches (exps/batch_test.txt, exps/gen_batch_test.jl; exps/test.jl:71-105 called
 * at :132), in the form of the lockstep calls of sdplr_hip.h, whose batch conventions hold here too.
 *
 * Each item is exactly the argument list of sdplr_hip_round.  The small instances of the call share ONE launch — one
 * workgroup per (instance, block of 64 trials) goes from R to that block's cuts, Γ and the arguments of the whole batch go
 * up as one table, all cuts come back in one copy, and x_best / labels take at most one more launch and one more copy for
 * the whole batch.  Every other item (an instance too large for the kernel's on-chip arrays, a handle with per-kernel
 * profiling on) is served by sdplr_hip_round on the library's own worker threads, so the call is total; `route` says
 * which of the two served an item.  Instances may differ in n, r, graph, trial count, mode and slot.
 *
 * Results are bit-identical to sdplr_hip_round on the same item: cuts (the cut's summation order is the one that call
 * uses, a function of the edge list alone), best, x_best and labels.
 *
 * `status` is what sdplr_hip_round would have returned for that item (no graph, bad mode / slot / trial count, null
 * pointer: that item alone fails and the others are served); the function returns the first non-zero status, or an
 * argument error: handles must be distinct (a duplicate is SDPLR_ERR_INVALID_ARG for the call, and nothing is written)
 * and live on one device.  count == 0 is SDPLR_OK.  Without a device: SDPLR_ERR_NO_DEVICE, before any item is looked at.
 * The call reads solver state and writes none of it.
 *
 * Environment (read per call): SDPLR_HIP_BATCH_ROUND_NMAX lowers the largest n the shared launch takes;
 * SDPLR_HIP_NO_BATCH_ROUND=1 sends every item to sdplr_hip_round.
 */
#ifndef SDPLR_HIP_ROUND_BATCH_H
#define SDPLR_HIP_ROUND_BATCH_H

#include "sdplr_hip_round.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct sdplr_hip_round_item {     /* sdplr_hip_round */
  sdplr_hip_solver* s;
  int32_t mode, slot;
  int64_t trials;
  const double* gauss;                    /* [r_of_that_handle × trials], as sdplr_hip_round */
  double* cuts;                           /* [trials] */
  int64_t best;                           /* out */
  int8_t* x_best;                         /* NULL or [n] */
  int8_t* labels;                         /* NULL or [trials·n] */
  int32_t route;                          /* out: 1 = served by the shared launch, 0 = by sdplr_hip_round */
  int32_t status;                         /* out: what sdplr_hip_round would have returned for this item */
} sdplr_hip_round_item;
int32_t sdplr_hip_batch_round(int32_t count, sdplr_hip_round_item* items);

#ifdef __cplusplus
}
#endif
#endif /* SDPLR_HIP_ROUND_BATCH_H */

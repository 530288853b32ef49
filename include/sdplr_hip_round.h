/*
 * sdplr_hip_round.h — randomized rounding of a solution factor on the device: the callbacks with which the
 * reference's experiment runner finishes every MaxCut and MinimumBisection solve (exps/test.jl:67-105, called at :132).
 * An extension of sdplr_hip.h, whose conventions hold here too: int32 status, borrowed host pointers, IEEE FP64, calls on
 * one handle serialised by the caller, no CPU fallback.
 *
 * Definitions
 *   - projection: z_it = Σ_k R_ik·γ_kt, the products added one after the other for k = 0 … r−1, one rounding per multiply
 *     and per add (a loop over k in any IEEE FP64 arithmetic reproduces z bit for bit).
 *   - mode 0, hyperplane (exps/test.jl:76-87): x_it = −1 if z_it < 0, else +1 (±0.0 give +1).  Best = the first trial with
 *     the largest cut.
 *   - mode 1, bisection (exps/test.jl:89-105): in the order of a stable ascending sort of z_t (−0.0 = 0.0, equal keys by
 *     vertex index) the first ⌊n/2⌋ vertices get +1, the rest −1.  Best = the first trial with the smallest cut.
 *   - cut_t = Σ over the stored edges i < j with x_it ≠ x_jt of a_ij  (= ¼·xᵀLx, exps/test.jl:67-69).  The order of the sum
 *     is a function of the edge list alone: two calls on the same input return the same bits.
 * The library draws no random numbers: the caller supplies the Gaussian vectors.
 */
#ifndef SDPLR_HIP_ROUND_H
#define SDPLR_HIP_ROUND_H

#include "sdplr_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The graph the cuts are scored on (the A of exps/test.jl:71,83), as COO triplets: entries with I < J are kept, all
 * others ignored (pass both triangles of A or the upper one); replaces an earlier graph; survives reset_rank.  An
 * empty edge list is legal (every cut is 0).  After finalize.  An index outside [0, n) after the base shift (kept or
 * ignored entry alike) is SDPLR_ERR_INVALID_ARG.                                                                    */
int32_t sdplr_hip_round_set_graph(sdplr_hip_solver* s, int64_t index_base, int64_t nnz,
                                  const int64_t* I, const int64_t* J, const double* W);

/* maxcut_rounding (mode 0, exps/test.jl:71-81) | minimumbisection_rounding (mode 1, exps/test.jl:83-98) on factor slot
 * `slot` (any SDPLR_F_* the handle holds; r = the handle's current rank).  gauss: r×trials column-major (trial t is r
 * contiguous doubles), 1 ≤ trials ≤ 4096.  cuts[trials]; *best = index of the best trial; x_best NULL or int8[n] (labels
 * of the best trial); labels NULL or int8[trials·n], trial-major (every trial's labels: for tests and small instances).
 * Reads solver state and writes none of it; nothing factor-sized crosses PCIe.
 * SDPLR_ERR_STATE before finalize or before a graph is set; SDPLR_ERR_INVALID_ARG for a bad mode, slot or trial count.  */
int32_t sdplr_hip_round(sdplr_hip_solver* s, int32_t mode, int32_t slot, int64_t trials,
                        const double* gauss, double* cuts, int64_t* best,
                        int8_t* x_best, int8_t* labels);

#ifdef __cplusplus
}
#endif
#endif /* SDPLR_HIP_ROUND_H */

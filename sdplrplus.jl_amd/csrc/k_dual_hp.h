// k_dual_hp.h — the prologue of the high-precision dual bound (dual_obj(...; highprecision=true), src/coreop.jl:384-385,
// :412) for a batch of instances: one workgroup of SDPLR_RS_NT threads per instance (block b ↔ row b of the argument
// table, as k_eig_resident_batch, which follows it on the same stream and reads the y and S.nzval written here).
//
// Per instance, what three launches of the single-instance route do:
//   * y ← −min(λ_ub, λ − σ·primal_vio_raw), y[m] = 1                      (k_copy2y, the same expression per element)
//   * triu_nzval[q] = Σ_e tval[e]·y[tmat[e]] in ascending e                (k_assemble_triu, the same order of terms)
//   * nzval[p] = triu_nzval[mapped[p]]                                     (k_assemble_full)
// so y and S are bit for bit those of enq_copy2y + enq_At_preprocess; and ⟨y[1:m], b⟩ (:412), summed lane → wave →
// workgroup in a fixed order (k_dot / k_reduce_slot group the same products by blocks of SDPLR_NT: this sum alone may
// differ from the single-instance route's, by round-off).
// The three stages read what the stage before wrote through global memory: a workgroup barrier orders them.
#pragma once
#include "common.h"
#include "k_resident.h"

struct DualHpArgs {
  int m, n_sparse, nnzT, nnzS;
  const DevCtrl* c;                          // σ
  const double *lam, *lam_ub, *pv_raw, *b;   // [m]
  double* y;                                 // [m + 1]
  const int *tptr, *tmat, *mapped;           // DevSparse's
  const double* tval;
  double *triu_nzval, *nzval;
  double* yb;                                // the instance's result: ⟨y[1:m], b⟩
  double* y_copy;                            // NULL or [m + 1]: y once more, next to the results (they come back in one copy)
};

__global__ void __launch_bounds__(SDPLR_RS_NT)
k_dual_hp_prologue(const DualHpArgs* __restrict__ items) {
  __shared__ double sred[SDPLR_RS_NW];
  constexpr int NT = SDPLR_RS_NT;
  const DualHpArgs a = items[blockIdx.x];
  const int tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
  const double sigma = a.c->sigma;
  double t = 0.0;
  for (int i = tid; i <= a.m; i += NT) {
    const double yi = (i == a.m) ? 1.0 : -fmin(a.lam_ub[i], a.lam[i] - sigma * a.pv_raw[i]);
    a.y[i] = yi;
    if (a.y_copy) a.y_copy[i] = yi;
    if (i < a.m) t += yi * a.b[i];
  }
  t = wave_sum(t);
  if (ln == 0) sred[wv] = t;
  __syncthreads();   // (y is complete for this workgroup, and so are the wave totals)
  if (tid == 0) {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < SDPLR_RS_NW; i++) s += sred[i];
    *a.yb = s;
  }
  if (a.n_sparse <= 0) return;   // (enq_At_preprocess: nothing to assemble)
  for (int q = tid; q < a.nnzT; q += NT) {
    double v = 0.0;
    for (int e = a.tptr[q]; e < a.tptr[q + 1]; e++) v += a.tval[e] * a.y[a.tmat[e]];
    a.triu_nzval[q] = v;
  }
  __syncthreads();
  for (int p = tid; p < a.nnzS; p += NT) a.nzval[p] = a.triu_nzval[a.mapped[p]];
}

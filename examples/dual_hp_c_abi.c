/* The high-precision dual bound of MaxCut — dual_obj(data, var, aux, trace_bound, iter; highprecision=true),
 * src/coreop.jl:376-415 — through include/sdplr_hip_dual_hp.h from plain C: one instance with sdplr_hip_dual_obj_hp, then
 * two instances with ONE sdplr_hip_batch_dual_obj_hp.
 *
 * Instance k is the circulant graph C_{n_k}(1,…,d_k) with unit weights; the problem is the one of the reference's
 * test/problem.jl:16-30 (C = −¼·L, A_i = e_i e_iᵀ, b_i = 1).  With λ = −1 and primal_vio_raw = 0 (a fresh handle) the bound's
 * y = −min(λ_ub, λ − σ·primal_vio_raw) is (1, …, 1; 1), S = I + C is circulant with the spectrum
 * 1 − d/2 + ½·Σ_t cos(2πjt/n), j = 0 … n − 1, and the bound is −n + trace_bound·min(λ_min, 0) with trace_bound = n.  The
 * program checks both calls against that formula, the copy of y the batch call returns, and that the handle holds y
 * afterwards.
 *
 *   gcc -O2 -Iinclude examples/dual_hp_c_abi.c -Lsdplrplus.jl_amd/lib -lsdplr_hip -lm -o dual_hp_c_abi
 *   LD_LIBRARY_PATH=sdplrplus.jl_amd/lib ./dual_hp_c_abi
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "sdplr_hip_dual_hp.h"

#define CK(call, handle)                                                                             \
  do {                                                                                               \
    int32_t rc__ = (call);                                                                           \
    if (rc__ != SDPLR_OK) {                                                                          \
      fprintf(stderr, "%s -> %d: %s\n", #call, (int)rc__, sdplr_hip_last_error(handle));             \
      return 1;                                                                                      \
    }                                                                                                \
  } while (0)

#define B 2
#define TOL 1e-6

static double exact_mineig(int64_t n, int64_t d) {
  double best = 1e300;
  for (int64_t j = 0; j < n; j++) {
    double lam = 1.0 - 0.5 * (double)d;
    for (int64_t t = 1; t <= d; t++) lam += 0.5 * cos(6.283185307179586 * (double)(j * t) / (double)n);
    if (lam < best) best = lam;
  }
  return best;
}

int main(void) {
  const int64_t r = 2, h = 4;
  const int64_t n[B] = {130, 96}, deg[B] = {3, 2};
  sdplr_hip_solver* s[B] = {NULL, NULL};
  int32_t ndev = 0;
  (void)sdplr_hip_device_count(&ndev);
  printf("%s, %d device(s); %d MaxCut instances\n", sdplr_hip_version(), (int)ndev, B);

  for (int k = 0; k < B; k++) {
    const int64_t nk = n[k], d = deg[k], m = nk;
    const int64_t n_sparse = nk + 1, E = nk + nk * (2 * d + 1);
    int64_t* ent_ptr = malloc((size_t)(n_sparse + 1) * sizeof *ent_ptr);
    int64_t* I = malloc((size_t)E * sizeof *I);
    int64_t* J = malloc((size_t)E * sizeof *J);
    double* V = malloc((size_t)E * sizeof *V);
    int64_t* gids = malloc((size_t)n_sparse * sizeof *gids);
    int64_t e = 0;
    for (int64_t i = 0; i < nk; i++) { /* A_i = e_i e_iᵀ */
      ent_ptr[i] = e;
      gids[i] = i;
      I[e] = J[e] = i;
      V[e++] = 1.0;
    }
    ent_ptr[nk] = e; /* C = −¼(Diag(deg) − A), global index m */
    gids[nk] = m;
    for (int64_t j = 0; j < nk; j++)
      for (int64_t t = -d; t <= d; t++) {
        I[e] = ((j + t) % nk + nk) % nk;
        J[e] = j;
        V[e] = t == 0 ? -0.25 * (double)(2 * d) : 0.25;
        e++;
      }
    ent_ptr[n_sparse] = e;
    CK(sdplr_hip_create(nk, m, r, h, &s[k]), NULL);
    CK(sdplr_hip_set_sparse_coo(s[k], 0, n_sparse, ent_ptr, I, J, V, gids), s[k]);
    CK(sdplr_hip_finalize(s[k]), s[k]);
    free(ent_ptr); free(I); free(J); free(V); free(gids);
    double* v = malloc((size_t)m * sizeof *v);
    for (int64_t i = 0; i < m; i++) v[i] = 1.0;
    CK(sdplr_hip_set_vec(s[k], SDPLR_V_B, v, m), s[k]);
    for (int64_t i = 0; i < m; i++) v[i] = -1.0;
    CK(sdplr_hip_set_vec(s[k], SDPLR_V_LAMBDA, v, m), s[k]);
    CK(sdplr_hip_set_scalar(s[k], SDPLR_S_SIGMA, 2.0), s[k]);
    free(v);
  }

  int ok = 1;
  /* ---- one instance: one call, scalars back ---- */
  double single_dv[B], single_ev[B];
  for (int k = 0; k < B; k++) {
    int64_t mv = 0, nc = 0;
    CK(sdplr_hip_dual_obj_hp(s[k], (double)n[k], 0, TOL, 100000, NULL, &single_dv[k], &single_ev[k], &mv, &nc), s[k]);
    const double exact = exact_mineig(n[k], deg[k]);
    const double want = -(double)n[k] + (double)n[k] * fmin(exact, 0.0);
    const double bound = 2.0 * TOL * fmax(1.0, fabs(exact + 1.0)); /* the convergence test's, on S + I */
    const int good = nc == 1 && fabs(single_ev[k] - exact) <= bound && fabs(single_dv[k] - want) <= (double)n[k] * bound;
    printf("single   %d: n = %4lld  d = %lld  lambda_min = %.12e  (exact %.12e)  dual = %.12e  matvecs = %lld%s\n", k, (long long)n[k],
           (long long)deg[k], single_ev[k], exact, single_dv[k], (long long)mv, good ? "" : "  <-- CHECK FAILED");
    ok = ok && good;
  }

  /* ---- both instances: ONE call; y of each bound comes back with the results ---- */
  sdplr_hip_dual_hp_item it[B];
  double* yout[B];
  for (int k = 0; k < B; k++) {
    yout[k] = calloc((size_t)(n[k] + 1), sizeof **yout);
    it[k].s = s[k];
    it[k].trace_bound = (double)n[k];
    it[k].ncv = 0; /* the default basis: min(n, 100) */
    it[k].tol = TOL;
    it[k].maxiter = 100000;
    it[k].v0 = NULL;
    it[k].y_out = yout[k];
  }
  CK(sdplr_hip_batch_dual_obj_hp(B, it), NULL);
  for (int k = 0; k < B; k++) {
    const double exact = exact_mineig(n[k], deg[k]);
    const double bound = 2.0 * TOL * fmax(1.0, fabs(exact + 1.0));
    double* y = malloc((size_t)(n[k] + 1) * sizeof *y);
    CK(sdplr_hip_get_vec(s[k], SDPLR_V_Y, y, n[k] + 1), s[k]);
    int y_ok = 1;
    for (int64_t i = 0; i <= n[k]; i++) y_ok = y_ok && y[i] == 1.0 && yout[k][i] == 1.0;
    const int good = it[k].status == SDPLR_OK && it[k].n_converged == 1 && y_ok && fabs(it[k].mineig - exact) <= bound &&
                     fabs(it[k].mineig - single_ev[k]) <= bound && fabs(it[k].dual_value - single_dv[k]) <= (double)n[k] * bound;
    printf("instance %d: n = %4lld  d = %lld  lambda_min = %.12e  dual = %.12e  matvecs = %lld  route = %d%s\n", k, (long long)n[k],
           (long long)deg[k], it[k].mineig, it[k].dual_value, (long long)it[k].n_matvec, (int)it[k].route,
           good ? "" : "  <-- CHECK FAILED");
    ok = ok && good;
    free(y); free(yout[k]);
    CK(sdplr_hip_destroy(s[k]), NULL);
  }
  printf("%s\n", ok ? "OK" : "CHECK FAILED");
  return ok ? 0 : 3;
}

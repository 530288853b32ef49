/* The eigenvalue certificate of a handful of small MaxCut instances with ONE sdplr_hip_batch_S_eigval
 * (include/sdplr_hip_eig_batch.h): the smallest eigenvalue of S = C − 𝒜*(λ) that the reference's DIMACS_errors asks
 * SDP_S_eigval for (src/coreop.jl:417-453, :351-374), for the whole batch, through the C ABI alone.
 *
 * Instance k is the circulant graph C_{n_k}(1,…,d_k) with unit weights; the problem is the one of the reference's
 * test/problem.jl:16-30 (C = −¼·L, A_i = e_i e_iᵀ, b_i = 1).  With y = (1, …, 1; 1) the matrix S = I + C is circulant and its
 * spectrum is known in closed form: 1 − d/2 + ½·Σ_t cos(2πjt/n), j = 0 … n − 1.  The program checks the batch call against
 * that formula and against sdplr_hip_S_eigval on the same handle, with which it agrees to the solver's accuracy.
 *
 *   gcc -O2 -Iinclude examples/batch_eig_c_abi.c -Lsdplrplus.jl_amd/lib -lsdplr_hip -lm -o batch_eig_c_abi
 *   LD_LIBRARY_PATH=sdplrplus.jl_amd/lib ./batch_eig_c_abi [B]
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "sdplr_hip_eig_batch.h"

#define CK(call, handle)                                                                             \
  do {                                                                                               \
    int32_t rc__ = (call);                                                                           \
    if (rc__ != SDPLR_OK) {                                                                          \
      fprintf(stderr, "%s -> %d: %s\n", #call, (int)rc__, sdplr_hip_last_error(handle));             \
      return 1;                                                                                      \
    }                                                                                                \
  } while (0)

int main(int argc, char** argv) {
  const int B = argc > 1 ? atoi(argv[1]) : 6;
  const int64_t r = 2, h = 4;
  if (B < 1 || B > 4096) return 2;
  sdplr_hip_solver** s = calloc((size_t)B, sizeof *s);
  int64_t* n = malloc((size_t)B * sizeof *n);
  int64_t* deg = malloc((size_t)B * sizeof *deg);
  int32_t ndev = 0;
  (void)sdplr_hip_device_count(&ndev);
  printf("%s, %d device(s); %d MaxCut instances\n", sdplr_hip_version(), (int)ndev, B);

  for (int k = 0; k < B; k++) {
    const int64_t nk = 96 + 24 * (k % 7) + 8 * (k / 7), d = 2 + k % 3, m = nk;
    n[k] = nk;
    deg[k] = d;
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
    double* y = malloc((size_t)(m + 1) * sizeof *y); /* S = Σ y_i·A_i + y_{m+1}·C = I + C */
    for (int64_t i = 0; i <= m; i++) y[i] = 1.0;
    CK(sdplr_hip_set_vec(s[k], SDPLR_V_Y, y, m + 1), s[k]);
    CK(sdplr_hip_At_preprocess(s[k]), s[k]);
    free(y);
  }

  /* ---- every instance's smallest eigenvalue: ONE call ---- */
  sdplr_hip_eig_item* ei = calloc((size_t)B, sizeof *ei);
  double* ev = malloc((size_t)B * sizeof *ev);
  for (int k = 0; k < B; k++) {
    ei[k].s = s[k];
    ei[k].nev = 1;
    ei[k].which = 0;   /* SA */
    ei[k].ncv = 0;     /* the default basis: min(n, 100) */
    ei[k].tol = 1e-10;
    ei[k].maxiter = 1000;
    ei[k].v0 = NULL;
    ei[k].evals = &ev[k];
  }
  CK(sdplr_hip_batch_S_eigval(B, ei), NULL);

  int ok = 1;
  for (int k = 0; k < B; k++) {
    const int64_t nk = n[k], d = deg[k];
    double exact = 1e300;
    for (int64_t j = 0; j < nk; j++) {
      double lam = 1.0 - 0.5 * (double)d;
      for (int64_t t = 1; t <= d; t++) lam += 0.5 * cos(6.283185307179586 * (double)(j * t) / (double)nk);
      if (lam < exact) exact = lam;
    }
    double one = 0.0;
    int64_t mv = 0, nc = 0;
    CK(sdplr_hip_S_eigval(s[k], 1, 0, 0, 1e-10, 1000, NULL, &one, &mv, &nc), s[k]);
    const double bound = 1e-8 * (1.0 + (double)d); /* ‖S‖∞ ≤ 1 + d */
    const int good = ei[k].status == SDPLR_OK && ei[k].n_converged == 1 && nc == 1 && fabs(ev[k] - exact) <= bound &&
                     fabs(ev[k] - one) <= bound;
    printf("instance %2d: n = %4lld  d = %lld  lambda_min = %.15e  (exact %.15e)  matvecs = %lld  route = %d%s\n", k, (long long)nk,
           (long long)d, ev[k], exact, (long long)ei[k].n_matvec, (int)ei[k].route, good ? "" : "  <-- CHECK FAILED");
    ok = ok && good;
    CK(sdplr_hip_destroy(s[k]), NULL);
  }
  free(ev); free(ei); free(s); free(n); free(deg);
  printf("%s\n", ok ? "OK" : "CHECK FAILED");
  return ok ? 0 : 3;
}

/* A MaxCut SDP solved and ROUNDED through the C ABI alone: the solve of examples/maxcut_c_abi.c (the circulant
 * C_n(1,2,3), the problem of the reference's test/problem.jl:16-30, driven by the skeleton of _sdplr, src/sdplr.jl:140-449)
 * followed by what the reference's runner does with the solution (exps/test.jl:71-81, called at :132): 100 random
 * hyperplanes through R, each scored by its cut, the best one kept.  The factor never leaves the device: the graph goes
 * up once (sdplr_hip_round_set_graph), the Gaussian vectors go up per call, the cuts and the best labelling come back
 * (include/sdplr_hip_round.h).  The library draws no random numbers; the vectors here are sums of twelve uniforms.
 *
 *   gcc -O2 -Iinclude examples/round_c_abi.c -Lsdplrplus.jl_amd/lib -lsdplr_hip -lm -o round_c_abi
 *   LD_LIBRARY_PATH=sdplrplus.jl_amd/lib ./round_c_abi [n] [r] [dump]
 *
 * dump: a file that receives n, r, T as three int64 and then R (n·r doubles, row i contiguous) and Γ (T·r doubles, trial t
 * contiguous) — what a checker needs to redo the rounding on the host.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "sdplr_hip.h"
#include "sdplr_hip_round.h"

#define CK(call)                                                                                     \
  do {                                                                                               \
    int32_t rc__ = (call);                                                                           \
    if (rc__ != SDPLR_OK) {                                                                          \
      fprintf(stderr, "%s -> %d: %s\n", #call, (int)rc__, sdplr_hip_last_error(s));                  \
      return 1;                                                                                      \
    }                                                                                                \
  } while (0)

#define TRIALS 100

static int cmp_i64(const void* a, const void* b) {
  const int64_t x = *(const int64_t*)a, y = *(const int64_t*)b;
  return (x > y) - (x < y);
}

static uint64_t rng_state = 88172645463325252ull;
static double uniform01(void) {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (double)(rng_state >> 11) / 9007199254740992.0;
}

int main(int argc, char** argv) {
  const int64_t n = argc > 1 ? atoll(argv[1]) : 4096, r = argc > 2 ? atoll(argv[2]) : 8, m = n, h = 4;
  const char* dump = argc > 3 ? argv[3] : NULL;
  sdplr_hip_solver* s = NULL;
  if (n < 8) return 2;

  /* ---- the SDP as COO triplets: A_k = e_k e_kᵀ (k < n), then C = −¼(6·I − A), both triangles (set_sparse_coo builds
   *      the aggregated layout of src/preprocess.jl:24-169 inside the library) ---- */
  const int64_t nnzC = 7 * n, nnz = n + nnzC;
  int64_t* ent_ptr = malloc((size_t)(n + 2) * sizeof *ent_ptr);
  int64_t* I = malloc((size_t)nnz * sizeof *I);
  int64_t* J = malloc((size_t)nnz * sizeof *J);
  double* V = malloc((size_t)nnz * sizeof *V);
  int64_t* gids = malloc((size_t)(n + 1) * sizeof *gids);
  /* ---- the graph itself, both triangles: entries with I < J are the edges the cuts are scored on ---- */
  int64_t* gi = malloc((size_t)(6 * n) * sizeof *gi);
  int64_t* gj = malloc((size_t)(6 * n) * sizeof *gj);
  double* gw = malloc((size_t)(6 * n) * sizeof *gw);
  int64_t e = 0, ge = 0;
  for (int64_t k = 0; k < n; k++) {
    ent_ptr[k] = e;
    gids[k] = k;
    I[e] = J[e] = k;
    V[e++] = 1.0;
  }
  ent_ptr[n] = e;
  gids[n] = m;
  for (int64_t j = 0; j < n; j++) {   /* column j: rows j and j ± 1, 2, 3 (mod n), ascending (findnz order) */
    int64_t rows[7];
    for (int d = -3; d <= 3; d++) rows[d + 3] = ((j + d) % n + n) % n;
    qsort(rows, 7, sizeof rows[0], cmp_i64);
    for (int q = 0; q < 7; q++) {
      const int64_t i = rows[q];
      I[e] = i;
      J[e] = j;
      V[e++] = i == j ? -0.25 * 6.0 : 0.25;
      if (i != j) { gi[ge] = i; gj[ge] = j; gw[ge++] = 1.0; }
    }
  }
  ent_ptr[n + 1] = e;

  int32_t ndev = 0;
  (void)sdplr_hip_device_count(&ndev);
  printf("%s, %d device(s); MaxCut on C_%lld(1,2,3), r = %lld, then %d random hyperplanes\n", sdplr_hip_version(), (int)ndev,
         (long long)n, (long long)r, TRIALS);
  CK(sdplr_hip_create(n, m, r, h, &s));
  CK(sdplr_hip_set_sparse_coo(s, 0, n + 1, ent_ptr, I, J, V, gids));
  CK(sdplr_hip_finalize(s));

  double* R = malloc((size_t)(n * r) * sizeof *R);
  double* b = malloc((size_t)m * sizeof *b);
  for (int64_t i = 0; i < n * r; i++) R[i] = 2.0 * uniform01() - 1.0;
  for (int64_t i = 0; i < m; i++) b[i] = 1.0;
  CK(sdplr_hip_set_factor(s, SDPLR_F_RT, R));
  CK(sdplr_hip_set_vec(s, SDPLR_V_B, b, m));
  const double normC = sqrt((double)n * (1.5 * 1.5 + 6 * 0.25 * 0.25)), normb = sqrt((double)m);

  double L, gnorm, pvnorm, alpha, obj = 0.0, sigma = 2.0;
  int64_t iters;
  int32_t reason;
  for (int major = 1; major <= 8; major++) {   /* λ update from the second round on, σ doubling: src/sdplr.jl:358-369 */
    CK(sdplr_hip_major_iteration(s, normC, normb, 1, 1, 0, major > 1, sigma, 1e-3 / major, 1e8 * 2.220446049250313e-16, 2000,
                                 0.0, &L, &gnorm, &pvnorm, &alpha, &iters, &reason));
    sigma *= 2.0;
  }
  CK(sdplr_hip_get_scalar(s, SDPLR_S_OBJ, &obj));
  printf("solved: obj = %.6f  |grad| = %.2e  |pv| = %.2e\n", obj, gnorm, pvnorm);

  /* ---- the rounding: graph up once, Γ up, cuts and the best labelling back ---- */
  double* gauss = malloc((size_t)(TRIALS * r) * sizeof *gauss);
  double* cuts = malloc(TRIALS * sizeof *cuts);
  int8_t* x = malloc((size_t)n);
  for (int64_t i = 0; i < TRIALS * r; i++) {
    double t = -6.0;
    for (int q = 0; q < 12; q++) t += uniform01();
    gauss[i] = t;
  }
  int64_t best = -1;
  CK(sdplr_hip_round_set_graph(s, 0, ge, gi, gj, gw));
  CK(sdplr_hip_round(s, 0, SDPLR_F_RT, TRIALS, gauss, cuts, &best, x, NULL));
  /* the labels that came back cut what the library says they cut */
  double check = 0.0;
  for (int64_t k = 0; k < ge; k++)
    if (gi[k] < gj[k] && x[gi[k]] != x[gj[k]]) check += gw[k];
  int ok = best >= 0 && best < TRIALS && check == cuts[best];
  for (int t = 0; t < TRIALS; t++) ok = ok && cuts[t] <= cuts[best];
  /* −obj is the SDP's bound on the maximum cut (C = −¼L); a hyperplane cut of a near-optimal R keeps ≥ 0.878 of it in
   * expectation (Goemans–Williamson), and the best of 100 is asked for 0.8; R is converged to a few per cent */
  ok = ok && cuts[best] <= -obj * 1.03 && cuts[best] >= 0.8 * -obj;
  printf("best cut = %.17g (trial %lld), SDP bound %.6f, ratio %.4f  ->  %s\n", cuts[best], (long long)best, -obj,
         cuts[best] / -obj, ok ? "OK" : "CHECK FAILED");
  if (dump) {
    CK(sdplr_hip_get_factor(s, SDPLR_F_RT, R));
    FILE* f = fopen(dump, "wb");
    const int64_t hdr[3] = {n, r, TRIALS};
    if (!f) return 4;
    fwrite(hdr, sizeof hdr[0], 3, f);
    fwrite(R, sizeof *R, (size_t)(n * r), f);
    fwrite(gauss, sizeof *gauss, (size_t)(TRIALS * r), f);
    fclose(f);
  }
  CK(sdplr_hip_destroy(s));
  return ok ? 0 : 3;
}

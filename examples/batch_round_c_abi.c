/* A handful of small MaxCut SDPs solved side by side with the lockstep calls of include/sdplr_hip.h (as
 * examples/batch_c_abi.c does), then ROUNDED with one sdplr_hip_batch_round (include/sdplr_hip_round_batch.h): the
 * reference's batch line — a solve followed by its rounding callback (exps/batch_test.txt, exps/test.jl:71-81 called at
 * :132) — for the whole batch, through the C ABI alone.
 *
 * Instance k is the circulant graph C_{n_k}(1,…,d_k) with unit weights; the problem is the one of the reference's
 * test/problem.jl:16-30 (C = −¼·L, A_i = e_i e_iᵀ, b_i = 1).  Six rounds of [λ update → σ doubles → fg! → inner loop] are
 * one sdplr_hip_batch_major_iteration each; then every instance's graph is set once (sdplr_hip_round_set_graph), the
 * Gaussian vectors are drawn on the host, and one call returns every instance's cuts, its best trial and that trial's
 * labels.  The program checks each best cut against the labels it got back, and against sdplr_hip_round on the same
 * handle, with which the batch call agrees bit for bit.
 *
 *   gcc -O2 -Iinclude examples/batch_round_c_abi.c -Lsdplrplus.jl_amd/lib -lsdplr_hip -lm -o batch_round_c_abi
 *   LD_LIBRARY_PATH=sdplrplus.jl_amd/lib ./batch_round_c_abi [B] [r] [trials]
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "sdplr_hip_round_batch.h"

#define CK(call, handle)                                                                             \
  do {                                                                                               \
    int32_t rc__ = (call);                                                                           \
    if (rc__ != SDPLR_OK) {                                                                          \
      fprintf(stderr, "%s -> %d: %s\n", #call, (int)rc__, sdplr_hip_last_error(handle));             \
      return 1;                                                                                      \
    }                                                                                                \
  } while (0)

static uint64_t rng_state = 88172645463325252ull;
static double uniform01(void) {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (double)((rng_state >> 11) + 1) / 9007199254740993.0; /* in (0, 1) */
}
static double gaussian(void) { /* Box–Muller */
  const double u = uniform01(), v = uniform01();
  return sqrt(-2.0 * log(u)) * cos(6.283185307179586 * v);
}

int main(int argc, char** argv) {
  const int B = argc > 1 ? atoi(argv[1]) : 6;
  const int64_t r = argc > 2 ? atoll(argv[2]) : 6, h = 4;
  const int64_t T = argc > 3 ? atoll(argv[3]) : 100;
  if (B < 1 || B > 4096 || r < 1 || T < 1 || T > 4096) return 2;
  sdplr_hip_solver** s = calloc((size_t)B, sizeof *s);
  int64_t* n = malloc((size_t)B * sizeof *n);
  int64_t* deg = malloc((size_t)B * sizeof *deg);
  double* normC = malloc((size_t)B * sizeof *normC);
  int32_t ndev = 0;
  (void)sdplr_hip_device_count(&ndev);
  printf("%s, %d device(s); %d MaxCut instances, r = %lld, %lld trials each\n", sdplr_hip_version(), (int)ndev, B, (long long)r,
         (long long)T);

  /* ---- set-up, instance by instance ---- */
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
    double c2 = 0.0;
    for (int64_t j = 0; j < nk; j++)
      for (int64_t t = -d; t <= d; t++) {
        I[e] = ((j + t) % nk + nk) % nk;
        J[e] = j;
        V[e] = t == 0 ? -0.25 * (double)(2 * d) : 0.25;
        c2 += V[e] * V[e];
        e++;
      }
    ent_ptr[n_sparse] = e;
    normC[k] = sqrt(c2);
    CK(sdplr_hip_create(nk, m, r, h, &s[k]), NULL);
    CK(sdplr_hip_set_sparse_coo(s[k], 0, n_sparse, ent_ptr, I, J, V, gids), s[k]);
    CK(sdplr_hip_finalize(s[k]), s[k]);
    free(ent_ptr); free(I); free(J); free(V); free(gids);
    double* R = malloc((size_t)(nk * r) * sizeof *R);
    double* b = malloc((size_t)m * sizeof *b);
    for (int64_t i = 0; i < nk * r; i++) R[i] = 2.0 * uniform01() - 1.0;
    for (int64_t i = 0; i < m; i++) b[i] = 1.0;
    CK(sdplr_hip_set_factor(s[k], SDPLR_F_RT, R), s[k]);
    CK(sdplr_hip_set_vec(s[k], SDPLR_V_B, b, m), s[k]);
    CK(sdplr_hip_set_scalar(s[k], SDPLR_S_SIGMA, 2.0), s[k]);
    free(R); free(b);
  }

  /* ---- the solves, in lockstep ---- */
  sdplr_hip_major_item* mi = calloc((size_t)B, sizeof *mi);
  double sigma = 2.0;
  for (int major = 1; major <= 6; major++) {
    for (int k = 0; k < B; k++) {
      mi[k].s = s[k];
      mi[k].normC = normC[k];
      mi[k].normb = sqrt((double)n[k]);
      mi[k].gtol_relative = mi[k].ptol_relative = 1;
      mi[k].use_armijo = 0;
      mi[k].update_lambda = major > 1;
      mi[k].sigma = sigma;
      mi[k].cur_gtol = 1e-3 / major;
      mi[k].fprec_eps = 1e8 * 2.220446049250313e-16;
      mi[k].max_local_iters = 2000;
      mi[k].time_budget_s = 0.0;
    }
    CK(sdplr_hip_batch_major_iteration(B, mi), NULL);
    sigma *= 2.0;
  }

  /* ---- the roundings: each graph once, the draws on the host, ONE call ---- */
  sdplr_hip_round_item* ri = calloc((size_t)B, sizeof *ri);
  double** gauss = malloc((size_t)B * sizeof *gauss);
  for (int k = 0; k < B; k++) {
    const int64_t nk = n[k], d = deg[k], E = nk * d;
    int64_t* I = malloc((size_t)E * sizeof *I);
    int64_t* J = malloc((size_t)E * sizeof *J);
    double* W = malloc((size_t)E * sizeof *W);
    int64_t e = 0;
    for (int64_t j = 0; j < nk; j++)
      for (int64_t t = 1; t <= d; t++) { /* each edge once; the library keeps the entries with I < J */
        const int64_t a = j, c = (j + t) % nk;
        I[e] = a < c ? a : c;
        J[e] = a < c ? c : a;
        W[e++] = 1.0;
      }
    CK(sdplr_hip_round_set_graph(s[k], 0, E, I, J, W), s[k]);
    free(I); free(J); free(W);
    gauss[k] = malloc((size_t)(r * T) * sizeof **gauss);
    for (int64_t i = 0; i < r * T; i++) gauss[k][i] = gaussian();
    ri[k].s = s[k];
    ri[k].mode = 0; /* hyperplane rounding, exps/test.jl:71-81 */
    ri[k].slot = SDPLR_F_RT;
    ri[k].trials = T;
    ri[k].gauss = gauss[k];
    ri[k].cuts = malloc((size_t)T * sizeof(double));
    ri[k].x_best = malloc((size_t)nk);
    ri[k].labels = NULL;
  }
  CK(sdplr_hip_batch_round(B, ri), NULL);

  /* ---- checks: the best cut is the cut of the labels returned, and what sdplr_hip_round returns, bit for bit ---- */
  int ok = 1;
  double* cuts1 = malloc((size_t)T * sizeof *cuts1);
  for (int k = 0; k < B; k++) {
    const int64_t nk = n[k], d = deg[k];
    double cut = 0.0;
    for (int64_t j = 0; j < nk; j++)
      for (int64_t t = 1; t <= d; t++)
        if (ri[k].x_best[j] != ri[k].x_best[(j + t) % nk]) cut += 1.0;
    int64_t best1 = -1;
    CK(sdplr_hip_round(s[k], 0, SDPLR_F_RT, T, gauss[k], cuts1, &best1, NULL, NULL), s[k]);
    int same = best1 == ri[k].best;
    for (int64_t t = 0; t < T; t++) same = same && cuts1[t] == ri[k].cuts[t];
    const double best_cut = ri[k].cuts[ri[k].best];
    const int good = ri[k].status == SDPLR_OK && same && cut == best_cut && best_cut > 0.5 * (double)(nk * d);
    printf("instance %2d: n = %4lld  %lld edges  best cut = %.1f (trial %lld)  route = %d%s\n", k, (long long)nk,
           (long long)(nk * d), best_cut, (long long)ri[k].best, (int)ri[k].route, good ? "" : "  <-- CHECK FAILED");
    ok = ok && good;
    CK(sdplr_hip_destroy(s[k]), NULL);
    free(gauss[k]); free(ri[k].cuts); free(ri[k].x_best);
  }
  free(cuts1); free(gauss); free(ri); free(mi); free(s); free(n); free(deg); free(normC);
  printf("%s\n", ok ? "OK" : "CHECK FAILED");
  return ok ? 0 : 3;
}

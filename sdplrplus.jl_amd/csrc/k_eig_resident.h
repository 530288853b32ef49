// k_eig_resident.h — the RESIDENT form of the thick-restart Lanczos of sdplr_hip_S_eigval (SDP_S_eigval,
// src/coreop.jl:351-374): one workgroup of SDPLR_RS_NT threads owns one instance for whole restart cycles, a batch of
// instances is one grid (block b ↔ row b of the argument table, as the k_rs_*_batch kernels of k_resident.h).
//
// The multi-launch form is about nine launches per Lanczos step on 6 KB vectors and a host Jacobi per restart cycle.
// Here a cycle never leaves the CU:
//   * v_j and w live in LDS; the basis [m + 1][ldv] and its restart twin live in global memory (2 × 650 KB at n = 800,
//     m = 100: the XCD's L2);
//   * w = S·v_j on the assembled S (CSC of the full pattern + the low-rank terms), as k_rs_lanczos applies it;
//   * classical Gram–Schmidt twice against V[0..j]: one wave per basis vector forms ⟨V_i, w⟩ (lanes stride over n), then one
//     thread per element subtracts Σ h_i·V_i;
//   * the projected matrix T lives in LDS as a packed upper triangle (m(m + 1)/2 doubles); its eigenvector matrix Y lives in
//     LDS too when both fit (EigResArgs::ylds), else in the item's global scratch;
//   * the projected eigenproblem is a PARALLEL Jacobi: the m(m − 1)/2 pairs are taken in m − 1 rounds of ⌊m/2⌋ disjoint
//     pairs (the round-robin tournament, a fixed schedule); within a round every 2×2 block (pair i, pair j), i ≤ j, of
//     Jᵀ·T·J belongs to one thread, which reads and writes only that block — no barrier between the two sides of the
//     rotation.  Stopping rule and sweep limit are the host's: off² ≤ 1e-30·‖T‖²_F, 60 sweeps;
//   * every sum is formed in a fixed order (lane → wave → workgroup); nothing depends on the block's position in the grid.
//
// A launch runs at most `cap` restart cycles of an instance (SDPLR_EIG_RS_CYCLES by default: a launch on a shared GPU
// stays bounded whatever maxiter says).  The restart state — the kept Ritz vectors (the current basis), their θ, k, the
// cycle and matvec counters — lives in the item's global scratch (`state`); the next launch continues from it, so the
// iterates are bit for bit those of an uncapped run.
#pragma once
#include "common.h"
#include "k_resident.h"

#ifndef SDPLR_EIG_RS_CYCLES
#define SDPLR_EIG_RS_CYCLES 8      /* restart cycles per launch and instance (SDPLR_HIP_BATCH_EIG_CYCLES overrides) */
#endif
#define SDPLR_EIG_RS_SWEEPS 60     /* Jacobi sweep limit (jacobi_eigh's) */
#define SDPLR_EIG_RS_TILE 8        /* Ritz vectors per pass of the restart rotation */

// state block of an item (doubles; the counters are integers far below 2^53)
enum { EIG_ST_STARTED = 0, EIG_ST_K, EIG_ST_CYCLE, EIG_ST_MATVECS, EIG_ST_CUR, EIG_ST_DONE, EIG_ST_NCONV, EIG_ST_THETA = 8 };

struct EigResArgs {
  int n, m, nev, which;    // which: 0 = SA, 1 = LA
  int ylds, cap;           // Y in LDS; restart cycles per launch
  long long maxiter, ldv;
  double tol, eps23;       // (tol > 0 already; eps^(2/3) as the host's pow gives it)
  const int *colptr, *rowval;
  const double* nzval;
  DevLowRank lr;
  const double* yvec;
  const double* v0;        // [n] start vector
  double* V[2];            // the two bases [m + 1][ldv]
  double* Yg;              // [m][m] (when !ylds)
  double* state;           // [EIG_ST_THETA + m]
  double* out;             // [nev] eigenvalues, then n_matvec, n_converged
};

__host__ __device__ inline long long eig_rs_tri(long long m) { return m * (m + 1) / 2; }
// doubles of dynamic LDS: v, w (n rounded to even), T packed, Y, h[m + 1], β[m], d[m], the rotations (c, s per pair), ord[m] (ints)
__host__ __device__ inline long long eig_rs_lds_doubles(long long n, long long m, bool ylds) {
  const long long npad = (n + 1) & ~1LL, mp = (m + 2) & ~1LL;
  return 2 * npad + ((eig_rs_tri(m) + 1) & ~1LL) + (ylds ? m * mp : 0) + 5 * mp;
}

__device__ __forceinline__ int eig_rs_tix(int i, int j, int m) {   // packed position of T(i, j), any order
  const int a = i < j ? i : j, b = i < j ? j : i;
  return a * (2 * m - a + 1) / 2 + (b - a);
}
// pair i of round `round` of the round-robin tournament on M2 players (M2 even): p < q
__device__ __forceinline__ void eig_rs_pair(int round, int i, int M2, int& p, int& q) {
  const int N1 = M2 - 1;
  int x, y;
  if (i == 0) { x = N1; y = round; }
  else { x = (round + i) % N1; y = (round + N1 - i) % N1; }
  p = x < y ? x : y;
  q = x < y ? y : x;
}

__device__ __forceinline__ void eig_rs_run(const EigResArgs& a) {
  extern __shared__ __attribute__((aligned(16))) double rs_lds[];
  __shared__ double sred[SDPLR_RS_NW];
  __shared__ int sh_i[4];
  constexpr int NT = SDPLR_RS_NT, LPR = SDPLR_RS_LZ_LPR, G = NT / LPR;
  const int tid = threadIdx.x, wv = tid >> 6, ln = tid & 63;
  const int n = a.n, m = a.m, nev = a.nev;
  const long long ldv = a.ldv;
  double* st = a.state;
  if (st[EIG_ST_DONE] != 0.0) return;
  const int npad = (n + 1) & ~1, mp = (m + 2) & ~1;
  double* v = rs_lds;
  double* w = v + npad;
  double* T = w + npad;
  double* Yl = T + ((eig_rs_tri(m) + 1) & ~1LL);
  double* h = Yl + (a.ylds ? (long long)m * mp : 0);
  double* beta = h + mp;
  double* d = beta + mp;
  double* rot = d + mp;                              // c of pair i at rot[2i], s at rot[2i + 1]
  int* ord = reinterpret_cast<int*>(rot + mp);       // ord[r] = column of the r-th smallest Ritz value
  const int ldy = a.ylds ? mp : m;
  auto bsum = [&](double x) -> double {   // block sum, every thread gets it (fixed order)
    x = wave_sum(x);
    __syncthreads();
    if (ln == 0) sred[wv] = x;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < SDPLR_RS_NW; i++) t += sred[i];
    return t;
  };
  int k = (int)st[EIG_ST_K], cur = (int)st[EIG_ST_CUR];
  long long cycle = (long long)st[EIG_ST_CYCLE], matvecs = (long long)st[EIG_ST_MATVECS];
  const bool started = st[EIG_ST_STARTED] != 0.0;
  double* V = a.V[cur];
  double* V2 = a.V[cur ^ 1];
  if (!started) {   // V[0] = v0/‖v0‖
    double s = 0.0;
    for (int i = tid; i < n; i += NT) {
      const double x = a.v0[i];
      v[i] = x;
      s += x * x;
    }
    const double nv = sqrt(bsum(s));
    const double inv = nv > 0.0 ? 1.0 / nv : 0.0;
    for (int i = tid; i < n; i += NT) {
      const double x = v[i] * inv;
      v[i] = x;
      V[i] = x;
    }
  } else {
    for (int i = tid; i < n; i += NT) v[i] = V[(long long)k * ldv + i];
  }
  for (int e = tid; e < (int)eig_rs_tri(m); e += NT) T[e] = 0.0;
  __syncthreads();
  for (int i = tid; i < k; i += NT) T[eig_rs_tix(i, i, m)] = st[EIG_ST_THETA + i];
  __syncthreads();

  for (int lc = 0; lc < a.cap; lc++) {
    // ---- Lanczos steps j = k .. m − 1 with full re-orthogonalisation ----
    for (int j = k; j < m; j++) {
      double coef[SDPLR_LRMAX];   // low-rank coefficients y[gid]·D_c·⟨B_c, v⟩ (src/structs.jl:117-127)
#pragma unroll
      for (int cc = 0; cc < SDPLR_LRMAX; cc++) {
        coef[cc] = 0.0;
        if (cc < a.lr.ST) {
          double s = 0.0;
          for (int i = tid; i < n; i += NT) s += a.lr.Bcat[(long long)cc * n + i] * v[i];
          coef[cc] = a.yvec[a.lr.col_gid[cc]] * a.lr.Dcat[cc] * bsum(s);
        }
      }
      {   // w = S·v
        const int grp = tid / LPR, lane = tid % LPR;
        for (int row = grp; row < n; row += G) {
          const int beg = a.colptr[row], end = a.colptr[row + 1];
          double tj = 0.0;
          for (int p = beg + lane; p < end; p += LPR) tj += a.nzval[p] * v[a.rowval[p]];
          tj = group_sum<LPR>(tj);
          if (lane == 0) {
#pragma unroll
            for (int cc = 0; cc < SDPLR_LRMAX; cc++)
              if (cc < a.lr.ST) tj += coef[cc] * a.lr.Bcat[(long long)cc * n + row];
            w[row] = tj;
          }
        }
      }
      __syncthreads();
      for (int pass = 0; pass < 2; pass++) {   // classical Gram–Schmidt, twice
        for (int i = wv; i <= j; i += SDPLR_RS_NW) {
          const double* Vi = V + (long long)i * ldv;
          double s = 0.0;
#pragma unroll 4
          for (int p = ln; p < n; p += 64) s += Vi[p] * w[p];
          s = wave_sum(s);
          if (ln == 0) {
            h[i] = s;
            const int t = eig_rs_tix(i, j, m);
            T[t] = pass ? T[t] + s : s;
          }
        }
        __syncthreads();
        for (int p = tid; p < n; p += NT) {
          double acc = w[p];
#pragma unroll 8
          for (int i = 0; i <= j; i++) acc -= h[i] * V[(long long)i * ldv + p];
          w[p] = acc;
        }
        __syncthreads();
      }
      double nn = 0.0;
      for (int p = tid; p < n; p += NT) nn += w[p] * w[p];
      const double be = sqrt(bsum(nn));
      const double inv = be > 1e-300 ? 1.0 / be : 0.0;   // (zero at round-off level: invariant subspace)
      if (tid == 0) beta[j] = be;
      double* Vn = V + (long long)(j + 1) * ldv;
      for (int p = tid; p < n; p += NT) {
        const double x = w[p] * inv;
        w[p] = x;
        Vn[p] = x;
      }
      matvecs++;
      double* t = v; v = w; w = t;
      __syncthreads();
    }
    // ---- the invariant-subspace rule (thread 0: m values) ----
    if (tid == 0) {
      double tnorm = 0.0;
      for (int i = 0; i < m; i++) tnorm = fmax(tnorm, fabs(T[eig_rs_tix(i, i, m)]));
      int me = m;
      for (int j = k; j < m - 1; j++)
        if (beta[j] <= 1e-13 * fmax(tnorm, 1e-300)) { me = j + 1; break; }
      sh_i[0] = me;
    }
    __syncthreads();
    const int meff = sh_i[0];
    // ---- eigen-decomposition of the leading meff × meff block: parallel Jacobi, eigenvectors as ROWS of Y ----
    auto y_init = [&](double* Y) {
      for (int e = tid; e < meff * meff; e += NT) {
        const int i = e / meff, l = e - i * meff;
        Y[(long long)i * ldy + l] = i == l ? 1.0 : 0.0;
      }
    };
    if (a.ylds) y_init(Yl); else y_init(a.Yg);
    const int M2 = meff + (meff & 1), np = M2 / 2;
    for (int sweep = 0; sweep < SDPLR_EIG_RS_SWEEPS; sweep++) {
      double off = 0.0, diag = 0.0;
      for (int e = tid; e < meff * meff; e += NT) {
        const int i = e / meff, l = e - i * meff;
        const double x = T[eig_rs_tix(i, l, m)];
        if (i == l) diag += x * x; else off += x * x;
      }
      off = bsum(off);
      diag = bsum(diag);
      if (off <= 1e-30 * (diag + off) || off == 0.0) break;
      for (int round = 0; round < M2 - 1; round++) {
        for (int i = tid; i < np; i += NT) {
          int p, q;
          eig_rs_pair(round, i, M2, p, q);
          double c = 1.0, sn = 0.0;
          if (q < meff) {
            const double apq = T[eig_rs_tix(p, q, m)];
            if (apq != 0.0) {
              const double app = T[eig_rs_tix(p, p, m)], aqq = T[eig_rs_tix(q, q, m)];
              const double theta = (aqq - app) / (2.0 * apq);
              const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
              c = 1.0 / sqrt(t * t + 1.0);
              sn = t * c;
            }
          }
          rot[2 * i] = c;
          rot[2 * i + 1] = sn;
        }
        __syncthreads();
        for (int b = tid; b < np * np; b += NT) {   // T ← Jᵀ·T·J, block (pair i, pair j), i ≤ j
          const int i = b / np, jj = b - i * np;
          if (i > jj) continue;
          int p, q, u, vv;
          eig_rs_pair(round, i, M2, p, q);
          const double ci = rot[2 * i], si = rot[2 * i + 1];
          if (i == jj) {
            if (q >= meff) continue;
            const int tpp = eig_rs_tix(p, p, m), tqq = eig_rs_tix(q, q, m), tpq = eig_rs_tix(p, q, m);
            const double app = T[tpp], aqq = T[tqq], apq = T[tpq];
            const double b00 = ci * app - si * apq, b01 = si * app + ci * apq;   // B·J
            const double b10 = ci * apq - si * aqq, b11 = si * apq + ci * aqq;
            T[tpp] = ci * b00 - si * b10;                                        // Jᵀ·(B·J)
            T[tqq] = si * b01 + ci * b11;
            T[tpq] = 0.0;
            continue;
          }
          eig_rs_pair(round, jj, M2, u, vv);
          const double cj = rot[2 * jj], sj = rot[2 * jj + 1];
          const bool qv = q < meff, vvv = vv < meff;
          const int tpu = eig_rs_tix(p, u, m), tpv = vvv ? eig_rs_tix(p, vv, m) : tpu;
          const int tqu = qv ? eig_rs_tix(q, u, m) : tpu, tqv = qv && vvv ? eig_rs_tix(q, vv, m) : tpu;
          const double apu = T[tpu], apv = vvv ? T[tpv] : 0.0, aqu = qv ? T[tqu] : 0.0, aqv = qv && vvv ? T[tqv] : 0.0;
          const double b00 = cj * apu - sj * apv, b01 = sj * apu + cj * apv;
          const double b10 = cj * aqu - sj * aqv, b11 = sj * aqu + cj * aqv;
          T[tpu] = ci * b00 - si * b10;
          if (vvv) T[tpv] = ci * b01 - si * b11;
          if (qv) T[tqu] = si * b00 + ci * b10;
          if (qv && vvv) T[tqv] = si * b01 + ci * b11;
        }
        auto y_rot = [&](double* Y) {   // rows p, q of Y
          for (int e = tid; e < np * meff; e += NT) {
            const int i = e / meff, l = e - i * meff;
            int p, q;
            eig_rs_pair(round, i, M2, p, q);
            if (q >= meff) continue;
            const double c = rot[2 * i], sn = rot[2 * i + 1];
            double* yp = Y + (long long)p * ldy + l;
            double* yq = Y + (long long)q * ldy + l;
            const double x = *yp, y = *yq;
            *yp = c * x - sn * y;
            *yq = sn * x + c * y;
          }
        };
        if (a.ylds) y_rot(Yl); else y_rot(a.Yg);
        __syncthreads();
      }
    }
    // ---- Ritz values ascending (rank sort; ties by column) ----
    for (int i = tid; i < meff; i += NT) d[i] = T[eig_rs_tix(i, i, m)];
    __syncthreads();
    for (int i = tid; i < meff; i += NT) {
      const double x = d[i];
      int r = 0;
      for (int l = 0; l < meff; l++) {
        const double y = d[l];
        r += (y < x || (y == x && l < i)) ? 1 : 0;
      }
      ord[r] = i;
    }
    __syncthreads();
    // ---- ARPACK's convergence test on the shifted operator S + I (:365-366) ----
    const int nw = nev < meff ? nev : meff;
    if (tid == 0) {
      const double bres = meff == m ? beta[m - 1] : 0.0;
      int nconv = 0;
      for (int i = 0; i < nw; i++) {
        const int col = ord[a.which == 0 ? i : meff - 1 - i];
        const double yl = a.ylds ? Yl[(long long)col * ldy + (meff - 1)] : a.Yg[(long long)col * ldy + (meff - 1)];
        const double res = fabs(bres * yl);
        if (res <= a.tol * fmax(a.eps23, fabs(d[col] + 1.0))) nconv++;
        else break;
      }
      const int fin = nconv >= nev || meff < m || meff == n || cycle + 1 >= a.maxiter;
      if (fin && (meff < m || meff == n)) nconv = nw;   // exact: the Krylov space closed
      sh_i[1] = nconv;
      sh_i[2] = fin;
    }
    __syncthreads();
    if (sh_i[2]) {
      for (int i = tid; i < nev; i += NT)
        a.out[i] = i < meff ? d[ord[a.which == 0 ? i : meff - 1 - i]] : __longlong_as_double(0x7ff8000000000000LL);
      if (tid == 0) {
        a.out[nev] = (double)matvecs;
        a.out[nev + 1] = (double)sh_i[1];
        st[EIG_ST_DONE] = 1.0;
        st[EIG_ST_NCONV] = (double)sh_i[1];
        st[EIG_ST_MATVECS] = (double)matvecs;
        st[EIG_ST_CYCLE] = (double)cycle;
      }
      return;
    }
    // ---- thick restart (meff = m): the knew wanted-end Ritz vectors, then the residual direction V[m] ----
    const int knew = max(nev + 1, min(m - 1, nev + (m - nev) / 2));
    auto rotate = [&](const double* Y) {
      const int nch = (knew + SDPLR_EIG_RS_TILE - 1) / SDPLR_EIG_RS_TILE;
      for (int e = tid; e < nch * n; e += NT) {
        const int ch = e / n, p = e - ch * n, i0 = ch * SDPLR_EIG_RS_TILE;
        const double* yr[SDPLR_EIG_RS_TILE];
        double acc[SDPLR_EIG_RS_TILE];
#pragma unroll
        for (int q = 0; q < SDPLR_EIG_RS_TILE; q++) {
          const int i = min(i0 + q, knew - 1);
          yr[q] = Y + (long long)ord[a.which == 0 ? i : m - 1 - i] * ldy;
          acc[q] = 0.0;
        }
        for (int l = 0; l < m; l++) {
          const double x = V[(long long)l * ldv + p];
#pragma unroll
          for (int q = 0; q < SDPLR_EIG_RS_TILE; q++) acc[q] += yr[q][l] * x;
        }
#pragma unroll
        for (int q = 0; q < SDPLR_EIG_RS_TILE; q++)
          if (i0 + q < knew) V2[(long long)(i0 + q) * ldv + p] = acc[q];
      }
    };
    if (a.ylds) rotate(Yl); else rotate(a.Yg);
    for (int p = tid; p < n; p += NT) V2[(long long)knew * ldv + p] = v[p];   // (v holds V[m])
    for (int i = tid; i < knew; i += NT) st[EIG_ST_THETA + i] = d[ord[a.which == 0 ? i : m - 1 - i]];
    for (int e = tid; e < (int)eig_rs_tri(m); e += NT) T[e] = 0.0;
    __syncthreads();
    for (int i = tid; i < knew; i += NT) T[eig_rs_tix(i, i, m)] = d[ord[a.which == 0 ? i : m - 1 - i]];
    { double* t = V; V = V2; V2 = t; }
    cur ^= 1;
    k = knew;
    cycle++;
    __syncthreads();
  }
  if (tid == 0) {   // the cap: the next launch continues from here
    st[EIG_ST_STARTED] = 1.0;
    st[EIG_ST_K] = (double)k;
    st[EIG_ST_CYCLE] = (double)cycle;
    st[EIG_ST_MATVECS] = (double)matvecs;
    st[EIG_ST_CUR] = (double)cur;
  }
}

__global__ void __launch_bounds__(SDPLR_RS_NT)
k_eig_resident_batch(const EigResArgs* __restrict__ items) {
  eig_rs_run(items[blockIdx.x]);
}

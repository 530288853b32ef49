// k_round_batch.h — the rounding of k_round.h for a whole batch of small instances in ONE launch
// (include/sdplr_hip_round_batch.h): one workgroup per (instance, block of 64 trials) goes from R to that block's cuts —
// projection, labels, score and fold — with the per-vertex arrays in the LDS and nothing handed to the host in between.
// The definitions and every bit of the results are those of k_round.h:
//   - projection: z_t = z_t + R_ik·γ_kt, k outermost, one rounding per multiply and per add; lane = vertex.  Γ's rows of
//     the trial block sit in the LDS (all r of them: the route rule bounds r·512 bytes) and are read as broadcasts.
//   - hyperplane: the lane holds the 64 projections of its vertex and so its whole label word.
//   - bisection: the trial block is taken eight trials at a time (one per wave).  The lanes write the eight keys of their
//     vertices to the LDS, keys[tt·n + i]; wave tt finds trial tt's threshold by the radix select of k_round_select (eight
//     passes of eight bits, a histogram of integer LDS atomics per wave, then the ordered pass over the tied keys only when
//     more tie than are taken); the lanes turn their vertices' keys into eight more bits of the label word.
//   - score: label words in the LDS, lane = trial, edges streamed from HBM.  k_round_score's grid has 4·nb waves; wave slot
//     v takes the groups of 64 edges v, v + 4·nb, … in edge order, a block's partial is ((s₀ + s₁) + s₂) + s₃ and
//     k_round_fold adds the partials to 0.0 in block order.  Here the eight waves take the wave slots of two such blocks per
//     round, and wave 0 adds the two block partials to the running cut, in block order: the same sums in the same order.
// No floating-point atomics; the accumulators are indexed by unrolled loops only.
#pragma once
#include "k_round.h"

#define SDPLR_ROUND_BATCH_NT 512     // threads of a workgroup: 8 waves, 2 per SIMD (room for the 64 accumulators)
#define SDPLR_ROUND_BATCH_TG 8       // bisection: trials per pass = waves of the workgroup
#define SDPLR_ROUND_BATCH_NMAX 2048  // largest n the shared launch takes (the LDS budget bounds it further: round_batch_lds)

struct RoundBatchArgs {   // one row per instance
  const double* R;        // [n × r], row i contiguous
  const double* gT;       // Γ transposed and padded as in k_round.h: gT[k·Tpad + t]
  const int* ei;
  const int* ej;
  const double* ew;
  round_u64* lab;         // [n × W] label words, for k_round_batch_labels
  double* cuts;           // [Tpad]
  long long E;
  int n, r, T, Tpad, W, mode, nb_score, pad_;
};
struct RoundBatchBlock { int item, w; };   // block b ↔ trial block w of instance `item`

// dynamic LDS of one workgroup: label words, Γ's rows of the trial block, the selection's histograms (their first half
// doubles as the score's wave sums), thresholds, and in bisection mode eight trials' keys
__host__ __device__ inline size_t round_batch_lds(long long n, long long r, int mode) {
  return (size_t)n * 8 + (size_t)r * 64 * 8 + (size_t)SDPLR_ROUND_BATCH_TG * 256 * 4 + (size_t)SDPLR_ROUND_BATCH_TG * 16 +
         (mode == 1 ? (size_t)SDPLR_ROUND_BATCH_TG * n * 8 : 0);
}

// z_t = Σ_k R_ik·γ_kt for the TG trials whose γ start at g (row stride 64), as k_round_project adds them
template <int TG>
__device__ __forceinline__ void round_batch_project(const double* __restrict__ Ri, int r, const double* g, double (&z)[TG]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int t = 0; t < TG; t++) z[t] = 0.0;
  for (int k = 0; k < r; k++) {
    const double a = Ri[k];
    const double* gk = g + k * 64;
#pragma unroll
    for (int t = 0; t < TG; t++) z[t] = z[t] + a * gk[t];
  }
}

// k_round_select for one wave and keys in the LDS: K = the key of 0-based rank half − 1, cut = the index of the last tied
// vertex taken (n when every tied vertex is taken).  hist: 256 counters of this wave's own.  half ≥ 1.
__device__ __forceinline__ void round_batch_select(const round_u64* key, int n, int half, unsigned int* hist, int lane,
                                                   round_u64* outK, long long* outCut) {
  round_u64 prefix = 0ull, mask = 0ull;
  unsigned int rem = (unsigned int)(half - 1), cnt_eq = 0u;
  for (int shift = 56; shift >= 0; shift -= 8) {
#pragma unroll
    for (int q = 0; q < 4; q++) hist[q * 64 + lane] = 0u;
    __builtin_amdgcn_wave_barrier();
    __threadfence_block();
    for (int i = lane; i < n; i += 64) {
      const round_u64 k = key[i];
      if ((k & mask) == prefix) atomicAdd(&hist[(unsigned int)(k >> shift) & 255u], 1u);
    }
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    // the digit d: the first with (count of digits ≤ d) > rem.  Lane l holds digits 4l … 4l + 3.
    unsigned int c[4], s = 0u;
#pragma unroll
    for (int q = 0; q < 4; q++) { c[q] = hist[4 * lane + q]; s += c[q]; }
    unsigned int incl = s;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const unsigned int up = __shfl_up(incl, o, 64);
      if (lane >= o) incl += up;
    }
    const round_u64 over = __ballot(incl > rem);   // (the matching keys number more than rem: some lane is over)
    const int L = over ? __ffsll((long long)over) - 1 : 63;
    unsigned int d = 0u, left = rem - (incl - s), ceq = c[0];
    if (left >= c[0]) { left -= c[0]; d = 1u; ceq = c[1];
      if (left >= c[1]) { left -= c[1]; d = 2u; ceq = c[2];
        if (left >= c[2]) { left -= c[2]; d = 3u; ceq = c[3]; } } }
    d = (unsigned int)__shfl((int)(4u * (unsigned int)lane + d), L, 64);
    rem = (unsigned int)__shfl((int)left, L, 64);
    cnt_eq = (unsigned int)__shfl((int)ceq, L, 64);
    prefix |= (round_u64)d << shift;
    mask |= 255ull << shift;
    __builtin_amdgcn_wave_barrier();
  }
  const round_u64 K = prefix;
  const unsigned int need = rem + 1u;   // tied vertices taken; cnt_eq = tied vertices in all
  long long cut = n;
  if (need < cnt_eq) {                  // the index of the need-th vertex (in index order) whose key is K
    unsigned int base = 0u;
    for (int i0 = 0; i0 < n; i0 += 64) {
      const int i = i0 + lane;
      const bool eq = i < n && key[i] == K;
      const round_u64 b = __ballot(eq);
      const unsigned int total = (unsigned int)__popcll(b);
      if (base + total >= need) {
        const unsigned int incl = base + (unsigned int)__popcll(b & ((2ull << lane) - 1ull));
        const round_u64 hit = __ballot(eq && incl == need);
        cut = i0 + __ffsll((long long)hit) - 1;
        break;
      }
      base += total;
    }
  }
  if (lane == 0) { *outK = K; *outCut = cut; }
}

__global__ void __launch_bounds__(SDPLR_ROUND_BATCH_NT) k_round_batch(const RoundBatchArgs* __restrict__ tab,
                                                                      const RoundBatchBlock* __restrict__ blocks) {
#pragma clang fp contract(off)
  extern __shared__ __align__(16) unsigned char round_batch_smem[];
  const RoundBatchBlock bk = blocks[blockIdx.x];
  const RoundBatchArgs a = tab[bk.item];
  const int n = a.n, r = a.r, w = bk.w, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int valid = min(64, a.T - 64 * w);
  round_u64* labw = reinterpret_cast<round_u64*>(round_batch_smem);                  // [n]
  double* sg = reinterpret_cast<double*>(labw + n);                                  // [r × 64]
  unsigned int* hist = reinterpret_cast<unsigned int*>(sg + (size_t)r * 64);         // [TG × 256]
  double* sh = reinterpret_cast<double*>(hist);                                      // [8 × 64] (after the selection)
  round_u64* selK = reinterpret_cast<round_u64*>(hist + SDPLR_ROUND_BATCH_TG * 256); // [TG]
  long long* selCut = reinterpret_cast<long long*>(selK + SDPLR_ROUND_BATCH_TG);     // [TG]
  round_u64* keys = reinterpret_cast<round_u64*>(selCut + SDPLR_ROUND_BATCH_TG);     // [TG × n] (bisection)

  for (int q = tid; q < r * 64; q += SDPLR_ROUND_BATCH_NT) sg[q] = a.gT[(size_t)(q >> 6) * a.Tpad + (size_t)w * 64 + (q & 63)];
  __syncthreads();

  if (a.mode == 0) {
    for (int i = tid; i < n; i += SDPLR_ROUND_BATCH_NT) {
      double z[64];
      round_batch_project<64>(a.R + (size_t)i * r, r, sg, z);
      round_u64 word = 0ull;
#pragma unroll
      for (int t = 0; t < 64; t++) word |= (round_u64)(z[t] < 0.0 ? 1 : 0) << t;
      if (valid < 64) word &= (1ull << valid) - 1ull;
      labw[i] = word;
    }
  } else {
    const int half = n / 2;
    for (int i = tid; i < n; i += SDPLR_ROUND_BATCH_NT) labw[i] = 0ull;
    for (int t0 = 0; t0 < valid; t0 += SDPLR_ROUND_BATCH_TG) {
      for (int i = tid; i < n; i += SDPLR_ROUND_BATCH_NT) {
        double z[SDPLR_ROUND_BATCH_TG];
        round_batch_project<SDPLR_ROUND_BATCH_TG>(a.R + (size_t)i * r, r, sg + t0, z);
#pragma unroll
        for (int tt = 0; tt < SDPLR_ROUND_BATCH_TG; tt++) keys[tt * n + i] = round_key(z[tt]);
      }
      __syncthreads();
      if (t0 + wv < valid) {
        if (half <= 0) { if (lane == 0) { selK[wv] = 0ull; selCut[wv] = -1; } }
        else round_batch_select(keys + (size_t)wv * n, n, half, hist + wv * 256, lane, &selK[wv], &selCut[wv]);
      }
      __syncthreads();
      for (int i = tid; i < n; i += SDPLR_ROUND_BATCH_NT) {
        round_u64 bits = 0ull;
#pragma unroll
        for (int tt = 0; tt < SDPLR_ROUND_BATCH_TG; tt++) {
          if (t0 + tt < valid) {
            const round_u64 k = keys[tt * n + i], K = selK[tt];
            const bool minus = !(k < K || (k == K && (long long)i <= selCut[tt]));
            bits |= (round_u64)(minus ? 1 : 0) << tt;
          }
        }
        labw[i] |= bits << t0;
      }
      __syncthreads();   // (the keys and thresholds are rewritten by the next pass)
    }
  }
  __syncthreads();
  for (int i = tid; i < n; i += SDPLR_ROUND_BATCH_NT) a.lab[(size_t)i * a.W + w] = labw[i];

  // score and fold: virtual block vb of k_round_score = wave slots 4·vb … 4·vb + 3; this workgroup's waves 0-3 and 4-7 take
  // the blocks 2·j and 2·j + 1 of round j
  const long long E = a.E;
  const int nb = a.nb_score;
  const long long nwaves = 4ll * nb;
  double cut = 0.0;   // (wave 0: lane = trial)
  for (int vb0 = 0; vb0 < nb; vb0 += 2) {
    const int vb = vb0 + (wv >> 2);
    double sum = 0.0;
    if (vb < nb) {
      const long long wave = 4ll * vb + (wv & 3);
      for (long long e0 = wave * 64; e0 < E; e0 += nwaves * 64) {
        const long long e = e0 + lane;
        round_u64 x = 0ull;
        double al_mine = 0.0;
        if (e < E) {
          x = labw[a.ei[e]] ^ labw[a.ej[e]];
          al_mine = a.ew[e];
        }
        const int cnt = (int)min((long long)64, E - e0);
        for (int l = 0; l < cnt; l++) {
          const round_u64 xl = __shfl(x, l, 64);
          const double al = __shfl(al_mine, l, 64);
          if ((xl >> lane) & 1ull) sum += al;
        }
      }
    }
    sh[tid] = sum;
    __syncthreads();
    if (wv == 0) {
      double t = sh[lane];
#pragma unroll
      for (int q = 1; q < 4; q++) t += sh[q * 64 + lane];
      cut += t;
      if (vb0 + 1 < nb) {
        double u = sh[256 + lane];
#pragma unroll
        for (int q = 1; q < 4; q++) u += sh[256 + q * 64 + lane];
        cut += u;
      }
    }
    __syncthreads();
  }
  if (wv == 0 && lane < valid) a.cuts[w * 64 + lane] = cut;
}

// ±1 labels as int8 for the whole batch, one row per request: trials t0 … t0 + nt − 1 of an instance, trial-major at out.
// grid (requests, SDPLR_ROUND_BATCH_LABEL_NY)
#define SDPLR_ROUND_BATCH_LABEL_NY 8
struct RoundBatchLabelArgs {
  const round_u64* lab;
  signed char* out;
  int n, W, t0, nt;
};
__global__ void __launch_bounds__(SDPLR_NT) k_round_batch_labels(const RoundBatchLabelArgs* __restrict__ tab) {
  const RoundBatchLabelArgs a = tab[blockIdx.x];
  const long long total = (long long)a.n * a.nt;
  for (long long q = (long long)blockIdx.y * SDPLR_NT + threadIdx.x; q < total; q += (long long)gridDim.y * SDPLR_NT) {
    const int i = (int)(q % a.n), t = a.t0 + (int)(q / a.n);
    a.out[q] = ((a.lab[(size_t)i * a.W + (t >> 6)] >> (t & 63)) & 1ull) ? (signed char)-1 : (signed char)1;
  }
}

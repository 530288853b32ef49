// k_round.h — randomized rounding of a factor on the device (exps/test.jl:67-105): T random projections of R, turned
// into ±1 labellings by sign (MaxCut, :76-87) or by splitting the sorted projection in halves (MinimumBisection, :89-105),
// each scored by its cut ¼·xᵀLx = Σ over edges i < j with x_i ≠ x_j of a_ij.
//
// Layout.  Trials are handled in blocks of 64.  The labels of vertex i are W = ⌈T/64⌉ words of 64 bits, lab[i·W + w],
// bit t of word w = trial 64·w + t, set ⇔ x = −1; bits of trials ≥ T are zero.  Γ arrives transposed and padded,
// gT[k·Tpad + t] (Tpad = 64·W, zeros beyond T), so that the 64 values of one k and one trial block are contiguous.
//
// Projection: one LANE per VERTEX, the 64 projections of a trial block in that lane's registers, k outermost:
// z_t = z_t + R_ik·γ_kt for k = 0 … r − 1 — one rounding per multiply and per add, in that order (the
// library is built -ffp-contract=off; the pragma below says it again).  γ_kt is the same for every lane (an LDS broadcast), every
// R_ik is read once per trial block, and the same kernel serves every rank: nothing is indexed dynamically, so the 64
// accumulators never leave the VGPRs.  A lane then holds the whole label word of its vertex (sign mode: no cross-lane
// step at all), or writes its 64 keys to the trial-major work array keys[t·n + i] — lanes = consecutive vertices, so every
// store is coalesced — for the selection that follows.
//
// Every sum of doubles here has a fixed order (lane-private in edge order, block partials folded in block order); the
// only atomics are integer LDS histogram counts, whose result does not depend on their order.
#pragma once
#include "common.h"

typedef unsigned long long round_u64;

#define SDPLR_ROUND_SEL_NT 1024     // threads of the one-workgroup-per-trial selection kernel
#define SDPLR_ROUND_SCORE_NB 256    // most blocks of the scoring kernel (= partials per trial)

// order-preserving key of a double: −0.0 folded onto 0.0, then sign-magnitude → unsigned (NaNs of either sign aside, the
// keys sort as the doubles do and equal doubles have equal keys)
__device__ __forceinline__ round_u64 round_key(double z) {
  round_u64 u = (round_u64)__double_as_longlong(z);
  if (u == 0x8000000000000000ull) u = 0ull;
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

// MODE 0: lab[i·W + w] = bits (z_it < 0); MODE 1: keys[t·n + i] = round_key(z_it) for the one trial block w0.
// grid (⌈n/256⌉, trial blocks); valid trials of block w: min(64, T − 64·w).  Γ's rows of the trial block pass through
// the LDS, SDPLR_ROUND_KC of them at a time, and are read back as broadcasts (every lane the same address).
#define SDPLR_ROUND_KC 32
template <int MODE>
__global__ void __launch_bounds__(SDPLR_NT) k_round_project(const double* __restrict__ R, long long n, int r,
                                                            const double* __restrict__ gT, int Tpad, int T, int w0,
                                                            round_u64* __restrict__ lab, int W,
                                                            round_u64* __restrict__ keys) {
#pragma clang fp contract(off)
  __shared__ double sg[SDPLR_ROUND_KC * 64];
  const int w = w0 + (int)blockIdx.y;
  const int valid = min(64, T - 64 * w);
  const double* __restrict__ g = gT + (size_t)w * 64;
  {   // (one vertex per thread: the grid covers n)
    const long long i = (long long)blockIdx.x * SDPLR_NT + threadIdx.x;
    const bool act = i < n;
    const double* __restrict__ Ri = R + (act ? i : 0) * r;
    // z starts at +0.0 and every product is added in turn: 0.0 + p is p (a −0.0 becomes +0.0, which neither the sign
    // test nor the folded keys can tell apart), so this is the sum p_0 + p_1 + … as defined
    double z[64];
#pragma unroll
    for (int t = 0; t < 64; t++) z[t] = 0.0;
    for (int k0 = 0; k0 < r; k0 += SDPLR_ROUND_KC) {
      const int kc = min(SDPLR_ROUND_KC, r - k0);
      __syncthreads();
      for (int q = threadIdx.x; q < kc * 64; q += SDPLR_NT) sg[q] = g[(size_t)(k0 + (q >> 6)) * Tpad + (q & 63)];
      __syncthreads();
      if (act) {
        for (int k = 0; k < kc; k++) {
          const double a = Ri[k0 + k];
          const double* gk = sg + k * 64;
#pragma unroll
          for (int t = 0; t < 64; t++) z[t] = z[t] + a * gk[t];
        }
      }
    }
    if (!act) return;
    if constexpr (MODE == 0) {
      round_u64 word = 0ull;
#pragma unroll
      for (int t = 0; t < 64; t++) word |= (round_u64)(z[t] < 0.0 ? 1 : 0) << t;
      if (valid < 64) word &= (1ull << valid) - 1ull;
      lab[i * W + w] = word;
    } else {
      round_u64* kp = keys + i;
#pragma unroll
      for (int t = 0; t < 64; t++) {
        if (t < valid) *kp = round_key(z[t]);
        kp += n;
      }
    }
  }
}

// Selection, one workgroup per trial of the block: the key K of 0-based rank half − 1 among keys[t·n .. t·n + n) by radix
// select (eight passes of eight bits, most significant first, LDS histogram of the keys that still match the prefix),
// then — only when more vertices tie at K than the +1 side still takes — one ordered pass for the index of the last tied
// vertex taken.  Vertex i of trial t gets +1 ⇔ key < K, or key = K and i ≤ cut.  half = 0 (n = 1): nobody.
__global__ void __launch_bounds__(SDPLR_ROUND_SEL_NT) k_round_select(const round_u64* __restrict__ keys, long long n,
                                                                       long long half, round_u64* __restrict__ selK,
                                                                       long long* __restrict__ selCut) {
  __shared__ unsigned int hist[256];
  __shared__ round_u64 sh_prefix;
  __shared__ unsigned int sh_remaining, sh_cnt_eq;
  __shared__ unsigned int wave_cnt[SDPLR_ROUND_SEL_NT / 64];
  __shared__ long long sh_cut;
  const int t = blockIdx.x, tid = threadIdx.x;
  const round_u64* __restrict__ key = keys + (size_t)t * n;
  if (half <= 0) {
    if (tid == 0) { selK[t] = 0ull; selCut[t] = -1; }
    return;
  }
  if (tid == 0) { sh_prefix = 0ull; sh_remaining = (unsigned int)(half - 1); sh_cnt_eq = 0u; }
  round_u64 mask = 0ull;
  for (int shift = 56; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0u;
    __syncthreads();
    const round_u64 prefix = sh_prefix;
    for (long long i = tid; i < n; i += SDPLR_ROUND_SEL_NT) {
      const round_u64 k = key[i];
      if ((k & mask) == prefix) atomicAdd(&hist[(unsigned int)(k >> shift) & 255u], 1u);
    }
    __syncthreads();
    if (tid == 0) {
      unsigned int rem = sh_remaining, d = 0;
      while (d < 255u && hist[d] <= rem) { rem -= hist[d]; d++; }   // (the matching keys number more than rem: d stops in range)
      sh_remaining = rem;
      sh_cnt_eq = hist[d];
      sh_prefix = prefix | ((round_u64)d << shift);
    }
    mask |= 255ull << shift;
    __syncthreads();
  }
  const round_u64 K = sh_prefix;
  const unsigned int need = sh_remaining + 1u, cnt_eq = sh_cnt_eq;   // tied vertices taken / tied vertices in all
  if (need >= cnt_eq) {                                             // every tied vertex is taken: no order needed
    if (tid == 0) { selK[t] = K; selCut[t] = n; }
    return;
  }
  // the index of the need-th vertex (in index order) whose key is K
  if (tid == 0) sh_cut = n;
  unsigned int base = 0u;
  const int lane = tid & 63, wv = tid >> 6;
  for (long long i0 = 0; i0 < n; i0 += SDPLR_ROUND_SEL_NT) {
    const long long i = i0 + tid;
    const bool eq = i < n && key[i] == K;
    const round_u64 b = __ballot(eq);
    if (lane == 0) wave_cnt[wv] = (unsigned int)__popcll(b);
    __syncthreads();
    unsigned int before = 0u, total = 0u;
    for (int q = 0; q < SDPLR_ROUND_SEL_NT / 64; q++) {
      const unsigned int c = wave_cnt[q];
      if (q < wv) before += c;
      total += c;
    }
    const unsigned int incl = base + before + (unsigned int)__popcll(b & ((2ull << lane) - 1ull));
    if (eq && incl == need) sh_cut = i;
    __syncthreads();                       // (wave_cnt is rewritten by the next round; sh_cut is read below)
    if (base + total >= need) break;       // uniform: base and total are the same in every thread
    base += total;
  }
  __syncthreads();
  if (tid == 0) { selK[t] = K; selCut[t] = sh_cut; }
}

// Bisection labels of trial block w into the label words: one wave per tile of 64 vertices, lane = vertex.  For each
// trial the wave's ballot is the 64-vertex bit column of that trial (lane t keeps column t); 64 more ballots transpose the
// 64 × 64 bit tile, and lane j stores the word of vertex i0 + j.  Reads of the keys are coalesced (trial-major).
__global__ void __launch_bounds__(SDPLR_NT) k_round_pack(const round_u64* __restrict__ keys, long long n, int valid,
                                                         const round_u64* __restrict__ selK,
                                                         const long long* __restrict__ selCut,
                                                         round_u64* __restrict__ lab, int W, int w) {
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * (SDPLR_NT / 64) + (threadIdx.x >> 6);
  const long long nwaves = (long long)gridDim.x * (SDPLR_NT / 64);
  for (long long i0 = wave * 64; i0 < n; i0 += nwaves * 64) {
    const long long i = i0 + lane;
    round_u64 mine = 0ull;
    for (int t = 0; t < valid; t++) {
      const round_u64 K = selK[t];
      const long long cut = selCut[t];
      bool minus = false;
      if (i < n) {
        const round_u64 k = keys[(size_t)t * n + i];
        minus = !(k < K || (k == K && i <= cut));
      }
      const round_u64 col = __ballot(minus);
      if (lane == t) mine = col;
    }
    round_u64 out = 0ull;
    for (int j = 0; j < 64; j++) {
      const round_u64 row = __ballot((mine >> j) & 1ull);
      if (lane == j) out = row;
    }
    if (i < n) lab[i * W + w] = out;
  }
}

// Cuts: lane = trial of block blockIdx.y.  A wave takes groups of 64 edges (group g, g + waves, …): lane l fetches edge
// e0 + l and the XOR of its endpoints' label words (64 gathers in flight), then the 64 edges are handed round in edge
// order and each lane adds w to its own sum when its bit is set.  The four waves of a block are added in wave order;
// part[blockIdx.x·Tpad + trial] is the block's partial.
__global__ void __launch_bounds__(SDPLR_NT) k_round_score(const int* __restrict__ ei, const int* __restrict__ ej,
                                                          const double* __restrict__ ew, long long E,
                                                          const round_u64* __restrict__ lab, int W, int Tpad,
                                                          double* __restrict__ part) {
  __shared__ double sh[SDPLR_NT];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, w = blockIdx.y;
  const long long wave = (long long)blockIdx.x * (SDPLR_NT / 64) + wv;
  const long long nwaves = (long long)gridDim.x * (SDPLR_NT / 64);
  double sum = 0.0;
  for (long long e0 = wave * 64; e0 < E; e0 += nwaves * 64) {
    const long long e = e0 + lane;
    round_u64 x = 0ull;
    double a = 0.0;
    if (e < E) {
      x = lab[(long long)ei[e] * W + w] ^ lab[(long long)ej[e] * W + w];
      a = ew[e];
    }
    const int cnt = (int)min((long long)64, E - e0);
    for (int l = 0; l < cnt; l++) {
      const round_u64 xl = __shfl(x, l, 64);
      const double al = __shfl(a, l, 64);
      if ((xl >> lane) & 1ull) sum += al;
    }
  }
  sh[threadIdx.x] = sum;
  __syncthreads();
  if (wv == 0) {
    double t = sh[lane];
#pragma unroll
    for (int q = 1; q < SDPLR_NT / 64; q++) t += sh[q * 64 + lane];
    part[(size_t)blockIdx.x * Tpad + w * 64 + lane] = t;
  }
}

// cuts[t] = Σ_b part[b·Tpad + t], b ascending
__global__ void __launch_bounds__(SDPLR_NT) k_round_fold(const double* __restrict__ part, int nb, int Tpad, int T,
                                                         double* __restrict__ cuts) {
  const int t = blockIdx.x * SDPLR_NT + threadIdx.x;
  if (t >= T) return;
  double s = 0.0;
  for (int b = 0; b < nb; b++) s += part[(size_t)b * Tpad + t];
  cuts[t] = s;
}

// ±1 labels of trials t0 … t0 + nt − 1 as int8, trial-major: out[(t − t0)·n + i]
__global__ void __launch_bounds__(SDPLR_NT) k_round_labels(const round_u64* __restrict__ lab, long long n, int W, int t0,
                                                           int nt, signed char* __restrict__ out) {
  for (long long i = (long long)blockIdx.x * SDPLR_NT + threadIdx.x; i < n; i += (long long)gridDim.x * SDPLR_NT)
    for (int t = t0; t < t0 + nt; t++)
      out[(size_t)(t - t0) * n + i] = ((lab[i * W + (t >> 6)] >> (t & 63)) & 1ull) ? (signed char)-1 : (signed char)1;
}

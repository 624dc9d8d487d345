// Sampled decoding head: temperature / top-k / top-p and one draw per row, on the device
// (include/inferd_span.h "Sampled decoding"; the reference's client runs transformers' warpers,
// a softmax and torch.multinomial on the host, client.py:95-120).
//
// One 1024-thread workgroup per row of bf16 logits [rows][vocab]:
//   A  the row's 16-column tile maxima as 16-bit order keys in registers (up to 24 per thread) --
//      the top 16 bits of the keys the lm_head GEMV's EPI_ARGMAX epilogue already wrote
//      ([rows][vocab / 16]), or computed from the logits when the caller has none (the single op);
//   B  tau = the top_k-th largest tile maximum (a digit-wise search, two bits per round: ballot
//      counts per wave, three LDS adds per wave and one barrier per round): at least top_k columns
//      are >= tau, so tau is a lower bound of the top-k threshold v_k;
//   C  only tiles whose maximum reaches tau are read from the logits; their columns >= tau are the
//      candidates (LDS list);
//   D  every candidate's rank in the order (s descending, column ascending) by counting; rank
//      top_k - 1 is v_k, the kept set {s >= v_k} (ties kept) is the order's prefix, capped at
//      SAMPLE_MAX_KEPT entries (error flag bit 2);
//   E  wave 0: fp32 softmax over the kept entries, the top-p cut, renormalisation and the draw with
//      the counter-based uniform of the row.
// More candidates than the list holds (more than 1024 columns at or above tau: mass ties) take
// an exact path over the whole row instead of C: v_k by the same bitwise search over all columns,
// the columns above v_k, then the ties at v_k in column order up to the capacity.
// All comparisons that decide membership are made on s = fp32(logit) / T, the value the definition
// names; the 16-bit keys only order the logits (s is monotone in them).
#include <math.h>

#include "common.h"
#include "kernels.h"

namespace {

constexpr int ST = 1024;         // threads per row
constexpr int CAND_CAP = 1024;   // candidate list entries
constexpr int MAX_KEPT = 256;    // INFERD_SAMPLE_MAX_KEPT
constexpr int KPT = SAMPLE_MAX_VOCAB / 16 / ST;  // tile maxima per thread
constexpr int ERR_SAMPLE_OVERFLOW = 4;  // inferd_span_error_flags bit 2

// 16-bit order key of a bf16 pattern (larger value -> larger key), -0 folded onto +0
__device__ __forceinline__ uint32_t canon16(uint32_t k) { return k == 0x7FFFu ? 0x8000u : k; }
__device__ __forceinline__ uint32_t okey16(u16 b) {
  return canon16((b & 0x8000u) ? (~(uint32_t)b & 0xFFFFu) : ((uint32_t)b | 0x8000u));
}
__device__ __forceinline__ float key16_value(uint32_t k) {
  return bf2f((u16)((k & 0x8000u) ? (k ^ 0x8000u) : (~k & 0xFFFFu)));
}
// (s descending, column ascending) as one descending 64-bit key, and back
__device__ __forceinline__ unsigned long long cand_key(float s, int col) {
  if (s == 0.f) s = 0.f;  // -0 -> +0: equal values tie on the column
  return ((unsigned long long)float_key(s) << 32) | (0xFFFFFFFFu - (uint32_t)col);
}
__device__ __forceinline__ float cand_s(unsigned long long k) {
  const uint32_t h = (uint32_t)(k >> 32);
  return __uint_as_float((h & 0x80000000u) ? (h ^ 0x80000000u) : ~h);
}
__device__ __forceinline__ int cand_col(unsigned long long k) { return (int)(0xFFFFFFFFu - (uint32_t)k); }

// sum of v over the workgroup's 16 waves, returned to every thread; buf alternates so that a
// call's reads are fenced from the next call's writes by the call between them
__device__ __forceinline__ int block_sum(int v, int (*buf)[16], int& ph) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  if ((threadIdx.x & 63) == 0) buf[ph][threadIdx.x >> 6] = v;
  __syncthreads();
  int t = 0;
#pragma unroll
  for (int w = 0; w < ST / 64; ++w) t += buf[ph][w];
  ph ^= 1;
  return t;
}

struct SampleArgs {
  const u16* logits;                 // [rows][vocab] row-major
  const unsigned long long* keys;    // [rows][vocab / 16] EPI_ARGMAX tile keys, or null
  int vocab;
  float T;
  int top_k;
  float top_p;
  uint64_t seed_key;                 // splitmix64(seed)
  const uint64_t* row_seeds;         // [rows] or null (the row index)
  const int32_t* positions;          // [rows]
  int32_t* ids;
  float* u_out;
  int32_t* flags;
};

__global__ __launch_bounds__(ST) void sample_kernel(const SampleArgs a) {
  __shared__ int red[2][16];
  __shared__ int cnt[8][3];  // B: the workgroup's counts of each search round
  __shared__ unsigned long long cand[CAND_CAP];
  __shared__ unsigned long long sorted[MAX_KEPT];
  __shared__ int n_cand;
  __shared__ float sh_vk;
  const int row = blockIdx.x, tid = threadIdx.x;
  const int vocab = a.vocab, n_tiles = vocab >> 4;
  const u16* lrow = a.logits + (int64_t)row * vocab;
  const u16x8* lrow8 = (const u16x8*)lrow;
  const float T = a.T;
  const int k_eff = a.top_k < vocab ? a.top_k : vocab;
  int ph = 0;

  // ---- A: tile maxima, thread t holding tiles t, t + 1024, ... in registers (0: no tile)
  uint32_t tk[KPT];
  if (a.keys) {  // the keys' high words: all loads in flight at once
    const uint32_t* kh = (const uint32_t*)(a.keys + (int64_t)row * n_tiles) + 1;
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      const int t = i * ST + tid;
      tk[i] = t < n_tiles ? kh[2 * (int64_t)t] : 0u;
    }
#pragma unroll
    for (int i = 0; i < KPT; ++i) tk[i] = (i * ST + tid < n_tiles) ? canon16(tk[i] >> 16) : 0u;
  } else {
#pragma unroll
    for (int i = 0; i < KPT; ++i) {
      const int t = i * ST + tid;
      uint32_t k = 0;
      if (t < n_tiles) {
        const u16x8 x0 = lrow8[2 * t], x1 = lrow8[2 * t + 1];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const uint32_t k0 = okey16(x0[j]), k1 = okey16(x1[j]);
          k = k0 > k ? k0 : k;
          k = k1 > k ? k1 : k;
        }
      }
      tk[i] = k;
    }
  }
  if (tid == 0) {
    n_cand = 0;
    sh_vk = -INFINITY;  // stays so when fewer than top_k candidates compare (NaN logits)
  }
  if (tid < 24) (&cnt[0][0])[tid] = 0;
  __syncthreads();

  // ---- B: tau = the top_k-th largest tile maximum (fewer tiles than top_k: every column is a
  // candidate).  The largest v with at least top_k maxima >= v, two bits per round (a round costs a
  // barrier and an LDS round trip, ~0.4 us): a wave counts the three thresholds with ballots, the
  // waves add into the round's cells; the counts fall with the threshold, so the largest digit
  // that still reaches top_k is the one bit-by-bit decisions would take
  float tau_s = -INFINITY;
  if (n_tiles >= a.top_k) {
    uint32_t v = 0;
    for (int r = 0; r < 8; ++r) {
      const int bit = 14 - 2 * r;
      const uint32_t c1 = v | (1u << bit), c2 = v | (2u << bit), c3 = v | (3u << bit);  // >= 1: an empty slot never counts
      int w1 = 0, w2 = 0, w3 = 0;
#pragma unroll
      for (int i = 0; i < KPT; ++i)
        if (i * ST < n_tiles) {  // a uniform condition
          w1 += __popcll(__ballot(tk[i] >= c1));
          w2 += __popcll(__ballot(tk[i] >= c2));
          w3 += __popcll(__ballot(tk[i] >= c3));
        }
      if ((tid & 63) == 0) {
        if (w1) atomicAdd(&cnt[r][0], w1);
        if (w2) atomicAdd(&cnt[r][1], w2);
        if (w3) atomicAdd(&cnt[r][2], w3);
      }
      __syncthreads();
      v = cnt[r][2] >= a.top_k ? c3 : cnt[r][1] >= a.top_k ? c2 : cnt[r][0] >= a.top_k ? c1 : v;
    }
    tau_s = key16_value(v) / T;
  }

  // ---- C: candidates = columns >= tau of the tiles whose maximum reaches tau
#pragma unroll
  for (int i = 0; i < KPT; ++i) {
    const int t = i * ST + tid;
    if (t >= n_tiles || !(key16_value(tk[i]) / T >= tau_s)) continue;
    const u16x8 x0 = lrow8[2 * t], x1 = lrow8[2 * t + 1];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float s = bf2f(j < 8 ? x0[j & 7] : x1[j & 7]) / T;
      if (s >= tau_s) {
        const int idx = atomicAdd(&n_cand, 1);
        if (idx < CAND_CAP) cand[idx] = cand_key(s, t * 16 + j);
      }
    }
  }
  __syncthreads();
  int nc = n_cand;
  int total = -1;  // columns with s >= v_k (the exact path knows it; else counted in D)

  if (nc > CAND_CAP) {
    // ---- mass ties: v_k over the whole row, the columns above it, then the ties in column order
    uint32_t v = 0;
    for (int bit = 15; bit >= 0; --bit) {
      const uint32_t c = v | (1u << bit);
      int cnt = 0;
      for (int i = tid; i < vocab / 8; i += ST) {
        const u16x8 x = lrow8[i];
#pragma unroll
        for (int j = 0; j < 8; ++j) cnt += okey16(x[j]) >= c;
      }
      if (block_sum(cnt, red, ph) >= k_eff) v = c;
    }
    const float vk = key16_value(v) / T;
    __syncthreads();  // every thread has read n_cand
    if (tid == 0) n_cand = 0;
    __syncthreads();
    for (int i = tid; i < vocab / 8; i += ST) {  // fewer than k_eff <= 64 columns lie above v_k
      const u16x8 x = lrow8[i];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float s = bf2f(x[j]) / T;
        if (s > vk) {
          const int idx = atomicAdd(&n_cand, 1);
          if (idx < CAND_CAP) cand[idx] = cand_key(s, i * 8 + j);
        }
      }
    }
    __syncthreads();
    const int ngt = n_cand < MAX_KEPT ? n_cand : MAX_KEPT;
    const int quota = MAX_KEPT - ngt;
    const int lane = tid & 63, wave = tid >> 6;
    int running = 0;  // ties seen so far (the same in every thread)
    for (int base = 0; base < vocab && running <= quota; base += ST) {
      const int col = base + tid;
      const bool tie = col < vocab && bf2f(lrow[col]) / T == vk;
      const unsigned long long m = __ballot(tie);
      if (lane == 0) red[ph][wave] = __popcll(m);
      __syncthreads();
      int off = 0, tot = 0;
#pragma unroll
      for (int w = 0; w < ST / 64; ++w) {
        const int c = red[ph][w];
        off += w < wave ? c : 0;
        tot += c;
      }
      ph ^= 1;
      const int slot = running + off + __popcll(m & ((1ull << lane) - 1ull));
      if (tie && slot < quota) cand[ngt + slot] = cand_key(vk, col);
      running += tot;
    }
    __syncthreads();
    nc = ngt + (running < quota ? running : quota);
    total = ngt + running;
  }

  // ---- D: ranks in the order (s descending, column ascending); v_k; the kept prefix
  unsigned long long my = 0;
  int rank = 0;
  const bool have = tid < nc;
  if (have) {
    my = cand[tid];
    for (int j = 0; j < nc; ++j) rank += cand[j] > my;
    if (rank == k_eff - 1) sh_vk = cand_s(my);
  }
  __syncthreads();
  const bool kept = have && cand_s(my) >= sh_vk;
  if (kept && rank < MAX_KEPT) sorted[rank] = my;
  const int counted = block_sum(kept ? 1 : 0, red, ph);  // its barrier also publishes sorted[]
  if (total < 0) total = counted;
  const int n = total < MAX_KEPT ? (total < nc ? total : nc) : MAX_KEPT;
  if (tid >= 64) return;
  if (tid == 0 && total > MAX_KEPT && a.flags) atomicOr(a.flags, ERR_SAMPLE_OVERFLOW);
  if (n < 1) {  // nothing compares (a row of NaN logits): an in-range column, no distribution
    if (tid == 0) {
      a.ids[row] = 0;
      if (a.u_out) a.u_out[row] = 0.f;
    }
    return;
  }

  // ---- E (wave 0): softmax, top-p, draw.  Lane l holds entries 4l .. 4l+3 of the order.
  const float s0 = cand_s(sorted[0]);
  float e[4], P[4], S[4];  // the entries' masses, their running sums and their tail sums
  float run = 0.f;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = 4 * tid + i;
    e[i] = j < n ? exp2f((cand_s(sorted[j]) - s0) * 1.44269504088896341f) : 0.f;
    run += e[i];
    P[i] = run;
  }
  float back = 0.f;
#pragma unroll
  for (int i = 3; i >= 0; --i) {
    back += e[i];
    S[i] = back;
  }
  float incl = run, tail = run;  // inclusive scans of the lanes' sums: from lane 0 up, from lane 63 down
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const float up = __shfl_up(incl, o), dn = __shfl_down(tail, o);
    if (tid >= o) incl += up;
    if (tid + o < 64) tail += dn;
  }
  const float Z = __shfl(incl, 63);
  const float before = __shfl_up(incl, 1), after = __shfl_down(tail, 1);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    P[i] += tid > 0 ? before : 0.f;
    S[i] += tid < 63 ? after : 0.f;
  }
  // top-p: entry j goes iff the mass of j and everything after it is <= 1 - p (never entry 0);
  // the masses shrink along the order, so what stays is a prefix of m entries.  The tail sums are
  // summed from the far end (no cancellation: with top_p = 1 only a zero mass goes)
  const float cut = (1.0f - a.top_p) * Z;
  int m = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int j = 4 * tid + i;
    m += __popcll(__ballot(j < n && (j == 0 || S[i] > cut)));
  }
  m = m < 1 ? 1 : m;  // NaN masses compare false everywhere: the first entry stays
  const int mq = (m - 1) & 3;
  const float pm = mq == 0 ? P[0] : mq == 1 ? P[1] : mq == 2 ? P[2] : P[3];
  const float Zm = __shfl(pm, (m - 1) >> 2);  // the mass that stays: renormalisation
  const uint64_t rs = a.row_seeds ? a.row_seeds[row] : (uint64_t)row;
  const uint64_t key = splitmix64(a.seed_key + rs);
  const float u = (float)(uint32_t)(splitmix64(key + (uint64_t)(int64_t)a.positions[row]) >> 40) * 5.9604644775390625e-8f;
  const float thr = u * Zm;
  int pick = 0;  // the first entry whose running mass exceeds u
#pragma unroll
  for (int i = 0; i < 4; ++i) pick += __popcll(__ballot(4 * tid + i < m && P[i] <= thr));
  pick = pick > m - 1 ? m - 1 : pick;
  if (tid == 0) {
    a.ids[row] = cand_col(sorted[pick]);
    if (a.u_out) a.u_out[row] = u;
  }
}

}  // namespace

void launch_sample(const u16* logits, int rows, int vocab, const unsigned long long* keys, float temperature,
                   int top_k, float top_p, uint64_t seed, const uint64_t* row_seeds, const int32_t* positions,
                   int32_t* ids, float* u_out, int32_t* flags, hipStream_t s) {
  const SampleArgs a = {logits, keys, vocab, temperature, top_k, top_p, splitmix64(seed), row_seeds, positions,
                        ids, u_out, flags};
  hipLaunchKernelGGL(sample_kernel, dim3(rows), dim3(ST), 0, s, a);
}

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
// The stages are device functions shared by two kernels: sample_kernel (the whole row) and
// sample_shard_kernel (one shard of a vocab-parallel head: A - C over the shard's columns, the
// running candidate record of the other shards appended to the list, D over both, then the new
// record and / or E; DESIGN.md §9 has the argument that the chain reproduces the whole row's kept
// list and overflow flag exactly).
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
constexpr int REC_ENTRIES = SAMPLE_CAND_ENTRIES;  // candidate record of a vocab-parallel sampled head
constexpr int REC_WORDS = SAMPLE_CAND_WORDS;

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

// ---- A: the row's tile maxima, thread t holding tiles t, t + 1024, ... in registers (0: no tile);
// from the EPI_ARGMAX keys of the row (krow) or, without them, from the logits
__device__ __forceinline__ void tile_maxima(uint32_t (&tk)[KPT], const unsigned long long* krow, const u16x8* lrow8,
                                            int n_tiles) {
  const int tid = threadIdx.x;
  if (krow) {  // the keys' high words: all loads in flight at once
    const uint32_t* kh = (const uint32_t*)krow + 1;
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
}

// ---- B: tau = the top_k-th largest tile maximum (fewer tiles than top_k: -inf, every column is a
// candidate).  The largest v with at least top_k maxima >= v, two bits per round (a round costs a
// barrier and an LDS round trip, ~0.4 us): a wave counts the three thresholds with ballots, the
// waves add into the round's cells; the counts fall with the threshold, so the largest digit
// that still reaches top_k is the one bit-by-bit decisions would take.  cnt: zeroed, behind a barrier
__device__ __forceinline__ float tile_threshold(const uint32_t (&tk)[KPT], int n_tiles, int top_k, float T,
                                                int (*cnt)[3]) {
  const int tid = threadIdx.x;
  if (n_tiles < top_k) return -INFINITY;
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
    v = cnt[r][2] >= top_k ? c3 : cnt[r][1] >= top_k ? c2 : cnt[r][0] >= top_k ? c1 : v;
  }
  return key16_value(v) / T;
}

// ---- C: candidates = columns >= tau of the tiles whose maximum reaches tau (col0: the global
// index of the row's first column); *n_cand counts them all, the list holds the first CAND_CAP
__device__ __forceinline__ void gather_candidates(const uint32_t (&tk)[KPT], const u16x8* lrow8, int n_tiles, float T,
                                                  float tau_s, int col0, unsigned long long* cand, int* n_cand) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < KPT; ++i) {
    const int t = i * ST + tid;
    if (t >= n_tiles || !(key16_value(tk[i]) / T >= tau_s)) continue;
    const u16x8 x0 = lrow8[2 * t], x1 = lrow8[2 * t + 1];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float s = bf2f(j < 8 ? x0[j & 7] : x1[j & 7]) / T;
      if (s >= tau_s) {
        const int idx = atomicAdd(n_cand, 1);
        if (idx < CAND_CAP) cand[idx] = cand_key(s, col0 + t * 16 + j);
      }
    }
  }
}

// ---- mass ties (more than CAND_CAP columns reach tau): v_k over the whole row, the columns above
// it, then the ties in column order, `keep` entries at the most.  Returns the list's length; *total
// = the columns with s >= v_k (exact up to keep, beyond it only "more than keep")
__device__ __forceinline__ int mass_ties(const u16* lrow, const u16x8* lrow8, int vocab, int col0, float T, int k_eff,
                                         int keep, unsigned long long* cand, int* n_cand, int (*red)[16], int& ph,
                                         int* total) {
  const int tid = threadIdx.x;
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
  if (tid == 0) *n_cand = 0;
  __syncthreads();
  for (int i = tid; i < vocab / 8; i += ST) {  // fewer than k_eff <= 64 columns lie above v_k
    const u16x8 x = lrow8[i];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float s = bf2f(x[j]) / T;
      if (s > vk) {
        const int idx = atomicAdd(n_cand, 1);
        if (idx < CAND_CAP) cand[idx] = cand_key(s, col0 + i * 8 + j);
      }
    }
  }
  __syncthreads();
  const int ngt = *n_cand < keep ? *n_cand : keep;
  const int quota = keep - ngt;
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
    if (tie && slot < quota) cand[ngt + slot] = cand_key(vk, col0 + col);
    running += tot;
  }
  __syncthreads();
  *total = ngt + running;
  return ngt + (running < quota ? running : quota);
}

// ---- D: ranks of the nc <= EPT * 1024 list entries in the order (s descending, column ascending)
// by counting; rank k - 1 is v_k (*sh_vk, preset to -inf: no such rank keeps everything); the kept
// set {s >= v_k} is the order's prefix, its first `keep` entries go to sorted[].  Returns the
// number of kept list entries; its last barrier also publishes sorted[]
template <int EPT>
__device__ __forceinline__ int rank_keep(const unsigned long long* cand, int nc, int k, int keep,
                                         unsigned long long* sorted, float* sh_vk, int (*red)[16], int& ph) {
  const int tid = threadIdx.x;
  unsigned long long my[EPT];
  int rank[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    my[e] = tid + e * ST < nc ? cand[tid + e * ST] : 0ull;
    rank[e] = 0;
  }
  if (tid < nc) {
    for (int j = 0; j < nc; ++j) {
      const unsigned long long c = cand[j];
#pragma unroll
      for (int e = 0; e < EPT; ++e) rank[e] += c > my[e];
    }
#pragma unroll
    for (int e = 0; e < EPT; ++e)
      if (tid + e * ST < nc && rank[e] == k - 1) *sh_vk = cand_s(my[e]);
  }
  __syncthreads();
  int mine = 0;
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    const bool kept = tid + e * ST < nc && cand_s(my[e]) >= *sh_vk;
    if (kept && rank[e] < keep) sorted[rank[e]] = my[e];
    mine += kept ? 1 : 0;
  }
  return block_sum(mine, red, ph);
}

// ---- E (wave 0): softmax, top-p and the draw over the order's first n >= 1 kept entries.  Lane l
// holds entries 4l .. 4l+3 of the order.
__device__ __forceinline__ void draw_row(const unsigned long long* sorted, int n, float top_p, uint64_t seed_key,
                                         const uint64_t* row_seeds, const int32_t* positions, int row, int32_t* ids,
                                         float* u_out) {
  const int tid = threadIdx.x;
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
  const float cut = (1.0f - top_p) * Z;
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
  const uint64_t rs = row_seeds ? row_seeds[row] : (uint64_t)row;
  const uint64_t key = splitmix64(seed_key + rs);
  const float u = (float)(uint32_t)(splitmix64(key + (uint64_t)(int64_t)positions[row]) >> 40) * 5.9604644775390625e-8f;
  const float thr = u * Zm;
  int pick = 0;  // the first entry whose running mass exceeds u
#pragma unroll
  for (int i = 0; i < 4; ++i) pick += __popcll(__ballot(4 * tid + i < m && P[i] <= thr));
  pick = pick > m - 1 ? m - 1 : pick;
  if (tid == 0) {
    ids[row] = cand_col(sorted[pick]);
    if (u_out) u_out[row] = u;
  }
}

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
  const int k_eff = a.top_k < vocab ? a.top_k : vocab;
  int ph = 0;

  uint32_t tk[KPT];
  tile_maxima(tk, a.keys ? a.keys + (int64_t)row * n_tiles : nullptr, lrow8, n_tiles);
  if (tid == 0) {
    n_cand = 0;
    sh_vk = -INFINITY;  // stays so when fewer than top_k candidates compare (NaN logits)
  }
  if (tid < 24) (&cnt[0][0])[tid] = 0;
  __syncthreads();
  const float tau_s = tile_threshold(tk, n_tiles, a.top_k, a.T, cnt);
  gather_candidates(tk, lrow8, n_tiles, a.T, tau_s, 0, cand, &n_cand);
  __syncthreads();
  int nc = n_cand;
  int total = -1;  // columns with s >= v_k (the exact path knows it; else counted in D)
  if (nc > CAND_CAP) nc = mass_ties(lrow, lrow8, vocab, 0, a.T, k_eff, MAX_KEPT, cand, &n_cand, red, ph, &total);

  const int counted = rank_keep<1>(cand, nc, k_eff, MAX_KEPT, sorted, &sh_vk, red, ph);
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
  draw_row(sorted, n, a.top_p, a.seed_key, a.row_seeds, a.positions, row, a.ids, a.u_out);
}

// One shard of a vocab-parallel sampled head (inferd_span_head_shard_sampled / inferd_sample_shard):
// A - C over the shard's columns (global indices first_col + c; tau from the shard's own tiles bounds
// the shard's v_k from below, which bounds the whole row's), the entries of the running candidate
// record cand_in appended to the list, D over the combined list, then the new record (cand_out)
// and / or E on its first MAX_KEPT entries (ids).  A record row is REC_WORDS uint64: the count
// (<= REC_ENTRIES) and the first REC_ENTRIES entries of {s >= v_k} of the columns seen so far, in
// the order, zero-filled; one entry beyond MAX_KEPT so that "more than MAX_KEPT qualify" survives
// the chain.  cand_out may alias cand_in (a row's record is in LDS before it is written).
struct ShardArgs {
  const u16* logits;                 // [rows][cols] row-major (null with cols == 0)
  const unsigned long long* keys;    // [rows][cols / 16] EPI_ARGMAX tile keys, or null
  int cols, first_col;
  float T;
  int top_k;
  float top_p;
  uint64_t seed_key;
  const uint64_t* row_seeds;
  const int32_t* positions;          // with ids
  const unsigned long long* cand_in; // [rows][REC_WORDS] or null
  unsigned long long* cand_out;      // [rows][REC_WORDS] or null
  int32_t* ids;                      // or null
  float* u_out;
  int32_t* flags;
};

__global__ __launch_bounds__(ST) void sample_shard_kernel(const ShardArgs a) {
  __shared__ int red[2][16];
  __shared__ int cnt[8][3];
  __shared__ unsigned long long cand[CAND_CAP + REC_ENTRIES];
  __shared__ unsigned long long sorted[REC_ENTRIES];
  __shared__ int n_cand;
  __shared__ float sh_vk;
  const int row = blockIdx.x, tid = threadIdx.x;
  const int cols = a.cols, n_tiles = cols >> 4;
  const u16* lrow = a.logits + (int64_t)row * cols;  // never read with cols == 0
  const u16x8* lrow8 = (const u16x8*)lrow;
  int ph = 0;

  uint32_t tk[KPT];
  tile_maxima(tk, a.keys ? a.keys + (int64_t)row * n_tiles : nullptr, lrow8, n_tiles);
  if (tid == 0) {
    n_cand = 0;
    sh_vk = -INFINITY;
  }
  if (tid < 24) (&cnt[0][0])[tid] = 0;
  __syncthreads();
  const float tau_s = tile_threshold(tk, n_tiles, a.top_k, a.T, cnt);
  gather_candidates(tk, lrow8, n_tiles, a.T, tau_s, a.first_col, cand, &n_cand);
  __syncthreads();
  int nc = n_cand;
  if (nc > CAND_CAP) {
    int total;
    nc = mass_ties(lrow, lrow8, cols, a.first_col, a.T, a.top_k < cols ? a.top_k : cols, REC_ENTRIES, cand, &n_cand,
                   red, ph, &total);
  }
  // the record of the shards before: its entries behind the shard's (nc <= CAND_CAP here)
  int n_in = 0;
  if (a.cand_in) {
    const unsigned long long* rec = a.cand_in + (int64_t)row * REC_WORDS;
    const unsigned long long c = rec[0];
    n_in = c < (unsigned long long)REC_ENTRIES ? (int)c : REC_ENTRIES;
    if (tid < n_in) cand[nc + tid] = rec[1 + tid];
  }
  __syncthreads();
  nc += n_in;
  // v_k of the columns so far: the min(top_k, columns)-th largest; a list shorter than top_k holds
  // every column seen (each side contributes its top_k or all it has)
  const int counted = rank_keep<2>(cand, nc, a.top_k < nc ? a.top_k : nc, REC_ENTRIES, sorted, &sh_vk, red, ph);
  const int n_rec = counted < REC_ENTRIES ? counted : REC_ENTRIES;
  if (a.cand_out && tid < REC_WORDS) {
    unsigned long long* rec = a.cand_out + (int64_t)row * REC_WORDS;
    rec[tid] = tid == 0 ? (unsigned long long)n_rec : (tid - 1 < n_rec ? sorted[tid - 1] : 0ull);
  }
  if (!a.ids || tid >= 64) return;
  if (tid == 0 && n_rec > MAX_KEPT && a.flags) atomicOr(a.flags, ERR_SAMPLE_OVERFLOW);
  const int n = n_rec < MAX_KEPT ? n_rec : MAX_KEPT;
  if (n < 1) {  // nothing compares (NaN logits, or no column at all): an in-range column
    if (tid == 0) {
      a.ids[row] = 0;
      if (a.u_out) a.u_out[row] = 0.f;
    }
    return;
  }
  draw_row(sorted, n, a.top_p, a.seed_key, a.row_seeds, a.positions, row, a.ids, a.u_out);
}

}  // namespace

void launch_sample(const u16* logits, int rows, int vocab, const unsigned long long* keys, float temperature,
                   int top_k, float top_p, uint64_t seed, const uint64_t* row_seeds, const int32_t* positions,
                   int32_t* ids, float* u_out, int32_t* flags, hipStream_t s) {
  const SampleArgs a = {logits, keys, vocab, temperature, top_k, top_p, splitmix64(seed), row_seeds, positions,
                        ids, u_out, flags};
  hipLaunchKernelGGL(sample_kernel, dim3(rows), dim3(ST), 0, s, a);
}

void launch_sample_shard(const u16* logits, int rows, int cols, int first_col, const unsigned long long* keys,
                         float temperature, int top_k, float top_p, uint64_t seed, const uint64_t* row_seeds,
                         const int32_t* positions, const unsigned long long* cand_in, unsigned long long* cand_out,
                         int32_t* ids, float* u_out, int32_t* flags, hipStream_t s) {
  const ShardArgs a = {logits, keys, cols, first_col, temperature, top_k, top_p, splitmix64(seed), row_seeds, positions,
                       cand_in, cand_out, ids, u_out, flags};
  hipLaunchKernelGGL(sample_shard_kernel, dim3(rows), dim3(ST), 0, s, a);
}

// Span runtime + C-ABI (include/inferd_span.h).
//
// An InferdSpan owns everything one pipeline stage needs on its GPU: the layer weights
// in the fragment-packed layout (fused [q;k;v] and [gate;up]), the embedding table
// (first span), final norm + packed lm_head (last span), the bf16 rope tables, the
// paged KV pool and the activation workspace.  inferd_span_forward chains the kernels
// of one Qwen3 decoder layer per span layer
// (qwen3_server_module.py:179-206):
//     rmsnorm -> qkv gemm -> qk-norm+rope+kv-write -> attention -> o gemm (+resid)
//     -> rmsnorm -> gate/up gemm (+SwiGLU) -> down gemm (+resid)
// with no allocation and no host synchronisation on the hot path.
#include <math.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/inferd_span.h"
#include "common.h"
#include "kernels.h"

static thread_local std::string g_err;

static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
int inferd_fail(int code, const std::string& msg) { return fail(code, msg); }

#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    if (_e != hipSuccess)                                                                  \
      return fail(INFERD_ERR_HIP, std::string(#expr " failed: ") + hipGetErrorString(_e)); \
  } while (0)

#define GEMM_TRY(call)                                                                      \
  do {                                                                                      \
    if (!(call)) return fail(INFERD_ERR_ARG, "internal: GEMM combination without a body"); \
  } while (0)

#define LAUNCH_CHECK()                                                                            \
  do {                                                                                            \
    hipError_t _e = hipGetLastError();                                                            \
    if (_e != hipSuccess)                                                                         \
      return fail(INFERD_ERR_HIP, std::string("kernel launch failed: ") + hipGetErrorString(_e)); \
  } while (0)

extern "C" const char* inferd_last_error(void) { return g_err.c_str(); }
extern "C" int inferd_abi_version(void) { return 5; }

namespace {

struct LayerW {
  u16* qkv = nullptr;     // packed [(H+2KV)*128][hidden]
  u16* o = nullptr;       // packed [hidden][H*128]
  u16* gateup = nullptr;  // packed [2*I][hidden]
  u16* down = nullptr;    // packed [hidden][I]
  u16* in_ln = nullptr;
  u16* post_ln = nullptr;
  u16* q_norm = nullptr;
  u16* k_norm = nullptr;
};

// tensor ids shared with oracle/weightgen.py
enum { T_Q = 0, T_K, T_V, T_O, T_QN, T_KN, T_INLN, T_POSTLN, T_GATE, T_UP, T_DOWN };
const uint32_t T_EMBED = 0xFFFF0000u, T_NORM = 0xFFFF0001u, T_LM = 0xFFFF0002u;
const float LINEAR_SCALE = 0.034641016151377546f;  // float32(0.02 * sqrt(3))
const float NORM_SCALE = 0.1f;

// kernel classes timed by inferd_span_profile_* (order = INFERD_PROF_* in the header)
enum { PROF_NORM = 0, PROF_QKV, PROF_ROPE, PROF_ATTN, PROF_O, PROF_GATEUP, PROF_DOWN, PROF_LMHEAD, PROF_NCLS };

uint64_t tensor_key(uint64_t seed, uint32_t tid) {
  return splitmix64(((seed & 0xFFFFFFFFull) << 32) | (uint64_t)tid);
}

// Decode q/k/v K-slices (reduced by the fused decode attention): the measured optimum
// (other slice counts, like every other A/B variant, live in tools/ lab
// builds -- the product library has one path per op and reads no environment).
#define QKV_KSL 2

}  // namespace

struct InferdSpan {
  InferdSpanConfig cfg;
  std::vector<LayerW> layers;
  u16* embed = nullptr;
  u16* final_norm = nullptr;
  u16* lm_head = nullptr;
  u16* cos_t = nullptr;
  u16* sin_t = nullptr;
  u16* kv_pool = nullptr;
  size_t kv_layer_elems = 0;
  // workspace
  u16 *xn = nullptr, *qkv = nullptr, *q = nullptr, *attn = nullptr, *act = nullptr, *h = nullptr,
      *last = nullptr;
  float* attn_ws = nullptr;
  size_t attn_ws_bytes = 0;
  // RMSNorms at the reference's rounding points (qwen3_server_module.py:19-25).  On the decode
  // GEMV path (<= 64 rows) the o and down GEMVs add the row sums of squares of their outputs
  // into SSQ slots (kernels.h DecodeNorm; slot 2l: layer l's o -> its gate/up, slot 2l+1: layer
  // l's down -> layer l+1's q/k/v), and those GEMVs normalise their A fragments from them; the
  // layer-0 rmsnorm_kernel zeroes the slots at the start of each such forward.  Otherwise (a
  // span's first layer, prefill) rmsnorm_kernel writes the normed rows to xn.
  unsigned long long* ssq = nullptr;
  GemmWs gws;                 // prefill tail-split workspace (per span: spans never share tickets)
  float* qkv_part = nullptr;  // decode split-K q/k/v partials [QKV_KSL][16][qkv_rows]
  unsigned long long* argmax_partial = nullptr;
  // sampled decoding (inferd_span_set_sampling): with sampling_on the head's next_ids are a draw
  // (sampling.hip) instead of argmax_reduce; sample_logits [64][vocab] holds the logits of calls
  // that pass none (allocated by the first set_sampling; a vocab-parallel shard's [64][head_rows]
  // for inferd_span_head_shard_sampled at creation: a call there may sit in a graph capture)
  bool sampling_on = false;
  InferdSampling sampling{};
  u16* sample_logits = nullptr;
  int32_t* err = nullptr;
  std::vector<void*> allocs;
  // optional per-kernel-class timing with HIP events on the launch stream
  bool prof_on = false;
  std::vector<hipEvent_t> prof_events;
  std::vector<int> prof_class;
  size_t prof_used = 0;

  ~InferdSpan() {
    for (hipEvent_t e : prof_events) (void)hipEventDestroy(e);
    for (void* p : allocs) (void)hipFree(p);
    gemm_ws_free(&gws);
  }
  // returns the pair index or -1
  long prof_begin(int cls, hipStream_t st) {
    if (!prof_on || prof_used + 2 > prof_events.size()) return -1;
    long i = (long)prof_used;
    prof_used += 2;
    prof_class[i / 2] = cls;
    (void)hipEventRecord(prof_events[i], st);
    return i;
  }
  void prof_end(long i, hipStream_t st) {
    if (i >= 0) (void)hipEventRecord(prof_events[i + 1], st);
  }
  int alloc(void** p, size_t bytes) {
    hipError_t e = hipMalloc(p, bytes < 256 ? 256 : bytes);
    if (e != hipSuccess) {
      *p = nullptr;
      return fail(INFERD_ERR_HIP, "hipMalloc(" + std::to_string(bytes) + ") failed: " + hipGetErrorString(e));
    }
    allocs.push_back(*p);
    return INFERD_OK;
  }
  int qkv_rows() const { return (cfg.heads + 2 * cfg.kv_heads) * HEAD_DIM; }
  // the halves of span-local layer l this span runs (InferdSpanConfig skip_first_attn /
  // skip_last_mlp); only layers with an attention half own a KV pool layer
  // has_qkv: input_layernorm + q/k/v weights; has_attn: the attention kernel and a KV pool
  // layer; has_o: o_proj + residual
  bool first_no_attn() const { return cfg.skip_first_attn || cfg.o_split_first; }
  bool last_qkv_only(int l) const { return l == cfg.n_layers - 1 && cfg.qkv_split_last; }
  // layer l is the MLP half a span starts at / ends in a hand-off record (before its attention or o)
  bool mlp_only(int l) const { return l == 0 && cfg.skip_first_attn; }
  bool ends_in_record(int l) const { return l == cfg.n_layers - 1 && (cfg.o_split_last || cfg.qkv_split_last); }
  // layer l's q/k/v rows arrive in x_in's record: pure decode calls at a q/k/v|attention boundary
  bool qkv_in_record(int l, bool decode) const { return l == 0 && cfg.qkv_split_first && decode; }
  bool has_qkv(int l) const { return !(l == 0 && first_no_attn()); }
  bool has_attn(int l) const { return has_qkv(l) && !last_qkv_only(l); }
  bool has_o(int l) const { return !mlp_only(l) && !ends_in_record(l); }
  bool has_mlp(int l) const { return !(l == cfg.n_layers - 1 && cfg.skip_last_mlp) && !ends_in_record(l); }
  // the last layer of a span that ends inside the layer's gate/up projection computes part of it
  bool has_gateup(int l) const { return has_mlp(l) || (l == cfg.n_layers - 1 && cfg.gateup_split_last); }
  int kv_layers() const { return cfg.n_layers - (first_no_attn() ? 1 : 0) - (cfg.qkv_split_last ? 1 : 0); }
  // the lm_head rows this span owns (InferdSpanConfig head_first / head_rows): all of them with
  // has_lm_head, else its vocab-parallel shard (0 rows: none)
  int lm_rows() const { return cfg.has_lm_head ? cfg.vocab : cfg.head_rows; }
  int lm_first() const { return cfg.has_lm_head ? 0 : cfg.head_first; }
  u16* kv_of(int l) const { return kv_pool + kv_layer_elems * (l - (first_no_attn() ? 1 : 0)); }
};

#define ALLOC(ptr, bytes)                                   \
  do {                                                      \
    int _rc = s->alloc((void**)&(ptr), (size_t)(bytes));    \
    if (_rc) return _rc;                                    \
  } while (0)

extern "C" int inferd_span_create(const InferdSpanConfig* cfg, InferdSpan** out) {
  if (!cfg || !out) return fail(INFERD_ERR_ARG, "null argument");
  const InferdSpanConfig& c = *cfg;
  if (c.head_dim != HEAD_DIM) return fail(INFERD_ERR_ARG, "head_dim must be 128");
  if ((int64_t)c.max_seqs * c.heads > 16384) return fail(INFERD_ERR_ARG, "max_seqs * heads must be <= 16384");
  if (c.kv_heads <= 0 || c.heads % c.kv_heads != 0 || c.heads / c.kv_heads > 16)
    return fail(INFERD_ERR_ARG, "heads must be a multiple of kv_heads with group size <= 16");
  if (c.hidden % 128 || c.intermediate % 64 || c.vocab % 16)
    return fail(INFERD_ERR_ARG, "hidden % 128, intermediate % 64 and vocab % 16 must be 0");
  if (c.n_layers < 0 || c.max_tokens <= 0 || c.max_seqs <= 0 || c.kv_pages <= 0 || c.max_positions <= 0)
    return fail(INFERD_ERR_ARG, "bad span sizes");
  if (c.has_lm_head && c.max_seqs > 64)
    return fail(INFERD_ERR_ARG, "a span with lm_head takes max_seqs <= 64 (the greedy argmax is per call of <= 64 rows)");
  if (c.kv_pages > (1 << 24)) return fail(INFERD_ERR_ARG, "kv_pages must be <= 2^24");
  if ((c.skip_first_attn | c.skip_last_mlp) & ~1) return fail(INFERD_ERR_ARG, "skip_first_attn / skip_last_mlp are 0 or 1");
  if (c.skip_first_attn && c.has_embed)
    return fail(INFERD_ERR_ARG, "a span with the embedding starts at a layer's attention half (skip_first_attn = 0)");
  if (c.skip_last_mlp && c.has_lm_head)
    return fail(INFERD_ERR_ARG, "a span with lm_head ends at a layer's MLP half (skip_last_mlp = 0)");
  if ((c.skip_first_attn || c.skip_last_mlp) && c.n_layers < 1)
    return fail(INFERD_ERR_ARG, "a half-layer boundary needs n_layers >= 1");
  if (c.skip_first_attn && c.skip_last_mlp && c.n_layers == 1)
    return fail(INFERD_ERR_ARG, "a one-layer span cannot skip both of its halves");
  for (int32_t col : {c.gateup_split_first, c.gateup_split_last})
    if (col < 0 || col % 128 || (col && col >= c.intermediate))
      return fail(INFERD_ERR_ARG, "gate/up split columns: 0, or a multiple of 128 below intermediate");
  if ((c.gateup_split_first && !c.skip_first_attn) || (c.gateup_split_last && !c.skip_last_mlp))
    return fail(INFERD_ERR_ARG, "a gate/up split refines a half-layer boundary (skip_first_attn / skip_last_mlp)");
  if ((c.o_split_first | c.o_split_last) & ~1) return fail(INFERD_ERR_ARG, "o_split_first / o_split_last are 0 or 1");
  if ((c.o_split_first && (c.skip_first_attn || c.has_embed)) || (c.o_split_last && (c.skip_last_mlp || c.has_lm_head)))
    return fail(INFERD_ERR_ARG, "an attention|o boundary excludes a half-layer boundary at the same end, the "
                                "embedding (first) and lm_head (last)");
  if ((c.o_split_first || c.o_split_last) && c.n_layers < 1)
    return fail(INFERD_ERR_ARG, "an attention|o boundary needs n_layers >= 1");
  if ((c.qkv_split_first | c.qkv_split_last) & ~1) return fail(INFERD_ERR_ARG, "qkv_split_first / qkv_split_last are 0 or 1");
  if ((c.qkv_split_first && (c.skip_first_attn || c.o_split_first || c.has_embed)) ||
      (c.qkv_split_last && (c.skip_last_mlp || c.o_split_last || c.has_lm_head)))
    return fail(INFERD_ERR_ARG, "a q/k/v|attention boundary excludes another sub-layer boundary at the same end, the "
                                "embedding (first) and lm_head (last)");
  if ((c.qkv_split_first || c.qkv_split_last) && c.n_layers < 1)
    return fail(INFERD_ERR_ARG, "a q/k/v|attention boundary needs n_layers >= 1");
  if (c.head_rows < 0 || c.head_first < 0 || c.head_rows % 16 || c.head_first % 16 ||
      (int64_t)c.head_first + c.head_rows > c.vocab)
    return fail(INFERD_ERR_ARG, "lm_head shard: rows [head_first, head_first + head_rows) within the vocabulary, "
                                "multiples of 16");
  if (c.final_norm_out & ~1) return fail(INFERD_ERR_ARG, "final_norm_out is 0 or 1");
  if (c.has_lm_head && (c.head_rows || c.final_norm_out))
    return fail(INFERD_ERR_ARG, "a span with the whole lm_head has no shard and no final_norm_out");
  if (c.final_norm_out && (c.skip_last_mlp || c.o_split_last || c.qkv_split_last || c.max_seqs > 64))
    return fail(INFERD_ERR_ARG, "a final_norm_out span ends at a layer boundary and takes max_seqs <= 64");
  if (c.n_layers == 1 && ((c.o_split_first && (c.o_split_last || c.skip_last_mlp)) ||
                          (c.o_split_last && c.skip_first_attn) ||
                          (c.qkv_split_last && (c.skip_first_attn || c.o_split_first || c.qkv_split_first)) ||
                          (c.qkv_split_first && c.o_split_last)))
    return fail(INFERD_ERR_ARG, "a one-layer span cannot end before the part it starts at");
  InferdSpan* s = new InferdSpan();
  s->cfg = c;
  const int h = c.hidden, I = c.intermediate, H = c.heads, KV = c.kv_heads;
  s->layers.resize(c.n_layers);
  int rc = 0;
  auto bail = [&](int code) {
    delete s;
    return code;
  };
#define SALLOC(ptr, bytes)                                  \
  do {                                                      \
    rc = s->alloc((void**)&(ptr), (size_t)(bytes));         \
    if (rc) return bail(rc);                                \
  } while (0)
  for (int l = 0; l < c.n_layers; ++l) {
    LayerW& L = s->layers[l];
    if (s->has_qkv(l)) {
      SALLOC(L.qkv, (size_t)s->qkv_rows() * h * 2);
      SALLOC(L.in_ln, (size_t)h * 2);
      SALLOC(L.q_norm, HEAD_DIM * 2);
      SALLOC(L.k_norm, HEAD_DIM * 2);
    }
    if (s->has_o(l)) SALLOC(L.o, (size_t)h * H * HEAD_DIM * 2);
    if (s->has_gateup(l)) {  // a gate/up boundary's sender owns gate/up too
      SALLOC(L.gateup, (size_t)2 * I * h * 2);
      SALLOC(L.post_ln, (size_t)h * 2);
    }
    if (s->has_mlp(l)) SALLOC(L.down, (size_t)h * I * 2);
  }
  if (c.has_embed) SALLOC(s->embed, (size_t)c.vocab * h * 2);
  if (c.has_lm_head || c.final_norm_out) SALLOC(s->final_norm, (size_t)h * 2);
  if (s->lm_rows() > 0) SALLOC(s->lm_head, (size_t)s->lm_rows() * h * 2);
  // rope tables
  SALLOC(s->cos_t, (size_t)c.max_positions * 64 * 2);
  SALLOC(s->sin_t, (size_t)c.max_positions * 64 * 2);
  {
    float inv[64];
    for (int i = 0; i < 64; ++i) {
      // HF default rope: 1 / theta ** (arange(0, d, 2) / d) evaluated in fp32 (torch pow)
      float e = (float)(2 * i) / (float)HEAD_DIM;
      inv[i] = 1.0f / powf(c.rope_theta, e);
    }
    float* dinv = nullptr;
    SALLOC(dinv, sizeof(inv));
    if (hipMemcpy(dinv, inv, sizeof(inv), hipMemcpyHostToDevice) != hipSuccess)
      return bail(fail(INFERD_ERR_HIP, "rope upload failed"));
    launch_rope_table(dinv, c.max_positions, s->cos_t, s->sin_t, 0);
  }
  // KV pool
  // whole super-pages (common.h: KV_SUPER)
  s->kv_layer_elems = (size_t)((c.kv_pages + KV_SUPER - 1) / KV_SUPER * KV_SUPER) * 2 * KV * KV_BLOCK_ELEMS;
  if (s->kv_layers() > 0) {
    SALLOC(s->kv_pool, s->kv_layer_elems * s->kv_layers() * 2);
    if (hipMemset(s->kv_pool, 0, s->kv_layer_elems * s->kv_layers() * 2) != hipSuccess)
      return bail(fail(INFERD_ERR_HIP, "kv memset failed"));
  }
  // workspace
  const size_t Mx = c.max_tokens;
  SALLOC(s->xn, ((Mx + 15) & ~(size_t)15) * h * 2);  // decode: whole packed tiles
  SALLOC(s->qkv, Mx * s->qkv_rows() * 2);
  SALLOC(s->q, Mx * H * HEAD_DIM * 2);
  SALLOC(s->attn, ((Mx + 15) & ~(size_t)15) * H * HEAD_DIM * 2);  // decode: whole packed tiles
  SALLOC(s->act, ((Mx + 15) & ~(size_t)15) * I * 2);  // decode: whole 16-row packed tiles
  SALLOC(s->h, ((Mx + 15) & ~(size_t)15) * h * 2);  // decode: whole packed tiles
  SALLOC(s->last, (((size_t)c.max_seqs + 15) & ~(size_t)15) * h * 2);  // whole packed tiles
  s->attn_ws_bytes = attn_decode_ws_bytes(c.max_seqs, H, c.max_positions);
  SALLOC(s->attn_ws, s->attn_ws_bytes);
  if (hipMemset(s->attn_ws, 0, s->attn_ws_bytes) != hipSuccess) return bail(fail(INFERD_ERR_HIP, "memset failed"));
  SALLOC(s->ssq, (size_t)(2 * c.n_layers) * SSQ_SLOT_WORDS * 8);
  if (s->lm_rows() > 0) SALLOC(s->argmax_partial, (size_t)(s->lm_rows() / 16) * 64 * 8);
  if (c.head_rows > 0) SALLOC(s->sample_logits, (size_t)64 * c.head_rows * 2);
  SALLOC(s->qkv_part, (size_t)QKV_KSL * 16 * s->qkv_rows() * 4);
  // the prefill tail split's workspace, once (a forward never allocates): only spans whose
  // calls can reach the 256x256 GEMMs (>= 512 rows) need it
  s->gws.split = c.max_tokens >= 512;
  if (gemm_ws_alloc(&s->gws) != (int)hipSuccess) return bail(fail(INFERD_ERR_HIP, "tail-split workspace allocation failed"));
  SALLOC(s->err, 256);
  if (hipMemset(s->err, 0, 4) != hipSuccess) return bail(fail(INFERD_ERR_HIP, "memset failed"));
  if (hipDeviceSynchronize() != hipSuccess) return bail(fail(INFERD_ERR_HIP, "init sync failed"));
  *out = s;
  return INFERD_OK;
#undef SALLOC
}

extern "C" void inferd_span_destroy(InferdSpan* span) { delete span; }

// bf16 elements of a forward / step call's x_in (which = 0) or x_out (which = 1): the hidden rows
// plus the record a sub-layer boundary carries (gate/up: the packed act over 16-row tiles in calls
// of <= 64 rows; attention|o: the attention output, 16-row tiles in pure decode calls; q/k/v|
// attention: the raw q/k/v rows in pure decode calls), or a final_norm_out span's normed last rows
// over 16-row tiles.  A pure function of the config: hosts size buffers before they create a span.
extern "C" int64_t inferd_span_io_elems(const InferdSpanConfig* c, int32_t n_tokens, int32_t n_seqs, int32_t decode,
                                        int32_t which) {
  if (!c || n_tokens < 0 || n_seqs < 0 || (which != 0 && which != 1)) {
    g_err = "inferd_span_io_elems: a config, n_tokens / n_seqs >= 0 and which 0 (x_in) or 1 (x_out)";
    return -1;
  }
  const int64_t M = n_tokens, h = c->hidden;
  const bool gemv = M <= 64;
  const int64_t rec = (M + 15) / 16 * 16 * (int64_t)c->intermediate;
  const int64_t orec = (decode && gemv ? (M + 15) / 16 * 16 : M) * (int64_t)c->heads * c->head_dim;
  const int64_t qrec = decode ? M * (int64_t)(c->heads + 2 * c->kv_heads) * c->head_dim : 0;
  if (which == 0)
    return M * h + (gemv && c->gateup_split_first ? rec : 0) + (c->o_split_first ? orec : 0) +
           (c->qkv_split_first ? qrec : 0);
  if (c->final_norm_out) return ((int64_t)n_seqs + 15) / 16 * 16 * h;
  return M * h + (gemv && c->gateup_split_last ? rec : 0) + (c->o_split_last ? orec : 0) +
         (c->qkv_split_last ? qrec : 0);
}

extern "C" int inferd_span_get_config(const InferdSpan* span, InferdSpanConfig* out) {
  if (!span || !out) return fail(INFERD_ERR_ARG, "null argument");
  *out = span->cfg;
  return INFERD_OK;
}

// ------------------------------------------------------------------ weights
namespace {
struct Target {
  u16* dst;       // destination base
  int packed;     // 1: fragment-pack at n-tile offset
  int64_t rows, cols;
  uint32_t tid_idx;
  int64_t elem0 = 0;  // generator counter of the first element (an lm_head shard: head_first * hidden)
};

int resolve_layer(InferdSpan* s, int layer, const char* name, Target* t);
bool owns_weight(const InferdSpan* s, int layer, const char* name);

int resolve(InferdSpan* s, int layer, const char* name, Target* t) {
  const InferdSpanConfig& c = s->cfg;
  const int h = c.hidden;
  if (layer < 0) {
    if (!strcmp(name, "embed_tokens") && s->embed) { *t = {s->embed, 0, c.vocab, h, T_EMBED}; return 0; }
    if (!strcmp(name, "norm") && s->final_norm) { *t = {s->final_norm, 0, 1, h, T_NORM}; return 0; }
    if (!strcmp(name, "lm_head") && s->lm_head) {
      *t = {s->lm_head, 1, s->lm_rows(), h, T_LM, (int64_t)s->lm_first() * h};
      return 0;
    }
    return fail(INFERD_ERR_ARG, std::string("unknown/unowned global weight ") + name);
  }
  if (layer >= c.n_layers) return fail(INFERD_ERR_ARG, "layer index out of span");
  if (resolve_layer(s, layer, name, t)) return INFERD_ERR_ARG;
  // by ownership, not by t->dst: a sub-tensor of an absent part (k_proj, up_proj) resolves to
  // an offset from a null base
  if (!owns_weight(s, layer, name))
    return fail(INFERD_ERR_ARG, std::string(name) + ": layer " + std::to_string(layer) +
                                    " of this span runs only its other half / part (skip_first_attn, skip_last_mlp, o_split_*, "
                                    "qkv_split_last)");
  return 0;
}

int resolve_layer(InferdSpan* s, int layer, const char* name, Target* t) {
  const InferdSpanConfig& c = s->cfg;
  const int h = c.hidden, I = c.intermediate, H = c.heads, KV = c.kv_heads;
  LayerW& L = s->layers[layer];
  const int64_t qrows = (int64_t)H * HEAD_DIM, kvrows = (int64_t)KV * HEAD_DIM;
  if (!strcmp(name, "q_proj")) { *t = {L.qkv, 1, qrows, h, T_Q}; return 0; }
  if (!strcmp(name, "k_proj")) { *t = {L.qkv + qrows * h, 1, kvrows, h, T_K}; return 0; }
  if (!strcmp(name, "v_proj")) { *t = {L.qkv + (qrows + kvrows) * h, 1, kvrows, h, T_V}; return 0; }
  if (!strcmp(name, "o_proj")) { *t = {L.o, 1, h, qrows, T_O}; return 0; }
  if (!strcmp(name, "gate_proj")) { *t = {L.gateup, 1, I, h, T_GATE}; return 0; }
  if (!strcmp(name, "up_proj")) { *t = {L.gateup + (int64_t)I * h, 1, I, h, T_UP}; return 0; }
  if (!strcmp(name, "down_proj")) { *t = {L.down, 1, h, I, T_DOWN}; return 0; }
  if (!strcmp(name, "q_norm")) { *t = {L.q_norm, 0, 1, HEAD_DIM, T_QN}; return 0; }
  if (!strcmp(name, "k_norm")) { *t = {L.k_norm, 0, 1, HEAD_DIM, T_KN}; return 0; }
  if (!strcmp(name, "input_layernorm")) { *t = {L.in_ln, 0, 1, h, T_INLN}; return 0; }
  if (!strcmp(name, "post_attention_layernorm")) { *t = {L.post_ln, 0, 1, h, T_POSTLN}; return 0; }
  return fail(INFERD_ERR_ARG, std::string("unknown layer weight ") + name);
}

// 1 if span-local layer `layer` runs the half that weight `name` belongs to
bool owns_weight(const InferdSpan* s, int layer, const char* name) {
  if (!strcmp(name, "down_proj")) return s->has_mlp(layer);
  if (!strcmp(name, "o_proj")) return s->has_o(layer);
  if (!strcmp(name, "gate_proj") || !strcmp(name, "up_proj") || !strcmp(name, "post_attention_layernorm"))
    return s->has_gateup(layer);
  return s->has_qkv(layer);
}
// packed sub-blocks start at an n-tile boundary: offset rows*K elements == (rows/16)*KT*512
}  // namespace

extern "C" int inferd_span_set_weight(InferdSpan* s, int32_t layer, const char* name,
                                      const void* src, int64_t rows, int64_t cols, void* stream) {
  if (!s || !name || !src) return fail(INFERD_ERR_ARG, "null argument");
  Target t;
  if (resolve(s, layer, name, &t)) return INFERD_ERR_ARG;
  if (rows != t.rows || cols != t.cols)
    return fail(INFERD_ERR_ARG, std::string("shape mismatch for ") + name + ": expected " +
                                    std::to_string(t.rows) + "x" + std::to_string(t.cols));
  hipStream_t st = (hipStream_t)stream;
  if (t.packed)
    launch_pack((const u16*)src, cols, (int)rows, (int)cols, t.dst, st);
  else
    HIP_TRY(hipMemcpyAsync(t.dst, src, rows * cols * 2, hipMemcpyDeviceToDevice, st));
  LAUNCH_CHECK();
  return INFERD_OK;
}

extern "C" int inferd_span_init_synthetic(InferdSpan* s, uint64_t seed, void* stream) {
  if (!s) return fail(INFERD_ERR_ARG, "null span");
  hipStream_t st = (hipStream_t)stream;
  const InferdSpanConfig& c = s->cfg;
  // temp buffer for the largest row-major tensor that needs packing
  int64_t biggest = (int64_t)c.hidden * (c.intermediate > c.heads * HEAD_DIM ? c.intermediate : c.heads * HEAD_DIM);
  if ((int64_t)s->lm_rows() * c.hidden > biggest) biggest = (int64_t)s->lm_rows() * c.hidden;
  u16* tmp = nullptr;
  HIP_TRY(hipMalloc((void**)&tmp, biggest * 2));
  static const char* layer_names[] = {"input_layernorm", "post_attention_layernorm", "q_norm", "k_norm",
                                      "q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj",
                                      "down_proj"};
  auto gen = [&](int layer, const char* name) -> int {
    Target t;
    if (resolve(s, layer, name, &t)) return INFERD_ERR_ARG;
    const bool is_norm = strstr(name, "norm") != nullptr;
    const float scale = is_norm ? NORM_SCALE : LINEAR_SCALE;
    const float center = is_norm ? 1.0f : 0.0f;
    const uint32_t tid = layer < 0 ? t.tid_idx : (uint32_t)((c.first_layer + layer) * 16 + t.tid_idx);
    const uint64_t key = tensor_key(seed, tid) + (uint64_t)t.elem0;
    const int64_t n = t.rows * t.cols;
    if (t.packed) {
      launch_weightgen(tmp, n, key, scale, center, st);
      launch_pack(tmp, t.cols, (int)t.rows, (int)t.cols, t.dst, st);
    } else {
      launch_weightgen(t.dst, n, key, scale, center, st);
    }
    return INFERD_OK;
  };
  int rc = 0;
  for (int l = 0; l < c.n_layers && !rc; ++l)
    for (const char* nm : layer_names)
      if (owns_weight(s, l, nm) && (rc = gen(l, nm))) break;
  if (!rc && c.has_embed) rc = gen(-1, "embed_tokens");
  if (!rc && s->final_norm) rc = gen(-1, "norm");
  if (!rc && s->lm_head) rc = gen(-1, "lm_head");
  hipError_t e = hipStreamSynchronize(st);
  (void)hipFree(tmp);
  if (rc) return rc;
  if (e != hipSuccess) return fail(INFERD_ERR_HIP, std::string("synthetic init: ") + hipGetErrorString(e));
  return INFERD_OK;
}

// ------------------------------------------------------------------ forward
static int check_batch(const InferdSpan* s, const InferdBatch* b) {
  const InferdSpanConfig& c = s->cfg;
  if (!b) return fail(INFERD_ERR_ARG, "null batch");
  if (b->n_tokens <= 0 || b->n_tokens > c.max_tokens)
    return fail(INFERD_ERR_ARG, "n_tokens out of range (max_tokens=" + std::to_string(c.max_tokens) + ")");
  if (b->n_seqs <= 0 || b->n_seqs > c.max_seqs) return fail(INFERD_ERR_ARG, "n_seqs out of range");
  if (b->max_ctx_len <= 0 || b->max_ctx_len > c.max_positions)
    return fail(INFERD_ERR_ARG, "max_ctx_len out of range");
  if (b->decode && b->n_tokens != b->n_seqs) return fail(INFERD_ERR_ARG, "decode batch needs one token per sequence");
  if (!b->seq_start || !b->positions || !b->ctx_lens || !b->block_table)
    return fail(INFERD_ERR_ARG, "batch arrays missing");
  if ((int64_t)b->max_pages * KV_PAGE < b->max_ctx_len) return fail(INFERD_ERR_ARG, "block table too narrow");
  return INFERD_OK;
}

// the attention's view of a batch
static AttnBatch to_attn(const InferdBatch* b) {
  AttnBatch a;
  a.seq_start = b->seq_start;
  a.positions = b->positions;
  a.ctx_lens = b->ctx_lens;
  a.block_table = b->block_table;
  a.max_pages = b->max_pages;
  a.B = b->n_seqs;
  a.M = b->n_tokens;
  a.max_q_len = b->max_q_len;
  a.max_ctx = b->max_ctx_len;
  return a;
}

namespace {
// One forward call, on its caller's stack: the arguments (the first seven members), what follows
// from them for the whole call, and the residual cursor.  Every helper returns INFERD_OK or fail().
struct Forward {
  InferdSpan* const s;
  const InferdBatch* const b;
  const void* const x_in;
  // a final_norm_out span: the caller's x_out receives the final-normed last rows (normed_out,
  // head()); the last layer's hidden rows stay in the workspace, as on a span with lm_head
  void* const x_out;
  void* const normed_out;
  void* const layer_out;
  const hipStream_t st;
  const InferdSpanConfig& c = s->cfg;
  const int M = b->n_tokens, B = b->n_seqs;
  const int h = c.hidden, I = c.intermediate, H = c.heads, KV = c.kv_heads, qkvN = s->qkv_rows();
  const float scale = 1.0f / sqrtf((float)HEAD_DIM);
  const AttnBatch ab = to_attn(b);
  // RMSNorms (qwen3_server_module.py:19-25, :173-176): see InferdSpan::ssq_in.  gemv: every
  // projection of this call is a decode GEMV (<= 64 rows), so the o / down GEMVs can hand the
  // next norm its row sums of squares.
  const bool gemv = M <= 64;
  // decode: the residual stream between layers (and h1 inside a layer) fragment-packed
  // (common.h packed_index) for the GEMVs that read it; the input and the last layer's
  // output stay row-major, and so does every layer's output when layer_out asks for them
  const bool pkx = gemv && !layer_out && h % 128 == 0 && I % 128 == 0;
  // decode: the attention output goes to the o projection's GEMV fragment-packed (also the
  // layout of an attention|o boundary record's second part)
  const bool pk_o = b->decode && gemv && !gemm_uses_tiled(M, h, H * HEAD_DIM, EPI_RESID);
  // a q/k/v|attention boundary: a pure decode call hands over the raw q/k/v rows behind x
  // (qkv_split_*); other calls hand over x and the receiver runs the whole layer
  const bool qrec = b->decode, q_in = c.qkv_split_first && qrec;
  // decode q/k/v K-slices (reduced inside the fused attention): M <= 16 and K/32 divisible by 4 * slices
  const int ksl = (b->decode && M <= 16 && (h / 32) % (4 * QKV_KSL) == 0) ? QKV_KSL : 1;
  const u16* x = nullptr;  // the residual stream: the current layer's input
  bool x_packed = false;   // x is fragment-packed
  // the first RMSNorm launch (layer 0's input norm) also runs the embedding gather and a
  // pending graph scheduler step (kernels.h NormPrologue): two graph nodes fewer per step
  NormPrologue pro;

  unsigned long long* slot(int i) const { return s->ssq + (size_t)i * SSQ_SLOT_WORDS; }
  // the second part of a hand-off record, behind its [M][hidden] first part
  u16* in_rec() const { return (u16*)x_in + (size_t)M * h; }
  u16* out_rec() const { return (u16*)x_out + (size_t)M * h; }
  // the span's input as its output (no layers), or as the first part of a one-layer span's record
  int copy_input_out() {
    if (x != (const u16*)x_out) HIP_TRY(hipMemcpyAsync(x_out, x, (size_t)M * h * 2, hipMemcpyDeviceToDevice, st));
    return INFERD_OK;
  }

  // ---- input_layernorm -> q/k/v projection (on a q_only layer of a call that hands over x
  // alone, only the span's first norm launch when it carries the prologue: the embedding /
  // scheduler step).  *roped: the projection's epilogue ran QK-norm + RoPE + the cache write.
  int qkv(int l, bool* roped) {
    const LayerW& W = s->layers[l];
    // a q/k/v|attention boundary: q_only -- this (last) layer runs its norm and q/k/v projection
    // only, into the record behind x (pure decode calls; other calls hand over x alone)
    const bool q_only = s->last_qkv_only(l);
    const u16* a_in = x;
    DecodeNorm dn = {DN_NONE, c.rms_eps, nullptr, nullptr};
    if (gemv && l > 0) {
      dn = {DN_EXACT, c.rms_eps, slot(2 * l - 1), W.in_ln};
    } else if (!(q_only && !qrec && l > 0)) {
      const long pe = s->prof_begin(PROF_NORM, st);
      launch_rmsnorm(x, h, nullptr, 0, W.in_ln, s->xn, h, M, h, c.rms_eps, st, false, gemv ? s->ssq : nullptr,
                     2 * c.n_layers, l == 0 ? &pro : nullptr);
      s->prof_end(pe, st);
      a_in = s->xn;
    }
    if (q_only && !qrec) return INFERD_OK;
    const long pe = s->prof_begin(PROF_QKV, st);
    // prefill: q/k norm + RoPE and the K/V cache write in the projection's epilogue when
    // the persistent GEMM runs it (else the separate qk_norm_rope_kv launch in attention())
    if (ksl > 1) {
      launch_gemm_decode_partial(a_in, h, W.qkv, M, qkvN, h, ksl, s->qkv_part, dn, st,
                                 (x_packed && a_in == x) ? GEMM_PACK_A : 0);
      // the record's q/k/v rows: the slices summed as the fused attention sums them
      if (q_only) launch_qkv_reduce(s->qkv_part, ksl, M, qkvN, out_rec(), st);
    } else {
      if (!b->decode && !q_only) {
        const QkvEpilogue qe = {b->positions, b->slots, W.q_norm, W.k_norm, s->cos_t, s->sin_t, s->q, s->kv_of(l),
                                H, KV, c.rms_eps};
        *roped = launch_gemm_qkv_fused(a_in, h, W.qkv, M, qkvN, h, qe, st);
      }
      if (!*roped)
        GEMM_TRY(launch_gemm(a_in, h, W.qkv, M, qkvN, h, q_only ? out_rec() : s->qkv, qkvN, nullptr, 0, EPI_NONE,
                             nullptr, st, &s->gws, &dn, nullptr, (x_packed && a_in == x) ? GEMM_PACK_A : 0));
    }
    s->prof_end(pe, st);
    return INFERD_OK;
  }

  // ---- attention into dst.  q_recv: this (first) layer's q/k/v rows arrive in x_in's record
  int attention(int l, bool q_recv, bool roped, u16* dst) {
    const LayerW& W = s->layers[l];
    u16* kv_l = s->kv_of(l);
    if (!b->decode && !roped) {
      const long pe = s->prof_begin(PROF_ROPE, st);
      launch_qk_norm_rope_kv(s->qkv, qkvN, b->positions, b->slots, W.q_norm, W.k_norm, s->cos_t, s->sin_t, s->q,
                             kv_l, M, H, KV, c.rms_eps, st);
      s->prof_end(pe, st);
    }
    // decode: QK-norm + RoPE + cache write inside attention, on the record's q/k/v rows, the
    // projection's K-slices (part) or the projection's rows
    const u16* rows = q_recv ? in_rec() : (ksl > 1 ? nullptr : s->qkv);
    const float* part = (!q_recv && ksl > 1) ? s->qkv_part : nullptr;
    const long pe = s->prof_begin(PROF_ATTN, st);
    if (b->decode)
      launch_attn_decode_fused(rows, qkvN, W.q_norm, W.k_norm, s->cos_t, s->sin_t, c.rms_eps, kv_l, ab, H, KV, scale,
                               dst, s->attn_ws, st, part, part ? ksl : 0, pk_o);
    else
      launch_attn_prefill(s->q, kv_l, ab, H, KV, scale, dst, st);
    s->prof_end(pe, st);
    return INFERD_OK;
  }

  // ---- h1 = x + o_proj(attn)   (in place when x == s->h: same-element read-then-write)
  int o_proj(int l, const u16* attn_src, u16* h1, bool h1_packed) {
    const long pe = s->prof_begin(PROF_O, st);
    GEMM_TRY(launch_gemm(attn_src, H * HEAD_DIM, s->layers[l].o, M, h, H * HEAD_DIM, h1, h, x, h, EPI_RESID, nullptr, st,
                         &s->gws, nullptr, gemv ? slot(2 * l) : nullptr,
                         (pk_o ? GEMM_PACK_A : 0) | (x_packed ? GEMM_PACK_R : 0) | (h1_packed ? GEMM_PACK_C : 0)));
    s->prof_end(pe, st);
    return INFERD_OK;
  }

  // ---- post_attention_layernorm -> gate/up (+SwiGLU) into actb -> out = r + down(actb), r being h1.
  // A gate/up boundary's receiver: columns [0, c0) of actb (the record's act) arrived with x_in.
  int mlp(int l, const u16* r, bool r_packed, int c0, u16* actb, u16* out, bool out_packed) {
    const LayerW& W = s->layers[l];
    // a span starting at this layer's MLP half: r is the caller's row-major h1, and
    // post_attention_layernorm runs as the span's first RMSNorm launch (slot zeroing and the
    // graph prologue included, like layer 0's input norm)
    const bool first = s->mlp_only(l);
    const u16* m_in = r;
    DecodeNorm dm = {DN_NONE, c.rms_eps, nullptr, nullptr};
    if (gemv && !first) {
      dm = {DN_EXACT, c.rms_eps, slot(2 * l), W.post_ln};
    } else {
      const long pe = s->prof_begin(PROF_NORM, st);
      launch_rmsnorm(r, h, nullptr, 0, W.post_ln, s->xn, h, M, h, c.rms_eps, st, false,
                     (first && gemv) ? s->ssq : nullptr, first ? 2 * c.n_layers : 0, first ? &pro : nullptr);
      s->prof_end(pe, st);
      m_in = s->xn;
    }
    long pe = s->prof_begin(PROF_GATEUP, st);
    // decode (the GEMV path): act goes between gate/up and down fragment-packed
    const int pk = (gemv && !gemm_uses_tiled(M, I, h, EPI_SILU) && !gemm_uses_tiled(M, h, I, EPI_RESID)) ? 1 : 0;
    GEMM_TRY(launch_gemm(m_in, h, W.gateup + (size_t)(c0 / 16) * (h / 32) * 512, M, I - c0, h,
                         actb + (size_t)(c0 / 32) * 512, I, nullptr, 0, EPI_SILU, nullptr, st, &s->gws, &dm, nullptr,
                         (pk ? GEMM_PACK_C : 0) | ((r_packed && m_in == r) ? GEMM_PACK_A : 0), c0 ? I / 16 : 0));
    s->prof_end(pe, st);
    pe = s->prof_begin(PROF_DOWN, st);
    GEMM_TRY(launch_gemm(actb, I, W.down, M, h, I, out, h, r, h, EPI_RESID, nullptr, st, &s->gws, nullptr,
                         (gemv && l + 1 < c.n_layers) ? slot(2 * l + 1) : nullptr,
                         (pk ? GEMM_PACK_A : 0) | (r_packed ? GEMM_PACK_R : 0) | (out_packed ? GEMM_PACK_C : 0)));
    s->prof_end(pe, st);
    return INFERD_OK;
  }

  // a gate/up boundary (decode): act columns [0, c1) go into x_out's record behind h1,
  // normed from the SSQ slot this layer's o GEMV just filled (the record's act is
  // fragment-packed with the whole projection's row length, as the receiver reads it)
  int gateup_prefix(int l, u16* h1, int c1) {
    const DecodeNorm dm = {DN_EXACT, c.rms_eps, slot(2 * l), s->layers[l].post_ln};
    const long pe = s->prof_begin(PROF_GATEUP, st);
    GEMM_TRY(launch_gemm(h1, h, s->layers[l].gateup, M, c1, h, h1 + (size_t)M * h, I, nullptr, 0, EPI_SILU, nullptr, st,
                         &s->gws, &dm, nullptr, GEMM_PACK_C, I / 16));
    s->prof_end(pe, st);
    return INFERD_OK;
  }

  // the layer's output (packed iff `packed`) becomes the next layer's input
  int end_layer(int l, const u16* out, bool packed) {
    x = out;
    x_packed = packed;
    if (layer_out)
      HIP_TRY(hipMemcpyAsync((u16*)layer_out + (size_t)l * M * h, x, (size_t)M * h * 2, hipMemcpyDeviceToDevice, st));
    LAUNCH_CHECK();
    return INFERD_OK;
  }

  int head(int32_t* next_ids, void* logits) {
    if (c.has_lm_head && (next_ids || logits)) {
      // last row of each sequence: seq_start[b+1] - 1
      const long pe = s->prof_begin(PROF_LMHEAD, st);
      // the final norm writes the last rows fragment-packed for the lm_head GEMV (its A operand
      // only; the logits it may also store stay row-major).  Folding this norm into the GEMV's A
      // path (DN_EXACT, as q/k/v) measured 213.8 us in the graph against 195 + 5 us (round 3).
      const bool pk_last = h % 32 == 0;
      launch_rmsnorm(x, h, b->seq_start + 1, 1, s->final_norm, s->last, h, B, h, c.rms_eps, st, pk_last);
      // a sampled head reads the logits of the tiles its keys select: they go to the span's own
      // buffer when the caller wants none
      const bool draw = s->sampling_on && next_ids;
      u16* lg = (draw && !logits) ? s->sample_logits : (u16*)logits;
      GEMM_TRY(launch_gemm(s->last, h, s->lm_head, B, c.vocab, h, lg, c.vocab, nullptr, 0, EPI_ARGMAX,
                           s->argmax_partial, st, nullptr, nullptr, nullptr, pk_last ? GEMM_PACK_A : 0));
      if (draw)
        launch_sample(lg, B, c.vocab, s->argmax_partial, s->sampling.temperature, s->sampling.top_k,
                      s->sampling.top_p, s->sampling.seed, s->sampling.row_seeds, b->ctx_lens, next_ids, nullptr,
                      s->err, st);
      else if (next_ids)
        launch_argmax_reduce(s->argmax_partial, c.vocab / 16, B, next_ids, st);
      s->prof_end(pe, st);
    }
    if (normed_out) {
      // vocab-parallel head: the last row of each sequence, final-normed and fragment-packed (the
      // A operand of every stage's inferd_span_head_shard), handed over instead of running lm_head
      const long pe = s->prof_begin(PROF_NORM, st);
      launch_rmsnorm(x, h, b->seq_start + 1, 1, s->final_norm, (u16*)normed_out, h, B, h, c.rms_eps, st, true);
      s->prof_end(pe, st);
    }
    LAUNCH_CHECK();
    return INFERD_OK;
  }

  // adv: the graph scheduler step the call's first launch runs (step_body), or null
  int run(const int32_t* ids, int32_t* next_ids, void* logits, const NormPrologue* adv) {
    if (normed_out && B > 64) return fail(INFERD_ERR_ARG, "final_norm_out supports <= 64 sequences per call");
    if (gemv && c.gateup_split_first && !x_in)
      return fail(INFERD_ERR_ARG, "a span starting inside a gate/up projection needs x_in (the hand-off record)");
    if ((c.o_split_last || c.qkv_split_last) && !x_out)
      return fail(INFERD_ERR_ARG, "a span ending before an o projection or an attention needs x_out (the hand-off record)");
    if (s->sampling_on && next_ids && logits && (uintptr_t)logits % 16)
      return fail(INFERD_ERR_ARG, "a sampled head reads `logits` back: it must be 16-byte aligned");
    if (c.has_embed && !ids) return fail(INFERD_ERR_ARG, "first span needs token ids");
    if (!c.has_embed && !x_in) return fail(INFERD_ERR_ARG, "span needs x_in hidden states");
    if (gemv && c.n_layers > 0 && !s->has_mlp(c.n_layers - 1) && c.gateup_split_last && !x_out)
      return fail(INFERD_ERR_ARG, "a span ending inside a gate/up projection needs x_out (the hand-off record)");
    if (c.has_lm_head && (next_ids || logits) && B > 64)
      return fail(INFERD_ERR_ARG, "lm_head argmax supports <= 64 sequences per call");
    // ---- the arguments hold: from here on, launches
    if (adv) pro = *adv;
    x = c.has_embed ? s->h : (const u16*)x_in;
    if (c.has_embed && c.n_layers > 0) {
      pro.ids = ids;
      pro.table = s->embed;
      pro.vocab = c.vocab;
      pro.err = s->err;
      pro.x_out = s->h;
    } else if (c.has_embed) {
      launch_embed(ids, s->embed, M, h, c.vocab, s->h, s->err, st);
    }
    int rc = INFERD_OK;
    if (c.n_layers == 0 && x_out && (rc = copy_input_out())) return rc;
    if ((c.o_split_first || q_in) && c.n_layers > 0 && (gemv || pro.positions)) {
      // a span starting at an o projection (or, decoding, at an attention) has no first RMSNorm
      // launch to carry the graph's scheduler step and the SSQ slot zeroing: a small launch of
      // its own
      launch_step_prologue(gemv ? s->ssq : nullptr, 2 * c.n_layers, M, &pro, st);
      pro = NormPrologue{};
    }
    for (int l = 0; l < c.n_layers; ++l) {
      // the residual written by this layer's last half: x_out after the span's last layer, and
      // (row-major) the input of a last layer that ends before its o projection -- the first part
      // of the hand-off record
      u16* out = (l == c.n_layers - 1 && x_out) ? (u16*)x_out : s->h;
      bool out_packed = pkx && l < c.n_layers - 1;
      if ((c.o_split_last || c.qkv_split_last) && l == c.n_layers - 2) {
        out = (u16*)x_out;
        out_packed = false;
      }
      const bool q_recv = s->qkv_in_record(l, b->decode);
      bool roped = false;
      if (s->has_qkv(l) && !q_recv && (rc = qkv(l, &roped))) return rc;
      // a span ending before this layer's o projection: the attention writes the record's second
      // part, behind the layer's input residual (row-major; copied there when it is the span's input)
      if (s->has_attn(l) && (rc = attention(l, q_recv, roped, s->has_o(l) ? s->attn : out_rec()))) return rc;
      if (s->ends_in_record(l)) {  // the record: x (first part; the span's input copied there), q/k/v or attention
        if (c.n_layers == 1 && (rc = copy_input_out())) return rc;
        LAUNCH_CHECK();
        continue;
      }
      // the residual the MLP half adds to: h1, or x where the span starts at this MLP half
      const u16* r = x;
      bool r_packed = x_packed;
      u16* h1 = nullptr;
      if (s->has_o(l)) {
        // h1 is packed iff pkx.  An in-place epilogue needs one layout on both sides, so h1 goes
        // to s->xn (free after the q/k/v projection) where s->h holds a row-major x (the first
        // span's embedding output) or is to receive this layer's row-major output (the last layer
        // without x_out).
        h1 = (pkx && ((x == s->h && !x_packed) || (out == s->h && !out_packed))) ? s->xn : s->h;
        bool h1_packed = pkx;
        if (!s->has_mlp(l)) {
          // a span ending at this layer's attention half: h1 is the span's (row-major) output;
          // without x_out it goes to s->xn (free after the q/k/v projection), never in place over
          // a packed x
          h1 = x_out ? (u16*)x_out : s->xn;
          h1_packed = false;
        }
        // the attention output the o projection reads: this layer's, or (a span starting at an o
        // projection; x is the record's residual part) the record's second part
        if ((rc = o_proj(l, s->has_attn(l) ? s->attn : in_rec(), h1, h1_packed))) return rc;
        r = h1;
        r_packed = h1_packed;
      }
      if (s->has_mlp(l)) {
        // a gate/up boundary (decode): columns [0, c0) of act arrived in x_in's record behind h1;
        // this span completes the record's act in place
        const int c0 = (gemv && s->mlp_only(l)) ? c.gateup_split_first : 0;
        if ((rc = mlp(l, r, r_packed, c0, c0 ? in_rec() : s->act, out, out_packed))) return rc;
        rc = end_layer(l, out, out_packed);
      } else {
        const int c1 = gemv ? c.gateup_split_last : 0;
        if (c1 && (rc = gateup_prefix(l, h1, c1))) return rc;
        rc = end_layer(l, h1, false);
      }
      if (rc) return rc;
    }
    return head(next_ids, logits);
  }
};

int forward_impl(InferdSpan* s, const InferdBatch* b, const int32_t* ids, const void* x_in, void* x_out,
                 int32_t* next_ids, void* logits, void* layer_out, hipStream_t st, const NormPrologue* adv) {
  if (!s) return fail(INFERD_ERR_ARG, "null span");
  if (int rc = check_batch(s, b)) return rc;
  Forward f{s, b, x_in, s->cfg.final_norm_out ? nullptr : x_out, s->cfg.final_norm_out ? x_out : nullptr, layer_out, st};
  return f.run(ids, next_ids, logits, adv);
}
}  // namespace

extern "C" int inferd_span_forward(InferdSpan* s, const InferdBatch* b, const int32_t* ids,
                                   const void* x_in, void* x_out, int32_t* next_ids, void* logits,
                                   void* layer_out, void* stream) {
  return forward_impl(s, b, ids, x_in, x_out, next_ids, logits, layer_out, (hipStream_t)stream, nullptr);
}

// Vocab-parallel lm_head shard: the greedy key of each row over this span's lm_head rows
// (InferdSpanConfig head_first / head_rows), column indices global.  The same GEMV and 16-column
// tiles as the whole head (inferd_span_forward's EPI_ARGMAX launch), so each logit is the one a
// single lm_head computes.
extern "C" int inferd_span_head_shard(InferdSpan* s, const void* normed, int32_t rows, const uint64_t* keys_in,
                                      uint64_t* keys_out, int32_t* ids, void* logits, void* stream) {
  if (!s || !normed || rows <= 0 || rows > 64) return fail(INFERD_ERR_ARG, "bad head_shard args (rows 1..64)");
  const InferdSpanConfig& c = s->cfg;
  const int n = s->lm_rows();
  if (n <= 0) return fail(INFERD_ERR_ARG, "span owns no lm_head rows");
  hipStream_t st = (hipStream_t)stream;
  const long pe = s->prof_begin(PROF_LMHEAD, st);
  GEMM_TRY(launch_gemm((const u16*)normed, c.hidden, s->lm_head, rows, n, c.hidden, (u16*)logits, n, nullptr, 0,
                       EPI_ARGMAX, s->argmax_partial, st, nullptr, nullptr, nullptr, GEMM_PACK_A));
  if (keys_out || ids)
    launch_argmax_keys(s->argmax_partial, n / 16, rows, s->lm_first(), (const unsigned long long*)keys_in,
                       (unsigned long long*)keys_out, ids, st);
  s->prof_end(pe, st);
  LAUNCH_CHECK();
  return INFERD_OK;
}

extern "C" int inferd_argmax_combine(const uint64_t* keys, int32_t n_parts, int32_t rows, int32_t* ids, void* stream) {
  if (!keys || !ids || n_parts <= 0 || rows <= 0) return fail(INFERD_ERR_ARG, "bad argmax_combine args");
  launch_argmax_combine((const unsigned long long*)keys, n_parts, rows, ids, (hipStream_t)stream);
  LAUNCH_CHECK();
  return INFERD_OK;
}

// ------------------------------------------------------------------ sampled decoding
// parameter ranges of InferdSampling, checked before any device call
static int check_sampling(const InferdSampling* p) {
  if (!(p->temperature > 0.f) || !(p->temperature <= 3.0e38f))
    return fail(INFERD_ERR_ARG, "sampling: temperature must be > 0 (and finite)");
  if (p->top_k < 1 || p->top_k > INFERD_SAMPLE_MAX_K)
    return fail(INFERD_ERR_ARG, "sampling: top_k must be 1 .. " + std::to_string(INFERD_SAMPLE_MAX_K));
  if (!(p->top_p > 0.f) || !(p->top_p <= 1.f)) return fail(INFERD_ERR_ARG, "sampling: top_p must be in (0, 1]");
  return INFERD_OK;
}

// the span's [64][lm_rows] logits buffer of sampled calls that pass no `logits`, on the span's own
// device (where its buffers live), whichever device the caller has current
static int ensure_sample_logits(InferdSpan* s) {
  if (s->sample_logits) return INFERD_OK;
  hipPointerAttribute_t at;
  int cur = 0;
  HIP_TRY(hipPointerGetAttributes(&at, s->err));
  HIP_TRY(hipGetDevice(&cur));
  if (at.device != cur) HIP_TRY(hipSetDevice(at.device));
  const int rc = s->alloc((void**)&s->sample_logits, (size_t)64 * s->lm_rows() * 2);
  if (at.device != cur) (void)hipSetDevice(cur);
  return rc;
}

extern "C" int inferd_span_set_sampling(InferdSpan* s, const InferdSampling* p) {
  if (p) {
    const int rc = check_sampling(p);
    if (rc) return rc;
  }
  if (!s) return fail(INFERD_ERR_ARG, "null span");
  if (!p) {
    s->sampling_on = false;
    return INFERD_OK;
  }
  if (!s->cfg.has_lm_head)
    return fail(INFERD_ERR_ARG, "sampling needs a span with the whole lm_head (has_lm_head; a vocab-parallel shard "
                                "samples per call: inferd_span_head_shard_sampled)");
  if (s->cfg.vocab > SAMPLE_MAX_VOCAB)
    return fail(INFERD_ERR_ARG, "sampling: vocab must be <= " + std::to_string(SAMPLE_MAX_VOCAB));
  if (const int rc = ensure_sample_logits(s)) return rc;
  s->sampling = *p;
  s->sampling_on = true;
  return INFERD_OK;
}

extern "C" int inferd_sample(const void* logits, int32_t rows, int32_t vocab, const InferdSampling* p,
                             const int32_t* positions, int32_t* ids, float* u_out, int32_t* flags, void* stream) {
  if (!p) return fail(INFERD_ERR_ARG, "sample: null parameters");
  const int rc = check_sampling(p);
  if (rc) return rc;
  if (!logits || !positions || !ids) return fail(INFERD_ERR_ARG, "sample: logits, positions and ids are required");
  if (rows < 1 || rows > 64 || vocab < 16 || vocab % 16 || vocab > SAMPLE_MAX_VOCAB)
    return fail(INFERD_ERR_ARG, "sample: rows 1 .. 64, vocab a multiple of 16 up to " + std::to_string(SAMPLE_MAX_VOCAB));
  if ((uintptr_t)logits % 16) return fail(INFERD_ERR_ARG, "sample: logits must be 16-byte aligned");
  launch_sample((const u16*)logits, rows, vocab, nullptr, p->temperature, p->top_k, p->top_p, p->seed, p->row_seeds,
                positions, ids, u_out, flags, (hipStream_t)stream);
  LAUNCH_CHECK();
  return INFERD_OK;
}

// ---- vocab-parallel sampled head: the candidate record chained over the shards (sampling.hip)
extern "C" int64_t inferd_sample_cand_bytes(int32_t rows) {
  if (rows < 1 || rows > 64) {
    g_err = "inferd_sample_cand_bytes: rows 1 .. 64";
    return -1;
  }
  return (int64_t)rows * SAMPLE_CAND_WORDS * 8;
}

// what both sampled shard calls require of their record / output pointers
static int check_shard_io(const char* who, const void* cand_in, const void* cand_out, const int32_t* positions,
                          const int32_t* ids) {
  if (!cand_out && !ids) return fail(INFERD_ERR_ARG, std::string(who) + ": cand_out or ids is required");
  if (ids && !positions) return fail(INFERD_ERR_ARG, std::string(who) + ": ids needs positions");
  if ((uintptr_t)cand_in % 8 || (uintptr_t)cand_out % 8)
    return fail(INFERD_ERR_ARG, std::string(who) + ": candidate records must be 8-byte aligned");
  return INFERD_OK;
}

extern "C" int inferd_sample_shard(const void* logits, int32_t rows, int32_t cols, int32_t first_col,
                                   const InferdSampling* p, const void* cand_in, void* cand_out,
                                   const int32_t* positions, int32_t* ids, float* u_out, int32_t* flags, void* stream) {
  if (!p) return fail(INFERD_ERR_ARG, "sample_shard: null parameters");
  if (const int rc = check_sampling(p)) return rc;
  if (rows < 1 || rows > 64) return fail(INFERD_ERR_ARG, "sample_shard: rows 1 .. 64");
  if (cols < 0 || cols % 16 || cols > SAMPLE_MAX_VOCAB)
    return fail(INFERD_ERR_ARG, "sample_shard: cols a multiple of 16 up to " + std::to_string(SAMPLE_MAX_VOCAB) +
                                    " (0: the record alone)");
  if (first_col < 0 || first_col % 16 || (int64_t)first_col + cols > INT32_MAX)
    return fail(INFERD_ERR_ARG, "sample_shard: first_col a multiple of 16, >= 0");
  if (cols > 0 && !logits) return fail(INFERD_ERR_ARG, "sample_shard: logits are required with cols > 0");
  if (cols > 0 && (uintptr_t)logits % 16) return fail(INFERD_ERR_ARG, "sample_shard: logits must be 16-byte aligned");
  if (const int rc = check_shard_io("sample_shard", cand_in, cand_out, positions, ids)) return rc;
  launch_sample_shard(cols ? (const u16*)logits : nullptr, rows, cols, first_col, nullptr, p->temperature, p->top_k,
                      p->top_p, p->seed, p->row_seeds, positions, (const unsigned long long*)cand_in,
                      (unsigned long long*)cand_out, ids, u_out, flags, (hipStream_t)stream);
  LAUNCH_CHECK();
  return INFERD_OK;
}

// The span's lm_head shard folded into the running candidate record: the same GEMV and tiles as
// inferd_span_head_shard (each logit is the one a single lm_head computes), its EPI_ARGMAX tile
// keys selecting the tiles the shard kernel reads back.  A span owning no rows runs the record
// alone (a finishing call on the stage behind the last shard).
extern "C" int inferd_span_head_shard_sampled(InferdSpan* s, const void* normed, int32_t rows, const InferdSampling* p,
                                              const void* cand_in, void* cand_out, const int32_t* positions,
                                              int32_t* ids, float* u_out, void* logits, void* stream) {
  if (!p) return fail(INFERD_ERR_ARG, "head_shard_sampled: null parameters");
  if (const int rc = check_sampling(p)) return rc;
  if (!s || rows <= 0 || rows > 64) return fail(INFERD_ERR_ARG, "bad head_shard_sampled args (rows 1..64)");
  if (const int rc = check_shard_io("head_shard_sampled", cand_in, cand_out, positions, ids)) return rc;
  const InferdSpanConfig& c = s->cfg;
  const int n = s->lm_rows();
  if (n > 0 && !normed) return fail(INFERD_ERR_ARG, "head_shard_sampled: normed rows are required");
  if (n > SAMPLE_MAX_VOCAB) return fail(INFERD_ERR_ARG, "sampling: vocab must be <= " + std::to_string(SAMPLE_MAX_VOCAB));
  if (logits && (n == 0 || (uintptr_t)logits % 16))
    return fail(INFERD_ERR_ARG, "head_shard_sampled: `logits` needs a span with lm_head rows and 16-byte alignment");
  hipStream_t st = (hipStream_t)stream;
  u16* lg = (u16*)logits;
  if (n > 0 && !lg) {
    if (const int rc = ensure_sample_logits(s)) return rc;  // has_lm_head spans only: shards own one from creation
    lg = s->sample_logits;
  }
  const long pe = s->prof_begin(PROF_LMHEAD, st);
  if (n > 0)
    GEMM_TRY(launch_gemm((const u16*)normed, c.hidden, s->lm_head, rows, n, c.hidden, lg, n, nullptr, 0, EPI_ARGMAX,
                         s->argmax_partial, st, nullptr, nullptr, nullptr, GEMM_PACK_A));
  launch_sample_shard(lg, rows, n, s->lm_first(), n > 0 ? s->argmax_partial : nullptr, p->temperature, p->top_k,
                      p->top_p, p->seed, p->row_seeds, positions, (const unsigned long long*)cand_in,
                      (unsigned long long*)cand_out, ids, u_out, s->err, st);
  s->prof_end(pe, st);
  LAUNCH_CHECK();
  return INFERD_OK;
}

// Final norm + lm_head over every row of x (LastStage.forward's logits over all T positions,
// partitioned_models.py:95-96); inferd_span_forward computes them for the last rows only.
extern "C" int inferd_span_lm_head(InferdSpan* s, const void* x, int32_t rows, void* logits, void* stream) {
  if (!s || !x || !logits || rows <= 0) return fail(INFERD_ERR_ARG, "bad lm_head args");
  const InferdSpanConfig& c = s->cfg;
  if (!c.has_lm_head) return fail(INFERD_ERR_ARG, "span has no lm_head");
  if (rows > c.max_tokens) return fail(INFERD_ERR_ARG, "rows > max_tokens");
  hipStream_t st = (hipStream_t)stream;
  launch_rmsnorm((const u16*)x, c.hidden, nullptr, 0, s->final_norm, s->xn, c.hidden, rows, c.hidden, c.rms_eps, st);
  GEMM_TRY(launch_gemm(s->xn, c.hidden, s->lm_head, rows, c.vocab, c.hidden, (u16*)logits, c.vocab, nullptr, 0, EPI_NONE,
              nullptr, st, &s->gws));
  LAUNCH_CHECK();
  return INFERD_OK;
}

// ------------------------------------------------------------------ decode graphs
struct InferdGraph {
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  ~InferdGraph() {
    if (exec) (void)hipGraphExecDestroy(exec);
    if (graph) (void)hipGraphDestroy(graph);
  }
};

namespace {
// the scheduler step of a decode replay (advance) + the forward, on `st` (captured or eager)
int step_body(InferdSpan* s, const InferdBatch* b, int32_t advance, const int32_t* ids, const void* x_in, void* x_out,
              int32_t* next_ids, void* logits, hipStream_t st) {
  NormPrologue adv;
  const bool in_norm = advance && s->cfg.n_layers > 0;
  if (in_norm) {  // run by the forward's first launch (layer 0's input norm: NormPrologue)
    adv.positions = (int32_t*)b->positions;
    adv.slots = (int32_t*)b->slots;
    adv.ctx_lens = (int32_t*)b->ctx_lens;
    adv.block_table = b->block_table;
    adv.max_pages = b->max_pages;
    adv.B = b->n_seqs;
    adv.err = s->err;
  } else if (advance) {
    launch_decode_advance((int32_t*)b->positions, (int32_t*)b->slots, (int32_t*)b->ctx_lens, b->block_table,
                          b->max_pages, b->n_seqs, s->err, st);
  }
  return forward_impl(s, b, ids, x_in, x_out, next_ids, logits, nullptr, st, in_norm ? &adv : nullptr);
}
}  // namespace

extern "C" int inferd_span_step(InferdSpan* s, const InferdBatch* b, int32_t advance, const int32_t* ids,
                                const void* x_in, void* x_out, int32_t* next_ids, void* logits, void* stream) {
  if (!s || !b) return fail(INFERD_ERR_ARG, "null argument");
  if (advance && !b->decode) return fail(INFERD_ERR_ARG, "advance needs a decode batch");
  return step_body(s, b, advance, ids, x_in, x_out, next_ids, logits, (hipStream_t)stream);
}

extern "C" int inferd_span_graph_capture(InferdSpan* s, const InferdBatch* b, int32_t advance, const int32_t* ids,
                                         const void* x_in, void* x_out, int32_t* next_ids, void* logits,
                                         void* stream, InferdGraph** out) {
  if (!s || !b || !out) return fail(INFERD_ERR_ARG, "null argument");
  if (!stream) return fail(INFERD_ERR_ARG, "graph capture needs a non-null stream");
  if (advance && !b->decode) return fail(INFERD_ERR_ARG, "advance needs a decode batch");
  hipStream_t st = (hipStream_t)stream;
  s->prof_on = false;  // event pairs are timed eagerly only (HIP cannot time captured events)
  HIP_TRY(hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
  const int rc = step_body(s, b, advance, ids, x_in, x_out, next_ids, logits, st);
  hipGraph_t g = nullptr;
  hipError_t e = hipStreamEndCapture(st, &g);
  if (rc) {
    if (g) (void)hipGraphDestroy(g);
    return rc;
  }
  if (e != hipSuccess) return fail(INFERD_ERR_HIP, std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
  InferdGraph* G = new InferdGraph();
  G->graph = g;
  e = hipGraphInstantiate(&G->exec, g, nullptr, nullptr, 0);
  if (e != hipSuccess) {
    delete G;
    return fail(INFERD_ERR_HIP, std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
  }
  *out = G;
  return INFERD_OK;
}

extern "C" int inferd_graph_launch(InferdGraph* g, void* stream) {
  if (!g) return fail(INFERD_ERR_ARG, "null graph");
  HIP_TRY(hipGraphLaunch(g->exec, (hipStream_t)stream));
  return INFERD_OK;
}

extern "C" void inferd_graph_destroy(InferdGraph* g) { delete g; }

extern "C" int inferd_span_error_flags(InferdSpan* s, int32_t* flags) {
  if (!s || !flags) return fail(INFERD_ERR_ARG, "null argument");
  HIP_TRY(hipMemcpy(flags, s->err, 4, hipMemcpyDeviceToHost));  // synchronises the device
  if (*flags) HIP_TRY(hipMemset(s->err, 0, 4));
  return INFERD_OK;
}

extern "C" int inferd_span_profile_start(InferdSpan* s, int32_t max_pairs) {
  if (!s || max_pairs <= 0) return fail(INFERD_ERR_ARG, "bad profile args");
  while (s->prof_events.size() < (size_t)max_pairs * 2) {
    hipEvent_t e;
    HIP_TRY(hipEventCreate(&e));
    s->prof_events.push_back(e);
  }
  s->prof_class.assign(s->prof_events.size() / 2, -1);
  s->prof_used = 0;
  s->prof_on = true;
  return INFERD_OK;
}

extern "C" int inferd_span_profile_stop(InferdSpan* s, double* total_ms, int32_t* counts, int32_t n_classes) {
  if (!s) return fail(INFERD_ERR_ARG, "null span");
  s->prof_on = false;
  for (int c = 0; c < n_classes; ++c) {
    total_ms[c] = 0.0;
    counts[c] = 0;
  }
  for (size_t i = 0; i + 1 < s->prof_used; i += 2) {
    HIP_TRY(hipEventSynchronize(s->prof_events[i + 1]));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, s->prof_events[i], s->prof_events[i + 1]));
    const int c = s->prof_class[i / 2];
    if (c >= 0 && c < n_classes) {
      total_ms[c] += ms;
      counts[c] += 1;
    }
  }
  s->prof_used = 0;
  return INFERD_OK;
}

extern "C" int inferd_span_kv_layer(InferdSpan* s, int32_t layer, void** out) {
  if (!s || !out) return fail(INFERD_ERR_ARG, "null argument");
  if (layer < 0 || layer >= s->cfg.n_layers) return fail(INFERD_ERR_ARG, "layer out of range");
  if (!s->has_attn(layer)) return fail(INFERD_ERR_ARG, "layer runs only its MLP half here (no KV)");
  *out = s->kv_of(layer);
  return INFERD_OK;
}

extern "C" int inferd_span_kv_clear(InferdSpan* s, void* stream) {
  if (!s) return fail(INFERD_ERR_ARG, "null span");
  if (s->kv_pool)
    HIP_TRY(hipMemsetAsync(s->kv_pool, 0, s->kv_layer_elems * s->kv_layers() * 2, (hipStream_t)stream));
  return INFERD_OK;
}

// ------------------------------------------------------------------ single ops
extern "C" int inferd_weightgen(void* dst, int64_t n, uint64_t seed, uint32_t tensor_id, float scale,
                                float center, void* stream) {
  if (!dst || n < 0) return fail(INFERD_ERR_ARG, "bad weightgen args");
  launch_weightgen((u16*)dst, n, tensor_key(seed, tensor_id), scale, center, (hipStream_t)stream);
  LAUNCH_CHECK();
  return INFERD_OK;
}

extern "C" int inferd_pack_weight(const void* src, int64_t rows, int64_t cols, void* dst, void* stream) {
  if (!src || !dst || rows % 16 || cols % 32) return fail(INFERD_ERR_ARG, "pack needs rows%16==0, cols%32==0");
  launch_pack((const u16*)src, cols, (int)rows, (int)cols, (u16*)dst, (hipStream_t)stream);
  LAUNCH_CHECK();
  return INFERD_OK;
}

extern "C" int inferd_unpack_weight(const void* src, int64_t rows, int64_t cols, void* dst, void* stream) {
  if (!src || !dst || rows % 16 || cols % 32) return fail(INFERD_ERR_ARG, "unpack needs rows%16==0, cols%32==0");
  launch_unpack((const u16*)src, (int)rows, (int)cols, (u16*)dst, (hipStream_t)stream);
  LAUNCH_CHECK();
  return INFERD_OK;
}

extern "C" int inferd_rmsnorm(const void* x, const void* w, void* y, int32_t rows, int32_t cols, float eps,
                              void* stream) {
  if (!x || !w || !y || rows <= 0 || cols % 8 || cols > 16384) return fail(INFERD_ERR_ARG, "bad rmsnorm args");
  launch_rmsnorm((const u16*)x, cols, nullptr, 0, (const u16*)w, (u16*)y, cols, rows, cols, eps,
                 (hipStream_t)stream);
  LAUNCH_CHECK();
  return INFERD_OK;
}

extern "C" int inferd_gemm(const void* a, const void* w, void* c, const void* r, int32_t m, int32_t n,
                           int32_t k, int32_t epi, void* stream) {
  if (!a || !w || !c || m <= 0 || n % 16 || k % 32) return fail(INFERD_ERR_ARG, "gemm needs n%16==0, k%32==0");
  if (epi < 0 || epi > 2) return fail(INFERD_ERR_ARG, "bad epilogue");
  if (epi == INFERD_EPI_RESID && !r) return fail(INFERD_ERR_ARG, "resid epilogue needs R");
  // the op API's own tail-split workspace: one per host thread, allocated on its first use and
  // freed when the thread exits (spans keep theirs)
  struct OpWs {
    GemmWs w;
    ~OpWs() { gemm_ws_free(&w); }
  };
  static thread_local OpWs op_ws;
  if (!op_ws.w.ws) {
    op_ws.w.split = 1;
    if (gemm_ws_alloc(&op_ws.w) != (int)hipSuccess) return fail(INFERD_ERR_HIP, "tail-split workspace allocation failed");
  }
  GEMM_TRY(launch_gemm((const u16*)a, k, (const u16*)w, m, n, k, (u16*)c, n, (const u16*)r, n, epi, nullptr,
              (hipStream_t)stream, &op_ws.w));
  LAUNCH_CHECK();
  return INFERD_OK;
}

extern "C" int inferd_rope_table(float theta, int32_t head_dim, int32_t max_pos, void* cos_t, void* sin_t,
                                 void* stream) {
  if (head_dim != HEAD_DIM || max_pos <= 0 || !cos_t || !sin_t) return fail(INFERD_ERR_ARG, "bad rope args");
  float inv[64];
  for (int i = 0; i < 64; ++i) inv[i] = 1.0f / powf(theta, (float)(2 * i) / (float)HEAD_DIM);
  float* dinv = nullptr;
  HIP_TRY(hipMalloc((void**)&dinv, sizeof(inv)));
  HIP_TRY(hipMemcpy(dinv, inv, sizeof(inv), hipMemcpyHostToDevice));
  launch_rope_table(dinv, max_pos, (u16*)cos_t, (u16*)sin_t, (hipStream_t)stream);
  hipError_t e = hipStreamSynchronize((hipStream_t)stream);
  (void)hipFree(dinv);
  if (e != hipSuccess) return fail(INFERD_ERR_HIP, hipGetErrorString(e));
  return INFERD_OK;
}

extern "C" int inferd_qk_norm_rope_kv(const void* qkv, const int32_t* positions, const int32_t* slots,
                                      const void* qn, const void* kn, const void* cos_t, const void* sin_t,
                                      void* q_out, void* kv_layer, int32_t m, int32_t H, int32_t KV, float eps,
                                      void* stream) {
  if (!qkv || !positions || !qn || !kn || !cos_t || !sin_t || !q_out || m <= 0 || KV <= 0 || H % KV)
    return fail(INFERD_ERR_ARG, "bad qk_norm_rope_kv args");
  if (slots && !kv_layer) return fail(INFERD_ERR_ARG, "slots given without a kv pool");
  const int ld = (H + 2 * KV) * HEAD_DIM;
  launch_qk_norm_rope_kv((const u16*)qkv, ld, positions, slots, (const u16*)qn, (const u16*)kn,
                         (const u16*)cos_t, (const u16*)sin_t, (u16*)q_out, (u16*)kv_layer, m, H, KV, eps,
                         (hipStream_t)stream);
  LAUNCH_CHECK();
  return INFERD_OK;
}

extern "C" int64_t inferd_attention_workspace_bytes(int32_t n_seqs, int32_t heads, int32_t max_ctx) {
  return (int64_t)attn_decode_ws_bytes(n_seqs, heads, max_ctx);
}

extern "C" int inferd_attention(const void* q, const void* kv_layer, const InferdBatch* b, int32_t H,
                                int32_t KV, void* out, void* ws, int64_t ws_bytes, void* stream) {
  if (!q || !kv_layer || !b || !out || KV <= 0 || H % KV || H / KV > 16) return fail(INFERD_ERR_ARG, "bad attention args");
  const AttnBatch ab = to_attn(b);
  const float scale = 1.0f / sqrtf((float)HEAD_DIM);
  if (b->decode) {
    if (!ws || ws_bytes < (int64_t)attn_decode_ws_bytes(b->n_seqs, H, b->max_ctx_len))
      return fail(INFERD_ERR_ARG, "decode attention workspace too small");
    launch_attn_decode((const u16*)q, (const u16*)kv_layer, ab, H, KV, scale, (u16*)out, (float*)ws,
                       (hipStream_t)stream);
  } else {
    launch_attn_prefill((const u16*)q, (const u16*)kv_layer, ab, H, KV, scale, (u16*)out, (hipStream_t)stream);
  }
  LAUNCH_CHECK();
  return INFERD_OK;
}

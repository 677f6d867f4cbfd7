// stages.h — what the stage-orchestration units (vision.hip, opt.hip, t5.hip, blocks.hip) share.  They are the C ABI of include/eilev.h on
// top of the gfx950 kernels: which kernel runs on which buffer; no arithmetic lives in them.  Every launch goes to the caller's stream,
// nothing allocates or synchronises (except eilev_prof_collect), so a whole stage can be captured into a hipGraph by the caller.
#pragma once
#include "common.h"

#define RC(expr)                 \
    do {                         \
        int _rc = (expr);        \
        if (_rc != 0) return _rc; \
    } while (0)

// Buffers taken one after the other from a workspace, each aligned to 256 bytes.  base == nullptr: a dry run that only adds up — a stage's
// *_workspace_bytes function runs the same carve as its forward function, so a buffer is named once.
struct Carver {
    char *base;
    size_t used = 0;
    template <typename T>
    T *take(size_t n) {
        T *q = base ? reinterpret_cast<T *>(base + used) : nullptr;
        used += align_up(n * sizeof(T), 256);
        return q;
    }
};

static inline GemmArgs mk_gemm(const bf16 *A, int64_t lda, const void *W, int64_t ldw, const void *bias, const bf16 *resid, int64_t ldr,
                               void *C, int64_t ldc, int64_t M, int N, int K, int epi) {
    GemmArgs g;
    g.A = A; g.lda = lda; g.W = (const bf16 *)W; g.ldw = ldw; g.bias = (const bf16 *)bias; g.resid = resid; g.ldr = ldr;
    g.C = C; g.ldc = ldc; g.M = (int)M; g.N = N; g.K = K; g.epi = epi; g.out_f32 = 0; g.scale = 1.0f; g.scale_cols = 0;
    g.patch_group = 0; g.scratch = nullptr; g.scratch_bytes = 0; g.dbg = 0;
    return g;
}

// The skinny scratch of the language models' workspaces, in halves: split-K partials of the decode GEMVs | flash-decoding partials (batch 32
// x 40 heads x 9 key splits x (128 + 2) floats = 6 MB)
constexpr size_t kSkinnyScratch = 16u << 20, kSkinnyHalf = kSkinnyScratch / 2;
// mk_gemm with the split-K half of `scratch` attached
static inline GemmArgs sk_gemm(float *scratch, const bf16 *A, int64_t lda, const void *W, int64_t ldw, const void *bias, const bf16 *resid,
                               int64_t ldr, void *C, int64_t ldc, int64_t M, int N, int K, int epi) {
    GemmArgs g = mk_gemm(A, lda, W, ldw, bias, resid, ldr, C, ldc, M, N, K, epi);
    g.scratch = scratch;
    g.scratch_bytes = kSkinnyHalf;
    return g;
}
// a decode attention of the q rows in `qkv` into `out`, its flash-decoding partials in the second half of `scratch`
static inline DecodeAttnArgs decode_attn_args(const bf16 *qkv, bf16 *out, float *scratch, int64_t batch, int heads, int hd) {
    DecodeAttnArgs a;
    a.qkv = qkv; a.out = out; a.batch = (int)batch; a.heads = heads; a.hd = hd;
    a.part = scratch + kSkinnyHalf / sizeof(float); a.part_bytes = kSkinnyHalf;
    return a;
}

// A KV cache of bf16 elements, [layers][k | v][batch][heads][cap][hd]; `width` = heads * hd
struct KvCache {
    size_t plane;  // the keys (or the values) of one layer
    KvCache(int64_t batch, int64_t width, int64_t cap) : plane((size_t)batch * cap * width) {}
    size_t per_layer() const { return 2 * plane; }
    size_t bytes(int layers) const { return (size_t)layers * per_layer() * sizeof(bf16); }
    template <typename T>
    T *k(T *cache, int l) const { return cache + l * per_layer(); }
    template <typename T>
    T *v(T *cache, int l) const { return cache + l * per_layer() + plane; }
};

// the n bf16 arrays p[0], p[1], ... of `each` elements sit back to back in memory (the engine packs q | k | v and k | v so): one GEMM can take
// them as one matrix, or one bias vector
static inline bool packed(const void *const *p, int n, size_t each) {
    for (int i = 1; i < n; ++i)
        if ((const bf16 *)p[i] != (const bf16 *)p[0] + i * each) return false;
    return true;
}

// one snapshot of the residual stream (`bytes` bytes) into slot i of a hidden-states output
static inline int copy_hidden(void *hidden_states, int64_t i, const void *x, size_t bytes, hipStream_t s) {
    EILEV_HIP_CHECK(hipMemcpyAsync((char *)hidden_states + i * bytes, x, bytes, hipMemcpyDeviceToDevice, s));
    return EILEV_OK;
}

static inline bool dims_ok_vit(const EilevDims *d) {
    return d->v_hidden % 8 == 0 && d->v_inter % 8 == 0 && d->v_heads > 0 && d->v_hidden % d->v_heads == 0 &&
           (d->v_hidden / d->v_heads) % 8 == 0 && d->v_hidden / d->v_heads <= 128 && d->v_hidden <= 4096 &&
           d->image_size % d->patch_size == 0;
}
static inline bool dims_ok_qf(const EilevDims *d) {
    return d->q_hidden % 8 == 0 && d->q_inter % 8 == 0 && d->q_heads > 0 && d->q_hidden % d->q_heads == 0 &&
           (d->q_hidden / d->q_heads) % 8 == 0 && d->q_hidden / d->q_heads <= 128 && d->q_hidden <= 4096 && d->q_cross_freq > 0;
}
static inline bool dims_ok_opt(const EilevDims *d) {
    return d->t_hidden % 8 == 0 && d->t_ffn % 8 == 0 && d->t_heads > 0 && d->t_hidden % d->t_heads == 0 &&
           (d->t_hidden / d->t_heads) % 8 == 0 && d->t_hidden / d->t_heads <= 128 && d->t_hidden <= 4096;
}
static inline bool dims_ok_t5(const EilevT5Dims *d) {
    return d->d_model % 8 == 0 && d->d_kv % 8 == 0 && d->d_kv <= 128 && d->heads > 0 && d->d_ff % 8 == 0 && d->d_model <= 4096 &&
           d->rel_buckets >= 4 && d->rel_max_dist > d->rel_buckets / 4;
}

// t5.hip: the beam form of the flan-t5 decode step (include/eilev_t5beam.h holds the layout; t5beam.hip is its C ABI).  Row r is beam
// r % beams of sample r / beams; the decoder start token's K / V sit in kv_start (one row per sample, capacity 1: eilev_t5_decode fills
// it), generated token g of a hypothesis in slot g of kv_gen (one row per beam slot, capacity gen_capacity), in row ancestors[g][r].
struct T5BeamArgs {
    int64_t beams;
    const void *kv_start;
    void *kv_gen;
    int64_t gen_capacity;
    const int32_t *ancestors;
};
// One step on `rows` rows: state[0] = generated tokens fed including this one (the decoder position of the query); incremented at the end.
int t5_decode_step_beam(const EilevT5Dims *d, const EilevT5Weights *w, const int64_t *tokens, int32_t *state, const int32_t *enc_mask,
                        int64_t rows, const T5BeamArgs &beam, const void *cross_kv, int64_t enc_len, float *logits, void *workspace,
                        size_t workspace_bytes, void *stream);
size_t t5_decode_step_beam_workspace_bytes(const EilevT5Dims *d, int64_t rows, int64_t enc_len, int64_t gen_capacity);

// opt.hip: the parts of an OPT block around its attention, shared with prefix.hip (include/eilev_prefix.h: the same block over a shared prefix)
struct OptBufs {
    bf16 *h, *x, *att, *qkv, *ffn;
    int32_t *pid;
    float *scratch;
    uint8_t *a8;      // fp8 (e4m3) copy of the current linear's input rows (EilevOptWeights.w8_act_fp8)
    float *a8_scale;  // one scale per row
    size_t used;      // the bytes they take
};
// the buffers of M activation rows from `ws` (null: none)
OptBufs carve_opt(const EilevDims *d, int64_t M, void *ws);
// q|k|v projection of b.x into b.qkv (q pre-scaled by head_dim^-0.5)
int opt_qkv(const EilevDims *d, const EilevOptWeights *w, int l, const OptBufs &b, int64_t M, hipStream_t s, int a_frag = 0);
// out_proj + residual, LN, fc1 + ReLU, fc2 + residual of block l: b.att, b.h -> b.h
int opt_tail(const EilevDims *d, const EilevOptWeights *w, int l, const OptBufs &b, int64_t M, hipStream_t s, const void *next_ln_w = nullptr,
             const void *next_ln_b = nullptr, int frag = 0, bool dry = false);

// opt.hip: the body of eilev_opt_decode_step_beam (include/eilev.h: same arguments, same contract).  shared_prompt: the attention reads a
// sample's prompt keys once for its rows (common.h DecodeAttnArgs.shared_prompt; head sizes 80 / 128, else EILEV_E_UNSUPPORTED) and the
// workspace holds opt_decode_step_beam_shared_bytes (0 for arguments the step refuses): include/eilev_prefix.h eilev_prefix_decode_step
int opt_decode_step_beam(const EilevDims *d, const EilevOptWeights *w, const int64_t *tokens, int32_t *state, const int32_t *attn_mask,
                         const int32_t *n_valid, int64_t rows, int64_t beams, int64_t seq_len, const void *kv_prompt, void *kv_gen, int64_t gen_capacity,
                         const int32_t *ancestors, float *logits, void *workspace, size_t workspace_bytes, void *stream, int shared_prompt);
size_t opt_decode_step_beam_shared_bytes(const EilevDims *d, int64_t rows, int64_t seq_len, int64_t gen_capacity);

// probe / test switches read outside the unit that defines them (set by eilev_debug_* of the probe build)
extern int g_decode_rows;  // opt.hip; eilev_linear_rows (blocks.hip) follows it

// opt.hip — the OPT language model (include/eilev.h): prefill, extend, the greedy and the beam decode step, and the selection wrappers the
// decode loop uses.
#include "stages.h"

// =====================================================================================================
// Stage 4/5: OPT
// =====================================================================================================
// rows of the activation buffers: a decode step of 17..32 rows keeps its activations in the 32-row row-block layout (common.h frag32_index)
namespace {
inline int64_t opt_ws_rows(int64_t M) { return (M > 16 && M < 32) ? 32 : M; }

}  // namespace

// the buffers of M activation rows from `ws` (null: none)
OptBufs carve_opt(const EilevDims *d, int64_t M, void *ws) {
    Carver cv{(char *)ws};
    OptBufs b;
    M = opt_ws_rows(M);
    b.h = cv.take<bf16>((size_t)M * d->t_hidden);
    b.x = cv.take<bf16>((size_t)M * d->t_hidden);
    b.att = cv.take<bf16>((size_t)M * d->t_hidden);
    b.qkv = cv.take<bf16>((size_t)M * 3 * d->t_hidden);
    b.ffn = cv.take<bf16>((size_t)M * d->t_ffn);
    b.pid = cv.take<int32_t>((size_t)M);
    b.scratch = cv.take<float>(kSkinnyScratch / sizeof(float));
    b.a8 = cv.take<uint8_t>((size_t)M * (d->t_ffn > d->t_hidden ? d->t_ffn : d->t_hidden));
    b.a8_scale = cv.take<float>((size_t)M);
    b.used = cv.used;
    return b;
}

extern "C" size_t eilev_opt_workspace_bytes(const EilevDims *d, int64_t batch, int64_t seq_len) {
    return carve_opt(d, batch * (seq_len > 1 ? seq_len : 1), nullptr).used + 256;
}

extern "C" size_t eilev_opt_kv_cache_bytes(const EilevDims *d, int64_t batch, int64_t kv_capacity) {
    return KvCache(batch, d->t_hidden, kv_capacity).bytes(d->t_layers);
}

namespace {
// fp8 form of a linear (EilevOptLayerW8): bytes + per-channel scales; large-M calls expand into w->w8_expand
int use_w8(GemmArgs &g, const EilevOptWeights *w, const uint8_t *w8, const float *sc, const OptBufs &b, hipStream_t s) {
    if (!w8 || !sc) return EILEV_E_BADARG;
    if (w->w8_act_fp8 && g.M > 32 && g.K % 128 == 0 && (int64_t)g.M * g.K < 0x7fff0000ll && (int64_t)g.N * g.K < 0x7fff0000ll) {
        // configs[4] "fp8 MFMA": quantise this linear's input rows per token and run the product on the fp8 MFMA
        RC(launch_quant_rows_e4m3(g.A, g.lda, b.a8, b.a8_scale, g.M, g.K, s));
        g.A8 = b.a8;
        g.ascale = b.a8_scale;
        g.lda = g.K;
        g.W8 = w8;
        g.wscale = sc;
        g.ldw = g.K;
        return EILEV_OK;
    }
    if (g.M > 32 || g.K % 256 != 0) {
        if (!w->w8_expand || w->w8_expand_bytes < (size_t)g.N * g.K * sizeof(bf16)) return EILEV_E_WORKSPACE;
        g.w8_scratch = (bf16 *)w->w8_expand;
    }
    g.W8 = w8;
    g.wscale = sc;
    g.ldw = g.K;
    return EILEV_OK;
}

}  // namespace

// q|k|v projection of x into b.qkv (q pre-scaled by head_dim^-0.5, hf modeling_opt.py:151)
int opt_qkv(const EilevDims *d, const EilevOptWeights *w, int l, const OptBufs &b, int64_t M, hipStream_t s, int a_frag) {
    const EilevOptLayer *L = &w->layers[l];
    const int D = d->t_hidden;
    const float scaling = 1.0f / sqrtf((float)(D / d->t_heads));
    const void *ws[3] = {L->q_w, L->k_w, L->v_w}, *bs[3] = {L->q_b, L->k_b, L->v_b};
    const bool bias_fused = packed(bs, 3, D);
    if (w->layers_w8) {
        if (!bias_fused && (L->q_b || L->k_b || L->v_b)) return EILEV_E_UNSUPPORTED;  // fp8 q|k|v is one matrix: one bias vector
        GemmArgs g = sk_gemm(b.scratch, b.x, D, nullptr, D, L->q_b, nullptr, 0, b.qkv, 3 * D, M, 3 * D, D, 0);
        g.scale = scaling; g.scale_cols = D;
        RC(use_w8(g, w, w->layers_w8[l].qkv_w8, w->layers_w8[l].qkv_scale, b, s));
        return launch_gemm(g, 5, s);
    }
    const bool fused = packed(ws, 3, (size_t)D * D) && bias_fused;
    for (int i = 0; i < (fused ? 1 : 3); ++i) {  // one [3 D, D] matrix, or q, k, v one by one
        GemmArgs g = sk_gemm(b.scratch, b.x, D, ws[i], D, bs[i], nullptr, 0, b.qkv + i * D, 3 * D, M, fused ? 3 * D : D, D, 0);
        if (i == 0) { g.scale = scaling; g.scale_cols = D; }
        if (fused && w->layers_stream && M > 16 && M <= 32) g.Wp = (const bf16 *)w->layers_stream[l].qkv_s;
        g.a_frag = a_frag;
        RC(launch_gemm(g, 5, s));
    }
    return EILEV_OK;
}

// out_proj + residual, LN, fc1 + ReLU, fc2 + residual (hf modeling_opt.py:178-179, 226-247)
// next_ln_w / next_ln_b (decode): the LayerNorm that consumes this block's output (the next block's self_attn_layer_norm, or
// final_layer_norm) — then b.x leaves as that LayerNorm of b.h, and both LayerNorms of the block ride on the split-K reductions of
// out_proj / fc2 (GemmArgs::ln_out)
// frag (decode steps of 17..32 rows, eilev_opt_decode_step): b.att, b.x and b.ffn in the row-block layout (common.h frag32_index); b.h stays row-major
int opt_tail(const EilevDims *d, const EilevOptWeights *w, int l, const OptBufs &b, int64_t M, hipStream_t s, const void *next_ln_w,
             const void *next_ln_b, int frag, bool dry) {
    const EilevOptLayer *L = &w->layers[l];
    const EilevOptLayerW8 *Q = w->layers_w8 ? &w->layers_w8[l] : nullptr;
    const int D = d->t_hidden, Ft = d->t_ffn;
    // (decode steps of 17..32 rows: the stream-layout copies of the three matrices, where the caller packed them)
    const EilevOptLayerStream *S = (w->layers_stream && !Q && M > 16 && M <= 32) ? &w->layers_stream[l] : nullptr;
    GemmArgs g = sk_gemm(b.scratch, b.att, D, L->o_w, D, L->o_b, b.h, D, b.h, D, M, D, D, 0);
    g.ln_gamma = (const bf16 *)L->ln2_w; g.ln_beta = (const bf16 *)L->ln2_b; g.ln_out = b.x; g.ln_eps = d->t_eps;
    if (S) g.Wp = (const bf16 *)S->o_s;
    g.a_frag = g.ln_frag = frag;
    if (dry && !gemm_rows32_takes(g)) return EILEV_E_UNSUPPORTED;
    if (Q) RC(use_w8(g, w, Q->o_w8, Q->o_scale, b, s));
    if (!dry) RC(launch_gemm(g, 5, s));
    g = sk_gemm(b.scratch, b.x, D, L->fc1_w, D, L->fc1_b, nullptr, 0, b.ffn, Ft, M, Ft, D, 2);
    if (S) g.Wp = (const bf16 *)S->fc1_s;
    g.a_frag = g.c_frag = frag;
    if (dry && !gemm_rows32_takes(g)) return EILEV_E_UNSUPPORTED;
    if (Q) RC(use_w8(g, w, Q->fc1_w8, Q->fc1_scale, b, s));
    if (!dry) RC(launch_gemm(g, 5, s));
    g = sk_gemm(b.scratch, b.ffn, Ft, L->fc2_w, Ft, L->fc2_b, b.h, D, b.h, D, M, D, Ft, 0);
    if (S) g.Wp = (const bf16 *)S->fc2_s;
    if (next_ln_w) {
        g.ln_gamma = (const bf16 *)next_ln_w; g.ln_beta = (const bf16 *)next_ln_b; g.ln_out = b.x; g.ln_eps = d->t_eps;
    }
    g.a_frag = frag;
    g.ln_frag = next_ln_w ? frag : 0;
    if (dry) return gemm_rows32_takes(g) ? EILEV_OK : EILEV_E_UNSUPPORTED;
    if (Q) RC(use_w8(g, w, Q->fc2_w8, Q->fc2_scale, b, s));
    return launch_gemm(g, 5, s);
}

namespace {
// ---- small-batch decode (M <= 4 rows): the block as 5 launches of gemv.hip + the attention -------------------------------------------
int g_decode_frag = 1;  // probe / test switch (eilev_debug_decode_frag, probe build): 0 = row-major activations in the 17..32-row decode step
}  // namespace
int g_decode_rows = 1;  // probe / test switch (eilev_debug_decode_rows): 0 = the MFMA weight-streaming kernels at every batch size
#ifdef EILEV_PROBES
extern "C" int eilev_debug_decode_rows(int on) { g_decode_rows = on; return 0; }
extern "C" int eilev_debug_decode_frag(int on) { g_decode_frag = on; return 0; }
#endif
namespace {

// q | k | v of every block must be ONE [3 D, D] matrix with one bias vector (the engine packs them so)
bool opt_qkv_packed(const EilevDims *d, const EilevOptWeights *w) {
    const int D = d->t_hidden;
    for (int l = 0; l < d->t_layers; ++l) {
        const EilevOptLayer *L = &w->layers[l];
        const void *ws[3] = {L->q_w, L->k_w, L->v_w}, *bs[3] = {L->q_b, L->k_b, L->v_b};
        if (!packed(ws, 3, (size_t)D * D) || !L->q_b || !packed(bs, 3, D)) return false;
    }
    return true;
}
// Measured (tools/beam_probe.py, OPT-2.7B, L = 960, ms per token under hipGraph): rows 1: 2.27 against 2.64 for the MFMA weight-streaming
// kernels, 2: 2.67 (~2.7), 3: 2.89 (~2.8), 5: 4.07 against 2.87 — every extra row costs the dot-product kernel a pass of LDS reads and
// v_dot2c per weight chunk, the MFMA kernels nothing up to 16 rows.  So: M <= 2 (latency mode; one sample per GPU of a strong-scaled step).
bool opt_rows_usable(const EilevDims *d, const EilevOptWeights *w, int64_t M) {
    if (!g_decode_rows || w->layers_w8 || M > 2) return false;
    const int D = d->t_hidden;
    return gemv_rows_ok((int)M, D, D) && gemv_rows_ok((int)M, D, d->t_ffn) && (D / d->t_heads) % 8 == 0 && opt_qkv_packed(d, w);
}
// batch 1 (latency mode; one sample per GPU of a strong-scaled step): gemv1_kernel + attn_decode1_kernel.  eilev_debug_decode_rows(3) = off
bool opt_rows1_usable(const EilevDims *d, const EilevOptWeights *w, int64_t M, int64_t cap) {
    if (M != 1 || g_decode_rows == 3 || !opt_rows_usable(d, w, M)) return false;
    const int D = d->t_hidden;
    return gemv1_ok(3 * D, D, 1) && gemv1_ok(D, D, 0) && gemv1_ok(d->t_ffn, D, 1) && gemv1_ok(D, d->t_ffn, 0) && gemv1_ok(d->vocab, D, 1) &&
           attn_decode1_ok(1, (int)cap, D / d->t_heads);
}
// 2..4 rows (beam search, a few samples per GPU): gemvm_kernel for every K = t_hidden linear, the one-pass attention where it applies
bool opt_rowsm_usable(const EilevDims *d, const EilevOptWeights *w, int64_t M) {
    // measured (OPT-2.7B, L = 960, ms per token): 2 rows 2.06 (row-dot kernels of round 3: 2.67), 4 rows 2.51, 5 rows 3.20 against 2.87 for the MFMA
    // weight-streaming kernels, whose cost is flat up to 16 rows: every extra row costs this kernel a pass of LDS reads + dot products
    if (M < 2 || M > 4 || g_decode_rows == 3 || !g_decode_rows || w->layers_w8) return false;
    const int D = d->t_hidden;
    return gemvm_ok((int)M, 3 * D, D, 1) && gemvm_ok((int)M, D, D, 0) && (D / d->t_heads) % 8 == 0 && !(d->vocab & 1) && opt_qkv_packed(d, w);
}
// block l without its attention: LayerNorm + q|k|v (before), out_proj + residual, LayerNorm + fc1 + ReLU, fc2 + residual (after)
int opt_rowsm_qkv(const EilevDims *d, const EilevOptWeights *w, int l, const OptBufs &b, int64_t M, hipStream_t s) {
    const EilevOptLayer *L = &w->layers[l];
    const int D = d->t_hidden;
    return launch_gemvm(1, b.h, D, (const bf16 *)L->ln1_w, (const bf16 *)L->ln1_b, d->t_eps, (const bf16 *)L->q_w, (const bf16 *)L->q_b, nullptr, 0, b.qkv, 3 * D, 0, (int)M,
                        3 * D, D, 0, 1.0f / sqrtf((float)(D / d->t_heads)), D, s);
}
int opt_rowsm_tail(const EilevDims *d, const EilevOptWeights *w, int l, const OptBufs &b, int64_t M, hipStream_t s) {
    const EilevOptLayer *L = &w->layers[l];
    const int D = d->t_hidden, Ft = d->t_ffn;
    RC(launch_gemvm(0, b.att, D, nullptr, nullptr, 0.f, (const bf16 *)L->o_w, (const bf16 *)L->o_b, b.h, D, b.h, D, 0, (int)M, D, D, 0, 1.0f, 0, s));
    RC(launch_gemvm(1, b.h, D, (const bf16 *)L->ln2_w, (const bf16 *)L->ln2_b, d->t_eps, (const bf16 *)L->fc1_w, (const bf16 *)L->fc1_b, nullptr, 0, b.ffn, Ft, 0, (int)M, Ft, D,
                    2, 1.0f, 0, s));
    if (gemv_rows_ok((int)M, D, Ft))  // K = t_ffn: the LDS-staged row-dot kernel (gemvm_kernel spills at K = 10240)
        return launch_gemv_rows(0, b.ffn, Ft, nullptr, nullptr, 0.f, nullptr, 0, 0, 0, (const bf16 *)L->fc2_w, (const bf16 *)L->fc2_b, b.h, D, b.h, D, 0, (int)M, D, Ft, 0, 1.0f,
                                0, s);
    return launch_gemm(sk_gemm(b.scratch, b.ffn, Ft, L->fc2_w, Ft, L->fc2_b, b.h, D, b.h, D, M, D, Ft, 0), 5, s);
}
int opt_rowsm_head(const EilevDims *d, const EilevOptWeights *w, const OptBufs &b, int64_t M, float *logits, hipStream_t s) {
    const int D = d->t_hidden;
    return launch_gemvm(1, b.h, D, (const bf16 *)w->final_ln_w, (const bf16 *)w->final_ln_b, d->t_eps, (const bf16 *)w->embed_tokens, nullptr, nullptr, 0, logits, d->vocab, 1,
                        (int)M, d->vocab, D, 0, 1.0f, 0, s);
}
// self_attn_layer_norm + q|k|v of block l from b.h into b.qkv (q pre-scaled)
int opt_rows_qkv(const EilevDims *d, const EilevOptWeights *w, int l, const OptBufs &b, int64_t M, hipStream_t s) {
    const EilevOptLayer *L = &w->layers[l];
    const int D = d->t_hidden;
    return launch_gemv_rows(1, b.h, D, (const bf16 *)L->ln1_w, (const bf16 *)L->ln1_b, d->t_eps, nullptr, 0, 0, 0, (const bf16 *)L->q_w, (const bf16 *)L->q_b,
                            nullptr, 0, b.qkv, 3 * D, 0, (int)M, 3 * D, D, 0, 1.0f / sqrtf((float)(D / d->t_heads)), D, s);
}
// merge + out_proj + residual, final_layer_norm + fc1 + ReLU, fc2 + residual: b.h -> b.h.  The attention's flash-decoding partials (nsplit
// ranges per row and head) are merged in the prologue of out_proj (every workgroup repeats the merge: M <= 2).
int opt_rows_tail(const EilevDims *d, const EilevOptWeights *w, int l, const OptBufs &b, int64_t M, const float *part, int nsplit, hipStream_t s) {
    const EilevOptLayer *L = &w->layers[l];
    const int D = d->t_hidden, Ft = d->t_ffn, H = d->t_heads;
    RC(launch_gemv_rows(2, nullptr, 0, nullptr, nullptr, 0.f, part, H, D / H, nsplit, (const bf16 *)L->o_w, (const bf16 *)L->o_b, b.h, D, b.h, D, 0,
                        (int)M, D, D, 0, 1.0f, 0, s));
    RC(launch_gemv_rows(1, b.h, D, (const bf16 *)L->ln2_w, (const bf16 *)L->ln2_b, d->t_eps, nullptr, 0, 0, 0, (const bf16 *)L->fc1_w, (const bf16 *)L->fc1_b, nullptr,
                        0, b.ffn, Ft, 0, (int)M, Ft, D, 2, 1.0f, 0, s));
    return launch_gemv_rows(0, b.ffn, Ft, nullptr, nullptr, 0.f, nullptr, 0, 0, 0, (const bf16 *)L->fc2_w, (const bf16 *)L->fc2_b, b.h, D, b.h, D, 0, (int)M, D, Ft,
                            0, 1.0f, 0, s);
}
// final_layer_norm + lm_head -> fp32 logits
int opt_rows_head(const EilevDims *d, const EilevOptWeights *w, const OptBufs &b, int64_t M, float *logits, hipStream_t s) {
    const int D = d->t_hidden;
    return launch_gemv_rows(1, b.h, D, (const bf16 *)w->final_ln_w, (const bf16 *)w->final_ln_b, d->t_eps, nullptr, 0, 0, 0, (const bf16 *)w->embed_tokens, nullptr,
                            nullptr, 0, logits, d->vocab, 1, (int)M, d->vocab, D, 0, 1.0f, 0, s);
}
// final_layer_norm rows (b.x) -> fp32 logits on the MFMA kernels (17..32 rows: the stream-layout copy of lm_head, where the caller packed it)
GemmArgs opt_lm_head(const EilevDims *d, const EilevOptWeights *w, const OptBufs &b, int64_t M, float *logits) {
    const int D = d->t_hidden;
    GemmArgs g = sk_gemm(b.scratch, b.x, D, w->embed_tokens, D, nullptr, nullptr, 0, logits, d->vocab, M, d->vocab, D, 0);
    g.out_f32 = 1;
    if (w->lm_head_stream && M > 16 && M <= 32) g.Wp = (const bf16 *)w->lm_head_stream;
    return g;
}
// the attention of block l, `a` that of block 0: its caches hold one block every kv_layer elements (the generation cache: gen_layer)
DecodeAttnArgs at_block(DecodeAttnArgs a, int l, size_t kv_layer, size_t gen_layer) {
    a.kc += l * kv_layer; a.vc += l * kv_layer;
    if (a.kg) { a.kg += l * gen_layer; a.vg += l * gen_layer; }
    return a;
}
// The blocks and the LM head of an OPT decode step of M rows, b.h (the embedded tokens) -> fp32 logits, `a` the attention of block 0: 2..4
// rows on gemvm_kernel (one_pass: attn_decode1_kernel), <= 2 on the row-dot kernels (the attention's partials merged in out_proj's
// prologue), more on the MFMA kernels (frag: their activations in the row-block layout).  The step's tail is the caller's.
int opt_decode_blocks(const EilevDims *d, const EilevOptWeights *w, const OptBufs &b, int64_t M, const DecodeAttnArgs &a, size_t kv_layer,
                      size_t gen_layer, bool one_pass, int frag, float *logits, hipStream_t s) {
    if (opt_rowsm_usable(d, w, M)) {  // round 4
        for (int l = 0; l < d->t_layers; ++l) {
            const DecodeAttnArgs al = at_block(a, l, kv_layer, gen_layer);
            RC(opt_rowsm_qkv(d, w, l, b, M, s));
            RC(one_pass ? launch_attn_decode1(al, s) : launch_attn_decode(al, s));
            RC(opt_rowsm_tail(d, w, l, b, M, s));
        }
        return opt_rowsm_head(d, w, b, M, logits, s);
    }
    if (opt_rows_usable(d, w, M)) {  // row-dot kernels with LayerNorm / merge in their prologues (gemv.hip): 5 launches + attention per block
        for (int l = 0; l < d->t_layers; ++l) {
            DecodeAttnArgs al = at_block(a, l, kv_layer, gen_layer);
            al.out = nullptr;
            int nsplit = 0;
            RC(opt_rows_qkv(d, w, l, b, M, s));
            RC(launch_attn_decode(al, s, &nsplit));
            RC(opt_rows_tail(d, w, l, b, M, al.part, nsplit, s));
        }
        return opt_rows_head(d, w, b, M, logits, s);
    }
    const int D = d->t_hidden;
    for (int l = 0; l < d->t_layers; ++l) {
        const EilevOptLayer *L = &w->layers[l];
        DecodeAttnArgs al = at_block(a, l, kv_layer, gen_layer);
        al.out_frag = frag;
        if (l == 0) RC(launch_layernorm(b.h, D, (const bf16 *)L->ln1_w, (const bf16 *)L->ln1_b, b.x, D, M, D, d->t_eps, s));
        RC(opt_qkv(d, w, l, b, M, s, l > 0 ? frag : 0));
        RC(launch_attn_decode(al, s));
        // the block's output goes straight into the LayerNorm that reads it next (the next block's, or final_layer_norm): b.x
        const bool last = l + 1 == d->t_layers;
        RC(opt_tail(d, w, l, b, M, s, last ? w->final_ln_w : w->layers[l + 1].ln1_w, last ? w->final_ln_b : w->layers[l + 1].ln1_b, frag));
    }
    GemmArgs g = opt_lm_head(d, w, b, M, logits);
    g.a_frag = frag;
    return launch_gemm(g, 5, s);
}

// The position embedding, the blocks and final_layer_norm of `rows` new token rows per sample at positions past_len .. past_len + rows - 1:
// inputs_embeds -> b.x, every block's keys / values into the cache.  The attention reads its keys / values from the cache, slots [0, past_len +
// rows) (from_cache: extend), or from the q|k|v rows (prefill: past_len == 0).  hidden (nullable): the hidden_states tuple.
int opt_blocks(const EilevDims *d, const EilevOptWeights *w, const OptBufs &b, const void *inputs_embeds, const int32_t *attn_mask, int64_t batch,
               int64_t rows, int64_t past_len, bool from_cache, void *kv_cache, int64_t kv_capacity, void *hidden, hipStream_t s) {
    const int D = d->t_hidden, H = d->t_heads, hd = D / H;
    const int64_t M = batch * rows, total = past_len + rows;
    RC(launch_pos_embed((const bf16 *)inputs_embeds, (const bf16 *)w->embed_positions, attn_mask, b.pid, b.h, (int)batch, (int)total, D,
                        s, (int)past_len));
    const KvCache kv(batch, D, kv_capacity);
    const size_t hs_bytes = (size_t)M * D * sizeof(bf16);  // one entry of the hidden_states tuple
    for (int l = 0; l < d->t_layers; ++l) {
        const EilevOptLayer *L = &w->layers[l];
        bf16 *kc = kv.k((bf16 *)kv_cache, l), *vc = kv.v((bf16 *)kv_cache, l);
        if (hidden) RC(copy_hidden(hidden, l, b.h, hs_bytes, s));  // the block's input
        RC(launch_layernorm(b.h, D, (const bf16 *)L->ln1_w, (const bf16 *)L->ln1_b, b.x, D, M, D, d->t_eps, s));
        RC(opt_qkv(d, w, l, b, M, s));
        RC(launch_kv_write(b.qkv, kc, vc, (int)batch, (int)rows, H, hd, (int)kv_capacity, (int)total, nullptr, s, (int)past_len));
        // queries: the new rows (in the q|k|v buffer); keys / values: the same rows, or the cache, slots [0, total)
        AttnArgs a = from_cache ? attn_cache(b.qkv, 3 * D, kc, vc, kv_capacity, b.att, batch, H, rows, total, hd, 1.0f)
                                : attn_rows(b.qkv, 3 * D, b.qkv + D, 3 * D, b.qkv + 2 * D, 3 * D, b.att, batch, H, rows, total, hd, 1.0f);
        a.causal = 1; a.key_mask = attn_mask; a.mask_ld = total;
        RC(launch_attention(a, s));
        RC(opt_tail(d, w, l, b, M, s));
    }
    RC(launch_layernorm(b.h, D, (const bf16 *)w->final_ln_w, (const bf16 *)w->final_ln_b, b.x, D, M, D, d->t_eps, s));
    if (hidden) RC(copy_hidden(hidden, d->t_layers, b.x, hs_bytes, s));
    return EILEV_OK;
}

int opt_prefill_impl(const EilevDims *d, const EilevOptWeights *w, const void *inputs_embeds, const int32_t *attn_mask, int64_t batch,
                     int64_t seq_len, void *kv_cache, int64_t kv_capacity, float *logits_last, float *logits_all, void *hidden,
                     void *workspace, size_t workspace_bytes, void *stream) {
    if (!d || !w || !inputs_embeds || !attn_mask || !kv_cache || !workspace || batch <= 0 || seq_len <= 0) return EILEV_E_BADARG;
    if (seq_len > kv_capacity || seq_len > d->max_pos) return EILEV_E_BADARG;
    if (!dims_ok_opt(d)) return EILEV_E_UNSUPPORTED;
    if (workspace_bytes < eilev_opt_workspace_bytes(d, batch, seq_len)) return EILEV_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int D = d->t_hidden;
    const int64_t M = batch * seq_len;
    const OptBufs b = carve_opt(d, M, workspace);
    RC(opt_blocks(d, w, b, inputs_embeds, attn_mask, batch, seq_len, 0, false, kv_cache, kv_capacity, hidden, s));
    if (logits_all) {
        GemmArgs g = mk_gemm(b.x, D, w->embed_tokens, D, nullptr, nullptr, 0, logits_all, d->vocab, M, d->vocab, D, 0);
        g.out_f32 = 1;
        RC(launch_gemm(g, 5, s));
    }
    if (logits_last) {
        // last position of every row: a strided [batch, D] view of x
        GemmArgs g = sk_gemm(b.scratch, b.x + (seq_len - 1) * (int64_t)D, seq_len * (int64_t)D, w->embed_tokens, D, nullptr, nullptr, 0,
                             logits_last, d->vocab, batch, d->vocab, D, 0);
        g.out_f32 = 1;
        RC(launch_gemm(g, 5, s));
    }
    return EILEV_OK;
}
}  // namespace

extern "C" int eilev_opt_prefill(const EilevDims *d, const EilevOptWeights *w, const void *inputs_embeds,
                                 const int32_t *attn_mask, int64_t batch, int64_t seq_len, void *kv_cache, int64_t kv_capacity,
                                 float *logits_last, float *logits_all, void *workspace, size_t workspace_bytes, void *stream) {
    return opt_prefill_impl(d, w, inputs_embeds, attn_mask, batch, seq_len, kv_cache, kv_capacity, logits_last, logits_all, nullptr, workspace,
                            workspace_bytes, stream);
}
extern "C" int eilev_opt_prefill_debug(const EilevDims *d, const EilevOptWeights *w, const void *inputs_embeds,
                                       const int32_t *attn_mask, int64_t batch, int64_t seq_len, void *kv_cache, int64_t kv_capacity,
                                       float *logits_last, float *logits_all, void *hidden_states, void *workspace, size_t workspace_bytes,
                                       void *stream) {
    if (!hidden_states) return EILEV_E_BADARG;
    return opt_prefill_impl(d, w, inputs_embeds, attn_mask, batch, seq_len, kv_cache, kv_capacity, logits_last, logits_all, hidden_states,
                            workspace, workspace_bytes, stream);
}

extern "C" int eilev_opt_extend(const EilevDims *d, const EilevOptWeights *w, const void *inputs_embeds, const int32_t *attn_mask,
                                int64_t batch, int64_t new_len, int64_t past_len, void *kv_cache, int64_t kv_capacity,
                                float *logits_all, void *workspace, size_t workspace_bytes, void *stream) {
    if (!d || !w || !inputs_embeds || !attn_mask || !kv_cache || !logits_all || !workspace || batch <= 0 || new_len <= 0 || past_len < 0)
        return EILEV_E_BADARG;
    const int64_t total = past_len + new_len;
    if (total > kv_capacity || total > d->max_pos) return EILEV_E_BADARG;
    if (!dims_ok_opt(d)) return EILEV_E_UNSUPPORTED;
    if (workspace_bytes < eilev_opt_workspace_bytes(d, batch, total)) return EILEV_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int D = d->t_hidden;
    const int64_t M = batch * new_len;
    const OptBufs b = carve_opt(d, batch * total, workspace);
    RC(opt_blocks(d, w, b, inputs_embeds, attn_mask, batch, new_len, past_len, true, kv_cache, kv_capacity, nullptr, s));
    GemmArgs g = sk_gemm(b.scratch, b.x, D, w->embed_tokens, D, nullptr, nullptr, 0, logits_all, d->vocab, M, d->vocab, D, 0);
    g.out_f32 = 1;
    return launch_gemm(g, 5, s);
}

extern "C" int eilev_greedy_select(const float *logits, int64_t batch, int64_t vocab, int32_t *state, uint8_t *finished,
                                   int64_t eos_id, int64_t pad_id, int64_t *tokens, int64_t *out_tokens, int64_t max_new,
                                   void *stream) {
    if (!logits || !state || !finished || !tokens || !out_tokens || batch <= 0) return EILEV_E_BADARG;
    return launch_select(logits, (int)batch, (int)vocab, state, finished, eos_id, pad_id, tokens, out_tokens, max_new,
                         (hipStream_t)stream);
}

extern "C" int eilev_topk_logprob(const float *logits, const float *row_score, int64_t rows, int64_t vocab, int64_t keep, float *out_val,
                                  int32_t *out_idx, void *stream) {
    if (!logits || !out_val || !out_idx || rows < 0 || vocab <= 0 || keep <= 0 || keep > vocab) return EILEV_E_BADARG;
    if (rows == 0) return EILEV_OK;
    return launch_topk_logprob(logits, row_score, (int)rows, (int)vocab, (int)keep, out_val, out_idx, (hipStream_t)stream);
}

extern "C" size_t eilev_beam_scratch_bytes(int64_t batch, int64_t beams, int64_t keep, int64_t max_new) {
    return sizeof(int64_t) * (size_t)batch * (size_t)(keep + 2 * beams) * (size_t)max_new;
}
extern "C" int eilev_beam_advance(const float *row_lp, const int32_t *row_tok, int64_t batch, int64_t beams, int64_t keep, int64_t max_new,
                                  const int32_t *state, const int64_t *eos_ids, int64_t n_eos, const float *len_pow, int len_pow_reciprocal,
                                  int early_stopping, int64_t *run_seq, float *run_score, int64_t *fin_seq, float *fin_score, int64_t *fin_len,
                                  uint8_t *finished, uint8_t *can_improve, int64_t *tokens, int32_t *anc, int64_t gen_cap, void *scratch,
                                  size_t scratch_bytes, void *stream) {
    if (!row_lp || !row_tok || !state || !len_pow || !run_seq || !run_score || !fin_seq || !fin_score || !fin_len || !finished || !can_improve ||
        !tokens || batch <= 0 || beams <= 0 || keep < beams || max_new <= 0 || n_eos < 0 || (n_eos > 0 && !eos_ids))
        return EILEV_E_BADARG;
    if (!scratch || scratch_bytes < eilev_beam_scratch_bytes(batch, beams, keep, max_new)) return EILEV_E_WORKSPACE;
    return launch_beam_advance(row_lp, row_tok, (int)batch, (int)beams, (int)keep, (int)max_new, state, eos_ids, (int)n_eos, len_pow,
                               len_pow_reciprocal, early_stopping, run_seq, run_score, fin_seq, fin_score, fin_len, finished, can_improve, tokens,
                               anc, (int)gen_cap, (int64_t *)scratch, (hipStream_t)stream);
}

extern "C" int eilev_opt_decode_step(const EilevDims *d, const EilevOptWeights *w, int64_t *tokens, int32_t *state,
                                     const int32_t *attn_mask, const int32_t *n_valid, int64_t batch, int64_t seq_len,
                                     void *kv_cache, int64_t kv_capacity, float *logits, uint8_t *finished, int64_t eos_id,
                                     int64_t pad_id, int64_t *out_tokens, int64_t max_new, void *workspace,
                                     size_t workspace_bytes, void *stream) {
    if (!d || !w || !tokens || !state || !attn_mask || !n_valid || !kv_cache || !logits || !finished || !out_tokens || !workspace)
        return EILEV_E_BADARG;
    if (batch <= 0 || seq_len + max_new > kv_capacity + 1) return EILEV_E_BADARG;
    if (!dims_ok_opt(d)) return EILEV_E_UNSUPPORTED;
    if (workspace_bytes < eilev_opt_workspace_bytes(d, batch, 1)) return EILEV_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int D = d->t_hidden, H = d->t_heads, hd = D / H;
    const OptBufs b = carve_opt(d, batch, workspace);
    RC(launch_decode_embed((const bf16 *)w->embed_tokens, (const bf16 *)w->embed_positions, tokens, n_valid, state, d->vocab,
                           d->max_pos + 1, b.h, (int)batch, D, s));
    const KvCache kv(batch, D, kv_capacity);
    DecodeAttnArgs a = decode_attn_args(b.qkv, b.att, b.scratch, batch, H, hd);  // block 0's
    a.kc = kv.k((const bf16 *)kv_cache, 0); a.vc = kv.v((const bf16 *)kv_cache, 0); a.attn_mask = attn_mask; a.state = state; a.seq_len = (int)seq_len; a.cap = (int)kv_capacity;
    a.fuse_new = 1;  // the new token's K / V go into the cache inside the attention kernel: one launch less per block
    if (opt_rows1_usable(d, w, batch, kv_capacity)) {  // ONE row (round 4): register-resident activations, one-pass attention: 5 launches per block
        for (int l = 0; l < d->t_layers; ++l) {
            const EilevOptLayer *L = &w->layers[l];
            const DecodeAttnArgs al = at_block(a, l, kv.per_layer(), 0);
            const int Ft = d->t_ffn;
            RC(launch_gemv1(1, b.h, (const bf16 *)L->ln1_w, (const bf16 *)L->ln1_b, d->t_eps, (const bf16 *)L->q_w, (const bf16 *)L->q_b, nullptr, b.qkv, 0, 3 * D, D, 0,
                            1.0f / sqrtf((float)hd), D, s));
            if (hd == 80 && g_decode_rows != 5) {  // 128-key splits over all CUs, merged in out_proj's prologue (eilev_debug_decode_rows(5): one workgroup per head)
                int nsplit = 0;
                RC(launch_attn_decode_part(al, s, &nsplit));
                RC(launch_gemv1(2, nullptr, nullptr, nullptr, 0.f, (const bf16 *)L->o_w, (const bf16 *)L->o_b, b.h, b.h, 0, D, D, 0, 1.0f, 0, s, al.part, H, hd,
                                nsplit));
            } else {
                RC(launch_attn_decode1(al, s));
                RC(launch_gemv1(0, b.att, nullptr, nullptr, 0.f, (const bf16 *)L->o_w, (const bf16 *)L->o_b, b.h, b.h, 0, D, D, 0, 1.0f, 0, s));
            }
            RC(launch_gemv1(1, b.h, (const bf16 *)L->ln2_w, (const bf16 *)L->ln2_b, d->t_eps, (const bf16 *)L->fc1_w, (const bf16 *)L->fc1_b, nullptr, b.ffn, 0, Ft, D, 2,
                            1.0f, 0, s));
            RC(launch_gemv1(0, b.ffn, nullptr, nullptr, 0.f, (const bf16 *)L->fc2_w, (const bf16 *)L->fc2_b, b.h, b.h, 0, D, Ft, 0, 1.0f, 0, s));
        }
        RC(launch_gemv1(1, b.h, (const bf16 *)w->final_ln_w, (const bf16 *)w->final_ln_b, d->t_eps, (const bf16 *)w->embed_tokens, nullptr, nullptr, logits, 1, d->vocab,
                        D, 0, 1.0f, 0, s));
        return launch_select(logits, 1, d->vocab, state, finished, eos_id, pad_id, tokens, out_tokens, max_new, s);
    }
    // 17..32 rows (round 5): the activations between the kernels of a block (attention rows, LayerNorm rows, fc1 rows) in the row-block layout
    // (common.h frag32_index) when every linear of the block runs on gemm_rows32_kernel and the attention on attn_decode_loop_kernel — a
    // dry run of the block's launches decides; the first q|k|v projection reads the row-major LayerNorm of the embedding rows
    int frag = 0;
    if (g_decode_frag && batch > 16 && batch <= 32 && !w->layers_w8 && D % 32 == 0 && d->t_ffn % 32 == 0 && attn_decode_loop_ok(a)) {
        GemmArgs gh = opt_lm_head(d, w, b, batch, logits);
        gh.a_frag = 1;
        GemmArgs gq = sk_gemm(b.scratch, b.x, D, w->layers[0].q_w, D, w->layers[0].q_b, nullptr, 0, b.qkv, 3 * D, batch, D, D, 0);  // q, k, v one by one
        gq.a_frag = 1;
        GemmArgs gq3 = gq;  // ... or as one [3 D, D] matrix (opt_qkv decides per block)
        gq3.N = 3 * D;
        frag = gemm_rows32_takes(gh) && gemm_rows32_takes(gq) && gemm_rows32_takes(gq3) &&
               opt_tail(d, w, 0, b, batch, s, w->final_ln_w, w->final_ln_b, 1, true) == EILEV_OK;
    }
    RC(opt_decode_blocks(d, w, b, batch, a, kv.per_layer(), 0, attn_decode1_ok((int)batch, (int)kv_capacity, hd), frag, logits, s));
    return launch_select(logits, (int)batch, d->vocab, state, finished, eos_id, pad_id, tokens, out_tokens, max_new, s);
}

namespace {
__global__ void bump_step_kernel(int32_t *state) {
    if (threadIdx.x == 0 && blockIdx.x == 0) state[0] += 1;
}
}  // namespace

// One decode step of beam search WITHOUT moving the KV cache (include/eilev.h): the prompt's keys / values stay in the prefill cache, one
// row per SAMPLE; the generated tokens' in a generation cache, one row per beam SLOT; `ancestors[g][r]` names the slot that holds the g-th
// generated token of the hypothesis now living in row r.  (Before: torch index_select of the whole cache per step — 1.6 GB at 5 beams.)
// shared_prompt (include/eilev_prefix.h eilev_prefix_decode_step): the attention reads a sample's prompt keys once for its rows
// (DecodeAttnArgs.shared_prompt); its partials lie behind the step's own workspace
size_t opt_decode_step_beam_shared_bytes(const EilevDims *d, int64_t rows, int64_t seq_len, int64_t gen_capacity) {
    if (!d || !dims_ok_opt(d) || rows <= 0 || rows > 32 || seq_len <= 0 || gen_capacity <= 0 || seq_len + gen_capacity > (1 << 20)) return 0;
    return align_up(eilev_opt_workspace_bytes(d, rows, 1), 256) +
           attn_decode_shared_part_bytes((int)rows, d->t_heads, d->t_hidden / d->t_heads, (int)seq_len, (int)gen_capacity);
}
int opt_decode_step_beam(const EilevDims *d, const EilevOptWeights *w, const int64_t *tokens, int32_t *state, const int32_t *attn_mask,
                         const int32_t *n_valid, int64_t rows, int64_t beams, int64_t seq_len, const void *kv_prompt, void *kv_gen, int64_t gen_capacity,
                         const int32_t *ancestors, float *logits, void *workspace, size_t workspace_bytes, void *stream, int shared_prompt) {
    if (!d || !w || !tokens || !state || !attn_mask || !n_valid || !kv_prompt || !kv_gen || !ancestors || !logits || !workspace) return EILEV_E_BADARG;
    if (rows <= 0 || beams <= 0 || rows % beams || seq_len <= 0 || gen_capacity <= 0 || rows > 32) return EILEV_E_BADARG;
    if (!dims_ok_opt(d)) return EILEV_E_UNSUPPORTED;
    const int D = d->t_hidden, H = d->t_heads, hd = D / H;
    if (shared_prompt) {
        if (hd != 80 && hd != 128) return EILEV_E_UNSUPPORTED;
        if (seq_len + gen_capacity > (1 << 20) || (((uintptr_t)kv_prompt | (uintptr_t)kv_gen | (uintptr_t)workspace) & 15) != 0) return EILEV_E_BADARG;
        if (workspace_bytes < opt_decode_step_beam_shared_bytes(d, rows, seq_len, gen_capacity)) return EILEV_E_WORKSPACE;
    }
    if (workspace_bytes < eilev_opt_workspace_bytes(d, rows, 1)) return EILEV_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t samples = rows / beams;
    const OptBufs b = carve_opt(d, rows, workspace);
    // block 0's attention: the prompt's keys in kv_prompt [layers][k | v][samples][heads][seq_len][hd], the generated ones in kv_gen (a row per beam slot)
    const KvCache kp(samples, D, seq_len), kg(rows, D, gen_capacity);
    DecodeAttnArgs a = decode_attn_args(b.qkv, b.att, b.scratch, rows, H, hd);
    if (shared_prompt) {
        a.shared_prompt = 1;
        a.part = reinterpret_cast<float *>((char *)workspace + align_up(eilev_opt_workspace_bytes(d, rows, 1), 256));
        a.part_bytes = attn_decode_shared_part_bytes((int)rows, H, hd, (int)seq_len, (int)gen_capacity);
    } else if (attn_decode_part_bytes((int)rows, H, hd, (int)(seq_len + gen_capacity)) > a.part_bytes) {
        return EILEV_E_WORKSPACE;
    }
    a.kc = kp.k((const bf16 *)kv_prompt, 0); a.vc = kp.v((const bf16 *)kv_prompt, 0); a.attn_mask = attn_mask; a.state = state; a.seq_len = a.cap = (int)seq_len; a.fuse_new = 1;
    a.kg = kg.k((bf16 *)kv_gen, 0); a.vg = kg.v((bf16 *)kv_gen, 0); a.anc = ancestors; a.beams = (int)beams; a.cap_g = (int)gen_capacity;
    RC(launch_decode_embed((const bf16 *)w->embed_tokens, (const bf16 *)w->embed_positions, tokens, n_valid, state, d->vocab, d->max_pos + 1, b.h,
                           (int)rows, D, s));
    RC(opt_decode_blocks(d, w, b, rows, a, kp.per_layer(), kg.per_layer(), false, 0, logits, s));
    bump_step_kernel<<<1, 64, 0, s>>>(state);  // the step counter lives on the device: a captured step replays for every step
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}
extern "C" int eilev_opt_decode_step_beam(const EilevDims *d, const EilevOptWeights *w, const int64_t *tokens, int32_t *state,
                                          const int32_t *attn_mask, const int32_t *n_valid, int64_t rows, int64_t beams, int64_t seq_len,
                                          const void *kv_prompt, void *kv_gen, int64_t gen_capacity, const int32_t *ancestors, float *logits,
                                          void *workspace, size_t workspace_bytes, void *stream) {
    return opt_decode_step_beam(d, w, tokens, state, attn_mask, n_valid, rows, beams, seq_len, kv_prompt, kv_gen, gen_capacity, ancestors, logits, workspace,
                                workspace_bytes, stream, 0);
}

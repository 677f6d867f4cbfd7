// t5.hip — the encoder-decoder language model, flan-t5 (include/eilev.h "encoder-decoder"): encoder, cross-attention cache, decoder.
#include "stages.h"

// =====================================================================================================
// Encoder-decoder language model: flan-t5 (hf models/t5/modeling_t5.py; include/eilev.h "encoder-decoder")
// =====================================================================================================
namespace {
struct T5Bufs {
    bf16 *h, *x, *qkv, *att, *ff, *gate;
    float *rel, *scratch;
    int64_t rel_n;
};
bool carve_t5(const EilevT5Dims *d, int64_t M, int64_t rel_n, void *ws, size_t bytes, T5Bufs &b) {
    const size_t I = (size_t)d->heads * d->d_kv;
    Carver cv{(char *)ws};
    b.h = cv.take<bf16>((size_t)M * d->d_model);
    b.x = cv.take<bf16>((size_t)M * d->d_model);
    b.qkv = cv.take<bf16>((size_t)M * 3 * I);
    b.att = cv.take<bf16>((size_t)M * I);
    b.ff = cv.take<bf16>((size_t)M * 2 * d->d_ff);
    b.gate = cv.take<bf16>((size_t)M * d->d_ff);
    b.rel = cv.take<float>((size_t)d->heads * rel_n);
    b.scratch = cv.take<float>(kSkinnyScratch / sizeof(float));
    b.rel_n = rel_n;
    return cv.used <= bytes;
}
GemmArgs t5_gemm(const T5Bufs &b, const bf16 *A, int64_t lda, const void *W, int64_t ldw, const bf16 *resid, int64_t ldr, void *Cp,
                 int64_t ldc, int64_t M, int N, int K) {
    return sk_gemm(b.scratch, A, lda, W, ldw, nullptr, resid, ldr, Cp, ldc, M, N, K, 0);
}
// up to three projections of x with a shared input: one GEMM when the weights sit back to back in memory (the engine packs them)
int t5_proj(const T5Bufs &b, const bf16 *x, int D, const void *w0, const void *w1, const void *w2, int n_each, bf16 *out, int64_t ldo,
            int64_t M, hipStream_t s) {
    const void *ws[3] = {w0, w1, w2};
    const int cnt = 1 + (w1 != nullptr) + (w2 != nullptr);
    if (packed(ws, cnt, (size_t)n_each * D)) return launch_gemm(t5_gemm(b, x, D, w0, D, nullptr, 0, out, ldo, M, cnt * n_each, D), 5, s);
    for (int i = 0; i < cnt; ++i) RC(launch_gemm(t5_gemm(b, x, D, ws[i], D, nullptr, 0, out + (size_t)i * n_each, ldo, M, n_each, D), 5, s));
    return EILEV_OK;
}
// h += wo(gelu_new(wi_0 x) * wi_1 x) with x = rmsnorm(h)   [T5LayerFF :126-141, T5DenseGatedActDense :97-124]
// normed_in: b.x already holds RMSNorm_ff(h) (written by the reduce of the GEMV before); next_ln: the RMSNorm weight whose output of the new h
// the wo GEMV's reduce should leave in b.x (decode steps: see t5_decode_impl)
int t5_ff(const EilevT5Dims *d, const EilevT5Layer *L, const T5Bufs &b, int64_t M, hipStream_t s, bool normed_in = false, const void *next_ln = nullptr) {
    const int D = d->d_model, F = d->d_ff;
    if (!normed_in) RC(launch_rmsnorm(b.h, D, (const bf16 *)L->ln_ff, b.x, D, M, D, d->eps, s));
    RC(t5_proj(b, b.x, D, L->wi0_w, L->wi1_w, nullptr, F, b.ff, 2 * F, M, s));
    RC(launch_gated_gelu(b.ff, 2 * F, b.gate, M, F, s));
    GemmArgs g = t5_gemm(b, b.gate, F, L->wo_w, F, b.h, D, b.h, D, M, D, F);
    if (next_ln) { g.ln_gamma = (const bf16 *)next_ln; g.ln_beta = nullptr; g.ln_out = b.x; g.ln_eps = d->eps; }
    return launch_gemm(g, 5, s);
}
}  // namespace

extern "C" size_t eilev_t5_workspace_bytes(const EilevT5Dims *d, int64_t batch, int64_t rows, int64_t kv_len) {
    const size_t M = (size_t)batch * rows, I = (size_t)d->heads * d->d_kv;
    const size_t rel_n = (size_t)(rows + kv_len + 1);
    return (M * (2 * (size_t)d->d_model + 4 * I + 3 * (size_t)d->d_ff)) * sizeof(bf16) + d->heads * rel_n * sizeof(float) + kSkinnyScratch +
           16 * 256;
}

// hidden_out (nullable): (enc_layers + 1, batch, enc_len, D) = hf T5Stack's hidden_states tuple: every block's input, then the output of
// final_layer_norm (modeling_t5.py T5Stack.forward: all_hidden_states)
static int t5_encode_impl(const EilevT5Dims *d, const EilevT5Weights *w, const void *inputs_embeds, const int32_t *attn_mask,
                          int64_t batch, int64_t enc_len, void *enc_out, void *hidden_out, void *workspace, size_t workspace_bytes,
                          void *stream) {
    if (!d || !w || !inputs_embeds || !attn_mask || !enc_out || !workspace || batch <= 0 || enc_len <= 0) return EILEV_E_BADARG;
    if (!dims_ok_t5(d)) return EILEV_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const int D = d->d_model, H = d->heads, hd = d->d_kv, I = H * hd;
    const int64_t M = batch * enc_len;
    T5Bufs b;
    if (!carve_t5(d, M, 2 * enc_len + 1, workspace, workspace_bytes, b)) return EILEV_E_WORKSPACE;
    EILEV_HIP_CHECK(hipMemcpyAsync(b.h, inputs_embeds, (size_t)M * D * sizeof(bf16), hipMemcpyDeviceToDevice, s));
    // bias(i, j) depends on j - i in [-(L-1), L-1]: table index (j - i) + L - 1
    RC(launch_t5_rel_table((const bf16 *)w->enc_rel_bias, b.rel, (int)(2 * enc_len - 1), (int)enc_len - 1, H, 1, d->rel_buckets,
                           d->rel_max_dist, s));
    const size_t hid_bytes = (size_t)M * D * sizeof(bf16);
    for (int l = 0; l < d->enc_layers; ++l) {
        const EilevT5Layer *L = &w->enc_layers[l];
        if (hidden_out) RC(copy_hidden(hidden_out, l, b.h, hid_bytes, s));
        RC(launch_rmsnorm(b.h, D, (const bf16 *)L->ln_sa, b.x, D, M, D, d->eps, s));
        RC(t5_proj(b, b.x, D, L->q_w, L->k_w, L->v_w, I, b.qkv, 3 * I, M, s));
        AttnArgs a = attn_rows(b.qkv, 3 * I, b.qkv + I, 3 * I, b.qkv + 2 * I, 3 * I, b.att, batch, H, enc_len, enc_len, hd, 1.0f);
        a.key_mask = attn_mask; a.mask_ld = enc_len;
        a.rel_tab = b.rel; a.rel_hs = 2 * enc_len - 1; a.rel_off = (int)enc_len - 1; a.rel_n = (int)(2 * enc_len - 1);
        RC(launch_attention(a, s));
        RC(launch_gemm(t5_gemm(b, b.att, I, L->o_w, I, b.h, D, b.h, D, M, D, I), 5, s));
        RC(t5_ff(d, L, b, M, s));
    }
    RC(launch_rmsnorm(b.h, D, (const bf16 *)w->enc_final_ln, (bf16 *)enc_out, D, M, D, d->eps, s));
    if (hidden_out) RC(copy_hidden(hidden_out, d->enc_layers, enc_out, hid_bytes, s));
    return EILEV_OK;
}

extern "C" int eilev_t5_encode(const EilevT5Dims *d, const EilevT5Weights *w, const void *inputs_embeds, const int32_t *attn_mask,
                               int64_t batch, int64_t enc_len, void *enc_out, void *workspace, size_t workspace_bytes, void *stream) {
    return t5_encode_impl(d, w, inputs_embeds, attn_mask, batch, enc_len, enc_out, nullptr, workspace, workspace_bytes, stream);
}
extern "C" int eilev_t5_encode_debug(const EilevT5Dims *d, const EilevT5Weights *w, const void *inputs_embeds, const int32_t *attn_mask,
                                     int64_t batch, int64_t enc_len, void *enc_out, void *hidden_out, void *workspace,
                                     size_t workspace_bytes, void *stream) {
    return t5_encode_impl(d, w, inputs_embeds, attn_mask, batch, enc_len, enc_out, hidden_out, workspace, workspace_bytes, stream);
}

extern "C" size_t eilev_t5_cross_kv_bytes(const EilevT5Dims *d, int64_t batch, int64_t enc_len) {
    return KvCache(batch, (int64_t)d->heads * d->d_kv, enc_len).bytes(d->dec_layers);
}
extern "C" size_t eilev_t5_self_kv_bytes(const EilevT5Dims *d, int64_t batch, int64_t kv_capacity) {
    return KvCache(batch, (int64_t)d->heads * d->d_kv, kv_capacity).bytes(d->dec_layers);
}

// k|v of every decoder block from the encoder output: one GEMM per layer (two when the weights are not packed back to back)
// into the workspace, then re-tiled per head into the cache planes.
extern "C" int eilev_t5_cross_kv(const EilevT5Dims *d, const EilevT5Weights *w, const void *enc_out, int64_t batch, int64_t enc_len,
                                 void *cross_kv, void *workspace, size_t workspace_bytes, void *stream) {
    if (!d || !w || !enc_out || !cross_kv || !workspace || batch <= 0 || enc_len <= 0) return EILEV_E_BADARG;
    if (!dims_ok_t5(d)) return EILEV_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const int D = d->d_model, H = d->heads, hd = d->d_kv, I = H * hd;
    const int64_t M = batch * enc_len;
    T5Bufs b;
    if (!carve_t5(d, M, 1, workspace, workspace_bytes, b)) return EILEV_E_WORKSPACE;
    const KvCache kv(batch, I, enc_len);
    for (int l = 0; l < d->dec_layers; ++l) {
        const EilevT5Layer *L = &w->dec_layers[l];
        bf16 *kc = kv.k((bf16 *)cross_kv, l), *vc = kv.v((bf16 *)cross_kv, l);
        RC(t5_proj(b, (const bf16 *)enc_out, D, L->ck_w, L->cv_w, nullptr, I, b.qkv, 2 * I, M, s));
        RC(launch_rows_to_cache(b.qkv, 2 * I, 0, kc, (int)batch, (int)enc_len, H, hd, (int)enc_len, 0, s));
        RC(launch_rows_to_cache(b.qkv, 2 * I, I, vc, (int)batch, (int)enc_len, H, hd, (int)enc_len, 0, s));
    }
    return EILEV_OK;
}

// `state` != null: single-token step whose position is state[0] on the device (host past_len = 0, the buffers are sized
// for the whole capacity); null: positions past_len .. past_len + new_len - 1 given by the host
// `beam` != null (with `state`; stages.h T5BeamArgs): the step of beam search that moves no cache row.  self_kv is then the START cache (one
// row per sample, capacity 1) and kv_capacity = 1 + gen_capacity; the self-attention takes the ancestor form of the split kernel (key 0 =
// the start token, key 1 + g = generation slot g of row ancestors[g][r], the new token to the row's own slot state[0] - 1), the
// cross-attention the kernel in which a sample's rows share its K / V (cross_kv and enc_mask have one row per SAMPLE)
static int t5_decode_impl(const EilevT5Dims *d, const EilevT5Weights *w, const int64_t *dec_ids, const int32_t *enc_mask,
                          int64_t batch, int64_t new_len, int64_t past_len, const int32_t *state, void *self_kv, int64_t kv_capacity,
                          const void *cross_kv, int64_t enc_len, float *logits, void *workspace, size_t workspace_bytes,
                          void *stream, const int32_t *dec_mask = nullptr, void *hidden_out = nullptr, const T5BeamArgs *beam = nullptr) {
    if (!d || !w || !dec_ids || !enc_mask || !self_kv || !cross_kv || !logits || !workspace) return EILEV_E_BADARG;
    if (state && (dec_mask || hidden_out)) return EILEV_E_BADARG;
    if (batch <= 0 || new_len <= 0 || past_len < 0 || past_len + new_len > kv_capacity || enc_len <= 0) return EILEV_E_BADARG;
    if (state && (new_len != 1 || past_len != 0)) return EILEV_E_BADARG;
    if (beam && (!state || !beam->kv_gen || !beam->ancestors || beam->beams <= 0 || beam->beams > 32 || batch > 32 || batch % beam->beams ||
                 beam->gen_capacity <= 0 || kv_capacity != beam->gen_capacity + 1))
        return EILEV_E_BADARG;
    if (!dims_ok_t5(d) || (beam && d->d_kv != 64)) return EILEV_E_UNSUPPORTED;
    hipStream_t s = (hipStream_t)stream;
    const int D = d->d_model, H = d->heads, hd = d->d_kv, I = H * hd;
    const int64_t M = batch * new_len, total = state ? kv_capacity : past_len + new_len;  // with `state`: an upper bound
    T5Bufs b;
    if (!carve_t5(d, M, total + 1, workspace, workspace_bytes, b)) return EILEV_E_WORKSPACE;
    RC(launch_embed_scatter((const bf16 *)w->shared, dec_ids, nullptr, nullptr, 0, M, d->vocab, b.h, D, s));
    // causal self-attention: key j of query at absolute position p: rel = j - p in [-(total-1), 0]: index rel + total - 1
    // (with `state` the table holds the single query row at position state[0]: entry j = bias of key j)
    RC(launch_t5_rel_table((const bf16 *)w->dec_rel_bias, b.rel, (int)total, (int)total - 1, H, 0, d->rel_buckets, d->rel_max_dist, s,
                           state));
    const int64_t samples = beam ? batch / beam->beams : batch;
    const KvCache skv(samples, I, beam ? 1 : kv_capacity), ckv(samples, I, enc_len), gkv(batch, I, beam ? beam->gen_capacity : 0);
    // single-query steps: the decode-attention kernels (the self-attention over keys 0 .. total - 1 of the cache, the bias of one query row)
    DecodeAttnArgs sa = decode_attn_args(b.qkv, b.att, b.scratch, batch, H, hd), ca = sa;
    sa.ldq = 3 * (int64_t)I; sa.attn_mask = dec_mask; sa.cap = (int)kv_capacity; sa.rel_tab = b.rel; sa.rel_hs = total;
    // with `state`: kv_total = 1 + state[0] on the device, the table is this query's row (entry j = key j), the kernel stores the new K / V
    sa.state = state; sa.seq_len = state ? 1 : (int)total; sa.rel_off = state ? -1 : (int)total - 1; sa.fuse_new = state ? 1 : 0;
    ca.ldq = I; ca.attn_mask = enc_mask; ca.seq_len = ca.cap = (int)enc_len;
    if (beam) { sa.cap = 1; sa.anc = beam->ancestors; sa.beams = (int)beam->beams; sa.cap_g = (int)beam->gen_capacity; }
    const int64_t kmax = kv_capacity > enc_len ? kv_capacity : enc_len;
    const bool single = new_len == 1 && attn_decode_part_bytes((int)batch, H, hd, (int)kmax) <= sa.part_bytes;
    if (state && !single) return EILEV_E_UNSUPPORTED;
    if (beam && attn_decode_part_bytes((int)batch, H, hd, (int)kv_capacity, 256) > sa.part_bytes) return EILEV_E_UNSUPPORTED;
    const size_t hid_bytes = (size_t)M * D * sizeof(bf16);
    const bool fuse_norm = single && M <= 32 && !hidden_out;  // the weight-streaming GEMVs of a decode step (their reduce can carry a norm)
    for (int l = 0; l < d->dec_layers; ++l) {
        const EilevT5Layer *L = &w->dec_layers[l];
        bf16 *kc = skv.k((bf16 *)self_kv, l), *vc = skv.v((bf16 *)self_kv, l);
        const bf16 *ck = ckv.k((const bf16 *)cross_kv, l), *cv = ckv.v((const bf16 *)cross_kv, l);
        if (hidden_out) RC(copy_hidden(hidden_out, l, b.h, hid_bytes, s));
        // ---- self-attention against the cache (T5LayerSelfAttention :372-401)
        // (decode steps, round 5: the RMSNorm in front of every projection is produced by the residual GEMV before it — its split-K reduce
        //  writes h and RMSNorm(h) in one launch (GemmArgs::ln_out with ln_beta == nullptr) — so only block 0 normalises here)
        if (!fuse_norm || l == 0) RC(launch_rmsnorm(b.h, D, (const bf16 *)L->ln_sa, b.x, D, M, D, d->eps, s));
        RC(t5_proj(b, b.x, D, L->q_w, L->k_w, L->v_w, I, b.qkv, 3 * I, M, s));
        // (graph-replayed decode steps, round 5: the new token's K / V go into the cache inside the attention kernel — fuse_new, as in the OPT step)
        if (!state) {
            RC(launch_rows_to_cache(b.qkv, 3 * I, I, kc, (int)batch, (int)new_len, H, hd, (int)kv_capacity, (int)past_len, s, state));
            RC(launch_rows_to_cache(b.qkv, 3 * I, 2 * I, vc, (int)batch, (int)new_len, H, hd, (int)kv_capacity, (int)past_len, s, state));
        }
        if (single) {
            sa.kc = kc; sa.vc = vc;
            if (beam) { sa.kg = gkv.k((bf16 *)beam->kv_gen, l); sa.vg = gkv.v((bf16 *)beam->kv_gen, l); }
            RC(launch_attn_decode(sa, s));
        } else {
            AttnArgs a = attn_cache(b.qkv, 3 * I, kc, vc, kv_capacity, b.att, batch, H, new_len, total, hd, 1.0f);
            a.causal = 1;
            a.key_mask = dec_mask; a.mask_ld = dec_mask ? total : 0;  // decoder_attention_mask: keys of padded target positions
            a.rel_tab = b.rel; a.rel_hs = total; a.rel_off = (int)total - 1; a.rel_n = (int)total;
            RC(launch_attention(a, s));
        }
        {
            GemmArgs go = t5_gemm(b, b.att, I, L->o_w, I, b.h, D, b.h, D, M, D, I);
            if (fuse_norm) { go.ln_gamma = (const bf16 *)L->ln_ca; go.ln_beta = nullptr; go.ln_out = b.x; go.ln_eps = d->eps; }
            RC(launch_gemm(go, 5, s));
        }
        // ---- cross-attention over the encoder output (T5LayerCrossAttention :404-432): no position bias, padding mask
        if (!fuse_norm) RC(launch_rmsnorm(b.h, D, (const bf16 *)L->ln_ca, b.x, D, M, D, d->eps, s));
        RC(launch_gemm(t5_gemm(b, b.x, D, L->cq_w, D, nullptr, 0, b.qkv, I, M, I, D), 5, s));
        if (beam) {
            RC(launch_attn_cross_shared(b.qkv, I, ck, cv, enc_mask, (int)batch, (int)beam->beams, H, hd, (int)enc_len, (int)enc_len, b.att, ca.part,
                                        ca.part_bytes, s));
        } else if (single) {
            ca.kc = ck; ca.vc = cv;
            RC(launch_attn_decode(ca, s));
        } else {
            AttnArgs c = attn_cache(b.qkv, I, ck, cv, enc_len, b.att, batch, H, new_len, enc_len, hd, 1.0f);
            c.key_mask = enc_mask; c.mask_ld = enc_len;
            RC(launch_attention(c, s));
        }
        {
            GemmArgs gc = t5_gemm(b, b.att, I, L->co_w, I, b.h, D, b.h, D, M, D, I);
            if (fuse_norm) { gc.ln_gamma = (const bf16 *)L->ln_ff; gc.ln_beta = nullptr; gc.ln_out = b.x; gc.ln_eps = d->eps; }
            RC(launch_gemm(gc, 5, s));
        }
        RC(t5_ff(d, L, b, M, s, fuse_norm, fuse_norm ? (l + 1 < d->dec_layers ? w->dec_layers[l + 1].ln_sa : w->dec_final_ln) : nullptr));
    }
    if (!fuse_norm) RC(launch_rmsnorm(b.h, D, (const bf16 *)w->dec_final_ln, b.x, D, M, D, d->eps, s));
    if (hidden_out) RC(copy_hidden(hidden_out, d->dec_layers, b.x, hid_bytes, s));
    GemmArgs g = t5_gemm(b, b.x, D, w->lm_head, D, nullptr, 0, logits, d->vocab, M, d->vocab, D);
    g.out_f32 = 1;
    if (d->scale_decoder_outputs) { g.scale = 1.0f / sqrtf((float)D); g.scale_cols = d->vocab; }
    return launch_gemm(g, 5, s);
}

extern "C" int eilev_t5_decode(const EilevT5Dims *d, const EilevT5Weights *w, const int64_t *dec_ids, const int32_t *enc_mask,
                               int64_t batch, int64_t new_len, int64_t past_len, void *self_kv, int64_t kv_capacity,
                               const void *cross_kv, int64_t enc_len, float *logits, void *workspace, size_t workspace_bytes,
                               void *stream) {
    return t5_decode_impl(d, w, dec_ids, enc_mask, batch, new_len, past_len, nullptr, self_kv, kv_capacity, cross_kv, enc_len, logits,
                          workspace, workspace_bytes, stream);
}

// eilev_t5_decode + decoder_attention_mask (dec_mask (batch, past_len + new_len) int32, nullable: keys of the target the self-attention must
// not see, on top of the causal rule; hf T5Stack: create_causal_mask(attention_mask = decoder_attention_mask)) + the per-block tensors
// (hidden_out (dec_layers + 1, batch, new_len, D), nullable)
extern "C" int eilev_t5_decode_debug(const EilevT5Dims *d, const EilevT5Weights *w, const int64_t *dec_ids, const int32_t *enc_mask,
                                     const int32_t *dec_mask, int64_t batch, int64_t new_len, int64_t past_len, void *self_kv,
                                     int64_t kv_capacity, const void *cross_kv, int64_t enc_len, float *logits, void *hidden_out,
                                     void *workspace, size_t workspace_bytes, void *stream) {
    return t5_decode_impl(d, w, dec_ids, enc_mask, batch, new_len, past_len, nullptr, self_kv, kv_capacity, cross_kv, enc_len, logits,
                          workspace, workspace_bytes, stream, dec_mask, hidden_out);
}

extern "C" int eilev_t5_decode_step(const EilevT5Dims *d, const EilevT5Weights *w, const int64_t *tokens, const int32_t *state,
                                    const int32_t *enc_mask, int64_t batch, void *self_kv, int64_t kv_capacity, const void *cross_kv,
                                    int64_t enc_len, float *logits, void *workspace, size_t workspace_bytes, void *stream) {
    if (!state) return EILEV_E_BADARG;
    return t5_decode_impl(d, w, tokens, enc_mask, batch, 1, 0, state, self_kv, kv_capacity, cross_kv, enc_len, logits, workspace,
                          workspace_bytes, stream);
}

// ---- the beam form as a plain C++ function for t5beam.hip (stages.h): not an entry of include/eilev.h -------------------------------------
namespace {
__global__ void t5_bump_step_kernel(int32_t *state) {
    if (threadIdx.x == 0) state[0] += 1;
}
}  // namespace
size_t t5_decode_step_beam_workspace_bytes(const EilevT5Dims *d, int64_t rows, int64_t enc_len, int64_t gen_capacity) {
    return eilev_t5_workspace_bytes(d, rows, 1, enc_len > gen_capacity + 1 ? enc_len : gen_capacity + 1);
}
int t5_decode_step_beam(const EilevT5Dims *d, const EilevT5Weights *w, const int64_t *tokens, int32_t *state, const int32_t *enc_mask,
                        int64_t rows, const T5BeamArgs &beam, const void *cross_kv, int64_t enc_len, float *logits, void *workspace,
                        size_t workspace_bytes, void *stream) {
    if (!state || !beam.kv_start) return EILEV_E_BADARG;
    RC(t5_decode_impl(d, w, tokens, enc_mask, rows, 1, 0, state, const_cast<void *>(beam.kv_start), beam.gen_capacity + 1, cross_kv, enc_len, logits,
                      workspace, workspace_bytes, stream, nullptr, nullptr, &beam));
    t5_bump_step_kernel<<<1, 64, 0, (hipStream_t)stream>>>(state);  // the step counter lives on the device: a captured step replays for every step
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}

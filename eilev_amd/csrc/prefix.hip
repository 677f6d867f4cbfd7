// prefix.hip — the C ABI of include/eilev_prefix.h (libeilev_hip_prefix.so): many rows of new positions that continue ONE cached prefix,
// stored once.  The attention kernel is this unit's own; the rest of a block is opt.hip's (stages.h) — build.py links this unit with the
// core library's objects.
//
// prefix_attn_kernel.  The rows * new_len queries are STACKED along the MFMA M dimension (stacked index s = r * new_len + t), a workgroup
// of 4 waves owns 64 of them for one head — with a small new_len (classify(): 2..8 tokens per class) a tile spans many rows.  The tile step
// and its arithmetic are attn_tile64.h's, shared with attn_prefill_kernel (head sizes 80 / 128 zero-padded to DP = 96 / 128).  Two phases
// over one running (max, sum, O):
//   1. the prefix key tiles [0, P) from the cache planes [heads][prefix_cap][hd]: every query sees every one of them — no mask beyond
//      "the key exists" (slots at or beyond P are never loaded: the tile holds zeros there and the score is dropped);
//   2. the window of stacked NEW keys that covers the tile's rows, [first row of the tile * new_len, last query of the tile], read from
//      the q|k|v rows of this call: key s' is visible to query s iff it belongs to the same row and s' <= s (row ids of the tile's keys
//      are worked out once per tile into LDS).
// No per-row cache is ever read.  Every global read is guarded by an index check; the only writes go to `out`, rows < rows * new_len.
//
// The decode entries at the end (eilev_prefix_decode_*) own no kernel: the beam form of the OPT decode step (opt.hip opt_decode_step_beam)
// with DecodeAttnArgs.shared_prompt set, whose attention is attn_decode.hip's launch_attn_decode_shared.
#include "../../include/eilev_prefix.h"
#include "attn_tile64.h"
#include "stages.h"

namespace {

struct PrefixAttnArgs {
    const bf16 *q, *kn, *vn;  // stacked rows (row strides ldq / ldk / ldv elements), head h at columns h * hd
    int64_t ldq, ldk, ldv;
    const bf16 *kp, *vp;      // prefix planes [heads][cap][hd], keys [0, P)
    bf16 *o;                  // [S][heads * hd]
    int P, cap, S, n, heads, hd;
    float scale;
};

template <int DP>
__global__ __launch_bounds__(256) void prefix_attn_kernel(const PrefixAttnArgs a) {
    using Tile = AttnTile64<DP>;
    __shared__ __attribute__((aligned(16))) char ks_[Tile::KS_BYTES];
    __shared__ __attribute__((aligned(16))) char vt_[Tile::VT_BYTES];
    __shared__ int krow_[64];  // phase 2: the row a tile's key belongs to, -1 where the tile has no key

    const int tid = threadIdx.x, wid = tid >> 6, l15 = tid & 15;
    const int h = blockIdx.y;
    const int s0 = blockIdx.x * 64;
    const int qs = s0 + wid * 16 + l15;  // this lane's stacked query
    const int qr = qs / a.n;             // ... and its row
    const float sl2 = a.scale * 1.44269504088896340736f;

    Tile t;
    t.init(qs < a.S, a.q + (int64_t)qs * a.ldq + h * a.hd, a.hd);

    // one tile of 64 keys [k0, k0 + 64) n [0, kend) of the key rows kb / vb (row strides ldk / ldv); NEW: the stacked new keys
    auto tile = [&](auto new_tag, const bf16 *kb, int64_t ldk, const bf16 *vb, int64_t ldv, int k0, int kend) {
        constexpr bool NEW = decltype(new_tag)::value;
        __syncthreads();  // everyone is done reading the previous tile
        Tile::stage(ks_, vt_, kb, ldk, vb, ldv, k0, kend, a.hd);
        if (NEW && tid < 64) krow_[tid] = k0 + tid < kend ? (k0 + tid) / a.n : -1;
        __syncthreads();
        // visibility from integers
        t.step(
            ks_, vt_, [&](int kl) { return NEW ? (krow_[kl] == qr && k0 + kl <= qs) : (k0 + kl < kend); }, [&](int, float s) { return s * sl2; },
            [](int, float p) { return p; });
    };

    // ---- phase 1: the shared prefix
    {
        const bf16 *kb = a.kp + (int64_t)h * a.cap * a.hd, *vb = a.vp + (int64_t)h * a.cap * a.hd;
        for (int k0 = 0; k0 < a.P; k0 += 64) tile(std::false_type{}, kb, a.hd, vb, a.hd, k0, a.P);
    }
    // ---- phase 2: the new keys of the rows this tile touches, up to its last query
    {
        const int w0 = (s0 / a.n) * a.n, wend = min(s0 + 64, a.S);
        for (int k0 = w0; k0 < wend; k0 += 64) tile(std::true_type{}, a.kn + h * a.hd, a.ldk, a.vn + h * a.hd, a.ldv, k0, wend);
    }

    if (qs < a.S) t.store(a.o + (int64_t)qs * a.heads * a.hd + h * a.hd, a.hd);
}

bool aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }

bool shape_ok(int64_t rows, int64_t new_len) {
    return rows > 0 && new_len > 0 && rows <= EILEV_PREFIX_MAX_ROWS && new_len <= EILEV_PREFIX_MAX_NEW && rows * new_len <= EILEV_PREFIX_MAX_STACKED;
}

int launch_prefix_attention(const PrefixAttnArgs &a, hipStream_t s) {
    const dim3 grid((unsigned)((a.S + 63) / 64), (unsigned)a.heads);
    if (a.hd == 80) hipLaunchKernelGGL(prefix_attn_kernel<96>, grid, dim3(256), 0, s, a);
    else if (a.hd == 128) hipLaunchKernelGGL(prefix_attn_kernel<128>, grid, dim3(256), 0, s, a);
    else return EILEV_E_UNSUPPORTED;
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}

// h[r * n + t] = emb[r * n + t] + pos[P + t + 2]: the prefix is one unpadded sequence, so position P + t has id P + t + 2 (hf modeling_opt.py:64-70)
__global__ __launch_bounds__(256) void prefix_pos_kernel(const bf16 *__restrict__ emb, const bf16 *__restrict__ pos, bf16 *__restrict__ h, int d, int n,
                                                         int P) {
    const int64_t i = blockIdx.x;
    const int t = (int)(i % n);
    const bf16 *e = emb + i * d, *p = pos + (int64_t)(P + t + 2) * d;
    for (int c = threadIdx.x; c < (d >> 3); c += 256) {
        float x[8], y[8];
        unpack8(*reinterpret_cast<const bf16x8 *>(e + c * 8), x);
        unpack8(*reinterpret_cast<const bf16x8 *>(p + c * 8), y);
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] += y[k];
        *reinterpret_cast<bf16x8 *>(h + i * d + c * 8) = pack8(x);
    }
}

}  // namespace

extern "C" int eilev_prefix_abi_version(void) { return EILEV_PREFIX_ABI_VERSION; }

extern "C" int eilev_prefix_attention(const void *q, int64_t ldq, const void *k_new, int64_t ldk, const void *v_new, int64_t ldv, const void *k_prefix,
                                      const void *v_prefix, int64_t prefix_len, int64_t prefix_cap, int64_t rows, int64_t new_len, int64_t heads,
                                      int64_t head_dim, float scale, void *out, void *stream) {
    if (!q || !k_new || !v_new || !k_prefix || !v_prefix || !out) return EILEV_E_BADARG;
    if (!shape_ok(rows, new_len) || heads <= 0 || heads > 1024 || head_dim <= 0 || head_dim > 1024) return EILEV_E_BADARG;
    if (prefix_len <= 0 || prefix_cap < prefix_len || prefix_cap > (1 << 20) || !(scale > 0.0f)) return EILEV_E_BADARG;
    const int64_t width = heads * head_dim;
    if (ldq < width || ldk < width || ldv < width || ldq > (1 << 24) || ldk > (1 << 24) || ldv > (1 << 24) || (ldq | ldk | ldv | head_dim) % 8) return EILEV_E_BADARG;
    if (!aligned16(q) || !aligned16(k_new) || !aligned16(v_new) || !aligned16(k_prefix) || !aligned16(v_prefix) || !aligned16(out)) return EILEV_E_BADARG;
    if (head_dim != 80 && head_dim != 128) return EILEV_E_UNSUPPORTED;
    PrefixAttnArgs a;
    a.q = (const bf16 *)q; a.kn = (const bf16 *)k_new; a.vn = (const bf16 *)v_new; a.ldq = ldq; a.ldk = ldk; a.ldv = ldv;
    a.kp = (const bf16 *)k_prefix; a.vp = (const bf16 *)v_prefix; a.o = (bf16 *)out;
    a.P = (int)prefix_len; a.cap = (int)prefix_cap; a.S = (int)(rows * new_len); a.n = (int)new_len; a.heads = (int)heads; a.hd = (int)head_dim;
    a.scale = scale;
    return launch_prefix_attention(a, (hipStream_t)stream);
}

extern "C" size_t eilev_prefix_workspace_bytes(const EilevDims *d, int64_t rows, int64_t new_len) {
    if (!d || !shape_ok(rows, new_len)) return 0;
    return carve_opt(d, rows * new_len, nullptr).used + 256;
}

// opt_blocks (opt.hip) with the attention over the shared prefix in place of launch_attention; the new K / V go to kv_rows where one is given
extern "C" int eilev_prefix_extend(const EilevDims *d, const EilevOptWeights *w, const void *inputs_embeds, int64_t rows, int64_t new_len,
                                   const void *kv_prefix, int64_t prefix_len, void *kv_rows, int64_t rows_capacity, float *logits_last,
                                   float *logits_all, void *workspace, size_t workspace_bytes, void *stream) {
    if (!d || !w || !inputs_embeds || !kv_prefix || !workspace || (!logits_last && !logits_all)) return EILEV_E_BADARG;
    if (!shape_ok(rows, new_len) || prefix_len <= 0 || prefix_len + new_len > d->max_pos) return EILEV_E_BADARG;
    if (kv_rows && (rows_capacity < new_len || rows_capacity > (1 << 20))) return EILEV_E_BADARG;
    if (!dims_ok_opt(d)) return EILEV_E_UNSUPPORTED;
    const int D = d->t_hidden, H = d->t_heads, hd = D / H;
    if (hd != 80 && hd != 128) return EILEV_E_UNSUPPORTED;
    if (workspace_bytes < eilev_prefix_workspace_bytes(d, rows, new_len)) return EILEV_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t M = rows * new_len;
    const OptBufs b = carve_opt(d, M, workspace);
    hipLaunchKernelGGL(prefix_pos_kernel, dim3((unsigned)M), dim3(256), 0, s, (const bf16 *)inputs_embeds, (const bf16 *)w->embed_positions, b.h, D,
                       (int)new_len, (int)prefix_len);
    EILEV_LAUNCH_CHECK();
    const KvCache kp(1, D, prefix_len), kr(rows, D, kv_rows ? rows_capacity : 0);
    PrefixAttnArgs a;
    a.q = b.qkv; a.kn = b.qkv + D; a.vn = b.qkv + 2 * D; a.ldq = a.ldk = a.ldv = 3 * D; a.o = b.att;
    a.P = a.cap = (int)prefix_len; a.S = (int)M; a.n = (int)new_len; a.heads = H; a.hd = hd; a.scale = 1.0f;  // (q is pre-scaled)
    for (int l = 0; l < d->t_layers; ++l) {
        const EilevOptLayer *L = &w->layers[l];
        RC(launch_layernorm(b.h, D, (const bf16 *)L->ln1_w, (const bf16 *)L->ln1_b, b.x, D, M, D, d->t_eps, s));
        RC(opt_qkv(d, w, l, b, M, s));
        if (kv_rows)
            RC(launch_kv_write(b.qkv, kr.k((bf16 *)kv_rows, l), kr.v((bf16 *)kv_rows, l), (int)rows, (int)new_len, H, hd, (int)rows_capacity, (int)new_len,
                               nullptr, s, 0));
        a.kp = kp.k((const bf16 *)kv_prefix, l); a.vp = kp.v((const bf16 *)kv_prefix, l);
        RC(launch_prefix_attention(a, s));
        RC(opt_tail(d, w, l, b, M, s));
    }
    RC(launch_layernorm(b.h, D, (const bf16 *)w->final_ln_w, (const bf16 *)w->final_ln_b, b.x, D, M, D, d->t_eps, s));
    if (logits_all) {
        GemmArgs g = mk_gemm(b.x, D, w->embed_tokens, D, nullptr, nullptr, 0, logits_all, d->vocab, M, d->vocab, D, 0);
        g.out_f32 = 1;
        RC(launch_gemm(g, 5, s));
    }
    if (logits_last) {
        // last new position of every row: a strided [rows, D] view of x
        GemmArgs g = sk_gemm(b.scratch, b.x + (new_len - 1) * (int64_t)D, new_len * (int64_t)D, w->embed_tokens, D, nullptr, nullptr, 0, logits_last,
                             d->vocab, rows, d->vocab, D, 0);
        g.out_f32 = 1;
        RC(launch_gemm(g, 5, s));
    }
    return EILEV_OK;
}

static_assert(EILEV_PREFIX_DECODE_PROMPT_KEYS == kSharedPromptKeys, "the header states the record count of a launch");
// ---- decoding with the prompt part of the attention shared among a sample's rows (common.h DecodeAttnArgs.shared_prompt) -----------------------
extern "C" int eilev_prefix_decode_attention(const void *qkv, int64_t ldq, const void *k_prompt, const void *v_prompt, int64_t seq_len,
                                             int64_t prompt_cap, const int32_t *attn_mask, const int32_t *state, void *k_gen, void *v_gen,
                                             int64_t gen_capacity, const int32_t *ancestors, int64_t rows, int64_t beams, int64_t heads, int64_t head_dim,
                                             void *out, void *part, size_t part_bytes, void *stream) {
    if (!qkv || !k_prompt || !v_prompt || !state || !k_gen || !v_gen || !ancestors || !out || !part) return EILEV_E_BADARG;
    if (rows <= 0 || beams <= 0 || rows % beams || rows > EILEV_PREFIX_DECODE_MAX_ROWS || heads <= 0 || heads > 1024 || head_dim <= 0 || head_dim > 1024 || (head_dim & 7)) return EILEV_E_BADARG;
    if (seq_len <= 0 || prompt_cap < seq_len || prompt_cap > (1 << 20) || gen_capacity <= 0 || gen_capacity > (1 << 20)) return EILEV_E_BADARG;
    if (ldq < 3 * heads * head_dim || ldq > (1 << 24) || (ldq & 7)) return EILEV_E_BADARG;
    if (!aligned16(qkv) || !aligned16(k_prompt) || !aligned16(v_prompt) || !aligned16(k_gen) || !aligned16(v_gen) || !aligned16(out) || !aligned16(part))
        return EILEV_E_BADARG;
    if (head_dim != 80 && head_dim != 128) return EILEV_E_UNSUPPORTED;
    DecodeAttnArgs a;
    a.qkv = (const bf16 *)qkv; a.ldq = ldq; a.kc = (const bf16 *)k_prompt; a.vc = (const bf16 *)v_prompt; a.out = (bf16 *)out;
    a.attn_mask = attn_mask; a.state = state; a.batch = (int)rows; a.seq_len = (int)seq_len; a.cap = (int)prompt_cap; a.heads = (int)heads; a.hd = (int)head_dim;
    a.part = (float *)part; a.part_bytes = part_bytes; a.fuse_new = 1;
    a.kg = (bf16 *)k_gen; a.vg = (bf16 *)v_gen; a.anc = ancestors; a.beams = (int)beams; a.cap_g = (int)gen_capacity;
    a.shared_prompt = 1;
    return launch_attn_decode(a, (hipStream_t)stream);
}

extern "C" size_t eilev_prefix_decode_workspace_bytes(const EilevDims *d, int64_t rows, int64_t seq_len, int64_t gen_capacity) {
    if (!d || (d->t_heads > 0 && d->t_hidden / d->t_heads != 80 && d->t_hidden / d->t_heads != 128)) return 0;
    return opt_decode_step_beam_shared_bytes(d, rows, seq_len, gen_capacity);
}

extern "C" int eilev_prefix_decode_step(const EilevDims *d, const EilevOptWeights *w, const int64_t *tokens, int32_t *state, const int32_t *attn_mask,
                                        const int32_t *n_valid, int64_t rows, int64_t beams, int64_t seq_len, const void *kv_prompt, void *kv_gen,
                                        int64_t gen_capacity, const int32_t *ancestors, float *logits, void *workspace, size_t workspace_bytes,
                                        void *stream) {
    return opt_decode_step_beam(d, w, tokens, state, attn_mask, n_valid, rows, beams, seq_len, kv_prompt, kv_gen, gen_capacity, ancestors, logits, workspace,
                                workspace_bytes, stream, 1);
}

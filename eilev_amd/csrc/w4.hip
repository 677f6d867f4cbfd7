// w4.hip — the C ABI of include/eilev_w4.h (libeilev_hip_w4.so): the M <= 32 linear over int4 weights with one bf16 scale per group of 128
// (the format and the matrix W' it MEANS are stated in the header), the expansion of the format into that bf16 matrix, and the OPT decode
// step whose four linears per block run on it.  Embedding, LayerNorm, attention, lm_head and selection are the core library's — build.py
// links this unit with the core library's objects.
//
// w4_skinny_kernel.  gemm_skinny_w8_kernel's shape for nibbles: grid (16-row weight blocks, K splits), four waves own consecutive runs of
// 256-wide K tiles.  A tile is 16 rows x 128 bytes = 2 KB, two LDS-DMA instructions of 64 x 16 bytes: piece i = rows 8 i .. 8 i + 7, lane p ->
// row 8 i + p / 8, LDS slot p % 8 <- the row's 16-byte chunk (p % 8) ^ (row & 7), so that the ds_read_b32 of an MFMA step (16 rows 128 bytes
// apart, four words of one chunk) touches every bank once.  A tile is half the bytes of the fp8 kernel's, so there is no ring: ALL of a
// wave's tiles (at most three, w4_plan) are requested before the first is used — with the activation fragments and the scales, which are
// requested first (loads return in order) and only converted after the first counted wait.  6 KB of weights per wave, 24 KB per workgroup in
// flight.  Registers bound the occupancy (the three-tile path holds 24 MB activation fragments): 140 VGPRs at MB = 1, 244 at MB = 2 as
// compiled, i.e. 3 / 2 waves per SIMD = 3 / 2 workgroups per CU (LDS alone would allow 5).
// Word d of a row holds weights 8 j .. 8 j + 7 with the even ones in the low half-word: (d >> 4 i) & 0x000f000f | 0x43004300 is the bf16
// pair (128 + u, 128 + u'), widened by a shift / a mask, minus 136, times the scale (both exact), one v_cvt_pk_bf16_f32: the bits of W'.
// Every global read is clamped to the matrix (rows past N read row N - 1, activation rows past M read row 0); stores are behind
// row < M && col < N.
#include "../../include/eilev_w4.h"
#include "stages.h"

#include <type_traits>

namespace {

constexpr int W4_TW = EILEV_W4_WAVE_TILES;
typedef __attribute__((ext_vector_type(4))) uint32_t w4_u32x4;
typedef __attribute__((address_space(3))) void w4_lds_void;
typedef __attribute__((address_space(1))) void w4_glb_void;

// the eight weights of word d, scale s: the bf16 bits of W' in MFMA fragment order (k = 8 j .. 8 j + 7)
__device__ __forceinline__ bf16x8 w4_dequant8(uint32_t d, float s) {
    w4_u32x4 o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t t = ((d >> (4 * i)) & 0x000f000fu) | 0x43004300u;  // bf16 (128 + u_even, 128 + u_odd)
        const float lo = (__uint_as_float(t << 16) - 136.0f) * s, hi = (__uint_as_float(t & 0xffff0000u) - 136.0f) * s;  // q s: exact
        const bf16x2 p = {(bf16)lo, (bf16)hi};  // the one rounding
        o[i] = __builtin_bit_cast(uint32_t, p);
    }
    return __builtin_bit_cast(bf16x8, o);
}

// ---- eilev_w4_expand: one word (8 weights, 16 output bytes) per thread ---------------------------------------------------------------------
__global__ __launch_bounds__(256) void w4_expand_kernel(const uint32_t *__restrict__ w4, const uint16_t *__restrict__ scales, bf16 *__restrict__ out,
                                                        int64_t words, int words_per_row) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= words) return;
    const int64_t n = i / words_per_row;
    const int j = (int)(i - n * words_per_row);
    const float s = __uint_as_float((uint32_t)scales[n * (words_per_row >> 4) + (j >> 4)] << 16);
    *reinterpret_cast<bf16x8 *>(out + i * 8) = w4_dequant8(w4[i], s);
}

// ---- the linear ---------------------------------------------------------------------------------------------------------------------------
struct W4Args {
    const bf16 *A;
    int64_t lda;
    const uint32_t *W4;
    const uint16_t *S;
    const bf16 *bias, *resid;
    int64_t ldr;
    void *C;
    int64_t ldc;
    int M, N, K, relu, out_f32;
    float scale;
    int scale_cols;
    float *part;  // [ks][16 MB][N]
    int ks;
};

__device__ __forceinline__ void w4_epilogue(const W4Args &a, int row, int col, float v) {
    if (a.bias) v += (float)a.bias[col];
    if (col < a.scale_cols) v *= a.scale;
    if (a.relu) v = fmaxf(v, 0.0f);
    if (a.resid) v += (float)a.resid[(int64_t)row * a.ldr + col];
    if (a.out_f32) reinterpret_cast<float *>(a.C)[(int64_t)row * a.ldc + col] = v;
    else reinterpret_cast<bf16 *>(a.C)[(int64_t)row * a.ldc + col] = (bf16)v;
}

template <int MB>
__global__ __launch_bounds__(256) void w4_skinny_kernel(const W4Args a) {
    __shared__ __attribute__((aligned(16))) char wbuf[4][W4_TW][2048];
    __shared__ float red[4][MB][64][4];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lg = lane >> 4;
    const int n0 = blockIdx.x * 16;
    // K range of this workgroup / wave in tiles of 256 (w4_plan: at most W4_TW per wave)
    const int ktiles = a.K / 256;
    const int per_wg = (ktiles + a.ks - 1) / a.ks;
    const int wg_beg = blockIdx.y * per_wg, wg_end = min(ktiles, wg_beg + per_wg);
    const int per_w = (max(wg_end - wg_beg, 0) + 3) / 4;
    const int beg = wg_beg + wid * per_w, end = min(wg_end, beg + per_w);
    const int nt = min(max(end - beg, 0), W4_TW);

    const int row_bytes = a.K >> 1;
    const char *src[2];  // DMA piece i: rows 8 i + lane / 8, LDS slot lane % 8 <- chunk slot ^ (row & 7)
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = 8 * i + (lane >> 3);
        int gr = n0 + row;
        gr = gr < a.N ? gr : a.N - 1;
        src[i] = reinterpret_cast<const char *>(a.W4) + (int64_t)gr * row_bytes + (((lane & 7) ^ (row & 7)) << 4);
    }
    const bf16 *ap[MB];  // rows past M read row 0: an output row depends on its own activation row only, and those are never stored
    f32x4 acc[MB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
        const int r = mb * 16 + l15;
        ap[mb] = a.A + (int64_t)(r < a.M ? r : 0) * a.lda + lg * 8 + beg * 256;
        acc[mb] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
    int wrow = n0 + l15;
    wrow = wrow < a.N ? wrow : a.N - 1;
    const uint32_t *sp = reinterpret_cast<const uint32_t *>(a.S + (int64_t)wrow * (a.K >> 7)) + beg;
    // One static instance per tile count of the wave: every request of a path is unconditional, so the fragments and scales cost no wait of
    // their own.  (hipcc still puts a vmcnt(0) in front of the first ds_read — it cannot tell which LDS-DMA a read depends on — so a wave
    // computes once all its tiles have landed and the counted waits below are upper bounds; the overlap comes from the other waves of the CU.)
    auto run = [&](auto nt_c) {
        constexpr int NT = decltype(nt_c)::value;
        // requests, oldest first: the activation fragments, the scales of the lane's weight row (one word = the two groups of a tile), the tiles
        bf16x8 av[MB][NT * 8];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int u = 0; u < NT * 8; ++u) av[mb][u] = *reinterpret_cast<const bf16x8 *>(ap[mb] + u * 32);
        uint32_t sc[NT];
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) sc[tt] = sp[tt];
#pragma unroll
        for (int tt = 0; tt < NT; ++tt)
#pragma unroll
            for (int i = 0; i < 2; ++i)
                __builtin_amdgcn_global_load_lds((w4_glb_void *)(src[i] + (beg + tt) * 128), (w4_lds_void *)(&wbuf[wid][tt][i * 1024]), 16, 0, 0);
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
            // tile tt has landed when at most the 2 pieces of each younger tile are outstanding (and everything requested before the tiles)
            if (NT - 1 - tt == 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else if (NT - 1 - tt == 1) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            const float s_lo = __uint_as_float(sc[tt] << 16), s_hi = __uint_as_float(sc[tt] & 0xffff0000u);
            const char *wb = &wbuf[wid][tt][0] + l15 * 128 + lg * 4;
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const uint32_t d = *reinterpret_cast<const uint32_t *>(wb + ((u ^ (l15 & 7)) << 4));
                const bf16x8 wv = w4_dequant8(d, u < 4 ? s_lo : s_hi);
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) acc[mb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[mb][tt * 8 + u], wv, acc[mb], 0, 0, 0);
            }
        }
    };
    static_assert(W4_TW == 3, "one instance per tile count");
    if (nt == 3) run(std::integral_constant<int, 3>{});
    else if (nt == 2) run(std::integral_constant<int, 2>{});
    else if (nt == 1) run(std::integral_constant<int, 1>{});
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int r = 0; r < 4; ++r) red[wid][mb][lane][r] = acc[mb][r];
    __syncthreads();
    if (wid < MB) {  // wave mb finishes row tile mb: the four K-quarter partials in a fixed order
        const int col = n0 + l15;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float v = 0.0f;
#pragma unroll
            for (int w = 0; w < 4; ++w) v += red[w][wid][lane][r];
            const int row = wid * 16 + lg * 4 + r;
            if (row < a.M && col < a.N) {
                if (a.ks == 1) w4_epilogue(a, row, col, v);
                else a.part[((int64_t)blockIdx.y * (16 * MB) + row) * a.N + col] = v;
            }
        }
    }
}

// the split-K partials summed in split order, then the epilogue (the form without LayerNorm rows; with them: launch_reduce_ln of norm.hip)
__global__ __launch_bounds__(256) void w4_reduce_kernel(const W4Args a, int mr) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.M * a.N) return;
    const int row = idx / a.N, col = idx - row * a.N;
    float v = 0.0f;
    for (int s = 0; s < a.ks; ++s) v += a.part[((int64_t)s * mr + row) * a.N + col];
    w4_epilogue(a, row, col, v);
}

struct W4Plan {
    int mb, ks, nb, per_wave;
};

// The form of an (m, n, k) linear, a function of the shape alone.  K splits: >= 512 workgroups where the matrix has fewer than 384 16-row
// blocks (gemm.hip launch_skinny's rule for the byte-streaming kernels), every wave at least one tile; then as many more as keep a wave
// at W4_TW tiles.
int w4_plan(int64_t m, int64_t n, int64_t k, W4Plan &p) {
    if (m < 1 || m > EILEV_W4_MAX_ROWS || n < 1 || k < 1) return EILEV_E_BADARG;
    if (k % EILEV_W4_KTILE || k > (1 << 20) || n > (1 << 24)) return EILEV_E_UNSUPPORTED;
    const int nb = (int)((n + 15) / 16), ktiles = (int)(k / 256);
    int ks = nb >= 384 ? 1 : (512 + nb - 1) / nb;
    if (ks > ktiles / 4) ks = ktiles / 4 > 0 ? ktiles / 4 : 1;
    const int need = (ktiles + 4 * W4_TW - 1) / (4 * W4_TW);
    if (ks < need) ks = need;
    p.mb = m <= 16 ? 1 : 2;
    p.ks = ks;
    p.nb = nb;
    p.per_wave = ((ktiles + ks - 1) / ks + 3) / 4;
    return EILEV_OK;
}

bool aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }

size_t w4_scratch_bytes(const W4Plan &p, int64_t n) { return p.ks > 1 ? (size_t)p.ks * 16 * p.mb * (size_t)n * sizeof(float) : 0; }

int w4_linear(const EilevW4Linear &l, hipStream_t s) {
    if (!l.a || !l.w.w4 || !l.w.scales || !l.c) return EILEV_E_BADARG;
    W4Plan p;
    RC(w4_plan(l.m, l.n, l.k, p));
    if (l.lda < l.k || (l.lda & 7) || l.ldc < l.n || (l.resid && l.ldr < l.n) || l.lda > (1 << 24) || l.ldc > (1 << 24) || l.ldr > (1 << 24)) return EILEV_E_BADARG;
    if (!aligned16(l.a) || !aligned16(l.w.w4) || !aligned16(l.w.scales) || (((uintptr_t)l.c) & (l.out_f32 ? 3 : 1)) || (((uintptr_t)l.bias) & 1) ||
        (((uintptr_t)l.resid) & 1))
        return EILEV_E_BADARG;
    if (l.scale_cols < 0 || l.scale_cols > l.n) return EILEV_E_BADARG;
    const bool ln = l.ln_out != nullptr;
    if (ln && (!l.ln_gamma || !l.ln_beta)) return EILEV_E_BADARG;
    if (ln && (l.out_f32 || (l.n & 7) || l.n > 4096 || !aligned16(l.ln_out) || !aligned16(l.ln_gamma) || !aligned16(l.ln_beta) || !aligned16(l.c) ||
               (l.ldc & 7)))
        return EILEV_E_UNSUPPORTED;
    const size_t need = w4_scratch_bytes(p, l.n);
    if (need && (!l.scratch || l.scratch_bytes < need || (((uintptr_t)l.scratch) & 15))) return EILEV_E_WORKSPACE;
    W4Args a;
    a.A = (const bf16 *)l.a; a.lda = l.lda; a.W4 = (const uint32_t *)l.w.w4; a.S = (const uint16_t *)l.w.scales;
    a.bias = (const bf16 *)l.bias; a.resid = (const bf16 *)l.resid; a.ldr = l.ldr; a.C = l.c; a.ldc = l.ldc;
    a.M = (int)l.m; a.N = (int)l.n; a.K = (int)l.k; a.relu = l.relu ? 1 : 0; a.out_f32 = l.out_f32 ? 1 : 0;
    a.scale = l.scale; a.scale_cols = l.scale_cols; a.part = (float *)l.scratch; a.ks = p.ks;
    const dim3 grid((unsigned)p.nb, (unsigned)p.ks);
    if (p.mb == 1) hipLaunchKernelGGL(w4_skinny_kernel<1>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(w4_skinny_kernel<2>, grid, dim3(256), 0, s, a);
    EILEV_LAUNCH_CHECK();
    const int mr = 16 * p.mb;
    if (p.ks > 1) {
        // the LayerNorm rows ride on the reduce where its 16-byte chunks apply (plain bias + residual epilogue, bf16)
        if (ln && !a.relu && a.scale_cols == 0 && (!a.bias || aligned16(a.bias)) && (!a.resid || (aligned16(a.resid) && (a.ldr & 7) == 0)))
            return launch_reduce_ln(a.part, p.ks, mr, a.M, a.N, nullptr, a.bias, a.resid, a.ldr, (bf16 *)a.C, a.ldc, (const bf16 *)l.ln_gamma,
                                    (const bf16 *)l.ln_beta, (bf16 *)l.ln_out, l.ln_eps, s);
        hipLaunchKernelGGL(w4_reduce_kernel, dim3((unsigned)((a.M * a.N + 255) / 256)), dim3(256), 0, s, a, mr);
        EILEV_LAUNCH_CHECK();
    }
    if (ln) return launch_layernorm((const bf16 *)a.C, a.ldc, (const bf16 *)l.ln_gamma, (const bf16 *)l.ln_beta, (bf16 *)l.ln_out, a.N, a.M, a.N, l.ln_eps, s);
    return EILEV_OK;
}

bool step_shape_ok(const EilevDims *d, int64_t batch) {
    return d && batch > 0 && batch <= EILEV_W4_MAX_ROWS && dims_ok_opt(d) && d->t_layers > 0 && d->t_hidden % EILEV_W4_KTILE == 0 && d->t_hidden <= 4096 &&  // (ln_out: N <= 4096)
           d->t_ffn % EILEV_W4_KTILE == 0;
}

EilevW4Linear step_linear(const OptBufs &b, const bf16 *A, int64_t K, const EilevW4Matrix &w, const void *bias, const bf16 *resid, void *C, int64_t M,
                          int64_t N, int relu) {
    EilevW4Linear l = {};
    l.a = A; l.lda = K; l.w = w; l.bias = bias; l.resid = resid; l.ldr = N; l.c = C; l.ldc = N; l.m = M; l.n = N; l.k = K; l.relu = relu;
    l.scale = 1.0f; l.scratch = b.scratch; l.scratch_bytes = kSkinnyHalf;
    return l;
}

}  // namespace

extern "C" int eilev_w4_abi_version(void) { return EILEV_W4_ABI_VERSION; }

extern "C" int eilev_w4_expand(const void *w4, const void *scales, int64_t n, int64_t k, void *out_bf16, void *stream) {
    if (!w4 || !scales || !out_bf16 || n < 1 || k < 1) return EILEV_E_BADARG;
    if (!aligned16(w4) || !aligned16(scales) || !aligned16(out_bf16)) return EILEV_E_BADARG;
    if (k % EILEV_W4_GROUP || k > (1 << 20) || n > (1 << 24)) return EILEV_E_UNSUPPORTED;  // (whole groups; the linear needs whole tiles)
    const int64_t words = n * (k / 8), blocks = ceil_div64(words, 256);
    if (blocks > 0x7fffffffll) return EILEV_E_UNSUPPORTED;
    hipLaunchKernelGGL(w4_expand_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const uint32_t *)w4, (const uint16_t *)scales,
                       (bf16 *)out_bf16, words, (int)(k / 8));
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}

extern "C" int eilev_w4_plan(int64_t m, int64_t n, int64_t k, int32_t *form) {
    if (!form) return EILEV_E_BADARG;
    W4Plan p;
    RC(w4_plan(m, n, k, p));
    form[0] = p.mb; form[1] = p.ks; form[2] = p.nb; form[3] = p.ks; form[4] = p.per_wave;
    return EILEV_OK;
}

extern "C" size_t eilev_w4_linear_scratch_bytes(int64_t m, int64_t n, int64_t k) {
    W4Plan p;
    return w4_plan(m, n, k, p) == EILEV_OK ? w4_scratch_bytes(p, n) : 0;
}

extern "C" int eilev_w4_linear(const EilevW4Linear *l, void *stream) {
    if (!l) return EILEV_E_BADARG;
    return w4_linear(*l, (hipStream_t)stream);
}

extern "C" size_t eilev_w4_workspace_bytes(const EilevDims *d, int64_t batch) {
    if (!step_shape_ok(d, batch)) return 0;
    return carve_opt(d, batch, nullptr).used + 256;
}

// eilev_opt_decode_step (opt.hip) with the block's linears on w4_skinny_kernel at every row count; activations row-major
extern "C" int eilev_w4_decode_step(const EilevDims *d, const EilevOptWeights *w, const EilevW4Layer *layers, int64_t *tokens, int32_t *state,
                                    const int32_t *attn_mask, const int32_t *n_valid, int64_t batch, int64_t seq_len, void *kv_cache,
                                    int64_t kv_capacity, float *logits, uint8_t *finished, int64_t eos_id, int64_t pad_id, int64_t *out_tokens,
                                    int64_t max_new, void *workspace, size_t workspace_bytes, void *stream) {
    if (!d || !w || !layers || !tokens || !state || !attn_mask || !n_valid || !kv_cache || !logits || !finished || !out_tokens || !workspace)
        return EILEV_E_BADARG;
    if (batch <= 0 || batch > EILEV_W4_MAX_ROWS || seq_len <= 0 || kv_capacity > (1 << 20) || seq_len + max_new > kv_capacity + 1) return EILEV_E_BADARG;
    if (!step_shape_ok(d, batch)) return EILEV_E_UNSUPPORTED;
    if (workspace_bytes < eilev_w4_workspace_bytes(d, batch)) return EILEV_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int D = d->t_hidden, H = d->t_heads, hd = D / H, Ft = d->t_ffn;
    for (int l = 0; l < d->t_layers; ++l) {  // q | k | v is one matrix: one bias vector (or none)
        const EilevOptLayer *L = &w->layers[l];
        const void *bs[3] = {L->q_b, L->k_b, L->v_b};
        if ((L->q_b || L->k_b || L->v_b) && !(L->q_b && packed(bs, 3, D))) return EILEV_E_UNSUPPORTED;
    }
    const OptBufs b = carve_opt(d, batch, workspace);
    RC(launch_decode_embed((const bf16 *)w->embed_tokens, (const bf16 *)w->embed_positions, tokens, n_valid, state, d->vocab, d->max_pos + 1, b.h,
                           (int)batch, D, s));
    const KvCache kv(batch, D, kv_capacity);
    DecodeAttnArgs a = decode_attn_args(b.qkv, b.att, b.scratch, batch, H, hd);  // (the partials: the second half of the skinny scratch)
    a.attn_mask = attn_mask; a.state = state; a.seq_len = (int)seq_len; a.cap = (int)kv_capacity;
    a.fuse_new = 1;  // the new token's K / V go into the cache inside the attention kernel
    for (int l = 0; l < d->t_layers; ++l) {
        const EilevOptLayer *L = &w->layers[l];
        const EilevW4Layer *Q = &layers[l];
        if (l == 0) RC(launch_layernorm(b.h, D, (const bf16 *)L->ln1_w, (const bf16 *)L->ln1_b, b.x, D, batch, D, d->t_eps, s));
        EilevW4Linear g = step_linear(b, b.x, D, Q->qkv, L->q_b, nullptr, b.qkv, batch, 3 * D, 0);
        g.scale = 1.0f / sqrtf((float)hd); g.scale_cols = D;  // q pre-scaled by head_dim^-0.5 (hf modeling_opt.py:151)
        RC(w4_linear(g, s));
        a.kc = kv.k((const bf16 *)kv_cache, l); a.vc = kv.v((const bf16 *)kv_cache, l);
        RC(launch_attn_decode(a, s));
        g = step_linear(b, b.att, D, Q->o, L->o_b, b.h, b.h, batch, D, 0);
        g.ln_gamma = L->ln2_w; g.ln_beta = L->ln2_b; g.ln_out = b.x; g.ln_eps = d->t_eps;
        RC(w4_linear(g, s));
        RC(w4_linear(step_linear(b, b.x, D, Q->fc1, L->fc1_b, nullptr, b.ffn, batch, Ft, 1), s));
        // the block's output goes straight into the LayerNorm that reads it next (the next block's, or final_layer_norm): b.x
        const bool last = l + 1 == d->t_layers;
        g = step_linear(b, b.ffn, Ft, Q->fc2, L->fc2_b, b.h, b.h, batch, D, 0);
        g.ln_gamma = last ? w->final_ln_w : w->layers[l + 1].ln1_w; g.ln_beta = last ? w->final_ln_b : w->layers[l + 1].ln1_b;
        g.ln_out = b.x; g.ln_eps = d->t_eps;
        RC(w4_linear(g, s));
    }
    GemmArgs g = sk_gemm(b.scratch, b.x, D, w->embed_tokens, D, nullptr, nullptr, 0, logits, d->vocab, batch, d->vocab, D, 0);
    g.out_f32 = 1;
    if (w->lm_head_stream && batch > 16 && batch <= 32) g.Wp = (const bf16 *)w->lm_head_stream;
    RC(launch_gemm(g, 5, s));
    return launch_select(logits, (int)batch, d->vocab, state, finished, eos_id, pad_id, tokens, out_tokens, max_new, s);
}

// blocks.hip — housekeeping (the event profiler, ABI version, backend name) and the building-block entry points of include/eilev.h that
// unit parity tests and probes call: single linears, LayerNorm, attention.
#include <vector>

#include "stages.h"

// ---- kernel profiler --------------------------------------------------------------------------------
namespace {
struct ProfRec {
    hipEvent_t a, b;
    int kind;
    double flops;
};
std::vector<ProfRec> g_recs;
size_t g_used = 0;
bool g_prof_on = false;
constexpr size_t kMaxRecs = 65536;
}  // namespace

void prof_begin(int kind, double flops, hipStream_t s) {
    if (!g_prof_on || g_used >= kMaxRecs) return;
    if (g_used == g_recs.size()) {
        ProfRec r;
        if (hipEventCreate(&r.a) != hipSuccess || hipEventCreate(&r.b) != hipSuccess) return;
        g_recs.push_back(r);
    }
    g_recs[g_used].kind = kind;
    g_recs[g_used].flops = flops;
    (void)hipEventRecord(g_recs[g_used].a, s);
}
void prof_end(hipStream_t s) {
    if (!g_prof_on || g_used >= kMaxRecs || g_used >= g_recs.size()) return;
    (void)hipEventRecord(g_recs[g_used].b, s);
    ++g_used;
}

extern "C" int eilev_prof_enable(int on) {
    g_prof_on = on != 0;
    g_used = 0;
    return 0;
}
extern "C" int eilev_prof_collect(int kind, int64_t *launches, double *total_ms, double *total_flops) {
    int64_t n = 0;
    double ms = 0.0, fl = 0.0;
    for (size_t i = 0; i < g_used; ++i) {
        if (kind != 0 && g_recs[i].kind != kind) continue;
        if (hipEventSynchronize(g_recs[i].b) != hipSuccess) continue;
        float t = 0.0f;
        if (hipEventElapsedTime(&t, g_recs[i].a, g_recs[i].b) != hipSuccess) continue;
        ms += t;
        fl += g_recs[i].flops;
        ++n;
    }
    if (launches) *launches = n;
    if (total_ms) *total_ms = ms;
    if (total_flops) *total_flops = fl;
    return 0;
}

extern "C" int eilev_abi_version(void) { return EILEV_ABI_VERSION; }
extern "C" const char *eilev_backend(void) { return "hip-gfx950"; }

// =====================================================================================================
// Building blocks (unit parity tests, roofline probe)
// =====================================================================================================
namespace {
// eilev_attention_probs: one wave per (batch, head, query row); a lane owns keys lane, lane + 64, ... (up to 64 per lane = 4096 keys)
__global__ void __launch_bounds__(256) attn_probs_masked_kernel(const bf16 *__restrict__ q, const bf16 *__restrict__ k, bf16 *__restrict__ probs, int heads,
                                                                int sq, int skv, int hd, int64_t ldq, int64_t ldk, float scale, int causal,
                                                                const int32_t *__restrict__ key_mask, const float *__restrict__ rel_tab, int64_t rel_stride,
                                                                int rel_off, int rel_n) {
    const int bh = blockIdx.x, b = bh / heads, h = bh % heads;
    const int i = blockIdx.y * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= sq) return;
    const bf16 *qr = q + ((int64_t)b * sq + i) * ldq + h * hd;
    bf16 *out = probs + (((int64_t)b * heads + h) * sq + i) * skv;
    const int nt = (skv + 63) / 64;
    float mx = -INFINITY;
    // two passes over the keys (scores recomputed): no per-lane array of 64 scores
    for (int pass = 0; pass < 2; ++pass) {
        float sum = 0.0f;
        float keep_mx = mx;
        for (int t = 0; t < nt; ++t) {
            const int j = lane + 64 * t;
            float s = -INFINITY;
            if (j < skv && (!causal || j <= i + (skv - sq)) && (!key_mask || key_mask[(int64_t)b * skv + j] != 0)) {
                const bf16 *kr = k + ((int64_t)b * skv + j) * ldk + h * hd;
                s = 0.0f;
                for (int e = 0; e < hd; e += 8) {
                    const bf16x8 qa = *reinterpret_cast<const bf16x8 *>(qr + e), ka = *reinterpret_cast<const bf16x8 *>(kr + e);
#pragma unroll
                    for (int u = 0; u < 8; ++u) s = fmaf((float)qa[u], (float)ka[u], s);
                }
                s *= scale;
                if (rel_tab) s += rel_tab[(int64_t)h * rel_stride + min(max(j - i - (skv - sq) + rel_off, 0), rel_n - 1)];
            }
            if (pass == 0) mx = fmaxf(mx, s);
            else sum += s == -INFINITY ? 0.0f : __expf(s - keep_mx);
        }
        if (pass == 0) {
            mx = wave_max(mx);
            continue;
        }
        sum = wave_sum(sum);
        for (int t = 0; t < nt; ++t) {  // third walk: write (scores recomputed once more: this is the debug path)
            const int j = lane + 64 * t;
            if (j >= skv) continue;
            float p = 0.0f;
            if ((!causal || j <= i + (skv - sq)) && (!key_mask || key_mask[(int64_t)b * skv + j] != 0)) {
                const bf16 *kr = k + ((int64_t)b * skv + j) * ldk + h * hd;
                float s = 0.0f;
                for (int e = 0; e < hd; e += 8) {
                    const bf16x8 qa = *reinterpret_cast<const bf16x8 *>(qr + e), ka = *reinterpret_cast<const bf16x8 *>(kr + e);
#pragma unroll
                    for (int u = 0; u < 8; ++u) s = fmaf((float)qa[u], (float)ka[u], s);
                }
                s *= scale;
                if (rel_tab) s += rel_tab[(int64_t)h * rel_stride + min(max(j - i - (skv - sq) + rel_off, 0), rel_n - 1)];
                p = sum > 0.0f ? __expf(s - keep_mx) / sum : 0.0f;
            }
            out[j] = (bf16)p;
        }
    }
}
}  // namespace

extern "C" int eilev_attention_probs(const void *q, const void *k, void *probs, int64_t batch, int64_t heads, int64_t sq, int64_t skv, int64_t head_dim,
                                     int64_t ldq, int64_t ldk, float scale, int causal, const int32_t *key_mask, const float *rel_tab,
                                     int64_t rel_stride, int64_t rel_off, int64_t rel_n, void *stream) {
    if (!q || !k || !probs || batch < 0 || heads <= 0 || sq < 0 || skv <= 0 || skv > 4096) return EILEV_E_BADARG;
    if (rel_tab && (rel_n <= 0 || rel_stride < rel_n)) return EILEV_E_BADARG;
    if ((head_dim & 7) || (ldq & 7) || (ldk & 7) || ((uintptr_t)q & 15) || ((uintptr_t)k & 15)) return EILEV_E_UNSUPPORTED;
    if (batch == 0 || sq == 0) return EILEV_OK;
    attn_probs_masked_kernel<<<dim3((unsigned)(batch * heads), (unsigned)((sq + 3) / 4)), 256, 0, (hipStream_t)stream>>>(
        (const bf16 *)q, (const bf16 *)k, (bf16 *)probs, (int)heads, (int)sq, (int)skv, (int)head_dim, ldq, ldk, scale, causal, key_mask, rel_tab, rel_stride,
        (int)rel_off, (int)rel_n);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}

extern "C" int eilev_linear(const void *a, const void *w, const void *bias, const void *residual, void *c, int64_t m,
                            int64_t n, int64_t k, int epilogue, int out_f32, void *stream) {
    if (!a || !w || !c || m < 0 || n <= 0 || k <= 0 || m > 0x7fffffff || n > 0x7fffffff) return EILEV_E_BADARG;
    GemmArgs g = mk_gemm((const bf16 *)a, k, w, k, bias, (const bf16 *)residual, n, c, n, m, (int)n, (int)k, epilogue);
    g.out_f32 = out_f32;
    return launch_gemm(g, 5, (hipStream_t)stream);
}

extern "C" size_t eilev_linear_w8_scratch_bytes(int64_t m, int64_t n, int64_t k) {
    const size_t expand = m > 32 || k % 256 != 0 ? (size_t)n * k * sizeof(bf16) : 0;       // large M: weights expanded to bf16
    const size_t partials = m <= 32 ? (size_t)64 * 32 * n * sizeof(float) : 0;             // small M: split-K partial sums
    return expand > partials ? expand : partials;
}

extern "C" int eilev_linear_w8(const void *a, const uint8_t *w8, const float *w_scale, const void *bias, const void *residual, void *c,
                               int64_t m, int64_t n, int64_t k, int epilogue, int out_f32, void *scratch, size_t scratch_bytes, void *stream) {
    if (!a || !w8 || !w_scale || !c || m < 0 || n <= 0 || k <= 0 || m > 0x7fffffff || n > 0x7fffffff) return EILEV_E_BADARG;
    GemmArgs g = mk_gemm((const bf16 *)a, k, nullptr, k, bias, (const bf16 *)residual, n, c, n, m, (int)n, (int)k, epilogue);
    g.out_f32 = out_f32;
    g.W8 = w8;
    g.wscale = w_scale;
    if (m > 32 || k % 256 != 0) {
        if (!scratch || scratch_bytes < (size_t)n * k * sizeof(bf16)) return EILEV_E_WORKSPACE;
        g.w8_scratch = (bf16 *)scratch;
    } else if (scratch) {
        g.scratch = (float *)scratch;
        g.scratch_bytes = scratch_bytes;
    }
    return launch_gemm(g, 5, (hipStream_t)stream);
}

// LayerNorm folded into the consuming linear: the stages the folded ViT blocks are made of (include/eilev.h, ABI version 9)
extern "C" int eilev_fold_layernorm(const void *w, const void *gamma, const void *beta, const void *bias, int64_t n, int64_t k, void *w_out,
                                    float *csum, void *bias_out, void *stream) {
    if (n > 0x7fffffff || k > 0x7fffffff) return EILEV_E_BADARG;
    return launch_fold_layernorm((const bf16 *)w, (const bf16 *)gamma, (const bf16 *)beta, (const bf16 *)bias, (int)n, (int)k, (bf16 *)w_out,
                                 csum, (bf16 *)bias_out, (hipStream_t)stream);
}

extern "C" int eilev_linear_stats(const void *a, const void *w, const void *bias, const void *residual, void *c, int64_t m, int64_t n,
                                  int64_t k, float *stats, void *stream) {
    if (!a || !w || !c || !residual || !stats || m < 0 || n <= 0 || k <= 0 || m > 0x7fffffff || n > 0x7fffffff) return EILEV_E_BADARG;
    GemmArgs g = mk_gemm((const bf16 *)a, k, w, k, bias, (const bf16 *)residual, n, c, n, m, (int)n, (int)k, 0);
    g.stat_out = stats;
    g.stat_ld = m;
    return launch_gemm(g, 5, (hipStream_t)stream);
}

extern "C" int eilev_ln_finalize(const float *stats, int64_t m, int64_t n, float eps, float *ln_rows, void *stream) {
    if (n > 0x7fffffff) return EILEV_E_BADARG;
    return launch_ln_finalize(stats, (int)((n + 63) / 64), m, (int)n, eps, ln_rows, (hipStream_t)stream);
}

extern "C" int eilev_linear_lnfold(const void *a, const void *w_f, const void *bias_f, const float *csum, const float *ln_rows, void *c,
                                   int64_t m, int64_t n, int64_t k, int epilogue, void *stream) {
    if (!a || !w_f || !csum || !ln_rows || !c || m < 0 || n <= 0 || k <= 0 || m > 0x7fffffff || n > 0x7fffffff) return EILEV_E_BADARG;
    if (epilogue != 0 && epilogue != 1) return EILEV_E_UNSUPPORTED;
    GemmArgs g = mk_gemm((const bf16 *)a, k, w_f, k, bias_f, nullptr, 0, c, n, m, (int)n, (int)k, epilogue);
    g.ln_rows = ln_rows;
    g.ln_csum = csum;
    return launch_gemm(g, 5, (hipStream_t)stream);
}

extern "C" int eilev_quant_rows_e4m3(const void *x, uint8_t *q, float *scale, int64_t rows, int64_t cols, void *stream) {
    if (!x || !q || !scale || rows < 0 || cols <= 0 || cols > 0x7fffffff) return EILEV_E_BADARG;
    return launch_quant_rows_e4m3((const bf16 *)x, cols, q, scale, rows, (int)cols, (hipStream_t)stream);
}

extern "C" int eilev_linear_a8w8(const uint8_t *a8, const float *a_scale, const uint8_t *w8, const float *w_scale, const void *bias,
                                 const void *residual, void *c, int64_t m, int64_t n, int64_t k, int epilogue, int out_f32, void *stream) {
    if (!a8 || !a_scale || !w8 || !w_scale || !c || m < 0 || n <= 0 || k <= 0 || m > 0x7fffffff || n > 0x7fffffff) return EILEV_E_BADARG;
    if (epilogue != 0 && epilogue != 2) return EILEV_E_UNSUPPORTED;
    GemmArgs g = mk_gemm(nullptr, k, nullptr, k, bias, (const bf16 *)residual, n, c, n, m, (int)n, (int)k, epilogue);
    g.out_f32 = out_f32;
    g.A8 = a8; g.ascale = a_scale; g.W8 = w8; g.wscale = w_scale;
    return launch_gemm(g, 5, (hipStream_t)stream);
}

extern "C" int eilev_linear_rows(const void *x, const void *ln_gamma, const void *ln_beta, float eps, const void *w, const void *bias,
                                 const void *residual, void *c, int64_t m, int64_t n, int64_t k, int epilogue, int out_f32, void *stream) {
    if (!x || !w || !c || m <= 0 || n <= 0 || k <= 0 || n > 0x7fffffff || k > 0x7fffffff || (ln_gamma != nullptr) != (ln_beta != nullptr)) return EILEV_E_BADARG;
    if (m > 8 || !gemv_rows_ok((int)m, (int)n, (int)k) || (epilogue != 0 && epilogue != 2)) return EILEV_E_UNSUPPORTED;
    if (m == 1 && g_decode_rows != 3 && gemv1_ok((int)n, (int)k, ln_gamma ? 1 : 0) && !(((uintptr_t)bias | (uintptr_t)residual) & 3) && !(n & 1))  // round 4: one row (bias / residual are fetched as 32-bit pairs: even n only)
        return launch_gemv1(ln_gamma ? 1 : 0, (const bf16 *)x, (const bf16 *)ln_gamma, (const bf16 *)ln_beta, eps, (const bf16 *)w, (const bf16 *)bias,
                            (const bf16 *)residual, c, out_f32, (int)n, (int)k, epilogue, 1.0f, 0, (hipStream_t)stream);
    if (m >= 2 && g_decode_rows != 3 && gemvm_ok((int)m, (int)n, (int)k, ln_gamma ? 1 : 0) && !(((uintptr_t)bias | (uintptr_t)residual) & 3) && !(n & 1))
        return launch_gemvm(ln_gamma ? 1 : 0, (const bf16 *)x, k, (const bf16 *)ln_gamma, (const bf16 *)ln_beta, eps, (const bf16 *)w, (const bf16 *)bias,
                            (const bf16 *)residual, n, c, n, out_f32, (int)m, (int)n, (int)k, epilogue, 1.0f, 0, (hipStream_t)stream);
    return launch_gemv_rows(ln_gamma ? 1 : 0, (const bf16 *)x, k, (const bf16 *)ln_gamma, (const bf16 *)ln_beta, eps, nullptr, 0, 0, 0, (const bf16 *)w,
                            (const bf16 *)bias, (const bf16 *)residual, n, c, n, out_f32, (int)m, (int)n, (int)k, epilogue, 1.0f, 0, (hipStream_t)stream);
}

extern "C" int eilev_layernorm(const void *x, const void *gamma, const void *beta, void *y, int64_t rows, int64_t cols,
                               float eps, void *stream) {
    return launch_layernorm((const bf16 *)x, cols, (const bf16 *)gamma, (const bf16 *)beta, (bf16 *)y, cols, rows, (int)cols,
                            eps, (hipStream_t)stream);
}

extern "C" int eilev_attention(const void *q, const void *k, const void *v, void *o, int64_t batch, int64_t heads, int64_t sq,
                               int64_t skv, int64_t head_dim, int64_t ldq, int64_t ldk, int64_t ldv, float scale, int causal,
                               const int32_t *key_mask, void *stream) {
    AttnArgs a = attn_rows((const bf16 *)q, ldq, (const bf16 *)k, ldk, (const bf16 *)v, ldv, (bf16 *)o, batch, heads, sq, skv, head_dim, scale);
    a.causal = causal; a.key_mask = key_mask; a.mask_ld = skv;
    return launch_attention(a, (hipStream_t)stream);
}

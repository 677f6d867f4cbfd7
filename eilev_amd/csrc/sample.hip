// sample.hip — multinomial sampling on the device (include/eilev_sample.h): repetition penalty, minimum length, temperature, top-k,
// top-p and the draw of one decode step, one 1024-thread workgroup per row.  Standalone library (libeilev_hip_sample.so): it links
// nothing of the core library.  The row in registers, the penalty / ban tables, the rules on the chunks and the commit of the token are
// row_select.h's, shared with rules.hip and misc.hip; this file holds the two thresholds and the draw.
//
// Both thresholds are the same question — "keep x while the weight of the elements strictly above x is below Q" (top-k: weight 1,
// Q = k; top-p: weight = probability, Q = top_p * total) — answered by one radix select over 256-bin histograms in LDS.  Probabilities are
// 40-bit fixed point summed in 64-bit integers: the sums do not depend on the order of the LDS atomics, so the result is reproducible.
#include <climits>

#include "row_select.h"
#include "../../include/eilev_sample.h"

namespace {

typedef unsigned long long u64;

static_assert(EILEV_SAMPLE_MAX_VOCAB == kMaxVocab && EILEV_SAMPLE_MAX_EOS == kMaxEos, "include/eilev_sample.h and row_select.h disagree");
constexpr float kScale = 1099511627776.0f;  // 2^40

struct SelState {
    u64 hw[256];  // weight histogram of the current level; bin 0 holds the largest values
    u64 q;        // the target Q
    u64 cum;      // weight strictly above the current bin range
    u64 total;    // weight of all finite elements (level 0)
    uint32_t kmin, kmax;
    int bin, all;
};

// order-preserving image of a float (no NaN here; -0 was folded into +0)
__device__ __forceinline__ uint32_t fkey(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float keyf(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }
__device__ __forceinline__ u64 weight(float x, float mx) { return (u64)(expf(x - mx) * kScale); }

__device__ __forceinline__ u64 wave_incl_scan(u64 v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const u64 t = __shfl_up(v, o, 64);
        if (lane >= o) v += t;
    }
    return v;
}

// Wave 0: the bin with (weight above it) < Q <= (weight above it + its own).  first: also the total and Q of the select.
__device__ __forceinline__ void scan_bins(SelState &s, int lane, bool first, bool by_mass, double frac, u64 kq) {
    const u64 q_prev = s.q, cum_prev = s.cum;
    u64 a[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) a[i] = s.hw[4 * lane + i];
    const u64 t = (a[0] + a[1]) + (a[2] + a[3]);
    const u64 inc = wave_incl_scan(t, lane);
    const u64 total = __shfl(inc, 63, 64);
    u64 q, rem;
    if (first) {
        q = kq;
        if (by_mass) {  // W_gt < top_p * total  <=>  W_gt < ceil(top_p * total) for an integer W_gt; the largest token always stays
            q = (u64)ceil(frac * (double)total);
            if (q < 1) q = 1;
        }
        rem = q;
        if (lane == 0) {
            s.total = total;
            s.q = q;
            s.all = q > total ? 1 : 0;
        }
    } else {
        rem = q_prev - cum_prev;
    }
    u64 c = inc - t;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (c < rem && rem <= c + a[i]) {  // at most one bin of one lane
            s.bin = 4 * lane + i;
            s.cum = (first ? 0 : cum_prev) + c;
        }
        c += a[i];
    }
}

// The smallest kept key: an element stays iff the weight of the elements strictly above it is < Q.  0 = everything finite stays.
template <bool MASS>
__device__ __forceinline__ uint32_t select_threshold(const float4 (&e)[kChunks], float mx, float mn, double frac, u64 kq, SelState &s, int tid) {
    // level 0: 256 bins linear in max - x (the values of a row spread over them; the integer image would put a row into a few exponent bins)
    const float c = mx > mn ? 256.0f / (mx - mn) : 0.0f;
    auto bin0 = [&](float x) { return min(255, (int)((mx - x) * c)); };
    __syncthreads();
    if (tid < 256) s.hw[tid] = 0;
    if (tid == 0) {
        s.kmin = 0xffffffffu;
        s.kmax = 0;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < kChunks; ++j) {
        const float ev[4] = {e[j].x, e[j].y, e[j].z, e[j].w};
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (ev[u] > -INFINITY) atomicAdd(&s.hw[bin0(ev[u])], MASS ? weight(ev[u], mx) : 1ull);
    }
    __syncthreads();
    if (tid < 64) scan_bins(s, tid, true, MASS, frac, kq);
    __syncthreads();
    if (s.all) return 0;
    const int b0 = s.bin;
#pragma unroll
    for (int j = 0; j < kChunks; ++j) {
        const float ev[4] = {e[j].x, e[j].y, e[j].z, e[j].w};
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (ev[u] > -INFINITY && bin0(ev[u]) == b0) {
                atomicMin(&s.kmin, fkey(ev[u]));
                atomicMax(&s.kmax, fkey(ev[u]));
            }
    }
    __syncthreads();
    uint32_t kmin = s.kmin, kmax = s.kmax;
    // further levels: 8 bits of the integer image per level within [kmin, kmax] (a bin of level 0 is a contiguous range of it)
    for (int lvl = 0; lvl < 5 && kmax != kmin; ++lvl) {
        const int sft = max(0, (32 - __clz(kmax - kmin)) - 8);
        __syncthreads();
        if (tid < 256) s.hw[tid] = 0;
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kChunks; ++j) {
            const float ev[4] = {e[j].x, e[j].y, e[j].z, e[j].w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t k = fkey(ev[u]);
                if (ev[u] > -INFINITY && k >= kmin && k <= kmax) atomicAdd(&s.hw[(kmax - k) >> sft], MASS ? weight(ev[u], mx) : 1ull);
            }
        }
        __syncthreads();
        if (tid < 64) scan_bins(s, tid, false, MASS, frac, kq);
        __syncthreads();
        const uint32_t nmax = kmax - ((uint32_t)s.bin << sft), span = (1u << sft) - 1u;
        kmin = nmax - kmin >= span ? nmax - span : kmin;
        kmax = nmax;
    }
    return kmax;
}

__device__ __forceinline__ float4 mask_below(float4 v, uint32_t thr) {
    v.x = fkey(v.x) >= thr ? v.x : -INFINITY;
    v.y = fkey(v.y) >= thr ? v.y : -INFINITY;
    v.z = fkey(v.z) >= thr ? v.z : -INFINITY;
    v.w = fkey(v.w) >= thr ? v.w : -INFINITY;
    return v;
}

__global__ __launch_bounds__(kThreads) void sample_kernel(EilevSampleParams p, const float *__restrict__ logits, int vocab, int rows,
                                                          const float *__restrict__ uniforms, int32_t *__restrict__ state,
                                                          uint8_t *__restrict__ finished, int64_t *__restrict__ tokens,
                                                          int64_t *__restrict__ out_tokens, float *__restrict__ warped, int whole_step) {
    __shared__ uint32_t pen_bits[kBits], ban_bits[kBits];
    __shared__ SelState sel;
    __shared__ float red_a[16], red_b[16];
    __shared__ u64 wtot[16][kChunks];  // [wave][chunk] weight; the draw reuses row 0 .. as 16 wave totals
    __shared__ u64 draw_base, draw_tgt;
    __shared__ int draw_chunk, draw_tok;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int n4 = vocab >> 2;
    const int64_t step = (int64_t)state[0] + p.step_offset;
    const bool step_ok = step >= 0 && step < p.max_new;

    // ---- one bit per id: the row's history (repetition penalty) and the banned EOS ids (min_new); load, steps 1 - 3
    fill_tables(p, out_tokens + (int64_t)b * p.max_new, step, 0, vocab, tid, pen_bits, ban_bits);
    float4 e[kChunks];
    load_row(e, logits + (int64_t)b * vocab, n4, tid);
    apply_rules(e, pen_bits, ban_bits, p.repetition_penalty, p.temperature, tid);

    // ---- row maximum, and minimum over the finite entries
    float mx = -INFINITY, mn = INFINITY;
#pragma unroll
    for (int j = 0; j < kChunks; ++j) {
        const float ev[4] = {e[j].x, e[j].y, e[j].z, e[j].w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            mx = fmaxf(mx, ev[u]);
            mn = ev[u] > -INFINITY ? fminf(mn, ev[u]) : mn;
        }
    }
    mx = wave_max(mx);
    mn = -wave_max(-mn);
    if (lane == 0) {
        red_a[wid] = mx;
        red_b[wid] = mn;
    }
    __syncthreads();
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        mx = fmaxf(mx, red_a[w]);
        mn = fminf(mn, red_b[w]);
    }
    const bool any_finite = mx > -INFINITY && mx < INFINITY;

    // ---- steps 4 and 5
    if (any_finite && p.top_k > 0) {
        const uint32_t thr = select_threshold<false>(e, mx, mn, 0.0, (u64)p.top_k, sel, tid);
        if (thr) {
#pragma unroll
            for (int j = 0; j < kChunks; ++j) e[j] = mask_below(e[j], thr);
            mn = keyf(thr);
        }
    }
    if (any_finite && p.top_p < 1.0f) {
        const uint32_t thr = select_threshold<true>(e, mx, mn, (double)p.top_p, 0, sel, tid);
        if (thr) {
#pragma unroll
            for (int j = 0; j < kChunks; ++j) e[j] = mask_below(e[j], thr);
        }
    }
    if (warped) store_row(e, warped + (int64_t)b * vocab, n4, tid);

    // ---- step 6: the weight of every 4096-id chunk, the chunk that holds u * total, then a scan inside that chunk
#pragma unroll
    for (int j = 0; j < kChunks; ++j) {
        u64 sj = (weight(e[j].x, mx) + weight(e[j].y, mx)) + (weight(e[j].z, mx) + weight(e[j].w, mx));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sj += __shfl_xor(sj, o, 64);
        if (lane == 0) wtot[wid][j] = sj;
    }
    if (tid == 0) {
        draw_chunk = -1;
        draw_tok = -1;
    }
    __syncthreads();
    if (tid < 64) {
        u64 t = 0;
        if (lane < kChunks)
            for (int w = 0; w < 16; ++w) t += wtot[w][lane];
        const u64 inc = wave_incl_scan(t, lane);
        const u64 total = __shfl(inc, kChunks - 1, 64);
        const float uf = step_ok ? uniforms[step * rows + b] : 0.0f;
        const u64 tgt = (u64)((double)fminf(fmaxf(uf, 0.0f), 0.99999994f) * (double)total);  // < total
        if (lane < kChunks && inc - t <= tgt && tgt < inc) {
            draw_chunk = lane;
            draw_base = inc - t;
        }
        if (lane == 0) draw_tgt = tgt;
    }
    __syncthreads();
    const int jc = any_finite ? draw_chunk : -1;
    if (jc >= 0) {  // (uniform)
        u64 w4[4] = {0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < kChunks; ++j)
            if (j == jc) {
                w4[0] = weight(e[j].x, mx);
                w4[1] = weight(e[j].y, mx);
                w4[2] = weight(e[j].z, mx);
                w4[3] = weight(e[j].w, mx);
            }
        const u64 t = (w4[0] + w4[1]) + (w4[2] + w4[3]);
        const u64 inc = wave_incl_scan(t, lane);
        if (lane == 63) wtot[0][wid] = inc;  // (every thread read wtot before the barrier above)
        __syncthreads();
        u64 c = draw_base + (inc - t);
        for (int w = 0; w < wid; ++w) c += wtot[0][w];
        const u64 tgt = draw_tgt;
        if (c <= tgt && tgt < c + t) {  // exactly one thread
            int u = 0;
            while (u < 3 && c + w4[u] <= tgt) c += w4[u++];
            draw_tok = (tid + kThreads * jc) * 4 + u;
        }
    }
    __syncthreads();
    if (tid == 0) commit_token(p, draw_tok >= 0 ? draw_tok : 0, b, step, state, finished, tokens, out_tokens, whole_step);
}

}  // namespace

extern "C" int eilev_sample_abi_version(void) { return EILEV_SAMPLE_ABI_VERSION; }

extern "C" size_t eilev_sample_scratch_bytes(int64_t rows, int64_t vocab) {
    (void)rows;
    (void)vocab;
    return 0;
}

extern "C" int eilev_sample_select(const EilevSampleParams *p, const float *logits, int64_t rows, int64_t vocab, const float *uniforms,
                                   int32_t *state, uint8_t *finished, int64_t *tokens, int64_t *out_tokens, float *warped, void *scratch,
                                   size_t scratch_bytes, void *stream) {
    (void)scratch;
    if (!p || !logits || !uniforms || !state || !finished || !tokens || !out_tokens) return EILEV_E_BADARG;
    if (rows < 1 || rows >= INT_MAX || vocab < 1 || p->max_new < 1 || p->max_new >= INT_MAX || p->n_eos < 0 || p->n_eos > EILEV_SAMPLE_MAX_EOS)
        return EILEV_E_BADARG;
    if (!(p->temperature > 0.0f) || !(p->top_p > 0.0f) || !(p->repetition_penalty > 0.0f) || p->top_k < 0 || p->step_offset < -1 ||
        p->step_offset > 0 || (p->finalize != 0 && p->finalize != 1))
        return EILEV_E_BADARG;
    if (vocab > EILEV_SAMPLE_MAX_VOCAB || (vocab & 3) || (((uintptr_t)logits) & 15) || (warped && (((uintptr_t)warped) & 15))) return EILEV_E_UNSUPPORTED;
    if (scratch_bytes < eilev_sample_scratch_bytes(rows, vocab)) return EILEV_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sample_kernel, dim3((unsigned)rows), dim3(kThreads), 0, s, *p, logits, (int)vocab, (int)rows, uniforms, state, finished, tokens,
                       out_tokens, warped, rows == 1 ? 1 : 0);
    EILEV_LAUNCH_CHECK();
    if (rows == 1) return EILEV_OK;  // (the single workgroup finished the step itself)
    hipLaunchKernelGGL(row_finalize_kernel<>, dim3(1), dim3(64), 0, s, state, (const uint8_t *)finished, (int)rows, (int)p->step_offset,
                       (int)p->finalize);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}

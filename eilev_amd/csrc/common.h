// common.h — shared device helpers for the gfx950 kernels (wave64, bf16 storage, fp32 math).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/eilev.h"

typedef __bf16 bf16;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) __bf16 bf16x4;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;

#define EILEV_HIP_CHECK(expr)                          \
    do {                                               \
        hipError_t _e = (expr);                        \
        if (_e != hipSuccess) return (int)_e;          \
    } while (0)

// CUs of the current device (cached; 256 when the query fails).  hipDeviceGetAttribute, not hipGetDeviceProperties: the property STRUCT
// differs between the HIP runtime this library was built against and the one the process mapped first (PyTorch ships its own copy), and
// a failed query must not leave its error behind for the next launch check's hipGetLastError().
static inline int eilev_num_cu() {
    static int n = 0;
    if (!n) {
        int dev = 0, cu = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cu > 0) n = cu;
        else {
            (void)hipGetLastError();
            n = 256;
        }
    }
    return n;
}

// CUs the persistent kernels (one workgroup per CU: GEMM, frame attention) size their grids for: all of them, or fewer when the caller runs
// them on a CU-masked stream next to another stream (probe switch eilev_debug_grid_cus; tools/overlap_probe.py).  Never more than the device has.
extern int g_eilev_grid_cus;
static inline int eilev_grid_cus() {
    const int n = eilev_num_cu();
    return g_eilev_grid_cus > 0 && g_eilev_grid_cus < n ? g_eilev_grid_cus : n;
}

#define EILEV_LAUNCH_CHECK()                           \
    do {                                               \
        hipError_t _e = hipGetLastError();             \
        if (_e != hipSuccess) return (int)_e;          \
    } while (0)

// Launches the kernel instance KERNEL with `smem` bytes of dynamic LDS and checks the launch.  Before the instance is first launched with
// more dynamic LDS than it was allowed so far, its hipFuncAttributeMaxDynamicSharedMemorySize is raised to the size asked for (once per
// instance where the size is fixed).  hipFuncSetAttribute enqueues no stream work: this may run inside a graph capture.
template <auto KERNEL, typename... Args>
static inline int eilev_launch(dim3 grid, dim3 block, size_t smem, hipStream_t s, const Args &...args) {
    static size_t allowed = 0;
    if (smem > allowed) {
        EILEV_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(KERNEL), hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem));
        allowed = smem;
    }
    hipLaunchKernelGGL(KERNEL, grid, block, smem, s, args...);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}

// The runtime epilogue code (GemmArgs::epi: 0 none, 1 GELU, 2 ReLU) as a template argument: returns f(std::integral_constant<int, E>{}) for
// the E of EPIS... that equals `epi`, and for the first of EPIS... when none does.  EPIS... are the instances a launcher has.
template <int E0, int... EPIS, typename F>
static inline int eilev_with_epi(int epi, F &&f) {
    int rc = 0;
    const bool hit = ((epi == EPIS && (rc = f(std::integral_constant<int, EPIS>{}), true)) || ...);
    return hit ? rc : f(std::integral_constant<int, E0>{});
}

// Counter-based dropout mask (splitmix64 finaliser): the same function in the forward and the backward kernels and in the oracle,
// so a mask is never stored.  keep iff hash >= p * 2^32.
__host__ __device__ __forceinline__ uint32_t eilev_hash32(uint32_t seed, uint64_t idx) {
    uint64_t z = idx + 0x9E3779B97F4A7C15ull * ((uint64_t)seed + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (uint32_t)(z >> 32);
}
__host__ __forceinline__ uint32_t eilev_drop_threshold(float p) {
    const double t = (double)p * 4294967296.0;
    return t >= 4294967295.0 ? 4294967295u : (uint32_t)t;
}

__device__ __forceinline__ float bf2f(bf16 x) { return (float)x; }
__device__ __forceinline__ bf16 f2bf(float x) { return (bf16)x; }

// 16-byte vector of 8 bf16 <-> 8 floats
__device__ __forceinline__ void unpack8(const bf16x8 &v, float (&f)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = (float)v[i];
}
__device__ __forceinline__ bf16x8 pack8(const float (&f)[8]) {
    bf16x8 v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (bf16)f[i];
    return v;
}
__device__ __forceinline__ bf16x8 zero8() {
    bf16x8 v;
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = (bf16)0.0f;
    return v;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// Exact-erf GELU (hf ACT2FN["gelu"], Blip2MLP) = max(x, 0) - r(|x|) with r(u) = u * Phi(-u), a smooth bump (max 0.17 at u = 0.75).
// Two polynomial forms, no transcendental, no division, Horner in fp32:
//  * gelu_erf / gelu_erf_pk (everything but the two persistent kernels: Q-Former, training forward, small-tile launches, decode): Phi(-u) on
//    [0, 5] as a degree-12 polynomial in t = 0.4 u - 1 (weighted minimax fit): max abs error of the GELU 1.5e-6, i.e. below the bf16
//    rounding of the stored activation everywhere; r < 1.5e-6 beyond u = 5 (x < -5 returns -0.0-ish, approaching 0 like the exact form).
//  * gelu_erf_n<NP> = the FAST form of the persistent kernels' epilogues (gemm_pp4_kernel, gemm_w6_kernel: with a GELU only
//    the ViT fc1 reaches them — >= 192 tiles of 256 x 128): r itself on [0, 4] as a degree-8
//    polynomial in t = u / 2 - 1: max abs error 1.1e-4 (relative 2.2e-3 where |y| > 0.05; a constant -1.3e-4 for x < -4).  The stored
//    activation is bf16 (2^-9 relative) and the reference's own bf16 run evaluates GELU on a pre-activation that was itself rounded
//    to bf16 (an input error of 4e-3 |x|), so this is an order of magnitude inside the reference's own noise; 12 VALU operations per
//    element instead of 16: the epilogue runs with the MFMA pipe idle, the difference was worth +2.2 % on the fc1 GEMM (r2 A/B).
//    End-to-end effect on the logits: profiles/parity_r03.json `gelu_deg8_vs_deg12`.
typedef float f32x2 __attribute__((ext_vector_type(2)));
#define EILEV_GELU12_COEFFS                                                                                                 \
    {6.210111547e-03f, -4.381819814e-02f, 1.368895024e-01f, -2.397004068e-01f, 2.326955497e-01f, -6.489974260e-02f,       \
     -1.311938316e-01f, 1.613862813e-01f, -2.371504903e-02f, -7.562928647e-02f, 3.900733590e-02f, 1.263864804e-02f,        \
     -9.870870970e-03f}
__device__ __forceinline__ float gelu_erf(float x) {
    constexpr float c[13] = EILEV_GELU12_COEFFS;
    const float u = fminf(fabsf(x), 5.0f);
    const float t = fmaf(u, 0.4f, -1.0f);
    float p = c[12];
#pragma unroll
    for (int k = 11; k >= 0; --k) p = fmaf(p, t, c[k]);
    return fmaf(-u, p, fmaxf(x, 0.0f));
}
// 2 * NP elements at a time: independent Horner chains interleaved step by step (a dependent FMA waits ~4 cycles for its predecessor)
__device__ __forceinline__ float gelu_erf_n1(float x);  // (the fast form on one element: below)
template <int NP>
__device__ __forceinline__ void gelu_erf_pk(f32x2 (&x)[NP]) {
    constexpr float c[13] = EILEV_GELU12_COEFFS;
    float v[2 * NP], u[2 * NP], t[2 * NP], p[2 * NP];
#pragma unroll
    for (int n = 0; n < NP; ++n) { v[2 * n] = x[n].x; v[2 * n + 1] = x[n].y; }
#pragma unroll
    for (int n = 0; n < 2 * NP; ++n) {
        u[n] = fminf(fabsf(v[n]), 5.0f);
        t[n] = fmaf(u[n], 0.4f, -1.0f);
        p[n] = c[12];
    }
#pragma unroll
    for (int k = 11; k >= 0; --k)
#pragma unroll
        for (int n = 0; n < 2 * NP; ++n) p[n] = fmaf(p[n], t[n], c[k]);
#pragma unroll
    for (int n = 0; n < NP; ++n) x[n] = (f32x2){fmaf(-u[2 * n], p[2 * n], fmaxf(v[2 * n], 0.0f)), fmaf(-u[2 * n + 1], p[2 * n + 1], fmaxf(v[2 * n + 1], 0.0f))};
}
#define EILEV_GELU_DEG 8
#define EILEV_GELU_UMAX 4.0f
#define EILEV_GELU_COEFFS                                                                                                   \
    {4.543383146e-02f, -1.712931058e-01f, 2.188764488e-01f, 1.158597774e-02f, -3.094834958e-01f, 2.450403219e-01f,         \
     3.056864685e-02f, -8.538186866e-02f, 1.466789586e-02f}
// Round 6 (EILEV_GELU_PHI, the default): the same GELU as x * Phi(x) with Phi(x) = 1 / 2 + xc q(xc^2), xc = x clamped to +-3.95, q of degree 6
// (minimax with Phi(3.95) = 1 pinned, so that x > 3.95 returns x and x < -3.95 returns 0): max abs error 1.67e-4 (relative 2.6e-3 where
// |y| > 0.05) against 1.1e-4 / 2.2e-3 of the form above — both an order of magnitude inside the bf16 rounding of the pre-activation the
// reference evaluates GELU on.  What it buys is VALU issue slots, the one thing the epilogue costs (tools/probes/valu_shadow.hip: a SIMD of
// gfx950 does not run VALU and MFMA instructions concurrently, §5 of DESIGN.md): one unpacked operation (v_med3) and nine that hipcc packs
// into v_pk_mul / v_pk_fma_f32, against three unpacked (|x| min, max, the bias of the clamp) and nine packed.
#ifndef EILEV_GELU_PHI
#define EILEV_GELU_PHI 1
#endif
#define EILEV_GELU_PHI_C 3.95f
#define EILEV_GELU_PHI_COEFFS                                                                                               \
    {3.979867044e-01f, -6.472275670e-02f, 8.842919395e-03f, -8.290393928e-04f, 4.955192888e-05f, -1.681151575e-06f, 2.443575809e-08f}
// NP independent elements at a time: NP Horner chains interleaved step by step.
template <int NP>
__device__ __forceinline__ void gelu_erf_n(float (&x)[NP]) {
#if EILEV_GELU_PHI
    constexpr float q[7] = EILEV_GELU_PHI_COEFFS;
    if constexpr (NP % 2 == 0) {  // explicit pairs: v_pk_mul_f32 / v_pk_fma_f32 (left to itself hipcc emits one v_fmaak_f32 per element and step)
        f32x2 xv[NP / 2], xc[NP / 2], s[NP / 2], p[NP / 2];
#pragma unroll
        for (int n = 0; n < NP / 2; ++n) {
            xv[n] = (f32x2){x[2 * n], x[2 * n + 1]};
            xc[n] = (f32x2){__builtin_amdgcn_fmed3f(x[2 * n], -EILEV_GELU_PHI_C, EILEV_GELU_PHI_C), __builtin_amdgcn_fmed3f(x[2 * n + 1], -EILEV_GELU_PHI_C, EILEV_GELU_PHI_C)};
            s[n] = xc[n] * xc[n];
            p[n] = (f32x2){q[6], q[6]};
        }
#pragma unroll
        for (int k = 5; k >= 0; --k)
#pragma unroll
            for (int n = 0; n < NP / 2; ++n) p[n] = __builtin_elementwise_fma(p[n], s[n], (f32x2){q[k], q[k]});
#pragma unroll
        for (int n = 0; n < NP / 2; ++n) {
            const f32x2 y = xv[n] * __builtin_elementwise_fma(xc[n], p[n], (f32x2){0.5f, 0.5f});
            x[2 * n] = y.x;
            x[2 * n + 1] = y.y;
        }
    } else {
#pragma unroll
        for (int n = 0; n < NP; ++n) {
            const float xc = __builtin_amdgcn_fmed3f(x[n], -EILEV_GELU_PHI_C, EILEV_GELU_PHI_C), s = xc * xc;
            float p = q[6];
#pragma unroll
            for (int k = 5; k >= 0; --k) p = fmaf(p, s, q[k]);
            x[n] = x[n] * fmaf(xc, p, 0.5f);
        }
    }
#else
    constexpr float c[EILEV_GELU_DEG + 1] = EILEV_GELU_COEFFS;
    float t[NP], p[NP];
#pragma unroll
    for (int n = 0; n < NP; ++n) {
        t[n] = fmaf(fminf(fabsf(x[n]), EILEV_GELU_UMAX), 2.0f / EILEV_GELU_UMAX, -1.0f);
        p[n] = c[EILEV_GELU_DEG];
    }
#pragma unroll
    for (int k = EILEV_GELU_DEG - 1; k >= 0; --k)
#pragma unroll
        for (int n = 0; n < NP; ++n) p[n] = fmaf(p[n], t[n], c[k]);
#pragma unroll
    for (int n = 0; n < NP; ++n) x[n] = fmaxf(x[n], 0.0f) - p[n];
#endif
}

__device__ __forceinline__ float gelu_erf_n1(float x) {
    float v[1] = {x};
    gelu_erf_n<1>(v);
    return v[0];
}

static inline int64_t ceil_div64(int64_t a, int64_t b) { return (a + b - 1) / b; }
static inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---- probe bits ---------------------------------------------------------------------------------------------------------------
// GemmArgs::dbg (eilev_debug_gemm_flags) and AttnArgs::dbg (eilev_debug_attn_v1(dbg << 1)) of the -DEILEV_PROBES build; always 0 in the
// product library.  The values are an interface (tools/*.py and the A/B tests pass them as numbers): none may change.  Several share a bit
// with a field (noted): both meanings apply.
enum : int {
    DBG_GEMM_ROW0_STORES = 1 << 0,          // epilogues store output row 0 only (and pp4 takes no lean epilogue)
    DBG_GEMM_ONE_KSTEP = 1 << 1,            // K loops run one step
    DBG_GEMM_NO_DMA = 1 << 2,               // register-staged per-tile kernels only: no LDS-DMA, pp4, w6, split-K or 64 x 128 route
    DBG_GEMM_SKINNY_NO_DMA = 1 << 3,        // bf16 skinny launches: the plain kernel (no LDS-DMA, nb or rows32 kernels)
    DBG_GEMM_FORCE_SHIFT = 4,               // (dbg >> 4) & 15: the tile choice forced (GemmForce below)
    DBG_GEMM_SKINNY_NO_PRELOAD = 1 << 7,    // skinny kernels do not preload the activations (bit 3 of the force field)
    DBG_GEMM_ROW_MAJOR_TILES = 1 << 8,      // tiles walked in plain row-major order (no XCD / group remap)
    DBG_GEMM_NO_EPILOGUE = 1 << 10,         // no epilogue at all (accumulators kept alive)
    DBG_GEMM_NO_STORES = 1 << 11,           // epilogue without its store phase
    DBG_GEMM_A_ROW0 = 1 << 12,              // lda = 0: every A row aliases row 0
    DBG_GEMM_W_ROW0 = 1 << 13,              // ldw = 0: every W row aliases row 0
    DBG_GEMM_NO_WIDE = 1 << 14,             // 256 x 128 shapes are not promoted to the persistent kernels
    DBG_GEMM_NO_STREAM_LAYOUT = 1 << 15,    // rows32 ignores GemmArgs::Wp
    DBG_GEMM_C_ROW0 = 1 << 17,              // ldc = 0: every output row aliases row 0
    DBG_GEMM_NO_HALF_TILES = 1 << 19,       // no 128-column half-tile path (pp4, tiled)
    DBG_GEMM_WIDE_TILED = 1 << 20,          // a promoted 256 x 128 shape runs the per-tile 256 x 256 kernel, not pp4
    DBG_GEMM_NO_W6 = 1 << 21,               // w6 is never picked
    DBG_GEMM_GROUP_SHIFT = 22,              // (dbg >> 22) & 3: tile-group height 1: 4 rows, 2: 8, 3: 16
    DBG_GEMM_PP4_NO_PRESTAGE = 1 << 24,     // pp4 without the lean epilogue and the second pre-staged K-step
    DBG_GEMM_NB_SHIFT = 26,                 // (dbg >> 26) & 7: skinny weight blocks per workgroup 1 / 2 / 4 / (7) 8
    DBG_GEMM_ROWS32_FIRST_FIT = 1 << 27,    // rows32 first-fit plan, GemmArgs::Wp ignored (bit 1 of the nb field)
    DBG_GEMM_NO_ROWS32 = 1 << 28,           // rows32 never takes a launch (bit 2 of the nb field)
    DBG_GEMM_NO_REDUCE_LN = 1 << 29,        // split-K reduce and LayerNorm as two launches
    DBG_GEMM_NB_BLOCKS_ONLY = 1 << 30,      // the nb default counts weight blocks, not blocks x K splits

    DBG_ATTN_NO_COMPUTE = 1 << 0,           // attn_prefill_v2_kernel stages its key tiles but computes nothing
    DBG_ATTN_NO_PREFETCH = 1 << 1,          // attn_prefill_v2_kernel does not stage the next key tile early
    DBG_ATTN_NO_FRAME = 1 << 2,             // no whole-frame ViT kernel
    DBG_ATTN_FRAME3 = 1 << 4,               // the two-phase frame kernel at any frame count
    DBG_ATTN_NO_FRAME3 = 1 << 5,            // never the two-phase frame kernel
    DBG_ATTN_V2_4WAVES = 1 << 6,            // hd = 128: 4 waves per workgroup
    DBG_ATTN_FRAME_STAMPS = 1 << 8,         // attn_frame_kernel phase stamps
    DBG_ATTN_FRAME3_STAMPS = 1 << 9,        // attn_frame3_kernel phase stamps (and the two-phase kernel forced)
    DBG_ATTN_HEAD_MAJOR = 1 << 10,          // TIMING (wrong results): q / k / v read as if stored head-major
    DBG_ATTN_FRAME3_NO_STORES = 1 << 11,    // TIMING (no output): attn_frame3_kernel without its O stores
};
// (dbg >> DBG_GEMM_FORCE_SHIFT) & 15: 1-4 = that TileCfg (gemm.hip), or one kernel regardless of the shape
enum GemmForce : int { FORCE_NONE = 0, FORCE_PP4 = 9, FORCE_W6 = 12, FORCE_64x128 = 13, FORCE_128x128 = 14, FORCE_SPLIT_K = 15 };

// ---- host-side launchers shared between translation units -------------------------------------
struct GemmArgs {
    const bf16 *A;      // [M, K] row-major, leading dimension lda (elements, multiple of 8)
    int64_t lda;
    const bf16 *W;      // [N, K] row-major (checkpoint layout), leading dimension ldw
    int64_t ldw;
    const bf16 *Wp = nullptr;  // optional: the same matrix in the stream layout of gemm_rows32_kernel (gemm_skinny.h; eilev_stream_layout_pack)
    // Row-block layout of the <= 32 activation rows of a decode step (round 5; frag32_index below): only gemm_rows32_kernel reads (a_frag) or
    // writes (c_frag: plain bf16 epilogue; ln_frag: the LayerNorm rows that ride on a split-K reduce) it — any other kernel family refuses
    int a_frag = 0, c_frag = 0, ln_frag = 0;
    // Scattered output of the ViT q|k|v projection (round 5): C is not [M][N].  With the weight rows reordered so that, per third of N, the output
    // columns are [head h dims 0..63] for all hm_heads heads and then [head h dims 64..hm_hd-1] for all heads (engine: ensure_vit_fold), the
    // epilogue gives every (frame, q | k | v, head) one block of hm_tok * hm_hd elements: [token][64] followed by [token][hm_hd - 64].  The frame
    // attention stages a head's 45-KB image from two contiguous runs (row-major rows: 257 segments of 176 bytes, 8448 bytes apart, each
    // straddling 2-3 cache lines that the neighbouring heads fetch again), and a wave's store of 8 token rows x 64 columns of a [token][64]
    // block is one contiguous kilobyte (a plain head-major [token][88] layout made every store ~12 partial lines: profiles/r05_head_major_*).
    // Only the folded-LayerNorm 16 x 16 instance of the persistent kernel writes it (hm_takes below); everything else refuses.
    int hm_tok = 0, hm_heads = 0, hm_hd = 0;
    const bf16 *bias;   // [N] or null
    const bf16 *resid;  // [M, N] (ldr) or null; in patch mode: position table [1+group, N]
    int64_t ldr;
    void *C;            // bf16 or f32 [M(+CLS rows), N] with leading dimension ldc
    int64_t ldc;
    int M, N, K;
    int epi;            // 0 none, 1 GELU(erf), 2 ReLU
    int out_f32;
    float scale;        // columns [0, scale_cols) are multiplied by scale after the bias
    int scale_cols;
    int patch_group;    // > 0: patch-embedding row remap (see gemm.hip)
    int dbg;            // probe-only
    float *scratch;     // optional fp32 scratch for the skinny kernel's split-K partials
    size_t scratch_bytes;
    // fp8 (OCP e4m3) weights with one fp32 scale per output channel: C = (A . Wq^T) * wscale + bias (eilev_linear_w8)
    const float *wscale = nullptr;  // [N] or null
    const uint8_t *W8 = nullptr;    // [N, K] e4m3 bytes (ldw = K) when the weights are still quantised (skinny kernel)
    bf16 *w8_scratch = nullptr;     // [N, K] bf16: where a large-M call expands W8 to (exact: every e4m3 value is a bf16 value)
    // fp8 (e4m3) ACTIVATIONS with one fp32 scale per row (eilev_linear_a8w8): together with W8 the product runs on the fp8 MFMA
    // (v_mfma_f32_32x32x64_f8f6f4, twice the bf16 rate): C = (Aq . Wq^T) * ascale[m] * wscale[n] + bias.  lda / ldw count BYTES = k.
    const uint8_t *A8 = nullptr;    // [M, K] e4m3 bytes
    const float *ascale = nullptr;  // [M]
    // LayerNorm folded into the GEMM that consumes it (eilev_linear_lnfold; ViT ln1 -> qkv, ln2 -> fc1): A holds the RAW residual stream,
    // W = gamma (.) W_orig, bias = b + W_orig . beta, and C = rstd[m] * (A . W^T - mean[m] * csum[n]) + bias[n]: the accumulators start
    // from -mean[m] * csum[n], the epilogue multiplies by rstd[m].  ln_rows = (rstd, -mean) per row, csum[n] = sum_k W[n, k].
    const float *ln_rows = nullptr;  // [M][2] or null
    const float *ln_csum = nullptr;  // [N]
    // ... and the GEMM that PRODUCES the residual stream (proj / fc2 with the residual epilogue) emits, per 64-column slot and row, the
    // partial (sum, sum of squares) of what it writes: stat_out[(slot * stat_ld + row) * 2 + {0, 1}], slot = column / 64 (fixed order
    // of summation downstream: deterministic).  stat_ld = rows of the whole matrix (row-chunked launches shift stat_out, not stat_ld).
    float *stat_out = nullptr;
    int64_t stat_ld = 0;
    // LayerNorm of the finished output rows, written next to them: ln_out[m] = LN(C[m]) * ln_gamma + ln_beta over the bf16 rows of C.
    // Decode (M <= 32, split-K): done by the kernel that sums the partials (one launch instead of reduce + LayerNorm, bit-identical);
    // every other shape: a LayerNorm launch after the GEMM.
    const bf16 *ln_gamma = nullptr, *ln_beta = nullptr;
    bf16 *ln_out = nullptr;  // [M, N], leading dimension N
    float ln_eps = 0.0f;
    int k_slice = 0;                // > 0: split-K launch (gridDim.y slices of k_slice K-steps, f32 output accumulated atomically)
    // probe-only (tools/gemm_trace.py): per-tile phase timestamps of the persistent ping-pong kernel, 8 u64 per (workgroup, wave
    // group, tile): s_memrealtime at loop top / K-loop start / K-loop end / epilogue start / epilogue end, s_memtime at top / end
    unsigned long long *trace = nullptr;
    int trace_tiles = 0;
};

// Row-block ("fragment order") layout of up to 32 activation rows x K: element (row, col) at (col / 32) * 1024 + row * 32 + col % 32 — the 16
// rows x 32 columns an MFMA operand load of the decode GEMVs reads are ONE contiguous kilobyte (row-major gives it 16 segments of 64 bytes
// a row apart: 4.04 -> 3.85 ms / token at batch 32).  A buffer in this layout holds 32 rows whatever M is.  8-element chunks stay contiguous.
__host__ __device__ static inline int64_t frag32_index(int row, int col) { return (int64_t)(col >> 5) * 1024 + row * 32 + (col & 31); }

// Probe build only: the kernel instance launch_gemm launched last (eilev_debug_gemm reports it; tests/gemm_ref.py names the codes).  Low 16 bits:
// 1000 gemm_nt_kernel / 2000 gemm_glds_kernel + 10 * tile (1 256 x 256, 2 256 x 128 two stages, 3 256 x 128 one stage, 4 128 x 128,
// 5 64 x 128) + epi; 3000 + slices: split-K; 4000 + 100 * LN + 10 * instance (0 32 x 32 MFMAs, 1 / 2 the 16 x 16 forms M16K = 1 / 2, 3 A3,
// 4 fp8 MFMA) + epi: gemm_pp4_kernel; 5000 + epi: gemm_w6_kernel.  Bits above: the launch was cut into row chunks / its fp8 weights expanded.
// The M <= 32 family (gemm_skinny.h): 6000 gemm_skinny_kernel; 6100 + 10 MB + PRE gemm_skinny_dma_kernel; 6200 + 10 MB + NB gemm_skinny_nb_kernel;
// 6300 + KS gemm_rows32_kernel; 6400 + 10 MB + PRE gemm_skinny_w8_kernel.  Bits: K split over gridDim.y (GEMM_FORM_KS records the slice count),
// the reduce that also wrote the LayerNorm rows, the stream layout (GemmArgs::Wp) actually read.
// A plain global on purpose: GemmArgs::dbg would move the launch off the product's route.  The product library has neither.
#ifdef EILEV_PROBES
extern int g_gemm_form;
#define GEMM_FORM(code) (g_gemm_form = (g_gemm_form & ~0xffff) | (code))
#define GEMM_FORM_BIT(bit) (g_gemm_form |= (bit))
extern int g_gemm_ks;
#define GEMM_FORM_KS(n) (g_gemm_ks = (n))
#else
#define GEMM_FORM(code) ((void)0)
#define GEMM_FORM_BIT(bit) ((void)0)
#define GEMM_FORM_KS(n) ((void)0)
#endif
enum : int { GEMM_FORM_ROW_CHUNKS = 1 << 16, GEMM_FORM_W8_EXPANDED = 1 << 17, GEMM_FORM_SPLIT_K = 1 << 18, GEMM_FORM_REDUCE_LN = 1 << 19,
             GEMM_FORM_STREAM_LAYOUT = 1 << 20 };

int launch_gemm(const GemmArgs &g, int prof_kind, hipStream_t s);
bool gemm_rows32_takes(const GemmArgs &g);  // would launch_gemm run g on gemm_rows32_kernel (the one kernel of the row-block layout)?
int launch_pp4_ext(const GemmArgs &g, int grid, hipStream_t s);  // gemm_pp4_ext.hip
// every tile of a persistent-kernel launch can take the lean epilogue (what the 16 x 16 MFMA instances need: gemm_pp4.h M16)
// Probe build: the per-tile stamps of tools/gemm_trace.py / gemm_timeline.py run on the product's 16 x 16 instances.  (In rounds 2-5 a trace
// buffer — like any probe flag — made a launch fall back to the 32 x 32 instances, whose half tiles cost 0.85-1.0 of a whole tile instead of
// 0.72-0.77: a traced or flagged arm of an A/B measured another kernel than the product's.  Probe flags still do: an A/B of two flag values
// compares like with like, an A/B against flags = 0 does not.)
#ifdef EILEV_PROBES
#define EILEV_TRACE_M16 true
#else
#define EILEV_TRACE_M16 false
#endif
static inline bool pp4_all_lean(const GemmArgs &g) {
    // (column scaling — the q part of a fused q|k|v projection — only on plain bias-only launches, in whole 16-column blocks)
    const bool scale_ok = g.scale_cols == 0 || (g.scale_cols % 16 == 0 && g.epi == 0 && !g.resid && !g.ln_rows && !g.stat_out);
    return g.N % 128 == 0 && !g.out_f32 && g.patch_group == 0 && scale_ok && !g.wscale && !g.ascale && !g.dbg && (!g.trace || EILEV_TRACE_M16);
}
// the launch can write the head-major q|k|v layout (GemmArgs::hm_tok)
static inline bool hm_takes(const GemmArgs &g) {
    // (hm_tok >= 128: the 128 rows a wave stores cross at most ONE frame boundary — gemm_pp4.h lean_epilogue steps its offsets by a single frame)
    return g.hm_tok >= 128 && g.hm_heads > 0 && g.hm_hd > 64 && g.hm_hd % 8 == 0 && g.N == 3 * g.hm_heads * g.hm_hd && g.ln_rows && g.epi == 0 && !g.resid &&
           !g.stat_out && !g.scale_cols && pp4_all_lean(g) && g.N % 64 == 0 && g.M % g.hm_tok == 0 && (int64_t)g.M * g.N * 2 < 0xfffffff0ll;
}
// gemv.hip: nn.Linear on M <= 8 rows as row dot products with the LayerNorm / flash-decoding merge in its prologue
bool gemv_rows_ok(int M, int N, int K);
int launch_gemv_rows(int pro, const bf16 *x, int64_t ldx, const bf16 *gamma, const bf16 *beta, float eps, const float *part, int heads, int hd,
                     int nsplit, const bf16 *W, const bf16 *bias, const bf16 *resid, int64_t ldr, void *out, int64_t ldo, int out_f32, int M, int N,
                     int K, int epi, float scale, int scale_cols, hipStream_t s);
// gemv.hip, M = 1: activations in registers, a 4-deep ring of weight sub-blocks, one workgroup per CU (round 4)
bool gemv1_ok(int N, int K, int pro);
int launch_gemv1(int pro, const bf16 *x, const bf16 *gamma, const bf16 *beta, float eps, const bf16 *W, const bf16 *bias, const bf16 *resid, void *out,
                 int out_f32, int N, int K, int epi, float scale, int scale_cols, hipStream_t s, const float *part = nullptr, int heads = 0, int hd = 0,
                 int nsplit = 0);  // pro = 2: x = the merge of `part` (flash-decoding partials of one row: heads x nsplit x (hd + 2) floats)
bool gemvm_ok(int M, int N, int K, int pro);  // 2 <= M <= 8 rows with the same geometry, rows staged in LDS (round 4)
int launch_gemvm(int pro, const bf16 *x, int64_t ldx, const bf16 *gamma, const bf16 *beta, float eps, const bf16 *W, const bf16 *bias, const bf16 *resid,
                 int64_t ldr, void *out, int64_t ldo, int out_f32, int M, int N, int K, int epi, float scale, int scale_cols, hipStream_t s);
// misc.hip: the glue kernels
int launch_im2col(const void *pix, int dtype, bf16 *out, int64_t rows, int frames, int img, int patch, int kp, hipStream_t s);
int launch_pad_rows(const bf16 *w, bf16 *out, int rows, int k, int kp, hipStream_t s);
int launch_cls_rows(const bf16 *cls, const bf16 *pos, bf16 *x, int64_t frames_total, int tok, int d, hipStream_t s);
int launch_quant_rows_e4m3(const bf16 *x, int64_t ldx, uint8_t *q, float *scale, int64_t rows, int cols, hipStream_t s);
int launch_broadcast_rows(const bf16 *src, bf16 *dst, int64_t copies, int64_t n, hipStream_t s);
int launch_embed_scatter(const bf16 *embed, const int64_t *ids, const uint8_t *mask, const bf16 *feats, int64_t n_rows,
                         int64_t total, int vocab, bf16 *out, int d, hipStream_t s);
int launch_pos_embed(const bf16 *emb, const bf16 *pos, const int32_t *mask, int32_t *pid, bf16 *h, int batch, int L, int d, hipStream_t s,
                     int past = 0);
int launch_decode_embed(const bf16 *embed, const bf16 *pos, const int64_t *tokens, const int32_t *n_valid, const int32_t *state,
                        int vocab, int max_pid, bf16 *h, int batch, int d, hipStream_t s);
int launch_kv_write(const bf16 *qkv, bf16 *kc, bf16 *vc, int batch, int rows_per_b, int heads, int hd, int cap, int seq_len,
                    const int32_t *state, hipStream_t s, int slot0 = 0);
int launch_select(const float *logits, int batch, int vocab, int32_t *state, uint8_t *finished, int64_t eos_id, int64_t pad_id,
                  int64_t *tokens, int64_t *out_tokens, int64_t max_new, hipStream_t s);
int launch_topk_logprob(const float *logits, const float *row_score, int rows, int vocab, int keep, float *out_val, int32_t *out_idx, hipStream_t s);
int launch_beam_advance(const float *row_lp, const int32_t *row_tok, int batch, int beams, int keep, int max_new, const int32_t *state,
                        const int64_t *eos_ids, int n_eos, const float *len_pow, int recip, int early, int64_t *run_seq, float *run_score,
                        int64_t *fin_seq, float *fin_score, int64_t *fin_len, uint8_t *finished, uint8_t *can_improve, int64_t *tokens, int32_t *anc,
                        int gen_cap, int64_t *scratch, hipStream_t s);
int launch_t5_rel_table(const bf16 *rel_w, float *tab, int n, int off, int heads, int bidirectional, int num_buckets, int max_dist,
                        hipStream_t s, const int32_t *state = nullptr);
int launch_gated_gelu(const bf16 *ab, int64_t ld, bf16 *out, int64_t rows, int F, hipStream_t s);
int launch_rows_to_cache(const bf16 *src, int64_t ld, int col0, bf16 *plane, int batch, int rows_per_b, int heads, int hd, int cap,
                         int slot0, hipStream_t s, const int32_t *state = nullptr);
int launch_layernorm(const bf16 *x, int64_t ldx, const bf16 *g, const bf16 *b, bf16 *y, int64_t ldy, int64_t rows,
                     int cols, float eps, hipStream_t s);
int launch_fold_layernorm(const bf16 *w, const bf16 *gamma, const bf16 *beta, const bf16 *bias, int N, int K, bf16 *wf, float *csum, bf16 *bf,
                          hipStream_t s);
int launch_reduce_ln(const float *part, int ks, int mr, int M, int N, const float *wscale, const bf16 *bias, const bf16 *resid, int64_t ldr, bf16 *C,
                     int64_t ldc, const bf16 *gamma, const bf16 *beta, bf16 *ln_out, float eps, hipStream_t s, int ln_frag = 0);
int launch_ln_finalize(const float *part, int slots, int64_t rows, int cols, float eps, float *out, hipStream_t s);

struct AttnArgs {
    const bf16 *q, *k, *v;
    bf16 *o;
    int64_t q_bs, k_bs, v_bs, o_bs;  // batch strides (elements)
    int64_t q_hs, k_hs, v_hs, o_hs;  // head strides (elements)
    int64_t ldq, ldk, ldv, ldo;      // row strides (elements)
    int batch, heads, sq, skv, hd;
    float scale;
    int causal;
    const int32_t *key_mask;         // (batch, mask_ld) or null
    int64_t mask_ld;
    int dbg = 0;                     // probe-only: launch_attention sets it
    // T5 relative position bias (additive, before the softmax): bias(h, i, j) = rel_tab[h * rel_hs + (j - i - (skv - sq)) +
    // rel_off], a per-head table over the relative distance (built by launch_t5_rel_table); null = none
    const float *rel_tab = nullptr;
    int64_t rel_hs = 0;
    int rel_off = 0, rel_n = 0;
    // ViT frame attention on the scattered q|k|v of GemmArgs::hm_tok (round 5): q / k / v point at the first (frame, head) block of their
    // plane, *_bs = frame stride, *_hs = block stride (S * hd); a block is [S][64] followed by [S][hd - 64] elements.  ld* are ignored.
    int hm = 0;
    // dropout on the attention probabilities (training graph): element (b, h, i, j) is kept iff eilev_hash32(drop_seed, its linear
    // index) >= drop_thr, kept probabilities are scaled by drop_scale = 1 / (1 - p); drop_thr = 0: none
    uint32_t drop_thr = 0, drop_seed = 0;
    float drop_scale = 1.0f;
};
// The two layouts an attention is launched on; both return a fully initialised AttnArgs (no mask, not causal, no bias, no dropout) whose
// output is the dense [batch * sq][heads * hd] matrix `o`.  What is special about a launch (mask, causal, ...) is the caller's to set.
// Rows: q / k / v are columns of row-major activation buffers (row strides ldq / ldk / ldv; a head every hd elements), sq query and skv key
// rows per batch entry.
static inline AttnArgs attn_rows(const bf16 *q, int64_t ldq, const bf16 *k, int64_t ldk, const bf16 *v, int64_t ldv, bf16 *o, int64_t batch,
                                 int64_t heads, int64_t sq, int64_t skv, int64_t hd, float scale) {
    AttnArgs a;
    a.q = q; a.k = k; a.v = v; a.o = o;
    a.q_bs = sq * ldq; a.k_bs = skv * ldk; a.v_bs = skv * ldv; a.o_bs = sq * heads * hd;
    a.q_hs = a.k_hs = a.v_hs = a.o_hs = hd;
    a.ldq = ldq; a.ldk = ldk; a.ldv = ldv; a.ldo = heads * hd;
    a.batch = (int)batch; a.heads = (int)heads; a.sq = (int)sq; a.skv = (int)skv; a.hd = (int)hd; a.scale = scale; a.causal = 0;
    a.key_mask = nullptr; a.mask_ld = 0;
    return a;
}
// Cache planes: the queries are rows as above, keys and values the planes [batch][heads][cap][hd] of a KV cache, slots [0, skv) of each.
static inline AttnArgs attn_cache(const bf16 *q, int64_t ldq, const bf16 *kplane, const bf16 *vplane, int64_t cap, bf16 *o, int64_t batch,
                                  int64_t heads, int64_t sq, int64_t skv, int64_t hd, float scale) {
    AttnArgs a = attn_rows(q, ldq, kplane, hd, vplane, hd, o, batch, heads, sq, skv, hd, scale);
    a.k_bs = a.v_bs = heads * cap * hd;
    a.k_hs = a.v_hs = cap * hd;
    return a;
}
int launch_attention(const AttnArgs &a, hipStream_t s);

// attn_decode.hip: the single query of a decode step per (row, head) against a KV cache.  Host side only: the launchers choose a kernel and
// pass these values on as its arguments.
struct DecodeAttnArgs {
    const bf16 *qkv = nullptr;        // query rows, row stride ldq; with fuse_new q | k | v of the step (the new token's K / V follow q)
    int64_t ldq = 0;                  // 0: 3 * heads * hd (q | k | v rows)
    const bf16 *kc = nullptr, *vc = nullptr;  // cache planes [batch][heads][cap][hd] (beam form: the prompt cache, one row per sample)
    bf16 *out = nullptr;              // [batch][heads * hd]; null: launch_attn_decode leaves the partials of the 256-key split kernel in `part`
    const int32_t *attn_mask = nullptr;  // (batch, seq_len) or null: keys < seq_len obey it, newer ones are visible
    const int32_t *state = nullptr;   // kv_total = seq_len + state[0], read on the device (hipGraph replay); null: kv_total = seq_len
    int batch = 0, seq_len = 0, cap = 0, heads = 0, hd = 0;
    float *part = nullptr; size_t part_bytes = 0;  // flash-decoding partials: (max, sum, o[hd]) floats per (row, head, key range)
    int fuse_new = 0;                 // the newest key / value is still only in the q|k|v row: the kernel stores it into the cache
    // T5 position bias rel_tab[h * rel_hs + (key - query) + rel_off], the query at kv_total - 1 (rel_off < 0: this query row's table, entry j = key j)
    const float *rel_tab = nullptr;
    int64_t rel_hs = 0; int rel_off = 0;
    // beam search without moving the cache: row b is beam b % beams of sample b / beams; key seq_len + g is the g-th generated token of its
    // hypothesis, in row anc[g * batch + b] of the generation cache kg / vg (capacity cap_g); the new token goes to the row's own slot
    bf16 *kg = nullptr, *vg = nullptr;
    const int32_t *anc = nullptr;
    int beams = 1, cap_g = 0;
    int out_frag = 0;                 // `out` in the row-block layout (frag32_index): attn_decode_loop_kernel only (attn_decode_loop_ok)
    // beam form, head sizes 80 / 128: the prompt keys of a sample are read ONCE for its `beams` rows (attn_shared_prompt_kernel), the generated
    // keys per row in 128-key ranges that start at seq_len; partials of attn_decode_shared_part_bytes in `part`, attn_mask may be null
    int shared_prompt = 0;
    int64_t q_stride() const { return ldq ? ldq : 3 * (int64_t)heads * hd; }
    int keys() const { return anc ? seq_len + cap_g : cap; }  // the cache slots a row can attend to
};
// partials of `keys` keys in ranges of `range` keys; the 128-key ranges (the default) need the most of any form
size_t attn_decode_part_bytes(int batch, int heads, int hd, int keys, int range = 128);
// shared_prompt: key ranges per (row, head) = prompt ranges of kSharedPromptKeys keys + 128-key ranges of the cap_g generated keys, and their bytes
constexpr int kSharedPromptKeys = 128;
int attn_decode_shared_nsplit(int seq_len, int cap_g);
size_t attn_decode_shared_part_bytes(int batch, int heads, int hd, int seq_len, int cap_g);
bool attn_decode_loop_ok(const DecodeAttnArgs &a);  // the launch takes attn_decode_loop_kernel: the only form that writes the row-block layout
// The merged rows into a.out, the kernel chosen by batch size, head size and flags.  a.out == nullptr: the partials of the 256-key split
// kernel stay in a.part for the caller to merge (gemv_rows_kernel's prologue), *nsplit = their ranges per (row, head).
int launch_attn_decode(const DecodeAttnArgs &a, hipStream_t s, int *nsplit = nullptr);
// plain steps at small batch (state, fuse_new; no beams, no bias): one workgroup per (row, head), every key in one pass (round 4)
bool attn_decode1_ok(int batch, int cap, int hd);
int launch_attn_decode1(const DecodeAttnArgs &a, hipStream_t s);
// ... the same loading scheme over 128-key ranges, partials for gemv1_kernel's merge prologue; *nsplit = the ranges per (row, head)
int launch_attn_decode_part(const DecodeAttnArgs &a, hipStream_t s, int *nsplit);
// attn_decode_merge_kernel alone: the partials of `nsplit` key ranges per (row, head) -> out [batch][heads * hd] (kv8.hip leaves its own
// kernel's partials to it)
int launch_attn_decode_merge(const float *part, bf16 *out, int batch, int heads, int hd, int nsplit, hipStream_t s);
// flan-t5 beam search: the cross-attention of `rows` query rows (stride ldq, head size 64) of which every `beams` consecutive ones share one
// sample's keys / values — planes [rows / beams][heads][cap][hd], keys [0, enc_len), enc_mask (rows / beams, enc_len) or null — read once
// per (sample, head, 128-key range); partials in `part` (attn_decode_part_bytes(rows, heads, hd, enc_len)), merged into out [rows][heads * hd].
// No scale, no bias.  hd != 64: EILEV_E_UNSUPPORTED before any launch.
int launch_attn_cross_shared(const bf16 *q, int64_t ldq, const bf16 *kc, const bf16 *vc, const int32_t *enc_mask, int rows, int beams, int heads,
                             int hd, int enc_len, int cap, bf16 *out, float *part, size_t part_bytes, hipStream_t s);
int launch_rmsnorm(const bf16 *x, int64_t ldx, const bf16 *g, bf16 *y, int64_t ldy, int64_t rows, int cols, float eps, hipStream_t s);

void prof_begin(int kind, double flops, hipStream_t s);
void prof_end(hipStream_t s);

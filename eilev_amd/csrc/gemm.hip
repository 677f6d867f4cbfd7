// gemm.hip — bf16 MFMA GEMM family for gfx950:  C[M,N] = epi(A[M,K] . W[N,K]^T + bias) (+ resid)
//
// Replaces every nn.Linear on the path (hf modeling_blip_2.py:328,351,366-368,584-586,618,660,674;
// hf modeling_opt.py:151-179,239-247,512; ref:eilev/model/v2.py:308).  Weights stay in the checkpoint's
// [out,in] layout: both MFMA operands then read 8 consecutive k per lane (16-byte loads), no transposes.
//
// Tiled kernel (M > 16): BMxBNx64 tile, 64-lane waves each owning a (BM/NWM)x(BN/NWN) sub-tile made of
// 16x16x32 MFMAs (v_mfma_f32_16x16x32_bf16, fp32 accumulate).  Global->register->LDS staging with the
// next tile's loads issued before the current tile's MFMAs (register prefetch) and a 2-deep LDS ring,
// one barrier per K-step.  LDS rows are 128 B (64 bf16); the 16-byte chunk index is XOR-swizzled with
// (row & 7) so the ds_read_b128 fragment reads of 16 consecutive rows spread over all bank groups.
// Workgroup ids are remapped so that each XCD (private L2) walks a contiguous range of tiles.
//
// Skinny kernel (M <= 16, the decode step): one MFMA row-block of 16 weight rows per workgroup, the K
// range split over the 8 waves (and over gridDim.y when N is small) — HBM-bound weight streaming.
//
// Files: gemm_common.h (tile map, swizzle, general epilogue), gemm_tiled.h (per-tile kernels), gemm_pp4.h (persistent ping-pong kernel),
// gemm_w6.h (one wave per SIMD), gemm_skinny.h (M <= 32 weight streaming); this file: the dispatch.  gemm_pp4_ext.hip holds the fp8 /
// LayerNorm-folding instances of the persistent kernel as a second object so that the two long hipcc runs go side by side (build.py).
#include "gemm_common.h"
#include "gemm_tiled.h"
#include "gemm_pp4.h"
#include "gemm_w6.h"
#include "gemm_skinny.h"

int g_eilev_grid_cus = 0;  // 0 = every CU (common.h: eilev_grid_cus); written by the probe build only
#ifdef EILEV_PROBES  // the probe build only (build.py --variant probes -DEILEV_PROBES): the product library has neither the switches nor their state
int g_gemm_debug = 0;  // probe-only switches (tools/gemm_probe.py): GemmArgs::dbg, the DBG_GEMM_* bits of common.h
extern "C" int eilev_debug_gemm_flags(int f) { g_gemm_debug = f; return 0; }
extern "C" int eilev_debug_grid_cus(int n) { g_eilev_grid_cus = n; return 0; }
int g_gemm_form = 0;   // common.h GEMM_FORM: what eilev_debug_gemm (end of this file) reports
int g_gemm_ks = 0;     // common.h GEMM_FORM_KS: the K slices of the last M <= 32 launch (eilev_debug_gemm_skinny)
#endif
#ifdef EILEV_PROBES
unsigned long long *g_gemm_trace = nullptr;  // probe-only: see GemmArgs::trace
int g_gemm_trace_tiles = 0;
extern "C" int eilev_debug_gemm_trace(void *buf, int tiles) { g_gemm_trace = (unsigned long long *)buf; g_gemm_trace_tiles = tiles; return 0; }
#endif

namespace {

// Long K: the 16 x 16 persistent kernel with the A operand three K-steps deep (gemm_pp4.h A3).  An A/B build may set the threshold with -D.
#ifndef EILEV_A3_MIN_K
#define EILEV_A3_MIN_K 5120  /* profiles/r06_a3_min_k.log: flan-t5-xl wo (N = 2048, K = 5120) +10 %, K = 4096 / 2560 / 2048 shapes -3 ... +1 % */
#endif
bool a3_takes(const GemmArgs &g) { return g.epi == 0 && g.K >= EILEV_A3_MIN_K; }

int launch_pp4(const GemmArgs &g, hipStream_t s) {
    constexpr int smem = PP4_SMEM;
    const int tiles = ((g.M + 255) / 256) * ((g.N + 255) / 256);
    const int ncu = eilev_grid_cus();
    const int grid = tiles < ncu ? tiles : ncu / 8 * 8;
    if (g.A8 || g.ln_rows || g.stat_out) return launch_pp4_ext(g, grid, s);  // fp8 MFMA / LayerNorm-folding instances (the other object)
    // 16 x 16 x 32 MFMAs where every tile of the launch is a whole lean tile (gemm_pp4.h: M16)
    if (pp4_all_lean(g) && g.epi != 1) {
        if (a3_takes(g)) return GEMM_FORM(4030), eilev_launch<gemm_pp4_kernel<0, false, 0, 2, true>>(dim3(grid), dim3(512), smem, s, g);
        return eilev_with_epi<0, 2>(g.epi, [&](auto e) { return GEMM_FORM(4020 + decltype(e)::value), eilev_launch<gemm_pp4_kernel<decltype(e)::value, false, 0, 2>>(dim3(grid), dim3(512), smem, s, g); });
    }
    return eilev_with_epi<0, 1, 2>(g.epi, [&](auto e) { return GEMM_FORM(4000 + decltype(e)::value), eilev_launch<gemm_pp4_kernel<decltype(e)::value>>(dim3(grid), dim3(512), smem, s, g); });
}

constexpr int64_t kOffsetLimit = 0x7fff0000ll;  // bytes a 32-bit buffer offset (LDS-DMA, buffer loads) reaches, with room for the last tile
bool fits_offset(int64_t rows, int64_t ld) { return rows * ld * 2 < kOffsetLimit; }

// The launch's arguments with the probe build's process-global switches applied (the product library: none reaches a launch)
GemmArgs with_probes(const GemmArgs &g_in) {
    GemmArgs g = g_in;
#ifdef EILEV_PROBES
    g.dbg = g_gemm_debug;
    g.trace = g_gemm_trace;
    g.trace_tiles = g_gemm_trace_tiles;
#else
    g.dbg = 0;
    g.trace = nullptr;
    g.trace_tiles = 0;
#endif
    if (g.dbg & DBG_GEMM_A_ROW0) g.lda = 0;  // cache-resident operand
    if (g.dbg & DBG_GEMM_W_ROW0) g.ldw = 0;
    if (g.dbg & DBG_GEMM_C_ROW0) g.ldc = 0;  // stores stay in L2
    return g;
}

// One profiler record around one launch (prof_kind < 0: none)
int profiled(int (*launch)(const GemmArgs &, hipStream_t), const GemmArgs &g, int prof_kind, hipStream_t s) {
    if (prof_kind >= 0) prof_begin(prof_kind, 2.0 * g.M * (double)g.N * g.K, s);
    const int rc = launch(g, s);
    if (prof_kind >= 0) prof_end(s);
    return rc;
}

// fp8 activations x fp8 weights (eilev_linear_a8w8): the persistent ping-pong kernel on the fp8 MFMA, general epilogue with the row and
// column scales
int launch_a8w8(const GemmArgs &g, int prof_kind, hipStream_t s) {
    if (!g.W8 || !g.C || !g.wscale || !g.ascale || g.N <= 0 || g.K <= 0) return EILEV_E_BADARG;
    if ((g.K % 128) || g.lda != g.K || g.ldw != g.K || ((uintptr_t)g.A8 & 15) || ((uintptr_t)g.W8 & 15) || g.patch_group != 0 ||
        (int64_t)g.M * g.K >= kOffsetLimit || (int64_t)g.N * g.K >= kOffsetLimit)
        return EILEV_E_UNSUPPORTED;
    if (!g.out_f32 && ((g.ldc & 7) || (g.N & 3) || ((uintptr_t)g.C & 15) || (g.resid && ((g.ldr & 7) || ((uintptr_t)g.resid & 15))))) return EILEV_E_UNSUPPORTED;
    return profiled(launch_pp4, g, prof_kind, s);
}

// fp8 weights: M <= 32 (decode) streams them as bytes (the fp8 skinny kernel); larger M (prefill) expands them to bf16 in the caller's
// scratch (exact: every e4m3 value is a bf16 value) and runs the bf16 kernels with the per-channel scale in their epilogue.
bool w8_streams(const GemmArgs &g) { return g.M <= 32 && g.K % 256 == 0 && g.patch_group == 0; }
int w8_check(const GemmArgs &g) {
    if (!g.A || !g.C || !g.wscale || g.N <= 0 || g.K <= 0 || g.ldw != g.K || ((uintptr_t)g.W8 & 15) || (g.K & 15)) return EILEV_E_BADARG;
    if (!w8_streams(g) && !g.w8_scratch) return EILEV_E_WORKSPACE;
    return EILEV_OK;
}
int w8_expand(const GemmArgs &g, hipStream_t s) {
    const int64_t n16 = (int64_t)g.N * g.K / 16;
    hipLaunchKernelGGL(w8_expand_kernel, dim3((unsigned)ceil_div64(n16, 256)), dim3(256), 0, s, g.W8, g.w8_scratch, n16);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}

bool ln_fold(const GemmArgs &g) { return g.ln_rows != nullptr || g.stat_out != nullptr; }  // LayerNorm-folding variants: the persistent kernel only
// the weight-streaming skinny family (decode) with its LDS-DMA kernels
bool skinny_dma_ok(const GemmArgs &g) { return g.K % 256 == 0 && (!(g.dbg & DBG_GEMM_SKINNY_NO_DMA) || g.W8); }
bool skinny_takes(const GemmArgs &g) { return (g.M <= 16 || (g.M <= 32 && skinny_dma_ok(g))) && g.patch_group == 0 && !ln_fold(g); }

// EILEV_E_BADARG / EILEV_E_UNSUPPORTED of a bf16 launch (or of a W8 launch that streams its weights: g.W = the bytes)
int check_args(const GemmArgs &g) {
    if (!g.A || !g.W || !g.C || g.N <= 0 || g.K <= 0) return EILEV_E_BADARG;
    if ((g.K & 7) || (g.lda & 7) || (g.ldw & 7) || ((uintptr_t)g.A & 15) || ((uintptr_t)g.W & 15)) return EILEV_E_UNSUPPORTED;
    if (g.hm_tok && (!hm_takes(g) || !fits_offset(g.M, g.lda))) return EILEV_E_UNSUPPORTED;  // head-major q|k|v: common.h hm_takes
    if (ln_fold(g) && (g.W8 || g.wscale || g.out_f32 || g.patch_group || g.scale_cols || g.K % BK || !fits_offset(g.N, g.ldw))) return EILEV_E_UNSUPPORTED;
    const bool skinny = skinny_takes(g);
    if ((g.a_frag || g.c_frag || g.ln_frag) && !skinny) return EILEV_E_UNSUPPORTED;
    if (!skinny && !g.out_f32 && ((g.ldc & 7) || (g.N & 3) || ((uintptr_t)g.C & 15) || (g.resid && ((g.ldr & 7) || ((uintptr_t)g.resid & 15))) ||
                                   (g.bias && ((uintptr_t)g.bias & 7))))
        return EILEV_E_UNSUPPORTED;
    return EILEV_OK;
}

// ---- the skinny family (M <= 32: decode) ------------------------------------------------------------------------------------------

// Weight blocks per workgroup of gemm_skinny_nb_kernel (activation fragments reused across them).  Measured at M = 32 (tools/skinny_sweep.py,
// 2 LDS stages so that two workgroups share a CU): lm_head (3142 blocks) 2.82 -> 3.45 / 3.76 / 4.20 TB/s with 2 / 4 / 8 blocks per workgroup,
// qkv (480) 2.25 -> 2.46 with 2 (1.71 with 4: 120 workgroups leave CUs idle), fc1 (640) 2.17 -> 2.30 with 2; the 2560-row matrices and
// M <= 16 are best with one block: keep >= 240 workgroups.
int skinny_nbsel(const GemmArgs &g, int nb, int ks) {
    int nbsel = (g.dbg >> DBG_GEMM_NB_SHIFT) & 7;  // probe override
    if (nbsel == 0 && g.M > 16) {
        // (workgroups = blocks x K splits: fc2 of OPT-2.7B has 160 blocks x 4 splits)
        const int wgs = (g.dbg & DBG_GEMM_NB_BLOCKS_ONLY) ? nb : nb * ks;
        nbsel = wgs >= 8 * 240 ? 8 : (wgs >= 4 * 240 ? 4 : (wgs >= 2 * 240 ? 2 : 1));
    }
    if (nbsel == 7) nbsel = 8;  // probe encoding
    if (nbsel != 2 && nbsel != 4 && nbsel != 8) nbsel = 1;
    if (nbsel == 8 && g.M <= 16) nbsel = 4;
    return g.W8 ? 1 : nbsel;
}

// activations held across NB weight blocks per workgroup (see gemm_skinny_nb_kernel): 2 LDS-DMA stages + ping-pong partials =
// 64 KB + 2 x MB x 4 KB, so two workgroups share a CU
template <int MB, int NB>
int launch_skinny_nb(const SkinnyArgs &a, int nb, hipStream_t s) {
    const size_t sm = 4 * 2 * 8192 + (size_t)2 * 4 * MB * 64 * 4 * 4;
    return eilev_launch<gemm_skinny_nb_kernel<MB, NB, 2>>(dim3((nb + NB - 1) / NB, a.ks), dim3(256), sm, s, a);
}

// The split-K partials summed (+ bias + residual); with GemmArgs::ln_out the LayerNorm of the rows in the same launch (norm.hip)
int skinny_reduce(const GemmArgs &g, const SkinnyArgs &a, hipStream_t s, bool *ln_done) {
    if (g.ln_out && !(g.dbg & DBG_GEMM_NO_REDUCE_LN) && !g.out_f32 && g.epi == 0 && g.scale_cols == 0 && (g.N & 7) == 0 && g.N <= 4096 && (g.ldc & 7) == 0 &&
        (!g.resid || (g.ldr & 7) == 0)) {
        const int rc = launch_reduce_ln(a.part, a.ks, a.mr, g.M, g.N, g.wscale, g.bias, g.resid, g.ldr, reinterpret_cast<bf16 *>(g.C), g.ldc,
                                        g.ln_gamma, g.ln_beta, g.ln_out, g.ln_eps, s, g.ln_frag);
        if (rc == EILEV_OK) {
            *ln_done = true;
            GEMM_FORM_BIT(GEMM_FORM_REDUCE_LN);
        }
        return rc;
    }
    if (g.ln_frag) return EILEV_E_UNSUPPORTED;  // (the row-block LayerNorm rows exist in the fused reduce only)
    hipLaunchKernelGGL(skinny_reduce_kernel, dim3((g.M * g.N + 255) / 256), dim3(256), 0, s, a);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}

// Weight streaming: one MFMA row-block of 16 weight rows per workgroup, the K range split over the 8 waves and, with few blocks, over
// gridDim.y (partials in g.scratch, then skinny_reduce).  Not profiled.
int launch_skinny(const GemmArgs &g, hipStream_t s, bool *ln_done) {
    SkinnyArgs a;
    a.g = g;
    a.mr = g.M <= 16 ? 16 : 32;
    const int nb = (g.N + 15) / 16;
    int ks = nb >= 384 ? 1 : (512 + nb - 1) / nb;  // >= 1.5 workgroups per CU: no split (and no reduce launch); (1024: decode 5.03 -> 5.18 ms/token)
    const int ksteps = (g.K + 31) / 32;
    if (ks > ksteps / 32) ks = ksteps / 32 > 0 ? ksteps / 32 : 1;  // >= 8 K-steps of 32 per wave
    if (ks > 1 && (!g.scratch || (size_t)ks * a.mr * g.N * sizeof(float) > g.scratch_bytes)) ks = 1;
    a.ks = ks;
    a.part = g.scratch;
    // tiles of 256 per wave: ceil(ceil(K / 256 / ks) / 4); up to 3 (every decode shape) the activations are preloaded
    const bool pre = ((g.K / 256 + ks - 1) / ks + 3) / 4 <= 3 && !(g.dbg & DBG_GEMM_SKINNY_NO_PRELOAD);
    const int nbsel = skinny_nbsel(g, nb, ks);
    // gemm_rows32_kernel takes this launch?  (the row-block activation layouts exist in that kernel only; its plan may split K: ks, a.ks)
    int ks32 = 0, r32_grid = 0;
    const bool r32 = !g.W8 && g.M > 16 && !(g.dbg & DBG_GEMM_NO_ROWS32) && rows32_plan(g, nb, skinny_n_cu(), a, ks, ks32, r32_grid);
    if ((g.a_frag || g.c_frag || g.ln_frag) && !r32) return EILEV_E_UNSUPPORTED;
    const bool dma_ok = skinny_dma_ok(g), m32 = g.M > 16;
    const dim3 grid(nb, ks);
    int rc;
    GEMM_FORM_KS(ks);
    if (ks > 1) GEMM_FORM_BIT(GEMM_FORM_SPLIT_K);
    if (g.W8) {
        GEMM_FORM(6400 + (m32 ? 20 : 10) + (pre ? 1 : 0));
        if (m32) rc = pre ? eilev_launch<gemm_skinny_w8_kernel<2, true>>(grid, dim3(256), 0, s, a) : eilev_launch<gemm_skinny_w8_kernel<2, false>>(grid, dim3(256), 0, s, a);
        else rc = pre ? eilev_launch<gemm_skinny_w8_kernel<1, true>>(grid, dim3(256), 0, s, a) : eilev_launch<gemm_skinny_w8_kernel<1, false>>(grid, dim3(256), 0, s, a);
    } else if (r32) {
        // round 4 (gemm_rows32_kernel): one workgroup per CU, the 32 rows loaded once per CU; it deals the N weight rows over r32_grid
        // workgroups row by row (with a K split the grid is still one workgroup per CU).  The stream layout has no row stride, and a
        // first-fit plan's grid may differ from the one the copy was dealt for.
        if (a.g.Wp && (g.ldw != g.K || (g.dbg & (DBG_GEMM_NO_STREAM_LAYOUT | DBG_GEMM_ROWS32_FIRST_FIT)))) a.g.Wp = nullptr;
        if (a.g.Wp) GEMM_FORM_BIT(GEMM_FORM_STREAM_LAYOUT);
        GEMM_FORM(6300 + ks32);
        const dim3 g32(r32_grid, ks);
        if (ks32 == 10) rc = eilev_launch<gemm_rows32_kernel<2, 10, 3>>(g32, dim3(512), 0, s, a);
        else if (ks32 == 8) rc = eilev_launch<gemm_rows32_kernel<2, 8, 3>>(g32, dim3(512), 0, s, a);
        else rc = eilev_launch<gemm_rows32_kernel<2, 5, 4>>(g32, dim3(512), 0, s, a);
    } else if (dma_ok && pre && nbsel > 1) {
        GEMM_FORM(6200 + (m32 ? 20 : 10) + (m32 ? nbsel : (nbsel == 4 ? 4 : 2)));
        if (m32 && nbsel == 8) rc = launch_skinny_nb<2, 8>(a, nb, s);
        else if (m32 && nbsel == 4) rc = launch_skinny_nb<2, 4>(a, nb, s);
        else if (m32) rc = launch_skinny_nb<2, 2>(a, nb, s);
        else if (nbsel == 4) rc = launch_skinny_nb<1, 4>(a, nb, s);
        else rc = launch_skinny_nb<1, 2>(a, nb, s);
    } else if (dma_ok) {
        GEMM_FORM(6100 + (m32 ? 20 : 10) + (pre ? 1 : 0));
        if (m32) rc = pre ? eilev_launch<gemm_skinny_dma_kernel<2, true>>(grid, dim3(256), 0, s, a) : eilev_launch<gemm_skinny_dma_kernel<2, false>>(grid, dim3(256), 0, s, a);
        else rc = pre ? eilev_launch<gemm_skinny_dma_kernel<1, true>>(grid, dim3(256), 0, s, a) : eilev_launch<gemm_skinny_dma_kernel<1, false>>(grid, dim3(256), 0, s, a);
    } else {
        GEMM_FORM(6000);
        rc = eilev_launch<gemm_skinny_kernel>(grid, dim3(256), 0, s, a);
    }
    if (rc != EILEV_OK || ks == 1) return rc;
    return skinny_reduce(g, a, s, ln_done);
}

// ---- M > 32: the tile choice -----------------------------------------------------------------------------------------------------

// The persistent ping-pong kernel takes shapes of >= 1024 tiles of 256 x 256 whole (it addresses A per tile: no row chunks)
bool pp4_takes(const GemmArgs &g) {
    return g.K % BK == 0 && g.patch_group == 0 && ceil_div64(g.M, 256) * ceil_div64(g.N, 256) >= 1024 &&
           (g.N >= 2048 || ceil_div64(g.M, 256) * ceil_div64(g.N, 128) >= 512) && fits_offset(g.N, g.ldw) && !g.dbg;
}

// The LDS-DMA kernels address A through a 32-bit buffer offset: an A operand of 2 GiB or more (the Q-Former k|v projection of a whole
// step: 1.1 M rows x 1408) is processed as row chunks that fit, each with the fast kernels.  Rows per chunk, 0: no chunks.
int64_t chunk_rows(const GemmArgs &g) {
    if (fits_offset(g.M, g.lda) || g.K % BK || g.patch_group || g.dbg || pp4_takes(g)) return 0;
    const int64_t rows = (kOffsetLimit / (g.lda * 2)) / 256 * 256;
    return rows >= 256 ? rows : 0;
}
// Each chunk is a launch_gemm of its own (and its own profiler record); the caller normalises the whole matrix once (ln_out)
int launch_row_chunks(const GemmArgs &g, int64_t rows_per, int prof_kind, hipStream_t s) {
    for (int64_t r0 = 0; r0 < g.M; r0 += rows_per) {
        GemmArgs c = g;
        c.M = (int)((g.M - r0) < rows_per ? (g.M - r0) : rows_per);
        c.A = g.A + r0 * g.lda;
        if (g.resid) c.resid = g.resid + r0 * g.ldr;
        if (g.stat_out) c.stat_out = g.stat_out + r0 * 2;  // stat_ld stays the row count of the whole matrix
        if (g.ln_rows) c.ln_rows = g.ln_rows + r0 * 2;
        c.C = g.out_f32 ? (void *)(reinterpret_cast<float *>(g.C) + r0 * g.ldc) : (void *)(reinterpret_cast<bf16 *>(g.C) + r0 * g.ldc);
        c.ln_out = nullptr;
        const int rc = launch_gemm(c, prof_kind, s);
        if (rc != EILEV_OK) return rc;
    }
    GEMM_FORM_BIT(GEMM_FORM_ROW_CHUNKS);
    return EILEV_OK;
}

// Per-tile configurations by shape (also the probe force values 1-4)
enum TileCfg : int { CFG_256x256 = 1, CFG_256x128 = 2, CFG_256x128_1S = 3, CFG_128x128 = 4 };
TileCfg tile_cfg(const GemmArgs &g) {
    const int64_t tm256 = ceil_div64(g.M, 256);
    if (tm256 * ceil_div64(g.N, 256) >= 256 && g.N >= 2048) return CFG_256x256;  // 2 LDS stages, 1 WG/CU
    if (tm256 * ceil_div64(g.N, 128) >= 512) return CFG_256x128_1S;              // 1 stage, 2 WG/CU (N = 1408 / 1536)
    if (tm256 * ceil_div64(g.N, 128) >= 192) return CFG_256x128;                 // 2 stages
    return CFG_128x128;
}

// the one-wave-per-SIMD kernel (gemm_w6.h) can run the launch
bool w6_ok(const GemmArgs &g) {
    return g.K % 64 == 0 && g.K >= 256 && g.N % 128 == 0 && (!g.resid || (g.epi == 0 && (g.ldr & 7) == 0)) && !g.out_f32 && g.patch_group == 0 &&
           g.scale_cols == 0 && !g.wscale && fits_offset(g.M, g.lda) && fits_offset(g.N, g.ldw) && (g.ldc & 7) == 0;
}

// A 256 x 256 shape: w6 (256 x 128 tiles) rather than pp4?  Its smaller tiles balance better when there are fewer than 4 rounds of 256 x 256
// tiles (M = 7680 prefill GEMMs: +28 %); with more tiles the ping-pong kernel with the lean epilogue wins (qkv +5 %, OPT out_proj +3 %).
// Round 5 (profiles/r05_w6_vs_pp4_rows.log: rows swept 3840 .. 30 720 at N = 2048 / 2560 / 6144 / 7680 / 10 240): which of the two wins is
// the wave quantisation of its tile count over the CUs — 256 x 256 tiles fill ceil(t / CUs) rounds, the 256 x 128 tiles of w6 twice as
// many half-sized ones — times the ping-pong kernel's ~6 % higher rate at equal fill (e.g. flan-t5-xl wo / o at 30 720 rows: 960 tiles =
// 3.75 rounds, ping-pong 1144 / 995 TFLOP/s against 1071 / 864; OPT qkv at 15 360 rows: 1800 tiles = 7.03 rounds, w6 1166 against 1101).
// The old rule (w6 below 1024 tiles) stays for N that is not a whole number of 256-column tiles.
bool w6_pick(const GemmArgs &g) {
    const int64_t tm256 = ceil_div64(g.M, 256), tiles256 = tm256 * ceil_div64(g.N, 256);
    const int n_cu_q = eilev_num_cu() / 8 * 8;  // (the device's CUs in both builds: the probe build's grid override moves the M <= 32 family and the M <= 8 row-dot kernels of gemv.hip, not this rule)
    auto fill = [&](int64_t t) { return (double)t / (double)(ceil_div64(t, n_cu_q) * n_cu_q); };
    return g.N % 256 == 0 ? 1.06 * fill(tiles256) < fill(tm256 * ceil_div64(g.N, 128)) : tiles256 < 1024;
}

// weight-gradient shape (dW = dY^T X: a few output tiles, f32 out, K = rows of the step): split K over enough slices to fill the CUs
bool split_k_takes(const GemmArgs &g) {
    return g.out_f32 && !g.bias && !g.resid && g.epi == 0 && !g.wscale && g.scale_cols == 0 && g.patch_group == 0 && g.K % BK == 0 && g.K >= 8192 &&
           ceil_div64(g.M, 128) * ceil_div64(g.N, 128) <= 128 && fits_offset(g.M, g.lda) && fits_offset(g.N, g.ldw);
}
int launch_split_k(const GemmArgs &g, hipStream_t s) {
    const int tiles = (int)(ceil_div64(g.M, 128) * ceil_div64(g.N, 128)), nk = g.K / BK;
    int slices = 512 / tiles;
    slices = slices < 2 ? 2 : (slices > 16 ? 16 : slices);
    if (slices > nk / 8) slices = nk / 8 > 1 ? nk / 8 : 1;
    GemmArgs gs = g;
    gs.k_slice = (nk + slices - 1) / slices;
    slices = (nk + gs.k_slice - 1) / gs.k_slice;
    // the M x N output only: with ldc > N the columns between the rows (and the ldc - N words behind the last one) are not this launch's
    if (g.ldc == g.N) EILEV_HIP_CHECK(hipMemsetAsync(g.C, 0, (size_t)g.M * g.N * sizeof(float), s));
    else EILEV_HIP_CHECK(hipMemset2DAsync(g.C, (size_t)g.ldc * sizeof(float), 0, (size_t)g.N * sizeof(float), (size_t)g.M, s));
    GEMM_FORM(3000 + slices);
    return eilev_launch<gemm_glds_kernel<128, 128, 2, 2, 0, 2, 2, 0>>(dim3(tiles, slices), dim3(256), 2 * (128 + 128) * 128, s, gs);
}

// a handful of 128 x 128 tiles (Q-Former graph: 544 rows): 64 x 128, 2 waves, 3 WG/CU (+13 % at 544 x 768 x 768; slower from ~160 tiles on)
bool t64x128_takes(const GemmArgs &g) { return ceil_div64(g.M, 128) * ceil_div64(g.N, 128) < 96 && g.M > 64; }

// The kernel of an M > 32 launch without LayerNorm folding.  Probe terms (dbg, force) only ever move a launch off the product's choice.
int launch_wide(const GemmArgs &g, hipStream_t s) {
    const int force = (g.dbg >> DBG_GEMM_FORCE_SHIFT) & 15;
    const bool no_dma = g.dbg & DBG_GEMM_NO_DMA;
    int cfg = tile_cfg(g);
    bool promoted = false;  // a 256 x 128 shape sent to the persistent kernels
    // N = 1408 / 1536 with >= 512 column-half tiles: the persistent kernels win at every row count measured (fc2 at 34 952 rows:
    // per-tile 696 us, ping-pong 641, one-wave-per-SIMD 582; at 279 616 rows the ping-pong kernel despite its N padding).  With
    // fewer tiles (192-511 halves: 17-34 frames) the one-wave-per-SIMD kernel alone wins (fc2 at 4369 rows: 104 -> 77 us; pp4 124)
    if (cfg == CFG_256x128_1S && g.K % BK == 0 && !(g.dbg & DBG_GEMM_NO_WIDE)) cfg = CFG_256x256, promoted = true;
    if (cfg == CFG_256x128 && w6_ok(g) && force == FORCE_NONE && !(g.dbg & (DBG_GEMM_NO_WIDE | DBG_GEMM_NO_W6 | DBG_GEMM_NO_DMA))) cfg = CFG_256x256, promoted = true;
    if (force == FORCE_PP4) cfg = CFG_256x256;
    if (force == FORCE_64x128 || force == FORCE_128x128 || force == FORCE_SPLIT_K) cfg = CFG_128x128;
    else if (force >= CFG_256x256 && force <= CFG_128x128) cfg = force;

    if (w6_ok(g) && (force == FORCE_W6 || (force == FORCE_NONE && cfg == CFG_256x256 && w6_pick(g) && !(g.dbg & (DBG_GEMM_NO_W6 | DBG_GEMM_NO_DMA)))))
        return launch_w6(g, s);
    switch (cfg) {
        case CFG_256x256:
            if (!(promoted && (g.dbg & DBG_GEMM_WIDE_TILED)) && (force == FORCE_NONE || force == FORCE_PP4) && !no_dma && g.K % BK == 0 && fits_offset(g.N, g.ldw))
                return launch_pp4(g, s);  // persistent ping-pong kernel
            return launch_tiled<256, 256, 2, 4, 2, 2>(g, s);
        case CFG_256x128_1S: return launch_tiled<256, 128, 4, 2, 1, 4, 1>(g, s);
        case CFG_256x128: return launch_tiled<256, 128, 4, 2, 2, 2>(g, s);
        default:
            if (split_k_takes(g) && (force == FORCE_NONE || force == FORCE_SPLIT_K) && !no_dma) return launch_split_k(g, s);
            if ((force == FORCE_64x128 || (force == FORCE_NONE && t64x128_takes(g))) && g.M > 64 && !no_dma) return launch_tiled<64, 128, 1, 2, 2, 3>(g, s);
            return launch_tiled<128, 128, 2, 2, 2, 2>(g, s);
    }
}

}  // namespace


static int launch_gemm_core(const GemmArgs &g_in, int prof_kind, hipStream_t s, bool *ln_done);

// GemmArgs::ln_out: the LayerNorm of the output rows is either produced by the split-K reduction of the decode GEMV (launch_gemm_core
// sets ln_done) or by a LayerNorm launch here.
// Would launch_gemm run this <= 32-row launch on gemm_rows32_kernel (the one kernel that reads / writes the row-block activation layout)?
bool gemm_rows32_takes(const GemmArgs &g) {
    if (!g.A || !g.W || !g.C || g.W8 || g.wscale || g.M <= 16 || g.M > 32 || g.K % 256 || g.patch_group || g.ln_rows || g.stat_out) return false;
    if ((g.lda & 7) || (g.ldw & 7) || ((uintptr_t)g.A & 15) || ((uintptr_t)g.W & 15) || (g.dbg & DBG_GEMM_NO_ROWS32)) return false;
    SkinnyArgs a;
    a.g = g;
    a.mr = 32;
    int ks = 1, ksteps = 0, grid_x = 0;
    return rows32_plan(g, (g.N + 15) / 16, skinny_n_cu(), a, ks, ksteps, grid_x);
}

// include/eilev.h: eilev_stream_layout_pack
extern "C" int eilev_stream_layout_pack(const void *w, int64_t n, int64_t k, void *out, void *stream) {
    if (!w || !out || w == out || n < 1 || k < 1) return EILEV_E_BADARG;
    if (n > 0x7fffffff || k > 0x7fffffff || n * k > 0x7fffffff0ll) return EILEV_E_UNSUPPORTED;
    int ks = 0, ksteps = 0, grid_x = 0;
    if (!rows32_shape((int)n, (int)k, skinny_n_cu(), ks, ksteps, grid_x)) return EILEV_E_UNSUPPORTED;
    const int64_t chunks = n * (k >> 3);
    hipLaunchKernelGGL(stream_pack_kernel, dim3((unsigned)((chunks + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const bf16 *)w, (bf16 *)out, (int)n, (int)k, grid_x);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}

int launch_gemm(const GemmArgs &g, int prof_kind, hipStream_t s) {
    bool ln_done = false;
    // ln_out that neither the fused reduce nor a LayerNorm launch (norm.hip: cols % 8 == 0, cols <= 4096, ldx % 8 == 0) can write is refused
    // HERE: refused after the GEMM, the launch had written C (and the split-K planes) and then returned an error
    if (g.ln_out && g.M > 0 && (g.out_f32 || g.patch_group || (g.N & 7) || g.N > 4096 || (g.ldc & 7))) return EILEV_E_UNSUPPORTED;
    const int rc = launch_gemm_core(g, prof_kind, s, &ln_done);
    if (rc != EILEV_OK || !g.ln_out || ln_done || g.M <= 0) return rc;
    if (g.out_f32 || g.patch_group) return EILEV_E_UNSUPPORTED;
    if (!g.ln_beta) return launch_rmsnorm(reinterpret_cast<const bf16 *>(g.C), g.ldc, g.ln_gamma, g.ln_out, g.N, g.M, g.N, g.ln_eps, s);  // T5: RMS
    return launch_layernorm(reinterpret_cast<const bf16 *>(g.C), g.ldc, g.ln_gamma, g.ln_beta, g.ln_out, g.N, g.M, g.N, g.ln_eps, s);
}

static int launch_gemm_core(const GemmArgs &g_in, int prof_kind, hipStream_t s, bool *ln_done) {
    GemmArgs g = with_probes(g_in);
    if (g.M <= 0) return EILEV_OK;
    if (g.A8) return launch_a8w8(g, prof_kind, s);
    if (g.W8) {
        const int rc = w8_check(g);
        if (rc != EILEV_OK) return rc;
        if (!w8_streams(g)) {  // expanded, then this launch again on the bf16 copy
            const int rc_x = w8_expand(g, s);
            if (rc_x != EILEV_OK) return rc_x;
            GEMM_FORM_BIT(GEMM_FORM_W8_EXPANDED);
            GemmArgs e = g_in;
            e.W = g.w8_scratch;
            e.W8 = nullptr;
            return launch_gemm_core(e, prof_kind, s, ln_done);
        }
        g.W = reinterpret_cast<const bf16 *>(g.W8);  // (never dereferenced as bf16: the skinny fp8 kernel reads W8)
    }
    const int rc = check_args(g);
    if (rc != EILEV_OK) return rc;
    if (skinny_takes(g)) return launch_skinny(g, s, ln_done);
    if (const int64_t rows = chunk_rows(g)) return launch_row_chunks(g_in, rows, prof_kind, s);
    return profiled(ln_fold(g) ? launch_pp4 : launch_wide, g, prof_kind, s);
}

#ifdef EILEV_PROBES
// probe / test entry (tests/test_hip_gemm_wide.py): ONE launch_gemm on the caller's buffers.  The struct is GemmArgs field by field as plain
// pointers and integers, without dbg, trace, trace_tiles and k_slice (the ctypes mirror lives with the tests); struct_bytes must be its
// size, so a stale mirror is refused instead of run.  *form receives the code of the kernel instance that was launched (common.h
// GEMM_FORM; 0: none).  eilev_debug_gemm_flags applies as to every launch.
struct EilevDebugGemmArgs {
    const void *A; int64_t lda;
    const void *W; int64_t ldw;
    const void *bias, *resid; int64_t ldr;
    void *C; int64_t ldc;
    int32_t M, N, K, epi, out_f32;
    float scale;
    int32_t scale_cols, patch_group, hm_tok, hm_heads, hm_hd, pad0;
    const float *wscale;
    const void *W8;
    void *w8_scratch;
    const void *A8;
    const float *ascale, *ln_rows, *ln_csum;
    float *stat_out; int64_t stat_ld;
    const void *ln_gamma, *ln_beta;
    void *ln_out;
    float ln_eps;
    int32_t pad1;
};
static GemmArgs debug_gemm_args(const EilevDebugGemmArgs *args) {
    GemmArgs g = {};
    g.A = (const bf16 *)args->A; g.lda = args->lda; g.W = (const bf16 *)args->W; g.ldw = args->ldw;
    g.bias = (const bf16 *)args->bias; g.resid = (const bf16 *)args->resid; g.ldr = args->ldr; g.C = args->C; g.ldc = args->ldc;
    g.M = args->M; g.N = args->N; g.K = args->K; g.epi = args->epi; g.out_f32 = args->out_f32;
    g.scale = args->scale; g.scale_cols = args->scale_cols; g.patch_group = args->patch_group;
    g.hm_tok = args->hm_tok; g.hm_heads = args->hm_heads; g.hm_hd = args->hm_hd;
    g.wscale = args->wscale; g.W8 = (const uint8_t *)args->W8; g.w8_scratch = (bf16 *)args->w8_scratch;
    g.A8 = (const uint8_t *)args->A8; g.ascale = args->ascale; g.ln_rows = args->ln_rows; g.ln_csum = args->ln_csum;
    g.stat_out = args->stat_out; g.stat_ld = args->stat_ld;
    g.ln_gamma = (const bf16 *)args->ln_gamma; g.ln_beta = (const bf16 *)args->ln_beta; g.ln_out = (bf16 *)args->ln_out; g.ln_eps = args->ln_eps;
    return g;
}
extern "C" int eilev_debug_gemm(const EilevDebugGemmArgs *args, size_t struct_bytes, int *form, void *stream) {
    if (!args || struct_bytes != sizeof(EilevDebugGemmArgs)) return EILEV_E_BADARG;
    const GemmArgs g = debug_gemm_args(args);
    g_gemm_form = 0;
    const int rc = launch_gemm(g, -1, (hipStream_t)stream);
    if (form) *form = g_gemm_form;
    return rc;
}
// The same for the M <= 32 family (tests/test_hip_gemm_skinny.py): the struct above followed by what only a decode launch passes — the
// split-K scratch, the stream-layout copy of W and the three row-block layout switches.  *ks receives the K slices of the launch (0: none).
struct EilevDebugSkinnyArgs {
    EilevDebugGemmArgs g;
    void *scratch; uint64_t scratch_bytes;
    const void *Wp;
    int32_t a_frag, c_frag, ln_frag, pad2;
};
extern "C" int eilev_debug_gemm_skinny(const EilevDebugSkinnyArgs *args, size_t struct_bytes, int *form, int *ks, void *stream) {
    if (!args || struct_bytes != sizeof(EilevDebugSkinnyArgs)) return EILEV_E_BADARG;
    GemmArgs g = debug_gemm_args(&args->g);
    g.scratch = (float *)args->scratch; g.scratch_bytes = (size_t)args->scratch_bytes; g.Wp = (const bf16 *)args->Wp;
    g.a_frag = args->a_frag; g.c_frag = args->c_frag; g.ln_frag = args->ln_frag;
    g_gemm_form = 0;
    g_gemm_ks = 0;
    const int rc = launch_gemm(g, -1, (hipStream_t)stream);
    if (form) *form = g_gemm_form;
    if (ks) *ks = g_gemm_ks;
    return rc;
}
#endif

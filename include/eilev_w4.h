/*
 * eilev_w4.h — C ABI of the int4 weight-only companion library (eilev_amd/csrc/libeilev_hip_w4.so, gfx950).
 *
 * At one to a few rows a decode step streams the weights of the language model's linears and little else.  This library reads the four
 * linears of every OPT block from 4-bit codes with one bf16 scale per group of 128 weights: a quarter of the bf16 bytes (+ 1 / 64 for the
 * scales).  Embeddings, the tied lm_head, LayerNorms and biases stay bf16.
 *
 * Same conventions as eilev.h: C ABI, DEVICE pointers, caller-owned buffers, a hipStream_t `stream`, no allocation, no synchronisation
 * (every launching call may be captured); 0 on success, EILEV_E_BADARG / EILEV_E_UNSUPPORTED / EILEV_E_WORKSPACE (negative), a positive
 * value = hipError_t; bad or null arguments are refused before any launch.  EilevDims / EilevOptWeights are those of eilev.h.
 *
 * Like libeilev_hip_kv8.so this library needs the core library's attention, norms, lm_head GEMM and glue kernels, so it CARRIES ITS OWN COPY
 * OF THE CORE LIBRARY'S CODE (linked from the same objects; only the eilev_w4_* symbols are exported).  It does not link libeilev_hip.so
 * and shares no state with it; its copy of the timing recorder behind eilev_prof_* stays off.
 *
 * THE WEIGHT FORMAT of a matrix W [N][K] (row-major, K a multiple of 256 = EILEV_W4_KTILE)
 *   Quantiser (eilev_amd/quant.py quantize_int4; the library only READS the format): per (row n, group g of EILEV_W4_GROUP = 128 consecutive
 *             k) amax = max |w| in fp32, s = bf16_rne(amax / 7) (an all-zero group: s = 1), q = clamp(round_half_even(w / float(s)), -8, 7).
 *   Scales:   [N][K / 128] bf16, row-major.
 *   Codes:    u = q + 8 (0 .. 15; code 0 = -8 is legal).  [N][K / 8] little-endian 32-bit words, row-major: word j of a row holds the eight
 *             weights k = 8 j .. 8 j + 7, the weight 8 j + e in bits [4 p, 4 p + 4) with p = (e & 1) * 4 + (e >> 1) — the even weights in the
 *             low half-word, the odd ones in the high half-word, so that (word >> 4 i) & 0x000f000f is the pair (8 j + 2 i, 8 j + 2 i + 1).
 *             As bytes [N][K / 2]: byte 4 j + b holds weight 8 j + 4 (b & 1) + (b >> 1) in its low and weight 8 j + 4 (b & 1) + (b >> 1) + 2
 *             in its high nibble.
 *   Meaning:  the matrix a quantised linear multiplies by is W' = bf16_rne(float(q) * float(s)) — q * s is exact in fp32 (4 x 8 bits), so W'
 *             is one rounding and a plain bf16 matrix, the TWIN.  Every kernel here forms exactly the bits of W' in registers (0x4300 | u is
 *             the bf16 128 + u; (float(128 + u) - 136) * s is exact; v_cvt_pk_bf16_f32 rounds) and multiplies bf16 operands on the bf16 MFMA
 *             with fp32 accumulation: a result is that of a bf16 linear over W', up to the order of the fp32 sums.
 *
 * THE KERNEL (w4_skinny_kernel): 16 weight rows per workgroup, its K range dealt over four waves in tiles of 256 (128 bytes per row), every
 * tile of a wave (at most EILEV_W4_WAVE_TILES = 3, all requested before the first is used) brought into XOR-swizzled LDS by 16-byte LDS-DMA
 * pieces, the wave's scales loaded before them; MB = 1 (rows <= 16) or 2 (<= 32) activation tiles share a weight fragment.  The four waves'
 * partials meet in LDS in a fixed order.  K split over gridDim.y where the matrix has few 16-row blocks or a wave would own more than three
 * tiles: fp32 partials [ks][16 MB][N] in `scratch`, summed (in split order) by a second launch that also writes the LayerNorm rows.
 */
#ifndef EILEV_W4_H
#define EILEV_W4_H

#include <stddef.h>
#include <stdint.h>

#include "eilev.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EILEV_W4_ABI_VERSION 1
#define EILEV_W4_GROUP 128    /* weights per scale */
#define EILEV_W4_KTILE 256    /* K is a multiple of this */
#define EILEV_W4_MAX_ROWS 32  /* activation rows of one linear, rows of one decode step */
#define EILEV_W4_WAVE_TILES 3 /* K tiles of 256 a wave owns at most */

/* One quantised matrix: the codes and the scales of THE WEIGHT FORMAT, both 16-byte aligned. */
typedef struct EilevW4Matrix {
    const void *w4;     /* [N][K / 8] uint32 */
    const void *scales; /* [N][K / 128] bf16 */
} EilevW4Matrix;

/* The four linears of one OPT block; q | k | v is ONE [3 D][D] matrix (its bias: q_b, k_b, v_b of EilevOptLayer back to back). */
typedef struct EilevW4Layer {
    EilevW4Matrix qkv, o, fc1, fc2;
} EilevW4Layer;

/* eilev_w4_linear: C = epilogue((A . W'^T) + bias) (+ resid), M <= EILEV_W4_MAX_ROWS rows.
 *   v = sum_k A[m][k] W'[n][k] (fp32);  v += bias[n];  columns n < scale_cols: v *= scale;  relu: v = max(v, 0);  v += resid[m][n];
 *   C[m][n] = out_f32 ? v : bf16(v).  resid may be C (in place).
 *   ln_out (nullable; bf16 output only, N a multiple of 8, N <= 4096): ln_out[m] = LayerNorm(C[m]) * ln_gamma + ln_beta over the ROUNDED bf16
 *   row of C, leading dimension N — written by the launch that sums the split-K partials, or by a LayerNorm launch after an unsplit one. */
typedef struct EilevW4Linear {
    const void *a;      /* [M][K] bf16, leading dimension lda (a multiple of 8), 16-byte aligned */
    int64_t lda;
    EilevW4Matrix w;
    const void *bias;   /* [N] bf16 or NULL */
    const void *resid;  /* [M][N] bf16, leading dimension ldr, or NULL */
    int64_t ldr;
    void *c;            /* [M][N] bf16 or fp32, leading dimension ldc */
    int64_t ldc;
    int64_t m, n, k;
    int32_t relu, out_f32;
    float scale;
    int32_t scale_cols;
    const void *ln_gamma, *ln_beta; /* [N] bf16 (both, with ln_out) */
    void *ln_out;
    float ln_eps;
    void *scratch;      /* fp32 split-K partials: eilev_w4_linear_scratch_bytes(m, n, k) bytes (may be NULL when that is 0) */
    size_t scratch_bytes;
} EilevW4Linear;

int eilev_w4_abi_version(void);

/* W' of THE WEIGHT FORMAT into out_bf16 [n][k] (row-major, 16-byte aligned; may be the storage of the matrix that was quantised).
 * k a multiple of 128 (whole groups: the one call that takes a K that is not a multiple of 256). */
int eilev_w4_expand(const void *w4, const void *scales, int64_t n, int64_t k, void *out_bf16, void *stream);

/* Host only, launches nothing: the form eilev_w4_linear takes for (m, n, k).  form[0] = MB (1: m <= 16, 2: m <= 32), form[1] = K splits
 * (1: the epilogue runs in the kernel; more: partials + the reducing launch), form[2] / form[3] = the grid (16-row blocks, K splits),
 * form[4] = tiles of 256 per wave.  EILEV_E_BADARG: m outside 1 .. 32, n < 1, k < 1 or form NULL; EILEV_E_UNSUPPORTED: k not a multiple
 * of 256 or beyond 2^20, n beyond 2^24. */
int eilev_w4_plan(int64_t m, int64_t n, int64_t k, int32_t *form);

/* Bytes of EilevW4Linear.scratch (0: an unsplit form, or a shape eilev_w4_plan refuses). */
size_t eilev_w4_linear_scratch_bytes(int64_t m, int64_t n, int64_t k);

int eilev_w4_linear(const EilevW4Linear *l, void *stream);

/* Bytes of `workspace` for eilev_w4_decode_step on `batch` rows (0 for arguments it refuses). */
size_t eilev_w4_workspace_bytes(const EilevDims *d, int64_t batch);

/* One whole OPT decode step, its greedy selection included: the arguments and the contract of eilev_opt_decode_step (eilev.h; bf16 KV cache
 * of capacity kv_capacity), plus `layers`: HOST array of d->t_layers entries (device pointers inside).  The four linears of every block run
 * on the int4 kernel; embedding, LayerNorm, attention, lm_head and selection are the core library's, on row-major activations.  Every
 * per-step quantity is read from `state` on the device, so one captured step replays.  batch <= EILEV_W4_MAX_ROWS; t_hidden and t_ffn
 * multiples of 256, t_hidden <= 4096 (EILEV_E_UNSUPPORTED otherwise, before any launch). */
int eilev_w4_decode_step(const EilevDims *d, const EilevOptWeights *w, const EilevW4Layer *layers, int64_t *tokens, int32_t *state,
                         const int32_t *attn_mask, const int32_t *n_valid, int64_t batch, int64_t seq_len, void *kv_cache, int64_t kv_capacity,
                         float *logits, uint8_t *finished, int64_t eos_id, int64_t pad_id, int64_t *out_tokens, int64_t max_new, void *workspace,
                         size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* EILEV_W4_H */

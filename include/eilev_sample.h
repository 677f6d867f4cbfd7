/*
 * eilev_sample.h — C ABI of the device-sampling companion library (eilev_amd/csrc/libeilev_hip_sample.so, gfx950).
 *
 * generate(do_sample=True, num_beams=1) [hf generation/utils.py `_sample`]: the per-token work between two decode steps — the
 * repetition penalty, the minimum length, the temperature / top-k / top-p warpers and the multinomial draw — as ONE launch per row
 * (+ a 64-thread finalize for more than one row), so that the whole step replays from a captured hipGraph.  The core library
 * (include/eilev.h) runs the model: eilev_opt_decode_step / eilev_t5_decode_step produce the logits this library draws from.
 *
 * Same conventions as eilev.h: C ABI, DEVICE pointers, caller-owned buffers, a hipStream_t `stream`, no allocation, no
 * synchronisation; 0 on success, EILEV_E_BADARG / EILEV_E_UNSUPPORTED / EILEV_E_WORKSPACE (negative), a positive value = hipError_t.
 * The library is standalone: it does not link against libeilev_hip.so.  Its CPU restatement is eilev_amd/sampling.py
 * (`sample_select_reference`, `keep_bounds`, `draw_ok`).
 *
 * eilev_sample_select is eilev_greedy_select with a draw in place of the arg-max; it keeps that call's device state:
 *   state   (int32 [2])          [0] the step counter, [1] 1 while any row is unfinished, else 0 (always written);
 *   finished (uint8 [rows])      a row that drew any of the EOS ids becomes finished; finished rows emit pad_id;
 *   tokens  (int64 [rows])       the ids to feed to the next decode step;
 *   out_tokens (int64 [rows, max_new])  out_tokens[b * max_new + step] = the id of this step.
 * step = state[0] + step_offset; with `finalize` the call sets state[0] = step + 1.  (After eilev_opt_decode_step, whose built-in
 * selection has already advanced state[0]: step_offset = -1, finalize = 0.  On its own: step_offset = 0, finalize = 1.)
 *
 * Per row, in hf's order:
 *  1. repetition penalty (RepetitionPenaltyLogitsProcessor): for every DISTINCT id of the row's history — prefix_id if >= 0, then
 *     out_tokens[b, 0 .. step) — x = x < 0 ? x * penalty : x / penalty, computed from the unpenalised value;
 *  2. min_new: the EOS logits are -inf while step < min_new;
 *  3. temperature: x / temperature (fp32 division);
 *  4. top-k: keep x >= (k-th largest); ties of the k-th are kept;
 *  5. top-p (TopPLogitsWarper), with probabilities over what top-k left: token i is removed iff the mass of the tokens not larger than
 *     it, itself and its ties included, is <= 1 - top_p; the largest token always stays; equal values are kept or removed together;
 *  6. the draw, by inverse CDF in token-id order: u = uniforms[step * rows + b] in [0, 1); the lowest id whose inclusive prefix sum of
 *     kept probabilities exceeds u * total; if none does, the last kept id.
 * NaN logits count as -inf.  A row without a finite logit draws id 0.
 *
 * Arithmetic: probabilities are exp(x - max) in fp32, then held as 40-bit fixed point (floor(p * 2^40), 64-bit sums).  Integer sums
 * do not depend on the order of their terms, so every threshold and every draw is reproducible bit for bit, and a partial mass differs
 * from its exact value only by the rounding of x - max, of expf and of the 2^-40 quantisation (see tests/test_hip_device_sampling.py
 * for the bound).  The thresholds come from a radix select over the order-preserving integer image of the floats; nothing is sorted.
 */
#ifndef EILEV_SAMPLE_H
#define EILEV_SAMPLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EILEV_SAMPLE_ABI_VERSION 1
#define EILEV_SAMPLE_MAX_EOS 8
#define EILEV_SAMPLE_MAX_VOCAB 65536

typedef struct EilevSampleParams {
    float temperature;          /* > 0 */
    float top_p;                /* (0, 1]; 1 = off */
    float repetition_penalty;   /* > 0; 1 = off */
    int32_t top_k;              /* 0 = off */
    int64_t min_new;            /* EOS is banned while step < min_new */
    int64_t max_new;            /* row stride of out_tokens and of the history */
    int64_t n_eos;              /* 0 .. EILEV_SAMPLE_MAX_EOS */
    int64_t eos[EILEV_SAMPLE_MAX_EOS];
    int64_t pad_id;
    int64_t prefix_id;          /* < 0 = none; flan-t5's decoder start token, which hf's processors see in front of the generated ids */
    int32_t step_offset;        /* 0 or -1 */
    int32_t finalize;           /* 0 or 1 */
} EilevSampleParams;

int eilev_sample_abi_version(void);

/* Bytes of `scratch` for eilev_sample_select.  The kernels keep every intermediate in registers and LDS: 0 today (scratch may then
 * be NULL); callers size the buffer with this call so that a later version can use one. */
size_t eilev_sample_scratch_bytes(int64_t rows, int64_t vocab);

/* logits (rows, vocab) f32, 16-byte aligned; vocab <= EILEV_SAMPLE_MAX_VOCAB and vocab % 4 == 0, else EILEV_E_UNSUPPORTED.
 * uniforms (max_new, rows) f32 in [0, 1).  warped: NULL, or (rows, vocab) f32 that receives the scores after step 5 (-inf where a token
 * was removed) — for tests and tools.  One 1024-thread workgroup per row; rows > 1: + one 64-thread launch that writes `state`. */
int eilev_sample_select(const EilevSampleParams *p, const float *logits, int64_t rows, int64_t vocab, const float *uniforms, int32_t *state,
                        uint8_t *finished, int64_t *tokens, int64_t *out_tokens, float *warped, void *scratch, size_t scratch_bytes,
                        void *stream);

#ifdef __cplusplus
}
#endif

#endif /* EILEV_SAMPLE_H */

/*
 * eilev_t5beam.h — C ABI of the flan-t5 beam-search companion library (eilev_amd/csrc/libeilev_hip_t5beam.so, gfx950).
 *
 * generate(num_beams = k) for the encoder-decoder language model WITHOUT moving or replicating a cache: one decode step on all beam rows
 * whose layout mirrors eilev_opt_decode_step_beam (include/eilev.h), so that eilev_topk_logprob / eilev_rules_topk_logprob and
 * eilev_beam_advance drive it unchanged, the whole step capturable into one hipGraph.
 *
 * Same conventions as eilev.h: C ABI, DEVICE pointers, caller-owned buffers, a hipStream_t `stream`, no allocation, no synchronisation
 * (every call may be captured); 0 on success, EILEV_E_BADARG / EILEV_E_UNSUPPORTED / EILEV_E_WORKSPACE (negative), a positive value =
 * hipError_t; bad or null arguments are refused before any launch.  EilevT5Dims / EilevT5Weights are those of eilev.h.
 *
 * Unlike the other companions this library needs the decoder's GEMVs, norms and attention launchers, so it CARRIES ITS OWN COPY OF THE
 * CORE LIBRARY'S CODE (linked from the same objects; only the eilev_t5beam_* symbols are exported).  It does not link libeilev_hip.so and
 * shares no state with it.  The copy's one process-global, the timing recorder behind eilev_prof_*, is a SEPARATE INSTANCE that stays
 * off: the steps of this library never show up in eilev_prof_collect of the core library.
 *
 * Layout.  Row r is beam r % beams of sample r / beams; rows = samples * beams <= 32 per call.
 *  - Self-attention keys.  The decoder start token plays the part of OPT's prompt: its K / V live in `self_kv_start`, a cache
 *    [dec_layers][k | v][samples][heads][1][d_kv] — what eilev_t5_decode fills with batch = samples, new_len = 1, past_len = 0,
 *    kv_capacity = 1 (that call also returns the first logits).  The g-th generated token of a hypothesis lives in slot g of
 *    `self_kv_gen`, [dec_layers][k | v][rows][heads][gen_capacity][d_kv] (eilev_t5_self_kv_bytes(d, rows, gen_capacity) bytes), in row
 *    ancestors[g * rows + r] for the hypothesis now in row r; the token fed by this call goes to row r's own slot state[0] - 1.
 *  - state[0] = generated tokens fed, INCLUDING this call's: preset to 1, incremented by the call.  It is also the decoder position of the
 *    query (the start token is position 0).  A value outside 1 .. gen_capacity writes nowhere.
 *  - Cross-attention.  `cross_kv` is what eilev_t5_cross_kv writes for the SAMPLES (never replicated to the beams); enc_mask is
 *    (samples, enc_len) int32.  A sample's K and V are read from memory once per (sample, head, 128-key range) for all of its beams.
 * Head size d_kv = 64 only (EILEV_E_UNSUPPORTED otherwise).
 */
#ifndef EILEV_T5BEAM_H
#define EILEV_T5BEAM_H

#include <stddef.h>
#include <stdint.h>

#include "eilev.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EILEV_T5BEAM_ABI_VERSION 1

int eilev_t5beam_abi_version(void);

/* Bytes of `workspace` for eilev_t5beam_decode_step. */
size_t eilev_t5beam_workspace_bytes(const EilevT5Dims *d, int64_t rows, int64_t beams, int64_t enc_len, int64_t gen_capacity);

/* One decode step of beam search on `rows` rows (see the layout above).  tokens (rows) int64: the ids to feed; logits (rows, vocab) f32.
 * beams must divide rows; rows <= 32, beams <= 32. */
int eilev_t5beam_decode_step(const EilevT5Dims *d, const EilevT5Weights *w, const int64_t *tokens, int32_t *state, const int32_t *enc_mask,
                             int64_t rows, int64_t beams, const void *self_kv_start, void *self_kv_gen, int64_t gen_capacity,
                             const int32_t *ancestors, const void *cross_kv, int64_t enc_len, float *logits, void *workspace,
                             size_t workspace_bytes, void *stream);

/* The building block alone: the cross-attention of `rows` query rows q (bf16, row stride ldq elements, head h at columns h * hd ..) of
 * which every `beams` consecutive rows share one sample's keys / values kc / vc — bf16 planes [rows / beams][heads][cap][hd], 16-byte
 * aligned, keys [0, enc_len) — under enc_mask (rows / beams, enc_len) int32, NULL = every key visible.  softmax(q . k) . v with no scale
 * factor and no bias, P rounded to bf16 for the product, a row with no visible key gives zeros; out (rows, heads * hd) bf16.  Slots in
 * [enc_len, cap) and masked keys never reach a result.  part: (max, sum, o[hd]) f32 records per (row, head, 128-key range),
 * part_bytes >= 4 * rows * heads * ceil(enc_len / 128) * (hd + 2).  hd != 64: EILEV_E_UNSUPPORTED. */
int eilev_t5beam_cross_attention(const void *q, int64_t ldq, const void *kc, const void *vc, const int32_t *enc_mask, int64_t rows, int64_t beams,
                                 int64_t heads, int64_t hd, int64_t enc_len, int64_t cap, void *out, void *part, size_t part_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* EILEV_T5BEAM_H */

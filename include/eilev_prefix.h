/*
 * eilev_prefix.h — C ABI of the shared-prefix companion library (eilev_amd/csrc/libeilev_hip_prefix.so, gfx950).
 *
 * EILeV is an in-context learner: many queries (generate rows, classify() classes) follow ONE leading part — the example clips and their
 * texts.  This library runs `rows` rows of `new_len` new positions each through the OPT blocks as continuations of one prefix of
 * `prefix_len` positions whose keys / values are stored ONCE: no per-row copy of the prefix cache is made or read.
 *
 * Same conventions as eilev.h: C ABI, DEVICE pointers, caller-owned buffers, a hipStream_t `stream`, no allocation, no synchronisation
 * (every call may be captured); 0 on success, EILEV_E_BADARG / EILEV_E_UNSUPPORTED / EILEV_E_WORKSPACE (negative), a positive value =
 * hipError_t; bad or null arguments are refused before any launch.  EilevDims / EilevOptWeights are those of eilev.h.
 *
 * Like libeilev_hip_t5beam.so this library needs the core library's GEMMs, norms and glue kernels, so it CARRIES ITS OWN COPY OF THE CORE
 * LIBRARY'S CODE (linked from the same objects; only the eilev_prefix_* symbols are exported).  It does not link libeilev_hip.so and shares
 * no state with it; its copy of the timing recorder behind eilev_prof_* stays off.
 *
 * Visibility.  Query t of row r (position prefix_len + t) sees every prefix key 0 .. prefix_len - 1 and the new keys (r, t') with t' <= t;
 * no other row's new keys and no prefix slot at or beyond prefix_len.
 *
 * Arithmetic: that of the prefill kernels (attn_prefill_kernel): scores in fp32, P rounded to bf16 for the second product, the row sum
 * from the unrounded P, O / l rounded to bf16 once; `scale` multiplies q . k (the OPT path passes 1: q is pre-scaled).
 *
 * Limits of one call (chunk above them): rows <= EILEV_PREFIX_MAX_ROWS, new_len <= EILEV_PREFIX_MAX_NEW,
 * rows * new_len <= EILEV_PREFIX_MAX_STACKED.  Head sizes 80 and 128 (EILEV_E_UNSUPPORTED otherwise).
 *
 * Decoding after eilev_prefix_extend: with kv_rows as the generation cache, eilev_opt_decode_step_beam (eilev.h) continues the rows as `rows`
 * beams of one sample whose prompt cache is kv_prefix, its counter word preset to new_len + 1 and an identity ancestor table — the new
 * positions in slots [0, new_len) are to it new_len tokens already generated.  That step reads the prompt keys once PER ROW.
 *
 * Shared prompt reads (ABI 2): eilev_prefix_decode_step is the same step — same arguments, same contract, capturable — whose attention
 * reads a sample's prompt keys ONCE for all its `beams` rows; OPT beam search (rows = samples x beams) and the rows after a context (one
 * sample, beams = rows) both end in it.  The attention of a block, per (row, head), is cut into
 *     prompt ranges of EILEV_PREFIX_DECODE_PROMPT_KEYS keys over [0, seq_len): one workgroup per (head, sample, range) stages the range's K / V
 *         once and scores all the sample's rows against them on the MFMA (the 64 x 64 tile of the prefill kernels, the rows as its queries);
 *     ranges of EILEV_PREFIX_DECODE_GEN_KEYS keys over the generated keys [seq_len, seq_len + gen_capacity): per row, through the ancestor
 *         table, exactly as eilev_opt_decode_step_beam addresses them;
 * each leaving an un-normalised (max, sum, o[head_dim]) record of head_dim + 2 floats, and one merge.  Arithmetic: that of every decode kernel —
 * no scale (q is pre-scaled), fp32 scores, P rounded to bf16 for the product, the row sum from the unrounded P, one rounding of O / l.
 * The result is not bit-identical to eilev_opt_decode_step_beam's: the two sum in different orders.
 */
#ifndef EILEV_PREFIX_H
#define EILEV_PREFIX_H

#include <stddef.h>
#include <stdint.h>

#include "eilev.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EILEV_PREFIX_ABI_VERSION 2
#define EILEV_PREFIX_MAX_ROWS 4096
#define EILEV_PREFIX_MAX_NEW 2048
#define EILEV_PREFIX_MAX_STACKED 65536
#define EILEV_PREFIX_DECODE_PROMPT_KEYS 128
#define EILEV_PREFIX_DECODE_GEN_KEYS 128
#define EILEV_PREFIX_DECODE_MAX_ROWS 32

int eilev_prefix_abi_version(void);

/* The attention kernel alone.  q, k_new, v_new: bf16 rows (rows * new_len of them, row r * new_len + t = position t of row r; row strides
 * ldq / ldk / ldv elements, multiples of 8, head h at columns h * head_dim ..) — the three may be columns of one q|k|v buffer.  k_prefix,
 * v_prefix: bf16 planes [heads][prefix_cap][head_dim], keys [0, prefix_len), 1 <= prefix_len <= prefix_cap; slots behind prefix_len never
 * reach a result.  out: (rows, new_len, heads * head_dim) bf16, dense.  Every pointer 16-byte aligned.  Nothing outside `out` is written. */
int eilev_prefix_attention(const void *q, int64_t ldq, const void *k_new, int64_t ldk, const void *v_new, int64_t ldv, const void *k_prefix,
                           const void *v_prefix, int64_t prefix_len, int64_t prefix_cap, int64_t rows, int64_t new_len, int64_t heads,
                           int64_t head_dim, float scale, void *out, void *stream);

/* Bytes of `workspace` for eilev_prefix_extend: the activations of rows * new_len positions — not of rows * (prefix_len + new_len), as
 * eilev_opt_extend needs.  0 for arguments eilev_prefix_extend refuses. */
size_t eilev_prefix_workspace_bytes(const EilevDims *d, int64_t rows, int64_t new_len);

/* inputs_embeds (rows, new_len, t_hidden) bf16 at positions prefix_len .. prefix_len + new_len - 1 of every row, through all OPT blocks.
 * kv_prefix: what eilev_opt_prefill wrote for ONE unpadded sequence of prefix_len tokens with kv_capacity == prefix_len (the contract of
 * kv_prompt in eilev_opt_decode_step_beam); read only.  kv_rows (nullable): a cache of eilev_opt_kv_cache_bytes(d, rows, rows_capacity)
 * bytes, rows_capacity >= new_len, whose slots [0, new_len) of every row receive the new keys / values; NULL: none are written (rows_capacity
 * is ignored).  logits_last (rows, vocab) f32: the last new position of every row; logits_all (rows, new_len, vocab) f32; each nullable,
 * not both.  prefix_len + new_len <= max_pos. */
int eilev_prefix_extend(const EilevDims *d, const EilevOptWeights *w, const void *inputs_embeds, int64_t rows, int64_t new_len,
                        const void *kv_prefix, int64_t prefix_len, void *kv_rows, int64_t rows_capacity, float *logits_last, float *logits_all,
                        void *workspace, size_t workspace_bytes, void *stream);

/* The attention of the shared-prompt decode step alone, on caller buffers.  Row b is beam b % beams of sample b / beams; rows % beams == 0,
 * rows <= EILEV_PREFIX_DECODE_MAX_ROWS.  qkv: `rows` bf16 rows q | k | v of this step (row stride ldq >= 3 * heads * head_dim elements, a
 * multiple of 8; q pre-scaled).  k_prompt, v_prompt: bf16 planes [rows / beams][heads][prompt_cap][head_dim], keys [0, seq_len), 1 <= seq_len
 * <= prompt_cap.  attn_mask: (rows / beams, seq_len) int32, prompt key j of a sample is visible iff its entry != 0; NULL: every one is.
 * state[0] (read on the device) = generated tokens INCLUDING this step's: kv_total = seq_len + min(state[0], gen_capacity).  k_gen, v_gen:
 * bf16 planes [rows][heads][gen_capacity][head_dim]; key seq_len + g of row b is slot g of row ancestors[g * rows + b] (an entry outside
 * [0, rows) is clamped, never an address).  Slot kv_total - 1 - seq_len of the row's OWN planes receives this step's k / v from the qkv row,
 * and that key is scored from the row; a state[0] of 0, or above gen_capacity, writes nothing.  Prompt slots at or beyond seq_len, masked
 * prompt keys and generation slots at or beyond state[0] never reach a result, whatever they hold.  A row that sees no key gives zeros.
 * out: (rows, heads * head_dim) bf16.  part: the records, part_bytes >= 4 * rows * heads * (ceil(seq_len / EILEV_PREFIX_DECODE_PROMPT_KEYS) +
 * ceil(gen_capacity / EILEV_PREFIX_DECODE_GEN_KEYS)) * (head_dim + 2), else EILEV_E_WORKSPACE.  Every pointer 16-byte aligned.  Writes: out,
 * part, and the one new slot per (row, head) of k_gen / v_gen. */
int eilev_prefix_decode_attention(const void *qkv, int64_t ldq, const void *k_prompt, const void *v_prompt, int64_t seq_len, int64_t prompt_cap,
                                  const int32_t *attn_mask, const int32_t *state, void *k_gen, void *v_gen, int64_t gen_capacity,
                                  const int32_t *ancestors, int64_t rows, int64_t beams, int64_t heads, int64_t head_dim, void *out, void *part,
                                  size_t part_bytes, void *stream);

/* Bytes of `workspace` for eilev_prefix_decode_step: eilev_opt_workspace_bytes(d, rows, 1) and, behind it, the records of every key range
 * (the step's own workspace carves 8 MB for partials, which the smaller ranges outgrow).  0 for arguments the step refuses. */
size_t eilev_prefix_decode_workspace_bytes(const EilevDims *d, int64_t rows, int64_t seq_len, int64_t gen_capacity);

/* eilev_opt_decode_step_beam (eilev.h) with the prompt reads shared: the same arguments with the same meaning, state[0] incremented at the
 * end, no allocation, no synchronisation.  workspace: eilev_prefix_decode_workspace_bytes(d, rows, seq_len, gen_capacity) bytes, 16-byte
 * aligned like kv_prompt and kv_gen.  Head sizes other than 80 / 128: EILEV_E_UNSUPPORTED; bad or null arguments are refused before any launch. */
int eilev_prefix_decode_step(const EilevDims *d, const EilevOptWeights *w, const int64_t *tokens, int32_t *state, const int32_t *attn_mask,
                             const int32_t *n_valid, int64_t rows, int64_t beams, int64_t seq_len, const void *kv_prompt, void *kv_gen,
                             int64_t gen_capacity, const int32_t *ancestors, float *logits, void *workspace, size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* EILEV_PREFIX_H */

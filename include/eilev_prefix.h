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
 * Decoding after eilev_prefix_extend needs no entry of this library: with kv_rows as the generation cache, eilev_opt_decode_step_beam
 * (eilev.h) continues the rows as `rows` beams of one sample whose prompt cache is kv_prefix, its counter word preset to new_len + 1 and an
 * identity ancestor table — the new positions in slots [0, new_len) are to it new_len tokens already generated.
 */
#ifndef EILEV_PREFIX_H
#define EILEV_PREFIX_H

#include <stddef.h>
#include <stdint.h>

#include "eilev.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EILEV_PREFIX_ABI_VERSION 1
#define EILEV_PREFIX_MAX_ROWS 4096
#define EILEV_PREFIX_MAX_NEW 2048
#define EILEV_PREFIX_MAX_STACKED 65536

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

#ifdef __cplusplus
}
#endif

#endif /* EILEV_PREFIX_H */

/*
 * eilev_kv8.h — C ABI of the fp8 KV-cache companion library (eilev_amd/csrc/libeilev_hip_kv8.so, gfx950).
 *
 * Decoding is bound by HBM bytes, and from a few rows on most of them are the KV cache.  This library keeps the cache of the OPT decode
 * step in OCP e4m3 bytes with one power-of-two scale per head vector: half the bytes of the bf16 cache (+ 1 / head_dim for the scales).
 *
 * Same conventions as eilev.h: C ABI, DEVICE pointers, caller-owned buffers, a hipStream_t `stream`, no allocation, no synchronisation
 * (every call may be captured); 0 on success, EILEV_E_BADARG / EILEV_E_UNSUPPORTED / EILEV_E_WORKSPACE (negative), a positive value =
 * hipError_t; bad or null arguments are refused before any launch.  EilevDims / EilevOptWeights are those of eilev.h.
 *
 * Like libeilev_hip_prefix.so this library needs the core library's GEMMs, norms and glue kernels, so it CARRIES ITS OWN COPY OF THE CORE
 * LIBRARY'S CODE (linked from the same objects; only the eilev_kv8_* symbols are exported).  It does not link libeilev_hip.so and shares
 * no state with it; its copy of the timing recorder behind eilev_prof_* stays off.
 *
 * THE CACHE FORMAT
 *   Elements: OCP e4m3 (torch.float8_e4m3fn; gfx950 is OCP, not fnuz), one byte each.
 *   Scales:   every vector of head_dim elements — one (layer, k | v, row, head, slot) — has ONE scale 2^e, stored as the e8m0 byte
 *             e + 127.  e is the smallest integer with amax <= 448 * 2^e, clamped to e >= -126 (amax = the largest magnitude of the
 *             vector).  amax == 0 or a non-finite amax stores byte 127 (e = 0); with a non-finite amax the element bytes are unspecified.
 *   Rounding: element byte = e4m3_rne(x * 2^-e).  The scaling by a power of two is exact, so there is exactly one rounding; in torch,
 *             (x.float() * 2.0 ** -e).to(torch.float8_e4m3fn) gives the same bits.
 *   Value:    dq = e4m3 * 2^e, which is exactly a bf16 value: an fp8 cache has an exact bf16 twin.
 *   Layout:   byte planes [layers][k | v][batch][heads][cap][head_dim] uint8 (the order of the bf16 cache of eilev.h), then, from the next
 *             256-byte boundary, the exponent planes [layers][k | v][batch][heads][cap] uint8.  eilev_kv8_cache_bytes is the total.
 *   Head sizes 80 and 128 (a vector is 5 or 8 sixteen-byte chunks); any other head size: EILEV_E_UNSUPPORTED before any launch.
 *
 * THE ATTENTION (attn_decode8_kernel: the flash-decoding split of the bf16 decode kernels over ranges of EILEV_KV8_RANGE keys, its partials
 * merged by the bf16 kernels' merge).  q is pre-scaled by head_dim^-0.5 (no scale is applied here).  With kv_total = min(cap, seq_len +
 * state[0]) (state == NULL: seq_len):
 *   s_j = (sum_d q_d * float(k8_jd)) * 2^ek_j in fp32; keys below seq_len obey attn_mask, newer keys are visible;
 *   p_j = exp(s_j - max), the row sum from the unrounded p;  o_d = sum_j (bf16(p_j) * 2^ev_j) * float(v8_jd) in fp32;  out = bf16(o / sum).
 * fuse_new: the newest key / value (slot kv_total - 1) is still only in the q|k|v row of the step.  The kernel quantises it into that slot
 * (bytes and exponents; nothing else of the cache is written) and, in THIS step, scores it from the bf16 row; later steps read the
 * quantised form.  A row with no visible key gives zeros.
 */
#ifndef EILEV_KV8_H
#define EILEV_KV8_H

#include <stddef.h>
#include <stdint.h>

#include "eilev.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EILEV_KV8_ABI_VERSION 1
#define EILEV_KV8_RANGE 256   /* keys per workgroup of the attention: its partials are per (row, head, range) */
#define EILEV_KV8_MAX_ROWS 32 /* rows of one decode step */

int eilev_kv8_abi_version(void);

/* Bytes of an fp8 cache of `batch` rows and `cap` slots (both planes, rounded up to 256).  0 for a head size other than 80 / 128 or
 * arguments that are not positive. */
size_t eilev_kv8_cache_bytes(const EilevDims *d, int64_t batch, int64_t cap);

/* Bytes of `workspace` for eilev_kv8_decode_step on `batch` rows (0 for arguments it refuses). */
size_t eilev_kv8_workspace_bytes(const EilevDims *d, int64_t batch);

/* Slots [0, slots) of every (layer, k | v, row, head) of a bf16 cache of capacity src_cap (what eilev_opt_prefill wrote) into the fp8 cache
 * kv8 of capacity dst_cap, bytes and exponents; slots at or beyond `slots` of kv8 are not written.  slots <= src_cap, slots <= dst_cap.
 * Both caches 16-byte aligned. */
int eilev_kv8_quantize(const EilevDims *d, const void *kv_bf16, int64_t batch, int64_t src_cap, int64_t slots, void *kv8, int64_t dst_cap,
                       void *stream);

/* ONE attention launch (+ the merge) over the planes of one layer.  qkv: bf16 rows of stride ldq elements (a multiple of 8), q of head h at
 * columns h * head_dim .., with fuse_new the step's k at heads * head_dim + h * head_dim and v at 2 * heads * head_dim + h * head_dim.
 * k8 / v8: byte planes [batch][heads][cap][head_dim], 16-byte aligned; ek / ev: exponent planes [batch][heads][cap].  attn_mask (batch,
 * seq_len) int32 or NULL (every key visible); state: device int32 words, state[0] read by the kernel, or NULL.  0 <= seq_len <= cap.
 * part: fp32 partials (max, sum, o[head_dim]) per (row, head, range of EILEV_KV8_RANGE keys of cap), part_bytes >= 4 * batch * heads *
 * ceil(cap / EILEV_KV8_RANGE) * (head_dim + 2) (EILEV_E_WORKSPACE otherwise).  out: [batch][heads * head_dim] bf16. */
int eilev_kv8_attention(const void *qkv, int64_t ldq, void *k8, void *v8, void *ek, void *ev, const int32_t *attn_mask, const int32_t *state,
                        int64_t batch, int64_t seq_len, int64_t cap, int64_t heads, int64_t head_dim, int fuse_new, float *part,
                        size_t part_bytes, void *out, void *stream);

/* One whole decode step, its greedy selection included: the arguments of eilev_opt_decode_step (eilev.h) with the fp8 cache kv8 (capacity
 * kv_capacity; slots [0, seq_len) quantised by eilev_kv8_quantize) in place of kv_cache.  Every per-step quantity is read from `state` on
 * the device, so one captured step replays.  batch <= EILEV_KV8_MAX_ROWS. */
int eilev_kv8_decode_step(const EilevDims *d, const EilevOptWeights *w, int64_t *tokens, int32_t *state, const int32_t *attn_mask,
                          const int32_t *n_valid, int64_t batch, int64_t seq_len, void *kv8, int64_t kv_capacity, float *logits,
                          uint8_t *finished, int64_t eos_id, int64_t pad_id, int64_t *out_tokens, int64_t max_new, void *workspace,
                          size_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* EILEV_KV8_H */

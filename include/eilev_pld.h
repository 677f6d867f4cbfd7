/*
 * eilev_pld.h — C ABI of the prompt-lookup decoding companion library (eilev_amd/csrc/libeilev_hip_pld.so, gfx950).
 *
 * generate(prompt_lookup_num_tokens=k, max_matching_ngram_size=n) at batch 1 (hf generation/candidate_generator.py
 * PromptLookupCandidateGenerator + generation/utils.py `_assisted_decoding` with greedy verification).  The core library
 * (include/eilev.h) runs the model: eilev_opt_extend / eilev_t5_decode verify a window [last committed id, d1 .. dm],
 * eilev_opt_decode_step / eilev_t5_decode_step serve the steps without a draft.  This library holds the per-step work around
 * them: finding the draft in the corpus, and accepting / committing the verified ids.
 *
 * Same conventions as eilev.h: C ABI, DEVICE pointers, caller-owned buffers, a hipStream_t `stream`, no allocation, no
 * synchronisation; 0 on success, EILEV_E_BADARG / EILEV_E_WORKSPACE (negative) for bad arguments, a positive value = hipError_t.
 * The library is standalone: it does not link against libeilev_hip.so.  Its CPU restatement is eilev_amd/pld.py.
 *
 * Device state of one generation (batch 1), all int64 ids:
 *   corpus  [corpus_cap]   the row's visible text ids (no left padding, no video placeholder), then every committed id;
 *   corpus_len (int32)     its length;
 *   window  [k + 1]        [0] the last committed id (= the decode steps' `tokens` buffer), [1 .. m] the draft;
 *   state   (int32 [2])    the decode step's counter: state[0] = committed count after every commit (state[1] = 1 - done);
 *   out     [max_new]      the generated ids;
 *   status  (int32 [4])    [0] committed count c, [1] draft length m, [2] done, [3] draft ids accepted by the last step.
 *                          The host reads this block back once per step; it sets it to zeros before the first call.
 */
#ifndef EILEV_PLD_H
#define EILEV_PLD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EILEV_PLD_ABI_VERSION 1
#define EILEV_PLD_MAX_K 64   /* prompt_lookup_num_tokens */
#define EILEV_PLD_MAX_EOS 8

typedef struct EilevPldParams {
    int64_t k;            /* prompt_lookup_num_tokens, 1 .. EILEV_PLD_MAX_K */
    int64_t ngram;        /* max_matching_ngram_size >= 1 */
    int64_t max_new;      /* max_new_tokens: the generated ids the call may commit */
    int64_t slot_base;    /* cache slot of generated id 1 (OPT: the prompt length L; flan-t5: 1, the start token holds slot 0) */
    int64_t slot_limit;   /* the verify window occupies slots slot_base + c - 1 .. slot_base + c - 1 + m, all below slot_limit
                             (OPT: min(kv_capacity, max_position_embeddings); flan-t5: kv_capacity) */
    int64_t corpus_cap;   /* capacity of `corpus` (text ids + max_new) */
    int64_t n_eos;        /* 0 .. EILEV_PLD_MAX_EOS */
    int64_t eos[EILEV_PLD_MAX_EOS];
} EilevPldParams;

int eilev_pld_abi_version(void);

/* Draft of the current corpus (status[0] = committed count c): for n = min(ngram, len - 1) .. 1 the first occurrence, left to
 * right, of the corpus's last n ids whose continuation corpus[idx + n : min(idx + n + k, len)] is non-empty; the continuation is cut
 * before its first EOS id, then capped at max_new - c - 1 ids and at slot_limit - slot_base - c ids.  Writes window[1 .. m] and
 * status[1] = m; status[0], [2], [3] stay.  One workgroup. */
int eilev_pld_draft(const EilevPldParams *p, const int64_t *corpus, const int32_t *corpus_len, int64_t *window, int32_t *status,
                    void *stream);

/* Scratch of eilev_pld_step: per-row partial arg-maxima. */
size_t eilev_pld_scratch_bytes(int64_t rows, int64_t vocab);

/* Accept, commit and the next draft, after the model ran the window [window[0], d1 .. dm] (rows = m + 1 = status[1] + 1 as the
 * previous call left it; rows = 1: a single decode step).  logits (rows, vocab) f32.
 *  - g_i = arg max of row i (ties: the lowest id, NaN never wins, a row without a number gives 0 — eilev_greedy_select's rule);
 *  - a = the longest prefix with g_i == d_(i+1); the ids d1 .. da, g_a are committed in order, up to and including the first EOS
 *    id and up to max_new ids in all: each goes to out[c], to the corpus and to window[0]; c += 1;
 *  - done = an EOS id was committed or c == max_new; state[0] = c, state[1] = !done;
 *  - then the draft of eilev_pld_draft (m = 0 when done); status = [c, m, done, a].
 * Two launches: a row-split arg-max over (rows x vocab / 4096) workgroups, then one workgroup for the rest. */
int eilev_pld_step(const EilevPldParams *p, const float *logits, int64_t rows, int64_t vocab, int64_t *corpus, int32_t *corpus_len,
                   int64_t *window, int32_t *state, int64_t *out, int32_t *status, void *scratch, size_t scratch_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* EILEV_PLD_H */

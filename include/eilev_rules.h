/*
 * eilev_rules.h — C ABI of the logits-rules companion library (eilev_amd/csrc/libeilev_hip_rules.so, gfx950).
 *
 * generate(do_sample=False) with `repetition_penalty`, `no_repeat_ngram_size`, `min_new_tokens` or several EOS ids: the rules a row's own
 * generated ids put on its next-token scores, applied on the device in front of the two deterministic selections — greedy search
 * (eilev_rules_select = eilev_greedy_select with the rules and up to 8 EOS ids) and beam search (eilev_rules_topk_logprob =
 * eilev_topk_logprob with the rules on the log-probabilities) — so that these calls replay from the same captured step as the plain
 * ones.  eilev_rules_ban is the n-gram ban alone, in place, for the step in front of eilev_sample_select (include/eilev_sample.h).
 *
 * Same conventions as eilev.h / eilev_sample.h: C ABI, DEVICE pointers, caller-owned buffers, a hipStream_t `stream`, no allocation,
 * no synchronisation (every call may be captured); parameters by value; 0 on success, EILEV_E_BADARG / EILEV_E_UNSUPPORTED /
 * EILEV_E_WORKSPACE (negative), a positive value = hipError_t.  The library is standalone: it links neither libeilev_hip.so nor
 * libeilev_hip_sample.so.  Its CPU restatement is eilev_amd/rules.py.
 *
 * The rules, per row, with the history h = [prefix_id if >= 0] + the row's ids of steps 0 .. step-1 (m = len(h)):
 *  - repetition penalty (hf RepetitionPenaltyLogitsProcessor): for every DISTINCT id of h, x = x < 0 ? x * penalty : x / penalty, from
 *    the unpenalised value (IEEE fp32 multiply and true division);
 *  - n-gram ban (hf NoRepeatNGramLogitsProcessor, size n): nothing if m + 1 < n; else for every i in 0 .. m-n with
 *    h[i .. i+n-2] == h[m-n+1 .. m-1], id h[i+n-1] becomes -inf (n = 1: every id of h);
 *  - min_new: the EOS ids are -inf while step < min_new.
 * NaN counts as -inf; -0 is +0; ids outside [0, vocab) in a history neither receive a penalty nor a ban (they still compare as ids
 * inside an n-gram).  The three rules commute.
 *
 * One 1024-thread workgroup per row; the row's <= 16 chunks of 16 bytes stay in registers, the penalised and the banned set are one bit
 * per id in LDS; the history is scanned by the workgroup, one thread per start position.  Every selection compares (value, id) pairs,
 * so the result does not depend on the order in which the workgroup combines them.
 */
#ifndef EILEV_RULES_H
#define EILEV_RULES_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EILEV_RULES_ABI_VERSION 1
#define EILEV_RULES_MAX_EOS 8
#define EILEV_RULES_MAX_VOCAB 65536
#define EILEV_RULES_MAX_KEEP 64

typedef struct EilevRulesParams {
    float repetition_penalty;   /* > 0; 1 = off */
    int32_t no_repeat_ngram;    /* >= 0; 0 = off */
    int64_t min_new;            /* EOS is banned while step < min_new */
    int64_t max_new;            /* row stride of the history (out_tokens / run_seq) */
    int64_t n_eos;              /* 0 .. EILEV_RULES_MAX_EOS */
    int64_t eos[EILEV_RULES_MAX_EOS];
    int64_t pad_id;
    int64_t prefix_id;          /* < 0 = none; flan-t5's decoder start token, which hf's processors see in front of the generated ids */
    int32_t step_offset;        /* 0 or -1 */
    int32_t finalize;           /* 0 or 1 (eilev_rules_select only) */
} EilevRulesParams;

int eilev_rules_abi_version(void);

/* Bytes of `scratch`: 0 today (scratch may then be NULL); callers size the buffer with this call. */
size_t eilev_rules_scratch_bytes(int64_t rows, int64_t vocab);

/* Greedy search.  logits (rows, vocab) f32, 16-byte aligned; vocab <= EILEV_RULES_MAX_VOCAB and vocab % 4 == 0, else EILEV_E_UNSUPPORTED.
 * state / finished / tokens / out_tokens: as eilev_sample_select — step = state[0] + step_offset, history of row b =
 * out_tokens[b * max_new + 0 .. step); the arg-max of the scores after the rules (equal maxima: the lowest id; a row whose maximum is
 * -inf: id 0) goes to tokens[b] and out_tokens[b * max_new + step]; finished rows emit pad_id; a row that picks any EOS id becomes
 * finished; state[1] = 1 while any row is unfinished; with `finalize`, state[0] = step + 1.  processed: NULL, or (rows, vocab) f32 that
 * receives the scores after the rules.  rows > 1: + one 64-thread launch that writes `state`. */
int eilev_rules_select(const EilevRulesParams *p, const float *logits, int64_t rows, int64_t vocab, int32_t *state, uint8_t *finished,
                       int64_t *tokens, int64_t *out_tokens, float *processed, void *scratch, size_t scratch_bytes, void *stream);

/* Beam search: per row the best `keep` (<= EILEV_RULES_MAX_KEEP) of rules(log_softmax(logits)) + row_score[row] — the log-softmax over
 * the logits as they are, exactly as eilev_topk_logprob evaluates it, THEN the rules (hf `_beam_search` hands its processors the
 * log-probabilities), then the row's running score (row_score may be NULL = 0).  History of row r = run_seq[r * max_new + 0 .. cur),
 * cur = state[0] - 1 + step_offset; the EOS ids are banned while cur < min_new.  out_val / out_idx (rows, keep) f32 / int32, descending,
 * equal values by ascending id — what eilev_beam_advance consumes.  processed: NULL, or (rows, vocab) f32 that receives the
 * log-probabilities after the rules (without row_score).  Nothing is written to state or run_seq. */
int eilev_rules_topk_logprob(const EilevRulesParams *p, const float *logits, const float *row_score, int64_t rows, int64_t vocab, int64_t keep,
                             const int32_t *state, const int64_t *run_seq, float *out_val, int32_t *out_idx, float *processed, void *scratch,
                             size_t scratch_bytes, void *stream);

/* The n-gram ban alone: logits[b, id] = -inf for every banned id of row b, everything else untouched.  step = state[0] + step_offset,
 * history as eilev_rules_select.  Launch it between the decode step and eilev_sample_select (hf applies the ban before the warpers). */
int eilev_rules_ban(const EilevRulesParams *p, float *logits, int64_t rows, int64_t vocab, const int32_t *state, const int64_t *out_tokens,
                    void *stream);

#ifdef __cplusplus
}
#endif

#endif /* EILEV_RULES_H */

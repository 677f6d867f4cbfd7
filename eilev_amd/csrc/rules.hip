// rules.hip — the logits rules of greedy and beam search on the device (include/eilev_rules.h): repetition penalty, n-gram ban, minimum
// length and several EOS ids in front of the arg-max (rules_select_kernel) and of the per-row top-`keep` of the log-probabilities
// (rules_topk_kernel); the n-gram ban alone for the sampling step (rules_ban_kernel).  Standalone library (libeilev_hip_rules.so): it
// links nothing of the core library.  Every step of the kernels is row_select.h's, shared with sample.hip and misc.hip
// topk_logprob_kernel; this file strings them together.
#include <climits>

#include "row_select.h"
#include "../../include/eilev_rules.h"

namespace {

static_assert(EILEV_RULES_MAX_VOCAB == kMaxVocab && EILEV_RULES_MAX_EOS == kMaxEos, "include/eilev_rules.h and row_select.h disagree");

__global__ __launch_bounds__(kThreads) void rules_select_kernel(EilevRulesParams p, const float *__restrict__ logits, int vocab, int32_t *__restrict__ state,
                                                                uint8_t *__restrict__ finished, int64_t *__restrict__ tokens,
                                                                int64_t *__restrict__ out_tokens, float *__restrict__ processed, int whole_step) {
    __shared__ uint32_t pen_bits[kBits], ban_bits[kBits];
    __shared__ float wv[16];
    __shared__ int wi[16];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int n4 = vocab >> 2;
    const int64_t step = (int64_t)state[0] + p.step_offset;
    fill_tables(p, out_tokens + (int64_t)b * p.max_new, step, p.no_repeat_ngram, vocab, tid, pen_bits, ban_bits);

    float4 e[kChunks];
    load_row(e, logits + (int64_t)b * vocab, n4, tid);
    apply_rules(e, pen_bits, ban_bits, p.repetition_penalty, 1.0f, tid);
    if (processed) store_row(e, processed + (int64_t)b * vocab, n4, tid);

    float best = -INFINITY;
    int bi = kNone;
#pragma unroll
    for (int j = 0; j < kChunks; ++j) {  // ascending ids within a thread: a strict > keeps the lowest id of equal values
        const float ev[4] = {e[j].x, e[j].y, e[j].z, e[j].w};
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (ev[u] > best) {
                best = ev[u];
                bi = (tid + kThreads * j) * 4 + u;
            }
    }
    block_best(best, bi, wv, wi, lane, wid);
    if (tid == 0) commit_token(p, bi == kNone ? 0 : bi, b, step, state, finished, tokens, out_tokens, whole_step);  // (kNone: no score above -inf)
}

__global__ __launch_bounds__(kThreads) void rules_topk_kernel(EilevRulesParams p, const float *__restrict__ logits, const float *__restrict__ row_score,
                                                              int vocab, int keep, const int32_t *__restrict__ state, const int64_t *__restrict__ run_seq,
                                                              float *__restrict__ out_val, int32_t *__restrict__ out_idx, float *__restrict__ processed) {
    __shared__ uint32_t pen_bits[kBits], ban_bits[kBits];
    __shared__ float wv[16];
    __shared__ int wi[16];
    __shared__ float bcast[2];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int n4 = vocab >> 2;
    const int64_t cur = (int64_t)state[0] - 1 + p.step_offset;
    fill_tables(p, run_seq + (int64_t)row * p.max_new, cur, p.no_repeat_ngram, vocab, tid, pen_bits, ban_bits);

    float4 e[kChunks];
    load_row(e, logits + (int64_t)row * vocab, n4, tid);
    // ---- log_softmax of the logits as they are, evaluated as topk_logprob_kernel (and torch) does
    float mx, lg;
    row_log_softmax(e, n4, wv, bcast, tid, lane, wid, mx, lg);
    const float sc = row_score ? row_score[row] : 0.0f;
#pragma unroll
    for (int j = 0; j < kChunks; ++j) e[j] = make_float4((e[j].x - mx) - lg, (e[j].y - mx) - lg, (e[j].z - mx) - lg, (e[j].w - mx) - lg);
    // ---- the rules act on the log-probabilities, then the running score
    apply_rules(e, pen_bits, ban_bits, p.repetition_penalty, 1.0f, tid);
    if (processed) store_row(e, processed + (int64_t)row * vocab, n4, tid);
#pragma unroll
    for (int j = 0; j < kChunks; ++j) e[j] = make_float4(e[j].x + sc, e[j].y + sc, e[j].z + sc, e[j].w + sc);
    topk_rounds(e, n4, keep, wv, wi, tid, lane, wid, [&](int k, float v, int ix) {
        out_val[(int64_t)row * keep + k] = v;
        out_idx[(int64_t)row * keep + k] = ix;
    });
}

// The ban alone: the thread that finds a repeated (n-1)-gram writes -inf itself (several may write the same word: the same value).
__global__ __launch_bounds__(kThreads) void rules_ban_kernel(EilevRulesParams p, float *__restrict__ logits, int vocab, const int32_t *__restrict__ state,
                                                             const int64_t *__restrict__ out_tokens) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t step = (int64_t)state[0] + p.step_offset;
    const int64_t nh = step < 0 ? 0 : (step < p.max_new ? step : p.max_new);
    float *row = logits + (int64_t)b * vocab;
    scan_history(
        out_tokens + (int64_t)b * p.max_new, nh, p.prefix_id, (int64_t)p.no_repeat_ngram, false, tid, [](int64_t) {},
        [&](int64_t id) {
            if (id >= 0 && id < vocab) row[id] = -INFINITY;
        });
}

bool params_ok(const EilevRulesParams *p) {
    return p->max_new >= 1 && p->max_new < INT_MAX && p->n_eos >= 0 && p->n_eos <= EILEV_RULES_MAX_EOS && p->repetition_penalty > 0.0f &&
           p->no_repeat_ngram >= 0 && p->step_offset >= -1 && p->step_offset <= 0 && (p->finalize == 0 || p->finalize == 1);
}

}  // namespace

extern "C" int eilev_rules_abi_version(void) { return EILEV_RULES_ABI_VERSION; }

extern "C" size_t eilev_rules_scratch_bytes(int64_t rows, int64_t vocab) {
    (void)rows;
    (void)vocab;
    return 0;
}

extern "C" int eilev_rules_select(const EilevRulesParams *p, const float *logits, int64_t rows, int64_t vocab, int32_t *state, uint8_t *finished,
                                  int64_t *tokens, int64_t *out_tokens, float *processed, void *scratch, size_t scratch_bytes, void *stream) {
    (void)scratch;
    if (!p || !logits || !state || !finished || !tokens || !out_tokens) return EILEV_E_BADARG;
    if (rows < 1 || rows >= INT_MAX || vocab < 1 || !params_ok(p)) return EILEV_E_BADARG;
    if (vocab > EILEV_RULES_MAX_VOCAB || (vocab & 3) || (((uintptr_t)logits) & 15) || (processed && (((uintptr_t)processed) & 15))) return EILEV_E_UNSUPPORTED;
    if (scratch_bytes < eilev_rules_scratch_bytes(rows, vocab)) return EILEV_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(rules_select_kernel, dim3((unsigned)rows), dim3(kThreads), 0, s, *p, logits, (int)vocab, state, finished, tokens, out_tokens,
                       processed, rows == 1 ? 1 : 0);
    EILEV_LAUNCH_CHECK();
    if (rows == 1) return EILEV_OK;  // (the single workgroup finished the step itself)
    hipLaunchKernelGGL(row_finalize_kernel<>, dim3(1), dim3(64), 0, s, state, (const uint8_t *)finished, (int)rows, (int)p->step_offset, (int)p->finalize);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}

extern "C" int eilev_rules_topk_logprob(const EilevRulesParams *p, const float *logits, const float *row_score, int64_t rows, int64_t vocab, int64_t keep,
                                        const int32_t *state, const int64_t *run_seq, float *out_val, int32_t *out_idx, float *processed, void *scratch,
                                        size_t scratch_bytes, void *stream) {
    (void)scratch;
    if (!p || !logits || !state || !run_seq || !out_val || !out_idx) return EILEV_E_BADARG;
    if (rows < 1 || rows >= INT_MAX || vocab < 1 || keep < 1 || keep > vocab || !params_ok(p)) return EILEV_E_BADARG;
    if (vocab > EILEV_RULES_MAX_VOCAB || (vocab & 3) || keep > EILEV_RULES_MAX_KEEP || (((uintptr_t)logits) & 15) ||
        (processed && (((uintptr_t)processed) & 15)))
        return EILEV_E_UNSUPPORTED;
    if (scratch_bytes < eilev_rules_scratch_bytes(rows, vocab)) return EILEV_E_WORKSPACE;
    hipLaunchKernelGGL(rules_topk_kernel, dim3((unsigned)rows), dim3(kThreads), 0, (hipStream_t)stream, *p, logits, row_score, (int)vocab, (int)keep, state,
                       run_seq, out_val, out_idx, processed);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}

extern "C" int eilev_rules_ban(const EilevRulesParams *p, float *logits, int64_t rows, int64_t vocab, const int32_t *state, const int64_t *out_tokens,
                               void *stream) {
    if (!p || !logits || !state || !out_tokens) return EILEV_E_BADARG;
    if (rows < 1 || rows >= INT_MAX || vocab < 1 || !params_ok(p)) return EILEV_E_BADARG;
    if (vocab > EILEV_RULES_MAX_VOCAB || (vocab & 3)) return EILEV_E_UNSUPPORTED;
    if (p->no_repeat_ngram == 0) return EILEV_OK;
    hipLaunchKernelGGL(rules_ban_kernel, dim3((unsigned)rows), dim3(kThreads), 0, (hipStream_t)stream, *p, logits, (int)vocab, state, out_tokens);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}

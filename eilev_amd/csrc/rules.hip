// rules.hip — the logits rules of greedy and beam search on the device (include/eilev_rules.h): repetition penalty, n-gram ban, minimum
// length and several EOS ids in front of the arg-max (rules_select_kernel) and of the per-row top-`keep` of the log-probabilities
// (rules_topk_kernel); the n-gram ban alone for the sampling step (rules_ban_kernel).  Standalone library (libeilev_hip_rules.so): it
// shares common.h's macros with the core library and nothing else.
//
// As sample.hip / misc.hip topk_logprob_kernel: one 1024-thread workgroup per row, the row's <= 16 chunks of 16 bytes in registers, the
// penalised and the banned set as one bit per id in LDS.  The history (<= max_new ids of the row, in global memory) is scanned by the
// workgroup: one thread per start position, n - 1 compares against the row's last n - 1 ids.  Every reduction compares (value, id), so
// its result does not depend on the order of its steps: a replayed graph gives the eager launch's bits.
#include <climits>

#include "common.h"
#include "../../include/eilev_rules.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kChunks = 16;                       // float4 chunks per thread: 1024 * 16 * 4 = 65536 = EILEV_RULES_MAX_VOCAB
constexpr int kBits = EILEV_RULES_MAX_VOCAB / 32;  // words of a one-bit-per-id table
constexpr int kNone = 0x7fffffff;

// The row's history h = [prefix if >= 0] + hist[0 .. nh): seen(id) for every id of h (want_seen), ban(id) for every id that would complete
// an n-gram already in h.  Ids are compared as they are; the callbacks drop those outside the vocabulary.
template <class Seen, class Ban>
__device__ __forceinline__ void scan_history(const int64_t *__restrict__ hist, int64_t nh, int64_t prefix, int64_t n, bool want_seen, int tid,
                                             Seen seen, Ban ban) {
    const int64_t off = prefix >= 0 ? 1 : 0, m = nh + off;
    auto h = [&](int64_t i) { return (off && i == 0) ? prefix : hist[i - off]; };
    if (want_seen)
        for (int64_t i = tid; i < m; i += kThreads) seen(h(i));
    if (n > 0 && m + 1 >= n) {
        const int64_t tail = m - n + 1;  // the last n - 1 ids start here
        for (int64_t i = tid; i + n <= m; i += kThreads) {
            bool eq = true;
            for (int64_t k = 0; k < n - 1 && eq; ++k) eq = h(i + k) == h(tail + k);
            if (eq) ban(h(i + n - 1));
        }
    }
}

// Both tables of a row: zeroed, filled from the history and the EOS ids, then a barrier.
__device__ __forceinline__ void fill_tables(const EilevRulesParams &p, const int64_t *__restrict__ hist, int64_t step, int vocab, int tid,
                                            uint32_t *pen_bits, uint32_t *ban_bits) {
    for (int i = tid; i < kBits; i += kThreads) {
        pen_bits[i] = 0;
        ban_bits[i] = 0;
    }
    __syncthreads();
    const int64_t nh = step < 0 ? 0 : (step < p.max_new ? step : p.max_new);
    scan_history(
        hist, nh, p.prefix_id, (int64_t)p.no_repeat_ngram, p.repetition_penalty != 1.0f, tid,
        [&](int64_t id) {
            if (id >= 0 && id < vocab) atomicOr(&pen_bits[id >> 5], 1u << (id & 31));
        },
        [&](int64_t id) {
            if (id >= 0 && id < vocab) atomicOr(&ban_bits[id >> 5], 1u << (id & 31));
        });
    if (step < p.min_new && tid < EILEV_RULES_MAX_EOS && tid < p.n_eos && p.eos[tid] >= 0 && p.eos[tid] < vocab)
        atomicOr(&ban_bits[p.eos[tid] >> 5], 1u << (p.eos[tid] & 31));
    __syncthreads();
}

// NaN -> -inf, the penalty, the ban, -0 -> +0, on the chunks in registers
__device__ __forceinline__ void apply_rules(float4 (&e)[kChunks], const uint32_t *pen_bits, const uint32_t *ban_bits, float pen, int tid) {
#pragma unroll
    for (int j = 0; j < kChunks; ++j) {
        const int id0 = (tid + kThreads * j) * 4;  // a multiple of 4: the chunk's four bits share a word
        const uint32_t pb = (pen_bits[(id0 >> 5) & (kBits - 1)] >> (id0 & 31)) & 15u, bb = (ban_bits[(id0 >> 5) & (kBits - 1)] >> (id0 & 31)) & 15u;
        float ev[4] = {e[j].x, e[j].y, e[j].z, e[j].w};
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float x = ev[u];
            if (x != x) x = -INFINITY;
            if ((pb >> u) & 1u) x = x < 0.0f ? x * pen : x / pen;
            if ((bb >> u) & 1u) x = -INFINITY;
            ev[u] = x + 0.0f;
        }
        e[j] = make_float4(ev[0], ev[1], ev[2], ev[3]);
    }
}

__device__ __forceinline__ void load_row(float4 (&e)[kChunks], const float *__restrict__ row, int n4, int tid) {
    const float4 *l4 = reinterpret_cast<const float4 *>(row);
#pragma unroll
    for (int j = 0; j < kChunks; ++j) e[j] = tid + kThreads * j < n4 ? l4[tid + kThreads * j] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
}

__device__ __forceinline__ void store_row(const float4 (&e)[kChunks], float *__restrict__ row, int n4, int tid) {
    float4 *w4 = reinterpret_cast<float4 *>(row);
#pragma unroll
    for (int j = 0; j < kChunks; ++j)
        if (tid + kThreads * j < n4) w4[tid + kThreads * j] = e[j];
}

// (value, id) of the workgroup's best pair: larger value, then lower id.  wv / wi: 16 words of LDS each, free to overwrite.
__device__ __forceinline__ void block_best(float &b, int &ix, float *wv, int *wi, int lane, int wid) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(b, o, 64);
        const int oi = __shfl_xor(ix, o, 64);
        if (ov > b || (ov == b && oi < ix)) {
            b = ov;
            ix = oi;
        }
    }
    __syncthreads();  // (the previous use of wv / wi has been read)
    if (lane == 0) {
        wv[wid] = b;
        wi[wid] = ix;
    }
    __syncthreads();
    b = wv[0];
    ix = wi[0];
#pragma unroll
    for (int w = 1; w < 16; ++w)
        if (wv[w] > b || (wv[w] == b && wi[w] < ix)) {
            b = wv[w];
            ix = wi[w];
        }
}

__global__ __launch_bounds__(kThreads) void rules_select_kernel(EilevRulesParams p, const float *__restrict__ logits, int vocab, int32_t *__restrict__ state,
                                                                uint8_t *__restrict__ finished, int64_t *__restrict__ tokens,
                                                                int64_t *__restrict__ out_tokens, float *__restrict__ processed, int whole_step) {
    __shared__ uint32_t pen_bits[kBits], ban_bits[kBits];
    __shared__ float wv[16];
    __shared__ int wi[16];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int n4 = vocab >> 2;
    const int64_t step = (int64_t)state[0] + p.step_offset;
    const bool step_ok = step >= 0 && step < p.max_new;
    fill_tables(p, out_tokens + (int64_t)b * p.max_new, step, vocab, tid, pen_bits, ban_bits);

    float4 e[kChunks];
    load_row(e, logits + (int64_t)b * vocab, n4, tid);
    apply_rules(e, pen_bits, ban_bits, p.repetition_penalty, tid);
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
    if (tid == 0) {
        const int64_t pick = bi == kNone ? 0 : bi;  // (no score above -inf)
        const bool was = finished[b] != 0;
        const int64_t tok = was ? p.pad_id : pick;
        bool eos = false;
        for (int k = 0; k < EILEV_RULES_MAX_EOS; ++k) eos = eos || (k < p.n_eos && p.eos[k] >= 0 && tok == p.eos[k]);
        tokens[b] = tok;
        if (step_ok) out_tokens[(int64_t)b * p.max_new + step] = tok;
        if (eos && !was) finished[b] = 1;
        if (whole_step) {
            if (p.finalize) state[0] = (int32_t)(step + 1);
            state[1] = (was || eos) ? 0 : 1;
        }
    }
}

// rows > 1: the step counter and the "any row unfinished" word, after every row's workgroup
__global__ void rules_finalize_kernel(int32_t *__restrict__ state, const uint8_t *__restrict__ finished, int rows, int step_offset, int finalize) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        int unf = 0;
        for (int b = 0; b < rows; ++b) unf |= finished[b] ? 0 : 1;
        if (finalize) state[0] = state[0] + step_offset + 1;
        state[1] = unf;
    }
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
    fill_tables(p, run_seq + (int64_t)row * p.max_new, cur, vocab, tid, pen_bits, ban_bits);

    float4 e[kChunks];
    load_row(e, logits + (int64_t)row * vocab, n4, tid);
    // ---- log_softmax of the logits as they are, evaluated as topk_logprob_kernel (and torch) does: (x - max) - log(sum exp(x - max))
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < kChunks; ++j) mx = fmaxf(fmaxf(mx, fmaxf(e[j].x, e[j].y)), fmaxf(e[j].z, e[j].w));
    mx = wave_max(mx);
    if (lane == 0) wv[wid] = mx;
    __syncthreads();
    if (tid == 0) {
        float m = wv[0];
        for (int w = 1; w < 16; ++w) m = fmaxf(m, wv[w]);
        bcast[0] = m;
    }
    __syncthreads();
    mx = bcast[0];
    float sm = 0.0f;
#pragma unroll
    for (int j = 0; j < kChunks; ++j)
        if (tid + kThreads * j < n4) sm += (expf(e[j].x - mx) + expf(e[j].y - mx)) + (expf(e[j].z - mx) + expf(e[j].w - mx));
    sm = wave_sum(sm);
    __syncthreads();  // (wv is reused)
    if (lane == 0) wv[wid] = sm;
    __syncthreads();
    if (tid == 0) {
        float t = 0.0f;
        for (int w = 0; w < 16; ++w) t += wv[w];
        bcast[1] = logf(t);
    }
    __syncthreads();
    const float lg = bcast[1], sc = row_score ? row_score[row] : 0.0f;
#pragma unroll
    for (int j = 0; j < kChunks; ++j) e[j] = make_float4((e[j].x - mx) - lg, (e[j].y - mx) - lg, (e[j].z - mx) - lg, (e[j].w - mx) - lg);
    // ---- the rules act on the log-probabilities, then the running score
    apply_rules(e, pen_bits, ban_bits, p.repetition_penalty, tid);
    if (processed) store_row(e, processed + (int64_t)row * vocab, n4, tid);
#pragma unroll
    for (int j = 0; j < kChunks; ++j) e[j] = make_float4(e[j].x + sc, e[j].y + sc, e[j].z + sc, e[j].w + sc);
    // ---- `keep` rounds of arg-max; `taken`: bit (j * 4 + u) = element u of chunk j already won
    unsigned long long taken = 0;
    float best;
    int bi;
    auto rescan = [&]() {
        best = -INFINITY;
        bi = kNone;
#pragma unroll
        for (int j = 0; j < kChunks; ++j) {
            const float ev[4] = {e[j].x, e[j].y, e[j].z, e[j].w};
            const int i = tid + kThreads * j;
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (i < n4 && !((taken >> (j * 4 + u)) & 1ull) && (ev[u] > best || (ev[u] == best && i * 4 + u < bi))) {
                    best = ev[u];
                    bi = i * 4 + u;
                }
        }
    };
    rescan();
    for (int k = 0; k < keep; ++k) {
        float b = best;
        int ix = bi;
        block_best(b, ix, wv, wi, lane, wid);
        if (tid == 0) {
            out_val[(int64_t)row * keep + k] = b;
            out_idx[(int64_t)row * keep + k] = ix == kNone ? 0 : ix;
        }
        if (ix != kNone && ((ix >> 2) & 1023) == tid) {  // this thread owned the winner: chunk j = (ix / 4) / 1024, element ix % 4
            taken |= 1ull << ((((ix >> 2) >> 10) << 2) + (ix & 3));
            rescan();
        }
    }
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
    hipLaunchKernelGGL(rules_finalize_kernel, dim3(1), dim3(64), 0, s, state, (const uint8_t *)finished, (int)rows, (int)p->step_offset, (int)p->finalize);
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

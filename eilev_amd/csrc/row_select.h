// row_select.h — the device code that the three "pick the next token of a row" kernel families share: sample.hip (sample_kernel),
// rules.hip (rules_select_kernel, rules_topk_kernel, rules_ban_kernel) and misc.hip (topk_logprob_kernel).  One 1024-thread workgroup
// per row; the row's <= 16 chunks of 16 bytes (chunk j = float4 index tid + 1024 j) stay in registers, so every pass after the load is
// VALU + LDS; the penalised and the banned set are one bit per id in LDS.  Every reduction compares (value, id), so its result does not
// depend on the order of its steps: a replayed graph gives the eager launch's bits.
//
// Device-only, everything `__device__ __forceinline__` in an anonymous namespace: each library gets its own copy of what it calls.
// The parameter structs (EilevSampleParams, EilevRulesParams) are template arguments: both have repetition_penalty, min_new, max_new,
// n_eos, eos, pad_id, prefix_id and finalize.
#pragma once
#include "common.h"

namespace {

constexpr int kThreads = 1024;
constexpr int kChunks = 16;                         // float4 chunks per thread
constexpr int kMaxVocab = kThreads * kChunks * 4;   // 65536 = EILEV_SAMPLE_MAX_VOCAB = EILEV_RULES_MAX_VOCAB
constexpr int kBits = kMaxVocab / 32;               // words of a one-bit-per-id table
constexpr int kMaxEos = 8;                          // = EILEV_SAMPLE_MAX_EOS = EILEV_RULES_MAX_EOS
constexpr int kNone = 0x7fffffff;                   // "no index": loses every (value, id) comparison against a real id

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

// The row's history h = [prefix if >= 0] + hist[0 .. nh): seen(id) for every id of h (want_seen), ban(id) for every id that would complete
// an n-gram already in h (n = 0: none).  Ids are compared as they are; the callbacks drop those outside the vocabulary.  One thread per
// start position, n - 1 compares against the row's last n - 1 ids.
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

// Both tables of a row: zeroed, filled from the history (penalty: every id; ban: n-grams of length `ngram`) and the EOS ids (below
// min_new), then a barrier.
template <class Params>
__device__ __forceinline__ void fill_tables(const Params &p, const int64_t *__restrict__ hist, int64_t step, int64_t ngram, int vocab, int tid,
                                            uint32_t *pen_bits, uint32_t *ban_bits) {
    for (int i = tid; i < kBits; i += kThreads) {
        pen_bits[i] = 0;
        ban_bits[i] = 0;
    }
    __syncthreads();
    const int64_t nh = step < 0 ? 0 : (step < p.max_new ? step : p.max_new);
    scan_history(
        hist, nh, p.prefix_id, ngram, p.repetition_penalty != 1.0f, tid,
        [&](int64_t id) {
            if (id >= 0 && id < vocab) atomicOr(&pen_bits[id >> 5], 1u << (id & 31));
        },
        [&](int64_t id) {
            if (id >= 0 && id < vocab) atomicOr(&ban_bits[id >> 5], 1u << (id & 31));
        });
    if (step < p.min_new && tid < kMaxEos && tid < p.n_eos && p.eos[tid] >= 0 && p.eos[tid] < vocab)
        atomicOr(&ban_bits[p.eos[tid] >> 5], 1u << (p.eos[tid] & 31));
    __syncthreads();
}

// NaN -> -inf, the penalty, the ban, the temperature (1: none), -0 -> +0 (equal values have equal integer images), on the chunks in registers
__device__ __forceinline__ void apply_rules(float4 (&e)[kChunks], const uint32_t *pen_bits, const uint32_t *ban_bits, float pen, float temp, int tid) {
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
            if (temp != 1.0f) x = x / temp;
            ev[u] = x + 0.0f;
        }
        e[j] = make_float4(ev[0], ev[1], ev[2], ev[3]);
    }
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

// log_softmax of the row as torch evaluates it, fp32: x -> (x - mx) - lg with mx the row maximum and lg = log(sum exp(x - mx)) (padding
// entries are -inf: exp = 0).  wv: 16 words of LDS, bcast: 2.
__device__ __forceinline__ void row_log_softmax(const float4 (&e)[kChunks], int n4, float *wv, float *bcast, int tid, int lane, int wid, float &mx,
                                                float &lg) {
    mx = -INFINITY;
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
    lg = bcast[1];
}

// `keep` rounds of (workgroup arg-max, the owning thread drops the winner and rescans its own <= 64 elements); thread 0 calls
// emit(k, value, index) for round k (index 0 when nothing is left).  The values are compared as they are in `e`.
template <class Emit>
__device__ __forceinline__ void topk_rounds(const float4 (&e)[kChunks], int n4, int keep, float *wv, int *wi, int tid, int lane, int wid, Emit emit) {
    unsigned long long taken = 0;  // bit (j * 4 + u) = element u of chunk j already won
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
        if (tid == 0) emit(k, b, ix == kNone ? 0 : ix);
        if (ix != kNone && ((ix >> 2) & 1023) == tid) {  // this thread owned the winner: chunk j = (ix / 4) / 1024, element ix % 4
            taken |= 1ull << ((((ix >> 2) >> 10) << 2) + (ix & 3));
            rescan();
        }
    }
}

// Thread 0 commits the row's token: the pad id if the row had finished, the EOS test, tokens / out_tokens / finished, and the step
// counter and "unfinished" word when this workgroup is the whole step (rows == 1).
template <class Params>
__device__ __forceinline__ void commit_token(const Params &p, int64_t pick, int b, int64_t step, int32_t *__restrict__ state,
                                             uint8_t *__restrict__ finished, int64_t *__restrict__ tokens, int64_t *__restrict__ out_tokens,
                                             int whole_step) {
    const bool was = finished[b] != 0;
    const int64_t tok = was ? p.pad_id : pick;
    bool eos = false;
    for (int k = 0; k < kMaxEos; ++k) eos = eos || (k < p.n_eos && p.eos[k] >= 0 && tok == p.eos[k]);
    tokens[b] = tok;
    if (step >= 0 && step < p.max_new) out_tokens[(int64_t)b * p.max_new + step] = tok;
    if (eos && !was) finished[b] = 1;
    if (whole_step) {
        if (p.finalize) state[0] = (int32_t)(step + 1);
        state[1] = (was || eos) ? 0 : 1;
    }
}

// rows > 1: the step counter and the "any row unfinished" word, after every row's workgroup.  (A template only so that a file that
// never launches it emits no copy of it.)
template <int = 0>
__global__ void row_finalize_kernel(int32_t *__restrict__ state, const uint8_t *__restrict__ finished, int rows, int step_offset, int finalize) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        int unf = 0;
        for (int b = 0; b < rows; ++b) unf |= finished[b] ? 0 : 1;
        if (finalize) state[0] = state[0] + step_offset + 1;
        state[1] = unf;
    }
}

}  // namespace

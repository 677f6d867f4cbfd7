// pld.hip — prompt-lookup decoding at batch 1 (include/eilev_pld.h): the draft search and the accept / commit step that wrap the
// core library's verify (eilev_opt_extend, eilev_t5_decode) and single-token steps (eilev_opt_decode_step, eilev_t5_decode_step).
// Standalone library (libeilev_hip_pld.so): it shares common.h's macros with the core library and nothing else.
#include <climits>

#include "common.h"
#include "../../include/eilev_pld.h"

namespace {

constexpr int kArgThreads = 256;
constexpr int kArgPerThread = 16;
constexpr int kSplit = kArgThreads * kArgPerThread;  // logits of one row per arg-max workgroup
constexpr int kStepThreads = 1024;

// eilev_greedy_select's order (misc.hip select_kernel): the larger value wins, equal values go to the lower id, NaN never wins
__device__ __forceinline__ void take(float v, int i, float &best, int &bi) {
    if (v > best || (v == best && i < bi)) {
        best = v;
        bi = i;
    }
}

__device__ __forceinline__ bool is_eos(const EilevPldParams &p, int64_t id) {
    for (int e = 0; e < p.n_eos; ++e)
        if (p.eos[e] == id) return true;
    return false;
}

// arg-max of logits[row, split * kSplit .. + kSplit) -> part[row * nsplit + split]; grid (nsplit, rows)
__global__ __launch_bounds__(kArgThreads) void pld_argmax_part_kernel(const float *__restrict__ logits, int vocab, float *__restrict__ part_v,
                                                                       int *__restrict__ part_i) {
    __shared__ float wv[kArgThreads / 64];
    __shared__ int wi[kArgThreads / 64];
    const int split = blockIdx.x, row = blockIdx.y, nsplit = gridDim.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const float *lr = logits + (int64_t)row * vocab;
    const int base = split * kSplit;
    float v[kArgPerThread];
#pragma unroll
    for (int j = 0; j < kArgPerThread; ++j) {
        const int i = base + j * kArgThreads + tid;
        v[j] = i < vocab ? lr[i] : NAN;
    }
    float best = -INFINITY;
    int bi = INT_MAX;
#pragma unroll
    for (int j = 0; j < kArgPerThread; ++j) take(v[j], base + j * kArgThreads + tid, best, bi);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        take(ov, oi, best, bi);
    }
    if (lane == 0) {
        wv[wid] = best;
        wi[wid] = bi;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < kArgThreads / 64; ++w) take(wv[w], wi[w], best, bi);
        part_v[(int64_t)row * nsplit + split] = best;
        part_i[(int64_t)row * nsplit + split] = bi;
    }
}

// The draft for committed count c and corpus length len (the whole workgroup calls it; the result is valid in thread 0, which also
// writes window[1 .. m]).  PromptLookupCandidateGenerator.get_candidates: for n = min(ngram, len - 1) .. 1, the first idx (left to
// right) with corpus[idx .. idx + n) == the last n ids and idx + n < len (a non-empty continuation); the continuation is cut before its
// first EOS id; then the caps of the budget (the verify also commits the bonus id) and of the cache.
__device__ int draft_block(const EilevPldParams &p, const int64_t *__restrict__ corpus, int len, int64_t c, bool done,
                           int64_t *__restrict__ window) {
    __shared__ int first;
    const int tid = threadIdx.x;
    int64_t cap = p.k;
    cap = min(cap, p.max_new - c - 1);
    cap = min(cap, p.slot_limit - p.slot_base - c);
    if (done || cap <= 0) return 0;
    const int nmax = (int)min((int64_t)len - 1, p.ngram);
    for (int n = nmax; n >= 1; --n) {
        if (tid == 0) first = INT_MAX;
        __syncthreads();
        const int64_t *suf = corpus + (len - n);
        for (int idx = tid; idx + n < len; idx += blockDim.x) {
            bool eq = true;
            for (int j = 0; j < n && eq; ++j) eq = corpus[idx + j] == suf[j];
            if (eq) {  // a thread meets its indices in increasing order: its first match is its smallest
                atomicMin(&first, idx);
                break;
            }
        }
        __syncthreads();
        const int f = first;
        __syncthreads();  // every thread has read `first` before the next size resets it
        if (f != INT_MAX) {
            int m = 0;
            if (tid == 0) {
                const int64_t s = (int64_t)f + n, e = min(s + p.k, (int64_t)len);
                for (int64_t i = s; i < e && m < cap; ++i) {
                    const int64_t id = corpus[i];
                    if (is_eos(p, id)) break;
                    window[1 + m++] = id;
                }
            }
            return m;
        }
    }
    return 0;
}

__global__ __launch_bounds__(kStepThreads) void pld_draft_kernel(EilevPldParams p, const int64_t *__restrict__ corpus,
                                                                  const int32_t *__restrict__ corpus_len, int64_t *__restrict__ window,
                                                                  int32_t *__restrict__ status) {
    const int m = draft_block(p, corpus, corpus_len[0], status[0], status[2] != 0, window);
    if (threadIdx.x == 0) status[1] = m;
}

// merge of the partial arg-maxima, accept, commit, next draft: one workgroup
__global__ __launch_bounds__(kStepThreads) void pld_commit_kernel(EilevPldParams p, const float *__restrict__ part_v, const int *__restrict__ part_i,
                                                                   int rows, int nsplit, int64_t *__restrict__ corpus, int32_t *__restrict__ corpus_len,
                                                                   int64_t *__restrict__ window, int32_t *__restrict__ state,
                                                                   int64_t *__restrict__ out, int32_t *__restrict__ status) {
    __shared__ int64_t g[EILEV_PLD_MAX_K + 1];
    __shared__ int sh_len, sh_done;
    __shared__ int64_t sh_c;
    const int tid = threadIdx.x;
    if (tid < rows) {
        float best = -INFINITY;
        int bi = INT_MAX;
        for (int s = 0; s < nsplit; ++s) take(part_v[tid * nsplit + s], part_i[tid * nsplit + s], best, bi);
        g[tid] = bi == INT_MAX ? 0 : bi;
    }
    __syncthreads();
    int a = 0;
    if (tid == 0) {
        int64_t c = status[0];
        int len = corpus_len[0];
        const int m = rows - 1;
        while (a < m && g[a] == window[1 + a]) ++a;
        bool done = c >= p.max_new;
        int64_t last = window[0];
        for (int i = 0; i <= a && !done; ++i) {
            const int64_t id = i < a ? window[1 + i] : g[a];
            out[c] = id;
            if (len < p.corpus_cap) corpus[len++] = id;
            ++c;
            last = id;
            done = is_eos(p, id) || c >= p.max_new;
        }
        window[0] = last;
        state[0] = (int32_t)c;
        state[1] = done ? 0 : 1;
        sh_c = c;
        sh_len = len;
        sh_done = done;
    }
    __syncthreads();  // window[1 ..] was read above before the draft overwrites it
    const int64_t c = sh_c;
    const int len = sh_len;
    const bool done = sh_done != 0;
    const int m = draft_block(p, corpus, len, c, done, window);
    if (tid == 0) {
        corpus_len[0] = len;
        status[0] = (int32_t)c;
        status[1] = m;
        status[2] = done ? 1 : 0;
        status[3] = a;
    }
}

bool params_ok(const EilevPldParams *p) {
    return p && p->k >= 1 && p->k <= EILEV_PLD_MAX_K && p->ngram >= 1 && p->max_new >= 1 && p->max_new < INT_MAX && p->slot_base >= 0 &&
           p->corpus_cap >= 1 && p->corpus_cap < INT_MAX && p->n_eos >= 0 && p->n_eos <= EILEV_PLD_MAX_EOS;
}

int64_t n_splits(int64_t vocab) { return (vocab + kSplit - 1) / kSplit; }

}  // namespace

extern "C" int eilev_pld_abi_version(void) { return EILEV_PLD_ABI_VERSION; }

extern "C" size_t eilev_pld_scratch_bytes(int64_t rows, int64_t vocab) {
    if (rows <= 0 || vocab <= 0) return 0;
    return (size_t)rows * (size_t)n_splits(vocab) * (sizeof(float) + sizeof(int));
}

extern "C" int eilev_pld_draft(const EilevPldParams *p, const int64_t *corpus, const int32_t *corpus_len, int64_t *window, int32_t *status,
                               void *stream) {
    if (!params_ok(p) || !corpus || !corpus_len || !window || !status) return EILEV_E_BADARG;
    hipLaunchKernelGGL(pld_draft_kernel, dim3(1), dim3(kStepThreads), 0, (hipStream_t)stream, *p, corpus, corpus_len, window, status);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}

extern "C" int eilev_pld_step(const EilevPldParams *p, const float *logits, int64_t rows, int64_t vocab, int64_t *corpus, int32_t *corpus_len,
                              int64_t *window, int32_t *state, int64_t *out, int32_t *status, void *scratch, size_t scratch_bytes,
                              void *stream) {
    if (!params_ok(p) || !logits || !corpus || !corpus_len || !window || !state || !out || !status) return EILEV_E_BADARG;
    if (rows < 1 || rows > p->k + 1 || vocab < 1 || vocab >= INT_MAX) return EILEV_E_BADARG;
    if (!scratch || scratch_bytes < eilev_pld_scratch_bytes(rows, vocab)) return EILEV_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int64_t ns = n_splits(vocab);
    float *part_v = (float *)scratch;
    int *part_i = (int *)(part_v + rows * ns);
    hipLaunchKernelGGL(pld_argmax_part_kernel, dim3((unsigned)ns, (unsigned)rows), dim3(kArgThreads), 0, s, logits, (int)vocab, part_v, part_i);
    EILEV_LAUNCH_CHECK();
    hipLaunchKernelGGL(pld_commit_kernel, dim3(1), dim3(kStepThreads), 0, s, *p, (const float *)part_v, (const int *)part_i, (int)rows, (int)ns,
                       corpus, corpus_len, window, state, out, status);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}

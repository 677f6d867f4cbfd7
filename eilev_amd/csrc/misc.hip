// misc.hip — the HBM-bound glue kernels of the path: patch gather (im2col), embedding gather/scatter,
// OPT position ids, KV-cache writes, greedy selection.  (Single-query decode attention: attn_decode.hip.)
#include "row_select.h"

namespace {

// ---- patch gather -------------------------------------------------------------------------------
// Conv2d(3->D, k=P, s=P) of hf modeling_blip_2.py:246 as a GEMM: row (n, t, py, px) gathers 3*P*P pixels of
// frame t of clip n straight from the (N, 3, T, H, W) tensor (the permute+flatten of
// ref:eilev/model/v2.py:57 is pure addressing).  K is zero-padded to KP (multiple of 64).
template <typename T>
__global__ void im2col_kernel(const T *__restrict__ pix, bf16 *__restrict__ out, int64_t rows, int frames, int img,
                              int patch, int kp) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int chunks = kp >> 3;
    if (idx >= rows * chunks) return;
    const int64_t row = idx / chunks;
    const int c = (int)(idx - row * chunks);
    const int g = img / patch, gg = g * g, pp = patch * patch;
    const int64_t f = row / gg;
    const int p = (int)(row - f * gg), py = p / g, px = p - py * g;
    const int64_t n = f / frames;
    const int t = (int)(f - n * frames);
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = c * 8 + e;
        float val = 0.0f;
        if (k < 3 * pp) {
            const int ch = k / pp, rem = k - ch * pp, dy = rem / patch, dx = rem - dy * patch;
            val = (float)pix[(((n * 3 + ch) * frames + t) * img + py * patch + dy) * (int64_t)img + px * patch + dx];
        }
        v[e] = val;
    }
    *reinterpret_cast<bf16x8 *>(out + row * kp + c * 8) = pack8(v);
}

// Same result, frame tensor read with coalesced 16-byte loads: one workgroup per (frame, patch row) stages the 3 x patch x img
// strip of pixels in LDS (as bf16) and writes the strip's img / patch im2col rows with coalesced 16-byte stores.
// IMG / PATCH are compile-time (ViT-g/14 at 224): every index division becomes a multiply-shift.
template <typename T, int IMG, int PATCH>
__global__ __launch_bounds__(256) void im2col_strip_kernel(const T *__restrict__ pix, bf16 *__restrict__ out, int frames, int kp) {
    constexpr int img = IMG, patch = PATCH;
    extern __shared__ __attribute__((aligned(16))) char im2col_smem[];
    bf16 *strip = reinterpret_cast<bf16 *>(im2col_smem);  // [3][patch][img]
    const int g = img / patch, pp = patch * patch;
    const int64_t f = blockIdx.x / g;
    const int py = (int)(blockIdx.x - f * g);
    const int64_t n = f / frames;
    const int t = (int)(f - n * frames);
    const int cpr = img >> 3;  // 8-pixel chunks per image row
    for (int i = threadIdx.x; i < 3 * patch * cpr; i += blockDim.x) {
        const int ch = i / (patch * cpr), rem = i - ch * patch * cpr, dy = rem / cpr, cx = rem - dy * cpr;
        const T *src = pix + (((n * 3 + ch) * frames + t) * img + py * patch + dy) * (int64_t)img + cx * 8;
        float v[8];
        if constexpr (sizeof(T) == 2) {
            const bf16x8 q = *reinterpret_cast<const bf16x8 *>(src);
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = (float)q[e];
        } else {
            const float4 a = *reinterpret_cast<const float4 *>(src), b = *reinterpret_cast<const float4 *>(src + 4);
            v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
        }
        *reinterpret_cast<bf16x8 *>(strip + (ch * patch + dy) * img + cx * 8) = pack8(v);
    }
    __syncthreads();
    const int chunks = kp >> 3;
    for (int i = threadIdx.x; i < g * chunks; i += blockDim.x) {
        const int px = i / chunks, c = i - px * chunks;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int k = c * 8 + e;
            float val = 0.0f;
            if (k < 3 * pp) {
                const int ch = k / pp, rem = k - ch * pp, dy = rem / patch, dx = rem - dy * patch;
                val = (float)strip[(ch * patch + dy) * img + px * patch + dx];
            }
            v[e] = val;
        }
        *reinterpret_cast<bf16x8 *>(out + ((f * g + py) * g + px) * (int64_t)kp + c * 8) = pack8(v);
    }
}

__global__ void pad_rows_kernel(const bf16 *__restrict__ w, bf16 *__restrict__ out, int rows, int k, int kp) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * kp) return;
    const int r = idx / kp, c = idx - r * kp;
    out[idx] = c < k ? w[(int64_t)r * k + c] : (bf16)0.0f;
}

__global__ void cls_rows_kernel(const bf16 *__restrict__ cls, const bf16 *__restrict__ pos, bf16 *__restrict__ x,
                                int64_t frames_total, int tok, int d) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= frames_total * d) return;
    const int64_t f = idx / d;
    const int c = (int)(idx - f * d);
    x[f * tok * (int64_t)d + c] = (bf16)((float)cls[c] + (float)pos[c]);
}

__global__ void broadcast_rows_kernel(const bf16 *__restrict__ src, bf16 *__restrict__ dst, int64_t copies, int64_t n) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= copies * n) return;
    dst[idx] = src[idx % n];
}

// ---- embedding gather + video-feature scatter (ref:eilev/model/v2.py:314-316) -----------------------
// Pass 1 (one workgroup): exclusive rank of every set bit of video_mask in row-major (B, L) order, parked
// in the first 4 bytes of the destination row.  Pass 2 (workgroup per row): copy either
// video_feats[rank] or embed_tokens[id].
__global__ __launch_bounds__(1024) void mask_rank_kernel(const uint8_t *__restrict__ mask, bf16 *__restrict__ out,
                                                         int64_t total, int d) {
    __shared__ int wsum[16];
    __shared__ int base;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    if (tid == 0) base = 0;
    __syncthreads();
    for (int64_t start = 0; start < total; start += 1024) {
        const int64_t i = start + tid;
        const int bit = (i < total && mask && mask[i]) ? 1 : 0;
        int incl = bit;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (lane == 63) wsum[wid] = incl;
        __syncthreads();
        int woff = 0;
        for (int w = 0; w < wid; ++w) woff += wsum[w];
        const int rank = base + woff + incl - bit;
        if (i < total) *reinterpret_cast<int *>(out + i * (int64_t)d) = bit ? rank : -1;
        __syncthreads();
        if (tid == 1023) base = base + woff + incl;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void embed_rows_kernel(const bf16 *__restrict__ embed, const int64_t *__restrict__ ids,
                                                         const bf16 *__restrict__ feats, int64_t n_rows, int vocab,
                                                         bf16 *__restrict__ out, int d) {
    __shared__ int rank_s;
    const int64_t i = blockIdx.x;
    bf16 *dst = out + i * (int64_t)d;
    if (threadIdx.x == 0) rank_s = *reinterpret_cast<const int *>(dst);
    __syncthreads();
    const int rank = rank_s;
    const bf16 *src;
    if (rank >= 0 && feats && rank < n_rows) {
        src = feats + (int64_t)rank * d;
    } else {
        int64_t id = ids[i];
        id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
        src = embed + id * d;
    }
    __syncthreads();
    for (int c = threadIdx.x; c < (d >> 3); c += 256)
        *reinterpret_cast<bf16x8 *>(dst + c * 8) = *reinterpret_cast<const bf16x8 *>(src + c * 8);
}

// ---- OPT learned positions: pid = cumsum(mask) * mask - 1 + 2 (hf modeling_opt.py:64-70) ---------------
__global__ __launch_bounds__(1024) void pos_ids_kernel(const int32_t *__restrict__ mask, int32_t *__restrict__ pid, int L) {
    __shared__ int wsum[16];
    __shared__ int base;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int64_t b = blockIdx.x;
    if (tid == 0) base = 0;
    __syncthreads();
    for (int start = 0; start < L; start += 1024) {
        const int i = start + tid;
        const int bit = (i < L && mask[b * L + i] != 0) ? 1 : 0;
        int incl = bit;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int t = __shfl_up(incl, o, 64);
            if (lane >= o) incl += t;
        }
        if (lane == 63) wsum[wid] = incl;
        __syncthreads();
        int woff = 0;
        for (int w = 0; w < wid; ++w) woff += wsum[w];
        const int cum = base + woff + incl;
        if (i < L) pid[b * L + i] = cum * bit - 1 + 2;
        __syncthreads();
        if (tid == 1023) base = cum;
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void add_pos_kernel(const bf16 *__restrict__ emb, const bf16 *__restrict__ pos,
                                                      const int32_t *__restrict__ pid, bf16 *__restrict__ h, int d,
                                                      int rows_per_b, int pid_ld, int pid_off) {
    const int64_t i = blockIdx.x;  // row b * rows_per_b + r reads pid[b * pid_ld + pid_off + r]
    const int64_t pb = i / rows_per_b, pr = i - pb * rows_per_b;
    const bf16 *e = emb + i * d, *p = pos + (int64_t)pid[pb * pid_ld + pid_off + pr] * d;
    for (int c = threadIdx.x; c < (d >> 3); c += 256) {
        float x[8], y[8];
        unpack8(*reinterpret_cast<const bf16x8 *>(e + c * 8), x);
        unpack8(*reinterpret_cast<const bf16x8 *>(p + c * 8), y);
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] += y[k];
        *reinterpret_cast<bf16x8 *>(h + i * d + c * 8) = pack8(x);
    }
}

// decode: h[b] = embed[tokens[b]] + pos[n_valid[b] + step - 1 + 2], step = state[0]
__global__ __launch_bounds__(256) void decode_embed_kernel(const bf16 *__restrict__ embed, const bf16 *__restrict__ pos,
                                                           const int64_t *__restrict__ tokens,
                                                           const int32_t *__restrict__ n_valid,
                                                           const int32_t *__restrict__ state, int vocab, int max_pid,
                                                           bf16 *__restrict__ h, int d) {
    const int b = blockIdx.x;
    int64_t id = tokens[b];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    int pidx = n_valid[b] + state[0] - 1 + 2;
    pidx = pidx > max_pid ? max_pid : pidx;
    const bf16 *e = embed + id * d, *p = pos + (int64_t)pidx * d;
    for (int c = threadIdx.x; c < (d >> 3); c += 256) {
        float x[8], y[8];
        unpack8(*reinterpret_cast<const bf16x8 *>(e + c * 8), x);
        unpack8(*reinterpret_cast<const bf16x8 *>(p + c * 8), y);
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] += y[k];
        *reinterpret_cast<bf16x8 *>(h + (int64_t)b * d + c * 8) = pack8(x);
    }
}

// ---- KV cache: [B][H][cap][hd] per layer and per k/v (DynamicCache.update, hf modeling_opt.py:161) ----
// qkv: rows of 3*D (q | k | v).  Prefill: rows_per_b = L, slot0 = 0.  Decode: rows_per_b = 1, slot from state.
__global__ __launch_bounds__(256) void kv_write_kernel(const bf16 *__restrict__ qkv, bf16 *__restrict__ kc,
                                                       bf16 *__restrict__ vc, int rows_per_b, int heads, int hd, int cap,
                                                       int seq_len, const int32_t *__restrict__ state, int slot0) {
    const int64_t row = blockIdx.x;  // b * rows_per_b + r
    const int b = (int)(row / rows_per_b), r = (int)(row - (int64_t)b * rows_per_b);
    const int slot = state ? (seq_len + state[0] - 1) : slot0 + r;
    const int d = heads * hd, ch = hd >> 3;
    const bf16 *src = qkv + row * 3 * (int64_t)d;
    for (int c = threadIdx.x; c < 2 * heads * ch; c += 256) {
        const int which = c / (heads * ch), rem = c - which * heads * ch, hh = rem / ch, cc = rem - hh * ch;
        const bf16x8 v = *reinterpret_cast<const bf16x8 *>(src + (1 + which) * d + hh * hd + cc * 8);
        bf16 *dst = (which ? vc : kc) + (((int64_t)b * heads + hh) * cap + slot) * hd + cc * 8;
        *reinterpret_cast<bf16x8 *>(dst) = v;
    }
}

// ---- greedy selection (hf generation/utils.py:2894-2937) ------------------------------------------------
// finalize != 0 (one row: this block is the whole step): the step counter / unfinished count of finalize_step_kernel written here
__global__ __launch_bounds__(1024) void select_kernel(const float *__restrict__ logits, int vocab,
                                                      int32_t *__restrict__ state, uint8_t *__restrict__ finished,
                                                      int64_t eos_id, int64_t pad_id, int64_t *__restrict__ tokens,
                                                      int64_t *__restrict__ out_tokens, int64_t max_new, int finalize) {
    __shared__ float wv[16];
    __shared__ int wi[16];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const float *lr = logits + (int64_t)b * vocab;
    float best = -INFINITY;
    int bi = 0x7fffffff;
    auto take = [&](float v, int i) {
        if (v > best || (v == best && i < bi)) {
            best = v;
            bi = i;
        }
    };
    if ((vocab & 3) == 0 && (((uintptr_t)lr) & 15) == 0) {
        // 16-byte loads, four independent requests in flight per thread (the scalar walk below was one dependent 4-byte load per step:
        // 20.6 us per step for 200 KB of logits, r4); a thread still meets its indices in increasing order: same winner on ties
        const float4 *l4 = reinterpret_cast<const float4 *>(lr);
        const int n4 = vocab >> 2;
        for (int i0 = tid; i0 < n4; i0 += 4 * 1024) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = i0 + u * 1024 < n4 ? l4[i0 + u * 1024] : make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = (i0 + u * 1024) * 4;
                if (i >= vocab) continue;
                take(v[u].x, i);
                take(v[u].y, i + 1);
                take(v[u].z, i + 2);
                take(v[u].w, i + 3);
            }
        }
    } else {
        for (int i = tid; i < vocab; i += 1024) take(lr[i], i);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(best, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > best || (ov == best && oi < bi)) {
            best = ov;
            bi = oi;
        }
    }
    if (lane == 0) {
        wv[wid] = best;
        wi[wid] = bi;
    }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 16; ++w)
            if (wv[w] > best || (wv[w] == best && wi[w] < bi)) {
                best = wv[w];
                bi = wi[w];
            }
        if (bi == 0x7fffffff) bi = 0;
        const int step = state[0];
        const int64_t tok = finished[b] ? pad_id : (int64_t)bi;
        tokens[b] = tok;
        if (step < max_new) out_tokens[(int64_t)b * max_new + step] = tok;
        const bool fin = finished[b] || (eos_id >= 0 && tok == eos_id);
        if (eos_id >= 0 && tok == eos_id) finished[b] = 1;
        if (finalize) {
            state[0] = step + 1;
            state[1] = fin ? 0 : 1;
        }
    }
}

// ---- beam search: the best `keep` continuations of every row (hf generation/utils.py `_get_top_k_continuations`: log_softmax of the row's
// logits + the row's running score, top 2K over beams x vocabulary — the global top 2K lie among the per-row top 2K, which is this
// kernel; the merge over a sample's rows is K x 2K numbers).  One 1024-thread workgroup per row: max, sum of exp (log_softmax exactly as
// torch evaluates it: (x - max) - log(sum exp(x - max)), fp32), then `keep` rounds of (workgroup arg-max, the owning thread drops the
// winner and rescans its own <= 64 elements, which it holds in registers).  vocab <= 65536, vocab % 4 == 0.
__global__ __launch_bounds__(1024) void topk_logprob_kernel(const float *__restrict__ logits, const float *__restrict__ row_score, int vocab,
                                                            int keep, float *__restrict__ out_val, int32_t *__restrict__ out_idx) {
    __shared__ float wv[16];
    __shared__ int wi[16];
    __shared__ float bcast[2];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int n4 = vocab >> 2;
    float4 e[kChunks];
    load_row(e, logits + (int64_t)row * vocab, n4, tid);
    float mx, lg;
    row_log_softmax(e, n4, wv, bcast, tid, lane, wid, mx, lg);
    const float sc = row_score ? row_score[row] : 0.0f;
    // the rounds compare the logits themselves; the log-probability of a winner is formed when it is written
    topk_rounds(e, n4, keep, wv, wi, tid, lane, wid, [&](int k, float v, int ix) {
        out_val[(int64_t)row * keep + k] = ((v - mx) - lg) + sc;
        out_idx[(int64_t)row * keep + k] = ix;
    });
}

// ---- beam search bookkeeping of one step (include/eilev.h eilev_beam_advance; oracle/eilev_ref.c holds the plain restatement).  One
// workgroup per sample: lane-parallel arg-max rounds for the three small top-k selections, thread 0 for the scalar rules, all threads
// for the sequence rows (T int64 each).  Everything a step needs from the previous one is read before the first write (LDS / registers),
// then a barrier, then the in-place update.
struct BeamAdvanceArgs {
    const float *row_lp;
    const int32_t *row_tok;
    const int32_t *state;
    const float *len_pow;
    int64_t eos[8];
    int n_eos, beams, keep, T, early, recip, gen_cap, batch;
    int64_t *run_seq, *fin_seq, *fin_len, *tokens, *scratch;  // scratch: (batch, keep + 2 * beams, T)
    float *run_score, *fin_score;
    uint8_t *finished, *can_improve;
    int32_t *anc;
};

__device__ __forceinline__ void beam_topk_lds(float *v, int n, int k, int *out, float *red_v, int *red_i) {  // v is consumed (winners -> -inf-like)
    const int tid = threadIdx.x;
    for (int a = 0; a < k; ++a) {
        float b = -INFINITY;
        int bi = 0x7fffffff;
        for (int i = tid; i < n; i += 256) {
            const float x = v[i];
            if (!(__builtin_bit_cast(unsigned, x) == 0xffc00001u) && (bi == 0x7fffffff || x > b)) {  // (0xffc00001: the "taken" marker, a NaN no score is)
                b = x;
                bi = i;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(b, o, 64);
            const int oi = __shfl_xor(bi, o, 64);
            if (oi != 0x7fffffff && (bi == 0x7fffffff || ov > b || (ov == b && oi < bi))) {
                b = ov;
                bi = oi;
            }
        }
        if ((tid & 63) == 0) {
            red_v[tid >> 6] = b;
            red_i[tid >> 6] = bi;
        }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < 4; ++w)
                if (red_i[w] != 0x7fffffff && (bi == 0x7fffffff || red_v[w] > b || (red_v[w] == b && red_i[w] < bi))) {
                    b = red_v[w];
                    bi = red_i[w];
                }
            out[a] = bi;
            v[bi] = __builtin_bit_cast(float, 0xffc00001u);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void beam_advance_kernel(const BeamAdvanceArgs a) {
    constexpr float NEG = -1.0e9f;
    __shared__ float cv[2048], cv0[2048], live[64], live0[64], top_lp[64], all_score[96], all_score0[96], red_v[4], nfsc[32], nrsc[32];
    __shared__ int order[64], nxt[32], best[32], src[64], red_i[4], hit[64], jd[64];
    __shared__ int64_t tok[64], nfl[32];
    __shared__ uint8_t nfd[32];
    __shared__ int32_t acol[32 * 64];  // gen_cap <= 64 ancestor rows of the sample's columns (larger tables: scratch-free second pass below)
    const int b = blockIdx.x, tid = threadIdx.x, K = a.beams, keep = a.keep, T = a.T, C = K * keep, R = a.batch * K;
    // state[0] counts the generated tokens including this step's: 1 .. T (include/eilev.h).  It is a device value the host entry cannot
    // check, so a caller that forgot `state[0] = 1` or advanced past max_new gets NO update instead of out-of-range reads of len_pow,
    // the candidate column and the ancestor row (attn_decode_split_kernel guards the same counter the same way).
    const int cur = a.state[0] - 1;
    if (cur < 0 || cur >= T) return;
    for (int c = tid; c < C; c += 256) cv[c] = cv0[c] = a.row_lp[(int64_t)(b * K + c / keep) * keep + c % keep];
    __syncthreads();
    beam_topk_lds(cv, C, keep, order, red_v, red_i);
    if (tid < keep) {
        const int k = tid, o = order[k];
        top_lp[k] = cv0[o];
        src[k] = o / keep;
        const int64_t t_ = a.row_tok[(int64_t)(b * K + src[k]) * keep + o % keep];
        tok[k] = t_;
        int h = cur + 1 >= T;
        for (int e = 0; e < a.n_eos; ++e) h |= t_ == a.eos[e];
        hit[k] = h;
        live[k] = live0[k] = top_lp[k] + (h ? 1.0f : 0.0f) * NEG;
    }
    __syncthreads();
    // candidate sequences -> scratch rows 0 .. keep - 1
    int64_t *cand = a.scratch + (int64_t)b * (keep + 2 * K) * T, *nfs = cand + (int64_t)keep * T, *nrs = nfs + (int64_t)K * T;
    for (int i = tid; i < keep * T; i += 256) {
        const int k = i / T, p = i - k * T;
        cand[i] = p == cur ? tok[k] : a.run_seq[(int64_t)(b * K + src[k]) * T + p];
    }
    beam_topk_lds(live, keep, K, nxt, red_v, red_i);
    if (tid == 0) {
        int all_fin = 1;
        for (int j = 0; j < K; ++j) all_fin &= a.finished[b * K + j] != 0;
        const float lp_f = a.len_pow[cur];
        const bool ci = a.can_improve[b] != 0;
        for (int k = 0; k < keep; ++k) {
            jd[k] = hit[k] && k < K;
            float d = a.recip ? top_lp[k] * lp_f : top_lp[k] / lp_f;
            if (a.early == 1) d = d + (all_fin ? 1.0f : 0.0f) * NEG;
            d = d + (ci ? 0.0f : 1.0f) * NEG;
            d = d + (jd[k] ? 0.0f : 1.0f) * NEG;
            all_score[K + k] = all_score0[K + k] = d;
        }
        for (int j = 0; j < K; ++j) all_score[j] = all_score0[j] = a.fin_score[b * K + j];
    }
    __syncthreads();
    beam_topk_lds(all_score, K + keep, K, best, red_v, red_i);
    if (tid == 0) {
        for (int j = 0; j < K; ++j) {
            const int s_ = best[j];
            nfsc[j] = all_score0[s_];
            nfl[j] = s_ < K ? a.fin_len[b * K + s_] : (int64_t)(cur + 1);
            nfd[j] = s_ < K ? a.finished[b * K + s_] : (uint8_t)jd[s_ - K];
            nrsc[j] = live0[nxt[j]];
        }
        const float rp = a.len_pow[a.early == 2 ? T - 1 : cur];
        const float best_running = a.recip ? nrsc[0] * rp : nrsc[0] / rp;
        float mn = nfsc[0];
        for (int j = 1; j < K; ++j) mn = fminf(mn, nfsc[j]);
        int any = 0;
        for (int j = 0; j < K; ++j) any |= best_running > (nfd[j] ? mn : NEG);
        a.can_improve[b] = (uint8_t)(a.can_improve[b] && any);
    }
    __syncthreads();
    // new finished / running rows -> scratch (they gather from rows that are about to be overwritten), ancestor columns -> LDS
    for (int i = tid; i < K * T; i += 256) {
        const int j = i / T, p = i - j * T, s_ = best[j];
        nfs[i] = s_ < K ? a.fin_seq[(int64_t)(b * K + s_) * T + p] : cand[(int64_t)(s_ - K) * T + p];
        nrs[i] = cand[(int64_t)nxt[j] * T + p];
    }
    if (a.anc)
        for (int i = tid; i < a.gen_cap * K; i += 256) {
            const int g = i / K, j = i - g * K;
            acol[i] = a.anc[(int64_t)g * R + b * K + src[nxt[j]]];
        }
    __syncthreads();
    __threadfence_block();
    for (int i = tid; i < K * T; i += 256) {
        a.fin_seq[(int64_t)b * K * T + i] = nfs[i];
        a.run_seq[(int64_t)b * K * T + i] = nrs[i];
    }
    if (a.anc)
        for (int i = tid; i < a.gen_cap * K; i += 256) {
            const int g = i / K, j = i - g * K;
            a.anc[(int64_t)g * R + b * K + j] = g == cur ? b * K + j : acol[i];
        }
    if (tid < K) {
        const int j = tid;
        a.tokens[b * K + j] = tok[nxt[j]];
        a.run_score[b * K + j] = nrsc[j];
        a.fin_score[b * K + j] = nfsc[j];
        a.fin_len[b * K + j] = nfl[j];
        a.finished[b * K + j] = nfd[j];
    }
}

__global__ void finalize_step_kernel(int32_t *__restrict__ state, const uint8_t *__restrict__ finished, int batch) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        int unf = 0;
        for (int b = 0; b < batch; ++b) unf += finished[b] ? 0 : 1;
        state[0] = state[0] + 1;
        state[1] = unf;
    }
}

}  // namespace

// ---- host launchers ------------------------------------------------------------------------------------
// ---- T5 (flan-t5) glue -----------------------------------------------------------------------------------
// Relative position bias table: tab[h][idx] = rel_w[bucket(idx - off)][h] (hf T5Attention.compute_bias :264-279).  The
// bucket of a distance >= max_exact is max_exact + #{thresholds <= distance}; the thresholds are computed on the host with
// the float32 formula of _relative_position_bucket :217-262 (same libm logf as the oracle), so the device needs no log.
struct T5Buckets {
    int bidirectional, nb, max_exact, nthr;
    int thr[32];
};
// state != null (decode step under a graph): the table of the single query at position state[0]: n = state[0] + 1 entries,
// entry idx = bias of key idx (off = state[0]); `stride` is the row stride of the table.
__global__ void t5_rel_table_kernel(const bf16 *__restrict__ rel_w, float *__restrict__ tab, int n, int off, int heads, T5Buckets bk,
                                    const int32_t *__restrict__ state, int stride) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (state) {
        off = state[0];
        n = min(off + 1, stride);
    }
    if (idx >= n) return;
    const int rel = idx - off;
    int ret = 0, rp;
    if (bk.bidirectional) {
        if (rel > 0) ret += bk.nb;
        rp = rel < 0 ? -rel : rel;
    } else {
        rp = rel < 0 ? -rel : 0;
    }
    int b = rp;
    if (rp >= bk.max_exact) {
        b = bk.max_exact;
        for (int i = 0; i < bk.nthr; ++i) b += rp >= bk.thr[i];
    }
    for (int h = 0; h < heads; ++h) tab[(int64_t)h * stride + idx] = (float)rel_w[(int64_t)(ret + b) * heads + h];
}
// gated activation: out = bf16(bf16(gelu_new(a)) * b), gelu_new = tanh form (hf activations NewGELUActivation);
// a = cols [0, F), b = cols [F, 2F) of rows of ld elements
__global__ __launch_bounds__(256) void gated_gelu_kernel(const bf16 *__restrict__ ab, int64_t ld, bf16 *__restrict__ out, int64_t rows, int F) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int ch = F >> 3;
    if (idx >= rows * ch) return;
    const int64_t r = idx / ch;
    const int c = (int)(idx - r * ch);
    const bf16x8 a = *reinterpret_cast<const bf16x8 *>(ab + r * ld + c * 8);
    const bf16x8 b = *reinterpret_cast<const bf16x8 *>(ab + r * ld + F + c * 8);
    bf16x8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float x = (float)a[e];
        const float u = 0.79788456080286535588f * (x + 0.044715f * x * x * x);
        const float t = 1.0f - 2.0f / (1.0f + __expf(2.0f * u));  // tanh(u), finite for any u
        const float g = 0.5f * x * (1.0f + t);
        o[e] = (bf16)((float)(bf16)g * (float)b[e]);
    }
    *reinterpret_cast<bf16x8 *>(out + r * F + c * 8) = o;
}
// rows (b, t) of a projection [M, ld] (columns col0 .. col0 + heads*hd) -> cache plane [B][H][cap][hd] at slots slot0 + t
__global__ __launch_bounds__(256) void rows_to_cache_kernel(const bf16 *__restrict__ src, int64_t ld, int col0, bf16 *__restrict__ plane,
                                                            int rows_per_b, int heads, int hd, int cap, int slot0,
                                                            const int32_t *__restrict__ state) {
    if (state) slot0 += state[0];
    const int64_t row = blockIdx.x;
    const int b = (int)(row / rows_per_b), t = (int)(row - (int64_t)b * rows_per_b);
    const int ch = hd >> 3;
    for (int c = threadIdx.x; c < heads * ch; c += 256) {
        const int hh = c / ch, cc = c - hh * ch;
        *reinterpret_cast<bf16x8 *>(plane + (((int64_t)b * heads + hh) * cap + slot0 + t) * hd + cc * 8) =
            *reinterpret_cast<const bf16x8 *>(src + row * ld + col0 + hh * hd + cc * 8);
    }
}

int launch_t5_rel_table(const bf16 *rel_w, float *tab, int n, int off, int heads, int bidirectional, int num_buckets, int max_dist,
                        hipStream_t s, const int32_t *state) {
    T5Buckets bk;
    int nb = num_buckets;
    if (bidirectional) nb /= 2;
    bk.bidirectional = bidirectional;
    bk.nb = nb;
    bk.max_exact = nb / 2;
    bk.nthr = 0;
    if (nb - bk.max_exact - 1 > 32) return EILEV_E_UNSUPPORTED;
    // thresholds: smallest distance whose bucket reaches max_exact + i, i = 1 .. nb - max_exact - 1 (float32 formula of hf :247-256)
    int prev = bk.max_exact;
    for (int rp = bk.max_exact; rp <= 2 * max_dist && prev < nb - 1; ++rp) {
        const float v = logf((float)rp / (float)bk.max_exact) / (float)log((double)max_dist / (double)bk.max_exact) * (float)(nb - bk.max_exact);
        int big = bk.max_exact + (int)v;
        if (big > nb - 1) big = nb - 1;
        while (prev < big) {
            bk.thr[bk.nthr++] = rp;
            ++prev;
        }
    }
    hipLaunchKernelGGL(t5_rel_table_kernel, dim3((n + 255) / 256), dim3(256), 0, s, rel_w, tab, n, off, heads, bk, state, n);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}
int launch_gated_gelu(const bf16 *ab, int64_t ld, bf16 *out, int64_t rows, int F, hipStream_t s) {
    if (F & 7) return EILEV_E_UNSUPPORTED;
    const int64_t total = rows * (F >> 3);
    hipLaunchKernelGGL(gated_gelu_kernel, dim3((unsigned)ceil_div64(total, 256)), dim3(256), 0, s, ab, ld, out, rows, F);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}
int launch_rows_to_cache(const bf16 *src, int64_t ld, int col0, bf16 *plane, int batch, int rows_per_b, int heads, int hd, int cap,
                         int slot0, hipStream_t s, const int32_t *state) {
    hipLaunchKernelGGL(rows_to_cache_kernel, dim3(batch * rows_per_b), dim3(256), 0, s, src, ld, col0, plane, rows_per_b, heads, hd, cap, slot0,
                       state);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}
int launch_im2col(const void *pix, int dtype, bf16 *out, int64_t rows, int frames, int img, int patch, int kp, hipStream_t s) {
    const int g = img / patch;
    const size_t strip_bytes = (size_t)3 * patch * img * sizeof(bf16);
    if (img == 224 && patch == 14 && rows % ((int64_t)g * g) == 0 && ((uintptr_t)pix & 15) == 0 && (dtype == EILEV_F32 || dtype == EILEV_BF16)) {
        const unsigned nblk = (unsigned)(rows / g);  // (frame, patch row) pairs
        if (dtype == EILEV_F32) hipLaunchKernelGGL((im2col_strip_kernel<float, 224, 14>), dim3(nblk), dim3(256), strip_bytes, s, (const float *)pix, out, frames, kp);
        else hipLaunchKernelGGL((im2col_strip_kernel<bf16, 224, 14>), dim3(nblk), dim3(256), strip_bytes, s, (const bf16 *)pix, out, frames, kp);
        EILEV_LAUNCH_CHECK();
        return EILEV_OK;
    }
    const int64_t total = rows * (kp >> 3);
    const dim3 grid((unsigned)ceil_div64(total, 256)), block(256);
    if (dtype == EILEV_F32) hipLaunchKernelGGL(im2col_kernel<float>, grid, block, 0, s, (const float *)pix, out, rows, frames, img, patch, kp);
    else if (dtype == EILEV_BF16) hipLaunchKernelGGL(im2col_kernel<bf16>, grid, block, 0, s, (const bf16 *)pix, out, rows, frames, img, patch, kp);
    else return EILEV_E_UNSUPPORTED;
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}
int launch_pad_rows(const bf16 *w, bf16 *out, int rows, int k, int kp, hipStream_t s) {
    hipLaunchKernelGGL(pad_rows_kernel, dim3((rows * kp + 255) / 256), dim3(256), 0, s, w, out, rows, k, kp);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}
int launch_cls_rows(const bf16 *cls, const bf16 *pos, bf16 *x, int64_t frames_total, int tok, int d, hipStream_t s) {
    hipLaunchKernelGGL(cls_rows_kernel, dim3((unsigned)ceil_div64(frames_total * d, 256)), dim3(256), 0, s, cls, pos, x, frames_total, tok, d);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}
int launch_broadcast_rows(const bf16 *src, bf16 *dst, int64_t copies, int64_t n, hipStream_t s) {
    hipLaunchKernelGGL(broadcast_rows_kernel, dim3((unsigned)ceil_div64(copies * n, 256)), dim3(256), 0, s, src, dst, copies, n);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}
int launch_embed_scatter(const bf16 *embed, const int64_t *ids, const uint8_t *mask, const bf16 *feats, int64_t n_rows,
                         int64_t total, int vocab, bf16 *out, int d, hipStream_t s) {
    hipLaunchKernelGGL(mask_rank_kernel, dim3(1), dim3(1024), 0, s, mask, out, total, d);
    EILEV_LAUNCH_CHECK();
    hipLaunchKernelGGL(embed_rows_kernel, dim3((unsigned)total), dim3(256), 0, s, embed, ids, feats, n_rows, vocab, out, d);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}
int launch_pos_embed(const bf16 *emb, const bf16 *pos, const int32_t *mask, int32_t *pid, bf16 *h, int batch, int L, int d, hipStream_t s,
                     int past) {
    // mask / pid cover all L positions; the rows of emb / h are the last L - past positions of every sequence
    hipLaunchKernelGGL(pos_ids_kernel, dim3(batch), dim3(1024), 0, s, mask, pid, L);
    EILEV_LAUNCH_CHECK();
    hipLaunchKernelGGL(add_pos_kernel, dim3(batch * (L - past)), dim3(256), 0, s, emb, pos, pid, h, d, L - past, L, past);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}
int launch_decode_embed(const bf16 *embed, const bf16 *pos, const int64_t *tokens, const int32_t *n_valid, const int32_t *state,
                        int vocab, int max_pid, bf16 *h, int batch, int d, hipStream_t s) {
    hipLaunchKernelGGL(decode_embed_kernel, dim3(batch), dim3(256), 0, s, embed, pos, tokens, n_valid, state, vocab, max_pid, h, d);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}
int launch_kv_write(const bf16 *qkv, bf16 *kc, bf16 *vc, int batch, int rows_per_b, int heads, int hd, int cap, int seq_len,
                    const int32_t *state, hipStream_t s, int slot0) {
    hipLaunchKernelGGL(kv_write_kernel, dim3(batch * rows_per_b), dim3(256), 0, s, qkv, kc, vc, rows_per_b, heads, hd, cap, seq_len, state, slot0);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}
int launch_topk_logprob(const float *logits, const float *row_score, int rows, int vocab, int keep, float *out_val, int32_t *out_idx, hipStream_t s) {
    if (vocab > 65536 || (vocab & 3) || keep < 1 || keep > 64 || (((uintptr_t)logits) & 15)) return EILEV_E_UNSUPPORTED;
    hipLaunchKernelGGL(topk_logprob_kernel, dim3(rows), dim3(1024), 0, s, logits, row_score, vocab, keep, out_val, out_idx);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}
int launch_beam_advance(const float *row_lp, const int32_t *row_tok, int batch, int beams, int keep, int max_new, const int32_t *state,
                        const int64_t *eos_ids, int n_eos, const float *len_pow, int recip, int early, int64_t *run_seq, float *run_score,
                        int64_t *fin_seq, float *fin_score, int64_t *fin_len, uint8_t *finished, uint8_t *can_improve, int64_t *tokens, int32_t *anc,
                        int gen_cap, int64_t *scratch, hipStream_t s) {
    if (beams * keep > 2048 || keep > 64 || beams > 32 || (anc && gen_cap * beams > 32 * 64) || n_eos > 8) return EILEV_E_UNSUPPORTED;
    BeamAdvanceArgs a;
    a.row_lp = row_lp; a.row_tok = row_tok; a.state = state; a.len_pow = len_pow;
    for (int e = 0; e < n_eos; ++e) a.eos[e] = eos_ids[e];  // (host array)
    a.n_eos = n_eos; a.beams = beams; a.keep = keep; a.T = max_new; a.early = early; a.recip = recip; a.gen_cap = gen_cap; a.batch = batch;
    a.run_seq = run_seq; a.fin_seq = fin_seq; a.fin_len = fin_len; a.tokens = tokens; a.scratch = scratch;
    a.run_score = run_score; a.fin_score = fin_score; a.finished = finished; a.can_improve = can_improve; a.anc = anc;
    hipLaunchKernelGGL(beam_advance_kernel, dim3(batch), dim3(256), 0, s, a);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}
int launch_select(const float *logits, int batch, int vocab, int32_t *state, uint8_t *finished, int64_t eos_id, int64_t pad_id,
                  int64_t *tokens, int64_t *out_tokens, int64_t max_new, hipStream_t s) {
    hipLaunchKernelGGL(select_kernel, dim3(batch), dim3(1024), 0, s, logits, vocab, state, finished, eos_id, pad_id, tokens, out_tokens, max_new,
                       batch == 1 ? 1 : 0);
    EILEV_LAUNCH_CHECK();
    if (batch == 1) return EILEV_OK;  // (the single block finished the step itself)
    hipLaunchKernelGGL(finalize_step_kernel, dim3(1), dim3(64), 0, s, state, finished, batch);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}

// ---- stage 0: frames -> pixel_values (include/eilev.h: eilev_process_frames) --------------------------------------------
// Pillow's 8-bit two-pass resample, bit-exact: per output byte the 22-bit fixed-point taps of its row of the coefficient
// table, 1 << 21 rounding, arithmetic shift, clip to 0..255; then the byte indexes the 3 x 256 normalisation table.
// HBM-bound byte work: one thread per output byte, adjacent threads read adjacent (horizontal pass: overlapping) bytes.
namespace {
constexpr int kResampleBits = 32 - 8 - 2;

__device__ __forceinline__ int clip8(int v) {
    v >>= kResampleBits;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// 4 adjacent output bytes per thread (one 4-byte store); w_out % 4 == 0
__global__ void resample_h_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst, const int32_t *__restrict__ coef,
                                  const int32_t *__restrict__ bounds, int ksize, int64_t rows, int w_in, int w_out) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int wq = w_out >> 2;
    if (idx >= rows * wq) return;
    const int64_t row = idx / wq;
    const int x0 = (int)(idx - row * wq) * 4;
    const uint8_t *srow = src + row * w_in;
    unsigned packed = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int xx = x0 + e;
        const int xmin = bounds[xx * 2], n = bounds[xx * 2 + 1];
        const int32_t *k = coef + (int64_t)xx * ksize;
        const uint8_t *s = srow + xmin;
        int ss = 1 << (kResampleBits - 1);
        for (int x = 0; x < n; ++x) ss += (int)s[x] * k[x];
        packed |= (unsigned)clip8(ss) << (8 * e);
    }
    *reinterpret_cast<unsigned *>(dst + row * w_out + x0) = packed;
}

// Horizontal pass, tiled: a workgroup stages 32 consecutive input rows (one contiguous block of the plane-major tensor, read
// with coalesced 16-byte loads) in LDS; thread xx owns output column xx of all 32 rows: each tap's coefficient is read once and
// applied to the 32 row accumulators (byte reads from LDS), the 32 x w_out result tile leaves through LDS as coalesced stores.
__global__ __launch_bounds__(256) void resample_h_tile_kernel(const uint8_t *__restrict__ src, uint8_t *__restrict__ dst,
                                                              const int32_t *__restrict__ coef, const int32_t *__restrict__ bounds, int ksize,
                                                              int64_t rows, int w_in, int w_out) {
    constexpr int R = 32;
    extern __shared__ __attribute__((aligned(16))) uint8_t rs_smem[];
    uint8_t *in = rs_smem;                                    // [R][w_in]
    uint8_t *outp = rs_smem + (((size_t)R * w_in + 15) & ~(size_t)15);  // [R][w_out]
    const int64_t row0 = (int64_t)blockIdx.x * R;
    const int nrow = (int)((rows - row0) < R ? (rows - row0) : R);
    const int64_t nbytes = (int64_t)nrow * w_in;
    const uint8_t *base = src + row0 * w_in;                  // 16-byte aligned: R * w_in is a multiple of 32
    for (int64_t i = (int64_t)threadIdx.x * 16; i < nbytes; i += 256 * 16) {
        if (i + 16 <= nbytes) *reinterpret_cast<uint4 *>(in + i) = *reinterpret_cast<const uint4 *>(base + i);
        else for (int64_t j = i; j < nbytes; ++j) in[j] = base[j];
    }
    __syncthreads();
    for (int xx = threadIdx.x; xx < w_out; xx += 256) {
        const int xmin = bounds[xx * 2], n = bounds[xx * 2 + 1];
        const int32_t *k = coef + (int64_t)xx * ksize;
        int acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = 1 << (kResampleBits - 1);
        for (int x = 0; x < n; ++x) {
            const int c = k[x];
            const uint8_t *s = in + xmin + x;
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] += (int)s[r * w_in] * c;
        }
#pragma unroll
        for (int r = 0; r < R; ++r) outp[r * w_out + xx] = (uint8_t)clip8(acc[r]);
    }
    __syncthreads();
    const int64_t obytes = (int64_t)nrow * w_out;             // contiguous in dst too; w_out % 4 == 0
    uint8_t *obase = dst + row0 * w_out;
    for (int64_t i = (int64_t)threadIdx.x * 4; i < obytes; i += 256 * 4)
        *reinterpret_cast<unsigned *>(obase + i) = *reinterpret_cast<const unsigned *>(outp + i);
}

// 4 adjacent columns per thread: 4-byte loads per tap, one 16-byte (fp32) / 8-byte (bf16) store; w % 4 == 0
template <typename OutT>
__global__ void resample_v_lut_kernel(const uint8_t *__restrict__ src, OutT *__restrict__ dst, const int32_t *__restrict__ coef,
                                      const int32_t *__restrict__ bounds, int ksize, const float *__restrict__ lut, int64_t planes,
                                      int frames, int h_in, int h_out, int w) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int wq = w >> 2;
    if (idx >= planes * h_out * wq) return;
    const int x = (int)(idx % wq) * 4;
    const int64_t py = idx / wq;
    const int yy = (int)(py % h_out);
    const int64_t p = py / h_out;
    int v[4];
    if (coef) {
        const int ymin = bounds[yy * 2], n = bounds[yy * 2 + 1];
        const int32_t *k = coef + (int64_t)yy * ksize;
        const uint8_t *s = src + (p * h_in + ymin) * w + x;
        int ss[4] = {1 << (kResampleBits - 1), 1 << (kResampleBits - 1), 1 << (kResampleBits - 1), 1 << (kResampleBits - 1)};
        for (int y = 0; y < n; ++y) {
            const unsigned q = *reinterpret_cast<const unsigned *>(s + (int64_t)y * w);
            const int kv = k[y];
#pragma unroll
            for (int e = 0; e < 4; ++e) ss[e] += (int)((q >> (8 * e)) & 255u) * kv;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = clip8(ss[e]);
    } else {
        const unsigned q = *reinterpret_cast<const unsigned *>(src + (p * h_in + yy) * w + x);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = (int)((q >> (8 * e)) & 255u);
    }
    const float *l = lut + ((p / frames) % 3) * 256;
    OutT *o = dst + (p * h_out + yy) * w + x;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = (OutT)l[v[e]];
}
}  // namespace

extern "C" size_t eilev_process_workspace_bytes(int64_t batch, int64_t frames, int64_t h_in, int64_t w_out) {
    return (size_t)(batch * 3 * frames * h_in * w_out);
}

extern "C" int eilev_process_frames(const uint8_t *video, int64_t batch, int64_t frames, int64_t h_in, int64_t w_in, int64_t h_out,
                                    int64_t w_out, const int32_t *coef_h, const int32_t *bounds_h, int32_t ksize_h,
                                    const int32_t *coef_v, const int32_t *bounds_v, int32_t ksize_v, const float *lut, void *out,
                                    int32_t out_dtype, void *workspace, size_t workspace_bytes, void *stream) {
    if (!video || !lut || !out || batch < 0 || frames < 0 || h_in <= 0 || w_in <= 0 || h_out <= 0 || w_out <= 0) return EILEV_E_BADARG;
    if ((!coef_h) != (!bounds_h) || (!coef_v) != (!bounds_v)) return EILEV_E_BADARG;
    if ((!coef_h && w_in != w_out) || (!coef_v && h_in != h_out)) return EILEV_E_BADARG;
    if (out_dtype != 0 && out_dtype != 1) return EILEV_E_UNSUPPORTED;
    if (frames > 0x7fffffff || h_in > 0x7fffffff || w_in > 0x7fffffff || h_out > 0x7fffffff || w_out > 0x7fffffff) return EILEV_E_UNSUPPORTED;
    if (w_out % 4 != 0 || ((uintptr_t)video & 3) || (!coef_h && (w_in & 3))) return EILEV_E_UNSUPPORTED;  // 4 columns per thread
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int64_t planes = batch * 3 * frames;
    if (planes == 0) return EILEV_OK;
    const uint8_t *mid = video;
    if (coef_h) {
        if (!workspace || workspace_bytes < eilev_process_workspace_bytes(batch, frames, h_in, w_out)) return EILEV_E_WORKSPACE;
        const int64_t rows = planes * h_in, total = rows * (w_out / 4);
        const size_t tile_lds = (((size_t)32 * w_in + 15) & ~(size_t)15) + (size_t)32 * w_out;
        if (tile_lds <= 64 * 1024 && ((uintptr_t)video & 15) == 0 && ((uintptr_t)workspace & 3) == 0)
            hipLaunchKernelGGL(resample_h_tile_kernel, dim3((unsigned)((rows + 31) / 32)), dim3(256), tile_lds, s, video, (uint8_t *)workspace, coef_h,
                               bounds_h, ksize_h, rows, (int)w_in, (int)w_out);
        else
            hipLaunchKernelGGL(resample_h_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, video, (uint8_t *)workspace, coef_h,
                               bounds_h, ksize_h, rows, (int)w_in, (int)w_out);
        EILEV_LAUNCH_CHECK();
        mid = (const uint8_t *)workspace;
    }
    const int64_t total = planes * h_out * (w_out / 4);
    if (out_dtype == 0)
        hipLaunchKernelGGL(resample_v_lut_kernel<float>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, mid, (float *)out, coef_v,
                           bounds_v, ksize_v, lut, planes, (int)frames, (int)h_in, (int)h_out, (int)w_out);
    else
        hipLaunchKernelGGL(resample_v_lut_kernel<bf16>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, mid, (bf16 *)out, coef_v,
                           bounds_v, ksize_v, lut, planes, (int)frames, (int)h_in, (int)h_out, (int)w_out);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}


// ---- per-row (per-token) dynamic quantisation of activations to OCP e4m3 (eilev_quant_rows_e4m3, include/eilev.h) -----------------
// scale[r] = absmax / 448 (1 for an all-zero row), q = e4m3_rne(clamp(x * (448 / absmax), +-448)).  One wave per row, two passes
// (the second read of the row hits L2); 16-byte loads, 8-byte stores.  HBM-bound: 2 bytes in, 1 byte out per element.
namespace {
__global__ __launch_bounds__(256) void quant_rows_e4m3_kernel(const bf16 *__restrict__ x, int64_t ldx, uint8_t *__restrict__ q, float *__restrict__ scale,
                                                              int64_t rows, int cols) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const bf16 *xr = x + row * ldx;
    const int nch = cols >> 3;
    float amax = 0.0f;
    for (int c = lane; c < nch; c += 64) {
        const bf16x8 t = *reinterpret_cast<const bf16x8 *>(xr + c * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) amax = fmaxf(amax, fabsf((float)t[e]));
    }
    amax = wave_max(amax);
    const float inv = amax > 0.0f ? 448.0f / amax : 0.0f;
    if (lane == 0) scale[row] = amax > 0.0f ? amax / 448.0f : 1.0f;
    uint8_t *qr = q + row * (int64_t)cols;
    for (int c = lane; c < nch; c += 64) {
        const bf16x8 t = *reinterpret_cast<const bf16x8 *>(xr + c * 8);
        float y[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) y[e] = fminf(fmaxf((float)t[e] * inv, -448.0f), 448.0f);
        int lo = 0, hi = 0;
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], lo, false);
        lo = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], lo, true);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], hi, false);
        hi = __builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], hi, true);
        *reinterpret_cast<int2 *>(qr + c * 8) = make_int2(lo, hi);
    }
}
}  // namespace

int launch_quant_rows_e4m3(const bf16 *x, int64_t ldx, uint8_t *q, float *scale, int64_t rows, int cols, hipStream_t s) {
    if (rows <= 0) return EILEV_OK;
    if (!x || !q || !scale) return EILEV_E_BADARG;
    if ((cols & 7) || (ldx & 7) || ((uintptr_t)x & 15) || ((uintptr_t)q & 7)) return EILEV_E_UNSUPPORTED;
    hipLaunchKernelGGL(quant_rows_e4m3_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, x, ldx, q, scale, rows, cols);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}

// attn_decode.hip — single-query attention of a decode step against the KV cache: the flash-decoding split kernel and its merge, the
// one-pass and 128-key-range kernels of small batches, the per-head loop of larger ones, and their launchers (common.h DecodeAttnArgs).
#include "attn_tile64.h"
#include "common.h"

namespace {

// ---- single-query attention against the cache (decode step) ---------------------------------------------
// Flash-decoding split: grid (heads, batch, nsplit); each workgroup owns KEYS_PER_WG = 256 consecutive cache
// slots of one (batch, head) and writes an un-normalised partial (max, sum, o[hd]) to `part`; a second tiny
// kernel merges the splits.  kv_total = seq_len + state[0] is read on the device (hipGraph replay); keys
// < seq_len obey attn_mask, newer ones are visible.  One key per thread for the scores (its whole K row:
// hd/8 independent 16-byte loads in flight), thread = (key subset, d chunk) for p.V; HBM-bound.
constexpr int DEC_KEYS = 256;

// T5 use: state == nullptr (kv_total = seq_len, given by the host), attn_mask may be null (every key visible), ldq = row
// stride of the query rows, rel_tab = per-head relative position bias over (key - query position), query at kv_total - 1.
__global__ __launch_bounds__(256) void attn_decode_split_kernel(const bf16 *__restrict__ qkv, const bf16 *__restrict__ kc,
                                                                const bf16 *__restrict__ vc, float *__restrict__ part,
                                                                const int32_t *__restrict__ attn_mask,
                                                                const int32_t *__restrict__ state, int seq_len, int cap,
                                                                int heads, int hd, int64_t ldq, const float *__restrict__ rel_tab,
                                                                int64_t rel_hs, int rel_off, int fuse_new,
                                                                const bf16 *__restrict__ kg = nullptr, const bf16 *__restrict__ vg = nullptr,
                                                                const int32_t *__restrict__ anc = nullptr, int beams = 1, int cap_g = 0,
                                                                int rows = 0) {
    // Beam search without moving the cache (anc != nullptr; eilev_opt_decode_step_beam): row b is beam b % beams of sample b / beams.
    // Keys [0, seq_len) are the sample's PROMPT, held once in the prefill cache (kc / vc: `cap` = its capacity, row = sample); key
    // seq_len + g is the g-th generated token of the hypothesis, written by whichever row held that hypothesis when it was generated:
    // physical row anc[g * rows + b] of the generation cache (kg / vg, capacity cap_g).  The new token goes to this row's own slot.
    __shared__ __attribute__((aligned(16))) float qs[128];
    __shared__ float sc[DEC_KEYS];
    __shared__ float red[DEC_KEYS * 17];  // per-key chunk partials (stride 17), later the p.V partials (nks * hd <= 2048)
    __shared__ float wred[4];
    __shared__ float bc[2];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int h = blockIdx.x, b = blockIdx.y, sp = blockIdx.z, nsplit = gridDim.z;
    const int d = heads * hd, nch = hd >> 3;
    const int kv_total = anc ? min(seq_len + cap_g, seq_len + state[0]) : min(cap, seq_len + (state ? state[0] : 0));
    const int k0 = sp * DEC_KEYS, k1 = min(kv_total, k0 + DEC_KEYS);
    const int srow = anc ? b / beams : b;  // row of the prompt cache and of the attention mask
    float *po = part + (((int64_t)b * heads + h) * nsplit + sp) * (hd + 2);
    if (k0 >= kv_total) {  // nothing in this split yet
        if (tid == 0) {
            po[0] = -1e30f;
            po[1] = 0.0f;
        }
        return;
    }
    const bf16 *kbase = kc + ((int64_t)srow * heads + h) * cap * hd;
    const bf16 *vbase = vc + ((int64_t)srow * heads + h) * cap * hd;
    auto key_row = [&](const bf16 *base, const bf16 *gen, int j) -> const bf16 * {
        if (!anc || j < seq_len) return base + (int64_t)j * hd;
        const int gi = j - seq_len;
        int a = anc[(int64_t)gi * rows + b];  // a table entry outside [0, rows) must not become an address (the host fills it: ADVICE r3)
        a = a < 0 ? 0 : (a >= rows ? rows - 1 : a);
        return gen + (((int64_t)a * heads + h) * cap_g + gi) * hd;
    };
    if (tid < hd) qs[tid] = (float)qkv[(int64_t)b * ldq + h * hd + tid];
    // fuse_new: the newest key / value (slot kv_total - 1) is still only in the q|k|v row of this step.  The split that owns the
    // slot reads it from there and stores it into the cache (what a separate kv_write launch did before the attention).
    // beam form: state[0] counts the generated tokens INCLUDING this step's, so it is >= 1 here; a caller that passes 0 (or more than the
    // generation cache holds: kv_total is clamped above) must not make this row write outside its own generation slots
    const int slot_raw = fuse_new ? kv_total - 1 : -1;
    const int slot_new = (anc && (slot_raw < seq_len || state[0] > cap_g)) ? -1 : slot_raw;
    const bf16 *knew = qkv + (int64_t)b * ldq + d + h * hd, *vnew = knew + d;
    if (slot_new >= k0 && slot_new < k1 && tid < 2 * nch) {
        const int which = tid / nch, cc = tid - which * nch;
        bf16 *dst = anc ? const_cast<bf16 *>(which ? vg : kg) + (((int64_t)b * heads + h) * cap_g + (slot_new - seq_len)) * hd + cc * 8
                        : const_cast<bf16 *>(which ? vbase : kbase) + (int64_t)slot_new * hd + cc * 8;
        *reinterpret_cast<bf16x8 *>(dst) = *reinterpret_cast<const bf16x8 *>((which ? vnew : knew) + cc * 8);
    }
    __syncthreads();

    // scores: thread = (key subset ks, d chunk c) so that consecutive lanes read consecutive 16-byte chunks (a K row is
    // hd * 2 = 160 contiguous bytes); the nch partial dot products of a key meet in LDS, then thread t owns key k0 + t
    const int nks = 256 / nch;
    const int c = tid % nch, ks = tid / nch;
    const int nkeys = k1 - k0;
    if (ks < nks) {
        const float4 q0 = *reinterpret_cast<const float4 *>(&qs[c * 8]);
        const float4 q1 = *reinterpret_cast<const float4 *>(&qs[c * 8 + 4]);
#pragma unroll 4
        for (int jj = ks; jj < nkeys; jj += nks) {
            float kv[8];
            unpack8(*reinterpret_cast<const bf16x8 *>((k0 + jj == slot_new ? knew : key_row(kbase, kg, k0 + jj)) + c * 8), kv);
            red[jj * 17 + c] = kv[0] * q0.x + kv[1] * q0.y + kv[2] * q0.z + kv[3] * q0.w + kv[4] * q1.x + kv[5] * q1.y + kv[6] * q1.z + kv[7] * q1.w;
        }
    }
    __syncthreads();
    const int j = k0 + tid;
    float s = -1e30f;
    if (j < k1) {
        float acc = 0.0f;
        for (int cc = 0; cc < nch; ++cc) acc += red[tid * 17 + cc];
        const bool vis = j >= seq_len || !attn_mask || attn_mask[(int64_t)srow * seq_len + j] != 0;
        if (rel_tab) acc += rel_tab[(int64_t)h * rel_hs + (rel_off >= 0 ? (j - (kv_total - 1)) + rel_off : j)];  // rel_off < 0: table of this query row
        s = vis ? acc : -1e30f;
    }
    float mxw = wave_max(s);
    if (lane == 0) wred[wid] = mxw;
    __syncthreads();
    const float mx = fmaxf(fmaxf(wred[0], wred[1]), fmaxf(wred[2], wred[3]));
    const float p = s > -1e29f ? __expf(s - mx) : 0.0f;
    sc[tid] = (float)(bf16)p;  // P rounded to bf16 like the prefill kernel's MFMA operand
    float sw = wave_sum(p);
    __syncthreads();
    if (lane == 0) wred[wid] = sw;
    __syncthreads();
    const float lsum = wred[0] + wred[1] + wred[2] + wred[3];

    // p.V: same (ks, c) mapping
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
    if (ks < nks) {
#pragma unroll 4
        for (int jj = ks; jj < nkeys; jj += nks) {
            float vv[8];
            unpack8(*reinterpret_cast<const bf16x8 *>((k0 + jj == slot_new ? vnew : key_row(vbase, vg, k0 + jj)) + c * 8), vv);
            const float pj = sc[jj];
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += pj * vv[e];
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) red[ks * hd + c * 8 + e] = acc[e];
    }
    __syncthreads();
    if (tid < hd) {
        float v = 0.0f;
        for (int k2 = 0; k2 < nks; ++k2) v += red[k2 * hd + tid];
        po[2 + tid] = v;
    }
    if (tid == 0) {
        po[0] = mx;
        po[1] = lsum;
    }
}

// ---- the register-resident key-range step of attn_decode1_kernel, attn_decode_part_kernel and attn_decode_loop_kernel, stated once -------------
// A workgroup of THREADS threads owns a range of up to KEYS keys [k0, k1) of one (row, head).  Thread (kg, c) = (tid / NCH, tid % NCH) owns
// 16-byte chunk c of keys k0 + kg, k0 + kg + G, ... (VK of them), all requested before anything is computed; thread t < KEYS owns key
// k0 + t for the softmax.  P is rounded to bf16 for the product, the row sum comes from the unrounded values.  The members are the thread's
// flash-decoding state (max, sum, its share of o): from the initial state ONE step leaves exactly the one-pass softmax (scale exp(-huge) = 0).
template <int NCH, int VK, int THREADS, int KEYS>
struct DecodeRange {
    static constexpr int hd = NCH * 8, G = THREADS / NCH, NW = THREADS / 64;
    static constexpr int RS = NCH + 1;  // row stride of the per-key chunk partials (odd: conflict-free column sums)
    static constexpr int RED = KEYS * RS > G * hd ? KEYS * RS : G * hd;  // red[]: [key][chunk] score partials, afterwards the p . V partials [key group][hd]
    static_assert(G * VK >= KEYS && KEYS <= THREADS, "every key of a range needs an owner");
    float m = -1e30f, l = 0.0f, acc[8] = {};

    // slot_new's row is `fresh` (the q|k|v row of this step), every other key's is row(key).  An index at or beyond k1 is clamped into the
    // range; what it loads is never used.
    template <class Row>
    static __device__ __forceinline__ void load(bf16x8 (&r)[VK], int k0, int k1, int slot_new, const bf16 *fresh, Row row) {
        const int c = threadIdx.x % NCH, kg = threadIdx.x / NCH;
#pragma unroll
        for (int i = 0; i < VK; ++i) {
            int key = k0 + kg + i * G;
            key = key < k1 ? key : k1 - 1;
            r[i] = *reinterpret_cast<const bf16x8 *>((key == slot_new ? fresh : row(key)) + c * 8);
        }
    }
    // the last 2 NCH threads copy the new token's K / V (the q|k|v row of this step) into its cache slot (what a separate kv_write launch did)
    static __device__ __forceinline__ void store_new(bf16 *kdst, bf16 *vdst, const bf16 *knew, const bf16 *vnew) {
        const int t2 = threadIdx.x - (THREADS - 2 * NCH), which = t2 / NCH, cc = t2 - which * NCH;
        if (t2 >= 0) *reinterpret_cast<bf16x8 *>((which ? vdst : kdst) + cc * 8) = *reinterpret_cast<const bf16x8 *>((which ? vnew : knew) + cc * 8);
    }
    // One range into (m, l, acc).  q0 | q1: elements c * 8 .. c * 8 + 7 of the query; between() runs once the score partials are written (the
    // loop kernel requests the next range's keys there); score_of(raw) is the score of key k0 + tid, -1e30 where it is not visible.  Ends
    // with ps, red and wred still in use: a barrier before the next step.
    template <class Between, class ScoreOf>
    __device__ __forceinline__ void step(const bf16x8 (&kr)[VK], const bf16x8 (&vr)[VK], const float4 q0, const float4 q1, int k0, int k1, float *red, float *ps,
                                         float *wred, Between between, ScoreOf score_of) {
        const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, c = tid % NCH, kg = tid / NCH;
        if (kg < G) {
#pragma unroll
            for (int i = 0; i < VK; ++i) {
                const int kk = kg + i * G;
                float kv[8];
                unpack8(kr[i], kv);
                if (kk < KEYS) red[kk * RS + c] = kv[0] * q0.x + kv[1] * q0.y + kv[2] * q0.z + kv[3] * q0.w + kv[4] * q1.x + kv[5] * q1.y + kv[6] * q1.z + kv[7] * q1.w;
            }
        }
        between();
        __syncthreads();
        float s = -1e30f;
        if (KEYS == THREADS || tid < KEYS) {
            float a = 0.0f;
#pragma unroll
            for (int cc = 0; cc < NCH; ++cc) a += red[tid * RS + cc];
            s = score_of(a);
        }
        const float mxw = wave_max(s);
        if (lane == 0) wred[wid] = mxw;
        __syncthreads();
        float mx = wred[0];
#pragma unroll
        for (int w = 1; w < NW; ++w) mx = fmaxf(mx, wred[w]);
        const float m_new = fmaxf(m, mx);
        const float p = s > -1e29f ? __expf(s - m_new) : 0.0f;
        if (KEYS == THREADS || tid < KEYS) ps[tid] = (float)(bf16)p;
        const float sw = wave_sum(p);
        if (lane == 0) wred[NW + wid] = sw;
        __syncthreads();  // (also: every thread has read its column of red[])
        float rs = wred[NW];
#pragma unroll
        for (int w = 1; w < NW; ++w) rs += wred[NW + w];
        const float scale = __expf(m - m_new);
        l = l * scale + rs;
        m = m_new;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] *= scale;
#pragma unroll
        for (int i = 0; i < VK; ++i) {
            const int kk = kg + i * G;
            const float pj = (kk < KEYS && k0 + kk < k1) ? ps[kk] : 0.0f;
            float vv[8];
            unpack8(vr[i], vv);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] += pj * vv[e];
        }
    }
    // the key groups' partial rows -> red[kg * hd + d] (a barrier inside); group_sum: their sum for output element d, in key-group order
    __device__ __forceinline__ void put_partials(float *red) const {
        const int c = threadIdx.x % NCH, kg = threadIdx.x / NCH;
        if (kg < G) {
#pragma unroll
            for (int e = 0; e < 8; ++e) red[kg * hd + c * 8 + e] = acc[e];
        }
        __syncthreads();
    }
    static __device__ __forceinline__ float group_sum(const float *red, int d) {
        float v = 0.0f;
        for (int k2 = 0; k2 < G; ++k2) v += red[k2 * hd + d];
        return v;
    }
};

// ---- small-batch form (round 4): ONE workgroup per (row, head), every key in one pass, no partials, no merge -------------------------------
// At batch 1 the split kernel above costs 13.9 us per block for 9.8 MB of keys and values (profiles/r04_decode_b1_kernel_stats.md): 128
// workgroups each walk three dependent load rounds, and the merge of their partials was repeated by every workgroup of out_proj.  Here a
// 1024-thread workgroup owns a head as ONE DecodeRange: the head's K and V (307 KB at 960 keys x 80) arrive in one round trip, the
// normalised row goes straight to `out`; the new token's K / V come from the q|k|v row and are stored to the cache here (fuse_new of the
// split kernel).  Needs cap <= 1024 and cap <= VK * (1024 / NCH).
template <int NCH, int VK>
__global__ __launch_bounds__(1024) void attn_decode1_kernel(const bf16 *__restrict__ qkv, bf16 *__restrict__ kc, bf16 *__restrict__ vc,
                                                            bf16 *__restrict__ out, const int32_t *__restrict__ attn_mask,
                                                            const int32_t *__restrict__ state, int seq_len, int cap, int heads, int64_t ldq) {
    using R = DecodeRange<NCH, VK, 1024, 1024>;  // one range [0, kv_total), kv_total <= cap <= 1024 = KEYS (G * VK may exceed it: those owners idle)
    constexpr int hd = R::hd, G = R::G;
    __shared__ __attribute__((aligned(16))) float qs[128];
    __shared__ float ps[1024];
    __shared__ float wred[32];
    __shared__ float red[R::RED];
    const int tid = threadIdx.x, c = tid % NCH;
    const int h = blockIdx.x, b = blockIdx.y, d = heads * hd;
    const int kv_total = min(cap, seq_len + state[0]);
    const int slot_new = kv_total - 1;
    bf16 *kbase = kc + ((int64_t)b * heads + h) * cap * hd, *vbase = vc + ((int64_t)b * heads + h) * cap * hd;
    const bf16 *knew = qkv + (int64_t)b * ldq + d + h * hd, *vnew = knew + d;
    // every load of the workgroup is requested here (one key row per thread instead would touch 64 cache lines per instruction and re-fetch
    // each of them NCH times: 15 us)
    bf16x8 kr[VK], vr[VK];
    R::load(kr, 0, kv_total, slot_new, knew, [&](int key) { return kbase + (int64_t)key * hd; });
    R::load(vr, 0, kv_total, slot_new, vnew, [&](int key) { return vbase + (int64_t)key * hd; });
    const bool vis = tid < kv_total && (tid >= seq_len || !attn_mask || attn_mask[(int64_t)b * seq_len + tid] != 0);
    if (tid < hd) qs[tid] = (float)qkv[(int64_t)b * ldq + h * hd + tid];
    R::store_new(kbase + (int64_t)slot_new * hd, vbase + (int64_t)slot_new * hd, knew, vnew);
    __syncthreads();
    R r;
    r.step(kr, vr, *reinterpret_cast<const float4 *>(&qs[c * 8]), *reinterpret_cast<const float4 *>(&qs[c * 8 + 4]), 0, kv_total, red, ps, wred, [] {},
           [&](float a) { return vis ? a : -1e30f; });
    r.put_partials(red);
    // G partial rows -> one: two levels (a single thread per output element walking all G partials is a chain of G dependent LDS reads:
    // ~5 us of the 12 this kernel took)
    constexpr int P2 = 1024 / hd;  // threads per output element in the first level
    const int dd = tid % hd, j = tid / hd;
    if (j < P2) {
        float v = 0.0f;
        for (int k2 = j; k2 < G; k2 += P2) v += red[k2 * hd + dd];
        ps[j * hd + dd] = v;  // (ps is free: every p was consumed before the barrier above; P2 * hd <= 1024)
    }
    __syncthreads();
    if (tid < hd) {
        float v = 0.0f;
#pragma unroll
        for (int jj = 0; jj < P2; ++jj) v += ps[jj * hd + tid];
        out[((int64_t)b * heads + h) * hd + tid] = (bf16)(r.l > 0.0f ? v / r.l : 0.0f);
    }
}

// DecodeRange over a RANGE of keys: 256 threads own keys [128 sp, 128 sp + 128) of one (row, head) and leave the un-normalised
// partial (max, sum, o[hd]) in `part` — the flash-decoding format of attn_decode_split_kernel, merged by the consumer (gemv1_kernel's prologue
// of out_proj).  One workgroup per head pulls 307 KB through ONE CU (12.1 us at batch 1); 8 splits put 38 KB on each of 256 CUs.
// BEAM (r4, eilev_opt_decode_step_beam at <= 8 rows of head size 80): the addressing of attn_decode_split_kernel's beam form — keys below
// seq_len in the prompt cache of sample b / beams, key seq_len + g in generation-cache row anc[g][b], the new token to this row's own slot —
// with this kernel's 128-key ranges and up-front loads: 5 rows x 32 heads x 8 ranges = 1280 workgroups where the 256-key split kernel ran 640
// of twice the length (15.3 us per block for 5 rows).
// WIN (the generated keys of the shared-prompt form, launch_attn_decode_shared): the ranges cover the key window that starts at seq_len —
// range sp = keys [seq_len + sp * KEYS, ..) — and their records are nos. rec0 + sp of the nrec that a (row, head) has; the prompt keys
// belong to attn_shared_prompt_kernel.
template <int NCH, int VK, bool BEAM = false, int KEYS = 128, bool WIN = false>
__global__ __launch_bounds__(256) void attn_decode_part_kernel(const bf16 *__restrict__ qkv, bf16 *__restrict__ kc, bf16 *__restrict__ vc,
                                                               float *__restrict__ part, const int32_t *__restrict__ attn_mask,
                                                               const int32_t *__restrict__ state, int seq_len, int cap, int heads, int64_t ldq,
                                                               bf16 *__restrict__ kg_ = nullptr, bf16 *__restrict__ vg_ = nullptr,
                                                               const int32_t *__restrict__ anc = nullptr, int beams = 1, int cap_g = 0, int rows = 0,
                                                               int rec0 = 0, int nrec = 0) {
    static_assert(BEAM || !WIN, "the key window is the generated keys of the beam form");
    using R = DecodeRange<NCH, VK, 256, KEYS>;
    constexpr int hd = R::hd;
    __shared__ __attribute__((aligned(16))) float qs[128];
    __shared__ float ps[KEYS];
    __shared__ float wred[8];
    __shared__ float red[R::RED];
    const int tid = threadIdx.x, c = tid % NCH;
    const int h = blockIdx.x, b = blockIdx.y, sp = blockIdx.z, nsplit = WIN ? nrec : gridDim.z, d = heads * hd;
    const int kv_total = BEAM ? min(seq_len + cap_g, seq_len + state[0]) : min(cap, seq_len + state[0]);
    // (beam form: a caller that passes a step count of 0, or more than the generation cache holds, must not make this row write outside its slots)
    const int slot_new = BEAM && (kv_total - 1 < seq_len || state[0] > cap_g) ? -1 : kv_total - 1;
    const int k0 = (WIN ? seq_len : 0) + sp * KEYS, k1 = min(kv_total, k0 + KEYS);
    float *po = part + (((int64_t)b * heads + h) * nsplit + (WIN ? rec0 : 0) + sp) * (hd + 2);
    if (k0 >= kv_total) {  // nothing in this split yet
        if (tid == 0) {
            po[0] = -1e30f;
            po[1] = 0.0f;
        }
        return;
    }
    const int srow = BEAM ? b / beams : b;  // row of the prompt cache and of the attention mask
    bf16 *kbase = kc + ((int64_t)srow * heads + h) * cap * hd, *vbase = vc + ((int64_t)srow * heads + h) * cap * hd;
    const bf16 *knew = qkv + (int64_t)b * ldq + d + h * hd, *vnew = knew + d;
    const int64_t rows_w = rows, heads_w = heads, cap_gw = cap_g;  // (widened once: the 12 row addresses of a thread share them)
    auto key_row = [&](const bf16 *base, const bf16 *gen, int j) -> const bf16 * {
        if (!BEAM || j < seq_len) return base + (int64_t)j * hd;
        const int gi = j - seq_len;
        int a = anc[gi * rows_w + b];  // (an entry outside [0, rows) must not become an address)
        a = a < 0 ? 0 : (a >= rows ? rows - 1 : a);
        return gen + ((a * heads_w + h) * cap_gw + gi) * hd;
    };
    bf16x8 kr[VK], vr[VK];
    R::load(kr, k0, k1, slot_new, knew, [&](int key) { return key_row(kbase, kg_, key); });
    R::load(vr, k0, k1, slot_new, vnew, [&](int key) { return key_row(vbase, vg_, key); });
    const int jt = k0 + tid;  // thread t < KEYS owns key k0 + t for the softmax
    const bool vis = tid < KEYS && jt < k1 && (jt >= seq_len || !attn_mask || attn_mask[(int64_t)srow * seq_len + jt] != 0);
    if (tid < hd) qs[tid] = (float)qkv[(int64_t)b * ldq + h * hd + tid];
    if (slot_new >= k0 && slot_new < k1) {  // the split that owns the newest slot stores it to the cache
        const int64_t at = BEAM ? (((int64_t)b * heads + h) * cap_g + (slot_new - seq_len)) * hd : (int64_t)slot_new * hd;
        R::store_new((BEAM ? kg_ : kbase) + at, (BEAM ? vg_ : vbase) + at, knew, vnew);
    }
    __syncthreads();
    R r;
    r.step(kr, vr, *reinterpret_cast<const float4 *>(&qs[c * 8]), *reinterpret_cast<const float4 *>(&qs[c * 8 + 4]), k0, k1, red, ps, wred, [] {},
           [&](float a) { return vis ? a : -1e30f; });
    r.put_partials(red);
    if (tid < hd) po[2 + tid] = R::group_sum(red, tid);
    if (tid == 0) {
        po[0] = r.m;
        po[1] = r.l;
    }
}

// ---- (round 5) any batch size: ONE workgroup per (row, head) walks the head's keys in ranges of KEYS (DecodeRange) ----------------------
// At batch 32 the 128-key ranges were 8192 workgroups + a merge launch (60.7 + 6.4 us per block), 256-key ranges 4096 + 5.0 us.  Here the
// 256 threads of a workgroup keep the flash-decoding state (max, sum, o) in registers across the ranges — the online form of the merge
// kernel's arithmetic — and request range r + 1's keys as soon as range r's scores exist (its values after p . V): no partials, no merge
// launch, the normalised row straight to `out`.  32 rows x 32 heads = 1024 workgroups = 4 per CU, all resident at once.
// (measured and not kept: 128-key ranges at 4 workgroups per CU, 4.33 against 4.28 ms / token; 256-key ranges forced to 128 registers spill)
template <int NCH, int VK, int KEYS>
__global__ __launch_bounds__(256) void attn_decode_loop_kernel(const bf16 *__restrict__ qkv, bf16 *__restrict__ kc, bf16 *__restrict__ vc,
                                                               bf16 *__restrict__ out, const int32_t *__restrict__ attn_mask,
                                                               const int32_t *__restrict__ state, int seq_len, int cap, int heads, int64_t ldq,
                                                               int out_frag, int fuse_new, const float *__restrict__ rel_tab = nullptr,
                                                               int64_t rel_hs = 0, int rel_off = 0) {
    // state == nullptr: kv_total = seq_len, given by the host (the flan-t5 cross-attention: keys = encoder positions, attn_mask = their
    // padding mask, q rows of stride ldq); fuse_new == 0: every key is in the cache already
    using R = DecodeRange<NCH, VK, 256, KEYS>;
    constexpr int hd = R::hd;
    __shared__ __attribute__((aligned(16))) float qs[128];
    __shared__ float ps[KEYS];
    __shared__ float wred[8];
    __shared__ float red[R::RED];
    const int tid = threadIdx.x, c = tid % NCH;
    const int h = blockIdx.x, b = blockIdx.y, d = heads * hd;
    const int kv_total = min(cap, seq_len + (state ? state[0] : 0));
    const int slot_new = fuse_new ? kv_total - 1 : -1;
    bf16 *kbase = kc + ((int64_t)b * heads + h) * cap * hd, *vbase = vc + ((int64_t)b * heads + h) * cap * hd;
    const bf16 *knew = qkv + (int64_t)b * ldq + d + h * hd, *vnew = knew + d;
    bf16x8 kr[VK], vr[VK];
    auto load_k = [&](int k0) { R::load(kr, k0, min(kv_total, k0 + KEYS), slot_new, knew, [&](int key) { return kbase + (int64_t)key * hd; }); };
    auto load_v = [&](int k0) { R::load(vr, k0, min(kv_total, k0 + KEYS), slot_new, vnew, [&](int key) { return vbase + (int64_t)key * hd; }); };
    load_k(0);
    load_v(0);
    if (tid < hd) qs[tid] = (float)qkv[(int64_t)b * ldq + h * hd + tid];
    if (fuse_new) R::store_new(kbase + (int64_t)slot_new * hd, vbase + (int64_t)slot_new * hd, knew, vnew);  // (fuse_new of the split kernel)
    __syncthreads();
    const float4 q0 = *reinterpret_cast<const float4 *>(&qs[c * 8]), q1 = *reinterpret_cast<const float4 *>(&qs[c * 8 + 4]);
    R r;
    for (int k0 = 0; k0 < kv_total; k0 += KEYS) {
        const int k1 = min(kv_total, k0 + KEYS);
        // (uniform) the next range's keys are requested as soon as this range's are consumed: in flight under its softmax and p . V
        r.step(
            kr, vr, q0, q1, k0, k1, red, ps, wred, [&] { if (k0 + KEYS < kv_total) load_k(k0 + KEYS); },
            [&](float a) {
                const int jt = k0 + tid;
                if (jt >= k1 || !(jt >= seq_len || !attn_mask || attn_mask[(int64_t)b * seq_len + jt] != 0)) return -1e30f;
                // (flan-t5 self-attention: per-head position bias over key - query position, the query at kv_total - 1; rel_off < 0: the table of this query row)
                if (rel_tab) a += rel_tab[(int64_t)h * rel_hs + (rel_off >= 0 ? (jt - (kv_total - 1)) + rel_off : jt)];
                return a;
            });
        if (k0 + KEYS < kv_total) load_v(k0 + KEYS);
        __syncthreads();  // ps / red / wred are rewritten by the next range
    }
    r.put_partials(red);
    if (tid < hd) {
        const float v = R::group_sum(red, tid);
        // out_frag: the row-block layout out_proj's GEMV reads at 17..32 rows (common.h frag32_index)
        out[out_frag ? frag32_index(b, h * hd + tid) : ((int64_t)b * heads + h) * hd + tid] = (bf16)(r.l > 0.0f ? v / r.l : 0.0f);
    }
}

__global__ __launch_bounds__(128) void attn_decode_merge_kernel(const float *__restrict__ part, bf16 *__restrict__ out,
                                                                int heads, int hd, int nsplit) {
    const int h = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const float *pp = part + ((int64_t)b * heads + h) * nsplit * (hd + 2);
    float mx = -1e30f;
    for (int s = 0; s < nsplit; ++s) mx = fmaxf(mx, pp[s * (hd + 2)]);
    float l = 0.0f, o = 0.0f;
    for (int s = 0; s < nsplit; ++s) {
        const float *ps = pp + s * (hd + 2);
        const float w = ps[1] > 0.0f ? __expf(ps[0] - mx) : 0.0f;
        l += w * ps[1];
        if (t < hd && w > 0.0f) o += w * ps[2 + t];
    }
    if (t < hd) out[((int64_t)b * heads + h) * hd + t] = (bf16)(l > 0.0f ? o / l : 0.0f);
}

// ---- flan-t5 beam search: the cross-attention of the `beams` rows of one sample over THAT SAMPLE's encoder keys -------------------------------
// The rows of a sample attend to the same K / V (eilev_t5_cross_kv writes them once per sample; nothing is replicated to the beams).  Grid
// (heads, samples, 128-key ranges): thread (kg, c) requests 16-byte chunk c of keys kg, kg + 32, kg + 64, kg + 96 of the range, K and V,
// straight to registers, ONCE, and keeps them while the sample's rows pass by in groups of 8: per group the scores of every row (the 8
// chunk products of a key meet by shuffles among 8 neighbouring lanes), a softmax per row (waves 0 / 1 own rows 0..3 of the group, waves
// 2 / 3 rows 4..7; thread = key), p . V with 8 x 8 accumulators, the key groups of a wave by shuffles, the four waves through LDS.  The
// arithmetic of the other decode kernels: no scale, P rounded to bf16 for the product, the row sum from the unrounded P.  Leaves (max, sum,
// o[64]) per (row, head, range) in the layout of attn_decode_part_bytes for attn_decode_merge_kernel.  Head size 64 only.
// Slots at / beyond enc_len are never requested (the index is clamped into the range); a masked key's K may be anything (its score is
// replaced before it is used) and its V is zeroed in registers, so 0 * NaN never reaches a sum.
constexpr int XS_ROWS = 8, XS_KEYS = 128;
__global__ __launch_bounds__(256) void attn_cross_shared_kernel(const bf16 *__restrict__ q, int64_t ldq, const bf16 *__restrict__ kc,
                                                                const bf16 *__restrict__ vc, float *__restrict__ part,
                                                                const int32_t *__restrict__ mask, int beams, int enc_len, int cap, int heads) {
    constexpr int hd = 64, G = 32, VK = 4, NR = XS_ROWS, KEYS = XS_KEYS;
    __shared__ __attribute__((aligned(16))) float qs[NR * hd];
    __shared__ float sc[NR * KEYS];  // the scores of a group's rows, then their P rounded to bf16
    __shared__ float wmax[NR * 2], wsum[NR * 2];
    __shared__ float wacc[4 * NR * hd];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int h = blockIdx.x, smp = blockIdx.y, sp = blockIdx.z, nsplit = gridDim.z;
    const int k0 = sp * KEYS, k1 = min(enc_len, k0 + KEYS);
    auto rec = [&](int row) { return part + (((int64_t)row * heads + h) * nsplit + sp) * (hd + 2); };
    if (k0 >= k1) {  // (the launcher sizes the grid by enc_len: not reached; a range with nothing in it)
        if (tid < beams) {
            float *po = rec(smp * beams + tid);
            po[0] = -1e30f;
            po[1] = 0.0f;
        }
        return;
    }
    const bf16 *kbase = kc + ((int64_t)smp * heads + h) * cap * hd, *vbase = vc + ((int64_t)smp * heads + h) * cap * hd;
    const int32_t *mrow = mask ? mask + (int64_t)smp * enc_len : nullptr;
    const int c = tid & 7, kg = tid >> 3;
    bf16x8 kr[VK], vr[VK];
#pragma unroll
    for (int i = 0; i < VK; ++i) {
        const int key = k0 + kg + i * G;
        kr[i] = *reinterpret_cast<const bf16x8 *>(kbase + (int64_t)(key < k1 ? key : k1 - 1) * hd + c * 8);
    }
#pragma unroll
    for (int i = 0; i < VK; ++i) {
        const int key = k0 + kg + i * G;
        vr[i] = *reinterpret_cast<const bf16x8 *>(vbase + (int64_t)(key < k1 ? key : k1 - 1) * hd + c * 8);
    }
    float kf[VK][8], vf[VK][8];
#pragma unroll
    for (int i = 0; i < VK; ++i) {
        const int key = k0 + kg + i * G;
        const bool vis = key < k1 && (!mrow || mrow[key < k1 ? key : k1 - 1] != 0);
        unpack8(kr[i], kf[i]);
        unpack8(vis ? vr[i] : zero8(), vf[i]);
    }
    const int key2 = tid & (KEYS - 1), half = tid >> 7;  // the softmax: thread = key, rows half * 4 .. half * 4 + 3 of the group
    const bool vis2 = k0 + key2 < k1 && (!mrow || mrow[k0 + key2] != 0);
    for (int r0 = 0; r0 < beams; r0 += NR) {
        const int nr = min(NR, beams - r0);
        for (int x = tid; x < nr * hd; x += 256) qs[x] = (float)q[(int64_t)(smp * beams + r0 + (x >> 6)) * ldq + h * hd + (x & 63)];
        __syncthreads();  // (also: the group before has read sc, wmax, wsum and wacc)
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            if (r < nr) {
                const float4 q0 = *reinterpret_cast<const float4 *>(&qs[r * hd + c * 8]), q1 = *reinterpret_cast<const float4 *>(&qs[r * hd + c * 8 + 4]);
#pragma unroll
                for (int i = 0; i < VK; ++i) {
                    const float *kv = kf[i];
                    float dot = kv[0] * q0.x + kv[1] * q0.y + kv[2] * q0.z + kv[3] * q0.w + kv[4] * q1.x + kv[5] * q1.y + kv[6] * q1.z + kv[7] * q1.w;
                    dot += __shfl_xor(dot, 1, 64);
                    dot += __shfl_xor(dot, 2, 64);
                    dot += __shfl_xor(dot, 4, 64);
                    if (c == 0) sc[r * KEYS + kg + i * G] = dot;
                }
            }
        }
        __syncthreads();
        float s4[NR / 2];
#pragma unroll
        for (int rr = 0; rr < NR / 2; ++rr) {
            const int r = half * (NR / 2) + rr;  // (uniform in a wave)
            s4[rr] = -1e30f;
            if (r < nr) {
                s4[rr] = vis2 ? sc[r * KEYS + key2] : -1e30f;
                const float m = wave_max(s4[rr]);
                if (lane == 0) wmax[r * 2 + (wid & 1)] = m;
            }
        }
        __syncthreads();
#pragma unroll
        for (int rr = 0; rr < NR / 2; ++rr) {
            const int r = half * (NR / 2) + rr;
            if (r < nr) {
                const float mx = fmaxf(wmax[r * 2], wmax[r * 2 + 1]);
                const float p = s4[rr] > -1e29f ? __expf(s4[rr] - mx) : 0.0f;
                sc[r * KEYS + key2] = (float)(bf16)p;  // P rounded to bf16 for the product; the row sum from the unrounded values
                const float sw = wave_sum(p);
                if (lane == 0) wsum[r * 2 + (wid & 1)] = sw;
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < NR; ++r) {
            if (r < nr) {
                float acc[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
#pragma unroll
                for (int i = 0; i < VK; ++i) {
                    const float pj = sc[r * KEYS + kg + i * G];  // (0 for a key at / beyond k1 and for a masked one)
#pragma unroll
                    for (int e = 0; e < 8; ++e) acc[e] += pj * vf[i][e];
                }
#pragma unroll
                for (int e = 0; e < 8; ++e) {  // the 8 key groups of a wave hold chunk c in lanes c, c + 8, ...
                    float v = acc[e];
                    v += __shfl_xor(v, 8, 64);
                    v += __shfl_xor(v, 16, 64);
                    v += __shfl_xor(v, 32, 64);
                    if (lane < 8) wacc[(wid * NR + r) * hd + c * 8 + e] = v;
                }
            }
        }
        __syncthreads();
        for (int x = tid; x < nr * hd; x += 256) {
            const int r = x >> 6, dd = x & 63;
            rec(smp * beams + r0 + r)[2 + dd] = (wacc[r * hd + dd] + wacc[(NR + r) * hd + dd]) + (wacc[(2 * NR + r) * hd + dd] + wacc[(3 * NR + r) * hd + dd]);
        }
        if (tid < nr) {
            float *po = rec(smp * beams + r0 + tid);
            po[0] = fmaxf(wmax[tid * 2], wmax[tid * 2 + 1]);
            po[1] = wsum[tid * 2] + wsum[tid * 2 + 1];
        }
    }
}

// ---- OPT beam search and generate(context=): the PROMPT keys of a sample, read once for its `beams` rows (DecodeAttnArgs.shared_prompt) ----------
// Grid (heads, samples, ranges of 64 TILES prompt keys).  The sample's rows are the queries of attn_tile64.h's 64 x 64 tile, stacked along M as
// prefix_attn_kernel stacks its rows: query slot wave * 16 + (lane & 15) is live below `beams` (rows <= 32: waves 2 and 3 only help staging).
// A tile's K and V come from HBM once into LDS; S^T = K Q^T and O^T = V^T P^T run on the 16x16x32 MFMA with the tile's arithmetic — no
// scale (q is pre-scaled), fp32 scores, P rounded to bf16 for the product, the row sum from the unrounded P.  Each live query leaves its
// un-normalised (max, sum, o[hd]) as record no. `range` of the nsplit that a (row, head) has (layout of attn_decode_part_bytes); the tile's
// scores are base-2, the record's maximum is the natural-log one attn_decode_merge_kernel takes.  A range in which a row sees nothing leaves
// (-1e30, 0).  Key j is visible iff j < seq_len and attn_mask[sample][j] != 0 (null: every key); slots at or beyond seq_len are never
// loaded; a masked key's K may hold anything (its score is dropped) and its V is zeroed in LDS, so 0 * NaN never reaches a sum.
template <int DP, int TILES>
__global__ __launch_bounds__(256) void attn_shared_prompt_kernel(const bf16 *__restrict__ qkv, int64_t ldq, const bf16 *__restrict__ kc,
                                                                 const bf16 *__restrict__ vc, float *__restrict__ part,
                                                                 const int32_t *__restrict__ attn_mask, int beams, int seq_len, int cap, int heads,
                                                                 int hd, int nsplit) {
    using Tile = AttnTile64<DP>;
    __shared__ __attribute__((aligned(16))) char ks_[Tile::KS_BYTES];
    __shared__ __attribute__((aligned(16))) char vt_[Tile::VT_BYTES];
    __shared__ int vis_[64];  // the tile's key is visible
    const int tid = threadIdx.x, wid = tid >> 6, l15 = tid & 15, lg = (tid & 63) >> 4;
    const int h = blockIdx.x, smp = blockIdx.y, sp = blockIdx.z;
    const int r0 = sp * 64 * TILES, r1 = min(seq_len, r0 + 64 * TILES);
    const int slot = wid * 16 + l15;
    const bool live = slot < beams, wave_live = wid * 16 < beams;
    const int row = smp * beams + (live ? slot : 0);
    Tile t;
    t.init(live, qkv + (int64_t)row * ldq + h * hd, hd);
    const bf16 *kb = kc + ((int64_t)smp * heads + h) * cap * hd, *vb = vc + ((int64_t)smp * heads + h) * cap * hd;
    const int32_t *mrow = attn_mask ? attn_mask + (int64_t)smp * seq_len : nullptr;
    for (int k0 = r0; k0 < r1; k0 += 64) {
        __syncthreads();  // everyone is done reading the previous tile
        Tile::stage(ks_, vt_, kb, hd, vb, hd, k0, r1, hd);
        bool hidden = false;
        if (tid < 64) {
            const int j = k0 + tid;
            const bool v = j < r1 && (!mrow || mrow[j] != 0);
            vis_[tid] = v;
            hidden = j < r1 && !v;
        }
        if (__syncthreads_or(hidden)) {  // (uniform) some staged key is masked: its V column out of the product
            for (int id = tid; id < 64 * DP; id += 256) {
                const int key = id & 63, dd = id >> 6;
                if (!vis_[key]) *reinterpret_cast<bf16 *>(vt_ + dd * Tile::VSTR + key * 2) = (bf16)0.0f;
            }
            __syncthreads();
        }
        if (wave_live)
            t.step(
                ks_, vt_, [&](int kl) { return vis_[kl] != 0; }, [](int, float s) { return s * 1.44269504088896340736f; }, [](int, float p) { return p; });
    }
    if (live) {  // o[dt][r] = O[q = l15][d = dt * 16 + lg * 4 + r]
        float *po = part + (((int64_t)row * heads + h) * nsplit + sp) * (hd + 2);
        if (lg == 0) {
            po[0] = t.l_run > 0.0f ? t.m_run * 0.69314718055994530942f : -1e30f;
            po[1] = t.l_run;
        }
#pragma unroll
        for (int dt = 0; dt < Tile::DT; ++dt) {
            const int d0 = dt * 16 + lg * 4;
            if (d0 < hd) {  // (records are 8-byte aligned: hd + 2 is even)
                *reinterpret_cast<float2 *>(po + 2 + d0) = make_float2(t.o[dt][0], t.o[dt][1]);
                *reinterpret_cast<float2 *>(po + 4 + d0) = make_float2(t.o[dt][2], t.o[dt][3]);
            }
        }
    }
}

}  // namespace

// The rows of a sample share its K / V (flan-t5 beam search): attn_cross_shared_kernel over 128-key ranges, then the merge.  q: `rows` query
// rows of stride ldq; kc / vc: planes [rows / beams][heads][cap][64], keys [0, enc_len); enc_mask (rows / beams, enc_len) or null.
int launch_attn_cross_shared(const bf16 *q, int64_t ldq, const bf16 *kc, const bf16 *vc, const int32_t *enc_mask, int rows, int beams, int heads,
                             int hd, int enc_len, int cap, bf16 *out, float *part, size_t part_bytes, hipStream_t s) {
    if (!q || !kc || !vc || !out || !part) return EILEV_E_BADARG;
    if (rows <= 0 || beams <= 0 || rows % beams || rows > 32 || beams > 32 || heads <= 0 || enc_len <= 0 || cap < enc_len || ldq < (int64_t)heads * hd)
        return EILEV_E_BADARG;
    if ((((uintptr_t)kc | (uintptr_t)vc) & 15) != 0) return EILEV_E_BADARG;  // (16-byte loads)
    if (hd != 64) return EILEV_E_UNSUPPORTED;
    if (part_bytes < attn_decode_part_bytes(rows, heads, hd, enc_len, XS_KEYS)) return EILEV_E_WORKSPACE;
    const int ns = (int)ceil_div64(enc_len, XS_KEYS);
    hipLaunchKernelGGL(attn_cross_shared_kernel, dim3(heads, rows / beams, ns), dim3(256), 0, s, q, ldq, kc, vc, part, enc_mask, beams, enc_len, cap, heads);
    EILEV_LAUNCH_CHECK();
    hipLaunchKernelGGL(attn_decode_merge_kernel, dim3(heads, rows), dim3(128), 0, s, part, out, heads, hd, ns);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}

// the partials of `nsplit` key ranges per (row, head) (layout of attn_decode_part_bytes) -> out [batch][heads * hd]
int launch_attn_decode_merge(const float *part, bf16 *out, int batch, int heads, int hd, int nsplit, hipStream_t s) {
    if (!part || !out || batch <= 0 || heads <= 0 || hd <= 0 || hd > 128 || nsplit <= 0) return EILEV_E_BADARG;
    hipLaunchKernelGGL(attn_decode_merge_kernel, dim3(heads, batch), dim3(128), 0, s, part, out, heads, hd, nsplit);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}

// ---- DecodeAttnArgs.shared_prompt: the beam form with the prompt part shared among a sample's rows ------------------------------------------
// Records per (row, head): [0, np) the prompt ranges of kSharedPromptKeys keys (attn_shared_prompt_kernel, one workgroup per (head, sample,
// range)), [np, np + ng) the 128-key ranges of the generated keys [seq_len, seq_len + cap_g) (attn_decode_part_kernel<.., BEAM, 128, WIN>, per
// row through the ancestor table: it stores and scores this step's K / V as the plain beam form does); one merge, or none where the caller
// merges (a.out == nullptr).
constexpr int kSharedGenKeys = 128;
int attn_decode_shared_nsplit(int seq_len, int cap_g) { return (int)(ceil_div64(seq_len, kSharedPromptKeys) + ceil_div64(cap_g, kSharedGenKeys)); }
size_t attn_decode_shared_part_bytes(int batch, int heads, int hd, int seq_len, int cap_g) {
    return sizeof(float) * (size_t)batch * heads * attn_decode_shared_nsplit(seq_len, cap_g) * (hd + 2);
}
static int launch_attn_decode_shared(const DecodeAttnArgs &a, hipStream_t s, int *nsplit) {
    if (!a.anc || !a.state || !a.fuse_new || a.rel_tab || a.out_frag) return EILEV_E_UNSUPPORTED;  // the beam form of a decode step only
    if (!a.qkv || !a.kc || !a.vc || !a.kg || !a.vg || !a.part) return EILEV_E_BADARG;
    if (a.batch <= 0 || a.batch > 32 || a.beams <= 0 || a.batch % a.beams || a.heads <= 0 || a.seq_len <= 0 || a.cap < a.seq_len || a.cap_g <= 0 ||
        a.q_stride() < 3 * (int64_t)a.heads * a.hd || (a.q_stride() & 7))
        return EILEV_E_BADARG;
    if ((((uintptr_t)a.qkv | (uintptr_t)a.kc | (uintptr_t)a.vc | (uintptr_t)a.kg | (uintptr_t)a.vg | (uintptr_t)a.part) & 15) != 0) return EILEV_E_BADARG;
    if (a.hd != 80 && a.hd != 128) return EILEV_E_UNSUPPORTED;
    if (a.part_bytes < attn_decode_shared_part_bytes(a.batch, a.heads, a.hd, a.seq_len, a.cap_g)) return EILEV_E_WORKSPACE;
    constexpr int TILES = kSharedPromptKeys / 64;
    const int np = (int)ceil_div64(a.seq_len, kSharedPromptKeys), ng = (int)ceil_div64(a.cap_g, kSharedGenKeys), ns = np + ng;
    const int64_t ldq = a.q_stride();
    bf16 *kc = const_cast<bf16 *>(a.kc), *vc = const_cast<bf16 *>(a.vc);
    const dim3 gp(a.heads, a.batch / a.beams, np), gg(a.heads, a.batch, ng);
    if (a.hd == 80) {
        hipLaunchKernelGGL((attn_shared_prompt_kernel<96, TILES>), gp, dim3(256), 0, s, a.qkv, ldq, a.kc, a.vc, a.part, a.attn_mask, a.beams, a.seq_len, a.cap,
                           a.heads, a.hd, ns);
        EILEV_LAUNCH_CHECK();
        hipLaunchKernelGGL((attn_decode_part_kernel<10, 6, true, kSharedGenKeys, true>), gg, dim3(256), 0, s, a.qkv, kc, vc, a.part, a.attn_mask, a.state,
                           a.seq_len, a.cap, a.heads, ldq, a.kg, a.vg, a.anc, a.beams, a.cap_g, a.batch, np, ns);
    } else {
        hipLaunchKernelGGL((attn_shared_prompt_kernel<128, TILES>), gp, dim3(256), 0, s, a.qkv, ldq, a.kc, a.vc, a.part, a.attn_mask, a.beams, a.seq_len, a.cap,
                           a.heads, a.hd, ns);
        EILEV_LAUNCH_CHECK();
        hipLaunchKernelGGL((attn_decode_part_kernel<16, 8, true, kSharedGenKeys, true>), gg, dim3(256), 0, s, a.qkv, kc, vc, a.part, a.attn_mask, a.state,
                           a.seq_len, a.cap, a.heads, ldq, a.kg, a.vg, a.anc, a.beams, a.cap_g, a.batch, np, ns);
    }
    EILEV_LAUNCH_CHECK();
    if (!a.out) {  // the caller merges the partials itself (gemv.hip: in the prologue of out_proj)
        *nsplit = ns;
        return EILEV_OK;
    }
    return launch_attn_decode_merge(a.part, a.out, a.batch, a.heads, a.hd, ns, s);
}

static int g_beam_part = 1;
static int g_attn_part32 = 1;  // 1 = by batch size (launch_attn_decode); probe build: 0 = the 256-key split kernel, 2 / 3 = force a form
#ifdef EILEV_PROBES
extern "C" int eilev_debug_attn_part32(int on) { g_attn_part32 = on; return 0; }  // probe: the 128-key up-front-load kernel at any batch size
extern "C" int eilev_debug_beam_part(int on) { g_beam_part = on; return 0; }  // probe / test switch: 0 = the 256-key split kernel for beam rows too (round 3)
#endif
size_t attn_decode_part_bytes(int batch, int heads, int hd, int keys, int range) {
    return sizeof(float) * (size_t)batch * heads * ceil_div64(keys, range) * (hd + 2);
}
// the launch takes attn_decode_loop_kernel (one workgroup per (row, head), no partials): the only form that can write the row-block layout
bool attn_decode_loop_ok(const DecodeAttnArgs &a) {
    return g_attn_part32 == 1 && !a.anc && a.out && a.state && a.fuse_new && !a.rel_tab && a.hd == 80 && a.keys() <= 2048 &&
           a.batch * a.heads >= 2 * eilev_num_cu() && a.batch <= 32;
}
int launch_attn_decode(const DecodeAttnArgs &a, hipStream_t s, int *nsplit) {
    if (!a.out && !nsplit) return EILEV_E_BADARG;  // partials are left only to a caller that merges them
    if (a.shared_prompt) return launch_attn_decode_shared(a, s, nsplit);  // (asked for: what it does not take is an error, never another kernel)
    if (a.out_frag && !attn_decode_loop_ok(a)) return EILEV_E_UNSUPPORTED;
    const int batch = a.batch, heads = a.heads, hd = a.hd, cap_all = a.keys();  // beam form: prompt keys (prefill cache) + generated keys (generation cache)
    if (hd > 128 || (hd & 7)) return EILEV_E_UNSUPPORTED;
    const int64_t ldq = a.q_stride();
    bf16 *kc = const_cast<bf16 *>(a.kc), *vc = const_cast<bf16 *>(a.vc);
    auto fits = [&](int range) { return a.part && a.part_bytes >= attn_decode_part_bytes(batch, heads, hd, cap_all, range); };
    auto merge = [&](int ns) {
        hipLaunchKernelGGL(attn_decode_merge_kernel, dim3(heads, batch), dim3(128), 0, s, a.part, a.out, heads, hd, ns);
        EILEV_LAUNCH_CHECK();
        return EILEV_OK;
    };
    if (a.anc && a.out && a.state && a.fuse_new && !a.rel_tab && hd == 80 && batch <= 8 && cap_all <= 2048 && g_beam_part) {
        // (r4) beam search at <= 8 rows: 128-key ranges with up-front loads (attn_decode_part_kernel<.., BEAM>), then the same merge
        const int ns = (int)ceil_div64(cap_all, 128);
        if (fits(128)) {
            hipLaunchKernelGGL((attn_decode_part_kernel<10, 6, true>), dim3(heads, batch, ns), dim3(256), 0, s, a.qkv, kc, vc, a.part, a.attn_mask, a.state,
                               a.seq_len, a.cap, heads, ldq, a.kg, a.vg, a.anc, a.beams, a.cap_g, batch);
            EILEV_LAUNCH_CHECK();
            return merge(ns);
        }
    }
    // (r5) hd 64 (flan-t5: the cross-attention over 960 encoder keys — state == nullptr, nothing to store — and the self-attention with its position bias): the per-head loop too
    if (g_attn_part32 == 1 && !a.anc && a.out && hd == 64 && batch * heads >= 2 * eilev_num_cu()) {
        hipLaunchKernelGGL((attn_decode_loop_kernel<8, 8, 256>), dim3(heads, batch), dim3(256), 0, s, a.qkv, kc, vc, a.out, a.attn_mask, a.state, a.seq_len,
                           a.cap, heads, ldq, 0, a.fuse_new, a.rel_tab, a.rel_hs, a.rel_off);
        EILEV_LAUNCH_CHECK();
        return EILEV_OK;
    }
    if (g_attn_part32 && !a.anc && a.out && a.state && a.fuse_new && !a.rel_tab && hd == 80 && cap_all <= 2048) {
        // (r5) plain decode steps of head size 80 at any batch size, same-box ms / token at batch 32: 256-key split kernel + merge 4.70,
        // 128-key up-front-load ranges + merge 4.61 (mode 1), 256-key ranges 4.38 (mode 2), one workgroup per head looping over 256-key
        // ranges with no partials and no merge 4.27 (mode 3, the default from 2 workgroups per CU; fewer rows keep the ranges: more workgroups)
        const int mode = g_attn_part32 != 1 ? g_attn_part32 : (batch * heads >= 2 * eilev_num_cu() ? 3 : 1);
        if (mode == 3) {
            hipLaunchKernelGGL((attn_decode_loop_kernel<10, 11, 256>), dim3(heads, batch), dim3(256), 0, s, a.qkv, kc, vc, a.out, a.attn_mask, a.state,
                               a.seq_len, a.cap, heads, ldq, a.out_frag, 1);
            EILEV_LAUNCH_CHECK();
            return EILEV_OK;
        }
        const int keys = mode == 2 ? 256 : 128;
        const int ns = (int)ceil_div64(cap_all, keys);
        if (fits(keys)) {
            if (keys == 256)
                hipLaunchKernelGGL((attn_decode_part_kernel<10, 11, false, 256>), dim3(heads, batch, ns), dim3(256), 0, s, a.qkv, kc, vc, a.part, a.attn_mask,
                                   a.state, a.seq_len, a.cap, heads, ldq, nullptr, nullptr, nullptr, 1, 0, batch);
            else
                hipLaunchKernelGGL((attn_decode_part_kernel<10, 6, false>), dim3(heads, batch, ns), dim3(256), 0, s, a.qkv, kc, vc, a.part, a.attn_mask,
                                   a.state, a.seq_len, a.cap, heads, ldq, nullptr, nullptr, nullptr, 1, 0, batch);
            EILEV_LAUNCH_CHECK();
            return merge(ns);
        }
    }
    const int ns = (int)ceil_div64(cap_all, DEC_KEYS);
    if (!fits(DEC_KEYS)) return EILEV_E_WORKSPACE;
    hipLaunchKernelGGL(attn_decode_split_kernel, dim3(heads, batch, ns), dim3(256), 0, s, a.qkv, a.kc, a.vc, a.part, a.attn_mask, a.state, a.seq_len, a.cap,
                       heads, hd, ldq, a.rel_tab, a.rel_hs, a.rel_off, a.fuse_new, a.kg, a.vg, a.anc, a.beams, a.cap_g, batch);
    EILEV_LAUNCH_CHECK();
    if (!a.out) {  // the caller merges the partials itself (gemv.hip: in the prologue of out_proj)
        *nsplit = ns;
        return EILEV_OK;
    }
    return merge(ns);
}
// plain decode step at small batch (no beams, no relative bias): true if the one-pass kernel took it
bool attn_decode1_ok(int batch, int cap, int hd) {
    if (batch > 8 || cap > 1024) return false;
    if (hd == 80) return cap <= 12 * (1024 / 10);
    if (hd == 64) return cap <= 8 * (1024 / 8);
    return false;  // (head size 128: 74 KB of static LDS for the partials — the split kernel)
}
int launch_attn_decode1(const DecodeAttnArgs &a, hipStream_t s) {
    if (!attn_decode1_ok(a.batch, a.cap, a.hd) || !a.state || !a.out) return EILEV_E_UNSUPPORTED;
    bf16 *kc = const_cast<bf16 *>(a.kc), *vc = const_cast<bf16 *>(a.vc);
    const dim3 grid(a.heads, a.batch);
    if (a.hd == 80) hipLaunchKernelGGL((attn_decode1_kernel<10, 12>), grid, dim3(1024), 0, s, a.qkv, kc, vc, a.out, a.attn_mask, a.state, a.seq_len, a.cap, a.heads, a.q_stride());
    else hipLaunchKernelGGL((attn_decode1_kernel<8, 8>), grid, dim3(1024), 0, s, a.qkv, kc, vc, a.out, a.attn_mask, a.state, a.seq_len, a.cap, a.heads, a.q_stride());
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}
int launch_attn_decode_part(const DecodeAttnArgs &a, hipStream_t s, int *nsplit) {
    if (a.hd != 80 || a.cap > 1024 || !a.state || !a.part) return EILEV_E_UNSUPPORTED;
    if (a.part_bytes < attn_decode_part_bytes(a.batch, a.heads, a.hd, a.cap)) return EILEV_E_WORKSPACE;
    const int ns = (int)ceil_div64(a.cap, 128);
    hipLaunchKernelGGL((attn_decode_part_kernel<10, 6>), dim3(a.heads, a.batch, ns), dim3(256), 0, s, a.qkv, const_cast<bf16 *>(a.kc), const_cast<bf16 *>(a.vc),
                       a.part, a.attn_mask, a.state, a.seq_len, a.cap, a.heads, a.q_stride());
    EILEV_LAUNCH_CHECK();
    *nsplit = ns;
    return EILEV_OK;
}

#ifdef EILEV_PROBES
// probe / test entry (tests/test_hip_attn_decode.py): ONE launch of a decode-attention launcher on the caller's buffers.  The struct is
// DecodeAttnArgs field by field as plain pointers and integers (the ctypes mirror lives with the tests); struct_bytes must be its size, so
// a stale mirror is refused instead of run.  launcher: 0 launch_attn_decode, 1 launch_attn_decode1, 2 launch_attn_decode_part.
struct EilevDebugAttnDecodeArgs {
    const void *qkv; int64_t ldq;
    const void *kc, *vc;
    void *out;
    const int32_t *attn_mask, *state;
    int32_t batch, seq_len, cap, heads, hd, fuse_new;
    float *part; uint64_t part_bytes;
    const float *rel_tab; int64_t rel_hs; int32_t rel_off, beams;
    void *kg, *vg;
    const int32_t *anc;
    int32_t cap_g, out_frag;
};
extern "C" int eilev_debug_attn_decode(const EilevDebugAttnDecodeArgs *args, size_t struct_bytes, int launcher, int *nsplit_out, void *stream) {
    if (!args || struct_bytes != sizeof(EilevDebugAttnDecodeArgs) || launcher < 0 || launcher > 2) return EILEV_E_BADARG;
    DecodeAttnArgs a;
    a.qkv = (const bf16 *)args->qkv; a.ldq = args->ldq;
    a.kc = (const bf16 *)args->kc; a.vc = (const bf16 *)args->vc;
    a.out = (bf16 *)args->out;
    a.attn_mask = args->attn_mask; a.state = args->state;
    a.batch = args->batch; a.seq_len = args->seq_len; a.cap = args->cap; a.heads = args->heads; a.hd = args->hd; a.fuse_new = args->fuse_new;
    a.part = args->part; a.part_bytes = (size_t)args->part_bytes;
    a.rel_tab = args->rel_tab; a.rel_hs = args->rel_hs; a.rel_off = args->rel_off; a.beams = args->beams;
    a.kg = (bf16 *)args->kg; a.vg = (bf16 *)args->vg;
    a.anc = args->anc;
    a.cap_g = args->cap_g; a.out_frag = args->out_frag;
    hipStream_t s = (hipStream_t)stream;
    if (launcher == 1) return launch_attn_decode1(a, s);
    if (launcher == 2) return nsplit_out ? launch_attn_decode_part(a, s, nsplit_out) : EILEV_E_BADARG;
    return launch_attn_decode(a, s, nsplit_out);
}
#endif

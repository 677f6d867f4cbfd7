// kv8.hip — the C ABI of include/eilev_kv8.h (libeilev_hip_kv8.so): the OPT decode step over a KV cache of e4m3 bytes with one power-of-two
// scale per head vector (the format is stated in the header).  The quantiser and the attention kernel are this unit's own; the rest of a
// block is opt.hip's (stages.h), the merge of the partials attn_decode.hip's — build.py links this unit with the core library's objects.
//
// attn_decode8_kernel.  The flash-decoding split of attn_decode_split_kernel for bytes: grid (heads, rows, ranges of 256 keys), a workgroup
// leaves (max, sum, o[hd]) of its range in the layout of attn_decode_part_bytes, attn_decode_merge_kernel finishes.  A head vector is
// NCH = hd / 16 chunks of 16 bytes.  Thread (kg, c) = (tid / NCH, tid % NCH) owns chunk c of keys k0 + kg, k0 + kg + G, ... (G = 256 / NCH
// key groups, VK keys each): consecutive lanes read consecutive chunks — a key's 80 or 128 bytes are one contiguous run — and all 2 VK
// loads of a thread (K and V) are requested before anything is computed: the kernel is bound by load latency and HBM bytes, a range is
// 40 / 64 KB in flight per workgroup.  The NCH partial dot products of a key meet in LDS; thread t owns key k0 + t for the softmax and
// applies both scales there: the score is multiplied by 2^ek, the bf16-rounded probability by 2^ev (exact in fp32), so the p . V loop is
// the bf16 kernels' with a byte conversion in front.
// fuse_new: the workgroup whose range owns slot kv_total - 1 quantises the step's K and V from the q|k|v row into that slot (waves 0 / 1,
// four elements per lane) and scores the slot from the bf16 row in this step.
// Every global read is behind an index check (key < k1, never the new slot, whose bytes may not be written yet); the only stores are the
// partials and the one new slot.
#include "../../include/eilev_kv8.h"
#include "stages.h"

namespace {

constexpr int KV8_KEYS = EILEV_KV8_RANGE;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;

// ---- the format ---------------------------------------------------------------------------------------------------------------------------
// where the planes of layer l are (host side)
struct Kv8Cache {
    size_t plane_e, plane_8, exp_off, total;  // exponents / bytes of the keys (or the values) of one layer; offset of the exponent planes
    Kv8Cache(int layers, int64_t batch, int heads, int hd, int64_t cap) {
        plane_e = (size_t)batch * heads * cap;
        plane_8 = plane_e * hd;
        exp_off = align_up(2 * (size_t)layers * plane_8, 256);
        total = align_up(exp_off + 2 * (size_t)layers * plane_e, 256);
    }
    uint8_t *k8(void *c, int l) const { return (uint8_t *)c + 2 * (size_t)l * plane_8; }
    uint8_t *v8(void *c, int l) const { return k8(c, l) + plane_8; }
    uint8_t *ek(void *c, int l) const { return (uint8_t *)c + exp_off + 2 * (size_t)l * plane_e; }
    uint8_t *ev(void *c, int l) const { return ek(c, l) + plane_e; }
};

// |x| as bits: for non-negative floats the integer order is the float order, and a NaN is larger than every number (it is not dropped, as
// fmaxf would drop it)
__device__ __forceinline__ uint32_t abs_bits(float x) { return __float_as_uint(x) & 0x7fffffffu; }
// the e8m0 byte e + 127 of a vector whose largest |x| has the bits `m`: the smallest e with amax <= 448 * 2^e = 1.75 * 2^(8 + e), e >= -126
__device__ __forceinline__ uint32_t exp_byte(uint32_t m) {
    const int E = (int)(m >> 23);
    if (m == 0 || E == 255) return 127;  // a zero vector, or a non-finite amax
    if (E == 0) return 1;                // (a subnormal amax: the clamp)
    const int e = E - 127 - ((m & 0x7fffffu) <= 0x600000u ? 8 : 7);
    return (uint32_t)((e < -126 ? -126 : e) + 127);
}
__device__ __forceinline__ float scale_of(uint32_t byte) { return __uint_as_float(byte << 23); }            // 2^e
__device__ __forceinline__ float inv_scale_of(uint32_t byte) { return __uint_as_float((254u - byte) << 23); }  // 2^-e (byte in [1, 247])
// four scaled values -> four e4m3 bytes (round to nearest even; |y| <= 448 by the choice of e)
__device__ __forceinline__ uint32_t pack4_e4m3(float y0, float y1, float y2, float y3) {
    int w = 0;
    w = __builtin_amdgcn_cvt_pk_fp8_f32(y0, y1, w, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(y2, y3, w, true);
    return (uint32_t)w;
}
// 16 e4m3 bytes -> 16 floats (exact)
__device__ __forceinline__ void unpack16_e4m3(const u32x4 &r, float (&f)[16]) {
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)r[w], false), hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)r[w], true);
        f[4 * w] = lo.x; f[4 * w + 1] = lo.y; f[4 * w + 2] = hi.x; f[4 * w + 3] = hi.y;
    }
}
__device__ __forceinline__ void unpack16_bf16(const bf16 *p, float (&f)[16]) {
    float a[8], b[8];
    unpack8(*reinterpret_cast<const bf16x8 *>(p), a);
    unpack8(*reinterpret_cast<const bf16x8 *>(p + 8), b);
#pragma unroll
    for (int e = 0; e < 8; ++e) { f[e] = a[e]; f[8 + e] = b[e]; }
}

// ---- eilev_kv8_quantize: 16 lanes per vector (hd / 8 of them hold 8 elements each), 16 vectors per workgroup -----------------------------
// vector v = ((layer, k | v, row, head) index ph, slot): both caches are [ph][cap][hd], so ph is the same number in both
template <int NCH8>
__global__ __launch_bounds__(256) void kv8_quantize_kernel(const bf16 *__restrict__ src, uint8_t *__restrict__ dst8, uint8_t *__restrict__ dst_e,
                                                           int64_t vectors, int slots, int src_cap, int dst_cap) {
    constexpr int hd = NCH8 * 8;
    const int tid = threadIdx.x, c = tid & 15;
    const int64_t v = (int64_t)blockIdx.x * 16 + (tid >> 4);
    const bool on = v < vectors && c < NCH8;
    const int64_t ph = v / slots;
    const int slot = (int)(v - ph * slots);
    float x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = 0.0f;
    if (on) unpack8(*reinterpret_cast<const bf16x8 *>(src + (ph * src_cap + slot) * hd + c * 8), x);
    uint32_t m = 0;
#pragma unroll
    for (int e = 0; e < 8; ++e) m = max(m, abs_bits(x[e]));
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));  // (the 16 lanes of the vector)
    const uint32_t byte = exp_byte(m);
    const float inv = inv_scale_of(byte);
    if (on) {
        const int64_t at = ph * dst_cap + slot;
        *reinterpret_cast<uint2 *>(dst8 + at * hd + c * 8) =
            make_uint2(pack4_e4m3(x[0] * inv, x[1] * inv, x[2] * inv, x[3] * inv), pack4_e4m3(x[4] * inv, x[5] * inv, x[6] * inv, x[7] * inv));
        if (c == 0) dst_e[at] = (uint8_t)byte;
    }
}

// ---- the attention ---------------------------------------------------------------------------------------------------------------------------
struct Attn8Args {
    const bf16 *qkv;  // q rows (stride ldq); with fuse_new the step's k and v follow q at heads * hd and 2 * heads * hd
    int64_t ldq;
    uint8_t *k8, *v8, *ek, *ev;  // the planes of one layer: [batch][heads][cap][hd] bytes, [batch][heads][cap] exponents
    float *part;
    const int32_t *attn_mask, *state;
    int seq_len, cap, heads, fuse_new;
};

template <int NCH>
__global__ __launch_bounds__(256) void attn_decode8_kernel(const Attn8Args a) {
    constexpr int hd = NCH * 16, G = 256 / NCH, VK = (KV8_KEYS + G - 1) / G, RS = NCH + 1;
    constexpr int RED = KV8_KEYS * RS > G * hd ? KV8_KEYS * RS : G * hd;  // [key][chunk] score partials, afterwards the p . V partials [key group][hd]
    constexpr int P2 = 256 / hd;                                           // threads per output element in the first level of the last sum
    static_assert(G * VK >= KV8_KEYS && P2 * hd <= KV8_KEYS, "every key of a range needs an owner");
    __shared__ float red[RED];
    __shared__ float ps[KV8_KEYS];
    __shared__ float wred[8];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, c = tid % NCH, kg = tid / NCH;
    const int h = blockIdx.x, b = blockIdx.y, sp = blockIdx.z, nsplit = gridDim.z;
    const int kv_total = min(a.cap, a.seq_len + (a.state ? a.state[0] : 0));
    const int k0 = sp * KV8_KEYS, k1 = min(kv_total, k0 + KV8_KEYS);
    float *po = a.part + (((int64_t)b * a.heads + h) * nsplit + sp) * (hd + 2);
    if (k0 >= kv_total) {  // nothing in this range yet
        if (tid == 0) {
            po[0] = -1e30f;
            po[1] = 0.0f;
        }
        return;
    }
    const int slot_new = a.fuse_new ? kv_total - 1 : -1;
    const int64_t vec0 = ((int64_t)b * a.heads + h) * a.cap;  // the first vector of this (row, head)
    uint8_t *kb = a.k8 + vec0 * hd, *vb = a.v8 + vec0 * hd, *ekb = a.ek + vec0, *evb = a.ev + vec0;
    const bf16 *qrow = a.qkv + (int64_t)b * a.ldq + h * hd, *knew = qrow + a.heads * hd, *vnew = knew + a.heads * hd;

    // every load of the thread is requested here
    u32x4 kr[VK], vr[VK];
#pragma unroll
    for (int i = 0; i < VK; ++i) {
        const int key = k0 + kg + i * G;
        const bool ld = kg < G && key < k1 && key != slot_new;
        kr[i] = ld ? *reinterpret_cast<const u32x4 *>(kb + (int64_t)key * hd + c * 16) : (u32x4){0, 0, 0, 0};
    }
#pragma unroll
    for (int i = 0; i < VK; ++i) {
        const int key = k0 + kg + i * G;
        const bool ld = kg < G && key < k1 && key != slot_new;
        vr[i] = ld ? *reinterpret_cast<const u32x4 *>(vb + (int64_t)key * hd + c * 16) : (u32x4){0, 0, 0, 0};
    }
    const int jt = k0 + tid;  // thread t owns key k0 + t for the softmax
    const bool own = jt < k1;
    float sk = 1.0f, sv = 1.0f;  // (the new slot is taken from the bf16 row: no scale)
    if (own && jt != slot_new) {
        sk = scale_of(ekb[jt]);
        sv = scale_of(evb[jt]);
    }
    const bool vis = own && (jt >= a.seq_len || !a.attn_mask || a.attn_mask[(int64_t)b * a.seq_len + jt] != 0);
    float q[16];
    unpack16_bf16(qrow + c * 16, q);

    // the range that owns the newest slot quantises the step's K (wave 0) and V (wave 1) into it
    if (slot_new >= k0 && slot_new < k1 && wid < 2) {
        const bf16 *src = wid ? vnew : knew;
        const bool on = lane < hd / 4;
        float x[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (on) {
            const bf16x4 t = *reinterpret_cast<const bf16x4 *>(src + lane * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) x[e] = (float)t[e];
        }
        uint32_t m = max(max(abs_bits(x[0]), abs_bits(x[1])), max(abs_bits(x[2]), abs_bits(x[3])));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
        const uint32_t byte = exp_byte(m);
        const float inv = inv_scale_of(byte);
        if (on) *reinterpret_cast<uint32_t *>((wid ? vb : kb) + (int64_t)slot_new * hd + lane * 4) = pack4_e4m3(x[0] * inv, x[1] * inv, x[2] * inv, x[3] * inv);
        if (lane == 0) (wid ? evb : ekb)[slot_new] = (uint8_t)byte;
    }

    // scores: the NCH chunk products of a key meet in LDS
    if (kg < G) {
#pragma unroll
        for (int i = 0; i < VK; ++i) {
            const int kk = kg + i * G;
            if (kk < KV8_KEYS) {
                float kf[16];
                if (k0 + kk == slot_new) unpack16_bf16(knew + c * 16, kf);
                else unpack16_e4m3(kr[i], kf);
                float dot = 0.0f;
#pragma unroll
                for (int e = 0; e < 16; ++e) dot += kf[e] * q[e];
                red[kk * RS + c] = dot;
            }
        }
    }
    __syncthreads();
    float s = -1e30f;
    if (vis) {
        float acc = 0.0f;
#pragma unroll
        for (int cc = 0; cc < NCH; ++cc) acc += red[tid * RS + cc];
        s = acc * sk;
    }
    const float mxw = wave_max(s);
    if (lane == 0) wred[wid] = mxw;
    __syncthreads();
    const float mx = fmaxf(fmaxf(wred[0], wred[1]), fmaxf(wred[2], wred[3]));
    const float p = s > -1e29f ? __expf(s - mx) : 0.0f;
    ps[tid] = p > 0.0f ? (float)(bf16)p * sv : 0.0f;  // P rounded to bf16 like the bf16 kernels', times the value scale (a power of two: exact)
    const float sw = wave_sum(p);
    if (lane == 0) wred[4 + wid] = sw;
    __syncthreads();  // (also: every thread has read its column of red[])
    const float lsum = (wred[4] + wred[5]) + (wred[6] + wred[7]);

    // p . V: same (kg, c) mapping
    float acc[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.0f;
    if (kg < G) {
#pragma unroll
        for (int i = 0; i < VK; ++i) {
            const int kk = kg + i * G;
            if (kk < KV8_KEYS) {
                float vf[16];
                if (k0 + kk == slot_new) unpack16_bf16(vnew + c * 16, vf);
                else unpack16_e4m3(vr[i], vf);  // (a key at or beyond k1: zeros, and p = 0)
                const float pj = ps[kk];
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[e] += pj * vf[e];
            }
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) red[kg * hd + c * 16 + e] = acc[e];
    }
    __syncthreads();
    // G partial rows -> one, in two levels (one thread per element walking all G rows is a chain of G dependent LDS reads)
    const int dd = tid % hd, j2 = tid / hd;
    if (j2 < P2) {
        float v = 0.0f;
        for (int k2 = j2; k2 < G; k2 += P2) v += red[k2 * hd + dd];
        ps[j2 * hd + dd] = v;  // (ps is free: every p was consumed before the barrier above)
    }
    __syncthreads();
    if (tid < hd) {
        float v = 0.0f;
#pragma unroll
        for (int jj = 0; jj < P2; ++jj) v += ps[jj * hd + tid];
        po[2 + tid] = v;
    }
    if (tid == 0) {
        po[0] = mx;
        po[1] = lsum;
    }
}

bool aligned16(const void *p) { return (((uintptr_t)p) & 15) == 0; }
bool hd_ok(int64_t hd) { return hd == 80 || hd == 128; }

// the partials of every (row, head, range) of `cap` slots, then their merge into out [batch][heads * hd]
int launch_attention8(const Attn8Args &a, int batch, int hd, bf16 *out, hipStream_t s) {
    const int ns = (int)ceil_div64(a.cap, KV8_KEYS);
    const dim3 grid((unsigned)a.heads, (unsigned)batch, (unsigned)ns);
    if (hd == 80) hipLaunchKernelGGL(attn_decode8_kernel<5>, grid, dim3(256), 0, s, a);
    else if (hd == 128) hipLaunchKernelGGL(attn_decode8_kernel<8>, grid, dim3(256), 0, s, a);
    else return EILEV_E_UNSUPPORTED;
    EILEV_LAUNCH_CHECK();
    return launch_attn_decode_merge(a.part, out, batch, a.heads, hd, ns, s);
}

bool step_shape_ok(const EilevDims *d, int64_t batch) { return d && batch > 0 && batch <= EILEV_KV8_MAX_ROWS && dims_ok_opt(d) && hd_ok(d->t_hidden / d->t_heads); }

}  // namespace

extern "C" int eilev_kv8_abi_version(void) { return EILEV_KV8_ABI_VERSION; }

extern "C" size_t eilev_kv8_cache_bytes(const EilevDims *d, int64_t batch, int64_t cap) {
    if (!d || batch <= 0 || cap <= 0 || cap > (1 << 20) || batch > (1 << 16) || !dims_ok_opt(d) || d->t_layers <= 0 || !hd_ok(d->t_hidden / d->t_heads)) return 0;
    return Kv8Cache(d->t_layers, batch, d->t_heads, d->t_hidden / d->t_heads, cap).total;
}

extern "C" size_t eilev_kv8_workspace_bytes(const EilevDims *d, int64_t batch) {
    if (!step_shape_ok(d, batch)) return 0;
    return carve_opt(d, batch, nullptr).used + 256;
}

extern "C" int eilev_kv8_quantize(const EilevDims *d, const void *kv_bf16, int64_t batch, int64_t src_cap, int64_t slots, void *kv8, int64_t dst_cap,
                                  void *stream) {
    if (!d || !kv_bf16 || !kv8 || batch <= 0 || batch > (1 << 16) || slots <= 0 || slots > src_cap || slots > dst_cap || src_cap > (1 << 20) || dst_cap > (1 << 20))
        return EILEV_E_BADARG;
    if (!aligned16(kv_bf16) || !aligned16(kv8)) return EILEV_E_BADARG;
    if (!dims_ok_opt(d) || d->t_layers <= 0) return EILEV_E_UNSUPPORTED;
    const int H = d->t_heads, hd = d->t_hidden / H;
    if (!hd_ok(hd)) return EILEV_E_UNSUPPORTED;
    const Kv8Cache c(d->t_layers, batch, H, hd, dst_cap);
    const int64_t vectors = 2 * (int64_t)d->t_layers * batch * H * slots;
    const int64_t blocks = ceil_div64(vectors, 16);
    if (blocks > 0x7fffffffll) return EILEV_E_BADARG;
    auto kernel = hd == 80 ? kv8_quantize_kernel<10> : kv8_quantize_kernel<16>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (const bf16 *)kv_bf16, c.k8(kv8, 0), c.ek(kv8, 0), vectors, (int)slots,
                       (int)src_cap, (int)dst_cap);
    EILEV_LAUNCH_CHECK();
    return EILEV_OK;
}

extern "C" int eilev_kv8_attention(const void *qkv, int64_t ldq, void *k8, void *v8, void *ek, void *ev, const int32_t *attn_mask, const int32_t *state,
                                   int64_t batch, int64_t seq_len, int64_t cap, int64_t heads, int64_t head_dim, int fuse_new, float *part,
                                   size_t part_bytes, void *out, void *stream) {
    if (!qkv || !k8 || !v8 || !ek || !ev || !part || !out) return EILEV_E_BADARG;
    if (batch <= 0 || batch > 4096 || heads <= 0 || heads > 1024 || head_dim <= 0 || head_dim > 1024 || seq_len < 0 || cap <= 0 || cap < seq_len || cap > (1 << 20))
        return EILEV_E_BADARG;
    const int64_t width = (fuse_new ? 3 : 1) * heads * head_dim;
    if (ldq < width || ldq > (1 << 24) || (ldq | head_dim) % 8) return EILEV_E_BADARG;
    if (!aligned16(qkv) || !aligned16(k8) || !aligned16(v8) || !aligned16(out) || (((uintptr_t)part) & 3)) return EILEV_E_BADARG;
    if (!hd_ok(head_dim)) return EILEV_E_UNSUPPORTED;
    if (part_bytes < attn_decode_part_bytes((int)batch, (int)heads, (int)head_dim, (int)cap, KV8_KEYS)) return EILEV_E_WORKSPACE;
    Attn8Args a;
    a.qkv = (const bf16 *)qkv; a.ldq = ldq; a.k8 = (uint8_t *)k8; a.v8 = (uint8_t *)v8; a.ek = (uint8_t *)ek; a.ev = (uint8_t *)ev;
    a.part = part; a.attn_mask = attn_mask; a.state = state; a.seq_len = (int)seq_len; a.cap = (int)cap; a.heads = (int)heads; a.fuse_new = fuse_new ? 1 : 0;
    return launch_attention8(a, (int)batch, (int)head_dim, (bf16 *)out, (hipStream_t)stream);
}

// eilev_opt_decode_step (opt.hip) on the MFMA weight-streaming kernels at every row count, with this unit's attention in place of
// launch_attn_decode; activations row-major (the row-block layout of 17..32 rows belongs to attn_decode_loop_kernel)
extern "C" int eilev_kv8_decode_step(const EilevDims *d, const EilevOptWeights *w, int64_t *tokens, int32_t *state, const int32_t *attn_mask,
                                     const int32_t *n_valid, int64_t batch, int64_t seq_len, void *kv8, int64_t kv_capacity, float *logits,
                                     uint8_t *finished, int64_t eos_id, int64_t pad_id, int64_t *out_tokens, int64_t max_new, void *workspace,
                                     size_t workspace_bytes, void *stream) {
    if (!d || !w || !tokens || !state || !attn_mask || !n_valid || !kv8 || !logits || !finished || !out_tokens || !workspace) return EILEV_E_BADARG;
    if (batch <= 0 || batch > EILEV_KV8_MAX_ROWS || seq_len <= 0 || kv_capacity > (1 << 20) || seq_len + max_new > kv_capacity + 1 || !aligned16(kv8))
        return EILEV_E_BADARG;
    if (!step_shape_ok(d, batch) || d->t_layers <= 0) return EILEV_E_UNSUPPORTED;
    if (workspace_bytes < eilev_kv8_workspace_bytes(d, batch)) return EILEV_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int D = d->t_hidden, H = d->t_heads, hd = D / H;
    if (attn_decode_part_bytes((int)batch, H, hd, (int)kv_capacity, KV8_KEYS) > kSkinnyHalf) return EILEV_E_WORKSPACE;
    const OptBufs b = carve_opt(d, batch, workspace);
    RC(launch_decode_embed((const bf16 *)w->embed_tokens, (const bf16 *)w->embed_positions, tokens, n_valid, state, d->vocab, d->max_pos + 1, b.h,
                           (int)batch, D, s));
    const Kv8Cache kv(d->t_layers, batch, H, hd, kv_capacity);
    const DecodeAttnArgs half = decode_attn_args(b.qkv, b.att, b.scratch, batch, H, hd);  // (the partials: the second half of the skinny scratch)
    Attn8Args a;
    a.qkv = b.qkv; a.ldq = 3 * (int64_t)D; a.part = half.part; a.attn_mask = attn_mask; a.state = state; a.seq_len = (int)seq_len; a.cap = (int)kv_capacity;
    a.heads = H; a.fuse_new = 1;
    for (int l = 0; l < d->t_layers; ++l) {
        const EilevOptLayer *L = &w->layers[l];
        if (l == 0) RC(launch_layernorm(b.h, D, (const bf16 *)L->ln1_w, (const bf16 *)L->ln1_b, b.x, D, batch, D, d->t_eps, s));
        RC(opt_qkv(d, w, l, b, batch, s));
        a.k8 = kv.k8(kv8, l); a.v8 = kv.v8(kv8, l); a.ek = kv.ek(kv8, l); a.ev = kv.ev(kv8, l);
        RC(launch_attention8(a, (int)batch, hd, b.att, s));
        // the block's output goes straight into the LayerNorm that reads it next (the next block's, or final_layer_norm): b.x
        const bool last = l + 1 == d->t_layers;
        RC(opt_tail(d, w, l, b, batch, s, last ? w->final_ln_w : w->layers[l + 1].ln1_w, last ? w->final_ln_b : w->layers[l + 1].ln1_b));
    }
    GemmArgs g = sk_gemm(b.scratch, b.x, D, w->embed_tokens, D, nullptr, nullptr, 0, logits, d->vocab, batch, d->vocab, D, 0);
    g.out_f32 = 1;
    if (w->lm_head_stream && batch > 16 && batch <= 32) g.Wp = (const bf16 *)w->lm_head_stream;
    RC(launch_gemm(g, 5, s));
    return launch_select(logits, (int)batch, d->vocab, state, finished, eos_id, pad_id, tokens, out_tokens, max_new, s);
}

// attn_tile64.h — the 64-query x 64-key flash tile of attn_prefill_kernel (attention.hip) and prefix_attn_kernel (prefix.hip), stated once.
//
// A workgroup of 4 waves owns 64 queries of one head.  A tile of 64 keys is staged in LDS (K row-major, V transposed, head sizes zero-padded
// to DP in {64, 96, 128}).  Scores are computed TRANSPOSED, S^T = K Q^T, so that after the 16x16x32 MFMA each lane owns one query
// (col = lane & 15) and 16 of the tile's 64 keys: the online-softmax statistics are per-lane scalars (+2 cross-lane-group shuffles) and the
// probabilities are already in the B-operand layout of the second MFMA, O^T = V^T P^T (MFMA k-slots are an arbitrary but consistent
// permutation of the keys) — no LDS round trip for P.  fp32 softmax, P rounded to bf16 for the product, the row sum from the unrounded P,
// fp32 accumulate, O / l rounded to bf16 once; a query without a visible key writes zeros.  The kernels keep their addressing, LDS arrays,
// mask words, barriers and key loops.  Templates only: prefix.o is linked with attention.o into one library.
#pragma once
#include "common.h"

template <int DP>
struct AttnTile64 {
    static constexpr int KD = DP / 32;        // MFMA k-steps over the head dim
    static constexpr int DT = DP / 16;        // 16-row tiles of O^T
    static constexpr int CH = DP / 8;         // 16-byte chunks per K/V row
    static constexpr int KSTR = DP * 2 + 16;  // LDS row stride of the K tile (bytes): +16 keeps b128 reads conflict-free
    static constexpr int VSTR = 64 * 2 + 16;  // LDS row stride of the transposed V tile (64 keys per row)
    static constexpr int KS_BYTES = 64 * KSTR, VT_BYTES = DP * VSTR;

    bf16x8 qf[KD];  // this lane's query (wave wid, col l15), the B operand of S^T = K Q^T
    float m_run = -1e30f, l_run = 0.0f;
    f32x4 o[DT] = {};

    __device__ __forceinline__ void init(bool live, const bf16 *q, int hd) {  // q: the lane's query row, read only where live
        const int lg = (threadIdx.x & 63) >> 4;
#pragma unroll
        for (int kd = 0; kd < KD; ++kd) {
            const int d0 = kd * 32 + lg * 8;
            qf[kd] = (live && d0 < hd) ? *reinterpret_cast<const bf16x8 *>(q + d0) : zero8();
        }
    }

    // keys [k0, k0 + 64) n [0, kend) of the key rows kb / vb (row strides ldk / ldv elements) -> ks / vt; zeros elsewhere
    static __device__ __forceinline__ void stage(char *ks, char *vt, const bf16 *kb, int64_t ldk, const bf16 *vb, int64_t ldv, int k0, int kend, int hd) {
        const int tid = threadIdx.x;
        // ---- stage K (row-major, coalesced 16-byte loads)
        for (int id = tid; id < 64 * CH; id += 256) {
            const int key = id / CH, c = id - key * CH;
            const int gk = k0 + key;
            bf16x8 val = (gk < kend && c * 8 < hd) ? *reinterpret_cast<const bf16x8 *>(kb + (int64_t)gk * ldk + c * 8) : zero8();
            *reinterpret_cast<bf16x8 *>(ks + key * KSTR + c * 16) = val;
        }
        // ---- stage V transposed: vt[d][key]
        for (int id = tid; id < 64 * CH; id += 256) {
            const int key = id & 63, c = id >> 6;
            const int gk = k0 + key;
            bf16x8 val = (gk < kend && c * 8 < hd) ? *reinterpret_cast<const bf16x8 *>(vb + (int64_t)gk * ldv + c * 8) : zero8();
#pragma unroll
            for (int e = 0; e < 8; ++e) *reinterpret_cast<bf16 *>(vt + (c * 8 + e) * VSTR + key * 2) = val[e];
        }
    }

    // One staged tile into (m, l, o).  Tile-local key kl: vis(kl) = the lane's query sees it, score(kl, raw dot product) = its base-2 score,
    // pmap(kl, p) = what multiplies V once p is in the row sum (identity, or dropout).
    template <class Vis, class Score, class PMap>
    __device__ __forceinline__ void step(const char *ks, const char *vt, Vis vis, Score score, PMap pmap) {
        const int lane = threadIdx.x & 63, l15 = lane & 15, lg = lane >> 4;
        // ---- S^T = K Q^T : st[ct][r] = S[q = l15][key = ct*16 + lg*4 + r]
        f32x4 st[4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct) {
            st[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kd = 0; kd < KD; ++kd) {
                const bf16x8 kf = *reinterpret_cast<const bf16x8 *>(ks + (ct * 16 + l15) * KSTR + (kd * 4 + lg) * 16);
                st[ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[kd], st[ct], 0, 0, 0);
            }
        }
        // ---- mask, online softmax (per-lane row statistics)
        float mx = -1e30f;
        bool okv[4][4];
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int kl = ct * 16 + lg * 4 + r;
                const bool ok = vis(kl);
                okv[ct][r] = ok;
                const float s = score(kl, st[ct][r]);
                st[ct][r] = s;
                if (ok) mx = fmaxf(mx, s);
            }
        mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);
        const float alpha = exp2f(m_run - m_new);
        float rs = 0.0f;
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = okv[ct][r] ? exp2f(st[ct][r] - m_new) : 0.0f;
                rs += p;
                st[ct][r] = pmap(ct * 16 + lg * 4 + r, p);
            }
        rs += __shfl_xor(rs, 16, 64);
        rs += __shfl_xor(rs, 32, 64);
        l_run = l_run * alpha + rs;
        m_run = m_new;
#pragma unroll
        for (int i = 0; i < DT; ++i) o[i] *= alpha;

        // ---- O^T += V^T P^T.  k-slot (lg, j) of step ks2  <->  key 32 ks2 + (j < 4 ? lg*4 + j : 16 + lg*4 + j - 4)
        bf16x8 pb[2];
#pragma unroll
        for (int ks2 = 0; ks2 < 2; ++ks2)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pb[ks2][j] = (bf16)st[2 * ks2][j];
                pb[ks2][4 + j] = (bf16)st[2 * ks2 + 1][j];
            }
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            const char *vrow = vt + (dt * 16 + l15) * VSTR + lg * 8;
#pragma unroll
            for (int ks2 = 0; ks2 < 2; ++ks2) {
                const bf16x4 lo = *reinterpret_cast<const bf16x4 *>(vrow + ks2 * 64);
                const bf16x4 hi = *reinterpret_cast<const bf16x4 *>(vrow + ks2 * 64 + 32);
                bf16x8 vf;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    vf[j] = lo[j];
                    vf[4 + j] = hi[j];
                }
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pb[ks2], o[dt], 0, 0, 0);
            }
        }
    }

    // ---- finalize: o[dt][r] = O[q = l15][d = dt*16 + lg*4 + r] -> op, the lane's output row (head offset applied)
    __device__ __forceinline__ void store(bf16 *op, int hd) const {
        const int lg = (threadIdx.x & 63) >> 4;
        const float inv = l_run > 0.0f ? 1.0f / l_run : 0.0f;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            const int d0 = dt * 16 + lg * 4;
            if (d0 < hd) {
                bf16x4 w;
#pragma unroll
                for (int r = 0; r < 4; ++r) w[r] = (bf16)(o[dt][r] * inv);
                *reinterpret_cast<bf16x4 *>(op + d0) = w;
            }
        }
    }
};

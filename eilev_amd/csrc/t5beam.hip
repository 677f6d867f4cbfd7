// t5beam.hip — the C ABI of include/eilev_t5beam.h (libeilev_hip_t5beam.so): the flan-t5 decode step of beam search and its shared-sample
// cross-attention.  Argument checks only; the step is t5.hip's t5_decode_step_beam, the kernel attn_decode.hip's — build.py links this unit
// with the core library's objects.
#include "../../include/eilev_t5beam.h"
#include "stages.h"

extern "C" int eilev_t5beam_abi_version(void) { return EILEV_T5BEAM_ABI_VERSION; }

static bool rows_ok(int64_t rows, int64_t beams) { return rows > 0 && beams > 0 && rows <= 32 && beams <= 32 && rows % beams == 0; }

extern "C" size_t eilev_t5beam_workspace_bytes(const EilevT5Dims *d, int64_t rows, int64_t beams, int64_t enc_len, int64_t gen_capacity) {
    if (!d || !rows_ok(rows, beams) || enc_len <= 0 || gen_capacity <= 0) return 0;
    return t5_decode_step_beam_workspace_bytes(d, rows, enc_len, gen_capacity);
}

extern "C" int eilev_t5beam_decode_step(const EilevT5Dims *d, const EilevT5Weights *w, const int64_t *tokens, int32_t *state,
                                        const int32_t *enc_mask, int64_t rows, int64_t beams, const void *self_kv_start, void *self_kv_gen,
                                        int64_t gen_capacity, const int32_t *ancestors, const void *cross_kv, int64_t enc_len, float *logits,
                                        void *workspace, size_t workspace_bytes, void *stream) {
    if (!d || !w || !tokens || !state || !enc_mask || !self_kv_start || !self_kv_gen || !ancestors || !cross_kv || !logits || !workspace)
        return EILEV_E_BADARG;
    if (!rows_ok(rows, beams) || gen_capacity <= 0 || gen_capacity > (1 << 20) || enc_len <= 0 || enc_len > (1 << 20)) return EILEV_E_BADARG;
    if (!dims_ok_t5(d) || d->d_kv != 64) return EILEV_E_UNSUPPORTED;
    if (workspace_bytes < t5_decode_step_beam_workspace_bytes(d, rows, enc_len, gen_capacity)) return EILEV_E_WORKSPACE;
    const T5BeamArgs beam{beams, self_kv_start, self_kv_gen, gen_capacity, ancestors};
    return t5_decode_step_beam(d, w, tokens, state, enc_mask, rows, beam, cross_kv, enc_len, logits, workspace, workspace_bytes, stream);
}

extern "C" int eilev_t5beam_cross_attention(const void *q, int64_t ldq, const void *kc, const void *vc, const int32_t *enc_mask, int64_t rows,
                                            int64_t beams, int64_t heads, int64_t hd, int64_t enc_len, int64_t cap, void *out, void *part,
                                            size_t part_bytes, void *stream) {
    if (!q || !kc || !vc || !out || !part) return EILEV_E_BADARG;
    if (!rows_ok(rows, beams) || heads <= 0 || heads > 1024 || hd <= 0 || hd > 1024 || enc_len <= 0 || cap < enc_len || cap > (1 << 24)) return EILEV_E_BADARG;
    return launch_attn_cross_shared((const bf16 *)q, ldq, (const bf16 *)kc, (const bf16 *)vc, enc_mask, (int)rows, (int)beams, (int)heads, (int)hd,
                                    (int)enc_len, (int)cap, (bf16 *)out, (float *)part, part_bytes, (hipStream_t)stream);
}

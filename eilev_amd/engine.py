"""Host-side driver of the HIP library: owns bf16 device weights, workspaces and the decode graph.

PyTorch is plumbing here (device memory, the current HIP stream, graph capture); every FLOP of the
path is executed by ``libeilev_hip.so`` through the C ABI of include/eilev.h.  There is no fallback:
constructing an engine without the built library or without a GPU raises.
"""
from __future__ import annotations

import ctypes as C
import gc

import torch

from . import abi, route
from .sampling import eos_list


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class PrefixContext:
    """A prefilled prefix that many rows continue (HipEngine.prefill_context): ``kv`` the OPT cache of ONE unpadded sequence with capacity
    ``P``, ``last_logits`` (1, vocab) fp32 of its last position."""

    def __init__(self, kv, P, last_logits):
        self.kv, self.P, self.last_logits = kv, int(P), last_logits


class HipEngine:
    """Runs the stages of VideoBlipForConditionalGeneration.forward/generate on gfx950 kernels."""

    def __init__(self, config, named_tensors: dict, device=None, parts=None, lm_weights: str = "bf16", vit_ln_fold: bool = True,
                 decode_stream_layout: bool = True, vit_block_order: bool = True):
        # the weight mode is checked from the arguments alone, before anything touches a device
        if lm_weights not in ("bf16", "fp8", "fp8_mfma", "int4"):
            raise ValueError("lm_weights must be 'bf16', 'fp8' (e4m3 weights, bf16 activations), 'fp8_mfma' (e4m3 weights AND per-token "
                             "e4m3 activations on the fp8 MFMA for prefill) or 'int4' (4-bit weights with group scales in the captured decode step)")
        if lm_weights == "int4":
            from .quant import int4_refusal

            why = int4_refusal(config)
            if why is None and parts is not None and "opt" not in parts:
                why = "the int4 kernels are built for the OPT language model, which this engine does not hold"
            if why is not None:
                raise NotImplementedError(f"lm_weights='int4': {why}")
        if not torch.cuda.is_available():
            raise RuntimeError("HipEngine needs an AMD GPU (torch.cuda.is_available() is False); there is no CPU fallback")
        self.lib = abi.load_hip()
        self.config = config
        self.dims = abi.dims_from_config(config)
        self.is_t5 = getattr(config.text_config, "model_type", "opt") == "t5"
        self.t5dims = abi.t5_dims_from_config(config) if self.is_t5 else None
        if parts is None:
            parts = ("vit", "qf", "t5" if self.is_t5 else "opt")
        self.device = torch.device(device) if device is not None else next(iter(named_tensors.values())).device
        if self.device.type != "cuda":
            raise RuntimeError(f"HipEngine weights must live on the GPU, got {self.device}")
        self._keep = {}
        self._ws = {}
        self.timing = None  # bench.py sets this to a list to collect phase events
        self._decode_warm = False
        self._dec_cache = None  # most recent captured decode step + the buffers it is bound to
        self._ctx_cache = None  # ... and that of greedy_decode_context (rows after a shared prefix)
        self.context_stats = None    # per greedy_decode_context call: dict(path="shared", rows=, prefix=, new=, steps=) (+ reads="shared" with the switch below)
        # opt-in: OPT beam search and the rows after a context run eilev_prefix_decode_step (include/eilev_prefix.h), whose attention reads a
        # sample's prompt keys once for all its rows, in place of eilev_opt_decode_step_beam, which reads them once per row
        self.shared_prompt_reads = False
        self.beam_stats = None       # per beam_decode call that reached the beam-form step: dict(rows=, beams=, prompt=, reads="shared" | "per_row")
        self.device_sampling = True  # generate(do_sample=True, num_beams=1): the draw runs in the captured step (sample_decode_device); False: the host loop
        self.sample_stats = None     # per sampling call: dict(path="device" | "host", steps=generated tokens per row)
        self.device_rules = True     # greedy / beam search with repetition_penalty, no_repeat_ngram_size, min_new_tokens or several EOS ids: the
        self.rules_stats = None      # rules run in the captured step (include/eilev_rules.h); per such call: dict(path="device" | "host", steps=)
        self.beam_device_loop = True     # plain beam search selects on the device (beam.py beam_search_device); False: the host loop beam_search
        self.beam_topk_kernel = True     # its per-row top-k is eilev_topk_logprob; False: torch ops
        self.beam_advance_kernel = True  # its bookkeeping of a step is eilev_beam_advance; False: torch ops
        self.beam_capture = False        # replay the fused step (both kernels) from a hipGraph; it buys nothing per token there
        self.parts = tuple(parts)
        if lm_weights in ("fp8", "fp8_mfma") and (self.is_t5 or "opt" not in self.parts):
            raise NotImplementedError("fp8 weights are built for the OPT language model")
        self.lm_weights = lm_weights
        self._load(named_tensors)
        # per call on an int4 engine: dict(step="eilev_w4_decode_step" (None: one new token, no step), rows=, route=, steps=decode steps run) where the captured int4 step ran, dict(step="twin", route=)
        # where the call ran the bf16 kernels on the twin weights (beams, context, prompt lookup, host loops)
        self.w4_stats = None
        self._w4 = None  # (library, per-layer table, the tensors it points to) of lm_weights="int4"
        if lm_weights == "int4":
            self._quantize_opt_int4()
        elif lm_weights != "bf16":
            self._quantize_opt(act_fp8=lm_weights == "fp8_mfma")
        # LayerNorm folding of the ViT blocks (profiles/HISTORY.md §3f): the folded qkv / fc1 copies (+1.1 GB at ViT-g) are built lazily by the first
        # launch large enough to use them (>= 24576 token rows); vit_ln_fold=False keeps the LayerNorm kernels for every launch
        self.vit_ln_fold = bool(vit_ln_fold)
        self.vit_block_order = bool(vit_block_order)
        self._vit_folded = False
        # Stream-layout copies of the OPT decode matrices (eilev_stream_layout_pack; + one copy of the language model's linears and of the
        # lm_head, 5.3 GB at OPT-2.7B): built lazily by the first greedy decode of 17..32 rows; decode_stream_layout=False keeps one copy
        self.decode_stream_layout = bool(decode_stream_layout)
        self._stream_keep = None
        self.tokens_per_frame = (self.dims.image_size // self.dims.patch_size) ** 2 + 1

    # ---- weights ------------------------------------------------------------------------------------
    def _load(self, named):
        d = self.dims
        bf = lambda t: t.detach().to(device=self.device, dtype=torch.bfloat16).contiguous()
        store = {}

        def pack(keys):
            """Concatenate tensors along dim 0 into one buffer; return per-key views (contiguous in memory)."""
            parts = [bf(named[k]) for k in keys]
            flat = torch.cat([p.reshape(-1) for p in parts])
            off = 0
            for k, p in zip(keys, parts):
                store[k] = flat[off: off + p.numel()].view(p.shape)
                off += p.numel()

        def part_of(key):
            if key.startswith("vision_model."):
                return "vit"
            if key.startswith(("qformer.", "language_projection.")) or key == "query_tokens":
                return "qf"
            return "t5" if self.is_t5 else "opt"

        if self.is_t5 and "t5" in self.parts:
            t5 = self.t5dims
            for stack, n in (("encoder", t5.enc_layers), ("decoder", t5.dec_layers)):
                for i in range(n):
                    k = abi.t5_layer_keys(stack, i)
                    pack([k["q_w"], k["k_w"], k["v_w"]])       # one q|k|v GEMM
                    pack([k["wi0_w"], k["wi1_w"]])             # one gate|up GEMM
                    if stack == "decoder":
                        pack([k["ck_w"], k["cv_w"]])           # one cross k|v GEMM per layer

        for i in range(d.t_layers if "opt" in self.parts else 0):
            p = abi.OPT_PREFIX.format(i) + "self_attn."
            pack([p + "q_proj.weight", p + "k_proj.weight", p + "v_proj.weight"])
            pack([p + "q_proj.bias", p + "k_proj.bias", p + "v_proj.bias"])
        for i in range(d.q_layers if "qf" in self.parts else 0):
            p = abi.QF_PREFIX.format(i)
            pack([p + f"attention.attention.{n}.weight" for n in ("query", "key", "value")])
            pack([p + f"attention.attention.{n}.bias" for n in ("query", "key", "value")])
            if i % d.q_cross_freq == 0:
                pack([p + f"crossattention.attention.{n}.weight" for n in ("key", "value")])
                pack([p + f"crossattention.attention.{n}.bias" for n in ("key", "value")])

        def addr(key):
            if part_of(key) not in self.parts:
                return None
            if key not in store:
                store[key] = bf(named[key])
            return store[key].data_ptr()

        def addr_t5(key):
            if key == "language_model.lm_head.weight" and key not in named:
                raise KeyError(key)  # tied to `shared`
            return addr(key)

        t5d = self.t5dims if (self.is_t5 and "t5" in self.parts) else None
        self.pack = abi.WeightPack(d, addr_t5 if t5d is not None else addr, t5d)
        self._keep = store

    def _quantize_opt(self, act_fp8: bool = False):
        """fp8 (e4m3) weights for the OPT linears (BASELINE configs[4]): per output channel absmax / 448 scales
        (eilev_amd/quant.py); q|k|v as one [3 D, D] matrix.  Embeddings / lm_head, LayerNorms and biases stay bf16."""
        from .quant import quantize_e4m3_per_channel

        d = self.dims
        per_layer, keep = [], []
        for i in range(d.t_layers):
            p = abi.OPT_PREFIX.format(i)
            w = lambda k: self._keep[p + k]
            mats = {"qkv": torch.cat([w("self_attn.q_proj.weight"), w("self_attn.k_proj.weight"), w("self_attn.v_proj.weight")], 0),
                    "o": w("self_attn.out_proj.weight"), "fc1": w("fc1.weight"), "fc2": w("fc2.weight")}
            entry = {}
            for name, m in mats.items():
                q, sc = quantize_e4m3_per_channel(m)
                keep += [q, sc]
                entry[name] = (q.data_ptr(), sc.data_ptr())
            per_layer.append(entry)
        nb = max(d.t_ffn, 3 * d.t_hidden) * d.t_hidden * 2
        expand = torch.empty(nb, dtype=torch.uint8, device=self.device)
        self._w8_keep = (keep, expand)
        abi.attach_opt_w8(self.pack, per_layer, expand.data_ptr(), nb, act_fp8=act_fp8)

    def _quantize_opt_int4(self):
        """int4 weights with group scales for the OPT linears (include/eilev_w4.h; eilev_amd/quant.py): q|k|v (one [3 D, D] matrix), out_proj,
        fc1 and fc2 of every block are quantised and packed, and eilev_w4_expand writes the matrix the int4 kernels multiply by — the bf16
        TWIN — into the storage the bf16 weights occupy: every bf16 route of this engine (prefill, beams, context, prompt lookup, host loops,
        classify, debug outputs) computes with the same model as the captured int4 decode step.  The int4 copies are a quarter as much memory
        again.  Embeddings / lm_head, LayerNorms and biases stay bf16."""
        from .quant import pack_int4, quantize_int4

        d = self.dims
        w4 = abi.load_w4()
        if not abi.w4_supported(d):
            raise NotImplementedError("lm_weights='int4': the int4 kernels take OPT widths that are multiples of 256")
        table, keep = (abi.W4Layer * d.t_layers)(), []
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        for i in range(d.t_layers):
            p = abi.OPT_PREFIX.format(i)
            q_w = self._keep[p + "self_attn.q_proj.weight"]
            mats = {"qkv": torch.as_strided(q_w, (3 * d.t_hidden, d.t_hidden), (d.t_hidden, 1)),  # q | k | v are one buffer (_load packs them so)
                    "o": self._keep[p + "self_attn.out_proj.weight"], "fc1": self._keep[p + "fc1.weight"], "fc2": self._keep[p + "fc2.weight"]}
            for name, m in mats.items():
                q, sc = quantize_int4(m)
                packed = pack_int4(q)
                keep += [packed, sc]
                setattr(table[i], name, abi.W4Matrix(packed.data_ptr(), sc.data_ptr()))
                abi.check(w4.eilev_w4_expand(_ptr(packed), _ptr(sc), m.shape[0], m.shape[1], _ptr(m), st), "eilev_w4_expand")
        self._w4 = (w4, table, keep)

    def _w4_twin(self, route_name):
        """An int4 engine records that a call ran the bf16 kernels on the twin weights."""
        if getattr(self, "lm_weights", "bf16") == "int4":
            self.w4_stats = dict(step="twin", route=route_name)

    def ensure_stream_layout(self, rows: int) -> bool:
        """Decode steps of 17..32 rows stream every OPT matrix once per token through gemm_rows32_kernel; in the checkpoint layout each of its
        load instructions reads 16 segments of 64 bytes a weight row apart.  Pack second copies in the kernel's fragment order (same values,
        same arithmetic: bit-identical logits; measured 4.35 -> 4.01 ms / token at batch 32).  Returns True if the copies are attached."""
        if self._stream_keep is not None:
            return bool(self._stream_keep)
        if (not self.decode_stream_layout or self.is_t5 or "opt" not in self.parts or self.lm_weights not in ("bf16", "int4") or not 16 < rows <= 32):
            return False
        head_only = self.lm_weights == "int4"  # the int4 step streams the block linears as nibbles: only its bf16 lm_head has a stream copy
        d = self.dims
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        keep, per_layer = [], []

        def packed(w):
            n, k = w.shape
            out = torch.empty_like(w)
            rc = self.lib.eilev_stream_layout_pack(_ptr(w), n, k, _ptr(out), st)
            if rc == -2:  # EILEV_E_UNSUPPORTED: the decode kernel does not take this shape — it keeps reading the checkpoint layout
                return None
            abi.check(rc, "eilev_stream_layout_pack")
            keep.append(out)
            return out.data_ptr()

        for i in range(d.t_layers):
            if head_only:
                per_layer.append({})
                continue
            p = abi.OPT_PREFIX.format(i)
            q = self._keep[p + "self_attn.q_proj.weight"]
            qkv = torch.as_strided(q, (3 * d.t_hidden, d.t_hidden), (d.t_hidden, 1))  # q | k | v are one buffer (_load packs them so)
            per_layer.append({"qkv": packed(qkv), "o": packed(self._keep[p + "self_attn.out_proj.weight"]),
                              "fc1": packed(self._keep[p + "fc1.weight"]), "fc2": packed(self._keep[p + "fc2.weight"])})
        head = packed(self._keep["language_model.model.decoder.embed_tokens.weight"])
        abi.attach_opt_stream(self.pack, per_layer, head)
        self._stream_keep = keep
        self._dec_cache = self._ctx_cache = None  # a captured decode step holds the old pointers
        return bool(keep)

    def ensure_vit_fold(self):
        """Build the folded qkv / fc1 copies now (normally done by the first launch of >= 24576 token rows); no-op when folding is off."""
        if self.vit_ln_fold and not self._vit_folded:
            self._fold_vit_layernorms()

    def _fold_vit_layernorms(self):
        """layer_norm1 / layer_norm2 of every ViT block folded into qkv / fc1 (`eilev_fold_layernorm`, include/eilev.h ABI 9): large
        encode launches then run without LayerNorm kernels.  +1.1 GB of device memory at ViT-g (a second copy of qkv / fc1)."""
        d = self.dims
        self._vit_folded = True
        if d.v_hidden % 64 or d.v_inter % 64:
            return
        st = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        per_layer, keep = [], []
        for i in range(d.v_layers):
            k = abi.vit_layer_keys(i)
            entry = {}
            for name, ln in (("qkv", "ln1"), ("fc1", "ln2")):
                w, b = self._keep[k[f"{name}_w"]], self._keep[k[f"{name}_b"]]
                wf, bf = torch.empty_like(w), torch.empty_like(b)
                cs = torch.empty(w.shape[0], dtype=torch.float32, device=self.device)
                abi.check(self.lib.eilev_fold_layernorm(w.data_ptr(), self._keep[k[f"{ln}_w"]].data_ptr(), self._keep[k[f"{ln}_b"]].data_ptr(),
                                                        b.data_ptr(), w.shape[0], w.shape[1], wf.data_ptr(), cs.data_ptr(), bf.data_ptr(), st),
                          "eilev_fold_layernorm")
                keep += [wf, bf, cs]
                entry[name] = (wf.data_ptr(), bf.data_ptr(), cs.data_ptr())
            per_layer.append(entry)
        self._vit_fold_keep = keep
        abi.attach_vit_fold(self.pack, per_layer)
        self._attach_vit_block_order(per_layer)

    def _attach_vit_block_order(self, per_layer):
        """Second copy of the folded q|k|v matrices with their rows in BLOCK ORDER (include/eilev.h ABI 15; + 0.46 GB at
        ViT-g): launches of >= 512 frames write q, k, v of a (frame, head) as [token][64] + [token][24] blocks, which the frame attention
        stages as two contiguous runs (932 -> ~800 us per 1088 frames) and the GEMM stores as whole lines.  Only ViT-g's geometry (257
        tokens, head size 88) takes it; `vit_block_order=False` keeps one copy."""
        d = self.dims
        hd = d.v_hidden // d.v_heads
        if not self.vit_block_order or self.tokens_per_frame != 257 or hd != 88:
            return
        D, H, tok = d.v_hidden, d.v_heads, self.tokens_per_frame
        lo, hi = 64, hd - 64
        # new column order of a third: [h][0..63] for every head, then [h][64..hd-1]
        third = torch.cat([torch.arange(H).repeat_interleave(lo) * hd + torch.arange(lo).repeat(H),
                           torch.arange(H).repeat_interleave(hi) * hd + lo + torch.arange(hi).repeat(H)])
        perm = torch.cat([p * D + third for p in range(3)]).to(self.device)
        keep, per = [], []
        for i, entry in enumerate(per_layer):
            wf, bf, cs = (t for t in self._vit_fold_keep[6 * i: 6 * i + 3])  # the folded q|k|v of block i (w, b, csum)
            wp, bp, cp = wf.index_select(0, perm).contiguous(), bf.index_select(0, perm).contiguous(), cs.index_select(0, perm).contiguous()
            keep += [wp, bp, cp]
            per.append((wp.data_ptr(), bp.data_ptr(), cp.data_ptr()))
        self._vit_hm_keep = keep
        abi.attach_vit_fold_hm(self.pack, per)

    # ---- workspaces ----------------------------------------------------------------------------------
    def _workspace(self, tag, nbytes):
        cur = self._ws.get(tag)
        if cur is None or cur.numel() < nbytes:
            self._ws[tag] = cur = torch.empty(int(nbytes), dtype=torch.uint8, device=self.device)
        return cur

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    # ---- stages --------------------------------------------------------------------------------------
    def vit(self, pixel_values: torch.Tensor, want_pooler: bool = False, max_frames_per_call: int = 1088):
        """(N, 3, T, H, W) fp32/bf16 -> (N, T*tokens, Dv) bf16 [ref:eilev/model/v2.py:24-103]."""
        if pixel_values is None:
            raise ValueError("You have to specify pixel_values")
        d = self.dims
        px = pixel_values.to(self.device)
        if px.dtype not in (torch.float32, torch.bfloat16):
            px = px.float()
        px = px.contiguous()
        N, ch, T, Hh, Ww = px.shape
        if ch != 3 or Hh != d.image_size or Ww != d.image_size:
            raise ValueError(f"pixel_values must be (N, 3, T, {d.image_size}, {d.image_size}), got {tuple(px.shape)}")
        out = torch.empty((N, T * self.tokens_per_frame, d.v_hidden), dtype=torch.bfloat16, device=self.device)
        pool = torch.empty((N, T, d.v_hidden), dtype=torch.bfloat16, device=self.device) if want_pooler else None
        step = max(1, max_frames_per_call // T)
        if min(N, step) * T * self.tokens_per_frame >= 24576:
            self.ensure_vit_fold()
        dt = abi_dtype(px)
        for n0 in range(0, N, step):
            n1 = min(N, n0 + step)
            nb = self.lib.eilev_vit_workspace_bytes(C.byref(d), n1 - n0, T)
            ws = self._workspace("vit", nb)
            abi.check(self.lib.eilev_vit_forward(C.byref(d), C.byref(self.pack.vit), _ptr(px[n0:n1]), dt, n1 - n0, T,
                                                 _ptr(out[n0:n1]), _ptr(pool[n0:n1]) if want_pooler else None,
                                                 _ptr(ws), ws.numel(), self._stream()), "eilev_vit_forward")
        return (out, pool) if want_pooler else out

    def vit_debug(self, pixel_values: torch.Tensor, want_hidden: bool = True, want_attn: bool = True):
        """Slow path of the vision wrapper's debug outputs [ref:eilev/model/v2.py:76-103]: returns (last_hidden_state (N, T*tok, Dv),
        pooler (N, T, Dv), hidden_states (layers + 1, N, T*tok, Dv) or None, attentions (layers, N, T, heads, tok, tok) or None)."""
        d = self.dims
        px = pixel_values.to(self.device)
        if px.dtype not in (torch.float32, torch.bfloat16):
            px = px.float()
        px = px.contiguous()
        N, ch, T, Hh, Ww = px.shape
        if ch != 3 or Hh != d.image_size or Ww != d.image_size:
            raise ValueError(f"pixel_values must be (N, 3, T, {d.image_size}, {d.image_size}), got {tuple(px.shape)}")
        tok = self.tokens_per_frame
        bf = dict(dtype=torch.bfloat16, device=self.device)
        out = torch.empty((N, T * tok, d.v_hidden), **bf)
        pool = torch.empty((N, T, d.v_hidden), **bf)
        hid = torch.empty((d.v_layers + 1, N, T * tok, d.v_hidden), **bf) if want_hidden else None
        att = torch.empty((d.v_layers, N, T, d.v_heads, tok, tok), **bf) if want_attn else None
        nb = self.lib.eilev_vit_workspace_bytes(C.byref(d), N, T)
        ws = self._workspace("vit", nb)
        abi.check(self.lib.eilev_vit_forward_debug(C.byref(d), C.byref(self.pack.vit), _ptr(px), abi_dtype(px), N, T, _ptr(out), _ptr(pool),
                                                   _ptr(hid), _ptr(att), _ptr(ws), ws.numel(), self._stream()), "eilev_vit_forward_debug")
        return out, pool, hid, att

    def qformer(self, image_embeds: torch.Tensor):
        d = self.dims
        img = image_embeds.contiguous()
        assert img.dtype == torch.bfloat16
        N, kv = img.shape[:2]
        out = torch.empty((N, d.num_query, d.q_hidden), dtype=torch.bfloat16, device=self.device)
        nb = self.lib.eilev_qformer_workspace_bytes(C.byref(d), N, kv)
        ws = self._workspace("qf", nb)
        abi.check(self.lib.eilev_qformer_forward(C.byref(d), C.byref(self.pack.qf), _ptr(img), N, kv, _ptr(out), _ptr(ws),
                                                 ws.numel(), self._stream()), "eilev_qformer_forward")
        return out

    # ---- attention WEIGHTS of the Q-Former and the language model (slow path: `output_attentions=True` inside the full forward) ------------
    def _lin(self, x2d, wname, bname=None, resid=None):
        w = self._keep[wname]
        b = self._keep[bname] if bname else None
        m, k = x2d.shape
        n = w.shape[0]
        out = torch.empty((m, n), dtype=torch.bfloat16, device=self.device)
        abi.check(self.lib.eilev_linear(_ptr(x2d.contiguous()), _ptr(w), _ptr(b), _ptr(resid), _ptr(out), m, n, k, 0, 0, self._stream()), "eilev_linear")
        return out

    def _ln(self, x2d, wname, bname, eps):
        out = torch.empty_like(x2d)
        abi.check(self.lib.eilev_layernorm(_ptr(x2d.contiguous()), _ptr(self._keep[wname]), _ptr(self._keep[bname]), _ptr(out), x2d.shape[0], x2d.shape[1],
                                           C.c_float(eps), self._stream()), "eilev_layernorm")
        return out

    def _probs(self, q, k, B, H, sq, skv, hd, scale, causal=False, key_mask=None, rel=None):
        """rel = (table (heads, n) f32, offset): the additive relative position bias of eilev_attention_rel (T5)."""
        out = torch.empty((B, H, sq, skv), dtype=torch.bfloat16, device=self.device)
        km = None if key_mask is None else key_mask.to(self.device, torch.int32).contiguous()
        tab, off = rel if rel is not None else (None, 0)
        abi.check(self.lib.eilev_attention_probs(_ptr(q), _ptr(k), _ptr(out), B, H, sq, skv, hd, q.shape[-1], k.shape[-1], C.c_float(scale), int(causal),
                                                 _ptr(km), _ptr(tab), 0 if tab is None else tab.shape[1], off, 0 if tab is None else tab.shape[1],
                                                 self._stream()), "eilev_attention_probs")
        return out

    def t5_rel_table(self, stack: str, L: int):
        """f32 (heads, 2 L - 1) relative position bias over key - query in [-(L-1), L-1] and the offset L - 1 (hf T5Attention.compute_bias /
        _relative_position_bucket, modeling_t5.py: the same torch ops in the same order, on the stack's relative_attention_bias weight)."""
        import math

        d = self.t5dims
        w = self._keep[f"language_model.{stack}.block.0.layer.0.SelfAttention.relative_attention_bias.weight"]  # (buckets, heads)
        rp = torch.arange(-(L - 1), L, device=w.device)  # memory position - context position
        nb = d.rel_buckets
        ret = torch.zeros_like(rp)
        if stack == "encoder":  # bidirectional
            nb //= 2
            ret = ret + (rp > 0).to(torch.long) * nb
            rp = rp.abs()
        else:
            rp = -torch.min(rp, torch.zeros_like(rp))
        max_exact = nb // 2
        large = max_exact + (torch.log(rp.float() / max_exact) / math.log(d.rel_max_dist / max_exact) * (nb - max_exact)).to(torch.long)
        large = torch.min(large, torch.full_like(large, nb - 1))
        bucket = ret + torch.where(rp < max_exact, rp, large)
        return w.float()[bucket].t().contiguous(), L - 1

    def _rms(self, x2d, wname, eps):
        out = torch.empty_like(x2d)
        abi.check(self.lib.eilev_rmsnorm(_ptr(x2d.contiguous()), _ptr(self._keep[wname]), _ptr(out), x2d.shape[0], x2d.shape[1], C.c_float(eps), self._stream()),
                  "eilev_rmsnorm")
        return out

    def t5_attentions(self, enc_hs, dec_hs, attention_mask, decoder_attention_mask=None):
        """`output_attentions` of the T5 stacks [ref:eilev/model/v2.py:228-238 -> hf T5Attention: softmax(q . k + position_bias + mask), no
        scaling]: (encoder self (layers, B, H, L, L), decoder self (layers, B, H, T, T), cross (layers, B, H, T, L)) bf16.  enc_hs / dec_hs = the
        tuples of t5_forward_debug (block inputs, final norm last); q / k are recomputed from them with the C-ABI calls the stacks are built from
        (the decoder's cross-attention queries need the block's self-attention output: attention, o + residual, layer norm)."""
        from .abi import t5_layer_keys

        d = self.t5dims
        H, hd = d.heads, d.d_kv
        I = H * hd
        B, L, D = enc_hs.shape[1:]
        T = dec_hs.shape[2]
        am = attention_mask.to(self.device, torch.int32).contiguous()
        dm = None if decoder_attention_mask is None else (decoder_attention_mask.to(self.device) != 0).to(torch.int32).contiguous()
        enc_rel, dec_rel = self.t5_rel_table("encoder", L), self.t5_rel_table("decoder", T)
        enc_a, dec_a, cross_a = [], [], []
        for l in range(d.enc_layers):
            k_ = t5_layer_keys("encoder", l)
            x = self._rms(enc_hs[l].reshape(B * L, D), k_["ln_sa"], d.eps)
            enc_a.append(self._probs(self._lin(x, k_["q_w"]), self._lin(x, k_["k_w"]), B, H, L, L, hd, 1.0, key_mask=am, rel=enc_rel))
        enc_out = enc_hs[-1].reshape(B * L, D).contiguous()
        for l in range(d.dec_layers):
            k_ = t5_layer_keys("decoder", l)
            h = dec_hs[l].reshape(B * T, D).contiguous()
            x = self._rms(h, k_["ln_sa"], d.eps)
            q, k, v = self._lin(x, k_["q_w"]), self._lin(x, k_["k_w"]), self._lin(x, k_["v_w"])
            dec_a.append(self._probs(q, k, B, H, T, T, hd, 1.0, causal=True, key_mask=dm, rel=dec_rel))
            ctx = torch.empty_like(q)
            abi.check(self.lib.eilev_attention_rel(_ptr(q), _ptr(k), _ptr(v), _ptr(ctx), B, H, T, T, hd, I, I, I, C.c_float(1.0), 1, _ptr(dm), _ptr(dec_rel[0]),
                                                   dec_rel[0].shape[1], dec_rel[1], dec_rel[0].shape[1], self._stream()), "eilev_attention_rel")
            x2 = self._rms(self._lin(ctx, k_["o_w"], resid=h), k_["ln_ca"], d.eps)
            cross_a.append(self._probs(self._lin(x2, k_["cq_w"]), self._lin(enc_out, k_["ck_w"]), B, H, T, L, hd, 1.0, key_mask=am))
        return torch.stack(enc_a), torch.stack(dec_a), torch.stack(cross_a)

    def lm_attentions(self, hidden_states: torch.Tensor, attention_mask: torch.Tensor):
        """`output_attentions` of the OPT language model [ref:eilev/model/v2.py:220-227 -> hf modeling_opt.py eager_attention_forward]:
        per block softmax(causal + padding mask over scale * q . k), (t_layers, B, heads, L, L) bf16.  hidden_states = the tuple of
        `prefill(..., hidden_states=True)` (every block's input); q and k are recomputed from it (LayerNorm + the two projections)."""
        d = self.dims
        Lyr, B, L, D = hidden_states.shape[0] - 1, *hidden_states.shape[1:]
        H, hd = d.t_heads, d.t_hidden // d.t_heads
        out = []
        for l in range(Lyr):
            p = abi.OPT_PREFIX.format(l)
            x = self._ln(hidden_states[l].reshape(B * L, D), p + "self_attn_layer_norm.weight", p + "self_attn_layer_norm.bias", d.t_eps)
            q = self._lin(x, p + "self_attn.q_proj.weight", p + "self_attn.q_proj.bias")
            k = self._lin(x, p + "self_attn.k_proj.weight", p + "self_attn.k_proj.bias")
            out.append(self._probs(q, k, B, H, L, L, hd, hd ** -0.5, causal=True, key_mask=attention_mask))
        return torch.stack(out)

    def qformer_attentions(self, image_embeds: torch.Tensor, hidden_states):
        """`output_attentions` of the Q-Former [ref:eilev/model/v2.py:187-193 -> hf Blip2QFormerLayer]: (self-attention weights of every block
        (q_layers, N, heads, nq, nq), cross-attention weights of the blocks that have one (list of (N, heads, nq, kv))).  hidden_states = the
        tuple of `qformer_hidden_states` (block inputs); the cross-attention's queries come from the block's self-attention output, which is
        recomputed here (attention, output dense + residual, LayerNorm) with the same C-ABI calls the stage itself is built from."""
        d = self.dims
        img = image_embeds.contiguous()
        N, kv, Dv = img.shape
        nq, Dq, H = d.num_query, d.q_hidden, d.q_heads
        hd = Dq // H
        selfs, crosses = [], []
        for i in range(d.q_layers):
            p = f"qformer.encoder.layer.{i}."
            h = hidden_states[i].reshape(N * nq, Dq).contiguous()
            q = self._lin(h, p + "attention.attention.query.weight", p + "attention.attention.query.bias")
            k = self._lin(h, p + "attention.attention.key.weight", p + "attention.attention.key.bias")
            selfs.append(self._probs(q, k, N, H, nq, nq, hd, hd ** -0.5))
            if i % d.q_cross_freq == 0:
                v = self._lin(h, p + "attention.attention.value.weight", p + "attention.attention.value.bias")
                ctx = torch.empty_like(q)
                abi.check(self.lib.eilev_attention(_ptr(q), _ptr(k), _ptr(v), _ptr(ctx), N, H, nq, nq, hd, Dq, Dq, Dq, C.c_float(hd ** -0.5), 0, None,
                                                   self._stream()), "eilev_attention")
                ao = self._ln(self._lin(ctx, p + "attention.output.dense.weight", p + "attention.output.dense.bias", resid=h),
                              p + "attention.output.LayerNorm.weight", p + "attention.output.LayerNorm.bias", d.q_eps)
                qc = self._lin(ao, p + "crossattention.attention.query.weight", p + "crossattention.attention.query.bias")
                kc = self._lin(img.reshape(N * kv, Dv), p + "crossattention.attention.key.weight", p + "crossattention.attention.key.bias")
                crosses.append(self._probs(qc, kc, N, H, nq, kv, hd, hd ** -0.5))
        return torch.stack(selfs), crosses

    def qformer_hidden_states(self, image_embeds: torch.Tensor):
        """Debug outputs of the Q-Former [ref:eilev/model/v2.py:187-193 `output_hidden_states`]: the tuple hf returns — the embedding output
        (LayerNorm of the query tokens) and every block's output, each (N, num_query, Dq) bf16.  Slow path: the stack is run with its first
        i blocks for i = 1 .. L (the C ABI has no per-block export; 78 block executions instead of 12 at L = 12)."""
        d = self.dims
        img = image_embeds.contiguous()
        N, kv = img.shape[:2]
        qt = self._keep["query_tokens"].reshape(d.num_query, d.q_hidden).contiguous()
        emb = torch.empty_like(qt)
        abi.check(self.lib.eilev_layernorm(_ptr(qt), _ptr(self._keep["qformer.layernorm.weight"]), _ptr(self._keep["qformer.layernorm.bias"]), _ptr(emb),
                                           d.num_query, d.q_hidden, C.c_float(d.q_eps), self._stream()), "eilev_layernorm")
        outs = [emb.unsqueeze(0).expand(N, -1, -1).contiguous()]
        nb = self.lib.eilev_qformer_workspace_bytes(C.byref(d), N, kv)
        ws = self._workspace("qf", nb)
        for i in range(1, d.q_layers + 1):
            di = type(d).from_buffer_copy(d)
            di.q_layers = i
            out = torch.empty((N, d.num_query, d.q_hidden), dtype=torch.bfloat16, device=self.device)
            abi.check(self.lib.eilev_qformer_forward(C.byref(di), C.byref(self.pack.qf), _ptr(img), N, kv, _ptr(out), _ptr(ws), ws.numel(), self._stream()),
                      "eilev_qformer_forward")
            outs.append(out)
        return tuple(outs)

    def project(self, query_out: torch.Tensor, out: torch.Tensor = None):
        d = self.dims
        q = query_out.reshape(-1, d.q_hidden).contiguous()
        if out is None:
            out = torch.empty((q.shape[0], d.t_hidden), dtype=torch.bfloat16, device=self.device)
        elif out.shape != (q.shape[0], d.t_hidden) or out.dtype != torch.bfloat16 or not out.is_contiguous():
            raise ValueError("project(out=...): need a contiguous bf16 (rows, t_hidden) buffer")
        abi.check(self.lib.eilev_project_rows(C.byref(d), self.pack.proj_w, self.pack.proj_b, _ptr(q), q.shape[0], _ptr(out),
                                              self._stream()), "eilev_project_rows")
        return out

    def encode_clips(self, pixel_values, out: torch.Tensor = None):
        """pixels -> projected query tokens (N*num_query, Dt): ViT + Q-Former + language_projection."""
        return self.project(self.qformer(self.vit(pixel_values)), out=out)

    def encode_and_exchange(self, pixel_values, exchange):
        """Sharded encode: this rank's dealt clips go through ViT + Q-Former + projection in chunks of the exchange plan; every
        chunk is handed to `exchange` (eilev_amd.comm.ClipExchange) as soon as it is projected, so its transfer (RCCL on a side
        stream) runs under the next chunk's ViT.  Returns the projected rows of the clips whose samples THIS rank's language
        model runs, in global clip order.  At world == 1 the chunks are written straight into the result (no copy)."""
        plan = exchange.plan
        if pixel_values.shape[0] != plan.n_local:
            raise ValueError(f"rank {plan.rank} was dealt {plan.n_local} clips, got {pixel_values.shape[0]}")
        for j in range(plan.rounds):
            a, b = plan.chunk_range(j)
            buf = exchange.chunk_buffer(j)
            if b > a:
                self.encode_clips(pixel_values[a:b], out=buf)
            exchange.send_round(j, buf)
        return exchange.finish()

    def embed_scatter(self, input_ids, video_mask, video_feats, validated: bool = False):
        """Token embeddings with the video feature rows scattered over the masked positions [ref:eilev/model/v2.py:308-316].
        The two contract checks of the reference's path — `nn.Embedding`'s id range and boolean `index_put`'s count — read values back
        from the device (a host sync each) and run on EVERY call.  ``validated=True`` is the caller's statement that this exact
        (ids, mask, row count) submission already passed them (bench.py's timed loop re-submits one checked batch); nothing is
        inferred from tensor addresses: the caching allocator hands the next batch the same storage."""
        d = self.dims
        ids = input_ids.to(self.device, torch.int64).contiguous()
        B, L = ids.shape
        vm = None
        n_rows = 0
        if video_mask is not None and video_feats is not None:
            vm = (video_mask.to(self.device) != 0).to(torch.uint8).contiguous()
            n_rows = int(video_feats.shape[0])
            if not validated:
                n_set = int(vm.sum().item())
                if n_set != n_rows:  # same contract as torch's boolean index_put (ref:eilev/model/v2.py:316)
                    raise RuntimeError(f"shape mismatch: video_input_mask selects {n_set} positions but there are {n_rows} video feature rows")
            video_feats = video_feats.contiguous()
        if not validated and ids.numel():
            lo, hi = torch.aminmax(ids)
            if int(lo) < 0 or int(hi) >= d.vocab:
                raise IndexError("input_ids out of range")
        out = torch.empty((B, L, d.t_hidden), dtype=torch.bfloat16, device=self.device)
        abi.check(self.lib.eilev_embed_scatter(C.byref(d), self.pack.embed_tokens, _ptr(ids), _ptr(vm),
                                               _ptr(video_feats) if vm is not None else None, n_rows, B, L, _ptr(out),
                                               self._stream()), "eilev_embed_scatter")
        return out

    def ce_rows(self, logits32: torch.Tensor, targets: torch.Tensor):
        """Per-row cross entropy of fp32 logits (rows, vocab) against int64 targets; rows with target < 0 (ignore_index -100) give 0
        [hf loss_utils.ForCausalLMLoss / F.cross_entropy(reduction='none')] — `eilev_ce_loss` without the gradient output."""
        lg = logits32.contiguous()
        if lg.dtype != torch.float32:
            raise ValueError("ce_rows needs fp32 logits")
        tg = targets.to(self.device, torch.int64).contiguous()
        rows, vocab = lg.shape
        out = torch.empty(rows, dtype=torch.float32, device=self.device)
        if rows:
            abi.check(self.lib.eilev_ce_loss(_ptr(lg), _ptr(tg), 1.0, _ptr(out), None, rows, vocab, self._stream()), "eilev_ce_loss")
        return out

    def ce_mean(self, logits32: torch.Tensor, targets: torch.Tensor):
        """Mean over the rows with a valid target (NaN when there is none, as F.cross_entropy gives)."""
        tg = targets.to(self.device, torch.int64).reshape(-1)
        rows = self.ce_rows(logits32.reshape(-1, logits32.shape[-1]), tg)
        return rows.sum() / (tg >= 0).sum().to(torch.float32)

    def new_kv_cache(self, batch, capacity):
        nb = self.lib.eilev_opt_kv_cache_bytes(C.byref(self.dims), batch, capacity)
        # not zeroed (10 GB at batch 32): every slot is written (kv_write) before any kernel reads it
        return torch.empty(int(nb), dtype=torch.uint8, device=self.device)

    def _kv8(self, kv_dtype):
        """The fp8 KV-cache library for kv_dtype "fp8", None for "bf16" / None; no fall-back: a model it does not take is an error."""
        if kv_dtype in (None, "bf16"):
            return None
        if kv_dtype != "fp8":
            raise ValueError(f"kv_dtype must be 'bf16' or 'fp8', not {kv_dtype!r}")
        if getattr(self, "lm_weights", "bf16") == "int4":
            raise NotImplementedError("kv_cache_dtype='fp8' together with lm_weights='int4' is not built: the int4 decode step reads a bf16 KV cache")
        if not abi.kv8_supported(self.dims):
            raise NotImplementedError("kv_dtype='fp8': the fp8 KV-cache kernels take OPT head sizes 80 and 128")
        return abi.load_kv8()

    def new_kv8_cache(self, batch, capacity):
        """An fp8 (e4m3) KV cache with its exponent planes (include/eilev_kv8.h); not zeroed, like new_kv_cache."""
        nb = abi.load_kv8().eilev_kv8_cache_bytes(C.byref(self.dims), batch, capacity)
        if not nb:
            raise RuntimeError("eilev_kv8_cache_bytes refused the shape")
        return torch.empty(int(nb), dtype=torch.uint8, device=self.device)

    def prefill(self, inputs_embeds, attention_mask, kv_cache=None, kv_capacity=None, all_logits=False, last_logits=True, hidden_states=False):
        """OPT prefill.  ``hidden_states=True`` appends the tuple hf returns under ``output_hidden_states`` (every block's input, then the
        output of final_layer_norm; `eilev_opt_prefill_debug`) as a fourth result, (t_layers + 1, B, L, Dt) bf16."""
        d = self.dims
        x = inputs_embeds.contiguous()
        B, L, _ = x.shape
        cap = int(kv_capacity or L)
        am = attention_mask.to(self.device, torch.int32).contiguous()
        if kv_cache is None:
            kv_cache = self.new_kv_cache(B, cap)
        last = torch.empty((B, d.vocab), dtype=torch.float32, device=self.device) if last_logits else None
        alll = torch.empty((B, L, d.vocab), dtype=torch.float32, device=self.device) if all_logits else None
        nb = self.lib.eilev_opt_workspace_bytes(C.byref(d), B, L)
        ws = self._workspace("opt", nb)
        if hidden_states:
            hs = torch.empty((d.t_layers + 1, B, L, d.t_hidden), dtype=torch.bfloat16, device=self.device)
            abi.check(self.lib.eilev_opt_prefill_debug(C.byref(d), C.byref(self.pack.opt), _ptr(x), _ptr(am), B, L, _ptr(kv_cache), cap,
                                                       _ptr(last), _ptr(alll), _ptr(hs), _ptr(ws), ws.numel(), self._stream()), "eilev_opt_prefill_debug")
            return last, alll, kv_cache, hs
        abi.check(self.lib.eilev_opt_prefill(C.byref(d), C.byref(self.pack.opt), _ptr(x), _ptr(am), B, L, _ptr(kv_cache), cap,
                                             _ptr(last), _ptr(alll), _ptr(ws), ws.numel(), self._stream()), "eilev_opt_prefill")
        return last, alll, kv_cache

    def extend(self, new_embeds, full_mask, past_len, kv_cache, kv_capacity):
        """Run ``new_embeds`` (B, Ln, Dt) as positions past_len.. of sequences whose first ``past_len`` KV entries are in
        ``kv_cache``; returns fp32 logits (B, Ln, vocab) [second LM call of classify(), ref:eilev/model/v2.py:461-466]."""
        d = self.dims
        x = new_embeds.contiguous()
        B, Ln, _ = x.shape
        am = full_mask.to(self.device, torch.int32).contiguous()
        assert am.shape == (B, past_len + Ln)
        out = torch.empty((B, Ln, d.vocab), dtype=torch.float32, device=self.device)
        nb = self.lib.eilev_opt_workspace_bytes(C.byref(d), B, past_len + Ln)
        ws = self._workspace("opt", nb)
        abi.check(self.lib.eilev_opt_extend(C.byref(d), C.byref(self.pack.opt), _ptr(x), _ptr(am), B, Ln, past_len, _ptr(kv_cache),
                                            int(kv_capacity), _ptr(out), _ptr(ws), ws.numel(), self._stream()), "eilev_opt_extend")
        return out

    def prefill_context(self, inputs_embeds):
        """Prefill ONE unpadded sequence (1, P, Dt) into a cache of capacity P — the layout eilev_prefix_extend and the beam form of the decode
        step read as a shared prefix.  Returns a PrefixContext: the cache, P and the last position's logits (1, vocab)."""
        x = inputs_embeds.contiguous()
        if x.dim() != 3 or x.shape[0] != 1 or x.shape[1] < 1:
            raise ValueError(f"a context is one unpadded sequence (1, P, Dt), got {tuple(x.shape)}")
        P = int(x.shape[1])
        am = torch.ones((1, P), dtype=torch.int32, device=self.device)
        last, _, kv = self.prefill(x, am, kv_capacity=P)
        return PrefixContext(kv=kv, P=P, last_logits=last)

    def extend_shared(self, ctx, new_embeds, kv_rows=None, cap=None, all_logits=False):
        """``new_embeds`` (R, n, Dt) as positions P .. P + n - 1 of R rows that all continue the prefix ``ctx`` (eilev_prefix_extend: the prefix
        cache is read once, never copied per row).  ``kv_rows``: a cache of ``new_kv_cache(R, cap)`` whose slots [0, n) receive the rows' new
        K / V (None: none are written).  Returns fp32 logits: (R, vocab) of the last new position, or (R, n, vocab) with ``all_logits``.
        Without ``kv_rows`` the rows run in parts where one call's limits (include/eilev_prefix.h) are exceeded."""
        d = self.dims
        px = abi.load_prefix()
        x = new_embeds.contiguous()
        R, n, _ = x.shape
        if n > abi.PREFIX_MAX_NEW:
            raise ValueError(f"at most {abi.PREFIX_MAX_NEW} new positions per row after a shared prefix, got {n}")
        per = min(abi.PREFIX_MAX_ROWS, abi.PREFIX_MAX_STACKED // n)
        if R > per and kv_rows is not None:
            raise ValueError(f"at most {per} rows of {n} new positions per call when their K / V are kept")
        out = torch.empty((R, n, d.vocab) if all_logits else (R, d.vocab), dtype=torch.float32, device=self.device)
        for i in range(0, R, per):
            r = min(per, R - i)
            ws = self._workspace("prefix", px.eilev_prefix_workspace_bytes(C.byref(d), r, n))
            abi.check(px.eilev_prefix_extend(C.byref(d), C.byref(self.pack.opt), _ptr(x[i:]), r, n, _ptr(ctx.kv), ctx.P, _ptr(kv_rows), int(cap or 0),
                                             None if all_logits else _ptr(out[i:]), _ptr(out[i:]) if all_logits else None, _ptr(ws), ws.numel(),
                                             self._stream()), "eilev_prefix_extend")
        return out

    def greedy_decode_context(self, ctx, new_embeds, max_new_tokens, eos_id=-1, pad_id=1, use_graph=True, trace=None, poll_every=8):
        """Greedy decoding of R rows (R, n, Dt) that continue the prefix ``ctx``: extend_shared into a generation cache of capacity n +
        max_new, the first token from eilev_greedy_select on its logits, then ONE captured step per token made of two existing entries —
        eilev_opt_decode_step_beam with the R rows as R beams of one sample whose prompt cache is the prefix (identity ancestor table, its
        counter preset to n + 1: position, KV slot and the number of visible generated keys all follow from that word, so the n new positions in
        slots [0, n) are to it n tokens already generated) and eilev_greedy_select on a second counter.  The most recent graph is kept with
        its buffers and reused by a call of the same shape on the same context.  ``trace``: a list that receives the extend's logits and every
        eager step's; it turns capture off.  Returns int64 (R, steps) new tokens."""
        self._w4_twin("greedy_context")
        d = self.dims
        R, n, _ = new_embeds.shape
        if max_new_tokens <= 0:
            return torch.empty((R, 0), dtype=torch.int64, device=self.device)
        if R > 32:
            if trace is not None:
                raise ValueError("trace: at most 32 decode rows")
            stats = []

            def part(i, j):
                ids = self.greedy_decode_context(ctx, new_embeds[i:j], max_new_tokens, eos_id, pad_id, use_graph, None, poll_every)
                stats.append(self.context_stats["steps"])
                return ids

            out = self._chunked_rows(part, R, pad_id)
            self.context_stats = dict(path="shared", rows=R, prefix=ctx.P, new=n, steps=max(stats), **self._reads_record(getattr(self, "shared_prompt_reads", False)))
            return out
        eos = eos_list(eos_id)
        if len(eos) > 1:
            raise NotImplementedError("greedy_decode_context takes one EOS id")
        P, gen_cap, n_dec = ctx.P, n + max_new_tokens, max_new_tokens - 1
        if n_dec > 0:
            self.ensure_stream_layout(R)
        graphable = use_graph and n_dec > 1 and trace is None
        shared = bool(getattr(self, "shared_prompt_reads", False))
        step_fn, step_name, ws_bytes = self._beam_form_step(shared, R, P, gen_cap)
        key = (ctx.kv.data_ptr(), P, R, n, max_new_tokens, tuple(eos), int(pad_id), shared)
        ent = self._ctx_cache if (graphable and self._ctx_cache is not None and self._ctx_cache["key"] == key) else None
        if ent is None:
            ent = dict(key=key, graph=None, ctx=ctx,  # (the entry keeps the context alive: its graph holds the prefix cache's address)
                       kv_rows=self.new_kv_cache(R, gen_cap),
                       am=torch.ones((1, P), dtype=torch.int32, device=self.device),
                       n_valid=torch.full((R,), P, dtype=torch.int32, device=self.device),
                       anc=torch.arange(R, dtype=torch.int32, device=self.device).repeat(gen_cap, 1).contiguous(),
                       step_state=torch.zeros(2, dtype=torch.int32, device=self.device),  # the decode step's counter: tokens in the generation cache + 1
                       sel_state=torch.zeros(2, dtype=torch.int32, device=self.device),   # the selection's: the output column, the rows left
                       finished=torch.zeros(R, dtype=torch.uint8, device=self.device),
                       tokens=torch.zeros(R, dtype=torch.int64, device=self.device),
                       out=torch.empty((R, max_new_tokens), dtype=torch.int64, device=self.device),
                       logits=torch.empty((R, d.vocab), dtype=torch.float32, device=self.device),
                       ws=self._workspace("dec", ws_bytes))
            if graphable:
                self._ctx_cache = None
                self._ctx_cache = ent
        kv_rows, am, n_valid, anc, step_state, sel_state = ent["kv_rows"], ent["am"], ent["n_valid"], ent["anc"], ent["step_state"], ent["sel_state"]
        finished, tokens, out, logits, ws = ent["finished"], ent["tokens"], ent["out"], ent["logits"], ent["ws"]
        step_state.copy_(torch.tensor([n + 1, 0], dtype=torch.int32))
        sel_state.zero_()
        finished.zero_()
        out.fill_(int(pad_id))
        eos1 = eos[0] if eos else -1
        last = self.extend_shared(ctx, new_embeds, kv_rows=kv_rows, cap=gen_cap)
        if trace is not None:
            trace.append(last.clone())
        self._greedy_select(last, R, d.vocab, sel_state, finished, eos1, pad_id, tokens, out)

        def one_step():
            abi.check(step_fn(
                C.byref(d), C.byref(self.pack.opt), _ptr(tokens), _ptr(step_state), _ptr(am), _ptr(n_valid), R, R, P, _ptr(ctx.kv), _ptr(kv_rows),
                gen_cap, _ptr(anc), _ptr(logits), _ptr(ws), ws.numel(), self._stream()), step_name)
            self._greedy_select(logits, R, d.vocab, sel_state, finished, eos1, pad_id, tokens, out)

        graph = ent["graph"] if graphable else None
        if graphable and graph is None:  # (the warm run writes KV slot n of every row, as the first replay does)
            graph = ent["graph"] = self._capture_step(one_step, (step_state, sel_state, finished, tokens, out), warm=True)
        done = self._run_steps(n_dec, one_step, graph, sel_state, eos, poll_every, trace, logits)
        self.context_stats = dict(path="shared", rows=R, prefix=P, new=n, steps=1 + done, **self._reads_record(shared))
        return self._trim_at_eos(out, 1 + done, eos)

    def _beam_form_step(self, shared, rows, seq_len, gen_cap):
        """(entry, its name, workspace bytes) of the beam form of the OPT decode step: eilev_opt_decode_step_beam, or with ``shared`` its drop-in
        eilev_prefix_decode_step (include/eilev_prefix.h) — no fallback: a model that step does not take is an error."""
        d = self.dims
        if not shared:
            return self.lib.eilev_opt_decode_step_beam, "eilev_opt_decode_step_beam", self.lib.eilev_opt_workspace_bytes(C.byref(d), rows, 1)
        if not abi.prefix_supported(d):
            raise NotImplementedError("shared_prompt_reads: the shared-prompt decode step takes OPT head sizes 80 and 128")
        px = abi.load_prefix()
        nbytes = px.eilev_prefix_decode_workspace_bytes(C.byref(d), rows, seq_len, gen_cap)
        if nbytes == 0:
            raise ValueError(f"eilev_prefix_decode_step refuses rows={rows}, seq_len={seq_len}, gen_capacity={gen_cap}")
        return px.eilev_prefix_decode_step, "eilev_prefix_decode_step", nbytes

    @staticmethod
    def _reads_record(shared):
        """The ``reads`` entry of context_stats: present (reads="shared") only with the switch on, so the record of a plain call is what it was."""
        return dict(reads="shared") if shared else {}

    def classify_loglik(self, prompt_embeds, prompt_mask, class_input_ids, class_attention_mask=None, class_batch_size=None,
                        share_prompt_cache=False):
        """Mean log-likelihood of every class continuation after every prompt: (B, num_classes) fp32
        [ref:eilev/model/v2.py:403-501].  The prompt is prefilled once; its KV cache is replicated per class chunk — or, with
        ``share_prompt_cache``, stays ONE copy: each prompt row is stripped of its left padding, prefilled alone into a cache of its own
        length and the classes run through extend_shared, which keeps no K / V of theirs."""
        d = self.dims
        B, L, _ = prompt_embeds.shape
        cls_ids = class_input_ids.to(self.device, torch.int64)
        n_cls, Lc = cls_ids.shape
        cls_mask = torch.ones_like(cls_ids) if class_attention_mask is None else class_attention_mask.to(self.device, torch.int64)
        pm = prompt_mask.to(self.device, torch.int32).contiguous()
        step = n_cls if class_batch_size is None else int(class_batch_size)
        if share_prompt_cache:
            ctxs = []
            for b, nv in enumerate(pm.sum(dim=1).tolist()):
                if nv < 1 or not bool(pm[b, L - nv:].all()):
                    raise ValueError("share_prompt_cache takes left-padded prompts with at least one visible position")
                ctxs.append(self.prefill_context(prompt_embeds[b:b + 1, L - nv:]))
            last = torch.cat([c.last_logits for c in ctxs], dim=0)
        else:
            cap = L + Lc
            last, _, kv = self.prefill(prompt_embeds, pm, kv_capacity=cap)
        planes = 2 * d.t_layers
        cols = []
        for i in range(0, n_cls, step):
            ids, msk = cls_ids[i:i + step], cls_mask[i:i + step]
            nc = ids.shape[0]
            rows_ids = ids.unsqueeze(0).expand(B, -1, -1).reshape(B * nc, Lc)
            rows_msk = msk.unsqueeze(0).expand(B, -1, -1).reshape(B * nc, Lc)
            if share_prompt_cache:
                emb = self.embed_scatter(ids, None, None)  # the classes' embeddings are the same after every prompt
                logits = torch.cat([self.extend_shared(c, emb, all_logits=True) for c in ctxs], dim=0)
            else:
                full = torch.cat((pm.repeat_interleave(nc, dim=0), rows_msk.to(torch.int32)), dim=1)
                kv_rows = kv.view(planes, B, -1).repeat_interleave(nc, dim=1).contiguous()
                emb = self.embed_scatter(rows_ids, None, None)
                logits = self.extend(emb, full, L, kv_rows, cap)
                del kv_rows
            shift = torch.cat((last.repeat_interleave(nc, dim=0)[:, None], logits[:, :-1]), dim=1)
            labels = torch.where(rows_msk != 0, rows_ids, torch.full_like(rows_ids, -100))
            nll = self.ce_rows(shift.reshape(-1, d.vocab), labels.reshape(-1))
            cols.append(-nll.view(B, nc, Lc).sum(-1) / msk.sum(-1).unsqueeze(0).to(torch.float32))
        return torch.cat(cols, dim=1)

    def greedy_decode(self, inputs_embeds, attention_mask, max_new_tokens, eos_id=-1, pad_id=1, use_graph=True,
                      poll_every=8, return_step_logits=False, kv_dtype="bf16"):
        """Prefill + KV-cached greedy decode [ref:eilev/model/v2.py:318-322 -> hf generation/utils.py:2783-2941]: _select_decode_device
        with the decode step's own arg-max as the selection.

        Returns int64 (B, n_steps) of NEW tokens only (OPT path)."""
        B = inputs_embeds.shape[0]
        if max_new_tokens <= 0:
            return torch.empty((B, 0), dtype=torch.int64, device=self.device)
        if B > 32:
            if return_step_logits:
                raise NotImplementedError("return_step_logits with more than 32 rows")
            return self._chunked_rows(lambda i, j: self.greedy_decode(inputs_embeds[i:j], attention_mask[i:j], max_new_tokens, eos_id, pad_id, use_graph,
                                                                      poll_every, kv_dtype=kv_dtype), B, pad_id)
        trace = [] if return_step_logits else None
        ids = self._select_decode_device(inputs_embeds, attention_mask, max_new_tokens, eos_list(eos_id), pad_id, ("greedy",), None, None, use_graph,
                                         poll_every, trace, kv_dtype)
        return (ids, trace) if return_step_logits else ids

    def _pld_buffers(self, text_ids, max_new_tokens, k, vocab):
        """Device state of one prompt-lookup generation (include/eilev_pld.h): corpus (text ids, room for max_new ids), its length, the
        window [last, d1 .. dk], the decode step's state words, the output ids, the status block, the arg-max scratch, the window logits."""
        pld = abi.load_pld()
        text = text_ids.to(self.device, torch.int64).reshape(-1)
        n_text = int(text.numel())
        b = dict(corpus=torch.zeros(n_text + max_new_tokens, dtype=torch.int64, device=self.device),
                 corpus_len=torch.full((1,), n_text, dtype=torch.int32, device=self.device),
                 window=torch.zeros(k + 1, dtype=torch.int64, device=self.device),
                 state=torch.zeros(2, dtype=torch.int32, device=self.device),
                 out=torch.zeros(max_new_tokens, dtype=torch.int64, device=self.device),
                 status=torch.zeros(4, dtype=torch.int32, device=self.device),
                 scratch=torch.empty(int(pld.eilev_pld_scratch_bytes(k + 1, vocab)), dtype=torch.uint8, device=self.device),
                 logits=torch.empty((k + 1, vocab), dtype=torch.float32, device=self.device))
        b["corpus"][:n_text] = text
        return pld, b, n_text

    def _pld_commit(self, pld, params, b, logits, rows, vocab):
        abi.check(pld.eilev_pld_step(C.byref(params), _ptr(logits), rows, vocab, _ptr(b["corpus"]), _ptr(b["corpus_len"]), _ptr(b["window"]),
                                     _ptr(b["state"]), _ptr(b["out"]), _ptr(b["status"]), _ptr(b["scratch"]), b["scratch"].numel(),
                                     self._stream()), "eilev_pld_step")
        return b["status"].tolist()  # the one read-back of the step

    def _lookup_head(self, B, num_tokens, ngram, max_new_tokens):
        """What the two prompt-lookup loops begin with: batch 1, draft length and n-gram size in range, ``pld_stats`` reset -> (k, n_new)."""
        if B != 1:
            raise ValueError("assisted generate is only supported for batch_size = 1")
        k, n_new = int(num_tokens), int(max_new_tokens)
        if not 1 <= k <= abi.PLD_MAX_K or int(ngram) < 1:
            raise ValueError(f"prompt_lookup_num_tokens must be in 1..{abi.PLD_MAX_K} and max_matching_ngram_size >= 1")
        self.pld_stats = dict(verify=0, single=0, accepted=0)
        return k, n_new

    def _lookup_tail(self, status, verify, single, commit, out):
        """... and end with: eilev_amd/pld.py lookup_loop from the first status block; the committed ids (1, c), a view of ``out``."""
        from .pld import lookup_loop

        c = lookup_loop(status, verify, single, commit, self.pld_stats)
        return out[:c].reshape(1, c)

    def greedy_lookup_decode(self, inputs_embeds, attention_mask, text_ids, max_new_tokens, num_tokens=10, ngram=2, eos_id=-1, pad_id=1, trace=None):
        """Greedy decoding with prompt-lookup drafts [hf generate(prompt_lookup_num_tokens=k, max_matching_ngram_size=n), batch 1]:
        returns the ids of greedy_decode, int64 (1, n) of NEW tokens.  ``text_ids``: the row's visible text ids (no left padding, no
        video placeholder), the corpus the drafts are looked up in together with the committed ids.  ``eos_id``: an id, a list of
        ids, or < 0.  The prompt is prefilled once; each step verifies [last, d1 .. dm] with eilev_opt_extend, or runs the plain
        decode step when there is no draft; libeilev_hip_pld.so commits and drafts.  No hipGraph: the shapes change per step.
        Counters of the call: ``self.pld_stats``.  ``trace``: a list that receives a copy of the logits every commit read (tests)."""
        d = self.dims
        self._w4_twin("greedy_lookup")
        B, L, _ = inputs_embeds.shape
        k, n_new = self._lookup_head(B, num_tokens, ngram, max_new_tokens)
        if n_new <= 0:
            return torch.empty((1, 0), dtype=torch.int64, device=self.device)
        eos = eos_list(eos_id)
        cap = L + n_new + k
        pld, b, n_text = self._pld_buffers(text_ids, n_new, k, d.vocab)
        params = abi.pld_params(k, ngram, n_new, L, min(cap, d.max_pos), n_text + n_new, eos)
        am = attention_mask.to(self.device, torch.int32).reshape(1, L).contiguous()
        full = torch.ones((1, cap), dtype=torch.int32, device=self.device)  # [prompt mask, ones]: every verify window reads a prefix
        full[:, :L] = am
        n_valid = am.sum(dim=1, dtype=torch.int32)
        finished = torch.zeros(1, dtype=torch.uint8, device=self.device)
        kv = self.new_kv_cache(1, cap)
        emb = torch.empty((1, k + 1, d.t_hidden), dtype=torch.bfloat16, device=self.device)
        ws = self._workspace("pld", self.lib.eilev_opt_workspace_bytes(C.byref(d), 1, cap))
        ws1 = self._workspace("dec", self.lib.eilev_opt_workspace_bytes(C.byref(d), 1, 1))
        window, logits, state, out = b["window"], b["logits"], b["state"], b["out"]
        last, _, _ = self.prefill(inputs_embeds, am, kv_cache=kv, kv_capacity=cap)

        def verify(c, m):
            abi.check(self.lib.eilev_embed_scatter(C.byref(d), self.pack.embed_tokens, _ptr(window), None, None, 0, 1, m + 1, _ptr(emb),
                                                   self._stream()), "eilev_embed_scatter")
            abi.check(self.lib.eilev_opt_extend(C.byref(d), C.byref(self.pack.opt), _ptr(emb), _ptr(full), 1, m + 1, L + c - 1, _ptr(kv), cap,
                                                _ptr(logits), _ptr(ws), ws.numel(), self._stream()), "eilev_opt_extend")
            return logits

        def single(c):  # state[0] == c and window[0] == the last committed id: the plain greedy step, its arithmetic and its KV slot
            abi.check(self.lib.eilev_opt_decode_step(C.byref(d), C.byref(self.pack.opt), _ptr(window), _ptr(state), _ptr(am), _ptr(n_valid), 1, L,
                                                     _ptr(kv), cap, _ptr(logits), _ptr(finished), -1, int(pad_id), _ptr(out), n_new, _ptr(ws1),
                                                     ws1.numel(), self._stream()), "eilev_opt_decode_step")
            return logits

        def commit(lg, rows):
            if trace is not None:
                trace.append(lg[:rows].clone())
            return self._pld_commit(pld, params, b, lg, rows, d.vocab)

        return self._lookup_tail(commit(last, 1), verify, single, commit, out).clone()  # the first id: the prefill's last logits

    def beam_decode(self, inputs_embeds, attention_mask, max_new_tokens, num_beams, length_penalty=1.0, eos_id=-1, pad_id=1,
                    early_stopping=False, num_return_sequences=1, sampler=None, min_new_tokens=0, use_graph=True, trace=None, rules=None,
                    kv_dtype="bf16"):
        """Beam search on the HIP path [sample default: num_beams=5, length_penalty=-1; hf generation/utils.py:3208+].
        ``trace``: a list that receives (tokens fed, parent rows, fp32 logits) of every step (tests replay the hypotheses teacher-forced).
        ``rules``: dict(processors=, stopping=, prefix=) for the host loops (eilev_amd/sampling.py, beam.py): hf logits processors / stopping criteria;
        and the numbers repetition_penalty= / no_repeat_ngram_size=, which — like min_new_tokens and several EOS ids — run on the device in the
        step when the plan (eilev_amd/route.py plan_decode) says so (``self.rules_stats`` says which path ran), else as transformers' processors in the host loops.

        The prompt is prefilled ONCE per sample; no cache row is ever copied (see below); one HIP decode step on all rows per
        generated token, captured into a hipGraph and replayed.

        ``kv_dtype="fp8"`` is served by the two device routes of num_beams == 1 (sample_decode_device, rules_decode_device) only: a call that
        would take a host loop, or beams, is refused."""
        d = self.dims
        B, L, _ = inputs_embeds.shape
        R = B * num_beams
        if num_beams > 32:
            raise NotImplementedError("num_beams > 32")
        plan = route.plan_decode(route.Caps.of(self), num_beams, sampler, rules, eos_id, min_new_tokens, max_new_tokens, trace is not None, kv_dtype,
                                 in_search_loop=True)
        device = dict(sample_device=self.sample_decode_device, rules_device=self.rules_decode_device).get(plan.route)
        if device is not None:
            return device(inputs_embeds, attention_mask, max_new_tokens, eos_id=eos_id, pad_id=pad_id, use_graph=use_graph, kv_dtype=kv_dtype,
                          **plan.dev_kw)
        if self._kv8(kv_dtype) is not None:
            raise NotImplementedError("kv_cache_dtype='fp8' is built for the captured device routes only: this call takes beam search or a host loop")
        self._w4_twin(plan.route)
        if B > plan.chunk:
            # at most 32 decode rows per call: beam search of a large batch runs sample group by sample group (groups are independent in beam
            # search); every part is planned again from the caller's arguments
            if trace is not None:
                raise ValueError("trace: at most 32 decode rows")
            if plan.rules and plan.rules.get("prefix") is not None:
                raise NotImplementedError("prefix ids with more than 32 decode rows")
            return self._chunked_rows(lambda i, j: self.beam_decode(
                inputs_embeds[i:j], attention_mask[i:j], max_new_tokens, num_beams, length_penalty, eos_id, pad_id, early_stopping, num_return_sequences,
                sampler, min_new_tokens, use_graph, None, rules), B, pad_id, per=plan.chunk)
        gen_cap = max(1, max_new_tokens)
        am = attention_mask.to(self.device, torch.int32).contiguous()
        # The KV cache is never moved (round 3; before: a torch index_select of the whole cache per step, 1.6 GB at 5 beams x L = 960):
        # the prompt's keys / values stay in the prefill cache (one row per SAMPLE, capacity L), generated tokens go to a generation
        # cache (one row per beam slot, capacity max_new_tokens) and `anc[g][r]` names the slot holding token g of the hypothesis now in
        # row r — include/eilev.h eilev_opt_decode_step_beam.  A step = gather of that small table by the parents + one captured launch.
        last, _, kv_prompt = self.prefill(inputs_embeds, am, kv_capacity=L)
        kv_gen = torch.empty(int(self.lib.eilev_opt_kv_cache_bytes(C.byref(d), R, gen_cap)), dtype=torch.uint8, device=self.device)
        anc = torch.zeros((gen_cap, R), dtype=torch.int32, device=self.device)
        ident32 = torch.arange(R, dtype=torch.int32, device=self.device)
        n_valid = am.sum(dim=1).to(torch.int32).repeat_interleave(num_beams).contiguous()
        state = torch.zeros(2, dtype=torch.int32, device=self.device)
        tokens = torch.zeros(R, dtype=torch.int64, device=self.device)
        logits = torch.empty((R, d.vocab), dtype=torch.float32, device=self.device)
        shared = bool(getattr(self, "shared_prompt_reads", False))
        step_fn, step_name, nb = self._beam_form_step(shared, R, L, gen_cap)
        warm_flag = "_shared_warm" if shared else "_decode_warm"  # (each library loads its kernels lazily: one warm run each)
        ws = self._workspace("dec", nb)
        steps = [0]
        graph = [None]
        self.beam_stats = dict(rows=R, beams=num_beams, prompt=L, reads="shared" if shared else "per_row")

        def launch():
            abi.check(step_fn(
                C.byref(d), C.byref(self.pack.opt), _ptr(tokens), _ptr(state), _ptr(am), _ptr(n_valid), R, num_beams, L, _ptr(kv_prompt), _ptr(kv_gen),
                gen_cap, _ptr(anc), _ptr(logits), _ptr(ws), ws.numel(), self._stream()), step_name)

        def step(next_tokens, beam_src):
            t = steps[0]  # tokens generated before this one
            if t > 0:
                anc[:t] = anc[:t].index_select(1, beam_src)  # row r continues the hypothesis that lived in row beam_src[r]
            anc[t] = ident32                                   # the token fed now: its K / V go to row r's own slot t
            steps[0] = t + 1
            tokens.copy_(next_tokens)
            if t == 0:
                state[0] = 1  # (the call increments it: every per-step quantity is on the device, so ONE captured step replays)
            if use_graph and max_new_tokens > 2:
                if graph[0] is None:  # (once per engine the launch also runs outside capture; it rewrote this step's slot only)
                    graph[0] = self._capture_step(launch, (state,), warm=not getattr(self, warm_flag, False))
                    setattr(self, warm_flag, True)
                graph[0].replay()
            else:
                launch()
            if trace is not None:
                trace.append((next_tokens.clone(), beam_src.clone(), logits.clone()))
            return logits

        if plan.route == "beam_device":
            # (r4) plain beam search — the sample script's call: selection, ancestor-table update and the decode step as ONE captured graph per
            # generated token, nothing indexed by the step on the host (eilev_amd/beam.py::beam_search_device)
            out = self._beam_device_loop(launch, last, B, num_beams, max_new_tokens, d.vocab, state, tokens, anc, logits, length_penalty, eos_id, pad_id,
                                         early_stopping, num_return_sequences, use_graph, plan.dev_kw, plan.topk_ok, plan.advance_ok)
            setattr(self, warm_flag, True)
            return out
        return self._host_loop(plan, step, last, B, num_beams, max_new_tokens, length_penalty, eos_id, pad_id, early_stopping, num_return_sequences,
                               min_new_tokens)

    def _beam_device_loop(self, launch, first, B, num_beams, max_new_tokens, vocab, state, tokens, anc, logits, length_penalty, eos_id, pad_id,
                          early_stopping, num_return_sequences, use_graph, rules_kw, topk_ok, advance_ok, prefix_id=-1):
        """beam_search_device around ``launch()``, a decode step in the beam form (eilev_opt_decode_step_beam, eilev_t5beam_decode_step) that
        feeds ``tokens`` (R,), reads the ancestor table ``anc`` (gen_cap, R) and the counter ``state``, leaves the logits in ``logits`` (R, vocab)
        and increments state[0].  ``first``: the (B, vocab) logits in front of the first selection.  ``prefix_id``: the id the rules see in front
        of a hypothesis (flan-t5's decoder start token)."""
        from .beam import beam_search_device

        eos_l = eos_list(eos_id)
        keep = max(2, 1 + len(eos_l)) * num_beams
        gen_cap, R = anc.shape
        tpos = torch.zeros(1, dtype=torch.int64, device=self.device)
        ident_row = torch.arange(R, dtype=torch.int32, device=self.device).view(1, R)
        state[0] = 1

        def step_dev(next_tokens, beam_src):
            anc.copy_(anc.index_select(1, beam_src))  # rows of steps not reached yet hold stale slots: row t is set before it is ever read
            anc.index_copy_(0, tpos, ident_row)
            tokens.copy_(next_tokens)
            launch()
            tpos.add_(1)

        topk_fn = None
        if topk_ok:
            row_lp = torch.empty((R, keep), dtype=torch.float32, device=self.device)
            row_tok = torch.empty((R, keep), dtype=torch.int32, device=self.device)

            def topk_fn(buf, run_score):
                abi.check(self.lib.eilev_topk_logprob(_ptr(buf), _ptr(run_score), R, vocab, keep, _ptr(row_lp), _ptr(row_tok), self._stream()),
                          "eilev_topk_logprob")
                return row_lp, row_tok

        advance_fn = None
        if advance_ok:
            eos_arr = (C.c_int64 * max(1, len(eos_l)))(*eos_l)
            scratch = torch.empty(int(self.lib.eilev_beam_scratch_bytes(B, num_beams, keep, max_new_tokens)), dtype=torch.uint8, device=self.device)

            def advance_fn(lp_rows, tok_rows, st):  # the whole bookkeeping of a step, the tokens to feed and the ancestor table: one kernel
                abi.check(self.lib.eilev_beam_advance(
                    _ptr(lp_rows), _ptr(tok_rows), B, num_beams, keep, max_new_tokens, _ptr(state), eos_arr, len(eos_l), _ptr(st["pow_tab"]),
                    int(st["reciprocal"]), int(st["early"]), _ptr(st["run_seq"]), _ptr(st["run_score"]), _ptr(st["fin_seq"]), _ptr(st["fin_score"]),
                    _ptr(st["fin_len"]), _ptr(st["finished"]), _ptr(st["can_improve"]), _ptr(tokens), _ptr(anc), gen_cap, _ptr(scratch),
                    scratch.numel(), self._stream()), "eilev_beam_advance")

            def step_dev(next_tokens, beam_src):  # noqa: F811 (tokens / ancestors were written by eilev_beam_advance)
                launch()

        # with the two selection kernels a step is ONE C call that enqueues ~260 kernels (2.5 ms of GPU work): capturing it buys nothing per
        # token (2.565 vs 2.554 ms) and costs ~1.2 ms per generate() call — replayed graphs only on request (`engine.beam_capture = True`)
        # or when the selection runs as torch ops
        capture = use_graph and (advance_fn is None or self.beam_capture)
        if rules_kw is not None:
            # the rules of the call inside the per-row selection (eilev_rules_topk_logprob): row r's history is run_seq[r, 0 .. cur), which
            # eilev_beam_advance keeps in place, and cur = state[0] - 1 is the decode step's device counter (allow_device: advance_ok holds)
            rl = abi.load_rules()
            p_rules = abi.rules_params(rules_kw["repetition_penalty"], rules_kw["no_repeat_ngram_size"], rules_kw["min_new_tokens"], max_new_tokens,
                                       eos_l, pad_id, prefix_id, 0, 0)

            def topk_fn(buf, run_score, run_seq, cur_t):  # noqa: F811
                abi.check(rl.eilev_rules_topk_logprob(C.byref(p_rules), _ptr(buf), _ptr(run_score), R, vocab, keep, _ptr(state), _ptr(run_seq),
                                                      _ptr(row_lp), _ptr(row_tok), None, None, 0, self._stream()), "eilev_rules_topk_logprob")
                return row_lp, row_tok

        out = beam_search_device(step_dev, logits, first, B, num_beams, max_new_tokens, length_penalty, eos_id, pad_id, early_stopping,
                                 num_return_sequences, use_graph=capture, topk_fn=topk_fn, advance_fn=advance_fn, topk_history=rules_kw is not None)
        if rules_kw is not None:
            self.rules_stats = dict(path="device", steps=int(out.shape[1]))
        return out

    def _host_loop(self, plan, step, first, B, num_beams, max_new_tokens, length_penalty, eos_id, pad_id, early_stopping, num_return_sequences,
                   min_new_tokens):
        """The host loop of a plan (eilev_amd/sampling.py sample_loop, beam.py beam_search) over the decode step ``step``, and what such a
        call records: sample_stats when it drew, rules_stats when it carried rules (beam-search sampling records the former only)."""
        from . import beam, sampling

        rules = plan.rules or {}
        if plan.loop == "sample_loop":  # multinomial sampling, and greedy search with host rules
            ids = sampling.sample_loop(step, first, max_new_tokens, eos_id, pad_id, **plan.sampler, **{k: v for k, v in rules.items() if k != "fill_id"})
        else:
            ids = beam.beam_search(step, first, B, num_beams, max_new_tokens, length_penalty, eos_id, pad_id, early_stopping, num_return_sequences,
                                   sampler=plan.sampler, min_new_tokens=min_new_tokens, **rules)
        rec = dict(path="host", steps=int(ids.shape[1]))
        if plan.sampler is not None:
            self.sample_stats = rec
        if plan.with_rules and (plan.sampler is None or num_beams == 1):
            self.rules_stats = dict(rec)
        return ids

    def sample_decode(self, inputs_embeds, attention_mask, max_new_tokens, eos_id=-1, pad_id=1, temperature=1.0, top_k=50, top_p=1.0,
                      generator=None, repetition_penalty=1.0, min_new_tokens=0):
        """`generate(do_sample=True)` [hf generation/utils.py `_sample`]: prefill once, then one HIP decode step per drawn token.  The draw runs
        on the device in the captured step (sample_decode_device) unless `self.device_sampling` is off or the kernel does not take the call."""
        return self.beam_decode(inputs_embeds, attention_mask, max_new_tokens, 1, eos_id=eos_id, pad_id=pad_id,
                                sampler=dict(temperature=temperature, top_k=top_k, top_p=top_p, generator=generator,
                                             repetition_penalty=repetition_penalty, min_new_tokens=min_new_tokens))

    def _sample_setup(self, R, vocab, max_new_tokens, generator, uniforms, **spec):
        """The sampling library, the uniforms of a whole call — (max_new, R), drawn ONCE on the generator's device — and a function that makes
        the parameter block of one eilev_sample_select call."""
        smp = abi.load_sample()
        if not abi.sample_supported(vocab):
            raise NotImplementedError(f"device sampling: vocab {vocab} (at most {abi.SAMPLE_MAX_VOCAB}, a multiple of 4)")
        if uniforms is None:
            gdev = generator.device if generator is not None else self.device
            uniforms = torch.rand((max_new_tokens, R), generator=generator, device=gdev, dtype=torch.float32)
        uniforms = uniforms.to(self.device, torch.float32).contiguous()
        assert uniforms.shape == (max_new_tokens, R), uniforms.shape

        def params(step_offset, finalize):
            return abi.sample_params(max_new=max_new_tokens, step_offset=step_offset, finalize=finalize, **spec)

        return smp, uniforms, params

    def _rules_setup(self, vocab, max_new_tokens, **spec):
        """The rules library and a function that makes the parameter block of one of its calls."""
        rl = abi.load_rules()
        if not abi.rules_supported(vocab):
            raise NotImplementedError(f"device rules: vocab {vocab} (at most {abi.RULES_MAX_VOCAB}, a multiple of 4)")

        def params(step_offset, finalize):
            return abi.rules_params(max_new=max_new_tokens, step_offset=step_offset, finalize=finalize, **spec)

        return rl, params

    def _stamp(self, name):
        """Optional phase stamps for bench.py (events on the launch stream, no sync)."""
        if self.timing is not None:
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self.timing.append((name, ev))

    def _greedy_select(self, logits, R, vocab, state, finished, eos_id, pad_id, tokens, out):
        abi.check(self.lib.eilev_greedy_select(_ptr(logits), R, vocab, _ptr(state), _ptr(finished), eos_id, pad_id, _ptr(tokens), _ptr(out), out.shape[1],
                                               self._stream()), "eilev_greedy_select")

    @staticmethod
    def _trim_at_eos(out, n, eos):
        """The first n columns of `out` (n = the steps done), cut after the column where the last row emits its first EOS id (hf stops there);
        finished rows already hold the pad id.  A copy: `out` may belong to a cached graph entry."""
        ids = out[:, :n]
        if eos:
            is_eos = torch.isin(ids, torch.tensor(eos, dtype=torch.int64, device=out.device))
            first = torch.where(is_eos.any(dim=1), is_eos.float().argmax(dim=1) + 1, torch.full((ids.shape[0],), n, device=out.device))
            ids = ids[:, : int(first.max().item())]
        return ids.clone()

    def _capture_step(self, one_step, buffers, warm):
        """One decode step as a hipGraph, captured on a side stream that rejoins the current one.  ``warm``: run the step once outside capture
        first (lazy module loading of the kernels) and put ``buffers`` (the words the step advances) back; the cache slot it wrote is the
        one the first replay rewrites.  Capture does not execute: nothing has run for the step afterwards."""
        graph = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream(self.device)
        side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(side):
            if warm:
                snap = [b.clone() for b in buffers]
                one_step()
                for b, keep in zip(buffers, snap):
                    b.copy_(keep)
            # no cyclic garbage collection inside the capture: a dead reference cycle that still holds a device resource (an earlier
            # CUDAGraph, say) would be finalised by whichever allocation happens to trigger the collector, and releasing it while a
            # capture is open aborts the process (torch.cuda.graph no longer collects before it begins)
            gc_was_on = gc.isenabled()
            gc.disable()
            try:
                with torch.cuda.graph(graph, stream=side):
                    one_step()
            finally:
                if gc_was_on:
                    gc.enable()
        torch.cuda.current_stream(self.device).wait_stream(side)
        return graph

    def _run_steps(self, n_steps, one_step, graph, state, eos, poll_every, trace, logits, poll_last=False):
        """Replay (or launch) up to n_steps steps; with EOS ids, read state[1] back every poll_every steps and stop once no row is left.
        Returns the steps done."""
        done = 0
        while done < n_steps:
            if graph is not None:
                graph.replay()
            else:
                one_step()
                if trace is not None:
                    trace.append(logits.clone())
            done += 1
            if eos and (done % poll_every == 0 or (poll_last and done == n_steps)) and int(state[1].item()) == 0:
                break
        return done

    def _chunked_rows(self, call, B, pad_id, stats_name=None, per=32):
        """More decode rows than one call takes (the decode kernels stream the weights once for up to 32 rows; the reference accepts any batch
        size): ``call(i, j)`` on consecutive slices of ``per`` samples, shorter parts padded like hf pads rows that stopped early.
        ``stats_name``: the stats record of the whole call holds the longest part's steps."""
        parts, n_steps = [], 0
        for i in range(0, B, per):
            parts.append(call(i, min(i + per, B)))
            if stats_name:
                n_steps = max(n_steps, getattr(self, stats_name)["steps"])
        n = max(p.shape[1] for p in parts)
        if stats_name:
            setattr(self, stats_name, dict(path="device", steps=n_steps))
        return torch.cat([torch.nn.functional.pad(p, (0, n - p.shape[1]), value=int(pad_id)) for p in parts], dim=0)

    def _select_decode_device(self, inputs_embeds, attention_mask, max_new_tokens, eos, pad_id, key, extra, bind, use_graph, poll_every, trace,
                              kv_dtype="bf16"):
        """The cached OPT decode: one KV cache of capacity L + max_new, the stream layout, ONE captured step replayed per token (every per-step
        quantity is read from `state` on the device).  ``bind is None`` (greedy_decode): the decode step's own arg-max selects, the first token
        comes from eilev_greedy_select on the prefill's logits.  Else a selection of the caller's runs after the decode step (the draw of
        sample_decode_device, the rules + arg-max of rules_decode_device): the step's arg-max writes to scratch buffers (eos -1) and the
        selection then overwrites `tokens`.

        The captured step only depends on buffer ADDRESSES and on ``key`` — the kind of the call and what its selection depends on (the
        parameter block is passed by value) — plus (B, L, cap, eos, pad): the most recent graph is kept with its buffers in ONE slot and reused
        by calls of the same key (a call of another kind replaces it, so one KV cache is kept at a time).  ``extra(B)``: the selection's own
        buffers of a new entry.  ``bind(ent, step_offset, finalize) -> select(logits)``: the selection's closure over the entry's buffers, asked
        for twice per call; (0, 1) selects from the prefill's logits (state[0] = 0, it finalizes the step itself), (-1, 0) from the decode
        step's (which has already advanced state[0]).  ``trace``: a list that receives the prefill's logits and a copy of every eager step's; it turns capture off.  At most 32
        rows.  Returns int64 (B, n) new tokens.

        ``kv_dtype="fp8"`` (include/eilev_kv8.h): the prompt is prefilled into a bf16 cache of capacity L, quantised into an e4m3 cache of
        capacity L + max_new (eilev_kv8_quantize), the bf16 cache dropped, and the steps run eilev_kv8_decode_step.  The dtype is part of the
        graph's key.

        An engine of ``lm_weights="int4"`` runs eilev_w4_decode_step (include/eilev_w4.h) on the same buffers; the weight mode is part of the
        graph's key, ``self.w4_stats`` records the step."""
        d = self.dims
        B, L, _ = inputs_embeds.shape
        cap = L + max_new_tokens
        n_dec = max_new_tokens - 1
        if n_dec > 0:
            self.ensure_stream_layout(B)
        kv8 = self._kv8(kv_dtype)
        w4 = self._w4[0] if self.lm_weights == "int4" else None  # (an int4 engine: the int4 step; never together with kv8, which _kv8 refuses)
        graphable = use_graph and n_dec > 1 and trace is None
        route_name = str(key[0])
        key = tuple(key) + (str(self.lm_weights), B, L, cap, max_new_tokens, tuple(eos), int(pad_id), str(kv_dtype))
        ent = self._dec_cache if (graphable and self._dec_cache is not None and self._dec_cache["key"] == key) else None
        if ent is None:
            ent = dict(key=key, graph=None,
                       am=torch.empty((B, L), dtype=torch.int32, device=self.device),
                       n_valid=torch.empty(B, dtype=torch.int32, device=self.device),
                       kv=self.new_kv_cache(B, cap) if kv8 is None else self.new_kv8_cache(B, cap),
                       state=torch.zeros(2, dtype=torch.int32, device=self.device),
                       finished=torch.zeros(B, dtype=torch.uint8, device=self.device),
                       tokens=torch.zeros(B, dtype=torch.int64, device=self.device),
                       out=torch.empty((B, max_new_tokens), dtype=torch.int64, device=self.device),
                       logits=torch.empty((B, d.vocab), dtype=torch.float32, device=self.device),
                       ws=self._workspace("dec", (w4.eilev_w4_workspace_bytes(C.byref(d), B) if w4 is not None else
                                                  self.lib.eilev_opt_workspace_bytes(C.byref(d), B, 1) if kv8 is None else
                                                  kv8.eilev_kv8_workspace_bytes(C.byref(d), B))))
            if bind is not None:  # the decode step's own selection goes to buffers that are never read
                ent.update(argmax_out=torch.zeros((B, max_new_tokens), dtype=torch.int64, device=self.device),
                           argmax_fin=torch.zeros(B, dtype=torch.uint8, device=self.device), **extra(B))
            if graphable:
                self._dec_cache = None  # drop the previous entry (its KV cache) before keeping this one
                self._dec_cache = ent
        am, n_valid, kv = ent["am"], ent["n_valid"], ent["kv"]
        state, finished, tokens, out, logits, ws = ent["state"], ent["finished"], ent["tokens"], ent["out"], ent["logits"], ent["ws"]
        am.copy_(attention_mask.to(self.device, torch.int32))
        n_valid.copy_(am.sum(dim=1))
        state.zero_()
        finished.zero_()
        out.fill_(int(pad_id))
        if bind is None:
            step_fin, step_eos, step_out = finished, (eos[0] if eos else -1), out
            first, step = (lambda lg: self._greedy_select(lg, B, d.vocab, state, finished, step_eos, pad_id, tokens, out)), (lambda lg: None)
        else:
            step_fin, step_eos, step_out = ent["argmax_fin"], -1, ent["argmax_out"]
            first, step = bind(ent, 0, 1), bind(ent, -1, 0)  # (the decode step has already advanced state[0]: step_offset -1, no finalize)
        if kv8 is None:
            last, _, _ = self.prefill(inputs_embeds, am, kv_cache=kv, kv_capacity=cap)
        else:  # (the call's peak memory holds one bf16 cache of the prompt: the prefill kernels write bf16)
            last, _, kv16 = self.prefill(inputs_embeds, am, kv_capacity=L)
            abi.check(kv8.eilev_kv8_quantize(C.byref(d), _ptr(kv16), B, L, L, _ptr(kv), cap, self._stream()), "eilev_kv8_quantize")
            del kv16
        self._stamp("prefill_done")
        if trace is not None:
            trace.append(last.clone())
        first(last)

        step_fn, step_name = (self.lib.eilev_opt_decode_step, "eilev_opt_decode_step") if kv8 is None else (kv8.eilev_kv8_decode_step, "eilev_kv8_decode_step")
        table = ()
        if w4 is not None:  # the same arguments with the per-layer table of int4 matrices after the weights
            step_fn, step_name, table = w4.eilev_w4_decode_step, "eilev_w4_decode_step", (self._w4[1],)
            self.w4_stats = dict(step=step_name if n_dec > 0 else None, rows=B, route=route_name, steps=0)  # (one new token: the prefill alone)

        def one_step():
            abi.check(step_fn(
                C.byref(d), C.byref(self.pack.opt), *table, _ptr(tokens), _ptr(state), _ptr(am), _ptr(n_valid), B, L, _ptr(kv), cap,
                _ptr(logits), _ptr(step_fin), step_eos, pad_id, _ptr(step_out), max_new_tokens, _ptr(ws), ws.numel(),
                self._stream()), step_name)
            step(logits)

        graph = ent["graph"] if graphable else None
        if graphable and graph is None:  # (once per engine the step also runs outside capture; it wrote KV slot L, as the first replay does)
            graph = ent["graph"] = self._capture_step(one_step, (state, finished, tokens, out), warm=not self._decode_warm)
            self._decode_warm = True
        done_steps = self._run_steps(n_dec, one_step, graph, state, eos, poll_every, trace, logits)
        if w4 is not None:
            self.w4_stats["steps"] = int(done_steps)
        return self._trim_at_eos(out, 1 + done_steps, eos)

    def _sampling_selection(self, rows, vocab, max_new, prefix_id, eos, pad_id, generator=None, uniforms=None, no_repeat_ngram_size=0, **warp):
        """Sampling (+ n-gram ban) as a selection (key, extra, bind, uniforms) of the two decode loops: eilev_sample_select after the decode
        step, eilev_rules_ban in front of it (hf applies the ban before the warpers).  ``extra(rows)``: the selection's own buffers;
        ``bind(bufs, step_offset, finalize)``: its closure over the loop's buffers and those; ``uniforms``: the whole call's, (max_new, rows)."""
        ngram, min_new = int(no_repeat_ngram_size or 0), warp.pop("min_new_tokens", 0)
        smp, uni_all, params = self._sample_setup(rows, vocab, max_new, generator, uniforms, eos_ids=eos, pad_id=pad_id, prefix_id=prefix_id,
                                                  min_new=min_new, **warp)
        rl, ban_params = self._rules_setup(vocab, max_new, no_repeat_ngram=ngram, eos_ids=eos, pad_id=pad_id, prefix_id=prefix_id) if ngram else (None, None)

        def extra(rows):
            return dict(uni=torch.empty((max_new, rows), dtype=torch.float32, device=self.device),
                        scratch=torch.empty(int(smp.eilev_sample_scratch_bytes(rows, vocab)), dtype=torch.uint8, device=self.device))

        def bind(b, step_offset, finalize):
            p_ban, p_draw = (ban_params(step_offset, 0) if ngram else None), params(step_offset, finalize)
            if finalize:  # (asked once per call: the call's uniforms go into the loop's buffer)
                b["uni"].copy_(uni_all)

            state, out, scratch = b["state"], b["out"], b["scratch"]

            def select(lg):
                if ngram:
                    abi.check(rl.eilev_rules_ban(C.byref(p_ban), _ptr(lg), rows, vocab, _ptr(state), _ptr(out), self._stream()), "eilev_rules_ban")
                abi.check(smp.eilev_sample_select(C.byref(p_draw), _ptr(lg), rows, vocab, _ptr(b["uni"]), _ptr(state), _ptr(b["finished"]), _ptr(b["tokens"]),
                                                  _ptr(out), None, _ptr(scratch) if scratch.numel() else None, scratch.numel(), self._stream()),
                          "eilev_sample_select")
            return select

        key = ("sample", float(warp["temperature"]), int(warp["top_k"] or 0), float(warp["top_p"]), float(warp["repetition_penalty"]), int(min_new), ngram)
        return key, extra, bind, uni_all

    def _rules_selection(self, rows, vocab, max_new, prefix_id, eos, pad_id, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0):
        """The logits rules as a selection of the two decode loops (see _sampling_selection): eilev_rules_select — repetition penalty, n-gram
        ban, minimum length, up to 8 EOS ids, then the arg-max — after the decode step."""
        ngram = int(no_repeat_ngram_size or 0)
        rl, params = self._rules_setup(vocab, max_new, repetition_penalty=repetition_penalty, no_repeat_ngram=ngram, min_new=min_new_tokens, eos_ids=eos,
                                       pad_id=pad_id, prefix_id=prefix_id)

        def bind(b, step_offset, finalize):
            p = params(step_offset, finalize)
            return lambda lg: abi.check(rl.eilev_rules_select(C.byref(p), _ptr(lg), rows, vocab, _ptr(b["state"]), _ptr(b["finished"]), _ptr(b["tokens"]),
                                                              _ptr(b["out"]), None, None, 0, self._stream()), "eilev_rules_select")

        return ("rules", float(repetition_penalty), ngram, int(min_new_tokens)), (lambda rows: {}), bind, None

    def _decode_selected(self, selection, stats_name, inputs_embeds, attention_mask, max_new_tokens, eos_id, pad_id, start_id, use_graph, poll_every,
                         trace, kv_dtype="bf16", **spec):
        """The four device entry points: ``selection`` (_sampling_selection, _rules_selection) with ``spec`` on the OPT loop, or with a
        ``start_id`` on the flan-t5 loop, whose ids begin with the start token, which the rules see (prefix_id) as hf's processors do.
        More than 32 rows run in parts (the selection of the whole call is made first: its uniforms are drawn ONCE).  Records
        ``stats_name`` = dict(path="device", steps=n)."""
        t5, B = start_id is not None, inputs_embeds.shape[0]
        start = torch.full((B, 1 if t5 else 0), int(start_id or 0), dtype=torch.int64, device=self.device)
        if max_new_tokens <= 0:
            return start
        eos = eos_list(eos_id)
        key, extra, bind, uniforms = selection(B, (self.t5dims if t5 else self.dims).vocab, max_new_tokens, int(start_id) if t5 else -1, eos, pad_id, **spec)
        if B > 32:
            if trace is not None:
                raise ValueError("trace: at most 32 decode rows")
            part = lambda i, j: spec if uniforms is None else dict(spec, generator=None, uniforms=uniforms[:, i:j])  # noqa: E731
            ids = self._chunked_rows(lambda i, j: self._decode_selected(
                selection, stats_name, inputs_embeds[i:j], attention_mask[i:j], max_new_tokens, eos_id, pad_id, start_id, use_graph, poll_every, None,
                kv_dtype, **part(i, j))[:, start.shape[1]:], B, pad_id, stats_name)
            return torch.cat((start, ids), dim=1)
        if t5:
            ids = self._t5_select_device(inputs_embeds, attention_mask, max_new_tokens, eos, pad_id, start_id,
                                         lambda b, step_offset, finalize: bind(dict(b, **extra(B)), step_offset, finalize), use_graph, poll_every, trace)
        else:
            ids = self._select_decode_device(inputs_embeds, attention_mask, max_new_tokens, eos, pad_id, key, extra, bind, use_graph, poll_every, trace,
                                             kv_dtype)
        setattr(self, stats_name, dict(path="device", steps=int(ids.shape[1])))
        return torch.cat((start, ids), dim=1) if t5 else ids

    def sample_decode_device(self, inputs_embeds, attention_mask, max_new_tokens, eos_id=-1, pad_id=1, temperature=1.0, top_k=50, top_p=1.0,
                             repetition_penalty=1.0, min_new_tokens=0, generator=None, use_graph=True, poll_every=8, trace=None, uniforms=None,
                             no_repeat_ngram_size=0, kv_dtype="bf16"):
        """Multinomial sampling with the draw on the device (include/eilev_sample.h): _select_decode_device with _sampling_selection.
        ``eos_id``: an id or up to 8 ids.  ``trace``: a list that receives a copy of every step's logits (use_graph=False; the n-gram ban is
        already written into them).  ``uniforms``: (max_new, rows) in [0, 1) instead of the ones drawn from ``generator``.  Returns int64
        (B, n) new tokens."""
        return self._decode_selected(self._sampling_selection, "sample_stats", inputs_embeds, attention_mask, max_new_tokens, eos_id, pad_id, None,
                                     use_graph, poll_every, trace, kv_dtype, temperature=temperature, top_k=top_k, top_p=top_p,
                                     repetition_penalty=repetition_penalty, min_new_tokens=min_new_tokens, generator=generator, uniforms=uniforms,
                                     no_repeat_ngram_size=no_repeat_ngram_size)

    def rules_decode_device(self, inputs_embeds, attention_mask, max_new_tokens, eos_id=-1, pad_id=1, repetition_penalty=1.0, no_repeat_ngram_size=0,
                            min_new_tokens=0, use_graph=True, poll_every=8, trace=None, kv_dtype="bf16"):
        """Greedy search with logits rules on the device (include/eilev_rules.h): _select_decode_device with _rules_selection.  ``trace``: a
        list that receives a copy of every step's logits (use_graph=False).  Returns int64 (B, n) new tokens."""
        return self._decode_selected(self._rules_selection, "rules_stats", inputs_embeds, attention_mask, max_new_tokens, eos_id, pad_id, None,
                                     use_graph, poll_every, trace, kv_dtype, repetition_penalty=repetition_penalty,
                                     no_repeat_ngram_size=no_repeat_ngram_size, min_new_tokens=min_new_tokens)

    def _t5_select_device(self, inputs_embeds, attention_mask, max_new_tokens, eos, pad_id, start_id, bind, use_graph, poll_every, trace):
        """The flan-t5 decode loop: encoder and cross K/V once, then one decoder step + the caller's selection (position and bookkeeping read
        from a device `state` word) captured into a hipGraph and replayed.  ``bind``: as in _select_decode_device, asked for (0, 1).  At most
        32 rows.  Returns the new ids (B, n), without the start token."""
        d = self.t5dims
        B = inputs_embeds.shape[0]
        enc = self.t5_encode(inputs_embeds, attention_mask)
        self._stamp("t5_encoder_done")
        ckv = self.t5_cross_kv(enc)
        self._stamp("prefill_done")  # encoder + cross K/V = what the prefill is for the decoder-only model
        L = enc.shape[1]
        cap = max_new_tokens
        am = attention_mask.to(self.device, torch.int32).contiguous()
        skv = torch.empty(int(self.lib.eilev_t5_self_kv_bytes(C.byref(d), B, cap)), dtype=torch.uint8, device=self.device)
        state = torch.zeros(2, dtype=torch.int32, device=self.device)
        finished = torch.zeros(B, dtype=torch.uint8, device=self.device)
        tokens = torch.full((B,), int(start_id), dtype=torch.int64, device=self.device)
        out = torch.full((B, max_new_tokens), int(pad_id), dtype=torch.int64, device=self.device)
        logits = torch.empty((B, d.vocab), dtype=torch.float32, device=self.device)
        ws = self._workspace("t5dec", self.lib.eilev_t5_workspace_bytes(C.byref(d), B, 1, max(L, cap)))
        step = bind(dict(state=state, finished=finished, tokens=tokens, out=out), 0, 1)  # (every step selects and finalizes itself)

        def one_step():
            abi.check(self.lib.eilev_t5_decode_step(C.byref(d), C.byref(self.pack.t5), _ptr(tokens), _ptr(state), _ptr(am), B, _ptr(skv), cap,
                                                    _ptr(ckv), L, _ptr(logits), _ptr(ws), ws.numel(), self._stream()), "eilev_t5_decode_step")
            step(logits)

        graph = None
        if use_graph and max_new_tokens > 1 and trace is None:  # (the warm-up step only touches cache slot 0, which the replay rewrites)
            graph = self._capture_step(one_step, (state, finished, tokens, out), warm=True)
        n = self._run_steps(max_new_tokens, one_step, graph, state, eos, poll_every, trace, logits, poll_last=True)
        return self._trim_at_eos(out, n, eos)

    def t5_sample_device(self, inputs_embeds, attention_mask, max_new_tokens, eos_id=1, pad_id=0, start_id=0, temperature=1.0, top_k=50, top_p=1.0,
                         repetition_penalty=1.0, min_new_tokens=0, generator=None, use_graph=True, poll_every=8, trace=None, uniforms=None,
                         no_repeat_ngram_size=0):
        """t5_greedy with _sampling_selection in place of the arg-max: decoder ids (B, 1 + n) INCLUDING the start token.  ``trace`` /
        ``uniforms``: as sample_decode_device."""
        return self._decode_selected(self._sampling_selection, "sample_stats", inputs_embeds, attention_mask, max_new_tokens, eos_id, pad_id, start_id,
                                     use_graph, poll_every, trace, temperature=temperature, top_k=top_k, top_p=top_p,
                                     repetition_penalty=repetition_penalty, min_new_tokens=min_new_tokens, generator=generator, uniforms=uniforms,
                                     no_repeat_ngram_size=no_repeat_ngram_size)

    def t5_rules_device(self, inputs_embeds, attention_mask, max_new_tokens, eos_id=1, pad_id=0, start_id=0, repetition_penalty=1.0,
                        no_repeat_ngram_size=0, min_new_tokens=0, use_graph=True, poll_every=8, trace=None):
        """t5_greedy with _rules_selection in place of eilev_greedy_select: decoder ids (B, 1 + n) INCLUDING the start token.  ``trace``: as
        rules_decode_device."""
        return self._decode_selected(self._rules_selection, "rules_stats", inputs_embeds, attention_mask, max_new_tokens, eos_id, pad_id, start_id,
                                     use_graph, poll_every, trace, repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                                     min_new_tokens=min_new_tokens)

    # ---- encoder-decoder LM (flan-t5) ------------------------------------------------------------------------
    def t5_encode(self, inputs_embeds, attention_mask):
        """Encoder stack [hf T5Stack]: (B, L, D) bf16 -> encoder last_hidden_state (B, L, D)."""
        d = self.t5dims
        x = inputs_embeds.contiguous()
        B, L, _ = x.shape
        am = attention_mask.to(self.device, torch.int32).contiguous()
        out = torch.empty_like(x)
        nb = self.lib.eilev_t5_workspace_bytes(C.byref(d), B, L, L)
        ws = self._workspace("t5", nb)
        abi.check(self.lib.eilev_t5_encode(C.byref(d), C.byref(self.pack.t5), _ptr(x), _ptr(am), B, L, _ptr(out), _ptr(ws), ws.numel(),
                                           self._stream()), "eilev_t5_encode")
        return out

    def t5_cross_kv(self, enc_out):
        d = self.t5dims
        B, L, _ = enc_out.shape
        kv = torch.empty(int(self.lib.eilev_t5_cross_kv_bytes(C.byref(d), B, L)), dtype=torch.uint8, device=self.device)
        nb = self.lib.eilev_t5_workspace_bytes(C.byref(d), B, L, L)
        ws = self._workspace("t5", nb)
        abi.check(self.lib.eilev_t5_cross_kv(C.byref(d), C.byref(self.pack.t5), _ptr(enc_out.contiguous()), B, L, _ptr(kv), _ptr(ws),
                                             ws.numel(), self._stream()), "eilev_t5_cross_kv")
        return kv

    def t5_decode(self, dec_ids, enc_mask, past_len, self_kv, cap, cross_kv, enc_len):
        """Decoder over dec_ids (B, T) at positions past_len..: fp32 logits (B, T, vocab)."""
        d = self.t5dims
        ids = dec_ids.to(self.device, torch.int64).contiguous()
        B, T = ids.shape
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= d.vocab):
            raise IndexError("decoder_input_ids out of range")
        am = enc_mask.to(self.device, torch.int32).contiguous()
        logits = torch.empty((B, T, d.vocab), dtype=torch.float32, device=self.device)
        nb = self.lib.eilev_t5_workspace_bytes(C.byref(d), B, T, max(enc_len, past_len + T))
        ws = self._workspace("t5", nb)
        abi.check(self.lib.eilev_t5_decode(C.byref(d), C.byref(self.pack.t5), _ptr(ids), _ptr(am), B, T, past_len, _ptr(self_kv), cap,
                                           _ptr(cross_kv), enc_len, _ptr(logits), _ptr(ws), ws.numel(), self._stream()), "eilev_t5_decode")
        return logits

    def t5_forward(self, inputs_embeds, attention_mask, decoder_input_ids):
        """Teacher-forced logits (B, T, vocab) fp32 + encoder output [ref:eilev/model/v2.py:228-238]."""
        d = self.t5dims
        enc = self.t5_encode(inputs_embeds, attention_mask)
        ckv = self.t5_cross_kv(enc)
        B, T = decoder_input_ids.shape
        skv = torch.empty(int(self.lib.eilev_t5_self_kv_bytes(C.byref(d), B, T)), dtype=torch.uint8, device=self.device)
        return self.t5_decode(decoder_input_ids, attention_mask, 0, skv, T, ckv, enc.shape[1]), enc

    def t5_forward_debug(self, inputs_embeds, attention_mask, decoder_input_ids, decoder_attention_mask=None, hidden_states=False):
        """t5_forward with what the reference's forward can also pass down (ref:eilev/model/v2.py:228-238): decoder_attention_mask (B, T)
        and output_hidden_states -> (logits, enc, encoder hidden_states (layers + 1, B, L, D) | None, decoder hidden_states | None)."""
        d = self.t5dims
        x = inputs_embeds.contiguous()
        B, L, D = x.shape
        am = attention_mask.to(self.device, torch.int32).contiguous()
        enc = torch.empty_like(x)
        enc_hs = torch.empty((d.enc_layers + 1, B, L, D), dtype=x.dtype, device=self.device) if hidden_states else None
        ws = self._workspace("t5", self.lib.eilev_t5_workspace_bytes(C.byref(d), B, L, L))
        abi.check(self.lib.eilev_t5_encode_debug(C.byref(d), C.byref(self.pack.t5), _ptr(x), _ptr(am), B, L, _ptr(enc),
                                                 _ptr(enc_hs) if hidden_states else None, _ptr(ws), ws.numel(), self._stream()), "eilev_t5_encode_debug")
        ckv = self.t5_cross_kv(enc)
        ids = decoder_input_ids.to(self.device, torch.int64).contiguous()
        T = ids.shape[1]
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) >= d.vocab):
            raise IndexError("decoder_input_ids out of range")
        dm = None
        if decoder_attention_mask is not None:
            dm = (decoder_attention_mask.to(self.device) != 0).to(torch.int32).contiguous()
            if dm.shape != ids.shape:
                raise ValueError(f"decoder_attention_mask {tuple(dm.shape)} does not match decoder_input_ids {tuple(ids.shape)}")
            if not bool(dm[:, 0].all()):  # a query row with no visible key at all: hf adds two finfo.min there, not a defined attention
                raise NotImplementedError("decoder_attention_mask must keep the first target position of every row")
        skv = torch.empty(int(self.lib.eilev_t5_self_kv_bytes(C.byref(d), B, T)), dtype=torch.uint8, device=self.device)
        logits = torch.empty((B, T, d.vocab), dtype=torch.float32, device=self.device)
        dec_hs = torch.empty((d.dec_layers + 1, B, T, D), dtype=x.dtype, device=self.device) if hidden_states else None
        ws = self._workspace("t5", self.lib.eilev_t5_workspace_bytes(C.byref(d), B, T, max(L, T)))
        abi.check(self.lib.eilev_t5_decode_debug(C.byref(d), C.byref(self.pack.t5), _ptr(ids), _ptr(am), None if dm is None else _ptr(dm), B, T, 0,
                                                 _ptr(skv), T, _ptr(ckv), L, _ptr(logits), _ptr(dec_hs) if hidden_states else None, _ptr(ws),
                                                 ws.numel(), self._stream()), "eilev_t5_decode_debug")
        return logits, enc, enc_hs, dec_hs

    def t5_greedy(self, inputs_embeds, attention_mask, max_new_tokens, eos_id=1, pad_id=0, start_id=0, use_graph=True, poll_every=8):
        """Greedy generation for the encoder-decoder LM [ref:eilev/model/v2.py:318-322 -> hf _sample]: returns decoder ids
        (B, 1 + n) INCLUDING the start token, like HF does for encoder-decoder models.  _t5_select_device with eilev_greedy_select as
        the selection."""
        B, vocab = inputs_embeds.shape[0], self.t5dims.vocab
        start = torch.full((B, 1), int(start_id), dtype=torch.int64, device=self.device)
        if max_new_tokens <= 0:
            return start
        ids = self._t5_select_device(
            inputs_embeds, attention_mask, max_new_tokens, eos_list(eos_id), pad_id, start_id,
            lambda b, step_offset, finalize: (lambda lg: self._greedy_select(lg, B, vocab, b["state"], b["finished"], eos_id, pad_id, b["tokens"], b["out"])),
            use_graph, poll_every, None)
        return torch.cat((start, ids), dim=1)

    def t5_greedy_lookup(self, inputs_embeds, attention_mask, text_ids, max_new_tokens, num_tokens=10, ngram=2, eos_id=1, pad_id=0, start_id=0):
        """t5_greedy with prompt-lookup drafts (batch 1): returns the decoder ids of t5_greedy, start id included.  The corpus is the
        encoder's text ids (``text_ids``), then the generated decoder ids.  Each step verifies [last, d1 .. dm] with eilev_t5_decode
        (past_len = committed count) or runs eilev_t5_decode_step when there is no draft.  Counters of the call: ``self.pld_stats``."""
        d = self.t5dims
        k, n_new = self._lookup_head(inputs_embeds.shape[0], num_tokens, ngram, max_new_tokens)
        enc = self.t5_encode(inputs_embeds, attention_mask)
        ckv = self.t5_cross_kv(enc)
        L = enc.shape[1]
        start = torch.full((1, 1), int(start_id), dtype=torch.int64, device=self.device)
        if n_new <= 0:
            return start
        cap = n_new + k
        pld, b, n_text = self._pld_buffers(text_ids, n_new, k, d.vocab)
        params = abi.pld_params(k, ngram, n_new, 1, cap, n_text + n_new, eos_list(eos_id))
        am = attention_mask.to(self.device, torch.int32).contiguous()
        skv = torch.empty(int(self.lib.eilev_t5_self_kv_bytes(C.byref(d), 1, cap)), dtype=torch.uint8, device=self.device)
        ws = self._workspace("t5pld", self.lib.eilev_t5_workspace_bytes(C.byref(d), 1, k + 1, max(L, cap)))
        window, logits, state, out = b["window"], b["logits"], b["state"], b["out"]
        window[0] = int(start_id)

        def verify(c, m):
            abi.check(self.lib.eilev_t5_decode(C.byref(d), C.byref(self.pack.t5), _ptr(window), _ptr(am), 1, m + 1, c, _ptr(skv), cap, _ptr(ckv), L,
                                               _ptr(logits), _ptr(ws), ws.numel(), self._stream()), "eilev_t5_decode")
            return logits

        def single(c):  # state[0] == c tokens fed, window[0] == the next one to feed
            abi.check(self.lib.eilev_t5_decode_step(C.byref(d), C.byref(self.pack.t5), _ptr(window), _ptr(state), _ptr(am), 1, _ptr(skv), cap,
                                                    _ptr(ckv), L, _ptr(logits), _ptr(ws), ws.numel(), self._stream()), "eilev_t5_decode_step")
            return logits

        abi.check(pld.eilev_pld_draft(C.byref(params), _ptr(b["corpus"]), _ptr(b["corpus_len"]), _ptr(window), _ptr(b["status"]), self._stream()),
                  "eilev_pld_draft")
        ids = self._lookup_tail(b["status"].tolist(), verify, single, lambda lg, rows: self._pld_commit(pld, params, b, lg, rows, d.vocab), out)
        return torch.cat((start, ids), dim=1)

    def t5_beam(self, inputs_embeds, attention_mask, max_new_tokens, num_beams, length_penalty=1.0, eos_id=1, pad_id=0, start_id=0,
                early_stopping=False, num_return_sequences=1, sampler=None, min_new_tokens=0, rules=None, use_graph=True):
        """Beam search for the encoder-decoder LM [sample default num_beams=5, length_penalty=-1; hf generation/utils.py:3208+].

        The device loop (plain beam search and the numeric rules, head size 64, at most 32 beams; `_t5_beam_device`): the encoder and the cross
        K/V once per SAMPLE, no cache row ever copied or replicated, selection + ancestor table + decode step per token as in beam_decode.
        Everything else (beam-search sampling, user processors, stopping criteria, num_beams == 1, other head sizes, ``beam_device_loop =
        False``) keeps the host loop: the cross K/V replicated to the beams, every step reorders the self-attention cache rows by the
        surviving beams' parents and runs eilev_t5_decode on all rows.  ``self.t5_beam_stats`` = dict(path="device" | "host", steps=n)."""
        plan = route.plan_decode(route.Caps.of(self), num_beams, sampler, rules, eos_id, min_new_tokens, max_new_tokens, False, in_search_loop=True)
        # hf generation/utils.py:3319 `output_fill_value = pad_token_id or eos_token_id[0] ...`: T5's pad id 0 is falsy, finished hypotheses get the EOS id
        if pad_id == 0 and plan.pad_from_eos:
            pad_id = (eos_list(eos_id) or [-1])[0]
        d = self.t5dims
        device = dict(sample_device=self.t5_sample_device, rules_device=self.t5_rules_device).get(plan.route)
        if device is not None:
            return device(inputs_embeds, attention_mask, max_new_tokens, eos_id=eos_id, pad_id=pad_id, start_id=start_id, **plan.dev_kw)
        if plan.chunk and inputs_embeds.shape[0] > plan.chunk:  # at most 32 decode rows per call: sample group by sample group, each planned again
            return self._chunked_rows(lambda i, j: self.t5_beam(
                inputs_embeds[i:j], attention_mask[i:j], max_new_tokens, num_beams, length_penalty, eos_id, pad_id, start_id, early_stopping,
                num_return_sequences, sampler, min_new_tokens, rules, use_graph), inputs_embeds.shape[0], pad_id, "t5_beam_stats", per=plan.chunk)
        if plan.route == "beam_device":
            return self._t5_beam_device(inputs_embeds, attention_mask, max_new_tokens, num_beams, length_penalty, eos_id, pad_id, start_id,
                                        early_stopping, num_return_sequences, use_graph, plan.dev_kw, plan.topk_ok, plan.advance_ok)
        if plan.start_prefix:  # hf's processors see the start token (the plan's own copy of the rules: the caller's dict stays as it is)
            plan = plan._replace(rules=dict(plan.rules, prefix=torch.full((inputs_embeds.shape[0], 1), int(start_id), dtype=torch.int64,
                                                                          device=self.device)))
        enc = self.t5_encode(inputs_embeds, attention_mask)
        B, L, _ = enc.shape
        R = B * num_beams
        planes = 2 * d.dec_layers
        ckv = self.t5_cross_kv(enc).view(planes, B, -1).repeat_interleave(num_beams, dim=1).contiguous()
        am = attention_mask.to(self.device, torch.int32).repeat_interleave(num_beams, dim=0).contiguous()
        cap = max_new_tokens + 1
        skv = torch.zeros(int(self.lib.eilev_t5_self_kv_bytes(C.byref(d), R, cap)), dtype=torch.uint8, device=self.device).view(planes, R, -1)
        start = torch.full((R, 1), int(start_id), dtype=torch.int64, device=self.device)
        first = self.t5_decode(start, am, 0, skv, cap, ckv, L)[:, 0]
        steps = [0]

        def step(next_tokens, beam_src):
            nonlocal skv
            skv = skv.index_select(1, beam_src)
            steps[0] += 1
            return self.t5_decode(next_tokens.view(R, 1), am, steps[0], skv, cap, ckv, L)[:, 0]

        ids = self._host_loop(plan, step, first[::num_beams].contiguous(), B, num_beams, max_new_tokens, length_penalty, eos_id, pad_id,
                              early_stopping, num_return_sequences, min_new_tokens)
        self.t5_beam_stats = dict(path="host", steps=int(ids.shape[1]))
        head = torch.full((ids.shape[0], 1), int(start_id), dtype=torch.int64, device=self.device)
        return torch.cat((head, ids), dim=1)

    def _t5_beam_device(self, inputs_embeds, attention_mask, max_new_tokens, num_beams, length_penalty, eos_id, pad_id, start_id, early_stopping,
                        num_return_sequences, use_graph, rules_kw, topk_ok, advance_ok):
        """The device loop of t5_beam on B * num_beams <= 32 rows (include/eilev_t5beam.h holds the layout).  The decoder start token plays the
        part of OPT's prompt: eilev_t5_decode on the B samples fills a start cache of capacity 1 and gives the first logits; generated
        tokens go to a generation cache with one row per beam slot, found through the ancestor table that eilev_beam_advance keeps; the
        cross K/V and the padding mask stay one row per sample.  `_beam_device_loop` with eilev_t5beam_decode_step as the step; the rules
        see the start token in front of a hypothesis (prefix_id), as hf's processors do."""
        d = self.t5dims
        tb = abi.load_t5beam()
        enc = self.t5_encode(inputs_embeds, attention_mask)
        B, L, _ = enc.shape
        R = B * num_beams
        gen_cap = max(1, max_new_tokens)
        ckv = self.t5_cross_kv(enc)
        am = attention_mask.to(self.device, torch.int32).contiguous()
        kv_start = torch.empty(int(self.lib.eilev_t5_self_kv_bytes(C.byref(d), B, 1)), dtype=torch.uint8, device=self.device)
        start = torch.full((B, 1), int(start_id), dtype=torch.int64, device=self.device)
        first = self.t5_decode(start, am, 0, kv_start, 1, ckv, L)[:, 0].contiguous()
        kv_gen = torch.empty(int(self.lib.eilev_t5_self_kv_bytes(C.byref(d), R, gen_cap)), dtype=torch.uint8, device=self.device)
        anc = torch.zeros((gen_cap, R), dtype=torch.int32, device=self.device)
        state = torch.zeros(2, dtype=torch.int32, device=self.device)
        tokens = torch.zeros(R, dtype=torch.int64, device=self.device)
        logits = torch.empty((R, d.vocab), dtype=torch.float32, device=self.device)
        ws = self._workspace("t5beam", int(tb.eilev_t5beam_workspace_bytes(C.byref(d), R, num_beams, L, gen_cap)))

        def launch():
            abi.check(tb.eilev_t5beam_decode_step(
                C.byref(d), C.byref(self.pack.t5), _ptr(tokens), _ptr(state), _ptr(am), R, num_beams, _ptr(kv_start), _ptr(kv_gen), gen_cap, _ptr(anc),
                _ptr(ckv), L, _ptr(logits), _ptr(ws), ws.numel(), self._stream()), "eilev_t5beam_decode_step")

        ids = self._beam_device_loop(launch, first, B, num_beams, max_new_tokens, d.vocab, state, tokens, anc, logits, length_penalty, eos_id, pad_id,
                                     early_stopping, num_return_sequences, use_graph, rules_kw, topk_ok, advance_ok, prefix_id=int(start_id))
        self.t5_beam_stats = dict(path="device", steps=int(ids.shape[1]))
        head = torch.full((ids.shape[0], 1), int(start_id), dtype=torch.int64, device=self.device)
        return torch.cat((head, ids), dim=1)


    def t5_sample(self, inputs_embeds, attention_mask, max_new_tokens, eos_id=1, pad_id=0, start_id=0, temperature=1.0, top_k=50, top_p=1.0,
                  generator=None, repetition_penalty=1.0, min_new_tokens=0):
        """`generate(do_sample=True)` for the encoder-decoder LM (the decoder start token in front, like t5_greedy / t5_beam); the draw runs on
        the device (t5_sample_device) under the conditions of sample_decode."""
        return self.t5_beam(inputs_embeds, attention_mask, max_new_tokens, 1, eos_id=eos_id, pad_id=pad_id, start_id=start_id,
                            sampler=dict(temperature=temperature, top_k=top_k, top_p=top_p, generator=generator,
                                         repetition_penalty=repetition_penalty, min_new_tokens=min_new_tokens))


def abi_dtype(t: torch.Tensor) -> int:
    return 0 if t.dtype == torch.float32 else 1

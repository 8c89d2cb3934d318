"""Python handle on the native LLaMA decoder engine (``ss_llama_*`` in the C ABI).

Owns the device memory (torch tensors) the engine works in — merged/concatenated weights, the
KV-cache slab and activation workspace — and exposes the KV cache in the reference's layout
(``past_key_values``: tuple over layers of ``(k, v)`` each ``[1, n_heads, len, head_dim]``, keys
post-RoPE) as zero-copy views.
"""
import contextlib
import ctypes as C

import torch

from . import _lib, ops, tune
from ._lib import check, lib

ATTN_PROJ = ("q_proj", "k_proj", "v_proj", "o_proj")
MLP_PROJ = ("gate_proj", "up_proj", "down_proj")


def rope_tables(head_dim, max_pos, dtype, base=10000.0):
    """cos/sin tables of LlamaRotaryEmbedding (modeling_llama_xformer.py:118-134): fp32
    ``cat(freqs, freqs)``, cast to the model dtype by the module-level ``.to(dtype)``."""
    inv_freq = 1.0 / (base ** (torch.arange(0, head_dim, 2).float() / head_dim))
    t = torch.arange(max_pos, dtype=inv_freq.dtype)
    freqs = torch.einsum("i,j->ij", t, inv_freq)
    emb = torch.cat((freqs, freqs), dim=-1)
    return emb.cos().to(dtype), emb.sin().to(dtype)


def _merged(sd, name, dtype, device, lora_scaling):
    """W (+ (alpha/r) B A when LoRA factors are present), merged in fp32 on the device."""
    w = sd[name + ".weight"].to(device=device)
    a = sd.get(name + ".lora_A.weight", sd.get(name + ".lora_A.default.weight"))
    b = sd.get(name + ".lora_B.weight", sd.get(name + ".lora_B.default.weight"))
    if a is not None and b is not None:
        w = w.float() + lora_scaling * (b.to(device=device).float() @ a.to(device=device).float())
    return w.to(dtype).contiguous()


def _prefill_chunked(eng, emb, want_hidden):
    """``eng.prefill`` of ``emb`` on the selected slot, ``max_rows`` (what the engine was sized for) rows per call."""
    step = int(eng.max_rows)
    parts = [eng.prefill(emb[i:i + step], want_hidden=want_hidden) for i in range(0, emb.shape[0], step)]
    return torch.cat([p.clone() for p in parts]) if want_hidden and len(parts) > 1 else parts[0]


def knob_decode_weights(dtype):
    """What ``decode_weights=None`` means for an engine of ``dtype``: the tuning knobs ``llama_decode_w8`` / ``llama_decode_mx4``
    are a default for the engines that can take the option; fp32 (gate mode) engines stay as they are.  Both knobs set is an
    error."""
    w8, mx4 = _lib.get_tuning("llama_decode_w8", 0), _lib.get_tuning("llama_decode_mx4", 0)
    if dtype not in (torch.bfloat16, torch.float16):
        return None
    if w8 and mx4:
        raise ValueError("the tuning knobs llama_decode_w8 and llama_decode_mx4 are both set: fp8 and MXFP4 decode weights "
                         "exclude each other (clear one, or pass decode_weights=)")
    return "fp8" if w8 else "mxfp4" if mx4 else None


class LlamaEngine:
    def __init__(self, state_dict, *, hidden, n_heads, n_layers, inter, vocab, dtype=torch.bfloat16, device="cuda:0",
                 rms_eps=1e-5, max_pos=4096, cache_cap=2048, max_new=512, max_prefill_rows=1024, img_ids=(),
                 eos_id=2, lora_scaling=2.0, n_seq=1, decode_weights=None, kv_cache=None, speculate=None):
        """``speculate``: rows (2..8) of a prompt-lookup speculative step of ``generate`` (``set_speculation``); None = the
        ``llama_spec_rows`` tuning knob decides (default 0 = off), 0 = off whatever the knob says.
        ``decode_weights``: None = the ``llama_decode_w8`` / ``llama_decode_mx4`` tuning knobs decide (default off),
        "fp8" = decode tokens stream e4m3 copies of the five projections (``enable_decode_fp8``), "mxfp4" = MXFP4 copies
        (``enable_decode_mxfp4``), "16bit" = off whatever the knobs say.
        ``kv_cache``: the same three values for the e4m3 shadow of the KV cache that decode attention reads
        (``enable_kv_fp8``; knob ``llama_kv8``, default off)."""
        self.n_seq = int(n_seq)
        self.device = torch.device(device)
        self.dtype = dtype
        self.hidden, self.n_heads, self.n_layers, self.inter, self.vocab = hidden, n_heads, n_layers, inter, vocab
        self.hd = hidden // n_heads
        self.cache_cap, self.max_new, self.max_rows = cache_cap, max_new, max_prefill_rows
        self.img_ids = [int(i) for i in img_ids]
        self.eos_id = eos_id
        sd = state_dict
        dev = self.device
        self._keep = []  # tensors the engine points into
        self._proj = []  # per layer (wqkv, wo, wgu, wdown): what enable_decode_fp8 quantises

        def own(t):
            t = t.to(device=dev, dtype=dtype).contiguous()
            self._keep.append(t)
            return t

        self.embed = own(sd["model.embed_tokens.weight"])
        self.lm_head = own(sd["lm_head.weight"])
        self.final_norm = own(sd["model.norm.weight"])
        cos, sin = rope_tables(self.hd, max_pos, dtype)
        self.rope_cos, self.rope_sin = own(cos), own(sin)
        layers = (_lib.LlamaLayerWeights * n_layers)()
        for l in range(n_layers):
            pfx = "model.layers.%d." % l
            q, k, v, o = (_merged(sd, pfx + "self_attn." + n, dtype, dev, lora_scaling) for n in ATTN_PROJ)
            g, u, d = (_merged(sd, pfx + "mlp." + n, dtype, dev, lora_scaling) for n in MLP_PROJ)
            wqkv = torch.cat([q, k, v], dim=0).contiguous()
            wgu = torch.cat([g, u], dim=0).contiguous()
            ln1 = own(sd[pfx + "input_layernorm.weight"])
            ln2 = own(sd[pfx + "post_attention_layernorm.weight"])
            self._keep += [wqkv, o, wgu, d]
            self._proj.append((wqkv, o, wgu, d))
            layers[l] = _lib.LlamaLayerWeights(wqkv.data_ptr(), o.data_ptr(), wgu.data_ptr(), d.data_ptr(),
                                               ln1.data_ptr(), ln2.data_ptr())
            del q, k, v, g, u
        self._layers = layers
        self._init_engine(max_pos, rms_eps)
        self._init_decode_weights(decode_weights)
        self._init_kv_cache(kv_cache)
        self._init_speculation(speculate)

    @classmethod
    def from_prebuilt(cls, *, embed, lm_head, final_norm, layers, hidden, n_heads, n_layers, inter, vocab,
                      dtype=torch.bfloat16, device="cuda:0", rms_eps=1e-5, max_pos=4096, cache_cap=2048, max_new=512,
                      max_prefill_rows=1024, img_ids=(), eos_id=2, n_seq=1, decode_weights=None, kv_cache=None, speculate=None):
        """Engine over already merged/concatenated device tensors: ``layers`` is a list of
        ``(wqkv, wo, wgu, wdown, ln1, ln2)`` (used by the synthetic-weight benchmark, which
        creates the 13.5 GB of weights directly on the GPU)."""
        self = cls.__new__(cls)
        self.n_seq = int(n_seq)
        self.device = torch.device(device)
        self.dtype = dtype
        self.hidden, self.n_heads, self.n_layers, self.inter, self.vocab = hidden, n_heads, n_layers, inter, vocab
        self.hd = hidden // n_heads
        self.cache_cap, self.max_new, self.max_rows = cache_cap, max_new, max_prefill_rows
        self.img_ids = [int(i) for i in img_ids]
        self.eos_id = eos_id
        self.embed, self.lm_head, self.final_norm = embed, lm_head, final_norm
        cos, sin = rope_tables(self.hd, max_pos, dtype)
        self.rope_cos, self.rope_sin = cos.to(self.device), sin.to(self.device)
        self._keep = [embed, lm_head, final_norm, self.rope_cos, self.rope_sin, layers]
        self._proj = [tuple(t[:4]) for t in layers]
        arr = (_lib.LlamaLayerWeights * n_layers)()
        for l, t in enumerate(layers):
            arr[l] = _lib.LlamaLayerWeights(*[x.data_ptr() for x in t])
        self._layers = arr
        self._init_engine(max_pos, rms_eps)
        self._init_decode_weights(decode_weights)
        self._init_kv_cache(kv_cache)
        self._init_speculation(speculate)
        return self

    def _init_engine(self, max_pos, rms_eps):
        cfg = _lib.LlamaConfig(self.hidden, self.n_heads, self.n_layers, self.inter, self.vocab, max_pos, rms_eps,
                               ops.dt(self.dtype), self.cache_cap, self.max_new, len(self.img_ids), self.eos_id,
                               self.n_seq)
        self._cfg = cfg
        w = _lib.LlamaWeights(self.embed.data_ptr(), self.lm_head.data_ptr(), self.final_norm.data_ptr(),
                              self.rope_cos.data_ptr(), self.rope_sin.data_ptr(), self._layers)
        nbytes = lib().ss_llama_workspace_bytes(C.byref(cfg), self.max_rows)
        self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        ids = (C.c_int32 * max(1, len(self.img_ids)))(*self.img_ids)
        h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(lib().ss_llama_create(C.byref(cfg), C.byref(w), self._ws.data_ptr(), nbytes, self.max_rows, ids,
                                        C.byref(h)), "ss_llama_create")
        self._h = h
        self._views = {}
        self._cur = 0
        self._capture = None       # (maps, row0, head) while attention-map capture is on
        self._w8 = None            # tensors of the fp8 decode planes while the option is on
        self.decode_weights = None
        self._kv8 = None           # the four shadow planes (k_codes, v_codes, k_scale, v_scale) while kv_cache="fp8" is on
        self.kv_cache = None
        self._rules_slots = set()  # slots whose history rules are on (set_logits_rules)
        self._lp = None            # the result tensors of set_logprobs (model, policy, top ids, top values) while any slot records
        self._lp_slots = {}        # slot -> top_n of the slots that record
        self.last_logprobs = None  # what the image-block generate methods assembled for their last call
        self._spec = None          # (workspace, given-draft tensor or None) while speculation is on
        self.speculate = 0         # rows of a speculative step, 0 = off

    def __del__(self):
        h = getattr(self, "_h", None)
        if h:
            lib().ss_llama_destroy(h)
            self._h = None

    # ---- zero-copy views into the engine workspace -------------------------------------------
    def select(self, seq):
        """Address sequence slot ``seq`` (0 <= seq < n_seq) with the single-sequence methods
        below (views, lengths, prefill, generate, kv_gather).  Returns self."""
        check(lib().ss_llama_select(self._h, int(seq)), "ss_llama_select")
        self._cur = int(seq)
        return self

    def _buf(self, which, shape, dtype):
        key = (self._cur, which, tuple(shape), dtype)
        if key not in self._views:
            ptr = lib().ss_llama_buffer(self._h, which)
            base = self._ws.data_ptr()
            off = ptr - base
            n = 1
            for s in shape:
                n *= s
            esz = torch.empty(0, dtype=dtype).element_size()
            self._views[key] = self._ws[off:off + n * esz].view(dtype).view(*shape)
        return self._views[key]

    @property
    def k_cache(self):
        return self._buf(0, (self.n_layers, self.n_heads, self.cache_cap, self.hd), self.dtype)

    @property
    def v_cache(self):
        return self._buf(1, (self.n_layers, self.n_heads, self.cache_cap, self.hd), self.dtype)

    @property
    def gen_ids(self):
        return self._buf(2, (self.max_new,), torch.int32)

    @property
    def hidden_rows(self):
        return self._buf(3, (self.max_new, self.hidden), self.dtype)

    @property
    def logits(self):
        return self._buf(4, (self.vocab,), self.dtype)

    @property
    def state(self):
        return self._buf(5, (8,), torch.int32)

    @property
    def history(self):
        """int32 ``[cache_cap + max_new]`` view of the selected slot's token history (``set_history``); its length is the
        engine's"""
        return self._buf(6, (self.cache_cap + self.max_new,), torch.int32)

    @property
    def history_bitmap(self):
        """int32 ``[ceil(vocab / 32)]`` view of the rule-1 bitmap of the selected slot's history (one bit per id)"""
        return self._buf(7, ((self.vocab + 31) // 32,), torch.int32)

    # ---- lengths / cache management --------------------------------------------------------------
    def lengths(self):
        kv, pos = C.c_int64(), C.c_int64()
        check(lib().ss_llama_get_lengths(self._h, C.byref(kv), C.byref(pos)), "ss_llama_get_lengths")
        return kv.value, pos.value

    def set_lengths(self, kv_len, pos):
        check(lib().ss_llama_set_lengths(self._h, kv_len, pos, ops.stream()), "ss_llama_set_lengths")

    def reset(self):
        self.set_lengths(0, 0)

    def past_key_values(self, length=None):
        """Reference-layout views of the live cache (modeling_llama_xformer.py:239-242)."""
        n = self.lengths()[0] if length is None else length
        k, v = self.k_cache, self.v_cache
        return tuple((k[l, :, :n].unsqueeze(0), v[l, :, :n].unsqueeze(0)) for l in range(self.n_layers))

    def load_past_key_values(self, past, pos=None):
        """Copy an external reference-layout cache into the slab (no-op for our own views)."""
        n = past[0][0].shape[2]
        wrote = False
        for l, (k, v) in enumerate(past):
            dk, dv = self.k_cache[l, :, :n], self.v_cache[l, :, :n]
            if k.data_ptr() != dk.data_ptr():
                dk.copy_(k[0])
                wrote = True
            if v.data_ptr() != dv.data_ptr():
                dv.copy_(v[0])
                wrote = True
        if wrote:       # rows written through the views: their fp8 shadow rows (kv_cache="fp8") are stale
            self.kv_invalidate(0)
        self.set_lengths(n, n if pos is None else pos)

    def kv_gather(self, keep_idx):
        idx = torch.as_tensor(keep_idx, dtype=torch.int32, device=self.device).contiguous()
        check(lib().ss_llama_kv_gather(self._h, idx.data_ptr(), idx.numel(), ops.stream()), "ss_llama_kv_gather")

    def fork(self, src=None, dsts=None):
        """Put every slot of ``dsts`` (None: every other slot) in the state slot ``src`` (None: the selected slot) is in, on
        the device (ss_llama_fork; include/seedstory_hip.h): its cache rows below the cache length, last logits, lengths, token
        history and, with ``kv_cache="fp8"``, the shadow below its watermark — each packet read once and written to all
        destinations, asynchronously on the current stream.  ``generate`` / ``generate_batch`` / ``prefill`` on a destination
        then behave as on ``src``; sampling and rule parameters, recording and the result rings stay the slot's own.  The
        selected slot is unchanged.  Returns the destination list.  A bad slot list raises ``SSError`` and changes nothing."""
        src = self._cur if src is None else int(src)
        dsts = [b for b in range(self.n_seq) if b != src] if dsts is None else [int(b) for b in dsts]
        for b in [src] + dsts:
            if not -2 ** 31 <= b < 2 ** 31:
                raise _lib.SSError("fork: slot %d is no int32" % b)
        arr = (C.c_int32 * max(1, len(dsts)))(*dsts)
        check(lib().ss_llama_fork(self._h, src, arr, len(dsts), ops.stream()), "ss_llama_fork")
        return dsts

    # ---- attention maps (the reference's config.output_attentions) --------------------------------------
    def attn_capture_on(self, rows, cols, head=0, row0=None):
        """Start recording head ``head``'s attention map of every layer (pre-softmax scores + mask in the model dtype, as the
        reference's ``output_attentions`` returns them; include/seedstory_hip.h).  Allocates and returns
        ``[n_layers, rows, cols]`` filled with NaN: row r belongs to the query whose key sits at cache index ``row0 + r``
        (default: the current cache length), so ``prefill`` / ``generate`` / ``generate_img_block`` of the selected slot fill
        one row per fed token, real up to that call's key count and NaN beyond — the reference's merged map.  The lock-step
        batch entry points raise while capture is on."""
        if row0 is None:
            row0 = self.lengths()[0]
        maps = torch.full((self.n_layers, int(rows), int(cols)), float("nan"), dtype=self.dtype, device=self.device)
        self._set_capture(maps, int(row0), int(head), 0)
        self._capture = (maps, int(row0), int(head))
        return maps

    def attn_capture_off(self):
        if self._capture is not None:
            self._capture = None
            check(lib().ss_llama_set_attn_capture(self._h, None, 0, 0, 0, 0, 0), "ss_llama_set_attn_capture")

    @contextlib.contextmanager
    def attn_capture(self, rows, cols, head=0):
        """``with eng.attn_capture(rows, cols) as maps: ...`` — ``attn_capture_on`` / ``attn_capture_off`` as a context."""
        maps = self.attn_capture_on(rows, cols, head)
        try:
            yield maps
        finally:
            self.attn_capture_off()

    def _set_capture(self, maps, row0, head, row_calls):
        torch.cuda.current_stream(self.device).synchronize()       # the NaN fill precedes the engine's (blocking) descriptor copy
        check(lib().ss_llama_set_attn_capture(self._h, maps.data_ptr(), maps.shape[1], maps.shape[2], row0, head, row_calls),
              "ss_llama_set_attn_capture")

    def _refuse_capture(self, what):
        if self._capture is not None:
            raise _lib.SSError("%s: attention capture is a single-sequence tool (use the single-sequence methods on the "
                               "selected slot)" % what)

    # ---- fp8 (e4m3) weight-only decode -------------------------------------------------------------------
    def _init_decode_weights(self, decode_weights):
        if decode_weights is None:
            decode_weights = knob_decode_weights(self.dtype)
        if decode_weights not in (None, "16bit", "fp8", "mxfp4"):
            raise ValueError("decode_weights must be None, '16bit', 'fp8' or 'mxfp4', not %r" % (decode_weights,))
        if decode_weights == "fp8":
            self.enable_decode_fp8()
        elif decode_weights == "mxfp4":
            self.enable_decode_mxfp4()

    def enable_decode_fp8(self):
        """Quantise the engine's own merged weights on the device (one e4m3 scale per output row, ``amax / 448``) and
        switch the decode projections to them: ``generate`` / ``generate_batch`` / ``profile_decode`` then stream half the
        weight bytes per token.  Prefill, the image-token block and the one-row lm_head at the end of a prefill keep the
        16-bit weights, so those stay resident: the option COSTS memory, one byte per projection weight on top (about 6.7 GB
        for LLaMA-7B).  Off by default: what e4m3 weights do to stories on a real checkpoint has not been measured."""
        layers = [tuple(ops.quantize_weight_rows_fp8(w) for w in lw) for lw in self._proj]
        self.set_decode_fp8(layers, ops.quantize_weight_rows_fp8(self.lm_head))

    def set_decode_fp8(self, layers, lm_head):
        """Caller-supplied planes: ``layers[l]`` = four ``(q uint8 [N, K], scale fp32 [N])`` pairs for wqkv, wo, wgu
        (= [gate; up]) and wdown in the engine's layouts, ``lm_head`` one such pair.  ``layers=None`` switches the option off.
        Raises ``SSError`` on an fp32 engine or a projection shape the fp8 kernel does not take."""
        if layers is None:
            return self.disable_decode_fp8()
        shapes = ((3 * self.hidden, self.hidden), (self.hidden, self.hidden), (2 * self.inter, self.hidden), (self.hidden, self.inter))
        if len(layers) != self.n_layers:
            raise _lib.SSError("set_decode_fp8: %d layers given, the engine has %d" % (len(layers), self.n_layers))
        keep = []

        def plane(pair, shape, what):
            q, s = pair
            if q.dtype != torch.uint8 or tuple(q.shape) != shape or s.numel() != shape[0]:
                raise _lib.SSError("set_decode_fp8: %s must be (uint8 %s, scale [%d])" % (what, list(shape), shape[0]))
            q = q.to(self.device).contiguous()
            s = s.to(device=self.device, dtype=torch.float32).contiguous()
            keep.extend((q, s))
            return q, s

        arr = (_lib.LlamaLayerW8 * self.n_layers)()
        for l, lw in enumerate(layers):
            qs = [plane(pr, sh, "layer %d projection %d" % (l, j)) for j, (pr, sh) in enumerate(zip(lw, shapes))]
            arr[l] = _lib.LlamaLayerW8(*([q.data_ptr() for q, _ in qs] + [s.data_ptr() for _, s in qs]))
        ql, sl = plane(lm_head, (self.vocab, self.hidden), "lm_head")
        torch.cuda.current_stream(self.device).synchronize()
        check(lib().ss_llama_set_decode_w8(self._h, arr, ql.data_ptr(), sl.data_ptr()), "ss_llama_set_decode_w8")
        self._w8 = keep            # (the engine dropped the MXFP4 planes, if any, with this call)
        self.decode_weights = "fp8"

    def disable_decode_fp8(self):
        torch.cuda.current_stream(self.device).synchronize()
        check(lib().ss_llama_set_decode_w8(self._h, None, None, None), "ss_llama_set_decode_w8")
        if self.decode_weights == "fp8":
            self._w8 = None
            self.decode_weights = None

    # ---- MXFP4 (e2m1 codes + e8m0 block scales) weight-only decode ----------------------------------------
    def enable_decode_mxfp4(self):
        """Quantise the engine's own merged weights on the device to OCP MXFP4 (``ops.quantize_weight_rows_mxfp4``: two
        e2m1 codes per byte, one power-of-two scale per 32 consecutive k) and switch the decode projections to them:
        ``generate`` / ``generate_batch`` / ``profile_decode`` then stream 0.53 bytes per weight.  Prefill, the image-token
        block and the one-row lm_head at the end of a prefill keep the 16-bit weights, so those stay resident: the option
        COSTS memory, about 3.5 GB on top for LLaMA-7B.  Excludes the fp8 option (the later call wins).  Off by default:
        what round-to-nearest MXFP4 weights do to stories on a real checkpoint has not been measured."""
        layers = [tuple(ops.quantize_weight_rows_mxfp4(w) for w in lw) for lw in self._proj]
        self.set_decode_mxfp4(layers, ops.quantize_weight_rows_mxfp4(self.lm_head))

    def set_decode_mxfp4(self, layers, lm_head):
        """Caller-supplied planes in the public layout (include/seedstory_hip.h, ss_gemv_mx4): ``layers[l]`` = four
        ``(codes uint8 [N, K / 2], scales uint8 [N, K / 32])`` pairs for wqkv, wo, wgu (= [gate; up]) and wdown in the
        engine's layouts, ``lm_head`` one such pair.  ``layers=None`` switches the option off.  Raises ``SSError`` on an fp32
        engine or a projection shape the MXFP4 kernel does not take."""
        if layers is None:
            return self.disable_decode_mxfp4()
        shapes = ((3 * self.hidden, self.hidden), (self.hidden, self.hidden), (2 * self.inter, self.hidden), (self.hidden, self.inter))
        if len(layers) != self.n_layers:
            raise _lib.SSError("set_decode_mxfp4: %d layers given, the engine has %d" % (len(layers), self.n_layers))
        keep = []

        def plane(pair, shape, what):
            q, s = pair
            N, K = shape
            if (q.dtype != torch.uint8 or s.dtype != torch.uint8 or K % 32 or tuple(q.shape) != (N, K // 2)
                    or tuple(s.shape) != (N, K // 32)):
                raise _lib.SSError("set_decode_mxfp4: %s must be (uint8 codes [%d, %d / 2], uint8 scales [%d, %d / 32])"
                                   % (what, N, K, N, K))
            q = q.to(self.device).contiguous()
            s = s.to(self.device).contiguous()
            keep.extend((q, s))
            return q, s

        arr = (_lib.LlamaLayerMx4 * self.n_layers)()
        for l, lw in enumerate(layers):
            qs = [plane(pr, sh, "layer %d projection %d" % (l, j)) for j, (pr, sh) in enumerate(zip(lw, shapes))]
            arr[l] = _lib.LlamaLayerMx4(*([q.data_ptr() for q, _ in qs] + [s.data_ptr() for _, s in qs]))
        ql, sl = plane(lm_head, (self.vocab, self.hidden), "lm_head")
        torch.cuda.current_stream(self.device).synchronize()
        check(lib().ss_llama_set_decode_mx4(self._h, arr, ql.data_ptr(), sl.data_ptr()), "ss_llama_set_decode_mx4")
        self._w8 = keep            # (the engine dropped the fp8 planes, if any, with this call)
        self.decode_weights = "mxfp4"

    def disable_decode_mxfp4(self):
        torch.cuda.current_stream(self.device).synchronize()
        check(lib().ss_llama_set_decode_mx4(self._h, None, None, None), "ss_llama_set_decode_mx4")
        if self.decode_weights == "mxfp4":
            self._w8 = None
            self.decode_weights = None

    # ---- fp8 (e4m3) shadow of the KV cache for decode attention --------------------------------------------------
    def _init_kv_cache(self, kv_cache):
        if kv_cache is None:            # the knob, like llama_decode_w8, is ignored by fp32 (gate mode) engines
            on = _lib.get_tuning("llama_kv8", 0) and self.dtype in (torch.bfloat16, torch.float16)
            kv_cache = "fp8" if on else None
        if kv_cache not in (None, "16bit", "fp8"):
            raise ValueError("kv_cache must be None, '16bit' or 'fp8', not %r" % (kv_cache,))
        if kv_cache == "fp8":
            self.enable_kv_fp8()

    def enable_kv_fp8(self):
        """Allocate the e4m3 shadow of the KV cache (codes + one fp32 power-of-two scale per slot, layer, head and position;
        the definition is in include/seedstory_hip.h) and switch decode attention to it: ``generate`` / ``generate_batch`` /
        ``profile_decode`` then read half the key / value bytes per token.  The 16-bit cache stays the truth — prefill, the
        image-token block, ``past_key_values``, ``kv_gather`` and attention-map capture keep using it — so the option COSTS
        memory: ``hd + 4`` bytes per cached row on top (0.27 MB per position per slot for LLaMA-7B).  The engine quantises
        rows it has not seen at the start of each decode call; write cache rows through ``k_cache`` / ``v_cache`` yourself and
        you owe it a ``kv_invalidate``.  Off by default: what an e4m3 cache does to stories on a real checkpoint has not been
        measured.  Raises ``SSError`` on an fp32 engine or a head dim the kernel does not take."""
        nc, ns = C.c_size_t(), C.c_size_t()
        check(lib().ss_llama_kv8_bytes(C.byref(self._cfg), C.byref(nc), C.byref(ns)), "ss_llama_kv8_bytes")
        shape = (self.n_seq, self.n_layers, self.n_heads, self.cache_cap)
        planes = [torch.zeros(shape + (self.hd,), dtype=torch.uint8, device=self.device) for _ in range(2)]
        planes += [torch.ones(shape, dtype=torch.float32, device=self.device) for _ in range(2)]
        assert planes[0].numel() == nc.value and planes[2].numel() * 4 == ns.value
        torch.cuda.current_stream(self.device).synchronize()
        check(lib().ss_llama_set_kv8(self._h, *[t.data_ptr() for t in planes]), "ss_llama_set_kv8")
        self._kv8 = planes
        self.kv_cache = "fp8"

    def disable_kv_fp8(self):
        torch.cuda.current_stream(self.device).synchronize()
        check(lib().ss_llama_set_kv8(self._h, None, None, None, None), "ss_llama_set_kv8")
        self._kv8 = None
        self.kv_cache = None

    def kv_invalidate(self, from_row=0):
        """Tell the engine that 16-bit cache rows of the selected slot from ``from_row`` on were written behind its back
        (through the ``k_cache`` / ``v_cache`` views): their shadow rows are rebuilt by the next decode call.  A no-op while
        ``kv_cache`` is off."""
        check(lib().ss_llama_kv8_invalidate(self._h, int(from_row)), "ss_llama_kv8_invalidate")

    def _kv8_plane(self, i):
        if self._kv8 is None:
            raise _lib.SSError("the fp8 KV shadow is off (kv_cache='fp8' / enable_kv_fp8)")
        return self._kv8[i][self._cur]

    @property
    def k_codes(self):
        """uint8 ``[n_layers, n_heads, cache_cap, hd]`` view of the selected slot's key codes (``v_codes``, and the fp32
        ``k_scale`` / ``v_scale`` ``[n_layers, n_heads, cache_cap]``, likewise); rows the engine has not synced yet are stale."""
        return self._kv8_plane(0)

    @property
    def v_codes(self):
        return self._kv8_plane(1)

    @property
    def k_scale(self):
        return self._kv8_plane(2)

    @property
    def v_scale(self):
        return self._kv8_plane(3)

    # ---- prompt-lookup speculative decoding ------------------------------------------------------------------------
    def _init_speculation(self, speculate):
        if speculate is None:
            speculate = _lib.get_tuning("llama_spec_rows", 0)
        if speculate:
            self.set_speculation(int(speculate))

    def set_speculation(self, rows, max_ngram=2, draft_ids=None):
        """Speculative steps in ``generate`` (and so in the free tokens of ``generate_img_block``): each decode launch
        forwards ``rows`` (2..8) rows of the selected slot in one sweep of the weights — the token greedy chose plus drafted
        successors — and the next one keeps the prefix the model agrees with, so a launch emits 1..``rows`` tokens and the ids
        are greedy's (away from near-ties of the top two logits).  Drafts: prompt lookup with n-grams of up to
        ``max_ngram`` (1..8) tokens in the slot's history — hand the prompt ids over with ``set_history``; generated tokens join
        it on the device — or, with ``draft_ids`` (a list or int32 tensor indexed by generated position), the caller's own.
        ``generate_batch``, ``fork``, best-of-n and ``beam_search`` run as they always do.  ``generate`` raises ``SSError``
        before anything is launched when the slot also has sampling, logits rules, log-probability recording, the fp8 KV shadow
        or attention-map capture on.  Off by default: what prompt lookup accepts on real captions has not been measured."""
        rows, max_ngram = int(rows), int(max_ngram)
        if not 2 <= rows <= _lib.SPEC_MAX_ROWS:
            raise ValueError("set_speculation: rows %d outside [2, %d]" % (rows, _lib.SPEC_MAX_ROWS))
        if not 1 <= max_ngram <= 8:
            raise ValueError("set_speculation: max_ngram %d outside [1, 8]" % max_ngram)
        given = None
        if draft_ids is not None:
            given = torch.as_tensor(draft_ids, dtype=torch.int32).reshape(-1).to(self.device).contiguous()
            if given.numel() == 0:
                given = torch.zeros(1, dtype=torch.int32, device=self.device)[:0]
        nbytes = C.c_size_t()
        check(lib().ss_llama_spec_bytes(C.byref(self._cfg), rows, C.byref(nbytes)), "ss_llama_spec_bytes")
        ws = torch.zeros(nbytes.value, dtype=torch.uint8, device=self.device)
        sp = _lib.SpecParams(rows, max_ngram, _lib.SPEC_LOOKUP if given is None else _lib.SPEC_GIVEN,
                             0 if given is None else given.numel(),
                             None if given is None else (given.data_ptr() or ws.data_ptr()))
        torch.cuda.current_stream(self.device).synchronize()
        check(lib().ss_llama_set_speculation(self._h, C.byref(sp), ws.data_ptr()), "ss_llama_set_speculation")
        self._spec = (ws, given)
        self.speculate = rows

    def clear_speculation(self):
        """Speculation off (the default): ``generate`` launches the plain decode token again."""
        torch.cuda.current_stream(self.device).synchronize()
        check(lib().ss_llama_set_speculation(self._h, None, None), "ss_llama_set_speculation")
        self._spec = None
        self.speculate = 0

    def spec_stats(self, slot=None):
        """Counters of the last ``generate`` call with speculation on: ``{"steps", "drafted", "accepted", "emitted"}`` —
        speculative forwards, rows drafted, drafts accepted, tokens emitted."""
        out = (C.c_int64 * 4)()
        check(lib().ss_llama_spec_stats(self._h, -1 if slot is None else int(slot), out), "ss_llama_spec_stats")
        return dict(zip(("steps", "drafted", "accepted", "emitted"), (int(v) for v in out)))

    # ---- sampling ------------------------------------------------------------------------------------------------
    def set_sampling(self, temperature=1.0, top_k=0, top_p=1.0, seed=0, slot=None):
        """Sampling instead of the arg max in ``generate`` / ``generate_batch`` (and the image-block variants), for ``slot``
        or, with None, every slot: image-token processor -> temperature -> top-k (0 = off) -> top-p -> one Philox4x32-10 draw
        with key ``seed`` and counter (draw, slot) — slots given one seed still diverge.  The definition and its two
        deviations from Hugging Face's warpers (the image-token successor is certain; top-p keeps tied values together) are
        in include/seedstory_hip.h.  Runs on the device inside the decode token (eager or captured; a graph of its own, cached
        apart from the greedy one); the parameters and the per-slot draw counter live in device memory, so another
        temperature or seed does not re-capture.  Forced tokens and the certain successor take no draw.  The counter
        persists across calls and is reset by this method and ``set_greedy``.  Bad parameters raise ``SSError``."""
        sp = ops.sampling_struct(temperature, top_k, top_p, seed)
        self._set_sampling(slot, C.byref(sp))

    def set_greedy(self, slot=None):
        """Back to the arg max (the default) for ``slot`` or, with None, every slot."""
        self._set_sampling(slot, None)

    def _set_sampling(self, slot, sp):
        torch.cuda.current_stream(self.device).synchronize()
        check(lib().ss_llama_set_sampling(self._h, -1 if slot is None else int(slot), sp), "ss_llama_set_sampling")

    # ---- history rules -------------------------------------------------------------------------------------------
    def set_logits_rules(self, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, spare_img_ids=False, slot=None):
        """Hugging Face's ``repetition_penalty`` -> ``no_repeat_ngram_size`` -> ``min_new_tokens`` on the logits of every decode
        token of ``generate`` / ``generate_batch`` (and the image-block variants), in front of the image-token processor and
        the arg max or sampler, for ``slot`` or, with None, every slot.  The definition is in include/seedstory_hip.h
        (``ss_process_logits``): the penalty is bit-equal to ``RepetitionPenaltyLogitsProcessor``; ``spare_img_ids=True`` is
        the one deviation (the ids of ``img_ids`` are exempt from the penalty).  The rules see the slot's token history: hand
        the prompt ids over with ``set_history``; every token the loop produces, and every image-block token, is appended
        by the engine while the slot's rules are on.  One more kernel per token, eager or captured (a graph of its own); the
        rules, the history and its bitmap live in device memory, so other values do not re-capture.  EOS for
        ``min_new_tokens`` is the engine's ``eos_id``.  Bad values raise ``SSError``."""
        rp = ops.logits_rules_struct(repetition_penalty, no_repeat_ngram_size, min_new_tokens, spare_img_ids)
        self._set_logits_rules(slot, C.byref(rp))
        self._rules_slots |= set(range(self.n_seq)) if slot is None else {int(slot)}

    def clear_logits_rules(self, slot=None):
        """Rules off (the default) for ``slot`` or, with None, every slot: the decode token is what it was without them."""
        self._set_logits_rules(slot, None)
        self._rules_slots -= set(range(self.n_seq)) if slot is None else {int(slot)}

    def _set_logits_rules(self, slot, rp):
        torch.cuda.current_stream(self.device).synchronize()
        check(lib().ss_llama_set_logits_rules(self._h, -1 if slot is None else int(slot), rp), "ss_llama_set_logits_rules")

    def set_history(self, ids, slot=None, append=False):
        """The token history the rules of ``slot`` (None: the selected slot) see: ``ids`` = the whole running ``input_ids``
        as Hugging Face's processors would get them; its length becomes ``prompt_len`` for ``min_new_tokens``.
        ``append=True`` adds ``ids`` behind the history instead (tokens fed outside the decode loop).  Ids outside
        [0, vocab) raise ``SSError``."""
        ids = [int(t) for t in (ids.reshape(-1).tolist() if isinstance(ids, torch.Tensor) else ids)]
        for t in ids:
            if not -2 ** 31 <= t < 2 ** 31:
                raise _lib.SSError("set_history: id %d is no int32" % t)
        arr = (C.c_int32 * max(1, len(ids)))(*ids)
        torch.cuda.current_stream(self.device).synchronize()
        check(lib().ss_llama_set_history(self._h, -1 if slot is None else int(slot), arr, len(ids), 1 if append else 0),
              "ss_llama_set_history")

    def _history_append(self, slot, toks):
        """image-block tokens of ``slot`` join its history (they were fed as one batched forward, outside the decode loop)"""
        # getattr: tests bind the block methods onto stand-in engines.  With speculation on the history feeds the drafts.
        if toks and (slot in getattr(self, "_rules_slots", ()) or getattr(self, "_spec", None) is not None):
            self.set_history(toks, slot=slot, append=True)

    # ---- token log-probabilities -----------------------------------------------------------------------------------
    def set_logprobs(self, on=True, top_n=0, slot=None):
        """Record, for every token the decode loop produces on ``slot`` (None: every slot), how likely it was: ``model_logprob``
        (the model's log-softmax of the untouched lm_head row), ``logprob`` (the log of the probability with which the policy
        picked it: greedy = log-softmax of the edited row, sampling = the sampler's own ``log(w / Z_P)``, 0.0 for a forced
        token and for the certain image-token successor) and the ``top_n`` (at most 8) most likely tokens of the model with
        their log-probabilities.  The definition is in include/seedstory_hip.h (``ss_token_logprobs``).  Runs on the device
        inside the decode token (eager or captured; a graph of its own, cached apart from the others): two more small
        kernels, nothing goes back to the host, and tokens, hidden rows and the draw counter stay bit-equal.  The engine owns
        the result tensors (``logprobs(n)``); entry i lines up with ``gen_ids[i]`` of the last ``generate`` call.
        ``on=False`` switches it off (the default).  Bad values raise ``SSError``."""
        slots = list(range(self.n_seq)) if slot is None else [int(slot)]
        if not 0 <= slots[0] < self.n_seq:
            raise _lib.SSError("set_logprobs: sequence slot %d out of range (< %d)" % (slots[0], self.n_seq))
        if on and (int(top_n) != top_n or not -2 ** 31 <= int(top_n) < 2 ** 31):
            raise _lib.SSError("top_n must be an integer, not %r" % (top_n,))
        top_n = int(top_n) if on else 0
        torch.cuda.current_stream(self.device).synchronize()
        if not on:
            check(lib().ss_llama_set_logprobs(self._h, -1 if slot is None else int(slot), None, None, None, None, 0),
                  "ss_llama_set_logprobs")
            for b in slots:
                self._lp_slots.pop(b, None)
            if not self._lp_slots:
                self._lp = None
            return
        if self._lp is None:
            S, N = self.n_seq, self.max_new
            self._lp = (torch.zeros(S, N, dtype=torch.float32, device=self.device), torch.zeros(S, N, dtype=torch.float32, device=self.device),
                        torch.full((S, N, 8), -1, dtype=torch.int32, device=self.device),
                        torch.full((S, N, 8), float("-inf"), dtype=torch.float32, device=self.device))
            torch.cuda.current_stream(self.device).synchronize()
        m, q, ti, tl = self._lp
        for b in slots:     # (each slot's [max_new][top_n] block starts at its own [max_new][8] block of the tensors)
            check(lib().ss_llama_set_logprobs(self._h, b, m[b].data_ptr(), q[b].data_ptr(), ti[b].data_ptr() if top_n > 0 else None,
                                              tl[b].data_ptr() if top_n > 0 else None, top_n), "ss_llama_set_logprobs")
            self._lp_slots[b] = top_n

    def logprobs(self, n, slot=None):
        """Views of the first ``n`` recorded entries of ``slot`` (None: the selected slot): ``{"logprob", "model_logprob"``
        float32 [n], ``"top_ids"`` int32 [n, top_n], ``"top_logprobs"`` float32 [n, top_n]``}``.  The next ``generate`` call on
        the slot overwrites them."""
        b = self._cur if slot is None else int(slot)
        if b not in self._lp_slots:
            raise _lib.SSError("slot %d records no log-probabilities (set_logprobs)" % b)
        k, n = self._lp_slots[b], int(n)
        m, q, ti, tl = self._lp
        return {"logprob": q[b, :n], "model_logprob": m[b, :n],
                "top_ids": ti[b].view(-1)[:n * k].view(n, k), "top_logprobs": tl[b].view(-1)[:n * k].view(n, k)}

    def _lp_segment(self, slot, n):
        """a copy of the loop's first ``n`` entries of ``slot``, or None when the slot records nothing"""
        if slot not in getattr(self, "_lp_slots", {}):      # getattr: tests bind the block methods onto stand-in engines
            return None
        return {k: v.clone() for k, v in self.logprobs(n, slot).items()}

    def _lp_block(self, slot, logits, toks):
        """the entries of image-block tokens ``toks``: row i of ``logits`` (lm_head of the block's hidden rows) scores
        ``toks[i]``; the policy did not choose them, so their ``logprob`` is 0.0"""
        k = self._lp_slots[slot]
        r = ops.token_logprobs(logits, toks, top_n=k)
        lp, ti, tl = r if k > 0 else (r, torch.zeros(len(toks), 0, dtype=torch.int32, device=logits.device),
                                      torch.zeros(len(toks), 0, dtype=torch.float32, device=logits.device))
        return {"logprob": torch.zeros_like(lp), "model_logprob": lp, "top_ids": ti, "top_logprobs": tl}

    @staticmethod
    def _lp_join(parts):
        return {k: torch.cat([p[k] for p in parts]) for k in parts[0]} if parts else None

    # ---- forward paths ---------------------------------------------------------------------------------
    def _ensure_prefill_tiles(self, M):
        if M > 128:      # the four prefill projections of this row-count bucket (tile table: seedstory/tune.py)
            code, Hd, I = ops.dt(self.dtype), self.hidden, self.inter
            for n, k in ((3 * Hd, Hd), (Hd, Hd), (2 * I, Hd), (Hd, I)):
                tune.ensure_gemm(M, n, k, code, 0, self.device)

    def prefill(self, embeds, pos_ids=None, want_hidden=False):
        """embeds [M, hidden] rows appended after the cached prefix.  Returns the post-final-norm
        hidden rows [M, hidden] if want_hidden; the last row's logits land in ``self.logits``."""
        embeds = embeds.to(device=self.device, dtype=self.dtype).contiguous()
        M = embeds.shape[0]
        hid = torch.empty(M, self.hidden, dtype=self.dtype, device=self.device) if want_hidden else None
        pid = None if pos_ids is None else pos_ids.to(device=self.device, dtype=torch.int32).contiguous()
        self._ensure_prefill_tiles(M)
        check(lib().ss_llama_prefill(self._h, embeds.data_ptr(), M, ops.p(pid), ops.p(hid), ops.stream()),
              "ss_llama_prefill")
        return hid

    def prefill_batch(self, embeds, want_hidden=False):
        """``prefill`` for several sequence slots in ONE sweep of the weights (ss_llama_prefill_batch): ``embeds[b]`` =
        slot b's new rows [M_b, hidden] or None.  Returns the per-slot hidden rows (or None) — each slot's last row's
        logits land in that slot's logits buffer and its lengths advance by M_b."""
        self._refuse_capture("prefill_batch")
        S = self.n_seq
        assert len(embeds) == S
        rows = [0 if e is None else int(e.shape[0]) for e in embeds]
        live = [e.to(device=self.device, dtype=self.dtype) for e in embeds if e is not None and e.shape[0]]
        if not live:
            return [None] * S
        M = sum(rows)
        if M > self.max_rows:                      # engine sized for fewer stacked rows: slot by slot, max_rows at a time
            keep = self._cur
            out = [_prefill_chunked(self.select(b), e, want_hidden) if rows[b] else None for b, e in enumerate(embeds)]
            self.select(keep)
            return out
        stack = live[0].contiguous() if len(live) == 1 else torch.cat(live, dim=0)
        hid = torch.empty(M, self.hidden, dtype=self.dtype, device=self.device) if want_hidden else None
        self._ensure_prefill_tiles(M)
        arr = (C.c_int64 * S)(*rows)
        check(lib().ss_llama_prefill_batch(self._h, stack.data_ptr(), arr, ops.p(hid), ops.stream()), "ss_llama_prefill_batch")
        if not want_hidden:
            return [None] * S
        out, r0 = [], 0
        for b in range(S):
            out.append(hid[r0:r0 + rows[b]] if rows[b] else None)
            r0 += rows[b]
        return out

    def generate(self, n_steps, last_prompt_id, forced=None):
        """Decode from the current logits — greedy, or sampled after ``set_sampling``; ``forced`` tokens win over either.
        Returns the number of generated tokens."""
        forced = [] if forced is None else [int(t) for t in forced]
        arr = (C.c_int32 * max(1, len(forced)))(*forced)
        n = C.c_int64()
        check(lib().ss_llama_generate(self._h, n_steps, int(last_prompt_id), arr, len(forced), C.byref(n),
                                      ops.stream()), "ss_llama_generate")
        return n.value

    def generate_batch(self, n_steps, last_prompt_ids, forced=None, active=None):
        """Decode of all ``n_seq`` slots in lock-step (one sweep of the weights per token for the whole batch): greedy, or
        per slot sampled after ``set_sampling`` (mixed batches work).  ``last_prompt_ids[b]``, optional ``forced[b]`` token lists and
        ``active[b]`` flags are per slot; returns the per-slot generated-token counts."""
        self._refuse_capture("generate_batch")
        S = self.n_seq
        assert len(last_prompt_ids) == S
        forced = [[] for _ in range(S)] if forced is None else [[int(t) for t in (f or [])] for f in forced]
        ld = max(1, max(len(f) for f in forced))
        flat = (C.c_int32 * (S * ld))()
        for b, f in enumerate(forced):
            for i, t in enumerate(f):
                flat[b * ld + i] = t
        nf = (C.c_int64 * S)(*[len(f) for f in forced])
        last = (C.c_int32 * S)(*[int(t) for t in last_prompt_ids])
        act = None if active is None else (C.c_int32 * S)(*[1 if a else 0 for a in active])
        out = (C.c_int64 * S)()
        check(lib().ss_llama_generate_batch(self._h, n_steps, last, flat, ld, nf, act, out, ops.stream()),
              "ss_llama_generate_batch")
        return [int(v) for v in out]

    # ---- beam search --------------------------------------------------------------------------------------------
    _EARLY = {False: 0, True: 1, "never": 2}

    def _beam_ws(self, n):
        """the engine's beam-search workspace for ``n`` beams (kept: its address is part of the captured graph's key)"""
        ws = getattr(self, "_beam_bufs", None)
        if ws is None:
            ws = self._beam_bufs = {}
        if n not in ws:
            nbytes = lib().ss_llama_beam_bytes(C.byref(self._cfg), n)
            if nbytes == 0:
                raise _lib.SSError("beam_search: num_beams %d outside [1, 8]" % n)
            ws[n] = torch.zeros(nbytes, dtype=torch.uint8, device=self.device)
            torch.cuda.current_stream(self.device).synchronize()
        return ws[n]

    def beam_search(self, n_steps, last_prompt_id, num_beams, length_penalty=1.0, early_stopping=False):
        """Beam search from the current logits of slot 0, on the device inside the captured decode token
        (``ss_llama_beam_search``; the definition — Hugging Face's ``_beam_search`` on the log-softmax of the row after the
        history rules and the image-token processor, ties by ascending ``beam * vocab + token`` — is in
        include/seedstory_hip.h).  Slot 0 is forked to slots 1 .. ``num_beams`` - 1, which then carry the running hypotheses;
        stop ids are the engine's ``eos_id`` and the id of ``set_stop_id``.  Returns ``{"sequences": list of n id lists,
        "scores": float32 [n], "finished": bool [n]}``, the finished table best first (entries never filled: ``[]``, -inf,
        False).  Afterwards the slots hold the RUNNING hypotheses' caches: rewind (``set_lengths``) and feed the winner to go on
        from it.  Refused with ``SSError`` before anything changes: see the header."""
        n = int(num_beams)
        if early_stopping not in (False, True, "never"):
            raise _lib.SSError("early_stopping must be False, True or 'never', not %r" % (early_stopping,))
        if not -2 ** 31 <= n < 2 ** 31 or not -2 ** 63 <= int(n_steps) < 2 ** 63:
            raise _lib.SSError("beam_search: num_beams / n_steps out of the integer range")
        if not 1 <= n <= min(self.n_seq, _lib.BEAM_MAX):
            raise _lib.SSError("beam_search: num_beams %d outside [1, min(n_seq = %d, %d)]" % (n, self.n_seq, _lib.BEAM_MAX))
        ws = self._beam_ws(n)
        bp = _lib.BeamParams(n, float(length_penalty), self._EARLY[early_stopping])
        check(lib().ss_llama_beam_search(self._h, C.byref(bp), ws.data_ptr(), int(n_steps), int(last_prompt_id), ops.stream()),
              "ss_llama_beam_search")
        return self._beam_result(ws, n)

    def _beam_result(self, ws, n):
        host = ws.cpu()         # (the search has synchronised: the state is final)
        st = _lib.BeamState.from_buffer_copy(host[:C.sizeof(_lib.BeamState)].numpy().tobytes())
        off = lib().ss_llama_beam_seq_offset()
        seqs = host[off:off + 4 * n * self.max_new * 4].view(torch.int32).view(2, 2, n, self.max_new)  # running | finished
        fin = seqs[1, st.step & 1]
        flags = [bool(st.fin_flag[i]) for i in range(n)]
        self.last_beam_state = st
        return {"sequences": [fin[i, :st.fin_len[i]].tolist() if flags[i] else [] for i in range(n)],
                "scores": torch.tensor([st.fin_score[i] for i in range(n)], dtype=torch.float32),
                "finished": torch.tensor(flags, dtype=torch.bool)}

    def _beam_permute(self, parent, kv0, hist0=0):
        """test hook (``ss_llama_beam_permute``): one cache / history permutation of slots [0, len(parent)) by ``parent``"""
        n = len(parent)
        arr = (C.c_int32 * max(1, n))(*[int(b) for b in parent])
        check(lib().ss_llama_beam_permute(self._h, self._beam_ws(n).data_ptr(), arr, n, int(kv0), int(hist0), ops.stream()),
              "ss_llama_beam_permute")

    # ---- image-token block decode ---------------------------------------------------------------------------
    # After ``<img>`` the logits processor FORCES the next 65 tokens (``<img_00000>`` .. ``<img_00063>``, ``</img>``:
    # generation.py:19-31 sets their score to max + 10), so their forwards do not depend on one another's sampled
    # output: the decode loop stops at ``<img>`` (ss_llama_set_stop_id), the forced block is fed as ONE batched
    # continuation — the same layers, the same causal attention, the same hidden rows and KV entries, but the 13.2 GB
    # of weights are streamed once for 66 rows instead of 66 times — and the loop resumes from the block's last logits.
    # lm_head is still applied to every block row (the reference computes those logits; they cannot change a forced
    # token), so no arithmetic of the sequential loop is skipped.
    @staticmethod
    def img_block_enabled():
        """Default ON; ``SEEDSTORY_IMG_BLOCK=0`` or the ``img_block_decode`` tuning knob set to 0 restore the token-by-token loop."""
        import os
        return _lib.get_tuning("img_block_decode", 0 if os.environ.get("SEEDSTORY_IMG_BLOCK", "1") == "0" else 1) != 0

    def set_stop_id(self, token_id):
        check(lib().ss_llama_set_stop_id(self._h, int(token_id)), "ss_llama_set_stop_id")

    def _img_block_plan(self, remaining, forced):
        """(tokens the block contributes, rows to feed) for a slot whose loop has just produced ``<img>``."""
        blk = self.img_ids
        m = min(remaining, len(blk) - 1)                          # tokens the block contributes: blk[1 .. m]
        if forced[:m] != blk[1:m + 1][:len(forced[:m])]:
            raise _lib.SSError("forced tokens contradict the image-token schedule that follows <img>")
        rows = m + 1 if remaining > len(blk) - 1 else m            # </img> is fed only when generation goes on after it
        return m, rows

    def _img_block(self, remaining, forced):
        """The slot's decode loop has just produced ``<img>`` (not fed yet).  Feeds the forced block; returns
        (tokens appended, hidden rows [rows, H], id of the last token fed or None when the block ended the budget)."""
        blk = self.img_ids
        m, rows = self._img_block_plan(remaining, forced)
        ids = torch.tensor(blk[:rows], dtype=torch.int32, device=self.device)
        emb = ops.gather_rows(self.embed, ids)
        capture = getattr(self, "_capture", None)     # getattr: tests/test_host_cpu.py binds this method onto a stand-in engine
        if capture is not None:             # the reference feeds these rows one call each: every map row is a one-row call
            self._set_capture(*capture, 1)
        try:
            hb = _prefill_chunked(self, emb, True)
        finally:
            if capture is not None:
                self._set_capture(*capture, 0)
        if getattr(self, "_cur", 0) in getattr(self, "_lp_slots", {}):      # kept, whatever the knob says: row i scores blk[i + 1]
            self._blk_lp = LlamaEngine._lp_block(self, getattr(self, "_cur", 0), ops.gemm(hb, self.lm_head)[:m], blk[1:m + 1])
        elif _lib.get_tuning("img_block_logits", 1):
            ops.gemm(hb, self.lm_head)                             # the reference's per-position logits (unused: forced)
        return blk[1:m + 1], hb, (blk[rows - 1] if rows == m + 1 else None)

    def generate_img_block(self, n_steps, last_prompt_id, forced=None):
        """``generate`` with the forced image-token runs batched.  Returns (ids LongTensor [n] on the host side list,
        hidden rows [n - 1, hidden]) — the same tokens / rows the token-by-token loop yields."""
        if len(self.img_ids) < 3:
            n = self.generate(n_steps, last_prompt_id, forced)
            self.last_logprobs = LlamaEngine._lp_segment(self, getattr(self, "_cur", 0), n)
            return self.gen_ids[:n].tolist(), self.hidden_rows[:max(n - 1, 0)]
        boi = self.img_ids[0]
        forced = [] if forced is None else [int(t) for t in forced]
        ids, hid, rem, last = [], [], min(int(n_steps), 1 << 30), int(last_prompt_id)
        cur = getattr(self, "_cur", 0)
        lps = [] if cur in getattr(self, "_lp_slots", {}) else None        # per-token values of the whole call, segment by segment
        self.last_logprobs = None
        self.set_stop_id(boi)
        try:
            while rem > 0:
                n = self.generate(rem, last, forced)
                g = self.gen_ids[:n].tolist()
                ids += g
                hid.append(self.hidden_rows[:max(n - 1, 0)].clone())
                if lps is not None:
                    lps.append(LlamaEngine._lp_segment(self, cur, n))
                forced, rem = forced[n:], rem - n
                if n == 0 or g[-1] != boi or rem == 0:
                    break                                           # EOS, the token limit, or the budget ended at <img>
                toks, hb, last_fed = self._img_block(rem, forced)
                LlamaEngine._history_append(self, getattr(self, "_cur", 0), toks)
                if lps is not None:
                    lps.append(self._blk_lp)
                ids += toks
                hid.append(hb)
                forced, rem = forced[len(toks):], rem - len(toks)
                if last_fed is None:
                    break
                last = last_fed
        finally:
            self.set_stop_id(-1)
        if lps is not None:
            self.last_logprobs = LlamaEngine._lp_join(lps)
        return ids, torch.cat(hid)[:max(len(ids) - 1, 0)]

    def generate_batch_img_block(self, n_steps, last_prompt_ids, forced=None, active=None):
        """``generate_batch`` with the forced image-token runs batched, per slot.  Returns (ids per slot, hidden rows per
        slot).  Slots are independent: one may be inside its block while another still writes its caption.
        ``active[b]`` false (None: every slot takes part): slot b is never read, fed or written; its entries of the results
        are ``[]`` and ``None``."""
        S = self.n_seq
        on = [True] * S if active is None else [bool(a) for a in active]
        assert len(on) == S
        if len(self.img_ids) < 3:
            ns = self.generate_batch(n_steps, last_prompt_ids, forced) if active is None else \
                self.generate_batch(n_steps, last_prompt_ids, forced, on)
            self.last_logprobs = ([LlamaEngine._lp_segment(self, b, ns[b]) if on[b] else None for b in range(S)]
                                  if getattr(self, "_lp_slots", {}) else None)
            return ([self.select(b).gen_ids[:ns[b]].tolist() if on[b] else [] for b in range(S)],
                    [self.select(b).hidden_rows[:max(ns[b] - 1, 0)] if on[b] else None for b in range(S)])
        boi = self.img_ids[0]
        forced = [[] for _ in range(S)] if forced is None else [[int(t) for t in (f or [])] for f in forced]
        ids, hid = [[] for _ in range(S)], [[] for _ in range(S)]
        rem, last, active = [int(n_steps)] * S, [int(t) for t in last_prompt_ids], list(on)
        lp_slots = getattr(self, "_lp_slots", {})
        lps = [[] if b in lp_slots and on[b] else None for b in range(S)]
        self.last_logprobs = None
        self.set_stop_id(boi)
        try:
            blk = self.img_ids
            while any(active):
                n_call = min(rem[b] for b in range(S) if active[b])
                ns = self.generate_batch(n_call, last, forced, active)
                feed = [None] * S          # rows every slot feeds after this call: ONE stacked continuation (weights once)
                plan = {}
                for b in range(S):
                    if not active[b]:
                        continue
                    n = ns[b]
                    self.select(b)
                    g = self.gen_ids[:n].tolist()
                    ids[b] += g
                    hid[b].append(self.hidden_rows[:max(n - 1, 0)].clone())
                    if lps[b] is not None:
                        lps[b].append(LlamaEngine._lp_segment(self, b, n))
                    forced[b], rem[b] = forced[b][n:], rem[b] - n
                    if n == 0 or rem[b] == 0 or g[-1] == self.eos_id:
                        active[b] = False
                    elif g[-1] == boi:      # the forced image-token block of this slot
                        m, rows = self._img_block_plan(rem[b], forced[b])
                        feed[b] = torch.tensor(blk[:rows], dtype=torch.int32, device=self.device)
                        plan[b] = (m, rows)
                    else:       # stopped by this call's common limit: feed its last token, resume from fresh logits
                        feed[b] = torch.tensor([g[-1]], dtype=torch.int32, device=self.device)
                        plan[b] = None
                if plan:
                    hbs = self.prefill_batch([None if f is None else ops.gather_rows(self.embed, f) for f in feed],
                                             want_hidden=True)
                    blocks = [b for b, v in plan.items() if v is not None]
                    if blocks and (_lib.get_tuning("img_block_logits", 1) or any(lps[b] is not None for b in blocks)):
                        # the reference's per-position logits of the block rows (those tokens are forced): unused, or kept for
                        # the slots that record log-probabilities (row i of a slot's rows scores blk[i + 1])
                        lg = ops.gemm(torch.cat([hbs[b] for b in blocks]).contiguous(), self.lm_head)
                        r0 = 0
                        for b in blocks:
                            if lps[b] is not None:
                                lps[b].append(LlamaEngine._lp_block(self, b, lg[r0:r0 + plan[b][0]], blk[1:plan[b][0] + 1]))
                            r0 += hbs[b].shape[0]
                    for b, v in plan.items():
                        hid[b].append(hbs[b].clone())
                        if v is None:
                            last[b] = ids[b][-1]
                            continue
                        m, rows = v
                        toks = blk[1:m + 1]
                        LlamaEngine._history_append(self, b, toks)
                        ids[b] += toks
                        forced[b], rem[b] = forced[b][len(toks):], rem[b] - len(toks)
                        if rows == m + 1:
                            last[b] = blk[rows - 1]
                        else:
                            active[b] = False
        finally:
            self.set_stop_id(-1)
        if lp_slots:
            self.last_logprobs = [None if l is None else LlamaEngine._lp_join(l) for l in lps]
        return ids, [torch.cat(h)[:max(len(i) - 1, 0)] if h else None for h, i in zip(hid, ids)]

    def profile_decode(self, n_tokens=4):
        ms = (C.c_float * 8)()
        by = (C.c_double * 4)()
        check(lib().ss_llama_profile_decode(self._h, n_tokens, ms, by, ops.stream()), "ss_llama_profile_decode")
        return {"gemv_ms": ms[0], "attn_ms": ms[1], "gemv_down_ms": ms[2], "misc_ms": ms[3], "token_ms": ms[4],
                "gemv_bytes": by[0], "gemv_launches": by[1], "gemv_down_bytes": by[2], "gemv_down_launches": by[3]}

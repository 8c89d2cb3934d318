"""MI355X-native drop-in for the reference's ``src/models_clm/modeling_llama_xformer.py``.

``LlamaForCausalLM`` keeps the reference's surface that the hot path touches:
``from_pretrained(path, low_cpu_mem_usage, torch_dtype)``, HF parameter names
(``model.embed_tokens.weight`` … ``lm_head.weight``), ``get_input_embeddings()``,
``resize_token_embeddings()``, and the mutable attributes ``use_kv_cache_head`` /
``kv_cache_head`` / ``past_key_values`` (reference :676-678) that the drivers poke
(gen_george.py:165, vis_george_sink.py:171-173,244,293).

The decoder stack itself (reference LlamaRMSNorm :97-115, rotary :118-173, LlamaAttention
:217-301 with xformers FMHA, LlamaMLP :176-191, LlamaModel.forward :532-666) runs inside the
native engine (``seedstory.llama.LlamaEngine`` -> ``ss_llama_*``): there is no torch compute
here and no CPU path.
"""
import json
import os

import torch
from torch import nn

from seedstory.llama import LlamaEngine


class LlamaConfig:
    """The handful of transformers.LlamaConfig fields the path needs."""

    def __init__(self, hidden_size=4096, intermediate_size=11008, num_hidden_layers=32, num_attention_heads=32,
                 vocab_size=32000, max_position_embeddings=4096, rms_norm_eps=1e-5, eos_token_id=2, bos_token_id=1,
                 **kwargs):
        self.hidden_size = hidden_size
        self.intermediate_size = intermediate_size
        self.num_hidden_layers = num_hidden_layers
        self.num_attention_heads = num_attention_heads
        self.vocab_size = vocab_size
        self.max_position_embeddings = max_position_embeddings
        self.rms_norm_eps = rms_norm_eps
        self.eos_token_id = eos_token_id
        self.bos_token_id = bos_token_id
        self.use_cache = True
        self.output_attentions = bool(kwargs.get("output_attentions", False))    # the reference's switch for attention maps

    @classmethod
    def from_pretrained(cls, path):
        with open(os.path.join(path, "config.json")) as f:
            return cls(**json.load(f))


class _W(nn.Module):
    def __init__(self, o, i):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(o, i), requires_grad=False)


class _Norm(nn.Module):
    def __init__(self, d):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d), requires_grad=False)


class _Attn(nn.Module):
    def __init__(self, h):
        super().__init__()
        self.q_proj, self.k_proj, self.v_proj, self.o_proj = _W(h, h), _W(h, h), _W(h, h), _W(h, h)


class _MLP(nn.Module):
    def __init__(self, h, i):
        super().__init__()
        self.gate_proj, self.up_proj, self.down_proj = _W(i, h), _W(i, h), _W(h, i)


class _Layer(nn.Module):
    def __init__(self, h, i):
        super().__init__()
        self.self_attn = _Attn(h)
        self.mlp = _MLP(h, i)
        self.input_layernorm = _Norm(h)
        self.post_attention_layernorm = _Norm(h)


class _Embedding(nn.Module):
    def __init__(self, v, h):
        super().__init__()
        self.weight = nn.Parameter(torch.empty(v, h), requires_grad=False)

    def forward(self, input_ids):
        from seedstory import ops
        shape = tuple(input_ids.shape)
        rows = ops.gather_rows(self.weight.data, input_ids.reshape(-1))
        return rows.view(*shape, self.weight.shape[1])


class _Model(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.embed_tokens = _Embedding(cfg.vocab_size, cfg.hidden_size)
        self.layers = nn.ModuleList([_Layer(cfg.hidden_size, cfg.intermediate_size)
                                     for _ in range(cfg.num_hidden_layers)])
        self.norm = _Norm(cfg.hidden_size)


class LlamaForCausalLM(nn.Module):

    def __init__(self, config):
        super().__init__()
        self.config = config
        self.model = _Model(config)
        self.lm_head = _W(config.vocab_size, config.hidden_size)
        self.past_key_values = None
        self.kv_cache_head = None
        self.use_kv_cache_head = True
        self._engine = None
        self._engine_sig = None
        # engine sizing knobs (KV slots, generated-token ring, rows per prefill call)
        self.cache_cap = 2048
        self.max_new = 512
        self.max_prefill_rows = 1280
        self.decode_weights = None      # "fp8": e4m3 weight-only decode projections (LlamaEngine.enable_decode_fp8), "mxfp4": MXFP4
                                        # ones (enable_decode_mxfp4); None = the knobs
        self.kv_cache = None            # "fp8": decode attention reads an e4m3 shadow of the KV cache (LlamaEngine.enable_kv_fp8); None = the knob
        self.n_seq = 1                  # sequence slots of the engine: generate(num_return_sequences=n) needs n_seq >= n
        self._candidates = None         # (slots, kv_cache_head per candidate) of the last generate(num_return_sequences > 1)

    # generate(num_beams=n > 1, do_sample=False) runs beam search on the device (needs n_seq >= n); False: num_beams stays inert
    beam_search = False
    # generate(prompt_lookup_num_tokens=k) runs prompt-lookup speculative steps of k + 1 rows (at most 8) in the single-sequence
    # greedy loop (LlamaEngine.set_speculation); 0: prompt_lookup_num_tokens stays inert and no new call is made
    speculative = 0

    # ---- reference surface ------------------------------------------------------------------
    def get_input_embeddings(self):
        return self.model.embed_tokens

    def get_output_embeddings(self):
        return self.lm_head

    def resize_token_embeddings(self, vocab_size):
        """Grow/shrink embed_tokens and lm_head rows (peft_models.py:43-45); new rows keep the
        mean of the old table like HF's default initialiser is NOT reproduced (random there)."""
        for holder in (self.model.embed_tokens, self.lm_head):
            old = holder.weight.data
            new = torch.zeros(vocab_size, old.shape[1], dtype=old.dtype, device=old.device)
            n = min(vocab_size, old.shape[0])
            new[:n] = old[:n]
            holder.weight = nn.Parameter(new, requires_grad=False)
        self.config.vocab_size = vocab_size
        self._engine = None
        return self.model.embed_tokens

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, low_cpu_mem_usage=True, torch_dtype=None, **kwargs):
        """Loads an HF LLaMA folder (config.json + *.safetensors / pytorch_model*.bin)."""
        cfg = LlamaConfig.from_pretrained(pretrained_model_name_or_path)
        model = cls(cfg)
        from seedstory import ckpt as _ckpt
        sd = _ckpt.read_weights(pretrained_model_name_or_path)
        # HF checkpoints carry the RoPE inverse-frequency buffers of older transformers versions; they are derived data
        _ckpt.load_checked(model, {k: v for k, v in sd.items() if not k.endswith("rotary_emb.inv_freq")}, "llama:")
        if torch_dtype is not None:
            model = model.to(torch_dtype)
        return model

    def init_synthetic(self, seed=0, std=0.02):
        """N(0, 0.02) weights like the reference ``_init_weights`` (:399-408), on the current device."""
        for name, p in self.named_parameters():
            if p.dim() == 1:
                p.data.fill_(1.0)
            elif p.is_cuda:
                p.data.normal_(0.0, std)
            else:
                g = torch.Generator().manual_seed(seed + hash(name) % 10007)
                p.data.copy_(torch.randn(p.shape, generator=g) * std)
        self._engine = None
        return self

    # ---- engine --------------------------------------------------------------------------------
    # ---- generation (HF-4.34 greedy search semantics) -------------------
    def collect_flat_state(self):
        """HF-named flat weights for the engine: unwraps the peft-style children that
        ``get_peft_model_with_resize_embedding`` grafts on (LoRA factors, modules_to_save norms)."""
        flat = {}
        for name, prm in self.named_parameters():
            if ".original_module." in name:
                continue
            name = name.replace(".modules_to_save.default.", ".")
            flat[name] = prm.data
        return flat

    def engine_for_generation(self, img_ids):
        self._img_ids = tuple(img_ids)      # forward() reuses the engine of the last generate() instead of rebuilding
        lora = getattr(self, "_lora_scaling", None)
        p0 = self.lm_head.weight
        sig = (p0.data_ptr(), p0._version, p0.dtype, str(p0.device), tuple(img_ids), self.cache_cap, self.max_new,
               self.max_prefill_rows, self.decode_weights, self.kv_cache) + (int(self.n_seq),)
        if self._engine is None or self._engine_sig != sig:
            if not p0.is_cuda:
                raise RuntimeError("LlamaForCausalLM must be moved to the GPU first (no CPU path)")
            c = self.config
            self._engine = LlamaEngine(self.collect_flat_state(), hidden=c.hidden_size,
                                       n_heads=c.num_attention_heads, n_layers=c.num_hidden_layers,
                                       inter=c.intermediate_size, vocab=c.vocab_size, dtype=p0.dtype, device=p0.device,
                                       rms_eps=c.rms_norm_eps, max_pos=c.max_position_embeddings,
                                       cache_cap=self.cache_cap, max_new=self.max_new,
                                       max_prefill_rows=self.max_prefill_rows, img_ids=img_ids,
                                       eos_id=c.eos_token_id, lora_scaling=lora if lora is not None else 2.0,
                                       decode_weights=self.decode_weights, kv_cache=self.kv_cache,
                                       **({"n_seq": int(self.n_seq)} if int(self.n_seq) > 1 else {}))
            self._engine_sig = sig
        return self._engine

    # ---- single forward call (reference :703-794, inference part) ------------------------------------------
    @torch.no_grad()
    def forward(self, input_ids=None, attention_mask=None, position_ids=None, past_key_values=None, inputs_embeds=None,
                labels=None, use_cache=None, output_attentions=None, output_hidden_states=None, return_dict=None):
        """One model call with the reference's argument meaning: ``inputs_embeds`` (or ``input_ids``) [1, q] rows are fed
        after ``past_key_values`` (tuple over layers of (k, v) [1, heads, kv, head_dim], keys post-RoPE); ``position_ids``
        [1, q] default to kv .. kv+q-1; the mask is always the bottom-right causal one (the reference passes
        ``attention_mask=None`` down from ``prepare_inputs_for_generation``, :826,844).  Returns logits for ALL q rows
        (lm_head on every row, :759), the grown cache, and — unlike the reference, which can return every layer's input —
        ``hidden_states = (last,)``: the post-final-norm states, the only entry the path reads (models.py:182-197 uses
        ``hidden_states[-1]``).  Side effects as the reference: ``self.past_key_values`` (:778), ``kv_cache_head``
        (:780-784).  With ``labels`` or a batch of sequences: `_forward_sequences` (loss :761-772, forward only).
        ``output_attentions`` (default ``config.output_attentions``): ``attentions`` = tuple over layers of ``[1, q, kv + q]``,
        what the reference returns there (:299-301, 591-596) — head 0's PRE-softmax scores with the mask added in the model
        dtype; computed by a kernel of their own next to the flash attention (ss_attn_scores), not on the default path."""
        want_attn = bool(getattr(self.config, "output_attentions", False) if output_attentions is None else output_attentions)
        eng = self.engine_for_generation(tuple(getattr(self, "_img_ids", ())))
        dev = eng.device
        if inputs_embeds is None:
            inputs_embeds = self.model.embed_tokens(input_ids.to(dev))
        if labels is not None or inputs_embeds.shape[0] != 1:
            if past_key_values is not None:
                raise ValueError("the batched / loss forward takes whole sequences (no past_key_values)")
            if want_attn:
                raise ValueError("attention maps are returned by single-sequence calls only (not by the batched / loss forward)")
            return self._forward_sequences(eng, inputs_embeds.to(dev), labels, position_ids, output_hidden_states, return_dict)
        rows = inputs_embeds[0].to(dev)
        q = rows.shape[0]
        if past_key_values is None:
            eng.reset()
            kv = 0
        else:
            eng.load_past_key_values(past_key_values)
            kv = eng.lengths()[0]
        pos = None
        if position_ids is not None:
            pos = position_ids.reshape(-1).to(device=dev, dtype=torch.int32)
        elif kv:
            pos = torch.arange(kv, kv + q, dtype=torch.int32, device=dev)
        maps = eng.attn_capture_on(q, kv + q, row0=kv) if want_attn else None
        try:
            hid = eng.prefill(rows, pos_ids=pos, want_hidden=True)                # [q, H], post final norm
        finally:
            if want_attn:
                eng.attn_capture_off()
        from seedstory import ops as _ops
        logits = _ops.gemm(hid.contiguous(), self.lm_head.weight).unsqueeze(0)     # [1, q, V]
        pkv = eng.past_key_values()
        self.past_key_values = pkv
        if self.use_kv_cache_head and not self.training:
            n_in = q if input_ids is None else input_ids.shape[1]
            self.kv_cache_head = n_in if self.kv_cache_head is None else self.kv_cache_head + n_in
        attentions = tuple(maps[l].unsqueeze(0) for l in range(maps.shape[0])) if want_attn else None
        out = CausalLMOutputWithPast(logits=logits, past_key_values=pkv,
                                     hidden_states=(hid.unsqueeze(0),) if output_hidden_states else None,
                                     attentions=attentions)
        if return_dict is False:
            return (logits, pkv) + ((out.hidden_states,) if output_hidden_states else ()) + ((attentions,) if want_attn else ())
        return out


    def _forward_sequences(self, eng, inputs_embeds, labels, position_ids, output_hidden_states, return_dict):
        """The training-side call (reference :703-794 with ``labels``; forward only): ``inputs_embeds``
        [bz, sq, H] are bz independent causal sequences.  ``attention_mask`` plays no role in the outputs — the reference's
        xformers call ignores it too (``attn_bias=LowerTriangularMask()``, :281-295; the additive mask of :274 only
        touches ``attn_weights``, which is discarded), so right-padded rows are ordinary tokens whose labels are -100.
        logits for every row (:759); loss = CrossEntropyLoss over logits[..., :-1, :] / labels[..., 1:] (:761-772), one
        fixed-order reduction on the device, rounded to the model dtype like torch's."""
        from seedstory import ops as _ops
        bz, sq, H = inputs_embeds.shape
        if sq > eng.max_rows:
            raise ValueError("sequence length %d exceeds max_prefill_rows=%d" % (sq, eng.max_rows))
        hid = torch.empty(bz, sq, H, dtype=inputs_embeds.dtype, device=inputs_embeds.device)
        V = self.lm_head.weight.shape[0]
        logits = torch.empty(bz, sq, V, dtype=inputs_embeds.dtype, device=inputs_embeds.device)
        for b in range(bz):
            eng.reset()
            pos = None
            if position_ids is not None:
                pr = position_ids if position_ids.dim() == 1 or position_ids.shape[0] == 1 else position_ids[b]
                pos = pr.reshape(-1).to(device=inputs_embeds.device, dtype=torch.int32)
            hb = eng.prefill(inputs_embeds[b].contiguous(), pos_ids=pos, want_hidden=True)     # [sq, H], post final norm
            hid[b].copy_(hb)
            _ops.gemm(hid[b], self.lm_head.weight, out=logits[b])
        eng.reset()
        loss = None
        if labels is not None:
            labels = labels.to(inputs_embeds.device)
            if labels.shape != (bz, sq):
                raise ValueError("labels must be [batch, sequence]")
            bad = (labels != -100) & ((labels < 0) | (labels >= V))
            if bool(bad.any()):
                raise ValueError("label outside [0, vocab) (and not -100)")
            shift_logits = logits[:, :-1, :].reshape(-1, V).contiguous()
            shift_labels = labels[:, 1:].reshape(-1)
            loss, n_valid = _ops.cross_entropy(shift_logits, shift_labels, -100)
            if float(n_valid) == 0.0:
                loss = torch.full((), float("nan"), device=loss.device)      # CrossEntropyLoss over no target
            loss = loss.to(inputs_embeds.dtype)
        self.past_key_values = None
        out = CausalLMOutputWithPast(logits=logits, past_key_values=None,
                                     hidden_states=(hid,) if output_hidden_states else None, loss=loss)
        if return_dict is False:
            t = (logits, None) + ((out.hidden_states,) if output_hidden_states else ())
            return ((loss,) + t) if loss is not None else t
        return out

    def prepare_inputs_for_generation(self, input_ids, past_key_values=None, attention_mask=None, inputs_embeds=None,
                                      **kwargs):
        """What HF's greedy loop feeds each step (reference :796-852).  With ``use_kv_cache_head`` and a cache, the rows
        ``[kv_cache_head:]`` of the running sequence go in (ids, and embeds when more than one row is left) with the
        matching slice of ``cumsum(mask) - 1`` as positions; otherwise the last token only.  Embeddings are used on the
        first step only.  The mask itself is dropped (the attention is bottom-right causal by construction)."""
        head_mode = self.use_kv_cache_head and not self.training
        cut = self.kv_cache_head if head_mode else -1
        if past_key_values:
            input_ids = input_ids[:, cut:]
            if head_mode and inputs_embeds is not None:
                inputs_embeds = inputs_embeds[:, cut:]
        position_ids = kwargs.get("position_ids", None)
        if attention_mask is not None and position_ids is None:
            position_ids = attention_mask.long().cumsum(-1) - 1
            position_ids.masked_fill_(attention_mask == 0, 1)
            if past_key_values:
                position_ids = position_ids[:, cut:].unsqueeze(-1) if head_mode else position_ids[:, -1].unsqueeze(-1)
        if inputs_embeds is not None and past_key_values is None:
            model_inputs = {"inputs_embeds": inputs_embeds, "input_ids": input_ids}
        elif head_mode and past_key_values is not None and input_ids.shape[1] > 1:
            model_inputs = {"inputs_embeds": inputs_embeds, "input_ids": input_ids}
        else:
            model_inputs = {"input_ids": input_ids}
        model_inputs.update({"position_ids": position_ids, "past_key_values": past_key_values,
                             "use_cache": kwargs.get("use_cache"), "attention_mask": None})
        return model_inputs

    @torch.no_grad()
    def generate(self, input_ids=None, inputs_embeds=None, logits_processor=None, past_key_values=None,
                 max_new_tokens=120, output_hidden_states=True, return_dict_in_generate=True, forced_tokens=None,
                 output_attentions=None, do_sample=False, temperature=1.0, top_k=0, top_p=1.0, seed=None, num_beams=1,
                 repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, spare_img_ids=False, output_logprobs=False,
                 top_logprobs=0, num_return_sequences=1, length_penalty=1.0, early_stopping=False, prompt_lookup_num_tokens=None,
                 max_matching_ngram_size=None, **unused):
        """Greedy search as ``ContinuousLVLM.generate`` drives it (reference models.py:146-153): ``inputs_embeds`` feed
        step 0, ``input_ids`` is the running sequence, the image-token logits processor is applied on device.
        ``do_sample=False`` (the default): temperature / top_k / top_p / seed are inert, as in Hugging Face.
        ``do_sample=True``: every free token is drawn on the device, inside the decode token — processor -> temperature ->
        top-k -> top-p -> one Philox draw (``LlamaEngine.set_sampling``; the definition and where it departs from the
        warpers: include/seedstory_hip.h).  ``top_k=0`` means off: Hugging Face's default of 50 is NOT adopted.
        ``seed=None`` takes ``torch.initial_seed()`` plus a per-model call counter, so ``torch.manual_seed`` governs the run
        and successive calls differ; an explicit seed reproduces a call exactly.  The engine is greedy again when the call
        returns or raises.  ``num_beams > 1`` with ``do_sample`` raises ``NotImplementedError``.
        ``repetition_penalty`` / ``no_repeat_ngram_size`` / ``min_new_tokens`` (Hugging Face's defaults 1.0 / 0 / 0: inert) act on
        greedy search and on sampling alike, on the device, in HF's order in front of the image-token processor
        (``LlamaEngine.set_logits_rules``; include/seedstory_hip.h): when one of them is active ``input_ids[0]`` is handed over as
        the token history and the rules are cleared when the call returns or raises.  ``spare_img_ids=True`` (a declared
        deviation, off by default) exempts the image-token ids from the penalty.
        ``output_attentions`` (default ``config.output_attentions``, the reference's switch): ``attentions`` = tuple over steps
        of tuple over layers — step 0 ``[1, q0, kv0 + q0]``, step j ``[1, 1, kv0 + q0 + j]``, as many as ``hidden_states`` —
        all VIEWS of one capture buffer, which ``attention_maps`` [layers, rows, width] hands out whole (one row per fed token,
        NaN beyond each row's key count: what the reference's pad-and-concatenate merge builds, models.py:164-179).
        ``output_logprobs=True``: the output's ``logprobs`` (the log of the probability with which the policy — greedy or
        sampling, after the rules and the processor — picked each token; 0.0 for a forced token and a processor-forced image
        token), ``model_logprobs`` (the model's own log-softmax of the untouched logits) and, with ``top_logprobs`` = 1 .. 8,
        ``top_logprob_ids`` / ``top_logprob_values`` [n, top_logprobs] hold one float32 entry per generated token, computed
        on the device inside the decode token (``LlamaEngine.set_logprobs``; include/seedstory_hip.h); the engine records
        nothing any more when the call returns or raises.  ``output_scores`` / ``output_logits`` (full [vocab] rows per
        step) are not part of this and stay ignored.
        ``num_return_sequences=n`` (> 1; needs ``do_sample=True`` and ``n <= self.n_seq``, the engine's slot count, set before
        the first ``generate``): n sampled continuations of the one prompt.  The prompt is prefilled once, on slot 0 (with
        ``past_key_values``: on the selected slot), the slot is forked on the device to the n - 1 lowest other slots
        (``LlamaEngine.fork``), and all candidates decode in lock-step, one sweep of the weights per token; they share the
        seed and diverge because the slot is part of the Philox counter.  ``sequences`` is ``[n, S + longest]``, right-padded
        with ``config.pad_token_id`` (EOS when that is None); ``candidates`` holds n outputs in the batch-1 layout (candidate 0
        = the source slot, then ascending slots); the top-level ``hidden_states`` / log-probability fields are candidate 0's,
        ``self.past_key_values`` and the ``kv_cache_head`` advance refer to it, and ``select_candidate(i)`` switches to
        another.  ``num_beams`` stays inert without ``do_sample`` while ``LlamaForCausalLM.beam_search`` is False (the default).
        ``beam_search = True`` and ``num_beams=n`` (> 1, ``do_sample=False``, ``n <= self.n_seq``): the free tokens up to the first
        stop — EOS, ``<img>`` or ``max_new_tokens`` — come from a beam search on the device inside the decode token
        (``LlamaEngine.beam_search``; the definition, Hugging Face's ``_beam_search`` with ``length_penalty`` /
        ``early_stopping`` on the log-softmax of the row AFTER the rules and the image-token processor, is in
        include/seedstory_hip.h).  The prompt is prefilled once on slot 0; the winner ``t_1 .. t_m`` is then made real on
        slot 0 — the cache rewound to the prompt end, ``t_1 .. t_{m-1}`` fed as one prefill — and everything behind it is the
        existing greedy path with ``t_m`` forced: the image block behind a winner that ends in ``<img>`` and whatever follows
        ``</img>``.  The winner's hidden rows therefore come from the prefill GEMMs while the search scored them with the
        decode GEMVs (the image block already mixes the two).  The output is the usual batch-1 one, plus
        ``sequences_scores`` (the winner's score) and ``beams`` (the n finished hypotheses, best first, as dicts of
        ``sequence`` / ``score`` / ``finished``); ``past_key_values`` and the ``kv_cache_head`` advance are the winner's.  The
        rules apply to every beam.  Raised before the engine is touched: ``ValueError`` for ``num_beams > n_seq``,
        ``forced_tokens`` and ``num_return_sequences > 1``; ``NotImplementedError`` for ``output_attentions``,
        ``output_logprobs`` and ``kv_cache == "fp8"``."""
        want_attn = bool(getattr(self.config, "output_attentions", False) if output_attentions is None else output_attentions)
        if do_sample and num_beams is not None and int(num_beams) > 1:
            raise NotImplementedError("beam-search sampling (do_sample=True with num_beams=%d) is not implemented" % int(num_beams))
        n_ret = 1 if num_return_sequences is None else int(num_return_sequences)
        n_beams = int(num_beams) if (self.beam_search and not do_sample and num_beams is not None) else 1
        if n_beams > 1:
            if n_beams > int(self.n_seq) or n_beams > 8:
                raise ValueError("num_beams=%d exceeds the engine's sequence slots: set LlamaForCausalLM.n_seq (now %d, at most 8) "
                                 "before the first generate()" % (n_beams, int(self.n_seq)))
            if forced_tokens:
                raise ValueError("forced_tokens cannot be combined with beam search (num_beams=%d)" % n_beams)
            if n_ret > 1:
                raise ValueError("num_return_sequences=%d with beam search is not supported (the hypotheses are in `beams`)" % n_ret)
            if early_stopping not in (False, True, "never"):
                raise ValueError("early_stopping must be False, True or 'never', not %r" % (early_stopping,))
            if want_attn:
                raise NotImplementedError("attention maps are a single-sequence tool (output_attentions with num_beams=%d)" % n_beams)
            if output_logprobs:
                raise NotImplementedError("output_logprobs with beam search is not implemented (num_beams=%d)" % n_beams)
            if self.kv_cache == "fp8":
                raise NotImplementedError("beam search with kv_cache='fp8' is not implemented: the search does not permute the "
                                          "fp8 shadow")
        if n_ret > 1:
            if not do_sample:
                raise ValueError("num_return_sequences=%d needs do_sample=True: greedy search has one continuation" % n_ret)
            if n_ret > int(self.n_seq):
                raise ValueError("num_return_sequences=%d exceeds the engine's sequence slots: set LlamaForCausalLM.n_seq "
                                 "(now %d, at most 8) before the first generate()" % (n_ret, int(self.n_seq)))
            if want_attn:
                raise NotImplementedError("attention maps are a single-sequence tool (output_attentions with num_return_sequences=%d)" % n_ret)
        # prompt-lookup speculation (Hugging Face's names): only with the switch on, only for the single greedy sequence
        spec_rows = 0
        if self.speculative and prompt_lookup_num_tokens and n_ret == 1 and n_beams == 1:
            spec_rows = min(int(prompt_lookup_num_tokens) + 1, 8)
            ngram = 2 if max_matching_ngram_size is None else int(max_matching_ngram_size)
            if spec_rows < 2 or not 1 <= ngram <= 8:
                raise ValueError("prompt_lookup_num_tokens=%r / max_matching_ngram_size=%r: at least 1 token, n-grams of 1..8"
                                 % (prompt_lookup_num_tokens, max_matching_ngram_size))
            rules_on = (repetition_penalty not in (None, 1.0) or no_repeat_ngram_size not in (None, 0) or min_new_tokens not in (None, 0))
            for bad, what in ((do_sample, "do_sample=True (speculative sampling)"), (rules_on, "the logits rules"),
                              (output_logprobs, "output_logprobs"), (want_attn, "output_attentions"),
                              (self.kv_cache == "fp8", "kv_cache='fp8'")):
                if bad:
                    raise NotImplementedError("prompt-lookup speculation with %s is not implemented" % what)
        img_ids = ()
        for proc in (logits_processor or []):
            img_ids = tuple(getattr(proc, "img_ids_list", ()))
        eng = self.engine_for_generation(img_ids)
        dev = eng.device
        input_ids = input_ids.to(dev)
        S = input_ids.shape[1]
        if inputs_embeds is None:
            inputs_embeds = self.model.embed_tokens(input_ids)
        rows = inputs_embeds[0]
        if (n_ret > 1 or n_beams > 1) and past_key_values is None:
            eng.select(0)
        if do_sample:
            if seed is None:
                self._sample_calls = getattr(self, "_sample_calls", 0) + 1
                seed = (torch.initial_seed() + self._sample_calls - 1) & (2 ** 64 - 1)
            eng.set_sampling(temperature=temperature, top_k=top_k, top_p=top_p, seed=seed)     # raises on a bad parameter
        # (Hugging Face also takes None for "off")
        rules = (repetition_penalty not in (None, 1.0) or no_repeat_ngram_size not in (None, 0) or min_new_tokens not in (None, 0))
        try:
            if spec_rows:
                eng.set_speculation(spec_rows, max_ngram=ngram)
                eng.set_history(input_ids[0].tolist())
            if output_logprobs:
                eng.set_logprobs(True, top_n=top_logprobs)                            # raises on a bad value
            if rules:
                eng.set_logits_rules(repetition_penalty=1.0 if repetition_penalty is None else repetition_penalty,
                                     no_repeat_ngram_size=no_repeat_ngram_size or 0, min_new_tokens=min_new_tokens or 0,
                                     spare_img_ids=bool(spare_img_ids))               # raises on a bad value
                eng.set_history(input_ids[0].tolist())
            if n_ret > 1:
                return self._generate_candidates(eng, n_ret, input_ids, rows, S, img_ids, past_key_values, max_new_tokens,
                                                 output_hidden_states, forced_tokens, bool(output_logprobs))
            if n_beams > 1:
                return self._generate_beams(eng, n_beams, 1.0 if length_penalty is None else float(length_penalty), early_stopping,
                                            input_ids, rows, S, img_ids, past_key_values, max_new_tokens, output_hidden_states, rules)
            return self._generate(eng, input_ids, rows, S, img_ids, past_key_values, max_new_tokens, output_hidden_states,
                                  forced_tokens, want_attn, **({"want_logprobs": True} if output_logprobs else {}))
        finally:
            if spec_rows:
                eng.clear_speculation()
            if output_logprobs:
                eng.set_logprobs(False)
            if rules:
                eng.clear_logits_rules()
            if do_sample:
                eng.set_greedy()
            if want_attn:
                eng.attn_capture_off()

    def _generate(self, eng, input_ids, rows, S, img_ids, past_key_values, max_new_tokens, output_hidden_states,
                  forced_tokens, want_attn, want_logprobs=False):
        dev = eng.device
        maps, kv0, fed0, hid0 = self._feed_prompt(eng, rows, S, past_key_values, max_new_tokens, output_hidden_states, want_attn)
        self._candidates = None
        if img_ids and eng.img_block_enabled():
            # the 65 processor-forced tokens behind <img> run as one batched continuation (seedstory/llama.py)
            gen_list, hr = eng.generate_img_block(max_new_tokens, int(input_ids[0, -1]), forced_tokens)
            n = len(gen_list)
            gen = torch.tensor(gen_list, dtype=torch.long, device=dev)
            lp = eng.last_logprobs if want_logprobs else None
        else:
            n = eng.generate(max_new_tokens, int(input_ids[0, -1]), forced_tokens)
            gen = eng.gen_ids[:n].to(torch.long)
            hr = eng.hidden_rows[:max(n - 1, 0)]
            lp = {k: v.clone() for k, v in eng.logprobs(n).items()} if want_logprobs else None
        self.past_key_values = eng.past_key_values()
        if self.use_kv_cache_head:
            adv = fed0 + max(n - 1, 0)
            self.kv_cache_head = adv if self.kv_cache_head is None else self.kv_cache_head + adv
        attentions = attention_maps = None
        if want_attn:
            fed = fed0 + max(n - 1, 0)
            attentions = attention_step_views(maps, kv0, fed0, fed)
            attention_maps = maps[:, :fed, :kv0 + fed]
        return self._output(input_ids, gen, hid0, hr, lp, output_hidden_states, attentions, attention_maps)

    @staticmethod
    def _output(input_ids, gen, hid0, hr, lp, output_hidden_states, attentions=None, attention_maps=None):
        """one sequence's ``GenerateOutput`` in the batch-1 layout"""
        sequences = torch.cat([input_ids[0], gen]).unsqueeze(0)
        hidden_states = None
        if output_hidden_states:
            steps = [(hid0.unsqueeze(0),)]
            steps += [(hr[j].view(1, 1, -1),) for j in range(hr.shape[0])]
            hidden_states = tuple(steps)
        scores = {}
        if lp is not None:
            scores = dict(logprobs=lp["logprob"], model_logprobs=lp["model_logprob"], top_logprob_ids=lp["top_ids"],
                          top_logprob_values=lp["top_logprobs"])
        return GenerateOutput(sequences=sequences, hidden_states=hidden_states, attentions=attentions,
                              attention_maps=attention_maps, **scores)

    def _feed_prompt(self, eng, rows, S, past_key_values, max_new_tokens, output_hidden_states, want_attn):
        """The prompt rows (all of them, or those behind ``past_key_values``) on the selected slot; returns (capture buffer,
        cache length before, rows fed, their hidden rows)."""
        dev = eng.device
        maps, kv0 = None, 0
        if past_key_values is None:
            eng.reset()
            fed0 = S
            if want_attn:
                maps = eng.attn_capture_on(fed0 + max_new_tokens, fed0 + max_new_tokens, row0=0)
            hid0 = eng.prefill(rows, want_hidden=output_hidden_states)
        else:
            head = self.kv_cache_head if (self.use_kv_cache_head and self.kv_cache_head is not None) else S - 1
            eng.load_past_key_values(past_key_values)
            fed0 = S - head
            kv0 = eng.lengths()[0]
            if want_attn:
                maps = eng.attn_capture_on(fed0 + max_new_tokens, kv0 + fed0 + max_new_tokens, row0=kv0)
            pos = torch.arange(head, S, dtype=torch.int32, device=dev)      # cumsum(mask)-1 sliced (:811-816)
            hid0 = eng.prefill(rows[head:], pos_ids=pos, want_hidden=output_hidden_states)
            eng.set_lengths(eng.lengths()[0], S)
        if max_new_tokens > eng.max_new:
            raise ValueError("max_new_tokens=%d exceeds the engine's generated-token ring (max_new=%d): raise "
                             "LlamaForCausalLM.max_new before the first generate()" % (max_new_tokens, eng.max_new))
        return maps, kv0, fed0, hid0

    def _generate_candidates(self, eng, n_ret, input_ids, rows, S, img_ids, past_key_values, max_new_tokens,
                             output_hidden_states, forced_tokens, want_logprobs):
        """``generate(num_return_sequences=n_ret)``: one prefill on the selected (source) slot, a device fork to the n_ret - 1
        lowest other slots, one lock-step decode of the n_ret candidates.  The caller has set sampling, rules, the source's
        history and recording (each for every slot; the fork hands the history on) and restores them."""
        dev = eng.device
        NS = int(eng.n_seq)
        src = int(getattr(eng, "_cur", 0))
        _, _, fed0, hid0 = self._feed_prompt(eng, rows, S, past_key_values, max_new_tokens, output_hidden_states, False)
        others = [b for b in range(NS) if b != src][:n_ret - 1]
        eng.fork(src, others)
        slots = [src] + others
        on = [b in slots for b in range(NS)]
        last = int(input_ids[0, -1])
        forced = [list(forced_tokens or []) if on[b] else [] for b in range(NS)]
        if img_ids and eng.img_block_enabled():
            ids, hrs = eng.generate_batch_img_block(max_new_tokens, [last] * NS, forced, active=on)
            lps = eng.last_logprobs if want_logprobs else None
        else:
            ns = eng.generate_batch(max_new_tokens, [last] * NS, forced, on)
            ids, hrs, lps = [[] for _ in range(NS)], [None] * NS, [None] * NS
            for b in slots:
                eng.select(b)
                ids[b] = eng.gen_ids[:ns[b]].tolist()
                hrs[b] = eng.hidden_rows[:max(ns[b] - 1, 0)]
                if want_logprobs:
                    lps[b] = {k: v.clone() for k, v in eng.logprobs(ns[b], b).items()}
        eng.select(src)
        cands = [self._output(input_ids, torch.tensor(ids[b], dtype=torch.long, device=dev), hid0, hrs[b],
                              lps[b] if want_logprobs else None, output_hidden_states) for b in slots]
        self.past_key_values = eng.past_key_values()
        base = self.kv_cache_head
        heads = [None] * n_ret
        if self.use_kv_cache_head:
            heads = [(0 if base is None else base) + fed0 + max(len(ids[b]) - 1, 0) for b in slots]
            self.kv_cache_head = heads[0]
        self._candidates = (slots, heads)
        pad = getattr(self.config, "pad_token_id", None)
        pad = self.config.eos_token_id if pad is None else pad
        width = max(c.sequences.shape[1] for c in cands)
        sequences = torch.full((n_ret, width), int(pad), dtype=cands[0].sequences.dtype, device=dev)
        for i, c in enumerate(cands):
            sequences[i, :c.sequences.shape[1]] = c.sequences[0]
        c0 = cands[0]
        return GenerateOutput(sequences=sequences, hidden_states=c0.hidden_states, attentions=None, logprobs=c0.logprobs,
                              model_logprobs=c0.model_logprobs, top_logprob_ids=c0.top_logprob_ids,
                              top_logprob_values=c0.top_logprob_values, candidates=cands)

    def _generate_beams(self, eng, n_beams, length_penalty, early_stopping, input_ids, rows, S, img_ids, past_key_values,
                        max_new_tokens, output_hidden_states, rules):
        """``generate(num_beams=n_beams)`` with ``beam_search`` on: prefill on slot 0, the search, the winner made real on slot
        0, the rest by the greedy path with the winner's last token forced.  The caller has set the rules and the history
        and clears them."""
        from seedstory import ops
        from seedstory.llama import _prefill_chunked
        dev = eng.device
        _, _, fed0, hid0 = self._feed_prompt(eng, rows, S, past_key_values, max_new_tokens, output_hidden_states, False)
        self._candidates = None
        kv_end, pos_end = eng.lengths()
        last = int(input_ids[0, -1])
        has_img = bool(img_ids) and len(img_ids) >= 3
        block = has_img and eng.img_block_enabled()
        if has_img:
            eng.set_stop_id(img_ids[0])             # a hypothesis that opens an image is finished: the ids behind <img> are forced
        try:
            res = eng.beam_search(max_new_tokens, last, n_beams, length_penalty=length_penalty, early_stopping=early_stopping)
        finally:
            if has_img:
                eng.set_stop_id(-1)
        win = [int(t) for t in res["sequences"][0]]
        m = len(win)
        # the winner on slot 0: back to the prompt end, t_1 .. t_{m-1} as one continuation (its history likewise)
        eng.select(0)
        eng.set_lengths(kv_end, pos_end)
        if rules:
            eng.set_history(input_ids[0].tolist())
            if m > 1:
                eng.set_history(win[:-1], append=True)
        parts = []
        if m > 1:
            emb = ops.gather_rows(eng.embed, torch.tensor(win[:-1], dtype=torch.int32, device=dev))
            parts.append(_prefill_chunked(eng, emb, True))
        rem = max_new_tokens - (m - 1)
        prev = win[-2] if m > 1 else last
        if block:
            tail, hr = eng.generate_img_block(rem, prev, [win[-1]])
        else:
            n = eng.generate(rem, prev, [win[-1]])
            tail, hr = eng.gen_ids[:n].tolist(), eng.hidden_rows[:max(n - 1, 0)]
        parts.append(hr)
        gen_list = win[:-1] + [int(t) for t in tail]
        gen = torch.tensor(gen_list, dtype=torch.long, device=dev)
        hr = torch.cat([p.to(parts[-1].dtype) for p in parts]) if len(parts) > 1 else parts[0]
        self.past_key_values = eng.past_key_values()
        if self.use_kv_cache_head:
            adv = fed0 + max(len(gen_list) - 1, 0)
            self.kv_cache_head = adv if self.kv_cache_head is None else self.kv_cache_head + adv
        out = self._output(input_ids, gen, hid0, hr, None, output_hidden_states)
        out.sequences_scores = res["scores"][:1].clone()
        out.beams = [dict(sequence=list(q), score=float(sc), finished=bool(f))
                     for q, sc, f in zip(res["sequences"], res["scores"].tolist(), res["finished"].tolist())]
        return out

    def select_candidate(self, i):
        """After ``generate(num_return_sequences=n)``: continue from candidate ``i`` — its slot becomes the selected one,
        ``past_key_values`` and ``kv_cache_head`` refer to it.  Returns the slot."""
        if self._candidates is None:
            raise ValueError("select_candidate: the last generate() returned one sequence")
        slots, heads = self._candidates
        if not 0 <= int(i) < len(slots):
            raise ValueError("select_candidate: candidate %d outside [0, %d)" % (int(i), len(slots)))
        eng = self._engine if self._engine is not None else self.engine_for_generation(tuple(getattr(self, "_img_ids", ())))
        eng.select(slots[int(i)])
        self.past_key_values = eng.past_key_values()
        if self.use_kv_cache_head:
            self.kv_cache_head = heads[int(i)]
        return slots[int(i)]


def attention_step_views(maps, kv0, fed0, fed):
    """HF's ``attentions`` of a greedy run as views of the capture buffer ``maps`` [layers, rows, width] (row r = the r-th fed
    token, cache length ``kv0`` before the run): tuple over steps of tuple over layers, step 0 = the ``fed0`` rows of the first
    call ``[1, fed0, kv0 + fed0]``, step j = row ``fed0 + j - 1`` as ``[1, 1, kv0 + fed0 + j]``, up to ``fed`` rows in all."""
    L = maps.shape[0]
    steps = [tuple(maps[l, :fed0, :kv0 + fed0].unsqueeze(0) for l in range(L))]
    steps += [tuple(maps[l, fed0 + j - 1:fed0 + j, :kv0 + fed0 + j].unsqueeze(0) for l in range(L))
              for j in range(1, fed - fed0 + 1)]
    return tuple(steps)


class CausalLMOutputWithPast:
    def __init__(self, logits, past_key_values, hidden_states=None, loss=None, attentions=None):
        self.loss, self.logits, self.past_key_values = loss, logits, past_key_values
        self.hidden_states, self.attentions = hidden_states, attentions

    def __getitem__(self, i):
        if isinstance(i, str):        # ModelOutput's dict-style access (models.py:69 reads output_lm['loss'])
            return getattr(self, i)
        return (self.logits, self.past_key_values, self.hidden_states)[i]


class GenerateOutput:
    def __init__(self, sequences, hidden_states, attentions, attention_maps=None, logprobs=None, model_logprobs=None,
                 top_logprob_ids=None, top_logprob_values=None, candidates=None):
        self.sequences = sequences
        self.hidden_states = hidden_states
        self.attentions = attentions
        self.attention_maps = attention_maps      # [layers, rows, width]: the buffer every entry of `attentions` is a view of
        # float32, one entry per generated token (generate(output_logprobs=True)); None when not asked for
        self.logprobs, self.model_logprobs = logprobs, model_logprobs
        self.top_logprob_ids, self.top_logprob_values = top_logprob_ids, top_logprob_values
        # generate(num_return_sequences=n > 1): the n outputs in the batch-1 layout (`sequences` above is then [n, S + longest])
        self.candidates = candidates
        # generate(num_beams=n > 1) with LlamaForCausalLM.beam_search on: the winner's score [1] and the n hypotheses, best first
        self.sequences_scores, self.beams = None, None

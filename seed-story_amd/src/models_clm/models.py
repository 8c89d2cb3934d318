"""MI355X-native drop-in for the reference's ``src/models_clm/models.py`` (inference part).

``ContinuousLVLM`` keeps the constructor, ``from_pretrained`` and ``generate`` signatures and
the returned dict keys of the reference (models.py:20-31, 98-230).  ``generate`` does what the
reference does — embed + splice image features (:127-135), greedy decode with the image-token
logits processor (:137-153), slice the 64 last-layer states in front of the last ``</img>``
(:182-197) and regress them to a 256x4096 ViT-space feature with the output resampler (:205) —
but every tensor op is a HIP kernel of libseedstory_hip.so and the T-iteration decode loop runs
from one hipGraph with no per-token host sync.  ``forward`` (:33-96) is the training-side forward WITHOUT autograd:
losses and the regressed features as the reference computes them, no backward kernels.
"""
import torch
from torch import nn

from seedstory import ops

from .generation import AutoImageTokenGenerationProcessor, LogitsProcessorList

BOI_TOKEN = '<img>'
EOI_TOKEN = '</img>'
IMG_TOKEN = '<img_{:05d}>'


def candidate_score(ids, model_logprobs, img_ids):
    """Score of one sampled candidate for best-of-n: the mean of ``model_logprobs`` (the model's own log-probability of
    each generated token, ``generate(output_logprobs=True)``) over the generated positions whose id is not in ``img_ids``
    — the 65 ids the image-token processor forces behind ``<img>``, which the model did not choose.  ``-inf`` when no such
    position exists.  Pure host arithmetic on lists or tensors."""
    skip = set(int(t) for t in img_ids)
    ids = ids.tolist() if isinstance(ids, torch.Tensor) else list(ids)
    lps = model_logprobs.tolist() if isinstance(model_logprobs, torch.Tensor) else list(model_logprobs)
    vals = [float(v) for t, v in zip(ids, lps) if int(t) not in skip]
    return sum(vals) / len(vals) if vals else float("-inf")


def best_candidate(scores):
    """index of the highest score; ties (and all ``-inf``) go to the lowest index"""
    best = 0
    for i, v in enumerate(scores):
        if v > scores[best]:
            best = i
    return best


class ContinuousLVLM(nn.Module):

    def __init__(self, llm, input_resampler, output_resampler, lm_loss_scale=1.0, rec_loss_scale=1.0) -> None:
        super().__init__()
        self.llm = llm
        self.input_resampler = input_resampler
        self.output_resampler = output_resampler
        self.lm_loss_scale = lm_loss_scale
        self.rec_loss_scale = rec_loss_scale
        self._regressor_fp32 = None

    def enable_fp32_regressor(self, on=True):
        """Mixed mode: keep the 16-bit LLM but run the image-feature REGRESSOR (the output resampler on the
        64 last-layer rows, < 0.1 % of a story step) in exact fp32 on an fp32 copy of its weights; the result is rounded
        once to the model dtype.  OFF by default: measured at hidden 4096 it moves the bf16 ``img_gen_feat`` distance to the
        fp32 reference from 3.0e-2 to ~2.8e-2 — the error is carried by the 64 bf16 rows coming out of the decoder stack,
        not by the regressor (tests/test_frontend_full_gpu.py prints both)."""
        if on:
            import copy
            r = self.output_resampler
            cache, r._cache = getattr(r, "_cache", None), {}      # the prepared-weights cache holds ctypes structs (not copyable)
            try:
                self._regressor_fp32 = copy.deepcopy(r).float()
            finally:
                if cache is not None:
                    r._cache = cache
        else:
            self._regressor_fp32 = None
        return self

    def _regress(self, rows):
        if self._regressor_fp32 is not None and rows.dtype != torch.float32:
            return self._regressor_fp32(rows.float()).to(rows.dtype)
        return self.output_resampler(rows)

    @torch.no_grad()
    def forward(self, input_ids, attention_mask, labels, image_embeds, embeds_gen_mask, embeds_cmp_mask, ids_gen_mask,
                ids_cmp_mask, return_recon_image_embeds=False):
        """The training-side forward of the reference (models.py:33-96), FORWARD ONLY (no autograd):
        splice the input-resampled features of the comprehension images into the embedded batch (:54-56), run the LLM on
        the bz sequences with the token cross-entropy (:64-69), regress the last-layer states at the generation slots
        through the output resampler and score them with the cosine loss against the target ViT features (:73-81),
        ``total = lm_loss_scale * lm + rec_loss_scale * rec`` (:92).  The reference's placeholder branches for batches
        without images multiply random tensors by 0.0 (:41-47, 58-62, 82-90): here the corresponding terms are exactly 0."""
        embed = self.llm.get_input_embeddings()
        dev = embed.weight.device
        input_ids = input_ids.to(dev)
        input_embeds = embed(input_ids)                                   # [bz, sq, H]   (:36)
        bz, sq, dim = input_embeds.shape
        has_image = image_embeds is not None
        has_image_input = has_image and int(embeds_cmp_mask.sum().item()) > 0
        has_image_output = has_image and int(embeds_gen_mask.sum().item()) > 0
        if has_image:
            image_embeds = image_embeds.to(dev)
        if has_image_input:
            image_embeds_lm = self.input_resampler(image_embeds)          # [Nimg, nq, H]  (:40)
            sel = image_embeds_lm[embeds_cmp_mask.to(dev)].reshape(-1, dim).contiguous()
            idx = torch.nonzero(ids_cmp_mask.to(dev).reshape(-1), as_tuple=False).flatten()
            assert idx.numel() == sel.shape[0], "ids_cmp_mask / embeds_cmp_mask disagree"
            flat = input_embeds.reshape(-1, dim)
            ops.scatter_rows_(flat, idx, sel)                             # (:55)
            input_embeds = flat.view(bz, sq, dim)
        output_lm = self.llm(attention_mask=attention_mask, inputs_embeds=input_embeds, labels=labels,
                             output_hidden_states=True, return_dict=True)
        lm_loss = output_lm['loss']
        last_hidden_state = output_lm.hidden_states[-1]                   # [bz, sq, H]
        recon_image_embeds = None
        if has_image_output:
            target_embeds = image_embeds[embeds_gen_mask.to(dev)].contiguous()       # [Ngen, 256, 4096]  (:74)
            num_imgs_for_rec = target_embeds.shape[0]
            gidx = torch.nonzero(ids_gen_mask.to(dev).reshape(-1), as_tuple=False).flatten()
            rows = ops.gather_rows(last_hidden_state.reshape(-1, dim).contiguous(), gidx.to(torch.int32))
            output_image_embeds = rows.view(num_imgs_for_rec, -1, dim)               # (:76)
            recon_image_embeds = self.output_resampler(output_image_embeds)          # (:79)
            rec_loss = ops.cosine_loss(recon_image_embeds.contiguous(), target_embeds).to(input_embeds.dtype)   # (:81)
        else:
            rec_loss = torch.zeros((), dtype=input_embeds.dtype, device=dev)
        total_loss = self.lm_loss_scale * lm_loss + self.rec_loss_scale * rec_loss   # (:92)
        out = {'total_loss': total_loss, 'lm_loss': lm_loss, 'rec_loss': rec_loss}
        if return_recon_image_embeds and has_image_output:
            out['recon_image_embeds'] = recon_image_embeds
        return out

    @torch.no_grad()
    def generate(self, tokenizer, prompt=None, input_ids=None, image_embeds=None, embeds_cmp_mask=None,
                 ids_cmp_mask=None, logits_processor=None, num_img_gen_tokens=64, temperature=0.7, num_beams=1,
                 max_new_tokens=120, top_p=0.5, past_key_values=None, dtype=torch.float16, device='cuda',
                 forced_tokens=None, do_sample=False, top_k=0, seed=None, repetition_penalty=1.0, no_repeat_ngram_size=0,
                 min_new_tokens=0, spare_img_ids=False, output_logprobs=False, top_logprobs=0, num_return_sequences=1,
                 length_penalty=1.0, early_stopping=False, prompt_lookup_num_tokens=None, max_matching_ngram_size=None):
        """``prompt_lookup_num_tokens=k`` / ``max_matching_ngram_size`` (Hugging Face's names) are handed to
        ``LlamaForCausalLM.generate``: prompt-lookup speculative steps in the greedy loop while ``llm.speculative`` is set, inert
        (and not passed on) otherwise.
        ``do_sample=False`` (the default, what the reference passes): greedy; ``temperature`` / ``top_p`` / ``top_k`` /
        ``seed`` are inert.  ``do_sample=True`` hands them to ``LlamaForCausalLM.generate``: on-device sampling
        (``top_k=0`` = off, ``seed=None`` = governed by ``torch.manual_seed``).  ``repetition_penalty`` /
        ``no_repeat_ngram_size`` / ``min_new_tokens`` (Hugging Face's defaults: inert) and ``spare_img_ids`` are handed on only
        when one of the three is active: they act on greedy search and on sampling (``LlamaForCausalLM.generate``).
        ``output_logprobs=True`` adds ``'logprobs'``, ``'model_logprobs'`` (float32, one entry per generated id) and
        ``'top_logprobs'`` = (ids, values) [n, top_logprobs] to the returned dict (``LlamaForCausalLM.generate``).
        ``num_return_sequences=n`` (> 1, with ``do_sample=True`` and ``llm.n_seq >= n``): best-of-n.  n candidates are sampled
        from the one prompt (``LlamaForCausalLM.generate``), each is scored with ``candidate_score`` (mean model
        log-probability of its free tokens; recording is switched on internally), the highest wins (ties: the lowest index),
        ``llm.select_candidate(best)`` makes its cache the one ``'past_key_values'`` returns, and the dict is the winner's,
        plus ``'candidates'`` (the n dicts with ``'score'``, ``'text'``, ``'generate_ids'``, ``'has_img_output'``,
        ``'img_gen_feat'``) and ``'best'``.  The output resampler runs once, on the stacked rows of every candidate that
        produced an image.
        ``num_beams=n`` (> 1, ``do_sample=False``) with ``llm.beam_search = True`` and ``llm.n_seq >= n``: the free tokens come
        from a beam search on the device (``LlamaForCausalLM.generate``); ``length_penalty`` / ``early_stopping`` (Hugging
        Face's defaults 1.0 / False) are handed on only when one of them is set, and the dict gains ``'sequences_scores'``
        (the winner's score) and ``'beams'`` (the n hypotheses).  While ``llm.beam_search`` is False ``num_beams`` is inert."""
        if logits_processor is None:
            logits_processor = LogitsProcessorList()
            logits_processor.append(
                AutoImageTokenGenerationProcessor(tokenizer=tokenizer, num_img_gen_tokens=num_img_gen_tokens))
        if prompt is not None:
            input_ids = tokenizer(prompt, return_tensors="pt").input_ids
        if isinstance(input_ids, list):
            input_ids = torch.tensor(input_ids)
        embed = self.llm.get_input_embeddings()
        dev = embed.weight.device
        input_ids = input_ids.to(device=dev)
        input_embeds = embed(input_ids)                                   # [1, S, H]   (:127)
        bz, sq, dim = input_embeds.shape
        assert bz == 1, "the story path is batch 1"
        if image_embeds is not None:
            assert embeds_cmp_mask is not None and ids_cmp_mask is not None
            image_embeds_lm = self.input_resampler(image_embeds.to(dev))  # [Nimg, 64, H] (:133)
            sel = image_embeds_lm[embeds_cmp_mask.to(dev)].reshape(-1, dim).contiguous()
            idx = torch.nonzero(ids_cmp_mask[0].to(dev), as_tuple=False).flatten()
            assert idx.numel() == sel.shape[0], "ids_cmp_mask / embeds_cmp_mask disagree"
            ops.scatter_rows_(input_embeds.view(-1, dim), idx, sel)       # (:135)

        rules = {}
        if repetition_penalty not in (None, 1.0) or no_repeat_ngram_size not in (None, 0) or min_new_tokens not in (None, 0):
            rules = dict(repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                         min_new_tokens=min_new_tokens, spare_img_ids=spare_img_ids)
        n_ret = 1 if num_return_sequences is None else int(num_return_sequences)
        want_lp = bool(output_logprobs) or n_ret > 1
        output = self.llm.generate(input_ids=input_ids, inputs_embeds=input_embeds, output_hidden_states=True,
                                   return_dict_in_generate=True, logits_processor=logits_processor,
                                   past_key_values=past_key_values, max_new_tokens=max_new_tokens,
                                   temperature=temperature, num_beams=num_beams, top_p=top_p, do_sample=do_sample,
                                   forced_tokens=forced_tokens, **({"top_k": top_k, "seed": seed} if do_sample else {}), **rules,
                                   **({"output_logprobs": True, "top_logprobs": top_logprobs} if want_lp else {}),
                                   **({"num_return_sequences": n_ret} if n_ret > 1 else {}),
                                   **({"length_penalty": length_penalty, "early_stopping": early_stopping}
                                      if (length_penalty not in (None, 1.0) or early_stopping not in (None, False)) else {}),
                                   **({"prompt_lookup_num_tokens": prompt_lookup_num_tokens,
                                       "max_matching_ngram_size": max_matching_ngram_size} if prompt_lookup_num_tokens else {}))
        boi_token_id = tokenizer.encode(BOI_TOKEN, add_special_tokens=False)[0]
        eoi_token_id = tokenizer.encode(EOI_TOKEN, add_special_tokens=False)[0]
        if n_ret > 1:
            return self._best_of(tokenizer, output, input_ids, past_key_values, logits_processor, eoi_token_id,
                                 num_img_gen_tokens, bool(output_logprobs))
        output_past_key_values = self.llm.past_key_values
        generate_ids = output.sequences[0][input_ids.shape[1]:]
        img_gen_feats = self._img_rows(output, input_ids, past_key_values, eoi_token_id, num_img_gen_tokens)
        num_gen_imgs = 1 if img_gen_feats is not None else 0
        has_img_output = num_gen_imgs > 0
        img_gen_feat = self._regress(img_gen_feats) if has_img_output else None                     # (:205)
        generate_text = tokenizer.decode(generate_ids, skip_special_tokens=False)
        # one merged attention map per decoder layer when the LLM ran with config.output_attentions (:162-179): the reference
        # pads the running map with a NaN column per step and concatenates; here every step wrote its row into one NaN-filled
        # buffer, so the merged map is a slice of it
        attn_weights = ()
        if output.attentions is not None:
            attn_weights = tuple(output.attention_maps[l].unsqueeze(0) for l in range(output.attention_maps.shape[0]))
        scores = {}
        if output_logprobs:
            scores = {'logprobs': output.logprobs, 'model_logprobs': output.model_logprobs,
                      'top_logprobs': (output.top_logprob_ids, output.top_logprob_values)}
        if getattr(output, "beams", None) is not None:
            scores.update({'sequences_scores': output.sequences_scores, 'beams': output.beams})
        return {
            **scores,
            'text': generate_text,
            'generate_ids': generate_ids,
            'has_img_output': has_img_output,
            'img_gen_feat': img_gen_feat,
            'num_gen_imgs': num_gen_imgs,
            'attn_weights': attn_weights,
            'past_key_values': output_past_key_values
        }

    @staticmethod
    def _img_rows(output, input_ids, past_key_values, eoi_token_id, num_img_gen_tokens):
        """the ``num_img_gen_tokens`` last-layer rows in front of the last ``</img>`` of a batch-1 output ``[1, n, H]``
        (:182-197), or None when it produced no image"""
        generate_ids = output.sequences[0][input_ids.shape[1]:]
        last_hidden_states = torch.cat([hs[-1] for hs in output.hidden_states], dim=1)   # (:182)
        if past_key_values is None:
            last_hidden_states = last_hidden_states[0, input_ids.shape[1]:, :]
            eoi_indices = torch.where(generate_ids == eoi_token_id)[0].tolist()
        else:
            last_hidden_states = last_hidden_states[0, :, :]
            hidden_len = last_hidden_states.shape[0]
            eoi_indices = torch.where(output.sequences[0][-hidden_len:] == eoi_token_id)[0].tolist()

        if not eoi_indices:
            return None
        e = eoi_indices[-1]
        return last_hidden_states[e - num_img_gen_tokens:e].unsqueeze(0).contiguous()               # (:197)

    def _best_of(self, tokenizer, output, input_ids, past_key_values, logits_processor, eoi_token_id, num_img_gen_tokens,
                 output_logprobs):
        """the dict of ``generate(num_return_sequences=n)``: the winner's, plus ``'candidates'`` and ``'best'``"""
        img_ids = ()
        for proc in (logits_processor or []):
            img_ids = tuple(getattr(proc, "img_ids_list", ()))
        S = input_ids.shape[1]
        cands, rows = [], []
        for c in output.candidates:
            gen = c.sequences[0][S:]
            r = self._img_rows(c, input_ids, past_key_values, eoi_token_id, num_img_gen_tokens)
            rows.append(r)
            d = {'score': candidate_score(gen, c.model_logprobs, img_ids[1:]),
                 'text': tokenizer.decode(gen, skip_special_tokens=False), 'generate_ids': gen,
                 'has_img_output': r is not None, 'img_gen_feat': None, 'num_gen_imgs': 1 if r is not None else 0}
            if output_logprobs:
                d.update({'logprobs': c.logprobs, 'model_logprobs': c.model_logprobs,
                          'top_logprobs': (c.top_logprob_ids, c.top_logprob_values)})
            cands.append(d)
        with_img = [i for i, r in enumerate(rows) if r is not None]
        if with_img:        # ONE pass of the output resampler over every candidate's image rows
            feats = self._regress(torch.cat([rows[i] for i in with_img], dim=0).contiguous())
            for j, i in enumerate(with_img):
                cands[i]['img_gen_feat'] = feats[j:j + 1]
        best = best_candidate([d['score'] for d in cands])
        self.llm.select_candidate(best)
        win = {k: v for k, v in cands[best].items() if k != 'score'}
        return {**win, 'attn_weights': (), 'past_key_values': self.llm.past_key_values, 'candidates': cands, 'best': best}

    @classmethod
    def from_pretrained(cls, llm, input_resampler, output_resampler, pretrained_model_path=None, **kwargs):
        model = cls(llm=llm, input_resampler=input_resampler, output_resampler=output_resampler, **kwargs)
        if pretrained_model_path is not None:
            from seedstory import ckpt as _ckpt
            _ckpt.load_checked(model, _ckpt.read_weights(pretrained_model_path), 'agent model,')
        return model

"""Host side of the slot fork and of best-of-n (no GPU): the C ABI declares and exports ``ss_llama_fork``; ``candidate_score``;
the plumbing of ``generate(num_return_sequences=n)`` through ``LlamaForCausalLM`` and ``ContinuousLVLM`` on stand-in engines."""
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG = list(range(3000, 3066))


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_exports_fork():
    from seedstory import _lib
    with open(os.path.join(ROOT, "include", "seedstory_hip.h")) as f:
        header = f.read()
    assert "int ss_llama_fork(ss_llama* h, int32_t src, const int32_t* host_dst, int32_t n_dst, void* stream);" in header
    assert "#define SS_ABI_VERSION 1" in header
    assert "ss_llama_fork" in _lib.PROTOTYPES
    lib = _lib.lib()
    assert lib.ss_llama_fork is not None and lib.ss_abi_version() == 1
    # refused without a handle, before anything touches a device
    assert lib.ss_llama_fork(None, 0, None, 1, None) == -1 and b"llama_fork" in lib.ss_last_error()


# ---- candidate_score -------------------------------------------------------------------------------------------------------------
def test_candidate_score():
    from src.models_clm.models import best_candidate, candidate_score
    forced = IMG[1:]
    # image ids excluded: <img> itself is the model's choice and counts, the 65 ids behind it do not
    ids = [5, 6, IMG[0]] + forced + [7]
    lps = [-1.0, -2.0, -3.0] + [-50.0] * 65 + [-6.0]
    assert candidate_score(ids, lps, forced) == pytest.approx((-1.0 - 2.0 - 3.0 - 6.0) / 4)
    assert candidate_score(torch.tensor(ids), torch.tensor(lps), forced) == pytest.approx(-3.0)
    assert candidate_score(ids, lps, ()) == pytest.approx(sum(lps) / len(lps))
    # nothing left: -inf
    assert candidate_score([], [], forced) == float("-inf")
    assert candidate_score(forced, [-1.0] * 65, forced) == float("-inf")
    assert candidate_score(torch.zeros(0, dtype=torch.long), torch.zeros(0), forced) == float("-inf")
    # the mean, not the sum: a longer candidate is not punished for its length
    assert candidate_score([1, 2, 3, 4], [-1.0] * 4, forced) == candidate_score([1], [-1.0], forced)
    # ties go to the lowest index, also when every score is -inf
    assert best_candidate([-2.0, -1.0, -1.0]) == 1 and best_candidate([-1.0, -1.0, -3.0]) == 0
    assert best_candidate([float("-inf")] * 3) == 0 and best_candidate([float("-inf"), -5.0]) == 1


# ---- stand-in engine -----------------------------------------------------------------------------------------------------------------
def _llm_and_engine(monkeypatch, n_seq=4, eos_slot=None):
    from test_host_cpu import _FakeDecodeEngine
    from seedstory import _lib, ops
    from src.models_clm.generation import AutoImageTokenGenerationProcessor
    from src.models_clm.modeling_llama_xformer import LlamaConfig, LlamaForCausalLM
    _lib.lib()
    monkeypatch.setattr(ops, "gather_rows", lambda table, ids: table[ids.long()])
    monkeypatch.setattr(ops, "gemm", lambda a, w, **kw: a @ w.t())

    def token_logprobs(logits, toks, top_n=0):          # the block tokens' model log-probability: -9 each
        lp = torch.full((len(toks),), -9.0)
        return (lp, torch.zeros(len(toks), top_n, dtype=torch.int32), torch.zeros(len(toks), top_n)) if top_n > 0 else lp
    monkeypatch.setattr(ops, "token_logprobs", token_logprobs)

    class Eng(_FakeDecodeEngine):
        """slots with a cache each (``fed``); under sampling the toy model's free tokens depend on the slot, as the Philox
        counter makes them; ``eos_slot`` ends that slot's run after three free tokens"""
        max_new = 512

        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.calls, self.sampling, self.rules, self.hist = [], None, None, {}
            self._cur, self._rules_slots, self._lp_slots = 0, set(), {}

        def select(self, b):
            self.cur = self._cur = int(b)
            return self

        def reset(self):
            self.fed[self.cur] = []

        def lengths(self):
            return (len(self.fed[self.cur]), len(self.fed[self.cur]))

        def set_lengths(self, kv, pos):
            self.fed[self.cur] = self.fed[self.cur][:kv]

        def past_key_values(self):
            return (self.cur, tuple(self.fed[self.cur]))

        def load_past_key_values(self, past):
            pass

        def fork(self, src=None, dsts=None):
            src = self.cur if src is None else src
            dsts = [b for b in range(self.n_seq) if b != src] if dsts is None else list(dsts)
            self.calls.append(("fork", src, dsts))
            for b in dsts:
                self.fed[b] = list(self.fed[src])
                if src in self.hist:
                    self.hist[b] = list(self.hist[src])
            return dsts

        def set_sampling(self, temperature=1.0, top_k=0, top_p=1.0, seed=0, slot=None):
            self.sampling = dict(temperature=temperature, top_k=top_k, top_p=top_p, seed=seed)
            self._free = [[] for _ in range(self.n_seq)]                             # (the draw counters restart)
            self.calls.append(("sampling", slot, dict(self.sampling)))

        def set_greedy(self, slot=None):
            self.sampling = None
            self.calls.append(("greedy", slot))

        def set_logits_rules(self, slot=None, **kw):
            self.rules = kw
            self._rules_slots = set(range(self.n_seq))
            self.calls.append(("rules", slot))

        def clear_logits_rules(self, slot=None):
            self.rules = None
            self._rules_slots = set()
            self.calls.append(("rules_off", slot))

        def set_history(self, ids, slot=None, append=False):
            b = self.cur if slot is None else slot
            self.hist[b] = (self.hist.get(b, []) if append else []) + list(ids)
            self.calls.append(("history", b, bool(append)))

        def set_logprobs(self, on=True, top_n=0, slot=None):
            self._lp_slots = {b: top_n for b in range(self.n_seq)} if on else {}
            self.calls.append(("logprobs", bool(on)))

        def logprobs(self, n, slot=None):
            b = self.cur if slot is None else slot
            k = self._lp_slots[b]
            base = -torch.arange(1, n + 1, dtype=torch.float32)
            return {"logprob": base.clone(), "model_logprob": base - 0.25 * b, "top_ids": torch.zeros(n, k, dtype=torch.int32),
                    "top_logprobs": torch.zeros(n, k)}

        def _next(self, b, last):
            t = super()._next(b, last)
            if self.sampling is None or last in self.img_ids[:-1]:
                return t
            if eos_slot == b and len(self._free[b]) >= 3:
                return self.eos_id
            self._free[b].append(t)
            return 3 + (t + 11 * b) % 200 if t not in self.img_ids else t

        def generate_batch(self, n_steps, lasts, forced=None, active=None):
            self.calls.append(("generate_batch", None if active is None else [bool(a) for a in active]))
            return super().generate_batch(n_steps, lasts, forced, active)

        def generate(self, n_steps, last_prompt_id, forced=None):
            self.calls.append(("generate", self.cur))
            return super().generate(n_steps, last_prompt_id, forced)

    class Tok:
        def encode(self, s, add_special_tokens=False):
            return list(IMG)

    m = LlamaForCausalLM(LlamaConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=1, vocab_size=50))
    eng = Eng(IMG, n_seq=n_seq, max_rows=128)
    eng._free = [[] for _ in range(n_seq)]
    touched = []
    monkeypatch.setattr(m, "engine_for_generation", lambda ids, eng=eng: touched.append(1) or eng)
    m.use_kv_cache_head = False
    m.n_seq = n_seq
    ids = torch.tensor([[1, 40, 41, 42]])
    kw = dict(input_ids=ids, inputs_embeds=ids.float().unsqueeze(-1), logits_processor=[AutoImageTokenGenerationProcessor(tokenizer=Tok())])
    return m, eng, kw, touched


def _names(eng):
    return [c[0] for c in eng.calls]


# ---- LlamaForCausalLM ------------------------------------------------------------------------------------------------------------------
def test_defaults_hand_nothing_new_to_the_engine(monkeypatch):
    m, eng, kw, _ = _llm_and_engine(monkeypatch)
    a = m.generate(max_new_tokens=12, **kw)
    b = m.generate(max_new_tokens=12, num_return_sequences=1, **kw)
    c = m.generate(max_new_tokens=12, num_return_sequences=None, num_beams=4, **kw)
    assert a.sequences.tolist() == b.sequences.tolist() == c.sequences.tolist() and a.sequences.shape[0] == 1
    assert a.candidates is None and set(_names(eng)) == {"generate"}                 # no fork, no batch call, no select
    assert all(c == ("generate", 0) for c in eng.calls)
    with pytest.raises(ValueError):
        m.select_candidate(0)
    # do_sample with one sequence is the single path too
    eng.calls.clear()
    m.generate(max_new_tokens=12, do_sample=True, seed=3, **kw)
    assert _names(eng) == ["sampling", "generate", "greedy"]


def test_n_seq_reaches_the_engine_only_above_one(monkeypatch):
    from src.models_clm import modeling_llama_xformer as M
    built = []

    class P:
        is_cuda, _version, dtype, device = True, 0, torch.bfloat16, "cuda:0"

        def data_ptr(self):
            return 64

    class Holder:
        weight = P()

    monkeypatch.setattr(M, "LlamaEngine", lambda sd, **kw: built.append(kw) or object())
    m = M.LlamaForCausalLM(M.LlamaConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=1, vocab_size=50))
    m.__dict__["lm_head"] = Holder()
    assert m.n_seq == 1
    e1 = m.engine_for_generation(())
    assert len(built) == 1 and "n_seq" not in built[0]                                # stand-in engines without the argument construct
    assert m.engine_for_generation(()) is e1 and len(built) == 1
    m.n_seq = 4                                                                       # part of the signature: a new engine
    e4 = m.engine_for_generation(())
    assert e4 is not e1 and len(built) == 2 and built[1]["n_seq"] == 4
    assert m.engine_for_generation(()) is e4 and len(built) == 2


def test_refusals_come_before_any_engine_call(monkeypatch):
    m, eng, kw, touched = _llm_and_engine(monkeypatch)
    with pytest.raises(ValueError, match="do_sample"):
        m.generate(max_new_tokens=5, num_return_sequences=2, **kw)
    with pytest.raises(ValueError, match="n_seq"):
        m.generate(max_new_tokens=5, num_return_sequences=5, do_sample=True, **kw)
    m.n_seq = 1
    with pytest.raises(ValueError, match="n_seq"):
        m.generate(max_new_tokens=5, num_return_sequences=2, do_sample=True, **kw)
    m.n_seq = 4
    with pytest.raises(NotImplementedError):
        m.generate(max_new_tokens=5, num_return_sequences=2, do_sample=True, output_attentions=True, **kw)
    m.config.output_attentions = True
    with pytest.raises(NotImplementedError):
        m.generate(max_new_tokens=5, num_return_sequences=2, do_sample=True, **kw)
    assert not touched and not eng.calls


def test_candidates_flow_and_padded_layout(monkeypatch):
    monkeypatch.setenv("SEEDSTORY_IMG_BLOCK", "0")
    m, eng, kw, _ = _llm_and_engine(monkeypatch, eos_slot=1)
    S = kw["input_ids"].shape[1]
    out = m.generate(max_new_tokens=12, do_sample=True, seed=7, num_return_sequences=3, **kw)
    # one prefill on slot 0, one fork to the two lowest other slots, one lock-step call with slot 3 sitting out
    assert _names(eng) == ["sampling", "fork", "generate_batch", "greedy"]
    assert eng.calls[0][1] is None and eng.calls[0][2]["seed"] == 7                  # every slot, the one seed
    assert eng.calls[1] == ("fork", 0, [1, 2]) and eng.calls[2] == ("generate_batch", [True, True, True, False])
    assert eng.fed[3] == [] and eng._cur == 0
    lens = [c.sequences.shape[1] - S for c in out.candidates]
    assert lens[0] == 12 and lens[2] == 12 and lens[1] == 4                          # slot 1 met EOS after three free tokens
    assert tuple(out.sequences.shape) == (3, S + 12)
    for i, c in enumerate(out.candidates):
        assert c.sequences.shape[0] == 1 and out.sequences[i, :S + lens[i]].tolist() == c.sequences[0].tolist()
        assert c.sequences[0, :S].tolist() == kw["input_ids"][0].tolist() and len(c.hidden_states) == lens[i]
        assert c.logprobs is None and c.candidates is None
    assert out.sequences[1, S + 4:].tolist() == [2] * 8                              # pad_token_id is None: EOS pads
    assert out.candidates[1].sequences[0, -1] == 2
    assert len({tuple(c.sequences[0].tolist()) for c in out.candidates}) == 3
    assert out.hidden_states is out.candidates[0].hidden_states and out.attentions is None
    assert m.past_key_values[0] == 0                                                 # the source slot's cache
    # config.pad_token_id wins when it is set
    m.config.pad_token_id = 0
    out0 = m.generate(max_new_tokens=12, do_sample=True, seed=7, num_return_sequences=3, **kw)
    assert out0.sequences[1, S + 4:].tolist() == [0] * 8 and out0.sequences[0].tolist() == out.sequences[0].tolist()
    # select_candidate: the slot, the cache and (kv_cache_head in use) the head of the candidate picked
    for i in (2, 1, 0):
        assert m.select_candidate(i) == i and eng._cur == i and m.past_key_values[0] == i
        assert len(m.past_key_values[1]) == S + lens[i] - 1
    with pytest.raises(ValueError):
        m.select_candidate(3)
    # with past_key_values the selected slot is the source; the others follow in ascending order
    eng.calls.clear()
    eng.select(2)
    m.generate(max_new_tokens=6, do_sample=True, seed=7, num_return_sequences=3, past_key_values=m.past_key_values, **kw)
    assert ("fork", 2, [0, 1]) in eng.calls and eng._cur == 2 and m.past_key_values[0] == 2
    assert [c for c in eng.calls if c[0] == "generate_batch"][0][1] == [True, True, True, False]
    assert m.select_candidate(1) == 0 and m.select_candidate(2) == 1 and m.select_candidate(0) == 2


def test_kv_cache_head_follows_the_candidate(monkeypatch):
    monkeypatch.setenv("SEEDSTORY_IMG_BLOCK", "0")
    m, eng, kw, _ = _llm_and_engine(monkeypatch, eos_slot=2)
    m.use_kv_cache_head = True
    S = kw["input_ids"].shape[1]
    out = m.generate(max_new_tokens=9, do_sample=True, seed=1, num_return_sequences=3, **kw)
    lens = [c.sequences.shape[1] - S for c in out.candidates]
    assert lens == [9, 9, 4] and m.kv_cache_head == S + 8
    m.select_candidate(2)
    assert m.kv_cache_head == S + 3 == len(m.past_key_values[1])
    m.select_candidate(1)
    assert m.kv_cache_head == S + 8


def test_options_are_set_for_all_candidates_and_restored(monkeypatch):
    m, eng, kw, _ = _llm_and_engine(monkeypatch)
    forced = [5, IMG[0]]
    out = m.generate(max_new_tokens=72, do_sample=True, seed=7, num_return_sequences=4, forced_tokens=forced, repetition_penalty=1.3,
                     output_logprobs=True, top_logprobs=2, **kw)
    names = _names(eng)
    assert names[:4] == ["sampling", "logprobs", "rules", "history"] and names[-3:] == ["logprobs", "rules_off", "greedy"]
    assert eng.calls[3] == ("history", 0, False)                                     # the source's history, before the fork
    assert names.index("fork") > 3 and eng.calls[names.index("fork")] == ("fork", 0, [1, 2, 3])
    assert eng.sampling is None and eng.rules is None and not eng._lp_slots and not eng._rules_slots and eng.stop2 == -1
    S = kw["input_ids"].shape[1]
    for b, c in enumerate(out.candidates):                                            # forced tokens apply to every candidate
        g = c.sequences[0, S:].tolist()
        assert g[:2] == forced and g[2:67] == IMG[1:] and len(g) == 72
        assert c.logprobs.shape == c.model_logprobs.shape == (72,) and c.top_logprob_ids.shape == (72, 2)
        assert c.model_logprobs[0] == -1.0 - 0.25 * b and c.model_logprobs[2:67].tolist() == [-9.0] * 65
        assert eng.hist[b][:4] == kw["input_ids"][0].tolist() and eng.hist[b][4:] == IMG[1:]    # the block joined each slot's history
    assert out.logprobs is out.candidates[0].logprobs and out.model_logprobs is out.candidates[0].model_logprobs
    # an exception inside (the token-ring guard, after the prefill) restores everything too
    eng.calls.clear()
    with pytest.raises(ValueError):
        m.generate(max_new_tokens=513, do_sample=True, seed=7, num_return_sequences=2, no_repeat_ngram_size=3, output_logprobs=True, **kw)
    names = _names(eng)
    assert names[0] == "sampling" and names[-3:] == ["logprobs", "rules_off", "greedy"] and "fork" not in names
    assert eng.sampling is None and eng.rules is None and not eng._lp_slots


def test_generate_batch_img_block_active_mask(monkeypatch):
    """an inactive slot is never read, fed or written; None is every slot"""
    m, eng, kw, _ = _llm_and_engine(monkeypatch)
    for b in range(4):
        eng.select(b).prefill(torch.tensor([[1.0], [40.0 + b]]))
    fed3 = list(eng.fed[3])
    ids, hid = eng.generate_batch_img_block(80, [40, 41, 42, 43], forced=[[5, IMG[0]], [], [IMG[0]], [6, IMG[0]]], active=[1, 1, 1, 0])
    assert ids[3] == [] and hid[3] is None and eng.fed[3] == fed3 and eng._gen[3] == []
    assert all(c[1][3] is False for c in eng.calls if c[0] == "generate_batch")
    assert len(ids[0]) == 80 and ids[0][1:67] == IMG and hid[0].shape[0] == 79
    ref = _llm_and_engine(monkeypatch)[1]
    for b in range(4):
        ref.select(b).prefill(torch.tensor([[1.0], [40.0 + b]]))
    ids_all, hid_all = ref.generate_batch_img_block(80, [40, 41, 42, 43], forced=[[5, IMG[0]], [], [IMG[0]], [6, IMG[0]]])
    assert ids_all[:3] == ids[:3] and all(torch.equal(a, b) for a, b in zip(hid_all[:3], hid[:3])) and len(ids_all[3]) == 80
    # nobody active: nothing happens
    eng.calls.clear()
    ids0, hid0 = eng.generate_batch_img_block(10, [40, 41, 42, 43], active=[0, 0, 0, 0])
    assert ids0 == [[], [], [], []] and hid0 == [None] * 4 and not eng.calls


# ---- ContinuousLVLM -----------------------------------------------------------------------------------------------------------------------
def _agent(llm):
    from src.models_clm.models import ContinuousLVLM
    agent = ContinuousLVLM.__new__(ContinuousLVLM)
    torch.nn.Module.__init__(agent)
    agent.__dict__["llm"] = llm
    agent.__dict__["_regressor_fp32"] = None
    return agent


class _Tok:
    def encode(self, s, add_special_tokens=False):
        return [9]

    def decode(self, ids, skip_special_tokens=False):
        return " ".join(str(int(t)) for t in ids)


def test_continuous_lvlm_default_call_is_unchanged():
    seen = []

    class Out:
        sequences = torch.tensor([[1, 5, 6, 7]])
        hidden_states = ((torch.zeros(1, 2, 4),), (torch.zeros(1, 1, 4),), (torch.zeros(1, 1, 4),))
        attentions = None

    class LLM:
        past_key_values = None

        def get_input_embeddings(self):
            return torch.nn.Embedding(16, 4)

        def generate(self, **kw):
            seen.append(kw)
            return Out()

    agent = _agent(LLM())
    ids = torch.tensor([[1, 5]])
    out = agent.generate(_Tok(), input_ids=ids, logits_processor=[])
    agent.generate(_Tok(), input_ids=ids, logits_processor=[], num_return_sequences=1)
    agent.generate(_Tok(), input_ids=ids, logits_processor=[], num_return_sequences=None)
    for kw in seen:
        assert "num_return_sequences" not in kw and "output_logprobs" not in kw
    assert set(out) == {"text", "generate_ids", "has_img_output", "img_gen_feat", "num_gen_imgs", "attn_weights", "past_key_values"}


def test_continuous_lvlm_returns_the_best_candidate():
    from src.models_clm.modeling_llama_xformer import GenerateOutput
    seen, picked, regress = [], [], []
    S = 2

    def cand(gen, mlp):
        n = len(gen)
        hs = ((torch.zeros(1, S, 4),),) + tuple((torch.full((1, 1, 4), float(j)),) for j in range(1, n))
        return GenerateOutput(sequences=torch.tensor([[1, 5] + gen]), hidden_states=hs, attentions=None,
                              logprobs=torch.zeros(n), model_logprobs=torch.tensor(mlp), top_logprob_ids=torch.zeros(n, 0, dtype=torch.int32),
                              top_logprob_values=torch.zeros(n, 0))

    # id 9 = </img>; the processor's forced ids are 8 and 9 (img_ids_list[1:]): they do not count
    cands = [cand([3, 4, 6], [-3.0, -1.0, -2.0]),                        # mean -2
             cand([3, 7, 8, 9, 6], [-1.0, -1.0, -90.0, -90.0, -2.5]),     # mean -1.5 over three free tokens: the winner, with an image
             cand([4, 6], [-1.0, -2.0]),                                  # mean -1.5 as well: the tie goes to the lower index
             cand([7, 8, 9], [-4.0, -0.1, -0.1])]                         # mean -4, with an image

    class Proc:
        img_ids_list = [7, 8, 9]

    class LLM:
        past_key_values = "cache of the source"

        def get_input_embeddings(self):
            return torch.nn.Embedding(16, 4)

        def generate(self, **kw):
            seen.append(kw)
            return GenerateOutput(sequences=torch.zeros(4, 7, dtype=torch.long), hidden_states=cands[0].hidden_states, attentions=None,
                                  candidates=cands)

        def select_candidate(self, i):
            picked.append(i)
            self.past_key_values = "cache of candidate %d" % i

    agent = _agent(LLM())
    agent.__dict__["output_resampler"] = lambda rows: regress.append(tuple(rows.shape)) or rows.sum(dim=1, keepdim=True) + 100.0
    out = agent.generate(_Tok(), input_ids=torch.tensor([[1, 5]]), logits_processor=[Proc()], num_img_gen_tokens=2, do_sample=True,
                         seed=4, num_return_sequences=4)
    kw = seen[0]
    assert kw["num_return_sequences"] == 4 and kw["output_logprobs"] is True and kw["do_sample"] is True and kw["seed"] == 4
    assert [c["score"] for c in out["candidates"]] == pytest.approx([-2.0, -1.5, -1.5, -4.0])
    assert out["best"] == 1 and picked == [1] and out["past_key_values"] == "cache of candidate 1"
    win = out["candidates"][1]
    assert out["text"] == win["text"] == "3 7 8 9 6" and out["generate_ids"] is win["generate_ids"]
    assert out["has_img_output"] is True and out["img_gen_feat"] is win["img_gen_feat"] and out["num_gen_imgs"] == 1
    # one resampler pass over the two candidates with an image; each gets its own rows' result
    assert regress == [(2, 2, 4)]
    assert [c["has_img_output"] for c in out["candidates"]] == [False, True, False, True]
    assert out["candidates"][0]["img_gen_feat"] is None and out["candidates"][2]["img_gen_feat"] is None
    # candidate 1: </img> is generated id 3, the two rows in front of it hold 2 and 3 (row k of the generated part holds k + 1)
    assert win["img_gen_feat"].shape == (1, 1, 4) and win["img_gen_feat"].flatten().tolist() == [105.0] * 4
    assert out["candidates"][3]["img_gen_feat"].flatten().tolist() == [103.0] * 4
    # log-probabilities were switched on internally: the caller did not ask for them, so the dicts do not carry them
    assert "model_logprobs" not in out and all("model_logprobs" not in c for c in out["candidates"])
    asked = agent.generate(_Tok(), input_ids=torch.tensor([[1, 5]]), logits_processor=[Proc()], num_img_gen_tokens=2, do_sample=True,
                           seed=4, num_return_sequences=4, output_logprobs=True)
    assert asked["model_logprobs"] is cands[1].model_logprobs and all("model_logprobs" in c for c in asked["candidates"])


# ---- drivers ---------------------------------------------------------------------------------------------------------------------------
def test_best_of_driver_arguments():
    import argparse
    from src.inference.gen_george import add_best_of_argument, apply_best_of, report_candidates, sample_kwargs
    ap = argparse.ArgumentParser()
    add_best_of_argument(ap)
    ap.add_argument("--sample", action="store_true")
    ap.add_argument("--temperature", type=float, default=0.7)
    ap.add_argument("--top-k", type=int, default=0)
    ap.add_argument("--top-p", type=float, default=0.5)
    ap.add_argument("--seed", type=int, default=None)

    class Llama:
        n_seq = 1
    plain = ap.parse_args([])
    assert plain.best_of == 1 and sample_kwargs(plain, 0, 1) == {}                   # the default call is unchanged
    llama = Llama()
    apply_best_of(plain, llama)
    assert llama.n_seq == 1
    assert "num_return_sequences" not in sample_kwargs(ap.parse_args(["--sample"]), 0, 1)
    args = ap.parse_args(["--best-of", "4", "--seed", "5"])                          # implies --sample
    kw = sample_kwargs(args, 2, 3)
    assert kw == dict(do_sample=True, temperature=0.7, top_k=0, top_p=0.5, seed=5 + 100003 * 2 + 3, num_return_sequences=4)
    apply_best_of(args, llama)
    assert llama.n_seq == 4
    with pytest.raises(SystemExit):
        apply_best_of(ap.parse_args(["--best-of", "9"]), llama)
    report_candidates(args, 0, 1, {"text": "x"})                                     # no candidates: prints nothing

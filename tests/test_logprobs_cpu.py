"""Token log-probabilities, the CPU side: the error allowance of the kernels, the fp64 reference (tests/logprobs_ref.py)
against torch and against the sampler's oracle, the C ABI surface, and the host plumbing of ``output_logprobs`` driven with
stand-in engines."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

import logprobs_ref as R
from test_sampling_cpu import DELTA, U32, oracle, processor_edit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the error allowance of a log-probability ----------------------------------------------------------------------------------
# u32 = 2^-24 is the unit roundoff of fp32; expf and logf are good to 1 ulp = 2 u32 (as in tests/test_sampling_cpu.py).
# Plain form, lp = (v - m) - logf(S), S = sum expf(z_i - m) >= 1 (the maximum's term is exactly 1), log S <= log 65535 < 11.1:
#   d = v - m rounds once: u32 |d|, and |d| = |lp + log S| <= |lp| + 11.1;
#   S: per thread at most 64 terms added one after the other, 6 levels of the wave butterfly, 4 levels over the 16 wave sums:
#     74 u32 relative, whatever the values (non-negative terms).  Each term is expf of x = z_i - m, rounded once, so the term is
#     off by a relative u32 |x|: terms with |x| <= 16 contribute at most 16 u32 of S, the rest (each below e^-16, at most 65535
#     of them, x e^-x decreasing) less than 1 u32; expf itself 2 u32.  Together 93 u32, and log(1 + e) <= 1.0001 e for these e;
#   logf(S): 2 u32 |log S| <= 22.2 u32;
#   the last subtraction rounds once: u32 |lp|.
#   Sum: (11.1 + 93.01 + 22.2) u32 + 2 u32 |lp|, rounded up to  LP_A + LP_B |lp|  with LP_A = 127 u32, LP_B = 2 u32.
# Sampling form, lp = x - logf(Z_P), x = (z_tok - z_max) * (1 / T), Z_P >= 1 (the arg max is always kept), log Z_P < 11.1:
#   x: the subtraction, the reciprocal and the product round once each: 3 u32 |x| <= 3 u32 (|lp| + 11.1);
#   Z_P: the sampler's mass, DELTA without its 3 u32 for the top-p threshold: 125 u32 relative (the scan that sums it is
#     shallower than a mass; tests/test_sampling_cpu.py);
#   logf and the last subtraction as above.
#   Sum: (33.3 + 125.02 + 22.2) u32 + 4 u32 |lp|, rounded up to  LPS_A + LPS_B |lp|  with LPS_A = 181 u32, LPS_B = 4 u32.
# The sampling form is compared only where the oracle reports the kept set as decided at DELTA.
LP_A, LP_B = 127 * U32, 2 * U32
LPS_A, LPS_B = 181 * U32, 4 * U32
assert 11.1 + 93 * 1.0001 + 22.2 <= 127 and 3 * 11.1 + (DELTA / U32 - 3) * 1.0001 + 22.2 <= 181 and math.log(65535) < 11.1


# ---- the reference -------------------------------------------------------------------------------------------------------------
def test_reference_equals_torch_log_softmax_on_finite_rows():
    g = torch.Generator().manual_seed(3)
    for vocab in (7, 1003, 32066):
        z = torch.randn(3, vocab, generator=g, dtype=torch.float64) * 4.0
        want = torch.log_softmax(z, dim=-1).numpy()
        for r in range(3):
            got = R.log_softmax(z[r].numpy())
            assert np.allclose(got, want[r], rtol=0, atol=1e-12), vocab
            ids, lps = R.top_n(z[r].numpy(), 5)
            tv, ti = torch.topk(z[r], 5)
            assert ids.tolist() == ti.tolist() and np.allclose(lps, want[r][ti.numpy()], rtol=0, atol=1e-12)
            assert R.model_logprob(z[r].numpy(), 4) == got[4] and R.policy_logprob(z[r].numpy(), 4)[0] == got[4]


def test_reference_definition_cases():
    inf, nan = np.inf, np.nan
    assert R.log_softmax([-inf, 2.5, -inf]).tolist() == [-inf, 0.0, -inf]                  # one entry with mass: exactly 0
    assert np.allclose(R.log_softmax(np.full(9, 1.5)), -math.log(9), rtol=0, atol=1e-15)
    got = R.log_softmax([1.0, nan, 1.0, -inf])
    assert got[0] == got[2] == -math.log(2) and np.isnan(got[1]) and got[3] == -inf        # NaN carries no mass and stays NaN
    none = R.log_softmax([-inf, nan])
    assert none[0] == -inf and np.isnan(none[1])                                           # a row without mass: by the entry alone
    big = R.log_softmax(np.array([3.4e38, -3.4e38, 3.4e38]))
    assert not np.isnan(big).any() and big[0] == -math.log(2) and big[1] < -6e38
    ids, lps = R.top_n([1.0, 3.0, nan, 3.0, -inf, 2.0], 5)                                 # ties by ascending id; 4 entries with mass
    assert ids.tolist() == [1, 3, 5, 0, -1] and lps[4] == -inf and lps[0] == lps[1] > lps[2] > lps[3]
    assert R.top_n([nan, -inf], 2)[0].tolist() == [-1, -1]


@pytest.mark.parametrize("T,top_k,top_p", [(0.7, 0, 0.5), (1.0, 50, 0.9), (1.3, 0, 1.0), (0.9, 5, 1.0)])
def test_reference_sampling_form_is_the_oracles_probability(T, top_k, top_p):
    g = torch.Generator().manual_seed(29)
    sp = dict(temperature=T, top_k=top_k, top_p=top_p)
    for vocab in (64, 1003):
        z = (torch.randn(vocab, generator=g) * 4.0).to(torch.bfloat16).double().numpy()
        o = oracle(z, T, top_k, top_p, u=0.3)
        for tok in list(np.flatnonzero(o["kept"])[:6]) + list(np.flatnonzero(~o["kept"])[:3]):
            lp, decided = R.policy_logprob(z, int(tok), sp)
            assert decided == o["decided"]
            assert math.isclose(math.exp(lp), o["prob"][tok], rel_tol=1e-12, abs_tol=0.0) if o["kept"][tok] else lp == -np.inf
    assert R.policy_logprob([np.nan, -np.inf], 0, sp)[0] == -np.inf


def test_within_applies_the_bound():
    assert R.within(-1.0 - 1e-7, -1.0, LP_A, LP_B) and not R.within(-1.0 - 1e-4, -1.0, LP_A, LP_B)
    assert R.within(float("nan"), float("nan"), LP_A, LP_B) and not R.within(float("nan"), -1.0, LP_A, LP_B)
    assert R.within(-np.inf, -np.inf, LP_A, LP_B) and not R.within(-1e30, -np.inf, LP_A, LP_B) and not R.within(-np.inf, -1e30, LP_A, LP_B)
    assert R.within(-np.inf, -6.8e38, LP_A, LP_B)                     # beyond the fp32 range: its fp32 value
    assert LP_A < 1e-5 and LPS_A < 2e-5                               # the allowance is a few 1e-6, not a loose figure


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_logprob_symbols_declared_bound_exported():
    from seedstory import _lib
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "seedstory_hip.h")).read()
    declared = set(re.findall(r"\b(ss_[a-z0-9_]+)\s*\(", hdr))
    for name in ("ss_token_logprobs", "ss_llama_set_logprobs"):
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert len(_lib.PROTOTYPES["ss_token_logprobs"][1]) == 12 and len(_lib.PROTOTYPES["ss_llama_set_logprobs"][1]) == 7


def test_c_abi_refuses_bad_parameters_before_any_launch():
    """SS_EINVAL for every parameter outside its range, checked on the host before anything is launched or written (the
    pointers are never dereferenced, so no GPU is needed)."""
    from seedstory import _lib, ops
    lib = _lib.lib()
    buf = (C.c_float * 64)()
    a = C.addressof(buf)

    def call(logits=a, rows=1, vocab=64, ld=64, ids=a, sp=None, top_n=0, lp=a, tid=None, tlp=None, dtype=_lib.SS_F32):
        return lib.ss_token_logprobs(logits, rows, vocab, ld, ids, C.byref(sp) if sp is not None else None, top_n, lp, tid, tlp, dtype, None)
    S = _lib.Sampling
    bad = [dict(logits=None), dict(ids=None), dict(lp=None), dict(rows=0), dict(vocab=0), dict(vocab=65536, ld=65536), dict(ld=63),
           dict(top_n=-1), dict(top_n=9, tid=a, tlp=a), dict(top_n=3), dict(top_n=3, tid=a), dict(top_n=3, tlp=a), dict(dtype=7),
           dict(sp=S(0.0, 1.0, 0, 0)), dict(sp=S(1.0, 0.0, 0, 0)), dict(sp=S(1.0, 1.5, 0, 0)), dict(sp=S(1.0, 1.0, -1, 0)),
           dict(sp=S(float("nan"), 1.0, 0, 0))]
    for kw in bad:
        assert call(**kw) == -1, kw
        assert lib.ss_last_error()
    # the engine entry point: top_n and the set of buffers are checked before the handle is looked at
    for args, word in (((a, a, None, None, 9), b"top_n"), ((a, a, None, None, -1), b"top_n"), ((a, None, None, None, 0), b"NULL"),
                       ((None, a, None, None, 0), b"NULL"), ((a, a, a, None, 3), b"top-n"), ((a, a, None, a, 3), b"top-n"),
                       ((a, a, None, None, 3), b"top-n"), ((a, a, a, a, 0), b"top-n"), ((None, None, a, a, 2), b"NULL"),
                       ((a, a, None, None, 0), b"null handle"), ((None, None, None, None, 0), b"null handle")):
        assert lib.ss_llama_set_logprobs(None, 0, *args) == -1, args
        assert word in lib.ss_last_error(), (args, lib.ss_last_error())
    with pytest.raises(_lib.SSError):
        ops.token_logprobs(torch.zeros(2, 64), [1, 2])                 # no CPU path


# ---- host plumbing with stand-in engines ---------------------------------------------------------------------------------------
IMG = list(range(3000, 3066))


def _engine_classes():
    from test_host_cpu import _FakeDecodeEngine
    from seedstory import _lib

    class Eng(_FakeDecodeEngine):
        max_new = 512

        def reset(self):
            self.fed[0] = []

        def lengths(self):
            return (len(self.fed[0]), len(self.fed[0]))

        def set_lengths(self, kv, pos):
            self.fed[0] = self.fed[0][:kv]

        def past_key_values(self):
            return tuple(self.fed[0])

    class LpEng(Eng):
        """records the calls; the loop's entry i of slot b is (-(i + 1), -(i + 1) - 0.5), its top ids are the token itself"""

        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.calls, self._lp_slots, self._cur = [], {}, 0

        def select(self, b):
            self._cur = b
            return super().select(b)

        def set_logprobs(self, on=True, top_n=0, slot=None):
            if on and not 0 <= top_n <= 8:
                raise _lib.SSError("top_n")
            self.calls.append(("logprobs", bool(on), top_n if on else 0))
            slots = range(self.n_seq) if slot is None else [slot]
            for b in slots:
                if on:
                    self._lp_slots[b] = top_n
                else:
                    self._lp_slots.pop(b, None)

        def logprobs(self, n, slot=None):
            b = self._cur if slot is None else slot
            k = self._lp_slots[b]
            i = torch.arange(1, n + 1, dtype=torch.float32)
            g = torch.tensor(self._gen[b][:n], dtype=torch.int32).view(n, 1)
            return {"logprob": -i, "model_logprob": -i - 0.5, "top_ids": g.expand(n, k).contiguous(), "top_logprobs": torch.zeros(n, k)}

        def generate(self, n_steps, last_prompt_id, forced=None):
            self.calls.append(("generate", dict(self._lp_slots)))
            return super().generate(n_steps, last_prompt_id, forced)
    return Eng, LpEng


def _patch_ops(monkeypatch, seen):
    from seedstory import _lib, ops
    _lib.lib()
    monkeypatch.setattr(ops, "gather_rows", lambda table, ids: table[ids.long()])
    monkeypatch.setattr(ops, "gemm", lambda a, w, **kw: a @ w.t())

    def token_logprobs(logits, ids, sampling=None, top_n=0):
        seen.append((logits.clone(), list(ids), sampling, top_n))
        lp = -100.0 - torch.arange(len(ids), dtype=torch.float32)
        return (lp, torch.tensor(ids, dtype=torch.int32).view(-1, 1).expand(-1, top_n).contiguous(), torch.ones(len(ids), top_n)) if top_n else lp
    monkeypatch.setattr(ops, "token_logprobs", token_logprobs)


def _llm(monkeypatch, eng):
    from src.models_clm.generation import AutoImageTokenGenerationProcessor
    from src.models_clm.modeling_llama_xformer import LlamaConfig, LlamaForCausalLM

    class Tok:
        def encode(self, s, add_special_tokens=False):
            return list(IMG)

    m = LlamaForCausalLM(LlamaConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=1, vocab_size=50))
    monkeypatch.setattr(m, "engine_for_generation", lambda ids, eng=eng: eng)
    m.use_kv_cache_head = False
    ids = torch.tensor([[1, 40, 41, 42]])
    return m, dict(input_ids=ids, inputs_embeds=ids.float().unsqueeze(-1), logits_processor=[AutoImageTokenGenerationProcessor(tokenizer=Tok())])


def test_default_arguments_call_nothing_new(monkeypatch):
    monkeypatch.setenv("SEEDSTORY_IMG_BLOCK", "0")
    seen = []
    _patch_ops(monkeypatch, seen)
    Eng, LpEng = _engine_classes()
    m, kw = _llm(monkeypatch, Eng(IMG))                        # this stand-in HAS no set_logprobs / logprobs
    out = m.generate(max_new_tokens=12, **kw)
    assert (out.logprobs, out.model_logprobs, out.top_logprob_ids, out.top_logprob_values) == (None, None, None, None)
    same = m.generate(max_new_tokens=12, output_logprobs=False, top_logprobs=3, output_scores=True, **kw)     # top_logprobs alone is inert
    assert same.sequences.tolist() == out.sequences.tolist() and same.logprobs is None
    eng = LpEng(IMG)
    m2, kw2 = _llm(monkeypatch, eng)
    m2.generate(max_new_tokens=12, **kw2)
    assert [c[0] for c in eng.calls] == ["generate"] and not seen
    monkeypatch.setenv("SEEDSTORY_IMG_BLOCK", "1")             # the block path as well
    eng.calls.clear()
    m2.generate(max_new_tokens=200, **kw2)
    assert {c[0] for c in eng.calls} == {"generate"} and not seen and eng.last_logprobs is None


def test_output_logprobs_sets_and_clears_the_feature(monkeypatch):
    from seedstory import _lib
    monkeypatch.setenv("SEEDSTORY_IMG_BLOCK", "0")
    seen = []
    _patch_ops(monkeypatch, seen)
    _, LpEng = _engine_classes()
    eng = LpEng(IMG)
    m, kw = _llm(monkeypatch, eng)
    out = m.generate(max_new_tokens=12, output_logprobs=True, top_logprobs=3, **kw)
    assert eng.calls == [("logprobs", True, 3), ("generate", {0: 3}), ("logprobs", False, 0)] and eng._lp_slots == {}
    n = out.sequences.shape[1] - 4
    assert n == 12 and out.logprobs.tolist() == [-(i + 1.0) for i in range(n)] and out.model_logprobs.tolist() == [-(i + 1.5) for i in range(n)]
    assert out.top_logprob_ids.shape == (n, 3) and out.top_logprob_values.shape == (n, 3)
    assert out.top_logprob_ids[:, 0].tolist() == out.sequences[0, 4:].tolist()
    assert out.logprobs.dtype == out.model_logprobs.dtype == out.top_logprob_values.dtype == torch.float32
    # top_logprobs = 0: the fields are there, the top-n ones empty
    out0 = m.generate(max_new_tokens=5, output_logprobs=True, **kw)
    assert out0.logprobs.shape == (5,) and out0.top_logprob_ids.shape == (5, 0)
    # an exception inside _generate (the token-ring guard) still clears it; so does a refused top_n
    eng.calls.clear()
    with pytest.raises(ValueError):
        m.generate(max_new_tokens=513, output_logprobs=True, **kw)
    assert eng.calls[0] == ("logprobs", True, 0) and eng.calls[-1] == ("logprobs", False, 0) and eng._lp_slots == {}
    eng.calls.clear()
    with pytest.raises(_lib.SSError):
        m.generate(max_new_tokens=5, output_logprobs=True, top_logprobs=9, **kw)
    assert eng.calls == [("logprobs", False, 0)] and eng._lp_slots == {}


def test_block_tokens_get_zero_logprob_and_the_right_logits_row(monkeypatch):
    """The block path: the loop's segments come from ``logprobs``, the block's from ``ops.token_logprobs`` on
    lm_head(hidden rows) — row i (the row of fed token blk[i]) scores blk[i + 1] — with ``logprob`` 0.0; the assembled call
    lines up with the ids, whatever the ``img_block_logits`` knob says."""
    from seedstory import _lib
    seen = []
    _patch_ops(monkeypatch, seen)
    monkeypatch.setattr(_lib, "get_tuning", lambda k, d=0: 0 if k == "img_block_logits" else (1 if k == "img_block_decode" else d))
    _, LpEng = _engine_classes()
    eng = LpEng(IMG)
    eng.lm_head = torch.eye(2)                                 # logits row = the hidden row = [position, fed token]
    eng.set_logprobs(True, top_n=2)
    eng.prefill(torch.tensor([[1.0], [40.0]]))
    ids, hid = eng.generate_img_block(3 + 65 + 4, 40, forced=[7, 8, IMG[0]] + IMG[1:] + [9, 10, 11, 12])
    lp = eng.last_logprobs
    i0 = ids.index(IMG[0])
    assert i0 == 2 and ids[i0:i0 + 66] == IMG and ids[i0 + 66:] == [9, 10, 11, 12]
    assert {k: tuple(v.shape) for k, v in lp.items()} == {"logprob": (len(ids),), "model_logprob": (len(ids),), "top_ids": (len(ids), 2),
                                                          "top_logprobs": (len(ids), 2)}
    assert len(seen) == 1
    logits, toks, sampling, top_n = seen[0]
    assert toks == IMG[1:] and sampling is None and top_n == 2
    assert logits.shape == (65, 2) and logits[:, 1].tolist() == [float(t) for t in IMG[:65]]      # row i: fed blk[i], scores blk[i + 1]
    blk = slice(i0 + 1, i0 + 66)
    assert lp["logprob"][blk].tolist() == [0.0] * 65
    assert lp["model_logprob"][blk].tolist() == [-100.0 - i for i in range(65)] and lp["top_ids"][blk, 0].tolist() == IMG[1:]
    assert lp["logprob"][:i0 + 1].tolist() == [-1.0, -2.0, -3.0] and lp["logprob"][i0 + 66] == -1.0   # loop segments: their own entries
    assert lp["top_ids"][:, 0].tolist() == ids
    # the budget ends inside the block: m block tokens, rows 0 .. m - 1
    seen.clear()
    eng.reset()
    ids2, _ = eng.generate_img_block(3 + 10, 40, forced=[7, 8, IMG[0]])
    assert ids2 == [7, 8] + IMG[:11] and seen[0][1] == IMG[1:11] and seen[0][0][:, 1].tolist() == [float(t) for t in IMG[:10]]
    assert eng.last_logprobs["logprob"].tolist() == [-1.0, -2.0, -3.0] + [0.0] * 10
    # feature off again: nothing is assembled and the operator is not called
    seen.clear()
    eng.set_logprobs(False)
    eng.reset()
    eng.generate_img_block(100, 40, forced=[7, 8, IMG[0]])
    assert eng.last_logprobs is None and not seen


def test_batch_block_path_assembles_per_slot(monkeypatch):
    seen = []
    _patch_ops(monkeypatch, seen)
    _, LpEng = _engine_classes()
    eng = LpEng(IMG, n_seq=2, max_rows=128)
    eng.lm_head = torch.eye(2)
    eng.set_logprobs(True, top_n=1, slot=1)                    # slot 0 records nothing
    ids, _ = eng.generate_batch_img_block(90, [40, 41], forced=[[5, IMG[0]], [IMG[0]]])
    lp = eng.last_logprobs
    assert lp[0] is None and lp[1]["logprob"].shape == (len(ids[1]),) and lp[1]["top_ids"][:, 0].tolist() == ids[1]
    assert ids[1][:66] == IMG and lp[1]["logprob"][1:66].tolist() == [0.0] * 65 and lp[1]["logprob"][0] == -1.0
    # slot 0's blocks are not scored; slot 1's first block is whole (a later one may be cut short by the budget)
    assert all(s[3] == 1 and s[1] == IMG[1:len(s[1]) + 1] and s[0][:, 1].tolist() == [float(t) for t in IMG[:len(s[1])]] for s in seen)
    assert seen[0][1] == IMG[1:] and sum(len(s[1]) for s in seen) == int((lp[1]["logprob"] == 0.0).sum())


def test_continuous_lvlm_forwards_and_adds_keys_only_when_asked():
    from src.models_clm.models import ContinuousLVLM
    seen = []

    class Out:
        sequences = torch.tensor([[1, 5, 6, 7]])
        hidden_states = ((torch.zeros(1, 2, 4),), (torch.zeros(1, 1, 4),), (torch.zeros(1, 1, 4),))
        attentions = None
        logprobs, model_logprobs = torch.tensor([-1.0, -2.0]), torch.tensor([-3.0, -4.0])
        top_logprob_ids, top_logprob_values = torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 3)

    class LLM:
        past_key_values = None

        def get_input_embeddings(self):
            return torch.nn.Embedding(16, 4)

        def generate(self, **kw):
            seen.append(kw)
            return Out()

    class Tok:
        def encode(self, s, add_special_tokens=False):
            return [9]

        def decode(self, ids, skip_special_tokens=False):
            return "x"

    agent = ContinuousLVLM.__new__(ContinuousLVLM)
    torch.nn.Module.__init__(agent)
    agent.__dict__["llm"] = LLM()
    ids = torch.tensor([[1, 5]])
    plain = agent.generate(Tok(), input_ids=ids, logits_processor=[])
    asked = agent.generate(Tok(), input_ids=ids, logits_processor=[], output_logprobs=True, top_logprobs=3)
    assert set(plain) == {"text", "generate_ids", "has_img_output", "img_gen_feat", "num_gen_imgs", "attn_weights", "past_key_values"}
    assert "output_logprobs" not in seen[0] and "top_logprobs" not in seen[0]
    assert seen[1]["output_logprobs"] is True and seen[1]["top_logprobs"] == 3
    assert set(asked) - set(plain) == {"logprobs", "model_logprobs", "top_logprobs"}
    assert asked["logprobs"] is Out.logprobs and asked["model_logprobs"] is Out.model_logprobs
    assert asked["top_logprobs"][0] is Out.top_logprob_ids and asked["top_logprobs"][1] is Out.top_logprob_values

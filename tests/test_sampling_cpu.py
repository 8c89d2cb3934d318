"""On-device sampling, the CPU side: the C ABI surface, the ORACLE of the sampler (an fp64 restatement of the definition in
include/seedstory_hip.h, `ss_sample_logits`, plus a numpy Philox4x32-10; tests/test_sampling_gpu.py imports it), and the host
plumbing of ``do_sample`` driven with stand-in engines."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the error allowance of the kernel's fp32 masses -------------------------------------------------------------------------
# u32 = 2^-24 is the unit roundoff of fp32.  A mass of the kernel is a sum of non-negative fp32 weights: per thread at most 64
# terms added one after the other, then 6 levels of the wave butterfly and 4 levels over the 16 wave sums: a relative error of
# (64 + 6 + 4) u32 at most, whatever the values (every partial sum is below the total).  Each weight is expf of
# x = (z - z_max) * (1 / T): the subtraction, the reciprocal and the product round once each, so x is off by 3 u32 |x| and the
# weight by a relative 3 u32 |x|; weights with |x| <= 16 contribute at most 48 u32 of the mass, and the rest (each below e^-16,
# at most 65535 of them, x e^-x decreasing) at most 65535 * 16 e^-16 * 3 u32 < 1 u32.  expf itself is good to 1 ulp = 2 u32.
# The threshold top_p * Z_k is one more product and the comparison sees both roundings: 3 u32.  The index-ordered scan behind the
# draw is shallower than a mass (4 + 6 levels for the prefix of the wave sums, 6 for the lane scan, at most 8 inside a run).
# Total: 74 + 48 + 1 + 2 + 3 = 128 u32 = 2^-17 ~ 7.6e-6.
U32 = 2.0 ** -24
DELTA = (64 + 6 + 4 + 48 + 1 + 2 + 3) * U32
assert DELTA == 2.0 ** -17


# ---- Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) ---------------------------
def philox4x32_10(counter, key):
    """counter: 4 words, key: 2 words (each a Python int or an array of uint32, broadcast together) -> 4 arrays of uint32"""
    c = [np.asarray(v, dtype=np.uint64) & 0xFFFFFFFF for v in counter]
    k = [np.asarray(v, dtype=np.uint64) & 0xFFFFFFFF for v in key]
    for r in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]          # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return [v.astype(np.uint32) for v in c]


def philox_u(seed, draw, lane):
    """the engine's uniform: key = seed as (lo, hi), counter = (draw, lane, 0, 0), u = (out0 >> 8) * 2^-24 (float32, exact)"""
    seed = int(seed) & (2 ** 64 - 1)
    out0 = philox4x32_10((draw, lane, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))[0]
    return ((out0 >> 8).astype(np.float64) * 2.0 ** -24).astype(np.float32)


# ---- the oracle --------------------------------------------------------------------------------------------------------------
def processor_edit(row, last_id, img_ids):
    """AutoImageTokenGenerationProcessor on one row (a torch tensor of the model dtype), in place -> the successor id or -1"""
    ids = list(img_ids)
    if last_id in ids[:-1]:
        succ = ids[ids.index(last_id) + 1]
        row[succ] = (row.float().max() + 10.0).to(row.dtype)     # fp32 add, one rounding to the model dtype
        return succ
    if len(ids) > 1:
        row[torch.tensor(ids[1:])] = 0.0
    return -1


def oracle(z, temperature, top_k, top_p, u=None, delta=DELTA):
    """z: one row, the values of the model dtype (any array, taken to fp64 exactly).  temperature / top_p / u are used at their
    float32 values, which is what the C ABI receives.  -> dict: kept (bool mask), n_kept, decided (no distinct value's A within
    delta * Z_k of top_p * Z_k), and with u: token, t, C (inclusive cumulative kept weight), Z_P, prob (w / Z_P)."""
    z = np.asarray(z, dtype=np.float64)
    T, P = float(np.float32(temperature)), float(np.float32(top_p))
    valid = ~np.isnan(z) & (z > -np.inf)
    out = {"decided": True}
    if not valid.any():
        out.update(kept=np.zeros(z.shape, bool), n_kept=0, token=0)
        return out
    zmax = z[valid].max()
    keep = valid.copy()
    if 0 < top_k < z.size:
        desc = np.sort(z[valid])[::-1]
        keep &= z >= desc[min(top_k, desc.size) - 1]                # ties are all kept
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.where(keep, np.where(z == zmax, 1.0, np.exp((z - zmax) / T)), 0.0)
    Zk = w.sum()
    if P < 1.0:
        vals, inv = np.unique(z[keep], return_inverse=True)         # ascending distinct values
        mass = np.bincount(inv, weights=w[keep], minlength=vals.size)
        above = np.concatenate([np.cumsum(mass[::-1])[::-1][1:], [0.0]])   # A of each distinct value: the mass strictly above it
        out["decided"] = bool(np.all(np.abs(above - P * Zk) > delta * Zk))
        kv = above < P * Zk
        k2 = np.zeros(z.shape, bool)
        k2[np.flatnonzero(keep)] = kv[inv]
        keep = k2
        w = np.where(keep, w, 0.0)
    out.update(kept=keep, n_kept=int(keep.sum()))
    if u is not None:
        Cm = np.cumsum(w)
        ZP = Cm[-1]
        t = float(np.float32(u)) * ZP
        hit = np.flatnonzero(keep & (Cm > t))
        out.update(token=int(hit[0]) if hit.size else int(np.flatnonzero(keep)[-1]), t=t, C=Cm, Z_P=ZP, prob=w / ZP)
    return out


def token_within_bound(o, token, delta=DELTA):
    """C_{i-1} - delta Z_P <= t < C_i + delta Z_P for a kept i, against the oracle's fp64 cumulative weights"""
    if not (0 <= token < o["kept"].size) or not o["kept"][token]:
        return False
    lo = o["C"][token - 1] if token > 0 else 0.0
    return lo - delta * o["Z_P"] <= o["t"] < o["C"][token] + delta * o["Z_P"]


# ---- tests -------------------------------------------------------------------------------------------------------------------
def test_sampling_symbols_declared_bound_exported():
    from seedstory import _lib
    lib = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "seedstory_hip.h")).read()
    declared = set(re.findall(r"\b(ss_[a-z0-9_]+)\s*\(", hdr))
    for name in ("ss_llama_set_sampling", "ss_sample_logits"):
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert "typedef struct ss_sampling" in hdr
    # the ctypes mirror of ss_sampling { float temperature; float top_p; int32_t top_k; uint64_t seed; }
    assert [f[0] for f in _lib.Sampling._fields_] == ["temperature", "top_p", "top_k", "seed"]
    assert C.sizeof(_lib.Sampling) == 24 and _lib.Sampling.seed.offset == 16


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10"""
    def run(ctr, key):
        return ["%08x" % int(v) for v in philox4x32_10(ctr, key)]
    assert run((0, 0, 0, 0), (0, 0)) == ["6627e8d5", "e169c58d", "bc57ac4c", "9b00dbd8"]
    f = 0xFFFFFFFF
    assert run((f, f, f, f), (f, f)) == ["408f276d", "41c83b0e", "a20bc7c6", "6d5451fd"]
    assert run((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0)) == ["d16cfe09", "94fdcceb", "5001e420", "24126ea1"]
    # vectorised over lanes == one at a time; u in [0, 1) on the 2^-24 grid
    lanes = np.arange(5)
    many = philox4x32_10((7, lanes, 0, 0), (123, 456))[0]
    assert [int(v) for v in many] == [int(philox4x32_10((7, int(l), 0, 0), (123, 456))[0]) for l in lanes]
    u = philox_u(0x123456789ABCDEF, np.arange(1000), 3)
    assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all() and np.all(u * 2.0 ** 24 == np.round(u * 2.0 ** 24))
    assert 0.4 < float(u.mean()) < 0.6


@pytest.mark.parametrize("T,top_k,top_p", [(0.7, 0, 0.5), (1.0, 50, 0.9), (1.3, 0, 1.0), (0.7, 0, 0.95), (0.9, 5, 1.0)])
def test_oracle_kept_set_equals_hf_warpers(T, top_k, top_p):
    """Temperature -> TopK -> TopP of the installed transformers, in fp64 on the CPU, keep the oracle's set (inputs without
    ties near the boundary: continuous fp64 draws; undecided cases are not compared)."""
    from transformers import TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper
    warpers = [TemperatureLogitsWarper(float(np.float32(T)))]
    if top_k > 0:
        warpers.append(TopKLogitsWarper(top_k))
    if top_p < 1.0:
        warpers.append(TopPLogitsWarper(float(np.float32(top_p))))
    g = torch.Generator().manual_seed(17)
    compared = 0
    for vocab in (64, 1000, 32066):
        for _ in range(4):
            z = torch.randn(vocab, generator=g, dtype=torch.float64) * 4.0
            o = oracle(z.numpy(), T, top_k, top_p)
            if not o["decided"]:
                continue
            s = z.unsqueeze(0).clone()
            for wp in warpers:
                s = wp(torch.zeros(1, 1, dtype=torch.long), s)
            hf = torch.isfinite(s[0]).numpy()
            assert np.array_equal(hf, o["kept"]), (vocab, int(hf.sum()), o["n_kept"])
            compared += 1
    assert compared >= 10


def test_oracle_definition_cases():
    z = np.array([1.0, 3.0, 2.0, 3.0, -np.inf, np.nan, 0.0])
    o = oracle(z, 1.0, 1, 1.0, u=0.75)              # top-1 with a tie: both maxima kept, equal weights
    assert o["kept"].tolist() == [False, True, False, True, False, False, False] and o["token"] == 3
    assert oracle(z, 1.0, 1, 1.0, u=0.25)["token"] == 1
    o = oracle(z, 1.0, 0, 1.0, u=0.0)
    assert o["n_kept"] == 5 and o["token"] == 0      # -inf and NaN are never kept; u = 0 -> the first kept index
    assert oracle(z, 1.0, 0, 1e-6, u=0.9)["kept"].tolist() == [False, True, False, True, False, False, False]   # the arg max always stays
    assert oracle(np.full(4, np.nan), 1.0, 0, 1.0, u=0.5)["token"] == 0
    # top-p: A strictly above.  weights 1, e^-1, e^-2 (Z = 1.503): p Z = 0.9 keeps {3.0}; 1.2 adds 2.0 (A = 1); 1.4 all (A = 1.368)
    z = np.array([3.0, 2.0, 1.0])
    Z = 1 + np.exp(-1) + np.exp(-2)
    assert [oracle(z, 1.0, 0, p / Z)["n_kept"] for p in (0.9, 1.2, 1.4)] == [1, 2, 3]
    o = oracle(z, 1.0, 0, 1.0, u=np.float32(1 - 2.0 ** -24))
    assert o["token"] == 2 and token_within_bound(o, 2) and not token_within_bound(o, 0)


def test_c_abi_refuses_bad_parameters_before_any_launch():
    """SS_EINVAL for every parameter outside its range: checked on the host before a launch, so it is testable without a GPU
    (the pointers are never dereferenced)."""
    from seedstory import _lib, ops
    lib = _lib.lib()
    buf = (C.c_float * 64)()
    tok = (C.c_int32 * 1)()
    addr = C.addressof(buf)

    def call(sp, vocab=64, rows=1, ld=64, logits=addr, out=C.addressof(tok)):
        return lib.ss_sample_logits(logits, rows, vocab, ld, C.byref(sp) if sp is not None else None, None, 0, None, None, 0, out,
                                    None, _lib.SS_F32, None)
    S = _lib.Sampling
    for sp in (S(0.0, 1.0, 0, 0), S(-1.0, 1.0, 0, 0), S(float("nan"), 1.0, 0, 0), S(float("inf"), 1.0, 0, 0), S(1.0, 0.0, 0, 0),
               S(1.0, 1.5, 0, 0), S(1.0, float("nan"), 0, 0), S(1.0, -0.1, 0, 0), S(1.0, 1.0, -1, 0), None):
        assert call(sp) == -1, sp and (sp.temperature, sp.top_p, sp.top_k)
        assert lib.ss_last_error()
    ok = S(1.0, 1.0, 0, 0)
    assert call(ok, vocab=65536, ld=65536) == -1 and call(ok, rows=0) == -1 and call(ok, ld=63) == -1
    assert call(ok, logits=None) == -1 and call(ok, out=None) == -1
    assert lib.ss_llama_set_sampling(None, 0, C.byref(ok)) == -1
    with pytest.raises(_lib.SSError):
        ops.sampling_struct(top_k=1.5)
    sp = ops.sampling_struct(0.7, 40, 0.9, -1)
    assert (round(sp.temperature, 6), sp.top_k, round(sp.top_p, 6), sp.seed) == (0.7, 40, 0.9, 2 ** 64 - 1)


# ---- host plumbing with stand-in engines -----------------------------------------------------------------------------------
def _llm_and_engine(monkeypatch, with_sampling):
    from test_host_cpu import _FakeDecodeEngine
    from seedstory import _lib, ops
    from src.models_clm.generation import AutoImageTokenGenerationProcessor
    from src.models_clm.modeling_llama_xformer import LlamaConfig, LlamaForCausalLM
    _lib.lib()
    monkeypatch.setattr(ops, "gather_rows", lambda table, ids: table[ids.long()])
    monkeypatch.setattr(ops, "gemm", lambda a, w, **kw: a @ w.t())
    img = list(range(3000, 3066))

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

    class SamplingEng(Eng):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.calls, self.sampling = [], None

        def set_sampling(self, temperature=1.0, top_k=0, top_p=1.0, seed=0, slot=None):
            ops.sampling_struct(temperature, top_k, top_p, seed)
            self.sampling = dict(temperature=temperature, top_k=top_k, top_p=top_p, seed=seed)
            self.calls.append(("sampling", dict(self.sampling)))

        def set_greedy(self, slot=None):
            self.sampling = None
            self.calls.append(("greedy",))

        def generate(self, n_steps, last_prompt_id, forced=None):
            self.calls.append(("generate", None if self.sampling is None else dict(self.sampling)))
            return super().generate(n_steps, last_prompt_id, forced)

    class Tok:
        def encode(self, s, add_special_tokens=False):
            return list(img)

    m = LlamaForCausalLM(LlamaConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=1, vocab_size=50))
    eng = (SamplingEng if with_sampling else Eng)(img)
    monkeypatch.setattr(m, "engine_for_generation", lambda ids, eng=eng: eng)
    m.use_kv_cache_head = False
    ids = torch.tensor([[1, 40, 41, 42]])
    kw = dict(input_ids=ids, inputs_embeds=ids.float().unsqueeze(-1), logits_processor=[AutoImageTokenGenerationProcessor(tokenizer=Tok())])
    return m, eng, kw


def test_do_sample_sets_and_restores_sampling(monkeypatch):
    monkeypatch.setenv("SEEDSTORY_IMG_BLOCK", "0")
    m, eng, kw = _llm_and_engine(monkeypatch, True)
    m.generate(max_new_tokens=12, do_sample=True, temperature=0.7, top_k=40, top_p=0.9, seed=1234, **kw)
    want = dict(temperature=0.7, top_k=40, top_p=0.9, seed=1234)
    assert eng.calls == [("sampling", want), ("generate", want), ("greedy",)] and eng.sampling is None
    # an exception inside _generate (the token-ring guard) still restores greedy
    eng.calls.clear()
    with pytest.raises(ValueError):
        m.generate(max_new_tokens=513, do_sample=True, seed=1, **kw)
    assert eng.calls[0][0] == "sampling" and eng.calls[-1] == ("greedy",) and eng.sampling is None
    # seed=None: torch.initial_seed() + a per-model call counter -> torch.manual_seed governs, successive calls differ
    seeds = []
    for _ in range(2):
        torch.manual_seed(99)
        mm, ee, kk = _llm_and_engine(monkeypatch, True)
        for _ in range(2):
            mm.generate(max_new_tokens=5, do_sample=True, **kk)
        seeds.append([c[1]["seed"] for c in ee.calls if c[0] == "sampling"])
    assert seeds[0] == seeds[1] == [99, 100]
    # defaults: temperature 1, top_k 0 = off (Hugging Face's 50 is not adopted), top_p 1
    assert [c for c in ee.calls if c[0] == "sampling"][0][1] == dict(temperature=1.0, top_k=0, top_p=1.0, seed=99)


def test_do_sample_false_never_touches_sampling(monkeypatch):
    monkeypatch.setenv("SEEDSTORY_IMG_BLOCK", "0")
    m, eng, kw = _llm_and_engine(monkeypatch, False)            # this stand-in HAS no set_sampling / set_greedy
    a = m.generate(max_new_tokens=12, **kw).sequences.tolist()
    b = m.generate(max_new_tokens=12, do_sample=False, temperature=0.7, top_p=0.5, top_k=3, seed=5, num_beams=4, **kw).sequences.tolist()
    assert a == b
    m2, eng2, kw2 = _llm_and_engine(monkeypatch, True)
    m2.generate(max_new_tokens=12, temperature=0.7, top_p=0.5, **kw2)
    assert [c[0] for c in eng2.calls] == ["generate"]


def test_do_sample_bad_parameters_raise(monkeypatch):
    from seedstory import _lib
    m, eng, kw = _llm_and_engine(monkeypatch, True)
    with pytest.raises(NotImplementedError):
        m.generate(max_new_tokens=5, do_sample=True, num_beams=2, **kw)
    with pytest.raises(_lib.SSError):
        m.generate(max_new_tokens=5, do_sample=True, top_k=2.5, **kw)
    assert eng.sampling is None and ("generate", None) not in eng.calls and not any(c[0] == "generate" for c in eng.calls)


def test_continuous_lvlm_forwards_sampling_arguments():
    from src.models_clm.models import ContinuousLVLM
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

    class Tok:
        def encode(self, s, add_special_tokens=False):
            return [9]

        def decode(self, ids, skip_special_tokens=False):
            return "x"

    agent = ContinuousLVLM.__new__(ContinuousLVLM)
    torch.nn.Module.__init__(agent)
    agent.__dict__["llm"] = LLM()
    ids = torch.tensor([[1, 5]])
    agent.generate(Tok(), input_ids=ids, logits_processor=[])
    agent.generate(Tok(), input_ids=ids, logits_processor=[], do_sample=True, temperature=0.9, top_p=0.8, top_k=7, seed=11)
    base = {k: v for k, v in seen[0].items() if k not in ("input_ids", "inputs_embeds")}
    # the default call is what it has always been
    assert base == dict(output_hidden_states=True, return_dict_in_generate=True, logits_processor=[], past_key_values=None,
                        max_new_tokens=120, temperature=0.7, num_beams=1, top_p=0.5, do_sample=False, forced_tokens=None)
    s = seen[1]
    assert (s["do_sample"], s["temperature"], s["top_p"], s["top_k"], s["seed"]) == (True, 0.9, 0.8, 7, 11)

"""The history rules (repetition penalty -> no-repeat n-gram -> min_new_tokens), the CPU side: the ORACLE (a short torch
restatement of the definition in include/seedstory_hip.h, `ss_process_logits`; tests/test_logits_rules_gpu.py imports it and the
case generator below), pinned here against the installed `transformers` processors (version caveat: at the pin), the C ABI
surface, and the host plumbing of the new ``generate`` kwargs driven with stand-in engines."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
NAME = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}
MAX_NGRAM = 8


def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def bits_nan_canonical(t):
    """bit patterns with every NaN given one payload: torch's CPU ``scatter`` (inside RepetitionPenaltyLogitsProcessor) rewrites
    the payload of bf16 NaN entries it does not even address (0x7FC0 comes back as 0xFFFF), so against transformers a NaN can
    only be compared as "NaN here, NaN there"; every other entry, +-inf and zeros included, is compared bit for bit"""
    return bits(torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t))


# ---- the oracle --------------------------------------------------------------------------------------------------------------
def banned_ngram_ids(hist, n):
    """ids that have followed an earlier occurrence of the last n - 1 ids of hist (n >= 1; empty while len(hist) + 1 < n)"""
    L = len(hist)
    if n <= 0 or L + 1 < n:
        return []
    h = np.asarray(hist, dtype=np.int64)
    if L < n:
        return []
    ok = np.ones(L - n + 1, dtype=bool)
    for k in range(n - 1):
        ok &= h[k:L - n + 1 + k] == h[L - (n - 1) + k]
    return sorted(set(h[n - 1:][ok].tolist()))


def oracle(row, hist, prompt_len=0, p=1.0, n=0, m=0, eos=-1, spare=False, img_ids=()):
    """The three rules on one row (a 1-D torch tensor of the model dtype) -> the edited copy.  Ids of hist outside [0, vocab)
    are never used as an index (they still take part in the n-gram comparison)."""
    z = row.clone()
    V = z.numel()
    hist = [int(t) for t in hist]
    if p != 1.0:
        ids = sorted({t for t in hist if 0 <= t < V} - (set(int(i) for i in img_ids) if spare else set()))
        if ids:
            idx = torch.tensor(ids)
            v = z[idx].float()
            pf = torch.tensor(p, dtype=torch.float32)           # p at its float32 value, fp32 arithmetic, one rounding to T
            out = torch.where(v < 0, v * pf, v / pf).to(z.dtype)
            z[idx] = torch.where(torch.isnan(v), z[idx], out)   # NaN stays NaN: the entry keeps its bits
    ban = [t for t in banned_ngram_ids(hist, n) if 0 <= t < V]
    if ban:
        z[torch.tensor(ban)] = float("-inf")
    if len(hist) - prompt_len < m and 0 <= eos < V:
        z[eos] = float("-inf")
    return z


# ---- the cases of the kernel test (built here so that their premise is checked without a GPU) ---------------------------------------
VOCABS = [64, 1000, 32066, 65535]
EOS = 2
# (name, p, n, m, spare): each rule alone, all three, spare on / off, n = 1 and the cap, a penalty below 1
CONFIGS = [("penalty", 1.2, 0, 0, False), ("ngram3", 1.0, 3, 0, False), ("min_new", 1.0, 0, 3, False), ("all", 1.3, 3, 3, False),
           ("all_spare", 1.3, 2, 3, True), ("ngram1", 1.0, 1, 0, False), ("ngram_cap", 0.75, MAX_NGRAM, 0, True)]


def history_lengths(n):
    n = n if n > 0 else 3
    return [0, 1, max(n - 2, 0), n - 1, 1023, 1025, 3000]


def make_history(g, length, alphabet, n):
    """a block of 11 ids from the small alphabet, repeated with one id in twelve redrawn: n-grams up to the cap really repeat"""
    block = alphabet[torch.randint(len(alphabet), (11,), generator=g)]
    h = block.repeat(length // 11 + 1)[:length].clone()
    redraw = torch.rand(length, generator=g) < 1.0 / 12.0
    h[redraw] = alphabet[torch.randint(len(alphabet), (int(redraw.sum()),), generator=g)]
    if n > 1 and length >= 11 + 2 * n:      # the last n - 1 ids repeat an earlier stretch, so the context has a predecessor for certain
        h[length - (n - 1):] = h[11:11 + n - 1]
    return h.tolist()


def make_case(dtype, vocab, cfg):
    """-> dict(z [rows, vocab], hist (list per row), prompt_len, img_ids, want [rows, vocab]) for one kernel call: one row per
    history length; ids 0, 31, 32 and vocab - 1 (bitmap word edges) are in the alphabet; the rows hold negative, zero, +-inf,
    NaN and (in fp16) overflowing entries at ids of the alphabet."""
    name, p, n, m, spare = cfg
    g = torch.Generator().manual_seed(1000 * VOCABS.index(vocab) + 10 * [c[0] for c in CONFIGS].index(name) + DTYPES.index(dtype))
    extra = torch.randint(33, vocab - 1, (4,), generator=g)
    alphabet = torch.cat([torch.tensor([0, 31, 32, vocab - 1]), extra])
    lens = history_lengths(n)
    z = (torch.randn(len(lens), vocab, generator=g) * 4.0).to(dtype)
    z[:, 0] = 0.0
    z[:, 31] = -z[:, 31].abs() - 0.5
    z[0::2, 32], z[1::2, 32] = float("inf"), float("-inf")
    z[0::3, vocab - 1] = float("nan")
    z[:, int(extra[0])] = -60000.0          # fp16: times a penalty above 1 it overflows to -inf
    z[:, int(extra[1])] = 60000.0
    hist = [make_history(g, L, alphabet, n) for L in lens]
    # min_new_tokens: even rows are still inside the first m new tokens, odd rows are past them (or have an empty prompt)
    prompt_len = [max(L - 1, 0) if r % 2 == 0 else 0 for r, L in enumerate(lens)]
    img_ids = [31, vocab - 1, int(extra[2]), 5]
    want = torch.stack([oracle(z[r], hist[r], prompt_len[r], p, n, m, EOS, spare, img_ids) for r in range(len(lens))])
    return dict(z=z, hist=hist, lens=lens, prompt_len=prompt_len, img_ids=img_ids, want=want, p=p, n=n, m=m, spare=spare)


def case_bites(case):
    """the oracle changes at least one entry of the call and leaves at least one untouched"""
    same = bits(case["want"]) == bits(case["z"])
    return bool((~same).any()) and bool(same.any())


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_kernel_cases_bite(dtype):
    for vocab in VOCABS:
        for cfg in CONFIGS:
            case = make_case(dtype, vocab, cfg)
            assert case_bites(case), (NAME[dtype], vocab, cfg[0])
            if cfg[2] > 1:                  # the n-gram rule bans something in the long histories
                long_rows = [r for r, L in enumerate(case["lens"]) if L >= 1023]
                assert all(banned_ngram_ids(case["hist"][r], cfg[2]) for r in long_rows), (vocab, cfg[0])


# ---- the oracle pinned against transformers -----------------------------------------------------------------------------------
def _hf(row, hist, prompt_len, p, n, m, eos):
    """Hugging Face's processors in the order of its processor list.  pinned: checked against the transformers installed here
    (5.x); the reference pins transformers 4.34, whose three classes compute the same thing."""
    import transformers.generation.logits_process as lp
    ids = torch.tensor([hist], dtype=torch.long)
    s = row.clone().unsqueeze(0)
    if p != 1.0:
        s = lp.RepetitionPenaltyLogitsProcessor(penalty=p)(ids, s)
    if n > 0:
        s = lp.NoRepeatNGramLogitsProcessor(n)(ids, s)
    if m > 0:
        s = lp.MinNewTokensLengthLogitsProcessor(prompt_len, m, eos, device="cpu")(ids, s)
    return s[0]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: NAME[d])
def test_oracle_is_bit_equal_to_transformers(dtype):
    """Rows with negative, zero, +-inf and NaN entries, histories with duplicates: torch.equal on the bit patterns (NaN payloads
    canonicalised, see bits_nan_canonical), every rule alone and together."""
    g = torch.Generator().manual_seed(7 + DTYPES.index(dtype))
    compared = 0
    for vocab in (64, 1000):
        for p, n, m in ((1.2, 0, 0), (0.8, 0, 0), (1.0, 3, 0), (1.0, 1, 0), (1.0, 0, 4), (1.3, 2, 4), (1.7, MAX_NGRAM, 1)):
            for L in (1, 2, 9, 200):
                z = (torch.randn(vocab, generator=g) * 4.0).to(dtype)
                alphabet = torch.randint(0, vocab, (5,), generator=g)
                hist = make_history(g, L, alphabet, n)
                for k, v in enumerate((0.0, float("inf"), float("-inf"), float("nan"), -3.0)):
                    z[int(alphabet[k])] = v
                for prompt_len in (0, max(L - 2, 0)):
                    a = oracle(z, hist, prompt_len, p, n, m, EOS)
                    b = _hf(z, hist, prompt_len, p, n, m, EOS)
                    assert torch.equal(bits_nan_canonical(a), bits_nan_canonical(b)), (NAME[dtype], vocab, p, n, m, L, prompt_len)
                    assert not bool((torch.isnan(a) & ~torch.isnan(z)).any())   # nothing becomes NaN (a NaN may be banned to -inf)
                    compared += 1
    assert compared >= 100


def test_oracle_definition_cases():
    z = torch.tensor([2.0, -2.0, 0.0, float("inf"), float("-inf"), float("nan"), 1.0, 1.0])
    o = oracle(z, [0, 1, 0, 0, 3, 4, 5, 2], p=2.0)             # id 0 occurs three times: penalised once
    assert o[:5].tolist() == [1.0, -4.0, 0.0, float("inf"), float("-inf")] and bool(torch.isnan(o[5])) and o[6:].tolist() == [1.0, 1.0]
    assert oracle(z, [0, 1], p=2.0, spare=True, img_ids=[1])[:2].tolist() == [1.0, -2.0]
    assert banned_ngram_ids([1, 2, 3, 1, 2], 3) == [3] and banned_ngram_ids([1, 2, 3, 1, 2], 1) == [1, 2, 3]
    assert banned_ngram_ids([1, 2], 3) == [] and banned_ngram_ids([1], 3) == [] and banned_ngram_ids([7, 7, 7], 2) == [7]
    assert banned_ngram_ids([1, 2, 1, 3, 1], 2) == [2, 3]
    inf = float("-inf")
    assert oracle(z, [6, 6], prompt_len=1, m=2, eos=7)[7] == inf and oracle(z, [6, 6], prompt_len=0, m=2, eos=7)[7] == 1.0
    assert oracle(z, [99, -1, 6], p=2.0, n=1)[6] == inf         # ids outside [0, vocab) are skipped


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("ss_process_logits", "ss_llama_set_logits_rules", "ss_llama_set_history")


def test_new_names_in_header_library_and_binding():
    from seedstory import _lib
    with open(os.path.join(ROOT, "include", "seedstory_hip.h")) as f:
        header = f.read()
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.PROTOTYPES and getattr(lib, name)
    assert "typedef struct ss_logits_rules" in header
    assert re.search(r"#define\s+SS_LOGITS_RULES_MAX_NGRAM\s+%d\b" % MAX_NGRAM, header)
    assert [f[0] for f in _lib.LogitsRules._fields_] == ["repetition_penalty", "no_repeat_ngram", "min_new_tokens", "spare_img_ids"]
    assert C.sizeof(_lib.LogitsRules) == 16


def test_c_abi_refuses_bad_values_before_any_launch():
    """SS_EINVAL for every value outside its range: checked on the host before a launch, so it is testable without a GPU (the
    pointers are never dereferenced)."""
    from seedstory import _lib, ops
    lib = _lib.lib()
    buf = (C.c_float * 64)()
    ints = (C.c_int32 * 8)()
    addr, iaddr = C.addressof(buf), C.addressof(ints)
    R = _lib.LogitsRules

    def call(rp, vocab=64, rows=1, ld=64, logits=addr, hist=iaddr, hist_ld=4, hist_len=iaddr, n_img=0, img=None):
        return lib.ss_process_logits(logits, rows, vocab, ld, C.byref(rp) if rp is not None else None, hist, hist_ld, hist_len, None, 2,
                                     img, n_img, _lib.SS_F32, None)
    for rp in (R(0.0, 0, 0, 0), R(-1.2, 0, 0, 0), R(float("nan"), 0, 0, 0), R(float("inf"), 0, 0, 0), R(1.2, -1, 0, 0),
               R(1.2, MAX_NGRAM + 1, 0, 0), R(1.2, 0, -1, 0), None):
        assert call(rp) == -1, rp and (rp.repetition_penalty, rp.no_repeat_ngram, rp.min_new_tokens)
        msg = lib.ss_last_error()
        assert msg
    call(R(1.2, MAX_NGRAM + 1, 0, 0))
    assert b"no_repeat_ngram" in lib.ss_last_error() and str(MAX_NGRAM).encode() in lib.ss_last_error()
    ok = R(1.2, 3, 0, 0)
    assert call(ok, vocab=65536, ld=65536) == -1 and call(ok, rows=0) == -1 and call(ok, ld=63) == -1
    assert call(ok, logits=None) == -1 and call(ok, hist_len=None) == -1 and call(ok, hist=None) == -1 and call(ok, hist_ld=-1) == -1
    assert call(ok, n_img=1025, img=iaddr) == -1 and call(ok, n_img=2, img=None) == -1
    assert lib.ss_llama_set_logits_rules(None, 0, C.byref(ok)) == -1
    assert lib.ss_llama_set_logits_rules(None, -1, None) == -1
    assert lib.ss_llama_set_history(None, 0, ints, 4, 0) == -1
    for kw in (dict(no_repeat_ngram_size=2.5), dict(min_new_tokens=1.5), dict(no_repeat_ngram_size=2 ** 31)):
        with pytest.raises(_lib.SSError):
            ops.logits_rules_struct(**kw)
    rp = ops.logits_rules_struct(1.2, 3, 5, True)
    assert (round(rp.repetition_penalty, 6), rp.no_repeat_ngram, rp.min_new_tokens, rp.spare_img_ids) == (1.2, 3, 5, 1)
    with pytest.raises(_lib.SSError):
        ops.process_logits(torch.zeros(2, 64), [[1], [2]], repetition_penalty=1.2)        # no CPU path


# ---- host plumbing with stand-in engines -----------------------------------------------------------------------------------
def _llm_and_engine(monkeypatch, with_rules):
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

    class RulesEng(Eng):
        def __init__(self, *a, **kw):
            super().__init__(*a, **kw)
            self.calls, self.rules = [], None

        def set_logits_rules(self, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, spare_img_ids=False, slot=None):
            ops.logits_rules_struct(repetition_penalty, no_repeat_ngram_size, min_new_tokens, spare_img_ids)
            self.rules = dict(repetition_penalty=repetition_penalty, no_repeat_ngram_size=no_repeat_ngram_size,
                              min_new_tokens=min_new_tokens, spare_img_ids=spare_img_ids)
            self.calls.append(("rules", dict(self.rules)))

        def clear_logits_rules(self, slot=None):
            self.rules = None
            self.calls.append(("clear",))

        def set_history(self, ids, slot=None, append=False):
            self.calls.append(("history", list(ids), append))

        def generate(self, n_steps, last_prompt_id, forced=None):
            self.calls.append(("generate", None if self.rules is None else dict(self.rules)))
            return super().generate(n_steps, last_prompt_id, forced)

    class Tok:
        def encode(self, s, add_special_tokens=False):
            return list(img)

    m = LlamaForCausalLM(LlamaConfig(hidden_size=128, intermediate_size=256, num_hidden_layers=1, num_attention_heads=1, vocab_size=50))
    eng = (RulesEng if with_rules else Eng)(img)
    monkeypatch.setattr(m, "engine_for_generation", lambda ids, eng=eng: eng)
    m.use_kv_cache_head = False
    ids = torch.tensor([[1, 40, 41, 42]])
    kw = dict(input_ids=ids, inputs_embeds=ids.float().unsqueeze(-1), logits_processor=[AutoImageTokenGenerationProcessor(tokenizer=Tok())])
    return m, eng, kw


def test_rule_kwargs_reach_the_engine_and_are_cleared(monkeypatch):
    monkeypatch.setenv("SEEDSTORY_IMG_BLOCK", "0")
    m, eng, kw = _llm_and_engine(monkeypatch, True)
    m.generate(max_new_tokens=12, repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=5, spare_img_ids=True, **kw)
    want = dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=5, spare_img_ids=True)
    assert eng.calls == [("rules", want), ("history", [1, 40, 41, 42], False), ("generate", want), ("clear",)] and eng.rules is None
    # one active kwarg is enough; the others keep Hugging Face's inert defaults, spare_img_ids is off
    for one, full in ((dict(repetition_penalty=1.3), dict(repetition_penalty=1.3, no_repeat_ngram_size=0, min_new_tokens=0)),
                      (dict(no_repeat_ngram_size=2), dict(repetition_penalty=1.0, no_repeat_ngram_size=2, min_new_tokens=0)),
                      (dict(min_new_tokens=7), dict(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=7))):
        eng.calls.clear()
        m.generate(max_new_tokens=12, **one, **kw)
        assert eng.calls[0] == ("rules", dict(full, spare_img_ids=False)) and eng.calls[-1] == ("clear",)
    # an exception inside _generate (the token-ring guard) still clears the rules
    eng.calls.clear()
    with pytest.raises(ValueError):
        m.generate(max_new_tokens=513, repetition_penalty=1.2, **kw)
    assert eng.calls[0][0] == "rules" and eng.calls[-1] == ("clear",) and eng.rules is None
    assert not any(c[0] == "generate" for c in eng.calls)


def test_default_kwargs_never_touch_the_rules(monkeypatch):
    monkeypatch.setenv("SEEDSTORY_IMG_BLOCK", "0")
    m, eng, kw = _llm_and_engine(monkeypatch, False)            # this stand-in HAS no set_logits_rules / set_history
    a = m.generate(max_new_tokens=12, **kw).sequences.tolist()
    b = m.generate(max_new_tokens=12, repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, spare_img_ids=True,
                   **kw).sequences.tolist()
    c = m.generate(max_new_tokens=12, repetition_penalty=None, no_repeat_ngram_size=None, min_new_tokens=None, **kw).sequences.tolist()
    assert a == b == c
    m2, eng2, kw2 = _llm_and_engine(monkeypatch, True)
    m2.generate(max_new_tokens=12, **kw2)
    assert [c[0] for c in eng2.calls] == ["generate"]


def test_bad_rule_values_raise_and_leave_the_rules_off(monkeypatch):
    from seedstory import _lib
    m, eng, kw = _llm_and_engine(monkeypatch, True)
    with pytest.raises(_lib.SSError):
        m.generate(max_new_tokens=5, no_repeat_ngram_size=2.5, **kw)
    assert eng.rules is None and not any(c[0] == "generate" for c in eng.calls)


def test_img_block_tokens_join_the_history(monkeypatch):
    """the block path appends the tokens it feeds outside the decode loop, for the slots whose rules are on and no others"""
    from test_host_cpu import _FakeDecodeEngine
    from seedstory import ops
    from seedstory.llama import LlamaEngine
    monkeypatch.setattr(ops, "gather_rows", lambda table, ids: table[ids.long()])
    monkeypatch.setattr(ops, "gemm", lambda a, w, **kw: a @ w.t())
    img = list(range(3000, 3006))
    for on in (False, True):
        eng = _FakeDecodeEngine(img)
        seen = []
        eng.set_history = lambda ids, slot=None, append=False: seen.append((list(ids), slot, append))
        eng._cur = 0
        if on:
            eng._rules_slots = {0}
        ids, _ = eng.generate_img_block(40, 5, [7, img[0]])
        assert ids[:2] == [7, img[0]] and ids[2:7] == img[1:]
        blocks = [(ids[i + 1:i + len(img)], 0, True) for i, t in enumerate(ids) if t == img[0] and i + 1 < len(ids)]
        assert blocks and seen == (blocks if on else [])
    eng = _FakeDecodeEngine(img, n_seq=2)
    seen = []
    eng.set_history = lambda ids, slot=None, append=False: seen.append((list(ids), slot, append))
    eng._rules_slots = {1}
    ids, _ = eng.generate_batch_img_block(12, [5, 6], [[img[0]], [7, img[0]]])
    assert img[0] in ids[0] and seen == [(ids[1][i + 1:i + len(img)], 1, True) for i, t in enumerate(ids[1]) if t == img[0] and i + 1 < len(ids[1])]
    assert LlamaEngine._history_append.__doc__


def test_continuous_lvlm_forwards_rule_arguments():
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
    agent.generate(Tok(), input_ids=ids, logits_processor=[], repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=4,
                   spare_img_ids=True)
    agent.generate(Tok(), input_ids=ids, logits_processor=[], min_new_tokens=4)
    base = {k: v for k, v in seen[0].items() if k not in ("input_ids", "inputs_embeds")}
    # the default call is what it has always been
    assert base == dict(output_hidden_states=True, return_dict_in_generate=True, logits_processor=[], past_key_values=None,
                        max_new_tokens=120, temperature=0.7, num_beams=1, top_p=0.5, do_sample=False, forced_tokens=None)
    s = seen[1]
    assert (s["repetition_penalty"], s["no_repeat_ngram_size"], s["min_new_tokens"], s["spare_img_ids"]) == (1.2, 3, 4, True)
    s = seen[2]
    assert (s["repetition_penalty"], s["no_repeat_ngram_size"], s["min_new_tokens"], s["spare_img_ids"]) == (1.0, 0, 4, False)


def test_driver_flags():
    import argparse
    from src.inference.gen_george import add_rules_arguments, rules_kwargs
    ap = argparse.ArgumentParser()
    add_rules_arguments(ap)
    assert rules_kwargs(ap.parse_args([])) == {}
    a = ap.parse_args(["--repetition-penalty", "1.2", "--no-repeat-ngram-size", "3", "--min-new-tokens", "8"])
    assert rules_kwargs(a) == dict(repetition_penalty=1.2, no_repeat_ngram_size=3, min_new_tokens=8, spare_img_ids=True)
    assert rules_kwargs(ap.parse_args(["--min-new-tokens", "8"]))["spare_img_ids"] is False

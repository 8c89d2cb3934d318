"""Slot fork on the device (``ss_llama_fork`` / ``LlamaEngine.fork``) and what stands on it: ``generate(num_return_sequences=n)``
and best-of-n through ``ContinuousLVLM.generate``.  Everything here is an exact check: a fork is a copy, and a forked slot must
decode bit for bit what a slot that prefilled the same prompt itself decodes.  The tiny model of tests/golden/hotpath_tiny.json,
built as tests/test_sampling_gpu.py builds it."""
import contextlib

import pytest
import torch

import kernel_check as KC
import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
S4 = 4
PROMPT = synth.randint(91, (21,), 3, 250)
SAMPLING = dict(temperature=1.5, top_k=0, top_p=0.95)
LASTS = [int(PROMPT[-1])] * S4
SENTINEL = -7.0


@contextlib.contextmanager
def knobs(**kw):
    from seedstory import _lib
    old = {k: _lib.get_tuning(k, 0) for k in kw}
    for k, v in kw.items():
        _lib.set_tuning(k, v)
    try:
        yield
    finally:
        for k, v in old.items():
            _lib.set_tuning(k, v)


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _raw(t):
    """fp32 scales as their bit patterns, uint8 codes as they are"""
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _img_ids(meta):
    lo, hi = meta["IMG_IDS"]
    return list(range(lo, hi + 1))


def _weights(meta, dtype):
    d = meta["LLAMA"]
    return synth.llama_weights(11, d["hidden"], d["n_heads"], d["n_layers"], d["inter"], d["vocab"], dtype=dtype)


def _engine(meta, dtype, img_ids=None, **kw):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (no CPU fallback exists)")
    from seedstory.llama import LlamaEngine
    d = meta["LLAMA"]
    wd = _weights(meta, dtype)
    eng = LlamaEngine(wd, hidden=d["hidden"], n_heads=d["n_heads"], n_layers=d["n_layers"], inter=d["inter"],
                      vocab=d["vocab"], dtype=dtype, device=DEV, cache_cap=256, max_new=128, max_prefill_rows=64,
                      img_ids=_img_ids(meta) if img_ids is None else img_ids, n_seq=S4, **kw)
    return eng, wd["model.embed_tokens.weight"]


def _snapshot(eng):
    """every slot's K, V, logits and lengths, cloned"""
    out = []
    for b in range(eng.n_seq):
        eng.select(b)
        out.append((eng.k_cache.clone(), eng.v_cache.clone(), eng.logits.clone(), eng.lengths()))
    eng.select(0)
    return out


def _snapshots_equal(a, b):
    return all(_same(x[0], y[0]) and _same(x[1], y[1]) and _same(x[2], y[2]) and x[3] == y[3] for x, y in zip(a, b))


# ---- 1. the copy itself ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 21, 200])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=lambda d: KC.NAME[d])
def test_fork_is_an_exact_copy(golden, dtype, rows):
    from seedstory.llama import _prefill_chunked
    _, meta = golden
    eng, emb = _engine(meta, dtype)
    for b in (1, 2, 3):
        eng.select(b)
        eng.k_cache.fill_(SENTINEL)
        eng.v_cache.fill_(SENTINEL)
    eng.select(0)
    # an empty source: the state alone is copied, no K or V byte moves
    assert eng.fork(0) == [1, 2, 3]
    for b in (1, 2, 3):
        eng.select(b)
        assert bool((eng.k_cache == SENTINEL).all()) and bool((eng.v_cache == SENTINEL).all()) and eng.lengths() == (0, 0)
    eng.select(0)
    _prefill_chunked(eng, emb[synth.randint(92, (rows,), 3, 250)], False)        # 200 rows: four calls of at most 64
    assert eng.lengths() == (rows, rows)
    assert eng.fork(0, [1, 3]) == [1, 3]
    assert eng._cur == 0                                                         # the selected slot is unchanged
    k0, v0, lg0 = eng.k_cache.clone(), eng.v_cache.clone(), eng.logits.clone()
    assert bool(torch.isfinite(k0[:, :, :rows].float()).all()) and float(k0[:, :, :rows].float().abs().max()) > 0
    for b in (1, 3):
        eng.select(b)
        for c, c0 in ((eng.k_cache, k0), (eng.v_cache, v0)):
            assert _same(c[:, :, :rows], c0[:, :, :rows]), b                     # every layer and head, bit for bit
            assert bool((c[:, :, rows:] == SENTINEL).all()), b                   # rows at and above kv_len: not touched
        assert _same(eng.logits, lg0) and eng.lengths() == (rows, rows), b
    eng.select(2)
    assert bool((eng.k_cache == SENTINEL).all()) and bool((eng.v_cache == SENTINEL).all())
    assert eng.lengths() == (0, 0) and not bool(eng.logits.float().abs().any())


# ---- 2. / 3. a forked slot decodes what a slot that prefilled the prompt itself decodes -----------------------------------------
def _state_a(eng, emb, warm=0):
    """the prompt prefilled into each slot (``warm`` decode tokens per slot first bring the fp8 shadow up to the cache)"""
    for b in range(S4):
        eng.select(b).reset()
        eng.prefill(emb[PROMPT])
        if warm:
            assert eng.generate(warm, LASTS[0]) == warm
    eng.select(0)


def _state_b(eng, emb, warm=0):
    """the prompt prefilled into slot 0, which is forked to the others"""
    eng.select(0).reset()
    eng.prefill(emb[PROMPT])
    if warm:
        assert eng.generate(warm, LASTS[0]) == warm
    assert eng.fork() == [1, 2, 3]


def _decode(eng, n=20, lp=False):
    ns = eng.generate_batch(n, LASTS)
    out = []
    for b in range(S4):
        eng.select(b)
        rec = {k: v.clone() for k, v in eng.logprobs(ns[b], b).items()} if lp else {}
        out.append((eng.gen_ids[:ns[b]].tolist(), eng.hidden_rows[:max(ns[b] - 1, 0)].clone(), rec))
    eng.select(0)
    return out


def _assert_equal_runs(ra, rb, what):
    for b in range(S4):
        assert ra[b][0] == rb[b][0], (what, b, ra[b][0], rb[b][0])
        assert _same(ra[b][1], rb[b][1]), (what, b)
        for k in ra[b][2]:
            assert ra[b][2][k].shape == rb[b][2][k].shape and torch.equal(ra[b][2][k].view(torch.int32), rb[b][2][k].view(torch.int32)), (what, b, k)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=lambda d: KC.NAME[d])
def test_fork_equals_independent_prefill(golden, dtype):
    _, meta = golden
    A, emb = _engine(meta, dtype)
    B, _ = _engine(meta, dtype)
    for graph in (1, 0):
        with knobs(llama_graph=graph):
            for sample in (False, True):
                for eng, state in ((A, _state_a), (B, _state_b)):
                    if sample:
                        eng.set_sampling(seed=9, **SAMPLING)
                    else:
                        eng.set_greedy()
                    state(eng, emb)
                ra, rb = _decode(A), _decode(B)
                _assert_equal_runs(ra, rb, (graph, sample))
                assert all(len(r[0]) == 20 for r in rb)
                if sample:
                    assert len({tuple(r[0]) for r in rb}) == S4                  # one prompt, one seed, one prefill: the slots diverge
                else:
                    assert len({tuple(r[0]) for r in rb}) == 1


@pytest.mark.parametrize("sample", [False, True], ids=["greedy", "sampling"])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=lambda d: KC.NAME[d])
def test_fork_with_history_rules(golden, dtype, sample):
    _, meta = golden
    A, emb = _engine(meta, dtype)
    B, _ = _engine(meta, dtype)
    for eng in (A, B):
        eng.set_logits_rules(repetition_penalty=1.2, no_repeat_ngram_size=3)
        if sample:
            eng.set_sampling(seed=9, **SAMPLING)
    plain = None
    if not sample:          # the rules do change this run (so the history that the fork hands on matters)
        C, _ = _engine(meta, dtype)
        _state_a(C, emb)
        plain = _decode(C)
    _state_a(A, emb)
    for b in range(S4):
        A.set_history(PROMPT, slot=b)
    B.select(0).reset()
    B.prefill(emb[PROMPT])
    B.set_history(PROMPT, slot=0)            # the source only, before the fork
    B.fork()
    ra, rb = _decode(A), _decode(B)
    _assert_equal_runs(ra, rb, "rules")
    if plain is not None:
        assert ra[1][0] != plain[1][0]
    # the second call continues the histories the first one grew on both engines
    ra2, rb2 = _decode(A, 8), _decode(B, 8)
    _assert_equal_runs(ra2, rb2, "rules, second call")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=lambda d: KC.NAME[d])
def test_fork_with_logprob_recording(golden, dtype):
    _, meta = golden
    A, emb = _engine(meta, dtype)
    B, _ = _engine(meta, dtype)
    for eng, state in ((A, _state_a), (B, _state_b)):
        eng.set_sampling(seed=9, **SAMPLING)
        eng.set_logprobs(True, top_n=3)
        state(eng, emb)
    ra, rb = _decode(A, lp=True), _decode(B, lp=True)
    _assert_equal_runs(ra, rb, "logprobs")
    assert all(set(r[2]) == {"logprob", "model_logprob", "top_ids", "top_logprobs"} and r[2]["model_logprob"].shape == (20,) for r in rb)
    assert all(bool((r[2]["model_logprob"] < 0).all()) for r in rb)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=lambda d: KC.NAME[d])
def test_fork_with_fp8_kv_shadow(golden, dtype):
    _, meta = golden
    A, emb = _engine(meta, dtype, kv_cache="fp8")
    B, _ = _engine(meta, dtype, kv_cache="fp8")
    # five decode tokens on the source first: its watermark then stands at the cache length, so the fork has shadow rows to copy
    _state_a(A, emb, warm=5)
    _state_b(B, emb, warm=5)
    w = len(PROMPT) + 4                    # (the fifth token is emitted, not fed)
    assert B.lengths() == (w, w)
    B.select(0)
    src = [t.clone() for t in (B.k_codes, B.v_codes, B.k_scale, B.v_scale)]
    assert bool(src[0][:, :, :w].any()) and bool(src[1][:, :, :w].any())
    for b in (1, 2, 3):
        A.select(b)
        B.select(b)
        assert B.lengths() == (w, w)
        for t, s, a in zip((B.k_codes, B.v_codes, B.k_scale, B.v_scale), src, (A.k_codes, A.v_codes, A.k_scale, A.v_scale)):
            assert torch.equal(_raw(t[:, :, :w]), _raw(s[:, :, :w])), b          # codes and scales below the watermark: the source's
            assert torch.equal(_raw(t[:, :, :w]), _raw(a[:, :, :w])), b          # ... and what engine A's slot b made itself
        # above the watermark the destination's planes keep what they held (fresh planes: zero codes, unit scales)
        assert not bool(B.k_codes[:, :, w:].any()) and bool((B.k_scale[:, :, w:] == 1).all()), b
    A.select(0)
    B.select(0)
    ra, rb = _decode(A), _decode(B)
    _assert_equal_runs(ra, rb, "kv8")
    # a fork before the shadow was ever synchronised (watermark 0): the decode call quantises the copied 16-bit rows itself
    _state_a(A, emb)
    _state_b(B, emb)
    _assert_equal_runs(_decode(A), _decode(B), "kv8, cold shadow")


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------
def test_fork_refusals_change_nothing(golden):
    import ctypes as C
    from seedstory import _lib
    _, meta = golden
    eng, emb = _engine(meta, torch.bfloat16)
    eng.select(0).prefill(emb[PROMPT])
    eng.fork(0, [2])
    eng.select(1).prefill(emb[PROMPT[:7]])
    eng.select(0)
    before = _snapshot(eng)
    bad = [dict(src=-1, dsts=[1]), dict(src=4, dsts=[1]), dict(src=0, dsts=[]), dict(src=0, dsts=[4]), dict(src=0, dsts=[-1]),
           dict(src=0, dsts=[0]), dict(src=0, dsts=[1, 0]), dict(src=0, dsts=[1, 1]), dict(src=0, dsts=[1, 2, 3, 1]),
           dict(src=0, dsts=[1, 2, 3, 1, 2, 3, 1, 2, 3]), dict(src=2, dsts=[3, 2])]
    for kw in bad:
        with pytest.raises(_lib.SSError):
            eng.fork(**kw)
    lib = _lib.lib()
    one = (C.c_int32 * 1)(1)
    for args in ((None, 0, one, 1, None), (eng._h, 0, None, 1, None), (eng._h, 0, one, 0, None), (eng._h, 0, one, -3, None)):
        assert lib.ss_llama_fork(*args) == -1 and lib.ss_last_error(), args
        with pytest.raises(_lib.SSError):
            _lib.check(lib.ss_llama_fork(*args), "ss_llama_fork")
    torch.cuda.synchronize()
    assert _snapshots_equal(before, _snapshot(eng))
    from seedstory.llama import LlamaEngine
    d = meta["LLAMA"]
    e1 = LlamaEngine(_weights(meta, torch.bfloat16), hidden=d["hidden"], n_heads=d["n_heads"], n_layers=d["n_layers"], inter=d["inter"],
                     vocab=d["vocab"], dtype=torch.bfloat16, device=DEV, cache_cap=64, max_new=16, max_prefill_rows=32)
    with pytest.raises(_lib.SSError):        # one slot: there is nobody to fork to
        e1.fork()


# ---- 5. LlamaForCausalLM.generate(num_return_sequences=n) ------------------------------------------------------------------------
class _Tok:
    def __init__(self, ids):
        self.ids = ids

    def encode(self, s, add_special_tokens=False):
        if s == "<img>":
            return [self.ids[0]]
        if s == "</img>":
            return [self.ids[-1]]
        return list(self.ids)

    def decode(self, ids, skip_special_tokens=False):
        return " ".join(str(int(i)) for i in ids)


def _llm(meta, dtype, n_seq):
    from src.models_clm.modeling_llama_xformer import LlamaConfig, LlamaForCausalLM
    d = meta["LLAMA"]
    cfg = LlamaConfig(hidden_size=d["hidden"], intermediate_size=d["inter"], num_hidden_layers=d["n_layers"],
                      num_attention_heads=d["n_heads"], vocab_size=d["vocab"])
    llm = LlamaForCausalLM(cfg)
    wd = _weights(meta, dtype)
    llm.load_state_dict(wd, strict=False)
    llm = llm.to(DEV, dtype=dtype)
    llm.cache_cap, llm.max_new, llm.max_prefill_rows = 256, 128, 64
    llm.n_seq = n_seq
    llm.use_kv_cache_head = False
    return llm, wd


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=lambda d: KC.NAME[d])
def test_llm_generate_num_return_sequences(golden, dtype):
    from src.models_clm.generation import AutoImageTokenGenerationProcessor
    _, meta = golden
    img = _img_ids(meta)
    llm, wd = _llm(meta, dtype, S4)
    never, _ = _llm(meta, dtype, 1)                 # a model that never samples
    proc = [AutoImageTokenGenerationProcessor(tokenizer=_Tok(img))]
    ids = PROMPT.unsqueeze(0)
    S = ids.shape[1]
    kw = dict(input_ids=ids, inputs_embeds=wd["model.embed_tokens.weight"][ids].to(DEV), logits_processor=proc)
    greedy = never.generate(max_new_tokens=20, **kw).sequences.tolist()

    # the engine-level run: one prefill, a fork to slots 1 and 2, the three candidates decode in lock-step, slot 3 sits out
    eng, emb = _engine(meta, dtype)
    eng.select(0).prefill(emb[PROMPT])
    eng.fork(0, [1, 2])
    eng.set_sampling(seed=31, **SAMPLING)
    ns = eng.generate_batch(20, LASTS, active=[1, 1, 1, 0])
    want = [eng.select(b).gen_ids[:ns[b]].tolist() for b in range(3)]
    assert ns[3] == 0 and eng.select(3).lengths() == (0, 0)

    def call(seed):
        return llm.generate(max_new_tokens=20, do_sample=True, seed=seed, num_return_sequences=3, **SAMPLING, **kw)
    out = call(31)
    L = S + max(len(w) for w in want)
    assert tuple(out.sequences.shape) == (3, L) and len(out.candidates) == 3
    pad = llm.config.eos_token_id
    for i in range(3):
        row = out.sequences[i].tolist()
        assert row[:S + len(want[i])] == PROMPT.tolist() + want[i], i
        assert row[S + len(want[i]):] == [pad] * (L - S - len(want[i])), i
        c = out.candidates[i]
        assert c.sequences.tolist() == [PROMPT.tolist() + want[i]] and len(c.hidden_states) == max(len(want[i]), 1), i
    assert len({tuple(w) for w in want}) == 3
    assert out.hidden_states is out.candidates[0].hidden_states
    assert call(31).sequences.tolist() == out.sequences.tolist()
    assert call(32).sequences.tolist() != out.sequences.tolist()
    # everything is restored: the next plain call is the greedy sequence of a model that never sampled
    assert llm.generate(max_new_tokens=20, **kw).sequences.tolist() == greedy
    e = llm._engine
    assert e.n_seq == S4 and not e._rules_slots and not e._lp_slots

    # forced tokens ending in <img>: every candidate goes through the image-token block
    out = llm.generate(max_new_tokens=80, do_sample=True, seed=31, num_return_sequences=3, forced_tokens=[5, img[0]],
                       output_logprobs=True, repetition_penalty=1.2, **SAMPLING, **kw)
    lens = []
    for i, c in enumerate(out.candidates):
        g = c.sequences[0][S:].tolist()
        assert g[:2] == [5, img[0]] and g[2:2 + 65] == img[1:], i
        assert len(c.hidden_states) == len(g) and c.model_logprobs.shape == c.logprobs.shape == (len(g),), i
        assert c.logprobs[:67].tolist() == [0.0] * 67, i
        lens.append(len(g))
    assert len({tuple(c.sequences[0].tolist()) for c in out.candidates}) == 3
    assert e._cur == 0 and e.lengths()[0] == S + lens[0] - 1
    for i in (2, 1, 0):
        assert llm.select_candidate(i) == i
        assert e.lengths()[0] == S + lens[i] - 1 and llm.past_key_values[0][0].shape[2] == S + lens[i] - 1
        assert llm.past_key_values[0][0].data_ptr() == e.k_cache.data_ptr()
    with pytest.raises(ValueError):
        llm.select_candidate(3)
    assert not e._rules_slots and not e._lp_slots
    assert llm.generate(max_new_tokens=20, **kw).sequences.tolist() == greedy
    with pytest.raises(ValueError):
        llm.select_candidate(0)                     # the last call returned one sequence


# ---- 6. best-of-n through ContinuousLVLM.generate -----------------------------------------------------------------------------------
def test_continuous_lvlm_best_of_n(golden, monkeypatch):
    from src.models.qwen_visual import Resampler
    from src.models_clm.models import ContinuousLVLM, candidate_score
    _, meta = golden
    dtype = torch.bfloat16
    img = _img_ids(meta)
    llm, wd = _llm(meta, dtype, S4)
    rin = Resampler(grid_size=meta["RES_IN"]["grid"], embed_dim=256, num_heads=2, kv_dim=256)
    rin.load_state_dict(synth.resampler_weights(21, "", meta["RES_IN"]["grid"], 256))
    rout = Resampler(grid_size=meta["RES_OUT"]["grid"], embed_dim=256, num_heads=2, kv_dim=256)
    rout.load_state_dict(synth.resampler_weights(22, "", meta["RES_OUT"]["grid"], 256))
    agent = ContinuousLVLM(llm, rin, rout).eval().to(DEV, dtype)
    agent.llm.n_seq = S4
    calls = []
    real = agent._regress
    monkeypatch.setattr(agent, "_regress", lambda rows: calls.append(tuple(rows.shape)) or real(rows))
    ids = PROMPT.unsqueeze(0)
    S = ids.shape[1]
    out = agent.generate(tokenizer=_Tok(img), input_ids=ids, max_new_tokens=80, num_img_gen_tokens=64, forced_tokens=[5, img[0]],
                         do_sample=True, seed=31, num_return_sequences=3, output_logprobs=True, **SAMPLING)
    cands = out["candidates"]
    assert len(cands) == 3 and len(calls) == 1 and calls[0][0] == 3            # one resampler pass over the three image blocks
    scores = []
    for c in cands:
        g, m = c["generate_ids"].tolist(), c["model_logprobs"].tolist()
        free = [v for t, v in zip(g, m) if t not in img[1:]]
        assert 0 < len(free) <= len(g) - 65 and c["has_img_output"] and c["img_gen_feat"].shape[0] == 1
        scores.append(sum(free) / len(free))
        assert c["score"] == candidate_score(g, m, img[1:]) and abs(c["score"] - scores[-1]) < 1e-6
    best = max(range(3), key=lambda i: (scores[i], -i))
    assert out["best"] == best and len(set(scores)) == 3
    win = cands[best]
    assert out["text"] == win["text"] and out["generate_ids"].tolist() == win["generate_ids"].tolist()
    assert out["has_img_output"] and torch.equal(out["img_gen_feat"], win["img_gen_feat"])
    assert torch.equal(out["model_logprobs"], win["model_logprobs"])
    # past_key_values is the winner's cache: candidate i sits in slot i
    eng = agent.llm._engine
    n = len(win["generate_ids"])
    assert eng._cur == best and eng.lengths()[0] == S + n - 1
    k = out["past_key_values"][0][0]
    assert k.shape[2] == S + n - 1 and k.data_ptr() == eng.select(best).k_cache.data_ptr()
    # the engine is clean afterwards
    assert not eng._lp_slots and not eng._rules_slots

"""Beam search on the GPU: the stand-alone selection step (``ss_beam_step``) against the fp64 reference of tests/beam_ref.py,
the cache / history permutation against a host gather, the engine's search (``LlamaEngine.beam_search``) against a host-driven
search built from existing primitives, one beam against greedy, ``generate(num_beams=)`` end to end, and the refusals."""
import ctypes as C
import functools
import itertools

import pytest
import torch

import beam_ref
import kernel_check as KC
import logprobs_ref as R
import synth
from test_logprobs_cpu import LP_A, LP_B

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (no CPU fallback exists)")
    from seedstory import ops as _ops
    return _ops


def _bits(t):
    return t.contiguous().view(torch.int32 if t.dtype in (torch.float32, torch.int32) else torch.int16)


def _bound(ref, terms=1):
    """the allowance of ``terms`` log-probabilities summed to ``ref`` (tests/test_logprobs_cpu.py derives the one-term bound)"""
    return terms * (LP_A + LP_B * abs(ref))


# ---- 1. ss_beam_step against the reference --------------------------------------------------------------------------------------
def _guarded_step(z, scores, stops):
    """ss_beam_step through the C ABI, the rows and every output in guarded buffers -> (scores, beams, tokens) on the CPU"""
    from seedstory import _lib, ops
    rows, vocab = z.shape
    K = beam_ref.n_candidates(rows, stops)
    src = KC.GuardedOut(rows, vocab, z.dtype, device=DEV, ld=vocab + 3)
    src.out.copy_(z.to(DEV))
    sc = torch.tensor(scores, dtype=torch.float32, device=DEV)
    outs = [KC.GuardedOut(1, K, torch.float32, device=DEV) for _ in range(3)]       # (int32 in 4-byte guarded buffers)
    arr = (C.c_int32 * max(1, len(stops)))(*stops)
    _lib.check(_lib.lib().ss_beam_step(src.data_ptr(), rows, vocab, src.ld if rows > 1 else vocab, sc.data_ptr(), len(stops), arr,
                                       outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), ops.dt(z.dtype), ops.stream()),
               "ss_beam_step")
    what = "beam_step %s rows %d vocab %d K %d" % (KC.NAME[z.dtype], rows, vocab, K)
    assert torch.equal(_bits(src.check(what + " (input)")), _bits(z))
    cs = outs[0].check(what + " (scores)").view(-1)
    cb = outs[1].check(what + " (beams)").view(torch.int32).view(-1)
    ct = outs[2].check(what + " (tokens)").view(torch.int32).view(-1)
    return cs, cb, ct


def _rows(g, dtype, rows, vocab):
    """N(0, 4^2) rows rounded to the dtype, with the special rows: a NaN and a -inf in row 0; from 3 rows on, row 1 all -inf but
    one entry and row 2 a copy of row 0 (exact duplicates across rows: the tie rule)"""
    z = (torch.randn(rows, vocab, generator=g) * 4.0).to(dtype)
    z[0, int(torch.randint(vocab, (1,), generator=g))] = NAN
    z[0, int(torch.randint(vocab, (1,), generator=g))] = -INF
    if rows >= 3:
        z[1] = -INF
        z[1, int(torch.randint(vocab, (1,), generator=g))] = 1.5
        z[2] = z[0]
    return z


def _compare_step(z, scores, stops, got):
    """-> (positions, positions inside a gap); asserts everything else"""
    rows, vocab = z.shape
    K = beam_ref.n_candidates(rows, stops)
    ref = beam_ref.step(z.double(), scores, K, torch.float64, extra=1)
    cs, cb, ct = got
    what = (KC.NAME[z.dtype], rows, vocab, K)
    loose = 0
    for j in range(K):
        s, b, t = ref[j]
        if b < 0:
            assert float(cs[j]) == -INF and (int(cb[j]), int(ct[j])) == (-1, -1), (what, j)
            continue
        tol = 2 * _bound(s)
        # an exact tie of the reference is decided by the tie rule, like a clear gap; only a gap inside (0, tol] may swap
        near = [abs(s - ref[i][0]) for i in (j - 1, j + 1) if 0 <= i <= K and ref[i][1] >= 0 and ref[i][0] != s]
        if near and min(near) <= tol:
            loose += 1                      # (the neighbour's score may stand here: its own allowance on top of the gap)
            assert abs(float(cs[j]) - s) <= tol + _bound(s), (what, j, float(cs[j]), s)
            continue
        assert R.within(cs[j], s, LP_A, LP_B), (what, j, float(cs[j]), s)
        assert (int(cb[j]), int(ct[j])) == (b, t), (what, j, int(cb[j]), int(ct[j]), b, t)
    return K, loose


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: KC.NAME[d])
def test_beam_step_against_reference(ops, dtype):
    g = torch.Generator().manual_seed(977 + DTYPES.index(dtype))
    total = loose = 0
    for rows, vocab, stops in itertools.product((1, 3, 8), (50, 1000, 32066), ((2,), (2, 11))):
        z = _rows(g, dtype, rows, vocab)
        for step0 in (False, True):
            # running scores: the step-0 vector [0, dead ...], or a spread of sums with equal scores on the duplicated rows
            scores = [0.0] + [-INF] * (rows - 1) if step0 else [-(0.37 * (b % 2) + 0.11 * (b // 3)) for b in range(rows)]
            got = _guarded_step(z, scores, list(stops))
            k, l = _compare_step(z, scores, list(stops), got)
            total, loose = total + k, loose + l
        # the Python wrapper returns the same bits
        w = ops.beam_step(z.to(DEV), scores, stops)
        assert all(torch.equal(_bits(a.cpu()), _bits(b)) for a, b in zip(w, got))
    assert loose <= 0.05 * total, (loose, total)


def test_beam_step_refuses_bad_arguments(ops):
    from seedstory import _lib
    z = torch.zeros(2, 50, device=DEV)
    with pytest.raises(_lib.SSError):
        ops.beam_step(z.cpu(), [0.0, 0.0])
    with pytest.raises(_lib.SSError):
        ops.beam_step(z, [0.0])
    with pytest.raises(_lib.SSError):
        ops.beam_step(z, [0.0, 0.0], stop_ids=[1, 2, 3])
    with pytest.raises(_lib.SSError):
        ops.beam_step(z, [0.0, 0.0], stop_ids=[50])
    with pytest.raises(_lib.SSError):
        ops.beam_step(torch.zeros(9, 50, device=DEV), [0.0] * 9)


# ---- tiny engines -------------------------------------------------------------------------------------------------------------------
VOCAB = 300
PROMPT = synth.randint(93, (9,), 3, 250).tolist()


@functools.lru_cache(maxsize=None)
def _weights(dtype, hd):
    wd = synth.llama_weights(17, 2 * hd, 2, 2, 4 * hd, VOCAB, dtype=dtype)
    wd["lm_head.weight"] = (wd["lm_head.weight"].float() * 15.0).to(dtype)         # logits with a spread of a few units
    return wd


def _engine(dtype, n_seq, hd=64, eos_id=-1, img_ids=(), **kw):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (no CPU fallback exists)")
    from seedstory.llama import LlamaEngine
    wd = _weights(dtype, hd)
    eng = LlamaEngine(wd, hidden=2 * hd, n_heads=2, n_layers=2, inter=4 * hd, vocab=VOCAB, dtype=dtype, device=DEV, cache_cap=96,
                      max_new=32, max_prefill_rows=64, img_ids=list(img_ids), eos_id=eos_id, n_seq=n_seq, **kw)
    return eng, wd["model.embed_tokens.weight"]


# ---- 2. the permutation ----------------------------------------------------------------------------------------------------------------
PARENTS = ([0, 1, 2, 3], [1, 2, 3, 0], [1, 1, 0, 0], [3, 3, 3, 3])


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=lambda d: KC.NAME[d])
def test_beam_permute_is_a_gather(dtype, hd):
    eng, _ = _engine(dtype, 4, hd=hd)
    eng.set_logits_rules(repetition_penalty=1.3)
    g = torch.Generator().manual_seed(5)
    for kv0, suffix, parent in itertools.product((0, 5), (1, 9, 40), PARENTS):
        kv = kv0 + suffix
        hist0, hlen = 4 + kv0, 4 + kv0 + suffix
        before = []
        for b in range(4):
            eng.select(b)
            eng.k_cache.copy_(torch.randn(eng.k_cache.shape, generator=g).to(dtype))
            eng.v_cache.copy_(torch.randn(eng.v_cache.shape, generator=g).to(dtype))
            eng.set_lengths(kv, kv)
            eng.set_history(torch.randint(0, VOCAB, (hlen,), generator=g).tolist())
            before.append((eng.k_cache.clone(), eng.v_cache.clone(), eng.history.clone(), eng.history_bitmap.clone()))
        eng.select(0)
        eng._beam_permute(parent, kv0, hist0)
        torch.cuda.synchronize()
        for b in range(4):
            eng.select(b)
            src = before[parent[b]]
            for c, own, par in ((eng.k_cache, before[b][0], src[0]), (eng.v_cache, before[b][1], src[1])):
                what = (KC.NAME[dtype], hd, kv0, suffix, parent, b)
                assert torch.equal(_bits(c[:, :, kv0:kv]), _bits(par[:, :, kv0:kv])), what       # bit-equal to the host gather
                assert torch.equal(_bits(c[:, :, :kv0]), _bits(own[:, :, :kv0])), what           # the shared prompt: not moved
                assert torch.equal(_bits(c[:, :, kv:]), _bits(own[:, :, kv:])), what             # rows at and above kv_len
            assert torch.equal(eng.history[hist0:hlen], src[2][hist0:hlen]) and torch.equal(eng.history[:hist0], before[b][2][:hist0])
            assert torch.equal(eng.history[hlen:], before[b][2][hlen:])
            assert torch.equal(eng.history_bitmap, src[3])
            assert eng.lengths() == (kv, kv)
    eng.clear_logits_rules()


# ---- 3. the engine's search against a host-driven one ---------------------------------------------------------------------------------
def _move_slots(H, parents, spare):
    """slot i <- what slot parents[i] holds, for every i, with ``fork`` through the spare slot"""
    pending = {i: p for i, p in enumerate(parents) if p != i}
    while pending:
        free = [i for i in pending if i not in pending.values()]
        if free:
            i = free[0]
            H.fork(pending.pop(i), [i])
            continue
        i = next(iter(pending))             # only cycles are left: park slot i's content
        H.fork(i, [spare])
        pending = {d: (spare if s == i else s) for d, s in pending.items()}


def _host_search(ops, H, emb, n, stops, limit, lp, es, ngram):
    def logits_fn(seqs, parents):
        if parents is None:
            H.select(0).reset()
            H.prefill(emb[PROMPT])
            rows = H.logits.clone()[None]
        else:
            _move_slots(H, parents, n)
            m = len(seqs)
            # two tokens: the forced one is fed, the second stops at the limit before it is fed (one forward, fresh logits)
            H.generate_batch(2, [PROMPT[-1]] * (n + 1), [[s[-1]] for s in seqs] + [[]] * (n + 1 - m), [True] * m + [False] * (n + 1 - m))
            rows = torch.stack([H.select(i).logits.clone() for i in range(m)])
        H.select(0)
        if ngram:
            ops.process_logits(rows, [PROMPT + s for s in seqs], prompt_len=[len(PROMPT)] * len(seqs), no_repeat_ngram_size=ngram)
        return rows.cpu()
    return beam_ref.search(logits_fn, n, stops, limit, lp, es, dtype=torch.float64)


def _first_cut(r):
    """the first step whose closest pair of distinct neighbouring candidates is inside twice the allowance of their sums"""
    for t, cands in enumerate(r["steps"]):
        live = [c[0] for c in cands if c[1] >= 0]
        for a, b in zip(live, live[1:]):
            if a != b and a - b <= 2 * _bound(b, t + 1):
                return t
    return None


@functools.lru_cache(maxsize=None)
def _engine_case(dtype, n, ngram, reachable):
    """-> the step the case was cut at (None: not cut); asserts the comparison"""
    from seedstory import ops
    limit, (lp, es) = 12, ((0.7, "never") if ngram else (1.0, False))
    H, emb = _engine(dtype, n + 1)
    H.select(0).reset()
    H.prefill(emb[PROMPT])
    eos = int(H.logits.float().topk(2).indices[1]) if reachable else -1       # the prompt's second-best token ends a hypothesis
    stops = [eos] if reachable else []
    r = _host_search(ops, H, emb, n, stops, limit, lp, es, ngram)
    cut = _first_cut(r)
    if cut is not None:
        if cut == 0:
            return 0
        limit = cut                                                           # both searches again, up to the last decided step
        r = _host_search(ops, H, emb, n, stops, limit, lp, es, ngram)
        assert _first_cut(r) is None
    E, _ = _engine(dtype, n, eos_id=eos)
    if ngram:
        E.set_logits_rules(no_repeat_ngram_size=ngram)
        E.set_history(PROMPT, slot=0)
    E.select(0).reset()
    E.prefill(emb[PROMPT])
    got = E.beam_search(limit, PROMPT[-1], n, length_penalty=lp, early_stopping=es)
    what = (KC.NAME[dtype], n, ngram, reachable, cut)
    assert got["sequences"] == r["sequences"], (what, got["sequences"], r["sequences"])
    assert got["finished"].tolist() == r["finished"], what
    for s, ref, seq in zip(got["scores"].tolist(), r["scores"], r["sequences"]):
        L = max(len(seq), 1)
        assert abs(s - ref) <= _bound(ref * L ** lp, L) / L ** lp + 2.0 ** -23 * abs(ref), (what, s, ref)
    assert E.last_beam_state.step == len(r["steps"]) and E.last_beam_state.ended == 1
    if reachable:
        assert any(c[2] == eos for cands in r["steps"] for c in cands[:n]), what      # a hypothesis finished at the stop id
    return cut


CASES = list(itertools.product([torch.float32, torch.bfloat16], [2, 4], [0, 2], [False, True]))


@pytest.mark.parametrize("dtype,n,ngram,reachable", CASES, ids=lambda v: KC.NAME.get(v, str(v)) if isinstance(v, torch.dtype) else str(v))
def test_engine_search_equals_host_driven_search(ops, dtype, n, ngram, reachable):
    _engine_case(dtype, n, ngram, reachable)


def test_engine_search_cases_are_mostly_uncut(ops):
    cuts = [_engine_case(*c) for c in CASES]
    assert sum(1 for c in cuts if c is not None and c < 6) <= 1, cuts


# ---- 4. one beam is greedy ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=lambda d: KC.NAME[d])
def test_one_beam_equals_greedy(dtype):
    limit, eos = 12, 7
    eng, emb = _engine(dtype, 2, eos_id=eos, img_ids=list(range(260, 290)))
    eng.lm_head[eos].zero_()                                    # the stop id unreachable: a zero row, and banned up to the limit
    eng.set_logits_rules(min_new_tokens=limit)
    runs = []
    for beam in (False, True):
        eng.select(0).reset()
        eng.set_history(PROMPT, slot=0)
        eng.prefill(emb[PROMPT])
        if beam:
            r = eng.beam_search(limit, PROMPT[-1], 1)
            assert r["finished"].tolist() == [True]
            runs.append(r["sequences"][0])
        else:
            assert eng.generate(limit, PROMPT[-1]) == limit
            runs.append(eng.gen_ids[:limit].tolist())
    assert runs[0] == runs[1] and len(runs[0]) == limit and eos not in runs[0]
    eng.clear_logits_rules()


# ---- 5. refusals change nothing ------------------------------------------------------------------------------------------------------
def _fingerprint(eng):
    out = []
    for b in range(eng.n_seq):
        eng.select(b)
        out.append((eng.state.cpu().tolist(), eng.lengths(), int(_bits(eng.k_cache).long().sum()), int(_bits(eng.v_cache).long().sum()),
                    int(_bits(eng.logits).long().sum())))
    eng.select(0)
    return out


def test_refusals_change_nothing():
    from seedstory import _lib, ops
    eng, emb = _engine(torch.bfloat16, 4, eos_id=2)
    eng.select(0).reset()
    eng.prefill(emb[PROMPT])
    torch.cuda.synchronize()
    fp = _fingerprint(eng)
    ws = eng._beam_ws(4)

    def raw(n=2, lp=1.0, es=0, steps=4):
        bp = _lib.BeamParams(n, lp, es)
        return _lib.lib().ss_llama_beam_search(eng._h, C.byref(bp), ws.data_ptr(), steps, PROMPT[-1], ops.stream())

    def refused(fn, *a, **kw):
        with pytest.raises(_lib.SSError):
            fn(*a, **kw)
        torch.cuda.synchronize()
        assert _fingerprint(eng) == fp

    for n in (0, 5, 9):
        refused(eng.beam_search, 4, PROMPT[-1], n)
    assert raw(n=5) == -1 and b"num_beams" in _lib.lib().ss_last_error()
    assert raw(steps=eng.max_new + 1) == -1 and b"n_steps" in _lib.lib().ss_last_error()
    assert raw(steps=0) == -1
    assert raw(lp=NAN) == -1 and b"length_penalty" in _lib.lib().ss_last_error()
    assert raw(lp=INF) == -1
    assert raw(es=3) == -1 and b"early_stopping" in _lib.lib().ss_last_error()
    refused(eng.beam_search, 4, PROMPT[-1], 2, early_stopping="always")
    eng.select(1)
    assert raw() == -1 and b"slot 0" in _lib.lib().ss_last_error()
    eng.select(0)
    eng.set_sampling(temperature=1.2, seed=1, slot=1)
    refused(eng.beam_search, 4, PROMPT[-1], 2)
    eng.set_greedy()
    eng.set_logprobs(True, slot=0)
    refused(eng.beam_search, 4, PROMPT[-1], 2)
    eng.set_logprobs(False)
    eng.set_logits_rules(no_repeat_ngram_size=2, slot=1)        # rules on for a part of the group
    refused(eng.beam_search, 4, PROMPT[-1], 2)
    eng.clear_logits_rules()
    maps = eng.attn_capture_on(8, 64)
    refused(eng.beam_search, 4, PROMPT[-1], 2)
    eng.attn_capture_off()
    eng.enable_kv_fp8()
    with pytest.raises(_lib.SSError, match="fp8 KV shadow"):
        eng.beam_search(4, PROMPT[-1], 2)
    eng.disable_kv_fp8()
    torch.cuda.synchronize()
    assert _fingerprint(eng) == fp
    # and the same call goes through once nothing stands in its way
    r = eng.beam_search(4, PROMPT[-1], 2)
    assert r["finished"].tolist() == [True, True] and all(len(s) <= 4 for s in r["sequences"])


# ---- 6. generate(num_beams=) end to end on the golden tiny model --------------------------------------------------------------------
def test_llm_generate_num_beams(golden):
    from src.models_clm.generation import AutoImageTokenGenerationProcessor
    from test_fork_gpu import PROMPT as P, _Tok, _engine as _golden_engine, _img_ids, _llm
    _, meta = golden
    dtype = torch.bfloat16
    img = _img_ids(meta)
    llm, wd = _llm(meta, dtype, 4)
    llm.beam_search = True
    off, _ = _llm(meta, dtype, 4)
    proc = [AutoImageTokenGenerationProcessor(tokenizer=_Tok(img))]
    ids = P.unsqueeze(0)
    S = ids.shape[1]
    emb_w = wd["model.embed_tokens.weight"]
    kw = dict(input_ids=ids, inputs_embeds=emb_w[ids].to(DEV), logits_processor=proc)
    # switch off: num_beams is inert, bit for bit
    a = off.generate(max_new_tokens=10, **kw)
    b = off.generate(max_new_tokens=10, num_beams=3, length_penalty=2.0, **kw)
    assert a.sequences.tolist() == b.sequences.tolist() and b.beams is None
    assert all(torch.equal(_bits(x[0]), _bits(y[0])) for x, y in zip(a.hidden_states, b.hidden_states))
    # switch on: the winner is the engine's
    eng, emb = _golden_engine(meta, dtype)
    eng.select(0).prefill(emb[P])
    eng.set_stop_id(img[0])
    r = eng.beam_search(10, int(P[-1]), 3)
    eng.set_stop_id(-1)
    win = r["sequences"][0]
    out = llm.generate(max_new_tokens=10, num_beams=3, **kw)
    gen = out.sequences[0, S:].tolist()
    assert out.sequences[0, :S].tolist() == P.tolist() and gen[:len(win)] == win and 1 <= len(win) <= len(gen) <= 10
    assert [q["sequence"] for q in out.beams] == r["sequences"] and [q["finished"] for q in out.beams] == r["finished"].tolist()
    assert torch.equal(_bits(out.sequences_scores), _bits(r["scores"][:1]))
    assert torch.equal(_bits(torch.tensor([q["score"] for q in out.beams])), _bits(r["scores"]))
    assert len(out.hidden_states) == max(len(gen), 1) and out.hidden_states[0][0].shape[1] == S
    e = llm._engine
    assert e._cur == 0 and e.lengths()[0] == S + len(gen) - 1 and not e._rules_slots
    assert llm.past_key_values[0][0].shape[2] == S + len(gen) - 1 and llm.past_key_values[0][0].data_ptr() == e.k_cache.data_ptr()
    # the winner's cache is a real one: greedy from it equals greedy from a prompt that spells the winner out
    nxt = out.sequences.cpu()
    c = llm.generate(input_ids=nxt, inputs_embeds=emb_w[nxt].to(DEV), logits_processor=proc, past_key_values=llm.past_key_values,
                     max_new_tokens=6)
    d = off.generate(input_ids=nxt, inputs_embeds=emb_w[nxt].to(DEV), logits_processor=proc, max_new_tokens=6)
    assert c.sequences.shape[1] > nxt.shape[1] and c.sequences[0, :nxt.shape[1]].tolist() == nxt[0].tolist()
    assert c.sequences.shape == d.sequences.shape
    # and a beam search from the returned cache works too; rules reach the beams and are cleared
    f = llm.generate(input_ids=nxt, inputs_embeds=emb_w[nxt].to(DEV), logits_processor=proc, past_key_values=llm.past_key_values,
                     max_new_tokens=6, num_beams=2, no_repeat_ngram_size=2, early_stopping=True)
    assert f.beams is not None and f.sequences[0, :nxt.shape[1]].tolist() == nxt[0].tolist() and not e._rules_slots


@pytest.mark.parametrize("block", [1, 0], ids=["block", "token_by_token"])
def test_continuous_lvlm_beams_open_an_image(golden, block):
    """``<img>`` ends a hypothesis whether the forced ids behind it then run as one batched block or token by token"""
    from seedstory import _lib
    from src.models.qwen_visual import Resampler
    from src.models_clm.models import ContinuousLVLM
    from test_fork_gpu import PROMPT as P, _Tok, _img_ids, _llm
    _, meta = golden
    dtype = torch.bfloat16
    img = _img_ids(meta)
    probe, wd = _llm(meta, dtype, 1)
    ids = P.unsqueeze(0)
    S = ids.shape[1]
    h = probe.generate(input_ids=ids, inputs_embeds=wd["model.embed_tokens.weight"][ids].to(DEV), max_new_tokens=1).hidden_states[0][0][0, -1].float()
    llm, _ = _llm(meta, dtype, 4)
    llm.beam_search = True
    llm.lm_head.weight.data[img[0]] = (8.0 / float(h @ h) * h).to(dtype)       # <img> is the prompt's likeliest continuation
    rin = Resampler(grid_size=meta["RES_IN"]["grid"], embed_dim=256, num_heads=2, kv_dim=256)
    rin.load_state_dict(synth.resampler_weights(21, "", meta["RES_IN"]["grid"], 256))
    rout = Resampler(grid_size=meta["RES_OUT"]["grid"], embed_dim=256, num_heads=2, kv_dim=256)
    rout.load_state_dict(synth.resampler_weights(22, "", meta["RES_OUT"]["grid"], 256))
    agent = ContinuousLVLM(llm, rin, rout).eval().to(DEV, dtype)
    agent.llm.n_seq = 4
    old = _lib.get_tuning("img_block_decode", 1)
    _lib.set_tuning("img_block_decode", block)
    try:
        out = agent.generate(tokenizer=_Tok(img), input_ids=ids, max_new_tokens=80, num_img_gen_tokens=64, num_beams=2,
                             length_penalty=1.0, early_stopping=True)
    finally:
        _lib.set_tuning("img_block_decode", old)
    g = out["generate_ids"].tolist()
    assert out["beams"][0]["sequence"] == [img[0]] and out["beams"][0]["finished"]
    assert out["sequences_scores"].shape == (1,) and float(out["sequences_scores"]) == out["beams"][0]["score"] < 0
    assert g[0] == img[0] and g[1:66] == img[1:]                               # the image block follows the winner
    assert out["has_img_output"] and out["img_gen_feat"].shape[0] == 1
    eng = agent.llm._engine
    assert eng._cur == 0 and eng.lengths()[0] == S + len(g) - 1 and out["past_key_values"][0][0].shape[2] == S + len(g) - 1

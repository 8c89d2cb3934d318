"""Token log-probabilities on the GPU: ``ss_token_logprobs`` against the fp64 reference of tests/logprobs_ref.py within the
allowance derived in tests/test_logprobs_cpu.py (every element, guarded outputs), exact probes, the sampling form against the
sampler's oracle, and the engine paths (recorded values == the operator on the replayed logits bit for bit, greedy / sampling /
rules, captured and eager, nothing else changes, mixed slots, the image-token block, ``LlamaForCausalLM.generate``)."""
import contextlib
import math

import numpy as np
import pytest
import torch

import kernel_check as KC
import logprobs_ref as R
import synth
from test_logprobs_cpu import LP_A, LP_B, LPS_A, LPS_B
from test_sampling_cpu import oracle

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
VOCABS = [7, 1003, 32066, 65535]            # below one wave | no multiple of the block | the story model's | the largest
INF, NAN = float("inf"), float("nan")


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (no CPU fallback exists)")
    from seedstory import ops as _ops
    return _ops


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
    return t.contiguous().view(torch.int32 if t.dtype in (torch.float32, torch.int32) else torch.int16)


def _guarded_call(z, ids, top_n, sampling=None, ld=None, offset=0):
    """ss_token_logprobs through the C ABI: the rows in a guarded buffer (row stride ld: the gaps hold the NaN sentinel),
    every output in a guarded buffer of its own -> (lp [rows], top_ids [rows, top_n], top_lp [rows, top_n]) on the CPU.
    Asserts the rows were only read, every output element was written and nothing around any of them."""
    import ctypes as C
    from seedstory import _lib, ops
    rows, vocab = z.shape
    src = KC.GuardedOut(rows, vocab, z.dtype, device=DEV, ld=ld, offset=offset)
    src.out.copy_(z.to(DEV))
    tok = torch.tensor(ids, dtype=torch.int32, device=DEV)
    lp = KC.GuardedOut(rows, 1, torch.float32, device=DEV)
    tid = KC.GuardedOut(rows, max(top_n, 1), torch.float32, device=DEV)      # int32 ids in a 4-byte guarded buffer
    tlp = KC.GuardedOut(rows, max(top_n, 1), torch.float32, device=DEV)
    sps = None if sampling is None else ops.sampling_struct(**sampling)
    _lib.check(_lib.lib().ss_token_logprobs(src.data_ptr(), rows, vocab, src.ld if rows > 1 else vocab, tok.data_ptr(),
                                            None if sps is None else C.byref(sps), top_n, lp.data_ptr(),
                                            tid.data_ptr() if top_n else None, tlp.data_ptr() if top_n else None, ops.dt(z.dtype),
                                            ops.stream()), "ss_token_logprobs")
    what = "token_logprobs %s vocab %d rows %d" % (KC.NAME[z.dtype], vocab, rows)
    assert torch.equal(_bits(src.check(what + " (input)")), _bits(z))
    got = lp.check(what + " (lp)").view(-1)
    if not top_n:
        for b in (tid, tlp):        # not touched at all
            assert all("never written" in m for m in b.problems()[0]), what
        return got, None, None
    return got, tid.check(what + " (top ids)").view(torch.int32), tlp.check(what + " (top lp)")


def _check_rows(z, ids, got, a, b, what, sampling=None, need_decided=True):
    lp, tid, tlp = got
    for r in range(z.shape[0]):
        row = z[r].double().numpy()
        ref, decided = R.policy_logprob(row, ids[r], sampling)
        assert decided or not need_decided, (what, r, "the oracle does not decide this row's kept set")
        if not decided:
            continue                # (engine replays only: a threshold tie the fp32 masses may settle either way)
        assert R.within(lp[r], ref, a, b), (what, r, ids[r], float(lp[r]), ref, a + b * abs(ref))
        if tid is not None:
            rid, rlp = R.top_n(row, tid.shape[1])
            assert tid[r].tolist() == rid.tolist(), (what, r, tid[r].tolist(), rid.tolist())
            for j in range(tid.shape[1]):
                assert R.within(tlp[r, j], rlp[j], LP_A, LP_B), (what, r, j, float(tlp[r, j]), rlp[j])


# ---- the operator against the reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: KC.NAME[d])
def test_operator_against_reference(ops, dtype):
    """N(0, 4^2) logits rounded to the dtype (16-bit rows are full of ties: the top-n ids must still be the reference's), one id
    per row: the row's arg max, a random id, the row's arg min.  ld > vocab with NaN in the padding; one row also off a 16-byte
    boundary.  Every element of every output within the allowance."""
    g = torch.Generator().manual_seed(4321 + DTYPES.index(dtype))
    for vocab in VOCABS:
        for rows in (1, 3):
            z = (torch.randn(rows, vocab, generator=g) * 4.0).to(dtype)
            pick = [int(z[0].float().argmax()), int(torch.randint(vocab, (1,), generator=g)), int(z[rows - 1].float().argmin())]
            ids = pick[:rows] if rows == 3 else pick[1:2]
            for top_n in (0, 5, 8):
                got = _guarded_call(z, ids, top_n, ld=vocab + 5, offset=1 if rows == 1 else 0)
                _check_rows(z, ids, got, LP_A, LP_B, (KC.NAME[dtype], vocab, rows, top_n))
            # the Python wrapper returns the same bits
            lp, tid, tlp = ops.token_logprobs(z.to(DEV), ids, top_n=5)
            assert torch.equal(_bits(lp.cpu()), _bits(got[0])) and torch.equal(tid.cpu()[:, :5], got[1][:, :5])


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: KC.NAME[d])
def test_operator_exact_probes(ops, dtype):
    big = float(torch.finfo(dtype).max)
    for vocab in (7, 1003, 32066):
        a, b, c = 1, vocab // 2, vocab - 1
        # one finite entry among -inf: exactly 0.0; a chosen -inf entry: -inf; fewer live entries than top_n: -1 / -inf
        z = torch.full((2, vocab), -INF)
        z[:, b] = -3.25
        lp, tid, tlp = _guarded_call(z.to(dtype), [b, a], 3)
        assert lp.tolist() == [0.0, -INF] and tid.tolist() == [[b, -1, -1]] * 2 and tlp.tolist() == [[0.0, -INF, -INF]] * 2
        # V equal entries: -log V, and the top-n in id order
        z = torch.full((1, vocab), 1.5)
        lp, tid, tlp = _guarded_call(z.to(dtype), [c], 4)
        assert R.within(lp[0], -math.log(vocab), LP_A, LP_B) and tid.tolist() == [[0, 1, 2, 3]]
        assert tlp[0].tolist() == [float(lp[0])] * 4
        # two equal maxima over a floor far below: -log 2 each up to the allowance, ties by ascending id, then the floor by id
        z = torch.full((2, vocab), -80.0)
        z[:, a] = z[:, c] = 7.0
        lp, tid, tlp = _guarded_call(z.to(dtype), [a, c], 3)
        assert lp[0] == lp[1] and R.within(lp[0], -math.log(2), LP_A, LP_B) and tid.tolist() == [[a, c, 0]] * 2
        assert tlp[0, 0] == tlp[0, 1] == lp[0] and R.within(tlp[0, 2], -87.0 - math.log(2), LP_A, LP_B)
        # a NaN elsewhere in the row carries no mass: the bits of the row with -inf in its place; a chosen NaN gives NaN
        g = torch.Generator().manual_seed(vocab)
        z = (torch.randn(2, vocab, generator=g) * 3.0).to(dtype)
        zn, zi = z.clone(), z.clone()
        zn[:, b], zi[:, b] = NAN, -INF
        got_n, got_i = _guarded_call(zn, [a, b], 5), _guarded_call(zi, [a, b], 5)
        assert torch.equal(_bits(got_n[0][:1]), _bits(got_i[0][:1])) and math.isnan(float(got_n[0][1])) and float(got_i[0][1]) == -INF
        assert torch.equal(got_n[1], got_i[1]) and torch.equal(_bits(got_n[2]), _bits(got_i[2])) and not torch.isnan(got_n[2]).any()
        _check_rows(zn, [a, b], got_n, LP_A, LP_B, ("nan", KC.NAME[dtype], vocab))
        # entries at +- the largest finite value: no overflow turns into a NaN
        z = (torch.randn(2, vocab, generator=g) * 3.0).to(dtype)
        z[:, a], z[:, c] = big, -big
        z[1, b] = big
        got = _guarded_call(z, [a, c], 4)
        assert not torch.isnan(got[0]).any() and not torch.isnan(got[2]).any()
        _check_rows(z, [a, c], got, LP_A, LP_B, ("extremes", KC.NAME[dtype], vocab))
        assert got[0][0] == 0.0 and R.within(got[0][1], -2.0 * big - math.log(2), LP_A, LP_B)
        # no entry with mass at all: by the entry alone
        z = torch.full((2, vocab), -INF)
        z[:, a] = NAN
        lp, tid, tlp = _guarded_call(z.to(dtype), [a, b], 2)
        assert math.isnan(float(lp[0])) and float(lp[1]) == -INF and tid.tolist() == [[-1, -1]] * 2 and tlp.tolist() == [[-INF, -INF]] * 2
    # an id outside the row is never used as an index
    z = torch.zeros(2, 64).to(dtype)
    lp = ops.token_logprobs(z.to(DEV), [64, -1]).cpu()
    assert torch.isnan(lp).all()
    lp = ops.token_logprobs(z.to(DEV), [64, -1], sampling=dict(temperature=1.0)).cpu()
    assert lp.tolist() == [-INF, -INF]


SAMPLING_CASES = [(0.7, 0, 0.5), (1.0, 50, 0.9), (1.3, 0, 1.0), (0.7, 0, 0.95), (0.9, 5, 1.0)]      # (temperature, top_k, top_p)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: KC.NAME[d])
def test_operator_sampling_form(ops, dtype):
    """log(w / Z_P) over the sampler's kept set: four rows per case from a fixed seed, scored at the arg max, at two other kept
    ids (when there are that many) and at an id outside the set (-inf).  The oracle decides every row's kept set at DELTA —
    asserted, none skipped."""
    for vocab in VOCABS:
        for ci, (T, k, p) in enumerate(SAMPLING_CASES):
            g = torch.Generator().manual_seed(1000 * ci + vocab % 997 + 10 * DTYPES.index(dtype))
            z = (torch.randn(4, vocab, generator=g) * 4.0).to(dtype)
            ids = []
            for r in range(4):
                o = oracle(z[r].double().numpy(), T, k, p, u=0.0)
                kept, out = np.flatnonzero(o["kept"]), np.flatnonzero(~o["kept"])
                by_w = kept[np.argsort(-o["prob"][kept], kind="stable")]
                ids.append(int(out[0]) if r == 3 and out.size else int(by_w[min(r, by_w.size - 1)]))
            sp = dict(temperature=T, top_k=k, top_p=p)
            got = _guarded_call(z, ids, 3 if ci % 2 else 0, sampling=sp, ld=vocab + 3)
            _check_rows(z, ids, got, LPS_A, LPS_B, ("sampling", KC.NAME[dtype], vocab, (T, k, p)), sampling=sp)
            if vocab == 1003:       # one row off a 16-byte boundary (the sampler's other load path): the same allowance
                got1 = _guarded_call(z[:1], ids[:1], 0, sampling=sp, offset=3)
                _check_rows(z[:1], ids[:1], got1, LPS_A, LPS_B, ("sampling, offset", KC.NAME[dtype], (T, k, p)), sampling=sp)


def test_operator_error_cases(ops):
    from seedstory import _lib
    z = torch.zeros(2, 64, device=DEV)
    for kw in (dict(top_n=9), dict(top_n=-1), dict(top_n=1.5), dict(sampling=dict(temperature=0.0)), dict(sampling=dict(top_p=1.5))):
        with pytest.raises(_lib.SSError):
            ops.token_logprobs(z, [1, 2], **kw)
    with pytest.raises(_lib.SSError):
        ops.token_logprobs(z, [1, 2, 3])
    with pytest.raises(_lib.SSError):
        ops.token_logprobs(torch.zeros(1, 65536, device=DEV), [0])


# ---- the engine ------------------------------------------------------------------------------------------------------------------
def _img_ids(meta):
    lo, hi = meta["IMG_IDS"]
    return list(range(lo, hi + 1))


def _engine(meta, dtype, img_ids=None, **kw):
    from seedstory.llama import LlamaEngine
    d = meta["LLAMA"]
    wd = synth.llama_weights(11, d["hidden"], d["n_heads"], d["n_layers"], d["inter"], d["vocab"], dtype=dtype)
    eng = LlamaEngine(wd, hidden=d["hidden"], n_heads=d["n_heads"], n_layers=d["n_layers"], inter=d["inter"],
                      vocab=d["vocab"], dtype=dtype, device=DEV, cache_cap=256, max_new=128, max_prefill_rows=80,
                      img_ids=_img_ids(meta) if img_ids is None else img_ids, **kw)
    return eng, wd["model.embed_tokens.weight"]


PROMPT = torch.cat([synth.randint(91, (12,), 3, 250)] * 2)[:21]        # a prompt that repeats itself: every id is in the history
ENGINE_DTYPES = [torch.bfloat16, torch.float16]
SAMPLING = dict(temperature=1.5, top_k=0, top_p=0.95)
# a penalty below 1 RAISES the ids of the history: the chosen tokens are penalised ones (asserted where it is used)
RULES = dict(repetition_penalty=0.6, no_repeat_ngram_size=4, min_new_tokens=0)
TOP = 3


def _run(eng, emb, n, history=False, **kw):
    eng.reset()
    eng.prefill(emb[PROMPT])
    if history:
        eng.set_history(PROMPT.tolist())
    k = eng.generate(n, int(PROMPT[-1]), **kw)
    out = dict(ids=eng.gen_ids[:k].tolist(), hid=eng.hidden_rows[:max(k - 1, 0)].clone(), logits=eng.logits.clone())
    if eng._lp_slots:
        out["lp"] = {key: v.clone().cpu() for key, v in eng.logprobs(k).items()}
    return out


def _replay_and_check(ops, rep, emb, img, run, n_forced=0, sampling=None, rules=None):
    """`rep` is an engine over the same weights WITHOUT image ids, every option off: its opening kernel leaves the logits row
    alone, so before step j its logits are the raw row the recording engine saw (the same decode kernels on the same inputs),
    and ``generate(2, last, forced=[tok, 3])`` feeds tok (a one-token call would emit it without feeding it).  The recorded
    values equal the operator on those rows bit for bit, and the reference within the allowance.  -> how many tokens were
    free, how many of those were ids of the history"""
    ids, lp = run["ids"], run["lp"]
    rep.reset()
    rep.prefill(emb[PROMPT])
    hist, last = PROMPT.tolist(), int(PROMPT[-1])
    free = penalised = 0
    for j, tok in enumerate(ids):
        raw = rep.logits.clone().view(1, -1)
        m_lp, m_ids, m_top = ops.token_logprobs(raw, [tok], top_n=TOP)
        assert torch.equal(_bits(lp["model_logprob"][j:j + 1]), _bits(m_lp.cpu())), (j, tok)
        assert torch.equal(lp["top_ids"][j], m_ids.cpu()[0]) and torch.equal(_bits(lp["top_logprobs"][j]), _bits(m_top.cpu()[0])), (j, tok)
        _check_rows(raw.cpu(), [tok], (lp["model_logprob"][j:j + 1], lp["top_ids"][j:j + 1], lp["top_logprobs"][j:j + 1]), LP_A, LP_B,
                    ("engine model_logprob", j))
        z = raw.clone()
        if rules:
            ops.process_logits(z, [hist], prompt_len=[len(PROMPT)], eos_id=rep.eos_id, img_ids=img, **rules)
        ops.imgproc_argmax(z.view(-1), last, img)
        got = lp["logprob"][j:j + 1]
        if j < n_forced or last in img[:-1]:
            assert float(got) == 0.0 and math.copysign(1.0, float(got)) == 1.0, (j, tok, float(got))
        else:
            free += 1
            penalised += int(tok in hist)
            want = ops.token_logprobs(z, [tok], sampling=sampling).cpu()
            assert torch.equal(_bits(got), _bits(want)), (j, tok, float(got), float(want))
            a, b = (LPS_A, LPS_B) if sampling else (LP_A, LP_B)
            _check_rows(z.cpu(), [tok], (got, None, None), a, b, ("engine logprob", j), sampling=sampling, need_decided=False)
            assert float(got) <= 0.0 and math.isfinite(float(got))
        if tok == rep.eos_id or j + 1 == len(ids):
            break
        assert rep.generate(2, last, forced=[tok, 3]) == 2
        hist.append(tok)
        last = tok
    return free, penalised


@pytest.mark.parametrize("graph", [1, 0], ids=["captured", "eager"])
@pytest.mark.parametrize("dtype", ENGINE_DTYPES, ids=lambda d: KC.NAME[d])
def test_engine_records_what_the_operator_computes(ops, golden, dtype, graph):
    """Greedy, sampling, and rules + greedy (whose chosen tokens are penalised ones), each recorded once and replayed; a run
    that starts with forced tokens ending in <img> covers the forced and the certain-successor zeros.  With the feature on,
    ids, hidden rows and the last logits row are the bits of a run with it off."""
    _, meta = golden
    img = _img_ids(meta)
    eng, emb = _engine(meta, dtype)
    rep, _ = _engine(meta, dtype, img_ids=[])
    with knobs(llama_graph=graph):
        cases = [("greedy", None, None, {}), ("forced", None, None, dict(forced=[5, img[0]])), ("sampling", SAMPLING, None, {}),
                 ("rules", None, RULES, {})]
        for name, sampling, rules, kw in cases:
            def once(lp_on):
                eng.set_logprobs(lp_on, top_n=TOP)
                if sampling:
                    eng.set_sampling(seed=77, **sampling)
                if rules:
                    eng.set_logits_rules(**rules)
                try:
                    return _run(eng, emb, 16, history=bool(rules), **kw)
                finally:
                    eng.set_greedy()
                    eng.clear_logits_rules()
                    eng.set_logprobs(False)
            off, on = once(False), once(True)
            assert on["ids"] == off["ids"] and torch.equal(_bits(on["hid"]), _bits(off["hid"])), name
            assert torch.equal(_bits(on["logits"]), _bits(off["logits"])), name
            assert len(on["ids"]) == 16 and "lp" not in off
            free, penalised = _replay_and_check(ops, rep, emb, img, on, n_forced=len(kw.get("forced", [])), sampling=sampling, rules=rules)
            if name == "forced":
                assert on["ids"][:6] == [5] + img[:5] and on["lp"]["logprob"].tolist() == [0.0] * 16 and free == 0
                assert (on["lp"]["model_logprob"] < 0).all()
            else:
                assert free >= 1, (name, free)
            if name == "rules":
                assert penalised >= 1, "no chosen token was an id of the history: the rules case shows nothing"
                assert not torch.equal(on["lp"]["logprob"], on["lp"]["model_logprob"])
            if name == "greedy":        # every top-1 entry of a free greedy token under the processor's zeros is at least the token's
                assert (on["lp"]["top_logprobs"][:, 0] >= on["lp"]["model_logprob"]).all()


@pytest.mark.parametrize("dtype", ENGINE_DTYPES, ids=lambda d: KC.NAME[d])
def test_engine_draw_counter_untouched(golden, dtype):
    """Two sampled calls in a row without resetting the sampler: the second depends on the draw counter the first left."""
    _, meta = golden
    eng, emb = _engine(meta, dtype)
    runs = {}
    for lp_on in (False, True):
        eng.set_logprobs(lp_on, top_n=2)
        eng.set_sampling(seed=5, **SAMPLING)
        runs[lp_on] = [_run(eng, emb, 12), _run(eng, emb, 12)]
    eng.set_logprobs(False)
    eng.set_greedy()
    for a, b in zip(runs[False], runs[True]):
        assert a["ids"] == b["ids"] and torch.equal(_bits(a["hid"]), _bits(b["hid"])) and torch.equal(_bits(a["logits"]), _bits(b["logits"]))
    assert runs[True][0]["ids"] != runs[True][1]["ids"]


@pytest.mark.parametrize("dtype", ENGINE_DTYPES, ids=lambda d: KC.NAME[d])
def test_engine_mixed_slots_leave_off_slots_untouched(golden, dtype):
    _, meta = golden
    S, SENT = 4, -777.0
    eng, emb = _engine(meta, dtype, n_seq=S)
    lasts = [int(PROMPT[-1])] * S
    forced = [[], [7], [8, 9], [10]]            # the slots diverge; slot 3 stops early at EOS

    def run(slots):
        eng.set_logprobs(False)
        for b in slots:
            eng.set_logprobs(True, top_n=2, slot=b)
        if eng._lp is not None:
            for t in eng._lp:
                t.fill_(SENT)
        for b in range(S):
            eng.select(b).reset()
            eng.select(b).prefill(emb[PROMPT])
        ns = eng.generate_batch(10, lasts, forced=[forced[0], forced[1], forced[2], forced[3] + [eng.eos_id]])
        ids = [eng.select(b).gen_ids[:ns[b]].tolist() for b in range(S)]
        return ns, ids, None if eng._lp is None else [t.clone().cpu() for t in eng._lp]

    ns0, ids0, none = run([])
    assert none is None and ns0[3] == 2 and ns0[0] == 10
    ns_all, ids_all, all_on = run(range(S))
    ns_mix, ids_mix, mix = run([1, 3])
    assert ids_all == ids0 and ids_mix == ids0
    for t_all, t_mix in zip(all_on, mix):
        for b in range(S):
            k = ns0[b] * (2 if t_mix.dim() == 3 else 1)
            flat_all, flat_mix = t_all[b].reshape(-1), t_mix[b].reshape(-1)
            if b in (1, 3):
                assert torch.equal(_bits(flat_mix[:k]), _bits(flat_all[:k])), b
                assert (flat_mix[:k] != SENT).all()
                assert (flat_mix[k:] == SENT).all() and (flat_all[k:] == SENT).all(), b      # a done slot writes nothing
            else:
                assert (flat_mix == SENT).all(), b                                           # a feature-off slot writes nothing
    assert all_on[1][3, :2].tolist() == [0.0, 0.0] and all_on[1][1, 0] == 0.0 and all_on[1][1, 1] < 0.0      # forced, then free
    eng.set_logprobs(False)


@pytest.mark.parametrize("dtype", ENGINE_DTYPES, ids=lambda d: KC.NAME[d])
def test_engine_img_block_values(ops, golden, dtype):
    """The block path: two forced tokens ending in <img>, the 65 block tokens as one batched forward, four free tokens.  Block
    entries: ``logprob`` 0.0 and the operator / the reference on ``ops.gemm(hidden rows of the block, lm_head)`` recomputed
    here; the loop's entries are the engine's own.  ``img_block_logits`` off changes nothing."""
    _, meta = golden
    img = _img_ids(meta)
    eng, emb = _engine(meta, dtype)
    n = 2 + 65 + 4
    outs = []
    for knob in (1, 0):
        with knobs(img_block_decode=1, img_block_logits=knob):
            eng.set_logprobs(True, top_n=TOP)
            eng.reset()
            eng.prefill(emb[PROMPT])
            ids, hid = eng.generate_img_block(n, int(PROMPT[-1]), forced=[5, img[0]])
            outs.append((ids, hid.clone(), {k: v.clone().cpu() for k, v in eng.last_logprobs.items()}))
            eng.set_logprobs(False)
    ids, hid, lp = outs[0]
    assert ids[:67] == [5] + img and len(ids) == n
    assert outs[1][0] == ids and all(torch.equal(_bits(outs[1][2][k]), _bits(lp[k])) for k in lp)
    assert {k: tuple(v.shape) for k, v in lp.items()} == {"logprob": (n,), "model_logprob": (n,), "top_ids": (n, TOP), "top_logprobs": (n, TOP)}
    # hidden row j belongs to the fed token ids[j] and scores ids[j + 1]: the block fed ids[1 .. 67) as 66 rows
    lg = ops.gemm(hid[1:67].contiguous(), eng.lm_head)[:65]
    toks = ids[2:67]
    w_lp, w_ids, w_top = ops.token_logprobs(lg, toks, top_n=TOP)
    blk = slice(2, 67)
    assert lp["logprob"][:67].tolist() == [0.0] * 67                                   # forced, forced, the block
    assert torch.equal(_bits(lp["model_logprob"][blk]), _bits(w_lp.cpu())) and torch.equal(lp["top_ids"][blk], w_ids.cpu())
    assert torch.equal(_bits(lp["top_logprobs"][blk]), _bits(w_top.cpu()))
    _check_rows(lg.cpu(), toks, (lp["model_logprob"][blk], lp["top_ids"][blk], lp["top_logprobs"][blk]), LP_A, LP_B, "block")
    tail = lp["logprob"][67:]
    assert (tail < 0).all() and torch.isfinite(tail).all() and torch.isfinite(lp["model_logprob"]).all()
    # with the feature off nothing is assembled
    eng.reset()
    eng.prefill(emb[PROMPT])
    assert eng.generate_img_block(n, int(PROMPT[-1]), forced=[5, img[0]])[0] == ids and eng.last_logprobs is None


def test_engine_refuses_bad_arguments(golden):
    from seedstory import _lib
    _, meta = golden
    eng, emb = _engine(meta, torch.bfloat16)
    greedy = _run(eng, emb, 8)["ids"]
    for kw in (dict(top_n=9), dict(top_n=-1), dict(top_n=2.5), dict(slot=1), dict(slot=-2)):
        with pytest.raises(_lib.SSError):
            eng.set_logprobs(True, **kw)
    with pytest.raises(_lib.SSError):
        eng.logprobs(4)                         # nothing records
    # the C entry point itself: a bad slot, top_n and a half-NULL set are refused before anything is written
    buf = torch.zeros(eng.max_new * 8, device=DEV)
    p, lib = buf.data_ptr(), _lib.lib()
    for args in ((1, p, p, None, None, 0), (-2, p, p, None, None, 0), (0, p, p, p, p, 9), (0, p, None, None, None, 0), (0, p, p, p, None, 2),
                 (-1, None, None, p, p, 2)):
        assert lib.ss_llama_set_logprobs(eng._h, *args) == -1 and lib.ss_last_error(), args
    assert not eng._lp_slots and _run(eng, emb, 8)["ids"] == greedy


class _Tok:
    def __init__(self, ids):
        self.ids = ids

    def encode(self, s, add_special_tokens=False):
        return list(self.ids)


@pytest.mark.parametrize("block", [1, 0], ids=["img_block", "token_loop"])
@pytest.mark.parametrize("dtype", ENGINE_DTYPES, ids=lambda d: KC.NAME[d])
def test_llm_generate_output_logprobs(golden, dtype, block):
    from src.models_clm.generation import AutoImageTokenGenerationProcessor
    from src.models_clm.modeling_llama_xformer import LlamaConfig, LlamaForCausalLM
    _, meta = golden
    d = meta["LLAMA"]
    wd = synth.llama_weights(11, d["hidden"], d["n_heads"], d["n_layers"], d["inter"], d["vocab"], dtype=dtype)
    cfg = LlamaConfig(hidden_size=d["hidden"], intermediate_size=d["inter"], num_hidden_layers=d["n_layers"],
                      num_attention_heads=d["n_heads"], vocab_size=d["vocab"])
    llm = LlamaForCausalLM(cfg)
    llm.load_state_dict(wd, strict=False)
    llm = llm.to(DEV, dtype=dtype)
    llm.cache_cap, llm.max_new, llm.max_prefill_rows = 256, 96, 80
    llm.use_kv_cache_head = False
    img = _img_ids(meta)
    proc = [AutoImageTokenGenerationProcessor(tokenizer=_Tok(img))]
    ids = PROMPT.unsqueeze(0)
    kw = dict(input_ids=ids, inputs_embeds=wd["model.embed_tokens.weight"][ids].to(DEV), logits_processor=proc,
              forced_tokens=[5, img[0]])
    with knobs(img_block_decode=block):
        plain = llm.generate(max_new_tokens=72, **kw)
        out = llm.generate(max_new_tokens=72, output_logprobs=True, top_logprobs=3, **kw)
        n = out.sequences.shape[1] - ids.shape[1]
        assert n == 72 and out.sequences.tolist() == plain.sequences.tolist() and plain.logprobs is None
        assert out.logprobs.shape == out.model_logprobs.shape == (n,) and out.top_logprob_ids.shape == out.top_logprob_values.shape == (n, 3)
        assert out.logprobs.dtype == out.model_logprobs.dtype == out.top_logprob_values.dtype == torch.float32
        assert out.logprobs[:67].tolist() == [0.0] * 67 and (out.logprobs[67:] < 0).all() and (out.model_logprobs < 0).all()
        assert (out.top_logprob_values[:, 0] >= out.model_logprobs).all()
        assert (out.top_logprob_values[:, :-1] >= out.top_logprob_values[:, 1:]).all()
        eng = llm._engine
        assert not eng._lp_slots and eng._lp is None                    # the engine is clean afterwards
        with pytest.raises(ValueError):                                 # raised inside _generate, after the feature was switched on
            llm.generate(max_new_tokens=97, output_logprobs=True, **kw)
        assert not eng._lp_slots
        again = llm.generate(max_new_tokens=72, **kw)
        assert again.sequences.tolist() == plain.sequences.tolist() and again.logprobs is None

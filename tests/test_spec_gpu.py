"""Prompt-lookup speculative decoding in the engine, on the GPU: every case runs the tiny golden model twice — a plain greedy
engine and an engine with ``set_speculation`` — on the same weights and prompt, and asks for greedy's ids, count, lengths, hidden
rows and cache rows [0, kv_len) (tolerances of ``test_llama_slot_batched_decode_equals_single``), and for the counters
``tests/spec_ref.py`` predicts when it replays the call on the CPU with greedy's ids as the arg-max oracle.

The tie precondition.  A one-row token and an R-row token take different GEMV kernels and the speculative attention kernel orders
its sums differently from both, so the ids can only be equal away from near-ties of the top two logits.  Every case first ASSERTS
(``set_logprobs(top_n=2)`` on the greedy engine) that the top-2 log-probability margin of every free step exceeds m; m = 4 x the
largest per-token |delta log-prob| of the top two ids between one slot and N identical lock-step slots (N = 2, 4, 8) of the code
without speculation, measured on an MI355X over 20 prompts of 14 steps:

    bf16 0.00779 (fp8 decode weights 0.00400, MXFP4 0.00394)   ->  m = 0.03117 (0.016012, 0.015753)
    fp16 0.00097 (0.00098, 0.00099)                            ->  m = 0.003891 (0.003933, 0.003944)
    fp32 4.8e-7                                                ->  m = 1.9073e-06

The prompts (``synth.randint`` seeds, 8 ids repeated once so that lookup finds n-grams) were chosen from a scan of 400 seeds of
greedy's own margins on the GPU (plain and with the forced prefix of the lookup cases): three per dtype and weight mode that clear
m by a quarter or more in every case that uses them.  The CPU oracle was not used for the choice.
"""
import functools

import pytest
import torch

import kernel_check as KC
import spec_ref
import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF, FH, F32 = torch.bfloat16, torch.float16, torch.float32
EOS = 2
STEPS = 14              # 13 forwards: no multiple of 2, 4 or 8
# (dtype, decode weights) -> m
M = {(BF, None): 0.03117, (BF, "fp8"): 0.016012, (BF, "mxfp4"): 0.015753, (FH, None): 0.003891, (FH, "fp8"): 0.003933,
     (FH, "mxfp4"): 0.003944, (F32, None): 1.9073e-06}
# (dtype, decode weights) -> prompt seeds whose free steps all clear m
SEEDS = {(BF, None): [298, 259, 164], (BF, "fp8"): [298, 243, 396], (BF, "mxfp4"): [101, 73, 113], (FH, None): [298, 259, 164],
         (FH, "fp8"): [130, 40, 104], (FH, "mxfp4"): [101, 113, 73], (F32, None): [298, 259, 164]}


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _engine(meta, dtype, **kw):
    from seedstory.llama import LlamaEngine
    d = meta["LLAMA"]
    lo, hi = meta["IMG_IDS"]
    kw.setdefault("cache_cap", 256)
    kw.setdefault("max_new", 128)
    wd = synth.llama_weights(11, d["hidden"], d["n_heads"], d["n_layers"], d["inter"], d["vocab"], dtype=dtype)
    eng = LlamaEngine(wd, hidden=d["hidden"], n_heads=d["n_heads"], n_layers=d["n_layers"], inter=d["inter"], vocab=d["vocab"],
                      dtype=dtype, device=DEV, max_prefill_rows=64, img_ids=list(range(lo, hi + 1)), **kw)
    return eng, wd


def _prompt(seed):
    base = synth.randint(seed, (24,), 3, 250)
    return torch.cat([base[:8], base[:8], base[8:]])


_META = {}


@pytest.fixture(autouse=True)
def _meta(golden):
    _META["meta"] = golden[1]


@functools.lru_cache(maxsize=None)
def _greedy(dtype, dw, seed, steps=STEPS, forced=(), stop2=-1, cache_cap=256, max_new=128):
    """the plain greedy run (computed once per case and shared); asserts the tie precondition of its free steps"""
    eng, wd = _engine(_META["meta"], dtype, decode_weights=dw, cache_cap=cache_cap, max_new=max_new)
    pr = _prompt(seed)
    eng.set_logprobs(top_n=2)
    eng.set_stop_id(stop2)
    eng.prefill(wd["model.embed_tokens.weight"][pr])
    n = eng.generate(steps, last_prompt_id=int(pr[-1]), forced=list(forced))
    top = eng.logprobs(n)["top_logprobs"].cpu()
    free = top[len(forced):]
    m = M[(dtype, dw)]
    if free.numel():
        gap = float((free[:, 0] - free[:, 1]).min())
        print("top-2 margin %.5f (m = %.5f) %s %s seed %d" % (gap, m, KC.NAME[dtype], dw, seed))
        assert gap > m, "tie precondition: top-2 margin %.5f <= m = %.5f (%s, %s, seed %d)" % (gap, m, KC.NAME[dtype], dw, seed)
    kv = eng.lengths()[0]
    return {"n": n, "ids": eng.gen_ids[:n].tolist(), "lens": eng.lengths(), "hid": eng.hidden_rows[:max(n - 1, 0)].clone(),
            "k": eng.k_cache[:, :, :kv].clone(), "v": eng.v_cache[:, :, :kv].clone(), "logits": eng.logits.clone(), "prompt": pr}


def _spec_run(dtype, dw, seed, rows, *, source, steps=STEPS, forced=(), stop2=-1, cache_cap=256, max_new=128, given=None, max_ngram=2):
    """-> (engine after the speculative call, n, the replay's prediction)"""
    ref = _greedy(dtype, dw, seed, steps, tuple(forced), stop2, cache_cap, max_new)
    eng, wd = _engine(_META["meta"], dtype, decode_weights=dw, cache_cap=cache_cap, max_new=max_new)
    pr = ref["prompt"]
    eng.set_stop_id(stop2)
    eng.prefill(wd["model.embed_tokens.weight"][pr])
    if source == "given":
        eng.set_speculation(rows, draft_ids=ref["ids"] if given is None else given)
    else:
        eng.set_speculation(rows, max_ngram=max_ngram)
        eng.set_history(pr.tolist())
    n = eng.generate(steps, last_prompt_id=int(pr[-1]), forced=list(forced))
    stops = (EOS,) + ((stop2,) if stop2 >= 0 else ())
    want = spec_ref.replay(ref["ids"], rows=rows, limit=min(steps, max_new), max_new=max_new, kv_room=cache_cap - len(pr),
                           pos_room=4096 - len(pr), hist=pr.tolist() if source == "lookup" else (), source=source,
                           given=ref["ids"] if given is None else given, forced=list(forced), max_ngram=max_ngram, stops=stops,
                           vocab=eng.vocab)
    return eng, n, ref, want


def _same_as_greedy(eng, n, ref, dtype, what):
    tol = 1e-5 if dtype == F32 else 2e-2
    assert n == ref["n"] and eng.gen_ids[:n].tolist() == ref["ids"], what
    assert eng.lengths() == ref["lens"], what
    kv = ref["lens"][0]
    if n > 1:
        assert rel(eng.hidden_rows[:n - 1], ref["hid"]) < tol, what
    assert rel(eng.k_cache[:, :, :kv], ref["k"]) < tol and rel(eng.v_cache[:, :, :kv], ref["v"]) < tol, what
    assert rel(eng.logits, ref["logits"]) < tol, what


def _stats_as_predicted(eng, want, what):
    got = eng.spec_stats()
    assert got == {k: want[k] for k in ("steps", "drafted", "accepted", "emitted")}, (what, got, want["per_step"])


# ---- 1. given drafts = greedy's own continuation: every draft accepted --------------------------------------------------------------
@pytest.mark.parametrize("graph", [1, 0], ids=["graph", "eager"])
@pytest.mark.parametrize("dtype", [BF, FH, F32], ids=lambda d: KC.NAME[d])
@pytest.mark.parametrize("rows", [2, 4, 8])
def test_given_drafts_all_accepted(rows, dtype, graph):
    from seedstory import _lib
    _lib.set_tuning("llama_graph", graph)
    try:
        for seed in SEEDS[(dtype, None)]:
            what = "given R %d %s graph %d seed %d" % (rows, KC.NAME[dtype], graph, seed)
            eng, n, ref, want = _spec_run(dtype, None, seed, rows, source="given")
            _same_as_greedy(eng, n, ref, dtype, what)
            _stats_as_predicted(eng, want, what)
            st = eng.spec_stats()
            if n == STEPS:      # no stop id met: ceil((n - 1) / R) forwards, every full step accepts its R - 1 drafts
                assert st["steps"] == -(-(n - 1) // rows) and st["accepted"] == st["drafted"] == (n - 1) - st["steps"], what
            assert st["emitted"] == n, what
    finally:
        _lib.set_tuning("llama_graph", 1)


# ---- 2. given drafts corrupted at chosen generated positions --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF, FH, F32], ids=lambda d: KC.NAME[d])
@pytest.mark.parametrize("rows,bad", [(4, (2,)), (4, (1, 5, 6)), (8, (3, 12)), (2, (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13))])
def test_given_drafts_corrupted(rows, bad, dtype):
    seed = SEEDS[(dtype, None)][0]
    ids = _greedy(dtype, None, seed)["ids"]
    given = list(ids)
    for i in bad:
        if i < len(given):
            given[i] = 3 + (given[i] + 7) % 240      # another ordinary id: not the arg max, no stop id, no image id
            assert given[i] != ids[i]
    what = "corrupted R %d %s at %s" % (rows, KC.NAME[dtype], bad)
    eng, n, ref, want = _spec_run(dtype, None, seed, rows, source="given", given=given)
    assert want["accepted"] < want["drafted"], what                # the prediction itself sees the rejections
    _stats_as_predicted(eng, want, what)
    _same_as_greedy(eng, n, ref, dtype, what)                       # rejected K/V rows and hidden rows were overwritten


# ---- 3. lookup drafts ---------------------------------------------------------------------------------------------------------------------
LOOKUP_CASES = {
    "repetition": dict(),
    "forced_prefix": dict(forced=(7, 9, 11, 13, 15)),
    "forced_eos_midway": dict(forced=(5, 9, EOS, 4)),
    "one_row_short_of_cap": dict(cache_cap=33, steps=1),
    "cap_binds": dict(cache_cap=32 + 6, steps=6),
    "reaches_max_new": dict(max_new=12, steps=12),
    "beyond_max_new": dict(max_new=12, steps=50),
}


@pytest.mark.parametrize("dtype", [BF, FH, F32], ids=lambda d: KC.NAME[d])
@pytest.mark.parametrize("case", sorted(LOOKUP_CASES))
def test_lookup_drafts(case, dtype):
    kw = LOOKUP_CASES[case]
    for rows, seed in zip((4, 8, 2), SEEDS[(dtype, None)]):
        what = "lookup %s R %d %s seed %d" % (case, rows, KC.NAME[dtype], seed)
        eng, n, ref, want = _spec_run(dtype, None, seed, rows, source="lookup", **kw)
        _same_as_greedy(eng, n, ref, dtype, what)
        _stats_as_predicted(eng, want, what)
        assert torch.equal(eng.history[:len(ref["prompt"]) + n].cpu(), torch.tensor(ref["prompt"].tolist() + ref["ids"], dtype=torch.int32)), what


@pytest.mark.parametrize("dtype", [BF, FH, F32], ids=lambda d: KC.NAME[d])
def test_lookup_second_stop_id(dtype):
    seed = SEEDS[(dtype, None)][0]
    ids = _greedy(dtype, None, seed)["ids"]
    first = {}
    for i, t in enumerate(ids[:-1]):
        first.setdefault(t, i)
    stop2 = max(first, key=first.get)       # the id greedy meets last on its way: the call now ends at its first occurrence
    assert first[stop2] >= 3
    eng, n, ref, want = _spec_run(dtype, None, seed, 4, source="lookup", stop2=stop2)
    assert n == ids.index(stop2) + 1 < STEPS
    _same_as_greedy(eng, n, ref, dtype, "stop2")
    _stats_as_predicted(eng, want, "stop2")
    assert all(stop2 not in toks[1:] for toks, _ in want["per_step"])


def test_lookup_accepts_on_the_repeating_model():
    """random weights loop, so lookup must find and the model must accept drafts: the feature does something"""
    seed = SEEDS[(BF, None)][0]
    eng, n, ref, want = _spec_run(BF, None, seed, 4, source="lookup")
    st = eng.spec_stats()
    assert st["accepted"] > 0 and st["steps"] < n - 1


# ---- 5. fp8 / MXFP4 decode weights --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF, FH], ids=lambda d: KC.NAME[d])
@pytest.mark.parametrize("dw", ["fp8", "mxfp4"])
def test_speculation_with_quantised_decode_weights(dw, dtype):
    for source, seed in zip(("given", "lookup", "lookup"), SEEDS[(dtype, dw)]):
        what = "%s %s %s seed %d" % (dw, KC.NAME[dtype], source, seed)
        eng, n, ref, want = _spec_run(dtype, dw, seed, 4, source=source)
        assert eng.decode_weights == dw
        _same_as_greedy(eng, n, ref, dtype, what)
        _stats_as_predicted(eng, want, what)


# ---- 6. refusals, the batch bypass, off again ---------------------------------------------------------------------------------------------
def test_refusals_name_the_option(golden):
    from seedstory import _lib
    eng, wd = _engine(golden[1], BF)
    pr = _prompt(41)
    eng.prefill(wd["model.embed_tokens.weight"][pr])
    eng.set_speculation(4)
    before = (eng.lengths(), eng.logits.clone())
    cases = (
        ("sampling", lambda: eng.set_sampling(temperature=0.8, seed=3), eng.set_greedy),
        ("logits rules", lambda: eng.set_logits_rules(repetition_penalty=1.2), eng.clear_logits_rules),
        ("log-probabilities", lambda: eng.set_logprobs(top_n=2), lambda: eng.set_logprobs(False)),
        ("fp8 KV shadow", eng.enable_kv_fp8, eng.disable_kv_fp8),
        ("attention-map capture", lambda: eng.attn_capture_on(64, 64), eng.attn_capture_off),
    )
    for msg, on, off in cases:
        on()
        try:
            with pytest.raises(_lib.SSError, match="speculation is on.*" + msg):
                eng.generate(6, last_prompt_id=int(pr[-1]))
        finally:
            off()
        assert eng.lengths() == before[0] and torch.equal(eng.logits, before[1]), msg       # nothing was launched
    assert eng.generate(6, last_prompt_id=int(pr[-1])) == 6                                   # and the option still works
    with pytest.raises(_lib.SSError, match="rows"):
        _lib.check(_lib.lib().ss_llama_set_speculation(eng._h, _lib.SpecParams(9, 2, 0, 0, None), eng._spec[0].data_ptr()), "set")


def test_generate_batch_ignores_speculation(golden):
    outs = []
    for spec in (0, 4):
        eng, wd = _engine(golden[1], BF, n_seq=2)
        if spec:
            eng.set_speculation(spec)
        prompts = [_prompt(41), _prompt(43)]
        for b in range(2):
            eng.select(b).prefill(wd["model.embed_tokens.weight"][prompts[b]])
        ns = eng.generate_batch(10, [int(p[-1]) for p in prompts])
        out = []
        for b in range(2):
            eng.select(b)
            kv = eng.lengths()[0]
            out.append((ns[b], eng.gen_ids[:ns[b]].clone(), eng.hidden_rows[:ns[b] - 1].clone(), eng.k_cache[:, :, :kv].clone(),
                        eng.v_cache[:, :, :kv].clone()))
        outs.append(out)
    for a, b in zip(*outs):
        assert a[0] == b[0] and all(torch.equal(x, y) for x, y in zip(a[1:], b[1:]))


def test_clear_speculation_restores_the_plain_token(golden):
    ref = None
    for spec in (False, True):
        eng, wd = _engine(golden[1], BF)
        pr = _prompt(41)
        emb = wd["model.embed_tokens.weight"][pr]
        if spec:                        # a speculative call first, then off and the same call again from scratch
            eng.prefill(emb)
            eng.set_speculation(4)
            eng.set_history(pr.tolist())
            eng.generate(10, last_prompt_id=int(pr[-1]))
            eng.clear_speculation()
            eng.reset()
        eng.prefill(emb)
        n = eng.generate(10, last_prompt_id=int(pr[-1]))
        kv = eng.lengths()[0]
        got = (n, eng.gen_ids[:n].clone(), eng.hidden_rows[:n - 1].clone(), eng.k_cache[:, :, :kv].clone(), eng.v_cache[:, :, :kv].clone())
        if ref is None:
            ref = got
        else:
            assert got[0] == ref[0] and all(torch.equal(x, y) for x, y in zip(got[1:], ref[1:]))

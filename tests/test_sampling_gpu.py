"""On-device sampling on the GPU: ``ss_sample_logits`` against the fp64 oracle of tests/test_sampling_cpu.py (decided cases:
the kept set exactly, the token within the derived error allowance), exact probes, Philox frequencies, and the engine paths
(seeded, eager == captured, replay through the stand-alone operator, top_k = 1 == greedy, image-block == token-by-token,
lock-step slots, ``LlamaForCausalLM.generate(do_sample=True)``)."""
import contextlib
import math

import numpy as np
import pytest
import torch

import kernel_check as KC
import synth
from test_sampling_cpu import DELTA, oracle, philox_u, processor_edit, token_within_bound

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
VOCABS = [64, 1000, 32066, 65535]           # one run per thread | no multiple of the vector width or the block | the story model's | the largest
PARAMS = [(0.7, 0, 0.5), (1.0, 50, 0.9), (1.3, 0, 1.0), (0.7, 0, 0.95)]      # (temperature, top_k, top_p)


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
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def _guarded(z, ld=None, offset=0):
    """z [rows, vocab] (CPU, model dtype) in a guarded device buffer (row stride ld, first element `offset` elements past a
    16-byte boundary) -> the buffer; buffer.out is what the kernel gets"""
    buf = KC.GuardedOut(z.shape[0], z.shape[1], z.dtype, device=DEV, ld=ld, offset=offset)
    buf.out.copy_(z.to(DEV))
    return buf


# ---- the kernel against the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: KC.NAME[d])
def test_sample_kernel_against_oracle(ops, dtype):
    """N(0, 4^2) logits rounded to the dtype, u supplied.  Per row: skipped when top-p is undecided at DELTA (at most 5 % of the
    rows); otherwise n_kept equals the oracle's, the token lies within DELTA * Z_P of the oracle's cumulative interval, and on
    the parameter sets with top_p < 1 it IS the oracle's token in at least 95 % of the decided rows.  The logits are only read
    and nothing is written around them."""
    g = torch.Generator().manual_seed(1234 + DTYPES.index(dtype))
    total = skipped = 0
    eq = {p: [0, 0] for p in PARAMS}
    for vocab in VOCABS:
        for rows in (1, 8):
            z = (torch.randn(rows, vocab, generator=g) * 4.0).to(dtype)
            u = torch.rand(rows, generator=g, dtype=torch.float32)
            # 8 rows: a row stride that leaves the rows at every misalignment; 1 row: aligned, then off by one element
            for pi, (T, k, p) in enumerate(PARAMS):
                ld, offset = (vocab + 3, 0) if rows == 8 else (vocab, pi % 2)
                buf = _guarded(z, ld=ld, offset=offset)
                tok, kept = ops.sample_logits(buf.out, T, k, p, u=u.to(DEV), return_n_kept=True)
                tok, kept = tok.cpu().tolist(), kept.cpu().tolist()
                assert torch.equal(_bits(buf.check("sample_logits %s vocab %d" % (KC.NAME[dtype], vocab))), _bits(z))
                for r in range(rows):
                    o = oracle(z[r].double().numpy(), T, k, p, u=float(u[r]))
                    total += 1
                    if not o["decided"]:
                        skipped += 1
                        continue
                    what = (KC.NAME[dtype], vocab, rows, r, (T, k, p))
                    assert kept[r] == o["n_kept"], what
                    assert token_within_bound(o, tok[r]), (what, tok[r], o["token"], o["t"], o["Z_P"])
                    eq[(T, k, p)][0] += int(tok[r] == o["token"])
                    eq[(T, k, p)][1] += 1
    print("skipped %d of %d rows; equal tokens %s" % (skipped, total, eq))
    assert skipped <= 0.05 * total, (skipped, total)
    for (T, k, p), (same, n) in eq.items():
        if p < 1.0:
            assert same >= 0.95 * n, ((T, k, p), same, n)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: KC.NAME[d])
def test_sample_with_processor(ops, dtype):
    """last_ids + img_ids: the processor's edit first (in place, the only change to the buffer), then the certain successor
    (n_kept = 1, whatever u) or the sampler on the edited row."""
    vocab, img = 1000, [900, 17, 950, 3, 999]
    g = torch.Generator().manual_seed(77)
    lasts = [5, 900, 17, 3, 999, 950, 0, 998]            # 999 = </img> has no successor
    z = (torch.randn(len(lasts), vocab, generator=g) * 4.0).to(dtype)
    for u_val in (0.0, 0.37, 1.0 - 2.0 ** -24):
        u = torch.full((len(lasts),), u_val, dtype=torch.float32)
        buf = _guarded(z)
        tok, kept = ops.sample_logits(buf.out, 0.9, 0, 0.9, u=u.to(DEV), last_ids=lasts, img_ids=img, return_n_kept=True)
        tok, kept = tok.cpu().tolist(), kept.cpu().tolist()
        edited = z.clone()
        for r, last in enumerate(lasts):
            succ = processor_edit(edited[r], last, img)
            if succ >= 0:
                assert (tok[r], kept[r]) == (succ, 1), (r, last, u_val)
                continue
            o = oracle(edited[r].double().numpy(), 0.9, 0, 0.9, u=u_val)
            if o["decided"]:
                assert kept[r] == o["n_kept"] and token_within_bound(o, tok[r]), (r, last, u_val, tok[r], o["token"])
        assert torch.equal(_bits(buf.check("sample_logits + processor")), _bits(edited))


# ---- exact probes ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: KC.NAME[d])
def test_sample_exact_probes(ops, dtype):
    g = torch.Generator().manual_seed(5)
    img = [40, 41, 42]
    for vocab in (64, 1000, 32066, 65535):
        z = (torch.randn(4, vocab, generator=g) * 4.0).to(dtype)
        zd = z.to(DEV)
        greedy = [int(ops.imgproc_argmax(zd[r].clone(), 7, img)) for r in range(4)]
        edited = z.clone()
        for r in range(4):
            processor_edit(edited[r], 7, img)
        us = torch.tensor([0.0, 0.3, 0.77, 1.0 - 2.0 ** -24])
        # top_k = 1 and top_p = 1e-6 keep the arg max alone: ss_imgproc_argmax's token for any u
        for kw in (dict(top_k=1), dict(top_p=1e-6)):
            tok, kept = ops.sample_logits(zd.clone(), 0.8, u=us.to(DEV), last_ids=[7] * 4, img_ids=img, return_n_kept=True, **kw)
            ties = [int((edited[r] == edited[r].float().max().to(dtype)).sum()) for r in range(4)]
            assert kept.cpu().tolist() == ties
            assert [t for t, n in zip(tok.cpu().tolist(), ties) if n == 1] == [t for t, n in zip(greedy, ties) if n == 1]
        # u = 0 -> the first kept index, u = 1 - 2^-24 -> the last kept index (top_k = 3 of distinct values: equal to three
        # picked entries made the three largest with equal weights, so the last one owns the top third of [0, 1))
        zz = z.clone()
        big = (zz.float().max() + 8.0).to(dtype)
        picks = [3, vocab // 2, vocab - 1]
        zz[:, picks] = big
        for u_val, want in ((0.0, picks[0]), (0.5, picks[1]), (1.0 - 2.0 ** -24, picks[2])):
            tok, kept = ops.sample_logits(zz.to(DEV), 1.0, top_k=3, u=torch.full((4,), u_val, device=DEV), return_n_kept=True)
            assert tok.cpu().tolist() == [want] * 4 and kept.cpu().tolist() == [3] * 4, (vocab, u_val)
        # -inf entries are never returned: everything but two entries is -inf
        zi = torch.full((2, vocab), float("-inf")).to(dtype)
        zi[:, 1], zi[:, vocab - 2] = 0.5, 0.5
        for u_val, want in ((0.0, 1), (0.49, 1), (0.51, vocab - 2), (1.0 - 2.0 ** -24, vocab - 2)):
            tok, kept = ops.sample_logits(zi.to(DEV), 1.0, u=torch.full((2,), u_val, device=DEV), return_n_kept=True)
            assert tok.cpu().tolist() == [want] * 2 and kept.cpu().tolist() == [2] * 2, (vocab, u_val)
        # all-equal logits, top_k = 3: every entry ties with the third largest -> n_kept = vocab, token = floor(u vocab) +- 1
        flat = torch.full((3, vocab), 1.25).to(dtype)
        uu = torch.tensor([0.0, 0.6180339, 1.0 - 2.0 ** -24])
        tok, kept = ops.sample_logits(flat.to(DEV), 0.7, top_k=3, u=uu.to(DEV), return_n_kept=True)
        assert kept.cpu().tolist() == [vocab] * 3
        for t, u_val in zip(tok.cpu().tolist(), uu.tolist()):
            assert abs(t - math.floor(float(np.float32(u_val)) * vocab)) <= 1 and 0 <= t < vocab, (vocab, u_val, t)
        # an all-NaN row: token 0, the launch is fine
        nan = torch.full((2, vocab), float("nan")).to(dtype)
        tok, kept = ops.sample_logits(nan.to(DEV), 1.0, top_k=5, top_p=0.9, u=torch.tensor([0.0, 0.9], device=DEV), return_n_kept=True)
        torch.cuda.synchronize()
        assert tok.cpu().tolist() == [0, 0] and kept.cpu().tolist() == [0, 0]


def test_sample_error_cases(ops):
    """SS_EINVAL, nothing launched: the outputs keep their preset values"""
    from seedstory import _lib
    z = torch.zeros(2, 64, device=DEV)
    for kw in (dict(temperature=0.0), dict(temperature=-1.0), dict(temperature=float("nan")), dict(temperature=float("inf")),
               dict(top_p=0.0), dict(top_p=1.0001), dict(top_p=float("nan")), dict(top_k=-1)):
        with pytest.raises(_lib.SSError):
            ops.sample_logits(z, **kw)
    with pytest.raises(_lib.SSError):
        ops.sample_logits(torch.zeros(1, 65536, device=DEV))
    with pytest.raises(_lib.SSError):
        ops.sample_logits(z, u=torch.zeros(3, device=DEV))
    with pytest.raises(_lib.SSError):
        ops.sample_logits(torch.zeros(2, 64))


# ---- frequencies -----------------------------------------------------------------------------------------------------------
def _chi2_sf(x, k):
    """survival function of chi-square with integer k degrees of freedom (closed forms, Abramowitz & Stegun 26.4.4 / 26.4.5)"""
    h = x / 2.0
    if k % 2 == 0:
        term, s = 1.0, 1.0
        for j in range(1, k // 2):
            term *= h / j
            s += term
        return math.exp(-h) * s
    s, term = 0.0, math.sqrt(h) / math.gamma(1.5)
    for j in range(1, (k - 1) // 2 + 1):
        s += term
        term *= h / (j + 0.5)
    return math.erfc(math.sqrt(h)) + math.exp(-h) * s


def _chi2_quantile(q, k):
    lo, hi = 0.0, 1000.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if _chi2_sf(mid, k) > 1.0 - q else (lo, mid)
    return hi


def test_chi2_quantile_helper():
    assert abs(_chi2_quantile(0.95, 1) - 3.841) < 2e-3 and abs(_chi2_quantile(0.95, 10) - 18.307) < 2e-3
    assert abs(_chi2_quantile(0.99, 7) - 18.475) < 2e-3


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: KC.NAME[d])
@pytest.mark.parametrize("T,top_k,top_p", [(1.0, 0, 1.0), (0.8, 10, 1.0), (1.2, 0, 0.8)])
def test_sample_frequencies(ops, dtype, T, top_k, top_p):
    """4096 rows sharing one 16-entry logit vector, Philox draws with counter (draw0, row): Pearson chi-square of the counts
    against the oracle's probabilities below the 1 - 1e-6 quantile, and token for token what the numpy Philox's u gives."""
    rows, seed, draw0 = 4096, 0x1234567887654321, 3
    g = torch.Generator().manual_seed(31)
    z1 = (torch.randn(16, generator=g) * 1.5).to(dtype)
    o = oracle(z1.double().numpy(), T, top_k, top_p, u=0.5)
    assert o["decided"] and o["n_kept"] >= 4
    z = z1.unsqueeze(0).repeat(rows, 1).to(DEV)
    tok = ops.sample_logits(z, T, top_k, top_p, seed=seed, draw0=draw0)
    u = philox_u(seed, draw0, np.arange(rows))
    tok_u = ops.sample_logits(z, T, top_k, top_p, u=torch.from_numpy(u).to(DEV))
    assert torch.equal(tok, tok_u)
    assert torch.equal(tok, ops.sample_logits(z, T, top_k, top_p, seed=seed, draw0=draw0))
    assert not torch.equal(tok, ops.sample_logits(z, T, top_k, top_p, seed=seed, draw0=draw0 + 1))
    assert not torch.equal(tok, ops.sample_logits(z, T, top_k, top_p, seed=seed + (1 << 32), draw0=draw0))
    counts = np.bincount(tok.cpu().numpy(), minlength=16).astype(np.float64)
    prob = o["prob"]
    assert counts[prob == 0].sum() == 0
    kept = prob > 0
    chi2 = float((((counts - rows * prob) ** 2)[kept] / (rows * prob[kept])).sum())
    bound = _chi2_quantile(1.0 - 1e-6, int(kept.sum()) - 1)
    print("chi2 %.2f, bound %.2f at %d degrees of freedom" % (chi2, bound, int(kept.sum()) - 1))
    assert chi2 < bound


# ---- the engine ------------------------------------------------------------------------------------------------------------
def _img_ids(meta):
    lo, hi = meta["IMG_IDS"]
    return list(range(lo, hi + 1))


def _engine(meta, dtype, img_ids=None, **kw):
    from seedstory.llama import LlamaEngine
    d = meta["LLAMA"]
    wd = synth.llama_weights(11, d["hidden"], d["n_heads"], d["n_layers"], d["inter"], d["vocab"], dtype=dtype)
    eng = LlamaEngine(wd, hidden=d["hidden"], n_heads=d["n_heads"], n_layers=d["n_layers"], inter=d["inter"],
                      vocab=d["vocab"], dtype=dtype, device=DEV, cache_cap=256, max_new=128, max_prefill_rows=64,
                      img_ids=_img_ids(meta) if img_ids is None else img_ids, **kw)
    return eng, wd["model.embed_tokens.weight"]


PROMPT = synth.randint(91, (21,), 3, 250)
ENGINE_DTYPES = [torch.bfloat16, torch.float32]
# the synthetic model's logits have a spread of a few units: at this temperature no token holds the mass greedy would need
SAMPLING = dict(temperature=1.5, top_k=0, top_p=0.95)


def _run(eng, emb, n, **kw):
    eng.reset()
    eng.prefill(emb[PROMPT])
    k = eng.generate(n, int(PROMPT[-1]), **kw)
    return eng.gen_ids[:k].tolist(), eng.hidden_rows[:max(k - 1, 0)].clone()


@pytest.mark.parametrize("dtype", ENGINE_DTYPES, ids=lambda d: KC.NAME[d])
def test_engine_seeded_and_graph_equals_eager(golden, dtype):
    _, meta = golden
    eng, emb = _engine(meta, dtype)
    greedy = _run(eng, emb, 24)[0]
    out = {}
    for graph in (1, 0):
        with knobs(llama_graph=graph):
            for seed in (11, 11, 12):
                eng.set_sampling(seed=seed, **SAMPLING)
                out.setdefault((graph, seed), []).append(_run(eng, emb, 24))
    a, b = out[(1, 11)]
    assert a[0] == b[0] and torch.equal(a[1], b[1])                              # one seed, two runs
    assert a[0] != out[(1, 12)][0][0] and a[0] != greedy                         # another seed, and not the arg max
    for seed in (11, 12):                                                        # captured == eager
        assert out[(1, seed)][0][0] == out[(0, seed)][0][0] and torch.equal(out[(1, seed)][0][1], out[(0, seed)][0][1])
    eng.set_greedy()
    assert _run(eng, emb, 24)[0] == greedy


@pytest.mark.parametrize("dtype", ENGINE_DTYPES, ids=lambda d: KC.NAME[d])
def test_engine_replay_through_the_operator(ops, golden, dtype):
    """The sampled ids fed back as forced tokens one step at a time: before each step the stand-alone operator, on the
    engine's logits with the same seed, draw0 = the step's draw index and lane 0, returns the engine's token."""
    _, meta = golden
    img = _img_ids(meta)
    eng, emb = _engine(meta, dtype)
    seed = 2024
    eng.set_sampling(seed=seed, **SAMPLING)
    ids = _run(eng, emb, 20)[0]
    assert len(ids) == 20
    eng.set_greedy()
    eng.reset()
    eng.prefill(emb[PROMPT])
    last, draw = int(PROMPT[-1]), 0
    for j, want in enumerate(ids):
        tok = ops.sample_logits(eng.logits.clone().view(1, -1), seed=seed, draw0=draw, last_ids=[last], img_ids=img, **SAMPLING)
        assert int(tok) == want, (j, int(tok), want)
        draw += 0 if last in img[:-1] else 1         # the certain successor takes no draw
        if want == eng.eos_id:
            break
        assert eng.generate(2, last, forced=[want, 3]) == 2       # feeds `want`; the second token is emitted, not fed
        last = want


@pytest.mark.parametrize("dtype", ENGINE_DTYPES, ids=lambda d: KC.NAME[d])
def test_engine_top_k_1_is_greedy_bitwise(golden, dtype):
    _, meta = golden
    eng, emb = _engine(meta, dtype)
    greedy = _run(eng, emb, 24)
    eng.set_sampling(temperature=0.8, top_k=1, top_p=1.0, seed=5)
    sampled = _run(eng, emb, 24)
    assert sampled[0] == greedy[0] and torch.equal(sampled[1], greedy[1])


@pytest.mark.parametrize("dtype", ENGINE_DTYPES, ids=lambda d: KC.NAME[d])
def test_engine_img_block_equals_token_loop_under_sampling(golden, dtype):
    """A five-id image-token list whose <img> is a token the sampled run produces by itself after some draws: the block path
    (several generate calls around one batched continuation) and the token-by-token loop give the same ids, which needs the
    draw counter to persist across generate calls."""
    _, meta = golden
    eng0, emb = _engine(meta, dtype, img_ids=[])
    eng0.set_sampling(seed=77, **SAMPLING)
    free = _run(eng0, emb, 40)[0]
    del eng0
    spare = [t for t in range(300, 320) if t not in free][:4]
    done = False
    for j in range(2, 30):
        boi = free[j]
        if boi in free[:j] or boi in (2, int(PROMPT[-1])):
            continue
        img = [boi] + spare
        eng, emb = _engine(meta, dtype, img_ids=img)
        outs = {}
        for block in (0, 1):
            with knobs(img_block_decode=block):
                eng.set_sampling(seed=77, **SAMPLING)
                eng.reset()
                eng.prefill(emb[PROMPT])
                if eng.img_block_enabled():
                    outs[block] = eng.generate_img_block(40, int(PROMPT[-1]))[0]
                else:
                    n = eng.generate(40, int(PROMPT[-1]))
                    outs[block] = eng.gen_ids[:n].tolist()
        seq = outs[0]
        i = seq.index(boi) if boi in seq else -1
        if not 1 <= i <= len(seq) - 6:
            continue                        # zeroing the four spare logits moved this run away from <img>: next candidate
        assert seq[i:i + 5] == img                                           # the certain successors
        assert outs[1] == seq, (j, i)
        done = True
        break
    assert done, "no candidate <img> was reached by the sampled run"


@pytest.mark.parametrize("dtype", ENGINE_DTYPES, ids=lambda d: KC.NAME[d])
def test_engine_slots_diverge_and_greedy_is_untouched(golden, dtype):
    _, meta = golden
    S = 4
    eng, emb = _engine(meta, dtype, n_seq=S)
    lasts = [int(PROMPT[-1])] * S

    def run():
        for b in range(S):
            eng.select(b).reset()
            eng.select(b).prefill(emb[PROMPT])
        ns = eng.generate_batch(20, lasts)
        return [(eng.select(b).gen_ids[:ns[b]].tolist(), eng.select(b).hidden_rows[:max(ns[b] - 1, 0)].clone()) for b in range(S)]

    ref_eng, _ = _engine(meta, dtype, n_seq=S)          # an engine that never samples
    for b in range(S):
        ref_eng.select(b).prefill(emb[PROMPT])
    ns = ref_eng.generate_batch(20, lasts)
    ref = [(ref_eng.select(b).gen_ids[:ns[b]].tolist(), ref_eng.select(b).hidden_rows[:max(ns[b] - 1, 0)].clone()) for b in range(S)]
    eng.set_sampling(seed=9, **SAMPLING)
    sampled = run()
    assert len({tuple(s[0]) for s in sampled}) == S                              # one prompt, one seed: the slots diverge
    assert [s[0] for s in run()] != [s[0] for s in sampled]                      # the draw counters went on ...
    eng.set_sampling(seed=9, **SAMPLING)
    assert [s[0] for s in run()] == [s[0] for s in sampled]                      # ... until set_sampling reset them
    eng.set_greedy()
    back = run()
    for b in range(S):
        assert back[b][0] == ref[b][0] and torch.equal(back[b][1], ref[b][1]), b
    # mixed: slots 1 and 3 sample, 0 and 2 stay greedy bit for bit
    eng.set_sampling(seed=9, slot=1, **SAMPLING)
    eng.set_sampling(seed=9, slot=3, **SAMPLING)
    mixed = run()
    for b in (0, 2):
        assert mixed[b][0] == ref[b][0] and torch.equal(mixed[b][1], ref[b][1]), b
    assert mixed[1][0] == sampled[1][0] and mixed[3][0] == sampled[3][0] and mixed[1][0] != ref[1][0]


def test_engine_refuses_bad_sampling_parameters(golden):
    from seedstory import _lib
    _, meta = golden
    eng, emb = _engine(meta, torch.bfloat16)
    greedy = _run(eng, emb, 8)[0]
    for kw in (dict(temperature=0.0), dict(temperature=float("inf")), dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-2), dict(slot=1),
               dict(slot=-2)):
        with pytest.raises(_lib.SSError):
            eng.set_sampling(**kw)
    assert _run(eng, emb, 8)[0] == greedy


class _Tok:
    def __init__(self, ids):
        self.ids = ids

    def encode(self, s, add_special_tokens=False):
        return list(self.ids)


@pytest.mark.parametrize("dtype", ENGINE_DTYPES, ids=lambda d: KC.NAME[d])
def test_llm_generate_do_sample(golden, dtype):
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
    llm.cache_cap, llm.max_new, llm.max_prefill_rows = 256, 64, 64
    llm.use_kv_cache_head = False
    proc = [AutoImageTokenGenerationProcessor(tokenizer=_Tok(_img_ids(meta)))]
    ids = PROMPT.unsqueeze(0)
    kw = dict(input_ids=ids, inputs_embeds=wd["model.embed_tokens.weight"][ids].to(DEV), logits_processor=proc)

    def seq(**extra):
        return llm.generate(max_new_tokens=20, **kw, **extra).sequences[0].tolist()
    greedy = seq()
    a = seq(do_sample=True, seed=31, **SAMPLING)
    assert a == seq(do_sample=True, seed=31, **SAMPLING) and a != greedy
    assert a != seq(do_sample=True, seed=32, **SAMPLING)
    assert seq(do_sample=False, temperature=0.7, top_p=0.5) == greedy and seq() == greedy          # greedy afterwards
    torch.manual_seed(5)
    b = seq(do_sample=True, **SAMPLING)
    assert b != seq(do_sample=True, **SAMPLING)             # seed=None: the call counter moves on
    with pytest.raises(ValueError):                         # raised inside _generate, after sampling was switched on
        llm.generate(max_new_tokens=65, do_sample=True, seed=31, **SAMPLING, **kw)
    assert seq() == greedy
    with pytest.raises(NotImplementedError):
        seq(do_sample=True, num_beams=2)

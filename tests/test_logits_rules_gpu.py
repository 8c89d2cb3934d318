"""The history rules on the GPU: ``ss_process_logits`` bit-equal to the oracle of tests/test_logits_rules_cpu.py on guarded
buffers, and the engine paths on the tiny golden model (host replay, captured == eager, image block == token loop, mixed
lock-step slots, with seeded sampling, ``min_new_tokens`` against an early EOS, ``clear_logits_rules``,
``LlamaForCausalLM.generate(repetition_penalty=...)``)."""
import contextlib

import pytest
import torch

import kernel_check as KC
import synth
from test_logits_rules_cpu import CONFIGS, DTYPES, EOS, MAX_NGRAM, VOCABS, bits, case_bites, make_case, oracle
from test_sampling_cpu import processor_edit

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


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


def _guarded(z, ld=None, offset=0):
    buf = KC.GuardedOut(z.shape[0], z.shape[1], z.dtype, device=DEV, ld=ld, offset=offset)
    buf.out.copy_(z.to(DEV))
    return buf


def _hist_tensor(hist, pad=-7):
    """histories of different lengths as one [rows, hist_ld] int32 tensor; the padding is an id the kernel must never read as
    history (out of range, so a read past a row's length would also show as a skipped id, not as a fault)"""
    ld = max(1, max(len(h) for h in hist))
    t = torch.full((len(hist), ld), pad, dtype=torch.int32)
    for r, h in enumerate(hist):
        t[r, :len(h)] = torch.tensor(h, dtype=torch.int32)
    return t


# ---- the kernel against the oracle -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: KC.NAME[d])
def test_process_logits_bit_equal_to_oracle(ops, dtype):
    """Every vocabulary x rule set of the CPU file's case table, one call per case with one row per history length (0, 1, n - 2,
    n - 1, 1023, 1025, 3000), once contiguous and aligned, once with ld = vocab + 3 and the first row one element past a 16-byte
    boundary (so every row starts at another misalignment): the edited rows are the oracle's bit for bit, the gaps and guards
    keep their sentinels."""
    for vocab in VOCABS:
        for cfg in CONFIGS:
            case = make_case(dtype, vocab, cfg)
            assert case_bites(case), (vocab, cfg[0])
            hist = _hist_tensor(case["hist"]).to(DEV)
            for ld, offset in ((vocab, 0), (vocab + 3, 1)):
                buf = _guarded(case["z"], ld=ld, offset=offset)
                ops.process_logits(buf.out, hist, hist_len=case["lens"], prompt_len=case["prompt_len"], repetition_penalty=case["p"],
                                   no_repeat_ngram_size=case["n"], min_new_tokens=case["m"], spare_img_ids=case["spare"], eos_id=EOS,
                                   img_ids=case["img_ids"])
                got = buf.check("process_logits %s vocab %d %s ld %d" % (KC.NAME[dtype], vocab, cfg[0], ld))
                diff = (bits(got) != bits(case["want"])).nonzero()
                assert diff.numel() == 0, (KC.NAME[dtype], vocab, cfg[0], ld, diff[:4].tolist(),
                                           [(float(got[r, c]), float(case["want"][r, c]), float(case["z"][r, c])) for r, c in diff[:4].tolist()])


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: KC.NAME[d])
def test_process_logits_skips_ids_outside_the_vocabulary(ops, dtype):
    """a device history may hold anything: ids below 0 or at / above vocab are never used as an index (the guard words around
    the rows stay intact) and the result is the oracle's, which skips them too"""
    vocab = 1000
    g = torch.Generator().manual_seed(3)
    z = (torch.randn(2, vocab, generator=g) * 4.0).to(dtype)
    hist = [[5, -1, vocab, 5, 2 ** 31 - 1, -2 ** 31, 7, vocab + 31, 5, -1, vocab, 9, 1 << 20, 5, -1, vocab],
            [vocab, vocab, vocab, 65535, 65536, -5, -5, -5, 3, -5, -5, -5]]
    for p, n in ((1.5, 0), (1.0, 1), (1.0, 3), (1.5, 3), (1.5, 4)):
        want = torch.stack([oracle(z[r], hist[r], 0, p, n, 0, EOS) for r in range(2)])
        buf = _guarded(z, ld=vocab + 5, offset=3)
        ops.process_logits(buf.out, _hist_tensor(hist).to(DEV), hist_len=[len(h) for h in hist], repetition_penalty=p,
                           no_repeat_ngram_size=n, eos_id=EOS)
        assert torch.equal(bits(buf.check("out-of-range ids p=%g n=%d" % (p, n))), bits(want)), (p, n)
    assert not torch.equal(bits(want), bits(z))


def test_process_logits_error_cases(ops):
    """SS_EINVAL, nothing launched: the rows keep their values"""
    from seedstory import _lib
    z = torch.randn(2, 64, device=DEV)
    keep = z.clone()
    hist = torch.zeros(2, 4, dtype=torch.int32, device=DEV)
    for kw in (dict(repetition_penalty=0.0), dict(repetition_penalty=-1.0), dict(repetition_penalty=float("nan")),
               dict(repetition_penalty=float("inf")), dict(no_repeat_ngram_size=-1), dict(no_repeat_ngram_size=MAX_NGRAM + 1),
               dict(min_new_tokens=-1)):
        with pytest.raises(_lib.SSError):
            ops.process_logits(z, hist, **kw)
    with pytest.raises(_lib.SSError):
        ops.process_logits(torch.zeros(1, 65536, device=DEV), hist[:1], repetition_penalty=1.2)
    with pytest.raises(_lib.SSError):
        ops.process_logits(z, hist[:1], repetition_penalty=1.2)
    with pytest.raises(_lib.SSError):
        ops.process_logits(z, hist, hist_len=[1, 2, 3], repetition_penalty=1.2)
    torch.cuda.synchronize()
    assert torch.equal(z, keep)


def banned_free(ids, prompt, n):
    """no n-gram of prompt + ids occurs twice with its last id among `ids` (what no_repeat_ngram_size = n promises)"""
    full = list(prompt) + list(ids)
    seen = {tuple(full[i:i + n]) for i in range(len(prompt) - n + 1)}
    for i in range(len(prompt) - n + 1, len(full) - n + 1):
        g = tuple(full[i:i + n])
        if g in seen:
            return False
        seen.add(g)
    return True


def nothing_comes_again(ids, prompt, img):
    """what no_repeat_ngram_size = 1 promises: no id of the prompt or of the run so far is produced — except the ids img[1:]:
    the processor runs after the rules and ASSIGNS 0.0 to them whenever no image is open, which overwrites their ban (the order
    is Hugging Face's)"""
    free = [t for t in ids if t not in set(img[1:])]
    return len(set(free)) == len(free) and not set(free) & set(prompt)


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


# a prompt with repeats: the penalty and the n-gram ban have something to act on from the first token
PROMPT = torch.cat([synth.randint(91, (12,), 3, 250)] * 2)[:21]
ENGINE_DTYPES = [torch.bfloat16, torch.float32]
RULES = dict(repetition_penalty=1.3, no_repeat_ngram_size=3, min_new_tokens=0)


def _run(eng, emb, n, history=True, prompt=PROMPT, **kw):
    eng.reset()
    eng.prefill(emb[prompt])
    if history:
        eng.set_history(prompt.tolist())
    k = eng.generate(n, int(prompt[-1]), **kw)
    return eng.gen_ids[:k].tolist(), eng.hidden_rows[:max(k - 1, 0)].clone()


def _run_no_history(eng, n, prompt=PROMPT):
    """decode from the state a prefill left, with the history as the caller set it"""
    k = eng.generate(n, int(prompt[-1]))
    return eng.gen_ids[:k].tolist()


def _replay(eng, emb, ids, img, prompt=PROMPT, eos=None, **rules):
    """The run `ids` again with the engine's rules OFF, one step at a time: the logits of each step, the oracle on the host,
    the processor's edit, then the arg max must be the engine's token; `ids[j]` is then fed as a forced token."""
    eng.clear_logits_rules()
    eng.reset()
    eng.prefill(emb[prompt])
    hist, last = prompt.tolist(), int(prompt[-1])
    eos = eng.eos_id if eos is None else eos
    for j, want in enumerate(ids):
        z = oracle(eng.logits.clone().cpu(), hist, len(prompt), rules.get("repetition_penalty", 1.0), rules.get("no_repeat_ngram_size", 0),
                   rules.get("min_new_tokens", 0), eos, rules.get("spare_img_ids", False), img)
        processor_edit(z, last, img)
        tok = int(torch.argmax(z.float()))
        assert tok == want, (j, tok, want)
        if want == eos or j + 1 == len(ids):
            break
        assert eng.generate(2, last, forced=[want, 3]) == 2       # feeds `want`; the second token is emitted, not fed
        hist.append(want)
        last = want


@pytest.mark.parametrize("dtype", ENGINE_DTYPES, ids=lambda d: KC.NAME[d])
def test_engine_rules_equal_host_replay_and_graph_equals_eager(golden, dtype):
    _, meta = golden
    img = _img_ids(meta)
    eng, emb = _engine(meta, dtype)
    greedy = _run(eng, emb, 24, history=False)
    out = {}
    for graph in (1, 0):
        with knobs(llama_graph=graph):
            eng.set_logits_rules(**RULES)
            out[graph] = [_run(eng, emb, 24), _run(eng, emb, 24)]
    a, b = out[1]
    assert a[0] == b[0] and torch.equal(a[1], b[1])                          # set_history starts every run from the prompt alone
    assert a[0] == out[0][0][0] and torch.equal(a[1], out[0][0][1])          # captured == eager
    assert a[0] != greedy[0]
    _replay(eng, emb, a[0], img, **RULES)
    # the rules went off inside _replay: greedy is what it was on an engine that never had rules
    back = _run(eng, emb, 24, history=False)
    assert back[0] == greedy[0] and torch.equal(back[1], greedy[1])
    # the spared image ids: another run (the prompt's ids are not image ids here, so only the declared exemption differs)
    eng.set_logits_rules(spare_img_ids=True, **RULES)
    spared = _run(eng, emb, 24)[0]
    _replay(eng, emb, spared, img, spare_img_ids=True, **RULES)


@pytest.mark.parametrize("dtype", ENGINE_DTYPES, ids=lambda d: KC.NAME[d])
def test_engine_img_block_equals_token_loop_under_rules(golden, dtype):
    """A five-id image-token list whose <img> is a token the rules-on run produces by itself: the block path (several generate
    calls around one batched continuation, whose tokens are appended to the history from the host) and the token-by-token loop
    give the same ids — which needs the history, and min_new_tokens' count, to persist across generate calls."""
    _, meta = golden
    rules = dict(repetition_penalty=1.3, no_repeat_ngram_size=2, min_new_tokens=30)
    eng0, emb = _engine(meta, dtype, img_ids=[])
    eng0.set_logits_rules(**rules)
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
                eng.set_logits_rules(**rules)
                eng.reset()
                eng.prefill(emb[PROMPT])
                eng.set_history(PROMPT.tolist())
                if eng.img_block_enabled():
                    outs[block] = eng.generate_img_block(40, int(PROMPT[-1]))[0]
                else:
                    n = eng.generate(40, int(PROMPT[-1]))
                    outs[block] = eng.gen_ids[:n].tolist()
        seq = outs[0]
        i = seq.index(boi) if boi in seq else -1
        if not 1 <= i <= len(seq) - 6:
            continue                        # zeroing the four spare logits moved this run away from <img>: next candidate
        assert seq[i:i + 5] == img                                           # the certain successors survive the rules
        assert outs[1] == seq, (j, i)
        _replay(eng, emb, seq, img, **rules)
        done = True
        break
    assert done, "no candidate <img> was reached by the rules-on run"


@pytest.mark.parametrize("dtype", ENGINE_DTYPES, ids=lambda d: KC.NAME[d])
def test_engine_eight_slots_rules_on_two(golden, dtype):
    _, meta = golden
    S = 8
    eng, emb = _engine(meta, dtype, n_seq=S)
    lasts = [int(PROMPT[-1])] * S

    def run(e):
        for b in range(S):
            e.select(b).reset()
            e.select(b).prefill(emb[PROMPT])
            e.set_history(PROMPT.tolist(), slot=b)
        ns = e.generate_batch(20, lasts)
        return [(e.select(b).gen_ids[:ns[b]].tolist(), e.select(b).hidden_rows[:max(ns[b] - 1, 0)].clone()) for b in range(S)]

    ref_eng, _ = _engine(meta, dtype, n_seq=S)          # an engine that never has rules
    ref = run(ref_eng)
    eng.set_logits_rules(slot=2, **RULES)
    eng.set_logits_rules(slot=5, repetition_penalty=1.0, no_repeat_ngram_size=1)
    mixed = run(eng)
    for b in range(S):
        if b in (2, 5):
            assert mixed[b][0] != ref[b][0], b
        else:
            assert mixed[b][0] == ref[b][0] and torch.equal(mixed[b][1], ref[b][1]), b
    assert nothing_comes_again(mixed[5][0], PROMPT.tolist(), _img_ids(meta))
    assert banned_free(mixed[2][0], PROMPT.tolist(), 3)
    eng.clear_logits_rules()
    back = run(eng)
    for b in range(S):
        assert back[b][0] == ref[b][0] and torch.equal(back[b][1], ref[b][1]), b


@pytest.mark.parametrize("dtype", ENGINE_DTYPES, ids=lambda d: KC.NAME[d])
def test_engine_rules_with_seeded_sampling(golden, dtype):
    _, meta = golden
    eng, emb = _engine(meta, dtype, img_ids=[])         # no image ids: no processor edit between the rules and the sampler
    sampling = dict(temperature=1.5, top_k=0, top_p=0.95)
    eng.set_sampling(seed=11, **sampling)
    plain = _run(eng, emb, 24, history=False)[0]
    out = {}
    for seed in (11, 11, 12):
        eng.set_sampling(seed=seed, **sampling)
        eng.set_logits_rules(repetition_penalty=1.0, no_repeat_ngram_size=1)
        out.setdefault(seed, []).append(_run(eng, emb, 24)[0])
    assert out[11][0] == out[11][1] and out[11][0] != out[12][0] and out[11][0] != plain
    for ids in (out[11][0], out[12][0]):                # the sampler never keeps a banned (-inf) entry
        assert len(ids) == 24 and nothing_comes_again(ids, PROMPT.tolist(), [])
    eng.clear_logits_rules()
    eng.set_sampling(seed=11, **sampling)
    assert _run(eng, emb, 24, history=False)[0] == plain


@pytest.mark.parametrize("dtype", ENGINE_DTYPES, ids=lambda d: KC.NAME[d])
def test_engine_min_new_tokens_holds_eos_back(golden, dtype):
    """EOS is made the token plain greedy produces fourth, so plain greedy stops after 4 tokens; with min_new_tokens = 10 the
    first 10 tokens hold no EOS, and the run is the host replay's."""
    _, meta = golden
    img = _img_ids(meta)
    eng0, emb = _engine(meta, dtype)
    free = _run(eng0, emb, 12, history=False)[0]
    del eng0
    eos = next(t for i, t in enumerate(free[1:6], 1) if t not in free[:i] and t not in img)
    stop_at = free.index(eos)
    eng, emb = _engine(meta, dtype, eos_id=eos)
    plain = _run(eng, emb, 24, history=False)[0]
    assert plain == free[:stop_at + 1]                                       # greedy stops early: the test bites
    rules = dict(min_new_tokens=10)
    eng.set_logits_rules(**rules)
    held = _run(eng, emb, 24)[0]
    assert eos not in held[:10] and len(held) > 10 and held[:stop_at] == free[:stop_at]
    _replay(eng, emb, held, img, eos=eos, **rules)
    # counted from the history, not from the tokens of one generate call: with 9 of the 10 already in the history that was handed
    # over (prompt_len = the prompt's), EOS is held back for one more token only
    eng.set_logits_rules(**rules)
    eng.reset()
    eng.prefill(emb[PROMPT])
    eng.set_history(PROMPT.tolist())
    eng.set_history([3] * 9, append=True)
    late = _run_no_history(eng, 24)
    if stop_at >= 1:
        assert late == plain                                                 # the ban covered token 0 only: plain greedy's run


@pytest.mark.parametrize("dtype", [torch.bfloat16], ids=lambda d: KC.NAME[d])
def test_engine_rules_with_attention_capture_and_fp8(golden, dtype):
    _, meta = golden
    eng, emb = _engine(meta, dtype)
    eng.set_logits_rules(**RULES)
    want = _run(eng, emb, 16)[0]
    eng.reset()
    with eng.attn_capture(21 + 16, 21 + 16):
        eng.prefill(emb[PROMPT])
        eng.set_history(PROMPT.tolist())
        k = eng.generate(16, int(PROMPT[-1]))
        assert eng.gen_ids[:k].tolist() == want
    eng.enable_decode_fp8()
    outs = []
    for graph in (1, 0):
        with knobs(llama_graph=graph):
            outs.append(_run(eng, emb, 16)[0])
    assert outs[0] == outs[1] and len(outs[0]) == 16
    seen = set(PROMPT.tolist())
    eng.set_logits_rules(repetition_penalty=1.0, no_repeat_ngram_size=1)
    ids = _run(eng, emb, 16)[0]
    assert nothing_comes_again(ids, seen, _img_ids(meta))


def test_engine_refuses_bad_rules_and_histories(golden):
    from seedstory import _lib
    _, meta = golden
    eng, emb = _engine(meta, torch.bfloat16)
    greedy = _run(eng, emb, 8, history=False)[0]
    for kw in (dict(repetition_penalty=0.0), dict(repetition_penalty=float("inf")), dict(no_repeat_ngram_size=-1),
               dict(no_repeat_ngram_size=MAX_NGRAM + 1), dict(min_new_tokens=-1), dict(slot=1), dict(slot=-2)):
        with pytest.raises(_lib.SSError):
            eng.set_logits_rules(**kw)
    for ids in ([1, 2, eng.vocab], [-1], list(range(3)) * 200):              # outside [0, vocab); longer than cache_cap + max_new
        with pytest.raises(_lib.SSError):
            eng.set_history(ids)
    with pytest.raises(_lib.SSError):
        eng.set_history([1], slot=1)
    assert _run(eng, emb, 8, history=False)[0] == greedy
    # a rules-on call whose tokens the history buffer could not take is refused before any launch
    eng.set_logits_rules(**RULES)
    eng.reset()
    eng.prefill(emb[PROMPT])
    eng.set_history([3] * (eng.cache_cap + eng.max_new - 4))
    with pytest.raises(_lib.SSError):
        eng.generate(8, int(PROMPT[-1]))
    eng.clear_logits_rules()
    assert _run(eng, emb, 8, history=False)[0] == greedy


class _Tok:
    def __init__(self, ids):
        self.ids = ids

    def encode(self, s, add_special_tokens=False):
        return list(self.ids)


@pytest.mark.parametrize("dtype", ENGINE_DTYPES, ids=lambda d: KC.NAME[d])
def test_llm_generate_with_rules(golden, dtype):
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
    img = _img_ids(meta)
    proc = [AutoImageTokenGenerationProcessor(tokenizer=_Tok(img))]
    ids = PROMPT.unsqueeze(0)
    kw = dict(input_ids=ids, inputs_embeds=wd["model.embed_tokens.weight"][ids].to(DEV), logits_processor=proc)

    def seq(**extra):
        return llm.generate(max_new_tokens=20, **kw, **extra).sequences[0].tolist()
    greedy = seq()
    # the engine-level greedy run of the same prompt: the default call is what it was before the kwargs existed
    eng, emb = _engine(meta, dtype)
    free = img[0] not in greedy         # (a run that opens an image goes through the batched block in `llm`, not in `_run`)
    assert not free or greedy[21:] == _run(eng, emb, 20, history=False)[0]
    new = greedy[21:]
    assert len(set(new)) < len(new) or set(new) & set(PROMPT.tolist())       # plain greedy repeats a token: the penalty has a target
    a = seq(repetition_penalty=1.3)
    assert a != greedy and a[:21] == greedy[:21]
    eng.set_logits_rules(repetition_penalty=1.3)
    assert img[0] in a or a[21:] == _run(eng, emb, 20)[0]
    assert nothing_comes_again(seq(no_repeat_ngram_size=1)[21:], PROMPT.tolist(), img)
    assert seq() == greedy                                                    # cleared on return
    assert seq(repetition_penalty=1.0, no_repeat_ngram_size=0, min_new_tokens=0, spare_img_ids=True) == greedy
    with pytest.raises(ValueError):                                          # raised inside _generate, after the rules were set
        llm.generate(max_new_tokens=65, repetition_penalty=1.3, **kw)
    assert seq() == greedy
    # with sampling: the rules act there too, and the seed still reproduces
    s1 = seq(do_sample=True, seed=5, temperature=1.5, top_p=0.95, no_repeat_ngram_size=1)
    assert s1 == seq(do_sample=True, seed=5, temperature=1.5, top_p=0.95, no_repeat_ngram_size=1)
    assert nothing_comes_again(s1[21:], PROMPT.tolist(), img)

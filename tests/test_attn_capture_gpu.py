"""Attention maps (``output_attentions`` / ``attn_weights``): the ss_attn_scores kernel element-wise against fp64, the engine
against the REAL reference's maps (tests/golden/attn_maps_tiny.safetensors, tools/make_golden_attn_maps.py), generate + merge
against the oracle, the bit-exact invariants, the image-token block, the sink path and the refusals.

What a map holds (reference modeling_llama_xformer.py:246-276, 299-301; all roundings in the model dtype T): head 0's
``s = rnd_T(rnd_T(q . k) / sqrt(head_dim))``; a call of several rows adds the additive causal mask (``rnd_T(s + finfo(T).min)``
on masked keys), a one-row call adds its bool mask (``rnd_T(s + 1)`` on the row's own key).  The merged map has one row per
fed token, real up to that call's key count and NaN beyond.

Bounds.  Kernel: kernel_check's own (v, t) derivation — accumulate (Kacc = head_dim), mid round, one fp32 op for the scale, mid
round, the add, final round; no tuned constant.  Engine / generate / sink: the gates the project already applies to these same
calls — fp32 relative norm <= 1e-4 (test_engine_gpu.py), 16-bit distance to the fp32 reference <= 1.5 x the reference's own
16-bit-vs-fp32 distance on the same entries (+ 3e-4 for fp16, test_fp16_gpu.py); the own distance always comes from the
reference side, never from the engine's output.

Worst error / bound of the kernel cases (test_zz_worst_ratio prints it; above 1 fails the case that produced it), measured on
an MI355X:

  attn_scores            bf16  worst error / bound = 0.875
  attn_scores            fp16  worst error / bound = 0.687
  attn_scores            fp32  worst error / bound = 0.029
"""
import contextlib
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

import kernel_check as KC
import seedstory_oracle as O
import synth

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, FH, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [F32, BF, FH]
TAG = {F32: "f32", BF: "bf16", FH: "f16"}
EPS16 = {F32: 0.0, BF: 0.0, FH: 3e-4}          # the additive term of tests/test_fp16_gpu.py::gate

# M x kv: the listed shapes, then one case on each side of the kernel's tile edges (32 query rows, 64 keys per workgroup)
SHAPES = [(1, 1), (1, 47), (9, 46), (37, 37), (65, 130), (130, 130),
          (31, 63), (32, 64), (33, 65), (5, 63), (5, 64), (5, 65), (31, 40), (32, 40), (33, 40), (64, 128), (65, 129)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (no CPU fallback exists)")
    from seedstory import ops as _ops
    return _ops


@contextlib.contextmanager
def knobs(**kw):
    from seedstory import _lib
    old = {k: _lib.get_tuning(k) for k in kw}
    try:
        for k, v in kw.items():
            _lib.set_tuning(k, v)
        yield
    finally:
        for k, v in old.items():
            _lib.set_tuning(k, v)


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def same(a, b):
    """torch.equal with NaNs treated as equal"""
    a, b = a.cpu(), b.cpu()
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


# ---- the rules, restated ------------------------------------------------------------------------------------------------------
def own_col(M, kv):
    return torch.arange(M) + (kv - M)


def rule_masks(M, kv, row_calls):
    """-> (written, plus_one, masked) bool [M, kv]"""
    j, own = torch.arange(kv)[None, :], own_col(M, kv)[:, None]
    single = row_calls or M == 1
    written = (j <= own) if single else torch.ones(M, kv, dtype=torch.bool)
    plus_one = (j == own) if single else torch.zeros(M, kv, dtype=torch.bool)
    masked = torch.zeros(M, kv, dtype=torch.bool) if single else (j > own)
    return written, plus_one, masked


def ref_call(q, k, dtype, row_calls=False):
    """One reference call restated in torch arithmetic of the model dtype (the oracle side of the generate / sink tests):
    q [M, hd], k [kv, hd] of head 0 -> [M, kv], NaN where the mode writes nothing."""
    q, k = q.to(dtype), k.to(dtype)
    M, kv = q.shape[0], k.shape[0]
    written, plus_one, masked = rule_masks(M, kv, row_calls)
    s = torch.matmul(q, k.t()) / math.sqrt(q.shape[1])
    lo = torch.full((), torch.finfo(dtype).min, dtype=dtype)
    s = torch.where(masked, s + lo, s)
    s = torch.where(plus_one, s + torch.ones((), dtype=dtype), s)
    return torch.where(written, s, torch.full_like(s, float("nan")))


def merged_map(calls, dtype):
    """calls: [(q [M, hd], k [kv, hd], row_calls)] in feeding order -> [rows, width] (NaN beyond each call's key count)"""
    rows = sum(c[0].shape[0] for c in calls)
    width = calls[-1][1].shape[0]
    out = torch.full((rows, width), float("nan"), dtype=dtype)
    r = 0
    for q, k, rc in calls:
        out[r:r + q.shape[0], :k.shape[0]] = ref_call(q, k, dtype, rc)
        r += q.shape[0]
    return out


def merge_attn_weights(steps):
    """the reference's merge (models.py:164-173), restated: pad with one NaN column per step, concatenate along the query axis"""
    merged = steps[0]
    for a in steps[1:]:
        merged = F.pad(merged, (0, 1), "constant", float("nan"))
        merged = torch.cat([merged, a], dim=1)
    return merged


def gate_maps(y, ref_t, ref32, dtype, what):
    """y: engine map; ref_t / ref32: the reference side in the model dtype / in fp32 (same shape, same NaN pattern).  NaN pattern
    identical; masked entries exactly finfo(T).min; the rest under the project's gates."""
    y, ref_t, ref32 = y.cpu(), ref_t.cpu(), ref32.cpu()
    assert y.shape == ref_t.shape == ref32.shape and y.dtype == dtype, (what, y.shape, ref_t.shape, y.dtype)
    assert torch.equal(torch.isnan(y), torch.isnan(ref_t)), "%s: NaN pattern differs" % what
    lo = torch.finfo(dtype).min
    masked = ref_t == lo
    assert torch.equal(y == lo, masked), "%s: masked entries are not exactly finfo.min where the reference's are" % what
    vis = ~torch.isnan(ref_t) & ~masked
    assert bool(torch.isfinite(y[vis]).all())
    d32 = rel(y[vis], ref32[vis])
    if dtype == F32:
        print("%s fp32: HIP vs reference %.2e" % (what, d32))
        assert d32 <= 1e-4, (what, d32)
    else:
        own = rel(ref_t[vis], ref32[vis])
        print("%s %s: HIP vs ref-fp32 %.2e | reference %s vs fp32 %.2e" % (what, KC.NAME[dtype], d32, KC.NAME[dtype], own))
        assert d32 <= 1.5 * own + EPS16[dtype], (what, d32, own)
    # the + 1 of a one-row call sits on the same entries (an entry off by one whole unit is no rounding matter)
    assert float((y[vis].double() - ref32[vis].double()).abs().max()) < 0.5, what


# ---- kernel, element-wise -----------------------------------------------------------------------------------------------------
def scores_bound(q, k, dtype, row_calls):
    """(v, t) of every entry the mode writes, by kernel_check's steps; plus the masks."""
    M, kv, hd = q.shape[0], k.shape[0], q.shape[1]
    written, plus_one, masked = rule_masks(M, kv, row_calls)
    v, t = KC.accumulate(q, k, kacc=hd)
    v, t = KC.mid_round(v, t, dtype)
    v, t = KC.op32(v / math.sqrt(hd), t / math.sqrt(hd))
    v, t = KC.mid_round(v, t, dtype)
    s_v, s_t = v, t
    add = plus_one.double() + masked.double() * float(torch.finfo(dtype).min)
    v, t = KC.op32(v + add, t)
    v, t = KC.final_round(v, t, dtype)
    return v, t, s_v, s_t, written, plus_one, masked


def run_scores(ops, q, k, dtype, row_calls):
    """-> ([M, kv] on the CPU, NaN = never written); asserts nothing outside the mode's elements was touched"""
    M, kv = q.shape[0], k.shape[0]
    g = KC.GuardedOut(M + 2, kv, dtype, device=DEV, ld=kv + 3)        # NaN sentinels; rows 0 and M + 1 are guard rows
    qbuf = torch.zeros(M, 3 * q.shape[1], dtype=dtype, device=DEV)     # q rows with a stride, like the engine's
    qv = qbuf[:, q.shape[1]:2 * q.shape[1]]
    qv.copy_(q)
    ops.attn_scores(qv, k.to(DEV).contiguous(), g.out[1:M + 1], row_calls=row_calls)
    msgs, pay = g.problems()
    msgs = [m for m in msgs if "never written" not in m]               # leaving elements alone is this kernel's contract
    assert not msgs, "; ".join(msgs)
    bits = pay.view(KC._INT[dtype])
    untouched = bits == KC.SENTINEL[dtype]
    assert bool(untouched[0].all()) and bool(untouched[M + 1].all()), "a guard row was written"
    written = rule_masks(M, kv, row_calls)[0]
    assert torch.equal(~untouched[1:M + 1], written), "the set of written elements is not the mode's (M=%d kv=%d)" % (M, kv)
    return pay[1:M + 1]


@pytest.mark.parametrize("row_calls", [False, True], ids=["one_call", "row_calls"])
@pytest.mark.parametrize("hd", [128, 64])
@pytest.mark.parametrize("dtype", DTYPES, ids=KC.NAME.get)
def test_attn_scores_elementwise(ops, dtype, hd, row_calls):
    for n, (M, kv) in enumerate(SHAPES):
        g = torch.Generator().manual_seed(9000 + 100 * n + hd + int(row_calls))
        q, k = torch.randn(M, hd, generator=g).to(dtype), torch.randn(kv, hd, generator=g).to(dtype)
        y = run_scores(ops, q, k, dtype, row_calls)
        v, t, s_v, s_t, written, plus_one, masked = scores_bound(q, k, dtype, row_calls)
        what = "attn_scores %s hd=%d M=%d kv=%d row_calls=%d" % (KC.NAME[dtype], hd, M, kv, row_calls)
        checked = written & ~masked
        yd = torch.where(checked, y.double(), v)                        # the others are checked exactly below
        KC.check(yd, v, torch.where(checked, t, torch.zeros_like(t)), what, family="attn_scores", dtype=dtype)
        assert bool(torch.isfinite(y[checked]).all()), what
        if masked.any():        # exactly rnd_T(s + finfo.min), for every s the bound allows
            lo_add = float(torch.finfo(dtype).min)
            lo, hi = (s_v - s_t + lo_add).to(dtype).double(), (s_v + s_t + lo_add).to(dtype).double()
            ym = y.double()
            assert bool(((ym >= lo) & (ym <= hi))[masked].all()), what
            assert bool((lo == hi)[masked].all()), what                 # (these cases leave no room: the value is pinned)


def test_probe_fp16_mask_is_added_and_rounded(ops):
    """q . k = 724 -> rnd(724 / sqrt(128)) = 64.0; 64 - 65504 = -65440 is an fp16 number: a stored constant would read -65504."""
    q, k = torch.zeros(2, 128, dtype=FH), torch.zeros(2, 128, dtype=FH)
    q[0, :4] = torch.tensor([16., 16., 8., 2.], dtype=FH)
    k[1, :4] = torch.tensor([16., 16., 26., 2.], dtype=FH)
    y = run_scores(ops, q, k, FH, False)
    assert float(y[0, 1]) == -65440.0, float(y[0, 1])
    assert float(y[0, 0]) == 0.0 and float(y[1, 0]) == 0.0 and float(y[1, 1]) == 0.0


def exact_operands(M, kv, hd, dtype):
    """small integer scores, exact in every dtype: q . k = 8 ((j % 5 - 2) + (i % 3) (j % 2)), sqrt(64) = 8 -> s in [-2, 4]"""
    assert hd == 64
    q, k = torch.zeros(M, hd), torch.zeros(kv, hd)
    q[:, 0], q[:, 63] = 8.0, 8.0 * (torch.arange(M) % 3).float()
    k[:, 0], k[:, 63] = (torch.arange(kv) % 5 - 2).float(), (torch.arange(kv) % 2).float()
    s = (q.double() @ k.double().t()) / 8.0
    return q.to(dtype), k.to(dtype), s


@pytest.mark.parametrize("dtype", DTYPES, ids=KC.NAME.get)
def test_probe_single_row_plus_one_on_last_column_only(ops, dtype):
    q, k, s = exact_operands(1, 47, 64, dtype)
    y = run_scores(ops, q, k, dtype, False).double()
    exp = s.clone()
    exp[0, -1] += 1.0
    assert torch.equal(y, exp), (y - s)


@pytest.mark.parametrize("dtype", DTYPES, ids=KC.NAME.get)
def test_probe_row_calls_own_column_and_nan_beyond(ops, dtype):
    M, kv = 37, 70                      # two row tiles, two key tiles
    q, k, s = exact_operands(M, kv, 64, dtype)
    y = run_scores(ops, q, k, dtype, True).double()
    for i in range(M):
        own = kv - M + i
        assert float(y[i, own]) == float(s[i, own]) + 1.0, (i, own)
        assert torch.equal(y[i, :own], s[i, :own]), i
        if own + 1 < kv:
            assert bool(torch.isnan(y[i, own + 1:]).all()), i


def test_zz_worst_ratio():
    """prints the table of the module docstring; the cases above have already failed on any ratio over 1"""
    print("\n" + KC.worst_table())
    assert all(r <= 1.0 for (family, _), r in KC.WORST.items() if family == "attn_scores")


# ---- engine against the real reference ------------------------------------------------------------------------------------------
def _img_ids(meta):
    lo, hi = meta["IMG_IDS"]
    return list(range(lo, hi + 1))


def _engine(meta, dtype, **kw):
    from seedstory.llama import LlamaEngine
    d = meta["LLAMA"]
    wd = synth.llama_weights(11, d["hidden"], d["n_heads"], d["n_layers"], d["inter"], d["vocab"], dtype=dtype)
    eng = LlamaEngine(wd, hidden=d["hidden"], n_heads=d["n_heads"], n_layers=d["n_layers"], inter=d["inter"],
                      vocab=d["vocab"], dtype=dtype, device=DEV, cache_cap=256, max_new=128, max_prefill_rows=96,
                      img_ids=_img_ids(meta), **kw)
    return eng, wd


@pytest.fixture(scope="module")
def maps_golden():
    import os
    from safetensors.torch import load_file
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return load_file(os.path.join(root, "tests", "golden", "attn_maps_tiny.safetensors"))


@pytest.mark.parametrize("dtype", DTYPES, ids=KC.NAME.get)
def test_engine_maps_match_the_reference(golden, maps_golden, dtype):
    """prefill 37, continuation 9, one forced decode token through the graph: the maps the real LlamaForCausalLM returned."""
    g, meta = golden
    eng, wd = _engine(meta, dtype)
    emb = wd["model.embed_tokens.weight"]
    with eng.attn_capture(48, 48) as maps:
        eng.prefill(emb[g["llama_f32.ids"][0]])
        eng.prefill(emb[g["llama_f32.ids2"][0]])
        tok = int(g["llama_f32.ids3"][0, 0])
        n = eng.generate(2, last_prompt_id=5, forced=[tok, 3])
        assert n == 2 and eng.lengths() == (47, 47)
    maps = maps.cpu()
    assert maps.shape == (2, 48, 48)
    for l in range(2):
        for call, r0, r1, kv in (("prefill", 0, 37, 37), ("cont", 37, 46, 46), ("decode", 46, 47, 47)):
            ref_t, ref32 = maps_golden["%s.%s.%d" % (TAG[dtype], call, l)], maps_golden["f32.%s.%d" % (call, l)]
            gate_maps(maps[l, r0:r1, :kv], ref_t, ref32, dtype, "layer %d %s" % (l, call))
            assert bool(torch.isnan(maps[l, r0:r1, kv:]).all())        # beyond the call's key count: the caller's NaN
        assert bool(torch.isnan(maps[l, 47:]).all())
        # the decode row, column by column: the last one carries the + 1 (the fp32 reference holds s + 1 there), every other one
        # is within rounding of the reference's bare s.  Scores are O(1) here; 0.05 is 6 bf16 ulps of 1, far from the whole unit
        # a missing or misplaced + 1 makes.  (rnd_T(s + 1) itself is pinned bit for bit by the M == 1 probe above.)
        dec, ref32 = maps[l, 46, :47].double(), maps_golden["f32.decode.%d" % l][0].double()
        assert abs(float(dec[46] - ref32[46])) < 0.05, (l, float(dec[46]), float(ref32[46]))
        assert float((dec[:46] - ref32[:46]).abs().max()) < 0.05, l


# ---- generate and merge against the oracle ----------------------------------------------------------------------------------------
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


def _agent(meta, dtype, output_attentions=True):
    from src.models.qwen_visual import Resampler
    from src.models_clm.modeling_llama_xformer import LlamaConfig, LlamaForCausalLM
    from src.models_clm.models import ContinuousLVLM
    d = meta["LLAMA"]
    cfg = LlamaConfig(hidden_size=d["hidden"], intermediate_size=d["inter"], num_hidden_layers=d["n_layers"],
                      num_attention_heads=d["n_heads"], vocab_size=d["vocab"])
    cfg.output_attentions = output_attentions                   # the one bit the reference's users flip
    llm = LlamaForCausalLM(cfg)
    wd = synth.llama_weights(11, d["hidden"], d["n_heads"], d["n_layers"], d["inter"], d["vocab"], dtype=dtype)
    missing, unexpected = llm.load_state_dict(wd, strict=False)
    assert not missing and not unexpected
    llm.cache_cap, llm.max_new, llm.max_prefill_rows = 256, 128, 96
    llm.use_kv_cache_head = False
    rin = Resampler(grid_size=meta["RES_IN"]["grid"], embed_dim=256, num_heads=2, kv_dim=256)
    rin.load_state_dict(synth.resampler_weights(21, "", meta["RES_IN"]["grid"], 256))
    rout = Resampler(grid_size=meta["RES_OUT"]["grid"], embed_dim=256, num_heads=2, kv_dim=256)
    rout.load_state_dict(synth.resampler_weights(22, "", meta["RES_OUT"]["grid"], 256))
    return ContinuousLVLM(llm, rin, rout).eval().to(DEV, dtype), wd


class Recorder:
    """stands in for seedstory_oracle.attention_bottom_right_causal: records head 0's (q, k) of every call, then does its job"""

    def __init__(self, monkeypatch):
        self.calls = []
        self.orig = O.attention_bottom_right_causal
        monkeypatch.setattr(O, "attention_bottom_right_causal", self)

    def __call__(self, q, k, v):
        self.calls.append((q[0, 0].clone(), k[0, 0].clone()))
        return self.orig(q, k, v)

    def take(self, n_layers):
        """-> per layer, the list of (q, k) in feeding order"""
        per = [self.calls[l::n_layers] for l in range(n_layers)]
        self.calls = []
        return per


def oracle_maps(rec, meta, dtype, ids, forced, n_new, img_ids):
    """merged maps [layers][rows, width] of the oracle's greedy run in `dtype`; image-token block rows are one-row calls anyway
    (the oracle feeds every generated token alone, like the reference)"""
    d = meta["LLAMA"]
    dims = O.LlamaDims(d["hidden"], d["n_heads"], d["n_layers"], d["inter"], d["vocab"])
    wd = synth.llama_weights(11, d["hidden"], d["n_heads"], d["n_layers"], d["inter"], d["vocab"], dtype=dtype)
    gen, _, _, _ = O.greedy_generate(wd, dims, ids, wd["model.embed_tokens.weight"][ids], img_ids, n_new, forced=forced)
    assert gen == list(forced)
    return [merged_map([(q, k, False) for q, k in calls], dtype) for calls in rec.take(d["n_layers"])]


@pytest.mark.parametrize("dtype", DTYPES, ids=KC.NAME.get)
def test_generate_attn_weights_match_the_oracle(golden, monkeypatch, dtype):
    g, meta = golden
    img = _img_ids(meta)
    S, n = 12, 20
    ids = synth.randint(61, (1, S), 3, 250)
    forced = synth.randint(62, (5,), 3, 250).tolist() + [img[0]] + img[1:15]          # 20 tokens, one <img> block
    rec = Recorder(monkeypatch)
    ref_t = oracle_maps(rec, meta, dtype, ids, forced, n, img)
    ref32 = ref_t if dtype == F32 else oracle_maps(rec, meta, F32, ids, forced, n, img)
    agent, _ = _agent(meta, dtype)
    outs = []
    real_generate = agent.llm.generate
    monkeypatch.setattr(agent.llm, "generate", lambda **kw: outs.append(real_generate(**kw)) or outs[-1])
    out = agent.generate(tokenizer=_Tok(img), input_ids=ids, max_new_tokens=n, num_img_gen_tokens=64, forced_tokens=forced)
    assert out["generate_ids"].tolist() == forced
    aw = out["attn_weights"]
    assert isinstance(aw, tuple) and len(aw) == meta["LLAMA"]["n_layers"]
    for l, a in enumerate(aw):
        assert a.shape == (1, S + n - 1, S + n - 1) and a.dtype == dtype
        gate_maps(a[0], ref_t[l], ref32[l], dtype, "generate layer %d" % l)
    # HF-style per-step tuples: as many as hidden_states, views of the one buffer, and the reference's merge gives attn_weights
    go = outs[0]
    assert len(go.attentions) == len(go.hidden_states) == n
    assert go.attentions[0][0].shape == (1, S, S) and go.attentions[3][1].shape == (1, 1, S + 3)
    base = go.attention_maps
    lo_ptr, hi_ptr = base.data_ptr(), base.data_ptr() + base.stride(0) * base.shape[0] * base.element_size()
    assert all(lo_ptr <= t.data_ptr() < hi_ptr for step in go.attentions for t in step)
    for l in range(len(aw)):
        assert same(merge_attn_weights([step[l] for step in go.attentions]), aw[l])


def test_generate_without_the_flag_returns_no_maps(golden):
    g, meta = golden
    img = _img_ids(meta)
    agent, _ = _agent(meta, F32, output_attentions=False)
    ids = synth.randint(61, (1, 12), 3, 250)
    out = agent.generate(tokenizer=_Tok(img), input_ids=ids, max_new_tokens=4, num_img_gen_tokens=64, forced_tokens=[7, 8, 9, 10])
    assert out["attn_weights"] == ()
    # the keyword alone works too, on the single forward call; a first call of ONE row follows the one-row rule
    emb = agent.llm.model.embed_tokens(ids.to(DEV))
    r = agent.llm(inputs_embeds=emb[:, :1], output_attentions=True)
    assert len(r.attentions) == 2 and r.attentions[0].shape == (1, 1, 1)
    r2 = agent.llm(inputs_embeds=emb[:, 1:6], past_key_values=r.past_key_values, output_attentions=True)
    assert r2.attentions[1].shape == (1, 5, 6) and float(r2.attentions[1][0, 0, 5]) == torch.finfo(F32).min
    assert agent.llm(inputs_embeds=emb[:, :3]).attentions is None


# ---- invariants, bit-exact --------------------------------------------------------------------------------------------------------
def _run(meta, g, dtype, capture, graph=1):
    with knobs(llama_graph=graph):
        eng, wd = _engine(meta, dtype)
        emb = wd["model.embed_tokens.weight"]
        maps = eng.attn_capture_on(64, 64) if capture else None
        try:
            eng.prefill(emb[g["llama_f32.ids"][0]])
            n = eng.generate(14, last_prompt_id=7, forced=[11, 12, 13])
        finally:
            eng.attn_capture_off()
        kv = eng.lengths()[0]
        return dict(n=n, ids=eng.gen_ids[:n].tolist(), hid=eng.hidden_rows[:n - 1].clone(), logits=eng.logits.clone(),
                    k=eng.k_cache[:, :, :kv].clone(), v=eng.v_cache[:, :, :kv].clone(),
                    maps=None if maps is None else maps.clone())


@pytest.mark.parametrize("dtype", [F32, BF], ids=KC.NAME.get)
def test_capture_changes_nothing_else_and_graph_equals_eager(golden, dtype):
    g, meta = golden
    off, on, eager = _run(meta, g, dtype, False), _run(meta, g, dtype, True), _run(meta, g, dtype, True, graph=0)
    assert on["n"] == off["n"] and on["ids"] == off["ids"]
    for key in ("hid", "logits", "k", "v"):
        assert torch.equal(on[key], off[key]), key
    assert same(on["maps"], eager["maps"])
    rows = 37 + on["n"] - 1
    assert not bool(torch.isnan(on["maps"][:, :rows, 0]).any()) and bool(torch.isnan(on["maps"][:, rows:]).all())


# ---- image-token block --------------------------------------------------------------------------------------------------------------
def test_img_block_on_against_off(golden):
    """The block feeds its 66 rows as one continuation (projections as GEMM), the loop feeds them one by one (GEMV): same NaN / + 1
    structure, values within 1e-4 relative — not bit-equal."""
    g, meta = golden
    img = _img_ids(meta)
    ids = synth.randint(61, (1, 12), 3, 250)
    forced = synth.randint(63, (4,), 3, 250).tolist() + img + synth.randint(64, (5,), 3, 250).tolist()
    res = []
    for on in (1, 0):
        with knobs(img_block_decode=on):
            agent, _ = _agent(meta, F32)
            out = agent.generate(tokenizer=_Tok(img), input_ids=ids, max_new_tokens=len(forced), num_img_gen_tokens=64,
                                 forced_tokens=forced)
            assert out["generate_ids"].tolist() == forced
            res.append(torch.stack([a[0] for a in out["attn_weights"]]).cpu())
    a, b = res
    assert a.shape == b.shape == (2, 12 + len(forced) - 1, 12 + len(forced) - 1)
    assert torch.equal(torch.isnan(a), torch.isnan(b))
    lo = torch.finfo(F32).min
    assert torch.equal(a == lo, b == lo)
    vis = ~torch.isnan(a) & (a != lo)
    assert rel(a[vis], b[vis]) <= 1e-4
    assert float((a[vis] - b[vis]).abs().max()) < 1e-3          # the + 1 sits on the same entries


# ---- sink path ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=KC.NAME.get)
def test_sink_path_maps_match_the_oracle(golden, monkeypatch, dtype):
    """prefill 37 -> kv_gather to a kept subset -> capture with row0 = the new length -> continuation 9 + 3 decode tokens."""
    g, meta = golden
    d = meta["LLAMA"]
    keep = list(range(0, 5)) + list(range(20, 37))
    ids1, ids2 = g["llama_f32.ids"], g["llama_f32.ids2"]
    toks = [21, 22, 23, 24]                                     # generate 4, feed 3
    dims = O.LlamaDims(d["hidden"], d["n_heads"], d["n_layers"], d["inter"], d["vocab"])
    rec = Recorder(monkeypatch)

    def oracle(dt):
        wd = synth.llama_weights(11, d["hidden"], d["n_heads"], d["n_layers"], d["inter"], d["vocab"], dtype=dt)
        emb = wd["model.embed_tokens.weight"]
        _, _, past = O.llama_forward(wd, dims, emb[ids1], torch.arange(37).unsqueeze(0), None)
        rec.take(d["n_layers"])
        past = [(k[:, :, keep], v[:, :, keep]) for k, v in past]
        _, _, past = O.llama_forward(wd, dims, emb[ids2], torch.arange(37, 46).unsqueeze(0), past)
        for i, t in enumerate(toks[:3]):
            _, _, past = O.llama_forward(wd, dims, emb[torch.tensor([[t]])], torch.tensor([[46 + i]]), past)
        return [merged_map([(q, k, False) for q, k in calls], dt) for calls in rec.take(d["n_layers"])]

    ref_t = oracle(dtype)
    ref32 = ref_t if dtype == F32 else oracle(F32)
    eng, wd = _engine(meta, dtype)
    emb = wd["model.embed_tokens.weight"]
    eng.prefill(emb[ids1[0]])
    eng.kv_gather(keep)
    assert eng.lengths() == (len(keep), 37)
    with eng.attn_capture(13, len(keep) + 13) as maps:          # row0 = the cache length after the gather
        eng.prefill(emb[ids2[0]])
        assert eng.generate(4, last_prompt_id=int(ids2[0, -1]), forced=toks) == 4
    rows, width = 12, len(keep) + 12
    assert bool(torch.isnan(maps[:, rows:]).all()) and bool(torch.isnan(maps[:, :, width:]).all())
    for l in range(d["n_layers"]):
        assert ref_t[l].shape == (rows, width)
        gate_maps(maps[l, :rows, :width], ref_t[l], ref32[l], dtype, "sink layer %d" % l)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_start_no_device_work(golden):
    from seedstory import _lib
    from seedstory._lib import lib
    g, meta = golden
    eng, wd = _engine(meta, BF, n_seq=2)
    emb = wd["model.embed_tokens.weight"]
    rows = emb[g["llama_f32.ids"][0]]
    k_before = eng.k_cache.clone()

    def untouched():
        return eng.lengths() == (0, 0) and torch.equal(eng.k_cache, k_before)

    maps = eng.attn_capture_on(64, 64)
    with pytest.raises(_lib.SSError):
        eng.prefill_batch([rows[:5], rows[:7]])
    with pytest.raises(_lib.SSError):
        eng.generate_batch(4, [5, 6])
    with pytest.raises(_lib.SSError):
        eng.generate_batch_img_block(4, [5, 6])
    # the C ABI refuses by itself too
    one = (C.c_int64 * 2)(5, 5)
    stack = rows[:10].to(DEV, BF).contiguous()
    assert lib().ss_llama_prefill_batch(eng._h, stack.data_ptr(), one, None, None) == -1
    last, out = (C.c_int32 * 2)(5, 6), (C.c_int64 * 2)()
    assert lib().ss_llama_generate_batch(eng._h, 4, last, None, 0, None, None, out, None) == -1
    assert untouched() and bool(torch.isnan(maps).all())
    eng.attn_capture_off()
    for r, c in ((10, 64), (64, 10)):                           # too few rows, too few columns
        maps = eng.attn_capture_on(r, c)
        with pytest.raises(_lib.SSError):
            eng.prefill(rows)
        assert untouched() and bool(torch.isnan(maps).all())
        eng.attn_capture_off()
    maps = eng.attn_capture_on(8, 8)
    eng.prefill(rows[:5])
    before = (eng.lengths(), eng.gen_ids.clone(), maps.clone())
    with pytest.raises(_lib.SSError):
        eng.generate(10, last_prompt_id=5, forced=[7, 8, 9])    # 5 + 10 rows do not fit 8
    assert eng.lengths() == before[0] and torch.equal(eng.gen_ids, before[1]) and same(maps, before[2])
    assert eng.generate(3, last_prompt_id=5, forced=[7, 8, 9]) == 3     # 5 + 3 do
    eng.attn_capture_off()
    assert eng.generate(2, last_prompt_id=9, forced=[7, 8]) == 2        # off again: the plain loop

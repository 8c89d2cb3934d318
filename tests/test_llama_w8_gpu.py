"""LlamaEngine with fp8 (e4m3) weight-only decode projections (decode_weights="fp8", ss_llama_set_decode_w8).

The toy LLaMA of tests/golden/hotpath_tiny.json.  Its weights are quantised per output row with POWER-OF-TWO scales, so
s * dec(q) is exactly representable in the model dtype: an engine that decodes from the fp8 planes and a 16-bit engine whose
weights are the de-quantised tensors compute the same function with the same rounding points, apart from the fp32 summation
order of the GEMV forms.  Under teacher-forced tokens their hidden rows and K / V cache rows must agree within the tolerance the
suite already uses for two 16-bit engines that differ only in GEMV form: rel < 2e-2 in bf16
(test_llama_slot_batched_decode_equals_single), 5e-3 in fp16 (tests/test_fp16_gpu.py, the same comparison)."""
import math

import pytest
import torch

import synth
from test_engine_gpu import DEV, _img_ids, rel
from test_kernel_edges_gpu import knobs

pytestmark = pytest.mark.gpu
F8 = torch.float8_e4m3fn
TOL = {torch.bfloat16: 2e-2, torch.float16: 5e-3}
PROJ = [("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj"), ("self_attn.o_proj",), ("mlp.gate_proj", "mlp.up_proj"),
        ("mlp.down_proj",)]


def quant_pow2(w):
    """w [N, K] -> (q uint8, s fp32 [N] powers of two with amax / s in (224, 448], de-quantised fp64)"""
    amax = w.float().abs().amax(dim=1).clamp_min(2.0 ** -40)
    s = 2.0 ** torch.ceil(torch.log2(amax / 448.0))
    q = (w.float() / s[:, None]).to(F8).view(torch.uint8)
    assert not ((q & 0x7f) == 0x7f).any()
    return q, s, q.view(F8).double() * s.double()[:, None]


_CACHE = {}


def toy(meta, dtype):
    """(state dict of de-quantised weights in `dtype`, per-layer fp8 planes, lm_head plane), computed once per dtype"""
    if dtype not in _CACHE:
        d = meta["LLAMA"]
        wd = dict(synth.llama_weights(11, d["hidden"], d["n_heads"], d["n_layers"], d["inter"], d["vocab"], dtype=dtype))
        layers = []
        for l in range(d["n_layers"]):
            planes = []
            for names in PROJ:
                qs, ss = [], []
                for n in names:
                    key = "model.layers.%d.%s.weight" % (l, n)
                    q, s, back = quant_pow2(wd[key])
                    wd[key] = back.to(dtype)
                    assert torch.equal(wd[key].double(), back), key       # s * dec(q) is exact in the model dtype
                    qs.append(q), ss.append(s)
                planes.append((torch.cat(qs), torch.cat(ss)))
            layers.append(planes)
        q, s, back = quant_pow2(wd["lm_head.weight"])
        wd["lm_head.weight"] = back.to(dtype)
        assert torch.equal(wd["lm_head.weight"].double(), back)
        _CACHE[dtype] = (wd, layers, (q, s))
    return _CACHE[dtype]


def engine(meta, dtype, fp8, **kw):
    from seedstory.llama import LlamaEngine
    d = meta["LLAMA"]
    wd, layers, lm = toy(meta, dtype if dtype != torch.float32 else torch.bfloat16)
    eng = LlamaEngine(wd, hidden=d["hidden"], n_heads=d["n_heads"], n_layers=d["n_layers"], inter=d["inter"], vocab=d["vocab"],
                      dtype=dtype, device=DEV, cache_cap=256, max_new=128, max_prefill_rows=64, img_ids=_img_ids(meta), **kw)
    if fp8:
        eng.set_decode_fp8([[(q.to(DEV), s.to(DEV)) for q, s in planes] for planes in layers], (lm[0].to(DEV), lm[1].to(DEV)))
        assert eng.decode_weights == "fp8"
    return eng, wd


def prompts_forced(n_seq, steps):
    prompts = [synth.randint(140 + b, (19 + 5 * b,), 3, 250) for b in range(n_seq)]
    forced = [synth.randint(240 + b, (steps,), 3, 250).tolist() for b in range(n_seq)]
    return prompts, forced


def run(eng, wd, prompts, forced, steps):
    """prefill + teacher-forced decode of every slot -> per slot (n, ids, hidden rows, K rows, V rows, prefill logits)"""
    S = len(prompts)
    emb = wd["model.embed_tokens.weight"]
    pre = []
    for b in range(S):
        eng.select(b).prefill(emb[prompts[b]])
        pre.append(eng.logits.clone())
    if S == 1:
        ns = [eng.select(0).generate(steps, last_prompt_id=int(prompts[0][-1]), forced=forced[0])]
    else:
        ns = eng.generate_batch(steps, [int(p[-1]) for p in prompts], forced=forced)
    out = []
    for b in range(S):
        eng.select(b)
        n, kv = ns[b], eng.lengths()[0]
        out.append((n, eng.gen_ids[:n].tolist(), eng.hidden_rows[:max(n - 1, 0)].clone(), eng.k_cache[:, :, :kv].clone(),
                    eng.v_cache[:, :, :kv].clone(), pre[b]))
    return out


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("n_seq", [1, 8])
def test_llama_w8_decode_equals_dequantised_16bit(golden, n_seq, dtype):
    """fp8 planes vs the 16-bit engine over the de-quantised weights, teacher-forced; at 8 slots the last one is forced to EOS at
    its third token and stops early.  The prefill is the 16-bit one in both engines: its logits are bit-identical."""
    _, meta = golden
    steps = 10
    prompts, forced = prompts_forced(n_seq, steps)
    if n_seq > 1:
        forced[-1] = forced[-1][:2] + [2]
    e8, wd = engine(meta, dtype, True, n_seq=n_seq)
    a = run(e8, wd, prompts, forced, steps)
    e16, _ = engine(meta, dtype, False, n_seq=n_seq)
    b = run(e16, wd, prompts, forced, steps)
    for s in range(n_seq):
        want = 3 if (n_seq > 1 and s == n_seq - 1) else steps
        assert a[s][0] == b[s][0] == want and a[s][1] == b[s][1] == forced[s][:want], s
        assert torch.equal(a[s][5], b[s][5]), "prefill logits differ (slot %d): prefill must not see the fp8 planes" % s
        assert a[s][3].shape == b[s][3].shape
        for j, name in ((2, "hidden rows"), (3, "K rows"), (4, "V rows")):
            r = rel(a[s][j], b[s][j])
            print("w8 vs dequantised 16-bit, %s n_seq %d slot %d %s: rel %.3g" % (dtype, n_seq, s, name, r))
            assert math.isfinite(r) and r < TOL[dtype], (s, name, r)
    if n_seq == 1:      # the fp8 token really is another kernel: not bit-identical to the 16-bit forms at every row
        assert a[0][2].shape[0] == steps - 1


def test_llama_w8_graph_equals_eager_and_toggle(golden):
    """graph decode == eager decode bit for bit with fp8 on; on -> off -> on returns bit-identical results (no stale graph), off
    is the 16-bit engine bit for bit, and new planes are what the next decode reads"""
    _, meta = golden
    dtype, steps = torch.bfloat16, 12
    prompts, forced = prompts_forced(1, steps)
    forced = [forced[0][:4]]                    # four forced tokens, then greedy
    outs = {}
    for use_graph in (1, 0):
        with knobs(llama_graph=use_graph):
            eng, wd = engine(meta, dtype, True)
            outs[use_graph] = run(eng, wd, prompts, forced, steps)[0]
    assert outs[1][1] == outs[0][1]
    for j in (2, 3, 4):
        assert torch.equal(outs[1][j], outs[0][j])
    # one engine: on (graph captured), off (16-bit graph), on again (planes set anew)
    eng, wd = engine(meta, dtype, True)
    _, layers, lm = toy(meta, dtype)
    planes = [[(q.to(DEV), s.to(DEV)) for q, s in pl] for pl in layers], (lm[0].to(DEV), lm[1].to(DEV))
    on1 = run(eng, wd, prompts, forced, steps)[0]
    eng.reset()
    eng.set_decode_fp8(None, None)
    assert eng.decode_weights is None
    off = run(eng, wd, prompts, forced, steps)[0]
    eng.reset()
    eng.set_decode_fp8(*planes)
    on2 = run(eng, wd, prompts, forced, steps)[0]
    ref16, _ = engine(meta, dtype, False)
    r16 = run(ref16, wd, prompts, forced, steps)[0]
    assert on1[1] == on2[1] == outs[1][1] and off[1] == r16[1]
    for j in (2, 3, 4):
        assert torch.equal(on1[j], on2[j]) and torch.equal(on1[j], outs[1][j]), "fp8 on -> off -> on changed the result"
        assert torch.equal(off[j], r16[j]), "fp8 off is not the 16-bit engine"
    # the decode really reads the planes it was given: with the lm_head scales doubled (a power of two: exact) the decode logits
    # double bit for bit, while the prefill logits (16-bit lm_head) and the hidden rows stay what they were
    eng.reset()
    eng.set_decode_fp8(planes[0], (planes[1][0], planes[1][1] * 2.0))
    forced_all = [on1[1]]                       # the tokens of the run above, teacher-forced: the sampled ones must not move
    x2 = run(eng, wd, prompts, forced_all, steps)[0]
    log2 = eng.logits.clone()
    eng.reset()
    eng.set_decode_fp8(*planes)
    x1 = run(eng, wd, prompts, forced_all, steps)[0]
    assert x1[1] == x2[1] == on1[1] and torch.equal(x1[2], x2[2]) and torch.equal(x1[2], on1[2])
    assert torch.equal(x1[5], x2[5]) and torch.equal(x1[5], on1[5])
    assert torch.isfinite(log2).all() and torch.equal(log2, eng.logits * 2.0) and bool(eng.logits.abs().sum() > 0)


def test_llama_w8_prefill_untouched_and_attn_capture(golden):
    """prefill hidden rows and logits are bit-identical with the option on and off; attention-map capture with fp8 on runs (eager and
    graph) and fills one row per decode token, equal to the rows the 16-bit engine over the same weights captures within TOL"""
    _, meta = golden
    dtype, steps = torch.bfloat16, 6
    prompts, forced = prompts_forced(1, steps)
    emb = None
    res = {}
    for fp8 in (True, False):
        eng, wd = engine(meta, dtype, fp8)
        emb = wd["model.embed_tokens.weight"]
        hid = eng.prefill(emb[prompts[0]], want_hidden=True)
        P = prompts[0].numel()
        maps = eng.attn_capture_on(steps, P + steps)
        n = eng.generate(steps, last_prompt_id=int(prompts[0][-1]), forced=forced[0])
        eng.attn_capture_off()
        res[fp8] = (hid.clone(), eng.logits.clone(), maps.clone(), n)
    assert torch.equal(res[True][0], res[False][0])
    m8, m16 = res[True][2].float().cpu(), res[False][2].float().cpu()
    P = prompts[0].numel()
    fed = res[True][3] - 1                       # the token that hits the limit is sampled, not forwarded
    assert res[True][3] == res[False][3] == steps
    for r in range(fed):
        row8, row16 = m8[:, r, :P + r + 1], m16[:, r, :P + r + 1]
        assert torch.isfinite(row8).all(), r
        assert torch.isnan(m8[:, r, P + r + 1:]).all()
        assert rel(row8, row16) < TOL[dtype], r


def test_llama_w8_refusals_and_own_weights(golden):
    """an fp32 engine refuses; enable_decode_fp8 (the engine's own merged weights, amax / 448 scales) and decode_weights="fp8" /
    the llama_decode_w8 knob switch it on; profile_decode reports the bytes the fp8 token streams.  Records the relative logits
    error of fp8 decode against the 16-bit decode of the same (un-quantised) toy weights."""
    from seedstory._lib import SSError
    from seedstory.llama import LlamaEngine
    _, meta = golden
    d = meta["LLAMA"]
    e32, _ = engine(meta, torch.float32, False)
    with pytest.raises(SSError, match="bf16 / fp16"):
        _, layers, lm = toy(meta, torch.bfloat16)
        e32.set_decode_fp8([[(q.to(DEV), s.to(DEV)) for q, s in pl] for pl in layers], (lm[0].to(DEV), lm[1].to(DEV)))
    wd = synth.llama_weights(11, d["hidden"], d["n_heads"], d["n_layers"], d["inter"], d["vocab"], dtype=torch.bfloat16)
    kw = dict(hidden=d["hidden"], n_heads=d["n_heads"], n_layers=d["n_layers"], inter=d["inter"], vocab=d["vocab"],
              dtype=torch.bfloat16, device=DEV, cache_cap=256, max_new=128, max_prefill_rows=64, img_ids=_img_ids(meta))
    with pytest.raises(ValueError):
        LlamaEngine(wd, decode_weights="int4", **kw)
    e16 = LlamaEngine(wd, **kw)
    assert e16.decode_weights is None
    e8 = LlamaEngine(wd, decode_weights="fp8", **kw)
    with knobs(llama_decode_w8=1):
        ek = LlamaEngine(wd, **kw)
        e32k = LlamaEngine(wd, **dict(kw, dtype=torch.float32))     # the knob leaves fp32 engines alone
    assert e8.decode_weights == "fp8" and ek.decode_weights == "fp8" and e32k.decode_weights is None
    prompts, forced = prompts_forced(1, 8)
    outs = [run(e, wd, prompts, forced, 8)[0] for e in (e16, e8, ek)]
    assert torch.equal(outs[1][2], outs[2][2])
    r = rel(outs[1][2], outs[0][2])
    rl = rel(e8.logits, e16.logits)
    print("fp8 decode (amax / 448 row scales) vs 16-bit decode, toy engine: hidden rows rel %.3g, last logits rel %.3g" % (r, rl))
    # e4m3 keeps 4 significand bits: 2^-4 / sqrt(3) = 3.6e-2 rms per weight; not a gate on quality, a gate against a broken path
    assert math.isfinite(r) and 0 < r < 0.25
    H, I, L, V = d["hidden"], d["inter"], d["n_layers"], d["vocab"]
    p8, p16 = e8.profile_decode(2), e16.profile_decode(2)
    assert p16["gemv_bytes"] == (L * (4 * H * H + 2 * H * I) + V * H) * 2 and p16["gemv_down_bytes"] == L * H * I * 2
    assert p8["gemv_bytes"] == L * (4 * H * H + 2 * H * I) + V * H + 4 * (L * (4 * H + 2 * I) + V)
    assert p8["gemv_down_bytes"] == L * H * I + 4 * L * H
    assert p8["gemv_launches"] == p16["gemv_launches"] and p8["token_ms"] > 0

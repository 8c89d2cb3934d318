"""LlamaEngine with MXFP4 weight-only decode projections (decode_weights="mxfp4", ss_llama_set_decode_mx4).

The toy LLaMA of tests/golden/hotpath_tiny.json (hidden 256, inter 512: multiples of 32).  Its weights are quantised with
tests/mxfp4_ref.py; dec * 2^X is exactly representable in the model dtype, so an engine that decodes from the MXFP4 planes and a
16-bit engine whose weights are the de-quantised tensors compute the same function with the same rounding points, apart from
the fp32 summation order of the GEMV forms.  Under teacher-forced tokens their hidden rows and K / V cache rows must agree
within the tolerance the suite already uses for two engines that differ only in GEMV form: rel < 2e-2 in bf16
(test_llama_slot_batched_decode_equals_single), 5e-3 in fp16 (tests/test_fp16_gpu.py, the same comparison)."""
import math

import pytest
import torch

import mxfp4_ref as R
import synth
from test_engine_gpu import DEV, _img_ids, rel
from test_kernel_edges_gpu import knobs
from test_llama_w8_gpu import PROJ, TOL, prompts_forced, run
from test_llama_w8_gpu import engine as engine_w8

pytestmark = pytest.mark.gpu

_CACHE = {}


def toy(meta, dtype):
    """(state dict of de-quantised weights in `dtype`, per-layer MXFP4 planes, lm_head planes), computed once per dtype"""
    if dtype not in _CACHE:
        d = meta["LLAMA"]
        wd = dict(synth.llama_weights(11, d["hidden"], d["n_heads"], d["n_layers"], d["inter"], d["vocab"], dtype=dtype))

        def quant(key):
            cu, su, back = R.quantize_packed(wd[key])
            wd[key] = back.to(dtype)
            assert torch.equal(wd[key].double(), back), key           # dec * 2^X is exact in the model dtype
            return cu, su

        layers = []
        for l in range(d["n_layers"]):
            planes = []
            for names in PROJ:
                parts = [quant("model.layers.%d.%s.weight" % (l, n)) for n in names]
                planes.append((torch.cat([c for c, _ in parts]), torch.cat([s for _, s in parts])))
            layers.append(planes)
        _CACHE[dtype] = (wd, layers, quant("lm_head.weight"))
    return _CACHE[dtype]


def dev_planes(layers, lm):
    return [[(c.to(DEV), s.to(DEV)) for c, s in pl] for pl in layers], (lm[0].to(DEV), lm[1].to(DEV))


def engine(meta, dtype, mx4, **kw):
    from seedstory.llama import LlamaEngine
    d = meta["LLAMA"]
    wd, layers, lm = toy(meta, dtype if dtype != torch.float32 else torch.bfloat16)
    eng = LlamaEngine(wd, hidden=d["hidden"], n_heads=d["n_heads"], n_layers=d["n_layers"], inter=d["inter"], vocab=d["vocab"],
                      dtype=dtype, device=DEV, cache_cap=256, max_new=128, max_prefill_rows=64, img_ids=_img_ids(meta), **kw)
    if mx4:
        eng.set_decode_mxfp4(*dev_planes(layers, lm))
        assert eng.decode_weights == "mxfp4"
    return eng, wd


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("n_seq", [1, 8])
def test_llama_mx4_decode_equals_dequantised_16bit(golden, n_seq, dtype):
    """MXFP4 planes vs the 16-bit engine over the de-quantised weights, teacher-forced; at 8 slots the last one is forced to EOS at
    its third token and stops early.  The prefill is the 16-bit one in both engines: its logits are bit-identical."""
    _, meta = golden
    steps = 10
    prompts, forced = prompts_forced(n_seq, steps)
    if n_seq > 1:
        forced[-1] = forced[-1][:2] + [2]
    e4, wd = engine(meta, dtype, True, n_seq=n_seq)
    a = run(e4, wd, prompts, forced, steps)
    e16, _ = engine(meta, dtype, False, n_seq=n_seq)
    b = run(e16, wd, prompts, forced, steps)
    for s in range(n_seq):
        want = 3 if (n_seq > 1 and s == n_seq - 1) else steps
        assert a[s][0] == b[s][0] == want and a[s][1] == b[s][1] == forced[s][:want], s
        assert torch.equal(a[s][5], b[s][5]), "prefill logits differ (slot %d): prefill must not see the MXFP4 planes" % s
        assert a[s][3].shape == b[s][3].shape
        for j, name in ((2, "hidden rows"), (3, "K rows"), (4, "V rows")):
            r = rel(a[s][j], b[s][j])
            print("mx4 vs dequantised 16-bit, %s n_seq %d slot %d %s: rel %.3g" % (dtype, n_seq, s, name, r))
            assert math.isfinite(r) and r < TOL[dtype], (s, name, r)
    if n_seq == 1:
        assert a[0][2].shape[0] == steps - 1


def test_llama_mx4_graph_equals_eager_and_toggle(golden):
    """graph decode == eager decode bit for bit with MXFP4 on; on -> off -> on returns bit-identical results (no stale graph), off
    is the 16-bit engine bit for bit, and the planes are really read: one more on every scale byte of the lm_head doubles the
    decode logits bit for bit while the prefill logits and hidden rows stay"""
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
    planes = dev_planes(layers, lm)
    on1 = run(eng, wd, prompts, forced, steps)[0]
    eng.reset()
    eng.set_decode_mxfp4(None, None)
    assert eng.decode_weights is None
    off = run(eng, wd, prompts, forced, steps)[0]
    eng.reset()
    eng.set_decode_mxfp4(*planes)
    on2 = run(eng, wd, prompts, forced, steps)[0]
    ref16, _ = engine(meta, dtype, False)
    r16 = run(ref16, wd, prompts, forced, steps)[0]
    assert on1[1] == on2[1] == outs[1][1] and off[1] == r16[1]
    for j in (2, 3, 4):
        assert torch.equal(on1[j], on2[j]) and torch.equal(on1[j], outs[1][j]), "mxfp4 on -> off -> on changed the result"
        assert torch.equal(off[j], r16[j]), "mxfp4 off is not the 16-bit engine"
    eng.reset()
    eng.set_decode_mxfp4(planes[0], (planes[1][0], planes[1][1] + 1))
    forced_all = [on1[1]]                       # the tokens of the run above, teacher-forced: the sampled ones must not move
    x2 = run(eng, wd, prompts, forced_all, steps)[0]
    log2 = eng.logits.clone()
    eng.reset()
    eng.set_decode_mxfp4(*planes)
    x1 = run(eng, wd, prompts, forced_all, steps)[0]
    assert x1[1] == x2[1] == on1[1] and torch.equal(x1[2], x2[2]) and torch.equal(x1[2], on1[2])
    assert torch.equal(x1[5], x2[5]) and torch.equal(x1[5], on1[5])
    assert torch.isfinite(log2).all() and torch.equal(log2, eng.logits * 2.0) and bool(eng.logits.abs().sum() > 0)


def test_llama_mx4_and_fp8_exclude_each_other(golden):
    """fp8 -> mxfp4 -> fp8 on ONE engine gives the fp8 results bit for bit (no stale graph, planes cleared), the mxfp4 leg in
    between runs other weights; switching one option off while the other is on leaves the other on"""
    _, meta = golden
    dtype, steps = torch.bfloat16, 10
    prompts, forced = prompts_forced(1, steps)
    forced = [forced[0][:4]]
    e8, wd8 = engine_w8(meta, dtype, True)              # (another quantisation of the toy: its own de-quantised prompt embeddings)
    from test_llama_w8_gpu import toy as toy_w8
    _, l8, lm8 = toy_w8(meta, dtype)
    p8 = [[(q.to(DEV), s.to(DEV)) for q, s in pl] for pl in l8], (lm8[0].to(DEV), lm8[1].to(DEV))
    wd4, l4, lm4 = toy(meta, dtype)
    p4 = dev_planes(l4, lm4)
    a = run(e8, wd8, prompts, forced, steps)[0]
    e8.reset()
    e8.set_decode_mxfp4(*p4)
    assert e8.decode_weights == "mxfp4"
    m = run(e8, wd8, prompts, forced, steps)[0]
    e8.disable_decode_fp8()                             # not what is on: nothing changes
    assert e8.decode_weights == "mxfp4"
    e8.reset()
    m2 = run(e8, wd8, prompts, forced, steps)[0]
    e8.reset()
    e8.set_decode_fp8(*p8)
    assert e8.decode_weights == "fp8"
    b = run(e8, wd8, prompts, forced, steps)[0]
    assert a[1] == b[1] and m[1] == m2[1]
    for j in (2, 3, 4):
        assert torch.equal(a[j], b[j]), "fp8 -> mxfp4 -> fp8 changed the fp8 result"
        assert torch.equal(m[j], m2[j])
    assert not torch.equal(a[2], m[2])                  # the middle leg really ran other weights


def test_llama_mx4_refusals_and_own_weights(golden):
    """an fp32 engine refuses; enable_decode_mxfp4 (the engine's own merged weights), decode_weights="mxfp4" and the
    llama_decode_mx4 knob switch it on and give identical outputs; both knobs together are refused; profile_decode reports the
    bytes the MXFP4 token streams.  Records (not a gate) the relative distance of MXFP4 decode from the 16-bit decode of the same
    un-quantised toy weights."""
    from seedstory._lib import SSError
    from seedstory.llama import LlamaEngine
    _, meta = golden
    d = meta["LLAMA"]
    e32, _ = engine(meta, torch.float32, False)
    with pytest.raises(SSError, match="bf16 / fp16"):
        _, layers, lm = toy(meta, torch.bfloat16)
        e32.set_decode_mxfp4(*dev_planes(layers, lm))
    assert e32.decode_weights is None
    # a code plane that is not 16-byte aligned, a plane of the wrong shape, a missing layer: refused, and nothing is switched on
    e16a, _ = engine(meta, torch.bfloat16, False)
    _, layers, lm = toy(meta, torch.bfloat16)
    pl, plm = dev_planes(layers, lm)
    c0 = pl[0][0][0]
    odd = torch.zeros(c0.numel() + 16, dtype=torch.uint8, device=DEV)[8:8 + c0.numel()].view(c0.shape).copy_(c0)
    assert odd.data_ptr() % 16 == 8
    with pytest.raises(SSError, match="16-byte aligned"):
        e16a.set_decode_mxfp4([[(odd, pl[0][0][1])] + pl[0][1:]] + pl[1:], plm)
    with pytest.raises(SSError, match="set_decode_mxfp4"):
        e16a.set_decode_mxfp4([[(c0[:, :-1], pl[0][0][1])] + pl[0][1:]] + pl[1:], plm)
    with pytest.raises(SSError, match="layers given"):
        e16a.set_decode_mxfp4(pl[:-1], plm)
    assert e16a.decode_weights is None
    wd = synth.llama_weights(11, d["hidden"], d["n_heads"], d["n_layers"], d["inter"], d["vocab"], dtype=torch.bfloat16)
    kw = dict(hidden=d["hidden"], n_heads=d["n_heads"], n_layers=d["n_layers"], inter=d["inter"], vocab=d["vocab"],
              dtype=torch.bfloat16, device=DEV, cache_cap=256, max_new=128, max_prefill_rows=64, img_ids=_img_ids(meta))
    with pytest.raises(ValueError):
        LlamaEngine(wd, decode_weights="int4", **kw)
    e16 = LlamaEngine(wd, **kw)
    assert e16.decode_weights is None
    e4 = LlamaEngine(wd, decode_weights="mxfp4", **kw)
    ee = LlamaEngine(wd, **kw)
    ee.enable_decode_mxfp4()
    with knobs(llama_decode_mx4=1):
        ek = LlamaEngine(wd, **kw)
        e32k = LlamaEngine(wd, **dict(kw, dtype=torch.float32))     # the knob leaves fp32 engines alone
        eoff = LlamaEngine(wd, decode_weights="16bit", **kw)        # and an explicit argument wins
        with knobs(llama_decode_w8=1):
            with pytest.raises(ValueError, match="llama_decode_w8.*llama_decode_mx4"):
                LlamaEngine(wd, **kw)
            assert LlamaEngine(wd, decode_weights="mxfp4", **kw).decode_weights == "mxfp4"
    assert e4.decode_weights == ee.decode_weights == ek.decode_weights == "mxfp4"
    assert e32k.decode_weights is None and eoff.decode_weights is None
    # the engine's planes are the reference quantiser's, bit for bit
    rc, rs, _ = R.quantize_packed(wd["lm_head.weight"])
    assert torch.equal(e4._w8[-2].cpu(), rc) and torch.equal(e4._w8[-1].cpu(), rs)
    prompts, forced = prompts_forced(1, 8)
    outs = [run(e, wd, prompts, forced, 8)[0] for e in (e16, e4, ee, ek)]
    assert torch.equal(outs[1][2], outs[2][2]) and torch.equal(outs[1][2], outs[3][2])
    assert torch.equal(e4.logits, ee.logits) and torch.equal(e4.logits, ek.logits)
    r = rel(outs[1][2], outs[0][2])
    rl = rel(e4.logits, e16.logits)
    print("mxfp4 decode (round to nearest, blocks of 32) vs 16-bit decode, toy engine: hidden rows rel %.3g, last logits rel %.3g" % (r, rl))
    assert math.isfinite(r) and r > 0 and math.isfinite(rl) and rl > 0          # a record, not a gate
    H, I, L, V = d["hidden"], d["inter"], d["n_layers"], d["vocab"]
    p4, p16 = e4.profile_decode(2), e16.profile_decode(2)
    w_all, w_down = L * (4 * H * H + 2 * H * I) + V * H, L * H * I
    assert p16["gemv_bytes"] == w_all * 2 and p16["gemv_down_bytes"] == w_down * 2
    assert p4["gemv_bytes"] == w_all // 2 + w_all // 32 and p4["gemv_down_bytes"] == w_down // 2 + w_down // 32
    assert p4["gemv_launches"] == p16["gemv_launches"] and p4["token_ms"] > 0

"""LlamaEngine with the fp8 (e4m3) KV shadow cache for decode attention (kv_cache="fp8", ss_llama_set_kv8).

The toy LLaMA of tests/golden/hotpath_tiny.json.  (a) the shadow is, bit for bit, tests/kv8_ref.py of the 16-bit cache: the
prompt rows the engine quantises lazily AND the rows the fused decode kernel appends.  (b) a decode token over the shadow equals
a 16-bit engine's token over the de-quantised cache (exact in the model dtype): the same function with the same rounding points
apart from fp32 summation order, held to the tolerance the suite already uses for that situation (TOL of test_llama_w8_gpu.py).
(c) every path that rewrites 16-bit rows leaves a consistent shadow."""
import math

import pytest
import torch

import kv8_ref
import synth
from test_engine_gpu import DEV, rel
from test_kernel_edges_gpu import knobs
from test_llama_w8_gpu import TOL, engine, prompts_forced

pytestmark = pytest.mark.gpu
D16 = [torch.bfloat16, torch.float16]
STEPS = 10


def assert_shadow(eng, slots, what, upto=None):
    """shadow rows [0, kv_len) of every slot and layer == kv8_ref of the 16-bit rows, codes and scales, bit for bit"""
    for b in slots:
        eng.select(b)
        kv = eng.lengths()[0] if upto is None else upto
        assert kv > 0
        for name, cache, codes, scale in (("K", eng.k_cache, eng.k_codes, eng.k_scale), ("V", eng.v_cache, eng.v_codes, eng.v_scale)):
            c, s, _ = kv8_ref.quantize(cache[:, :, :kv].cpu())
            got_c, got_s = codes[:, :, :kv].cpu(), scale[:, :, :kv].cpu()
            bad = (got_c != c).any(-1) | (got_s.view(torch.int32) != s.view(torch.int32))
            assert not bad.any(), "%s: slot %d %s shadow rows differ from the quantiser at (layer, head, row) %s of %d rows" % (
                what, b, name, bad.nonzero()[:4].tolist(), kv)


def prefill_and_decode(eng, wd, prompts, forced, steps=STEPS):
    S = len(prompts)
    emb = wd["model.embed_tokens.weight"]
    for b in range(S):
        eng.select(b).prefill(emb[prompts[b]])
    if S == 1:
        return [eng.select(0).generate(steps, last_prompt_id=int(prompts[0][-1]), forced=forced[0])]
    return eng.generate_batch(steps, [int(p[-1]) for p in prompts], forced=forced)


def kv8_engine(meta, dtype, n_seq=1, w8=False, **kw):
    eng, wd = engine(meta, dtype, w8, n_seq=n_seq, kv_cache="fp8", **kw)
    assert eng.kv_cache == "fp8"
    return eng, wd


# ---- (a) --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D16, ids=["bf16", "fp16"])
@pytest.mark.parametrize("n_seq", [1, 3])
def test_kv8_shadow_consistency(golden, n_seq, dtype):
    _, meta = golden
    prompts, forced = prompts_forced(n_seq, STEPS)
    if n_seq > 1:
        forced[-1] = forced[-1][:2] + [2]            # EOS at its third token: the slot stops early
    eng, wd = kv8_engine(meta, dtype, n_seq)
    ns = prefill_and_decode(eng, wd, prompts, forced)
    for b in range(n_seq):
        want = 3 if (n_seq > 1 and b == n_seq - 1) else STEPS
        assert ns[b] == want and eng.select(b).lengths()[0] == prompts[b].numel() + want - 1
    assert_shadow(eng, range(n_seq), "prefill + %d decode tokens" % STEPS)
    # re-quantising is idempotent: the rows the fused kernel appended come out of the quantiser bit-identical
    eng.select(0)
    kv = eng.lengths()[0]
    before = [t[:, :, :kv].clone() for t in (eng.k_codes, eng.v_codes, eng.k_scale, eng.v_scale)]
    eng.kv_invalidate(0)
    assert eng.generate(2, last_prompt_id=forced[0][-1], forced=[5, 6]) == 2
    after = [t[:, :, :kv] for t in (eng.k_codes, eng.v_codes, eng.k_scale, eng.v_scale)]
    for x, y in zip(before, after):
        assert torch.equal(x.view(torch.uint8), y.contiguous().view(torch.uint8)), "kv_invalidate(0) + generate changed shadow rows"
    assert_shadow(eng, range(n_seq), "after kv_invalidate(0) + 2 tokens")


# ---- (b) --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", D16, ids=["bf16", "fp16"])
def test_kv8_decode_parity_with_16bit_over_dequantised_cache(golden, dtype):
    _, meta = golden
    prompts, forced = prompts_forced(1, STEPS)
    A, wd = kv8_engine(meta, dtype)
    assert prefill_and_decode(A, wd, prompts, forced) == [STEPS]
    L0 = prompts[0].numel()
    a_hid, a_k, a_v = A.hidden_rows[:STEPS - 1].clone(), A.k_cache.clone(), A.v_cache.clone()
    for k in (0, 4, 8):
        B, _ = engine(meta, dtype, False)
        n = L0 + k
        kd, vd = (kv8_ref.quantize(t[:, :, :n].cpu())[2].to(DEV) for t in (a_k, a_v))
        B.load_past_key_values(tuple((kd[l][None], vd[l][None]) for l in range(kd.shape[0])), pos=n)
        assert B.generate(2, last_prompt_id=3, forced=[forced[0][k], 7]) == 2
        for name, got, want in (("hidden row", B.hidden_rows[0], a_hid[k]), ("K row", B.k_cache[:, :, n], a_k[:, :, n]),
                                ("V row", B.v_cache[:, :, n], a_v[:, :, n])):
            r = rel(got, want)
            print("kv8 vs 16-bit over the de-quantised cache, %s token %d %s: rel %.3g" % (dtype, k, name, r))
            assert math.isfinite(r) and r < TOL[dtype], (k, name, r)


# ---- (c) --------------------------------------------------------------------------------------------------------------------
def test_kv8_graph_and_eager_paths(golden):
    _, meta = golden
    dtype = torch.bfloat16
    prompts, forced = prompts_forced(1, STEPS)
    outs = {}
    for use_graph in (1, 0):
        with knobs(llama_graph=use_graph):
            eng, wd = kv8_engine(meta, dtype)
            assert prefill_and_decode(eng, wd, prompts, forced) == [STEPS]
            assert_shadow(eng, [0], "llama_graph=%d" % use_graph)
            outs[use_graph] = (eng.hidden_rows[:STEPS - 1].clone(), eng.k_codes.clone(), eng.k_scale.clone())
    for x, y in zip(outs[1], outs[0]):
        assert torch.equal(x, y), "captured and eager decode differ"
    kv = eng.lengths()[0]
    p = eng.profile_decode(2)           # eager, greedy
    assert p["attn_ms"] > 0 and eng.lengths()[0] == kv + 2
    assert_shadow(eng, [0], "profile_decode")


def test_kv8_truncate_gather_load(golden):
    _, meta = golden
    dtype = torch.bfloat16
    prompts, forced = prompts_forced(1, STEPS)
    eng, wd = kv8_engine(meta, dtype)
    emb = wd["model.embed_tokens.weight"]
    assert prefill_and_decode(eng, wd, prompts, forced) == [STEPS]
    kv, pos = eng.lengths()
    # set_lengths truncation, then other rows in the place of the dropped ones (prefill writes the 16-bit cache only)
    eng.set_lengths(kv - 5, pos - 5)
    eng.prefill(emb[synth.randint(77, (3,), 3, 250)])
    assert eng.generate(3, last_prompt_id=9, forced=[11, 12, 13]) == 3
    assert eng.lengths()[0] == kv - 5 + 3 + 2
    assert_shadow(eng, [0], "set_lengths truncation + prefill + decode")
    # the sink gather moves rows
    kv = eng.lengths()[0]
    keep = [0, 1, 2] + list(range(9, kv, 2))
    eng.kv_gather(keep)
    assert eng.generate(2, last_prompt_id=9, forced=[14, 15]) == 2 and eng.lengths()[0] == len(keep) + 1
    assert_shadow(eng, [0], "kv_gather + decode")
    # a foreign cache loaded over rows that were already synced
    n = 21
    g = torch.Generator().manual_seed(31)
    past = tuple((torch.randn(1, eng.n_heads, n, eng.hd, generator=g).to(dtype).to(DEV), torch.randn(1, eng.n_heads, n, eng.hd, generator=g).to(dtype).to(DEV))
                 for _ in range(eng.n_layers))
    eng.load_past_key_values(past)
    assert eng.generate(2, last_prompt_id=9, forced=[16, 17]) == 2 and eng.lengths()[0] == n + 1
    assert torch.equal(eng.k_cache[1, :, :n], past[1][0][0])
    assert_shadow(eng, [0], "load_past_key_values + decode")
    # rows written through the views: the caller owes a kv_invalidate
    eng.k_cache[:, :, 4:9] *= 2.0
    eng.kv_invalidate(4)
    assert eng.generate(2, last_prompt_id=9, forced=[18, 19]) == 2
    assert_shadow(eng, [0], "view write + kv_invalidate + decode")


def test_kv8_with_fp8_weights_and_sampling(golden):
    _, meta = golden
    dtype = torch.bfloat16
    prompts, forced = prompts_forced(3, STEPS)
    eng, wd = kv8_engine(meta, dtype, 3, w8=True)
    assert eng.decode_weights == "fp8"
    assert prefill_and_decode(eng, wd, prompts, forced) == [STEPS] * 3
    assert_shadow(eng, range(3), "fp8 weights + fp8 KV")
    for b in range(3):
        assert torch.isfinite(eng.select(b).hidden_rows[:STEPS - 1].float()).all()
    eng, wd = kv8_engine(meta, dtype, 3)
    eng.set_sampling(temperature=0.8, top_k=20, top_p=0.9, seed=3)
    ns = prefill_and_decode(eng, wd, prompts, [f[:2] for f in forced])
    assert all(1 <= n <= STEPS for n in ns)
    assert_shadow(eng, range(3), "sampling + fp8 KV")
    for b in range(3):
        assert torch.isfinite(eng.select(b).hidden_rows[:max(ns[b] - 1, 0)].float()).all()


def test_kv8_off_is_the_16bit_engine_and_refusals(golden):
    from seedstory._lib import SSError
    _, meta = golden
    dtype = torch.bfloat16
    prompts, forced = prompts_forced(1, 12)
    forced = [forced[0][:4]]                        # four forced tokens, then greedy
    eng, wd = kv8_engine(meta, dtype)
    n_on = prefill_and_decode(eng, wd, prompts, forced, 12)
    on = (eng.gen_ids[:n_on[0]].tolist(), eng.hidden_rows[:n_on[0] - 1].clone())
    eng.disable_kv_fp8()
    assert eng.kv_cache is None
    with pytest.raises(SSError):
        eng.k_codes
    eng.reset()
    n_off = prefill_and_decode(eng, wd, prompts, forced, 12)
    ref, _ = engine(meta, dtype, False)
    assert ref.kv_cache is None
    n_ref = prefill_and_decode(ref, wd, prompts, forced, 12)
    assert n_off == n_ref and eng.gen_ids[:n_off[0]].tolist() == ref.gen_ids[:n_ref[0]].tolist()
    assert torch.equal(eng.hidden_rows[:n_off[0] - 1], ref.hidden_rows[:n_ref[0] - 1]), "kv_cache off is not the 16-bit engine"
    assert torch.equal(eng.k_cache, ref.k_cache) and torch.equal(eng.logits, ref.logits)
    # on again: new planes, a fresh shadow, the same tokens as the first time
    eng.enable_kv_fp8()
    eng.reset()
    n_on2 = prefill_and_decode(eng, wd, prompts, forced, 12)
    assert n_on2 == n_on and eng.gen_ids[:n_on[0]].tolist() == on[0] and torch.equal(eng.hidden_rows[:n_on[0] - 1], on[1])
    assert_shadow(eng, [0], "off -> on")
    # the knob is the default of kv_cache; fp32 engines ignore the knob and refuse the explicit request
    with knobs(llama_kv8=1):
        ek, _ = engine(meta, dtype, False)
        e32, _ = engine(meta, torch.float32, False)
        e16, _ = engine(meta, dtype, False, kv_cache="16bit")
    assert ek.kv_cache == "fp8" and e32.kv_cache is None and e16.kv_cache is None
    with pytest.raises(SSError, match="bf16 or fp16"):
        engine(meta, torch.float32, False, kv_cache="fp8")
    with pytest.raises(ValueError):
        engine(meta, dtype, False, kv_cache="int4")

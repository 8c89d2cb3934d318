"""Attention-map capture, the parts that need no GPU: the C ABI surface, the merge rule on synthetic buffers, the fixture recipe."""
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "attn_maps_tiny.safetensors")
NEW_SYMBOLS = ("ss_attn_scores", "ss_llama_set_attn_capture")


def same(a, b):
    """torch.equal with NaNs treated as equal"""
    return a.shape == b.shape and a.dtype == b.dtype and bool(((a == b) | (torch.isnan(a) & torch.isnan(b))).all())


def merge_attn_weights(steps):
    """the reference's merge (models.py:164-173), restated: pad the running map with one NaN column per step, then concatenate
    the step's rows along the query axis"""
    merged = steps[0]
    for a in steps[1:]:
        merged = F.pad(merged, (0, 1), "constant", float("nan"))
        merged = torch.cat([merged, a], dim=1)
    return merged


def test_capture_symbols_declared_bound_and_exported():
    from seedstory import _lib
    hdr = open(os.path.join(ROOT, "include", "seedstory_hip.h")).read()
    declared = set(re.findall(r"\b(ss_[a-z0-9_]+)\s*\(", hdr))
    lib = _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and name in _lib.PROTOTYPES and hasattr(lib, name), name
    assert lib.ss_abi_version() == 1        # additive: the ABI version stays


def test_capture_entry_points_fail_loudly_without_gpu():
    from seedstory import _lib, ops
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(_lib.SSError):
        ops.attn_scores(torch.zeros(2, 128), torch.zeros(2, 128), torch.zeros(2, 2))


@pytest.mark.parametrize("kv0,fed0,fed", [(0, 7, 7), (0, 7, 19), (0, 1, 6), (5, 1, 4), (11, 9, 12)])
def test_step_views_merge_to_the_buffer_slice(kv0, fed0, fed):
    """`GenerateOutput.attentions` are views of one NaN-filled buffer; the reference's pad-and-concatenate merge over them is the
    slice of the buffer that ContinuousLVLM.generate returns as `attn_weights`."""
    from src.models_clm.modeling_llama_xformer import attention_step_views
    L, rows, cols = 2, fed + 3, kv0 + fed + 3
    g = torch.Generator().manual_seed(kv0 * 100 + fed)
    maps = torch.full((L, rows, cols), float("nan"))
    for r in range(fed):                      # what the engine leaves: row r real up to its call's key count
        width = kv0 + fed0 if r < fed0 else kv0 + r + 1
        maps[:, r, :width] = torch.randn(L, width, generator=g)
    steps = attention_step_views(maps, kv0, fed0, fed)
    assert len(steps) == 1 + fed - fed0 and all(len(s) == L for s in steps)
    assert steps[0][0].shape == (1, fed0, kv0 + fed0)
    for j in range(1, len(steps)):
        assert steps[j][1].shape == (1, 1, kv0 + fed0 + j)
        assert steps[j][1].data_ptr() == maps[1, fed0 + j - 1].data_ptr()          # a view, not a copy
    for l in range(L):
        merged = merge_attn_weights([s[l] for s in steps])
        assert merged.shape == (1, fed, kv0 + fed)
        assert same(merged, maps[l, :fed, :kv0 + fed].unsqueeze(0))
        assert not torch.isnan(merged[0, -1]).any() and (fed == fed0 or torch.isnan(merged[0, 0, kv0 + fed0:]).all())


def test_fixture_holds_the_three_calls_in_three_dtypes():
    from safetensors.torch import load_file
    g = load_file(FIXTURE)
    assert len(g) == 18 and os.path.getsize(FIXTURE) < 64 * 1024
    for tag, dt in (("f32", torch.float32), ("bf16", torch.bfloat16), ("f16", torch.float16)):
        lo = torch.finfo(dt).min
        for l in range(2):
            for call, (q, kv) in (("prefill", (37, 37)), ("cont", (9, 46)), ("decode", (1, 47))):
                a = g["%s.%s.%d" % (tag, call, l)]
                assert a.shape == (q, kv) and a.dtype == dt
                masked = ~torch.ones(q, kv, dtype=torch.bool).tril(diagonal=kv - q)
                if q > 1:       # the additive mask rounds to finfo.min exactly for these small scores
                    assert bool((a[masked] == lo).all()) and bool((a[~masked] > lo / 2).all())
                else:           # the one-row call: finite everywhere, the 16-bit rows within rounding of the fp32 one
                    ref = g["f32.decode.%d" % l].double()
                    assert bool(((a.double() - ref).abs() < 0.05).all()) and bool(torch.isfinite(a).all())


def test_fixture_decode_row_has_plus_one_on_its_last_column_only():
    """The fp32 decode rows of the fixture against the oracle's own q . k / sqrt(hd) of that call: equal within fp32 rounding
    once 1 is added on the last column, and on no other."""
    import math
    import seedstory_oracle as O
    import synth
    from safetensors.torch import load_file
    g = load_file(FIXTURE)
    dims = O.LlamaDims(256, 2, 2, 512, 320)
    wd = synth.llama_weights(11, 256, 2, 2, 512, 320, dtype=torch.float32)
    emb = wd["model.embed_tokens.weight"]
    calls, orig = [], O.attention_bottom_right_causal

    def record(q, k, v):
        calls.append((q[0, 0].clone(), k[0, 0].clone()))
        return orig(q, k, v)

    O.attention_bottom_right_causal = record
    try:
        past, pos = None, 0
        for seed, rows in ((5, 37), (6, 9), (7, 1)):
            ids = synth.randint(seed, (1, rows), 3, 250)
            _, _, past = O.llama_forward(wd, dims, emb[ids], torch.arange(pos, pos + rows).unsqueeze(0), past)
            pos += rows
    finally:
        O.attention_bottom_right_causal = orig
    for l in range(2):
        q, k = calls[4 + l]                                 # the third call's layers
        s = (q.double() @ k.double().t())[0] / math.sqrt(128.0)
        row = g["f32.decode.%d" % l][0].double()
        assert abs(float(row[46] - (s[46] + 1.0))) < 1e-5
        assert float((row[:46] - s[:46]).abs().max()) < 1e-5


def test_fixture_regenerates_from_the_recipe(tmp_path):
    """tools/make_golden_attn_maps.py, run on the real reference classes, reproduces the committed fixture tensor for tensor.
    In a process of its own: importing the reference makes ITS `src` package win."""
    import ref_shims
    if not ref_shims.reference_available():
        pytest.skip("reference tree not present")
    from safetensors.torch import load_file
    out = str(tmp_path / "maps.safetensors")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_golden_attn_maps.py"), "--out", out], check=True,
                   capture_output=True, timeout=600)
    new, old = load_file(out), load_file(FIXTURE)
    assert sorted(new) == sorted(old)
    for k in old:
        assert new[k].dtype == old[k].dtype and torch.equal(new[k], old[k]), k

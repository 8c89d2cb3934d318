"""The two operators of prompt-lookup speculative decoding on the GPU (tests/kernel_check.py, tests/spec_ref.py).

``ops.attn_decode_spec``: every output element inside the a-priori bound of ``kernel_check.attention_bound`` against an fp64
reference with the mask ``causal_allow(A, L + A)`` and the new rows rotated by the bit-exact ``rope_exact``; the appended cache rows
bit-equal to that mirror and every other cache byte, every output row >= A and every guard untouched (poisoned cache tail,
``GuardedOut``); a selector probe that shows row r sees key L + r and not key L + r + 1.
``ops.spec_draft``: equal to ``spec_ref.draft`` on the grid that pins ``spec_ref.draft`` to transformers on the CPU.
"""
import math

import pytest
import torch

import kernel_check as KC
import spec_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, FH, F32 = torch.bfloat16, torch.float16, torch.float32
dname = lambda d: KC.NAME[d]
H = 3
NS = 16                 # decode_nsplit at one slot: the split count ss_attn_decode_spec runs with
CAP = 520
# (L, R, A): L on both sides of the split count (empty splits, one key per split), R = 1, 2, 3, 5, 8 (the 2-, 4- and 8-row
# instantiations, full and partly used), one case with A < R, L + R = cap, and L + R > cap with the overflowing rows inactive
CASES = [(L, R, R) for L in (0, 1, NS - 1, NS, NS + 1, 500) for R in (1, 2, 3, 5, 8)]
CASES += [(NS + 1, 5, 3), (40, 8, 1), (CAP - 8, 8, 8), (CAP - 3, 3, 3), (CAP - 5, 8, 5), (CAP - 1, 2, 1)]


@pytest.fixture(scope="module")
def ops():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU (no CPU fallback exists)")
    from seedstory import ops as _ops
    return _ops


def i32(v):
    return torch.tensor([v], dtype=torch.int32, device=DEV)


def guarded_planes(kplane, vplane, dtype):
    """[H, cap, hd] planes inside guarded allocations (the payload is the plane)"""
    out = []
    for pl in (kplane, vplane):
        g = KC.GuardedOut(pl.shape[0] * pl.shape[1], pl.shape[2], dtype, device=DEV)
        g.view(*pl.shape).copy_(pl.to(DEV))
        out.append(g)
    return out


def run(ops, qkv, kc, vc, cos, sin, L, P, A, dtype):
    """-> (out payload [R, E] with untouched mask, k plane, v plane) after one launch over guarded, partly poisoned buffers"""
    R, hd = qkv.shape[0], kc.shape[2]
    gk, gv = guarded_planes(kc, vc, dtype)
    go = KC.GuardedOut(R, H * hd, dtype, device=DEV)
    ops.attn_decode_spec(qkv.to(DEV), gk.view(*kc.shape), gv.view(*vc.shape), cos.to(DEV), sin.to(DEV), i32(L), i32(P), i32(A),
                         out=go.view(R, H * hd))
    y = go.check("out guards", payload=False)
    k1 = gk.check("k plane guards", payload=False).view(*kc.shape)
    v1 = gv.check("v plane guards", payload=False).view(*vc.shape)
    return y, go.untouched(y), k1, v1


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


@pytest.mark.parametrize("dtype", [BF, FH, F32], ids=dname)
@pytest.mark.parametrize("hd", [64, 128])
def test_attn_decode_spec_bound_append_and_untouched(ops, hd, dtype):
    E = H * hd
    scale = 1.0 / math.sqrt(hd)
    cos, sin = KC.rope_tables(hd, CAP + 16, dtype)
    for L, R, A in CASES:
        what = "attn_decode_spec hd %d %s L %d R %d A %d" % (hd, dname(dtype), L, R, A)
        g = torch.Generator().manual_seed(hd * 7 + L * 13 + R)
        P = L + 3                           # the RoPE position is its own argument
        qkv = torch.randn(R, 3 * E, generator=g).to(dtype)
        kc = torch.randn(H, CAP, hd, generator=g).to(dtype)
        vc = torch.randn(H, CAP, hd, generator=g).to(dtype)
        KC.poison_(kc[:, L:])
        KC.poison_(vc[:, L:])
        y, untouched, k1, v1 = run(ops, qkv, kc, vc, cos, sin, L, P, A, dtype)
        # the mirror: rows rotated bit-exactly, appended at L .. L + A - 1
        pos = torch.arange(P, P + R)
        q_rot = KC.rope_exact(qkv[:, :E].reshape(R, H, hd), cos, sin, pos)
        k_rot = KC.rope_exact(qkv[:, E:2 * E].reshape(R, H, hd), cos, sin, pos)
        v_new = qkv[:, 2 * E:].reshape(R, H, hd)
        ke, ve = kc.clone(), vc.clone()
        ke[:, L:L + A] = k_rot[:A].transpose(0, 1)
        ve[:, L:L + A] = v_new[:A].transpose(0, 1)
        assert torch.equal(bits(k1), bits(ke)), what + ": k plane (appended rows bit-equal to the mirror, every other byte untouched)"
        assert torch.equal(bits(v1), bits(ve)), what + ": v plane"
        # rows >= A are not written, rows < A completely
        assert bool(untouched[A:].all()) and not bool(untouched[:A].any()), what + ": output rows written"
        ref, tol = KC.attention_bound(q_rot[:A].transpose(0, 1), ke[:, :L + A], ve[:, :L + A], scale, KC.causal_allow(A, L + A), dtype)
        KC.check(y[:A].view(A, H, hd).transpose(0, 1), ref, tol, what, family="attn_decode_spec", dtype=dtype)


@pytest.mark.parametrize("dtype", [BF, FH, F32], ids=dname)
@pytest.mark.parametrize("hd", [64, 128])
def test_attn_decode_spec_selector(ops, hd, dtype):
    """scores 128 j / sqrt(hd) * 16 apart: every row selects the LAST key it may see, bit for bit — row r returns value L + r,
    so it saw key L + r and did not see key L + r + 1 (identity RoPE tables: the probe's vectors stay exact)"""
    E = H * hd
    cos = torch.ones(CAP + 16, hd).to(dtype)
    sin = torch.zeros(CAP + 16, hd).to(dtype)
    for L, R, A in CASES:
        what = "attn_decode_spec selector hd %d %s L %d R %d A %d" % (hd, dname(dtype), L, R, A)
        Lk = L + R
        qs, ks, vs = KC.attention_selector(R, Lk, hd, dtype, seed=L + R, H=H, kscale=16.0)
        kc = torch.zeros(H, CAP, hd).to(dtype)
        vc = torch.zeros(H, CAP, hd).to(dtype)
        KC.poison_(kc[:, L:])
        KC.poison_(vc[:, L:])
        kc[:, :L], vc[:, :L] = ks[:, :L], vs[:, :L]
        qkv = torch.cat([qs.transpose(0, 1).reshape(R, E), ks[:, L:].transpose(0, 1).reshape(R, E),
                         vs[:, L:].transpose(0, 1).reshape(R, E)], 1).contiguous()
        y, untouched, _, _ = run(ops, qkv, kc, vc, cos, sin, L, 0, A, dtype)
        exp = KC.attention_selector_expected(vs, R, Lk, True).transpose(0, 1).reshape(R, E)
        assert torch.equal(bits(y[:A]), bits(exp[:A])), what
        assert bool(untouched[A:].all()), what + ": rows >= A written"


def test_spec_draft_equals_reference(ops):
    for seq, g, k, stops in spec_ref.draft_grid():
        h = torch.tensor(seq, dtype=torch.int32, device=DEV)
        assert ops.spec_draft(h, g, k, stops) == spec_ref.draft(seq, g, k, stops), (seq, g, k, stops)


def test_spec_draft_edges(ops):
    def both(seq, g, k, stops=()):
        got = ops.spec_draft(torch.tensor(seq, dtype=torch.int32, device=DEV), g, k, stops)
        assert got == spec_ref.draft(seq, g, k, stops), (len(seq), g, k, stops)
        return got

    assert both([7], 2, 3) == []                                    # history length 1: no n-gram to match
    cap = 2048 + 512                                                # a history at the engine's hist_cap (cache_cap + max_new)
    rng = torch.Generator().manual_seed(5)
    long = torch.randint(0, 50, (cap,), generator=rng).tolist()
    long[-3:] = [61, 62, 63]
    long[1500:1503] = [61, 62, 63]
    long[1900:1903] = [61, 62, 63]                                   # two matches beyond one block's first sweep: the leftmost wins
    assert both(long, 3, 7) == long[1503:1510]
    assert both([4, 5, 6, 9, 4, 5], 2, 5) == [6, 9, 4, 5]          # the continuation runs into the end
    assert both([4, 5, 6, 4, 5], 8, 7) == [6, 4, 5]                # n-gram cap above len - 1

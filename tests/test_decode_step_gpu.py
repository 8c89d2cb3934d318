"""Decode attention as the engine launches it: ``ops.attn_decode_step`` / ``ops.attn_decode_kv8_step`` (ss_attn_decode_step,
ss_attn_decode_kv8_step) run attn_decode_kernel / attn_decode_kv8_kernel in their FUSED, BATCHED mode — q and the new k rotated in
the kernel, the new K / V row stored by one key group of one split and attended from registers, nb sequences on blockIdx.z with
per-sequence state words, planes, partial records and output rows, the done flag.  (tests/test_kernel_edges_gpu.py and
tests/test_kv8_kernels_gpu.py hold the plain, one-sequence mode of the same kernels.)

Every launch runs over the buffers of ``KC.decode_step_pack``: planes, code planes and scale planes inside guarded allocations,
16 poisoned rows between consecutive sequences, rows >= kv_len poisoned (codes 0x7f, NaN scales), an int32 state of 8 words per
sequence with kv_len, pos, done at words 0, 1, 3 and large garbage elsewhere, pos = kv_len + 3.  ``KC.decode_step_failures`` holds
the assertions (tests/test_kernel_check_cpu.py runs them over a simulated kernel on the same cases, and over nine mutants):
every output element inside ``KC.attention_bound`` over keys [0, kv_len] of an fp64 reference with the new row rotated by the
bit-exact ``rope_exact`` (shadow: de-quantised old keys, exact new key); the appended rows bit-equal to the mirror (shadow: to
tests/kv8_ref.py of the rotated row); every other byte of every buffer, the finished sequences' output rows and the state untouched.

Cases (``KC.DECODE_STEP_CASES``, hd 64 / 128, cap 640, 4 heads): n_old in {0, 1, ns - 2, ns - 1, ns, ns + 1, 63, 64, 500, 511,
512, 600, cap - 1, cap} at one sequence under 16 (default), 4 and 32 splits, and on the live sequences of batches of 2, 3, 4 and
8 (8, 8, 4, 4 splits), each batch with one finished sequence.

Worst error / bound, measured on an MI355X against the fp64 reference (test_zz_worst_ratios prints this table; a ratio above 1
fails the case that produced it):

  attn_decode step       bf16  worst error / bound = 0.319
  attn_decode step       fp16  worst error / bound = 0.301
  attn_decode step       fp32  worst error / bound = 0.004
  attn_decode_kv8 step   bf16  worst error / bound = 0.323
  attn_decode_kv8 step   fp16  worst error / bound = 0.304
"""
import types

import pytest
import torch

import kernel_check as KC
from test_kernel_edges_gpu import DEV, D16, F32, dev, dname, guarded, knobs, ops  # noqa: F401  (ops: the fixture)

pytestmark = pytest.mark.gpu

H, CAP = KC.DECODE_HEADS, KC.DECODE_STEP_CAP
WORDS = dict(kv_len_word=KC.ST_KV_LEN, pos_word=KC.ST_POS, done_word=KC.ST_DONE)
PARAMS = [(hd, dtype, False) for hd in (64, 128) for dtype in D16 + [F32]] + [(hd, dtype, True) for hd in (64, 128) for dtype in D16]
pid = lambda p: "%s%d-%s" % ("kv8-" if p[2] else "", p[0], dname(p[1]))


def identity_tables(hd, dtype):
    return torch.ones(CAP + 16, hd).to(dtype), torch.zeros(CAP + 16, hd).to(dtype)


def guarded_bytes(t):
    """a uint8 CPU tensor inside a guarded device allocation -> (guard, its uint8 view)"""
    g = KC.GuardedBytes(t.numel(), device=DEV)
    assert t.numel() % 4 == 0
    v = g.view(t.numel() // 4).view(torch.uint8)
    v.copy_(t.to(DEV))
    return g, v


def launch(ops, inp, cos_d, sin_d, what):
    """the buffers of KC.decode_step_pack inside guarded device allocations, ONE launch, every guard checked
    -> the `got` of KC.decode_step_failures (on the CPU)"""
    nb, E, dtype, stride = inp.nb, inp.H * inp.hd, inp.dtype, inp.cache_stride
    gk, gv, go = guarded(nb, stride, dtype), guarded(nb, stride, dtype), guarded(nb, E, dtype)
    gk.view(nb * stride).copy_(inp.kflat.to(DEV))
    gv.view(nb * stride).copy_(inp.vflat.to(DEV))
    state = dev(inp.state)
    kw = dict(WORDS, cache_stride=stride, out=go.view(nb, E))
    if inp.shadow:
        (gkq, kq), (gvq, vq) = guarded_bytes(inp.kq), guarded_bytes(inp.vq)
        gks, gvs = guarded(1, inp.ks.numel(), F32), guarded(1, inp.vs.numel(), F32)
        gks.view(inp.ks.numel()).copy_(inp.ks.to(DEV))
        gvs.view(inp.vs.numel()).copy_(inp.vs.to(DEV))
        ops.attn_decode_kv8_step(dev(inp.qkv), gk.view(nb * stride), gv.view(nb * stride), kq, vq, gks.view(inp.ks.numel()),
                                 gvs.view(inp.vs.numel()), cos_d, sin_d, state, inp.H, inp.cap, **kw)
    else:
        ops.attn_decode_step(dev(inp.qkv), gk.view(nb * stride), gv.view(nb * stride), cos_d, sin_d, state, inp.H, inp.cap, **kw)
    y = go.check(what + ": out guards", payload=False)
    got = types.SimpleNamespace(out=y, written=~go.untouched(y), state=state.cpu(),
                                kflat=gk.check(what + ": k plane guards", payload=False).reshape(-1),
                                vflat=gv.check(what + ": v plane guards", payload=False).reshape(-1))
    if inp.shadow:
        got.kq, got.vq = gkq.bytes(what + ": k code guards"), gvq.bytes(what + ": v code guards")
        got.ks = gks.check(what + ": k scale guards", payload=False).reshape(-1)
        got.vs = gvs.check(what + ": v scale guards", payload=False).reshape(-1)
    return got


def case_name(prefix, param, case):
    return "%s hd %d %s nb %d nsplit %d n_old %s" % (prefix, param[0], dname(param[1]), case[0], case[2], list(case[3]))


@pytest.mark.parametrize("param", PARAMS, ids=pid)
def test_decode_step_bound_append_untouched(ops, param):
    """every case of KC.DECODE_STEP_CASES, 16-bit / fp32 planes and the shadow: all assertions of KC.decode_step_failures"""
    hd, dtype, shadow = param
    cos, sin = KC.rope_tables(hd, CAP + 16, dtype)
    cos_d, sin_d = dev(cos), dev(sin)
    for case in KC.DECODE_STEP_CASES:
        what = case_name("attn_decode_kv8_step" if shadow else "attn_decode_step", param, case)
        inp = KC.decode_step_inputs(case, hd, dtype, shadow=shadow)
        with knobs(attn_decode_nsplit=case[1]):
            got = launch(ops, inp, cos_d, sin_d, what)
        exp = KC.decode_step_expect(inp.qkv, inp.kc, inp.vc, cos, sin, inp.kv_lens, inp.pos, inp.done, dtype, shadow)
        fails = KC.decode_step_failures(inp, exp, got, what)
        assert not fails, "\n".join("[%s] %s" % f for f in fails)


@pytest.mark.parametrize("dtype", D16 + [F32], ids=dname)
@pytest.mark.parametrize("hd", [64, 128])
def test_decode_step_equals_two_launches(ops, hd, dtype):
    """The fused launch against ops.rope_kv_append followed by ops.attn_decode over n_old + 1 keys, BIT FOR BIT, per live sequence
    and with attn_decode_nsplit forced to the fused launch's split count.  attn_decode_kernel runs both: the chunk, the key of
    thread group kg (k_lo + kg + i * NKG), the dot product, the online softmax and both merges do not depend on the mode; the
    only difference is `is_new ? knew : kk[i]`, the new row from registers instead of from the cache, and those are the bits
    rope_kv_append stores (both round rnd(rnd(x c) + rnd(rot(x) s)); the append assertion of the test above pins them to the same
    mirror).  The plain launch reads planes one row longer (cap + 1), so that n_old = cap has room for its row there: the cap
    only enters the row addresses.  (Not for the shadow: there the new key is attended unquantised, the plain launch knows only
    codes.)"""
    E = H * hd
    cos, sin = KC.rope_tables(hd, CAP + 16, dtype)
    cos_d, sin_d = dev(cos), dev(sin)
    for case in KC.DECODE_STEP_CASES:
        nb, knob, ns, n_olds, done = case
        what = case_name("attn_decode_step vs two launches", (hd, dtype), case)
        inp = KC.decode_step_inputs(case, hd, dtype)
        with knobs(attn_decode_nsplit=knob):
            got = launch(ops, inp, cos_d, sin_d, what)
        for b in range(nb):
            if done[b]:
                continue
            n = n_olds[b]
            k2, v2 = (KC.poison_(torch.empty(H, CAP + 1, hd, dtype=dtype)) for _ in range(2))
            k2[:, :CAP], v2[:, :CAP] = inp.kc[b], inp.vc[b]
            k2, v2 = dev(k2), dev(v2)
            q = ops.rope_kv_append(dev(inp.qkv[b:b + 1]), k2, v2, cos_d, sin_d, H, n, pos_start=inp.pos[b])
            g = guarded(1, E, dtype)
            with knobs(attn_decode_nsplit=ns):
                ops.attn_decode(q.view(E), k2, v2, torch.tensor([n + 1], dtype=torch.int32, device=DEV), out=g.view(E))
            y2 = g.check(what + " (plain launch)").view(E)
            assert bool(got.written[b].all()), "%s seq %d: output row not written" % (what, b)
            assert torch.equal(KC.bits(got.out[b]), KC.bits(y2)), "%s seq %d: %d elements differ" % (
                what, b, int((KC.bits(got.out[b]) != KC.bits(y2)).sum()))


@pytest.mark.parametrize("param", PARAMS, ids=pid)
def test_decode_step_selector(ops, param):
    """identity RoPE tables, KC.decode_step_selector_inputs: the new key is the last key and takes all the weight, so the output
    is the new V row bit for bit (shadow: the UNQUANTISED new V row); second probe: a zero new K row leaves the largest score on
    key n_old - 1 and the output is v[n_old - 1] — the new key does not mask the old ones"""
    hd, dtype, shadow = param
    cos_d, sin_d = (dev(t) for t in identity_tables(hd, dtype))
    for case in KC.decode_step_selector_cases():
        live = [b for b in range(case[0]) if not case[4][b]]
        for second in (False, True):
            if second and min(case[3][b] for b in live) < 2:
                continue
            what = case_name("decode step selector%s%s" % (" kv8" if shadow else "", " (zero new key)" if second else ""), param, case)
            inp, want = KC.decode_step_selector_inputs(case, hd, dtype, second, shadow)
            got = launch(ops, inp, cos_d, sin_d, what)
            assert bool(got.written[live].all()) and not bool(got.written[[b for b in range(case[0]) if b not in live]].any()), what
            assert torch.equal(KC.bits(got.out[live]), KC.bits(want[live])), what


def test_decode_step_refuses_bad_arguments(ops):
    """nb = 0, nb = 9, fp32 with the shadow, hd = 104, a misaligned plane, a too-small cache_stride: SSError before any launch —
    every buffer and guard as it was"""
    from seedstory._lib import SSError
    cap = 32

    def attempt(what, nb, hd, dtype, shadow, rows=None, stride_less=0, misalign=False):
        rows = nb if rows is None else rows                 # sequences the buffers are sized for
        stride = (H * cap + 16) * hd
        bufs = [guarded(rows, stride, dtype) for _ in range(2)] + [guarded(max(nb, 1), H * hd, dtype)]
        for g in bufs[:2]:
            g.view(rows * stride).fill_(1.0)
        planes = [g.view(rows * stride)[1:] if misalign and i == 0 else g.view(rows * stride) for i, g in enumerate(bufs[:2])]
        cos, sin = (torch.ones(cap + 16, hd, dtype=dtype, device=DEV) for _ in range(2))
        state = torch.zeros(nb, KC.DECODE_STEP_WORDS, dtype=torch.int32, device=DEV)
        qkv = torch.ones(nb, 3 * H * hd, dtype=dtype, device=DEV)
        kw = dict(WORDS, cache_stride=stride - stride_less, out=bufs[2].view(max(nb, 1), H * hd)[:nb])
        with pytest.raises(SSError):
            if shadow:
                codes = [torch.full((rows * stride,), 0x11, dtype=torch.uint8, device=DEV) for _ in range(2)]
                scales = [torch.full((rows * stride // hd,), 2.0, device=DEV) for _ in range(2)]
                ops.attn_decode_kv8_step(qkv, planes[0], planes[1], codes[0], codes[1], scales[0], scales[1], cos, sin, state, H, cap, **kw)
            else:
                ops.attn_decode_step(qkv, planes[0], planes[1], cos, sin, state, H, cap, **kw)
        for g in bufs[:2]:
            assert bool((g.check(what, payload=False) == 1.0).all()), what + ": a plane was written"
        y = bufs[2].check(what, payload=False)
        assert bool(bufs[2].untouched(y).all()), what + ": the output was written"
        if shadow:
            assert all(bool((c == 0x11).all()) for c in codes) and all(bool((s == 2.0).all()) for s in scales), what + ": the shadow was written"

    for shadow in (False, True):
        name = "attn_decode_kv8_step" if shadow else "attn_decode_step"
        attempt(name + " nb = 0", 0, 64, torch.bfloat16, shadow, rows=1)
        attempt(name + " nb = 9", 9, 64, torch.bfloat16, shadow)
        attempt(name + " hd = 104", 2, 104, torch.bfloat16, shadow)
        attempt(name + " misaligned plane", 2, 64, torch.bfloat16, shadow, rows=3, misalign=True)
        attempt(name + " cache_stride below a plane", 2, 64, torch.bfloat16, shadow, stride_less=17 * 64)
    attempt("attn_decode_kv8_step fp32", 2, 64, F32, True)


def test_zz_worst_ratios():
    print()
    print(KC.worst_table(families=tuple(KC.DECODE_STEP_FAMILY.values())))

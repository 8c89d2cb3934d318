"""GPU checks of the stochastic samplers: ``ss_randn_philox`` and ``ss_multistep_noise_step`` element by element, whole fp32
trajectories against ``tests/sde_ref.py``, and the pipeline's Euler-ancestral and DPM++ 2M SDE renders on the tiny synthetic UNet.

The noise bound (a priori, from the fp64 reference; nothing in it comes from the kernel's output).  The kernel computes, in fp32,
for one normal z = r c with the uniforms u0 (radius) and u1 (angle), both exact multiples of 2^-24:

    t = u0 + 2^-24                 exact (a multiple of 2^-24 in (0, 1])
    L = logf(t)                    library function: 4 u32 relative to the result (the allowance ``KC.exp32`` gives one)
    m = -2 L                       exact (a power of two)
    r = sqrtf(m)                   ``KC.sqrt32``: the operand's uncertainty through the square root, plus one rounding
    c = cospi(2 u1) | sinpi(2 u1)  library function, exact argument: 4 u32 ABSOLUTE (|c| <= 1)
    z = r c                        ``KC.op32`` on |c| t_r + |r| t_c + t_r t_c

u32 = 2^-24.  ``out`` in bf16 / fp16 adds the final half-ulp (``KC.final_round``); fp32 stores z as it stands.

``ss_multistep_noise_step``: ``test_dpmpp_gpu.ms_bound`` (two rows of eps) or ``test_guidance_gpu.ms1_bound`` (one) up to x', then the
two new operations  t7 = s z  (``KC.op32`` on |s| t_z, z carrying the bound above) and  x' = x' + t7  (``KC.op32`` on the sum of the
two uncertainties), then  xs = x' inv  and the final roundings as there.  d does not see the noise.

The pipeline bounds are the project's own for this UNet: 5e-4 against the reference loop, 2e-4 batch against single calls; the
trajectory bound is 1e-5 (``test_dpmpp_gpu.test_trajectories_fp32_equal_reference_and_are_second_order``).

Measured on an MI355X (``test_zz_worst_ratios`` prints the table, the other figures are printed by their tests): worst error / bound
randn_philox 0.996 / 0.998 / 0.413, noise_step x' 0.688 / 0.713 / 0.694, d 0.990 / 0.992 / 0.993, x_out 0.996 / 0.999 / 0.694, xin_next
0.996 / 0.998 / 0.647 in bf16 / fp16 / fp32.  Whole fp32 trajectories through the kernel against sde_ref: 3.0e-7 (2M SDE), 2.3e-7
(Euler ancestral), the noise moving the end point by 0.15 / 0.12 relative to the deterministic run.  Pipeline against sde_ref over the
oracle UNet: 4.5e-6 (2M SDE Karras), 4.2e-6 (Euler ancestral), 3.3e-6 (2M SDE Karras, interval u G G G u u).
"""
import math

import numpy as np
import pytest
import torch

import dpmpp_ref as R
import kernel_check as KC
import sde_ref as S
import sdxl_oracle as SO
from test_dpmpp_gpu import MS_SIGMAS, _cond, _models, coefficient_sets, f32, ms_inputs, rel
from test_guidance_gpu import FORMS, GUIDANCE, SS_EINVAL, _bits, eps_for, form_bound, run_form
from test_pointwise_edges_gpu import ALL, DEV, F32, dev, dname, ops  # noqa: F401  (ops: fixture)

pytestmark = pytest.mark.gpu

FAMILIES = {"randn_philox", "noise_step x'", "noise_step d", "noise_step x_out", "noise_step xin_next"}
SEED_S, SEED_T = 0x1234567800000009, 0xFEDCBA9876543210          # both above 2^32; T above 2^63
RANDN_N = [1, 3, 4, 5, 8, 9, 257, 1048576 + 3]
NS_SHAPES = [(1, 1), (1, 7), (3, 9), (3, 12), (1, 257), (2, 524288 + 4)]      # (batch, n_img)


# ---- the noise ------------------------------------------------------------------------------------------------------------------------
def z_bound(seed, step, n_img, dtype=F32):
    """-> (reference [n_img], bound [n_img]) of rnd_T(z(seed, step, j)), fp64 (see the module docstring)"""
    u_r, u_a, is_sin = S.lane_uniforms(seed, step, np.arange(n_img, dtype=np.int64))
    L = torch.from_numpy(np.log(u_r + S.TWO_M24))
    vm, tm = -2.0 * L, 2.0 * (4.0 * KC.U32 * L.abs())
    vr, tr = KC.sqrt32(vm, tm)
    ang = 2.0 * np.pi * u_a
    c = torch.from_numpy(np.where(is_sin, np.sin(ang), np.cos(ang)))
    tc = torch.full_like(c, 4.0 * KC.U32)
    vz, tz = KC.op32(vr * c, c.abs() * tr + vr.abs() * tc + tr * tc)
    return (vz, tz) if dtype == F32 else KC.final_round(vz, tz, dtype)


def seeds_dev(ops, seeds):
    return ops.noise_seeds(seeds, DEV)


def randn_call(ops, g, sd, n_img, step, dtype):
    ops.check(ops.lib().ss_randn_philox(g.data_ptr(), ops.p(sd), sd.numel(), n_img, step, ops.dt(dtype), ops.stream()), "ss_randn_philox")


@pytest.mark.parametrize("dtype", ALL, ids=dname)
@pytest.mark.parametrize("n_img", RANDN_N)
def test_randn_philox_elementwise(ops, n_img, dtype):
    """every element inside the bound at steps 0 and 19, batch 1 (two seeds) and batch 3 with seeds (S, T, S): rows 0 and 2 bit-equal,
    every row bit-equal to the batch-1 call with its seed; guards untouched"""
    worst = 0.0
    for step in (0, 19):
        single = {}
        for seed in (SEED_S, SEED_T):
            what = "randn %s n_img %d step %d seed %x" % (dname(dtype), n_img, step, seed)
            g = KC.GuardedOut(1, n_img, dtype, device=DEV)
            randn_call(ops, g, seeds_dev(ops, [seed]), n_img, step, dtype)
            single[seed] = g.check(what)
            ref, tol = z_bound(seed, step, n_img, dtype)
            worst = max(worst, KC.check(single[seed][0], ref, tol, what, family="randn_philox", dtype=dtype))
        g3 = KC.GuardedOut(3, n_img, dtype, device=DEV)
        randn_call(ops, g3, seeds_dev(ops, [SEED_S, SEED_T, SEED_S]), n_img, step, dtype)
        rows = g3.check("randn batch 3").view(KC._INT[dtype])
        assert torch.equal(rows[0], rows[2])
        for b, seed in enumerate((SEED_S, SEED_T, SEED_S)):
            assert torch.equal(rows[b], single[seed][0].view(KC._INT[dtype])), (b, step)
    print("randn_philox %s n_img %d: worst error / bound %.3f" % (dname(dtype), n_img, worst))


@pytest.mark.parametrize("dtype", ALL, ids=dname)
def test_randn_philox_seed_words_unaligned_base_and_wrapper(ops, dtype):
    """a seed >= 2^32 differs from its low word alone; steps differ; a base one element off a 16-byte boundary (single elements)
    gives the bits of the aligned call; the wrapper returns the same bits and checks its arguments"""
    from seedstory import _lib
    n_img = 264
    out = {}
    for key, seed, step, off in (("S", SEED_S, 3, 0), ("lo", SEED_S & 0xFFFFFFFF, 3, 0), ("step", SEED_S, 4, 0), ("off", SEED_S, 3, 1)):
        g = KC.GuardedOut(1, n_img, dtype, device=DEV, offset=off)
        randn_call(ops, g, seeds_dev(ops, [seed]), n_img, step, dtype)
        out[key] = g.check(key)[0].view(KC._INT[dtype])
    assert torch.equal(out["S"], out["off"])
    assert not torch.equal(out["S"], out["lo"]) and not torch.equal(out["S"], out["step"])
    sd = seeds_dev(ops, [SEED_S, SEED_T])
    got = ops.randn_philox(sd, n_img, 3, dtype)
    assert got.shape == (2, n_img) and got.dtype == dtype and torch.equal(got[0].cpu().view(KC._INT[dtype]), out["S"])
    buf = torch.zeros(2 * n_img, dtype=dtype, device=DEV)
    assert ops.randn_philox(sd, n_img, 3, dtype, out=buf) is buf and torch.equal(buf.view(2, n_img), got)
    for bad in (lambda: ops.randn_philox(sd.int(), n_img, 3, dtype), lambda: ops.randn_philox(sd, 0, 3, dtype),
                lambda: ops.randn_philox(sd, n_img, -1, dtype), lambda: ops.randn_philox(sd, n_img, 3, dtype, out=buf[:n_img])):
        with pytest.raises(_lib.SSError):
            bad()
    # refusals write nothing
    g = KC.GuardedOut(1, n_img, dtype, device=DEV)
    lib = ops.lib()
    for args in ((None, ops.p(sd), 1, n_img, 0, ops.dt(dtype)), (g.data_ptr(), None, 1, n_img, 0, ops.dt(dtype)),
                 (g.data_ptr(), ops.p(sd), 0, n_img, 0, ops.dt(dtype)), (g.data_ptr(), ops.p(sd), 1, 0, 0, ops.dt(dtype)),
                 (g.data_ptr(), ops.p(sd), 1, n_img, -1, ops.dt(dtype)), (g.data_ptr(), ops.p(sd), 1, n_img, 0, 9)):
        assert lib.ss_randn_philox(*args, ops.stream()) == SS_EINVAL, args
    torch.cuda.synchronize()
    assert bool((g.flat == KC.SENTINEL[dtype]).all())


# ---- ss_multistep_noise_step ------------------------------------------------------------------------------------------------------------
def noise_call(ops, gs, epsd, gx, gi, n, form, guidance, sigma, abc, s, inv, sd, n_img, step, dtype):
    return ops.lib().ss_multistep_noise_step(gs.data_ptr(), epsd.data_ptr(), None if gx is None else gx.data_ptr(),
                                             None if gi is None else gi.data_ptr(), n, form[0], form[1], guidance, sigma, abc[0],
                                             abc[1], abc[2], s, inv, None if sd is None else ops.p(sd), n_img, step, ops.dt(dtype),
                                             ops.stream())


def run_noise(ops, n, dtype, st, epsd, form, sigma, abc, s, inv, sd, n_img, step, offset=0, outs=(True, True), guidance=GUIDANCE):
    """``test_guidance_gpu.run_form`` through the new entry point"""
    gs = KC.GuardedOut(2, n, F32, device=DEV, offset=offset)
    gs.out.copy_(st)
    if abc[2] == 0.0:
        gs.out[1].fill_(float("nan"))               # c == 0: row 1 of state is not read
    gx = KC.GuardedOut(1, n, dtype, device=DEV, offset=offset) if outs[0] else None
    gi = KC.GuardedOut(form[1], n, dtype, device=DEV, offset=offset) if outs[1] else None
    ops.check(noise_call(ops, gs, epsd, gx, gi, n, form, guidance, sigma, abc, s, inv, sd, n_img, step, dtype), "ss_multistep_noise_step")
    return gs, gx, gi


def noise_bound(st, eps, eps_rows, sigma, abc, s, inv, z, dtype):
    """the plain step's bound up to x' (its fp32 form: nothing rounded to T yet), then t7 = s z, x' = x' + t7, xs = x' inv"""
    base = form_bound(st, eps, eps_rows, sigma, abc, inv, F32)
    vx, tx = base["x"]
    sv, iv = (torch.tensor(f32(v), dtype=torch.float64) for v in (s, inv))
    v7, t7 = KC.op32(sv * z[0], sv.abs() * z[1])
    vx, tx = KC.op32(vx + v7, tx + t7)
    vs, tsc = KC.op32(vx * iv, iv.abs() * tx)
    xo, xi = ((vx, tx), (vs, tsc)) if dtype == F32 else (KC.final_round(vx, tx, dtype), KC.final_round(vs, tsc, dtype))
    return {"x": (vx, tx), "d": base["d"], "x_out": xo, "xin_next": (torch.stack([xi[0], xi[0]]), torch.stack([xi[1], xi[1]]))}


def check_noise(ref, form, guards, what, dtype):
    gs, gx, gi = guards
    new = gs.check(what + " state")
    KC.check(new[0], *ref["x"], what + " x'", family="noise_step x'", dtype=dtype)
    KC.check(new[1], *ref["d"], what + " d", family="noise_step d", dtype=dtype)
    if gx is not None:
        KC.check(gx.check(what + " x_out")[0], *ref["x_out"], what + " x_out", family="noise_step x_out", dtype=dtype)
    if gi is not None:
        rv, rt = ref["xin_next"]
        KC.check(gi.check(what + " xin_next"), rv[:form[1]], rt[:form[1]], what + " xin_next", family="noise_step xin_next", dtype=dtype)


def shape_seeds(batch):
    return [SEED_S, SEED_T, SEED_S][:batch]


def shape_z(seeds, step, n_img):
    parts = {sd: z_bound(sd, step, n_img) for sd in set(seeds)}
    return torch.cat([parts[sd][0] for sd in seeds]), torch.cat([parts[sd][1] for sd in seeds])


@pytest.mark.parametrize("dtype", ALL, ids=dname)
@pytest.mark.parametrize("shape", NS_SHAPES, ids=lambda s: "%dx%d" % s)
def test_noise_step_elementwise(ops, shape, dtype):
    """the four forms, every coefficient set, s = sigma_n / 2 inside the bound and s = 0 bit-equal to ss_multistep_step (NULL seeds),
    at both ends of the 15-step Karras table (the last step has sigma_n = 0: s = 0 only)"""
    batch, n_img = shape
    n = batch * n_img
    seeds = shape_seeds(batch)
    sd = seeds_dev(ops, seeds)
    step = 7
    z = shape_z(seeds, step, n_img)
    for k, (sigma, sigma_next) in enumerate(MS_SIGMAS):
        inv = 1.0 / math.sqrt(sigma_next * sigma_next + 1.0)
        st, eps = ms_inputs(n, dtype, sigma, 1200 + 10 * k + n % 89)
        for eps_rows in (2, 1):
            epsd = eps_for(eps, eps_rows)
            for name, abc in coefficient_sets(sigma, sigma_next).items():
                s = 0.5 * sigma_next
                ref = noise_bound(st, eps, eps_rows, sigma, abc, s, inv, z, dtype) if s != 0.0 else None
                for xin_rows in (2, 1):
                    form = (eps_rows, xin_rows)
                    what = "%s %dx%d form %s sigma %g -> %g %s" % (dname(dtype), batch, n_img, form, sigma, sigma_next, name)
                    if ref is not None:
                        check_noise(ref, form, run_noise(ops, n, dtype, st, epsd, form, sigma, abc, s, inv, sd, n_img, step), what, dtype)
                    plain = [_bits(g) for g in run_form(ops, n, dtype, st, epsd, form, sigma, abc, inv)]
                    zero = [_bits(g) for g in run_noise(ops, n, dtype, st, epsd, form, sigma, abc, 0.0, inv, None, n_img, step)]
                    assert all(torch.equal(a, b) for a, b in zip(plain, zero)), what + ": s = 0 differs from ss_multistep_step"


@pytest.mark.parametrize("dtype", ALL, ids=dname)
@pytest.mark.parametrize("form", FORMS, ids=lambda f: "e%dx%d" % f)
def test_noise_step_unaligned_bases_and_null_outputs(ops, form, dtype):
    """buffers one element off a 16-byte boundary take the single-element path (3 x 8 and 1 x 1048579: one past what one sweep of the
    capped grid covers); each NULL output is skipped and the rest intact (2 x 264: packets)"""
    sigma, sigma_next = MS_SIGMAS[0]
    inv = 1.0 / math.sqrt(sigma_next * sigma_next + 1.0)
    abc = coefficient_sets(sigma, sigma_next)["middle"]
    s = 0.5 * sigma_next
    for batch, n_img in ((3, 8), (1, 1048576 + 3)):
        n, seeds = batch * n_img, shape_seeds(batch)
        st, eps = ms_inputs(n, dtype, sigma, 1260 + n % 89)
        ref = noise_bound(st, eps, form[0], sigma, abc, s, inv, shape_z(seeds, 2, n_img), dtype)
        guards = run_noise(ops, n, dtype, st, eps_for(eps, form[0], offset=1), form, sigma, abc, s, inv, seeds_dev(ops, seeds), n_img, 2, offset=1)
        check_noise(ref, form, guards, "%s %dx%d form %s unaligned" % (dname(dtype), batch, n_img, form), dtype)
    batch, n_img = 2, 264
    n, seeds = batch * n_img, shape_seeds(batch)
    st, eps = ms_inputs(n, dtype, sigma, 1280)
    ref = noise_bound(st, eps, form[0], sigma, abc, s, inv, shape_z(seeds, 2, n_img), dtype)
    epsd, sd = eps_for(eps, form[0]), seeds_dev(ops, seeds)
    for outs in ((True, False), (False, True), (False, False)):
        check_noise(ref, form, run_noise(ops, n, dtype, st, epsd, form, sigma, abc, s, inv, sd, n_img, 2, outs=outs),
                    "%s form %s outputs %s" % (dname(dtype), form, outs), dtype)


@pytest.mark.parametrize("shape", [(1, 7), (3, 12), (2, 264), (2, 524288 + 4)], ids=lambda s: "%dx%d" % s)
def test_noise_step_generator_is_randn_philox(ops, shape):
    """a = b = c = 0, s = 1, finite state: x' = 0 + 1 z, so state row 0 holds the bits ss_randn_philox writes in fp32 — the fused and
    the stand-alone generator are one function (single elements and packets); and the wrapper drives the same call"""
    batch, n_img = shape
    n, seeds = batch * n_img, shape_seeds(batch)
    sd = seeds_dev(ops, seeds)
    st, eps = ms_inputs(n, F32, 1.0, 1300 + n % 89)
    g = KC.GuardedOut(batch, n_img, F32, device=DEV)
    randn_call(ops, g, sd, n_img, 11, F32)
    want = g.check("randn").view(torch.int32).reshape(-1)
    for form in ((2, 2), (1, 1)):
        gs, gx, gi = run_noise(ops, n, F32, st, eps_for(eps, form[0]), form, 1.0, (0.0, 0.0, 0.0), 1.0, 1.0, sd, n_img, 11)
        assert torch.equal(gs.check("state")[0].view(torch.int32), want), form
        assert torch.equal(gx.check("x_out")[0].view(torch.int32), want), form
    state = dev(st)
    xo = torch.empty(n, device=DEV)
    ops.multistep_noise_step_(state, eps_for(eps, 2), GUIDANCE, 1.0, 0.0, 0.0, 0.0, 1.0, 1.0, sd, 11, x_out=xo)
    assert torch.equal(xo.cpu().view(torch.int32), want)


@pytest.mark.parametrize("dtype", ALL, ids=dname)
def test_noise_step_refusals_write_nothing(ops, dtype):
    from seedstory import _lib
    batch, n_img = 3, 88
    n = batch * n_img
    sigma, sigma_next = MS_SIGMAS[0]
    st, eps = ms_inputs(n, dtype, sigma, 1380)
    epsd = dev(eps)
    sd = seeds_dev(ops, shape_seeds(batch))
    abc = coefficient_sets(sigma, sigma_next)["middle"]
    gs, gx, gi = KC.GuardedOut(2, n, F32, device=DEV), KC.GuardedOut(1, n, dtype, device=DEV), KC.GuardedOut(2, n, dtype, device=DEV)
    gs.out.copy_(st)
    before = gs.flat.clone()
    inv = 1.0 / math.sqrt(sigma_next ** 2 + 1.0)
    nan, inf = float("nan"), float("inf")
    lib = ops.lib()

    def raw(state=None, e=None, n_=n, rows=(2, 2), g=GUIDANCE, sg=sigma, coef=abc, s=0.5, iv=inv, seeds=sd, ni=n_img, step=3, dt_=None):
        return lib.ss_multistep_noise_step(gs.data_ptr() if state is None else state[0], ops.p(epsd) if e is None else e[0], gx.data_ptr(),
                                           gi.data_ptr(), n_, rows[0], rows[1], g, sg, coef[0], coef[1], coef[2], s, iv,
                                           None if seeds is None else ops.p(seeds), ni, step, ops.dt(dtype) if dt_ is None else dt_, ops.stream())
    bad = [lambda: raw(state=(None,)), lambda: raw(e=(None,)), lambda: raw(n_=0), lambda: raw(n_=-n), lambda: raw(ni=0), lambda: raw(ni=-8),
           lambda: raw(ni=n_img + 1), lambda: raw(ni=2 * n), lambda: raw(step=-1), lambda: raw(seeds=None), lambda: raw(s=nan), lambda: raw(s=inf),
           lambda: raw(g=nan), lambda: raw(sg=inf), lambda: raw(coef=(nan, abc[1], abc[2])), lambda: raw(coef=(abc[0], inf, abc[2])),
           lambda: raw(coef=(abc[0], abc[1], nan)), lambda: raw(iv=nan), lambda: raw(dt_=9), lambda: raw(rows=(0, 2)), lambda: raw(rows=(3, 2)),
           lambda: raw(rows=(2, 0)), lambda: raw(rows=(1, 3))]
    for i, fn in enumerate(bad):
        assert fn() == SS_EINVAL, i
    torch.cuda.synchronize()
    assert torch.equal(gs.flat, before)
    for g in (gx, gi):
        assert bool((g.flat == KC.SENTINEL[dtype]).all())
    # the wrapper's own checks
    state = torch.zeros(2, n, device=DEV)
    for fn in (lambda: ops.multistep_noise_step_(state, epsd, GUIDANCE, sigma, *abc, 0.5, inv, sd, 0, eps_rows=1),       # eps has two rows
               lambda: ops.multistep_noise_step_(state, epsd, GUIDANCE, sigma, *abc, 0.5, inv, sd, 0, eps_rows=3),
               lambda: ops.multistep_noise_step_(state, epsd, GUIDANCE, sigma, *abc, 0.5, inv, None, 0),                 # s != 0 needs seeds
               lambda: ops.multistep_noise_step_(state, epsd, GUIDANCE, sigma, *abc, 0.5, inv, sd.int(), 0),
               lambda: ops.multistep_noise_step_(state, epsd, GUIDANCE, sigma, *abc, 0.5, inv, seeds_dev(ops, [1, 2, 3, 4, 5]), 0),
               lambda: ops.multistep_noise_step_(state, epsd, GUIDANCE, sigma, *abc, 0.5, inv, sd, 0,
                                                 xin_next=torch.empty(2, n, dtype=dtype, device=DEV), xin_rows=1)):
        with pytest.raises(_lib.SSError):
            fn()


# ---- whole trajectories in fp32 -------------------------------------------------------------------------------------------------------
def _kernel_run(ops, prob, sigmas, coefs4, seeds, n_img):
    """the kernel driven over a whole run; eps from the analytic model, evaluated in fp32 on the host from the state the kernel left"""
    n = len(prob["noise"])
    x0 = (prob["noise"] * math.sqrt(float(sigmas[0]) ** 2 + 1.0)).astype(np.float32)
    state = torch.zeros(2, n, dtype=torch.float32, device=DEV)
    state[0].copy_(torch.from_numpy(x0))
    sd = seeds_dev(ops, seeds)
    eps_fn = R.gaussian_eps(prob, sigmas, np.float32)
    for i in range(len(sigmas) - 1):
        e_u, e_c = eps_fn(state[0].cpu().numpy(), i)
        eps = torch.from_numpy(np.stack([e_u, e_c])).to(DEV)
        a, b, c, s = (float(v) for v in coefs4[i])
        ops.multistep_noise_step_(state, eps, prob["guidance"], float(sigmas[i]), a, b, c, s, 1.0 / math.sqrt(float(sigmas[i + 1]) ** 2 + 1.0), sd, i)
    return state[0].cpu().numpy().astype(np.float64), x0.astype(np.float64)


@pytest.mark.parametrize("sampler", ["2m-sde", "euler-a"])
def test_trajectories_fp32_equal_reference(ops, sampler):
    """4096 elements as two images of 2048 with their own seeds, 20 Karras steps, guidance 7.5"""
    prob = R.gaussian_problem()
    s = S.schedule(20, sampler, use_karras_sigmas=True)
    seeds = [41, SEED_T]
    got, x0 = _kernel_run(ops, prob, s["sigmas"], s["coefficients"], seeds, 2048)
    both = R.gaussian_eps(prob, s["sigmas"])
    ref = S.sample(lambda x, i, guided: both(x, i), x0, s["sigmas"], s["coefficients"], prob["guidance"], None, seeds, 2048)
    dist = R.rel_rms(got, ref)
    det = R.sample(both, x0, s["sigmas"], s["coefficients"][:, :3], prob["guidance"])
    print("%s, 20 Karras steps: kernel vs sde_ref %.3e (the noise moved the end point by %.3e)" % (sampler, dist, R.rel_rms(ref, det)))
    assert dist <= 1e-5
    assert R.rel_rms(ref, det) > 1e-2                       # the run really was stochastic


# ---- the pipeline on the tiny synthetic UNet ------------------------------------------------------------------------------------------
STEPS = 6
N_IMG = 4 * 8 * 8
INTERVAL, PATTERN = (0.3, 3.0), [False, True, True, True, False, False]      # 6 Karras steps: 5.906, 2.791, 1.205, 0.464, 0.154, 0.041


def render(pipe, cond, steps=STEPS, sl=slice(None), **kw):
    cp, cn, pp, pn, noise = (v[sl].to(DEV) for v in cond)
    return pipe(prompt_embeds=cp, negative_prompt_embeds=cn, pooled_prompt_embeds=pp, negative_pooled_prompt_embeds=pn, latents=noise,
                guidance_scale=7.5, num_inference_steps=steps, height=64, width=64, output_type="latent", **kw).images


def ref_latents(wd, c, cond, sampler, seeds, interval=None, steps=STEPS, size=64):
    """sde_ref's loop over the oracle's UNet (fp32 on the CPU)"""
    cp, cn, pp, pn, noise = cond
    sch = S.schedule(steps, sampler, use_karras_sigmas=sampler == "2m-sde")
    sig, ts = sch["sigmas"], sch["timesteps"]
    B = noise.shape[0]
    ids = torch.tensor([[size, size, 0, 0, size, size]] * (2 * B), dtype=noise.dtype)
    ctx, pooled = torch.cat([cn, cp], dim=0), torch.cat([pn, pp], dim=0)

    def eps_fn(x, i, guided):
        scale = math.sqrt(float(sig[i]) ** 2 + 1.0)
        if guided:
            e_neg, e_pos = SO.unet_forward(wd, c, torch.cat([x, x], dim=0) / scale, float(ts[i]), ctx, pooled, ids).chunk(2)
            return e_neg, e_pos
        return SO.unet_forward(wd, c, x / scale, float(ts[i]), cp, pp, ids[B:])
    return S.sample(eps_fn, noise * sch["init_noise_sigma"], sig, sch["coefficients"], 7.5, interval, seeds, N_IMG)


@pytest.fixture(scope="module")
def tiny():
    from seedstory.diffusion import DPMSolverMultistepSDEScheduler, EulerAncestralDiscreteScheduler, StableDiffusionXLPipeline
    m, vae, wd, c = _models(torch.float32)
    pipes = {"2m-sde": StableDiffusionXLPipeline(vae=vae, unet=m, scheduler=DPMSolverMultistepSDEScheduler(use_karras_sigmas=True)),
             "euler-a": StableDiffusionXLPipeline(vae=vae, unet=m, scheduler=EulerAncestralDiscreteScheduler())}
    return pipes, m, vae, wd, c


@pytest.mark.parametrize("case", [("2m-sde", None), ("euler-a", None), ("2m-sde", INTERVAL)], ids=lambda c: "%s-%s" % (c[0], "all" if c[1] is None else "interval"))
def test_pipeline_equals_reference_loop(tiny, case):
    """64 x 64, 6 steps, g = 7.5, fp32, B = 2 with two seeds; the same seeds twice give the same bits (replayed graphs), another
    noise_seed does not"""
    sampler, interval = case
    pipes, m, vae, wd, c = tiny
    pipe = pipes[sampler]
    cond = _cond(2, 1530)
    seeds = [SEED_S, 77]
    out = render(pipe, cond, noise_seed=seeds, guidance_interval=interval).clone()
    if interval is not None:
        assert pipe.last_guidance == {"mask": PATTERN, "unet_batches": [4 if g else 2 for g in PATTERN]}
    ref = ref_latents(wd, c, cond, sampler, seeds, interval)
    print("%s interval %s: pipeline vs sde_ref over the oracle UNet: %.3e" % (sampler, interval, rel(out, ref)))
    assert out.shape == ref.shape and rel(out, ref) < 5e-4
    assert torch.equal(render(pipe, cond, noise_seed=seeds, guidance_interval=interval), out)
    other = render(pipe, cond, noise_seed=[SEED_S, 78], guidance_interval=interval)
    assert torch.equal(other[0], out[0]) and rel(other[1:], out[1:]) > 1e-2


@pytest.mark.parametrize("sampler", ["2m-sde", "euler-a"])
def test_pipeline_graph_replay_is_bit_equal_to_eager(tiny, sampler):
    from seedstory import _lib
    pipes, m, vae, wd, c = tiny
    pipe = pipes[sampler]
    cond = _cond(2, 1630)
    outs = {}
    for interval in (None, INTERVAL):
        for mode in (1, 0):
            _lib.set_tuning("unet_graph", mode)
            try:
                outs[mode] = render(pipe, cond, noise_seed=[5, 6], guidance_interval=interval).clone()
                if mode == 1:
                    assert any(v is not None for v in pipe._graphs.values()), "graph path was not taken"
            finally:
                _lib.set_tuning("unet_graph", 1)
        assert torch.equal(outs[1], outs[0]), interval


@pytest.mark.parametrize("sampler", ["2m-sde", "euler-a"])
def test_pipeline_default_noise_seed(tiny, sampler):
    """None: the generator's initial seed when one is given, else 0; an int is every image's seed"""
    pipes, m, vae, wd, c = tiny
    pipe = pipes[sampler]
    cond = _cond(2, 1730)
    zero = render(pipe, cond).clone()
    assert torch.equal(render(pipe, cond, noise_seed=0), zero) and torch.equal(render(pipe, cond, noise_seed=[0, 0]), zero)
    gen = torch.Generator(DEV).manual_seed(1234)
    with_gen = render(pipe, cond, generator=gen).clone()
    assert torch.equal(render(pipe, cond, noise_seed=1234), with_gen) and not torch.equal(with_gen, zero)


@pytest.mark.parametrize("sampler", ["2m-sde", "euler-a"])
def test_pipeline_batch_equals_single_calls(tiny, sampler):
    """seeds (s0, s1, s0) on conditioning (c0, c1, c0): every image against its own batch-1 call; images 0 and 2 have the same bits"""
    pipes, m, vae, wd, c = tiny
    pipe = pipes[sampler]
    two = _cond(2, 1830)
    cond = [v[[0, 1, 0]] for v in two]
    seeds = [SEED_T, 9, SEED_T]
    for interval in (None, INTERVAL):
        lat = render(pipe, cond, noise_seed=seeds, guidance_interval=interval).clone()
        assert lat.shape == (3, 4, 8, 8)
        assert torch.equal(lat[0], lat[2]), interval
        for b in range(3):
            one = render(pipe, cond, sl=slice(b, b + 1), noise_seed=seeds[b], guidance_interval=interval)
            assert rel(lat[b:b + 1], one) < 2e-4, (interval, b)


def test_deterministic_schedulers_never_make_the_new_call(tiny, monkeypatch):
    """Euler and DPM++ 2M, with and without an interval: noise_seed is accepted and ignored (the bits of a call without it), and a
    spy on ops shows that neither new entry point is reached"""
    from seedstory import ops as O
    from seedstory.diffusion import DPMSolverMultistepScheduler, EulerDiscreteScheduler, StableDiffusionXLPipeline
    pipes, m, vae, wd, c = tiny
    cond = _cond(2, 1930)
    calls = []
    real = O.multistep_noise_step_
    monkeypatch.setattr(O, "multistep_noise_step_", lambda *a, **k: calls.append("step") or real(*a, **k))
    monkeypatch.setattr(O, "randn_philox", lambda *a, **k: calls.append("randn"))
    monkeypatch.setattr(O, "noise_seeds", lambda *a, **k: calls.append("seeds"))
    for sched in (EulerDiscreteScheduler(), DPMSolverMultistepScheduler(use_karras_sigmas=True)):
        pipe = StableDiffusionXLPipeline(vae=vae, unet=m, scheduler=sched)
        for interval in (None, INTERVAL):
            plain = render(pipe, cond, guidance_interval=interval).clone()
            assert torch.equal(render(pipe, cond, guidance_interval=interval, noise_seed=[3, 4]), plain)
    assert calls == []
    monkeypatch.undo()                                          # and the spy does see a stochastic render
    monkeypatch.setattr(O, "multistep_noise_step_", lambda *a, **k: calls.append("step") or real(*a, **k))
    render(pipes["euler-a"], cond, noise_seed=[3, 4])
    assert calls == ["step"] * STEPS


def test_zz_worst_ratios():
    print("\n" + KC.worst_table(FAMILIES))

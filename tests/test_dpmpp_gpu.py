"""GPU checks of the DPM-Solver++ 2M sampler: ``ss_multistep_cfg_step`` element by element, whole trajectories in fp32 against
``tests/dpmpp_ref.py`` and the exact solution, and the pipeline on the tiny synthetic UNet of ``tests/test_sdxl_gpu.py``.

The kernel's bound (a priori, from the fp64 reference; nothing in it comes from the kernel's output).  The kernel computes, in fp32,
with the six scalars g, sigma, a, b, c, inv as the fp32 values the C ABI receives (the reference uses exactly those):

    t1 = ec - eu;  t2 = g t1;  e = eu + t2;  t3 = sigma e;  d = x - t3;  t4 = a x;  t5 = b d;  x' = t4 + t5;
    c != 0:  t6 = c d_prev;  x' = x' + t6;          xs = x' inv

Every line is one correctly rounded fp32 operation (the library is built without contraction; a fused multiply-add would only
lose less).  Writing (v, t) for "exact value v, known to within t", an operation on operands known to t_in gives
t_out = t_in + u32 (|v| + t_in) with u32 = 2^-24 (``KC.op32``), where t_in is the operands' uncertainty carried through the exact
operation: |g| t for a product with a scalar, the sum of the two t for a sum.  So the bound of x' is u32 times the sum of the
magnitudes of the terms along its chain — |ec - eu|, |g (ec - eu)|, |e|, |sigma e|, |d|, |a x|, |b d|, |c d_prev|, |x'|, each
weighted by the factors that multiply it afterwards — and it does NOT shrink when the terms cancel.  The state rows are stored as
fp32: (x', t) and (d, t) as they stand.  ``x_out`` = rnd_T(x') and ``xin_next`` = rnd_T(xs) add the final half-ulp in T
(``KC.final_round``: u_T |v| + eta_T + (1 + u_T) t); in fp32 the store is exact and nothing is added.

Measured on an MI355X (test_zz_worst_ratios prints the table; the other figures are printed by their tests): worst error / bound
x' 0.855 / 0.858 / 0.854, d 0.991 / 0.994 / 0.997, x_out 0.996 / 0.999 / 0.854, xin_next 0.996 / 0.999 / 0.770 in bf16 / fp16 / fp32
(d at guidance 0 and the small-sigma end is two roundings, one of them negligible: the bound is then almost one rounding's).
Whole fp32 trajectories through the kernel against dpmpp_ref: 2.1e-7 .. 2.4e-7 (bound 1e-5); end-point error 6.10e-3 / 2.62e-3 /
1.36e-3 at 10 / 15 / 20 steps of 2M Karras, Euler 30: 9.81e-3.  Pipeline against dpmpp_ref over the oracle UNet: 3.6e-6 (bound 5e-4).
bf16 against the own fp32 run, 6 steps: Euler 2.85e-2, DPM++ 2M Karras 2.61e-2 (ratio 0.92, bound 2).
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import dpmpp_ref as R
import kernel_check as KC
import sdxl_oracle as S
import synth
from test_pointwise_edges_gpu import ALL, DEV, F32, call, dev, dname, guarded, ops  # noqa: F401  (ops: fixture)

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SS_EINVAL = -1
MS_N = [1, 7, 8, 9, 257, 1048576 + 3]          # the pack tail on either side of 8, and one element past the grid-stride cap
MS_GUIDANCE = [0.0, 1.0, 7.5]
K15 = R.schedule(15, use_karras_sigmas=True)
MS_SIGMAS = [(float(K15["sigmas"][0]), float(K15["sigmas"][1])), (float(K15["sigmas"][14]), 0.0)]   # both ends of the 15-step Karras table


def f32(v):
    return float(np.float32(v))


def coefficient_sets(sigma, sigma_next):
    """first step (c = 0), a middle step (second order, the table's own r where there is one), the last step, Euler's"""
    ratio = sigma_next / sigma if sigma_next > 0 else 0.25
    E = 1.0 - ratio
    return {"first": (ratio, E, 0.0), "middle": (ratio, E * 1.6, -E * 0.6), "last": (0.0, 1.0, 0.0), "euler": (ratio, 1.0 - ratio, 0.0)}


def ms_bound(state, eps, guidance, sigma, a, b, c, inv_next, dtype):
    """state [2, n] fp32, eps [2, n] T -> {"x", "d", "x_out", "xin_next"}: (reference, bound), fp64 (see the module docstring)"""
    g, sg, a, b, c, inv = (torch.tensor(f32(v), dtype=torch.float64) for v in (guidance, sigma, a, b, c, inv_next))
    x, dp = state[0].double(), state[1].double()
    eu, ec = eps[0].double(), eps[1].double()
    zero = torch.zeros_like(x)
    v1, t1 = KC.op32(ec - eu, zero)
    v2, t2 = KC.op32(g * v1, g.abs() * t1)
    ve, te = KC.op32(eu + v2, t2)
    v3, t3 = KC.op32(sg * ve, sg.abs() * te)
    vd, td = KC.op32(x - v3, t3)
    v4, t4 = KC.op32(a * x, zero)
    v5, t5 = KC.op32(b * vd, b.abs() * td)
    vx, tx = KC.op32(v4 + v5, t4 + t5)
    if float(c) != 0.0:
        v6, t6 = KC.op32(c * dp, zero)
        vx, tx = KC.op32(vx + v6, tx + t6)
    vs, tsc = KC.op32(vx * inv, inv.abs() * tx)
    xo, xi = ((vx, tx), (vs, tsc)) if dtype == F32 else (KC.final_round(vx, tx, dtype), KC.final_round(vs, tsc, dtype))
    return {"x": (vx, tx), "d": (vd, td), "x_out": xo, "xin_next": (torch.stack([xi[0], xi[0]]), torch.stack([xi[1], xi[1]]))}


def ms_inputs(n, dtype, sigma, seed):
    """x ~ N(0, sigma^2 + 1) (what the state is at that sigma), d_prev ~ N(0, 1), eps ~ N(0, 1) in T"""
    st = torch.stack([KC.randn_t((n,), F32, seed, std=math.sqrt(sigma * sigma + 1.0)), KC.randn_t((n,), F32, seed + 1)])
    return st, KC.randn_t((2, n), dtype, seed + 2)


def ms_call(ops, gs, epsd, gx, gi, n, guidance, sigma, abc, inv_next, dtype):
    return ops.lib().ss_multistep_cfg_step(gs.data_ptr(), ops.p(epsd), None if gx is None else gx.data_ptr(),
                                           None if gi is None else gi.data_ptr(), n, guidance, sigma, abc[0], abc[1], abc[2],
                                           inv_next, ops.dt(dtype), ops.stream())


def ms_run_check(ops, n, dtype, st, eps, epsd, guidance, sigma, sigma_next, abc, what, offset=0, outs=(True, True)):
    inv = 1.0 / math.sqrt(sigma_next * sigma_next + 1.0)
    gs = KC.GuardedOut(2, n, F32, device=DEV, offset=offset)
    gs.out.copy_(st)
    if abc[2] == 0.0:
        gs.out[1].fill_(float("nan"))               # c == 0: row 1 is not read (it is uninitialised on the first step)
    gx = KC.GuardedOut(1, n, dtype, device=DEV, offset=offset) if outs[0] else None
    gi = KC.GuardedOut(2, n, dtype, device=DEV, offset=offset) if outs[1] else None
    ops.check(ms_call(ops, gs, epsd, gx, gi, n, guidance, sigma, abc, inv, dtype), "ss_multistep_cfg_step")
    ref = ms_bound(st, eps, guidance, sigma, abc[0], abc[1], abc[2], inv, dtype)
    new = gs.check(what + " state")
    KC.check(new[0], *ref["x"], what + " x'", family="multistep x'", dtype=dtype)
    KC.check(new[1], *ref["d"], what + " d", family="multistep d", dtype=dtype)
    if gx is not None:
        KC.check(gx.check(what + " x_out")[0], *ref["x_out"], what + " x_out", family="multistep x_out", dtype=dtype)
    if gi is not None:
        KC.check(gi.check(what + " xin_next"), *ref["xin_next"], what + " xin_next", family="multistep xin_next", dtype=dtype)


# ---- the kernel, element by element ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ALL, ids=dname)
@pytest.mark.parametrize("n", MS_N)
def test_multistep_cfg_step_elementwise(ops, n, dtype):
    """x', d, x_out and xin_next inside the bound, guards untouched, NaN-poisoned row 1 harmless when c == 0: every guidance,
    coefficient set and sigma pair"""
    for k, (sigma, sigma_next) in enumerate(MS_SIGMAS):
        st, eps = ms_inputs(n, dtype, sigma, 700 + 10 * k + n % 89)
        epsd = dev(eps)
        for guidance in MS_GUIDANCE:
            for name, abc in coefficient_sets(sigma, sigma_next).items():
                what = "%s n %d sigma %g -> %g guidance %g %s" % (dname(dtype), n, sigma, sigma_next, guidance, name)
                ms_run_check(ops, n, dtype, st, eps, epsd, guidance, sigma, sigma_next, abc, what)


@pytest.mark.parametrize("dtype", ALL, ids=dname)
@pytest.mark.parametrize("n", [9, 1048576 + 3])
def test_multistep_cfg_step_unaligned_bases(ops, n, dtype):
    """buffers that start one element off a 16-byte boundary take the single-element path for everything: 1048579 elements there
    are one past what one sweep of the capped grid covers"""
    sigma, sigma_next = MS_SIGMAS[0]
    st, eps = ms_inputs(n, dtype, sigma, 760 + n % 89)
    ms_run_check(ops, n, dtype, st, eps, dev(eps), 7.5, sigma, sigma_next, coefficient_sets(sigma, sigma_next)["middle"],
                 "%s n %d unaligned" % (dname(dtype), n), offset=1)


@pytest.mark.parametrize("dtype", ALL, ids=dname)
def test_multistep_cfg_step_null_outputs_and_refusals(ops, dtype):
    n = 257
    sigma, sigma_next = MS_SIGMAS[0]
    st, eps = ms_inputs(n, dtype, sigma, 780)
    epsd = dev(eps)
    abc = coefficient_sets(sigma, sigma_next)["middle"]
    for outs in ((True, False), (False, True), (False, False)):          # each NULL output is skipped, the rest intact
        ms_run_check(ops, n, dtype, st, eps, epsd, 7.5, sigma, sigma_next, abc, "%s outputs %s" % (dname(dtype), outs), outs=outs)
    # a refused call writes nothing
    gs, gx, gi = KC.GuardedOut(2, n, F32, device=DEV), KC.GuardedOut(1, n, dtype, device=DEV), KC.GuardedOut(2, n, dtype, device=DEV)
    gs.out.copy_(st)
    before = gs.flat.clone()
    inv = 1.0 / math.sqrt(sigma_next ** 2 + 1.0)
    nan = float("nan")
    lib = ops.lib()
    bad = [lambda: ms_call(ops, gs, epsd, gx, gi, 0, 7.5, sigma, abc, inv, dtype),
           lambda: ms_call(ops, gs, epsd, gx, gi, -n, 7.5, sigma, abc, inv, dtype),
           lambda: lib.ss_multistep_cfg_step(None, ops.p(epsd), gx.data_ptr(), gi.data_ptr(), n, 7.5, sigma, *abc, inv, ops.dt(dtype), ops.stream()),
           lambda: lib.ss_multistep_cfg_step(gs.data_ptr(), None, gx.data_ptr(), gi.data_ptr(), n, 7.5, sigma, *abc, inv, ops.dt(dtype), ops.stream()),
           lambda: ms_call(ops, gs, epsd, gx, gi, n, 7.5, sigma, (nan, abc[1], abc[2]), inv, dtype),
           lambda: ms_call(ops, gs, epsd, gx, gi, n, 7.5, sigma, (abc[0], float("inf"), abc[2]), inv, dtype),
           lambda: ms_call(ops, gs, epsd, gx, gi, n, 7.5, sigma, (abc[0], abc[1], nan), inv, dtype),
           lambda: ms_call(ops, gs, epsd, gx, gi, n, nan, sigma, abc, inv, dtype),
           lambda: ms_call(ops, gs, epsd, gx, gi, n, 7.5, nan, abc, inv, dtype),
           lambda: ms_call(ops, gs, epsd, gx, gi, n, 7.5, sigma, abc, nan, dtype),
           lambda: lib.ss_multistep_cfg_step(gs.data_ptr(), ops.p(epsd), gx.data_ptr(), gi.data_ptr(), n, 7.5, sigma, *abc, inv, 9, ops.stream())]
    for i, fn in enumerate(bad):
        assert fn() == SS_EINVAL, i
    torch.cuda.synchronize()
    assert torch.equal(gs.flat, before)
    for g in (gx, gi):
        assert bool((g.flat == KC.SENTINEL[dtype]).all())


# ---- whole trajectories in fp32 -------------------------------------------------------------------------------------------------------
def _kernel_run(ops, prob, sigmas, coefs):
    """the kernel driven over a whole run; eps from the analytic model, evaluated in fp32 on the host from the state the kernel left"""
    n = len(prob["noise"])
    x0 = (prob["noise"] * math.sqrt(float(sigmas[0]) ** 2 + 1.0)).astype(np.float32)
    state = torch.zeros(2, n, dtype=torch.float32, device=DEV)
    state[0].copy_(torch.from_numpy(x0))
    eps_fn = R.gaussian_eps(prob, sigmas, np.float32)
    for i in range(len(sigmas) - 1):
        e_u, e_c = eps_fn(state[0].cpu().numpy(), i)
        eps = torch.from_numpy(np.stack([e_u, e_c])).to(DEV)
        a, b, c = (float(v) for v in coefs[i])
        ops.multistep_cfg_step_(state, eps, prob["guidance"], float(sigmas[i]), a, b, c, 1.0 / math.sqrt(float(sigmas[i + 1]) ** 2 + 1.0))
    return state[0].cpu().numpy().astype(np.float64), x0.astype(np.float64)


def test_trajectories_fp32_equal_reference_and_are_second_order(ops):
    prob = R.gaussian_problem()
    err = {}
    for name, n, karras, euler in (("2mk10", 10, True, False), ("2mk15", 15, True, False), ("2mk20", 20, True, False),
                                   ("euler30", 30, False, True)):
        s = R.schedule(n, use_karras_sigmas=karras)
        coefs = R.euler_coefficients(s["sigmas"]) if euler else s["coefficients"]
        got, x0 = _kernel_run(ops, prob, s["sigmas"], coefs)
        ref = R.sample(R.gaussian_eps(prob, s["sigmas"]), x0, s["sigmas"], coefs, prob["guidance"])
        dist = R.rel_rms(got, ref)
        err[name] = R.rel_rms(got, R.gaussian_exact(prob, x0, float(s["sigmas"][0])))
        print("%s: kernel vs dpmpp_ref %.3e, vs the exact end point %.3e" % (name, dist, err[name]))
        assert dist <= 1e-5, name
    assert err["2mk10"] / err["2mk20"] >= 3.0               # (a)
    assert err["2mk15"] <= 0.5 * err["euler30"]             # (b)


# ---- the pipeline on the tiny synthetic UNet ------------------------------------------------------------------------------------------
def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def _models(dtype):
    from seedstory.diffusion import AutoencoderKL, UNet2DConditionModel
    c = S.TINY_UNET
    wd = S.synth_weights(S.unet_shapes(c), 1)
    m = UNet2DConditionModel(c)
    missing, unexpected = m.load_state_dict(wd, strict=False)
    assert not missing and not unexpected
    vae = AutoencoderKL(S.TINY_VAE)
    vae.load_state_dict(S.synth_weights(S.vae_decoder_shapes(S.TINY_VAE), 2))
    return m.to(DEV, dtype), vae.to(DEV, dtype), wd, c


def _cond(B, seed, dtype=torch.float32):
    t = [synth.normal_like(seed, (B, 8, 128), 1.0), synth.normal_like(seed + 1, (B, 8, 128), 1.0), synth.normal_like(seed + 2, (B, 80), 1.0),
         synth.normal_like(seed + 3, (B, 80), 1.0), synth.normal_like(seed + 4, (B, 4, 8, 8), 1.0)]
    return [v.to(dtype) for v in t]


def _render(pipe, cond, steps, output_type="latent", sl=slice(None)):
    cp, cn, pp, pn, noise = (v[sl].to(DEV) for v in cond)
    return pipe(prompt_embeds=cp, negative_prompt_embeds=cn, pooled_prompt_embeds=pp, negative_pooled_prompt_embeds=pn, latents=noise,
                guidance_scale=7.5, num_inference_steps=steps, height=64, width=64, output_type=output_type).images


def _ref_latents(wd, c, cond, steps, karras=True, guidance=7.5, size=64):
    """dpmpp_ref's loop over the oracle's UNet (fp32 on the CPU)"""
    cp, cn, pp, pn, noise = cond
    sch = R.schedule(steps, use_karras_sigmas=karras)
    sig, ts = sch["sigmas"], sch["timesteps"]
    B = noise.shape[0]
    ids = torch.tensor([[size, size, 0, 0, size, size]] * (2 * B), dtype=noise.dtype)
    ctx, pooled = torch.cat([cn, cp], dim=0), torch.cat([pn, pp], dim=0)

    def eps_fn(x, i):
        xin = torch.cat([x, x], dim=0) / math.sqrt(float(sig[i]) ** 2 + 1.0)
        e_neg, e_pos = S.unet_forward(wd, c, xin, float(ts[i]), ctx, pooled, ids).chunk(2)
        return e_neg, e_pos
    return R.sample(eps_fn, noise * sch["init_noise_sigma"], sig, sch["coefficients"], guidance)


@pytest.fixture(scope="module")
def tiny():
    from seedstory.diffusion import DPMSolverMultistepScheduler, StableDiffusionXLPipeline
    m, vae, wd, c = _models(torch.float32)
    pipe = StableDiffusionXLPipeline(vae=vae, unet=m, scheduler=DPMSolverMultistepScheduler(use_karras_sigmas=True))
    return pipe, m, vae, wd, c


def test_pipeline_equals_reference_loop(tiny):
    """64 x 64, 6 steps, Karras, g = 7.5, fp32: the project's own bound for this UNet under Euler (the solver adds fp32 point-wise
    arithmetic only); output_type="pt" gives the uint8 image"""
    pipe, m, vae, wd, c = tiny
    cond = _cond(1, 30)
    ref = _ref_latents(wd, c, cond, 6)
    out = _render(pipe, cond, 6)
    print("pipeline vs dpmpp_ref over the oracle UNet: %.3e" % rel(out, ref))
    assert out.shape == ref.shape and rel(out, ref) < 5e-4
    img = _render(pipe, cond, 6, output_type="pt")
    assert img.dtype == torch.uint8 and img.shape == (64, 64, 3)
    ref_img = S.postprocess(S.vae_decode(S.synth_weights(S.vae_decoder_shapes(S.TINY_VAE), 2), S.TINY_VAE, ref))[0]
    assert (img.cpu().float() - ref_img.float()).abs().mean() < 1.0       # uint8 levels


def test_pipeline_graph_replay_is_bit_equal_to_eager(tiny):
    from seedstory import _lib
    pipe, m, vae, wd, c = tiny
    cond = _cond(2, 230)
    outs = {}
    for mode in (1, 0):
        _lib.set_tuning("unet_graph", mode)
        try:
            outs[mode] = _render(pipe, cond, 4).clone()
            if mode == 1:
                assert any(v is not None for v in pipe._graphs.values()), "graph path was not taken"
        finally:
            _lib.set_tuning("unet_graph", 1)
    assert torch.equal(outs[1], outs[0])


def test_pipeline_batch_equals_single_calls(tiny):
    pipe, m, vae, wd, c = tiny
    cond = _cond(3, 130)
    lat = _render(pipe, cond, 4)
    assert lat.shape == (3, 4, 8, 8)
    for b in range(3):
        one = _render(pipe, cond, 4, sl=slice(b, b + 1))
        assert rel(lat[b:b + 1], one) < 2e-4, b


def test_knob_on_an_euler_object_equals_the_explicit_scheduler(tiny):
    from seedstory import _lib
    from seedstory.diffusion import EulerDiscreteScheduler, StableDiffusionXLPipeline
    pipe, m, vae, wd, c = tiny
    cond = _cond(1, 330)
    explicit = _render(pipe, cond, 5).clone()
    other = StableDiffusionXLPipeline(vae=vae, unet=m, scheduler=EulerDiscreteScheduler())
    euler = _render(other, cond, 5).clone()
    try:
        _lib.set_tuning("sdxl_solver", 3)
        knob = _render(other, cond, 5).clone()
    finally:
        _lib.set_tuning("sdxl_solver", 0)
    assert torch.equal(knob, explicit)
    assert rel(euler, explicit) > 1e-3                      # and the knob really changed the sampler
    assert torch.equal(_render(other, cond, 5), euler)      # off again: Euler's bits


def test_pipeline_bf16_distance_against_eulers():
    """bf16 latents against the same sampler's fp32 run: no more than twice what the Euler pipeline (the parent's code) loses on the
    same inputs and step count — the margin covers one more rounded output per step"""
    from seedstory.diffusion import DPMSolverMultistepScheduler, EulerDiscreteScheduler, StableDiffusionXLPipeline
    steps = 6
    lat = {}
    for dtype in (torch.float32, BF):
        m, vae, wd, c = _models(dtype)
        cd = _cond(1, 430, dtype)
        for name, sched in (("euler", EulerDiscreteScheduler()), ("dpmpp", DPMSolverMultistepScheduler(use_karras_sigmas=True))):
            lat[name, dtype] = _render(StableDiffusionXLPipeline(vae=vae, unet=m, scheduler=sched), cd, steps).float().cpu()
    d_euler = rel(lat["euler", BF], lat["euler", torch.float32])
    d_dpmpp = rel(lat["dpmpp", BF], lat["dpmpp", torch.float32])
    print("bf16 vs fp32 latents, %d steps: Euler %.3e, DPM++ 2M Karras %.3e (ratio %.2f)" % (steps, d_euler, d_dpmpp, d_dpmpp / d_euler))
    assert d_dpmpp <= 2.0 * d_euler


def test_zz_worst_ratios():
    print("\n" + KC.worst_table({"multistep x'", "multistep d", "multistep x_out", "multistep xin_next"}))

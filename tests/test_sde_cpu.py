"""Host side of the stochastic samplers (no GPU): the reference noise's moments and independence, the coefficient identities, the
two scheduler classes against ``tests/sde_ref.py``, convergence on a Gaussian problem by exact moment propagation, the C ABI's
surface and refusals, the drivers' ``--scheduler`` names, ``noise_seed`` and the per-image ``seed`` of ``SDXLAdapter.generate``.

Convergence (``sde_ref.gaussian_end_std``: the covariance of (x, d_prev) through the linear recurrence, fp64, no sampling), relative
error of the end-point standard deviation on Karras sigmas at 10 / 20 / 40 / 80 steps:
    2M SDE           sigma_d 1: 7.8e-2 / 2.5e-2 / 5.5e-3 / 5.4e-4      sigma_d 2: 7.7e-2 / 2.1e-2 / 5.1e-3 / 9.4e-4
    Euler ancestral  sigma_d 1: 0.233 / 0.135 / 0.073 / 0.036          sigma_d 2: 0.215 / 0.123 / 0.066 / 0.033
"""
import argparse
import ctypes as C
import math
import os

import numpy as np
import pytest

import dpmpp_ref as R
import sde_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SS_EINVAL = -1


# ---- noise ----------------------------------------------------------------------------------------------------------------------------
def test_noise_moments():
    """2^20 reference normals: mean and variance within 5 standard errors, |z| <= 5.77"""
    N = 1 << 20
    z = S.noise([0x1234567887654321], 7, N)[0]
    mean, var = float(z.mean()), float(z.var())
    print("mean %.3e (5 se %.3e), var - 1 %.3e (5 se %.3e), max |z| %.3f" % (mean, 5 / math.sqrt(N), var - 1, 5 * math.sqrt(2 / N), np.abs(z).max()))
    assert abs(mean) <= 5.0 / math.sqrt(N)
    assert abs(var - 1.0) <= 5.0 * math.sqrt(2.0 / N)
    assert np.abs(z).max() <= 5.77 and np.isfinite(z).all()
    # the cos and the sin lanes, and the two pairs of a quad, are not correlated
    q = z.reshape(-1, 4)
    for a, b in ((0, 1), (0, 2), (1, 3), (2, 3)):
        assert abs(float(np.mean(q[:, a] * q[:, b]))) <= 5.0 / math.sqrt(N / 4)


def test_noise_depends_on_seed_words_step_and_index():
    j = np.arange(64)
    seed = 0x0000000500000009
    base = S.normals(seed, 3, j)
    assert np.array_equal(base, S.normals(seed, 3, j))
    for other in (S.normals(seed + 1, 3, j), S.normals(seed + (1 << 32), 3, j), S.normals(seed, 4, j)):
        assert (other != base).all()
    assert len(set(base.tolist())) == 64                                 # every j its own value
    assert (S.normals(seed & 0xFFFFFFFF, 3, j) != base).all()            # the high word is part of the key
    # counter word 2 = 1: not the token sampler's stream
    from test_sampling_cpu import philox4x32_10
    w_tok = philox4x32_10((0, 3, 0, 0), (seed & 0xFFFFFFFF, seed >> 32))
    u = S.uniform_parts(seed, 3, np.array([0]))
    assert all(float(u[k][0]) != float(int(w_tok[k]) >> 8) * 2.0 ** -24 for k in range(4))
    # rows of equal seeds are equal, a row does not depend on its neighbours
    z = S.noise([5, 6, 5], 2, 37)
    assert np.array_equal(z[0], z[2]) and np.array_equal(z[1], S.noise([6], 2, 37)[0]) and (z[0] != z[1]).all()


# ---- coefficients -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("karras", [False, True])
@pytest.mark.parametrize("n", [1, 2, 10, 20, 30])
def test_coefficient_identities(n, karras):
    sig = R.schedule(n, use_karras_sigmas=karras)["sigmas"]
    tables = {"euler-a": S.euler_ancestral_coefficients(sig)}
    for eta in (0.0, 0.5, 1.0, 2.0):
        for order in (1, 2):
            tables["2m-sde eta %g order %d" % (eta, order)] = S.dpmpp_2m_sde_coefficients(sig, eta, order)
    for name, t in tables.items():
        assert t.shape == (n, 4)
        assert np.abs(t[:, :3].sum(axis=1) - 1.0).max() <= 1e-12, name                                   # a + b + c = 1
        lhs = t[:, 0] ** 2 * sig[:n] ** 2 + t[:, 3] ** 2
        assert np.abs(lhs - sig[1:] ** 2).max() <= 1e-12 * max(1.0, float(sig[0]) ** 2), name            # a^2 s_i^2 + s^2 = s_n^2
        assert tuple(t[n - 1]) == (0.0, 1.0, 0.0, 0.0), name
    for order in (1, 2):
        t0 = S.dpmpp_2m_sde_coefficients(sig, 0.0, order)
        assert np.abs(t0[:, :3] - R.coefficients(sig, order)).max() <= 1e-12 and (t0[:, 3] == 0.0).all()
    ea = tables["euler-a"]
    assert (ea[:, 2] == 0.0).all() and (ea[:n - 1, 3] > 0.0).all()


@pytest.mark.parametrize("karras", [False, True])
def test_sde_class_equals_reference(karras):
    from seedstory.diffusion import DPMSolverMultistepSDEScheduler
    for n in (1, 6, 20):
        for eta, order in ((1.0, 2), (0.5, 2), (1.0, 1), (0.0, 2)):
            m = DPMSolverMultistepSDEScheduler(use_karras_sigmas=karras, solver_order=order, eta=eta)
            m.set_timesteps(n)
            ref = S.schedule(n, "2m-sde", use_karras_sigmas=karras, eta=eta, solver_order=order)
            assert m.coefficients.shape == (n, 4)
            np.testing.assert_allclose(m.sigmas, ref["sigmas"], rtol=1e-6)
            np.testing.assert_allclose(m.coefficients, ref["coefficients"], rtol=1e-6, atol=1e-12)
            np.testing.assert_allclose(m.timesteps, ref["timesteps"], rtol=0, atol=0)
            assert abs(m.init_noise_sigma - ref["init_noise_sigma"]) <= 1e-6 * ref["init_noise_sigma"]


def test_euler_ancestral_class_equals_reference():
    from seedstory.diffusion import EulerAncestralDiscreteScheduler, EulerDiscreteScheduler
    for n in (1, 6, 30):
        m = EulerAncestralDiscreteScheduler()
        m.set_timesteps(n)
        ref = S.schedule(n, "euler-a")
        e = EulerDiscreteScheduler()
        e.set_timesteps(n)
        assert m.coefficients.shape == (n, 4)
        np.testing.assert_allclose(m.sigmas, ref["sigmas"], rtol=1e-6)
        np.testing.assert_allclose(m.coefficients, ref["coefficients"], rtol=1e-6, atol=1e-12)
        assert np.array_equal(m.timesteps, e.timesteps) and m.init_noise_sigma == e.init_noise_sigma
        assert np.array_equal(m.sigmas.astype(np.float32), e.sigmas)


def test_construction_paths(tmp_path):
    import json
    from seedstory.diffusion import (DPMSolverMultistepScheduler, DPMSolverMultistepSDEScheduler, EulerAncestralDiscreteScheduler,
                                     EulerDiscreteScheduler)
    os.makedirs(tmp_path / "scheduler")
    cfg = {"_class_name": "EulerDiscreteScheduler", "num_train_timesteps": 1000, "beta_start": 0.00085, "beta_end": 0.012,
           "beta_schedule": "scaled_linear", "timestep_spacing": "trailing", "steps_offset": 1, "prediction_type": "epsilon"}
    with open(tmp_path / "scheduler" / "scheduler_config.json", "w") as f:
        json.dump(cfg, f)
    base = EulerDiscreteScheduler.from_pretrained(str(tmp_path), subfolder="scheduler")
    ref = S.schedule(8, "2m-sde", use_karras_sigmas=True, timestep_spacing="trailing")
    for m in (DPMSolverMultistepSDEScheduler.from_pretrained(str(tmp_path), subfolder="scheduler", use_karras_sigmas=True),
              DPMSolverMultistepSDEScheduler.from_base(base, use_karras_sigmas=True),
              DPMSolverMultistepSDEScheduler.from_base(DPMSolverMultistepScheduler.from_base(base), use_karras_sigmas=True)):
        m.set_timesteps(8)
        np.testing.assert_allclose(m.coefficients, ref["coefficients"], rtol=1e-6, atol=1e-12)
    ref = S.schedule(8, "euler-a", timestep_spacing="trailing")
    for m in (EulerAncestralDiscreteScheduler.from_pretrained(str(tmp_path), subfolder="scheduler"),
              EulerAncestralDiscreteScheduler.from_base(base),
              EulerAncestralDiscreteScheduler.from_base(DPMSolverMultistepSDEScheduler.from_base(base))):
        m.set_timesteps(8)
        np.testing.assert_allclose(m.coefficients, ref["coefficients"], rtol=1e-6, atol=1e-12)
    for bad in (dict(eta=-1.0), dict(eta=float("nan")), dict(eta="1"), dict(solver_order=3), dict(algorithm_type="dpmsolver++"),
                dict(solver_type="heun"), dict(thresholding=True), dict(no_such_key=1)):
        with pytest.raises(ValueError):
            DPMSolverMultistepSDEScheduler(**bad)
    with pytest.raises(ValueError):                       # the deterministic class does not grow the option
        DPMSolverMultistepScheduler(algorithm_type="sde-dpmsolver++")


# ---- convergence ----------------------------------------------------------------------------------------------------------------------
def test_convergence_by_moment_propagation():
    """the end point's standard deviation against sigma_d (see the module docstring): 2M SDE is second order, ancestral first"""
    for sigma_d in (1.0, 2.0):
        err = {smp: [S.gaussian_std_error(n, smp, sigma_d) for n in (10, 20, 40, 80)] for smp in ("2m-sde", "euler-a")}
        for smp, e in err.items():
            print("sigma_d %g %s: %s" % (sigma_d, smp, " / ".join("%.3g" % v for v in e)))
            assert e[0] > e[1] > e[2] > e[3], (smp, sigma_d, e)
        assert err["2m-sde"][1] / err["2m-sde"][2] >= 3.0
        assert 1.5 <= err["euler-a"][1] / err["euler-a"][2] <= 2.5


def test_reference_loop_adds_the_noise_of_each_step():
    """sde_ref.sample by hand on two images with different seeds; s = 0 everywhere is guidance_ref.sample"""
    import guidance_ref as G
    s = S.schedule(6, "2m-sde", use_karras_sigmas=True)
    sig, coefs = s["sigmas"], s["coefficients"]
    prob = R.gaussian_problem(n=64)
    both = R.gaussian_eps(prob, sig)

    def eps_fn(x, i, guided):
        e_u, e_c = both(x, i)
        return (e_u, e_c) if guided else e_c
    x0 = prob["noise"] * s["init_noise_sigma"]
    seeds = [11, 12]
    got = S.sample(eps_fn, x0, sig, coefs, 7.5, (0.3, 3.0), seeds, 32)
    mask = G.mask(sig[:6], (0.3, 3.0))
    x, dp = x0, None
    for i in range(6):
        e_u, e_c = both(x, i)
        x, dp = R.step(x, dp, e_u if mask[i] else e_c, e_c, 7.5, float(sig[i]), coefs[i][:3])
        x = x + coefs[i][3] * np.concatenate([S.normals(sd, i, np.arange(32)) for sd in seeds])
    assert np.array_equal(got, x)
    assert not np.array_equal(got, S.sample(eps_fn, x0, sig, coefs, 7.5, (0.3, 3.0), [11, 13], 32))
    det = np.concatenate([R.coefficients(sig), np.zeros((6, 1))], axis=1)
    assert np.array_equal(S.sample(eps_fn, x0, sig, det, 7.5, (0.3, 3.0), seeds, 32), G.sample(eps_fn, x0, sig, det[:, :3], 7.5, (0.3, 3.0)))


# ---- interface ------------------------------------------------------------------------------------------------------------------------
def test_abi_declares_and_refuses_before_any_device_call():
    from seedstory import _lib
    with open(os.path.join(ROOT, "include", "seedstory_hip.h")) as f:
        header = f.read()
    assert "#define SS_ABI_VERSION 1" in header
    for name in ("ss_randn_philox", "ss_multistep_noise_step"):
        assert name + "(" in header and name in _lib.PROTOTYPES, name
    lib = _lib.lib()
    err = lambda: lib.ss_last_error().decode()  # noqa: E731
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    ok = (7.5, 1.0, 0.5, 0.5, 0.0, 0.25, 1.0)             # guidance, sigma, a, b, c, s, inv_next

    def step(state=p, eps=p, n=8, rows=(1, 1), vals=ok, seeds=p, n_img=8, step_=0, dtype=_lib.SS_F32):
        return lib.ss_multistep_noise_step(state, eps, p, p, n, rows[0], rows[1], *vals, seeds, n_img, step_, dtype, None)
    assert step(state=None) == SS_EINVAL and "NULL" in err()
    assert step(eps=None) == SS_EINVAL and "NULL" in err()
    assert step(n=0) == SS_EINVAL and "n = 0" in err()
    assert step(n=-3) == SS_EINVAL and "n = -3" in err()
    for n_img in (0, -1, 3, 16):
        assert step(n_img=n_img) == SS_EINVAL and "n_img" in err(), n_img
    assert step(step_=-1) == SS_EINVAL and "step" in err()
    assert step(seeds=None) == SS_EINVAL and "seeds" in err()
    for rows in ((0, 2), (3, 2), (2, 0), (1, 3), (-1, 1)):
        assert step(rows=rows) == SS_EINVAL and "rows" in err(), rows
    for k in range(7):
        for bad in (float("nan"), float("inf")):
            vals = list(ok)
            vals[k] = bad
            assert step(vals=vals) == SS_EINVAL and "non-finite" in err(), (k, bad)
    assert step(dtype=7) == SS_EINVAL and "dtype" in err()
    rp = lib.ss_randn_philox
    assert rp(None, p, 1, 8, 0, _lib.SS_F32, None) == SS_EINVAL and "NULL" in err()
    assert rp(p, None, 1, 8, 0, _lib.SS_F32, None) == SS_EINVAL and "NULL" in err()
    assert rp(p, p, 0, 8, 0, _lib.SS_F32, None) == SS_EINVAL and "batch" in err()
    assert rp(p, p, 1, 0, 0, _lib.SS_F32, None) == SS_EINVAL and "n_img" in err()
    assert rp(p, p, 1, 8, -1, _lib.SS_F32, None) == SS_EINVAL and "step" in err()
    assert rp(p, p, 1, 8, 0, 7, None) == SS_EINVAL and "dtype" in err()
    assert all(v == 0.0 for v in buf)                          # nothing was written


def test_ops_wrappers_check_their_arguments():
    import torch
    from seedstory import _lib, ops
    t = torch.zeros(2, 8)
    sd = torch.zeros(1, dtype=torch.int64)
    for fn in (lambda: ops.multistep_noise_step_(t, t, 7.5, 1.0, 0.5, 0.5, 0.0, 0.1, 1.0, sd, 0),
               lambda: ops.randn_philox(sd, 8, 0, torch.float32)):
        with pytest.raises(_lib.SSError, match="GPU"):        # no CPU path
            fn()
    got = ops.noise_seeds([0, 1, 2 ** 63, 2 ** 64 - 1, -1, 2 ** 64 + 5], "cpu")
    assert got.dtype == torch.int64 and got.tolist() == [0, 1, -2 ** 63, -1, -1, 5]
    assert ops.noise_seeds(7, "cpu").tolist() == [7]


@pytest.mark.parametrize("driver", ("gen_george", "vis_george_sink"))
def test_driver_scheduler_names(driver, monkeypatch):
    import importlib
    import sys
    from seedstory.diffusion import DPMSolverMultistepSDEScheduler, EulerAncestralDiscreteScheduler
    from src.inference.gen_george import make_scheduler
    mod = importlib.import_module("src.inference." + driver)
    seen = {}

    class Stop(Exception):
        pass

    def fake_build(args, device, dtype):
        seen["args"] = args
        raise Stop()

    monkeypatch.setattr(mod, "build", fake_build)
    for name in ("euler-a", "dpmpp2m-sde", "dpmpp2m-sde-karras"):
        monkeypatch.setattr(sys, "argv", [driver, "--scheduler", name])
        with pytest.raises(Stop):
            mod.main()
        assert seen["args"].scheduler == name
        s = make_scheduler(seen["args"])
        if name == "euler-a":
            assert type(s) is EulerAncestralDiscreteScheduler
        else:
            assert type(s) is DPMSolverMultistepSDEScheduler and s.use_karras_sigmas == name.endswith("karras") and s.eta == 1.0
    for bad in ("heun", "dpmpp2m-sde-k", "euler_a"):
        monkeypatch.setattr(sys, "argv", [driver, "--scheduler", bad])
        with pytest.raises(SystemExit):
            mod.main()
    with pytest.raises(SystemExit):
        make_scheduler(argparse.Namespace(scheduler="dpm-sde"))


def test_noise_seed_resolution_and_refusal_before_any_launch():
    import torch
    from seedstory.diffusion import EulerAncestralDiscreteScheduler, EulerDiscreteScheduler, StableDiffusionXLPipeline, noise_seed_list
    g = torch.Generator().manual_seed(99)
    assert noise_seed_list(None, None, 3) == [0, 0, 0]
    assert noise_seed_list(None, g, 2) == [99, 99]
    assert noise_seed_list(5, g, 2) == [5, 5]
    assert noise_seed_list((1, 2 ** 40), None, 2) == [1, 2 ** 40]
    assert noise_seed_list(np.array([3, 4]), None, 2) == [3, 4]
    for bad in ((1, 2, 3), [], "ab", 1.5):
        with pytest.raises(ValueError):
            noise_seed_list(bad, None, 2)
    e = torch.zeros(2, 4, 8)
    for sched in (EulerAncestralDiscreteScheduler(), EulerDiscreteScheduler()):     # no device is needed to be refused
        pipe = StableDiffusionXLPipeline(vae=None, unet=None, scheduler=sched)
        with pytest.raises(ValueError, match="noise_seed"):
            pipe(e, e, e[:, 0], e[:, 0], noise_seed=[1, 2, 3])
        assert pipe.last_guidance is None


def test_generate_per_image_seeds_on_a_stub_pipeline():
    """seed = (s0, s1, s0): image b starts from the latents a batch-1 call with seed[b] draws and takes seed[b] as its noise seed;
    an int behaves as before (one draw repeated, the generator handed on, no noise_seed keyword)"""
    import torch
    from src.models_ipa.adapter_modules import SDXLAdapter
    calls = []

    class Out:
        images = "images"

    def pipe(**kw):
        calls.append(kw)
        return Out()

    ad = SDXLAdapter(unet=None, resampler=None)
    ad.device, ad.sdxl_pipe = "cpu", pipe

    def embeds(B):
        e, pe = torch.zeros(B, 4, 8), torch.zeros(B, 8)
        ad.get_image_embeds = lambda **kw: (e, e, pe, pe)
    embeds(3)
    assert ad.generate(image_embeds=0, seed=(7, 8, 7), height=64, width=64) == "images"
    kw = calls.pop()
    assert kw["noise_seed"] == [7, 8, 7] and kw["generator"] is None and kw["latents"].shape == (3, 4, 8, 8)
    for b, sd in enumerate((7, 8, 7)):
        embeds(1)
        ad.generate(image_embeds=0, seed=sd, height=64, width=64)
        one = calls.pop()
        assert "noise_seed" not in one and "latents" not in one and one["generator"].initial_seed() == sd
        want = torch.randn((1, 4, 8, 8), generator=torch.Generator("cpu").manual_seed(sd))
        assert torch.equal(kw["latents"][b:b + 1], want), b
    embeds(3)
    ad.generate(image_embeds=0, seed=7, height=64, width=64)                     # an int: as before
    kw = calls.pop()
    assert "noise_seed" not in kw and kw["generator"].initial_seed() == 7
    assert torch.equal(kw["latents"], torch.randn((1, 4, 8, 8), generator=torch.Generator("cpu").manual_seed(7)).repeat(3, 1, 1, 1))
    with pytest.raises(ValueError):
        ad.generate(image_embeds=0, seed=(1, 2), height=64, width=64)
    lat = torch.ones(3, 4, 8, 8)
    ad.generate(image_embeds=0, seed=[1, 2, 3], height=64, width=64, latents=lat)       # the caller's latents are kept
    assert calls.pop()["latents"] is lat


def test_no_new_knob_and_the_solver_knob_still_refuses_1():
    from seedstory import _lib
    from seedstory.diffusion import EulerDiscreteScheduler, StableDiffusionXLPipeline
    pipe = StableDiffusionXLPipeline(vae=None, unet=None, scheduler=EulerDiscreteScheduler())
    _lib.set_tuning("sdxl_solver", 1)
    try:
        with pytest.raises(_lib.SSError):
            pipe._sampler()
    finally:
        _lib.set_tuning("sdxl_solver", 0)

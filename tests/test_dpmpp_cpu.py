"""Host side of the DPM-Solver++ 2M sampler (no GPU): ``tests/dpmpp_ref.py`` against an exact solution, the
``DPMSolverMultistepScheduler`` class against ``dpmpp_ref``, the config keys it refuses, the knob, the C ABI's refusals and the
drivers' ``--scheduler`` argument.

The exact solution: per element the data are N(mu, s^2), so eps(x, sigma; mu) = sigma (x - mu) / (s^2 + sigma^2), CFG over two
means is the same eps at mu_u + g (mu_c - mu_u), and the probability-flow ODE from x_start at sigma_0 ends at
mu + (x_start - mu) s / sqrt(s^2 + sigma_0^2).  4096 elements, mu_u ~ N(0, 0.3), mu_c ~ N(0.2, 0.5), s ~ U(0.2, 1), g = 7.5;
relative RMS error of the end point (fp64; the fp32 loop gives the same figures to three digits):

    2M Karras   10 / 15 / 20 / 30 steps    6.3e-3 / 2.7e-3 / 1.4e-3 / 5e-4     (second order: 10 -> 20 steps divides by ~4.5)
    Euler, its own schedule, 30 steps      9.9e-3                              (10 -> 20 steps: 2.8e-2 -> 1.4e-2, first order)
    2M, NON-Karras leading schedule, 20    1.06e-2: does NOT beat Euler at 30 — recorded (printed), not asserted; it is why the
                                           recommended switch is the Karras one
"""
import argparse
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

import dpmpp_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SS_EINVAL = -1
NS = (1, 2, 3, 15, 30)


# ---- the solver against the exact solution -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def problem():
    return R.gaussian_problem()


def _err(problem, n, karras, euler=False, dtype=np.float64, euler_on_karras=False):
    s = R.schedule(n, use_karras_sigmas=karras or euler_on_karras)
    coefs = R.euler_coefficients(s["sigmas"]) if euler or euler_on_karras else s["coefficients"]
    return R.gaussian_error(problem, s["sigmas"], coefs, dtype)


def test_second_order_on_the_exact_solution(problem):
    e = {n: _err(problem, n, True) for n in (10, 15, 20, 30)}
    eu = {n: _err(problem, n, False, euler=True) for n in (10, 20, 30)}
    euk = _err(problem, 30, False, euler_on_karras=True)
    plain20 = _err(problem, 20, False)
    print("2M Karras %s | Euler %s | Euler on Karras sigmas, 30: %.3g | 2M non-Karras, 20: %.3g (Euler 30: %.3g)"
          % ({n: "%.3g" % v for n, v in e.items()}, {n: "%.3g" % v for n, v in eu.items()}, euk, plain20, eu[30]))
    assert e[10] / e[20] >= 3.0                          # (a) second order: ~4 (Euler: 1.9)
    assert eu[10] / eu[20] < 2.5                         # ... and the yardstick itself is first order
    assert e[15] <= 0.5 * eu[30]                         # (b) 15 steps of 2M Karras beat 30 Euler steps on Euler's own schedule
    assert e[30] < e[20] < e[15] < e[10]


def test_fp32_loop_gives_the_same_figures(problem):
    for n in (10, 20):
        a, b = _err(problem, n, True), _err(problem, n, True, dtype=np.float32)
        assert abs(a - b) <= 5e-3 * a, (n, a, b)


# ---- the class against the reference file ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", (1, 2))
@pytest.mark.parametrize("karras", (False, True))
@pytest.mark.parametrize("n", NS)
def test_class_equals_reference(n, karras, order):
    from seedstory.diffusion import DPMSolverMultistepScheduler
    m = DPMSolverMultistepScheduler(use_karras_sigmas=karras, solver_order=order)
    m.set_timesteps(n)
    ref = R.schedule(n, use_karras_sigmas=karras, solver_order=order)
    sig, ts, coef = np.asarray(m.sigmas, dtype=np.float64), np.asarray(m.timesteps, dtype=np.float64), np.asarray(m.coefficients)
    assert sig.shape == (n + 1,) and ts.shape == (n,) and coef.shape == (n, 3)
    np.testing.assert_allclose(sig, ref["sigmas"], rtol=1e-6, atol=0)
    np.testing.assert_allclose(ts, ref["timesteps"], rtol=1e-6, atol=0)
    np.testing.assert_allclose(coef, ref["coefficients"], rtol=1e-6, atol=0)
    assert abs(m.init_noise_sigma - ref["init_noise_sigma"]) <= 1e-6 * ref["init_noise_sigma"]
    assert m.init_noise_sigma == pytest.approx(math.sqrt(sig[0] ** 2 + 1.0), rel=1e-12)
    assert sig[-1] == 0.0 and np.all(np.diff(sig) < 0)                     # strictly decreasing to a final 0
    assert np.all(ts == np.round(ts)) and ts.min() >= 0 and ts.max() <= 999 and np.all(np.diff(ts) <= 0)
    assert tuple(coef[-1]) == (0.0, 1.0, 0.0)                              # the last step is x <- d
    assert np.all(coef[:, 2] == 0) if (order == 1 or n <= 2) else np.all(coef[1:-1, 2] < 0)
    assert coef[0, 2] == 0.0                                               # the first step never reads d_prev
    for i in range(n - 1):                                                 # a + b + c = 1 before the last step: a fixed point stays
        assert abs(coef[i].sum() - 1.0) < 1e-12


def test_one_and_two_steps():
    from seedstory.diffusion import DPMSolverMultistepScheduler
    for karras in (False, True):
        m = DPMSolverMultistepScheduler(use_karras_sigmas=karras)
        m.set_timesteps(1)
        assert m.coefficients.tolist() == [[0.0, 1.0, 0.0]] and len(m.sigmas) == 2      # a single step with x = d
        m.set_timesteps(2)
        assert np.all(m.coefficients[:, 2] == 0)                                        # both steps first order
        s0, s1 = m.sigmas[0], m.sigmas[1]
        assert m.coefficients[0].tolist() == pytest.approx([s1 / s0, 1.0 - s1 / s0, 0.0], rel=1e-12)


def test_base_schedule_is_eulers():
    """without Karras sigmas the table IS EulerDiscreteScheduler's; with them its end points and count"""
    from seedstory.diffusion import DPMSolverMultistepScheduler, EulerDiscreteScheduler
    for spacing in ("leading", "linspace", "trailing"):
        for n in NS:
            e = EulerDiscreteScheduler(timestep_spacing=spacing)
            e.set_timesteps(n)
            m = DPMSolverMultistepScheduler(timestep_spacing=spacing)
            m.set_timesteps(n)
            assert np.array_equal(np.asarray(m.sigmas, dtype=np.float32), e.sigmas) and np.array_equal(m.timesteps, e.timesteps)
            k = DPMSolverMultistepScheduler(timestep_spacing=spacing, use_karras_sigmas=True)
            k.set_timesteps(n)
            assert k.sigmas[0] == pytest.approx(float(e.sigmas[0]), rel=1e-12) and k.sigmas[n - 1] == pytest.approx(float(e.sigmas[n - 1]), rel=1e-12)
            f = DPMSolverMultistepScheduler.from_base(e, use_karras_sigmas=True)
            f.set_timesteps(n)
            assert np.array_equal(f.sigmas, k.sigmas) and np.array_equal(f.coefficients, k.coefficients)


def test_euler_outputs_unchanged():
    """the 30-step table the kernel tests quote (tests/kernel_check.py EULER_SIGMAS)"""
    from seedstory.diffusion import EulerDiscreteScheduler
    e = EulerDiscreteScheduler()
    e.set_timesteps(30)
    assert e.sigmas.dtype == np.float32 and len(e.sigmas) == 31
    # (that table was written in fp64; the class's fp32 betas sit 1e-6 relative from it)
    assert float(e.sigmas[0]) == pytest.approx(11.476846458, rel=1e-5) and float(e.sigmas[29]) == pytest.approx(0.041314412, rel=1e-5)
    assert e.init_noise_sigma == pytest.approx(math.sqrt(float(e.sigmas[0]) ** 2 + 1), rel=1e-7)


# ---- config keys ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,value", [("algorithm_type", "sde-dpmsolver++"), ("algorithm_type", "dpmsolver"), ("solver_order", 3),
                                       ("solver_order", 0), ("solver_type", "heun"), ("prediction_type", "v_prediction"),
                                       ("thresholding", True), ("final_sigmas_type", "sigma_min"), ("beta_schedule", "linear"),
                                       ("use_lu_lambdas", True), ("euler_at_final", True), ("trained_betas", [0.1, 0.2]),
                                       ("variance_type", "learned"), ("timestep_spacing", "karras"), ("no_such_key", 1)])
def test_rejected_config_keys_raise(key, value):
    from seedstory.diffusion import DPMSolverMultistepScheduler
    with pytest.raises(ValueError, match=key):
        DPMSolverMultistepScheduler(**{key: value})


def test_from_pretrained_round_trip(tmp_path):
    from seedstory.diffusion import DPMSolverMultistepScheduler
    cfg = {"_class_name": "DPMSolverMultistepScheduler", "_diffusers_version": "0.25.0", "algorithm_type": "dpmsolver++",
           "beta_end": 0.012, "beta_schedule": "scaled_linear", "beta_start": 0.00085, "dynamic_thresholding_ratio": 0.995,
           "euler_at_final": False, "final_sigmas_type": "zero", "lower_order_final": True, "num_train_timesteps": 1000,
           "prediction_type": "epsilon", "sample_max_value": 1.0, "solver_order": 2, "solver_type": "midpoint", "steps_offset": 1,
           "thresholding": False, "timestep_spacing": "leading", "trained_betas": None, "use_karras_sigmas": True,
           "use_lu_lambdas": False, "variance_type": None}
    os.makedirs(tmp_path / "scheduler")
    with open(tmp_path / "scheduler" / "scheduler_config.json", "w") as f:
        json.dump(cfg, f)
    m = DPMSolverMultistepScheduler.from_pretrained(str(tmp_path), subfolder="scheduler")
    assert m.use_karras_sigmas and m.solver_order == 2
    m.set_timesteps(15)
    ref = R.schedule(15, use_karras_sigmas=True)
    np.testing.assert_allclose(m.sigmas, ref["sigmas"], rtol=1e-6)
    np.testing.assert_allclose(m.coefficients, ref["coefficients"], rtol=1e-6)
    cfg["algorithm_type"] = "sde-dpmsolver++"
    with open(tmp_path / "scheduler" / "scheduler_config.json", "w") as f:
        json.dump(cfg, f)
    with pytest.raises(ValueError, match="algorithm_type"):
        DPMSolverMultistepScheduler.from_pretrained(str(tmp_path), subfolder="scheduler")


# ---- knob, C ABI, drivers ------------------------------------------------------------------------------------------------------------
def test_knob_is_declared_with_default_off():
    from seedstory import _lib
    assert _lib.get_tuning("sdxl_solver", -5) == 0
    with open(os.path.join(ROOT, "seed-story_amd", "csrc", "ss_knobs.h")) as f:
        assert "K_COUNT == 47" in f.read()


def test_pipeline_sampler_follows_the_knob():
    """0: the scheduler object as given; 2 / 3: DPM++ 2M / on Karras sigmas over the given Euler object's own betas and spacing"""
    from seedstory import _lib
    from seedstory.diffusion import DPMSolverMultistepScheduler, EulerDiscreteScheduler, StableDiffusionXLPipeline
    e = EulerDiscreteScheduler(beta_end=0.02, timestep_spacing="trailing")
    pipe = StableDiffusionXLPipeline(vae=None, unet=None, scheduler=e)
    assert pipe._sampler() is e
    try:
        for mode, karras in ((2, False), (3, True)):
            _lib.set_tuning("sdxl_solver", mode)
            s = pipe._sampler()
            assert isinstance(s, DPMSolverMultistepScheduler) and s.use_karras_sigmas == karras and s.solver_order == 2
            assert pipe._sampler() is s
            s.set_timesteps(7)
            ref = R.schedule(7, use_karras_sigmas=karras, beta_end=0.02, timestep_spacing="trailing")
            np.testing.assert_allclose(s.sigmas, ref["sigmas"], rtol=1e-6)
        _lib.set_tuning("sdxl_solver", 1)
        with pytest.raises(_lib.SSError):
            pipe._sampler()
    finally:
        _lib.set_tuning("sdxl_solver", 0)
    assert pipe._sampler() is e and e.sigmas is None          # the given object was never touched


def test_abi_declares_and_refuses_before_any_device_call():
    from seedstory import _lib
    with open(os.path.join(ROOT, "include", "seedstory_hip.h")) as f:
        header = f.read()
    assert "#define SS_ABI_VERSION 1" in header
    assert "ss_multistep_cfg_step(" in header and "ss_multistep_cfg_step" in _lib.PROTOTYPES
    lib = _lib.lib()
    err = lambda: lib.ss_last_error().decode()  # noqa: E731
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    ok = (7.5, 1.0, 0.5, 0.5, 0.0, 1.0)
    assert lib.ss_multistep_cfg_step(None, p, p, p, 8, *ok, _lib.SS_F32, None) == SS_EINVAL and "NULL" in err()
    assert lib.ss_multistep_cfg_step(p, None, p, p, 8, *ok, _lib.SS_F32, None) == SS_EINVAL and "NULL" in err()
    assert lib.ss_multistep_cfg_step(p, p, p, p, 0, *ok, _lib.SS_F32, None) == SS_EINVAL and "n = 0" in err()
    assert lib.ss_multistep_cfg_step(p, p, p, p, -3, *ok, _lib.SS_F32, None) == SS_EINVAL and "n = -3" in err()
    for k in range(6):
        for bad in (float("nan"), float("inf"), -float("inf")):
            vals = list(ok)
            vals[k] = bad
            assert lib.ss_multistep_cfg_step(p, p, p, p, 8, *vals, _lib.SS_F32, None) == SS_EINVAL and "non-finite" in err(), (k, bad)
    assert lib.ss_multistep_cfg_step(p, p, p, p, 8, *ok, 7, None) == SS_EINVAL and "dtype" in err()
    assert all(v == 0.0 for v in buf)                          # nothing was written


@pytest.mark.parametrize("driver", ("gen_george", "vis_george_sink"))
def test_driver_scheduler_argument(driver, monkeypatch):
    import importlib
    import sys
    mod = importlib.import_module("src.inference." + driver)
    seen = {}

    class Stop(Exception):
        pass

    def fake_build(args, device, dtype):
        seen["args"] = args
        raise Stop()

    monkeypatch.setattr(mod, "build", fake_build)
    for argv, want in (([], "euler"), (["--scheduler", "dpmpp2m"], "dpmpp2m"), (["--scheduler", "dpmpp2m-karras"], "dpmpp2m-karras")):
        monkeypatch.setattr(sys, "argv", [driver] + argv)
        with pytest.raises(Stop):
            mod.main()
        assert seen["args"].scheduler == want
    monkeypatch.setattr(sys, "argv", [driver, "--scheduler", "heun"])
    with pytest.raises(SystemExit):
        mod.main()


def test_make_scheduler():
    from seedstory.diffusion import DPMSolverMultistepScheduler, EulerDiscreteScheduler
    from src.inference.gen_george import make_scheduler
    assert type(make_scheduler(argparse.Namespace())) is EulerDiscreteScheduler
    assert type(make_scheduler(argparse.Namespace(scheduler="euler"))) is EulerDiscreteScheduler
    for name, karras in (("dpmpp2m", False), ("dpmpp2m-karras", True)):
        s = make_scheduler(argparse.Namespace(scheduler=name))
        assert isinstance(s, DPMSolverMultistepScheduler) and s.use_karras_sigmas == karras

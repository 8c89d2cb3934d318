"""Host side of limited-interval guidance (no GPU): ``seedstory.diffusion.guidance_mask`` against hand-written expectations and
``tests/guidance_ref.py``, the boundary semantics, the refusals, the drivers' ``--guidance-interval`` argument, the story worker's
keyword and the C ABI's surface and refusals.

The hand-written expectations were read off the printed tables: 20 Karras steps evaluate the model at 11.028, 8.979, 7.265, 5.84,
4.661, ..., 0.405, 0.291, 0.205, 0.142, 0.096, 0.064, 0.041, so (0.25, 6.0] leaves steps 0 - 2 and 15 - 19 unguided (8 of 20); the
30-step leading Euler table starts 11.477, 9.544, 8.004, 6.768, 5.768 and ends 0.344, 0.268, 0.182, 0.041, so the same interval
leaves steps 0 - 3 and 28 - 29 unguided (6 of 30).
"""
import argparse
import ctypes as C
import math
import os

import numpy as np
import pytest

import dpmpp_ref as R
import guidance_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SS_EINVAL = -1


def test_mask_20_step_karras_table():
    from seedstory.diffusion import DPMSolverMultistepScheduler, guidance_mask
    sig = R.schedule(20, use_karras_sigmas=True)["sigmas"][:20]
    want = [False] * 3 + [True] * 12 + [False] * 5
    assert guidance_mask(sig, (0.25, 6.0)) == want and want.count(False) == 8
    assert G.mask(sig, (0.25, 6.0)) == want
    s = DPMSolverMultistepScheduler(use_karras_sigmas=True)
    s.set_timesteps(20)
    assert guidance_mask(s.sigmas[:20], (0.25, 6.0)) == want               # the class's own table
    assert guidance_mask(sig, (0.25, math.inf)) == [True] * 15 + [False] * 5
    assert guidance_mask(sig, None) == [True] * 20


def test_mask_30_step_euler_table():
    from seedstory.diffusion import EulerDiscreteScheduler, guidance_mask
    e = EulerDiscreteScheduler()
    e.set_timesteps(30)
    want = [False] * 4 + [True] * 24 + [False] * 2
    assert guidance_mask(e.sigmas[:30], (0.25, 6.0)) == want and want.count(False) == 6
    assert G.mask(R.schedule(30)["sigmas"][:30], (0.25, 6.0)) == want


def test_mask_boundaries_and_empty_interval():
    from seedstory.diffusion import guidance_mask
    sig = [8.0, 4.0, 2.0, 1.0, 0.5]
    assert guidance_mask(sig, (1.0, 4.0)) == [False, True, True, False, False]    # == sigma_hi guided, == sigma_lo not
    assert guidance_mask(sig, (0.0, math.inf)) == [True] * 5
    assert guidance_mask(sig, (20.0, 30.0)) == [False] * 5                        # holds no step: legal, nothing guided
    assert guidance_mask(sig, (0.6, 0.9)) == [False] * 5
    assert guidance_mask(np.asarray(sig, dtype=np.float32), [1.0, 4.0]) == G.mask(sig, (1.0, 4.0))
    assert guidance_mask([], (0.25, 6.0)) == []


@pytest.mark.parametrize("bad", [(float("nan"), 1.0), (0.5, float("nan")), (-0.1, 1.0), (1.0, 1.0), (2.0, 1.0), (math.inf, math.inf),
                                 (1.0,), (1.0, 2.0, 3.0), "ab", 3.0])
def test_mask_refuses(bad):
    from seedstory.diffusion import guidance_mask
    with pytest.raises(ValueError):
        guidance_mask([4.0, 2.0], bad)


def test_pipeline_refuses_a_bad_interval_before_any_launch():
    """no device is needed to be refused: the models are never touched"""
    from seedstory.diffusion import EulerDiscreteScheduler, StableDiffusionXLPipeline
    import torch
    pipe = StableDiffusionXLPipeline(vae=None, unet=None, scheduler=EulerDiscreteScheduler())
    assert pipe.guidance_interval is None and pipe.last_guidance is None
    e = torch.zeros(1, 4, 8)
    for bad in ((2.0, 1.0), (-1.0, 1.0), (float("nan"), 1.0)):
        with pytest.raises(ValueError):
            pipe(e, e, e[:, 0], e[:, 0], guidance_interval=bad)
        pipe.guidance_interval = bad                        # the attribute is the default of calls that do not pass it
        with pytest.raises(ValueError):
            pipe(e, e, e[:, 0], e[:, 0])
        pipe.guidance_interval = None
    assert pipe.last_guidance is None


def test_reference_loop_uses_the_conditional_output_alone():
    """unguided steps never see an unconditional output, the history carries over a change of form, and an interval that covers
    every step is the plain sampler"""
    s = R.schedule(6, use_karras_sigmas=True)
    sig, coefs = s["sigmas"], s["coefficients"]
    prob = R.gaussian_problem(n=64)
    both = R.gaussian_eps(prob, sig)
    calls = []

    def eps_fn(x, i, guided):
        calls.append(guided)
        e_u, e_c = both(x, i)
        return (e_u, e_c) if guided else e_c
    x0 = prob["noise"] * s["init_noise_sigma"]
    got = G.sample(eps_fn, x0, sig, coefs, 7.5, (0.3, 3.0))
    assert calls == [False, True, True, True, False, False]
    # by hand
    x, dp = x0, None
    for i, guided in enumerate(calls):
        e_u, e_c = both(x, i)
        x, dp = R.step(x, dp, e_u if guided else e_c, e_c, 7.5 if guided else 0.0, float(sig[i]), coefs[i])
    assert np.array_equal(got, x)
    assert np.array_equal(G.sample(eps_fn, x0, sig, coefs, 7.5, (0.0, math.inf)), R.sample(both, x0, sig, coefs, 7.5))
    assert np.array_equal(G.sample(eps_fn, x0, sig, coefs, 7.5, (20.0, 30.0)), G.sample(eps_fn, x0, sig, coefs, 1.5, (20.0, 30.0)))


@pytest.mark.parametrize("driver", ("gen_george", "vis_george_sink"))
def test_driver_guidance_interval_argument(driver, monkeypatch):
    import importlib
    import sys
    mod = importlib.import_module("src.inference." + driver)
    from src.inference.gen_george import guidance_kwargs
    seen = {}

    class Stop(Exception):
        pass

    def fake_build(args, device, dtype):
        seen["args"] = args
        raise Stop()

    monkeypatch.setattr(mod, "build", fake_build)
    for argv, want in (([], {}), (["--guidance-interval", "0.25", "6.0"], {"guidance_interval": (0.25, 6.0)}),
                       (["--guidance-interval", "0.25", "inf"], {"guidance_interval": (0.25, math.inf)})):
        monkeypatch.setattr(sys, "argv", [driver] + argv)
        with pytest.raises(Stop):
            mod.main()
        assert guidance_kwargs(seen["args"]) == want
    for argv in (["--guidance-interval", "0.25"], ["--guidance-interval", "a", "b"]):
        monkeypatch.setattr(sys, "argv", [driver] + argv)
        with pytest.raises(SystemExit):
            mod.main()
    assert guidance_kwargs(argparse.Namespace()) == {}


def test_story_worker_passes_the_interval_on():
    import inspect
    from seedstory.parallel import StoryRingBackend
    assert inspect.signature(StoryRingBackend.__init__).parameters["guidance_interval"].default is None


def test_abi_declares_and_refuses_before_any_device_call():
    from seedstory import _lib
    with open(os.path.join(ROOT, "include", "seedstory_hip.h")) as f:
        header = f.read()
    assert "#define SS_ABI_VERSION 1" in header
    for name in ("ss_multistep_step", "ss_euler_step", "ss_euler_scale"):
        assert name + "(" in header and name in _lib.PROTOTYPES, name
    lib = _lib.lib()
    err = lambda: lib.ss_last_error().decode()  # noqa: E731
    buf = (C.c_float * 64)()
    p = C.addressof(buf)
    ok = (7.5, 1.0, 0.5, 0.5, 0.0, 1.0)
    for rows in ((0, 2), (3, 2), (2, 0), (1, 3), (-1, 1)):
        assert lib.ss_multistep_step(p, p, p, p, 8, rows[0], rows[1], *ok, _lib.SS_F32, None) == SS_EINVAL and "rows" in err(), rows
    assert lib.ss_multistep_step(None, p, p, p, 8, 1, 1, *ok, _lib.SS_F32, None) == SS_EINVAL and "NULL" in err()
    assert lib.ss_multistep_step(p, None, p, p, 8, 2, 1, *ok, _lib.SS_F32, None) == SS_EINVAL and "NULL" in err()
    assert lib.ss_multistep_step(p, p, p, p, 0, 1, 2, *ok, _lib.SS_F32, None) == SS_EINVAL and "n = 0" in err()
    assert lib.ss_multistep_step(p, p, p, p, -3, 2, 2, *ok, _lib.SS_F32, None) == SS_EINVAL and "n = -3" in err()
    for k in range(6):
        for bad in (float("nan"), float("inf")):
            vals = list(ok)
            vals[k] = bad
            assert lib.ss_multistep_step(p, p, p, p, 8, 1, 1, *vals, _lib.SS_F32, None) == SS_EINVAL and "non-finite" in err(), (k, bad)
    assert lib.ss_multistep_step(p, p, p, p, 8, 1, 1, *ok, 7, None) == SS_EINVAL and "dtype" in err()
    assert lib.ss_euler_step(None, p, 8, 1.0, 0.5, _lib.SS_F32, None) == SS_EINVAL
    assert lib.ss_euler_step(p, p, 0, 1.0, 0.5, _lib.SS_F32, None) == SS_EINVAL
    assert lib.ss_euler_step(p, p, 8, 1.0, 0.5, 7, None) == SS_EINVAL
    assert lib.ss_euler_scale(p, None, 8, 1, 1.0, _lib.SS_F32, None) == SS_EINVAL
    assert lib.ss_euler_scale(p, p, -1, 1, 1.0, _lib.SS_F32, None) == SS_EINVAL
    for rows in (0, 3):
        assert lib.ss_euler_scale(p, p, 8, rows, 1.0, _lib.SS_F32, None) == SS_EINVAL and "rows" in err()
    assert lib.ss_euler_scale(p, p, 8, 2, 1.0, 7, None) == SS_EINVAL
    assert all(v == 0.0 for v in buf)                          # nothing was written


def test_ops_wrappers_check_their_arguments():
    import torch
    from seedstory import _lib, ops
    t = torch.zeros(2, 8)
    for fn in (lambda: ops.multistep_step_(t, t, 7.5, 1.0, 0.5, 0.5, 0.0, 1.0), lambda: ops.euler_step_(t, t, 1.0, 0.5),
               lambda: ops.euler_scale(t, 1.0, 1)):
        with pytest.raises(_lib.SSError, match="GPU"):        # no CPU path
            fn()

"""Limited-interval guidance (Kynkäänniemi et al., "Applying Guidance in a Limited Interval Improves Sample and Distribution
Quality in Diffusion Models", NeurIPS 2024) written out in full: the reference of ``seedstory.diffusion.guidance_mask``, of the
pipeline's ``guidance_interval`` and of ``ss_multistep_step`` / ``ss_euler_step`` (include/seedstory_hip.h).

``interval = (sigma_lo, sigma_hi)`` is in the sampler's own sigma units and ``sigmas[i]`` is the level the model is evaluated at
in step i.  Step i is GUIDED iff sigma_lo < sigmas[i] <= sigma_hi:

    guided      the model runs on [uncond; cond]     e = e_u + g (e_c - e_u)
    unguided    the model runs on cond alone         e = e_c                     (g is not used)

then, whichever it was, d = x - sigma_i e and x <- a x + b d + c d_prev with the schedule's own (a, b, c) (``dpmpp_ref``): the
history d_prev is the d of the previous step, guided or not, and the coefficients and timesteps do not know the interval.  Euler
is the coefficient set (ratio, 1 - ratio, 0) (``dpmpp_ref.euler_coefficients``).  ``None`` guides every step.
"""
import math

import dpmpp_ref as R


def mask(sigmas, interval):
    """sigmas [n] (the levels the model is evaluated at, WITHOUT the final 0) -> [n] bools, True = guided"""
    if interval is None:
        return [True] * len(sigmas)
    lo, hi = float(interval[0]), float(interval[1])
    if math.isnan(lo) or math.isnan(hi) or lo < 0.0 or hi <= lo:
        raise ValueError("interval (%r, %r)" % (lo, hi))
    return [lo < float(s) and float(s) <= hi for s in sigmas]


def sample(eps_fn, x_start, sigmas, coefs, guidance, interval):
    """``eps_fn(x, i, guided)`` at sigma_i for the UNSCALED state x (the caller scales what its model sees) -> (e_u, e_c) when
    ``guided``, else e_c alone: the unguided model call has no unconditional half.  sigmas [n + 1] (final 0), coefs [n, 3]."""
    n = len(sigmas) - 1
    m = mask(sigmas[:n], interval)
    x, d_prev = x_start, None
    for i in range(n):
        if m[i]:
            e_u, e_c = eps_fn(x, i, True)
        else:
            e_c = eps_fn(x, i, False)
            e_u = e_c                         # e_u + g (e_c - e_u) with e_u = e_c is e_c exactly, whatever g
        x, d_prev = R.step(x, d_prev, e_u, e_c, guidance, float(sigmas[i]), coefs[i])
    return x

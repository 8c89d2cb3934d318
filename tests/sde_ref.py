"""The two stochastic samplers of the SDXL render and their noise, written out in fp64 numpy: the definition of
``EulerAncestralDiscreteScheduler``, ``DPMSolverMultistepSDEScheduler``, ``ss_randn_philox`` and ``ss_multistep_noise_step``
(include/seedstory_hip.h).  ``tests/test_sde_cpu.py`` checks it (moments, identities, convergence) and the classes
against it; the GPU tests then use it.

One step i, with sigma_i the level of the step, sigma_n the next one, e the guided (or, on an unguided step, the conditional)
prediction and d = x - sigma_i e:

    x' = a x + b d + c d_prev + s z            z ~ N(0, 1) per element, fresh at every step

Euler ancestral (k-diffusion ``sample_euler_ancestral``, eta = 1, s_noise = 1; diffusers EulerAncestralDiscreteScheduler):
    sigma_up = min(sigma_n, sqrt(sigma_n^2 (sigma_i^2 - sigma_n^2) / sigma_i^2));  sigma_down = sqrt(sigma_n^2 - sigma_up^2)
    (a, b, c, s) = (sigma_down / sigma_i, 1 - sigma_down / sigma_i, 0, sigma_up)

DPM++ 2M SDE (k-diffusion ``sample_dpmpp_2m_sde``, midpoint, s_noise = 1; diffusers ``sde-dpmsolver++`` at order 2), eta >= 0:
    h = ln sigma_i - ln sigma_n;  E = 1 - exp(-(1 + eta) h);  a = (sigma_n / sigma_i) exp(-eta h);  s = sigma_n sqrt(1 - exp(-2 eta h))
    first step, or order 1: (a, E, 0, s);  else, r = h_prev / h: (a, E (1 + 1 / (2 r)), -E / (2 r), s)

The last step (sigma_n = 0) of both is (0, 1, 0, 0).  Identities: a + b + c = 1; a^2 sigma_i^2 + s^2 = sigma_n^2 (the noise level of
x' is sigma_n); at eta = 0 the 2M SDE table is ``dpmpp_ref.coefficients`` with s = 0.

Noise: z for image seed S (64 bit), step i and flat element j of that image's latent depends on nothing else:
    q = j >> 2;  (w0, w1, w2, w3) = Philox4x32-10(counter (q, i, 1, 0), key (S & 0xFFFFFFFF, S >> 32))
    u(w) = (w >> 8) 2^-24;  r(w) = sqrt(-2 ln(u(w) + 2^-24))             (the log's argument lies in (0, 1]; r <= 5.77)
    element j = lane j & 3 of [r(w0) cos(2 pi u(w1)), r(w0) sin(2 pi u(w1)), r(w2) cos(2 pi u(w3)), r(w2) sin(2 pi u(w3))]
Counter word 2 = 1 keeps the stream apart from the token sampler's (draw, slot, 0, 0).  Images with equal seeds get equal noise.
"""
import math

import numpy as np

import dpmpp_ref as R
import guidance_ref as G
from test_sampling_cpu import philox4x32_10

TWO_M24 = 2.0 ** -24


def uniform_parts(seed, step, q):
    """-> (u(w0), u(w1), u(w2), u(w3)) of the quads q (array), fp64 (each exact)"""
    seed = int(seed) % (1 << 64)
    w = philox4x32_10((np.asarray(q, dtype=np.uint64), int(step), 1, 0), (seed & 0xFFFFFFFF, seed >> 32))
    return [(v >> 8).astype(np.float64) * TWO_M24 for v in w]


def lane_uniforms(seed, step, j):
    """-> (u_r, u_a, is_sin) of the elements j (array): the uniform under the radius, the one under the angle, sin or cos lane"""
    j = np.asarray(j, dtype=np.int64)
    u = uniform_parts(seed, step, j >> 2)
    lane = j & 3
    return np.where(lane < 2, u[0], u[2]), np.where(lane < 2, u[1], u[3]), (lane & 1) == 1


def normal_parts(seed, step, j):
    """-> (r, c) with z = r c: the radius and the cos | sin factor of the elements j (array) in fp64"""
    u_r, u_a, is_sin = lane_uniforms(seed, step, j)
    r = np.sqrt(-2.0 * np.log(u_r + TWO_M24))
    ang = 2.0 * np.pi * u_a
    return r, np.where(is_sin, np.sin(ang), np.cos(ang))


def normals(seed, step, j):
    r, c = normal_parts(seed, step, j)
    return r * c


def noise(seeds, step, n_img):
    """[len(seeds), n_img] fp64: row b is z(seeds[b], step, 0 .. n_img - 1)"""
    j = np.arange(n_img, dtype=np.int64)
    return np.stack([normals(s, step, j) for s in seeds])


# ---- coefficient tables ---------------------------------------------------------------------------------------------------------------
def euler_ancestral_coefficients(sigmas):
    """sigmas [n + 1] (final 0) -> (a, b, c, s) [n, 4] in double"""
    n = len(sigmas) - 1
    out = np.zeros((n, 4), dtype=np.float64)
    for i in range(n):
        si, sn = float(sigmas[i]), float(sigmas[i + 1])
        if sn == 0.0:
            out[i] = (0.0, 1.0, 0.0, 0.0)
            continue
        up = min(sn, math.sqrt(sn ** 2 * (si ** 2 - sn ** 2) / si ** 2))
        down = math.sqrt(sn ** 2 - up ** 2)
        out[i] = (down / si, 1.0 - down / si, 0.0, up)
    return out


def dpmpp_2m_sde_coefficients(sigmas, eta=1.0, solver_order=2):
    """sigmas [n + 1] (final 0) -> (a, b, c, s) [n, 4] in double, through expm1"""
    n = len(sigmas) - 1
    out = np.zeros((n, 4), dtype=np.float64)
    h_prev = None
    for i in range(n):
        si, sn = float(sigmas[i]), float(sigmas[i + 1])
        if sn == 0.0:
            out[i] = (0.0, 1.0, 0.0, 0.0)
            continue
        h = math.log(si) - math.log(sn)
        E = -math.expm1(-(1.0 + eta) * h)
        a = (sn / si) * math.exp(-eta * h)
        s = sn * math.sqrt(-math.expm1(-2.0 * eta * h))
        if i == 0 or solver_order == 1:
            out[i] = (a, E, 0.0, s)
        else:
            r = h_prev / h
            out[i] = (a, E * (1.0 + 1.0 / (2.0 * r)), -E / (2.0 * r), s)
        h_prev = h
    return out


def schedule(n, sampler, use_karras_sigmas=False, eta=1.0, solver_order=2, **base):
    """``dpmpp_ref.schedule`` with the [n, 4] table of ``sampler`` ("euler-a" | "2m-sde")"""
    s = R.schedule(n, use_karras_sigmas=use_karras_sigmas, **base)
    sig = s["sigmas"]
    s["coefficients"] = (euler_ancestral_coefficients(sig) if sampler == "euler-a"
                         else dpmpp_2m_sde_coefficients(sig, eta, solver_order))
    return s


# ---- the sampling loop ----------------------------------------------------------------------------------------------------------------
def _like(z, x):
    """the fp64 noise [B, n_img] in the shape and kind of the state x (numpy array or torch tensor)"""
    if isinstance(x, np.ndarray):
        return z.reshape(x.shape)
    import torch
    return torch.from_numpy(z).reshape(x.shape).to(x.dtype)


def sample(eps_fn, x_start, sigmas, coefs4, guidance, interval, seeds, n_img):
    """``guidance_ref.sample`` with the noise term: ``eps_fn(x, i, guided)`` as there, coefs4 [n, 4], ``seeds`` one per image,
    the state holds len(seeds) images of ``n_img`` elements each (image-major).  s == 0: no noise is generated."""
    n = len(sigmas) - 1
    m = G.mask(sigmas[:n], interval)
    x, d_prev = x_start, None
    for i in range(n):
        if m[i]:
            e_u, e_c = eps_fn(x, i, True)
        else:
            e_c = eps_fn(x, i, False)
            e_u = e_c
        x, d_prev = R.step(x, d_prev, e_u, e_c, guidance, float(sigmas[i]), coefs4[i][:3])
        s = float(coefs4[i][3])
        if s != 0.0:
            x = x + s * _like(noise(seeds, i, n_img), x)
    return x


# ---- convergence: the moments of a Gaussian problem, propagated exactly -------------------------------------------------------------------
def gaussian_end_std(sigmas, coefs4, sigma_d):
    """Per-element data N(m, sigma_d^2) with the exact denoiser D(x, sigma) = m + k (x - m), k = sigma_d^2 / (sigma_d^2 + sigma^2),
    no guidance, start x ~ N(m, sigma_d^2 + sigma_0^2).  d = x - sigma e IS D(x, sigma), so with y = x - m, p = d_prev - m (and
    a + b + c = 1) a step is linear:  (y', p') = [[a + b k, c], [k, 0]] (y, p) + (s z, 0).  The mean stays m; the covariance of
    (y, p) follows C' = M C M^T + diag(s^2, 0), exactly, in fp64 — no sampling.  -> the standard deviation of the end point."""
    C = np.array([[sigma_d ** 2 + float(sigmas[0]) ** 2, 0.0], [0.0, 0.0]], dtype=np.float64)
    for i in range(len(sigmas) - 1):
        a, b, c, s = (float(v) for v in coefs4[i])
        k = sigma_d ** 2 / (sigma_d ** 2 + float(sigmas[i]) ** 2)
        M = np.array([[a + b * k, c], [k, 0.0]], dtype=np.float64)
        C = M @ C @ M.T + np.array([[s * s, 0.0], [0.0, 0.0]])
    return math.sqrt(C[0, 0])


def gaussian_std_error(n, sampler, sigma_d, use_karras_sigmas=True, eta=1.0):
    """relative error of the end-point standard deviation against sigma_d, ``n`` steps"""
    s = schedule(n, sampler, use_karras_sigmas=use_karras_sigmas, eta=eta)
    return abs(gaussian_end_std(s["sigmas"], s["coefficients"], sigma_d) - sigma_d) / sigma_d

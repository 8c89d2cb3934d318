"""DPM-Solver++ 2M (optionally on Karras sigmas) written out in fp64 numpy: the reference of ``DPMSolverMultistepScheduler`` and
of ``ss_multistep_cfg_step`` (include/seedstory_hip.h).  ``tests/test_dpmpp_cpu.py`` checks it against an exact solution and the
class against it; the GPU tests then use it.

State convention (the pipeline's): x = x0 + sigma * noise; the model sees x / sqrt(sigma^2 + 1) and predicts eps.  One step i:

    e = e_u + g (e_c - e_u);  d = x - sigma_i e;  h = ln sigma_i - ln sigma_{i+1};  E = -expm1(-h)
    sigma_{i+1} == 0 (last step)        x <- d
    first step, or solver_order == 1    x <- (sigma_{i+1} / sigma_i) x + E d
    else, r = h_prev / h                x <- (sigma_{i+1} / sigma_i) x + E (1 + 1 / (2 r)) d - E / (2 r) d_prev

i.e. x <- a x + b d + c d_prev with (a, b, c) per step.  This is k-diffusion's ``sample_dpmpp_2m``; Euler's own step is
(sigma_{i+1} / sigma_i, 1 - sigma_{i+1} / sigma_i, 0) in the same form.
"""
import math

import numpy as np

KARRAS_RHO = 7.0


def train_sigmas(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012):
    """The training table sqrt((1 - abar) / abar) of the scaled-linear betas, in the fp32 arithmetic EulerDiscreteScheduler uses."""
    betas = np.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=np.float32) ** 2
    ac = np.cumprod(1.0 - betas)
    return ((1 - ac) / ac) ** 0.5


def base_schedule(n, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, timestep_spacing="leading", steps_offset=1):
    """(timesteps [n], sigmas [n]) of EulerDiscreteScheduler.set_timesteps(n): linearly interpolated, stored as fp32."""
    table = train_sigmas(num_train_timesteps, beta_start, beta_end)
    if timestep_spacing == "leading":
        ratio = num_train_timesteps // n
        ts = (np.arange(0, n) * ratio).round()[::-1].copy().astype(np.float32) + steps_offset
    elif timestep_spacing == "linspace":
        ts = np.linspace(0, num_train_timesteps - 1, n, dtype=np.float32)[::-1].copy()
    else:
        ratio = num_train_timesteps / n
        ts = (np.arange(num_train_timesteps, 0, -ratio)).round().astype(np.float32) - 1
    s = np.interp(ts, np.arange(0, len(table)), table).astype(np.float32)
    return ts.astype(np.float64), s.astype(np.float64), table.astype(np.float64)


def karras_sigmas(sigma_max, sigma_min, n, rho=KARRAS_RHO):
    if n == 1:
        return np.array([sigma_max], dtype=np.float64)
    ramp = np.arange(n, dtype=np.float64) / (n - 1)
    lo, hi = sigma_min ** (1.0 / rho), sigma_max ** (1.0 / rho)
    return (hi + ramp * (lo - hi)) ** rho


def sigma_to_timestep(sigmas, table):
    """log-sigma interpolation into the training table, rounded to the nearest integer, clipped to [0, len - 1]."""
    logt = np.log(table)
    out = []
    for s in sigmas:
        ls = math.log(max(float(s), 1e-10))
        low = int(np.clip(np.searchsorted(logt, ls, side="right") - 1, 0, len(logt) - 2))
        w = min(max((logt[low] - ls) / (logt[low] - logt[low + 1]), 0.0), 1.0)
        out.append((1.0 - w) * low + w * (low + 1))
    return np.clip(np.round(np.array(out, dtype=np.float64)), 0, len(table) - 1)


def coefficients(sigmas, solver_order=2):
    """sigmas [n + 1] (final 0) -> (a, b, c) [n, 3] in double."""
    n = len(sigmas) - 1
    out = np.zeros((n, 3), dtype=np.float64)
    h_prev = None
    for i in range(n):
        s, sn = float(sigmas[i]), float(sigmas[i + 1])
        if sn == 0.0:
            out[i] = (0.0, 1.0, 0.0)
            continue
        h = math.log(s) - math.log(sn)
        E = -math.expm1(-h)
        if i == 0 or solver_order == 1:
            out[i] = (sn / s, E, 0.0)
        else:
            r = h_prev / h
            out[i] = (sn / s, E * (1.0 + 1.0 / (2.0 * r)), -E / (2.0 * r))
        h_prev = h
    return out


def euler_coefficients(sigmas):
    s, sn = np.asarray(sigmas[:-1], dtype=np.float64), np.asarray(sigmas[1:], dtype=np.float64)
    return np.stack([sn / s, 1.0 - sn / s, np.zeros_like(s)], axis=1)


def schedule(n, use_karras_sigmas=False, solver_order=2, **base):
    """-> dict(timesteps [n], sigmas [n + 1], coefficients [n, 3], init_noise_sigma)"""
    ts, s, table = base_schedule(n, **base)
    if use_karras_sigmas:
        s = karras_sigmas(float(s[0]), float(s[n - 1]), n)
        ts = sigma_to_timestep(s, table)
    sig = np.concatenate([s, [0.0]])
    return {"timesteps": ts, "sigmas": sig, "coefficients": coefficients(sig, solver_order),
            "init_noise_sigma": math.sqrt(float(sig[0]) ** 2 + 1.0)}


def step(x, d_prev, e_u, e_c, guidance, sigma, abc):
    """-> (x', d).  Works on numpy arrays and on anything else with + and * (torch tensors)."""
    a, b, c = (float(v) for v in abc)
    e = e_u + guidance * (e_c - e_u)
    d = x - sigma * e
    xn = a * x + b * d
    if c != 0.0:
        xn = xn + c * d_prev
    return xn, d


def sample(eps_fn, x_start, sigmas, coefs, guidance):
    """``eps_fn(x, i)`` -> (e_u, e_c) at sigma_i for the UNSCALED state x (the caller scales what its model sees)."""
    x, d_prev = x_start, None
    for i in range(len(sigmas) - 1):
        e_u, e_c = eps_fn(x, i)
        x, d_prev = step(x, d_prev, e_u, e_c, guidance, float(sigmas[i]), coefs[i])
    return x


# ---- an exact solution: per element the data are N(mu, s^2) --------------------------------------------------------------------
def gaussian_problem(n=4096, seed=0, guidance=7.5):
    """eps(x, sigma; mu) = sigma (x - mu) / (s^2 + sigma^2); CFG over two means is the same eps at mu_u + g (mu_c - mu_u)."""
    rng = np.random.RandomState(seed)
    mu_u = rng.normal(0.0, 0.3, n)
    mu_c = rng.normal(0.2, 0.5, n)
    s = rng.uniform(0.2, 1.0, n)
    noise = rng.normal(0.0, 1.0, n)
    return {"mu_u": mu_u, "mu_c": mu_c, "s": s, "noise": noise, "guidance": guidance, "mu": mu_u + guidance * (mu_c - mu_u)}


def gaussian_eps(prob, sigmas, dtype=np.float64):
    mu_u, mu_c, s2 = prob["mu_u"].astype(dtype), prob["mu_c"].astype(dtype), (prob["s"] ** 2).astype(dtype)

    def fn(x, i):
        sg = dtype(sigmas[i])
        k = sg / (s2 + sg * sg)
        return k * (x - mu_u), k * (x - mu_c)
    return fn


def gaussian_exact(prob, x_start, sigma0):
    return prob["mu"] + (x_start - prob["mu"]) * prob["s"] / np.sqrt(prob["s"] ** 2 + sigma0 ** 2)


def rel_rms(x, ref):
    x, ref = np.asarray(x, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.sqrt(np.mean((x - ref) ** 2)) / np.sqrt(np.mean(ref ** 2)))


def gaussian_error(prob, sigmas, coefs, dtype=np.float64):
    """relative RMS error of a whole run from x_start = noise sqrt(sigma_0^2 + 1) against the exact end point."""
    x0 = prob["noise"] * math.sqrt(float(sigmas[0]) ** 2 + 1.0)
    x = sample(gaussian_eps(prob, sigmas, dtype), x0.astype(dtype), sigmas, coefs.astype(dtype) if dtype != np.float64 else coefs,
               dtype(prob["guidance"]))
    return rel_rms(x, gaussian_exact(prob, x0, float(sigmas[0])))

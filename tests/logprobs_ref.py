"""The fp64 reference of the token log-probabilities (include/seedstory_hip.h, ``ss_token_logprobs``), shared by
tests/test_logprobs_cpu.py and tests/test_logprobs_gpu.py, and the comparison of a kernel's fp32 value against it."""
import numpy as np

from test_sampling_cpu import oracle

FLT_MAX = float(np.finfo(np.float32).max)


def log_softmax(row):
    """lsm over one row (any array, taken to fp64 exactly): NaN and -inf entries carry no mass; a NaN entry gives NaN, a -inf
    entry -inf, and a row without any mass gives those two by the entry alone."""
    z = np.asarray(row, dtype=np.float64)
    valid = ~np.isnan(z) & (z > -np.inf)
    out = np.where(np.isnan(z), np.nan, -np.inf)
    if valid.any():
        zmax = z[valid].max()
        logz = np.log(np.exp(z[valid] - zmax).sum())
        out[valid] = (z[valid] - zmax) - logz
    return out


def model_logprob(raw, tok):
    return float(log_softmax(raw)[tok])


def top_n(raw, n):
    """(ids int64 [n], logprobs fp64 [n]): the n largest entries that carry mass, descending, equal values by ascending id;
    -1 / -inf where fewer carry mass"""
    z = np.asarray(raw, dtype=np.float64)
    lsm = log_softmax(z)
    live = np.flatnonzero(~np.isnan(z) & (z > -np.inf))
    order = live[np.lexsort((live, -z[live]))][:n]          # primary key: value descending; secondary: id ascending
    ids = np.full(n, -1, dtype=np.int64)
    lps = np.full(n, -np.inf)
    ids[:order.size] = order
    lps[:order.size] = lsm[order]
    return ids, lps


def policy_logprob(z, tok, sampling=None):
    """greedy (sampling None): lsm(z)[tok].  sampling = dict(temperature, top_k, top_p): log(w_tok / Z_P) over the oracle's kept
    set, -inf outside it -> (value, decided)"""
    if sampling is None:
        return float(log_softmax(z)[tok]), True
    z = np.asarray(z, dtype=np.float64)
    o = oracle(z, sampling["temperature"], sampling.get("top_k", 0), sampling.get("top_p", 1.0), u=0.0)
    if o["n_kept"] == 0 or not o["kept"][tok]:
        return -np.inf, o["decided"]
    T = float(np.float32(sampling["temperature"]))
    zmax = z[o["kept"]].max()
    return float((z[tok] - zmax) / T - np.log(o["Z_P"])), o["decided"]


def within(got, ref, a, b):
    """a kernel's fp32 value against the fp64 reference: NaN for NaN, -inf for -inf, |got - ref| <= a + b |ref| otherwise;
    a reference beyond the fp32 range (entries at -FLT_MAX under a maximum at +FLT_MAX) may come out as -inf, its fp32 value"""
    got = float(got)
    if np.isnan(ref):
        return bool(np.isnan(got))
    if np.isnan(got):
        return False
    if ref == -np.inf:
        return got == -np.inf
    if abs(ref) >= FLT_MAX * (1.0 - b) and got == -np.inf:
        return True
    return abs(got - ref) <= a + b * abs(ref)

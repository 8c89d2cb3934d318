"""Plain-Python beam search: the reference of the engine's on-device search (include/seedstory_hip.h, ss_llama_beam_search).

One batch item of transformers' ``GenerationMixin._beam_search`` written out without its -1e9 arithmetic (dead hypotheses and
empty table places are flags here), with the tie rule the engine adds: equal accumulated scores order by ascending
``beam * vocab + token``.  ``tests/test_beam_cpu.py`` pins it against the installed transformers; the GPU tests then use it.
"""
import math

import torch


def log_softmax_rows(rows, dtype=torch.float64):
    """log-softmax of each row in ``dtype``; NaN and -inf entries carry no mass and come out as -inf (never a candidate)."""
    x = rows.to(dtype)
    valid = x > float("-inf")                           # (a NaN never compares greater)
    xm = torch.where(valid, x, torch.full_like(x, float("-inf")))
    m = xm.max(dim=-1, keepdim=True).values
    m = torch.where(m > float("-inf"), m, torch.zeros_like(m))
    s = torch.where(valid, (xm - m).exp(), torch.zeros_like(x)).sum(dim=-1, keepdim=True)
    return torch.where(valid, (xm - m) - s.log(), torch.full_like(x, float("-inf")))


def step(rows, scores, K, dtype=torch.float64, extra=0):
    """The K (+ ``extra``) best of ``scores[b] + log_softmax(rows[b])[t]``: a list of ``(score, beam, token)``, descending, equal
    scores by ascending ``beam * vocab + token``; ``(-inf, -1, -1)`` where fewer candidates exist.  A score of -inf (or None)
    marks a dead row."""
    n, V = rows.shape
    sc = torch.tensor([float("-inf") if s is None else float(s) for s in scores], dtype=dtype)
    acc = log_softmax_rows(rows, dtype) + sc[:, None]
    acc = torch.where(acc == acc, acc, torch.full_like(acc, float("-inf"))).reshape(-1)     # (-inf + nothing stays -inf)
    k = min(K + extra, acc.numel())
    vals, idx = torch.sort(acc, descending=True, stable=True)                                # stable: ascending index on ties
    out = []
    for v, i in zip(vals[:k].tolist(), idx[:k].tolist()):
        out.append((v, i // V, i % V) if v > float("-inf") else (float("-inf"), -1, -1))
    while len(out) < K + extra:
        out.append((float("-inf"), -1, -1))
    return out


def n_candidates(n, stop_ids):
    return max(2, 1 + len(stop_ids)) * n


def search(logits_fn, n, stop_ids, limit, length_penalty=1.0, early_stopping=False, dtype=torch.float32):
    """``logits_fn(seqs, parents)`` -> tensor [len(seqs), vocab]: the logits rows of the running hypotheses ``seqs`` (lists of
    generated ids); ``parents[i]`` = the index hypothesis i had in the previous call (None on the first call, which has the one
    empty hypothesis).  Returns ``{"sequences", "scores", "finished"}`` (the finished table, best first, n entries), and
    ``"steps"``: per step the candidate list with one extra entry, for gap checks."""
    assert early_stopping in (False, True, "never")
    stop_ids = [int(t) for t in stop_ids]
    K = n_candidates(n, stop_ids)

    def f(v):                   # one rounding to the search's dtype, as the tensors of the original hold it
        return torch.as_tensor(v).to(dtype).item()

    run = [([], 0.0)]           # live hypotheses only: (ids, accumulated score)
    parents = None
    table = []                  # finished: (score, ids), best first
    unsat = True
    steps = []
    for t in range(limit):
        rows = logits_fn([s for s, _ in run], parents)
        cands = step(rows, [sc for _, sc in run], K, dtype, extra=1)
        steps.append(cands)
        cands = [c for c in cands[:K] if c[1] >= 0]
        hit = [tok in stop_ids or t + 1 >= limit for _, _, tok in cands]
        new_run, parents = [], []
        for (sc, b, tok), h in zip(cands, hit):
            if not h and len(new_run) < n:
                new_run.append((run[b][0] + [tok], sc))
                parents.append(b)
        pen = (t + 1) ** length_penalty
        fresh = [(f(torch.tensor(sc, dtype=dtype) / pen), run[b][0] + [tok])
                 for j, ((sc, b, tok), h) in enumerate(zip(cands, hit)) if h and j < n]
        merged, io, jn = [], 0, 0
        while len(merged) < n and (io < len(table) or jn < len(fresh)):
            if io < len(table) and (jn >= len(fresh) or table[io][0] >= fresh[jn][0]):
                merged.append(table[io]); io += 1
            else:
                merged.append(fresh[jn]); jn += 1
        table = merged
        run = new_run
        all_fin = len(table) == n
        if all_fin:
            hyp = limit if (early_stopping == "never" and length_penalty > 0.0) else t + 1
            best = f(torch.tensor(run[0][1], dtype=dtype) / (hyp ** length_penalty)) if run else float("-inf")
            if not best > table[-1][0]:
                unsat = False
        go = unsat and not (all_fin and early_stopping is True) and not all(hit) and bool(run) and bool(cands)
        if not go:
            break
    return {"sequences": [ids for _, ids in table] + [[]] * (n - len(table)),
            "scores": [sc for sc, _ in table] + [float("-inf")] * (n - len(table)),
            "finished": [True] * len(table) + [False] * (n - len(table)),
            "steps": steps, "running": run}


def min_gap(cands):
    """the smallest difference between neighbouring candidates of one step's list (inf where fewer than two exist)"""
    v = [c[0] for c in cands if c[1] >= 0]
    return min((a - b for a, b in zip(v, v[1:])), default=math.inf)

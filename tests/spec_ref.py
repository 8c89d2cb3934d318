"""Prompt-lookup speculative decoding in plain Python: the definitions the device kernels of ``csrc/ss_spec.h`` are tested
against (``include/seedstory_hip.h``, ss_llama_set_speculation).

``draft``   transformers' ``PromptLookupCandidateGenerator.get_candidates`` on a token history (pinned against the installed
            transformers by ``test_spec_cpu.py``).
``replay``  a whole speculative ``generate`` call given the per-position arg-max oracle — the ids plain greedy produces, which are
            what the model answers after any accepted prefix — : what every step drafts, how many drafts it accepts, how far
            ``kv_len`` moves and the four counters of ``LlamaEngine.spec_stats``.
``step``    one step of it.
"""
import random


def draft(hist, max_ngram, k, stops=(), vocab=None):
    """ids drafted after ``hist``: n-gram sizes from min(max_ngram, len - 1) down to 1, the leftmost match with a non-empty
    continuation, at most ``k`` ids, cut in front of the first stop id (an empty cut: no draft — no shorter n-gram is tried);
    also cut in front of an id outside [0, vocab) when ``vocab`` is given.  ``path`` of the last call is left in ``draft.path``:
    "none" | "match" | "clipped" (the continuation ran into the end) | "stop" (cut by a stop id), with "+fallback" when a longer
    n-gram was tried without a match first."""
    hist = [int(t) for t in hist]
    n = len(hist)
    draft.path = "none"
    top = min(max_ngram, n - 1)
    for g in range(top, 0, -1):
        tail = hist[n - g:]
        for idx in range(0, n - g):         # idx + g < n: the continuation is not empty
            if hist[idx:idx + g] == tail:
                start = idx + g
                out = hist[start:min(start + k, n)]
                path = "clipped" if start + k > n else "match"
                for i, t in enumerate(out):
                    if t in stops or (vocab is not None and not 0 <= t < vocab):
                        out, path = out[:i], "stop"
                        break
                draft.path = path + ("+fallback" if g < top else "")
                return out
    return []


draft.path = "none"


def draft_grid():
    """The cases the draft is pinned on, on the CPU against transformers and on the GPU against ``draft``; seeded: sequence
    lengths 2..40, vocabularies of 3..6 symbols (matches are common), n-gram caps 1..4, 1..7 output tokens, with and without
    stop ids"""
    rng = random.Random(20240)
    cases = []
    for length in range(2, 41):
        for rep in range(6):
            vocab = 3 + (length + rep) % 4
            seq = [rng.randrange(vocab) for _ in range(length)]
            g = 1 + rng.randrange(4)
            k = 1 + rng.randrange(7)
            stops = () if rep % 2 == 0 else ((rng.randrange(vocab),) if rep % 3 else (rng.randrange(vocab), rng.randrange(vocab)))
            cases.append((seq, g, k, stops))
    return cases


def _drafts(n, want, hist, rows, source, max_ngram, given, forced, stops, vocab):
    """the drafts of a step whose row 0 is generated index n - 1 (``n`` tokens emitted so far)"""
    if want <= 0:
        return []
    if n < len(forced) or source == "given":
        ids = forced if n < len(forced) else given
        out = []
        for c in range(want):
            if n + c >= len(ids):
                break
            t = int(ids[n + c])
            if t in stops or not 0 <= t < vocab:
                break
            out.append(t)
        return out
    return draft(hist, max_ngram, want, stops, vocab)


def step(oracle, n, pending, hist, *, rows, limit, max_new, kv_room, pos_room, source="lookup", max_ngram=2, given=(), forced=(),
         stops=(), vocab=1 << 30):
    """One opening kernel.  ``oracle[i]`` = the id greedy emits at generated index i; ``n`` ids are out, ``pending`` = the rows'
    tokens of the step in flight ([] before the first), ``hist`` the history (extended in place), ``kv_room`` / ``pos_room`` the
    cache rows / RoPE positions left AFTER the rows already counted as forwarded.  Returns a dict: ``emitted`` ids, ``accepted``
    drafts, ``kv_advance``, ``done``, ``rows`` = the next step's tokens ([] when done)."""
    adv = 1 if pending else 0
    r, acc, out, done = 0, 0, [], False
    while True:
        tok = int(oracle[n])
        done = tok in stops or n + 1 >= limit
        hist.append(tok)
        out.append(tok)
        n += 1
        if done:
            break
        if r + 1 < len(pending) and pending[r + 1] == tok:
            acc, adv, r = acc + 1, adv + 1, r + 1
            continue
        break
    nxt = []
    if not done:
        n0 = n - 1
        want = min(rows, limit - 1 - n0, max_new - n0, kv_room - adv, pos_room - adv) - 1
        nxt = [out[-1]] + _drafts(n, want, hist, rows, source, max_ngram, given, forced, stops, vocab)
    return {"emitted": out, "accepted": acc, "kv_advance": adv, "done": done, "rows": nxt}


def replay(oracle, *, rows, limit, max_new, kv_room, pos_room, hist=(), **kw):
    """A whole call.  Returns ``{"steps", "drafted", "accepted", "emitted", "kv_advance", "ids", "per_step"}``; ``per_step`` =
    one ``(row tokens, drafts accepted)`` pair per speculative forward."""
    hist = [int(t) for t in hist]
    n, pending, per = 0, [], []
    tot = {"steps": 0, "drafted": 0, "accepted": 0, "emitted": 0, "kv_advance": 0, "ids": []}
    while True:
        s = step(oracle, n, pending, hist, rows=rows, limit=limit, max_new=max_new, kv_room=kv_room - tot["kv_advance"],
                 pos_room=pos_room - tot["kv_advance"], **kw)
        if per:
            per[-1] = (per[-1][0], s["accepted"])
        n += len(s["emitted"])
        tot["ids"] += s["emitted"]
        tot["emitted"] += len(s["emitted"])
        tot["accepted"] += s["accepted"]
        tot["kv_advance"] += s["kv_advance"]
        if s["done"]:
            break
        pending = s["rows"]
        tot["steps"] += 1
        tot["drafted"] += len(pending) - 1
        per.append((list(pending), 0))
    tot["per_step"] = per
    return tot

"""Prompt-lookup speculative steps against the greedy decode token, same process, same box, variants alternating, on the synthetic
LLaMA-7B of bench.py (weights created on the GPU), one slot, 400 and 1100 cached positions:
  greedy                       ``generate`` of --tokens tokens, ms per forward
  spec R = 2, 4, 8 accepted    given drafts = the greedy run's own ids (what the model agrees with: every step emits R tokens
                               wherever the R-row and the 1-row kernels agree on the arg max; the counters say how often they did)
  spec R = 2, 4, 8 rejected    given drafts that are never the arg max: every step pays for R rows and emits one token
Reported per variant: ms per step (a step = one forward), ms per emitted token, the counters; per R the break-even mean number of
accepted drafts per step, ms_step(R, rejected) / ms_step(greedy) - 1.  Lookup acceptance on these weights is recorded as a curiosity
only: random weights loop, which says nothing about captions.
  python tools/spec_bench.py [--repeats 5] [--tokens 33] [--layers 32] [--out profiles/spec_decode.json]"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "seed-story_amd"))
from seedstory.llama import LlamaEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--tokens", type=int, default=33)
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--out", default=None, help="also write the records as one JSON list to this file")
args = ap.parse_args()
dev, dt = "cuda:0", torch.bfloat16
H, NH, NL, INTER, VOCAB = 4096, 32, args.layers, 11008, 32066
torch.manual_seed(1234)
rnd = lambda *s: torch.randn(*s, device=dev, dtype=dt) * 0.02  # noqa: E731
ones = lambda n: torch.ones(n, device=dev, dtype=dt)  # noqa: E731
shared = dict(layers=[(rnd(3 * H, H), rnd(H, H), rnd(2 * INTER, H), rnd(H, INTER), ones(H), ones(H)) for _ in range(NL)],
              embed=rnd(VOCAB, H), lm_head=rnd(VOCAB, H), final_norm=ones(H))
eng = LlamaEngine.from_prebuilt(hidden=H, n_heads=NH, n_layers=NL, inter=INTER, vocab=VOCAB, dtype=dt, device=dev, cache_cap=1280,
                                max_new=64, max_prefill_rows=128, img_ids=(), eos_id=-1, n_seq=1, **shared)
out = []


def emit(rec):
    out.append(rec)
    print(json.dumps(rec), flush=True)


def median(v):
    return sorted(v)[len(v) // 2]


def run(L, logits0):
    """one ``generate`` from the same state: L cached positions, the same logits row -> (ms, ids)"""
    eng.set_lengths(L, L)
    eng.logits.copy_(logits0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = eng.generate(args.tokens, last_prompt_id=5)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, eng.gen_ids[:n].tolist()


for L in (400, 1100):
    eng.clear_speculation()
    eng.set_lengths(0, 0)
    eng.prefill(shared["embed"][torch.arange(7, 7 + 16, device=dev)])      # a logits row to start every run from
    logits0 = eng.logits.clone()
    _, ids = run(L, logits0)
    wrong = [(t + 1) % VOCAB for t in ids]
    variants = [("greedy", 0, None)]
    for R in (2, 4, 8):
        variants += [("accepted", R, ids), ("rejected", R, wrong)]
    variants.append(("lookup", 4, "lookup"))
    times = {v[:2]: [] for v in variants}
    stats = {}
    for r in range(args.repeats + 1):               # round 0 warms every path (and captures every graph) and is dropped
        for name, R, drafts in variants:
            if R == 0:
                eng.clear_speculation()
            elif drafts == "lookup":
                eng.set_speculation(R, max_ngram=2)
                eng.set_history([5])
            else:
                eng.set_speculation(R, draft_ids=drafts)
            ms, got = run(L, logits0)
            if r:
                times[(name, R)].append(ms)
                stats[(name, R)] = (eng.spec_stats() if R else {"steps": len(got) - 1, "drafted": 0, "accepted": 0, "emitted": len(got)},
                                    got == ids)
    eng.clear_speculation()
    base = None
    for name, R, _ in variants:
        ts, (st, same) = times[(name, R)], stats[(name, R)]
        step = [t / max(st["steps"], 1) for t in ts]
        rec = {"what": "spec_decode", "cached": L, "variant": name, "rows": R, "layers": NL, "tokens": st["emitted"], "stats": st,
               "ids_equal_greedy": same, "ms_per_step": [round(t, 4) for t in step], "ms_per_step_median": round(median(step), 4),
               "ms_per_step_spread": round(max(step) - min(step), 4),
               "ms_per_token_median": round(median(ts) / max(st["emitted"] - 1, 1), 4)}
        if name == "greedy":
            base = median(step)
        elif name == "rejected":
            rec["break_even_accepted_per_step"] = round(median(step) / base - 1.0, 4)
        emit(rec)
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)

"""On-device sampling against the greedy decode token, same process, same box, interleaved, on the synthetic LLaMA-7B of bench.py
(weights created on the GPU): ``LlamaEngine.profile_decode`` at 1 and 8 sequence slots, alternating greedy / sampling for
--repeats rounds.  ``misc_ms`` is the launch class that holds the sampling kernel and the final norm, ``token_ms`` the whole token.
  python tools/sampling_bench.py [--repeats 5] [--tokens 8] [--layers 32] [--out FILE]  ->  JSON lines (+ the list in FILE)
The yardstick is the greedy token of the same process: sampling "costs" when its median token time exceeds greedy's by more than
the spread (max - min) of the greedy repeats."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "seed-story_amd"))
from seedstory.llama import LlamaEngine  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--tokens", type=int, default=8)
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
# greedy, the reference signature's defaults (top-p threshold search only), and both threshold searches
MODES = {"greedy": None, "sampling_T0.7_p0.5": dict(temperature=0.7, top_k=0, top_p=0.5),
         "sampling_T1.0_k50_p0.9": dict(temperature=1.0, top_k=50, top_p=0.9)}
out = []


def emit(rec):
    out.append(rec)
    print(json.dumps(rec), flush=True)


def median(v):
    return sorted(v)[len(v) // 2]


for n_seq in (1, 8):
    eng = LlamaEngine.from_prebuilt(hidden=H, n_heads=NH, n_layers=NL, inter=INTER, vocab=VOCAB, dtype=dt, device=dev, cache_cap=512,
                                    max_new=64, max_prefill_rows=128, img_ids=(), eos_id=2, n_seq=n_seq, **shared)
    runs = {m: [] for m in MODES}
    for r in range(args.repeats + 1):                   # round 0 warms every path up and is dropped
        for mode, kw in MODES.items():
            if kw is None:
                eng.set_greedy()
            else:
                eng.set_sampling(seed=1234 + r, **kw)
            for b in range(n_seq):
                eng.select(b).set_lengths(343, 343)
            p = eng.profile_decode(args.tokens)
            if r:
                runs[mode].append(p)
    eng.set_greedy()
    g = runs["greedy"]
    g_tok = [p["token_ms"] for p in g]
    spread = max(g_tok) - min(g_tok)
    for mode, ps in runs.items():
        tok = [round(p["token_ms"], 4) for p in ps]
        misc = [round(p["misc_ms"], 4) for p in ps]
        emit({"what": "profile_decode", "n_seq": n_seq, "mode": mode, "layers": NL, "vocab": VOCAB, "token_ms": tok,
              "token_ms_median": median(tok), "token_ms_spread": round(max(tok) - min(tok), 4), "misc_ms": misc,
              "misc_ms_median": median(misc)})
    for mode, ps in runs.items():
        if mode == "greedy":
            continue
        add_tok = median([p["token_ms"] for p in ps]) - median(g_tok)
        add_misc = median([p["misc_ms"] for p in ps]) - median([p["misc_ms"] for p in g])
        emit({"what": "verdict", "n_seq": n_seq, "mode": mode, "token_ms_greedy": round(median(g_tok), 4),
              "added_token_ms": round(add_tok, 4), "added_misc_ms": round(add_misc, 4), "spread_greedy_ms": round(spread, 4),
              "within_spread": bool(add_tok <= spread)})
    del eng
    torch.cuda.empty_cache()
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)

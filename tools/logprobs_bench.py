"""Token log-probabilities (``LlamaEngine.set_logprobs``) against the plain decode token, same process, same box, interleaved, on
the synthetic LLaMA-7B of bench.py (weights created on the GPU): ``LlamaEngine.profile_decode`` at 1 and 8 sequence slots,
alternating recording off / on with ``top_n`` 0 and 5, under greedy and under ``temperature=0.7, top_p=0.5``, for --repeats
rounds.  ``misc_ms`` is the launch class that holds the two recording kernels, the opening kernel and the final norm,
``token_ms`` the whole token.
  python tools/logprobs_bench.py [--repeats 5] [--tokens 8] [--layers 32] [--off-only] [--out FILE]  ->  JSON lines (+ the list in FILE)
The yardstick is the recording-off token of the same process and policy: recording "costs" when its median token time exceeds
it by more than the spread (max - min) of the recording-off repeats.  ``--off-only`` measures the recording-off modes alone and
runs on a tree without the feature: the parent commit's token for the same session (the engine geometry — cache_cap 512, 343
cached keys, vocab 32066 — is tools/sampling_bench.py's)."""
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
ap.add_argument("--off-only", action="store_true", help="only the recording-off modes (runs on a tree without the feature)")
ap.add_argument("--out", default=None, help="also write the records as one JSON list to this file")
args = ap.parse_args()
dev, dt = "cuda:0", torch.bfloat16
H, NH, NL, INTER, VOCAB = 4096, 32, args.layers, 11008, 32066
torch.manual_seed(1234)
rnd = lambda *s: torch.randn(*s, device=dev, dtype=dt) * 0.02  # noqa: E731
ones = lambda n: torch.ones(n, device=dev, dtype=dt)  # noqa: E731
shared = dict(layers=[(rnd(3 * H, H), rnd(H, H), rnd(2 * INTER, H), rnd(H, INTER), ones(H), ones(H)) for _ in range(NL)],
              embed=rnd(VOCAB, H), lm_head=rnd(VOCAB, H), final_norm=ones(H))
POLICIES = {"greedy": None, "sampling_T0.7_p0.5": dict(temperature=0.7, top_k=0, top_p=0.5)}
RECORD = {"off": None} if args.off_only else {"off": None, "on_top0": 0, "on_top5": 5}
MODES = [(p, r) for p in POLICIES for r in RECORD]
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
        for policy, record in MODES:
            if POLICIES[policy] is None:
                eng.set_greedy()
            else:
                eng.set_sampling(seed=1234 + r, **POLICIES[policy])
            if not args.off_only:
                eng.set_logprobs(RECORD[record] is not None, top_n=RECORD[record] or 0)
            for b in range(n_seq):
                eng.select(b).set_lengths(343, 343)
            p = eng.profile_decode(args.tokens)
            if r:
                runs[(policy, record)].append(p)
    eng.set_greedy()
    if not args.off_only:
        eng.set_logprobs(False)
    for (policy, record), ps in runs.items():
        tok = [round(p["token_ms"], 4) for p in ps]
        misc = [round(p["misc_ms"], 4) for p in ps]
        emit({"what": "profile_decode", "n_seq": n_seq, "policy": policy, "logprobs": record, "layers": NL, "vocab": VOCAB,
              "token_ms": tok, "token_ms_median": median(tok), "token_ms_spread": round(max(tok) - min(tok), 4), "misc_ms": misc,
              "misc_ms_median": median(misc)})
    for (policy, record), ps in runs.items():
        if record == "off":
            continue
        base = runs[(policy, "off")]
        b_tok = [p["token_ms"] for p in base]
        spread = max(b_tok) - min(b_tok)
        add_tok = median([p["token_ms"] for p in ps]) - median(b_tok)
        add_misc = median([p["misc_ms"] for p in ps]) - median([p["misc_ms"] for p in base])
        emit({"what": "verdict", "n_seq": n_seq, "policy": policy, "logprobs": record, "token_ms_off": round(median(b_tok), 4),
              "added_token_ms": round(add_tok, 4), "added_misc_ms": round(add_misc, 4), "spread_off_ms": round(spread, 4),
              "within_spread": bool(add_tok <= spread)})
    del eng
    torch.cuda.empty_cache()
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)

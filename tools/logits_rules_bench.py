"""The history rules (repetition penalty, no-repeat n-gram, min_new_tokens) against the plain decode token, same process, same box,
interleaved, on the synthetic LLaMA-7B of bench.py (weights created on the GPU): ``LlamaEngine.profile_decode`` at 1 and 8
sequence slots, alternating rules off / rules on (p = 1.2, n = 3, a history of 1500 ids per slot) for --repeats rounds.
``misc_ms`` is the launch class that holds the rules kernel, the opening kernel and the final norm, ``token_ms`` the whole token.
  python tools/logits_rules_bench.py [--repeats 5] [--tokens 8] [--layers 32] [--history 1500] [--out FILE]  ->  JSON lines
The yardstick is the rules-off token of the same process (greedy, what the engine launched before the rules existed): the rules
"cost" when their median token time exceeds it by more than the spread (max - min) of the rules-off repeats.  The engine
geometry (cache_cap 512, 343 cached keys, vocab 32066) is tools/sampling_bench.py's, so its "greedy" line is the same
measurement on a tree without the rules."""
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
ap.add_argument("--history", type=int, default=1500)
ap.add_argument("--out", default=None, help="also write the records as one JSON list to this file")
args = ap.parse_args()
dev, dt = "cuda:0", torch.bfloat16
H, NH, NL, INTER, VOCAB = 4096, 32, args.layers, 11008, 32066
torch.manual_seed(1234)
rnd = lambda *s: torch.randn(*s, device=dev, dtype=dt) * 0.02  # noqa: E731
ones = lambda n: torch.ones(n, device=dev, dtype=dt)  # noqa: E731
shared = dict(layers=[(rnd(3 * H, H), rnd(H, H), rnd(2 * INTER, H), rnd(H, INTER), ones(H), ones(H)) for _ in range(NL)],
              embed=rnd(VOCAB, H), lm_head=rnd(VOCAB, H), final_norm=ones(H))
MODES = {"off": None, "rules_p1.2_n3": dict(repetition_penalty=1.2, no_repeat_ngram_size=3),
         "rules_p1.2_n4_m20": dict(repetition_penalty=1.2, no_repeat_ngram_size=4, min_new_tokens=20)}
# a story-like history: 1500 ids over 400 distinct ones, so ids and trigrams repeat
g = torch.Generator().manual_seed(5)
history = torch.randint(3, 403, (args.history,), generator=g).tolist()
out = []


def emit(rec):
    out.append(rec)
    print(json.dumps(rec), flush=True)


def median(v):
    return sorted(v)[len(v) // 2]


for n_seq in (1, 8):
    # max_new 2048: the history buffer is cache_cap + max_new ids
    eng = LlamaEngine.from_prebuilt(hidden=H, n_heads=NH, n_layers=NL, inter=INTER, vocab=VOCAB, dtype=dt, device=dev, cache_cap=512,
                                    max_new=2048, max_prefill_rows=128, img_ids=(), eos_id=2, n_seq=n_seq,
                                    **shared)
    runs = {m: [] for m in MODES}
    for r in range(args.repeats + 1):                   # round 0 warms every path up and is dropped
        for mode, kw in MODES.items():
            if kw is None:
                eng.clear_logits_rules()
            else:
                eng.set_logits_rules(**kw)
            for b in range(n_seq):
                eng.select(b).set_lengths(343, 343)
                eng.set_history(history, slot=b)
            p = eng.profile_decode(args.tokens)
            if r:
                runs[mode].append(p)
    eng.clear_logits_rules()
    off = runs["off"]
    off_tok = [p["token_ms"] for p in off]
    spread = max(off_tok) - min(off_tok)
    for mode, ps in runs.items():
        tok = [round(p["token_ms"], 4) for p in ps]
        misc = [round(p["misc_ms"], 4) for p in ps]
        emit({"what": "profile_decode", "n_seq": n_seq, "mode": mode, "layers": NL, "vocab": VOCAB, "history": args.history,
              "token_ms": tok, "token_ms_median": median(tok), "token_ms_spread": round(max(tok) - min(tok), 4), "misc_ms": misc,
              "misc_ms_median": median(misc)})
    for mode, ps in runs.items():
        if mode == "off":
            continue
        add_tok = median([p["token_ms"] for p in ps]) - median(off_tok)
        add_misc = median([p["misc_ms"] for p in ps]) - median([p["misc_ms"] for p in off])
        emit({"what": "verdict", "n_seq": n_seq, "mode": mode, "token_ms_off": round(median(off_tok), 4),
              "added_token_ms": round(add_tok, 4), "added_misc_ms": round(add_misc, 4), "spread_off_ms": round(spread, 4),
              "within_spread": bool(add_tok <= spread)})
    del eng
    torch.cuda.empty_cache()
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)

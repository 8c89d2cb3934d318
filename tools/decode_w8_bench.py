"""fp8 (e4m3) weight-only decode against the 16-bit decode, same process, same box, interleaved, on the synthetic LLaMA-7B of
bench.py (weights created on the GPU): whole-token time of ``LlamaEngine.profile_decode`` at 1 and 8 sequence slots, alternating
16-bit / fp8 for --repeats rounds, and the relative error of the fp8 decode's logits and hidden rows against the 16-bit decode of
the same weights under teacher-forced tokens.
  python tools/decode_w8_bench.py [--repeats 5] [--tokens 8] [--layers 32] [--out FILE]  ->  JSON lines (+ the list in FILE)
The option "pays" when the 16-bit token time minus the fp8 token time exceeds the spread (max - min) of the 16-bit repeats."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "seed-story_amd"))
from seedstory import ops  # noqa: E402
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
planes = [tuple(ops.quantize_weight_rows_fp8(w) for w in lw[:4]) for lw in shared["layers"]]
lm8 = ops.quantize_weight_rows_fp8(shared["lm_head"])
out = []


def emit(rec):
    out.append(rec)
    print(json.dumps(rec), flush=True)


def rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


for n_seq in (1, 8):
    eng = LlamaEngine.from_prebuilt(hidden=H, n_heads=NH, n_layers=NL, inter=INTER, vocab=VOCAB, dtype=dt, device=dev, cache_cap=512,
                                    max_new=64, max_prefill_rows=128, img_ids=(), eos_id=2, n_seq=n_seq, **shared)
    runs = {"16bit": [], "fp8": []}
    for r in range(args.repeats + 1):                   # round 0 warms both paths up and is dropped
        for mode in ("16bit", "fp8"):
            if mode == "fp8":
                eng.set_decode_fp8(planes, lm8)
            else:
                eng.disable_decode_fp8()
            for b in range(n_seq):
                eng.select(b).set_lengths(343, 343)
            p = eng.profile_decode(args.tokens)
            if r:
                runs[mode].append(p)
    for mode, ps in runs.items():
        tok = [round(p["token_ms"], 4) for p in ps]
        gms = [p["gemv_ms"] + p["gemv_down_ms"] for p in ps]
        by = ps[0]["gemv_bytes"] + ps[0]["gemv_down_bytes"]
        emit({"what": "profile_decode", "n_seq": n_seq, "mode": mode, "layers": NL, "token_ms": tok, "token_ms_median": sorted(tok)[len(tok) // 2],
              "token_ms_spread": round(max(tok) - min(tok), 4), "gemv_ms_median": round(sorted(gms)[len(gms) // 2], 4),
              "attn_ms": round(ps[0]["attn_ms"], 4), "misc_ms": round(ps[0]["misc_ms"], 4), "gemv_bytes_per_token": by,
              "gemv_GBps": round(by / (sorted(gms)[len(gms) // 2] * 1e-3) / 1e9, 1)})
    a, b = runs["16bit"], runs["fp8"]
    m16, m8 = sorted(p["token_ms"] for p in a)[len(a) // 2], sorted(p["token_ms"] for p in b)[len(b) // 2]
    spread = max(p["token_ms"] for p in a) - min(p["token_ms"] for p in a)
    emit({"what": "verdict", "n_seq": n_seq, "token_ms_16bit": round(m16, 4), "token_ms_fp8": round(m8, 4), "gain_ms": round(m16 - m8, 4),
          "spread_16bit_ms": round(spread, 4), "speedup": round(m16 / m8, 3), "pays": bool(m16 - m8 > spread)})
    if n_seq == 1:      # quality record: teacher-forced decode of the same tokens through both paths
        g = torch.Generator().manual_seed(7)
        emb = shared["embed"][torch.randint(3, 32000, (48,), generator=g).to(dev)]
        forced = torch.randint(3, 32000, (12,), generator=g).tolist()
        res = {}
        for mode in ("16bit", "fp8"):
            if mode == "fp8":
                eng.set_decode_fp8(planes, lm8)
            else:
                eng.disable_decode_fp8()
            eng.select(0).reset()
            eng.prefill(emb)
            n = eng.generate(len(forced), last_prompt_id=5, forced=forced)
            res[mode] = (eng.logits.clone(), eng.hidden_rows[:n - 1].clone())
        emit({"what": "fp8 decode vs 16-bit decode, synthetic N(0, 0.02) weights, teacher-forced", "layers": NL,
              "logits_rel": round(rel(res["fp8"][0], res["16bit"][0]), 5), "hidden_rows_rel": round(rel(res["fp8"][1], res["16bit"][1]), 5)})
    del eng
    torch.cuda.empty_cache()
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)

"""MXFP4 weight-only decode against the fp8 and the 16-bit decode, same process, same box, interleaved, on the synthetic LLaMA-7B of
bench.py (weights created on the GPU): whole-token time of ``LlamaEngine.profile_decode`` at 1 and 8 sequence slots, alternating
16-bit / fp8 / MXFP4 for --repeats rounds; per projection shape the GEMV time of the three options over the 32 layers' planes
in rotation (they never sit in L2 / Infinity Cache); and the relative error of the fp8 and MXFP4 decodes' logits and hidden rows
against the 16-bit decode of the same weights under teacher-forced tokens.
  python tools/decode_mx4_bench.py [--repeats 5] [--tokens 8] [--layers 32] [--gemv-only] [--out FILE] [--quality FILE]  ->  JSON lines
MXFP4 "pays" in a cell when the fp8 token time minus the MXFP4 token time exceeds the spread (max - min) of the fp8 repeats."""
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
ap.add_argument("--gemv-only", action="store_true", help="the per-projection GEMV times alone")
ap.add_argument("--out", default=None, help="also write the records as one JSON list to this file")
ap.add_argument("--quality", default=None, help="also write the quality records as text lines to this file")
args = ap.parse_args()
dev, dt = "cuda:0", torch.bfloat16
H, NH, NL, INTER, VOCAB = 4096, 32, args.layers, 11008, 32066
torch.manual_seed(1234)
rnd = lambda *s: torch.randn(*s, device=dev, dtype=dt) * 0.02  # noqa: E731
ones = lambda n: torch.ones(n, device=dev, dtype=dt)  # noqa: E731
shared = dict(layers=[(rnd(3 * H, H), rnd(H, H), rnd(2 * INTER, H), rnd(H, INTER), ones(H), ones(H)) for _ in range(NL)],
              embed=rnd(VOCAB, H), lm_head=rnd(VOCAB, H), final_norm=ones(H))
planes8 = [tuple(ops.quantize_weight_rows_fp8(w) for w in lw[:4]) for lw in shared["layers"]]
lm8 = ops.quantize_weight_rows_fp8(shared["lm_head"])
planes4 = [tuple(ops.quantize_weight_rows_mxfp4(w) for w in lw[:4]) for lw in shared["layers"]]
lm4 = ops.quantize_weight_rows_mxfp4(shared["lm_head"])
MODES = ("16bit", "fp8", "mxfp4")
out = []


def emit(rec):
    out.append(rec)
    print(json.dumps(rec), flush=True)


def rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


def median(v):
    return sorted(v)[len(v) // 2]


def switch(eng, mode):
    if mode == "fp8":
        eng.set_decode_fp8(planes8, lm8)
    elif mode == "mxfp4":
        eng.set_decode_mxfp4(planes4, lm4)
    else:
        eng.disable_decode_fp8()
        eng.disable_decode_mxfp4()
    assert eng.decode_weights == (None if mode == "16bit" else mode)


def timed(calls, reps=3):
    """us per launch of the rotating `calls`"""
    for c in calls[:2]:
        c()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        for c in calls:
            c()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (reps * len(calls))


# ---- per projection shape: the three GEMV families over the layers' planes in rotation --------------------------------------------
SHAPES = [("qkv+norm", 0, 3 * H, H, dict(norm=True)), ("o+res", 1, H, H, dict(res=True)),
          ("gate|up+norm silu", 2, INTER, H, dict(norm=True, silu=True)), ("down+res", 3, H, INTER, dict(res=True))]
nw = ones(H)
for n_seq in (1, 8):
    for name, j, N, K, kw in SHAPES:
        x = torch.randn(n_seq, K, device=dev, dtype=dt)
        res = torch.randn(n_seq, N, device=dev, dtype=dt)
        ekw = dict(norm_w=nw if kw.get("norm") else None, eps=1e-5, residual=res if kw.get("res") else None, silu_mul=bool(kw.get("silu")))
        rows = 2 * N if kw.get("silu") else N
        us = {"16bit": timed([lambda w=lw[j]: ops.gemv_batched(w, x, **ekw) for lw in shared["layers"]]),
              "fp8": timed([lambda p=pl[j]: ops.gemv_w8(p[0], p[1], x, **ekw) for pl in planes8]),
              "mxfp4": timed([lambda p=pl[j]: ops.gemv_mx4(p[0], p[1], x, **ekw) for pl in planes4])}
        by = {"16bit": rows * K * 2, "fp8": rows * K + 4 * rows, "mxfp4": rows * K // 2 + rows * K // 32}
        emit({"what": "gemv", "shape": name, "N": N, "K": K, "n_seq": n_seq, "layers_in_rotation": NL,
              "us": {m: round(us[m], 2) for m in MODES}, "GBps_own_bytes": {m: round(by[m] / us[m] / 1e3, 1) for m in MODES}})

quality = []
for n_seq in (() if args.gemv_only else (1, 8)):
    eng = LlamaEngine.from_prebuilt(hidden=H, n_heads=NH, n_layers=NL, inter=INTER, vocab=VOCAB, dtype=dt, device=dev, cache_cap=512,
                                    max_new=64, max_prefill_rows=128, img_ids=(), eos_id=2, n_seq=n_seq, **shared)
    runs = {m: [] for m in MODES}
    for r in range(args.repeats + 1):                   # round 0 warms every path up and is dropped
        for mode in MODES:
            switch(eng, mode)
            for b in range(n_seq):
                eng.select(b).set_lengths(343, 343)
            p = eng.profile_decode(args.tokens)
            if r:
                runs[mode].append(p)
    for mode, ps in runs.items():
        tok = [round(p["token_ms"], 4) for p in ps]
        gms = [p["gemv_ms"] + p["gemv_down_ms"] for p in ps]
        by = ps[0]["gemv_bytes"] + ps[0]["gemv_down_bytes"]
        emit({"what": "profile_decode", "n_seq": n_seq, "mode": mode, "layers": NL, "token_ms": tok, "token_ms_median": median(tok),
              "token_ms_spread": round(max(tok) - min(tok), 4), "gemv_ms_median": round(median(gms), 4),
              "attn_ms": round(ps[0]["attn_ms"], 4), "misc_ms": round(ps[0]["misc_ms"], 4), "gemv_bytes_per_token": by,
              "gemv_GBps": round(by / (median(gms) * 1e-3) / 1e9, 1)})
    t = {m: [p["token_ms"] for p in runs[m]] for m in MODES}
    spread = {m: max(t[m]) - min(t[m]) for m in MODES}
    m16, m8, m4 = (median(t[m]) for m in MODES)
    emit({"what": "verdict", "n_seq": n_seq, "token_ms_16bit": round(m16, 4), "token_ms_fp8": round(m8, 4), "token_ms_mxfp4": round(m4, 4),
          "spread_16bit_ms": round(spread["16bit"], 4), "spread_fp8_ms": round(spread["fp8"], 4),
          "gain_over_fp8_ms": round(m8 - m4, 4), "speedup_over_fp8": round(m8 / m4, 3), "speedup_over_16bit": round(m16 / m4, 3),
          "pays_over_fp8": bool(m8 - m4 > spread["fp8"]), "pays_over_16bit": bool(m16 - m4 > spread["16bit"])})
    if n_seq == 1:      # quality record: teacher-forced decode of the same tokens through the three paths
        g = torch.Generator().manual_seed(7)
        emb = shared["embed"][torch.randint(3, 32000, (48,), generator=g).to(dev)]
        forced = torch.randint(3, 32000, (12,), generator=g).tolist()
        res = {}
        for mode in MODES:
            switch(eng, mode)
            eng.select(0).reset()
            eng.prefill(emb)
            n = eng.generate(len(forced), last_prompt_id=5, forced=forced)
            res[mode] = (eng.logits.clone(), eng.hidden_rows[:n - 1].clone())
        for mode in MODES[1:]:
            rec = {"what": "%s decode vs 16-bit decode, synthetic N(0, 0.02) weights, teacher-forced" % mode, "layers": NL,
                   "logits_rel": round(rel(res[mode][0], res["16bit"][0]), 5), "hidden_rows_rel": round(rel(res[mode][1], res["16bit"][1]), 5)}
            emit(rec)
            quality.append(rec)
    del eng
    torch.cuda.empty_cache()
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
if args.quality:
    with open(args.quality, "w") as f:
        f.write("MXFP4 / fp8 weight-only decode against the 16-bit decode of the same synthetic LLaMA-7B weights (N(0, 0.02), %d layers),\n"
                "48 prompt rows, 12 teacher-forced tokens; relative Frobenius distance.  Synthetic weights only: end quality on a real\n"
                "checkpoint has not been measured.\n" % NL)
        for rec in quality:
            f.write(json.dumps(rec) + "\n")

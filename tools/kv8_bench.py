"""The fp8 (e4m3) KV shadow cache (kv_cache="fp8") against the 16-bit decode attention, same process, same box, interleaved, on the
synthetic LLaMA-7B of bench.py (weights and cache contents created on the GPU): attention-class and whole-token time of
``LlamaEngine.profile_decode`` at 1 and 8 sequence slots, about 400 and about 1100 cached positions, with and without fp8 decode
weights, alternating option off / on for --repeats rounds; and the relative distance of a teacher-forced fp8-KV decode's logits
and hidden rows from the 16-bit decode of the same weights.
  python tools/kv8_bench.py [--repeats 5] [--tokens 8] [--layers 32] [--out profiles/kv8_decode.json] [--off-only]
The option "pays" in a cell when the option-off token time minus the option-on token time exceeds the spread (max - min) of the
option-off repeats of that cell.  --off-only measures the option-off cells alone (a library without the option can run it)."""
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
ap.add_argument("--off-only", action="store_true")
args = ap.parse_args()
dev, dt = "cuda:0", torch.bfloat16
H, NH, NL, INTER, VOCAB, CAP = 4096, 32, args.layers, 11008, 32066, 1152
torch.manual_seed(1234)
rnd = lambda *s: torch.randn(*s, device=dev, dtype=dt) * 0.02  # noqa: E731
ones = lambda n: torch.ones(n, device=dev, dtype=dt)  # noqa: E731
shared = dict(layers=[(rnd(3 * H, H), rnd(H, H), rnd(2 * INTER, H), rnd(H, INTER), ones(H), ones(H)) for _ in range(NL)],
              embed=rnd(VOCAB, H), lm_head=rnd(VOCAB, H), final_norm=ones(H))
planes = [tuple(ops.quantize_weight_rows_fp8(w) for w in lw[:4]) for lw in shared["layers"]]
lm8 = ops.quantize_weight_rows_fp8(shared["lm_head"])
modes = ("off",) if args.off_only else ("off", "on")
out = []


def emit(rec):
    out.append(rec)
    print(json.dumps(rec), flush=True)


def rel(a, b):
    return float((a.float() - b.float()).norm() / b.float().norm())


def med(v):
    return sorted(v)[len(v) // 2]


def kv8(eng, on):
    if args.off_only:
        return
    if on and eng.kv_cache != "fp8":
        eng.enable_kv_fp8()
    elif not on and eng.kv_cache == "fp8":
        eng.disable_kv_fp8()


for n_seq in (1, 8):
    eng = LlamaEngine.from_prebuilt(hidden=H, n_heads=NH, n_layers=NL, inter=INTER, vocab=VOCAB, dtype=dt, device=dev, cache_cap=CAP,
                                    max_new=64, max_prefill_rows=128, img_ids=(), eos_id=2, n_seq=n_seq, **shared)
    for b in range(n_seq):      # cache contents of the magnitude real keys / values have, not the workspace's zeros
        eng.select(b)
        eng.k_cache.normal_()
        eng.v_cache.normal_()
    for w8 in (False, True):
        if w8:
            eng.set_decode_fp8(planes, lm8)
        else:
            eng.disable_decode_fp8()
        for kv_len in (400, 1100):
            runs = {m: [] for m in modes}
            for r in range(args.repeats + 1):               # round 0 warms both paths up and is dropped
                for mode in modes:
                    kv8(eng, mode == "on")
                    for b in range(n_seq):
                        eng.select(b).set_lengths(kv_len, kv_len)
                    p = eng.profile_decode(args.tokens)
                    if r:
                        runs[mode].append(p)
            kv8(eng, False)
            cell = {"what": "cell", "n_seq": n_seq, "kv_len": kv_len, "decode_weights": "fp8" if w8 else "16bit", "layers": NL,
                    "tokens": args.tokens}
            for mode, ps in runs.items():
                tok, att = [p["token_ms"] for p in ps], [p["attn_ms"] for p in ps]
                cell.update({"token_ms_" + mode: round(med(tok), 4), "attn_ms_" + mode: round(med(att), 4),
                             "token_ms_%s_runs" % mode: [round(t, 4) for t in tok], "attn_ms_%s_runs" % mode: [round(t, 4) for t in att]})
            tok_off = [p["token_ms"] for p in runs["off"]]
            cell["token_ms_off_spread"] = round(max(tok_off) - min(tok_off), 4)
            if "on" in runs:
                gain = cell["token_ms_off"] - cell["token_ms_on"]
                cell.update({"gain_ms": round(gain, 4), "attn_gain_ms": round(cell["attn_ms_off"] - cell["attn_ms_on"], 4),
                             "pays": bool(gain > cell["token_ms_off_spread"])})
            emit(cell)
    if n_seq == 1 and not args.off_only:      # quality record: teacher-forced decode of the same tokens through both paths
        eng.disable_decode_fp8()
        g = torch.Generator().manual_seed(7)
        emb = shared["embed"][torch.randint(3, 32000, (48,), generator=g).to(dev)]
        forced = torch.randint(3, 32000, (12,), generator=g).tolist()
        res = {}
        for mode in modes:
            kv8(eng, mode == "on")
            eng.select(0).reset()
            eng.prefill(emb)
            n = eng.generate(len(forced), last_prompt_id=5, forced=forced)
            res[mode] = (eng.logits.clone(), eng.hidden_rows[:n - 1].clone())
        kv8(eng, False)
        emit({"what": "fp8-KV decode vs 16-bit decode, synthetic N(0, 0.02) weights, teacher-forced, 48-row prompt + 12 tokens", "layers": NL,
              "logits_rel": round(rel(res["on"][0], res["off"][0]), 5), "hidden_rows_rel": round(rel(res["on"][1], res["off"][1]), 5)})
    del eng
    torch.cuda.empty_cache()
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)

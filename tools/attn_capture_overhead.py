"""What attention-map capture costs at the real LLaMA-2-7B shapes (bf16, synthetic weights) -> one JSON line.

    python tools/attn_capture_overhead.py off          # capture OFF: whole decode token (ss_llama_profile_decode index 4), 8 slots
    python tools/attn_capture_overhead.py on           # capture ON vs OFF: a 2,500-row prefill and a decode token, one slot

``off`` is run once per build, alternating (``SEEDSTORY_HIP_LIB`` picks the library; a library from before the capture entry
points existed is accepted): the two builds' difference must lie inside the spread of one build's own runs.  A run's
records belong in profiles/attn_capture_overhead.json (DESIGN 6.0c says whether one has been recorded).
"""
import ctypes
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seed-story_amd"))
from seedstory import _lib  # noqa: E402

DEV = "cuda:0"
H, I, V, NH, NL = 4096, 11008, 32066, 32, 32


def load_lib():
    probe = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("ss_attn_scores", "ss_llama_set_attn_capture"):
        if not hasattr(probe, name):
            _lib.PROTOTYPES.pop(name)          # an older build: time what it has
    _lib.lib()


def engine(n_seq, cache_cap, max_new, max_rows):
    from seedstory.llama import LlamaEngine
    dt = torch.bfloat16
    g = torch.Generator(device=DEV).manual_seed(1)

    def rnd(*s):
        return torch.randn(*s, device=DEV, dtype=dt, generator=g) * 0.02

    ones = lambda: torch.ones(H, device=DEV, dtype=dt)      # noqa: E731
    layers = [(rnd(3 * H, H), rnd(H, H), rnd(2 * I, H), rnd(H, I), ones(), ones()) for _ in range(NL)]
    return LlamaEngine.from_prebuilt(embed=rnd(V, H), lm_head=rnd(V, H), final_norm=ones(), layers=layers, hidden=H, n_heads=NH,
                                     n_layers=NL, inter=I, vocab=V, dtype=dt, device=DEV, cache_cap=cache_cap, max_new=max_new,
                                     max_prefill_rows=max_rows, img_ids=list(range(32000, 32066)), n_seq=n_seq)


def mode_off():
    eng = engine(8, 1152, 512, 1024)
    kv = 343

    def rewind():
        for b in range(8):
            eng.select(b).set_lengths(kv + 3 * b, kv + 3 * b)

    rewind()
    eng.profile_decode(8)
    reps = []
    for _ in range(7):
        rewind()
        reps.append(eng.profile_decode(16)["token_ms"])
    return dict(mode="off", lib=_lib.LIB_PATH, slots=8, kv_len=kv, token_ms=[round(x, 4) for x in reps],
                token_ms_median=round(statistics.median(reps), 4))


def mode_on():
    S, n_tok = 2500, 64
    eng = engine(1, 3072, 128, 2560)
    g = torch.Generator(device=DEV).manual_seed(2)
    emb = torch.randn(S, H, device=DEV, dtype=torch.bfloat16, generator=g) * 0.02
    forced = torch.randint(3, 32000, (n_tok,), generator=torch.Generator().manual_seed(3)).tolist()

    def prefill_ms():
        eng.reset()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.prefill(emb)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def decode_ms():
        eng.set_lengths(S, S)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        n = eng.generate(n_tok, 5, forced)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / n

    res = {"prefill_ms": {"off": [], "on": []}, "decode_token_ms": {"off": [], "on": []}}
    prefill_ms(), decode_ms()                                   # tile lookups, the capture-off graph
    for rep in range(4):
        for state in ("off", "on"):
            if state == "on":
                eng.reset()
                eng.attn_capture_on(S + n_tok, S + n_tok)
            p, d = prefill_ms(), decode_ms()
            eng.attn_capture_off()
            if rep:                                             # the first round instantiates the capture-on graph
                res["prefill_ms"][state].append(round(p, 3))
                res["decode_token_ms"][state].append(round(d, 4))
    out = dict(mode="on", lib=_lib.LIB_PATH, prompt_rows=S, decode_tokens=n_tok, map_bytes_per_layer=S * S * 2, **res)
    for k in ("prefill_ms", "decode_token_ms"):
        off, on = statistics.median(res[k]["off"]), statistics.median(res[k]["on"])
        out[k + "_overhead"] = dict(off=off, on=on, delta=round(on - off, 4), percent=round(100.0 * (on - off) / off, 2))
    return out


if __name__ == "__main__":
    load_lib()
    print(json.dumps(mode_off() if sys.argv[1] == "off" else mode_on()))

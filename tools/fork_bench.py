"""Slot fork (``ss_llama_fork`` / ``LlamaEngine.fork``) and best-of-n sampling on the synthetic LLaMA-7B of bench.py (weights created
on the GPU), one process, the compared variants interleaved:
  fork          one slot forked to the 7 others at 400 and 1100 cached positions, against the same bytes moved by device-to-device
                plane copies (``hipMemcpy2DAsync``, one per K | V slab and destination: 14 calls) issued from this tool, and against
                what the fork replaces: prefilling the same prompt into the 7 other slots;
  generate      a whole ``LlamaForCausalLM.generate`` of a 600-position prompt + 50 sampled tokens with ``num_return_sequences`` 1, 4, 8.
  python tools/fork_bench.py [--repeats 5] [--layers 32] [--out profiles/best_of_n.json]  ->  JSON lines (+ the list in FILE)
GB/s counts one read plus seven writes of the K and V rows below the cache length.  Round 0 warms every path up and is dropped."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "seed-story_amd"))
from seedstory import ops  # noqa: E402
from seedstory.llama import _prefill_chunked  # noqa: E402
from src.models_clm.modeling_llama_xformer import LlamaConfig, LlamaForCausalLM  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--out", default=None, help="also write the records as one JSON list to this file")
args = ap.parse_args()
dev, dt = "cuda:0", torch.bfloat16
H, NH, NL, INTER, VOCAB, CAP, S8 = 4096, 32, args.layers, 11008, 32066, 1280, 8
HD = H // NH
torch.manual_seed(1234)
out = []


def emit(rec):
    out.append(rec)
    print(json.dumps(rec), flush=True)


def med(v):
    return sorted(v)[len(v) // 2]


def hip_runtime():
    """the HIP runtime this process already has loaded (torch's copy)"""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return C.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime loaded")


def timed(fn):
    """device time of fn() on the current stream, ms"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


torch.set_default_dtype(dt)
with torch.device(dev):
    llm = LlamaForCausalLM(LlamaConfig(hidden_size=H, intermediate_size=INTER, num_hidden_layers=NL, num_attention_heads=NH,
                                       vocab_size=VOCAB))
torch.set_default_dtype(torch.float32)
llm.init_synthetic()
llm.cache_cap, llm.max_new, llm.max_prefill_rows, llm.n_seq = CAP, 64, 1280, S8
llm.use_kv_cache_head = False
eng = llm.engine_for_generation(())
embed = llm.model.embed_tokens.weight.data
hip = hip_runtime()
hip.hipMemcpy2DAsync.restype = C.c_int
hip.hipMemcpy2DAsync.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int, C.c_void_p]
D2D = 3


def copy_chain(kv_len):
    """slot 0's rows [0, kv_len) of every (layer, head) to the 7 other slots: one 2-D copy per slab and destination"""
    pitch, width, height = CAP * HD * 2, kv_len * HD * 2, NL * NH
    src = (eng.select(0).k_cache.data_ptr(), eng.v_cache.data_ptr())
    for b in range(1, S8):
        eng.select(b)
        for d, s in zip((eng.k_cache.data_ptr(), eng.v_cache.data_ptr()), src):
            rc = hip.hipMemcpy2DAsync(d, pitch, s, pitch, width, height, D2D, ops.stream())
            assert rc == 0, rc
    eng.select(0)


def prefill_others(emb):
    for b in range(1, S8):
        eng.select(b).reset()
        _prefill_chunked(eng, emb, False)
    eng.select(0)


g = torch.Generator().manual_seed(7)
for kv_len in (400, 1100):
    emb = embed[torch.randint(3, 32000, (kv_len,), generator=g).to(dev)]
    eng.select(0).reset()
    _prefill_chunked(eng, emb, False)
    runs = {"fork": [], "copy_chain": [], "prefill_x7": []}
    for r in range(args.repeats + 1):
        for name, fn in (("fork", lambda: eng.fork(0)), ("copy_chain", lambda: copy_chain(kv_len)), ("prefill_x7", lambda: prefill_others(emb))):
            ms = timed(fn)
            if r:
                runs[name].append(round(ms, 4))
    # the fork's result against the source, once per length (the copy chain and the prefills wrote the same rows: cleared first)
    for b in range(1, S8):
        eng.select(b).k_cache[:, :, :kv_len].zero_()
    eng.fork(0)
    k0 = eng.select(0).k_cache[:, :, :kv_len].clone()
    ok = all(torch.equal(eng.select(b).k_cache[:, :, :kv_len], k0) and eng.lengths() == (kv_len, kv_len) for b in range(1, S8))
    eng.select(0)
    gb = 2 * NL * NH * kv_len * HD * 2 * 8 / 1e9           # K and V, one read + seven writes
    rec = {"what": "fork 1 -> 7 slots", "kv_len": kv_len, "layers": NL, "bytes_read_GB": round(gb / 8, 3), "bytes_written_GB": round(gb * 7 / 8, 3),
           "copies_bit_equal": bool(ok)}
    for name, v in runs.items():
        rec.update({name + "_ms": med(v), name + "_ms_runs": v})
    rec.update({"fork_GBps": round(gb / (rec["fork_ms"] * 1e-3), 1), "copy_chain_GBps": round(gb / (rec["copy_chain_ms"] * 1e-3), 1),
                "fork_not_slower_than_copy_chain": bool(rec["fork_ms"] <= rec["copy_chain_ms"]),
                "prefill_x7_over_fork": round(rec["prefill_x7_ms"] / rec["fork_ms"], 1)})
    emit(rec)

# a whole generate: 600-position prompt, 50 sampled tokens, 1 / 4 / 8 candidates (the slots of one engine)
ids = torch.randint(3, 32000, (1, 600), generator=g)
kw = dict(input_ids=ids, inputs_embeds=embed[ids.to(dev)], max_new_tokens=50, do_sample=True, temperature=1.0, top_k=0, top_p=0.9,
          output_hidden_states=True)
runs = {1: [], 4: [], 8: []}
toks = {}
for r in range(args.repeats + 1):
    for n in runs:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        o = llm.generate(seed=100 + r, **({"num_return_sequences": n} if n > 1 else {}), **kw)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        if r:
            runs[n].append(round(ms, 2))
        toks[n] = [c.sequences.shape[1] - 600 for c in o.candidates] if n > 1 else [o.sequences.shape[1] - 600]
for n, v in runs.items():
    emit({"what": "generate, 600-position prompt + 50 sampled tokens", "num_return_sequences": n, "layers": NL, "ms": med(v), "ms_runs": v,
          "tokens_per_candidate_last_run": toks[n], "ms_per_candidate": round(med(v) / n, 2),
          "over_one_sequence": round(med(v) / med(runs[1]), 3)})
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
llm._engine = None      # the engine goes while the library is still loaded
del eng

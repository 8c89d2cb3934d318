"""Beam search on the device (``ss_llama_beam_search`` / ``LlamaEngine.beam_search``) on the synthetic LLaMA-7B of bench.py (weights
created on the GPU), one process, the compared variants interleaved:
  token         the whole decode token of a search with n = 4 and n = 8 beams at 400 and 1100 cached positions (a 32-step search,
                fork and done polls included, divided by the steps it ran), against this tree's lock-step greedy token at the same
                slot count (``generate_batch`` of 32 tokens): the difference is top-K + advance + permute; the permutation alone
                (a rotation of all n slots over a 16- and a 32-row suffix) is timed through the test hook;
  generate      a whole ``LlamaForCausalLM.generate`` of a 600-position prompt + 50 tokens: greedy, ``num_beams=4``, and best-of-4
                (``do_sample=True, num_return_sequences=4``) for comparison.
  python tools/beam_bench.py [--repeats 5] [--layers 32] [--out profiles/beam_search.json]  ->  JSON lines (+ the list in FILE)
Round 0 warms every path up (graph capture included) and is dropped.  Synthetic weights: near-uniform logits, so what the search
chooses says nothing about caption quality; only the times mean something."""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "seed-story_amd"))
from seedstory.llama import _prefill_chunked  # noqa: E402
from src.models_clm.modeling_llama_xformer import LlamaConfig, LlamaForCausalLM  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--layers", type=int, default=32)
ap.add_argument("--out", default=None, help="also write the records as one JSON list to this file")
args = ap.parse_args()
dev, dt = "cuda:0", torch.bfloat16
H, NH, NL, INTER, VOCAB, CAP, STEPS = 4096, 32, args.layers, 11008, 32066, 1280, 32
torch.manual_seed(1234)
out = []


def emit(rec):
    out.append(rec)
    print(json.dumps(rec), flush=True)


def med(v):
    return sorted(v)[len(v) // 2]


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
llm.cache_cap, llm.max_new, llm.max_prefill_rows = CAP, 64, 1280
llm.use_kv_cache_head = False
embed = llm.model.embed_tokens.weight.data
g = torch.Generator().manual_seed(7)

for n in (4, 8):
    llm.n_seq = n
    eng = llm.engine_for_generation(())
    for kv_len in (400, 1100):
        emb = embed[torch.randint(3, 32000, (kv_len,), generator=g).to(dev)]
        runs = {"beam": [], "greedy": [], "permute16": [], "permute32": []}
        steps = 0

        def prompt():
            eng.select(0).reset()
            _prefill_chunked(eng, emb, False)

        def beam():
            global steps
            # "never" with a positive length penalty: the search runs to its step limit whatever the scores are
            eng.beam_search(STEPS, 5, n, length_penalty=1.0, early_stopping="never")
            steps = eng.last_beam_state.step

        for r in range(args.repeats + 1):
            prompt()
            ms = timed(beam)
            if r:
                runs["beam"].append(round(ms / steps, 4))
            prompt()
            eng.fork(0)
            ms = timed(lambda: eng.generate_batch(STEPS, [5] * n))
            if r:
                runs["greedy"].append(round(ms / STEPS, 4))            # (in both, the token at the limit stops before its forward)
            for rows in (16, 32):
                for b in range(n):
                    eng.select(b).set_lengths(kv_len + rows, kv_len + rows)
                eng.select(0)
                ms = timed(lambda: eng._beam_permute([(b + 1) % n for b in range(n)], kv_len))
                if r:
                    runs["permute%d" % rows].append(round(ms, 4))
        rec = {"what": "decode token, beam search vs lock-step greedy", "num_beams": n, "kv_len": kv_len, "layers": NL,
               "steps_run": steps}
        for name, v in runs.items():
            rec.update({name + "_ms": med(v), name + "_ms_runs": v})
        rec["beam_minus_greedy_ms"] = round(rec["beam_ms"] - rec["greedy_ms"], 4)
        rec["note"] = "both: a 32-token call (state upload, done polls; the search also its fork) divided by the tokens it ran"
        emit(rec)
    llm._engine = None
    del eng

# a whole generate: 600-position prompt + 50 tokens
llm.n_seq = 4
ids = torch.randint(3, 32000, (1, 600), generator=g)
kw = dict(input_ids=ids, inputs_embeds=embed[ids.to(dev)], max_new_tokens=50, output_hidden_states=True)
variants = {"greedy": {}, "num_beams=4": dict(num_beams=4, early_stopping="never"),
            "best-of-4": dict(do_sample=True, temperature=1.0, top_k=0, top_p=0.9, num_return_sequences=4)}
runs = {k: [] for k in variants}
toks = {}
for r in range(args.repeats + 1):
    for name, extra in variants.items():
        llm.beam_search = name == "num_beams=4"
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        o = llm.generate(**({"seed": 100 + r} if "do_sample" in extra else {}), **extra, **kw)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        if r:
            runs[name].append(round(ms, 2))
        toks[name] = int(o.sequences.shape[1] - 600)
llm.beam_search = False
for name, v in runs.items():
    emit({"what": "generate, 600-position prompt + 50 tokens", "variant": name, "layers": NL, "ms": med(v), "ms_runs": v,
          "tokens_last_run": toks[name], "over_greedy": round(med(v) / med(runs["greedy"]), 3)})
if args.out:
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
llm._engine = None      # the engine goes while the library is still loaded

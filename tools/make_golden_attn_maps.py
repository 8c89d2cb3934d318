"""TEST INFRASTRUCTURE ONLY — records the attention maps the REAL reference LlamaForCausalLM returns under
``output_attentions=True`` and writes them to ``tests/golden/attn_maps_tiny.safetensors``.

Run where the reference tree is present (like the ``oracle/make_golden*.py`` recipes, it imports the reference classes through
``oracle/ref_shims.py`` and only calls them):

    python tools/make_golden_attn_maps.py [--out FILE]

Same tiny config, weights (seed 11) and inputs (``synth.randint(5 | 6 | 7, ...)``) as ``golden_llama`` of
``oracle/make_golden.py``: a prefill of 37 rows, a continuation of 9 rows on the cached prefix, one decode row — in fp32, bf16
and fp16.  Per call and layer the reference returns ``[1, q, kv]``: head 0, pre-softmax scores, the mask added in the model
dtype.  Stored in the model dtype under ``<tag>.<call>.<layer>``.
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

LLAMA = dict(hidden=256, n_heads=2, n_layers=2, inter=512, vocab=320)
DTYPES = ((torch.float32, "f32"), (torch.bfloat16, "bf16"), (torch.float16, "f16"))
CALLS = ("prefill", "cont", "decode")
OUT = os.path.join(ROOT, "tests", "golden", "attn_maps_tiny.safetensors")


def record(llama_mod, dtype, tag, out):
    import synth
    from transformers import LlamaConfig
    d = LLAMA
    cfg = LlamaConfig(hidden_size=d["hidden"], intermediate_size=d["inter"], num_hidden_layers=d["n_layers"],
                      num_attention_heads=d["n_heads"], vocab_size=d["vocab"], max_position_embeddings=4096,
                      rms_norm_eps=1e-5)
    wd = synth.llama_weights(11, d["hidden"], d["n_heads"], d["n_layers"], d["inter"], d["vocab"], dtype=dtype)
    m = llama_mod.LlamaForCausalLM(cfg).eval()
    missing, unexpected = m.load_state_dict(wd, strict=False)
    assert not unexpected and all("rotary" in k or "inv_freq" in k for k in missing), (missing, unexpected)
    m = m.to(dtype)
    m.use_kv_cache_head = False
    past, pos = None, 0
    with torch.no_grad():
        for call, seed, rows in zip(CALLS, (5, 6, 7), (37, 9, 1)):
            ids = synth.randint(seed, (1, rows), 3, 250)
            emb = wd["model.embed_tokens.weight"][ids]
            r = m(inputs_embeds=emb, position_ids=torch.arange(pos, pos + rows).unsqueeze(0), past_key_values=past,
                  use_cache=True, output_attentions=True, output_hidden_states=True, return_dict=True)
            past, pos = r.past_key_values, pos + rows
            assert len(r.attentions) == d["n_layers"]
            for l, a in enumerate(r.attentions):
                assert a.shape == (1, rows, pos) and a.dtype == dtype, (a.shape, a.dtype)
                out["%s.%s.%d" % (tag, call, l)] = a[0].contiguous()


def build():
    import ref_shims
    torch.set_num_threads(8)
    llama_mod = ref_shims.import_reference()[0]
    out = {}
    for dtype, tag in DTYPES:
        record(llama_mod, dtype, tag, out)
    return out


def main():
    import argparse
    from safetensors.torch import save_file
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=OUT, help="file to write (default: the committed fixture)")
    path = ap.parse_args().out
    out = build()
    save_file(out, path)
    print("wrote %d tensors, %.1f KiB" % (len(out), os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()

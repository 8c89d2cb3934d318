"""Render loop only (latent output, no VAE) with limited-interval guidance: the synthetic SDXL-base UNet at 1024 x 1024, 8 images
per render (UNet batch 16 on guided steps, 8 on unguided ones), Euler-30 and DPM++ 2M Karras-20, each with the interval off,
(0.25, 6.0) and (0.25, inf), alternating in one process.
    python tools/guidance_bench.py [--repeats 5] [--images 8] [--out profiles/guidance_interval.json]
One warm-up render per variant first (GEMM tuning of the batch-8 shapes, graph capture of both forms).  Reports, per variant, the
mask, ms per render (median, min, max over the repeats) and, from replays of the two captured forwards on their own, the time of one
forward of each form, their ratio r = batch-8 / batch-16, and how far the measured loop is from guided + r * unguided forwards."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seed-story_amd"))
import torch  # noqa: E402

from seedstory import tune  # noqa: E402
from seedstory.diffusion import (DPMSolverMultistepScheduler, EulerDiscreteScheduler, StableDiffusionXLPipeline,  # noqa: E402
                                 UNet2DConditionModel)

SAMPLERS = (("euler_30", "euler", 30), ("dpmpp2m_karras_20", "dpmpp", 20))
INTERVALS = (("off", None), ("0.25_6", (0.25, 6.0)), ("0.25_inf", (0.25, math.inf)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--forward-replays", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "guidance_interval.json"))
    args = ap.parse_args()
    dev, dt, B = "cuda:0", torch.bfloat16, args.images
    unet = UNet2DConditionModel().to(dev, dt).init_synthetic(4)
    pipes = {"euler": StableDiffusionXLPipeline(vae=None, unet=unet, scheduler=EulerDiscreteScheduler()),
             "dpmpp": StableDiffusionXLPipeline(vae=None, unet=unet, scheduler=DPMSolverMultistepScheduler(use_karras_sigmas=True))}
    g = torch.Generator(device=dev).manual_seed(0)
    kw = dict(prompt_embeds=torch.randn(B, 64, 2048, device=dev, dtype=dt, generator=g),
              negative_prompt_embeds=torch.randn(B, 64, 2048, device=dev, dtype=dt, generator=g),
              pooled_prompt_embeds=torch.randn(B, 1280, device=dev, dtype=dt, generator=g),
              negative_pooled_prompt_embeds=torch.randn(B, 1280, device=dev, dtype=dt, generator=g),
              latents=torch.randn(B, 4, args.size // 8, args.size // 8, device=dev, dtype=dt, generator=g),
              guidance_scale=7.5, height=args.size, width=args.size, output_type="latent")
    variants = [(s + "/" + i, which, steps, interval) for s, which, steps in SAMPLERS for i, interval in INTERVALS]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def render_ms(which, steps, interval):
        ms, out = timed(lambda: pipes[which](num_inference_steps=steps, guidance_interval=interval, **kw).images)
        assert bool(torch.isfinite(out.float()).all())
        return ms

    tuned_before = len(tune.tuned_log())
    masks = {}
    for name, which, steps, interval in variants:
        print("warm-up %-28s %.1f ms" % (name, render_ms(which, steps, interval)), flush=True)
        masks[name] = list(pipes[which].last_guidance["mask"])
        print("        mask %s" % "".join("G" if m else "u" for m in masks[name]), flush=True)
    tuned = tune.tuned_log()[tuned_before:]
    ms = {v[0]: [] for v in variants}
    graphs_before = {which: {k: e["g"] for k, e in p._graphs.items() if e is not None} for which, p in pipes.items()}
    for r in range(args.repeats):
        for name, which, steps, interval in variants:
            ms[name].append(render_ms(which, steps, interval))
            print("repeat %d %-28s %.1f ms" % (r, name, ms[name][-1]), flush=True)
    recaptured = any(p._graphs.get(k) is None or p._graphs[k]["g"] is not gobj
                     for which, p in pipes.items() for k, gobj in graphs_before[which].items())

    # one forward of each form on its own: replays of the captured graphs (key[0][0] is the UNet batch)
    forward_ms = {}
    for which, p in pipes.items():
        for key, ent in p._graphs.items():
            if ent is None:
                continue
            ent["temb"].copy_(ent["temb_table"][1])
            ent["g"].replay()
            torch.cuda.synchronize()
            reps = [timed(ent["g"].replay)[0] for _ in range(args.forward_replays)]
            forward_ms.setdefault(key[0][0], []).extend(reps)
    fwd = {b: statistics.median(v) for b, v in forward_ms.items()}
    res = {"device": torch.cuda.get_device_name(0), "images_per_render": B, "unet_batch_guided": 2 * B, "unet_batch_unguided": B,
           "size": args.size, "dtype": "bf16", "repeats": args.repeats,
           "forward_ms": {str(b): {"median": round(fwd[b], 3), "min": round(min(forward_ms[b]), 3), "max": round(max(forward_ms[b]), 3),
                                   "replays": len(forward_ms[b])} for b in sorted(fwd)},
           "graphs_recaptured_during_repeats": recaptured,
           "shapes_tuned_in_warm_up": [{"kind": t[0], "shape": list(t[1]), "cfg": t[2], "xcd_group": t[3], "best_us": round(t[4], 2)}
                                       for t in tuned],
           "variants": {}}
    if B in fwd and 2 * B in fwd:
        res["r_unguided_over_guided_forward"] = round(fwd[B] / fwd[2 * B], 4)
    for name, which, steps, interval in variants:
        mask = masks[name]
        med = statistics.median(ms[name])
        v = {"steps": steps, "interval": None if interval is None else [interval[0], "inf" if math.isinf(interval[1]) else interval[1]],
             "mask": "".join("G" if m else "u" for m in mask), "guided_steps": sum(mask), "unguided_steps": steps - sum(mask),
             "render_ms_median": round(med, 2), "render_ms_min": round(min(ms[name]), 2), "render_ms_max": round(max(ms[name]), 2),
             "spread_rel": round((max(ms[name]) - min(ms[name])) / med, 4), "render_ms": [round(x, 2) for x in ms[name]]}
        if B in fwd and 2 * B in fwd:
            exp = sum(mask) * fwd[2 * B] + (steps - sum(mask)) * fwd[B]
            v["forwards_alone_ms"] = round(exp, 2)                      # guided + r * unguided forwards, nothing else
            v["render_over_forwards_alone"] = round(med / exp, 4)
        res["variants"][name] = v
    for s, _, _ in SAMPLERS:
        off = res["variants"][s + "/off"]["render_ms_median"]
        for i, _ in INTERVALS[1:]:
            res["variants"][s + "/" + i]["render_vs_interval_off"] = round(res["variants"][s + "/" + i]["render_ms_median"] / off, 4)
    torch.cuda.synchronize()
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

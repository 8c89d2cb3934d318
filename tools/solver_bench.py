"""Render loop only (latent output, no VAE): the synthetic SDXL-base UNet at 1024 x 1024, 8 images per render (UNet batch 16),
under Euler-30, DPM++ 2M Karras-20 and DPM++ 2M Karras-15, alternating in one process.
    python tools/solver_bench.py [--repeats 5] [--images 8] [--out profiles/dpmpp2m_render.json]
Reports ms per render and ms per step (median over the repeats) and the spread of the Euler repeats.  One warm-up render per
variant first (GEMM tuning, graph capture)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seed-story_amd"))
import torch  # noqa: E402

from seedstory.diffusion import (DPMSolverMultistepScheduler, EulerDiscreteScheduler, StableDiffusionXLPipeline,  # noqa: E402
                                 UNet2DConditionModel)

VARIANTS = (("euler_30", "euler", 30), ("dpmpp2m_karras_20", "dpmpp", 20), ("dpmpp2m_karras_15", "dpmpp", 15))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dpmpp2m_render.json"))
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

    def render_ms(which, steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = pipes[which](num_inference_steps=steps, **kw).images
        e1.record()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out.float()).all())
        return e0.elapsed_time(e1)

    for name, which, steps in VARIANTS:
        print("warm-up %-18s %.1f ms" % (name, render_ms(which, steps)), flush=True)
    ms = {name: [] for name, _, _ in VARIANTS}
    for r in range(args.repeats):
        for name, which, steps in VARIANTS:
            ms[name].append(render_ms(which, steps))
            print("repeat %d %-18s %.1f ms" % (r, name, ms[name][-1]), flush=True)
    res = {"device": torch.cuda.get_device_name(0), "images_per_render": B, "unet_batch": 2 * B, "size": args.size, "dtype": "bf16",
           "repeats": args.repeats, "variants": {}}
    for name, _, steps in VARIANTS:
        med = statistics.median(ms[name])
        res["variants"][name] = {"steps": steps, "render_ms_median": round(med, 2), "ms_per_step": round(med / steps, 3),
                                 "render_ms_min": round(min(ms[name]), 2), "render_ms_max": round(max(ms[name]), 2),
                                 "render_ms": [round(v, 2) for v in ms[name]]}
    e = res["variants"]["euler_30"]
    e["spread_rel"] = round((e["render_ms_max"] - e["render_ms_min"]) / e["render_ms_median"], 4)
    for name in ("dpmpp2m_karras_20", "dpmpp2m_karras_15"):
        res["variants"][name]["render_vs_euler_30"] = round(res["variants"][name]["render_ms_median"] / e["render_ms_median"], 4)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

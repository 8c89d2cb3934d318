"""Cost record of the stochastic samplers (Euler ancestral, DPM++ 2M SDE): the synthetic SDXL-base UNet at 1024 x 1024, 8 images
per render (UNet batch 16), bf16, latent output, no VAE.
    python tools/sde_bench.py [--repeats 5] [--images 8] [--parent-tree DIR] [--out profiles/sde_render.json]
Three measurements, every variant alternating with the others inside one process, median over the repeats, spread reported:
  step     one launch of ss_multistep_step against one of ss_multistep_noise_step (s != 0) at n = images * 4 * 128 * 128,
           form (2, 2): us per launch over a train of launches between two events
  render   the render loop under Euler-30 (the reference), DPM++ 2M Karras-20, DPM++ 2M SDE Karras-20 and Euler-a-30
  default  tools/solver_bench.py of this tree and, with --parent-tree (a checkout of the parent commit with its library built), of
           the parent, one fresh process each, one after the other in the same session: the default render has not moved
One warm-up render per variant first (GEMM tuning, graph capture)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "seed-story_amd"))
import torch  # noqa: E402

from seedstory import ops  # noqa: E402
from seedstory.diffusion import (DPMSolverMultistepScheduler, DPMSolverMultistepSDEScheduler, EulerAncestralDiscreteScheduler,  # noqa: E402
                                 EulerDiscreteScheduler, StableDiffusionXLPipeline, UNet2DConditionModel)

VARIANTS = (("euler_30", "euler", 30), ("dpmpp2m_karras_20", "dpmpp", 20), ("dpmpp2m_sde_karras_20", "sde", 20), ("euler_a_30", "euler_a", 30))
STEP_TRAIN = 200


def summary(vals, digits=2):
    med = statistics.median(vals)
    return {"median": round(med, digits), "min": round(min(vals), digits), "max": round(max(vals), digits),
            "spread_rel": round((max(vals) - min(vals)) / med, 4), "all": [round(v, digits) for v in vals]}


def step_launch(B, size, repeats, dev, dt):
    """us per launch, trains of STEP_TRAIN launches, plain and noise alternating"""
    n_img = 4 * (size // 8) ** 2
    n = B * n_img
    g = torch.Generator(device=dev).manual_seed(1)
    state = torch.randn(2, n, device=dev, generator=g)
    eps = torch.randn(2, n, device=dev, generator=g).to(dt)
    xin = torch.empty(2, n, device=dev, dtype=dt)
    seeds = ops.noise_seeds(list(range(B)), dev)
    coef = (0.7, 0.25, -0.05)          # a + b + c < 1: the state stays bounded over a train

    def train(noise):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(STEP_TRAIN):
            if noise:
                ops.multistep_noise_step_(state, eps, 7.5, 1.0, *coef, 0.5, 0.9, seeds, i % 30, xin_next=xin)
            else:
                ops.multistep_step_(state, eps, 7.5, 1.0, *coef, 0.9, xin_next=xin)
        e1.record()
        torch.cuda.synchronize()
        state[0].normal_(generator=g)            # keep the state finite over the trains
        return e0.elapsed_time(e1) * 1000.0 / STEP_TRAIN
    train(False), train(True)
    us = {"plain": [], "noise": []}
    for _ in range(repeats):
        us["plain"].append(train(False))
        us["noise"].append(train(True))
    res = {"n": n, "n_img": n_img, "launches_per_train": STEP_TRAIN, "plain_us": summary(us["plain"]), "noise_us": summary(us["noise"])}
    res["noise_minus_plain_us"] = round(res["noise_us"]["median"] - res["plain_us"]["median"], 2)
    return res


def solver_bench(tree, repeats, images):
    """tools/solver_bench.py of ``tree`` in a fresh process -> its result, or the reason it did not run"""
    script = os.path.join(tree, "tools", "solver_bench.py")
    if not os.path.exists(script):
        return {"not_run": "no tools/solver_bench.py under %s" % tree}
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "solver.json")
        rc = subprocess.call([sys.executable, script, "--repeats", str(repeats), "--images", str(images), "--out", out], cwd=tree,
                             stdout=subprocess.DEVNULL)
        if rc != 0 or not os.path.exists(out):
            return {"not_run": "exit status %d" % rc}
        with open(out) as f:
            return json.load(f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sde_render.json"))
    args = ap.parse_args()
    dev, dt, B = "cuda:0", torch.bfloat16, args.images
    res = {"device": torch.cuda.get_device_name(0), "images_per_render": B, "unet_batch": 2 * B, "size": args.size, "dtype": "bf16",
           "repeats": args.repeats}
    res["step_launch"] = step_launch(B, args.size, args.repeats, dev, dt)
    print(json.dumps(res["step_launch"]), flush=True)

    unet = UNet2DConditionModel().to(dev, dt).init_synthetic(4)
    scheds = {"euler": EulerDiscreteScheduler(), "dpmpp": DPMSolverMultistepScheduler(use_karras_sigmas=True),
              "sde": DPMSolverMultistepSDEScheduler(use_karras_sigmas=True), "euler_a": EulerAncestralDiscreteScheduler()}
    pipes = {k: StableDiffusionXLPipeline(vae=None, unet=unet, scheduler=s) for k, s in scheds.items()}
    g = torch.Generator(device=dev).manual_seed(0)
    kw = dict(prompt_embeds=torch.randn(B, 64, 2048, device=dev, dtype=dt, generator=g),
              negative_prompt_embeds=torch.randn(B, 64, 2048, device=dev, dtype=dt, generator=g),
              pooled_prompt_embeds=torch.randn(B, 1280, device=dev, dtype=dt, generator=g),
              negative_pooled_prompt_embeds=torch.randn(B, 1280, device=dev, dtype=dt, generator=g),
              latents=torch.randn(B, 4, args.size // 8, args.size // 8, device=dev, dtype=dt, generator=g),
              guidance_scale=7.5, height=args.size, width=args.size, output_type="latent", noise_seed=list(range(100, 100 + B)))

    def render_ms(which, steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = pipes[which](num_inference_steps=steps, **kw).images
        e1.record()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out.float()).all())
        return e0.elapsed_time(e1)

    for name, which, steps in VARIANTS:
        print("warm-up %-22s %.1f ms" % (name, render_ms(which, steps)), flush=True)
    ms = {name: [] for name, _, _ in VARIANTS}
    for r in range(args.repeats):
        for name, which, steps in VARIANTS:
            ms[name].append(render_ms(which, steps))
            print("repeat %d %-22s %.1f ms" % (r, name, ms[name][-1]), flush=True)
    res["variants"] = {}
    for name, _, steps in VARIANTS:
        s = summary(ms[name])
        res["variants"][name] = {"steps": steps, "render_ms": s, "ms_per_step": round(s["median"] / steps, 3)}
    v = res["variants"]
    v["dpmpp2m_sde_karras_20"]["ms_per_step_vs_dpmpp2m_karras_20"] = round(v["dpmpp2m_sde_karras_20"]["ms_per_step"] / v["dpmpp2m_karras_20"]["ms_per_step"], 4)
    v["euler_a_30"]["ms_per_step_vs_dpmpp2m_karras_20"] = round(v["euler_a_30"]["ms_per_step"] / v["dpmpp2m_karras_20"]["ms_per_step"], 4)
    for name in ("dpmpp2m_karras_20", "dpmpp2m_sde_karras_20", "euler_a_30"):
        v[name]["render_vs_euler_30"] = round(v[name]["render_ms"]["median"] / v["euler_30"]["render_ms"]["median"], 4)
    del unet, pipes
    torch.cuda.empty_cache()
    res["default_render"] = {"this_tree": solver_bench(ROOT, args.repeats, B),
                             "parent": solver_bench(args.parent_tree, args.repeats, B) if args.parent_tree else {"not_run": "no --parent-tree"}}
    a, b = res["default_render"]["this_tree"], res["default_render"]["parent"]
    if "variants" in a and "variants" in b:
        res["default_render"]["euler_30_this_over_parent"] = round(a["variants"]["euler_30"]["render_ms_median"] /
                                                                   b["variants"]["euler_30"]["render_ms_median"], 4)
    print(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

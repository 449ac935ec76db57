#!/usr/bin/env python3
"""Image-guided denoise (`generate(image_guidance_scale=1.5)`), fast path vs per-step path, on ONE GPU, one process, A/B/A/B.

cfg4 shape: FLUX.1-dev-shaped transformer (57 blocks, synthetic weights), 1024^2 image + 512^2 "cot" condition held as moments
(`Condition(moments=[32, 64, 64])`: 1024 condition tokens, S = 5632), FLUX-Corrector-shaped LoRA r = 32 on the condition rows
(merged form, the search drivers' default), T = 50, s = 1.5.

  A = the per-step path: forced by a no-op `callback_on_step_end` -- per step two `tranformer_forward` calls, one
      `condition.encode(pipe, empty=True)`, three torch element-wise ops, `scheduler.step`.  This is the code every guided call
      ran before the guided fast path existed.
  B = the fast path: tables and unconditional tokens up front, ONE rf_flux_denoise_guided call (one hipGraph replay at T >= 16).

`--image-form` adds the same pair with the condition as a 512^2 image on the HIP VAE (FLUX.1-dev VAE shape, synthetic weights):
A re-encodes the image every step, B encodes it once.  Each timed latent ends in a device synchronise; the two paths alternate and
share the warm-up.  Prints one JSON object (per-latent seconds of every repetition, medians, A-to-A and B-to-B spread, bit-equality
of the two paths' latents)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from reflectionflow_amd.flux.condition import Condition  # noqa: E402
from reflectionflow_amd.flux.generate import generate  # noqa: E402
from reflectionflow_amd.flux.pipeline import synthetic_lora_state_dict  # noqa: E402
from reflectionflow_amd.tts.utils import get_noises  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3, help="timed latents per path (the paths alternate)")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--scale", type=float, default=1.5)
    ap.add_argument("--image-form", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev, bf = torch.device("cuda:0"), torch.bfloat16
    pipe = bench.build_model(dev, {}, seed=0)
    pipe.load_lora_weights({k: v.to(dev) for k, v in synthetic_lora_state_dict(pipe.transformer, r=32, seed=1).items()},
                           adapter_name="reflection")
    pipe.enable_merged_lora()
    g = torch.Generator().manual_seed(1)
    pe = torch.randn(1, 512, 4096, generator=g).to(dev).to(bf)
    pooled = torch.randn(1, 768, generator=g).to(dev).to(bf)
    moments = torch.cat([torch.randn(16, 64, 64, generator=g), torch.randn(16, 64, 64, generator=g) - 2.0]).to(dev).to(bf)
    mc = {"union_cond_attn": True, "add_cond_attn": False, "latent_lora": False}
    noises = get_noises(2 ** 31 - 1, 1, 1024, 1024, device=dev, dtype=bf, seeds=[1])

    class VaeConfigOnly:                       # moments= conditions read the shift / scale constants off pipe.vae
        class config:
            shift_factor, scaling_factor = 0.1159, 0.3611

    def noop(p, i, t, kw):
        return {}

    def one(make_cond, per_step):
        kw = dict(callback_on_step_end=noop) if per_step else {}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = generate(pipe, conditions=[make_cond()], model_config=mc, default_lora=True, height=1024, width=1024,
                       num_inference_steps=args.steps, guidance_scale=3.5, latents=noises[1], prompt_embeds=pe,
                       pooled_prompt_embeds=pooled, output_type="latent", image_guidance_scale=args.scale, **kw).images
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    def ab(make_cond):
        _, ref_a = one(make_cond, True)        # warm-up of both paths (the fast path's first call also captures its graph)
        _, ref_b = one(make_cond, False)
        one(make_cond, False)
        ta, tb = [], []
        for _ in range(args.reps):
            ta.append(one(make_cond, True)[0])
            tb.append(one(make_cond, False)[0])
        ma, mb = statistics.median(ta), statistics.median(tb)
        return dict(per_step_s=[round(x, 4) for x in ta], fast_s=[round(x, 4) for x in tb], per_step_median_s=round(ma, 4),
                    fast_median_s=round(mb, 4), per_step_spread_s=round(max(ta) - min(ta), 4), fast_spread_s=round(max(tb) - min(tb), 4),
                    gain_s=round(ma - mb, 4), gain_pct=round(100 * (ma - mb) / ma, 2), latents_bit_equal=bool(torch.equal(ref_a, ref_b)))

    res = dict(workload=f"cfg4 shape, image_guidance_scale={args.scale}, T={args.steps}, merged LoRA r=32, 57 blocks, S=5632",
               device=torch.cuda.get_device_name(0), reps=args.reps)
    pipe.vae = VaeConfigOnly()

    def moments_cond():
        return Condition("cot", moments=moments, position_delta=[0, -32]).with_generator(torch.Generator().manual_seed(7))
    res["moments_form"] = ab(moments_cond)
    if args.image_form:
        from PIL import Image
        from reflectionflow_amd.flux import vae as V
        from reflectionflow_amd.flux.vae_hip import HipVAE
        pipe.vae = HipVAE(V.init_synthetic_vae_(V.AutoencoderKL(), seed=5).eval().to(dev).to(bf))
        pipe.image_processor = V.VaeImageProcessor(vae_scale_factor=16)
        px = torch.randint(0, 256, (512, 512, 3), generator=torch.Generator().manual_seed(2), dtype=torch.uint8).numpy()
        img = Image.fromarray(px)

        def image_cond():
            return Condition("cot", condition=img, position_delta=[0, -32]).with_generator(torch.Generator().manual_seed(7))
        res["image_form_hip_vae"] = ab(image_cond)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        open(args.out, "w").write(line + "\n")


if __name__ == "__main__":
    main()

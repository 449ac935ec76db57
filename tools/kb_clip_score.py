"""Times the CLIP-score verifier's stages at 1024^2 (device events, one warm-up pass): FLUX VAE decode (synthetic FLUX-shaped HIP
VAE), preprocess (rf_clip_preprocess, in place on the decoder's output), vision tower (rf_clip_vision_encode, synthetic weights of
--geometry: ViT-L/14, ViT-H/14 = head dim 80 + erf GELU, or ViT-L/14 at 336 px = 577 tokens on the streaming-keys attention), score (rf_clip_score) and the text tower of one prompt, for n = 1, 8, 32
candidates.  --reps timed passes after the warm-up: the figures are medians, `vision_ms_spread` is max - min.  One further pass
under ops.profile gives the towers' split by kernel class (`tower_us`: GEMM / attention / row kernels).  One JSON line per n.

    python tools/kb_clip_score.py [--n 1 8 32] [--size 1024] [--geometry vit_l14|vit_h14|vit_l14_336] [--reps 1]
"""
import argparse
import json
import os
import sys

import statistics

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--geometry", choices=["vit_l14", "vit_h14", "vit_l14_336"], default="vit_l14")
    ap.add_argument("--reps", type=int, default=1)
    args = ap.parse_args()
    from reflectionflow_amd import ops
    from reflectionflow_amd.flux import vae as V
    from reflectionflow_amd.flux.text_hip import HipClipTextEncoder, HipClipVisionEncoder, clip_score
    from reflectionflow_amd.flux.vae_hip import HipVAE
    from reflectionflow_amd.tts import clip_verifier as CV
    dev = torch.device("cuda:0")
    bf = torch.bfloat16
    vae = HipVAE(V.init_synthetic_vae_(V.AutoencoderKL(), seed=1).to(dev, bf).eval())
    cfg = CV.geometry(args.geometry)[0]
    t, v, act = cfg["text"], cfg["vision"], cfg.get("act", "quick_gelu")
    sd = CV.synthetic_clip_state(cfg, 0)
    enc = HipClipVisionEncoder({k: x for k, x in sd.items() if k.startswith("vision_model.") or k == "visual_projection.weight"}, v["heads"], dev,
                               head_dim=v["hidden"] // v["heads"], act=act, image_size=v["image_size"])
    tenc = HipClipTextEncoder({k: x for k, x in sd.items() if k.startswith("text_model.")}, t["heads"], dev, head_dim=t["hidden"] // t["heads"], act=act)
    ids = CV.synthetic_tokenize(t["vocab"])(["a red cube left of a blue ball"]).to(dev)
    txt = torch.randn(cfg["projection_dim"], device=dev).to(bf)
    # 2 FLOPs per multiply-add: per token 4 D^2 (q, k, v, out) + 2 D F (mlp) + 2 S D (QK^T, PV), + the patch and projection GEMMs
    D, F, S = v["hidden"], v["inter"], enc.tokens
    flops = 2.0 * (v["layers"] * S * (4 * D * D + 2 * D * F + 2 * S * D) + (enc.tokens - 1) * enc.k_pad * D + D * cfg["projection_dim"])
    h = args.size // 8
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    for n in args.n:
        z = torch.randn(n, 16, h, h, device=dev).to(bf)
        patches = enc.alloc_patches(n)
        runs = []
        for rep in range(1 + args.reps):                                # rep 0: warm-up (workspaces, code objects)
            e = [ev() for _ in range(6)]
            e[0].record()
            outs = [vae.decode_halo(z[i:i + 1])[0] for i in range(n)]
            e[1].record()
            for i, o in enumerate(outs):
                Hp, Wp, c = o.shape
                enc.preprocess(o[1:, 1:], (0, Wp * c, c, 1), 0.5, 0.5, patches[i:i + 1], Hp - 2, Wp - 2)
            e[2].record()
            emb = enc.encode(patches)
            e[3].record()
            sc = clip_score(emb, txt, 4.6)
            e[4].record()
            tenc.encode(ids)
            e[5].record()
            torch.cuda.synchronize()
            if rep:
                runs.append([e[i].elapsed_time(e[i + 1]) for i in range(5)])
            del outs
        ms = [statistics.median(r[i] for r in runs) for i in range(5)]
        with ops.profile(8192) as pr:
            enc.encode(patches)
            tenc.encode(ids)
            torch.cuda.synchronize()
        res = dict(geometry=args.geometry, n=n, size=args.size, reps=args.reps, vae_decode_ms=ms[0], preprocess_ms=ms[1], vision_ms=ms[2],
                   vision_ms_spread=max(r[2] for r in runs) - min(r[2] for r in runs), score_ms=ms[3], text_ms=ms[4],
                   vision_ms_per_image=ms[2] / n, verifier_ms_per_image=sum(ms[:4]) / n,
                   vision_tflops=flops * n / (ms[2] * 1e-3) / 1e12, finite=bool(torch.isfinite(sc).all()),
                   tower_us={k: round(c["us"], 1) for k, c in pr.classes.items()})
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

"""Times the CLIP-score verifier's stages at 1024^2 (device events, one warm-up pass): FLUX VAE decode (synthetic FLUX-shaped HIP
VAE), preprocess (rf_clip_preprocess, in place on the decoder's output), ViT-L/14 vision tower (rf_clip_vision_encode, synthetic
weights) and score (rf_clip_score), for n = 1, 8, 32 candidates.  Prints one JSON line per n.

    python tools/kb_clip_score.py [--n 1 8 32] [--size 1024]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, nargs="+", default=[1, 8, 32])
    ap.add_argument("--size", type=int, default=1024)
    args = ap.parse_args()
    from reflectionflow_amd.flux import vae as V
    from reflectionflow_amd.flux.text_hip import HipClipVisionEncoder, clip_score
    from reflectionflow_amd.flux.vae_hip import HipVAE
    from reflectionflow_amd.tts import clip_verifier as CV
    dev = torch.device("cuda:0")
    bf = torch.bfloat16
    vae = HipVAE(V.init_synthetic_vae_(V.AutoencoderKL(), seed=1).to(dev, bf).eval())
    sd = CV.synthetic_clip_state(CV.VIT_L14, 0)
    enc = HipClipVisionEncoder({k: v for k, v in sd.items() if k.startswith("vision_model.") or k == "visual_projection.weight"}, 16, dev)
    txt = torch.randn(768, device=dev).to(bf)
    h = args.size // 8
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    for n in args.n:
        z = torch.randn(n, 16, h, h, device=dev).to(bf)
        patches = enc.alloc_patches(n)
        res = None
        for rep in range(2):                                            # rep 0: warm-up (workspaces, code objects)
            e = [ev() for _ in range(5)]
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
            torch.cuda.synchronize()
            ms = [e[i].elapsed_time(e[i + 1]) for i in range(4)]
            res = dict(n=n, size=args.size, vae_decode_ms=ms[0], preprocess_ms=ms[1], vision_ms=ms[2], score_ms=ms[3],
                       vision_ms_per_image=ms[2] / n, verifier_ms_per_image=sum(ms) / n,
                       vision_tflops=162e9 * n / (ms[2] * 1e-3) / 1e12, finite=bool(torch.isfinite(sc).all()))
            del outs
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()

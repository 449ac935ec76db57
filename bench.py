#!/usr/bin/env python3
"""bench.py -- BASELINE.json's metric on its cfg2 workload.

    metric : 1024^2 latents/sec (50-step FLUX denoise) per node
    step   : ONE complete 50-step denoise of one 1024x1024 candidate (output_type="latent") through
             the reference-shaped `generate()` API: modulation tables for the 50 timesteps, then
             50 x (57-block transformer forward + Euler step) on the GPU.  Nothing is skipped or cached
             across steps/candidates inside the timed region.
    inputs : synthetic -- random-init FLUX.1-dev-shaped weights (N(0,0.02^2), seed 0), random
             T5/CLIP embeddings, seeded initial noise via the tts/utils.py protocol.  Inputs are resident in
             HBM when the timed region starts.
    N GPUs : one process per GPU, candidates sharded rank-round-robin, weights replicated; the only collective
             is the round-boundary all-gather of verifier scores (RCCL).  `python bench.py --gpus N` launches its
             own N ranks (re-exec under torch.distributed.run on 127.0.0.1) when it is not already running under
             one; rank 0 prints the line.  Candidate c of the round (c = j * N + rank) is seeded by c alone, so
             `selected_candidate` does not depend on N.
             Rehearsal on a 1-GPU box: `--gpus 2 --ranks-share-gpu --dist-backend gloo` runs both ranks on cuda:0
             (2 x 38 GB of 288 GB) with the collectives over gloo -- the same launch, model build, barriers, score
             exchange and rank-0 line as the 8-GPU run, at ~0.5x per-rank throughput (NOT a scaling number).

A plain run sets up, warms up, times the --steps latents and prints ONE JSON line on rank 0 (see the driver contract);
`--dump-outputs DIR` then also writes what the timed path returned in its last step (DIR/latents.npy, float32) and the round's
verifier scores (DIR/scores.npy, DIR/labels.npy), after the timed region.  Everything else the bench measures or checks runs only
with `--full`: the timed latent's parity against the per-step path, power / clock telemetry, and the extra objects
    roofline     -- the dominant kernel class (the 256x256-tile bf16 MFMA GEMM; persistent whole-tile launches of the ping-pong loop): algorithmic FLOPs of its launches /
                    their summed durations, both taken INSIDE the real forward sequence: right after the timed
                    region one more candidate is denoised for a few steps with the library's in-sequence timing hook
                    on (a hipEvent pair around every kernel launch on its launch stream, rf_profile_begin/_end), so
                    sum-of-kernel-time <= forward time holds on the same box (reported under `consistency`).
                    `isolated_shapes` keeps the round-1 style table (each launch shape re-launched back to back).
    cpu_baseline -- the CPU oracle (a port of the reference path) on the host's physical cores over a bounded sample:
                    cfg1 (256^2, 4 steps, fp32) end to end, and one warmed DoubleStream + SingleStream block at
                    the cfg2 sequence length extrapolated to the metric's unit (labelled as extrapolated).
    attention, vae, text_encoders, training -- the attention kernels' isolated cost, the VAE and text-encoder timings and one
                    LoRA training step (each reported separately from the metric).
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

PEAK_BF16_TFLOPS = 2500.0          # MI355X dense bf16 MFMA (MI355X_MICROARCH.md:42)
PROFILE_STEPS = 4                  # forwards in the profiled (event-instrumented) pass after the timed region


def flops_per_forward(S_txt, S_img, D=3072, mlp=12288, nd=19, ns=38, in_ch=64, joint=4096, S_cond=0):
    """2MNK per GEMM, 4 S^2 D per attention block; element-wise excluded."""
    S = S_txt + S_img + S_cond
    gemm = nd * S * (2 * D * 3 * D + 2 * D * D + 2 * 2 * D * mlp) + ns * S * (2 * D * (3 * D + mlp) + 2 * (D + mlp) * D)
    attn = (nd + ns) * 4 * S * S * D
    emb = 2 * (S_img + S_cond) * in_ch * D * 2 + 2 * S_txt * joint * D
    return gemm + attn + emb, gemm, attn


def build_model(dev, cfg=None, seed=0):
    """Random-init FLUX.1-dev-shaped transformer created directly in HBM (no checkpoint offline)."""
    from reflectionflow_amd.flux import modules as M
    from reflectionflow_amd.flux.pipeline import FluxPipeline
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with torch.device(dev):
            tr = M.FluxTransformer2DModel(**(cfg or {}))
    finally:
        torch.set_default_dtype(old)
    g = torch.Generator(device=dev).manual_seed(seed)
    with torch.no_grad():
        for name, p in tr.named_parameters():
            if name.endswith("weight") and p.ndim == 1:
                p.copy_(1.0 + 0.02 * torch.randn(p.shape, generator=g, device=dev, dtype=torch.float32))
            else:
                p.copy_(0.02 * torch.randn(p.shape, generator=g, device=dev, dtype=torch.float32))
    return FluxPipeline(tr)


# ------------------------------------------------------------------------------------------------------
# roofline
# ------------------------------------------------------------------------------------------------------
def isolated_shapes(dev, S_txt, S_img, D, mlp, heads, nd, ns):
    """Secondary table: every distinct launch shape of the dominant kernel re-launched back to back (warm
    operands, no neighbours), timed with hipEvents on the launch stream (rf_time_gemm)."""
    from reflectionflow_amd import ops
    from reflectionflow_amd.ops import RF_EPI_GATE_RES, RF_EPI_GELU, RF_EPI_QKV, RF_EPI_QKV_GELU, Group, Seg
    bf = torch.bfloat16
    S = S_txt + S_img
    r = lambda *s, sc=1.0: (torch.randn(*s, device=dev) * sc).to(bf)  # noqa: E731
    xn, att, hid = r(S, D), r(S, D), r(S, mlp)
    x = r(S, D)
    q, k, vt, s_pad = ops.alloc_attn_operands(heads, S, dev)
    gate, b3, b1, bm, bf_ = r(D), r(3 * D), r(D), r(mlp), r(3 * D + mlp)
    Wq, Wq2 = r(3 * D, D, sc=.02), r(3 * D, D, sc=.02)
    Wo, Wo2 = r(D, D, sc=.02), r(D, D, sc=.02)
    W1, W1b = r(mlp, D, sc=.02), r(mlp, D, sc=.02)
    W2, W2b = r(D, mlp, sc=.02), r(D, mlp, sc=.02)
    Wf, Ws = r(3 * D + mlp, D, sc=.02), r(D, D + mlp, sc=.02)
    t, i = slice(0, S_txt), slice(S_txt, S)
    nw = [r(128) for _ in range(4)]
    rope = (torch.rand(S, 128, device=dev), torch.rand(S, 128, device=dev))
    shapes = []

    def two(A, Wt, Wi, **kw):
        return [Group([Seg(A[t], Wt)], **{k_: (v[0] if isinstance(v, tuple) else v) for k_, v in kw.items()}),
                Group([Seg(A[i], Wi)], **{k_: (v[1] if isinstance(v, tuple) else v) for k_, v in kw.items()})]

    shapes.append(("dbl_qkv", nd, 2.0 * S * 3 * D * D,
                   lambda: ops.time_gemm(two(xn, Wq2, Wq, bias=b3, tok_offset=(0, S_txt), norm_q=(nw[2], nw[0]),
                                             norm_k=(nw[3], nw[1])), 3 * D, RF_EPI_QKV,
                                         q=q, k=k, vt=vt, heads=heads, s_pad=s_pad, rope=rope)))
    shapes.append(("dbl_out", nd, 2.0 * S * D * D,
                   lambda: ops.time_gemm(two(att, Wo2, Wo, bias=b1, gate=gate, out=(x[t], x[i]), residual=(x[t], x[i])),
                                         D, RF_EPI_GATE_RES)))
    shapes.append(("dbl_ff1", nd, 2.0 * S * mlp * D,
                   lambda: ops.time_gemm(two(xn, W1b, W1, bias=bm, out=(hid[t], hid[i])), mlp, RF_EPI_GELU)))
    shapes.append(("dbl_ff2", nd, 2.0 * S * D * mlp,
                   lambda: ops.time_gemm(two(hid, W2b, W2, bias=b1, gate=gate, out=(x[t], x[i]), residual=(x[t], x[i])),
                                         D, RF_EPI_GATE_RES)))
    shapes.append(("sgl_in", ns, 2.0 * S * (3 * D + mlp) * D,
                   lambda: ops.time_gemm([Group([Seg(xn, Wf)], bias=bf_, out=hid, tok_offset=0, norm_q=nw[0],
                                                norm_k=nw[1])], 3 * D + mlp, RF_EPI_QKV_GELU, n_split=3 * D, q=q, k=k,
                                         vt=vt, heads=heads, s_pad=s_pad, rope=rope)))
    shapes.append(("sgl_out", ns, 2.0 * S * D * (D + mlp),
                   lambda: ops.time_gemm([Group([Seg(att, Ws[:, :D]), Seg(hid, Ws[:, D:])], bias=b1, gate=gate, out=x,
                                                residual=x)], D, RF_EPI_GATE_RES)))
    per = {}
    for name, count, fl, fn in shapes:
        sec = fn()
        torch.cuda.synchronize()
        per[name] = {"launches_per_forward": count, "us": round(sec * 1e6, 1), "tflops": round(fl / sec / 1e12, 1)}
        mhz, loop_us = clock_probe(0)
        if mhz and loop_us <= sec * 1e6:     # (stream-K launches do not carry the probe: a stale value would be longer)
            per[name]["shader_mhz"] = round(mhz)
            per[name]["frac_at_clock"] = round(fl / sec / 1e12 / (PEAK_BF16_TFLOPS * mhz / NOMINAL_MHZ), 3)
    return per


NOMINAL_MHZ = 2400.0   # the clock the 2.5 PFLOP/s dense bf16 peak is quoted at


def vae_table(dev, res):
    """the metric's latent excludes the VAE ("reported separately").  Decode of one res x res candidate and encode of a
    512 x 512 condition image through the HIP path (rf_vae_decode / rf_vae_encode, FLUX.1-dev VAE shape, random-init weights)."""
    from reflectionflow_amd.flux.vae import AutoencoderKL, init_synthetic_vae_
    from reflectionflow_amd.flux.vae_hip import HipVAE
    hv = HipVAE(init_synthetic_vae_(AutoencoderKL(), seed=0).to(dev).to(torch.bfloat16).eval())
    out = {"path": "HIP (librf_flux.so rf_vae_decode / rf_vae_encode): convolutions = 3-K-segment launches of the bf16 MFMA GEMM"}
    for name, shape, fn in ((f"decode_{res}_ms", (1, 16, res // 8, res // 8), lambda t: hv.decode(t).sample),
                            ("encode_512_ms", (1, 3, 512, 512), lambda t: hv.encode_moments(t))):
        x = torch.randn(*shape, device=dev).to(torch.bfloat16)
        with torch.no_grad():
            fn(x); fn(x)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                fn(x)
            torch.cuda.synchronize()
        out[name] = round((time.perf_counter() - t0) / 10 * 1e3, 2)
    out["decode_frac_of_a_candidate"] = round(out[f"decode_{res}_ms"] / 1e3 / 3.1, 4)
    del hv
    torch.cuda.empty_cache()
    return out


def synthetic_t5_xxl_state(dev, layers=24, d_model=4096, heads=64, d_ff=10240, vocab=32128, seed=0):
    """T5-v1.1-XXL-shaped encoder weights (4.7 B parameters), drawn on the device in bf16 (transformers key names)."""
    g = torch.Generator(device=dev).manual_seed(seed)
    bf = torch.bfloat16
    r = lambda *shape, sc=1.0: (torch.randn(*shape, generator=g, device=dev, dtype=torch.float32) * sc).to(bf)  # noqa: E731
    inner = 64 * heads
    sd = {"shared.weight": r(vocab, d_model), "encoder.final_layer_norm.weight": torch.ones(d_model, device=dev, dtype=bf),
          "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight": r(32, heads)}
    s = d_model ** -0.5
    for i in range(layers):
        p = f"encoder.block.{i}.layer."
        for x in "qk":
            sd[p + f"0.SelfAttention.{x}.weight"] = r(inner, d_model, sc=s * 0.7)
        sd[p + "0.SelfAttention.v.weight"] = r(inner, d_model, sc=s)
        sd[p + "0.SelfAttention.o.weight"] = r(d_model, inner, sc=inner ** -0.5)
        sd[p + "0.layer_norm.weight"] = torch.ones(d_model, device=dev, dtype=bf)
        sd[p + "1.DenseReluDense.wi_0.weight"] = r(d_ff, d_model, sc=s)
        sd[p + "1.DenseReluDense.wi_1.weight"] = r(d_ff, d_model, sc=s)
        sd[p + "1.DenseReluDense.wo.weight"] = r(d_model, d_ff, sc=d_ff ** -0.5)
        sd[p + "1.layer_norm.weight"] = torch.ones(d_model, device=dev, dtype=bf)
    return sd


def text_table(dev):
    """the two encoder calls FluxPipeline.encode_prompt makes per prompt (per candidate and round in the reflection
    loop), on the HIP path: T5-v1.1-XXL shape at 512 tokens (24 layers, 4.7 B parameters) and CLIP-L shape at 77 tokens, random-init."""
    from reflectionflow_amd.flux.text_hip import HipClipTextEncoder, HipT5Encoder
    bf = torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(1)
    r = lambda *shape, sc=1.0: (torch.randn(*shape, generator=g, device=dev, dtype=torch.float32) * sc).to(bf)  # noqa: E731
    t5 = HipT5Encoder(synthetic_t5_xxl_state(dev), 64, dev)
    D, F, V = 768, 3072, 49408
    csd = {"embeddings.token_embedding.weight": r(V, D, sc=0.02), "embeddings.position_embedding.weight": r(77, D, sc=0.01),
           "final_layer_norm.weight": torch.ones(D, device=dev, dtype=bf), "final_layer_norm.bias": torch.zeros(D, device=dev, dtype=bf)}
    for i in range(12):
        p = f"encoder.layers.{i}."
        for x in ("q_proj", "k_proj", "v_proj", "out_proj"):
            csd[p + f"self_attn.{x}.weight"], csd[p + f"self_attn.{x}.bias"] = r(D, D, sc=D ** -0.5), r(D, sc=0.02)
        for n in ("layer_norm1", "layer_norm2"):
            csd[p + n + ".weight"], csd[p + n + ".bias"] = torch.ones(D, device=dev, dtype=bf), torch.zeros(D, device=dev, dtype=bf)
        csd[p + "mlp.fc1.weight"], csd[p + "mlp.fc1.bias"] = r(F, D, sc=D ** -0.5), r(F, sc=0.02)
        csd[p + "mlp.fc2.weight"], csd[p + "mlp.fc2.bias"] = r(D, F, sc=F ** -0.5), r(D, sc=0.02)
    clip = HipClipTextEncoder(csd, 12, dev)
    t5_ids = torch.randint(0, 32128, (1, 512), device=dev)
    clip_ids = torch.randint(0, 49406, (1, 77), device=dev)
    clip_ids[0, 20:] = 49407
    out = {"path": "HIP (librf_flux.so rf_t5_encode / rf_clip_text_encode): projections = launches of the bf16 MFMA GEMM, attention = one kernel "
                   "with K and V^T of a head resident in LDS"}
    t5_ids4, clip_ids4 = t5_ids.repeat(4, 1), clip_ids.repeat(4, 1)
    for name, fn in (("t5_xxl_512_tokens_ms", lambda: t5.encode(t5_ids)), ("clip_l_77_tokens_ms", lambda: clip.encode(clip_ids)),
                     ("t5_xxl_4_prompts_ms", lambda: t5.encode(t5_ids4)), ("clip_l_4_prompts_ms", lambda: clip.encode(clip_ids4))):
        fn(); fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            fn()
        torch.cuda.synchronize()
        out[name] = round((time.perf_counter() - t0) / 10 * 1e3, 2)
    out["t5_weight_bytes_gb"] = 9.4
    out["t5_tflops"] = round(2 * 512 * (24 * (4 * 4096 * 4096 + 3 * 4096 * 10240)) / (out["t5_xxl_512_tokens_ms"] * 1e-3) / 1e12, 1)
    # both rooflines of the B = 1 encode: the weights are streamed once per prompt
    out["t5_weight_stream_GBps"] = round(9.4e9 / (out["t5_xxl_512_tokens_ms"] * 1e-3) / 1e9, 1)
    out["t5_frac_of_hbm_8TBps"] = round(out["t5_weight_stream_GBps"] / 8000.0, 3)
    out["t5_frac_of_bf16_mfma_peak"] = round(out["t5_tflops"] / PEAK_BF16_TFLOPS, 3)
    out["per_prompt_ms_in_a_batch_of_4"] = round((out["t5_xxl_4_prompts_ms"] + out["clip_l_4_prompts_ms"]) / 4, 2)
    out["frac_of_a_candidate"] = round((out["t5_xxl_512_tokens_ms"] + out["clip_l_77_tokens_ms"]) / 1e3 / 3.1, 4)
    del t5, clip, csd
    torch.cuda.empty_cache()
    return out


def attention_table(dev, pipe, S, heads):
    """Which attention kernel the timed run used and what the alternatives cost (VERDICT r2 / ADVICE r2: the headline must
    carry its floor).  The engine hands the bounded-score kernel the bound it derives from the checkpoint's norm_q / norm_k
    weights (here synthetic, ~1); a checkpoint whose bound exceeds 100 takes the LAGGED-MAX kernel instead (exact for any
    weights) -- `isolated_us` prices that kernel, the bounded one and the online-softmax kernel on the same operands."""
    from reflectionflow_amd import _lib as L, ops
    bounds = []
    try:
        for blk in list(pipe.transformer.transformer_blocks) + list(pipe.transformer.single_transformer_blocks):
            a = blk.attn
            wq = [a.norm_q.weight] + ([a.norm_added_q.weight] if getattr(a, "norm_added_q", None) is not None else [])
            wk = [a.norm_k.weight] + ([a.norm_added_k.weight] if getattr(a, "norm_added_k", None) is not None else [])
            bounds.append(ops.qk_score_bound(tuple(wq), tuple(wk)))
    except Exception:           # noqa: BLE001 -- reporting only
        pass
    g = torch.Generator(device=dev).manual_seed(3)
    q, k, vt, s_pad = ops.alloc_attn_operands(heads, S, dev)
    q[:, :S] = (torch.randn(heads, S, 128, generator=g, device=dev) * ops.QK_PRESCALE).to(torch.bfloat16)
    k[:, :S] = torch.randn(heads, S, 128, generator=g, device=dev).to(torch.bfloat16)
    vt.copy_(torch.randn(vt.shape, generator=g, device=dev).to(torch.bfloat16))
    out = torch.empty(S, heads * 128, dtype=torch.bfloat16, device=dev)
    flops = 4.0 * S * S * 128 * heads
    tab = {}
    # "auto_*" = what the library picks on its own with / without a proven bound (the timed run's launch; at S = 4608 x 24 heads
    # the mixed-size grid of 256- and 192-query workgroups); the explicit rows are the plain one-size grids
    kernels = [("auto_with_bound", L.RF_ATTN_AUTO, 25.0), ("auto_without_bound", L.RF_ATTN_AUTO, 0.0),
               ("bounded_16x16x32", L.RF_ATTN_BOUNDED16, 25.0), ("lagged_max_16x16x32", L.RF_ATTN_LAGGED16, 0.0),
               ("online_softmax_256", L.RF_ATTN_ONLINE256, 0.0)]
    if S % 256 != 0:
        kernels = kernels[4:]
    paths = {1: "online_softmax_128", 2: "online_softmax_256", 4: "bounded_32x32x16", 5: "bounded_16x16x32", 6: "bounded_16x16x32 split launch",
             8: "lagged_max_16x16x32", 9: "lagged_max_16x16x32 split launch", 10: "bounded_16x16x32 mixed-size grid",
             11: "lagged_max_16x16x32 mixed-size grid"}
    for name, kern, bound in kernels:
        for _ in range(3):
            ops.attention(q, k, vt, S, out=out, q_prescaled=True, score_bound=bound, kernel=kern)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            ops.attention(q, k, vt, S, out=out, q_prescaled=True, score_bound=bound, kernel=kern)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / 20
        tab[name] = {"us": round(us, 1), "tflops": round(flops / us / 1e6, 1)}
        if kern == L.RF_ATTN_AUTO:
            tab[name]["launch"] = paths.get(L.load().rf_debug_last_attn_path(), "?")
    res = {"qk_bound_max_over_blocks": round(max(bounds), 2) if bounds else None,
           "bounded_kernel_precondition": "qk_bound <= 100, i.e. max|norm_q.weight| * max|norm_k.weight| <= ~6.0",
           "kernel_of_the_timed_run": "bounded-score (qk_bound <= 100)" if bounds and max(bounds) <= 100 else "lagged-max",
           "fallback_when_bound_exceeds_100": "lagged_max_16x16x32 (exact for any q, k; no online softmax)",
           "isolated_us": tab}
    if "auto_with_bound" in tab and "auto_without_bound" in tab:
        res["fallback_cost_frac_on_attention"] = round(tab["auto_without_bound"]["us"] / tab["auto_with_bound"]["us"] - 1.0, 4)
    return res


def clock_probe(which):
    """(shader MHz, main-loop us) of block 0 of the last 256x256 ping-pong GEMM (0) / bounded-score attention (1)
    launch: s_memtime over s_memrealtime, stored by the kernel itself (csrc/common.hpp ClkProbe)."""
    import ctypes as C
    from reflectionflow_amd import _lib
    mhz, us = C.c_double(0.0), C.c_double(0.0)
    if _lib.load().rf_debug_clock_probe(which, C.byref(mhz), C.byref(us)) != 0 or not (500.0 < mhz.value < 3000.0):
        return None, None
    return mhz.value, us.value


def pmc_traffic(S_txt, S_img, D, mlp):
    """Fabric bytes per launch cannot be measured from inside this process: they come from the committed rocprofv3 --pmc passes over the
    same launches (tools/pmc_collect.sh -> profiles/rNN_pmc_kernels.json, FETCH_SIZE doubled per the gfx950 correction),
    forward-weighted like `achieved`.  Newest round wins.  The file carries the git sha it was measured at and a hash of the kernel
    source: when csrc/gemm_bf16.hip has changed since, the number is REFUSED (traffic = None, `stale` says why) instead of being
    reported for a kernel it was not measured on.
    What the counter is: L2 <-> fabric requests INCLUDING Infinity-Cache hits (MI355X_MICROARCH.md, 'HBM'), i.e. L2-fill traffic -- an
    upper bound on HBM bytes, not HBM bytes; a launch's operands (<= 235 MB) fit the 256 MiB Infinity Cache."""
    if (S_txt, S_img, D, mlp) != (512, 4096, 3072, 12288):
        return None, None, None
    import hashlib
    cur = hashlib.sha256(open(os.path.join(ROOT, "reflectionflow_amd", "csrc", "gemm_bf16.hip"), "rb").read()).hexdigest()[:16]
    for rnd in ("r06", "r05", "r04", "r03", "r02", "r01"):
        pmc = os.path.join(ROOT, "profiles", f"{rnd}_pmc_kernels.json")
        if os.path.exists(pmc):
            pj = json.load(open(pmc))["_summary"]
            at = pj.get("measured_at") or {}
            stamp = {"file": f"profiles/{rnd}_pmc_kernels.json", "git_sha": at.get("git_sha"),
                     "kernel_source_unchanged_since": at.get("gemm_bf16_hip_sha256_16") == cur}
            if not stamp["kernel_source_unchanged_since"]:
                stamp["stale"] = ("csrc/gemm_bf16.hip differs from the source these passes measured (or the file carries no stamp): "
                                  "re-run tools/pmc_collect.sh")
                return None, None, stamp
            src = (f"profiles/{rnd}_pmc_kernels.json (rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE = L2 <-> fabric bytes incl. Infinity-Cache hits; "
                   f"algorithmic {round(pj['gemm_algorithmic_bytes_per_launch_avg'])} B/launch; MFMA busy "
                   f"{pj['gemm_mfma_busy_pct_weighted']:.1f} % of SIMD-cycles at the sustained clock)")
            return round(pj["gemm_traffic_bytes_per_launch_avg"]), src, stamp
    return None, None, None


def in_sequence_roofline(one_latent_steps, T_prof, ms_per_forward_timed, dims):
    """Denoise one more candidate for T_prof steps with the in-sequence timing hook on."""
    from reflectionflow_amd import ops
    torch.cuda.synchronize()
    one_latent_steps(T_prof)                                 # warm this T (allocations, modulation table shapes)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with ops.profile(max_launches=600 * T_prof) as pr:
        one_latent_steps(T_prof)
        torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    in_sequence_roofline.window = (t0, t0 + wall)
    clk_gemm, clk_attn = clock_probe(0)[0], clock_probe(1)[0]    # last launch of each kind inside the real forward
    cl = pr.classes
    gm = cl.get("gemm_main", {"launches": 0, "us": 0.0, "work": 0.0})
    if gm["launches"] == 0 or pr.dropped:
        return {"bound": "mfma", "error": f"profile incomplete (dropped {pr.dropped})"}
    ach = gm["work"] / (gm["us"] * 1e-6) / 1e12
    per_fwd = {k: {"launches_per_forward": v["launches"] / T_prof, "ms_per_forward": round(v["us"] / T_prof / 1e3, 3)}
               for k, v in cl.items()}
    if "attention" in cl:
        a = cl["attention"]
        per_fwd["attention"]["tflops"] = round(a["work"] / (a["us"] * 1e-6) / 1e12, 1)
        per_fwd["attention"]["avg_launch_us"] = round(a["us"] / a["launches"], 1)
    if "rowop" in cl:
        per_fwd["rowop"]["GBps"] = round(cl["rowop"]["work"] / (cl["rowop"]["us"] * 1e-6) / 1e9, 1)
    per_fwd["gemm_main"]["tflops"] = round(ach, 1)
    sum_ms = sum(v["us"] for v in cl.values()) / T_prof / 1e3
    traffic, traffic_src, traffic_stamp = pmc_traffic(*dims)
    sustained = None
    if clk_gemm:
        # MI355X throttles under dense MFMA + LDS + L2 traffic: `frac` is against the 2.4 GHz peak as the contract
        # asks; this block says what the matrix pipes could have delivered at the clock the kernel was given
        sustained = {"gemm_shader_mhz": round(clk_gemm), "attention_shader_mhz": round(clk_attn) if clk_attn else None,
                     "nominal_mhz": NOMINAL_MHZ, "peak_at_gemm_clock": round(PEAK_BF16_TFLOPS * clk_gemm / NOMINAL_MHZ, 1),
                     "frac_at_gemm_clock": round(ach / (PEAK_BF16_TFLOPS * clk_gemm / NOMINAL_MHZ), 4),
                     "method": "block 0 of the last launch of each kernel inside the profiled forwards: s_memtime "
                               "(shader clocks) / s_memrealtime (100 MHz) around its main loop"}
    return {"bound": "mfma", "kernel": "256x256x64 bf16 MFMA GEMM on 16x16x32 MFMAs, evenly loaded ping-pong loop (rf::gemm_bf16_pp16e_kernel; rf::gemm_bf16_sk_kernel<256,256,4,2,false,true> where stream-K qualifies)",
            "achieved": round(ach, 1), "peak": PEAK_BF16_TFLOPS, "unit": "TFLOP/s",
            "frac": round(ach / PEAK_BF16_TFLOPS, 4), "sustained_clock": sustained,
            "traffic": traffic, "traffic_unit": "bytes/launch",
            "traffic_source": traffic_src, "traffic_measured_at": traffic_stamp,
            "method": f"one hipEvent in front of every launch inside {T_prof} real forwards, duration = event-to-event "
                      "(kernel + the gap behind it; rf_profile_begin/_end), run right after the timed region in the "
                      "same process on the same box",
            "launches_per_forward": gm["launches"] / T_prof, "avg_launch_us": round(gm["us"] / gm["launches"], 1),
            "flops_per_launch_avg": gm["work"] / gm["launches"],
            "classes": per_fwd,
            # launch durations are event-to-event (kernel + gap), so they tile the profiled region exactly;
            # the profiled pass itself is a few % slower than the un-instrumented timed region (event records)
            "consistency": {"sum_kernel_ms_per_forward": round(sum_ms, 3),
                            "profiled_wall_ms_per_forward": round(wall * 1e3 / T_prof, 3),
                            "timed_ms_per_forward": round(ms_per_forward_timed, 3),
                            "event_overhead_frac": round(sum_ms / ms_per_forward_timed - 1.0, 4),
                            "holds": bool(sum_ms <= wall * 1e3 / T_prof)}}


# ------------------------------------------------------------------------------------------------------
# CPU baseline (the oracle = a port of the reference path; reported, not a target)
# ------------------------------------------------------------------------------------------------------
def host_cpu():
    model, cores = "unknown", set()
    try:
        phys = core = None
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name") and model == "unknown":
                model = line.split(":", 1)[1].strip()
            elif line.startswith("physical id"):
                phys = line.split(":", 1)[1].strip()
            elif line.startswith("core id"):
                core = line.split(":", 1)[1].strip()
            elif not line.strip():
                if phys is not None and core is not None:
                    cores.add((phys, core))
                phys = core = None
    except OSError:
        pass
    logical = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    physical = len(cores) or logical
    return model, min(physical, logical), logical


def cpu_baseline(S_txt, S_img, T, D=3072, heads=24, nd=19, ns=38):
    """(a) cfg1 end to end: 256^2, 4 Euler steps, fp32, through the oracle's denoise() -- the model is the
    FLUX.1-dev shape with ONE DoubleStream and ONE SingleStream block instance referenced 19 / 38 times (same FLOPs
    and the same per-block weight streaming: 1.4 GB / 0.6 GB fp32 per block do not fit any cache level; 47.6 GB of
    distinct fp32 weights would take minutes to initialise for no change in the timing).
    (b) the metric's own workload: one warmed DoubleStream + SingleStream block at the full sequence length,
    extrapolated x(19, 38) blocks x T steps."""
    import torch.nn as nn
    from oracle import flux_oracle as O
    model, cores, logical = host_cpu()
    torch.set_num_threads(cores)
    t_begin = time.perf_counter()
    with torch.no_grad():
        m = O.FluxTransformer2DModel(num_layers=1, num_single_layers=1, num_attention_heads=heads,
                                      attention_head_dim=D // heads).float().eval()
        dbl, sgl = m.transformer_blocks[0], m.single_transformer_blocks[0]
        g = torch.Generator().manual_seed(0)
        x, e = torch.randn(1, S_img, D, generator=g), torch.randn(1, S_txt, D, generator=g)
        temb = torch.randn(1, D, generator=g)
        side = int(round(S_img ** 0.5))
        ids = torch.cat([torch.zeros(S_txt, 3), O.prepare_latent_image_ids(side, side)])
        rope = O.FluxPosEmbed(10000, (16, 56, 56))(ids)
        xe = torch.cat([e, x], 1)
        O.block_forward(dbl, x, e, None, temb, None, image_rotary_emb=rope)              # warm-up (cold: ~4x slower)
        O.single_block_forward(sgl, xe, temb, image_rotary_emb=rope)
        # torch's CPU GEMMs do not scale to every core of a big host (128 threads measured SLOWER than 32 on these
        # shapes): take the best of a few thread counts, and say which
        best = None
        for n in sorted({cores, max(1, cores // 2), max(1, cores // 4), min(cores, 16)}, reverse=True):
            torch.set_num_threads(n)
            t0 = time.perf_counter()
            O.block_forward(dbl, x, e, None, temb, None, image_rotary_emb=rope)
            td_n = time.perf_counter() - t0
            if best is None or td_n < best[1]:
                best = (n, td_n)
        threads, td = best
        torch.set_num_threads(threads)
        t0 = time.perf_counter()
        O.single_block_forward(sgl, xe, temb, image_rotary_emb=rope)
        ts = time.perf_counter() - t0
        # cfg1 end to end
        m.transformer_blocks = nn.ModuleList([dbl] * nd)
        m.single_transformer_blocks = nn.ModuleList([sgl] * ns)
        lat = O.get_noises([0], 256, 256, dtype=torch.float32)[0]
        pe, pooled = torch.randn(1, S_txt, 4096, generator=g), torch.randn(1, 768, generator=g)
        # bounded sample: all 4 steps when one probe step says they fit ~75 s (SURVEY 8d asks for cfg1 end to end), else 1 step
        # timed and x4 stated
        t0 = time.perf_counter()
        out = O.denoise(m, lat, pe, pooled, 1, image_hw=(16, 16))
        t_step = time.perf_counter() - t0
        steps_timed = 1
        if 4 * t_step <= 75.0:
            t0 = time.perf_counter()
            out = O.denoise(m, lat, pe, pooled, 4, image_hw=(16, 16))
            t_cfg1, steps_timed = time.perf_counter() - t0, 4
        else:
            t_cfg1 = 4 * t_step
        assert torch.isfinite(out).all()
    per_latent = T * (nd * td + ns * ts)
    f1 = flops_per_forward(S_txt, 256, D, 4 * D, nd, ns)[0] * 4
    return {"value": 1.0 / per_latent, "unit": "latents/s", "cores": threads, "kind": "port",
            "cpu_model": model, "physical_cores": cores, "logical_cpus": logical, "threads": threads,
            "sample": f"oracle fp32, {threads} threads (best of a sweep up to the {cores} physical cores of {model}); after one warm-up call each: 1 DoubleStream "
                      f"({td:.2f} s) + 1 SingleStream ({ts:.2f} s) block at S={S_txt + S_img}, D={D}; extrapolated "
                      f"x({nd},{ns}) blocks x {T} steps = {per_latent:.0f} s/latent",
            "extrapolated": True,
            "cfg1_end_to_end": {"workload": "BASELINE cfg1: 256x256, 4 Euler steps, fp32, N=1 (weights of one block "
                                            "instance per kind reused over depth)", "seconds": round(t_cfg1, 2),
                                "steps_timed": steps_timed, "extrapolated": steps_timed != 4,
                                "latents_per_s": round(1.0 / t_cfg1, 5), "tflops": round(f1 / t_cfg1 / 1e12, 3)},
            "wall_s_spent": round(time.perf_counter() - t_begin, 1)}



# ------------------------------------------------------------------------------------------------------
# power / clock / temperature telemetry (attribute box-to-box differences)
# ------------------------------------------------------------------------------------------------------
def amdsmi_snapshot(card=0):
    """One `amd-smi metric --json` reading reduced to the numbers that attribute a clock: the firmware's THROTTLE ACCUMULATORS (time
    spent limited by package power tracking = PPT, by temperature, per-XCD "gfx clock below the host limit" split by cause), the
    energy counter (joules, unfiltered), socket power and the per-XCD shader clocks.  None when amd-smi is missing / fails."""
    import shutil
    if not shutil.which("amd-smi"):
        return None
    try:
        r = subprocess.run(["amd-smi", "metric", "-g", str(card), "--json"], capture_output=True, text=True, timeout=20)
        j = json.loads(r.stdout)
        g = (j.get("gpu_data") if isinstance(j, dict) else j)[0]
        val = lambda x: x.get("value") if isinstance(x, dict) else (None if x == "N/A" else x)   # noqa: E731
        th, ck = g.get("throttle", {}), g.get("clock", {})
        xcp = lambda k: (th.get(k) or {}).get("xcp_0") if isinstance(th.get(k), dict) else None   # noqa: E731
        return {"t": time.perf_counter(), "energy_j": val(g.get("energy", {}).get("total_energy_consumption")),
                "socket_power_w": val(g.get("power", {}).get("socket_power")),
                "accumulation_counter": th.get("accumulation_counter"), "ppt_accumulated": th.get("ppt_accumulated"),
                "socket_thermal_accumulated": th.get("socket_thermal_accumulated"), "hbm_thermal_accumulated": th.get("hbm_thermal_accumulated"),
                "vr_thermal_accumulated": th.get("vr_thermal_accumulated"), "prochot_accumulated": th.get("prochot_accumulated"),
                "gfx_below_host_limit_power": xcp("gfx_clk_below_host_limit_power_accumulated"),
                "gfx_below_host_limit_thermal": xcp("gfx_clk_below_host_limit_thermal_accumulated"),
                "gfx_below_host_limit_total": xcp("total_gfx_clk_below_host_limit_accumulated"),
                "low_utilization": xcp("low_utilization_accumulated"),
                "ppt_violation_activity_pct": val(th.get("ppt_violation_activity")),
                "gfx_clk_mhz": [val(ck.get(f"gfx_{i}", {}).get("clk")) for i in range(8)],
                "hotspot_c": val(g.get("temperature", {}).get("hotspot")), "mem_c": val(g.get("temperature", {}).get("mem"))}
    except Exception:                                          # noqa: BLE001 -- telemetry must never fail the bench
        return None


def amdsmi_delta(a, b):
    """What happened between two snapshots: joules -> average power, and the share of the firmware's accumulation ticks in which each
    limiter was active (ppt = package power limit; *_thermal; per-XCD gfx clock held below the host limit, by cause)."""
    if not a or not b:
        return None
    out = {"seconds": round(b["t"] - a["t"], 3)}
    if a.get("energy_j") is not None and b.get("energy_j") is not None and b["t"] > a["t"]:
        out["energy_j"] = round(b["energy_j"] - a["energy_j"], 1)
        out["avg_power_w_from_energy_counter"] = round((b["energy_j"] - a["energy_j"]) / (b["t"] - a["t"]), 1)
    ticks = (b.get("accumulation_counter") or 0) - (a.get("accumulation_counter") or 0)
    out["accumulation_ticks"] = ticks
    if ticks > 0:
        for k in ("ppt_accumulated", "socket_thermal_accumulated", "hbm_thermal_accumulated", "vr_thermal_accumulated", "prochot_accumulated"):
            if a.get(k) is not None and b.get(k) is not None:
                out[k.replace("_accumulated", "_limited_frac")] = round((b[k] - a[k]) / ticks, 4)
        for k in ("gfx_below_host_limit_power", "gfx_below_host_limit_thermal", "gfx_below_host_limit_total", "low_utilization"):
            if a.get(k) and b.get(k):
                out[k + "_frac_per_xcd"] = [round((y - x) / ticks, 4) for x, y in zip(a[k], b[k])]
    out["end_state"] = {k: b.get(k) for k in ("socket_power_w", "gfx_clk_mhz", "hotspot_c", "mem_c", "ppt_violation_activity_pct")}
    return out


class Telemetry:
    """Samples the GPU's socket power, temperatures and shader clock in a background thread while the bench runs: sysfs hwmon when the
    box exposes it (cheap, ~20 Hz), else `rocm-smi --json` (~3 Hz).  `window(t0, t1)` summarises the samples inside a wall-clock
    window, so the timed region and the in-sequence profile each get their own power state."""

    def __init__(self, card=0, period=0.05):
        import glob
        import threading
        self.samples = []                                     # (t, watts, sclk MHz, edge/junction temp C, hbm temp C)
        self.period = period
        self.static = {}
        base = f"/sys/class/drm/card{card}/device"
        hw = sorted(glob.glob(base + "/hwmon/hwmon*"))
        self.hw = hw[0] if hw else None
        self.src = None
        if self.hw and any(os.path.exists(os.path.join(self.hw, f)) for f in ("power1_average", "power1_input")):
            self.src = "sysfs hwmon"
            for f, k in (("power1_cap", "power_cap_w"), ("power1_cap_max", "power_cap_max_w")):
                v = self._read(os.path.join(self.hw, f))
                if v is not None:
                    self.static[k] = round(v / 1e6, 1)
        else:
            import shutil
            if shutil.which("rocm-smi"):
                self.src, self.period = "rocm-smi --showpower --showclocks --showtemp --json", 0.2
                try:
                    r = subprocess.run(["rocm-smi", "--showmaxpower", "--json"], capture_output=True, text=True, timeout=10)
                    d = json.loads(r.stdout)
                    d = d.get(f"card{card}", next(iter(d.values())))
                    for k, v in d.items():
                        if "Max" in k and "Power" in k:
                            self.static["power_cap_w"] = float(v)
                except Exception:                              # noqa: BLE001 -- telemetry must never fail the bench
                    pass
        self.card = card
        self._stop = threading.Event()
        self._th = threading.Thread(target=self._run, daemon=True) if self.src else None
        if self._th:
            self._th.start()

    @staticmethod
    def _read(path):
        try:
            with open(path) as f:
                return float(f.read().strip())
        except (OSError, ValueError):
            return None

    def _sample(self):
        if self.src == "sysfs hwmon":
            pw = self._read(os.path.join(self.hw, "power1_average"))
            if pw is None:
                pw = self._read(os.path.join(self.hw, "power1_input"))
            ck = self._read(os.path.join(self.hw, "freq1_input"))
            t1 = self._read(os.path.join(self.hw, "temp2_input"))          # junction where present
            if t1 is None:
                t1 = self._read(os.path.join(self.hw, "temp1_input"))
            t3 = self._read(os.path.join(self.hw, "temp3_input"))          # memory
            return (time.perf_counter(), pw / 1e6 if pw is not None else None, ck / 1e6 if ck is not None else None,
                    t1 / 1e3 if t1 is not None else None, t3 / 1e3 if t3 is not None else None)
        r = subprocess.run(["rocm-smi", "--showpower", "--showclocks", "--showtemp", "--json"], capture_output=True, text=True, timeout=5)
        d = json.loads(r.stdout)
        d = d.get(f"card{self.card}", next(iter(d.values())))
        pw = ck = tj = tm = None
        for k, v in d.items():
            try:
                if "Power (W)" in k and pw is None:
                    pw = float(v)
                elif k.startswith("sclk clock speed"):
                    ck = float(str(v).strip("()Mhz"))
                elif "Temperature" in k and "junction" in k:
                    tj = float(v)
                elif "Temperature" in k and ("mem" in k.lower() or "hbm" in k.lower()) and tm is None:
                    tm = float(v)
            except ValueError:
                pass
        return (time.perf_counter(), pw, ck, tj, tm)

    def _run(self):
        while not self._stop.is_set():
            try:
                self.samples.append(self._sample())
            except Exception:                                  # noqa: BLE001
                pass
            self._stop.wait(self.period)

    def stop(self):
        if self._th:
            self._stop.set()
            self._th.join(timeout=5)

    def window(self, t0, t1):
        rows = [r for r in self.samples if t0 <= r[0] <= t1]
        out = {"samples": len(rows)}

        def stat(i, name, nd=0):
            v = [r[i] for r in rows if r[i] is not None]
            if v:
                out[name] = {"min": round(min(v), nd), "mean": round(sum(v) / len(v), nd), "max": round(max(v), nd)}
        stat(1, "socket_power_w")
        stat(2, "sclk_mhz")
        stat(3, "temp_junction_c")
        stat(4, "temp_hbm_c")
        return out

    def report(self, windows):
        res = {"source": self.src, **self.static}
        for name, (t0, t1) in windows.items():
            res[name] = self.window(t0, t1)
        return res


# ------------------------------------------------------------------------------------------------------
# ------------------------------------------------------------------------------------------------------
# training step: the other caller of the hot functions, in front of the driver
# ------------------------------------------------------------------------------------------------------
def training_table(dev, pipe, target=1024, cond=512, rank=32, steps=4, warmup=2, optimizer="Prodigy", batch_size=1):
    """One LoRA training step of the 57-block model at the sizes the reference trains at (config.yaml:39-40: target_size 1024,
    condition_size 512 -> 512 text + 4096 image + 1024 condition = 5632 tokens; LoRA r = 32 on the FLUX-Corrector target list,
    config.yaml:50-53; optimizer = the shipped Prodigy config :55-61), batch 1: zero_grad, forward, per-block recompute + backward,
    optimizer update -- FluxTrainer.training_step, timed with events over `steps` steps after `warmup`.

    FLOPs (2 M N K per GEMM, 4 S^2 D per attention forward; element-wise work excluded):  forward F = GEMM_f + ATT_f;  backward
    B = GEMM_f (dX through every frozen weight) + 2.5 ATT_f (LoRA-factor GEMMs ~1 %, not counted);  executed = 2 F + B (every block is
    re-computed in its backward, train_flux/flux/transformer.py:139-157);  model = F + B.

    The result is checked, not only timed: the training forward's loss against the SAME prediction made by the inference path
    (tranformer_forward -> rf_flux_forward, the path the parity suite pins) on the same x_t, before any update."""
    from reflectionflow_amd import ops
    from reflectionflow_amd.flux.pipeline import synthetic_lora_state_dict
    from reflectionflow_amd.flux.transformer import tranformer_forward
    from reflectionflow_amd.train.step import FluxTrainer, lora_parameters
    BF = torch.bfloat16
    tr = pipe.transformer
    D, H = tr.inner_dim, tr.config.num_attention_heads
    nd, ns = len(tr.transformer_blocks), len(tr.single_transformer_blocks)
    mlp = tr.transformer_blocks[0].ff.net[0].proj.out_features if nd else 4 * D
    with torch.no_grad():
        pipe.load_lora_weights(synthetic_lora_state_dict(tr, r=rank, seed=3), adapter_name="default")
    St, Si, Sc = 512, (target // 16) ** 2, (cond // 16) ** 2
    S = St + Si + Sc
    g = torch.Generator(device=dev).manual_seed(1)
    r = lambda *s: torch.randn(*s, generator=g, device=dev).to(BF)   # noqa: E731
    gh, gc = target // 16, cond // 16

    def ids(n):
        return torch.stack([torch.zeros(n * n), torch.arange(n).repeat_interleave(n).float(), torch.arange(n).repeat(n).float()], 1).to(dev)
    cond_ids = ids(gc)
    cond_ids[:, 2] -= gc
    Bn = int(batch_size)      # the reference trains at batch 8 per GPU (config.yaml:11); the samples of a batch run one after the other here
    batch = dict(x_0=r(Bn, Si, 64), img_ids=ids(gh), prompt_embeds=r(Bn, St, tr.config.joint_attention_dim), pooled_prompt_embeds=r(Bn, tr.config.pooled_projection_dim),
                 text_ids=torch.zeros(St, 3, device=dev), condition_latents=r(Bn, Sc, 64), condition_ids=cond_ids, t=torch.full((Bn,), 0.5, device=dev),
                 x_1=r(Bn, Si, 64))
    cfg = {"union_cond_attn": True, "add_cond_attn": False, "latent_lora": False}
    trainer = FluxTrainer(tr, cfg)
    ocfg = {"Prodigy": {"type": "Prodigy", "params": {"lr": 1, "use_bias_correction": True, "safeguard_warmup": True, "weight_decay": 0.01}},
            "AdamW": {"type": "AdamW", "params": {"lr": 1e-4, "weight_decay": 0.01}}}[optimizer]
    opt = trainer.configure_optimizers(ocfg)
    n_lora = sum(p.numel() for p in lora_parameters(tr))
    # result check before any update: training forward vs the inference path on the same x_t (t = 0.5, guidance 1, model.py:209-213)
    with torch.no_grad():
        x_t = (0.5 * batch["x_0"].float() + 0.5 * batch["x_1"].float()).to(BF)
        pred_inf = tranformer_forward(tr, batch["condition_latents"], cond_ids, None, model_config=cfg, hidden_states=x_t,
                                      encoder_hidden_states=batch["prompt_embeds"], pooled_projections=batch["pooled_prompt_embeds"],
                                      timestep=batch["t"], guidance=torch.ones(Bn, device=dev), img_ids=batch["img_ids"], txt_ids=batch["text_ids"],
                                      return_dict=False)[0]
        loss_inf = float(torch.nn.functional.mse_loss(pred_inf, (batch["x_1"] - batch["x_0"]).to(pred_inf.dtype)))
    opt.zero_grad()
    loss0 = trainer.step(batch)
    loss_train = float(loss0.detach())
    loss0.backward()
    gnorm = float(opt.bucket.grad.float().norm())
    assert gnorm > 0 and torch.isfinite(opt.bucket.grad.float()).all(), "training step produced no / non-finite LoRA gradients"
    del loss0                                   # (a live loss keeps the step's autograd graph -- and the factors' gradient accumulators -- alive)
    rel = abs(loss_train - loss_inf) / abs(loss_inf)
    assert rel < 2e-2, f"training forward loss {loss_train} vs inference-path loss {loss_inf}"
    def timed():
        for _ in range(warmup):
            trainer.training_step(batch)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        h0 = time.perf_counter()
        e0.record()
        for _ in range(steps):
            last = trainer.training_step(batch)
        e1.record()
        host = (time.perf_counter() - h0) * 1000.0 / steps    # the host's time to enqueue a step (no sync inside)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / steps, host, last

    def grads_now():
        opt.zero_grad()
        trainer.step(batch).backward()
        return opt.bucket.grad.clone()

    # (1) the reference's flag: gradient_checkpointing true -- every block re-runs its forward inside the backward (transformer.py:139-157)
    trainer.gradient_checkpointing = True
    ms_ckpt, host_ckpt, loss = timed()
    # (2) "auto": blocks keep their intermediates while they fit the free HBM -- the same backward kernels on the same operands
    trainer.gradient_checkpointing = "auto"
    ms, host_ms, loss = timed()
    kept = trainer.kept_blocks * (Bn if Bn > 1 else 1)      # (a batch runs sample by sample in this mode: kept_blocks counts the last sample's)
    # both modes at the SAME parameters (no optimizer step in between): the flat gradient bucket, bit for bit
    g_auto = grads_now()
    trainer.gradient_checkpointing = True
    keep_equal = bool(torch.equal(g_auto, grads_now()))
    trainer.gradient_checkpointing = "auto"
    assert keep_equal, "gradients with kept activations != gradients with per-block recompute"
    del g_auto
    # (3) the same step replayed as ONE hipGraph (zero_grad + forward + backward captured; clip + optimizer update eager): what the host
    #     has to do per step shrinks from ~2700 enqueues to one replay + <= 8 launches.  Checked bit-equal to the eager step first.
    def snapshot():
        return opt.bucket.param.detach().clone(), {k: (v.detach().clone() if isinstance(v, torch.Tensor) else v) for k, v in opt.state_dict().items()}

    def restore(snap):
        with torch.no_grad():
            opt.bucket.param.copy_(snap[0])
        opt.load_state_dict(snap[1])
    hipgraph = None
    if Bn == 1:
        snap = snapshot()
        l_eager = trainer.training_step(batch).clone()
        p_eager = opt.bucket.param.clone()
        restore(snap)
        torch.cuda.empty_cache()
        run = trainer.capture_training_step(batch)
        l_graph = run(batch).clone()
        graph_equal = bool(torch.equal(p_eager, opt.bucket.param) and torch.equal(l_eager, l_graph))
        assert graph_equal, "the captured training step differs from the eager step"
        del p_eager
        for _ in range(max(1, warmup - 1)):
            run(batch)
        torch.cuda.synchronize()
        g0, g1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        hg0 = time.perf_counter()
        g0.record()
        for _ in range(steps):
            run(batch)
        g1.record()
        host_graph = (time.perf_counter() - hg0) * 1000.0 / steps
        torch.cuda.synchronize()
        hipgraph = {"what": "FluxTrainer.capture_training_step: zero_grad + forward + backward as one hipGraph replay, clip + optimizer update eager",
                    "ms_per_step": round(g0.elapsed_time(g1) / steps, 2), "host_enqueue_ms_per_step": round(host_graph, 2),
                    "bit_equal_to_the_eager_step": graph_equal}
        del run
        torch.cuda.empty_cache()
    o0, o1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    o0.record()
    for _ in range(4):
        opt.step()
    o1.record()
    torch.cuda.synchronize()
    opt_ms = o0.elapsed_time(o1) / 4
    with ops.profile(max_launches=4000 * Bn + 4000) as pr:
        trainer.training_step(batch)
        torch.cuda.synchronize()
    gemm_f = nd * S * (2 * D * 3 * D + 2 * D * D + 2 * 2 * D * mlp) + ns * S * (2 * D * (3 * D + mlp) + 2 * (D + mlp) * D)
    att_f = (nd + ns) * 4 * S * S * D
    F_, B_ = Bn * (gemm_f + att_f), Bn * (gemm_f + 2.5 * att_f)
    X_ = F_ + B_ + F_ * (1.0 - kept / float((nd + ns) * Bn))     # executed in 'auto' mode: a block that kept its intermediates runs no second forward
    cl = pr.classes
    state_bytes = opt.exp_avg.element_size()
    # (Prodigy starts at d0 = 1e-6: over the handful of steps timed here the loss does not move yet; d and the step count are reported)
    prodigy_state = {k: (round(v, 12) if isinstance(v, float) else v) for k, v in opt.d_state().items() if k in ("d", "d_hat", "k")} \
        if optimizer == "Prodigy" else None
    return {"what": f"ONE LoRA training step (train_flux/train/model.py:164-238 + optimizer), {nd} double + {ns} single blocks, S = {St} text + {Si} image "
                    f"({target}^2) + {Sc} condition ({cond}^2) = {S} tokens (config.yaml:39-40), LoRA r = {rank} on the condition rows, batch {Bn}"
                    + (" (the reference's config.yaml:11 trains at batch 8; samples of a batch run sequentially, one optimizer update per batch)" if Bn == 1 else
                       " (samples run sequentially; one optimizer update per batch)"),
            "batch_size": Bn, "ms_per_sample": round(ms / Bn, 2),
            "ms_per_step": round(ms, 2), "host_enqueue_ms_per_step": round(host_ms, 2), "steps": steps, "warmup": warmup,
            "hipgraph": hipgraph, "gradient_clip_val": trainer.gradient_clip_val,
            "activations": {"what": "FluxTrainer(gradient_checkpointing='auto'): a block keeps its forward intermediates while they fit the free HBM "
                                    "(~0.8 GB per block at 5632 tokens) instead of re-running its forward inside the backward; ms_per_step, the "
                                    "class table and tflops_model are this mode",
                            "blocks_keeping_their_intermediates": kept, "of": (nd + ns) * Bn,
                            "batch": "one sample at a time, each with 1 / B of the loss (FluxTrainer.training_step(sample_by_sample=True), the default "
                                     "for B > 1 here): one sample's activations alive at a time" if Bn > 1 else "1 sample",
                            "gradients_bit_equal_to_gradient_checkpointing": keep_equal},
            "gradient_checkpointing_true": {"what": "the reference's training flag (config.yaml gradient_checkpointing: true, transformer.py:139-157): "
                                                    "every block re-computed in its backward, executed FLOPs 2 F + B",
                                            "ms_per_step": round(ms_ckpt, 2), "host_enqueue_ms_per_step": round(host_ckpt, 2),
                                            "tflops_executed": round((2 * F_ + B_) / ms_ckpt / 1e9, 1),
                                            "frac_of_bf16_mfma_peak_executed": round((2 * F_ + B_) / ms_ckpt / 1e9 / PEAK_BF16_TFLOPS, 4),
                                            "frac_of_bf16_mfma_peak_model": round((F_ + B_) / ms_ckpt / 1e9 / PEAK_BF16_TFLOPS, 4)},
            "optimizer": {"type": optimizer, "params": ocfg["params"], "kernel": "rf_lora_prodigy (3 launches, d on the device)" if optimizer == "Prodigy" else "rf_lora_adamw (1 launch)",
                          "ms": round(opt_ms, 3), "lora_parameters": n_lora, "prodigy_distance_estimate": prodigy_state, "state": "bf16" if state_bytes == 2 else "fp32",
                          "parity": "unpinned (prodigyopt not available offline; oracle/optim_oracle.py restates the published algorithm)" if optimizer == "Prodigy"
                                    else "within 1 bf16 ulp of torch.optim.AdamW (tests/test_round5_gpu.py)"},
            "tflop": {"forward": round(F_ / 1e12, 2), "backward": round(B_ / 1e12, 2), "executed_with_recompute": round((2 * F_ + B_) / 1e12, 2),
                      "model": round((F_ + B_) / 1e12, 2), "executed_this_mode": round(X_ / 1e12, 2)},
            "tflops_executed": round(X_ / ms / 1e9, 1), "tflops_model": round((F_ + B_) / ms / 1e9, 1),
            "frac_of_bf16_mfma_peak_executed": round(X_ / ms / 1e9 / PEAK_BF16_TFLOPS, 4),
            "frac_of_bf16_mfma_peak_model": round((F_ + B_) / ms / 1e9 / PEAK_BF16_TFLOPS, 4),
            "loss": {"training_forward": round(loss_train, 6), "inference_path_same_inputs": round(loss_inf, 6), "rel_diff": round(rel, 6),
                     "after_timed_steps": round(float(loss), 6), "lora_grad_norm_step0": round(gnorm, 6)},
            "classes": {k: {"launches": v["launches"], "ms": round(v["us"] / 1e3, 3),
                            **({"tflops": round(v["work"] / v["us"] / 1e6, 1)} if k in ("gemm_main", "gemm_small", "attention", "attention_bwd") else
                               {"GBps": round(v["work"] / v["us"] / 1e3, 1)})} for k, v in cl.items() if v["launches"]},
            "profiled_sum_ms": round(sum(v["us"] for v in cl.values()) / 1e3, 2), "dropped_launches": pr.dropped,
            "peak_hbm_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)}


def self_launch(n: int) -> int:
    """`python bench.py --gpus N` outside a launcher: start N ranks of this script on this node."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC (RCCL across processes)
    env.setdefault("OMP_NUM_THREADS", "8")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    return subprocess.call(cmd, env=env)


def gather_per_rank(shard, values, device):
    """[world, len(values)] float64 on the host: every rank's own numbers (per-rank time spread of an N > 1 run)."""
    mine = torch.tensor(values, device=device, dtype=torch.float64)
    every = torch.empty(shard.world_size * mine.numel(), device=device, dtype=torch.float64)
    torch.distributed.all_gather_into_tensor(every, mine)
    return every.view(shard.world_size, mine.numel()).cpu()


def launch_check(args):
    """CPU plumbing test of the N-rank launch (tests/test_search_dist.py): process group + the round-boundary
    exchange with stub scores, no GPU work.  NOT a bench result."""
    from reflectionflow_amd.tts import search
    shard = search.init_distributed(backend="gloo")
    n = 2 * shard.world_size
    local = {i: (float(i) / n, i % 2) for i in shard.mine(n)}
    scores = search.allgather_scores(shard, n, local)
    best = search.select_topk(scores, 1)
    if shard.world_size > 1:
        every = gather_per_rank(shard, [float(shard.rank), 1.0, 2.0], torch.device("cpu"))
        assert every.shape == (shard.world_size, 3) and every[:, 0].tolist() == [float(r) for r in range(shard.world_size)]
        torch.distributed.barrier()
    if shard.rank == 0:
        print(json.dumps({"launch_check": True, "n_gpus": shard.world_size, "selected_candidate": best[0],
                          "scores": scores}), flush=True)
    if shard.world_size > 1:
        torch.distributed.destroy_process_group()


def dump_outputs(path, latent, scores):
    """What the timed path handed its caller in the last timed step: the latent generate() returned (bf16 -> float32, exact) and
    the round boundary's verifier records.  ~1 MB at 1024^2."""
    import numpy as np
    os.makedirs(path, exist_ok=True)
    np.save(os.path.join(path, "latents.npy"), latent.float().cpu().numpy())
    np.save(os.path.join(path, "scores.npy"), np.array([s for s, _ in scores], dtype=np.float32))
    np.save(os.path.join(path, "labels.npy"), np.array([lab for _, lab in scores], dtype=np.float32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=2, help="timed latents (each a full 50-step denoise) per GPU")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--res", type=int, default=1024)
    ap.add_argument("--denoise-steps", type=int, default=50)
    ap.add_argument("--full", action="store_true",
                    help="also run the parity check, telemetry and the separately reported tables (roofline, attention, VAE, text "
                         "encoders, CPU baseline, training); the --no-* options below switch single parts of it off")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last timed latent and the round's scores as DIR/*.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-roofline", action="store_true")
    ap.add_argument("--no-isolated-shapes", action="store_true")
    ap.add_argument("--small", action="store_true", help="debug: 2+2-block model (NOT a valid bench result)")
    ap.add_argument("--launch-check", action="store_true", help="CPU plumbing test of the N-rank launch (not a bench)")
    ap.add_argument("--dist-backend", choices=["nccl", "gloo"], default=None,
                    help="process-group backend for N > 1 (default nccl = RCCL); gloo for the shared-GPU rehearsal")
    ap.add_argument("--ranks-share-gpu", action="store_true",
                    help="rehearsal on a 1-GPU box: every rank uses cuda:0 (plumbing check, not a scaling measurement)")
    ap.add_argument("--no-attention-table", action="store_true")
    ap.add_argument("--no-vae", action="store_true", help="skip the (separately reported) VAE decode / encode timings")
    ap.add_argument("--no-text", action="store_true", help="skip the (separately reported) T5-XXL / CLIP-L text-encoder timings")
    ap.add_argument("--graph", action="store_true", help="force hipGraph replay of each candidate's denoise loop (RF_DENOISE_GRAPH=1; the default for T >= 16)")
    ap.add_argument("--no-graph", action="store_true", help="eager launches (RF_DENOISE_GRAPH=0)")
    ap.add_argument("--no-parity-check", action="store_true", help="skip the checksum of one timed latent against the per-step path")
    ap.add_argument("--lean", action="store_true", help="N > 1 rehearsals on one GPU: no graph capture, release the allocator cache (memory)")
    ap.add_argument("--no-train", action="store_true", help="skip the (separately reported) LoRA training-step measurement")
    ap.add_argument("--train-only", action="store_true", help="only the training-step measurement (prints its table, not a bench line)")
    ap.add_argument("--train-optimizer", choices=["Prodigy", "AdamW"], default="Prodigy")
    ap.add_argument("--train-target", type=int, default=1024)
    ap.add_argument("--train-cond", type=int, default=512)
    ap.add_argument("--train-batch", type=int, default=1, help="samples per training step (the reference's config trains at 8; default 1 keeps the default run short)")
    ap.add_argument("--n1-value", type=float, default=None,
                    help="the N = 1 value of this metric: with --gpus N > 1 the line then also carries scaling_efficiency = value / (N * n1_value)")
    args = ap.parse_args()

    if args.graph:
        os.environ["RF_DENOISE_GRAPH"] = "1"
    if args.no_graph or args.lean:
        os.environ["RF_DENOISE_GRAPH"] = "0"
    world_env = os.environ.get("WORLD_SIZE")
    if world_env is None and args.gpus > 1:
        sys.exit(self_launch(args.gpus))
    if args.launch_check:
        return launch_check(args)

    from reflectionflow_amd import _lib
    from reflectionflow_amd.tts import search
    from reflectionflow_amd.tts.utils import get_noises
    from reflectionflow_amd.flux.generate import generate

    _lib.load()
    local = 0 if args.ranks_share_gpu else int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    if args.ranks_share_gpu and args.dist_backend in (None, "nccl") and int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("--ranks-share-gpu needs --dist-backend gloo (RCCL refuses two ranks on one device)")
    if args.ranks_share_gpu:
        os.environ["LOCAL_RANK"] = "0"        # init_distributed() binds the rank to cuda:LOCAL_RANK for nccl
    shard = search.init_distributed(args.dist_backend)
    if shard.world_size != args.gpus:
        raise SystemExit(f"--gpus {args.gpus} but WORLD_SIZE={shard.world_size}")
    backend = torch.distributed.get_backend() if shard.world_size > 1 else None
    dev = torch.device("cuda", local)
    numa = search.bind_host_threads_to_gpu_numa_node(local) if shard.world_size > 1 else None
    ranks = search.describe_ranks(shard, local, numa)       # (a collective: every rank calls it)

    cfg = dict(num_layers=2, num_single_layers=2) if args.small else {}
    pipe = build_model(dev, cfg, seed=0)
    tr = pipe.transformer
    if args.train_only:
        out = training_table(dev, pipe, args.train_target, args.train_cond, optimizer=args.train_optimizer, batch_size=args.train_batch,
                             steps=4 if args.train_batch == 1 else 2, warmup=2 if args.train_batch == 1 else 1)
        if args.small:
            out["INVALID"] = "debug model (--small)"
        print(json.dumps({"training": out}), flush=True)
        return
    D, heads = tr.inner_dim, tr.config.num_attention_heads
    nd, ns = len(tr.transformer_blocks), len(tr.single_transformer_blocks)
    S_txt, S_img, T = 512, (args.res // 16) ** 2, args.denoise_steps
    g = torch.Generator().manual_seed(1)
    pe = torch.randn(1, S_txt, tr.config.joint_attention_dim, generator=g).to(dev).to(torch.bfloat16)
    pooled = torch.randn(1, tr.config.pooled_projection_dim, generator=g).to(dev).to(torch.bfloat16)
    n_total = (args.warmup + args.steps)
    # candidate c = j * world + rank of the timed round is seeded by c alone (world-size independent selection); warm-up
    # latents use seeds outside that range
    seeds = [10 ** 6 + 1000 * shard.rank + i for i in range(args.warmup)] + \
            [7919 * (j * shard.world_size + shard.rank) + 13 for j in range(args.steps)]
    noises = get_noises(2 ** 31 - 1, n_total, args.res, args.res, device=dev, dtype=torch.bfloat16, seeds=seeds)

    def one_latent(seed, steps=T):
        return generate(pipe, model_config={}, height=args.res, width=args.res, num_inference_steps=steps,
                        guidance_scale=3.5, latents=noises[seed], prompt_embeds=pe, pooled_prompt_embeds=pooled,
                        output_type="latent").images

    def barrier():
        if shard.world_size > 1:
            torch.distributed.barrier()

    tele = Telemetry(local) if shard.rank == 0 and args.full else None
    coll_dev = dev if backend == "nccl" else torch.device("cpu")

    def round_boundary(lat_list, seed_list, n_round):
        """ONE batched verifier call on the device for this rank's candidates (search.stub_score_batch: the score_batch contract a
        real on-device verifier plugs into), ONE all-gather of the 8-byte {f32 score, i32 label} records (RCCL), the same ordering
        on every rank (tts_reflectionflow.py:165-170)."""
        sc, lab = search.stub_score_batch(torch.stack([o.reshape(-1, o.shape[-1]) for o in lat_list]), seed_list)
        s_all, l_all = search.allgather_score_tensors(shard, n_round, sc, lab, device=coll_dev)
        scores = [(float(a), int(b)) for a, b in zip(s_all.tolist(), l_all.tolist())]
        return scores, search.select_topk(scores, 1)

    warm = []
    for i in range(args.warmup):
        warm.append(one_latent(seeds[i]))
    if warm:                                                 # the boundary's first-use costs (stack, stub kernels, the collective's
        for _ in range(2):                                   # connection set-up) belong to warm-up, as the denoise's do
            round_boundary(warm, seeds[:args.warmup], args.warmup * shard.world_size)
    del warm
    if args.lean:
        torch.cuda.empty_cache()
    torch.cuda.synchronize()
    barrier()
    smi0 = amdsmi_snapshot(local) if shard.rank == 0 and args.full else None
    t0 = time.perf_counter()
    outs = []
    for i in range(args.steps):
        outs.append(one_latent(seeds[args.warmup + i]))
    n_round = args.steps * shard.world_size
    torch.cuda.synchronize()                             # (so that round_boundary_ms is the boundary's own cost, not the last denoise draining)
    t_rb = time.perf_counter()
    dt_local = t_rb - t0                                 # this rank's own candidates, before it meets the others in the boundary's collective
    scores, best = round_boundary(outs, seeds[args.warmup:], n_round)
    torch.cuda.synchronize()
    round_boundary_s = time.perf_counter() - t_rb
    barrier()
    dt = time.perf_counter() - t0
    t_end = t0 + dt
    smi1 = amdsmi_snapshot(local) if shard.rank == 0 and args.full else None
    per_rank = None
    if shard.world_size > 1:
        # MAX over ranks: a device tensor over RCCL, a host tensor over gloo (gloo has no GPU all_reduce here)
        tmax = torch.tensor([dt], device=coll_dev, dtype=torch.float64)
        torch.distributed.all_reduce(tmax, op=torch.distributed.ReduceOp.MAX)
        dt = float(tmax.item())
        every = gather_per_rank(shard, [dt_local, round_boundary_s, torch.cuda.max_memory_allocated() / 2 ** 30], coll_dev)
        per_rank = {"seconds": [round(float(v), 3) for v in every[:, 0]],
                    "min_s": round(float(every[:, 0].min()), 3), "mean_s": round(float(every[:, 0].mean()), 3),
                    "max_s": round(float(every[:, 0].max()), 3),
                    "spread_frac": round(float((every[:, 0].max() - every[:, 0].min()) / every[:, 0].mean()), 4),
                    "round_boundary_ms": [round(float(v) * 1e3, 2) for v in every[:, 1]],
                    "peak_hbm_gib": [round(float(v), 1) for v in every[:, 2]]}
    assert all(torch.isfinite(o.float()).all() for o in outs), "non-finite latents"
    if args.dump_outputs and shard.rank == 0 and outs:
        dump_outputs(args.dump_outputs, outs[-1], scores)

    # the timed region proves RESULTS, not only work: the first timed latent -- produced by the fast path
    # (one C call / one hipGraph replay for the T steps) -- against the same candidate on the general PER-STEP path
    # (tranformer_forward + scheduler.step per step, eager launches), which the GPU parity suite pins to the oracle
    parity = None
    if args.full and not args.no_parity_check and shard.rank == 0 and not args.lean:
        import hashlib
        noop = lambda pipe_, i_, t_, kw: {}                  # noqa: E731 -- a callback selects the general path
        sd0 = seeds[args.warmup]
        ref = generate(pipe, model_config={}, height=args.res, width=args.res, num_inference_steps=T, guidance_scale=3.5,
                       latents=noises[sd0], prompt_embeds=pe, pooled_prompt_embeds=pooled, output_type="latent",
                       callback_on_step_end=noop).images
        a, b = outs[0].float(), ref.float()
        # ... and against the fast path launched eagerly (no hipGraph): must be bit-identical
        os.environ["RF_DENOISE_GRAPH"], env_graph = "0", os.environ.get("RF_DENOISE_GRAPH")
        try:
            eager = one_latent(sd0)
        finally:
            if env_graph is None:
                os.environ.pop("RF_DENOISE_GRAPH", None)
            else:
                os.environ["RF_DENOISE_GRAPH"] = env_graph
        # the per-step path forms the time embedding and the modulation row of ONE timestep (M = 1), the fast path those of all T at
        # once (M = T): both on rf_gemm_bf16, whose rows do not depend on M -- checked here, not assumed
        from reflectionflow_amd import engine as E_
        eng = E_.engine_for(tr)
        sch_ts = pipe.scheduler.timesteps.to(dev)
        ts_all = (sch_ts.to(torch.bfloat16) / 1000).to(torch.bfloat16) * 1000
        gd_all = torch.full((T,), 3.5, device=dev).to(torch.bfloat16) * 1000
        te_all = eng.temb(ts_all, gd_all, pooled.expand(T, -1))
        te_one = torch.cat([eng.temb(ts_all[i:i + 1], gd_all[i:i + 1], pooled) for i in range(T)])
        mod_all = eng.mod_table(te_all)
        mod_one = torch.cat([eng.mod_table(te_all[i:i + 1]) for i in range(0, T, max(1, T // 4))])
        parity = {"what": "timed latent 0 (fast path: T steps in one C call, replayed as a hipGraph) vs the same candidate (a) on the fast "
                          "path launched eagerly, (b) on the per-step general path (tranformer_forward + scheduler.step per step)",
                  "bit_equal_to_eager_fast_path": bool(torch.equal(outs[0], eager)),
                  "bit_equal_to_per_step_path": bool(torch.equal(outs[0], ref)),
                  "rel_l2_to_per_step_path": float(((a - b).norm() / b.norm()).item()),
                  "time_embedding_batched_equals_row_by_row": bool(torch.equal(te_all, te_one)),
                  "modulation_table_batched_equals_row_by_row": bool(torch.equal(mod_all[::max(1, T // 4)][:mod_one.shape[0]], mod_one)),
                  "sha256_timed": hashlib.sha256(outs[0].cpu().view(torch.int16).numpy().tobytes()).hexdigest()[:16],
                  "sha256_per_step": hashlib.sha256(ref.cpu().view(torch.int16).numpy().tobytes()).hexdigest()[:16]}
        assert parity["bit_equal_to_eager_fast_path"], f"hipGraph replay differs from the eager fast path: {parity}"
        # round 5: time_text_embed runs on the row-invariant rf_gemm_bf16 in BOTH paths (engine.temb), so the timed latent IS the
        # parity-pinned per-step path's latent, bit for bit, at any T
        assert parity["time_embedding_batched_equals_row_by_row"] and parity["modulation_table_batched_equals_row_by_row"], parity
        assert parity["bit_equal_to_per_step_path"] and parity["sha256_timed"] == parity["sha256_per_step"], \
            f"timed latent differs from the per-step path: {parity}"
        del eager, te_all, te_one, mod_all, mod_one
        del ref

    if shard.rank == 0:
        total_latents = args.steps * shard.world_size
        value = total_latents / dt
        mlp = tr.transformer_blocks[0].ff.net[0].proj.out_features if nd else 4 * D
        f_fwd, f_gemm, f_attn = flops_per_forward(S_txt, S_img, D, mlp, nd, ns, tr.config.in_channels,
                                                  tr.config.joint_attention_dim)
        step_tflops = f_fwd * T * total_latents / dt / 1e12
        res = {
            "metric": "1024^2 latents/sec (50-step FLUX denoise) per node", "value": round(value, 5), "unit": "latents/s",
            "n_gpus": shard.world_size, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(dt / args.steps * 1e3, 2), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
            "config": {"workload": f"FLUX.1-dev {args.res}x{args.res}, {T} Euler steps, 1 candidate per GPU per step "
                                   f"(BASELINE cfg2{'; candidates sharded, cfg3-style' if shard.world_size > 1 else ''})",
                       "tokens": S_txt + S_img, "blocks": f"{nd} double + {ns} single", "guidance": 3.5,
                       "parallelism": f"candidate-parallel x{shard.world_size}, weights replicated"},
            "whole_path": {"tflop_per_forward": round(f_fwd / 1e12, 2), "achieved_tflops_per_gpu": round(step_tflops / shard.world_size, 1),
                           "frac_of_bf16_mfma_peak": round(step_tflops / shard.world_size / PEAK_BF16_TFLOPS, 4)},
            "denoise_loop": "eager launches" if os.environ.get("RF_DENOISE_GRAPH", "") == "0" or (os.environ.get("RF_DENOISE_GRAPH", "") == "" and T < 16)
                            else "one hipGraph per (geometry, T) replayed per candidate",
            "selected_candidate": best[0], "selected_seed": 7919 * best[0] + 13,
            "round_boundary_ms": round(round_boundary_s * 1e3, 2),
            "round_boundary_frac_of_a_candidate": round(round_boundary_s / (dt / args.steps), 5),
            "timed_latent_parity": parity,
            "per_rank": per_rank,
            "peak_hbm_gib": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1),
            # N > 1: the world size as the BACKEND reports it, the collective library's version and every rank's device (name, PCI bus id,
            # uuid, host) -- what proves that N ranks on N devices produced this line; host threads pinned to the GPU's NUMA node
            "dist": dict(ranks, ranks_share_gpu=bool(args.ranks_share_gpu)) if shard.world_size > 1 else None,
        }
        if args.ranks_share_gpu:
            res["INVALID"] = "rehearsal: all ranks on one GPU (plumbing check, not a scaling measurement)"
        if args.small:
            res["INVALID"] = "debug model (--small), not the BASELINE workload"
        if shard.world_size == 1 and args.full:
            if not args.no_roofline:
                res["roofline"] = in_sequence_roofline(lambda steps: one_latent(seeds[0], steps), PROFILE_STEPS,
                                                       dt / args.steps * 1e3 / T, (S_txt, S_img, D, mlp))
                if not args.no_isolated_shapes:
                    res["roofline"]["isolated_shapes"] = isolated_shapes(dev, S_txt, S_img, D, 4 * D, heads, nd, ns)
            if not args.no_attention_table:
                res["attention"] = attention_table(dev, pipe, S_txt + S_img, heads)
            if not args.no_vae:
                res["vae"] = vae_table(dev, args.res)
            if not args.no_text:
                res["text_encoders"] = text_table(dev)
            if not args.no_cpu_baseline:
                res["cpu_baseline"] = cpu_baseline(S_txt, S_img, T, D, heads, nd, ns)
            if not args.no_train and not args.small and not args.lean:
                # last: it loads a LoRA into the model and re-homes its factors (the inference measurements above ran without one)
                res["training"] = training_table(dev, pipe, args.train_target, args.train_cond, optimizer=args.train_optimizer, batch_size=args.train_batch)
        if args.n1_value and shard.world_size > 1:
            res["scaling_efficiency"] = round(value / (shard.world_size * args.n1_value), 4)
            res["n1_value"] = args.n1_value
        if tele is not None:
            tele.stop()
            wins = {"timed_region": (t0, t_end)}
            if getattr(in_sequence_roofline, "window", None):
                wins["in_sequence_profile"] = in_sequence_roofline.window
            res["telemetry"] = tele.report(wins)
            res["telemetry"]["timed_region_firmware_counters"] = amdsmi_delta(smi0, smi1)
        print(json.dumps(res), flush=True)
    if shard.world_size > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()

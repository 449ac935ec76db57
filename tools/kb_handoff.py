"""Times the reflection search's ROUND BOUNDARY for one candidate at 1024^2 -> 512^2, host path against device path, in one process:

    save (PNG) + the verifier's score input (decode + rf_clip_preprocess) + the parent's "cot" condition for TWO children

host path   = `device_handoff: false`: three VAE decodes, a float image copied to the host, PIL resize, preprocess, one VAE encode per
              child, PNG compression on the calling thread;
device path = one decode, rf_image_levels, rf_pil_resize_to_vae_input, one VAE encode, PNG compression on the writer thread.  It is
              timed three ways: `device` (the caller's critical path: the writer thread is joined OUTSIDE the timed window, as it overlaps
              the next candidate's denoise loop in a search), `device_joined` (join inside the window) and `device_sync_png` (no thread:
              what the kernels and the single decode buy on their own).

Each sample is a host clock around work that ends in a device synchronise, with a device-event pair around the same window (the
event time misses host work done after the last launch).  The paths alternate within each repetition; the spread printed is min .. max
over the repetitions.  Then one synthetic search (pool + 1 round, N candidates, small transformer, FLUX-shaped VAE, ViT-L/14 CLIP) per
setting, alternating.  One JSON line per table; `amd-smi metric` snapshots bracket the run for the clock state.

    python tools/kb_handoff.py [--reps 7] [--size 1024] [--csize 512] [--search-reps 2] [--branch 4] > profiles/handoff_device.json
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SMALL_FLUX = dict(num_layers=1, num_single_layers=1, num_attention_heads=2, joint_attention_dim=256, pooled_projection_dim=64)


def stats(xs):
    return {"median_ms": round(statistics.median(xs), 3), "min_ms": round(min(xs), 3), "max_ms": round(max(xs), 3), "n": len(xs)}


def timed(fn, after=None):
    """(wall ms, device-event ms) of fn(), the wall clock ending in a synchronise; `after` runs outside the window."""
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    if after is not None:
        after()
    return wall, e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--size", type=int, default=1024)
    ap.add_argument("--csize", type=int, default=512)
    ap.add_argument("--search-reps", type=int, default=2)
    ap.add_argument("--branch", type=int, default=4)
    ap.add_argument("--candidate-ms", type=float, default=3000.0, help="the denoise time of one candidate the boundary is set against")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("kb_handoff: needs a GPU (a CPU run measures nothing)")
    import bench as B
    from reflectionflow_amd.flux.pipeline import FluxPipeline
    from reflectionflow_amd.tts import clip_verifier as CV
    from reflectionflow_amd.tts import runner, search
    dev = torch.device("cuda:0")
    H = W = args.size
    cs = args.csize
    snap0 = B.amdsmi_snapshot(0)
    pipe = FluxPipeline.synthetic(SMALL_FLUX, seed=0, device=dev, with_vae=True)          # FLUX.1-dev VAE shape
    pipe.set_progress_bar_config(disable=True)
    pipe.enable_hip_vae()
    v = CV.ClipScoreVerifier(pipe, CV.synthetic_clip_state(CV.VIT_L14, 0), CV.synthetic_tokenize(CV.VIT_L14["text"]["vocab"]), H, W)
    lat = (torch.randn(1, (H // 16) * (W // 16), 64, generator=torch.Generator().manual_seed(1)) * 1.2).to(dev, torch.bfloat16)
    patches = v.vision.alloc_patches(1)
    tmp = tempfile.mkdtemp(prefix="kb_handoff_")
    writer = runner.PngWriter()
    gens = lambda: [torch.Generator(device="cpu").manual_seed(s) for s in (5, 6)]          # noqa: E731

    def children(cond):
        return [cond.with_generator(g).encode(pipe)[0] for g in gens()]

    # ---- the stages of each path (each ends where the next begins; nothing synchronises in between) ------------------------------
    def host_save():
        runner._save(os.path.join(tmp, "host"), lat, pipe, H, W, device=False)

    def host_score_input():
        v._decode_into(lat, patches, 0)

    def host_condition():
        return children(runner.candidate_condition(pipe, lat, H, W, cs, device=False))

    def host():
        host_save(), host_score_input(), host_condition()

    def device(use_writer=True):
        halo = runner.decode_halo(pipe, lat, H, W)
        runner._save(os.path.join(tmp, "dev"), lat, pipe, H, W, halo=halo, writer=writer if use_writer else None)
        v._halo_into(halo, patches, 0)
        return children(runner.candidate_condition(pipe, lat, H, W, cs, halo=halo))

    def device_joined():
        device()
        writer.join()

    paths = {"host": (host, None), "device": (device, writer.join), "device_joined": (device_joined, None),
             "device_sync_png": (lambda: device(False), None)}
    stages = {"host_save": host_save, "host_score_input": host_score_input, "host_condition_2_children": host_condition,
              "decode_halo": lambda: runner.decode_halo(pipe, lat, H, W)}
    for fn, after in paths.values():                                                      # warm-up: workspaces, code objects, tables
        fn()
        if after:
            after()
    tok_h, tok_d = host_condition(), device()
    writer.join()
    torch.cuda.synchronize()
    same = all(torch.equal(a, b) for a, b in zip(tok_h, tok_d)) and \
        open(os.path.join(tmp, "host.png"), "rb").read() == open(os.path.join(tmp, "dev.png"), "rb").read()
    wall = {k: [] for k in paths}
    evt = {k: [] for k in paths}
    st = {k: [] for k in stages}
    for _ in range(args.reps):
        for k, (fn, after) in paths.items():                                              # alternate the paths inside a repetition
            w, e = timed(fn, after)
            wall[k].append(w)
            evt[k].append(e)
        for k, fn in stages.items():
            st[k].append(timed(fn)[0])
    out = {"table": "boundary_per_candidate", "size": H, "condition_size": cs, "children": 2, "identical_outputs": bool(same),
           "wall": {k: stats(x) for k, x in wall.items()}, "device_events": {k: stats(x) for k, x in evt.items()},
           "stages_wall": {k: stats(x) for k, x in st.items()}}
    h, d, dj, ds = (out["wall"][k]["median_ms"] for k in ("host", "device", "device_joined", "device_sync_png"))
    spread = max(out["wall"][k]["max_ms"] - out["wall"][k]["min_ms"] for k in ("host", "device"))
    out["summary"] = {"host_ms": h, "device_ms": d, "gain_ms": round(h - d, 3), "run_to_run_spread_ms": round(spread, 3),
                      "gain_without_png_thread_ms": round(h - ds, 3), "gain_from_png_thread_ms": round(ds - d, 3),
                      "png_thread_is_larger_part": bool(ds - d > h - ds),
                      "device_not_slower_than_host_within_spread": bool(d <= h + spread),
                      "boundary_share_of_candidate": {"candidate_ms": args.candidate_ms, "host": round(h / (args.candidate_ms + h), 4),
                                                      "device": round(d / (args.candidate_ms + d), 4),
                                                      "device_joined": round(dj / (args.candidate_ms + dj), 4)}}
    print(json.dumps(out), flush=True)

    # ---- one synthetic search (pool + 1 round) per setting ------------------------------------------------------------------------
    cfg = json.load(open(os.path.join(os.path.dirname(runner.__file__), "configs", "flux1_dev_mi355x.json")))
    cfg["pipeline_args"].update(height=H, width=W, condition_size=cs, num_inference_steps=2)
    cfg["search_args"].update(search_branch=args.branch, search_rounds=1)
    cfg["verifier_args"] = {"name": "clip"}

    def run(handoff, tag):
        cfg["pipeline_args"]["device_handoff"] = handoff
        t0 = time.perf_counter()
        log = runner.run_reflection_search(cfg, ["a red cube left of a blue ball"], os.path.join(tmp, tag), pipe, search.Shard(0, 1),
                                           score_batch=v.score_batch, score_images=v.score_images)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, log

    run(True, "warm_on"), run(False, "warm_off")
    t = {"device_handoff_true": [], "device_handoff_false": []}
    logs = {}
    for r in range(args.search_reps):
        for handoff in ((True, False) if r % 2 == 0 else (False, True)):
            ms, logs[handoff] = run(handoff, f"s{r}_{int(handoff)}")
            t[f"device_handoff_{str(handoff).lower()}"].append(ms)
    n_cand = 2 * args.branch
    res = {"table": "search_pool_plus_one_round", "size": H, "condition_size": cs, "branch": args.branch, "candidates": n_cand,
           "denoise_steps": 2, "transformer": "small synthetic (the boundary dominates; a FLUX.1-dev candidate is ~3 s of denoising)",
           "identical_logs": logs[True] == logs[False], **{k: stats(x) for k, x in t.items()}}
    res["gain_ms_per_candidate"] = round((res["device_handoff_false"]["median_ms"] - res["device_handoff_true"]["median_ms"]) / n_cand, 3)
    print(json.dumps(res), flush=True)
    writer.close()
    snap1 = B.amdsmi_snapshot(0)
    print(json.dumps({"table": "clock_state", "device": torch.cuda.get_device_name(0), "amdsmi": B.amdsmi_delta(snap0, snap1),
                      "start": snap0 and {k: snap0.get(k) for k in ("socket_power_w", "gfx_clk_mhz")}}), flush=True)


if __name__ == "__main__":
    main()

"""Per-tile K-loop and epilogue time of the 256x256 one-tile-per-block bf16 GEMM (gemm_bf16_pp16e_kernel) on cfg2 shapes, from the
kernel's own clock probe: block 0 / wave 0 stamps s_memrealtime at entry, at the end of its K loop and when its epilogue stores
are acknowledged (rf_debug_clock_probe 0 and 2).  One library per process:
    python tools/kb_gemm_epilogue_probe.py [--lib reflectionflow_amd/librf_flux_base.so] [--reps 9]"""
import argparse, ctypes as C, json, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--lib", default=None)
ap.add_argument("--reps", type=int, default=9)
a = ap.parse_args()
from reflectionflow_amd import _lib as L
if a.lib:
    L.LIB_PATH = os.path.abspath(a.lib)
from reflectionflow_amd import ops
lib = L.load()
dev = torch.device("cuda:0"); BF = torch.bfloat16
r = lambda *s, sc=1.0: (torch.randn(*s, device=dev) * sc).to(BF)
S, D, H, MLP = 4608, 3072, 24, 12288
q, k, vt, s_pad = ops.alloc_attn_operands(H, S, dev)
rope = (torch.rand(S, 128, device=dev), torch.rand(S, 128, device=dev))
nq, nk = r(128), r(128)
x, att = r(S, D), r(S, D)
hid, res = torch.empty(S, MLP, device=dev, dtype=BF), r(S, D)
Wq, Wo, Wf = r(3 * D, D, sc=.02), r(D, D, sc=.02), r(3 * D + MLP, D, sc=.02)
shapes = {
    "dbl_qkv": lambda: ops.time_gemm([ops.Group([ops.Seg(x, Wq)], bias=r(3 * D), norm_q=nq, norm_k=nk)], 3 * D, ops.RF_EPI_QKV,
                                     q=q, k=k, vt=vt, heads=H, s_pad=s_pad, rope=rope, schedule=L.RF_SCHED_TILE256, splitk_ws=False),
    "dbl_out": lambda: ops.time_gemm([ops.Group([ops.Seg(att, Wo)], bias=r(D), gate=r(D), out=res, residual=res)], D,
                                     ops.RF_EPI_GATE_RES, schedule=L.RF_SCHED_TILE256, splitk_ws=False),
    "sgl_in": lambda: ops.time_gemm([ops.Group([ops.Seg(x, Wf)], bias=r(3 * D + MLP), out=hid, norm_q=nq, norm_k=nk)], 3 * D + MLP,
                                    ops.RF_EPI_QKV_GELU, n_split=3 * D, q=q, k=k, vt=vt, heads=H, s_pad=s_pad, rope=rope,
                                    schedule=L.RF_SCHED_TILE256, splitk_ws=False),
}
out = {}
for name, fn in shapes.items():
    loop, epi, launch = [], [], []
    for _ in range(a.reps):
        launch.append(fn() * 1e6)
        torch.cuda.synchronize()
        mhz, us = C.c_double(), C.c_double()
        L.check(lib.rf_debug_clock_probe(0, C.byref(mhz), C.byref(us)), "probe")
        loop.append(us.value)
        L.check(lib.rf_debug_clock_probe(2, C.byref(mhz), C.byref(us)), "probe")
        epi.append(us.value)
    med = statistics.median
    out[name] = {"launch_us": round(med(launch), 1), "block0_loop_us": round(med(loop), 2), "block0_epilogue_us": round(med(epi), 2),
                 "epilogue_min_max": [round(min(epi), 2), round(max(epi), 2)]}
print(json.dumps({"lib": os.path.basename(L.LIB_PATH), "probe": out}), flush=True)

"""Poisson image fusion (ops.image_fusion_u8, csrc/image_fusion.hip) on one MI355X: time per call, time per V-cycle, cycles used and peak device memory at a
2048 x 2048 atlas with a full-atlas chart mask and with a single 512 x 512 blob; with --accuracy also d = max |float32 output - float64 oracle| per test
shape and cycle count, from which the contraction per V-cycle is read (tests/support/image_fusion_ref.py holds the oracle and the shapes).

    python tools/bench_image_fusion.py [--accuracy] [--iters N]

The figure to set the times against is the rest of the blended bake at the same atlas (README: 0.33 ms accumulation, 68 ms dilation loop)."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from unitex_amd.texturetools import ops      # noqa: E402


def _time(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def timings(iters):
    from unitex_amd.flux.ops import get_ctx
    lib = get_ctx(torch.cuda.current_device()).lib
    T = 2048
    g = torch.Generator().manual_seed(0)
    src = (torch.rand(T, T, 3, generator=g) * 255).to(torch.uint8).cuda()
    dst = (torch.rand(T, T, 3, generator=g) * 255).to(torch.uint8).cuda()
    yy, xx = torch.meshgrid(torch.arange(T), torch.arange(T), indexing="ij")
    charts = ((((xx // 256) + (yy // 256)) % 2 == 0) | ((xx % 256 > 40) & (yy % 256 > 60))).to(torch.uint8).mul(255)      # charts all over the atlas
    blob = (((xx - 900) ** 2 + (yy - 1100) ** 2) <= 256 ** 2).to(torch.uint8).mul(255)
    for name, mask in (("full-atlas chart mask", charts.cuda()), ("one 512 x 512 blob", blob.cuda())):
        rect = ops.mask_bbox(mask)
        cycles = lib.utx_image_fusion_cycles(rect[2], rect[3])
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        t = _time(lambda: ops.image_fusion_u8(src, dst, mask), iters)
        peak = torch.cuda.max_memory_allocated() - base
        t_lo = _time(lambda: ops.image_fusion_u8(src, dst, mask, cycles=2), iters)
        t_hi = _time(lambda: ops.image_fusion_u8(src, dst, mask, cycles=2 + 4), iters)
        t0 = time.perf_counter()
        ops.mask_bbox(mask)
        torch.cuda.synchronize()
        t_bbox = (time.perf_counter() - t0) * 1e3
        print("2048 x 2048, %-22s rect %-24s cycles %d: %.3f ms per call, %.3f ms per V-cycle, bounding rectangle with its read-back %.3f ms, "
              "peak device memory above the inputs %.1f MiB (workspace %.1f MiB)" %
              (name, rect, cycles, t, (t_hi - t_lo) / 4.0, t_bbox, peak / 2.0 ** 20, lib.utx_image_fusion_workspace_bytes(rect[2], rect[3]) / 2.0 ** 20))


def accuracy():
    from tests.support import image_fusion_ref as R
    cases = dict(R.edge_cases())
    cases["scale_1024_disc_400"] = R.scale_case()
    worst_d, worst_rho = 0.0, 0.0
    for name, case in cases.items():
        ref = R.fuse(case["src"], case["dst"], case["mask"], case["n"])
        if not ref["interior"].any():
            continue
        inside = ref["interior"]
        src, dst, mask = (torch.as_tensor(np.ascontiguousarray(case[k])).cuda() for k in ("src", "dst", "mask"))
        errs = []
        for cycles in range(1, 9):
            out_f = ops.image_fusion_u8(src, dst, mask, n_erode_pix=case["n"], return_float=True, cycles=cycles)[1].cpu().numpy().astype(np.float64)
            errs.append(float(np.abs(out_f - ref["f"])[inside].max()))
        e0 = float(np.abs(ref["f"] - case["dst"])[inside].max())
        d = float(np.abs(ops.image_fusion_u8(src, dst, mask, n_erode_pix=case["n"], return_float=True)[1].cpu().numpy().astype(np.float64) - ref["f"])[inside].max())
        seq = [e0] + errs
        rhos = [seq[k + 1] / seq[k] for k in range(len(seq) - 1) if seq[k + 1] > 20 * min(errs) and seq[k] > 0]      # above the float32 floor only
        rho = max(rhos) if rhos else 0.0
        worst_d, worst_rho = max(worst_d, d), max(worst_rho, rho)
        print("%-28s rect %-22s max|u| %6.1f  d by cycles 1..8: %s | default (%d cycles) d = %.3g, worst contraction %.3f" %
              (name, ref["rect"], e0, " ".join("%.1e" % e for e in errs), R.default_cycles(ref["rect"][2], ref["rect"][3]), d, rho))
    print("recorded: d = %.4g, contraction per V-cycle = %.3f" % (worst_d, worst_rho))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--iters", type=int, default=10)
    a = ap.parse_args()
    print("device:", torch.cuda.get_device_name(0))
    if a.accuracy:
        accuracy()
    timings(a.iters)

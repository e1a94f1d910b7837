"""Sliced optimal-transport colour transfer (color_transfer_ot.CTSOT, csrc/color_transfer.hip) on one MI355X: a 2048^2 x 3 and a 512^2 x 3 image at the defaults
(10 steps x 5 batches, sigma 16 / 5), wall-clock ms per call ending in a device synchronise, median of --reps with the sides interleaved: the whole call, the OT
loop alone, the bilateral filter alone; peak device memory; and the same OT loop in numpy on this machine's host (the restatement of tests/support, one call:
it takes tens of seconds).  The kernels' shares of the call -- rocPRIM's sorts, the other OT kernels, the filter -- come from a run of their own under
rocprofv3 --kernel-trace --stats (a fresh child process running --child once), grouped by kernel name.
    python tools/bench_color_transfer.py --log profiles/color_transfer_bench.log"""
import argparse
import csv
import glob
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.bench_uv_bake import _wall, interleaved, peak_mib  # noqa: E402
from unitex_amd.texturetools import color_transfer_ot as CT, ops  # noqa: E402

STEPS, BATCH, SIGMA_XY, SIGMA_V = 10, 5, 16.0, 5.0


def scene(side, dev):
    """two smooth images with different colour statistics plus noise, float32 in [0, 1], and the directions of a seeded numpy generator"""
    rng = np.random.default_rng(side)
    y, x = np.mgrid[0:side, 0:side].astype(np.float32) / np.float32(side)
    src = np.stack([0.5 + 0.4 * np.sin(7 * x + 3 * y), 0.5 + 0.4 * np.cos(5 * y), x * y], -1) + rng.uniform(-0.05, 0.05, (side, side, 3))
    dst = np.stack([0.3 + 0.2 * np.cos(4 * x), 0.6 + 0.3 * np.sin(6 * x * y), 0.2 + 0.5 * y], -1) + rng.uniform(-0.05, 0.05, (side, side, 3))
    np.random.seed(side)
    dirs = CT.draw_directions(STEPS, BATCH, 3)
    return src.astype(np.float32), dst.astype(np.float32), dirs


def child(side):
    """what the profiled run executes: one warm call, one call"""
    dev = torch.device("cuda:0")
    src, dst, dirs = scene(side, dev)
    s, d, dd = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev), torch.from_numpy(dirs).to(dev)
    for _ in range(2):
        CT.CTSOT(s, d, STEPS, BATCH, SIGMA_XY, SIGMA_V, dirs=dd)
    torch.cuda.synchronize()


def kernel_shares(side, timeout):
    """{group: (ms per call, launches per call)} from rocprofv3's kernel statistics of a child that makes two calls, or a string saying why there is none"""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return "rocprofv3 not found"
    out = tempfile.mkdtemp(prefix="ct_prof_")
    try:
        r = subprocess.run([exe, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__), "--child",
                            str(side)], capture_output=True, text=True, timeout=timeout)
        if r.returncode != 0:
            return "rocprofv3 exited with %d: %s" % (r.returncode, r.stderr[-300:].replace("\n", " "))
        files = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return "no kernel_stats.csv written"
        groups = {}
        for row in csv.DictReader(open(files[0])):
            name, calls, total = row.get("Name", ""), int(row.get("Calls", 0)), float(row.get("TotalDurationNs", 0.0))
            g = ("bilateral filter" if "bilateral_kernel" in name else "OT project / advect / update" if "ct_" in name
                 else "rocPRIM sorts" if ("rocprim" in name or "sort" in name) else "other (copies, elementwise)")
            ms, n = groups.get(g, (0.0, 0))
            groups[g] = (ms + total / 2e6, n + calls / 2.0)      # two calls in the child
        return groups
    except subprocess.TimeoutExpired:
        return "rocprofv3 run exceeded %d s" % timeout
    finally:
        shutil.rmtree(out, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sides", type=int, nargs="+", default=[2048, 512])
    ap.add_argument("--no-host", action="store_true", help="leave the numpy loop out")
    ap.add_argument("--no-profile", action="store_true", help="leave the rocprofv3 child out")
    ap.add_argument("--profile-timeout", type=int, default=300)
    ap.add_argument("--child", type=int, default=0, help=argparse.SUPPRESS)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    assert args.reps >= 20, "median of at least 20"
    assert torch.cuda.is_available(), "needs cuda:0"
    sys.path.insert(0, ROOT)
    from tests.support import color_transfer_ref as R
    dev = torch.device("cuda:0")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
    say("CTSOT, %s, %d steps x %d batches, reg_sigmaXY %g (r = %d), reg_sigmaV %g, 3 channels; wall-clock ms per call, median of %d, sides interleaved"
        % (torch.cuda.get_device_name(0), STEPS, BATCH, SIGMA_XY, ops.bilateral_radius(SIGMA_XY), SIGMA_V, args.reps))
    for side in args.sides:
        src, dst, dirs = scene(side, dev)
        s, d, dd = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev), torch.from_numpy(dirs).to(dev)
        new = ops.color_transfer_ot(s, d, dd, STEPS, BATCH)
        disp = (new - s).contiguous()
        sides = [("CTSOT (loop + filter)", lambda: CT.CTSOT(s, d, STEPS, BATCH, SIGMA_XY, SIGMA_V, dirs=dd)),
                 ("ops.color_transfer_ot (%d sorts of %d keys)" % (2 * STEPS * BATCH, side * side), lambda: ops.color_transfer_ot(s, d, dd, STEPS, BATCH)),
                 ("ops.bilateral_filter", lambda: ops.bilateral_filter(disp, SIGMA_V, SIGMA_XY))]
        t = interleaved(sides, _wall, args.reps, args.warmup)
        say("-- %d x %d x 3" % (side, side))
        for name, fn in sides:
            say("   %-52s %10.3f ms   peak %7.1f MiB" % (name, t[name], peak_mib(fn)))
        say("   workspace of the loop: %.1f MiB" % (ops.get_ctx(0).lib.utx_color_transfer_ot_workspace_bytes(side * side, 3) / 2.0 ** 20))
        if not args.no_profile:
            g = kernel_shares(side, args.profile_timeout)
            if isinstance(g, str):
                say("   kernel shares: not measured (%s)" % g)
            else:
                total = sum(ms for ms, _ in g.values())
                for k in sorted(g, key=lambda k: -g[k][0]):
                    say("   kernel time, %-32s %10.3f ms  %5.1f %%  %6.0f launches" % (k, g[k][0], 100.0 * g[k][0] / total, g[k][1]))
                say("   kernel time, sum %39.3f ms (rocprofv3 --kernel-trace --stats, a run of its own)" % total)
        if not args.no_host:
            t0 = time.perf_counter()
            host = R.ot_loop(src, dst, dirs, STEPS, BATCH)
            th = time.perf_counter() - t0
            same = host.tobytes() == new.cpu().numpy().tobytes()
            say("   the same loop in numpy on this host (one call, no filter): %.2f s = %.0f x the device loop; results bit-equal: %s"
                % (th, 1e3 * th / t[sides[1][0]], same))
    if args.log:
        os.makedirs(os.path.dirname(os.path.abspath(args.log)), exist_ok=True)
        with open(args.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

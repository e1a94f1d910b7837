#!/usr/bin/env python
"""Farthest-point sampling: utx_fps against the same loop written in torch-ROCm ops, on the same card, timed with HIP events.

usage: python tools/bench_sampling.py [--points 200000 4194304] [--picks 32768] [--rounds 3] [--out FILE.json]

The two sizes are the two uses of the reference: thinning the 200 000 surface / edge samples of sampling_on_mesh to 32 768 (pipeline.py:387-407) and
thinning the texels of a 2048^2 atlas (2^22 points, pipeline.py:507-514).  The parent of this code has no farthest-point sampling, so the baseline is what a
user would write with torch: per pick one distance computation, one minimum update and one arg-max, no host synchronisation in the loop.  Both arms run on
uniform random points in [-1, 1]^3 from one seed, are warmed up at their full size first, alternate within one process, and are checked to pick the same
indices over the first picks where float32 summation order cannot matter (the torch distance sums x, y, z in its own order).  One JSON line per size."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from unitex_amd.texturetools import ops  # noqa: E402


def torch_fps(pos, M, out):
    mind = torch.full((pos.shape[0],), float("inf"), device=pos.device)
    far = torch.zeros((), dtype=torch.int64, device=pos.device)
    for k in range(M):
        out[k] = far
        d = (pos - pos[far]).square_().sum(1)      # distance to the pick
        torch.minimum(mind, d, out=mind)           # min update
        far = mind.argmax()                        # arg-max
    return out


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    r = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, nargs="+", default=[200000, 1 << 22])
    ap.add_argument("--picks", type=int, default=32768)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sampling needs the GPU: a time taken anywhere else says nothing about it")
    lines = []
    for N in a.points:
        g = torch.Generator(device="cuda").manual_seed(14)
        pos = (torch.rand(N, 3, device="cuda", generator=g) * 2 - 1).contiguous()
        M = a.picks
        ref = torch.empty(M, dtype=torch.int64, device="cuda")
        hip_ms, torch_ms = [], []
        ops.fps(pos, M)
        torch_fps(pos, M, ref)          # warm-up at full size
        torch.cuda.synchronize()
        for _ in range(a.rounds):
            t, idx = timed(lambda: ops.fps(pos, M))
            hip_ms.append(t)
            t, _ = timed(lambda: torch_fps(pos, M, ref))
            torch_ms.append(t)
        same = int((idx.long() == ref).long().cumprod(0).sum().item())       # length of the common prefix of picks
        hip_ms.sort()
        torch_ms.sort()
        r = dict(points=N, picks=M, rounds=a.rounds, hip_ms_median=hip_ms[len(hip_ms) // 2], hip_ms_min=hip_ms[0], torch_ms_median=torch_ms[len(torch_ms) // 2],
                 torch_ms_min=torch_ms[0], speedup_median=torch_ms[len(torch_ms) // 2] / hip_ms[len(hip_ms) // 2], us_per_pick_hip=1e3 * hip_ms[len(hip_ms) // 2] / M,
                 us_per_pick_torch=1e3 * torch_ms[len(torch_ms) // 2] / M, common_prefix_of_picks=same,
                 # bytes one pick has to move at least: positions + mind read (mind is written back only where it shrinks)
                 gbps_algorithmic_hip=N * 16 * M / (hip_ms[len(hip_ms) // 2] * 1e-3) / 1e9)
        print(json.dumps(r), flush=True)
        lines.append(r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(lines, f, indent=1)


if __name__ == "__main__":
    main()

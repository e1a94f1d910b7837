#!/usr/bin/env python
"""Generate the geometry-sampling fixture under tests/golden/ from the REFERENCE's own Python, through the stub machinery of make_golden.py
(imported from there, unchanged):

    python tests/golden/make_golden_sampling.py            # writes tests/golden/g14_geometry_sampling.npz

  G14   select_sharp_edges and sample_on_edges_v2 (TextureTools/texturetools/geometry/sampling/edge_sampling.py:6-46, 84-119) on two meshes.
Seam: sample_on_edges_v2 hard-wires device='cuda' into torch.linspace.  For the duration of the call torch.linspace(..., device='cuda') is
replaced by the formula of torch's CUDA kernel [3p] (RangeFactories.cu: step = (end - start) / (steps - 1); index i below steps / 2 gives
start + step * i, the others end - step * (steps - 1 - i)), evaluated in float32 with every product and sum rounded on its own.  torch's
CPU linspace is NOT that formula (its vector path adds the lane offset to a rounded base) and differs from it in a few per cent of the
elements.  Everything else the two functions execute is the reference's own code on CPU tensors.

Meshes:
  * 'stair': a three-step staircase profile extruded along z, every vertex on a multiple of 1/64.  The z = lo end is capped (six coplanar
    triangles), the z = hi end is OPEN (eight boundary edges: non-manifold), the bottom is one coplanar quad cut into a four-triangle fan
    around its centre (interior edges must come out not sharp), the side quads are cut by one diagonal each (not sharp).  Every SELECTED
    edge is axis-aligned with a dyadic length (1/4, 1/2, 3/4), so every prefix sum of the selected lengths is exact in float32 in any
    order and the captured samples do not depend on the summation order of cumsum.  Captured with N = 1000 at 15 degrees.
  * 'torus': the flattened torus of make_golden_video_types.py (closed, smooth) from the same function at 96 x 48 segments: at G13's own 28 x 14 the
    facets meet at up to 26 degrees and 448 edges are sharp at 15; at 96 x 48 no edge is sharp at 15 degrees and 4560 of 13824 are at 5.  Masks for both
    thresholds; no samples (their prefix rounding is order-dependent -- the GPU test checks them against float64 geometry instead).
Stored: the meshes, edges_unique, both masks per threshold, and for the staircase samples / edge_index / edge_t."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import REF, install_stubs  # noqa: E402
from make_golden_video_types import _torus  # noqa: E402

N_STAIR = 1000
TORUS_SEGMENTS = dict(nu=96, nv=48)


def _staircase():
    s = 1.0 / 64.0
    prof = np.array([(0, 0), (0, 16), (16, 16), (16, 32), (32, 32), (32, 48), (48, 48), (48, 0)], np.float64)      # clockwise seen from +z, in 1/64
    n = len(prof)
    z0, z1 = -16.0, 16.0
    verts = [(x - 24, y - 24, z0) for x, y in prof] + [(x - 24, y - 24, z1) for x, y in prof] + [(0.0, -24.0, 0.0)]      # A_i, B_i, centre of the bottom quad
    A, B, C = (lambda i: i % n), (lambda i: n + i % n), 2 * n
    faces = [(A(0), A(1), A(2)), (A(0), A(2), A(7)), (A(2), A(3), A(4)), (A(2), A(4), A(7)), (A(4), A(5), A(6)), (A(4), A(6), A(7))]      # the z = z0 cap
    for i in range(n - 1):                                       # side quads over the profile edges P_i P_i+1, one diagonal each
        faces += [(A(i), A(i + 1), B(i + 1)), (A(i), B(i + 1), B(i))]
    faces += [(A(7), A(0), C), (A(0), B(0), C), (B(0), B(7), C), (B(7), A(7), C)]      # the bottom quad P_7 P_0 as a fan around its centre
    return (np.asarray(verts, np.float64) * s).astype(np.float32), np.asarray(faces, np.int32)


class _linspace_cuda_formula:
    def __enter__(self):
        self.orig = torch.linspace

        def linspace(start, end, steps, **kw):
            if str(kw.get("device", "cpu")).startswith("cuda"):
                assert kw.get("dtype") == torch.float32
                a, b = torch.tensor(start, dtype=torch.float32), torch.tensor(end, dtype=torch.float32)
                if steps == 1:
                    return a.reshape(1)
                step = (b - a) / torch.tensor(float(steps - 1), dtype=torch.float32)
                i = torch.arange(steps)
                return torch.where(i < steps // 2, a + step * i.float(), b - step * (steps - 1 - i).float())
            return self.orig(start, end, steps, **kw)
        torch.linspace = linspace
        return self

    def __exit__(self, *a):
        torch.linspace = self.orig


def g14_geometry_sampling(out):
    es = importlib.import_module("TextureTools.texturetools.geometry.sampling.edge_sampling")
    fix = {}
    sv, sf = _staircase()
    tv, tf = _torus(**TORUS_SEGMENTS)[:2]
    fix.update(stair_verts=sv, stair_faces=sf, torus_verts=tv, torus_faces=tf)
    for name, v, f in (("stair", sv, sf), ("torus", tv, tf)):
        vt, ft = torch.from_numpy(v), torch.from_numpy(f).long()
        for deg in (15, 5):
            edges, nonman, sharp = es.select_sharp_edges(vt, ft, None, angle_threhold_deg=float(deg))
            if name + "_edges" in fix:
                assert np.array_equal(fix[name + "_edges"], edges.numpy())
            fix[name + "_edges"] = edges.numpy().astype(np.int32)
            fix["%s_nonmanifold_%d" % (name, deg)] = nonman.numpy()
            fix["%s_sharp_%d" % (name, deg)] = sharp.numpy()
            print("G14 %s at %d deg: %d edges, %d non-manifold, %d sharp" % (name, deg, len(edges), int(nonman.sum()), int(sharp.sum())))
    assert fix["stair_nonmanifold_15"].sum() == 8 and fix["stair_sharp_15"].sum() == 16
    assert fix["torus_sharp_15"].sum() == 0 and fix["torus_sharp_5"].sum() > 0 and fix["torus_nonmanifold_15"].sum() == 0
    # the staircase's selected edges: axis-aligned, dyadic lengths
    sel = fix["stair_edges"][fix["stair_nonmanifold_15"] | fix["stair_sharp_15"]]
    d = sv[sel[:, 1]] - sv[sel[:, 0]]
    assert np.all((d != 0).sum(1) == 1) and set(np.abs(d).max(1).tolist()) <= {0.25, 0.5, 0.75}
    vt, ft = torch.from_numpy(sv), torch.from_numpy(sf).long()
    with _linspace_cuda_formula():
        samples, edge_index, edge_t = es.select_and_sample_on_edges(vt, ft, normals=None, method="equal_steps", angle_threhold_deg=15.0, N=N_STAIR, seed=666)
    assert samples.shape == (N_STAIR, 3) and edge_t.shape == (N_STAIR, 1) and samples.dtype == torch.float32
    fix.update(stair_samples=samples.numpy(), stair_edge_index=edge_index.numpy().astype(np.int32), stair_edge_t=edge_t.numpy()[:, 0])
    path = os.path.join(out, "g14_geometry_sampling.npz")
    np.savez_compressed(path, **fix)
    print("G14: %d arrays, %d bytes" % (len(fix), os.path.getsize(path)))


def main(out=HERE):
    sys.path.insert(0, REF)
    install_stubs()
    torch.set_num_threads(4)
    g14_geometry_sampling(out)
    print("wrote g14_geometry_sampling")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)

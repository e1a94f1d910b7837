#!/usr/bin/env python
"""Generate the ray-casting fixture under tests/golden/ from the REFERENCE's own Python:

    python tests/golden/make_golden_raytracing.py [path to the reference checkout]      # writes tests/golden/g24_raytracing.npz

  G24   self_rt, cross_rt (exhaustive and paired) and sphere_rt of TextureTools/texturetools/raytracing/check_visibility.py, run on the CPU.
Seams: the module is loaded by itself under a stand-in parent package (its `from . import RayTracing` finds a placeholder; the real package imports Slang);
its hard-coded device='cuda' is redirected to the CPU by handing the module a `torch` whose factory functions map that device; `bvh` is a STUB whose
intersects_closest is NOT a ray tracer of the reference but a seam written here, as G19's RaycastingScene was: the float64 brute force of
tests/support/raycast_ref.py (every ray against every triangle, both sides, the smallest t >= 0, ties to the lowest id), which returns loc = +inf on a miss.  The stub
records the directions it is handed: the HIP side replays them (dirs=), since torch.randn + normalize cannot be restated to the bit.
Stored: the meshes, the points, the recorded directions, the masks and ids the reference's functions return, and the margin flags of tests/support/raycast_ref.py for
every point / segment / ray (False: a float32 walk may legitimately decide it differently).  float32 / int32 / bool, data only."""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests.support import raycast_ref as RC  # noqa: E402

sys.path.insert(0, HERE)
from make_golden import REF as _REF  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else _REF


class _CpuTorch:
    """the torch module with device='cuda' read as the CPU"""

    def __getattr__(self, name):
        obj = getattr(torch, name)
        if name in ("zeros", "arange", "randn", "as_tensor", "Generator"):
            def wrapped(*a, **k):
                if k.get("device") == "cuda":
                    k["device"] = "cpu"
                return obj(*a, **k)
            return wrapped
        return obj


def load_check_visibility():
    pkg = types.ModuleType("utx_ref_raytracing")
    pkg.__path__ = []
    pkg.RayTracing = object
    sys.modules["utx_ref_raytracing"] = pkg
    path = os.path.join(REF, "TextureTools", "texturetools", "raytracing", "check_visibility.py")
    spec = importlib.util.spec_from_file_location("utx_ref_raytracing.check_visibility", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.torch = _CpuTorch()
    mod.tqdm = lambda it: it
    return mod


class StubBVH:
    def __init__(self, verts, faces):
        self.verts, self.faces, self.calls = verts, faces, []

    def intersects_closest(self, rays_o, rays_d, stream_compaction=False):
        o, d = rays_o.numpy().astype(np.float32), rays_d.numpy().astype(np.float32)
        self.calls.append((o.copy(), d.copy()))
        r = RC.brute_closest(self.verts, self.faces, o, d)
        hit = r["tid"] >= 0
        loc = np.where(hit[:, None], o.astype(np.float64) + r["t"][:, None] * d.astype(np.float64), np.inf).astype(np.float32)
        uv = np.stack([r["u"], r["v"]], -1).astype(np.float32)
        return torch.from_numpy(hit), torch.from_numpy(r["front"]), torch.from_numpy(r["tid"]), torch.from_numpy(loc), torch.from_numpy(uv)


def main():
    cv = load_check_visibility()
    out = {}
    rng = np.random.default_rng(24)
    for name in ("nested", "open"):
        v, f = RC.mesh(name)
        out["%s_verts" % name], out["%s_faces" % name] = v, f

    # self_rt: nested shells (points inside the inner shell, between the shells, outside) and the open sphere (points under the hole, deep inside, outside)
    n_rays = 16
    for name in ("nested", "open"):
        v, f = RC.mesh(name)
        N = 96
        p = rng.standard_normal((N, 3))
        p /= np.linalg.norm(p, axis=1, keepdims=True)
        k = np.arange(N) % 3
        r = np.where(k == 0, rng.uniform(0.02, 0.3, N), np.where(k == 1, rng.uniform(0.5, 0.75, N), rng.uniform(1.5, 2.5, N)))
        p = (p * r[:, None]).astype(np.float32)
        if name == "open":
            p[:8] = np.array([0.0, 0.0, 0.9], np.float32) + rng.uniform(-0.05, 0.05, (8, 3)).astype(np.float32)      # just under the hole
        bvh = StubBVH(v, f)
        mask = cv.self_rt(bvh, torch.from_numpy(p), n_rays=n_rays, chunk_size=40, seed=666).numpy()
        dirs = np.concatenate([d for _, d in bvh.calls]).reshape(N, n_rays, 3)
        inner, ok, _ = RC.brute_enclosed(v, f, p, dirs)
        assert (inner == mask).all()
        out.update({"self_%s_points" % name: p, "self_%s_dirs" % name: dirs, "self_%s_mask" % name: mask, "self_%s_ok" % name: ok})
        print("self_rt %s: %d of %d inner, %d margin-failing" % (name, mask.sum(), N, (~ok).sum()))

    # cross_rt is run with ONE chunk (chunk_size >= M): with more, the reference drops decided points from `points` but not from `outer_points` and its next
    # broadcast_tensors raises as soon as a point was dropped.  The masks do not depend on the chunking; the HIP side is tested with smaller chunks against them.
    # cross_rt on the nested shells: points inside the inner shell are hidden from every outer point, points between the shells and outside are not all hidden
    v, f = RC.mesh("nested")
    N, M = 60, 10
    p = rng.standard_normal((N, 3))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    p = (p * np.where(np.arange(N) % 2 == 0, rng.uniform(0.05, 0.3, N), rng.uniform(1.1, 1.6, N))[:, None]).astype(np.float32)
    outer = rng.standard_normal((M, 3))
    outer = (outer / np.linalg.norm(outer, axis=1, keepdims=True) * rng.uniform(2.0, 3.0, (M, 1))).astype(np.float32)
    bvh = StubBVH(v, f)
    mask = cv.cross_rt(bvh, torch.from_numpy(p), torch.from_numpy(outer), chunk_size=M, exhaustive_mode=True).numpy()
    a, b = np.repeat(outer[None], N, 0).reshape(-1, 3), np.repeat(p[:, None], M, 1).reshape(-1, 3)
    blocked, ok = RC.brute_any(v, f, a, b)
    assert (blocked.reshape(N, M).all(1) == mask).all(), "t < 1 on the segment and the reference's distance test disagree on this input"
    out.update(cross_points=p, cross_outer=outer, cross_mask=mask, cross_ok=ok.reshape(N, M).all(1))
    print("cross_rt exhaustive: %d of %d kept, %d margin-failing points" % (mask.sum(), N, (~out["cross_ok"]).sum()))
    pp = np.repeat(p[:, None], 6, 1).reshape(5, 12, 6, 3).copy()                                   # paired mode with a batch shape [5, 12]
    oo = (pp * 0 + rng.standard_normal((5, 12, 6, 3))).astype(np.float32)
    oo = (oo / np.linalg.norm(oo, axis=-1, keepdims=True) * rng.uniform(2.0, 3.0, (5, 12, 6, 1))).astype(np.float32)
    bvh = StubBVH(v, f)
    mask2 = cv.cross_rt(bvh, torch.from_numpy(pp), torch.from_numpy(oo), chunk_size=6, exhaustive_mode=False).numpy()
    blocked, ok = RC.brute_any(v, f, oo.reshape(-1, 3), pp.reshape(-1, 3))
    assert (blocked.reshape(5, 12, 6).all(-1) == mask2).all()
    out.update(pair_points=pp, pair_outer=oo, pair_mask=mask2, pair_ok=ok.reshape(5, 12, 6).all(-1))
    print("cross_rt paired: %d of %d kept, %d margin-failing points" % (mask2.sum(), mask2.size, (~out["pair_ok"]).sum()))

    # sphere_rt on the nested shells: only faces of the outer shell can be hit
    bvh = StubBVH(v, f)
    ids = cv.sphere_rt(bvh, n_rays=500, sample_offset=0.1).numpy()
    o, d = bvh.calls[0]
    r = RC.brute_closest(v, f, o, d)
    assert (ids < len(f) // 2).all() and len(ids) > 0
    out.update(sphere_dirs=(-d).astype(np.float32), sphere_origins=o, sphere_ids=ids.astype(np.int32), sphere_tid=r["tid"].astype(np.int32), sphere_ok=r["ok"],
               sphere_offset=np.float32(0.1))
    print("sphere_rt: %d hits on %d faces, %d margin-failing rays" % (len(ids), len(set(ids.tolist())), (~r["ok"]).sum()))
    # the axis rays of sphere_rt_nvdiffrast on the open sphere
    v, f = RC.mesh("open")
    ax, ang = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0), 0.3      # tilted (Rodrigues): an icosphere has vertices ON the axes, where no margin holds
    K = np.array([[0, -ax[2], ax[1]], [ax[2], 0, -ax[0]], [-ax[1], ax[0], 0]])
    v = (v.astype(np.float64) @ (np.eye(3) + np.sin(ang) * K + (1 - np.cos(ang)) * K @ K).T).astype(np.float32)
    out["axis_verts"], out["axis_faces"] = v, f
    for n in (4, 6):
        bvh = StubBVH(v, f)
        ids = cv.sphere_rt_nvdiffrast(bvh, n_cameras=n).numpy()
        r = RC.brute_closest(v, f, *bvh.calls[0])
        assert r["ok"].all() and len(ids) == n
        out["axis%d_ids" % n] = ids.astype(np.int32)
        print("sphere_rt_nvdiffrast %d: ids %s, ok %s" % (n, ids.tolist(), r["ok"].tolist()))
    path = os.path.join(HERE, "g24_raytracing.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()

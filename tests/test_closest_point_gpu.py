"""GPU tests of utx_bvh_closest_point (csrc/bvh_device.h, csrc/bvh.hip) through the C ABI: the tree walk, the exhaustive twin (flags & 1) and the numpy
restatement of oracle/closest_point_ref.py (pinned on the CPU in tests/test_closest_point_cpu.py) agree BIT FOR BIT; all three are bounded against a float64 brute
force by another formula with the bound that module's docstring counts."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from oracle import closest_point_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32
COUNTS = [1, 63, 64, 65, 257]


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _bvh(name):
    from unitex_amd.texturetools import ops
    v, f = R.mesh(name)
    return ops.BVH(torch.from_numpy(v).cuda().contiguous(), torch.from_numpy(f).cuda().contiguous())


@functools.lru_cache(maxsize=None)
def _reference(name, N):
    """(points, restatement, float64 distances), computed once and shared; never written to"""
    v, f = R.mesh(name)
    pts = R.queries(name, N)
    return pts, R.closest_point_f32(pts, v, f), R.brute_f64(pts, v, f)


@pytest.mark.parametrize("N", COUNTS)
@pytest.mark.parametrize("name", R.MESHES)
def test_walk_equals_exhaustive_equals_restatement_and_is_within_the_counted_bound(name, N):
    from unitex_amd.texturetools import ops
    v, f = R.mesh(name)
    pts, (dist, d2, face, uvw, q), d64 = _reference(name, N)
    p = torch.from_numpy(pts).cuda()
    got = {}
    for key, kw in (("walk", {}), ("brute", {"brute": True}), ("noseed", {"seed_descent": False})):
        o = ops.closest_point(_bvh(name), p, **kw)
        got[key] = {k: t.cpu().numpy() for k, t in o.items()}
    fin = np.isfinite(pts).all(1)
    for key, g in got.items():
        assert (_bits(g["dist"]) == _bits(dist)).all(), key          # the root of the restatement's d2; sqrtf is many-to-one, so this alone does not pin d2
        assert (g["face"] == face).all(), key
        assert (_bits(g["uvw"]) == _bits(uvw)).all() and (_bits(g["closest"]) == _bits(q)).all(), key
        # d2 itself, bit for bit, for each of the three: the kernel forms it as |p - closest|^2 summed like dot3, and the same sum from the RETURNED closest
        # point is the restatement's d2
        with np.errstate(all="ignore"):
            r = pts - g["closest"]
            assert (_bits(((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2])[fin]) == _bits(d2[fin])).all(), key
    g = got["walk"]
    # the face is the smallest id attaining the minimum of the per-triangle function
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    all_d2 = R.tri_closest_f32(pts[fin][:, None, :], a[None], b[None], c[None])[0]
    assert (g["face"][fin] == np.argmax(all_d2 == all_d2.min(1, keepdims=True), axis=1)).all()
    assert (g["face"][~fin] == -1).all() and np.isposinf(g["dist"][~fin]).all() and (g["uvw"][~fin] == 0).all() and (g["closest"][~fin] == 0).all()
    # bounds against float64: no query excluded
    tol = R.BOUND_U * R.U * R.scene_scale(pts, v)
    p64, v64 = pts[fin].astype(np.float64), v.astype(np.float64)
    err = np.abs(g["dist"][fin].astype(np.float64) - d64[fin]).max()
    err_face = np.abs(R.face_dist_f64(pts[fin], v, f, g["face"][fin]) - d64[fin]).max()
    w64 = g["uvw"][fin].astype(np.float64)
    err_q = np.abs(np.linalg.norm(p64 - (w64[:, :, None] * v64[f[g["face"][fin]]]).sum(1), axis=1) - d64[fin]).max()
    unit = tol / R.BOUND_U
    print("%s N=%d: multiples of u * scale: dist %.2f, returned face %.2f, sum uvw v %.2f (bound %g)" % (name, N, err / unit, err_face / unit, err_q / unit, R.BOUND_U))
    assert err <= tol and err_face <= tol and err_q <= tol
    assert (g["uvw"] >= 0).all() and np.abs(w64.sum(1) - 1.0).max() <= 4 * R.U


def test_exact_ties_among_up_to_six_faces_go_to_the_smallest_id():
    from unitex_amd.texturetools import ops
    v, f = R.mesh("grid")
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    pts = np.concatenate([v, (v[e[:, 0]] + v[e[:, 1]]) * F32(0.5)])
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    all_d2 = R.tri_closest_f32(pts[:, None, :], a[None], b[None], c[None])[0]
    tie = all_d2 == all_d2.min(1, keepdims=True)
    assert tie.sum(1).max() == 6 and (all_d2.min(1) == 0).all()
    for kw in ({}, {"brute": True}, {"seed_descent": False}):
        o = ops.closest_point(_bvh("grid"), torch.from_numpy(pts).cuda(), **kw)
        assert (o["face"].cpu().numpy() == np.argmax(tie, axis=1)).all() and (o["dist"].cpu().numpy() == 0).all()
        assert (o["closest"].cpu().numpy() == pts).all()


def test_the_walk_prunes():
    """nodes visited per query on the 80-face icosphere, for points near the surface: below the 2F - 1 of a walk that skips nothing, with and without the seed"""
    from unitex_amd.texturetools import ops
    v, f = R.mesh("ico")
    rng = np.random.default_rng(5)
    bw = rng.dirichlet(np.ones(3), 256).astype(F32)
    fi = rng.integers(0, len(f), 256)
    pts = ((bw[:, 0:1] * v[f[fi, 0]] + bw[:, 1:2] * v[f[fi, 1]]) + bw[:, 2:3] * v[f[fi, 2]]) * F32(1.01)
    p = torch.from_numpy(pts.astype(F32)).cuda()
    full = 2 * len(f) - 1
    o, n_seed = ops.closest_point(_bvh("ico"), p, count=True)
    o2, n_plain = ops.closest_point(_bvh("ico"), p, count=True, seed_descent=False)
    o3, n_brute = ops.closest_point(_bvh("ico"), p, count=True, brute=True)
    print("nodes per query: %.1f with the greedy seed, %.1f without, %d in the whole tree" % (n_seed / 256, n_plain / 256, full))
    assert n_brute == 0 and 0 < n_seed / 256 < full and 0 < n_plain / 256 < full
    for k in o:
        assert torch.equal(o[k], o2[k]) and torch.equal(o[k], o3[k])


def test_optional_outputs_empty_input_and_error_codes():
    from unitex_amd.texturetools import ops
    bvh = _bvh("tetra")
    ctx, lib = bvh.ctx, bvh.ctx.lib
    p = torch.from_numpy(R.queries("tetra", 65)).cuda()
    full = ops.closest_point(bvh, p)
    only = ops.closest_point(bvh, p, want=("dist",))
    assert list(only) == ["dist"] and torch.equal(only["dist"], full["dist"])
    empty = ops.closest_point(bvh, p[:0])
    assert empty["dist"].shape == (0,) and empty["uvw"].shape == (0, 3)
    with pytest.raises(ValueError):
        ops.closest_point(bvh, p.reshape(-1))
    with pytest.raises(ValueError):
        ops.closest_point(bvh, p, want=("dist", "normal"))
    d = torch.empty(65, dtype=torch.float32, device="cuda")
    pp, dp, z = C.c_void_p(p.data_ptr()), C.c_void_p(d.data_ptr()), C.c_void_p(0)
    call = lambda h, pts, n, dist, flags: lib.utx_bvh_closest_point(ctx.handle, h, pts, n, dist, z, z, z, z, flags, ctx.stream())
    assert call(bvh.handle, pp, 0, dp, 0) == 0 and call(bvh.handle, z, 0, z, 0) == 0          # N = 0 returns at once
    assert call(bvh.handle, pp, -1, dp, 0) == -2 and call(bvh.handle, pp, 2 ** 31, dp, 0) == -2
    assert call(z, pp, 65, dp, 0) == -2 and call(bvh.handle, z, 65, dp, 0) == -2 and call(bvh.handle, pp, 65, z, 0) == -2
    assert call(bvh.handle, pp, 65, dp, 4) == -2
    assert call(bvh.handle, pp, 65, dp, 0) == 0
    torch.cuda.synchronize()
    assert torch.equal(d, full["dist"])

"""GPU tests of the ray queries (csrc/raycast.hip) through the C ABI and of texturetools/raytracing.py: closest hit against the float64 brute force on the
margin-passing rays and BIT FOR BIT against the float32 restatement at the returned face; occlusion and enclosed points against their brute-force rules; the
direction stream bit for bit; the public functions against fixture G24 (the reference's check_visibility.py).  Inputs, margins and the exclusion cap are
tests/support/raycast_ref.py's; tests/test_raytracing_cpu.py asserts the cap for every input used here.  Both walks (packed, forced stack) run everywhere."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests.support import raycast_ref as RC

pytestmark = pytest.mark.gpu
F32 = np.float32
WALKS = [False, True]      # force_stack


def _cu(a):
    return torch.from_numpy(np.array(a, copy=True, order="C")).cuda()


@functools.lru_cache(maxsize=None)
def _bvh(name):
    from unitex_amd.texturetools import ops
    v, f = RC.mesh(name)
    return ops.BVH(_cu(v), _cu(f))


def _np(d):
    return {k: x.cpu().numpy() for k, x in d.items()}


def _check_intersect(name, o, d, ref, got):
    v, f = RC.mesh(name)
    ok = ref["ok"]
    assert (got["tid"][ok] == ref["tid"][ok]).all(), "%d margin-passing rays name another face" % (got["tid"][ok] != ref["tid"][ok]).sum()
    r = RC.tri_f32(v, f, o, d, got["tid"])
    assert (r["hit"] == (got["tid"] >= 0)).all()
    for k in ("t", "uv", "loc", "front"):
        assert got[k].tobytes() == r[k].tobytes(), k
    miss = got["tid"] < 0
    assert np.isposinf(got["t"][miss]).all() and not got["loc"][miss].any() and not got["uv"][miss].any() and not got["front"][miss].any()


@pytest.mark.parametrize("force_stack", WALKS)
@pytest.mark.parametrize("name,R", RC.INTERSECT_INPUTS)
def test_intersect_against_brute_force_and_restatement(name, R, force_stack):
    o, d, ref = RC.intersect_case(name, R)
    got = _np(_bvh(name).intersect(_cu(o), _cu(d), force_stack=force_stack))
    assert got["tid"].shape == (R,) and got["loc"].shape == (R, 3) and got["uv"].shape == (R, 2) and got["front"].dtype == np.uint8
    _check_intersect(name, o, d, ref, got)


@pytest.mark.parametrize("force_stack", WALKS)
def test_every_subset_of_outputs_gives_the_same_values(force_stack):
    from unitex_amd.texturetools import ops
    o, d, _ = RC.intersect_case("nested", 257)
    bvh = _bvh("nested")
    full = _np(bvh.intersect(_cu(o), _cu(d), force_stack=force_stack))
    keys = ops.INTERSECT_OUTPUTS
    for m in range(1 << len(keys)):
        want = tuple(k for i, k in enumerate(keys) if m >> i & 1)
        got = _np(bvh.intersect(_cu(o), _cu(d), want=want, force_stack=force_stack))
        assert tuple(got) == want
        for k in want:
            assert got[k].tobytes() == full[k].tobytes(), (want, k)
    mask = torch.zeros(len(RC.mesh("nested")[1]), dtype=torch.uint8, device="cuda")
    if force_stack:
        assert bvh.intersect(_cu(o), _cu(d), want=(), face_mask=mask, force_stack=True) == {}
    else:
        out, visited = bvh.intersect(_cu(o), _cu(d), want=(), face_mask=mask, count=True)
        assert out == {} and visited >= len(o)
    ref = np.zeros(len(mask), bool)
    ref[full["tid"][full["tid"] >= 0]] = True
    assert (mask.cpu().numpy().astype(bool) == ref).all()


@pytest.mark.parametrize("perspective", [True, False])
def test_tid_equals_visible_faces_rays_for_centroid_rays(perspective):
    from oracle import uv_project_ref as UP
    from unitex_amd.texturetools import ops
    v, f = RC.mesh("nested")
    c2w = np.eye(4, dtype=F32)[None].repeat(2, 0)
    c2w[0, :3, 3] = (0.3, -2.0, 1.1)
    c2w[1, :3, :3] = np.array([[0.6, 0.0, 0.8], [0.0, 1.0, 0.0], [-0.8, 0.0, 0.6]], F32)
    c2w[1, :3, 3] = (1.5, 0.4, 1.2)
    o, d = UP.centroid_rays(v, f, c2w, perspective)
    bvh = _bvh("nested")
    mask = ops.visible_faces_rays(bvh, _cu(c2w), perspective=perspective).cpu().numpy().astype(bool)
    for force_stack in WALKS:
        tid = bvh.intersect(_cu(o.reshape(-1, 3)), _cu(d.reshape(-1, 3)), want=("tid",), force_stack=force_stack)["tid"].cpu().numpy().reshape(2, -1)
        for b in range(2):
            ref = np.zeros(len(f), bool)
            ref[tid[b][tid[b] >= 0]] = True
            assert (ref == mask[b]).all() and ref.any() and not ref.all()


@pytest.mark.parametrize("force_stack", WALKS)
def test_degenerate_rays(force_stack):
    """the quad of two triangles with dyadic coordinates: every product of the triangle test is exact, so the expectations are exact"""
    bvh = _bvh("tri2")
    nan = float("nan")
    o = np.array([[0.25, 0.5, 0.0],      # starts on face 1: t = 0
                  [0.5, 0.5, 1.0],       # through the shared edge: both faces at t = 1 -> the smaller id
                  [0.0, 0.0, 2.0],       # through the shared vertex 0
                  [0.5, 0.75, 0.5],      # through the shared vertex 2, a corner of the mesh's box, along (0.5, 0.25, -0.5).  (An axis-parallel ray that runs INSIDE a
                                         # max-side face plane of a box -- from (1, 1, 0.5) along -z -- is outside the slab test's domain: its zero components become
                                         # 1e-30, the far bounds on x and y come out 0 and the box is left.  close_box's limit, recorded in DESIGN 8; not this test's subject.)
                  [0.75, 0.25, 1.0],     # face 0 from the front (normal +z, d = -z)
                  [0.75, 0.25, -1.0],    # face 0 from the back
                  [0.25, 0.5, 1.0], [0.25, 0.5, 1.0], [nan, 0.5, 1.0], [0.25, 0.5, 1.0],      # zero direction, NaN in d, NaN in o, pointing away
                  [0.25, 0.5, 1.0]], F32)      # parallel to the plane
    d = np.array([[0, 0, -1], [0, 0, -1], [0, 0, -1], [0.5, 0.25, -0.5], [0, 0, -1], [0, 0, 1], [0, 0, 0], [0, nan, -1], [0, 0, -1], [0, 0, 1], [1, 0, 0]], F32)
    got = _np(bvh.intersect(_cu(o), _cu(d), force_stack=force_stack))
    assert got["tid"].tolist() == [1, 0, 0, 0, 0, 0, -1, -1, -1, -1, -1]
    assert got["t"][:6].tolist() == [0.0, 1.0, 2.0, 1.0, 1.0, 1.0] and np.isposinf(got["t"][6:]).all()
    assert got["front"].tolist() == [1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0]
    assert got["loc"][:6].tolist() == [[0.25, 0.5, 0.0], [0.5, 0.5, 0.0], [0.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.75, 0.25, 0.0], [0.75, 0.25, 0.0]]
    assert got["uv"][:6].tolist() == [[0.25, 0.25], [0.0, 0.5], [0.0, 0.0], [0.0, 1.0], [0.5, 0.25], [0.5, 0.25]]
    assert not got["loc"][6:].any() and not got["uv"][6:].any()


@pytest.mark.parametrize("force_stack", WALKS)
def test_scaled_directions_name_the_same_face(force_stack):
    o, d, ref = RC.intersect_case("ico2", 257)
    bvh = _bvh("ico2")
    base = _np(bvh.intersect(_cu(o), _cu(d), want=("tid", "t"), force_stack=force_stack))
    sel = ref["ok"] & (ref["tid"] >= 0)
    for s in (1e-3, 1e3):
        got = _np(bvh.intersect(_cu(o), _cu((d * F32(s)).astype(F32)), want=("tid", "t"), force_stack=force_stack))
        assert (got["tid"][sel] == base["tid"][sel]).all() and (got["tid"][ref["ok"]] == ref["tid"][ref["ok"]]).all()
        # t scales with 1 / s: a dozen roundings of a float32 Moeller-Trumbore over a determinant of order 1e-2 (uv_project_ref's count), 1e-5 relative
        assert np.abs(got["t"][sel].astype(np.float64) * s / base["t"][sel] - 1.0).max() < 1e-5


# ---- occluded
@pytest.mark.parametrize("force_stack", WALKS)
@pytest.mark.parametrize("name,R", RC.OCCLUDED_INPUTS)
def test_occluded_against_brute_force_and_intersect(name, R, force_stack):
    a, b, blocked, ok = RC.occluded_case(name, R)
    bvh = _bvh(name)
    got = bvh.occluded(_cu(a), _cu(b), force_stack=force_stack).cpu().numpy()
    assert got.shape == (R,) and got.dtype == np.uint8 and (got <= 1).all()
    assert (got.astype(bool)[ok] == blocked[ok]).all()
    t = bvh.intersect(_cu(a), _cu((b - a).astype(F32)), want=("t",), force_stack=force_stack)["t"].cpu().numpy()
    assert ((t < 1)[ok] == got.astype(bool)[ok]).all()


@pytest.mark.parametrize("force_stack", WALKS)
def test_segments_ending_short_of_and_beyond_a_face(force_stack):
    bvh = _bvh("tri2")
    a = np.array([[0.25, 0.5, 1.0]] * 4 + [[0.25, 0.5, 0.0]], F32)
    b = np.array([[0.25, 0.5, 1e-3], [0.25, 0.5, -1e-3], [0.25, 0.5, 1.0], [0.25, 0.5, 0.0], [0.25, 0.5, -1.0]], F32)
    # short of the face; beyond it; zero length; ending ON the face (t = 1 exactly: strict, not blocked); starting on it (t = 0: blocked)
    assert bvh.occluded(_cu(a), _cu(b), force_stack=force_stack).cpu().tolist() == [0, 1, 0, 0, 1]
    o, d, ref = RC.intersect_case("ico2", 257)
    sel = ref["ok"] & (ref["tid"] >= 0)
    o, d, t = o[sel], d[sel], ref["t"][sel][:, None]
    bvh = _bvh("ico2")
    for s, want in ((1 - 1e-3, 0), (1 + 1e-3, 1)):
        end = (o + (t * s) * d).astype(F32)
        assert (bvh.occluded(_cu(o), _cu(end), force_stack=force_stack).cpu().numpy() == want).all()


# ---- enclosed points
def test_sphere_directions_equal_the_numpy_stream():
    from unitex_amd.texturetools import ops
    for n_points, n_rays, seed, sid in ((65, 33, RC.SEED, 0), (1, 1000, 666, 0), (3, 1024, 2 ** 40 + 5, 7), (300, 1, 1, 2 ** 32 - 1), (0, 4, 1, 0), (4, 0, 1, 0)):
        got = ops.sphere_directions(n_points, n_rays, seed, sid).cpu().numpy()
        assert got.shape == (n_points, n_rays, 3) and got.tobytes() == RC.sphere_directions(n_points, n_rays, seed, sid).tobytes(), (n_points, n_rays)


@pytest.mark.parametrize("force_stack", WALKS)
@pytest.mark.parametrize("name,N,n_rays", RC.ENCLOSED_INPUTS)
def test_points_enclosed_against_brute_force(name, N, n_rays, force_stack):
    p, dirs, inner, ok, hit = RC.enclosed_case(name, N, n_rays)
    bvh, seed = _bvh(name), RC.enclosed_seed(name, N, n_rays)
    pc = _cu(p)
    gen = bvh.points_enclosed(pc, n_rays, seed, force_stack=force_stack).cpu().numpy()
    rep = bvh.points_enclosed(pc, n_rays, 12345, dirs=_cu(dirs), force_stack=force_stack).cpu().numpy()
    full, hits = bvh.points_enclosed(pc, n_rays, seed, early_exit=False, want_hits=True, force_stack=force_stack)
    full, hits = full.cpu().numpy(), hits.cpu().numpy()
    assert gen.shape == (N,) and gen.dtype == np.uint8
    assert gen.tobytes() == rep.tobytes() == full.tobytes()
    assert (gen.astype(bool)[ok] == inner[ok]).all()
    if N:
        # hits with early exit off: the row sum of the any-hit over the same directions (long segments: the mesh lies within 4 units of every point)
        a = np.repeat(p, n_rays, 0)
        b = (a + F32(16) * dirs.reshape(-1, 3)).astype(F32)
        rows = bvh.occluded(_cu(a), _cu(b), force_stack=force_stack).cpu().numpy().reshape(N, n_rays).sum(1)
        _, decided = RC.brute_rays_hit(*RC.mesh(name), p, dirs)
        clear = decided.all(1)
        assert (hits[clear] == hit.sum(1)[clear]).all() and (hits[clear] == rows[clear]).all()
        assert ((hits == n_rays) == full.astype(bool)).all()


def test_points_enclosed_expected_pictures_and_splits():
    f = RC.g24()
    from unitex_amd.texturetools import ops
    for name in ("nested", "open"):
        bvh = ops.BVH(_cu(f["%s_verts" % name]), _cu(f["%s_faces" % name]))
        p, dirs, ok = f["self_%s_points" % name], f["self_%s_dirs" % name], f["self_%s_ok" % name]
        got = bvh.points_enclosed(_cu(p), dirs.shape[1], 0, dirs=_cu(dirs)).cpu().numpy().astype(bool)
        assert (got == f["self_%s_mask" % name])[ok].all()
        r = np.linalg.norm(p, axis=1)
        if name == "nested":      # inside either shell: inner; far outside: outer
            assert got[r < 0.85].all() and not got[r > 1.0].any()
        else:                     # under the hole: outer, for the recorded directions
            assert not got[:8].any() and got.any()
        # the same seed across splits of N: point i draws from counter (i, ray, attempt, stream), whatever the launch's size and grouping -- a prefix of the
        # points gives the prefix of the result, for a prefix that ends inside a wave, a block and a group alike, and with another n_rays grouping too
        for n_rays in (32, 5):
            whole = bvh.points_enclosed(_cu(p), n_rays, 777).cpu().numpy()
            for cut in (1, 40, 65):
                assert bvh.points_enclosed(_cu(p[:cut]), n_rays, 777).cpu().numpy().tobytes() == whole[:cut].tobytes()
        far = _cu((p / r[:, None] * F32(5)).astype(F32))
        assert not bvh.points_enclosed(far, 32, 777).any()


# ---- the public functions against fixture G24
def test_public_functions_against_g24():
    from unitex_amd.texturetools import ops, raytracing as RT
    f = RC.g24()
    rt = RT.RayTracing(_cu(f["nested_verts"]), _cu(f["nested_faces"]).long())
    assert (rt.V, rt.F) == (len(f["nested_verts"]), len(f["nested_faces"]))
    for name in ("nested", "open"):
        tree = rt if name == "nested" else ops.BVH(_cu(f["open_verts"]), _cu(f["open_faces"]))
        p, dirs, ok = f["self_%s_points" % name], f["self_%s_dirs" % name], f["self_%s_ok" % name]
        got = RT.self_rt(tree, _cu(p).reshape(4, 24, 3), n_rays=dirs.shape[1], dirs=_cu(dirs).reshape(4, 24, -1, 3))
        assert got.dtype == torch.bool and got.shape == (4, 24)
        assert (got.cpu().numpy().reshape(-1) == f["self_%s_mask" % name])[ok].all()
    got = RT.self_rt(rt, _cu(f["self_nested_points"]), seed=666)
    assert (got.cpu().numpy() == RT.self_rt(rt, _cu(f["self_nested_points"]), seed=666, chunk_size=7).cpu().numpy()).all()
    r = np.linalg.norm(f["self_nested_points"], axis=1)
    assert got.cpu().numpy()[r < 0.3].all() and not got.cpu().numpy()[r > 1.0].any()
    for chunk in (3, 4, 32):
        got = RT.cross_rt(rt, _cu(f["cross_points"]), _cu(f["cross_outer"]), chunk_size=chunk).cpu().numpy()
        assert got.shape == f["cross_mask"].shape and (got == f["cross_mask"])[f["cross_ok"]].all() and f["cross_ok"].all()
        got = RT.cross_rt(rt, _cu(f["pair_points"]), _cu(f["pair_outer"]), chunk_size=chunk, exhaustive_mode=False).cpu().numpy()
        assert got.shape == f["pair_mask"].shape == (5, 12) and (got == f["pair_mask"])[f["pair_ok"]].all()
    assert RT.cross_rt(rt, _cu(f["cross_points"]).reshape(2, 30, 3), _cu(f["cross_outer"])).shape == (2, 30)
    ids = RT.sphere_rt(rt, n_rays=500, sample_offset=float(f["sphere_offset"]), dirs=_cu(f["sphere_dirs"]))
    assert ids.dtype == torch.int64 and f["sphere_ok"].all() and sorted(ids.cpu().tolist()) == sorted(f["sphere_ids"].tolist())
    ids = RT.sphere_rt(rt, n_rays=500)
    assert len(ids) == 500 and (ids < rt.F // 2).all()      # the stream's own directions: every ray towards the origin hits the outer shell first
    assert (RT.outer_face_mask(rt, n_rays=500).cpu().numpy() == np.isin(np.arange(rt.F), ids.cpu().numpy())).all()
    axis = ops.BVH(_cu(f["axis_verts"]), _cu(f["axis_faces"]))
    for n in (4, 6):
        assert RT.sphere_rt_nvdiffrast(axis, n_cameras=n).cpu().tolist() == f["axis%d_ids" % n].tolist()
    assert len(RT.sphere_rt_nvdiffrast(rt, n_cameras=9)) == 9
    # batch shapes of intersects_closest, broadcast of a single origin against many directions
    d = _cu(RC.sphere_directions(6, 5, 3)).neg()
    hit, front, tri, loc, uv = rt.intersects_closest(torch.tensor([0.0, 0.0, 2.0], device="cuda"), d, stream_compaction=False)
    assert hit.shape == front.shape == tri.shape == (6, 5) and loc.shape == (6, 5, 3) and uv.shape == (6, 5, 2)
    assert hit.dtype == front.dtype == torch.bool and tri.dtype == torch.int64 and (tri[~hit] == -1).all() and not front[~hit].any() and hit.any()
    h2 = RT.ray_tracing(_cu(f["nested_verts"]), _cu(f["nested_faces"]).long(), torch.tensor([[0.0, 0.0, 2.0]], device="cuda"), d.reshape(-1, 3))
    assert (h2[2].reshape(6, 5) == tri).all()


def test_refusals_on_the_device():
    from unitex_amd.texturetools import ops, raytracing as RT
    bvh = _bvh("ico1")
    ctx, lib = bvh.ctx, bvh.ctx.lib
    z, out = torch.zeros(4, 3, device="cuda"), torch.zeros(4, dtype=torch.uint8, device="cuda")
    P = ops.ptr
    # zero counts return 0 at once, even with null operands
    assert lib.utx_bvh_intersect(ctx.handle, bvh.handle, None, None, 0, None, None, None, None, None, None, None, 0, None) == 0
    assert lib.utx_bvh_occluded(ctx.handle, bvh.handle, None, None, 0, None, None, 0, None) == 0
    assert lib.utx_points_enclosed(ctx.handle, bvh.handle, None, 0, 4, 0, 0, None, None, None, None, 0, None) == 0
    assert lib.utx_bvh_intersect(ctx.handle, bvh.handle, P(z), P(z), 4, None, None, None, None, None, None, None, 8, ctx.stream()) == -2
    assert lib.utx_bvh_occluded(ctx.handle, bvh.handle, P(z), P(z), 4, None, None, 0, ctx.stream()) == -2
    assert lib.utx_points_enclosed(ctx.handle, bvh.handle, P(z), 4, 1025, 0, 0, None, P(out), None, None, 0, ctx.stream()) == -2
    assert lib.utx_points_enclosed(ctx.handle, bvh.handle, P(z), 4, 4, 0, 0, None, P(out), None, None, 8, ctx.stream()) == -2
    for bad in (z.cpu(), z.long(), torch.zeros(4, 2, device="cuda"), torch.zeros(2, 4, 3, device="cuda")):
        with pytest.raises(ValueError):
            bvh.intersect(bad, z)
        with pytest.raises(ValueError):
            bvh.occluded(z, bad)
        with pytest.raises(ValueError):
            bvh.points_enclosed(bad, 4, 1)
    with pytest.raises(ValueError):
        bvh.intersect(z, z[:2])
    with pytest.raises(ValueError, match="unknown output"):
        bvh.intersect(z, z, want=("tid", "normal"))
    with pytest.raises(ValueError, match="face_mask"):
        bvh.intersect(z, z, face_mask=torch.zeros(3, dtype=torch.uint8, device="cuda"))
    for n in (0, 1025):
        with pytest.raises(ValueError, match="n_rays"):
            bvh.points_enclosed(z, n, 1)
    with pytest.raises(ValueError, match="dirs"):
        bvh.points_enclosed(z, 4, 1, dirs=torch.zeros(4, 5, 3, device="cuda"))
    with pytest.raises(ValueError):
        ops.sphere_directions(1 << 20, 1 << 20, 1)
    rt = RT.RayTracing(bvh.verts, bvh.faces)
    with pytest.raises(NotImplementedError):
        rt.intersects_closest(z, z, stream_compaction=True)
    with pytest.raises(ValueError, match="different devices"):
        rt.intersects_closest(z, z.cpu())
    with pytest.raises(ValueError, match="broadcast"):
        rt.intersects_closest(z, torch.zeros(3, 3, device="cuda"))
    with pytest.raises(ValueError):
        rt.intersects_closest(z.long(), z)
    with pytest.raises(ValueError, match="different devices"):
        RT.cross_rt(rt, z, z.cpu())

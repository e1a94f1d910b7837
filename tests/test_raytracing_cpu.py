"""Ray casting without a device: the direction stream's numpy restatement, the float64 restatement against fixture G24 (the reference's own check_visibility.py),
the exclusion cap of every input the GPU tests use, the host-layer refusals of texturetools/raytracing.py and the ABI conventions of the new declarations."""
import os
import re

import numpy as np
import pytest
import torch

from tests.support import raycast_ref as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the direction stream
def test_directions_are_unit_length():
    d = RC.sphere_directions(64, 100, RC.SEED).astype(np.float64)
    err = np.abs(np.linalg.norm(d, axis=-1) - 1.0)
    print("max | |d| - 1 | = %.3g = %.2f * 2^-23" % (err.max(), err.max() * 2 ** 23))
    assert err.max() <= 2.0 ** -23


def test_directions_do_not_depend_on_the_chunking():
    whole = RC.sphere_directions(10, 33, 666, stream_id=3)
    parts = np.concatenate([RC.sphere_directions(3, 33, 666, stream_id=3), RC.sphere_directions(7, 33, 666, stream_id=3, point0=3)])
    assert whole.tobytes() == parts.tobytes()
    assert RC.sphere_directions(10, 5, 666, stream_id=3).tobytes() == whole[:, :5].tobytes()      # ray j is ray j, whatever n_rays
    assert RC.sphere_directions(10, 33, 666, stream_id=4).tobytes() != whole.tobytes()
    assert RC.sphere_directions(10, 33, 667, stream_id=3).tobytes() != whole.tobytes()


def test_first_directions_are_pinned():
    """seed 666, stream 0, point 0, rays 0 .. 2: computed once from the definition (Philox4x32-10 of oracle/sampling_ref.py, whose known-answer vectors
    tests/test_sampling_cpu.py pins) and pinned here as float32 bit patterns"""
    got = RC.sphere_directions(1, 3, 666)[0].view(np.uint32)
    print([[hex(x) for x in r] for r in got.tolist()])
    assert got.tolist() == PINNED


PINNED = [[0x3e9aadf2, 0xbd363a41, 0x3f73c5aa], [0xbf76e7bf, 0xbe672c5c, 0xbe0c7f50], [0x3f6b5ce8, 0xbe4db118, 0x3ead2898]]


def test_rejection_counts_follow_the_attempt_counter():
    """a draw is rejected with probability 1 - pi / 4: the mean number of rejections is (1 - p) / p = 0.2732 with p = pi / 4.  20000 directions: standard error of
    the mean sqrt((1 - p)) / p / sqrt(n) = 0.0042, the bound is five of them.  Each direction must be the one its recorded attempt gives (the attempt counter is
    word 2 of the Philox counter), and none is exhausted."""
    d, rej = RC.sphere_directions(200, 100, 12345, want_attempts=True)
    p = np.pi / 4
    assert rej.max() < RC.MAX_ATTEMPTS
    assert abs(rej.mean() - (1 - p) / p) < 5 * np.sqrt(1 - p) / p / np.sqrt(rej.size)
    assert (rej > 0).any() and (rej > 1).any()
    from oracle.sampling_ref import philox4x32_10
    for i, j in ((0, 0), (7, 31), (199, 99)) + tuple(zip(*np.nonzero(rej > 1)))[:3]:
        a = int(rej[i, j])
        for attempt in range(a + 1):
            w = philox4x32_10(np.array([[i, j, attempt, 0]], np.uint32), np.array([[12345, 0]], np.uint32))[0]
            x = np.float32(2) * ((w[:2] >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)) - np.float32(1)
            s = x[0] * x[0] + x[1] * x[1]
            assert (s < 1) == (attempt == a)
        assert d[i, j, 2] == np.float32(1) - np.float32(2) * s


# ---- the restatement against the reference's own functions (fixture G24)
def test_restatement_agrees_with_the_reference_on_g24():
    f = RC.g24()
    for name in ("nested", "open"):
        v, fa = f["%s_verts" % name], f["%s_faces" % name]
        inner, ok, _ = RC.brute_enclosed(v, fa, f["self_%s_points" % name], f["self_%s_dirs" % name])
        assert (ok == f["self_%s_ok" % name]).all() and RC.excluded_share(ok) <= RC.EXCLUSION_CAP
        assert (inner == f["self_%s_mask" % name])[ok].all()
        assert inner.any() and not inner.all()
    v, fa = f["nested_verts"], f["nested_faces"]
    p, o = f["cross_points"], f["cross_outer"]
    N, M = len(p), len(o)
    blocked, ok = RC.brute_any(v, fa, np.repeat(o[None], N, 0).reshape(-1, 3), np.repeat(p[:, None], M, 1).reshape(-1, 3))
    ok = ok.reshape(N, M).all(1)
    assert RC.excluded_share(ok) <= RC.EXCLUSION_CAP and (blocked.reshape(N, M).all(1) == f["cross_mask"])[ok].all()
    blocked, ok = RC.brute_any(v, fa, f["pair_outer"].reshape(-1, 3), f["pair_points"].reshape(-1, 3))
    ok = ok.reshape(f["pair_mask"].shape + (-1,)).all(-1)
    assert RC.excluded_share(ok) <= RC.EXCLUSION_CAP and (blocked.reshape(f["pair_mask"].shape + (-1,)).all(-1) == f["pair_mask"])[ok].all()
    r = RC.brute_closest(v, fa, f["sphere_origins"], -f["sphere_dirs"])
    assert RC.excluded_share(r["ok"]) <= RC.EXCLUSION_CAP
    assert set(r["tid"][r["ok"] & (r["tid"] >= 0)].tolist()) <= set(f["sphere_ids"].tolist())
    # the fixture's expected pictures: the points under the hole of the open sphere are outer, the points inside either shell are inner, far points are outer
    assert not f["self_open_mask"][:8].any()
    pn = np.linalg.norm(f["self_nested_points"], axis=1)
    assert f["self_nested_mask"][pn < 0.85].all() and not f["self_nested_mask"][pn > 1.0].any()


# ---- the exclusion cap: a condition on the inputs, from the float64 numbers alone
@pytest.mark.parametrize("name,R", RC.INTERSECT_INPUTS)
def test_intersect_inputs_respect_the_exclusion_cap(name, R):
    o, d, ref = RC.intersect_case(name, R)
    share = RC.excluded_share(ref["ok"])
    print("%s R=%d: %d of %d rays excluded, %d hits" % (name, R, (~ref["ok"]).sum(), R, (ref["tid"] >= 0).sum()))
    assert share <= RC.EXCLUSION_CAP
    if R >= 63:
        assert (ref["tid"] >= 0).any()
        if name != "tri1":      # a single triangle seen from all around: both outcomes only on the closed meshes
            assert ref["front"].any() and (~ref["front"] & (ref["tid"] >= 0)).any()


@pytest.mark.parametrize("name,R", RC.OCCLUDED_INPUTS)
def test_occluded_inputs_respect_the_exclusion_cap(name, R):
    a, b, blocked, ok = RC.occluded_case(name, R)
    print("%s R=%d: %d excluded, %d blocked" % (name, R, (~ok).sum(), blocked.sum()))
    assert RC.excluded_share(ok) <= RC.EXCLUSION_CAP
    if R >= 63:
        assert blocked.any() and not blocked.all()


@pytest.mark.parametrize("name,N,n_rays", RC.ENCLOSED_INPUTS)
def test_enclosed_inputs_respect_the_exclusion_cap(name, N, n_rays):
    p, dirs, inner, ok, _ = RC.enclosed_case(name, N, n_rays)
    print("%s N=%d n_rays=%d: %d excluded, %d inner" % (name, N, n_rays, (~ok).sum(), inner.sum()))
    assert RC.excluded_share(ok) <= RC.EXCLUSION_CAP
    if N >= 65 and name not in ("tri1", "tri2"):
        assert inner.any() and not inner.all()


def test_float32_restatement_agrees_with_float64_on_clear_rays():
    v, f = RC.mesh("ico2")
    o, d, ref = RC.intersect_case("ico2", 257)
    r = RC.tri_f32(v, f, o, d, ref["tid"])
    sel = ref["ok"] & (ref["tid"] >= 0)
    assert r["hit"][sel].all() and not r["hit"][ref["tid"] < 0].any()
    assert np.abs(r["t"][sel] - ref["t"][sel]).max() < 1e-5 and np.abs(r["uv"][sel, 0] - ref["u"][sel]).max() < 1e-4
    assert (r["front"][sel].astype(bool) == ref["front"][sel]).all()


# ---- host layer
def test_raytracing_refusals_without_a_device():
    from unitex_amd.texturetools import raytracing as RT
    v, f = torch.zeros(3, 3), torch.tensor([[0, 1, 2]])
    with pytest.raises(NotImplementedError):
        RT.RayTracing(v, f, backend="nvdiffrast")
    with pytest.raises(NotImplementedError):
        RT.RayTracing(v, f, backend="embree")
    for bad_v, bad_f in ((v.long(), f), (torch.zeros(3, 2), f), (v, f.float()), (v, torch.zeros(0, 3, dtype=torch.int64)), (v, torch.zeros(2, 4, dtype=torch.int64))):
        with pytest.raises(ValueError):
            RT.RayTracing(bad_v, bad_f)
    with pytest.raises(ValueError, match="GPU"):
        RT.RayTracing(v, f)
    pts = torch.zeros(4, 3)
    for n in (0, 1025, -1, 2.5, True):
        with pytest.raises(ValueError, match="n_rays"):
            RT.self_rt(None, pts, n_rays=n)
    with pytest.raises(ValueError, match="n_rays"):
        RT.sphere_rt(None, n_rays=0)
    with pytest.raises(ValueError):
        RT.self_rt(None, pts.long())
    with pytest.raises(ValueError):
        RT.self_rt(None, torch.zeros(4, 2))
    with pytest.raises(ValueError, match="RayTracing or an ops.BVH"):
        RT.self_rt(object(), pts)
    with pytest.raises(ValueError, match="chunk_size"):
        RT.cross_rt(None, pts, pts, chunk_size=0)
    with pytest.raises(ValueError):
        RT.cross_rt(None, pts, pts.long())
    with pytest.raises(ValueError):
        RT.cross_rt(None, pts, pts, exhaustive_mode=False)      # paired mode needs [..., M, 3]
    with pytest.raises(ValueError, match="broadcast"):
        RT.cross_rt(_FakeTree(), torch.zeros(2, 3, 3), torch.zeros(2, 4, 3), exhaustive_mode=False)


class _FakeTree:
    """stands in for ops.BVH where only the shape handling is under test: every segment blocked / every point inner"""
    def __init__(self):
        self.seen = []

    def occluded(self, a, b):
        self.seen.append(a.shape[0])
        return torch.ones(a.shape[0], dtype=torch.uint8)

    def points_enclosed(self, p, n_rays, seed, dirs=None):
        self.seen.append((p.shape[0], n_rays, seed, None if dirs is None else tuple(dirs.shape)))
        return torch.ones(p.shape[0], dtype=torch.uint8)

    intersect = None


def test_batch_shapes_and_chunking_of_the_host_layer():
    from unitex_amd.texturetools import raytracing as RT
    t = _FakeTree()
    assert RT.self_rt(t, torch.zeros(2, 5, 3), n_rays=7, chunk_size=3).shape == (2, 5) and t.seen == [(10, 7, 666, None)]
    t = _FakeTree()
    RT.self_rt(t, torch.zeros(2, 5, 3), n_rays=7, dirs=torch.zeros(2, 5, 7, 3))
    assert t.seen == [(10, 7, 666, (10, 7, 3))]
    with pytest.raises(ValueError, match="dirs"):
        RT.self_rt(t, torch.zeros(2, 5, 3), n_rays=7, dirs=torch.zeros(10, 7, 3))
    t = _FakeTree()
    RT.self_rt(t, torch.zeros(1, 3), seed=None)
    RT.self_rt(t, torch.zeros(1, 3), seed=None)
    assert t.seen[0][2] != t.seen[1][2]
    t = _FakeTree()
    m = RT.cross_rt(t, torch.zeros(2, 3, 3), torch.zeros(10, 3), chunk_size=4)
    assert m.shape == (2, 3) and m.all() and t.seen == [24, 24, 12]
    t = _FakeTree()
    m = RT.cross_rt(t, torch.zeros(5, 2, 7, 3), torch.zeros(7, 3), chunk_size=32, exhaustive_mode=False)
    assert m.shape == (5, 2) and t.seen == [70]


# ---- ABI
def test_new_declarations_follow_the_abi_conventions():
    from unitex_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "unitex_hip.h")).read(), flags=re.S)
    for name in ("utx_bvh_intersect", "utx_bvh_occluded", "utx_points_enclosed", "utx_sphere_directions"):
        m = re.search(r"\bint %s\s*\(([^;]*)\);" % name, src)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        assert params[0] == "utx_ctx* ctx" and params[-1] == "utx_stream stream"
        restype, argtypes = _lib.SYMBOLS[name]
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
    from unitex_amd.csrc import build as b
    flags = dict(b.SOURCES)
    assert "-ffp-contract=off" in flags["raycast.hip"] and all(x in flags["raycast.hip"] for x in b.NO_PK)
    csrc = os.path.join(ROOT, "unitex_amd", "csrc")
    hits = [f for f in os.listdir(csrc) if f.endswith((".hip", ".h", ".cpp")) and re.search(r"void philox4x32_10\(", open(os.path.join(csrc, f)).read())]
    assert hits == ["philox_device.h"], hits


def test_abi_refusals_that_need_no_device():
    """every -2 of the new entry points is returned before any device call"""
    import ctypes as C
    from unitex_amd import _lib
    lib = _lib.load_library()
    buf = (C.c_float * 12)()
    out = (C.c_ubyte * 4)()
    fake = C.c_void_p(C.addressof(buf))      # never dereferenced: each call below is refused on its arguments first
    big = 1 << 31
    assert lib.utx_bvh_intersect(None, None, buf, buf, 1, None, None, None, None, None, None, None, 0, None) == -2
    assert lib.utx_bvh_occluded(None, None, buf, buf, 1, out, None, 0, None) == -2
    assert lib.utx_points_enclosed(None, None, buf, 1, 4, 0, 0, None, out, None, None, 0, None) == -2
    for R in (-1, big):
        assert lib.utx_bvh_intersect(None, fake, buf, buf, R, None, None, None, None, None, None, None, 0, None) == -2
        assert lib.utx_bvh_occluded(None, fake, buf, buf, R, out, None, 0, None) == -2
        assert lib.utx_points_enclosed(None, fake, buf, R, 4, 0, 0, None, out, None, None, 0, None) == -2
    assert lib.utx_bvh_intersect(None, fake, None, buf, 1, None, None, None, None, None, None, None, 0, None) == -2
    assert lib.utx_bvh_intersect(None, fake, buf, None, 1, None, None, None, None, None, None, None, 0, None) == -2
    assert lib.utx_bvh_intersect(None, fake, buf, buf, 1, None, None, None, None, None, None, None, 2, None) == -2
    assert lib.utx_bvh_occluded(None, fake, None, buf, 1, out, None, 0, None) == -2
    assert lib.utx_bvh_occluded(None, fake, buf, None, 1, out, None, 0, None) == -2
    assert lib.utx_bvh_occluded(None, fake, buf, buf, 1, None, None, 0, None) == -2
    assert lib.utx_bvh_occluded(None, fake, buf, buf, 1, out, None, 2, None) == -2
    for n in (0, -1, 1025):
        assert lib.utx_points_enclosed(None, fake, buf, 1, n, 0, 0, None, out, None, None, 0, None) == -2
    assert lib.utx_points_enclosed(None, fake, None, 1, 4, 0, 0, None, out, None, None, 0, None) == -2
    assert lib.utx_points_enclosed(None, fake, buf, 1, 4, 0, 0, None, None, None, None, 0, None) == -2
    assert lib.utx_points_enclosed(None, fake, buf, 1, 4, 0, 0, None, out, None, None, 4, None) == -2
    assert lib.utx_sphere_directions(None, -1, 4, 0, 0, buf, None) == -2
    assert lib.utx_sphere_directions(None, 4, -1, 0, 0, buf, None) == -2
    assert lib.utx_sphere_directions(None, 1 << 20, 1 << 20, 0, 0, buf, None) == -2
    assert lib.utx_sphere_directions(None, 1, 4, 0, 0, None, None) == -2
    assert lib.utx_sphere_directions(None, 0, 4, 0, 0, None, None) == 0 and lib.utx_sphere_directions(None, 4, 0, 0, 0, None, None) == 0

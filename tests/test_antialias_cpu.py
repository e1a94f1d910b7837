"""Silhouette antialiasing, the part that needs no GPU: the topology against an independent restatement, the rule on cases with dyadic coordinates (where
float32 is exact: equality, not closeness), its float32 restatement against the float64 one, six planted mistakes, and the Python argument checks.

Float32 against float64 on the GPU test's cases (GPU_CASES below; the kernel inherits the figure through bit-equality with antialias_f32, nothing here is
tuned on GPU output).  Pairs whose decisions (near triangle, chosen edge, silhouette) differ between the two restatements are counted and the pixels they touch
excluded; the excluded share of the pixels that receive a contribution is at most 1 % in every case.  Recorded, colours uniform in [-1, 1]:
    excluded pixels: 0 in every case (158 ... 1303 pixels receive a contribution);  max |f32 - f64| over the rest, at 17 x 63 / 64 x 257, three views:
    triangle 3.9e-06 / 2.9e-05, fan 1.7e-05 / 6.1e-05, folded 4.3e-06 / 2.1e-05, quads 7.0e-06 / 2.2e-04, sphere 5.6e-06 / 4.4e-05, sphere_w 2.5e-05 / 4.4e-05,
    bad_index 5.6e-06 / 4.4e-05, empty 0 / 0.  The figure is the conditioning of d = (Xa Yb - Xb Ya) / (Yb - Ya): coordinates of up to W pixels carry W 2^-24,
    and an edge nearly parallel to the pair divides that by a small Yb - Ya; it grows with the screen and is not asserted."""
import numpy as np
import pytest

from tests.support import antialias_ref as R

F32 = np.float32
M, H8, W8 = 4, 4, 8      # the exact cases: the tested edge lies between the centres of pixels M and M + 1 of an 8-pixel line, 4 lines


def _ndc(px, size):
    return px / size * 2.0 - 1.0


def _pos(points, H, W, transpose=False):
    """pixel coordinates (X, Y, depth) -> clip space with w = 1; transpose swaps the roles of x and y (the horizontal-edge twin)"""
    out = []
    for X, Y, z in points:
        if transpose:
            X, Y = Y, X
        out.append([_ndc(X, W), _ndc(Y, H), z, 1.0])
    return np.array(out, F32)


def _screen(transpose):
    return (W8, H8) if transpose else (H8, W8)      # (H, W)


def _line(img, transpose):
    """the 8-pixel lines across the tested edge as rows"""
    return np.swapaxes(img, 0, 1) if transpose else img


def _render(points, tri, transpose):
    H, W = _screen(transpose)
    pos = _pos(points, H, W, transpose)
    tri = np.array(tri, np.int32)
    return R._rasterize(pos, tri, H, W), pos, tri


def quad(d, transpose=False, z=0.0):
    """an axis-aligned quad whose edge lies at X = M + 0.5 + d, far larger than the screen on its other sides (its diagonal crosses no pixel centre)"""
    xe = M + 0.5 + d
    return _render([(-8, -4, z), (xe, -4, z), (xe, 8, z), (-8, 8, z)], [[0, 1, 2], [0, 2, 3]], transpose)


def wing_pair(d, folded):
    """a triangle left of the edge X = M + 0.5 + d that covers the screen there, and a second one on the edge: across it in the same plane (coplanar), or
    folded back onto the first one's side, behind it"""
    xe = M + 0.5 + d
    third = (-8, 2, 0.5) if folded else (xe + 16, 2, 0.0)      # the third coordinate is z / w: smaller is nearer, so the folded wing's tip lies behind
    pts = [(xe, -12, 0.0), (xe, 16, 0.0), (-24, 2, 0.0), third]
    return _render(pts, [[0, 1, 2], [1, 0, 3]], False)


def expected_alpha_line(d):
    a = np.zeros(W8, F32)
    a[:M] = 1.0
    a[M] = 1.0 - max(0.5 - d, 0.0)
    a[M + 1] = max(d - 0.5, 0.0)      # at d = 1 the edge runs through the centre of M + 1 (covered, inclusive) and the pair (M + 1, M + 2) blends it: 0.5 as well
    return a


DS = (0.0, 0.125, 0.5, 0.75, 1.0)


def _alpha(rast):
    return (rast[..., 3:4] > 0).astype(F32)


def _aa(color, rast, pos, tri, mistake=None):
    """the restatement on the PRODUCT's topology (meshes.edge_opposites): the exact cases hold the host half of the feature as well"""
    from unitex_amd.texturetools import meshes
    return R.antialias_f32(color, rast, pos, tri, opp=meshes.edge_opposites(tri), mistake=mistake)


def run_quad(d, transpose, mistake=None):
    rast, pos, tri = quad(d, transpose)
    return _line(_aa(_alpha(rast), rast, pos, tri, mistake)[..., 0], transpose)


def run_overlap(d, mistake=None):
    """the near quad of quad(d) in front of a far quad that covers the screen; colour 0.75 on the near one, 0.25 on the far one"""
    xe = M + 0.5 + d
    pts = [(-8, -4, -0.5), (xe, -4, -0.5), (xe, 8, -0.5), (-8, 8, -0.5), (-16, -8, 0.5), (24, -8, 0.5), (24, 12, 0.5), (-16, 12, 0.5)]
    rast, pos, tri = _render(pts, [[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], False)
    near = (rast[..., 3:4] == 1) | (rast[..., 3:4] == 2)
    assert (rast[..., 3] > 0).all() and near.any() and not near.all()
    color = np.where(near, F32(0.75), F32(0.25)).astype(F32)
    return _aa(color, rast, pos, tri, mistake)[..., 0], near[..., 0]


def expected_overlap_line(d):
    a = np.full(W8, 0.25, F32)
    a[:M] = 0.75
    a[M] = 0.75 + max(0.5 - d, 0.0) * (0.25 - 0.75)
    a[M + 1] = 0.25 + max(d - 0.5, 0.0) * (0.75 - 0.25)
    return a


def run_corner(mistake=None):
    """one triangle with a right angle at the centre of pixel (M, 2): that pixel takes 0.5 from its right and 0.5 from its lower neighbour, and the colours make
    the float32 sum depend on the order"""
    xe, ye = M + 0.5, 2.5
    rast, pos, tri = _render([(xe, -20, 0.0), (xe, ye, 0.0), (-30, ye, 0.0)], [[0, 1, 2]], False)
    u = 2.0 ** -24
    color = np.ones((H8, W8, 1), F32)
    color[2, M, 0], color[2, M + 1, 0], color[3, M, 0] = 1 + 2 * u, 1 + 4 * u, 1 + 8 * u
    return _aa(color, rast, pos, tri, mistake)[2, M, 0]


# ---- topology
def _grid(n):
    idx = np.arange((n + 1) * (n + 1)).reshape(n + 1, n + 1)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, 1:].ravel(), idx[1:, :-1].ravel()
    return np.concatenate([np.stack([a, b, c], 1), np.stack([a, c, d], 1)]).astype(np.int32)


@pytest.mark.parametrize("name", ["sphere", "grid", "fan", "triangle"])
def test_edge_opposites_equals_the_restatement(name):
    from unitex_amd.texturetools import meshes
    faces = {"sphere": R._icosphere()[1], "grid": _grid(5), "fan": np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int32),
             "triangle": np.array([[0, 1, 2]], np.int32)}[name]
    got, want = meshes.edge_opposites(faces), R.edge_opposites(faces)
    assert got.dtype == np.int32 and got.shape == faces.shape and np.array_equal(got, want)
    if name == "sphere":
        assert len(faces) == 80 and (got >= 0).all()
    if name == "grid":
        assert (got < 0).sum() == 4 * 5
    if name == "fan":
        assert got.tolist() == [[3, -1, -1], [2, -1, -1], [-1, -1, -1]]
    if name == "triangle":
        assert (got == -1).all()
    adj = meshes.face_adjacency(faces)
    assert np.array_equal(got < 0, adj < 0)
    for f, e in zip(*np.nonzero(adj >= 0)):
        assert got[f, e] in faces[adj[f, e]] and got[f, e] not in (faces[f, e], faces[f, (e + 1) % 3])


def test_the_mesh_caches_its_edge_opposites():
    import torch
    from unitex_amd.texturetools.renderer_inverse import DeviceMesh
    m = DeviceMesh.__new__(DeviceMesh)
    m.device, m.faces = torch.device("cpu"), torch.from_numpy(_grid(2))
    first = m.edge_opposites
    assert first is m.edge_opposites and first.dtype == torch.int32 and np.array_equal(first.numpy(), R.edge_opposites(_grid(2)))


# ---- exact cases
@pytest.mark.parametrize("transpose", [False, True])
@pytest.mark.parametrize("d", DS)
def test_axis_aligned_edge_gives_the_exact_area_coverage(d, transpose):
    got = run_quad(d, transpose)
    want = expected_alpha_line(d)
    assert got.shape == (H8, W8) and got.dtype == F32
    for line in got:
        assert line.tobytes() == want.tobytes(), (d, transpose, line, want)
        assert float(line.astype(np.float64).sum()) == M + 0.5 + d      # the quad covers [0, M + 0.5 + d] of the line


def test_coplanar_neighbour_leaves_the_interior_unchanged():
    rast, pos, tri = wing_pair(0.125, folded=False)
    ids = rast[..., 3]
    assert (ids > 0).all() and (ids == 1).any() and (ids == 2).any()      # the shared edge crosses the screen, which both triangles fill
    color = np.random.default_rng(3).uniform(-1, 1, (H8, W8, 3)).astype(F32)
    assert _aa(color, rast, pos, tri).tobytes() == color.tobytes()


@pytest.mark.parametrize("d", DS)
def test_folded_neighbour_blends_the_shared_edge(d):
    rast, pos, tri = wing_pair(d, folded=True)
    assert set(np.unique(rast[..., 3]).tolist()) == {0.0, 1.0}      # the wing hides behind the triangle
    assert R.edge_opposites(tri)[0, 0] == 3
    got = _aa(_alpha(rast), rast, pos, tri)[..., 0]
    for line in got:
        assert line.tobytes() == expected_alpha_line(d).tobytes(), (d, line)


@pytest.mark.parametrize("d", DS)
def test_overlapping_quads_blend_the_near_edge_with_the_far_colour(d):
    got, near = run_overlap(d)
    for line in got:
        assert line.tobytes() == expected_overlap_line(d).tobytes(), (d, line)
    assert np.array_equal(got[:, M + 2:], np.full((H8, W8 - M - 2), 0.25, F32))      # the far quad's own interior does not move


def test_corner_pixel_sums_in_the_fixed_order():
    c, kr, kd = F32(1 + 2.0 ** -23), F32(2.0 ** -24), F32(3 * 2.0 ** -24)
    want = F32(F32(c + kr) + kd)
    assert want != F32(F32(c + kd) + kr)      # the case can tell the orders apart
    assert run_corner() == want == F32(1 + 2.0 ** -21)


@pytest.mark.parametrize("name", R.CASES)
def test_constant_colour_returns_itself(name):
    case = R.render_case(name, 17, 63, B=1, C=3)
    color = np.full_like(case["color"], F32(0.3))
    assert _aa(color, case["rast"], case["pos"], case["tri"]).tobytes() == color.tobytes()
    for d in (0.125, 0.75):
        rast, pos, tri = quad(d)
        const = np.full((H8, W8, 2), F32(-1.7), F32)
        assert _aa(const, rast, pos, tri).tobytes() == const.tobytes()


# ---- planted mistakes
def _exact_cases_pass(mistake):
    """does the restatement with the planted mistake still pass each exact case?  -> {case: passed}"""
    res = {}
    for transpose in (False, True):
        res["quad_t%d" % transpose] = all((run_quad(d, transpose, mistake) == expected_alpha_line(d)).all() for d in DS)
    rast, pos, tri = wing_pair(0.125, folded=False)
    color = np.random.default_rng(3).uniform(-1, 1, (H8, W8, 3)).astype(F32)
    res["coplanar"] = _aa(color, rast, pos, tri, mistake).tobytes() == color.tobytes()
    rast, pos, tri = wing_pair(0.125, folded=True)
    res["folded"] = bool((_aa(_alpha(rast), rast, pos, tri, mistake)[..., 0] == expected_alpha_line(0.125)).all())
    res["overlap"] = all((run_overlap(d, mistake)[0] == expected_overlap_line(d)).all() for d in DS)
    res["corner"] = bool(run_corner(mistake) == F32(1 + 2.0 ** -21))
    return res


def test_the_exact_cases_pass_without_a_mistake():
    assert all(_exact_cases_pass(None).values())


@pytest.mark.parametrize("mistake,rejected_by", [("near", "overlap"), ("no_swap", "quad_t1"), ("d_from_q", "quad_t0"), ("wing_sign", "coplanar"),
                                                 ("no_border", "quad_t0"), ("order", "corner")])
def test_planted_mistake_is_rejected(mistake, rejected_by):
    assert mistake in R.MISTAKES
    res = _exact_cases_pass(mistake)
    assert not res[rejected_by], (mistake, res)


# ---- float32 against float64
GPU_CASES = [(name, 17, 63) for name in R.CASES] + [(name, 64, 257) for name in R.CASES]


@pytest.mark.parametrize("name,H,W", GPU_CASES)
def test_float32_against_float64(name, H, W):
    from unitex_amd.texturetools import meshes
    case = R.render_case(name, H, W, B=3, per_view=True, C=3)
    receives, excluded, err = R.compare_f32_f64(case["color"], case["rast"], case["pos"], case["tri"], meshes.edge_opposites(case["tri"]))
    print("%s %dx%d: %d pixels receive a contribution, %d excluded, max |f32 - f64| = %.3g" % (name, H, W, receives, excluded, err))
    if name == "empty":
        assert receives == 0 and err == 0.0
        return
    assert receives > 0
    assert excluded <= 0.01 * receives, (excluded, receives)


# ---- Python argument checks
def test_python_argument_checks_need_no_gpu(monkeypatch):
    """ValueError / TypeError come before the library is touched"""
    import torch
    from unitex_amd.texturetools import ops
    from unitex_amd.texturetools.renderer_inverse import NVDiffRendererInverse

    def no_ctx(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(ops, "get_ctx", no_ctx)
    rast, pos = torch.zeros(2, 4, 5, 4), torch.zeros(2, 6, 4)
    tri = torch.zeros(3, 3, dtype=torch.int32)
    opp = -torch.ones(3, 3, dtype=torch.int32)
    color, w = torch.zeros(2, 4, 5, 3), torch.zeros(2, 4, 5, 4)
    with pytest.raises(ValueError, match="rast is"):
        ops.antialias_weights(rast[..., :3], pos, tri, opp)
    with pytest.raises(ValueError, match="rast is expected"):
        ops.antialias_weights(rast.double(), pos, tri, opp)
    with pytest.raises(ValueError, match="pos_clip is"):
        ops.antialias_weights(rast, pos[:1], tri, opp)
    with pytest.raises(ValueError, match="pos_clip is"):
        ops.antialias_weights(rast, pos[..., :3], tri, opp)
    with pytest.raises(ValueError, match="tri is expected"):
        ops.antialias_weights(rast, pos, tri.long(), opp)
    with pytest.raises(ValueError, match="tri is .* and opp"):
        ops.antialias_weights(rast, pos, tri, opp[:2])
    with pytest.raises(ValueError, match="CUDA"):
        ops.antialias_weights(rast, pos, tri, opp)
    with pytest.raises(ValueError, match="weights is"):
        ops.antialias_apply(color, w[:, :3])
    with pytest.raises(ValueError, match="color is"):
        ops.antialias_apply(color[0, 0], w[0, 0])
    with pytest.raises(ValueError, match="CUDA"):
        ops.antialias_apply(color, w)
    with pytest.raises(ValueError, match="one screen"):
        ops.antialias(color[:, :3], rast, pos, tri)
    with pytest.raises(ValueError, match="tri is expected"):
        ops.antialias(color, rast, pos, tri.float())
    with pytest.raises(ValueError, match="CUDA"):
        ops.antialias(color, rast, pos, tri)      # opp=None: the topology is built on the host, then the device check refuses
    inv = NVDiffRendererInverse(device="cpu")
    cam = (torch.eye(4)[None], torch.eye(3)[None], (4, 5))
    with pytest.raises(NotImplementedError, match="render_voxel_attr"):
        inv.simple_rendering(*cam, antialias=True, render_voxel_attr=True)
    with pytest.raises(TypeError, match="antialias"):
        inv.global_inverse_rendering(None, *cam, 8, antialias=True)
    import inspect
    for name in ("simple_rendering", "geometry_rendering", "vertex_rendering", "uv_rendering"):
        assert inspect.signature(getattr(inv, name)).parameters["antialias"].default is False, name


def test_abi_binds_the_antialias_entry_points():
    import os
    from unitex_amd import _lib
    lib = _lib.load_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "unitex_hip.h")).read()
    for name, n_args in (("utx_antialias_analyze", 13), ("utx_antialias_apply", 9)):
        assert name in _lib.SYMBOLS and hasattr(lib, name) and "int %s(" % name in hdr and len(_lib.SYMBOLS[name][1]) == n_args
    # the argument checks come before any device call: no context, null pointers
    assert lib.utx_antialias_analyze(None, None, None, 0, None, None, 1, 3, 1, 4, 4, None, None) == -2
    assert lib.utx_antialias_apply(None, None, None, 1, 4, 4, 1, None, None) == -2


# ---- fixture G27
def test_g27_alpha_is_the_restatement_on_the_reference_s_rasters():
    """the reference's alpha = dr.antialias(mask.float(), rast, v_pos_clip, t_pos_idx) with dr.antialias bound to antialias_f32: recomputed here on the
    product's topology; the fixture holds what the issue asks for"""
    from unitex_amd.texturetools import meshes
    f = R.load_g27()
    H, W = R.G27_SCREEN
    verts, faces, uvs, nrm, v_attr, tex = R.g27_scene()
    for k, v in (("verts", verts), ("faces", faces), ("uvs", uvs), ("v_nrm", nrm), ("v_attr", v_attr), ("map_0", tex)):
        assert f[k].dtype == v.dtype and np.array_equal(f[k], v), k
    assert len(faces) == 81 and (meshes.edge_opposites(faces)[80] == -1).all()      # the 80-face sphere and the fin, whose three edges are borders
    for tag in ("p", "o"):
        rast, clip = f["rast_" + tag], f["clip_" + tag]
        assert rast.shape == (R.G27_VIEWS, H, W, 4) and clip.shape == (R.G27_VIEWS, len(verts), 4)
        cov = rast[..., 3:4] > 0
        alpha = _aa(cov.astype(F32), rast, clip, faces)
        assert alpha.tobytes() == f["alpha_" + tag].tobytes()
        assert ((alpha > 0) & (alpha < 1) & cov).any() and ((alpha > 0) & (alpha < 1) & ~cov).any()
        assert (rast[..., 3] == 81).reshape(R.G27_VIEWS, -1).any(1).all()      # every view shows the fin
        for k in R.G27_GEOMETRY + ("uv", "v_attr", "map_attr"):
            assert f["%s_%s" % (k, tag)].shape[:3] == (R.G27_VIEWS, H, W), k
        # world_position: lerp(-1, x, alpha) and the stencil, restated with numpy's float32 operations in torch.lerp's two forms
        from oracle import gbuffer_ref as GB
        x = np.where(cov, GB.interp_views(verts, rast, faces), F32(0.0)).astype(F32)
        a, fill = alpha, np.full_like(x, F32(-1.0))
        lerp = np.where(a < F32(0.5), fill + a * (x - fill), x - (x - fill) * (F32(1.0) - a)).astype(F32)
        got = _aa(lerp, rast, clip, faces)
        assert np.abs(got.astype(np.float64) - f["world_position_" + tag]).max() <= 5 * 6 * 2.0 ** -24 * 2      # torch may fuse the lerp: 6 u (1 + 1), spread by the stencil
    import os
    assert os.path.getsize(R.G27) < 1000 * 1000


def test_generator_reproduces_the_committed_g27(tmp_path):
    """re-runs tests/golden/make_golden_antialias.py and compares every array bit for bit; it imports the reference's own Python, which lives outside this
    repository: the test runs wherever that tree is present and skips, before doing any work, where it is not"""
    import os
    import subprocess
    import sys
    gold = os.path.dirname(R.G27)
    sys.path.insert(0, gold)
    try:
        from make_golden import REF
    finally:
        sys.path.remove(gold)
    if not os.path.isdir(REF):
        pytest.skip("the reference tree is not on this machine")
    r = subprocess.run([sys.executable, os.path.join(gold, "make_golden_antialias.py"), str(tmp_path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    new, old = np.load(str(tmp_path / "g27_antialias.npz")), R.load_g27()
    assert sorted(new.files) == sorted(old)
    for k in old:
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape and new[k].tobytes() == old[k].tobytes(), k

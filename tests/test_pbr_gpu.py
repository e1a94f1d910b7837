"""Image-based PBR shading on the GPU (csrc/pbr.hip) against the fp64 restatement of oracle/pbr_ref.py and the reference's own PBRModel.forward
(fixture G15).  ulp = np.spacing of the named magnitude in float32."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import pbr_ref as PC
from oracle import video_types_ref as VC

pytestmark = pytest.mark.gpu
F32 = np.float32
U = 2.0 ** -24


def _cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def _ulp(x):
    return float(np.spacing(F32(np.abs(x).max())))


# ---------------------------------------------------------------------------------------------------------------- cube orientation and seams
def _seam_dirs():
    out = []
    for a in range(3):                    # 12 edges x (+0, -0) third component, 6 axes x (+0, -0), 8 corners
        b, c = (a + 1) % 3, (a + 2) % 3
        for sa in (1.0, -1.0):
            for z in (0.0, -0.0):
                d = np.zeros(3); d[a] = sa; d[b] = z; d[c] = z
                out.append(d)
                for sb in (1.0, -1.0):
                    d = np.zeros(3); d[a] = sa; d[b] = sb; d[c] = z
                    out.append(d)
    for sx in (1.0, -1.0):
        for sy in (1.0, -1.0):
            for sz in (1.0, -1.0):
                out.append(np.array([sx, sy, sz]))
    return np.asarray(out, F32)


def test_cube_faces_centres_edges_and_corners():
    from unitex_amd.texturetools import ops
    N = 4
    const = np.broadcast_to((np.arange(6, dtype=F32) + 1)[:, None, None, None] * np.array([1.0, 0.5, 0.25], F32), (6, N, N, 3)).copy()
    axes = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], F32)
    assert np.array_equal(ops.cube_sample(_cu(const), _cu(axes)).cpu().numpy(), const[:, 0, 0])
    tex, _ = ops.cubemap_tables(N, None, "cuda")
    centres = tex[..., :3].contiguous()
    assert np.array_equal(ops.cube_sample(_cu(const), centres).cpu().numpy(), const)
    rng = np.random.default_rng(7)
    cube = rng.uniform(0, 1, (6, N, N, 3)).astype(F32)
    assert np.array_equal(ops.cube_sample(_cu(cube), centres).cpu().numpy(), cube), "a texel-centre direction returns that texel exactly"
    # edges, corners, axes with +-0: same taps and weights as the oracle (the inputs are exact in both); what differs is the rounding of three a + f (b - a)
    # blends (2 roundings each on values <= max) and of the corner mean (3 roundings): <= 9 half-ulps of the maximum -> 5 ulp
    d = _seam_dirs()
    got = ops.cube_sample(_cu(cube), _cu(d)).cpu().numpy()
    assert np.abs(got - PC.cube_lookup(cube, d)).max() <= 5 * _ulp(cube)
    # one ulp across an edge: the kernel moves by no more than the oracle does, plus the rounding of both evaluations (5 ulp each, as above) and the face
    # coordinate's own fp32 uncertainty (2 ulp of 1 in f, times N / 2 texels, times a texel difference <= max: 4 ulp of the maximum at N = 4)
    t = rng.uniform(-1, 1, 64).astype(F32)
    base = []
    for a in range(3):
        for sa in (1.0, -1.0):
            for sb in (1.0, -1.0):
                e = np.zeros((64, 3), F32); e[:, a] = sa; e[:, (a + 1) % 3] = sb; e[:, (a + 2) % 3] = t
                base.append(e)
    base = np.concatenate(base)
    lo, hi = base.copy(), base.copy()
    for i in range(base.shape[0]):
        a = int(np.argmax(np.abs(base[i]) == 1.0))
        lo[i, a] = np.nextafter(base[i, a], F32(0))
    k = ops.cube_sample(_cu(cube), _cu(np.concatenate([lo, hi]))).cpu().numpy()
    o = PC.cube_lookup(cube, np.concatenate([lo, hi]))
    n = base.shape[0]
    assert (np.abs(k[:n] - k[n:]) <= np.abs(o[:n] - o[n:]) + 14 * _ulp(cube)).all()


def test_latlong_to_cubemap():
    from unitex_amd.texturetools import ops
    lat = np.random.default_rng(11).uniform(0, 8, (4, 8, 3)).astype(F32)
    want, px = PC.latlong_to_cubemap(lat, 8)
    assert (px < 0).any() and (px > 7).any(), "texels whose tu wraps"
    got = ops.latlong_to_cubemap(_cu(lat), 8).cpu().numpy()
    err = np.abs(got - want).max()
    print("latlong max error / ulp(max):", err / _ulp(lat))
    assert err <= 4 * _ulp(lat)


# ---------------------------------------------------------------------------------------------------------------- prefilters
@pytest.mark.parametrize("N", [8, 16])
def test_diffuse_prefilter(N):
    """|got - fp64 sum| <= (n + 64) 2^-24 sum|terms|, n = 6 N^2: a sum of n fp32 terms in any order, plus 64 ulp for the per-term weight"""
    from unitex_amd.texturetools import ops
    cube = np.random.default_rng(N).uniform(0, 50, (6, N, N, 3)).astype(F32)
    n = 6 * N * N
    for c in (cube, np.ones_like(cube)):
        want, scale = PC.diffuse_prefilter(c)
        got = ops.cubemap_diffuse(_cu(c)).cpu().numpy()
        rel = (np.abs(got - want) / scale).max()
        print("diffuse N=%d: max error / sum|terms| = %.3g (bound %.3g)" % (N, rel, (n + 64) * U))
        assert rel <= (n + 64) * U
        assert np.array_equal(got, ops.cubemap_diffuse(_cu(c)).cpu().numpy()), "run-to-run identical"
    # the oracle's value for ones is near but not equal to 1: the 0.999 clamp and the short pi pull it down, pixel_area pulls it up (the products of angle
    # differences add up to (pi / 2)^2 per face against a true 2 pi / 3, at most 17.8 % high); 0.077 at N = 8, 0.116 at N = 16
    assert 1e-4 < np.abs(want - 1.0).max() < 0.178, "near but not equal to 1"


def test_diffuse_prefilter_refuses_odd_sizes():
    from unitex_amd._lib import ptr
    from unitex_amd.flux.ops import get_ctx
    from unitex_amd.texturetools import ops
    with pytest.raises(ValueError):
        ops.cubemap_tables(7, None, "cuda")
    ctx = get_ctx(0)
    cube, tab = torch.ones(6, 7, 7, 3, device="cuda"), torch.ones(6, 8, 8, 4, device="cuda")
    out = torch.empty_like(cube)
    assert ctx.lib.utx_cubemap_diffuse(ctx.handle, ptr(cube), 7, ptr(tab), ptr(out), ctx.stream()) < 0
    assert ctx.lib.utx_cubemap_specular(ctx.handle, ptr(cube), 7, ptr(tab), ptr(tab), 0.5, 0.9, ptr(out), ctx.stream()) < 0
    assert ctx.lib.utx_cubemap_diffuse(ctx.handle, ptr(None), 8, ptr(tab), ptr(out), ctx.stream()) < 0
    assert ctx.lib.utx_dfg_lut(ctx.handle, 0, 16, ptr(out), ctx.stream()) < 0


@pytest.mark.parametrize("roughness", [0.5, 0.08])
def test_specular_prefilter(roughness):
    """same tolerance form with n the accepted count of each output, against sum|c w| / sum w"""
    from unitex_amd.texturetools import ops
    N = 16
    cutoff = PC.specular_cutoff(N, roughness)
    cube = np.random.default_rng(16).uniform(0, 50, (6, N, N, 3)).astype(F32)
    want, scale, count = PC.specular_prefilter(cube, roughness, cutoff)
    got = ops.cubemap_specular(_cu(cube), roughness, cutoff).cpu().numpy()
    rel = np.abs(got - want) / scale / ((count[..., None] + 64) * U)
    print("specular r=%.2f cutoff=%.6f: accepted %d..%d, max error / bound = %.3g" % (roughness, cutoff, count.min(), count.max(), rel.max()))
    assert rel.max() <= 1.0
    assert np.array_equal(got, ops.cubemap_specular(_cu(cube), roughness, cutoff).cpu().numpy())
    ones = ops.cubemap_specular(_cu(np.ones_like(cube)), roughness, cutoff).cpu().numpy()
    assert np.array_equal(ones, np.ones_like(cube)), "a constant cubemap returns exactly 1.0f"
    if roughness == 0.08:
        single = count == 1
        assert single.any()
        assert np.array_equal(got[single], cube[single]), "a lobe of one texel returns that texel exactly"


# ---------------------------------------------------------------------------------------------------------------- DFG table
# max |fp64 twin (oracle/pbr_ref.py dfg_lut(256, 1024)) - the reference's bsdf_256_256.bin|, measured on the CPU: 0.012928 at (roughness row 64, cos column 0),
# mean 7.6e-4.  With Karis' separable k = a / 2 Smith term the difference was 0.35 (structural); the height-correlated term closed it.
FG_LUT_TWIN_DIFFERENCE = 0.012928


def test_dfg_lut_against_its_fp64_twin():
    from unitex_amd.texturetools import ops
    got = ops.dfg_lut(32, 1024).cpu().numpy()
    err = np.abs(got - PC.dfg_lut(32, 1024)).max()
    print("dfg R=32: max abs error", err)
    assert err <= 1e-5


def test_dfg_lut_against_the_references_table():
    """bound = 1.5 x the difference measured between the fp64 twin and the reference's table (third-party data of unknown provenance)"""
    from unitex_amd.texturetools import ops
    got = ops.dfg_lut(256, 1024).cpu().numpy()
    diff = np.abs(got - PC.load_fg_lut()).max()
    print("dfg R=256 vs the reference's table: max abs difference", diff)
    assert diff <= 1.5 * FG_LUT_TWIN_DIFFERENCE


# ---------------------------------------------------------------------------------------------------------------- shading
def _model(f):
    from unitex_amd.texturetools.pbr import PBRModel
    m = PBRModel.__new__(PBRModel)
    m.device = torch.device("cuda:0")
    m.light_diffuse, m.light_specular, m.FG_LUT = _cu(f["light_diffuse"]), _cu(f["light_specular"]), _cu(f["fg_lut"])[None]
    return m


def test_g15_forward_and_fused_shade():
    """16 ulp of each output's maximum.  Per term, in half-ulps of a unit value: two normalisations (dot 3, sqrt 1, divide 1 each), the reflection (3) and its
    normalisation (5) put ~ 8 u on a lookup direction; the face coordinate divides once more (1) and N / 2 = 4 texels per unit turn that into 4 * 9 u of a
    texel difference (<= the light's maximum); three blends add 6 u; the coefficient and the product 4 u: ~ 46 u = 23 ulp worst case if every rounding
    went the same way, 16 ulp being the issue's bound on what is actually reached."""
    from unitex_amd.texturetools import ops
    f = PC.load_g15()
    m = _model(f)
    t = lambda k: torch.from_numpy(f[k])
    d, s = m.forward(t("view_position").reshape(1, 1, 3), t("world_position"), t("world_normal"), t("map_Kd"), t("map_Ks"))
    args = (_cu(f["rast"]), _cu(f["faces"], torch.int32), _cu(f["verts"]), _cu(f["v_nrm"]), _cu(f["uvs"]), _cu(f["tex_Kd"]), _cu(f["tex_Ks"]), f["view_position"].tolist(),
            m.light_diffuse, m.light_specular, m.FG_LUT[0])
    _, fd = ops.pbr_shade(*args, lambda_diffuse=1.0, lambda_specular=0.0, want_rgba=True)
    _, fs = ops.pbr_shade(*args, lambda_diffuse=0.0, lambda_specular=1.0, want_rgba=True)
    u8, frgb = ops.pbr_shade(*args, want_rgba=True)
    for name, dense, fused in (("diffuse", d, fd), ("specular", s, fs)):
        for tag, got in (("forward", dense.cpu().numpy()), ("shade", fused[..., :3].cpu().numpy())):
            err = np.abs(got - f[name]).max() / _ulp(f[name])
            print("G15 %s through %s: %.2f ulp of the maximum" % (name, tag, err))
            assert err <= 16, (name, tag)
    assert (frgb[..., 3] == 1).all()
    want = (np.clip(f["diffuse"] + f["specular"], 0, 1) * F32(255.0)).astype(np.uint8)
    assert np.abs(u8.cpu().numpy().astype(np.int32) - want.astype(np.int32)).max() <= 1


@pytest.mark.parametrize("tag", ["p", "o"])
def test_torus_frame(tag):
    from unitex_amd.texturetools import camera, ops
    f = VC.load()
    persp, _, _ = VC.SETS[tag]
    size = 48
    rng = np.random.default_rng(8)
    ld, ls, lut = _cu(rng.uniform(0, 2, (6, 8, 8, 3)).astype(F32)), _cu(rng.uniform(0, 2, (6, 8, 8, 3)).astype(F32)), _cu(rng.uniform(0, 1, (16, 16, 2)).astype(F32))
    c2w = torch.from_numpy(f["c2ws_" + tag][:1])
    intr = torch.from_numpy(f["intr_" + tag])
    mvp = torch.matmul(camera.intr_to_proj(intr, perspective=persp), camera.c2w_to_w2c(c2w)).cuda().contiguous()
    verts, faces = _cu(f["verts"]), _cu(f["faces"], torch.int32)
    clip, _ = ops.transform_points(verts, mvp, want_ndc=False)
    rast = ops.rasterize(clip[0].contiguous(), faces, size, size)
    kd = _cu(np.ascontiguousarray(f["tex"][:, :, :3]).astype(F32) / F32(255.0))
    eye = c2w[0, :3, 3].tolist()
    bg = (0.25, 0.5, 0.75)
    base = (rast, faces, verts, _cu(f["v_nrm"]), _cu(f["uvs"]), kd)
    u8, rgba = ops.pbr_shade(*base, None, eye, ld, ls, lut, bg=bg, want_rgba=True)
    cov = (rast[..., 3] > 0).cpu().numpy()
    rgba, u8 = rgba.cpu().numpy(), u8.cpu().numpy()
    assert cov.any() and not cov.all()
    assert np.array_equal(rgba[..., 3], cov.astype(F32)), "alpha equals coverage"
    assert (rgba[~cov][:, :3] == np.array(bg, F32)).all() and (u8[~cov] == (np.array(bg, F32) * F32(255.0)).astype(np.uint8)).all()
    const = torch.tensor([1.0, 1.0, 0.0], device="cuda").expand(kd.shape).contiguous()
    u8c, rgbac = ops.pbr_shade(*base, const, eye, ld, ls, lut, bg=bg, want_rgba=True)
    assert np.array_equal(u8c.cpu().numpy(), u8) and np.array_equal(rgbac.cpu().numpy(), rgba), "Ks = None is bit-identical to the constant [1, 1, 0] texture"
    metal = torch.tensor([1.0, 0.5, 1.0], device="cuda").expand(kd.shape).contiguous()
    _, black = ops.pbr_shade(*base, metal, eye, ld, torch.zeros_like(ls), lut, bg=bg, want_rgba=True)
    assert (black.cpu().numpy()[cov][:, :3] == 0).all(), "metallic 1 with a black specular light gives black"


def test_export_orbit_video_with_and_without_a_model(tmp_path):
    from unitex_amd.texturetools.pbr import PBRModel
    from unitex_amd.texturetools.video import VideoExporter, read_mjpeg_mp4
    f = VC.load()
    mesh = (f["verts"], f["faces"], f["uvs"], f["tex"], f["v_nrm"])
    ex = VideoExporter(device="cuda:0")
    a = ex.export_orbit_video(mesh, str(tmp_path / "a.mp4"), n_frames=3, render_size=64, return_frames=True)
    b = ex.export_orbit_video(mesh, str(tmp_path / "b.mp4"), n_frames=3, render_size=64, return_frames=True, pbr_model=None)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    env = np.random.default_rng(2).uniform(0, 2, (8, 16, 3)).astype(F32)
    model = PBRModel(env, device="cuda:0", cube_res=16, roughness=0.5)
    assert model.light_diffuse.shape == (6, 16, 16, 3) and model.light_specular.shape == (6, 16, 16, 3) and model.FG_LUT.shape == (1, 256, 256, 2)
    ks = np.zeros(f["tex"].shape[:2] + (3,), np.uint8)
    ks[..., 1], ks[..., 2] = 128, 255
    p = str(tmp_path / "lit.mp4")
    lit = ex.export_orbit_video(mesh + (ks,), p, n_frames=3, render_size=64, fps=12, return_frames=True, pbr_model=model)
    fps, jpgs = read_mjpeg_mp4(p)
    assert fps == 12 and len(jpgs) == 3 and len(lit) == 3 and lit[0].shape == (64, 64, 3)
    assert not np.array_equal(lit[0], a[0])
    with pytest.raises(ValueError):
        ex.export_orbit_video(mesh, p, n_frames=2, render_size=32, video_type="world_normal", pbr_model=model)
    ones = PBRModel(None, device="cuda:0", cube_res=8, roughness=0.5, fg_lut=PC.load_fg_lut())
    assert ones.FG_LUT.shape == (1, 256, 256, 2) and np.array_equal(ones.light_specular.cpu().numpy(), np.ones((6, 8, 8, 3), F32))

"""Geometry-buffer video types of VideoExporter.export_orbit_video (TEST INFRASTRUCTURE ONLY): the table of the reference's simple_rendering
(render/nvdiffrast/renderer_base.py:153-241) and export_video (video/export_nvdiffrast_video.py:107-131) restated in numpy float32 in the
operation order of utx_gbuffer_shade, against the reference's own frames (fixture G13, tests/golden/make_golden_video_types.py; alpha =
coverage, dr.antialias stubbed).  tests/test_video_types_cpu.py pins it against the fixture; the GPU module (tests/test_video_types_gpu.py) uses
it at other sizes.

Bounds (u = 2^-24, the unit roundoff of float32; none of them was taken from the code under test):
  * world_position, camera_position, z_depth: every step (interpolation (a0*u + a1*v) + a2*w, select, (x - lo) / (hi - lo), x * 0.5 + 0.5,
    x * alpha + bg * (1 - alpha)) is a correctly rounded float32 operation in a fixed order on inputs that are the reference's own
    (the fixture stores the per-vertex attributes the reference handed to dr.interpolate): BIT-EXACT.
  * distance: torch.norm(p=2) over three components; its order and use of FMA are torch's.  Both sides compute sqrt(x^2 + y^2 + z^2) with
    at most 3 roundings under the root (relative 3u, halved by the root) and one for the root, so each is within 2.5u * d of the exact value
    and the two differ by at most 5u * d <= 5u * dmax.  The frame value is n = (d - lo) / (hi - lo), in units of u * dmax / (hi - lo):
    5 from d itself; 10 from lo and hi, which are such norms too (lo moves the numerator by 5, lo and hi move the denominator by 5 each,
    weighted by |n|, which the count takes as <= 1 for the sum of the two); 3 from the three roundings of the normalisation
    (subtraction, subtraction, division).  DIST_ULPS = 5 + 10 + 3 = 18.
  * world_normal, camera_normal: F.normalize = x / max(sqrt(sum of three squares), 1e-12).  The two lengths differ by at most 5u relative (as
    above), each division rounds once (u), so a component of the unit vector (|c| <= 1) differs by at most 7u; x * 0.5 is exact and + 0.5
    rounds once on each side (values in [0, 1]: u / 2 each): 3.5u + u < NORMAL_ULPS = 5 units of u on the frame value.
  * per-vertex attributes recomputed from the mesh and the cameras (what export_orbit_video does, with utx_transform_points' order
    ((x*m0 + y*m1) + z*m2) + m3) instead of the reference's torch.matmul, whose order is unspecified: a dot product of 4 terms has at most
    4 roundings on either side, so the two differ by at most 8u * S, S = sum |x_k m_k| (<= SMAX over the mesh); the 5 roundings of the
    interpolation and the 2 of the ndc map then act on values below SMAX: POS_ULPS = 8 + 5 + 2 <= 16 units of u * SMAX.  The camera normals'
    3-term product differs by at most 6u * sqrt(3), is normalised (7u) and interpolated and normalised again (5 + 7): CAMNRM_ULPS = 11 + 7
    + 12 = 30 units of u on a unit vector.
  * rgb (uint8 only: utx_texture_shade writes no float frame): the reference samples with grid_sample(bilinear, align_corners=False) at
    ((g + 1) * W - 1) / 2, g = interp(2 * uv - 1); the build at interp(uv) * W - 0.5 (dr.texture's convention: the same point).  W = 16 is a
    power of two, so the scalings are exact; the reference's coordinate carries 1 + 5 roundings on values <= 1 (scaled by W / 2) and two on
    values <= 2 and <= 2W (together 2uW): <= 5uW; the build's 5 on values <= 1 (scaled by W) and one on a value <= W: <= 6uW.  So the two
    sample points differ by <= 11uW per axis, bilinear interpolation of texels in [0, 1] is 1-Lipschitz per axis in texel units (also
    across a cell boundary: it is continuous): 22uW, plus at most 10 (build: two lerps of lerps) + 12 (reference: four weight products,
    four terms) roundings on values <= 1: RGB_ULPS = 22 * (W + 1) units of u.  The fixture's uvs keep every footprint inside the texture:
    over its border the reference zero-pads and the build's rgb path wraps (dr.texture), a difference by design that G13 does not enter.
uint8 frames: equal to trunc(clamp(x) * 255) of the fixture's float wherever that float * 255 is farther from an integer than 255 * the arm's
float bound, within 1 LSB elsewhere; with a bit-exact arm that is plain equality.  NaN (orthographic z_depth: clip w is 1 on every vertex, so
lo = hi and the reference computes 0 / 0) converts to 0 in the kernel (fmaxf(NaN, 0) = 0) and in numpy on x86; such pixels must be NaN in
the float frame and are held to 0 in the uint8 one."""
import os

import numpy as np

from . import geom_ref as G
from .pixel_ref import interp, len3, unit

GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
F32 = np.float32
U = 2.0 ** -24
GEOM_TYPES = ["world_normal", "camera_normal", "world_position", "camera_position", "z_depth", "distance"]
NORMALIZE = ("z_depth", "distance")
FILL = {"world_normal": -1.0, "camera_normal": -1.0, "world_position": -1.0, "camera_position": 0.0, "z_depth": 0.0, "distance": 0.0}
SETS = {"p": (True, 4, 64), "o": (False, 2, 48)}
NORMAL_ULPS, DIST_ULPS, POS_ULPS, CAMNRM_ULPS = 5, 18, 16, 30
RGB_ULPS = 22 * (16 + 1)


def load():
    return np.load(os.path.join(GOLD, "g13_video_types.npz"), allow_pickle=False)


def vertex_attr(video_type, verts, nrm, c2w, intr, perspective, w2c=None, mvp=None):
    """the per-vertex attribute export_orbit_video hands to utx_gbuffer_shade for one view, in the kernels' operation order
    (w2c / mvp [4,4]: the matrices the caller gave the GPU, where it did not build them with the oracle's functions)"""
    verts, nrm, c2w = np.asarray(verts, F32), np.asarray(nrm, F32), np.asarray(c2w, F32)
    if video_type == "world_normal":
        return nrm
    if video_type == "world_position":
        return verts
    if video_type == "camera_normal":       # utx_camera_normals
        R = c2w[:3, :3]
        c = (nrm[:, 0:1] * R[0] + nrm[:, 1:2] * R[1]) + nrm[:, 2:3] * R[2]
        return unit(c).astype(F32)
    w2c = G.c2w_to_w2c(c2w[None]).astype(F32) if w2c is None else np.asarray(w2c, F32)[None]
    if video_type == "z_depth":             # utx_transform_points(proj @ w2c)[..., 3]
        mvp = np.matmul(G.intr_to_proj(intr, perspective=perspective), w2c).astype(F32) if mvp is None else np.asarray(mvp, F32)[None]
        return G.transform_points(verts, mvp)[0][:, 3:4]
    return G.transform_points(verts, w2c)[0][:, :3]         # camera_position, distance


def buffer_of(video_type, rast, faces, attr):
    """the buffer before export_video: [H,W,3] float32 (lerp with alpha in {0, 1} = select), and the coverage"""
    p, cov = interp(attr, rast, faces)
    if video_type in ("world_normal", "camera_normal"):
        p = unit(p)
    elif video_type == "distance":
        p = np.repeat(len3(p), 3, -1)
    elif video_type == "z_depth":
        p = np.repeat(p, 3, -1)
    return np.where(cov[..., None], p, F32(FILL[video_type])).astype(F32), cov


def value_range(video_type, rast, faces, attr):
    """(lo, hi) over the covered pixels of this frame, or None if it covers nothing (utx_gbuffer_range)"""
    b, cov = buffer_of(video_type, rast, faces, attr)
    return (b[cov].min(), b[cov].max()) if cov.any() else None


def shade(video_type, rast, faces, attr, scale2=None, ndc=False, bg=(1.0, 1.0, 1.0)):
    """utx_gbuffer_shade: -> (float RGBA [H,W,4], uint8 [H,W,3])"""
    x, cov = buffer_of(video_type, rast, faces, attr)
    a = cov.astype(F32)[..., None]
    with np.errstate(invalid="ignore", divide="ignore"):
        if scale2 is not None:
            lo, hi = F32(scale2[0]), F32(scale2[1])
            x = np.where(cov[..., None], (x - lo) / (hi - lo), x)
        if ndc:
            x = x * F32(0.5) + F32(0.5)
        if bg is not None:
            x = x * a + np.asarray(bg, F32) * (F32(1.0) - a)
    x = x.astype(F32)
    return np.concatenate([x, a], -1), to_u8(x)


def to_u8(x):
    """clamp(0, 1) * 255 truncated; NaN -> 0 (see the module docstring)"""
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(x), F32(0.0), np.clip(x, F32(0.0), F32(1.0)) * F32(255.0)).astype(np.uint8)


def fixture_frames(f, video_type, tag):
    """float frames [n,H,W,3] of the fixture (z_depth / distance are stored as one channel)"""
    x = f["%s_%s" % (video_type, tag)]
    return np.repeat(x[..., None], 3, -1) if x.ndim == 3 else x


def fixture_attr(f, video_type, tag, i):
    """the per-vertex attribute the REFERENCE interpolated for frame i"""
    if video_type == "world_normal":
        return f["v_nrm"]
    if video_type == "world_position":
        return f["verts"]
    if video_type == "camera_normal":
        return f["v_nrm_cam_" + tag][i]
    if video_type == "z_depth":
        return f["v_clip_w_" + tag][i][:, None]
    return f["v_pos_cam_" + tag][i]


def float_bound(f, video_type, tag, own_attrs=False):
    """absolute bound on a float frame value for this arm (module docstring); 0.0 = bit-exact.  own_attrs: the per-vertex attributes
    are recomputed from mesh and cameras instead of being the reference's."""
    smax = float(np.abs(f["verts"]).sum(-1).max() + 2.8 + 1.0)      # sum |x_k m_k| <= |x| + |y| + |z| + |t|, rotation entries <= 1, |t| = 2.8
    b = 0.0
    if video_type in ("world_normal", "camera_normal"):
        b = NORMAL_ULPS * U
        if own_attrs and video_type == "camera_normal":
            b += CAMNRM_ULPS * U
    elif video_type == "distance":
        lo, hi = f["scale_distance_" + tag]
        dmax = float(np.nanmax(f["raw_distance_" + tag]))
        b = DIST_ULPS * U * dmax / float(hi - lo)
        if own_attrs:
            b += 4 * POS_ULPS * U * smax * dmax / float(hi - lo) ** 2      # value, lo and hi each move by sqrt(3) * POS_ULPS u SMAX <= 2 units; n <= dmax / (hi - lo)
    elif video_type == "camera_position" and own_attrs:
        b = POS_ULPS * U * smax
    return b


def check_frame(name, got_rgba, got_u8, ref_rgb, ref_alpha, bound):
    """the comparison both modules use: float frame within `bound` (0 = bit-exact, NaN where the reference has NaN), alpha equal, uint8 equal
    wherever the reference's float * 255 is farther from an integer than 255 * bound and within 1 LSB elsewhere.  Prints before asserting."""
    nan = np.isnan(ref_rgb)
    with np.errstate(invalid="ignore"):
        d = np.where(nan, 0.0, np.abs(got_rgba[..., :3].astype(np.float64) - ref_rgb.astype(np.float64)))
    ref_u8 = to_u8(ref_rgb)
    du = np.abs(got_u8.astype(np.int32) - ref_u8.astype(np.int32))
    with np.errstate(invalid="ignore"):
        y = np.where(nan, 0.5, np.clip(ref_rgb, 0, 1).astype(np.float64) * 255.0)
    near = np.abs(y - np.round(y)) <= 255.0 * bound
    print("%s: float max|diff| %.3g (bound %.3g), NaN %d, uint8 max diff %d, differing %d (near an integer: %d)" %
          (name, d.max(), bound, int(nan.sum()), int(du.max()), int((du > 0).sum()), int(near.sum())))
    assert np.array_equal(np.isnan(got_rgba[..., :3]), nan), name
    assert np.array_equal(got_rgba[..., 3], ref_alpha), name
    if bound == 0.0:
        assert np.array_equal(got_rgba[..., :3][~nan], ref_rgb[~nan]), "%s: not bit-exact, max|diff| %.3g" % (name, d.max())
        assert np.array_equal(got_u8, ref_u8), name
    else:
        assert d.max() <= bound, "%s: max|diff| %.3g > %.3g" % (name, d.max(), bound)
        assert du.max() <= 1 and not (du[~near] > 0).any(), name


def check_u8(name, got_u8, ref_rgb, bound):
    """uint8 frame against the reference's float frame: equal to trunc(clamp(x) * 255) wherever x * 255 is farther from an integer than
    255 * bound, within 1 LSB elsewhere.  Prints before asserting."""
    ref_u8 = to_u8(ref_rgb)
    du = np.abs(got_u8.astype(np.int32) - ref_u8.astype(np.int32))
    y = np.clip(ref_rgb, 0, 1).astype(np.float64) * 255.0
    near = np.abs(y - np.round(y)) <= 255.0 * bound
    print("%s: uint8 max diff %d, differing %d (of them away from an integer: %d)" % (name, int(du.max()), int((du > 0).sum()), int((du[~near] > 0).sum())))
    assert du.max() <= 1 and not (du[~near] > 0).any(), name


def rgb_texture(f):
    """the fixture's texture as utx_texture_shade wants it (fp32, row index growing with v: the fixture's row 0 is v = 0 already)"""
    return np.ascontiguousarray(f["tex"]).astype(F32) / F32(255.0)

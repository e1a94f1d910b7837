"""Restatement (TEST INFRASTRUCTURE ONLY) of the face / vertex visibility and of the atlas-space view projection (utx_visible_faces_rays, utx_visible_faces_raster,
utx_erode_faces, utx_visible_vertices, utx_uv_project) in numpy, shared by tests/test_uv_project_cpu.py and tests/test_uv_project_gpu.py and,
for the ray caster, by the fixture maker tests/golden/make_golden_uv_project.py; the loader of fixture G19, its cases and their comparison.  The
interpolation and the map lookups are oracle/pixel_ref.py's, the bound of the 'bilinear' lookup oracle/gbuffer_ref.py's map_bound.

The ray caster is a brute force in float64: every ray against every triangle, Moeller-Trumbore on both sides, the hit with the smallest t >= 0, ties
to the smallest face id.  margin() says which rays a float32 traversal may legitimately decide differently: those whose winner leads the next hit by no
more than MARGIN in t, or that pass within MARGIN (in barycentric units) of an edge of a triangle they could hit not later than that.  With
unit-scale geometry MARGIN = 1e-4 is about a hundred times the rounding of a float32 Moeller-Trumbore (a dozen operations at 6e-8 each on numbers
of order 1, divided by a determinant of order 1e-2 for the triangles of the test meshes)."""
import os

import numpy as np

from .gbuffer_ref import MODES, map_bound
from .pixel_ref import interp, sample

GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
F32, F64, U = np.float32, np.float64, 2.0 ** -24
MARGIN = 1e-4
TWO_SQRT3 = 2.0 * np.sqrt(3.0)


def centroid_rays(verts, faces, c2ws, perspective):
    """(origins, directions) [B,F,3] float32 as Mesh.get_visible_faces forms them (mesh/structure.py:805-811)"""
    verts, c2ws = np.asarray(verts, F32), np.asarray(c2ws, F32)
    tri = verts[np.asarray(faces)]
    cen = ((tri[:, 0] + tri[:, 1]) + tri[:, 2]) / F32(3.0)
    B = c2ws.shape[0]
    if perspective:
        o = np.broadcast_to(c2ws[:, None, :3, 3], (B,) + cen.shape)
        return o.astype(F32), (cen[None] - o).astype(F32)
    z = c2ws[:, None, :3, 2]
    return (cen[None] + F32(TWO_SQRT3) * z).astype(F32), np.broadcast_to(-z, (B,) + cen.shape).astype(F32)


def plane_hits(verts, faces, ro, rd):
    """float64 Moeller-Trumbore of R rays against F triangles: (t, u, v) [R,F]; t is nan where the ray is parallel to the plane"""
    tri = np.asarray(verts, F64)[np.asarray(faces)]
    v0, e1, e2 = tri[:, 0], tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    ro, rd = np.asarray(ro, F64).reshape(-1, 3), np.asarray(rd, F64).reshape(-1, 3)
    p = np.cross(rd[:, None, :], e2[None])
    det = (e1[None] * p).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(det != 0, 1.0 / det, np.nan)
        tv = ro[:, None, :] - v0[None]
        u = (tv * p).sum(-1) * inv
        q = np.cross(tv, e1[None])
        v = (rd[:, None, :] * q).sum(-1) * inv
        t = (e2[None] * q).sum(-1) * inv
    return t, u, v


def closest_hit(verts, faces, ro, rd):
    """primitive id [R] int64 of the closest hit with t >= 0 (ties to the smallest id), -1 for a miss; and the rays that pass margin()"""
    t, u, v = plane_hits(verts, faces, ro, rd)
    with np.errstate(invalid="ignore"):
        inside = (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t >= 0)
    th = np.where(inside, t, np.inf)
    hit = np.argmin(th, axis=1)                      # the first of equal minima: the smallest id
    tw = th[np.arange(th.shape[0]), hit]
    hit = np.where(np.isfinite(tw), hit, -1)
    return hit, margin(t, u, v, inside, tw)


def margin(t, u, v, inside, t_win):
    """[R] bool: the winner leads every other hit by more than MARGIN in t, and every plane hit with t <= t_win + MARGIN (and t >= -MARGIN) is more
    than MARGIN away, in each of its three barycentrics, from an edge -- clearly inside or clearly outside -- and not within MARGIN of t = 0"""
    th = np.where(inside, t, np.inf)
    second = np.sort(th, axis=1)[:, 1] if th.shape[1] > 1 else np.full(th.shape[0], np.inf)
    lead = ~np.isfinite(t_win) | (second - t_win > MARGIN)
    with np.errstate(invalid="ignore"):
        near = np.isfinite(t) & (t >= -MARGIN) & (t <= (t_win + MARGIN)[:, None])
        w = 1.0 - u - v
        clear = (np.abs(u) > MARGIN) & (np.abs(v) > MARGIN) & (np.abs(w) > MARGIN)
        clear &= (np.abs(t) > MARGIN) | (u < 0) | (v < 0) | (w < 0)
    return lead & (clear | ~near).all(1)


def visible_faces_rays(verts, faces, c2ws, perspective):
    """(mask [B,F] bool, hit [B,F] int64, ok [B,F] bool): the scatter of the first-hit ids (structure.py:837-844) and the rays that pass margin()"""
    ro, rd = centroid_rays(verts, faces, c2ws, perspective)
    B, F = ro.shape[:2]
    hit, ok = closest_hit(verts, faces, ro, rd)
    hit, ok = hit.reshape(B, F), ok.reshape(B, F)
    mask = np.zeros((B, F + 1), bool)
    for b in range(B):
        mask[b, hit[b] + 1] = True
    return mask[:, 1:], hit, ok


def decided_faces(verts, faces, c2ws, perspective):
    """What the float64 reference decides about a float32 traversal's mask, face by face: (ref [B,F], must_set [B,F], may_differ [B,F], share).
    must_set: the faces that a margin-passing ray hits -- they have to be marked.  may_differ: the faces that a margin-FAILING ray could
    legitimately hit first instead of, or besides, its float64 winner: walking the ray's plane hits in the order of t, every face it possibly
    hits (each barycentric >= -MARGIN, t >= -MARGIN) up to MARGIN beyond the first face it certainly hits (each barycentric > MARGIN,
    t > MARGIN).  A mask `got` is right iff must_set <= got and got == ref on every face outside may_differ (see mask_agrees).  share: the
    fraction of margin-failing rays, from the float64 numbers alone."""
    ro, rd = centroid_rays(verts, faces, c2ws, perspective)
    B, F = ro.shape[:2]
    t, u, v = plane_hits(verts, faces, ro, rd)
    with np.errstate(invalid="ignore"):
        inside = (u >= 0) & (u <= 1) & (v >= 0) & (u + v <= 1) & (t >= 0)
    th = np.where(inside, t, np.inf)
    hit = np.argmin(th, axis=1)
    tw = th[np.arange(th.shape[0]), hit]
    hit = np.where(np.isfinite(tw), hit, -1)
    ok = margin(t, u, v, inside, tw)
    ref, must_set, may_differ = np.zeros((B, F), bool), np.zeros((B, F), bool), np.zeros((B, F), bool)
    w = 1.0 - u - v
    for r in range(B * F):
        b = r // F
        if hit[r] >= 0:
            ref[b, hit[r]] = True
        if ok[r]:
            if hit[r] >= 0:
                must_set[b, hit[r]] = True
            continue
        with np.errstate(invalid="ignore"):
            possible = np.isfinite(t[r]) & (u[r] >= -MARGIN) & (v[r] >= -MARGIN) & (w[r] >= -MARGIN) & (t[r] >= -MARGIN)
            certain = np.isfinite(t[r]) & (u[r] > MARGIN) & (v[r] > MARGIN) & (w[r] > MARGIN) & (t[r] > MARGIN)
        t_stop = t[r][certain].min() if certain.any() else np.inf
        may_differ[b] |= possible & (t[r] <= t_stop + MARGIN)
    return ref, must_set, may_differ, 1.0 - ok.mean()


def mask_agrees(got, ref, must_set, may_differ):
    """None if `got` is a mask the reference allows, else what is wrong with it"""
    got = np.asarray(got, bool)
    if not (got | ~must_set).all():
        return "%d faces that a margin-passing ray hits are not marked" % int((must_set & ~got).sum())
    wrong = (got != ref) & ~may_differ
    if wrong.any():
        return "%d faces outside the reach of the margin-failing rays differ: %d marked beyond the reference, %d missing" % (
            int(wrong.sum()), int((wrong & got).sum()), int((wrong & ~got).sum()))
    return None


def visible_faces_raster(rast, F):
    """renderer_base.py:77-81: the faces whose id + 1 appears in rast [B,H,W,4]"""
    rast = np.asarray(rast)
    mask = np.zeros((rast.shape[0], F + 1), bool)
    for b in range(rast.shape[0]):
        mask[b, rast[b, ..., 3].astype(np.int64).ravel()] = True
    return mask[:, 1:]


def erode_faces(mask, faces, V, depth):
    """erode_face (topology.py:12-25) row by row: a face stays set iff none of its vertices belongs to an unset face, `depth` times"""
    mask, faces = np.asarray(mask, bool).copy(), np.asarray(faces)
    for _ in range(max(int(depth), 0)):
        for b in range(mask.shape[0]):
            touched = np.zeros(V, bool)
            touched[faces[~mask[b]].ravel()] = True
            mask[b] &= ~touched[faces].any(1)
    return mask


def visible_vertices(mask, faces, V):
    mask, faces = np.asarray(mask, bool), np.asarray(faces)
    out = np.zeros((mask.shape[0], V), bool)
    for b in range(mask.shape[0]):
        out[b, faces[mask[b]].ravel()] = True
    return out


def uv_project(rast2d, faces, face_mask, v_ndc, map_attr=None, rast_map=None, mode="bilinear", background=None):
    """the table of utx_uv_project in the kernel's operation order (float32): dict of uv_alpha [B,H,W,1], uv [B,H,W,2] and, with a map
    [Bm,Hm,Wm,C] and rast_map [B,Hm,Wm,4], map_attr [B,H,W,C] and cov [B,H,W] bool (the looked-up coverage)"""
    rast2d, faces, face_mask = np.asarray(rast2d, F32), np.asarray(faces), np.asarray(face_mask).astype(bool)
    B = face_mask.shape[0]
    tri = rast2d[..., 3].astype(np.int64) - 1
    vis = (tri >= 0)[None] & face_mask[:, np.clip(tri, 0, None)]
    uv = np.stack([np.where(vis[b][..., None], interp(np.asarray(v_ndc[b], F32), rast2d, faces)[0], F32(-1.0)) for b in range(B)]).astype(F32)
    out = {"uv": uv, "uv_alpha": vis.astype(F32)[..., None]}
    if map_attr is None:
        return out
    map_attr = np.asarray(map_attr, F32)
    Bm, Hm, Wm, C = map_attr.shape
    assert Bm in (1, B)
    s = np.stack([sample(map_attr[b if Bm > 1 else 0], uv[b], mode) for b in range(B)]).astype(F32)
    covmap = (np.asarray(rast_map)[..., 3:4] > 0).astype(F32)
    cov = np.stack([sample(covmap[b], uv[b], "nearest")[..., 0] for b in range(B)]) >= 1.0
    alpha = vis & cov
    if background is None:
        texel00 = np.stack([map_attr[b if Bm > 1 else 0, 0, 0] for b in range(B)])[:, None, None, :]
        m = np.where(cov[..., None], s, texel00)
    else:
        m = np.where(alpha[..., None], s, np.broadcast_to(np.asarray(background, F32), s.shape))
    out.update(map_attr=m.astype(F32), uv_alpha=alpha.astype(F32)[..., None], cov=cov)
    return out


# ---- fixture G19 and its cases
SETS = (("p", True), ("o", False))
ATLAS = (48, 40)
RASTER_SIZE = (40, 56)
B = 3
# (fixture key without the set, map index, per-view map, mode, background key or None)
BACKGROUNDS = (("map_0_1_bilinear_float", 0, False, "bilinear", "bg_float"), ("map_1_b_nearest_vec", 1, True, "nearest", "bg_vec_5"),
               ("map_0_b_nvdiffrast_dense", 0, True, "nvdiffrast", "bg_dense_3"), ("map_1_1_bilinear_vec", 1, False, "bilinear", "bg_vec_5"))
_FIX = {}


def load():
    """the fixture, read once and shared (the arrays are never written to)"""
    if not _FIX:
        with np.load(os.path.join(GOLD, "g19_uv_project.npz"), allow_pickle=False) as f:
            _FIX.update({k: f[k] for k in f.files})
        for v in _FIX.values():
            v.setflags(write=False)
    return _FIX


def cases(f, tag):
    """every stored map_attr of a camera set: (fixture key, map [Bm,Hm,Wm,C], map index, mode, background or None)"""
    out = []
    for i in (0, 1):
        for per_view in (False, True):
            for mode in MODES:
                out.append(("map_%d_%s_%s_%s" % (i, "b" if per_view else "1", mode, tag), f["map_%d" % i][:None if per_view else 1], i, mode, None))
    for key, i, per_view, mode, bg in BACKGROUNDS:
        out.append(("%s_%s" % (key, tag), f["map_%d" % i][:None if per_view else 1], i, mode, f[bg]))
    return out


def check_map(name, got, ref, mode, m):
    """bit-exact, or within MAP_BOUND for 'bilinear'; returns the largest deviation in u"""
    assert got.shape == ref.shape and got.dtype == ref.dtype == F32, (name, got.shape, ref.shape)
    d = np.abs(got.astype(F64) - ref.astype(F64))
    print("%s: max|diff| %.3g = %.2f u" % (name, d.max(), d.max() / U))
    if mode == "bilinear":
        for b in range(d.shape[0]):      # each view against the bound of the map it sampled
            bound = map_bound(mode, [m[b if m.shape[0] > 1 else 0]])
            assert (d[b] <= bound).all(), "%s view %d: %.2f u over a bound of %.2f u" % (name, b, d[b].max() / U, bound.max() / U)
    else:
        assert got.tobytes() == ref.tobytes(), "%s: max|diff| %.3g" % (name, d.max())
    return d.max() / U

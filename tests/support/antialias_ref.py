"""Numpy restatements of silhouette antialiasing (DESIGN 8 "Silhouette antialiasing", unitex_amd/csrc/antialias.hip), shared by the CPU and GPU tests, the
fixture generator tests/golden/make_golden_antialias.py and tools/bench_antialias.py.

One pixel pair at a time: p = (px, py) and q = p + (1, 0) (horizontal) or p + (0, 1) (vertical), both inside one view.  With a dtype argument: float32 follows
the kernel's operation order (every operation one rounded operation on numpy float32 scalars), float64 is the yardstick.
 (a) ip = int(rast[p].w) - 1, iq likewise; ip == iq: nothing.
 (b) far_p = ip < 0 or (iq >= 0 and rast[p].z > rast[q].z); t = iq if far_p else ip; t outside [0, F) or a vertex index of t outside [0, V): nothing.
 (c) per vertex (x, y, ., w) of t: not (x, y, w finite and w > 0): nothing.  cx = px + 0.5, cy = py + 0.5;
       sx = ((x / w) * 0.5 + 0.5) * W - cx,  sy = ((y / w) * 0.5 + 0.5) * H - cy;  (X, Y) = (sx, sy) for a horizontal pair, (sy, sx) for a vertical one.
 (d) edge e = (a, b) = (k, (k + 1) % 3) for e = 0, 1, 2: straddles if (Ya < 0) != (Yb < 0); d = (Xa * Yb - Xb * Ya) / (Yb - Ya); candidate if 0 <= d <= 1.
     The smallest d if t == ip, the largest if t == iq; a later edge replaces an earlier one only when strictly smaller / larger.  No candidate: nothing.
 (e) c = (k + 2) % 3; own = (Xb - Xa) * (Yc - Ya) - (Yb - Ya) * (Xc - Xa); own neither < 0 nor > 0: nothing.  o = opp[t][e]: a silhouette edge if o < 0,
     o >= V or o fails the test of (c); otherwise wing = (Xb - Xa) * (Yo - Ya) - (Yb - Ya) * (Xo - Xa) and the surface continues (nothing) exactly if own
     and wing have strictly opposite signs.
 (f) d < 0.5: p takes the weight 0.5 - d towards q;  d > 0.5: q takes d - 0.5 towards p;  d == 0.5: nothing.
weights[p] = (left, right, up, down);  out[p] = (((color[p] + k_left) + k_right) + k_up) + k_down with k_n = w_n * (color[n] - color[p]) where w_n != 0, else +0.

MISTAKES names six planted mistakes (the `mistake` argument) that tests/test_antialias_cpu.py shows the exact cases to reject."""
import os

import numpy as np

F32, F64 = np.float32, np.float64
MISTAKES = ("near", "no_swap", "d_from_q", "wing_sign", "no_border", "order")


# ---- topology, restated with a dict of edges (meshes.edge_opposites sorts keys and goes through face_adjacency)
def edge_opposites(faces):
    faces = np.asarray(faces)
    seen = {}
    for f, tri in enumerate(faces.tolist()):
        for e in range(3):
            a, b = tri[e], tri[(e + 1) % 3]
            seen.setdefault((min(a, b), max(a, b)), []).append((f, e))
    opp = -np.ones((len(faces), 3), np.int32)
    for users in seen.values():
        if len(users) < 2:
            continue
        (f0, e0), (f1, e1) = users[0], users[1]      # the first two faces link, the others keep -1
        for (f, e), (g, _) in (((f0, e0), (f1, e1)), ((f1, e1), (f0, e0))):
            ends = (faces[f][e], faces[f][(e + 1) % 3])
            rest = [v for v in faces[g].tolist() if v not in ends]
            opp[f, e] = rest[0] if rest else -1
    return opp


# ---- the rule
def _project(v, Wd, Hd, cx, cy, vertical, ft, swap=True):
    x, y, w = ft(v[0]), ft(v[1]), ft(v[3])
    if not (np.isfinite(x) and np.isfinite(y) and np.isfinite(w) and w > 0):
        return None
    half = ft(0.5)
    sx = ((x / w) * half + half) * ft(Wd) - cx
    sy = ((y / w) * half + half) * ft(Hd) - cy
    return (sy, sx) if (vertical and swap) else (sx, sy)


def pair(rast, pos, tri, opp, px, py, vertical, ft=F32, mistake=None):
    """the pair whose first pixel is (px, py) in one view (rast [H,W,4], pos [V,4]) -> (d or None, (t, e, silhouette)): d is the crossing where the pair
    contributes; the decisions are None from the step at which the rule stops"""
    H, W = rast.shape[:2]
    F, V = len(tri), len(pos)
    qx, qy = (px, py + 1) if vertical else (px + 1, py)
    ip, iq = int(rast[py, px, 3]) - 1, int(rast[qy, qx, 3]) - 1
    if ip == iq:
        return None, (None, None, None)
    far_p = ip < 0 or (iq >= 0 and rast[py, px, 2] > rast[qy, qx, 2])
    if mistake == "near":
        far_p = ip < 0 or (iq >= 0 and not rast[py, px, 2] > rast[qy, qx, 2])
    t = iq if far_p else ip
    if t < 0 or t >= F:
        return None, (None, None, None)
    idx = [int(i) for i in tri[t]]
    if any(i < 0 or i >= V for i in idx):
        return None, (t, None, None)
    cx, cy = ft(px) + ft(0.5), ft(py) + ft(0.5)
    swap = mistake != "no_swap"
    P = [_project(pos[i], W, H, cx, cy, vertical, ft, swap) for i in idx]
    if any(p is None for p in P):
        return None, (t, None, None)
    zero, one = ft(0.0), ft(1.0)
    best_d, best_e = None, -1
    with np.errstate(all="ignore"):
        for e in range(3):
            (Xa, Ya), (Xb, Yb) = P[e], P[(e + 1) % 3]
            if (Ya < zero) != (Yb < zero):
                d = (Xa * Yb - Xb * Ya) / (Yb - Ya)
                if d >= zero and d <= one and (best_e < 0 or (d > best_d if far_p else d < best_d)):
                    best_d, best_e = d, e
        if best_e < 0:
            return None, (t, None, None)
        e = best_e
        (Xa, Ya), (Xb, Yb), (Xc, Yc) = P[e], P[(e + 1) % 3], P[(e + 2) % 3]
        ex, ey = Xb - Xa, Yb - Ya
        own = ex * (Yc - Ya) - ey * (Xc - Xa)
        if not (own < zero or own > zero):
            return None, (t, e, None)
        o = int(opp[t, e])
        sil = True
        if o < 0 and mistake == "no_border":
            sil = False
        if 0 <= o < V:
            Po = _project(pos[o], W, H, cx, cy, vertical, ft, swap)
            if Po is not None:
                wing = ex * (Po[1] - Ya) - ey * (Po[0] - Xa)
                if mistake == "wing_sign":
                    wing = -wing
                if (own > zero and wing < zero) or (own < zero and wing > zero):
                    sil = False
    if not sil:
        return None, (t, e, False)
    if mistake == "d_from_q":
        best_d = one - best_d
    return best_d, (t, e, True)


def weights(rast, pos, tri, opp, ft=F32, mistake=None):
    """rast [B,H,W,4], pos [V,4] or [B,V,4] -> (weights [B,H,W,4] of ft, decisions {(b, px, py, vertical): (t, e, silhouette)} of the pairs with ip != iq)"""
    rast = np.asarray(rast, F32)
    B, H, W = rast.shape[:3]
    out = np.zeros((B, H, W, 4), ft)
    dec = {}
    ids = rast[..., 3].astype(np.int64)
    half = ft(0.5)
    for vertical in (False, True):
        differ = (ids[:, 1:, :] != ids[:, :-1, :]) if vertical else (ids[:, :, 1:] != ids[:, :, :-1])
        for b, py, px in zip(*np.nonzero(differ)):
            b, py, px = int(b), int(py), int(px)
            d, decision = pair(rast[b], pos[b] if np.ndim(pos) == 3 else pos, tri, opp, px, py, vertical, ft, mistake)
            dec[(b, px, py, vertical)] = decision
            if d is None:
                continue
            qx, qy = (px, py + 1) if vertical else (px + 1, py)
            if d < half:
                out[b, py, px, 3 if vertical else 1] = half - d      # p: its down / right weight
            elif d > half:
                out[b, qy, qx, 2 if vertical else 0] = d - half      # q: its up / left weight
    return out, dec


def apply(color, w, ft=F32, mistake=None):
    """color [B,H,W,C], w [B,H,W,4] -> out, the fixed order left, right, up, down per channel (vectorised over the image: every element sees the same
    scalar operations in the same order)"""
    c = np.asarray(color, ft)
    w = np.asarray(w, ft)
    B, H, W, _ = c.shape
    nb = np.zeros((4,) + c.shape, ft)      # the neighbour's colour where it exists
    nb[0, :, :, 1:], nb[1, :, :, :-1], nb[2, :, 1:], nb[3, :, :-1] = c[:, :, :-1], c[:, :, 1:], c[:, :-1], c[:, 1:]
    inside = np.zeros((4, B, H, W, 1), bool)
    inside[0, :, :, 1:], inside[1, :, :, :-1], inside[2, :, 1:], inside[3, :, :-1] = True, True, True, True
    out = c.copy()
    with np.errstate(all="ignore"):
        for n in ((3, 2, 1, 0) if mistake == "order" else (0, 1, 2, 3)):
            wn = w[..., n:n + 1]
            k = np.where((wn != 0) & inside[n], wn * (nb[n] - c), ft(0.0)).astype(ft)
            out = (out + k).astype(ft)
    return out


def _batched(color, rast):
    color, rast = np.asarray(color), np.asarray(rast)
    return (color[None], rast[None], True) if rast.ndim == 3 else (color, rast, False)


def antialias_f32(color, rast, pos, tri, opp=None, mistake=None):
    """sequential numpy float32 in the kernel's operation order"""
    color, rast, squeeze = _batched(color, rast)
    w, _ = weights(rast, pos, tri, edge_opposites(tri) if opp is None else opp, F32, mistake)
    out = apply(color, w, F32, mistake)
    return out[0] if squeeze else out


def antialias_f64(color, rast, pos, tri, opp=None):
    """the same rule in float64 -> (out, decisions per pair)"""
    color, rast, squeeze = _batched(color, rast)
    w, dec = weights(rast, pos, tri, edge_opposites(tri) if opp is None else opp, F64)
    out = apply(color, w, F64)
    return (out[0] if squeeze else out), dec


def compare_f32_f64(color, rast, pos, tri, opp):
    """-> (pixels that receive a contribution, pixels excluded because a pair that touches them decides differently, max |f32 - f64| over the rest)"""
    color, rast, _ = _batched(color, rast)
    w32, d32 = weights(rast, pos, tri, opp, F32)
    w64, d64 = weights(rast, pos, tri, opp, F64)
    B, H, W = rast.shape[:3]
    excluded = np.zeros((B, H, W), bool)
    for key in d32:
        if d32[key] != d64[key]:
            b, px, py, vertical = key
            excluded[b, py, px] = True
            excluded[(b, py + 1, px) if vertical else (b, py, px + 1)] = True
    receives = ((w32 != 0).any(-1)) | ((w64 != 0).any(-1))
    diff = np.abs(apply(color, w32, F32).astype(F64) - apply(color, w64, F64)).max(-1)
    rest = ~excluded
    return int(receives.sum()), int((excluded & receives).sum()), float(diff[rest].max()) if rest.any() else 0.0


# ---- the cases
def _rasterize(pos, tri, H, W):
    from oracle import geom_ref
    return geom_ref.rasterize(pos, tri, H, W)


def _icosphere():
    """the 80-face sphere: an icosahedron subdivided once, on the unit sphere"""
    from unitex_amd.texturetools import meshes
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, g, 0], [1, g, 0], [-1, -g, 0], [1, -g, 0], [0, -1, g], [0, 1, g], [0, -1, -g], [0, 1, -g], [g, 0, -1], [g, 0, 1], [-g, 0, -1],
                  [-g, 0, 1]], np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8], [3, 9, 4], [3, 4, 2],
                  [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], np.int32)
    v, f = meshes.subdivide_midpoint(v.astype(np.float32), f)
    v = v.astype(np.float64)
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v, np.ascontiguousarray(f, np.int32)


def _view(verts, angle, perspective):
    """clip-space [V,4] of world vertices seen after a turn about y (and a tilt): x, y scaled into the screen, z / w in (-1, 1)"""
    c, s = np.cos(angle), np.sin(angle)
    R = np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]]) @ np.array([[1, 0, 0], [0, np.cos(0.37), -np.sin(0.37)], [0, np.sin(0.37), np.cos(0.37)]])
    p = verts @ R.T
    w = (2.8 - p[:, 2]) if perspective else np.ones(len(p))
    k = 2.1 if perspective else 0.83
    return np.stack([k * p[:, 0] + 0.043 * w, k * p[:, 1] - 0.031 * w, -0.3 * p[:, 2] * w, w], 1).astype(F32)


CASES = ("triangle", "fan", "folded", "quads", "sphere", "sphere_w", "bad_index", "empty")
ANGLES = (0.3, 1.7, 4.1)


def render_case(name, H, W, B=1, per_view=False, C=3, seed=0):
    """one of CASES on a screen of H x W, B views -> dict(rast [B,H,W,4], pos [V,4] (shared; the views then show one raster) or [B,V,4] (per_view), tri, opp,
    color [B,H,W,C]); the rasters come from the CPU rasteriser the golden generators use (oracle/geom_ref.c)"""
    perspective = name in ("sphere", "sphere_w", "bad_index")
    if name == "triangle":
        verts, tri = np.array([[-0.71, -0.62, 0.1], [0.83, -0.33, -0.2], [-0.12, 0.77, 0.3]]), np.array([[0, 1, 2]], np.int32)
    elif name == "fan":      # three faces on the edge (0, 1): the first two link, the third gets -1
        verts = np.array([[-0.1, -0.8, 0.0], [0.15, 0.85, 0.0], [0.9, 0.1, 0.3], [-0.85, -0.05, 0.2], [0.6, 0.5, -0.6]])
        tri = np.array([[0, 1, 2], [1, 0, 3], [0, 1, 4]], np.int32)
    elif name == "folded":      # the wing (1, 0, 3) lies on the triangle's own side of the shared edge, behind it
        verts = np.array([[-0.3, -0.8, 0.0], [0.1, 0.85, 0.0], [0.9, 0.05, 0.1], [0.55, -0.2, -0.7]])
        tri = np.array([[0, 1, 2], [1, 0, 3]], np.int32)
    elif name == "quads":      # a near quad in front of a larger far one
        verts = np.array([[-0.42, -0.37, 0.5], [0.47, -0.31, 0.5], [0.41, 0.44, 0.5], [-0.36, 0.39, 0.5],
                          [-0.83, -0.78, -0.5], [0.86, -0.81, -0.5], [0.79, 0.84, -0.5], [-0.88, 0.76, -0.5]])
        tri = np.array([[0, 1, 2], [0, 2, 3], [4, 5, 6], [4, 6, 7]], np.int32)
    elif name == "empty":
        verts, tri = np.array([[3.0, 3.0, 0.0], [4.0, 3.0, 0.0], [3.0, 4.0, 0.0]]), np.array([[0, 1, 2]], np.int32)
    else:
        verts, tri = _icosphere()
        verts = 0.93 * verts
    views = [_view(np.asarray(verts, np.float64), a if (per_view or perspective) else 0.0, perspective) for a in ANGLES[:B]]
    if not perspective and not per_view:      # flat cases: the coordinates above are the screen's own
        views = [np.concatenate([np.asarray(verts, F32)[:, :2], -np.asarray(verts, F32)[:, 2:3], np.ones((len(verts), 1), F32)], 1)] * B
    if not per_view:
        views = [views[0]] * B
    pos = np.stack(views).astype(F32)
    tri = tri.copy()
    if name == "sphere_w":      # the vertex nearest to the first camera gets w <= 0: its faces are never drawn, so it is reachable only as an opp
        bad = int(np.argmin(pos[0, :, 2] / pos[0, :, 3]))
        pos[:, bad, 3] = -1.0
    rast = np.stack([_rasterize(pos[b], tri, H, W) for b in range(B)])
    if name == "bad_index":      # a face no pixel of any view shows, next to one that is shown: its far vertex becomes an index >= V
        shown = np.zeros(len(tri), bool)
        ids = rast[..., 3].astype(np.int64)
        shown[ids[ids > 0] - 1] = True
        from unitex_amd.texturetools import meshes
        adj = meshes.face_adjacency(tri)
        pick = [(f, e) for f in range(len(tri)) if not shown[f] for e in range(3) if adj[f, e] >= 0 and shown[adj[f, e]]]
        if pick:
            f, e = pick[0]
            tri[f, (e + 2) % 3] = len(verts) + 5
        else:      # a screen too small to hide a face next to a shown one: any hidden face
            f = int(np.nonzero(~shown)[0][0])
            tri[f, 2] = len(verts) + 5
    rng = np.random.default_rng(seed + 1000 * H + W)
    color = rng.uniform(-1.0, 1.0, (B, H, W, C)).astype(F32)
    return dict(rast=rast, pos=pos if per_view else pos[0], tri=tri, opp=edge_opposites(tri), color=color)


# ---- fixture G27 (tests/golden/make_golden_antialias.py): the reference's own simple_rendering(enable_antialis=True) with dr.antialias bound to antialias_f32
G27 = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden", "g27_antialias.npz")
G27_SCREEN = (48, 40)      # (H, W)
G27_VIEWS = 2
G27_GEOMETRY = ("z_depth", "world_normal", "camera_normal", "world_position", "camera_position", "distance", "ray_direction", "cos_ray_normal")
G27_BG_FLOAT = 0.25
_G27 = {}


def g27_scene():
    """the 80-face sphere with one fin (a triangle of border edges in front of the surface), unit vertex normals, spherical UVs, a 4-channel vertex attribute
    and a 16 x 24 x 3 map (values rounded to half precision) -> verts, faces, uvs, v_nrm, v_attr, map"""
    verts, faces = _icosphere()
    verts = 0.8 * verts
    fin = np.array([[0.0, 0.0, 0.8], [0.5, 0.9, 1.0], [-0.6, 0.7, 1.0]])
    faces = np.concatenate([faces, [[len(verts), len(verts) + 1, len(verts) + 2]]]).astype(np.int32)
    verts = np.concatenate([verts, fin]).astype(F32)
    nrm = (verts / np.linalg.norm(verts, axis=1, keepdims=True)).astype(F32)
    uvs = np.stack([np.arctan2(nrm[:, 0], nrm[:, 2]) / (2 * np.pi) + 0.5, np.arccos(np.clip(nrm[:, 1], -1, 1)) / np.pi], 1).astype(F32)
    rng = np.random.default_rng(27)
    v_attr = rng.uniform(-1, 1, (len(verts), 4)).astype(np.float16).astype(F32)
    return verts, faces, uvs, nrm, v_attr, rng.uniform(0, 1, (16, 24, 3)).astype(np.float16).astype(F32)


def load_g27():
    """the fixture, read once and shared (the arrays are never written to)"""
    if not _G27:
        with np.load(G27, allow_pickle=False) as f:
            _G27.update({k: f[k] for k in f.files})
        for v in _G27.values():
            v.setflags(write=False)
    return _G27

"""Nearest-surface queries (TEST INFRASTRUCTURE ONLY): the numpy restatement that tests/test_closest_point_gpu.py and tests/test_spatial_sampling_gpu.py hold
the HIP kernels to, the float64 brute force they are both bounded against, and the test meshes.  tests/test_closest_point_cpu.py pins them first, without a
GPU.  The sampling built on the queries is restated in oracle/sampling_ref.py.

tri_closest_f32 repeats csrc/bvh_device.h::tri_closest operation for operation in float32 (numpy rounds every product and sum on its own, as the kernel does
without contraction): the Voronoi-region form of Ericson, Real-Time Collision Detection, 5.1.5.  brute_f64 is NOT that formula: it drops p onto the face's plane,
keeps the foot if it lies inside the three edge half-planes, and otherwise takes the nearest of the three edge segments, all in float64 -- so the two do not
share a mistake.

The bound on | |p - q32| - d64 |.  Write u = 2^-24, S = max|p| + max|v| (every difference and every length below is at most S), L for the edge lengths.
  (a) evaluating the distance for GIVEN weights: q = (u a + v b) + w c is three products and two sums with weights in [0, 1] -- at most 4 u max|v| per
      component; r = p - q one more rounding, u |r|: at most 5 u S per component, sqrt(3) * 5 u S < 9 u S for the vector.  d2 = (rx^2 + ry^2) + rz^2: three
      products and two sums of positive terms, relative 3 u on d2, 1.5 u on its root, plus 0.5 u for sqrtf: 2 u S.  Together 11 u S.
  (b) the weights themselves.  ab, ap, ... are one rounding each; a dot3 is three products and two sums: d1..d6 carry at most 5 u |e||x|.  va, vb, vc are two
      products of two d's and a difference: (2 * 11 + 1) u = 23 u L^2 |x|^2.  A quotient adds u.  So a weight is off by at most dw = 24 u |x|^2 / (L^2 sin^2 A)
      (A the face's smallest angle; the edge regions divide one d by a difference of two: 11 u |x| / L, smaller), and q is off by at most L dw along the face --
      and never by more than L, because the weights are clamped to the face.  A misjudged region boundary moves q by the same amount, for the same reason.
      Near the surface (|x| <= 2 L, d ~ 0) that is 96 u L / sin^2 A <= 48 u S / sin^2 A, in full.  Away from it q32 moves ALONG the face while p - q* is normal to
      the feature q* lies on, so the distance changes in second order only: min(L, L dw)^2 / (2 d) <= 12 u S / sin^2 A at the worst |x| / L.
  With sin^2 A >= 1/4 (every face of the meshes below that has an area; a face without one is resolved by segment parameters alone, case (a) plus 11 u S):
      | |p - q32| - d64 |  <=  11 u S + 4 * 48 u S + 4 * 12 u S  <  256 u S  =  BOUND_U * u * S.
The same bound holds for the float64 distance from p to the returned face (it is at most |p - q32| + (a) and at least d64) and for |p - sum uvw_k v_k| evaluated
in float64 (the returned dist without the roundings of (a))."""
import numpy as np

F32 = np.float32
U = 2.0 ** -24
BOUND_U = 256.0


def scene_scale(points, verts):
    p = np.asarray(points, np.float64)
    p = p[np.isfinite(p).all(1)]
    return (np.abs(p).max() if len(p) else 0.0) + np.abs(np.asarray(verts, np.float64)).max()


# ---- float32 restatement of tri_closest, vectorised over points x faces ----
def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _div(n, d):
    with np.errstate(all="ignore"):
        return np.where(d > 0, n / np.where(d > 0, d, F32(1)), F32(0)).astype(F32)


def _eval(p, a, b, c, u, v, w):
    r = p - ((u[..., None] * a + v[..., None] * b) + w[..., None] * c)
    return _dot(r, r)


def _seg_t(xp, e):
    return np.minimum(np.maximum(_div(_dot(xp, e), _dot(e, e)), F32(0)), F32(1))


def tri_closest_f32(p, a, b, c):
    """p, a, b, c broadcastable [..., 3] float32 -> d2, u, v, w [...] float32"""
    p, a, b, c = (np.asarray(x, F32) for x in (p, a, b, c))
    p, a, b, c = np.broadcast_arrays(p, a, b, c)
    one, zero = F32(1), F32(0)
    with np.errstate(all="ignore"):
        ab, ac, bc, ap, bp, cp = b - a, c - a, c - b, p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = _dot(ab, ap), _dot(ac, ap), _dot(ab, bp), _dot(ac, bp), _dot(ab, cp), _dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        Z, O = np.zeros_like(d1), np.ones_like(d1)
        # the last branch first: the interior; and the three-segment answer, taken at the very end where the denominator is not > 0
        den = (va + vb) + vc
        inv = one / np.where(den > 0, den, one)
        vi = np.minimum(np.maximum(vb * inv, zero), one)
        wi = np.minimum(np.maximum(vc * inv, zero), one - vi)
        ui = (one - vi) - wi
        t0, t1, t2 = _seg_t(ap, ab), _seg_t(ap, ac), _seg_t(bp, bc)
        e0, e1, e2 = _eval(p, a, b, c, one - t0, t0, Z), _eval(p, a, b, c, one - t1, Z, t1), _eval(p, a, b, c, Z, one - t2, t2)
        us, vs, ws, e = one - t0, t0, Z, e0
        k1 = e1 < e
        us, vs, ws, e = np.where(k1, one - t1, us), np.where(k1, zero, vs), np.where(k1, t1, ws), np.where(k1, e1, e)
        k2 = e2 < e
        us, vs, ws = np.where(k2, zero, us), np.where(k2, one - t2, vs), np.where(k2, t2, ws)
        u, v, w = ui, vi, wi
        # then the regions in reverse priority, so that the first that holds wins
        wbc = _div(d4 - d3, (d4 - d3) + (d5 - d6))
        m = (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)
        u, v, w = np.where(m, Z, u), np.where(m, one - wbc, v), np.where(m, wbc, w)
        wac = _div(d2, d2 - d6)
        m = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        u, v, w = np.where(m, one - wac, u), np.where(m, Z, v), np.where(m, wac, w)
        m = (d6 >= 0) & (d5 <= d6)
        u, v, w = np.where(m, Z, u), np.where(m, Z, v), np.where(m, O, w)
        vab = _div(d1, d1 - d3)
        m = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        u, v, w = np.where(m, one - vab, u), np.where(m, vab, v), np.where(m, Z, w)
        m = (d3 >= 0) & (d4 <= d3)
        u, v, w = np.where(m, Z, u), np.where(m, O, v), np.where(m, Z, w)
        m = (d1 <= 0) & (d2 <= 0)
        u, v, w = np.where(m, O, u), np.where(m, Z, v), np.where(m, Z, w)
        flat = ~(den > 0)                           # no area: the regions mean nothing, the three segments decide
        u, v, w = np.where(flat, us, u), np.where(flat, vs, v), np.where(flat, ws, w)
        u, v, w = u.astype(F32), v.astype(F32), w.astype(F32)
        return _eval(p, a, b, c, u, v, w).astype(F32), u, v, w


def closest_point_f32(points, verts, faces, chunk=4096):
    """the exhaustive query as utx_bvh_closest_point defines it -> dist [N] f32, d2 [N] f32, face [N] i32, uvw [N,3] f32, closest [N,3] f32"""
    points, verts = np.asarray(points, F32).reshape(-1, 3), np.asarray(verts, F32)
    faces = np.asarray(faces).reshape(-1, 3)
    N = len(points)
    d2o, fo = np.full(N, np.inf, F32), np.full(N, -1, np.int32)
    uvw, q = np.zeros((N, 3), F32), np.zeros((N, 3), F32)
    a, b, c = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    for s in range(0, N, chunk):
        p = points[s:s + chunk]
        d2, u, v, w = tri_closest_f32(p[:, None, :], a[None], b[None], c[None])
        key = np.where(np.isnan(d2), F32(np.inf), d2)
        f = np.argmin(key, axis=1)                                # the first (smallest id) minimum
        r = np.arange(len(p))
        ok = np.isfinite(p).all(1) & (key[r, f] < np.inf)
        d2o[s:s + chunk] = np.where(ok, d2[r, f], F32(np.inf))
        fo[s:s + chunk] = np.where(ok, f, -1)
        w3 = np.stack([u[r, f], v[r, f], w[r, f]], -1)
        uvw[s:s + chunk] = np.where(ok[:, None], w3, F32(0))
        with np.errstate(all="ignore"):
            qq = (w3[:, 0:1] * a[f] + w3[:, 1:2] * b[f]) + w3[:, 2:3] * c[f]
        q[s:s + chunk] = np.where(ok[:, None], qq, F32(0))
    return np.sqrt(d2o), d2o, fo, uvw, q


# ---- float64 brute force, by another formula ----
def _seg_d64(p, a, b):
    e, x = b - a, p - a
    ee = (e * e).sum(-1)
    t = np.clip(np.where(ee > 0, (x * e).sum(-1) / np.where(ee > 0, ee, 1.0), 0.0), 0.0, 1.0)
    return np.linalg.norm(x - t[..., None] * e, axis=-1)


def tri_dist_f64(p, a, b, c):
    """distance from p to triangle (a, b, c), broadcastable [..., 3], in float64: foot of the perpendicular if inside, else the nearest edge segment"""
    p, a, b, c = np.broadcast_arrays(*(np.asarray(x, np.float64) for x in (p, a, b, c)))
    n = np.cross(b - a, c - a)
    nn = (n * n).sum(-1)
    has = nn > 0
    h = ((p - a) * n).sum(-1) / np.where(has, nn, 1.0)
    foot = p - h[..., None] * n
    inside = has
    for s, e in ((a, b), (b, c), (c, a)):
        inside = inside & ((np.cross(e - s, foot - s) * n).sum(-1) >= 0)
    edge = np.minimum(np.minimum(_seg_d64(p, a, b), _seg_d64(p, b, c)), _seg_d64(p, c, a))
    return np.where(inside, np.minimum(np.abs(h) * np.sqrt(nn), edge), edge)


def brute_f64(points, verts, faces, chunk=4096):
    """-> d64 [N]: the distance from every (finite) point to the mesh; +inf for a point with a non-finite coordinate"""
    points, verts = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(verts, np.float64)
    faces = np.asarray(faces).reshape(-1, 3)
    a, b, c = verts[faces[:, 0]], verts[faces[:, 1]], verts[faces[:, 2]]
    out = np.full(len(points), np.inf)
    fin = np.isfinite(points).all(1)
    idx = np.flatnonzero(fin)
    for s in range(0, len(idx), chunk):
        j = idx[s:s + chunk]
        out[j] = tri_dist_f64(points[j][:, None, :], a[None], b[None], c[None]).min(1)
    return out


def brute_f64_face(points, verts, faces, margin):
    """-> (d64 [N], face [N], alone [N]) for finite points: the float64 distance, the face attaining it (smallest id), and whether that face is the only one
    within `margin` of it.  Where it is not -- outside a convex edge both faces of the edge are at the same distance, up to rounding -- float64 and float32 may
    each name either, and only the distance can be compared"""
    points, verts = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(verts, np.float64)
    faces = np.asarray(faces).reshape(-1, 3)
    d = tri_dist_f64(points[:, None, :], verts[faces[:, 0]][None], verts[faces[:, 1]][None], verts[faces[:, 2]][None])
    best = d.min(1)
    return best, d.argmin(1).astype(np.int32), (d <= best[:, None] + margin).sum(1) == 1


def face_dist_f64(points, verts, faces, face):
    """float64 distance from point i to the one face face[i]"""
    verts, f = np.asarray(verts, np.float64), np.asarray(faces).reshape(-1, 3)[face]
    return tri_dist_f64(np.asarray(points, np.float64), verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]])


# ---- the meshes of the tests ----
def icosphere(level=1):
    """unit icosphere: 20 * 4^level faces (80 at level 1)"""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        cache, nf = {}, []

        def mid(i, j):
            k = (min(i, j), max(i, j))
            if k not in cache:
                m = v[i] + v[j]
                v.append(m / np.linalg.norm(m))
                cache[k] = len(v) - 1
            return cache[k]
        for a, b, c in f:
            ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v, F32), np.array(f, np.int32)


def grid4():
    """a 4 x 4 planar grid of squares (32 faces) with dyadic coordinates: every product and sum of tri_closest is exact, so distances TIE exactly among the up to
    six faces around a vertex"""
    g = np.arange(5, dtype=F32) * F32(0.25)
    v = np.stack([np.repeat(g, 5), np.tile(g, 5), np.full(25, 0.5, F32)], -1)
    f = []
    for i in range(4):
        for j in range(4):
            a, b, c, d = 5 * i + j, 5 * i + j + 1, 5 * (i + 1) + j, 5 * (i + 1) + j + 1
            f += [(a, b, d), (a, d, c)]
    return v, np.array(f, np.int32)


def mesh(name):
    if name == "one":
        return np.array([[0, 0, 0], [1, 0, 0], [0.25, 0.75, 0.5]], F32), np.array([[0, 1, 2]], np.int32)
    if name == "two":
        return np.array([[0, 0, 0], [1, 0, 0], [0.25, 0.75, 0.5], [0.75, -0.5, 0.25]], F32), np.array([[0, 1, 2], [1, 0, 3]], np.int32)
    if name == "tetra":
        return np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], F32) * F32(0.5), np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32)
    if name == "ico":
        return icosphere(1)
    if name == "grid":
        return grid4()
    if name == "ico_degenerate":          # + one face of no area (a repeated corner) and one face twice
        v, f = icosphere(1)
        return v, np.concatenate([f, [[f[3, 0], f[3, 1], f[3, 1]]], f[17:18]]).astype(np.int32)
    raise KeyError(name)


MESHES = ["one", "two", "tetra", "ico", "grid", "ico_degenerate"]


def queries(name, N):
    """N query points for mesh `name`: its own vertices and edge midpoints (exact ties on the dyadic grid), face interiors, points inside the bounding box, points
    10^3 away, and -- from N = 63 on -- one point with a NaN and one with an inf"""
    v, f = mesh(name)
    rng = np.random.default_rng(1000 * MESHES.index(name) + N)
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    mids = (v[e[:, 0]] + v[e[:, 1]]) * F32(0.5)
    bw = rng.dirichlet(np.ones(3), len(f)).astype(F32)
    inner = (bw[:, 0:1] * v[f[:, 0]] + bw[:, 1:2] * v[f[:, 1]]) + bw[:, 2:3] * v[f[:, 2]]
    lo, hi = v.min(0), v.max(0)
    box = (lo + (hi - lo) * rng.random((64, 3))).astype(F32)
    d = rng.normal(size=(32, 3))
    far = (1000.0 * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)
    groups = [v, mids, inner, box, far]
    pts = []
    k = 0
    while len(pts) < N:                    # round robin, so that a small N still sees every kind
        for g in groups:
            if k < len(g) and len(pts) < N:
                pts.append(g[k])
        k += 1
        if k > max(len(g) for g in groups):
            pts.append(box[len(pts) % len(box)] * F32(0.5))
    pts = np.array(pts[:N], F32)
    if N >= 63:
        pts[7, 1] = np.nan
        pts[N - 2, 2] = np.inf
    return pts

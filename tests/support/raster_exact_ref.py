"""An independent restatement of the rasteriser's rule (utx_rasterize / utx_interpolate), and the case sets that pin it.

Nothing here touches oracle/geom_ref or ctypes: numpy float32 for the float steps, Python integers (or numpy int64 under an
asserted magnitude bound) for the integer steps, fractions.Fraction for the exact values.

The rule, per triangle f = 0 .. F-1 of tri [F][3] over pos [V][4] (clip space x, y, z, w; float32), on an H x W image:
  1. the triangle is skipped unless x, y and w of its three vertices are finite and every w > 0 (no clipping);
  2. iw = 1 / w, ndc = x * iw (float32); s = floor(((double)ndc * 0.5 + 0.5) * size * 256 + 0.5) with size = W for x, H for y
     (8 sub-pixel bits, half-units round up); the triangle is skipped unless every |s| <= 2^30 (RANGE), H, W <= 2^22;
  3. area = (x1 - x0)(y2 - y0) - (y1 - y0)(x2 - x0); area == 0 is skipped; both signs are kept (no culling);
  4. pixel (px, py) has its centre at c = (256 px + 128, 256 py + 128); e0 = (x2 - x1)(cy - y1) - (y2 - y1)(cx - x1) and its two
     rotations; the pixel is inside when all e_i >= 0 (area > 0) or all e_i <= 0 (area < 0): edges are inclusive;
  5. b_i = float32(double(e_i) / double(area)) for i = 0, 1; b2 = (1 - b0) - b1; z_i = z * iw; zw = (b0 z0 + b1 z1) + b2 z2 (float32,
     no contraction); the pixel is kept only if -1 <= zw <= 1 (a NaN zw never claims a pixel);
  6. the smallest zw wins (-0 == +0), ties go to the lowest triangle id;
  7. record (u, v, zw, id + 1), 0 = empty; u, v = b0, b1, or, when any iw != 1, a_i = b_i iw_i, u = a0 / ((a0 + a1) + a2), v = a1 / (...).

Why 2^30: with all six snapped coordinates and both centre coordinates in [-M, M], every difference is at most 2M, every product at
most 4M^2, and area and e_i are twice the signed area of a triangle inside that square, at most 4M^2 as well.  4M^2 <= 2^62 < 2^63
for M = 2^30 and overflows for M = 2^31, so 2^30 is the largest power of two that keeps all int64 work exact; centres are at most
256 * 2^22 = 2^30.
"""
import functools
import math
from fractions import Fraction

import numpy as np

F32 = np.float32
SUBPIX = 256
RANGE = 1 << 30
_ONE = F32(1.0)


def _wrap64(x):
    return ((int(x) + (1 << 63)) % (1 << 64)) - (1 << 63)


class Rule:
    """The rule, with one method per decision so that a test can keep deliberately wrong variants next to it."""
    limit = RANGE          # None: no range rule (arbitrary-precision evaluation of steps 3-7 on whatever step 2 gives)
    wrapping = False       # True: every integer result is reduced to int64 two's complement, as C would

    def fix(self, x):
        return _wrap64(x) if self.wrapping else x

    def round_snap(self, v):
        return math.floor(v + 0.5)

    def snap(self, ndc, size):
        """the snapped coordinate (Python int), or None when the triangle has to be skipped"""
        v = (float(ndc) * 0.5 + 0.5) * float(size) * float(SUBPIX)
        if not math.isfinite(v):
            return None
        s = self.round_snap(v)
        if self.limit is not None and abs(s) > self.limit:
            return None
        return self.fix(s)

    def keep_area(self, area):
        return area != 0

    def inside(self, e, area, edges):
        """e: the three edge-function arrays; edges: ((dx, dy), ...) of edge i (opposite vertex i)"""
        if area > 0:
            return (e[0] >= 0) & (e[1] >= 0) & (e[2] >= 0)
        return (e[0] <= 0) & (e[1] <= 0) & (e[2] <= 0)

    def order_key(self, zw):
        """what 'nearest' compares (smaller wins); float compare: -0 == +0"""
        return zw

    def replaces(self, key_new, key_old):
        """triangles arrive in increasing id: strict '<' keeps the lowest id on ties"""
        return key_new < key_old

    # ------------------------------------------------------------------------------------------------------------
    def setup(self, pos, tri, f, H, W):
        p = [pos[int(tri[f, k])] for k in range(3)]
        for q in p:
            if not (np.isfinite(q[0]) and np.isfinite(q[1]) and np.isfinite(q[3]) and q[3] > 0):
                return None
        with np.errstate(all="ignore"):
            iw = [_ONE / q[3] for q in p]
            xs = [self.snap(q[0] * w, W) for q, w in zip(p, iw)]
            ys = [self.snap(q[1] * w, H) for q, w in zip(p, iw)]
            z = [q[2] * w for q, w in zip(p, iw)]
        if any(v is None for v in xs + ys):
            return None
        fx = self.fix
        area = fx(fx(fx(xs[1] - xs[0]) * fx(ys[2] - ys[0])) - fx(fx(ys[1] - ys[0]) * fx(xs[2] - xs[0])))
        if not self.keep_area(area):
            return None
        h = SUBPIX // 2
        pxlo = 0 if min(xs) - h < 0 else -((-(min(xs) - h)) // SUBPIX)
        pylo = 0 if min(ys) - h < 0 else -((-(min(ys) - h)) // SUBPIX)
        pxhi = min((max(xs) - h) // SUBPIX if max(xs) - h >= 0 else -1, W - 1)
        pyhi = min((max(ys) - h) // SUBPIX if max(ys) - h >= 0 else -1, H - 1)
        if pxlo > pxhi or pylo > pyhi:
            return None
        return dict(f=f, x=xs, y=ys, z=z, iw=iw, area=area, box=(pxlo, pxhi, pylo, pyhi),
                    persp=not (iw[0] == _ONE and iw[1] == _ONE and iw[2] == _ONE))

    def edge_functions(self, s):
        """(e0, e1, e2) over the triangle's clipped bounding box, [rows][cols]; int64 when that provably cannot wrap, else Python ints"""
        pxlo, pxhi, pylo, pyhi = s["box"]
        x, y = s["x"], s["y"]
        small = (not self.wrapping) and max(abs(v) for v in x + y) <= RANGE and max(pxhi, pyhi) < (1 << 22)
        dt = np.int64 if small else object
        cx = (np.arange(pxlo, pxhi + 1, dtype=np.int64) * SUBPIX + SUBPIX // 2).astype(dt)[None, :]
        cy = (np.arange(pylo, pyhi + 1, dtype=np.int64) * SUBPIX + SUBPIX // 2).astype(dt)[:, None]
        out, edges = [], []
        for j, k in ((1, 2), (2, 0), (0, 1)):
            dx, dy = self.fix(x[k] - x[j]), self.fix(y[k] - y[j])
            edges.append((dx, dy))
            if small:
                # |dx|, |dy|, |c - v| <= 2^31 and the result is twice a triangle area inside [-2^30, 2^30]^2: no wrap (module docstring)
                assert max(abs(dx), abs(dy)) <= 2 * RANGE
                e = np.int64(dx) * (cy - np.int64(y[j])) - np.int64(dy) * (cx - np.int64(x[j]))
            elif not self.wrapping:
                e = dx * (cy - y[j]) - dy * (cx - x[j])
            else:
                w = np.frompyfunc(_wrap64, 1, 1)
                e = w(w(dx * w(cy - y[j])) - w(dy * w(cx - x[j])))
                e = np.broadcast_to(e, (cy.shape[0], cx.shape[1]))
            out.append(e)
        return out, edges

    @staticmethod
    def _to_double(e):
        if e.dtype == object:
            return np.array([float(v) for v in e.ravel()], dtype=np.float64).reshape(e.shape)
        return e.astype(np.float64)

    def rasterize(self, pos, tri, H, W, aux=False):
        pos = np.ascontiguousarray(pos, dtype=F32)
        tri = np.ascontiguousarray(tri, dtype=np.int32)
        assert 0 < H <= (1 << 22) and 0 < W <= (1 << 22)
        rast = np.zeros((H, W, 4), dtype=F32)
        bary = np.zeros((H, W, 3), dtype=F32)
        key = None
        filled = np.zeros((H, W), dtype=bool)
        for f in range(tri.shape[0]):
            s = self.setup(pos, tri, f, H, W)
            if s is None:
                continue
            pxlo, pxhi, pylo, pyhi = s["box"]
            e, edges = self.edge_functions(s)
            ins = np.asarray(self.inside(e, s["area"], edges), dtype=bool)
            if not ins.any():
                continue
            with np.errstate(all="ignore"):
                area = float(s["area"])
                b0 = (self._to_double(e[0]) / area).astype(F32)
                b1 = (self._to_double(e[1]) / area).astype(F32)
                b2 = (_ONE - b0) - b1
                z, iw = s["z"], s["iw"]
                zw = (b0 * z[0] + b1 * z[1]) + b2 * z[2]
                u, v = b0, b1
                if s["persp"]:
                    a0, a1, a2 = b0 * iw[0], b1 * iw[1], b2 * iw[2]
                    sm = (a0 + a1) + a2
                    u, v = a0 / sm, a1 / sm
                ok = ins & (zw >= F32(-1.0)) & (zw <= F32(1.0))
                k = self.order_key(zw)
                if key is None:
                    key = np.zeros((H, W), dtype=np.asarray(k).dtype)
                sl = (slice(pylo, pyhi + 1), slice(pxlo, pxhi + 1))
                take = ok & (~filled[sl] | self.replaces(k, key[sl]))
            key[sl][take] = k[take]
            filled[sl][take] = True
            r = rast[sl]
            r[take, 0], r[take, 1], r[take, 2], r[take, 3] = u[take], v[take], zw[take], F32(f + 1)
            bb = bary[sl]
            bb[take, 0], bb[take, 1], bb[take, 2] = b0[take], b1[take], b2[take]
        return (rast, bary) if aux else rast


def rasterize_rule(pos, tri, H, W, aux=False):
    """the record [H][W][4] float32 = (u, v, zw, id + 1), bit for bit; aux=True: also the winner's (b0, b1, b2) [H][W][3]"""
    return Rule().rasterize(pos, tri, H, W, aux=aux)


def interpolate_rule(attr, rast, tri):
    """utx_interpolate: id = int(rast.w) - 1; w = (1 - u) - v; out = (a0 u + a1 v) + a2 w in float32; zeros where the pixel is empty"""
    attr = np.ascontiguousarray(attr, dtype=F32)
    tri = np.ascontiguousarray(tri, dtype=np.int32)
    rast = np.ascontiguousarray(rast, dtype=F32)
    H, W = rast.shape[:2]
    out = np.zeros((H, W, attr.shape[1]), dtype=F32)
    ids = rast[..., 3].astype(np.int32) - 1
    m = ids >= 0
    t = tri[ids[m]]
    u, v = rast[..., 0][m][:, None], rast[..., 1][m][:, None]
    with np.errstate(all="ignore"):
        w = (_ONE - u) - v
        out[m] = (attr[t[:, 0]] * u + attr[t[:, 1]] * v) + attr[t[:, 2]] * w
    return out


def interpolate_exact(attr, rast, tri, py, px):
    """the Fractions a0 u + a1 v + a2 (1 - u - v) of one covered pixel, on the float32 u, v of the record; one per channel"""
    attr = np.asarray(attr, dtype=F32)
    r = rast[py, px]
    t = tri[int(r[3]) - 1]
    u, v = Fraction(float(r[0])), Fraction(float(r[1]))
    return [Fraction(float(attr[t[0], c])) * u + Fraction(float(attr[t[1], c])) * v + Fraction(float(attr[t[2], c])) * (1 - u - v)
            for c in range(attr.shape[1])]


class ExactRaster:
    """Exact values of the rule's quantities on the snapped vertices and the float32 z_i, 1 / w_i it starts from.

    tris[f]: the set-up of every triangle that is not skipped; cand[(py, px)]: [(f, zw)] for every triangle whose closed snapped
    triangle holds the pixel centre and whose exact zw lies in [-1, 1]; edge[(py, px)]: the same without the zw condition."""

    def __init__(self, pos, tri, H, W):
        pos = np.ascontiguousarray(pos, dtype=F32)
        tri = np.ascontiguousarray(tri, dtype=np.int32)
        rule = Rule()
        self.H, self.W = H, W
        self.tris, self.cand, self.edge = {}, {}, {}
        for f in range(tri.shape[0]):
            s = rule.setup(pos, tri, f, H, W)
            if s is None or not all(np.isfinite(s["z"])):
                if s is not None:
                    s["nonfinite_z"] = True
                    self.tris[f] = s
                continue
            # z_i = n_i / D with one power-of-two D: zw = sum e_i n_i / (area D)
            zf = [Fraction(float(v)) for v in s["z"]]
            D = max(q.denominator for q in zf)
            s["zn"], s["zd"] = [int(q * D) for q in zf], D
            s["iwf"] = [Fraction(float(v)) for v in s["iw"]]
            self.tris[f] = s
            e, _ = rule.edge_functions(s)
            ins = rule.inside(e, s["area"], None)
            pxlo, _, pylo, _ = s["box"]
            for r, c in zip(*np.nonzero(ins)):
                ee = (int(e[0][r, c]), int(e[1][r, c]), int(e[2][r, c]))
                zw = Fraction(ee[0] * s["zn"][0] + ee[1] * s["zn"][1] + ee[2] * s["zn"][2], s["area"] * D)
                k = (pylo + int(r), pxlo + int(c))
                self.edge.setdefault(k, []).append((f, zw))
                if -1 <= zw <= 1:
                    self.cand.setdefault(k, []).append((f, zw))
        self.covered = np.zeros((H, W), dtype=bool)
        for (py, px) in self.cand:
            self.covered[py, px] = True

    def minimal(self, py, px):
        """(the triangles whose exact zw is the smallest at this pixel, that zw)"""
        c = self.cand[(py, px)]
        m = min(z for _, z in c)
        return {f for f, z in c if z == m}, m

    def values(self, f, py, px):
        s = self.tris[f]
        x, y, A = s["x"], s["y"], s["area"]
        cx, cy = px * SUBPIX + SUBPIX // 2, py * SUBPIX + SUBPIX // 2
        e = [(x[k] - x[j]) * (cy - y[j]) - (y[k] - y[j]) * (cx - x[j]) for j, k in ((1, 2), (2, 0), (0, 1))]
        b = [Fraction(v, A) for v in e]
        zw = Fraction(sum(ei * n for ei, n in zip(e, s["zn"])), A * s["zd"])
        u, v = b[0], b[1]
        den = None
        if s["persp"]:
            a = [bi * w for bi, w in zip(b, s["iwf"])]
            den = a[0] + a[1] + a[2]
            u, v = a[0] / den, a[1] / den
        return dict(b0=b[0], b1=b[1], b2=b[2], u=u, v=v, zw=zw, den=den, z=[Fraction(n, s["zd"]) for n in s["zn"]], iw=s["iwf"])


def rasterize_exact(pos, tri, H, W):
    return ExactRaster(pos, tri, H, W)


# ======================================================================================================================
# case sets, shared by the CPU and the GPU module
# ======================================================================================================================
class Case:
    def __init__(self, name, pos, tri, H, W, exact=True, attrs=False):
        self.name, self.H, self.W, self.exact, self.attrs = name, H, W, exact, attrs
        self.pos = np.ascontiguousarray(pos, dtype=F32)
        self.tri = np.ascontiguousarray(tri, dtype=np.int32)

    def __repr__(self):
        return self.name


def _xyzw(xy, z=0.0, w=1.0):
    xy = np.asarray(xy, dtype=np.float64)
    p = np.empty((xy.shape[0], 4), dtype=np.float64)
    p[:, :2], p[:, 2], p[:, 3] = xy, z, w
    return p.astype(F32)


def _sub_to_ndc(s, size):
    """the NDC value whose snap input is s sub-pixel units"""
    return np.asarray(s, dtype=np.float64) * 2.0 / (size * SUBPIX) - 1.0


def _soup(tris_xyzw):
    """[F][3][4] -> unshared vertices"""
    t = np.asarray(tris_xyzw, dtype=F32).reshape(-1, 4)
    return t, np.arange(t.shape[0], dtype=np.int32).reshape(-1, 3)


def _lattice(H, W, where, winding, seed, z=0.0):
    """where='centre': vertices on every pixel centre (each interior centre is a shared vertex of 6 faces); 'corner': vertices on
    every pixel corner, diagonals through the centres (each centre lies on the edge shared by 2 faces)"""
    rng = np.random.default_rng(seed)
    off, nx, ny = (0.5, W, H) if where == "centre" else (0.0, W + 1, H + 1)
    ix, iy = np.meshgrid(np.arange(nx), np.arange(ny))
    xy = np.stack([(ix.ravel() + off) / W * 2 - 1, (iy.ravel() + off) / H * 2 - 1], axis=-1)
    idx = (iy * nx + ix)
    a, b, c, d = idx[:-1, :-1].ravel(), idx[:-1, 1:].ravel(), idx[1:, :-1].ravel(), idx[1:, 1:].ravel()
    tri = np.concatenate([np.stack([a, b, d], -1), np.stack([a, d, c], -1)])
    tri = tri[rng.permutation(tri.shape[0])]
    if winding == "cw":
        tri = tri[:, ::-1]
    elif winding == "mixed":
        flip = rng.random(tri.shape[0]) < 0.5
        tri[flip] = tri[flip][:, ::-1]
    return Case("lattice-%s-%dx%d-%s" % (where, H, W, winding), _xyzw(xy, z), tri, H, W, attrs=True)


def lattice_cases():
    return [_lattice(H, W, where, wd, 11 + i) for i, (H, W) in enumerate(((16, 16), (33, 17)))
            for where in ("centre", "corner") for wd in ("ccw", "cw", "mixed")]


def snap_tie_cases():
    out = []
    for H, W, seed in ((16, 16, 1), (8, 32, 2)):
        rng = np.random.default_rng(seed)
        T = []

        def tri_sub(sx, sy, z=0.0):
            T.append(np.stack([_sub_to_ndc(sx, W), _sub_to_ndc(sy, H), np.full(3, z), np.ones(3)], -1))

        # vertices on exact half sub-pixel units, from one image size left / above the image to one size right / below it
        for i in range(60):
            kx = rng.integers(-W * SUBPIX, 2 * W * SUBPIX, 3) + 0.5
            ky = rng.integers(-H * SUBPIX, 2 * H * SUBPIX, 3) + 0.5
            tri_sub(kx, ky, z=0.01 * i)
        # small ones around pixel centres, so that a half-unit decides whether the centre is on an edge
        for i in range(60):
            cx, cy = rng.integers(0, W) * SUBPIX + 128, rng.integers(0, H) * SUBPIX + 128
            tri_sub(cx + rng.integers(-3, 4, 3) + 0.5 * rng.integers(0, 2, 3), cy + rng.integers(-3, 4, 3) + 0.5 * rng.integers(0, 2, 3), z=-0.5)
        # slivers narrower than one sub-pixel unit before the snap (quarter units are exact in float32 at these sizes)
        for i in range(20):
            x0, y0 = float(rng.integers(-200, W * SUBPIX)), float(rng.integers(-200, H * SUBPIX))
            tri_sub([x0 + 0.25, x0 + 0.75, x0 + 0.5 + 40 * SUBPIX], [y0 + 0.25, y0 + 0.75, y0 + 0.5 + 37 * SUBPIX], z=-0.25)
            tri_sub([x0 + 0.5, x0 + 1.0, x0 - 30 * SUBPIX], [y0 + 0.5, y0 + 0.0, y0 + 55 * SUBPIX + 0.5], z=-0.75)
        # zero area only after the snap: 10.5, 10.75, 11.25 all snap to 11; and a negative trio -3.5, -3.25, -2.75 -> -3
        tri_sub([10.5, 10.75, 11.25], [300.0, 700.0, 1200.0])
        tri_sub([300.0, 700.0, 1200.0], [-3.5, -3.25, -2.75])
        tri_sub([640.5, 640.75, 641.25], [0.0, 2000.0, 4000.0])
        # negative half units next to the image's first centre: -0.5 snaps to 0, -1.5 to -1
        tri_sub([-0.5, 128.0, -0.5], [-0.5, -0.5, 128.0], z=-0.9)
        tri_sub([-1.5, 128.5, -1.5], [-1.5, -1.5, 128.5], z=-0.95)
        # a negative coordinate off the half units: -255.75 snaps to floor(-255.25) = -256, which puts the centres of pixels (0, 0) and
        # (1, 1) exactly on the edge (-256, -256) - (512, 512); rounding toward zero (-255) would leave both outside
        tri_sub([-255.75, 512.0, 512.0], [-256.0, 512.0, -256.0], z=-0.99)
        pos, tri = _soup(T)
        out.append(Case("snap-ties-%dx%d" % (H, W), pos, tri, H, W))
    return out


def _quad(z, w=1.0, lo=-1.0, hi=1.0):
    """two triangles over [lo, hi]^2"""
    c = [(lo, lo), (hi, lo), (hi, hi), (lo, hi)]
    return [[(c[i][0] * w, c[i][1] * w, z * w, w) for i in k] for k in ((0, 1, 2), (0, 2, 3))]


def depth_cases():
    out = []
    rng = np.random.default_rng(5)
    # 64 full-screen quads at one depth, in random order (the per-quad vertex order is rotated too)
    T = []
    for i in rng.permutation(64):
        for t in _quad(0.25):
            T.append(np.roll(np.asarray(t), int(i) % 3, axis=0))
    out.append(Case("depth-64-quads", *_soup(T), 32, 32))
    # +0.0 / -0.0 pairs in both orders, over two halves of the image
    T = _quad(0.0, hi=0.0) + _quad(-0.0, hi=0.0) + _quad(-0.0, lo=0.0) + _quad(0.0, lo=0.0)
    out.append(Case("depth-signed-zero", *_soup(T), 16, 16))
    # negative, positive and mixed zw: tilted planes that cross zw = 0 and each other
    T = []
    for i in range(24):
        xy = rng.uniform(-1.3, 1.3, (3, 2))
        z = rng.uniform(-1, 1, 3) * (1.0 if i % 3 else 0.05) - (0.5 if i % 2 else 0.0)
        T.append(np.concatenate([xy, z[:, None], np.ones((3, 1))], -1))
    out.append(Case("depth-mixed-sign", *_soup(T), 32, 32))
    # zw exactly +-1 is kept, the float32 neighbours outside are dropped: a vertex on a pixel centre has b = (1, 0, 0) there;
    # and flat full-screen triangles at exactly +-1, whose float zw is 1 only where the three roundings allow it
    T = []
    up, dn = np.nextafter(F32(1), F32(2)), np.nextafter(F32(-1), F32(-2))
    for k, zv in enumerate((1.0, up, -1.0, dn)):
        cx = _sub_to_ndc((2 + 3 * k) * SUBPIX + 128, 16)
        cy = _sub_to_ndc(5 * SUBPIX + 128, 16)
        T.append([(cx, cy, zv, 1), (cx + 0.3, cy + 0.1, 0.5 * zv, 1), (cx + 0.1, cy + 0.4, 0.5 * zv, 1)])
    T += _quad(1.0, lo=-1.0, hi=0.0) + _quad(-1.0, lo=0.0, hi=1.0)
    out.append(Case("depth-unit-limits", *_soup(T), 16, 16))
    # two interpenetrating triangles
    T = [[(-0.9, -0.8, -0.6, 1), (0.9, -0.7, 0.7, 1), (0.0, 0.9, 0.1, 1)],
         [(-0.9, -0.7, 0.6, 1), (0.9, -0.8, -0.7, 1), (0.1, 0.9, 0.0, 1)]]
    out.append(Case("depth-interpenetrating", *_soup(T), 48, 48))
    return out


def _big_triangles(n, seed):
    """n triangles, each of which covers (more than) the whole [-1, 1]^2 or most of it: clipped bounding box = the image"""
    rng = np.random.default_rng(seed)
    T = []
    for i in range(n):
        jit = rng.uniform(-0.2, 0.2, (3, 2))
        xy = np.array([[-1.2, -1.2], [3.4, -1.2], [-1.2, 3.4]]) + jit if i % 2 else np.array([[1.2, 1.2], [-3.4, 1.2], [1.2, -3.4]]) + jit
        z = rng.uniform(-0.9, 0.9, 3)
        T.append(np.concatenate([xy, z[:, None], np.ones((3, 1))], -1))
    return T


def queue_cases():
    """BIG_BBOX = 2048: a triangle whose clipped bounding box has more pixels is queued for the workgroup-per-triangle kernel.
    2049 = 3 * 683 has no other factorisation, hence the 683-row image."""
    out = []
    H, W = 683, 4

    def box_tri(x0, x1, y0, y1, z):
        """right triangle whose snapped bounding box is pixel centres x0..x1, y0..y1"""
        sx = np.array([x0, x1, x0]) * SUBPIX + 128.0
        sy = np.array([y0, y0, y1]) * SUBPIX + 128.0
        return np.stack([_sub_to_ndc(sx, W), _sub_to_ndc(sy, H), np.full(3, z), np.ones(3)], -1)

    out.append(Case("queue-bbox-2048", *_soup([box_tri(0, 3, 0, 511, 0.1)]), H, W))
    out.append(Case("queue-bbox-2049", *_soup([box_tri(0, 2, 0, 682, 0.1)]), H, W))
    out.append(Case("queue-bbox-both", *_soup([box_tri(0, 3, 0, 511, 0.1), box_tri(0, 2, 0, 682, 0.2), box_tri(0, 3, 170, 681, -0.2)]), H, W))
    # the same 4 x 513 triangle with its first row above the image (clipped box 4 x 512 = 2048: per-thread path) and one pixel lower
    # (4 x 513 = 2052: queued); see queue_shift_pair
    out.append(Case("queue-shift-up", *_soup([box_tri(0, 3, -1, 511, 0.1)]), H, W))
    out.append(Case("queue-shift-down", *_soup([box_tri(0, 3, 0, 512, 0.1)]), H, W))
    out.append(Case("queue-1100-on-64x64", *_soup(_big_triangles(1100, 21)), 64, 64, exact=False))
    for F in (1, 256, 257):
        out.append(Case("queue-all-F%d" % F, *_soup(_big_triangles(F, 30 + F)), 48, 48, exact=(F == 1)))
    return out


def _random_triangles(n, seed, spread=1.4, w=None):
    rng = np.random.default_rng(seed)
    T = []
    for i in range(n):
        c = rng.uniform(-1, 1, 2)
        xy = c + rng.uniform(-spread, spread, (3, 2)) * rng.choice([0.05, 0.3, 1.0])
        z = rng.uniform(-1, 1, 3)
        ww = np.ones(3) if w is None else rng.choice(w, 3)
        T.append(np.concatenate([xy * ww[:, None], (z * ww)[:, None], ww[:, None]], -1))
    return T


def shape_cases():
    out = []
    for H, W in ((1, 1), (1, 300), (300, 1), (97, 131)):
        T = _random_triangles(60, H * 1000 + W) + _quad(0.9)
        out.append(Case("shape-%dx%d" % (H, W), *_soup(T), H, W))
    T = [[(-1.1, -1.1, 0.2, 1), (1.3, -1.0, 0.3, 1), (-1.0, 1.2, 0.1, 1)], [(1.1, 1.1, -0.2, 1), (-0.7, 1.0, 0.0, 1), (1.0, -0.9, 0.4, 1)]]
    out.append(Case("shape-1025x1024", *_soup(T), 1025, 1024, exact=False))
    return out


def perspective_cases():
    out = []
    ws = [0.25, 0.5, 0.75, 1.0, 1.5, 2.0, 3.0, 4.0]
    out.append(Case("persp-w-quarter-to-4", *_soup(_random_triangles(80, 41, w=ws)), 40, 56, attrs=True))
    # one vertex at w = 2^-20 (NDC in range: its clip x, y are tiny), as vertex 0, 1 and 2 of three triangles
    T = []
    tiny = 2.0 ** -20
    base = [(-0.8, -0.7, 0.3), (0.9, -0.5, -0.2), (0.1, 0.8, 0.6)]
    for k in range(3):
        t = []
        for i, (x, y, z) in enumerate(base):
            w = tiny if i == k else (1.0, 2.0, 0.5)[i]
            t.append((x * w, y * w, (z + 0.1 * k) * w, w))
        T.append(t)
    out.append(Case("persp-w-2^-20", *_soup(T), 24, 24, attrs=True))
    # w of 0, negative, +inf, NaN (each in one vertex of an otherwise fine triangle) between triangles that are drawn
    T = _random_triangles(6, 43, w=ws)
    for bad in (0.0, -0.0, -1.0, np.inf, -np.inf, np.nan):
        t = np.array(_quad(0.1)[0], dtype=np.float64)
        t[1, 3] = bad
        T.append(t)
    sub = np.float64(np.finfo(F32).smallest_subnormal)                        # 1 / w overflows: x / w is inf (or NaN for x = 0)
    T.append([(1e-40, 0.0, 0.0, sub), (0.5, -0.5, 0.1, 1), (0.0, 0.5, 0.1, 1)])
    T += _random_triangles(6, 44, w=ws)
    out.append(Case("persp-bad-w", *_soup(T), 24, 24))
    return out


def range_triangle(f):
    return [(-0.5, -0.5, 0.0, 1.0), (f, -0.9 * f, 0.0, 1.0), (-0.8 * f, f, 0.0, 1.0)]


RANGE_F = (3.0, 1e2, 4e3, 1e5, 1e6, 1e8, 1e12, 3e38)


def range_cases():
    out = []
    for size in (32, 256):
        for f in RANGE_F:
            # a small triangle behind, so that a dropped big one leaves something to see
            T = [np.array(range_triangle(f), dtype=np.float64)] + [[(-0.2, -0.2, 0.5, 1), (0.3, -0.1, 0.5, 1), (0.0, 0.4, 0.5, 1)]]
            out.append(Case("range-f%g-%d" % (f, size), *_soup(T), size, size, exact=(size == 32)))
    # the limit itself, on a 1 x 1 image where s = (ndc / 2 + 1 / 2) * 256: s = +-2^30 is kept (area = 2^62), one float32 step further is skipped
    a, b = float(2 ** 23 - 1), -float(2 ** 23 + 1)                              # s = 2^30, s = -2^30
    a2, b2 = float(2 ** 23), -float(2 ** 23 + 2)                                # s = 2^30 + 128, s = -2^30 - 128
    T = [[(b, b, 0.1, 1), (a, b, 0.1, 1), (a, a, 0.1, 1)], [(b, b, 0.0, 1), (a2, b, 0.0, 1), (a, a, 0.0, 1)],
         [(b, b2, -0.1, 1), (a, b, -0.1, 1), (a, a, -0.1, 1)], [(b, b, 0.3, 1), (a, a, 0.3, 1), (b, a, 0.3, 1)]]
    out.append(Case("range-limit-1x1", *_soup(T), 1, 1))
    out.append(Case("range-limit-32x32", *_soup(T), 32, 32))
    # inf / NaN in x, y or z of one vertex, between triangles that are drawn
    T = _random_triangles(5, 51)
    for col in (0, 1, 2):
        for bad in (np.inf, -np.inf, np.nan):
            t = np.array(_quad(0.2, lo=-0.9, hi=0.9)[0], dtype=np.float64)
            t[2, col] = bad
            T.append(t)
    t = np.array(_quad(0.2)[1], dtype=np.float64)
    t[:, 0] *= 3e38                                                             # finite x whose snap input overflows nothing but the range
    T.append(t)
    T += _random_triangles(5, 52)
    out.append(Case("range-nonfinite", *_soup(T), 32, 32))
    return out


CASE_SETS = {"lattice": lattice_cases, "snap": snap_tie_cases, "depth": depth_cases, "queue": queue_cases, "shapes": shape_cases,
             "perspective": perspective_cases, "range": range_cases}


@functools.lru_cache(maxsize=None)
def case_set(name):
    return tuple(CASE_SETS[name]())


def all_cases():
    return [c for n in CASE_SETS for c in case_set(n)]


@functools.lru_cache(maxsize=None)
def _rule_by_name(name):
    c = next(c for c in all_cases() if c.name == name)
    rast, bary = rasterize_rule(c.pos, c.tri, c.H, c.W, aux=True)
    rast.setflags(write=False)
    bary.setflags(write=False)
    return rast, bary


def rule_of(case):
    """the rule's (record, winner's b0 b1 b2) of a case, computed once per process and read-only"""
    return _rule_by_name(case.name)


def attrs_of(case, C):
    """[V][C] float32 vertex attributes of mixed sign and magnitude"""
    rng = np.random.default_rng(C * 7 + case.pos.shape[0])
    return (rng.standard_normal((case.pos.shape[0], C)) * np.array([1.0, 100.0, 1e-3, 7.0, 0.5])[:C]).astype(F32)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)

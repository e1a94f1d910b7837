"""The rasteriser's rule against an independent restatement and against exact arithmetic (CPU).

oracle/geom_ref.c was written beside raster.hip: the two agreeing bit for bit says little about a mistake they share.  Here
  * G.rasterize / G.interpolate equal tests/support/raster_exact_ref.py (numpy float32 + Python integers, no shared code) bit for bit
    on every case set the GPU module runs;
  * the rule itself is compared with fractions.Fraction values of the same quantities, inside bounds derived where they are asserted;
  * deliberately wrong variants of the rule must each differ from it on some case set, or the case sets would not be a test.

u below is float32's unit roundoff 2^-24: rounding a value x to float32 moves it by at most u |x| (normal range)."""
import math
from fractions import Fraction

import numpy as np
import pytest

from oracle import geom_ref as G
from tests.support import raster_exact_ref as R

U = 2.0 ** -24
SETS = list(R.CASE_SETS)


def _cases(exact_only=False):
    return [pytest.param(c, id=c.name) for c in R.all_cases() if c.exact or not exact_only]


def _same_bits(a, b, what):
    a, b = R.bits(a), R.bits(b)
    bad = np.argwhere(a != b)
    assert bad.shape[0] == 0, "%s: %d of %d values differ, first at %s: %s vs %s" % (
        what, bad.shape[0], a.size, tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])])


# ---------------------------------------------------------------------------------------------------------------- oracle parity
@pytest.mark.parametrize("case", _cases())
def test_oracle_rasterize_equals_the_restatement(case):
    ref, _ = R.rule_of(case)
    _same_bits(G.rasterize(case.pos, case.tri, case.H, case.W), ref, case.name)


@pytest.mark.parametrize("C", [1, 3, 5])
@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in R.all_cases() if c.attrs])
def test_oracle_interpolate_equals_the_restatement(case, C):
    rast, _ = R.rule_of(case)
    attr = R.attrs_of(case, C)
    ref = R.interpolate_rule(attr, rast, case.tri)
    _same_bits(G.interpolate(attr, rast, case.tri), ref, case.name)
    assert not ref[rast[..., 3] == 0].any(), "zeros where the pixel is empty"
    assert (rast[..., 3] == 0).any() or case.name.startswith("lattice"), "the perspective rasters have empty pixels"


def test_interpolate_within_the_counted_bound_of_the_exact_value():
    """out = fl(fl(fl(a0 u) + fl(a1 v)) + fl(a2 w)), w = fl(fl(1 - u) - v), against a0 u + a1 v + a2 (1 - u - v) in Fractions on the
    float32 u, v of the record.  u, v in [0, 1]: 1 - u and (1 - u) - v lie in [-1, 1] and each rounding moves them by at most 2^-25, so
    |w - (1 - u - v)| <= 2 u.  Three products and two sums round once each, relative u, on partial sums of magnitude at most
    S = |a0 u| + |a1 v| + |a2 w|: at most 3 u S (1 + 2^-20) for the first-order terms and their cross terms.  Together
    |out - exact| <= 3 u S (1 + 2^-20) + 2 u |a2| + 2^-147 (three possible underflows of 2^-150 each)."""
    worst = 0.0
    for case in (c for c in R.all_cases() if c.attrs and c.H * c.W <= 1024):
        rast, _ = R.rule_of(case)
        attr = R.attrs_of(case, 5)
        out = R.interpolate_rule(attr, rast, case.tri)
        for py, px in np.argwhere(rast[..., 3] > 0):
            ex = R.interpolate_exact(attr, rast, case.tri, py, px)
            t = case.tri[int(rast[py, px, 3]) - 1]
            u, v = float(rast[py, px, 0]), float(rast[py, px, 1])
            for c in range(5):
                a = [abs(float(attr[t[k], c])) for k in range(3)]
                bound = 3 * U * (a[0] * u + a[1] * v + a[2] * (abs(1 - u - v) + 2 * U)) * (1 + 2.0 ** -20) + 2 * U * a[2] + 2.0 ** -147
                err = abs(Fraction(float(out[py, px, c])) - ex[c])
                assert err <= bound, (case.name, py, px, c, float(err), bound)
                worst = max(worst, float(err) / bound)
    print("[interpolate] worst |out - exact| / bound = %.3f" % worst)
    assert worst > 0


# ---------------------------------------------------------------------------------------------------- exact parity of the rule
def _depth_bound(val):
    """|float zw - exact zw| of one triangle at one pixel, Z = max |z_i|:
    b0, b1: d = fl64(fl64(e) / fl64(area)) carries three double roundings, |d - q| <= 3 * 2^-53 (1 + 2^-52) q <= 2^-51 q, and the float32
      rounding of d at most u d: |b_i - q_i| <= q_i (u + 2^-51)                                                       [asserted below]
    b2 = fl(fl(1 - b0) - b1): both operands' results lie in [-1, 1], each rounding <= 2^-25, so |b2 - (1 - b0 - b1)| <= u, and
      |b2 - q2| <= u + (q0 + q1)(u + 2^-51) <= 2^-23 + 2^-51                                                           [asserted below]
    zw = fl(fl(fl(b0 z0) + fl(b1 z1)) + fl(b2 z2)) against sum b_i z_i: three products and two sums, relative u each, on magnitudes
      at most Z (|b0| + |b1| + |b2|) <= Z (1 + 2^-22): at most 3 u Z (1 + 2^-20), + 3 * 2^-150 for underflow   [asserted below: <= 2^-22 Z]
    sum b_i z_i against sum q_i z_i: Z sum |b_i - q_i| <= Z (u + 2 (q0 + q1)(u + 2^-51)) <= Z (3 u + 2^-50).
    Together: |zw - exact| <= Z (6 u (1 + 2^-20) + 2^-50) + 2^-147."""
    Z = max(abs(z) for z in val["z"])
    return float(Z) * (6 * U * (1 + 2.0 ** -20) + 2.0 ** -50) + 2.0 ** -147


@pytest.mark.parametrize("case", _cases(exact_only=True))
def test_rule_against_exact_arithmetic(case):
    """Coverage: the rule covers exactly the pixels whose centre lies in some closed snapped triangle with exact zw in [-1, 1], except
    where every such exact zw is within its depth bound of +-1 (the float zw may fall on the other side of the limit there; the
    flat triangles at +-1 of depth-unit-limits are the case).  Winner: float zw_w <= float zw_t for every t, so exact zw_w <= exact
    zw_min + bound_w + bound_min; and when the winner is not exactly minimal it must be within that.  Records: see _depth_bound; u, v
    of a perspective triangle are counted in the loop."""
    rast, bary = R.rule_of(case)
    ex = R.rasterize_exact(case.pos, case.tri, case.H, case.W)
    cov = rast[..., 3] > 0
    ratio = dict(b01=0.0, b2=0.0, zw_sum=0.0, zw=0.0, uv=0.0, win=0.0)
    n_nonmin = 0
    for py in range(case.H):
        for px in range(case.W):
            edge = ex.edge.get((py, px), [])
            if not cov[py, px]:
                # empty by the rule: no exact candidate, unless each one is within its bound of the limit
                for f, zw in ex.cand.get((py, px), []):
                    assert 1 - abs(zw) <= _depth_bound(ex.values(f, py, px)), (case.name, py, px, f, float(zw))
                continue
            f = int(rast[py, px, 3]) - 1
            assert f in {t for t, _ in edge}, (case.name, py, px, f, "winner does not hold the pixel centre")
            val = ex.values(f, py, px)
            D = _depth_bound(val)
            if (py, px) not in ex.cand or f not in {t for t, _ in ex.cand[(py, px)]}:
                assert abs(val["zw"]) - 1 <= D, (case.name, py, px, f, float(val["zw"]))
            else:
                mins, zmin = ex.minimal(py, px)
                if f not in mins:
                    n_nonmin += 1
                    Dm = max(_depth_bound(ex.values(t, py, px)) for t in mins)
                    assert val["zw"] - zmin <= D + Dm, (case.name, py, px, f, sorted(mins), float(val["zw"] - zmin))
                    ratio["win"] = max(ratio["win"], float(val["zw"] - zmin) / (D + Dm))
            b = [Fraction(float(v)) for v in bary[py, px]]
            q = [val["b0"], val["b1"], val["b2"]]
            for i in (0, 1):
                bound = q[i] * Fraction(U + 2.0 ** -51)
                assert abs(b[i] - q[i]) <= bound, (case.name, py, px, i, float(b[i] - q[i]))
                if bound:
                    ratio["b01"] = max(ratio["b01"], float(abs(b[i] - q[i]) / bound))
            bound2 = U + float(q[0] + q[1]) * (U + 2.0 ** -51)
            assert abs(b[2] - q[2]) <= bound2 <= 2.0 ** -23 + 2.0 ** -51, (case.name, py, px, float(b[2] - q[2]))
            ratio["b2"] = max(ratio["b2"], float(abs(b[2] - q[2])) / bound2)
            Z = float(max(abs(z) for z in val["z"]))
            zsum = sum(bi * zi for bi, zi in zip(b, val["z"]))
            zf = Fraction(float(rast[py, px, 2]))
            bound_s = 3 * U * Z * (1 + 2.0 ** -20) + 2.0 ** -147
            assert abs(zf - zsum) <= bound_s <= 2.0 ** -22 * Z + 2.0 ** -147, (case.name, py, px, float(zf - zsum))
            assert abs(zf - val["zw"]) <= D, (case.name, py, px, float(zf - val["zw"]), D)
            if Z:
                ratio["zw_sum"] = max(ratio["zw_sum"], float(abs(zf - zsum)) / bound_s)
                ratio["zw"] = max(ratio["zw"], float(abs(zf - val["zw"])) / D)
            uu, vv = Fraction(float(rast[py, px, 0])), Fraction(float(rast[py, px, 1]))
            if val["den"] is None:
                assert uu == b[0] and vv == b[1]
                continue
            # perspective: a_i = fl(b_i iw_i), sum = fl(fl(a0 + a1) + a2), u = fl(a0 / sum), against U = q0 iw0 / Den, Den = sum q_i iw_i.
            #   numerator: b0 carries (u + 2^-51), the product u: relative n <= 2 u + 2^-50.
            #   denominator, absolute: a0, a1 carry n each; a2 carries iw2 (|b2 - q2| (1 + u) + |q2| u) -- the error of b2 is absolute, so a
            #   large iw2 beside small iw0, iw1 amplifies it, which is the rule's own loss and is counted, not hidden; the two sums add
            #   u (A0 + A1) and u Den; second-order terms (each below u times a first-order one) are covered by the factor 1 + 2^-10.
            #   quotient: computed num in N (1 +- n), den in Den (1 +- d), then one rounding: |u / U - 1| <= (1 + n)(1 + u) / (1 - d) - 1.
            iw = [float(w) for w in val["iw"]]
            A = [float(q[i]) * iw[i] for i in range(3)]
            n = 2 * U + 2.0 ** -50
            d = (1 + 2.0 ** -10) * ((A[0] + A[1]) * n + iw[2] * (bound2 * (1 + U) + abs(float(q[2])) * U) + U * (A[0] + A[1]) + U * float(val["den"])) / float(val["den"])
            assert d < 1
            rel = (1 + n) * (1 + U) / (1 - d) - 1
            for got, want, num in ((uu, val["u"], A[0]), (vv, val["v"], A[1])):
                bound = float(want) * rel + 2.0 ** -149
                assert abs(got - want) <= bound, (case.name, py, px, float(got - want), bound, rel / U)
                if want:
                    ratio["uv"] = max(ratio["uv"], float(abs(got - want)) / bound)
    print("[exact %s] worst error / bound: b0,b1 %.3f  b2 %.3f  zw vs sum b z %.3f  zw vs exact %.3f  persp u,v %.3f;  "
          "%d winners not exactly minimal (worst gap / bound %.3f)" % (case.name, ratio["b01"], ratio["b2"], ratio["zw_sum"], ratio["zw"],
                                                                    ratio["uv"], n_nonmin, ratio["win"]))


@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in R.case_set("lattice")])
def test_lattice_has_no_hole_and_the_lowest_id_wins(case):
    """every pixel centre is a vertex shared by up to 6 faces (centre lattice: the border row / column of centres is on the mesh border)
    or lies on the diagonal shared by 2 faces (corner lattice); all zw are +0, so the winner is the lowest id that holds the centre"""
    rast, _ = R.rule_of(case)
    ex = R.rasterize_exact(case.pos, case.tri, case.H, case.W)
    assert (rast[..., 3] > 0).all(), "hole"
    share = [len(ex.edge[(py, px)]) for py in range(case.H) for px in range(case.W)]
    assert min(share) >= 1 and max(share) == (6 if "centre" in case.name else 2)
    if "corner" in case.name:
        assert min(share) == 2
    for (py, px), c in ex.edge.items():
        assert int(rast[py, px, 3]) - 1 == min(f for f, _ in c)


def test_queue_switch_does_not_move_pixels():
    """the 4 x 513 triangle one row up (clipped box 2048 pixels) and in place (2052 pixels) gives the same records, one row apart"""
    by = {c.name: c for c in R.case_set("queue")}
    up, _ = R.rule_of(by["queue-shift-up"])
    down, _ = R.rule_of(by["queue-shift-down"])
    assert np.array_equal(R.bits(up[:512]), R.bits(down[1:513])) and (down[1:513, :, 3] > 0).sum() > 1000


# ------------------------------------------------------------------------------------------------------ the cases discriminate
class _Exclusive(R.Rule):
    def inside(self, e, area, edges):
        return ((e[0] > 0) & (e[1] > 0) & (e[2] > 0)) if area > 0 else ((e[0] < 0) & (e[1] < 0) & (e[2] < 0))


class _TopLeft(R.Rule):
    def inside(self, e, area, edges):
        sg = 1 if area > 0 else -1
        ok = True
        for ei, (dx, dy) in zip(e, edges):
            dx, dy = sg * dx, sg * dy
            tl = dy > 0 or (dy == 0 and dx < 0)
            ok = ok & ((sg * ei > 0) | ((ei == 0) & tl))
        return ok


class _TruncSnap(R.Rule):
    def round_snap(self, v):
        return math.trunc(v + 0.5)


class _HighestId(R.Rule):
    def replaces(self, key_new, key_old):
        return key_new <= key_old


class _CullBack(R.Rule):
    def keep_area(self, area):
        return area > 0


class _RawBits(R.Rule):
    def order_key(self, zw):
        return (zw + R.F32(0.0)).view(np.uint32).astype(np.int64)


class _Wrapping(R.Rule):
    """what C's int64 gives once the range rule is missing"""
    limit = None
    wrapping = True


VARIANTS = {"exclusive edges": _Exclusive, "top-left fill": _TopLeft, "truncating snap": _TruncSnap, "ties to the highest id": _HighestId,
            "culled back faces": _CullBack, "zw ordered by raw bits": _RawBits, "int64 that wraps": _Wrapping}
# where each variant is looked for (the sets on which it must show; looking everywhere would only cost time)
LOOK = {"exclusive edges": ("lattice",), "top-left fill": ("lattice",), "truncating snap": ("snap",), "ties to the highest id": ("lattice", "depth"),
        "culled back faces": ("lattice",), "zw ordered by raw bits": ("depth",), "int64 that wraps": ("range",)}


@pytest.mark.parametrize("name", list(VARIANTS))
def test_each_wrong_variant_is_caught(name):
    caught = []
    for s in LOOK[name]:
        for case in R.case_set(s):
            if case.H * case.W > 4096 and name != "int64 that wraps":
                continue
            ref, _ = R.rule_of(case)
            got = VARIANTS[name]().rasterize(case.pos, case.tri, case.H, case.W)
            n = int((R.bits(got) != R.bits(ref)).any(axis=-1).sum())
            if n:
                caught.append("%s: %d pixels" % (case.name, n))
    print("[variant %s] differs on %s" % (name, "; ".join(caught) or "nothing"))
    assert caught, "no case set tells '%s' from the rule" % name


def test_range_rule_is_what_keeps_int64_exact():
    """without the range rule, arbitrary-precision integers and wrapping int64 agree up to f = 1e6 on 32 x 32 and part ways at 1e8
    (the finding that asked for the rule); with it, f >= 1e6 is skipped and the small triangle behind shows through"""
    class Unbounded(R.Rule):
        limit = None
    by = {c.name: c for c in R.case_set("range")}
    for f, same in ((3.0, True), (1e2, True), (4e3, True), (1e5, True), (1e6, True), (1e8, False)):
        c = by["range-f%g-32" % f]
        a = Unbounded().rasterize(c.pos, c.tri, 32, 32)
        w = _Wrapping().rasterize(c.pos, c.tri, 32, 32)
        assert np.array_equal(R.bits(a), R.bits(w)) == same, f
        drawn = 1.0 in np.unique(R.rule_of(c)[0][..., 3])
        assert drawn == (f <= 1e5), f                      # 1e6 * 0.5 * 32 * 256 = 4.1e9 > 2^30
    lim = R.rule_of(by["range-limit-1x1"])[0]
    assert lim[0, 0, 3] == 1.0, "the triangle with |s| = 2^30 (area 2^62) is drawn; its neighbours one float32 step outside are not"

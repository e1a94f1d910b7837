"""The checkers of the two grid nearest-neighbour searches, held on the CPU (oracle/nn_search_ref.py): the restated ring search equals the float32 brute force
on every constructed family, the brute force stays inside the float64 bound, every planted mistake is caught by a named case under the same two checks the GPU
module applies (tests/test_nn_search_edges_gpu.py), and the stop rule's factor 0.99999 is pinned by the measured worst case of the float32 cell rule."""
import numpy as np
import pytest

from oracle import geom_ref as G
from oracle import nn_search_ref as R

F = np.float32


def _same_as_brute(case, k, grid, **kw):
    """the two checks of the GPU module: bit-equal to the float32 brute force, and inside the float64 bound.  Returns None or what failed."""
    idx, d2 = R.ring_search(case["src"], case["dst"], k, case.get("src_mask"), grid=grid, **kw)
    ri, rd = G.knn_brute(case["src"], case["dst"], k, case.get("src_mask"))
    if not np.array_equal(idx, ri):
        return "index"
    if not np.array_equal(d2, rd):
        return "d2"
    return R.check64(case["src"], case["dst"], idx, k, case.get("src_mask"))


@pytest.mark.parametrize("k", [1, 4, 32])
def test_restated_search_equals_brute_force_on_every_family(k):
    for case in R.knn_cases(k) + R.one_cell(128, 5000, far=2) + [c for g in R.GRIDS for c in R.xrow_gap(g) + R.two_cell(g)]:
        ri, _ = G.knn_brute(case["src"], case["dst"], k, case.get("src_mask"))
        assert R.check64(case["src"], case["dst"], ri, k, case.get("src_mask")) is None, case["name"] + ": the brute force leaves its own float64 bound"
        for grid in R.GRIDS:
            assert _same_as_brute(case, k, grid) is None, "%s, grid %d" % (case["name"], grid)


@pytest.mark.parametrize("grid", R.GRIDS)
def test_restated_search_equals_brute_force_at_the_ring_stop(grid):
    """family B on the grid it was built for: every float32 d2 of the candidate around (r cs)^2 at k = 1; with k - 1 fillers every 16th (k = 4) and
    64th (k = 32) step at every r, r = G/2 included (this restatement is Python: the GPU module runs the full steps)"""
    for r in (1, 2, 3, grid // 2):
        cases = R.family_b(grid, r, 1)
        got, want = cases[-1]["distinct_d2"], cases[-1]["targets"]
        print("G = %d, r = %d: %d distinct float32 d2 of %d in the window" % (grid, r, got, want))
        assert got >= 0.95 * want, "the candidate's d2 must step through (nearly) every float32 of the window: %d of %d" % (got, want)
        for k, cs_ in [(1, cases), (4, R.family_b(grid, r, 4, steps=16)), (32, R.family_b(grid, r, 32, steps=64))]:
            for case in cs_:
                assert _same_as_brute(case, k, grid) is None, case["name"]


# every planted mistake, the cases it is run on, and the case that must reject it (asserted by name; the checks are those of _same_as_brute)
def _b(grid, r, k=1, steps=4):
    return lambda: R.family_b(grid, r, k, steps=steps)


PLANTED = [
    ("margin 1.0", dict(margin=F(1.0)), 128, 1, _b(128, 1), "B/G128/r1/k1/0"),
    ("margin above 1", dict(margin=F(1.0001)), 128, 1, _b(128, 1), "B/G128/r1/k1/0"),
    ("(r+1) cs in the stop rule", dict(mistakes=["stop_r_plus_1"]), 128, 1, _b(128, 2), "B/G128/r2/k1/0"),
    ("stop at have >= 1", dict(mistakes=["stop_have_1"]), 128, 4, lambda: R.k_edges(4), "D/k4/mask3"),
    ("tie to the higher index", dict(mistakes=["tie_high"]), 128, 1, lambda: R.lattice_ties(128), "C/ties/G128"),
    ("<= in the insertion", dict(mistakes=["le_insert"]), 128, 4, R.duplicates, "C/dups"),
    ("no clamp of the cell index", dict(mistakes=["no_clamp"]), 128, 1, lambda: R.outside("both"), "E/both"),
    ("x-row range ends with the first non-empty cell", dict(mistakes=["xrow_first_cell"]), 64, 1, lambda: R.xrow_gap(64), "G/xrow/G64"),
    ("far face of the shell skipped", dict(mistakes=["skip_far_face"]), 128, 1, lambda: R.lattice_ties(128), "C/ties/G128"),
    ("ring loop ends at G/2", dict(mistakes=["ring_half"]), 128, 1, lambda: R.one_cell(128, 50, far=2), "D/onecell/G128"),
]


@pytest.mark.parametrize("name,kw,grid,k,cases,named", PLANTED, ids=[p[0] for p in PLANTED])
def test_planted_mistake_is_rejected_by_a_named_case(name, kw, grid, k, cases, named):
    cases = cases()
    failed = [c["name"] for c in cases if _same_as_brute(c, k, grid, **kw) is not None]
    print("%s: rejected by %s" % (name, failed))
    assert named in failed, "%s must reject `%s`; rejected by %s" % (named, name, failed)
    assert all(_same_as_brute(c, k, grid) is None for c in cases), "the unplanted search must pass the same cases"


@pytest.mark.parametrize("grid", R.GRIDS)
def test_stop_factor_is_below_the_measured_worst_case(grid):
    """KNN_G = 128 and the three values nn_grid() returns.  worst = min (gap / (r cs))^2 over every face and r in (1, 2, 3, G/2), in float64; the float32
    d2 of an unseen point is >= its true d2 (1 - c u), and the kernels' threshold fl(fl(rr rr) 0.99999f) is <= (r cs)^2 0.99999f (1 + 2u)."""
    worst, r, c = R.margin_worst_case(grid, detail=True)
    print("G = %d: worst (gap / (r cs))^2 = 1 - %.4g at r = %d, cell %d" % (grid, 1 - worst, r, c))
    assert worst * (1 - R.C_D2 * R.U) ** 2 > float(R.MARGIN) * (1 + 2 * R.U)
    assert abs((1 - worst) - 2.0 ** -25 * grid) < 1e-9, "the narrowing is 2^-25 on a gap of one cell: 2 * 2^-25 / cs"


def test_cell_thresholds_sit_where_the_rounding_of_v_plus_1_puts_them():
    for grid in R.GRIDS:
        assert R.cell_threshold(grid // 2, grid) == F(-2.0 ** -25)             # fl(v + 1) = 1 from the midpoint up (ties to even)
        assert R.cell_threshold(grid // 4, grid) == F(-0.5)                    # v + 1 is exact on [-1, -0.5]
        assert R.cell_threshold(0, grid) == F(-1.0)


@pytest.mark.parametrize("kind", ["parallel", "opposed", "zero", "mixed"])
@pytest.mark.parametrize("C", [1, 9])
def test_mvpaint_float32_oracle_stays_inside_its_counted_bound(kind, C):
    k = 8
    for case in R.lattice_ties(128) + R.duplicates() + R.k_edges(k) + R.one_cell(128, 5000, far=2):
        src, dst = case["src"], case["dst"]
        attr = ((np.arange(len(src) * C).reshape(len(src), C) * 37) % 101).astype(F) / F(64) - F(0.5)
        sn, dn = R.normals(kind, len(src), len(dst))
        idx, d2 = G.knn_brute(src, dst, k, case.get("src_mask"))
        ref, bound = R.mvpaint64(idx, d2, attr, sn, dn)
        got = G.knn_gather(src, attr, dst, k, src_mask=case.get("src_mask"), mode="mvpaint", src_nrm=sn, dst_nrm=dn)
        assert np.isfinite(got).all()
        assert (np.abs(got - ref) <= bound).all(), "%s: worst excess %g" % (case["name"], np.nanmax(np.abs(got - ref) - bound))
        if kind == "parallel":
            assert np.isfinite(bound[(idx >= 0).any(1)]).all(), "parallel normals are well conditioned: the bound must be finite there"


def test_mvpaint_one_coincident_source_gives_its_own_value_and_two_give_zero():
    """the reference's nan_to_num(nan=0) leaves 1/0 at the largest finite float: one d2 = 0 neighbour has weight 1; two overflow the L1 sum -> 0"""
    src = np.array([[0.1, 0.2, 0.3], [0.2, 0.2, 0.3], [0.1, 0.25, 0.3], [0.2, 0.2, 0.3]], F)
    dst = src[:2]
    attr = np.array([[3.0], [5.0], [7.0], [11.0]], F)
    sn, dn = R.normals("parallel", 4, 2)
    idx, d2 = G.knn_brute(src, dst, 3)
    ref, bound = R.mvpaint64(idx, d2, attr, sn, dn)
    got = G.knn_gather(src, attr, dst, 3, mode="mvpaint", src_nrm=sn, dst_nrm=dn)
    assert ref[0, 0] == pytest.approx(3.0, rel=1e-12) and ref[1, 0] == 0.0
    assert (np.abs(got - ref) <= bound).all() and got[1, 0] == 0.0

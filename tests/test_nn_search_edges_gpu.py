"""The two uniform-grid nearest-neighbour searches at their edges, on the GPU: utx_knn (ops.knn_gather) and the 1-NN fill utx_nn_fill (ops.nn_fill) on the
constructed families A-H of oracle/nn_search_ref.py (cell faces, the ring stop, exact ties, k and occupancy extremes, points outside the cube, launch
geometry, the fill's channel paths and grid thresholds, the MVPaint weighting).  Two independent checks on every case: index lists and d2 bit-equal to the
float32 brute force (geom_ref.knn_brute), and the float64 neighbour check (nn_search_ref.check64), which does not use the float32 expression.  Means are
bit-equal to the oracle's float32 sequence: the kernel adds the neighbours' values in ascending-distance order and divides once, no fused multiply-add
(-ffp-contract=off) and IEEE division, which is exactly what numpy does.  MVPaint rows stay inside the counted bound of nn_search_ref.mvpaint64."""
import time

import numpy as np
import pytest
import torch

from oracle import geom_ref as G
from oracle import nn_search_ref as R

pytestmark = pytest.mark.gpu
F = np.float32
SENT = -7.5


def _ops():
    from unitex_amd.texturetools import ops
    return ops


def _cu(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().contiguous()


def _attr(n, C):
    return ((np.arange(n * C).reshape(n, C) * 37) % 101).astype(F) / F(64) - F(0.5)


def _guarded(n, dtype, fill):
    """a tensor of n elements inside a larger one: 64 sentinels in front and behind, which the launch must leave alone"""
    big = torch.full((n + 128,), fill, dtype=dtype, device="cuda")
    return big, big[64:64 + n]


def _run_knn(case, k, C=3, mode="mean", nrm=None):
    """one launch with sentinels around out_idx, out_d2 and out_attr; returns (idx, d2, out) as numpy after the guards were checked"""
    ops = _ops()
    src, dst = case["src"], case["dst"]
    M = len(dst)
    gi, idx = _guarded(M * k, torch.int32, -99); gd, d2 = _guarded(M * k, torch.float32, SENT); go, out = _guarded(M * C, torch.float32, SENT)
    kw = {}
    if case.get("src_mask") is not None:
        kw["src_mask"] = _cu(case["src_mask"].astype(np.uint8))
    if case.get("dst_mask") is not None:
        kw["dst_mask"] = _cu(case["dst_mask"].astype(np.uint8))
    if nrm is not None:
        kw.update(src_nrm=_cu(nrm[0]), dst_nrm=_cu(nrm[1]))
    ops.knn_gather(_cu(src), _cu(dst), k, src_attr=_cu(case["attr"] if "attr" in case else _attr(len(src), C)), out=out.view(M, C), mode=mode,
                   out_index=(idx.view(M, k), d2.view(M, k)), **kw)
    torch.cuda.synchronize()
    for g, fill in ((gi, -99), (gd, SENT), (go, SENT)):
        g = g.cpu().numpy()
        assert (g[:64] == fill).all() and (g[-64:] == fill).all(), case["name"] + ": a sentinel beside an output was overwritten"
    return idx.cpu().numpy().reshape(M, k), d2.cpu().numpy().reshape(M, k), out.cpu().numpy().reshape(M, C)


def _check_knn(case, k, C=3):
    src, dst, sm = case["src"], case["dst"], case.get("src_mask")
    idx, d2, out = _run_knn(case, k, C)
    ri, rd = G.knn_brute(src, dst, k, sm)
    assert np.array_equal(idx, ri), case["name"] + ": neighbour ids"
    assert np.array_equal(d2.view(np.uint32), rd.view(np.uint32)), case["name"] + ": squared distances"
    assert R.check64(src, dst, idx, k, sm) is None, case["name"]
    ref = G.knn_gather(src, _attr(len(src), C), dst, k, src_mask=sm, out=np.full((len(dst), C), SENT, F))
    assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)), case["name"] + ": means"
    if sm is not None and not sm.any():
        assert (idx == -1).all() and np.isposinf(d2).all() and (out == SENT).all(), case["name"] + ": no source: -1, +inf, out untouched"


@pytest.mark.parametrize("k", [1, 4, 32])
def test_knn_families_bit_exact_and_inside_the_float64_bound(k):
    """families A (faces of the 64, 128 and 256 grids), C (ties, 40 duplicates, query on a source), D (n_src around k), E (outside the cube)"""
    for case in R.knn_cases(k):
        _check_knn(case, k)


@pytest.mark.parametrize("C", [1, 3])
def test_knn_launch_geometry(C):
    """family F: M around the 128-thread block, N around the 256-thread key blocks, k = 4; and a dst_mask of zeros, which must write nothing"""
    for case in R.launch_geometry():
        _check_knn(case, 4, C)
    case = dict(R.launch_geometry()[-1]); case["dst_mask"] = np.zeros(len(case["dst"]), bool)
    idx, d2, out = _run_knn(case, 4, C)
    assert (idx == -99).all() and (d2 == SENT).all() and (out == SENT).all()


@pytest.mark.parametrize("k", [1, 4, 32])
@pytest.mark.parametrize("r", [1, 2, 3, 64])
def test_knn_ring_stop(r, k):
    """family B on KNN_G = 128: the candidate's d2 steps through every float32 around (r cs)^2 while a nearer point waits in ring r + 1; k > 1 with
    k - 1 fillers beside the query, so that the stop test reads a full list.  Every step at every k for r <= 3, and at r = 64 for k = 1 (dense rows,
    three launches).  At r = 64 with fillers only 2 x 2 isolated rows fit into the cube and every launch walks 65 rings: every 16th step there
    (16 launches, 5.5 s per k on the MI355X)."""
    if r <= 3:
        cases = R.family_b(128, r, k, max_rows={1: None, 4: 256, 32: 128}[k])
        assert sum(len(c["dst"]) for c in cases) == 2 * cases[0]["targets"]
    else:
        cases = R.family_b(128, r, k, steps=None if k == 1 else 16)
    for case in cases:
        _check_knn(case, k)


def test_knn_all_sources_in_one_cell():
    """family D: 5000 sources in one cell; queries in it, beside it, and 64 in the opposite corner (ring 127: each reads all 128^3 cells).
    Measured on the MI355X: 0.52 s per k for the launch with the 64 far queries together with its host-side checks (the test prints it)."""
    case = R.one_cell(128, 5000, far=64)[0]
    for k in (1, 32):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        _check_knn(case, k)
        print("one cell, 64 far queries, k = %d: %.3f s with the checks" % (k, time.perf_counter() - t0))


def _run_fill(a, grid):
    from unitex_amd import _lib
    ops = _ops()
    H, W, C = a["atlas"].shape
    big, atl = _guarded(H * W * C, torch.float32, SENT)
    atl.copy_(_cu(a["atlas"]).reshape(-1))
    try:
        _lib.set_option("UTX_NN_GRID", grid)
        idx = ops.nn_fill(atl.view(H, W, C), _cu(a["winner"]), _cu(a["rast2d"]), _cu(a["pos"]), want_index=True)
        torch.cuda.synchronize()
    finally:
        _lib.set_option("UTX_NN_GRID", 0)
    g = big.cpu().numpy()
    assert (g[:64] == SENT).all() and (g[-64:] == SENT).all(), "a sentinel beside the atlas was overwritten"
    return idx.cpu().numpy(), atl.cpu().numpy().reshape(H * W, C)


def _check_fill(a, grid, name, ref=None):
    idx, atl = _run_fill(a, grid)
    ref = R.nn_fill_index(a["pos"], a["winner"], a["rast2d"]) if ref is None else ref
    assert np.array_equal(idx, ref), "%s, grid %d: nearest-seen-texel index" % (name, grid)
    C = atl.shape[1]
    want = a["atlas"].reshape(-1, C).copy()
    want[ref >= 0] = want[ref[ref >= 0]]
    assert np.array_equal(atl, want), "%s, grid %d: every filled texel is atlas[idx], every other texel is untouched" % (name, grid)
    w = a["winner"].reshape(-1); rw = a["rast2d"].reshape(-1, 4)[:, 3]
    assert (idx[(w < 0) & ~(rw > 0)] == -1).all() and (idx[w >= 0] == -1).all()
    return ref


def _fill_cases(grid):
    g = grid or 64                                  # these atlases are far below 2^14 texels: the automatic grid is 64
    out = [c for gg in R.GRIDS for c in R.family_a(gg)] + R.lattice_ties(g) + R.duplicates() + R.xrow_gap(g) + R.two_cell(g)
    for w in ("src", "dst", "both"):
        if not (grid == 256 and w == "dst"):        # test_nn_fill_queries_out_of_reach_on_the_256_grid
            out += R.outside(w)
    return out


@pytest.mark.parametrize("grid", [0, 64, 128, 256])
@pytest.mark.parametrize("C", [1, 3, 4, 16])
def test_nn_fill_families_every_grid_and_channel_path(grid, C):
    """families A, C, E and G (E's queries that no source can stop: on the 256 grid in a test of their own) through the 3-channel kernel and through search + nn_copy_c_kernel; uncovered unseen texels (rast.w = 0, -1, -0.0) stay -1"""
    for case in _fill_cases(grid):
        a = R.as_atlas(case["src"], case["dst"], C)
        ref = _check_fill(a, grid, case["name"])
        q = a["queries"]
        bi, _ = G.knn_brute(case["src"], case["dst"], 1)
        assert np.array_equal(ref[q], bi[:, 0]), "the two brute-force statements agree"
        assert R.check64(case["src"], case["dst"], ref[q].reshape(-1, 1), 1) is None


def test_nn_fill_queries_out_of_reach_on_the_256_grid():
    """family E, outside queries over inside sources, forced grid 256.  A query more than 2 from every source never meets the stop rule ((r cs)^2 < 4 for
    every r < G), so it walks all G rings: every cell of the table, 16.8 M here, in one thread.  One launch, C = 4 (search, then copy).
    Measured on the MI355X: 16.2 s for the launch with its host-side checks (the test prints it); the same case runs on the 64 and 128
    grids and through C = 1, 3, 16 in test_nn_fill_families_every_grid_and_channel_path."""
    case = R.outside("dst")[0]
    torch.cuda.synchronize(); t0 = time.perf_counter()
    _check_fill(R.as_atlas(case["src"], case["dst"], 4), 256, case["name"])
    print("out-of-reach queries, grid 256: %.3f s with the checks" % (time.perf_counter() - t0))


@pytest.mark.parametrize("grid", [64, 128, 256])
def test_nn_fill_ring_stop(grid):
    """family B on each grid nn_grid() can return, C = 3 (copy in the query kernel) and C = 4 (search, then copy) alternating over the launches"""
    n = 0
    for r in (1, 2, 3, grid // 2):
        for case in R.family_b(grid, r, 1):
            _check_fill(R.as_atlas(case["src"], case["dst"], (3, 4)[n % 2], width=64), grid, case["name"]); n += 1


@pytest.mark.parametrize("H,W", [(127, 129), (128, 128), (511, 513), (512, 512)])
def test_nn_fill_automatic_grid_at_its_thresholds(H, W):
    """T just below and at 2^14 and 2^18: the automatic grid, every forced grid and the brute force at the queries agree"""
    a = R.big_atlas(H, W, 3)
    ref = None
    for grid in (0, 64, 128, 256):
        ref = _check_fill(a, grid, "%dx%d" % (H, W), ref)
    assert 200 < (ref >= 0).sum() <= 500
    _check_fill(R.big_atlas(H, W, 4), 0, "%dx%d, C = 4" % (H, W), ref)


@pytest.mark.parametrize("kind", ["parallel", "opposed", "zero", "mixed"])
@pytest.mark.parametrize("C", [1, 9])
def test_mvpaint_inside_its_counted_bound(kind, C):
    """family H: families C and D (n_src around k, and the 5000 sources of one cell) at k = 8; every row is held to mvpaint64's bound (ill-conditioned rows have a large or infinite bound, none is left
    out); rows whose weights are all exactly 0 must be exactly 0; every output is finite"""
    k = 8
    for case in R.lattice_ties(128) + R.duplicates() + R.k_edges(k) + R.one_cell(128, 5000, far=4):
        src, dst, sm = case["src"], case["dst"], case.get("src_mask")
        nrm = R.normals(kind, len(src), len(dst))
        idx, d2, out = _run_knn(case, k, C, mode="mvpaint", nrm=nrm)
        ri, rd = G.knn_brute(src, dst, k, sm)
        assert np.array_equal(idx, ri) and np.array_equal(d2, rd), case["name"]
        ref, bound = R.mvpaint64(idx, d2, _attr(len(src), C), nrm[0], nrm[1])
        rows = (idx >= 0).any(1)
        assert (out[~rows] == SENT).all() and np.isfinite(out).all()
        err = np.abs(out[rows] - ref[rows])
        print("%s %s C=%d: max err %.3g, finite-bound rows %d of %d" % (case["name"], kind, C, err.max() if err.size else 0, np.isfinite(bound[rows]).all(1).sum(), rows.sum()))
        if kind == "parallel":
            assert np.isfinite(bound[rows]).all(), case["name"] + ": parallel normals are well conditioned, the bound must be finite on every row"
        assert (err <= bound[rows]).all(), "%s: worst excess over the bound %g" % (case["name"], np.nanmax(err - bound[rows]))


def test_mvpaint_coincident_sources():
    """d2 = 0: one coincident source takes weight 1 and gives its own value (the reference's nan_to_num leaves 1/0 at the largest float); two give 0"""
    src = np.array([[0.1, 0.2, 0.3], [0.2, 0.2, 0.3], [0.1, 0.25, 0.3], [0.2, 0.2, 0.3]], F)
    case = dict(name="H/coincident", src=src, dst=src[:2], attr=np.array([[3.0], [5.0], [7.0], [11.0]], F))
    nrm = R.normals("parallel", 4, 2)
    idx, d2, out = _run_knn(case, 3, 1, mode="mvpaint", nrm=nrm)
    ref, bound = R.mvpaint64(idx, d2, case["attr"], nrm[0], nrm[1])
    assert d2[0, 0] == 0 and (d2[1, :2] == 0).all()
    assert abs(out[0, 0] - 3.0) <= bound[0, 0] and bound[0, 0] < 1e-5 and out[1, 0] == 0.0

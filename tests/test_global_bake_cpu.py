"""The scattered-sample UV bake on the CPU: the float64 restatement (tests/support/global_bake_ref.py) against the reference's own run (fixture G25,
tests/golden/g25_global_inverse.npz), the caps the GPU tests rely on, and the proof that the comparisons of compare_case reject deliberate kernel mistakes."""
import ctypes
import os

import numpy as np
import pytest

from tests.support import global_bake_ref as R


@pytest.fixture(scope="module")
def restated():
    return {name: R.restate_case(name) for name in R.CASES}


def _as_got(out):
    return dict(out)


@pytest.mark.parametrize("name", list(R.CASES))
def test_restatement_matches_g25(restated, name):
    assert R.compare_case(name, _as_got(restated[name]), ref=restated[name]) == []


def test_float32_restatement_within_the_bounds(restated):
    """the kernel's own roundings, emulated in numpy float32, pass the comparisons the GPU tests make"""
    for name in ("p_ray", "o_nrm"):
        got = R.restate_case(name, dtype=np.float32, knn=restated[name]["knn"])
        assert R.compare_case(name, got, ref=restated[name]) == []


def test_fixture_conditions(restated):
    fix = R.g25()
    assert os.path.getsize(R.GOLD) < 1024 * 1024
    assert fix["rast_p"].shape == (3, 48, 48, 4) and fix["rast2d"].shape == (64, 64, 4)
    r = restated["p_ray"]
    assert r["steps"] >= 2 and np.isnan(r["samples_y"]).any(), "propagation depth and the NaN path"
    assert (R.finish(r["samples_y"])[np.isnan(r["samples_y"]).any(-1)] == 0).all(), "the duplicate-position texel ends at colour 0"
    assert restated["p_mask"]["steps"] == 2 and (~restated["p_mask"]["map_mask"] & (fix["map_alpha"] > 0)).any()
    # two vertex records with one position (the hinge)
    assert (fix["verts"][-6] == fix["verts"][-3]).all() and not (fix["uvs"][-6] == fix["uvs"][-3]).all()


def test_undecided_nearest_texels_stay_under_the_cap(restated):
    for name, r in restated.items():
        best, d_best, d_second = r["nearest"]
        undecided = ~((d_second - d_best) > R.nearest_margin(d_second))
        assert undecided.sum() <= 0.005 * len(best), "%s: %d of %d" % (name, undecided.sum(), len(best))


# mistake -> the case whose comparisons must reject it
REJECTED_BY = {"normalize_after": "p_ray", "lt_k": "p_ray", "in_place": "p_ray", "self_dropped": "p_ray", "pending_included": "o_nrm", "ray_as_normal": "p_ray"}


@pytest.mark.parametrize("mistake", list(REJECTED_BY))
def test_mistakes_are_rejected(restated, mistake):
    name = REJECTED_BY[mistake]
    for dtype in (np.float64, np.float32):
        got = R.restate_case(name, dtype=dtype, mistakes={mistake}, knn=restated[name]["knn"])
        assert R.compare_case(name, got, ref=restated[name]) != [], "%s passed the comparisons of %s" % (mistake, name)


def test_no_wrap_is_rejected():
    """the views of G25 do not cross the image edge, so the mask comparison is made on them rolled by half a width: torch.roll's wrap keeps the samples
    next to the edge, the mistake drops them"""
    fix = R.g25()
    rast = np.roll(fix["rast_p"], 24, axis=2)
    uv = fix["uvs"] * np.float32(2) - np.float32(1)
    a = R.view_samples(rast, fix["faces"], uv, fix["v_pos_cam_p"], fix["v_nrm_cam_p"])[2]
    b = R.view_samples(rast, fix["faces"], uv, fix["v_pos_cam_p"], fix["v_nrm_cam_p"], mistakes={"no_wrap"})[2]
    assert (rast[:, :, 0, 3] > 0).any() and (rast[:, :, -1, 3] > 0).any()
    assert not np.array_equal(a, b) and (b <= a).all()
    assert np.array_equal(np.roll(a, -24, axis=2), R.view_samples(fix["rast_p"], fix["faces"], uv, fix["v_pos_cam_p"], fix["v_nrm_cam_p"])[2])


def test_stuck_island_and_step_cap():
    """six points: 0-2 known, 3 pending next to them, 4-5 a pending island far away whose lists (k = 3) hold one known point at most"""
    pos = np.array([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [0.05, 0.05, 0], [0.9, 0.9, 0], [0.9, 0.8, 0]], np.float32)
    idx, d = R.knn_self(pos, 3)
    nrm = np.tile(np.float32([0, 0, 1]), (6, 1))
    col = np.array([[0.2], [0.4], [0.6], [0], [0], [0]], np.float64)
    pend = np.array([0, 0, 0, 1, 1, 1], bool)
    y, p, steps, trace, _ = R.inpaint(idx, d * d, nrm, col, pend)
    assert steps == 1 and trace[0].tolist() == [False, False, False, True, False, False] and p.tolist() == [False] * 4 + [True, True]
    assert 0.2 < y[3, 0] < 0.6 and (y[4:] == 0).all()
    assert R.inpaint(idx, d * d, nrm, col, pend, n_iters_max=0)[2] == 0


def test_abi_declares_the_two_functions():
    from unitex_amd import _lib
    for name, nargs in (("utx_view_samples", 21), ("utx_knn_inpaint_step", 13)):
        restype, argtypes = _lib.SYMBOLS[name]
        assert restype is ctypes.c_int and len(argtypes) == nargs
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "unitex_hip.h")).read()
    assert "int utx_view_samples(" in header and "int utx_knn_inpaint_step(" in header

"""Sliced optimal-transport colour transfer (unitex_amd/csrc/color_transfer.hip, ops.color_transfer_ot / ops.bilateral_filter, color_transfer_ot.CTSOT), CPU
side: the sequential-float32 restatement (tests/support/color_transfer_ref.py) against the reference's own output (G26, bit for bit, with no two projections
equal), the key map's order, the bilateral restatement in float32 against float64 with the radius rule, signatures and refusals, the C ABI's -2 returns before
any device call, and the agreement of header, bindings and exports."""
import inspect
import os

import numpy as np
import pytest

from tests.support import color_transfer_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", R.G26_CASES)
def test_restatement_equals_the_reference_output_bit_for_bit(name):
    c = R.g26()[name]
    assert c["src"].dtype == np.float32 and c["out"].dtype == np.float32 and c["dirs"].shape == (c["steps"] * c["batch"], c["src"].shape[-1])
    assert {"a": ((37, 29, 3), 3, 2), "b": ((16, 9, 4), 2, 5)}[name] == (c["src"].shape, c["steps"], c["batch"])
    ties = []
    got = R.ot_loop(c["src"], c["dst"], c["dirs"], c["steps"], c["batch"], ties=ties)
    assert len(ties) == c["steps"] * c["batch"] and all(t == (0, 0) for t in ties), ties      # the fixture does not depend on a tie order
    assert got.tobytes() == c["out"].tobytes()
    assert np.abs(c["out"] - c["src"]).max() > 0.05      # and the loop did move the colours
    n = np.linalg.norm(c["dirs"].astype(np.float64), axis=1)
    assert np.abs(n - 1).max() < 1e-6
    assert os.path.getsize(R.GOLDEN) < 64 * 1024


def test_key_map_is_monotone_and_invertible():
    tiny = np.float32(1e-45)
    grid = np.array([-np.inf, -3.4028235e38, -1.5, -1.0, -1.1754944e-38, -2 * tiny, -tiny, -0.0, 0.0, tiny, 2 * tiny, 1.1754944e-38, 1e-3, 1.0,
                     np.nextafter(np.float32(1), np.float32(2)), 3.4028235e38, np.inf], np.float32)
    k = R.keys(grid)
    assert k.dtype == np.uint32 and (np.diff(k.astype(np.int64)) > 0).all()      # strictly increasing: -0 before +0, denormals in order
    assert R.unkeys(k).tobytes() == grid.tobytes()
    rng = np.random.default_rng(5)
    bits = rng.integers(0, 2 ** 32, 20000, dtype=np.uint64).astype(np.uint32)
    f = bits.view(np.float32)
    f = f[np.isfinite(f)]
    order = np.argsort(R.keys(f), kind="stable")
    s = f[order]
    assert (np.diff(s.astype(np.float64)) >= 0).all() and R.unkeys(R.keys(f)).tobytes() == f.tobytes()
    # the stable sort on the keys: equal values keep ascending index, -0 sorts before +0
    v = np.array([0.0, 1.0, -0.0, 1.0, 0.0, -0.0], np.float32)
    assert np.argsort(R.keys(v), kind="stable").tolist() == [2, 5, 0, 4, 1, 3]


def test_ot_loop_properties_of_the_restatement():
    rng = np.random.default_rng(9)
    src = rng.uniform(0, 1, (11, 13, 3)).astype(np.float32)
    dst = rng.uniform(0, 1, (11, 13, 3)).astype(np.float32)
    dirs = rng.normal(size=(6, 3)).astype(np.float32)
    dirs = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
    assert R.ot_loop(src, src, dirs, 3, 2).tobytes() == src.tobytes()      # equal ranks carry equal projections: nothing moves
    perm = rng.permutation(11 * 13)
    a = R.ot_loop(src, dst, dirs, 3, 2)
    b = R.ot_loop(src, dst.reshape(-1, 3)[perm].reshape(dst.shape), dirs, 3, 2)
    assert a.tobytes() == b.tobytes()      # only the sorted target projections enter
    assert R.ot_loop(src, dst, dirs[:0], 0, 5).tobytes() == src.tobytes()
    # one step, one direction, one channel: the result is dst's values in src's rank order
    s1, d1 = src[..., :1], dst[..., :1]
    out = R.ot_loop(s1, d1, np.ones((1, 1), np.float32), 1, 1).reshape(-1)
    assert np.abs(np.sort(out) - np.sort(d1.reshape(-1))).max() <= 2 ** -23 and (np.argsort(out) == np.argsort(s1.reshape(-1))).all()


def test_bilateral_radius_rule_and_space_table():
    from unitex_amd.texturetools import ops
    for sigma, r in ((0.5, 1), (1.0, 2), (3.0, 4), (16.0, 24), (0.1, 1), (0.25, 1), (5.0, 8), (7.0, 10), (2.0, 3), (18.0, 27)):
        assert R.bilateral_radius(sigma) == r and ops.bilateral_radius(sigma) == r, sigma      # 0.5 -> 1 by the floor of 1, 1.5 -> 2 and 4.5 -> 4: halves to even
    for sigma in R.BILATERAL_SIGMA_SPACE:
        t = R.space_weights(sigma)
        r = R.bilateral_radius(sigma)
        assert t.dtype == np.float32 and t.shape == (r + 1, r + 1) and t[0, 0] == 1.0 and (t == t.T).all()
        assert t.tobytes() == ops.bilateral_space_weights(sigma).tobytes()
        assert t[1, 1] == np.float32(np.exp(-2.0 / (2.0 * sigma * sigma))) and t[0, r] == np.float32(np.exp(-float(r * r) / (2.0 * sigma * sigma)))
    assert ops.BILATERAL_RADIUS_MAX >= 24      # the default sigma_space = 16 is accepted


def test_bilateral_float32_restatement_against_float64():
    """d = max |float32 - float64| per case is what the GPU test's bound 4 d is made of: reference-side on both ends"""
    worst = 0.0
    for (H, W) in R.BILATERAL_SIZES[:5]:
        for ss in R.BILATERAL_SIGMA_SPACE:
            for sc in R.BILATERAL_SIGMA_COLOR:
                for C in (1, 3):
                    c = R.bilateral_case(H, W, C, sc, ss)
                    worst = max(worst, c["d"])
                    assert c["f32"].dtype == np.float32 and c["f64"].dtype == np.float64 and c["f32"].shape == (H, W, C)
                    # a weighted mean of values in [0.1, 0.9] with up to 1961 taps: the float32 sums stay within a few hundred ulps of the float64 ones
                    assert c["d"] <= 1961 * 2.0 ** -24, (H, W, ss, sc, C, c["d"])
                    lo, hi = float(c["img"].min()), float(c["img"].max())
                    assert (c["f64"] >= lo - 1e-12).all() and (c["f64"] <= hi + 1e-12).all()      # a convex combination
    print("bilateral: worst d over the small cases = %.3g" % worst)
    # 1 x 1: every tap is the pixel itself
    c = R.bilateral_case(1, 1, 3, 0.05, 16.0)
    assert np.abs(c["f64"] - c["img"]).max() <= 2000 * 2.0 ** -52      # 1809 equal terms summed in float64
    # a constant image stays constant; a wide colour sigma on a small window is a Gaussian blur, a narrow one keeps an edge
    const = np.full((9, 7, 3), 0.25, np.float32)
    assert np.abs(R.bilateral(const, 5.0, 3.0, np.float64) - 0.25).max() <= 2000 * 2.0 ** -52
    edge = np.zeros((9, 12, 1), np.float32)
    edge[:, 6:] = 1.0
    assert np.abs(R.bilateral(edge, 0.05, 3.0, np.float64) - edge).max() < 1e-6
    assert 0.2 < R.bilateral(edge, 5.0, 3.0, np.float64)[4, 5, 0] < 0.5
    # reflect-101, repeatedly: 5 pixels, offsets far beyond the image
    assert R.reflect101(np.arange(-9, 14), 5).tolist() == [1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2, 3, 4, 3, 2, 1, 0, 1, 2, 3, 4, 3]
    assert R.reflect101(np.arange(-3, 4), 1).tolist() == [0] * 7


def test_signatures_defaults_and_refusals():
    import torch
    from unitex_amd.texturetools import color_transfer_ot as CT, image_fusion as IF, ops
    sig = inspect.signature(CT.CTSOT)
    assert list(sig.parameters) == ["src", "dst", "steps", "batch_size", "reg_sigmaXY", "reg_sigmaV", "dirs"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [10, 5, 16.0, 5.0, None]
    assert list(inspect.signature(ops.color_transfer_ot).parameters) == ["src", "dst", "dirs", "steps", "batch_size"]
    assert list(inspect.signature(ops.bilateral_filter).parameters) == ["img", "sigma_color", "sigma_space"]
    assert "read-back" in CT.CTSOT.__doc__ and "read-back" in ops.color_transfer_ot.__doc__
    # the directions: the reference's calls on numpy's global generator
    np.random.seed(7)
    a = CT.draw_directions(2, 3, 3)
    np.random.seed(7)
    for k in range(6):
        d = np.random.normal(size=(3,)).astype(np.float32)
        assert (d / np.linalg.norm(d, axis=-1)).tobytes() == a[k].tobytes()
    assert a.dtype == np.float32 and a.shape == (6, 3)
    # refusals by name, before any device is touched
    x = torch.zeros(4, 5, 3)
    with pytest.raises(ValueError, match="CUDA"):
        CT.CTSOT(x, x)
    with pytest.raises(ValueError, match="one shape"):
        CT.CTSOT(x, torch.zeros(4, 5, 4))
    with pytest.raises(ValueError, match="channels"):
        CT.CTSOT(torch.zeros(4, 5, 5), torch.zeros(4, 5, 5))
    with pytest.raises(ValueError, match="regularisation"):
        CT.CTSOT(torch.zeros(4, 5, 4), torch.zeros(4, 5, 4))
    with pytest.raises(ValueError, match="regularisation"):
        CT.CTSOT(torch.zeros(4, 5, 2), torch.zeros(4, 5, 2), reg_sigmaXY=2.0)
    with pytest.raises(ValueError, match="batch_size"):
        CT.CTSOT(x, x, batch_size=0)
    with pytest.raises(ValueError, match="steps"):
        CT.CTSOT(x, x, steps=-1)
    with pytest.raises(ValueError, match="CUDA"):
        ops.color_transfer_ot(x, x, torch.zeros(2, 3), 1, 2)
    with pytest.raises(ValueError, match="batch_size"):
        ops.color_transfer_ot(x, x, torch.zeros(0, 3), 1, 0)
    with pytest.raises(ValueError, match="CUDA"):
        ops.bilateral_filter(x, 5.0, 16.0)
    with pytest.raises(NotImplementedError, match="color_transfer=True"):      # the HSV shift of image_fusion stays refused
        IF.image_fusion(x[None], x[None], x[None, ..., :1], color_transfer=True)
    assert "CTSOT" in IF.__doc__


def test_header_bindings_exports_and_constants_agree():
    from unitex_amd import _lib
    from unitex_amd.csrc import build as b
    from unitex_amd.texturetools import ops
    lib = _lib.load_library()
    hdr = open(os.path.join(ROOT, "include", "unitex_hip.h")).read()
    for name, nargs in (("utx_color_transfer_ot_workspace_bytes", 2), ("utx_color_transfer_ot", 12), ("utx_bilateral_lds_bytes", 2), ("utx_bilateral_filter", 10)):
        assert name in _lib.SYMBOLS and hasattr(lib, name) and ("%s(" % name) in hdr
        assert len(_lib.SYMBOLS[name][1]) == nargs, name
    assert "#define UTX_COLOR_TRANSFER_N_MAX %dL" % ops.COLOR_TRANSFER_N_MAX in hdr and ops.COLOR_TRANSFER_N_MAX == 2 ** 30
    assert "#define UTX_BILATERAL_RADIUS_MAX %d\n" % ops.BILATERAL_RADIUS_MAX in hdr and "#define UTX_BILATERAL_SIDE_MAX %d\n" % ops.BILATERAL_SIDE_MAX in hdr
    flags = dict(b.SOURCES)["color_transfer.hip"]
    assert "-ffp-contract=off" in flags and all(f in flags for f in b.NO_PK)
    # the radius cap is the largest radius whose 3-channel tile (16 + 2 r)^2 x 12 bytes plus the (r + 1)^2 x 4 byte table fits the 64 KiB of a plain launch
    R_ = ops.BILATERAL_RADIUS_MAX
    assert lib.utx_bilateral_lds_bytes(24, 3) == 64 * 64 * 12 + 25 * 25 * 4 == 51652
    assert lib.utx_bilateral_lds_bytes(R_, 3) == (16 + 2 * R_) ** 2 * 12 + (R_ + 1) ** 2 * 4 <= 65536 < lib.utx_bilateral_lds_bytes(R_ + 1, 3)
    assert lib.utx_bilateral_lds_bytes(0, 3) == -2 and lib.utx_bilateral_lds_bytes(4, 5) == -2
    readme = open(os.path.join(ROOT, "README.md")).read()
    import re
    src = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    n = len(set(re.findall(r"\b(utx_[a-z0-9_]+)\s*\(", src)))
    assert "(%d functions)" % n in readme


def test_c_abi_refuses_bad_arguments_before_any_device_call():
    import ctypes as C
    from unitex_amd import _lib
    lib = _lib.load_library()
    buf = (C.c_char * 8192)()
    a = (C.addressof(buf) + 255) & ~255
    p = lambda off=0: C.c_void_p(a + off)
    wsb = lib.utx_color_transfer_ot_workspace_bytes
    assert wsb(0, 3) == 0 and wsb(2 ** 30, 3) == 0 and wsb(10, 0) == 0 and wsb(10, 5) == 0
    sizes = [int(wsb(n, 3)) for n in (1, 100, 10007, 300 * 301, 2048 * 2048)]
    assert all(x < y for x, y in zip(sizes, sizes[1:])) and sizes[-1] >= 2048 * 2048 * (6 * 4 + 3 * 4)
    assert wsb(2048 * 2048, 4) >= wsb(2048 * 2048, 3) + 2048 * 2048 * 4
    good = dict(src=p(), dst=p(512), dirs=p(1024), N=4, C=3, steps=1, batch=2, out=p(1536), work=p(2048), wb=10 ** 6)
    ot = lambda **k: lib.utx_color_transfer_ot(None, *[{**good, **k}[n] for n in ("src", "dst", "dirs", "N", "C", "steps", "batch", "out", "work", "wb")], None)
    for k in (dict(N=0), dict(N=-1), dict(N=2 ** 30), dict(C=0), dict(C=5), dict(steps=-1), dict(batch=0), dict(batch=-2), dict(src=None), dict(dst=None),
              dict(dirs=None), dict(out=None), dict(work=None), dict(out=p()), dict(out=p(512)), dict(src=p(1)), dict(dst=p(514)), dict(out=p(1538)),
              dict(dirs=p(1025)), dict(wb=int(wsb(4, 3)) - 1), dict(wb=0)):
        assert ot(**k) == -2, k
    good = dict(img=p(), H=4, W=4, C=3, r=2, ws=p(1024), coef=-0.5, out=p(2048))
    bf = lambda **k: lib.utx_bilateral_filter(None, *[{**good, **k}[n] for n in ("img", "H", "W", "C", "r", "ws", "coef", "out")], None)
    for k in (dict(H=0), dict(W=0), dict(H=32769), dict(W=32769), dict(H=32768, W=32768), dict(C=0), dict(C=2), dict(C=4), dict(r=0), dict(r=28), dict(r=-1),
              dict(coef=0.25), dict(coef=float("nan")), dict(img=None), dict(ws=None), dict(out=None), dict(out=p()), dict(img=p(2)), dict(ws=p(1026)),
              dict(out=p(2049))):
        assert bf(**k) == -2, k

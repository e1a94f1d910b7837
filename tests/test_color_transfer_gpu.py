"""Sliced optimal-transport colour transfer on the GPU: utx_color_transfer_ot through ops.color_transfer_ot BIT FOR BIT against the sequential-float32
restatement (tests/support/color_transfer_ref.py) and against the reference's own output (G26); utx_bilateral_filter through ops.bilateral_filter against the
float64 restatement with the per-case bound 4 d, d = max |float32 restatement - float64 restatement| measured on the CPU; CTSOT against the composition of the
two ops.

Measured on the first MI355X run (DESIGN 8 "Colour transfer" has the table): the OT loop equals the restatement and G26 bit for bit on every case; over the 96
bilateral cases |gpu - float64| is at most 1.23 d (worst 2.26e-6 at r = 24 with d = 2.26e-6), |gpu - float32 restatement| at most 2.98e-7, 28 cases bit-equal."""
import numpy as np
import pytest
import torch

from tests.support import color_transfer_ref as R

pytestmark = pytest.mark.gpu


def _cuda(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()      # a copy: the shared cases are read-only


def _dirs(rng, n, C):
    d = rng.normal(size=(n, C)).astype(np.float32)
    return (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)


def _images(seed, shape):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.2, 1.2, shape).astype(np.float32), (rng.uniform(0, 1, shape) ** 2).astype(np.float32), rng


def _run(src, dst, dirs, steps, batch):
    from unitex_amd.texturetools import ops
    return ops.color_transfer_ot(_cuda(src), _cuda(dst), _cuda(dirs), steps, batch).cpu().numpy()


# N = 1, around the wave (64) and the block (256), odd sizes, and one size above rocPRIM's single-block sorts (300 x 301 = 90300)
@pytest.mark.parametrize("N", [1, 63, 64, 65, 255, 256, 257, 1073, 4099, 300 * 301])
@pytest.mark.parametrize("C", [1, 3, 4])
def test_ot_loop_equals_the_restatement_bit_for_bit(N, C):
    src, dst, rng = _images(N * 10 + C, (N, C))
    dirs = _dirs(rng, 6, C)
    got = _run(src, dst, dirs, 3, 2)
    assert got.dtype == np.float32 and got.shape == (N, C)
    assert got.tobytes() == R.ot_loop(src, dst, dirs, 3, 2).tobytes()


@pytest.mark.parametrize("steps,batch", [(1, 1), (3, 2), (2, 5), (10, 5)])
def test_ot_loop_steps_and_batches(steps, batch):
    src, dst, rng = _images(100 * steps + batch, (37, 29, 3))
    dirs = _dirs(rng, steps * batch, 3)
    got = _run(src, dst, dirs, steps, batch)
    assert got.shape == (37, 29, 3) and got.tobytes() == R.ot_loop(src, dst, dirs, steps, batch).tobytes()


@pytest.mark.parametrize("name", R.G26_CASES)
def test_g26_the_reference_output_straight_against_the_kernel(name):
    c = R.g26()[name]
    got = _run(c["src"], c["dst"], c["dirs"], c["steps"], c["batch"])
    assert got.tobytes() == c["out"].tobytes()


def test_tied_inputs_follow_the_library_tie_rule():
    """equal projections: the stable sort gives them ascending pixel order, as the restatement's stable argsort does"""
    rng = np.random.default_rng(77)
    dirs = _dirs(rng, 6, 3)
    const = np.full((19, 23, 3), 0.375, np.float32)
    other = rng.uniform(0, 1, (19, 23, 3)).astype(np.float32)
    quant_a = (rng.integers(0, 256, (40, 33, 3)).astype(np.float32) / np.float32(255.0)).astype(np.float32)      # 3960 pixels on 256 levels per channel
    quant_b = (rng.integers(0, 8, (40, 33, 3)).astype(np.float32) / np.float32(7.0)).astype(np.float32)      # ... and on 8: hundreds of equal projections
    zeros = np.zeros((16, 17, 3), np.float32)
    zeros[::2] = -0.0
    zeros[:, ::3, 1] = 0.5
    zdst = np.where(rng.uniform(0, 1, zeros.shape) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    for src, dst in ((const, other), (other, const), (const, const), (quant_a, quant_b), (quant_b, quant_a), (zeros, zdst), (zdst, zeros)):
        ties = []
        want = R.ot_loop(src, dst, dirs, 3, 2, ties=ties)
        assert sum(a + b for a, b in ties) > 0      # the case does have ties
        assert _run(src, dst, dirs, 3, 2).tobytes() == want.tobytes()
    # one channel and the axis itself as direction: -0 and +0 are told apart by the key order alone
    z1 = np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0], np.float32).reshape(6, 1)
    d1 = np.array([3.0, -2.0, -0.0, 0.0, 5.0, 4.0], np.float32).reshape(6, 1)
    one = np.ones((1, 1), np.float32)
    assert _run(z1, d1, one, 1, 1).tobytes() == R.ot_loop(z1, d1, one, 1, 1).tobytes()


def test_ot_loop_properties():
    from unitex_amd.texturetools import ops
    src, dst, rng = _images(5, (31, 17, 3))
    dirs = _dirs(rng, 6, 3)
    s, d, dd = _cuda(src), _cuda(dst), _cuda(dirs)
    keep = s.clone()
    a = ops.color_transfer_ot(s, d, dd, 3, 2)
    assert torch.equal(s, keep) and a.data_ptr() != s.data_ptr()
    assert torch.equal(a, ops.color_transfer_ot(s, d, dd, 3, 2))      # two runs, the same bits
    assert torch.equal(ops.color_transfer_ot(s, s, dd, 3, 2), s)      # dst = src: equal ranks carry equal projections
    assert torch.equal(ops.color_transfer_ot(s, s.clone(), dd, 3, 2), s)
    perm = torch.from_numpy(rng.permutation(31 * 17)).cuda()
    assert torch.equal(a, ops.color_transfer_ot(s, d.reshape(-1, 3)[perm].reshape(d.shape).contiguous(), dd, 3, 2))      # dst's pixel order does not enter
    z = ops.color_transfer_ot(s, d, dd[:0], 0, 5)      # steps = 0: a copy
    assert torch.equal(z, s) and z.data_ptr() != s.data_ptr()
    # the transfer does what it is for: the projections onto a fresh direction are distributed as dst's
    out = ops.color_transfer_ot(s, d, _cuda(_dirs(rng, 50, 3)), 10, 5).cpu().numpy().reshape(-1, 3)
    e = np.array([0.6, 0.0, 0.8], np.float32)
    gap = lambda x: np.abs(np.sort(x @ e) - np.sort(dst.reshape(-1, 3) @ e)).mean()
    assert gap(out) < 0.2 * gap(src.reshape(-1, 3))
    # refusals by name
    with pytest.raises(ValueError, match="channels"):
        ops.color_transfer_ot(torch.zeros(4, 5, device="cuda"), torch.zeros(4, 5, device="cuda"), torch.zeros(2, 5, device="cuda"), 1, 2)
    with pytest.raises(ValueError, match="pixels"):
        ops.color_transfer_ot(torch.zeros(0, 3, device="cuda"), torch.zeros(0, 3, device="cuda"), dd, 3, 2)
    with pytest.raises(ValueError, match="dirs"):
        ops.color_transfer_ot(s, d, dd, 3, 3)
    with pytest.raises(ValueError, match="float32"):
        ops.color_transfer_ot(s.double(), d.double(), dd, 3, 2)
    with pytest.raises(ValueError, match="one shape"):
        ops.color_transfer_ot(s, d[:-1], dd, 3, 2)


def test_abi_sentinels_and_refusals_leave_the_output_alone():
    from unitex_amd._lib import ptr
    from unitex_amd.flux.ops import get_ctx
    ctx = get_ctx(0)
    src, dst, rng = _images(6, (65, 3))
    dirs = _dirs(rng, 2, 3)
    s, d, dd = _cuda(src), _cuda(dst), _cuda(dirs)
    N, C, pad, SENT = 65, 3, 64, 12345.0
    out = torch.full((pad + N * C + pad,), SENT, dtype=torch.float32, device="cuda")
    wb = int(ctx.lib.utx_color_transfer_ot_workspace_bytes(N, C))
    work = torch.full((wb + 512,), 0xAB, dtype=torch.uint8, device="cuda")
    call = lambda **k: ctx.lib.utx_color_transfer_ot(ctx.handle, ptr(s), ptr(d), ptr(dd), k.get("N", N), k.get("C", C), k.get("steps", 1), k.get("batch", 2),
                                                     ptr(out[pad:]), ptr(work[256:]), k.get("wb", wb), ctx.stream())
    assert call(C=5) == -2 and call(N=0) == -2 and call(steps=-1) == -2 and call(batch=0) == -2 and call(wb=wb - 1) == -2
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((work == 0xAB).all())
    ctx.check(call())
    torch.cuda.synchronize()
    o, w = out.cpu().numpy(), work.cpu().numpy()
    assert (o[:pad] == SENT).all() and (o[pad + N * C:] == SENT).all()      # nothing outside out ...
    assert (w[:256] == 0xAB).all() and (w[256 + wb:] == 0xAB).all()      # ... or outside the workspace is written
    assert o[pad:pad + N * C].tobytes() == R.ot_loop(src, dst, dirs, 1, 2).tobytes()


@pytest.mark.parametrize("H,W", R.BILATERAL_SIZES)
@pytest.mark.parametrize("sigma_space", R.BILATERAL_SIGMA_SPACE)
def test_bilateral_against_the_float64_restatement(H, W, sigma_space):
    from unitex_amd.texturetools import ops
    for sigma_color in R.BILATERAL_SIGMA_COLOR:
        for C in (1, 3):
            c = R.bilateral_case(H, W, C, sigma_color, sigma_space)
            img = _cuda(c["img"])
            got = ops.bilateral_filter(img, sigma_color, sigma_space)
            assert got.dtype == torch.float32 and tuple(got.shape) == (H, W, C) and got.data_ptr() != img.data_ptr()
            g = got.cpu().numpy()
            dev = float(np.abs(g.astype(np.float64) - c["f64"]).max())
            d32 = float(np.abs(g.astype(np.float64) - c["f32"].astype(np.float64)).max())
            print("bilateral %dx%dx%d sigma_space %g (r %d) sigma_color %g: |gpu - float64| = %.3g, |gpu - float32 restatement| = %.3g, d = %.3g, bound 4 d = %.3g"
                  % (H, W, C, sigma_space, R.bilateral_radius(sigma_space), sigma_color, dev, d32, c["d"], c["bound"]))
            assert dev <= c["bound"], (H, W, C, sigma_space, sigma_color, dev, c["d"])
            assert torch.equal(got, ops.bilateral_filter(img, sigma_color, sigma_space))      # two runs, the same bits


def test_bilateral_refusals_and_radius_cap():
    from unitex_amd.texturetools import ops
    img = torch.zeros(8, 9, 3, device="cuda")
    assert float((ops.bilateral_filter(img + 0.25, 5.0, 18.0) - 0.25).abs().max()) < 1e-6      # r = 27 = BILATERAL_RADIUS_MAX on an image smaller than the window
    with pytest.raises(ValueError, match="BILATERAL_RADIUS_MAX"):
        ops.bilateral_filter(img, 5.0, 19.0)      # r = 28
    with pytest.raises(ValueError, match="C 1 or 3"):
        ops.bilateral_filter(torch.zeros(8, 9, 4, device="cuda"), 5.0, 2.0)
    with pytest.raises(ValueError, match="positive"):
        ops.bilateral_filter(img, 0.0, 2.0)
    with pytest.raises(ValueError, match="positive"):
        ops.bilateral_filter(img, 5.0, -1.0)
    with pytest.raises(ValueError, match="float32"):
        ops.bilateral_filter(img.double(), 5.0, 2.0)


def test_ctsot_is_the_composition_and_draws_the_reference_directions():
    from unitex_amd.texturetools import color_transfer_ot as CT, ops
    src, dst, rng = _images(12, (33, 31, 3))
    s, d = _cuda(src), _cuda(dst)
    dirs = _dirs(rng, 6, 3)
    new = ops.color_transfer_ot(s, d, _cuda(dirs), 3, 2)
    assert torch.equal(CT.CTSOT(s, d, steps=3, batch_size=2, reg_sigmaXY=0.0, dirs=dirs), new)
    want = s + ops.bilateral_filter(new - s, 5.0, 3.0)
    got = CT.CTSOT(s, d, steps=3, batch_size=2, reg_sigmaXY=3.0, reg_sigmaV=5.0, dirs=_cuda(dirs))
    assert torch.equal(got, want) and not torch.equal(got, new)
    # no dirs: numpy's global generator, the reference's draws; a seeded caller gets the recorded directions
    for k in (0, 3):
        np.random.seed(k)
        rec = CT.draw_directions(3, 2, 3)
        np.random.seed(k)
        a = CT.CTSOT(s, d, steps=3, batch_size=2, reg_sigmaXY=3.0)
        assert torch.equal(a, CT.CTSOT(s, d, steps=3, batch_size=2, reg_sigmaXY=3.0, dirs=rec))
    # the defaults (10 steps, 5 batches, sigma 16 -> r = 24), one and four channels
    np.random.seed(1)
    out = CT.CTSOT(s, d)
    assert tuple(out.shape) == (33, 31, 3) and bool(torch.isfinite(out).all())
    c = R.g26()["b"]
    assert CT.CTSOT(_cuda(c["src"]), _cuda(c["dst"]), steps=c["steps"], batch_size=c["batch"], reg_sigmaXY=0.0, dirs=c["dirs"]).cpu().numpy().tobytes() == c["out"].tobytes()
    one = CT.CTSOT(s[..., :1].contiguous(), d[..., :1].contiguous(), steps=2, batch_size=2, reg_sigmaXY=1.0)
    assert tuple(one.shape) == (33, 31, 1)
    assert torch.equal(CT.CTSOT(s, d, steps=0), s)      # nothing moved: the filter of a zero displacement is zero
    with pytest.raises(ValueError, match="regularisation"):
        CT.CTSOT(_cuda(c["src"]), _cuda(c["dst"]))

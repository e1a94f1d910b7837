"""Pins oracle/dit_glue_fp64.py (the float64 reference the GPU edge tests judge the DiT glue kernels by) against the float32 restatement
oracle/dit_ref.py on random data, before it judges a kernel.  CPU only.

The two references round to bf16 at the same tensor boundaries and differ only in the precision of what lies between them, so they agree bit
for bit except where a float32 statistic moves a value across a bf16 rounding boundary: at most one bf16 step per rounded intermediate."""
import numpy as np
import torch

from oracle import dit_glue_fp64 as R64
from oracle import dit_ref

BF = torch.bfloat16


def _bf(t):
    return t.to(BF).float()


def _ulp(a):
    """bf16 spacing in the binade of |a| (8 significant bits)"""
    a = np.maximum(np.abs(a), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 7)


def test_bf16_rounding_is_round_to_nearest_even_straight_from_float64():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1 << 16, generator=g) * torch.exp(8 * torch.randn(1 << 16, generator=g))
    assert np.array_equal(R64.bf16(x.double().numpy()), _bf(x).double().numpy())            # float32 values: torch's conversion is the definition
    every = torch.arange(-(1 << 15), 1 << 15, dtype=torch.int32).to(torch.int16).view(BF).float()
    every = every[torch.isfinite(every)]
    assert np.array_equal(R64.bf16(every.double().numpy()), every.double().numpy())         # every finite bf16 is a fixed point
    # 1 + 2^-8 is the tie between 1 and 1 + 2^-7: a float64 just off the tie rounds to float32 ON the tie, and must still go to its own side
    tie = 1.0 + 2.0 ** -8
    got = R64.bf16(np.array([tie, tie + 2.0 ** -40, tie - 2.0 ** -40, -tie - 2.0 ** -40, 3.0 * 2.0 ** -9 + 1.0, 3.3895e38, 3.3962e38]))
    assert got.tolist() == [1.0, 1.0 + 2.0 ** -7, 1.0, -1.0 - 2.0 ** -7, 1.0 + 2.0 ** -7, 3.3895313892515355e38, float("inf")]


def test_ln_mod_and_qkv_post_agree_with_the_float32_restatement():
    """Same inputs as the GPU tests' randn cases.  Measured here: ln_mod 0.0003 % of the elements differ (cap 1 %), qkv_post 0.0013 % at
    q_scale 1 and 0.11 % at 0.1275 (cap 2 %), and no element by more than one bf16 step of each of the rounded values behind it."""
    g = torch.Generator().manual_seed(5)
    x = _bf(torch.randn(300, 3072, generator=g) * 2 + 0.3)
    shift, scale = _bf(torch.randn(3072, generator=g)), _bf(torch.randn(3072, generator=g) * 0.5)
    a = dit_ref.layer_norm_mod(x, shift, scale, 1e-6, True).double().numpy()
    b, t, gm, _, _ = R64.ln_mod(x.numpy(), shift.numpy(), scale.numpy(), 1e-6, parts=True)
    share = float((a != b).mean())
    print("ln_mod: float32 restatement differs from float64 on %.4f %% of the elements" % (100 * share))
    assert share < 0.01
    assert (np.abs(a - b) <= _ulp(t) * np.abs(gm) + _ulp(t * gm) * 2 + _ulp(b) * 2).all()
    H, S = 3, 200
    q = _bf(torch.randn(H, S, 128, generator=g))
    w = _bf(1 + 0.1 * torch.randn(128, generator=g))
    ids = torch.stack([torch.zeros(S), torch.arange(S) // 17, torch.arange(S) % 17], 1).float()
    cos, sin = dit_ref.rope_tables(ids)
    for qs in (1.0, 0.1275):
        a = _bf(dit_ref.apply_rope(dit_ref.rms_norm(q, w, 1e-6, True), cos, sin) * qs).double().numpy()
        b, t, r = R64.qkv_post(q.numpy(), w.numpy(), cos.numpy(), sin.numpy(), 1e-6, qs, parts=True)
        share = float((a != b).mean())
        print("qkv_post (q_scale %g): float32 restatement differs from float64 on %.4f %% of the elements" % (qs, 100 * share))
        assert share < 0.02
        assert (np.abs(a - b) <= 2 * _ulp(np.abs(r) + 1e-30)).all()


def test_gemv_sched_step_add3_agree_with_the_float32_restatement():
    g = torch.Generator().manual_seed(3)
    x = _bf(torch.randn(3, 520, generator=g))
    W = _bf(torch.randn(37, 520, generator=g) / 16)
    bias = _bf(torch.randn(37, generator=g))
    for si, so in ((False, False), (True, False), (False, True), (True, True)):
        xin = _bf(dit_ref.silu(x)) if si else x
        a = _bf(xin @ W.t() + bias)
        a = _bf(dit_ref.silu(a)) if so else a
        b = R64.gemv(x.numpy(), W.numpy(), bias.numpy(), si, so)
        assert (np.abs(a.double().numpy() - b) <= _ulp(b)).all() and float((a.double().numpy() != b).mean()) < 0.05
    lat, v = _bf(torch.randn(4096, generator=g)), _bf(torch.randn(4096, generator=g))
    cond = _bf(torch.randn(1024, generator=g))
    a = dit_ref.euler_step(lat[:3072], v[:3072], 0.5, 0.5 - 0.0371).double().numpy()
    ds = np.float32(0.5 - 0.0371) - np.float32(0.5)
    b = R64.sched_step(lat.numpy(), v.numpy(), float(0.5 - 0.0371) - 0.5, 3072, cond.numpy())
    assert (np.abs(a - b[:3072]) <= _ulp(b[:3072])).all() and float((a != b[:3072]).mean()) < 0.01 and ds != 0
    assert np.array_equal(b[3072:], cond.double().numpy())
    assert np.array_equal(R64.sched_step(lat.numpy(), v.numpy(), -0.0371, 3072, None)[3072:], lat.double().numpy()[3072:])
    c = _bf(torch.randn(4096, generator=g))
    assert np.array_equal(R64.add3(lat.numpy(), v.numpy(), c.numpy()), _bf(_bf(lat + v) + c).double().numpy())      # bf16 + bf16 is exact in float32
    assert np.array_equal(R64.add3(lat.numpy(), None, c.numpy()), _bf(lat + c).double().numpy())

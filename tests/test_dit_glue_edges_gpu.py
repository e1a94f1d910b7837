"""The small kernels between the GEMMs and attention (dit_elementwise.hip, gemv_bf16_kernel) against the float64 reference
oracle/dit_glue_fp64.py, at the sizes where their launch geometry changes: one lane, a full pass, a pass and one lane, ragged last blocks, padded
rows, the scalar tail of the V^T store, the second trip of a grid-stride loop.

Every output buffer is larger than what the contract says is written and pre-filled with a sentinel; every test checks that the sentinel survives
outside that region.  Bounds are bit-equality or a counted number of roundings (u = 2^-24, the float32 unit roundoff; ulp(a) = the bf16 spacing in
the binade of a); none was tuned on a kernel's output.  The `_k_*` functions are the only place that touches the GPU: CPU tensors in, CPU tensors
out."""
import ctypes as C
import itertools

import numpy as np
import pytest
import torch

from oracle import dit_glue_fp64 as R64
from oracle import dit_ref
from oracle import mx8_ref

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
U = 2.0 ** -24
SENT16 = 0x4B5A         # a finite bf16 (about 1.4e7) that no test's data produces
SENT8 = 0xA5
EPS = 1e-6


# ------------------------------------------------------------------------------------------------ helpers (CPU)
def _sent_bf(*shape):
    return torch.full(shape, SENT16, dtype=torch.int16).view(BF)


def _sent_u8(*shape):
    return torch.full(shape, SENT8, dtype=torch.uint8)


def _bits(t):
    return t.contiguous().view(torch.int16).numpy()


def _f64(t):
    return t.double().numpy()


def _randbf(g, *shape, scale=1.0, shift=0.0):
    return (torch.randn(*shape, generator=g) * scale + shift).to(BF)


def _ulp(a):
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(a), 2.0 ** -126))) - 7)


def _assert_sentinel(buf, written, what):
    """buf: bf16 / uint8 CPU tensor, written: bool numpy mask of the region the contract writes"""
    raw = _bits(buf) if buf.dtype == BF else buf.numpy()
    sent = SENT16 if buf.dtype == BF else SENT8
    assert (raw[~written] == sent).all(), "%s: wrote outside its region (%d elements)" % (what, int((raw[~written] != sent).sum()))


# ------------------------------------------------------------------------------------------------ kernel calls
def _ctx():
    from unitex_amd.flux import ops
    return ops.get_ctx(0)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _dev(t):
    return None if t is None else t.cuda()


def _k_ln_mod(xbuf, shift, scale, ybuf, n_tok, D, ldx, ldy, q=None, ldq=0, qs=None, rb=0, via_plan=False, null=()):
    """-> (rc, ybuf, q, qs) after the launch; buffers are flat or 2-D CPU tensors"""
    from unitex_amd._lib import LnModDesc
    ctx = _ctx()
    x_d, sh_d, sc_d, y_d, q_d, qs_d = (_dev(t) for t in (xbuf, shift, scale, ybuf, q, qs))
    d = LnModDesc()
    d.x, d.ldx, d.shift, d.scale = _p(None if "x" in null else x_d), ldx, _p(None if "shift" in null else sh_d), _p(None if "scale" in null else sc_d)
    d.y, d.ldy, d.n_tok, d.D, d.eps = _p(y_d), ldy, n_tok, D, EPS
    d.q, d.ldq, d.qs, d.qs_row_blocks = _p(q_d), ldq, _p(qs_d), rb
    if via_plan:
        rc = _run_plan(lambda lib, h: lib.utx_plan_add_ln_mod(h, C.byref(d)))
    else:
        rc = ctx.lib.utx_ln_mod(ctx.handle, C.byref(d), ctx.stream())
    torch.cuda.synchronize()
    return rc, (None if y_d is None else y_d.cpu()), (None if q_d is None else q_d.cpu()), (None if qs_d is None else qs_d.cpu())


def _run_plan(add):
    """one-entry plan: utx_plan_run calls the launcher directly, without the checks of the utx_* entry point in front of it"""
    ctx = _ctx()
    h = C.c_void_p()
    assert ctx.lib.utx_plan_create(ctx.handle, C.byref(h)) == 0
    try:
        rc = add(ctx.lib, h)
        if rc == 0:
            bad = C.c_int(-1)
            rc = ctx.lib.utx_plan_run(h, ctx.stream(), C.byref(bad))
    finally:
        ctx.lib.utx_plan_free(h)
    return rc


def _k_quant(x, ldx, q, ldq, s, lds_or_rb, M, K, packed):
    ctx = _ctx()
    x_d, q_d, s_d = _dev(x), _dev(q), _dev(s)
    fn = ctx.lib.utx_quant_mx8_packed if packed else ctx.lib.utx_quant_mx8
    rc = fn(ctx.handle, _p(x_d), ldx, _p(q_d), ldq, _p(s_d), lds_or_rb, M, K, ctx.stream())
    torch.cuda.synchronize()
    return rc, q_d.cpu(), s_d.cpu()


def _k_qkv_post(qkv, ld, cols, wq, wk, cos, sin, Qh, Kh, Vt, hs_qk, hs_v, S_pad, n_tok, tok_off, H, q_scale=1.0, skip_qk=0, hpg=0, gs_qk=0, gs_v=0,
                sub=0, gs2_qk=0, gs2_v=0):
    from unitex_amd._lib import QkvPostDesc
    ctx = _ctx()
    t = [_dev(a) for a in (qkv, wq, wk, cos, sin, Qh, Kh, Vt)]
    d = QkvPostDesc()
    d.qkv, d.ld = _p(t[0]), ld
    d.q_col, d.k_col, d.v_col = cols
    d.wq, d.wk, d.cosb, d.sinb, d.Qh, d.Kh, d.Vt = (_p(a) for a in t[1:])
    d.hs_qk, d.hs_v, d.S_pad, d.n_tok, d.tok_off, d.H, d.eps, d.q_scale = hs_qk, hs_v, S_pad, n_tok, tok_off, H, EPS, q_scale
    d.heads_per_group, d.gs_qk, d.gs_v, d.skip_qk, d.sub_heads, d.gs2_qk, d.gs2_v = hpg, gs_qk, gs_v, skip_qk, sub, gs2_qk, gs2_v
    rc = ctx.lib.utx_qkv_post(ctx.handle, C.byref(d), ctx.stream())
    torch.cuda.synchronize()
    return rc, t[5].cpu(), t[6].cpu(), t[7].cpu()


class _Gemv:
    """device copies of one case's operands, made once (W is up to 6 MB)"""

    def __init__(self, **cpu):
        self.t = {k: _dev(v) for k, v in cpu.items()}

    def __call__(self, x, ldx, W, ldw, bias, y, ldy, M, N, K, silu_in, silu_out, via_plan=False, null=()):
        from unitex_amd._lib import GemvDesc
        ctx = _ctx()
        y_d = _dev(y)
        d = GemvDesc()
        d.x, d.ldx, d.W, d.ldw = _p(None if "x" in null else self.t[x]), ldx, _p(None if "W" in null else self.t[W]), ldw
        d.bias, d.y, d.ldy, d.M, d.N, d.K = _p(self.t[bias] if bias else None), _p(None if "y" in null else y_d), ldy, M, N, K
        d.silu_in, d.silu_out = int(silu_in), int(silu_out)
        if via_plan:
            rc = _run_plan(lambda lib, h: lib.utx_plan_add_gemv(h, C.byref(d)))
        else:
            rc = ctx.lib.utx_gemv_bf16(ctx.handle, C.byref(d), ctx.stream())
        torch.cuda.synchronize()
        return rc, y_d.cpu()


def _k_sched(x, v, cond, n_noise, n_total, dsigma):
    from unitex_amd._lib import SchedDesc
    ctx = _ctx()
    x_d, v_d, c_d = _dev(x), _dev(v), _dev(cond)
    d = SchedDesc()
    d.x, d.v, d.cond, d.n_noise_elems, d.n_total_elems, d.dsigma = _p(x_d), _p(v_d), _p(c_d), n_noise, n_total, dsigma
    rc = ctx.lib.utx_sched_step(ctx.handle, C.byref(d), ctx.stream())
    torch.cuda.synchronize()
    return rc, x_d.cpu()


def _k_add3(a, b, c, out, n):
    a_d, b_d, c_d, o_d = _dev(a), _dev(b), _dev(c), _dev(out)
    rc = _run_plan(lambda lib, h: lib.utx_plan_add_add3(h, _p(a_d), _p(b_d), _p(c_d), _p(o_d), n))
    torch.cuda.synchronize()
    return rc, o_d.cpu()


# ------------------------------------------------------------------------------------------------ ln_mod, bf16 form
def _ln_bound(x, shift, parts):
    """|kernel - reference| for one element, counted.  The kernel's float32 statistics: the mean is 64 adds in a lane + 6 shuffle levels + a division
    (em = 72 u mean|x| with slack), the variance the same depth over squares of (x - mean) that carry em, rstd an add, a square root and a division:
        dvar = 2 em sigma + em^2 + 76 u var,   drstd / rstd = dvar / (2 (var + eps)) + 8 u,
        dt   = rstd (em + u |x - mean|) + |x - mean| rstd (drstd / rstd + 2 u)          the error of (x - mean) rstd in front of its rounding.
    Then one bf16 step for each rounded value that dt can push across a boundary, carried through what follows (|bf(a) - bf(b)| <= |a - b| + ulp):
        e_n = dt + ulp(|t| + dt)                                  n = bf16(LN(x))
        e_m = e_n |g| + ulp(|n g| + e_n |g|)                      m = bf16(n g), g = bf16(1 + scale) exact on both sides, n g exact in float32
        e_o = e_m + u |m + shift| + ulp(|m + shift| + e_m)        out = bf16(m + shift), the sum rounded to float32 first in the kernel
    With exact statistics (dt -> 0) that is ulp(n) |g| + ulp(m) + ulp(out)."""
    out, t, g, mean, var = parts
    em = 72 * U * np.abs(x).mean(-1, keepdims=True)
    a, rstd = np.abs(x - mean), 1.0 / np.sqrt(var + R64.f32(EPS))
    dvar = 2 * em * np.sqrt(var) + em ** 2 + 76 * U * var
    dt = rstd * (em + U * a) + a * rstd * (0.5 * dvar / (var + R64.f32(EPS)) + 8 * U + 2 * U)
    e_n = dt + _ulp(np.abs(t) + dt)
    ng = R64.bf16(t) * g
    e_m = e_n * np.abs(g) + _ulp(np.abs(ng) + e_n * np.abs(g))
    s = R64.bf16(ng) + shift
    return e_m + U * np.abs(s) + _ulp(np.abs(s) + e_m)


def _ln_run(x, shift, scale, n_tok, pad, extra_rows=2):
    """-> y [n_tok, D] float64 after the sentinel check; x rows are laid out ldx = D + pad apart with a value in the padding that would wreck the
    statistics if it were read"""
    D = x.shape[1]
    ld = D + pad
    xbuf = torch.full((n_tok, ld), 3.0e38, dtype=BF)
    xbuf[:, :D] = x[:n_tok]
    ybuf = _sent_bf(n_tok + extra_rows, ld)
    rc, y, _, _ = _k_ln_mod(xbuf, shift, scale, ybuf, n_tok, D, ld, ld)
    assert rc == 0, "utx_ln_mod(D=%d, n_tok=%d, ld=%d) -> %d" % (D, n_tok, ld, rc)
    written = np.zeros((n_tok + extra_rows, ld), dtype=bool)
    written[:n_tok, :D] = True
    _assert_sentinel(y, written, "ln_mod D=%d n_tok=%d ld=%d" % (D, n_tok, ld))
    return _f64(y[:n_tok, :D])


@pytest.mark.parametrize("D", [8, 504, 512, 520, 3072, 4096])
def test_ln_mod_bf16_at_the_lane_and_pass_edges(D):
    """One wave per token, four tokens per block, a lane owns chunks lane + 64 it: D = 8 one lane, 504 = 63 chunks, 512 = exactly one pass, 520 = a
    second pass with one lane, 3072 production, 4096 the maximum; n_tok 1 / 5 / 300 (ragged last block); rows D, D + 8, D + 64 apart.
    Bound per element: _ln_bound (counted there).  Share of elements not bit-equal to the float64 reference on the randn rows: cap 1 % (the
    float32 restatement dit_ref measures 0.0003 % on the same kind of input, tests/test_dit_glue_ref_cpu.py; the kernel on an MI355X at most
    0.0013 %, and at most 0.69 of the bound)."""
    g = torch.Generator().manual_seed(100 + D)
    x = _randbf(g, 300, D, scale=2.0, shift=0.3)
    shift, scale = _randbf(g, D), _randbf(g, D, scale=0.5)
    xs, sh, sc = _f64(x), _f64(shift), _f64(scale)
    parts = R64.ln_mod(xs, sh, sc, EPS, parts=True)
    bound = _ln_bound(xs, sh, parts)
    for n_tok, pad in itertools.product((1, 5, 300), (0, 8, 64)):
        y = _ln_run(x, shift, scale, n_tok, pad)
        err = np.abs(y - parts[0][:n_tok])
        share = float((y != parts[0][:n_tok]).mean())
        print("ln_mod D=%d n_tok=%d pad=%d: max err / bound %.3f, %.4f %% not bit-equal" % (D, n_tok, pad, float((err / bound[:n_tok]).max()), 100 * share))
        assert (err <= bound[:n_tok]).all(), "ln_mod D=%d n_tok=%d pad=%d: %d elements outside the counted bound" % (D, n_tok, pad, int((err > bound[:n_tok]).sum()))
        if n_tok == 300:
            assert share < 0.01, "ln_mod D=%d: %.3f %% of the elements differ from the float64 reference" % (D, 100 * share)


@pytest.mark.parametrize("D", [520, 3072])
def test_ln_mod_bf16_degenerate_rows(D):
    """Rows judged by the counted bound only (_ln_bound), and exactly where the contract is exact:
      0  constant row: the float32 sums of D <= 4096 equal bf16 values are exact, variance 0, rstd = eps^-1/2, out == bf16(shift) bit for bit
      1  1000 + 0.25 randn: in bf16 (spacing 4 at 1000) this IS a constant row -- same claim
      2  1000 + 4 randn, the same row with a spread bf16 can hold: E[x^2] - mean^2 in float32 would lose it, the two-pass kernel stays in the bound
      3  a single nonzero element
      4  randn
    and scale = -1 everywhere: g = bf16(1 + scale) = 0, out == shift bit for bit on every row."""
    g = torch.Generator().manual_seed(200 + D)
    x = torch.zeros(5, D)
    x[0] = 2.71875
    x[1] = 1000 + 0.25 * torch.randn(D, generator=g)
    x[2] = 1000 + 4 * torch.randn(D, generator=g)
    x[3, D // 2 + 3] = -37.5
    x[4] = torch.randn(D, generator=g)
    x = x.to(BF)
    assert float(x[1].float().std()) == 0.0 and float(x[2].float().std()) > 2.0
    shift, scale = _randbf(g, D), _randbf(g, D, scale=0.5)
    xs, sh, sc = _f64(x), _f64(shift), _f64(scale)
    parts = R64.ln_mod(xs, sh, sc, EPS, parts=True)
    y = _ln_run(x, shift, scale, 5, 8)
    err, bound = np.abs(y - parts[0]), _ln_bound(xs, sh, parts)
    print("ln_mod degenerate rows D=%d: max err / bound per row %s" % (D, (err / bound).max(-1)))
    assert (err[2:] <= bound[2:]).all()
    assert np.array_equal(y[0], sh) and np.array_equal(y[1], sh), "constant row: out must equal bf16(shift)"
    y = _ln_run(x, shift, torch.full((D,), -1.0, dtype=BF), 5, 0)
    assert np.array_equal(y, np.broadcast_to(sh, y.shape)), "scale = -1: out must equal shift"


def test_ln_mod_refusals():
    """Descriptors the launcher turns down before any launch: D = 4104 (> 4096), D = 12 (not whole 16-byte chunks), rows that overlap (ld < D with
    more than one row), and -- through a one-entry plan, which reaches the launcher without utx_ln_mod's own checks -- null x / shift / scale."""
    x = torch.zeros(4, 4104, dtype=BF)
    v = torch.zeros(4104, dtype=BF)
    for D in (4104, 12):
        rc, y, _, _ = _k_ln_mod(x, v, v, _sent_bf(4, 4104), 4, D, 4104, 4104)
        assert rc == -2 and (_bits(y) == SENT16).all(), D
    for ldx, ldy in ((504, 512), (512, 504)):
        rc, y, _, _ = _k_ln_mod(x, v, v, _sent_bf(4, 4104), 4, 512, ldx, ldy)
        assert rc == -2 and (_bits(y) == SENT16).all()
    for null in ("x", "shift", "scale"):
        rc, y, _, _ = _k_ln_mod(x, v, v, _sent_bf(4, 4104), 4, 512, 4104, 4104, via_plan=True, null=(null,))
        assert rc == -2 and (_bits(y) == SENT16).all(), null


# ------------------------------------------------------------------------------------------------ ln_mod, MX form; quant_mx8
def _rowmajor(qs, rows, K):
    from unitex_amd.flux.mx8 import PackedScales
    return PackedScales(qs, rows, K).rowmajor().numpy()


@pytest.mark.parametrize("D", [128, 3072])
@pytest.mark.parametrize("n_tok", [1, 130, 257])
def test_ln_mod_mx_equals_ln_mod_then_quant_packed(D, n_tok):
    """utx_ln_mod_desc.q: the fp8 bytes and the tile-packed scale dwords are EQUAL to utx_ln_mod followed by utx_quant_mx8_packed (the contract in
    unitex_hip.h), with qs_row_blocks = ceil(n_tok / 128) and one more; both are also what oracle/mx8_ref.quantize makes of the bf16 result.
    Scale words of rows >= n_tok inside the last 128-row block are UNTOUCHED by both producers (the sentinel survives).  The consumer
    (gemm_w4.hip) does fetch them -- a lane loads the 16 bytes of its four fragment rows, whole 512-byte slabs per wave -- but they scale only
    accumulator rows >= M, whose stores are masked; an MFMA row never mixes with another, so their value cannot reach the output."""
    g = torch.Generator().manual_seed(300 + D + n_tok)
    x = _randbf(g, n_tok, D, scale=2.0, shift=0.3)
    x[0, : min(D, 160)] = x[0, 0]                                  # a stretch of equal values inside a row
    shift, scale = _randbf(g, D), _randbf(g, D, scale=0.5)
    ldq = D + 16
    need = (n_tok + 127) // 128
    rc, y, _, _ = _k_ln_mod(x, shift, scale, _sent_bf(n_tok, D), n_tok, D, D, D)
    assert rc == 0
    q_ref, s_ref = mx8_ref.quantize(y)
    for rb in (need, need + 1):
        rc, q2, qs2 = _k_quant(y, D, _sent_u8(n_tok + 1, ldq), ldq, _sent_u8(D // 128, rb, 512), rb, n_tok, D, True)
        assert rc == 0
        rc, ynone, q1, qs1 = _k_ln_mod(x, shift, scale, None, n_tok, D, D, 0, q=_sent_u8(n_tok + 1, ldq), ldq=ldq, qs=_sent_u8(D // 128, rb, 512), rb=rb)
        assert rc == 0 and ynone is None
        assert torch.equal(q1, q2), "fp8 bytes differ from ln_mod -> quant_mx8_packed (rb=%d)" % rb
        assert torch.equal(qs1, qs2), "scale dwords differ from ln_mod -> quant_mx8_packed (rb=%d)" % rb
        written = np.zeros((n_tok + 1, ldq), dtype=bool)
        written[:n_tok, :D] = True
        _assert_sentinel(q1, written, "ln_mod MX q")
        assert torch.equal(q1[:n_tok, :D], q_ref), "fp8 bytes differ from mx8_ref.quantize of the bf16 result"
        rm = _rowmajor(qs1, rb * 128, D)
        assert np.array_equal(rm[:n_tok], s_ref.numpy()), "scales differ from mx8_ref.quantize of the bf16 result"
        assert (rm[n_tok:] == SENT8).all(), "scale words of rows >= n_tok must stay untouched"


def _mx8_special_blocks(g):
    """eight blocks of 32 that test_mx8_quantiser_bit_exact lacks or only grazes"""
    r = lambda s: torch.randn(32, generator=g) * s
    b = []
    b.append(torch.zeros(32))                                                        # all zeros: scale byte 0
    t = r(0.5).clamp(-3, 3); t[5] = 4.0; b.append(t)                                 # amax exactly a power of two
    t = r(0.5).clamp(-3, 3); t[31] = -(4.0 - 2.0 ** -6); b.append(t)                 # amax the bf16 just below a power of two
    t = torch.zeros(32)                                                              # amax 448 (e = 0): +-448 and e4m3 tie points in three binades + subnormals
    t[:16] = torch.tensor([448.0, -448.0, 272.0, 304.0, 336.0, -432.0, 1.0625, 1.1875, -1.3125, 2.0 ** -10, 3 * 2.0 ** -10, -5 * 2.0 ** -10,
                           2.0 ** -11, 17 * 2.0 ** -4, -0.0, 2.0 ** -6 + 2.0 ** -10])
    b.append(t)
    t = r(20.0); t[0] = 480.0; t[1] = -496.0; t[2] = 464.0; b.append(t)               # 1.875 2^8 and neighbours: scaled past 448, clamped (464 is the tie 448 / 480)
    t = torch.zeros(32); t[0] = 2.0 ** -133; t[1] = -3 * 2.0 ** -133; t[2] = 2.0 ** -127; t[3] = 127 * 2.0 ** -133; b.append(t)      # bf16 subnormals only
    t = r(1.0e30); t[7] = 3.3895313892515355e38; t[8] = -3.3895313892515355e38; b.append(t)                                           # the largest finite bf16
    b.append(r(1.0))
    blocks = torch.stack(b).to(BF)
    assert blocks[5].float().abs().max() < 2.0 ** -126 and float(blocks[6, 7]) == 3.3895313892515355e38
    return blocks


@pytest.mark.parametrize("packed,M,K", [(False, 129, 160), (True, 1, 256), (True, 129, 256)])
def test_quant_mx8_special_blocks(packed, M, K):
    """Bit-exact against oracle/mx8_ref.quantize on blocks test_mx8_quantiser_bit_exact does not hold: amax exactly on / just below a power of two,
    elements that scale to +-448, past it and onto e4m3 tie points (normal and subnormal), bf16 subnormals, the largest finite bf16, signed zero.
    Row-major with K = 160 (five blocks: no multiple of a K-tile), lds and ldq larger than needed; packed with M = 1 and 129 (a row-block tail),
    row_blocks as needed and one more.  Sentinels: q padding and rows behind M, scale padding, packed scale words of rows >= M."""
    g = torch.Generator().manual_seed(400 + M + K)
    nb = K // 32
    x = (torch.randn(M, K, generator=g) * torch.exp(4 * torch.randn(M, 1, generator=g))).to(BF)
    sp = _mx8_special_blocks(g)
    flat = x.view(M * nb, 32)
    for i in range(min(M * nb, 8)):
        flat[i] = sp[i]
    if M > 1:
        for i in range(8):
            flat[M * nb - 1 - i] = sp[i]                       # and again in the last rows (the row-block tail)
    ldx, ldq = K + 8, K + 16
    xbuf = torch.full((M, ldx), 3.0e38, dtype=BF); xbuf[:, :K] = x
    q_ref, s_ref = mx8_ref.quantize(x)
    written_q = np.zeros((M + 1, ldq), dtype=bool); written_q[:M, :K] = True
    if not packed:
        lds = nb + 3
        rc, q, s = _k_quant(xbuf, ldx, _sent_u8(M + 1, ldq), ldq, _sent_u8(M + 1, lds), lds, M, K, False)
        assert rc == 0
        written_s = np.zeros((M + 1, lds), dtype=bool); written_s[:M, :nb] = True
        _assert_sentinel(s, written_s, "quant_mx8 scales")
        assert torch.equal(s[:M, :nb], s_ref), "E8M0 scales"
    else:
        need = (M + 127) // 128
        for rb in (need, need + 1):
            rc, q, s = _k_quant(xbuf, ldx, _sent_u8(M + 1, ldq), ldq, _sent_u8(K // 128, rb, 512), rb, M, K, True)
            assert rc == 0
            rm = _rowmajor(s, rb * 128, K)
            assert np.array_equal(rm[:M], s_ref.numpy()), "E8M0 scales (packed, rb=%d)" % rb
            assert (rm[M:] == SENT8).all(), "packed scale words of rows >= M must stay untouched"
    _assert_sentinel(q, written_q, "quant_mx8 q")
    assert torch.equal(q[:M, :K], q_ref), "e4m3 bytes"


# ------------------------------------------------------------------------------------------------ qkv_post
def _qk_bound(w, cos, sin, qs, parts):
    """|kernel - reference| for one element of Q or K, counted.  Sum of squares in float32: the squares are exact (8 x 8 bits), 8 adds in a lane + 4
    shuffle levels, / 128 exact, + eps, square root, reciprocal, then x rstd: the relative error of x rstd in front of its rounding is below
    (12 / 2 + 1 / 2 + 2 + 2.5 + 1) u = 12 u; 17 u is taken.
        e_n = 17 u |t| + ulp(...)                                   n = bf16(x rstd)
        e_a = e_n |w| + ulp(|n w| + e_n |w|)                        a = bf16(n w), n w exact in float32
        e_r = (e_a0 |c| + e_a1 |s| + 4 u (|a0 c| + |a1 s|)) |qs|    the rotation: two products, a sum, the q_scale product in float32
        e   = e_r + ulp(|r| + e_r)                                  the one bf16 rounding of the result"""
    _, t, r = parts
    dt = 17 * U * np.abs(t)
    e_n = dt + _ulp(np.abs(t) + dt)
    nw = R64.bf16(t) * w
    e_a = e_n * np.abs(w) + _ulp(np.abs(nw) + e_n * np.abs(w))
    a = np.abs(R64.bf16(nw))
    c, s = np.abs(cos), np.abs(sin)
    d0 = e_a[..., 0::2] * c + e_a[..., 1::2] * s + 4 * U * (a[..., 0::2] * c + a[..., 1::2] * s)
    d1 = e_a[..., 1::2] * c + e_a[..., 0::2] * s + 4 * U * (a[..., 1::2] * c + a[..., 0::2] * s)
    e_r = np.stack([d0, d1], -1).reshape(t.shape) * abs(float(np.float32(qs)))
    return e_r + _ulp(np.abs(r) + e_r)


def _rope(S):
    ids = torch.stack([torch.zeros(S), (torch.arange(S) // 7).float(), (torch.arange(S) % 7).float()], 1)
    return dit_ref.rope_tables(ids)


def _qkv_case(x, n_tok, tok_off, H, qs, reorder, wq, wk, cos, sin, S_extra=0, skip_qk=0):
    """x [n_tok, 3, H, 128] bf16 (q, k, v).  -> (Q [H, n_tok, 128], K, Vt [H, 128, n_tok]) float64 / bf16 bits after the sentinel checks"""
    W = H * 128
    if reorder:                      # v | pad | q | k | pad: a non-default column order in rows wider than 3 H 128
        cols, ld = (W + 64, 2 * W + 64, 0), 3 * W + 128
    else:
        cols, ld = (0, W, 2 * W), 3 * W
    qkv = torch.full((n_tok, ld), 3.0e38, dtype=BF)
    for i in range(3):
        qkv[:, cols[i]: cols[i] + W] = x[:, i].reshape(n_tok, W)
    S_pad = (tok_off + n_tok + 63) // 64 * 64 + S_extra
    Qb, Kb, Vb = _sent_bf(H + 1, S_pad, 128), _sent_bf(H + 1, S_pad, 128), _sent_bf(H + 1, 128, S_pad)
    rc, Q, K, Vt = _k_qkv_post(qkv, ld, cols, wq, wk, cos, sin, Qb, Kb, Vb, S_pad * 128, 128 * S_pad, S_pad, n_tok, tok_off, H, q_scale=qs, skip_qk=skip_qk)
    what = "qkv_post n_tok=%d tok_off=%d H=%d" % (n_tok, tok_off, H)
    assert rc == 0, what
    wr = np.zeros((H + 1, S_pad, 128), dtype=bool)
    if not skip_qk:
        wr[:H, tok_off: tok_off + n_tok] = True
    _assert_sentinel(Q, wr, what + " Q")
    _assert_sentinel(K, wr, what + " K")
    wv = np.zeros((H + 1, 128, S_pad), dtype=bool)
    wv[:H, :, tok_off: tok_off + n_tok] = True
    _assert_sentinel(Vt, wv, what + " Vt (columns >= S and < tok_off)")
    v_exp = x[:, 2].permute(1, 2, 0)      # [H, 128, n_tok]
    assert np.array_equal(_bits(Vt[:H, :, tok_off: tok_off + n_tok]), _bits(v_exp)), what + ": Vt is a pure copy and must be bit-equal"
    return Q[:H, tok_off: tok_off + n_tok], K[:H, tok_off: tok_off + n_tok], Vt


@pytest.mark.parametrize("tok_off", [0, 8, 72])
@pytest.mark.parametrize("n_tok", [1, 7, 8, 63, 64, 65, 71, 136])
def test_qkv_post_token_tails_and_offsets(n_tok, tok_off):
    """A block is 64 tokens x one head; V^T leaves in chunks of 8 tokens with a scalar tail (n_tok 1, 7, 63, 65, 71: tails of 1, 7, 7, 1, 7; 8, 64, 136:
    none), at token offsets that are multiples of 8 but not of 64.  H = 1 and 3, q_scale 1 and 0.1275, columns in the default order and as
    v | q | k inside wider rows, S_pad as needed and 64 more, skip_qk (Q / K keep the sentinel, V^T as in the plain call).
    V^T bit-equal.  Q / K: every element inside _qk_bound (counted there); share not bit-equal to the float64 reference below the 2 % cap (the
    float32 restatement dit_ref measures 0.0013 % at q_scale 1 and 0.11 % at 0.1275, tests/test_dit_glue_ref_cpu.py) -- asserted where there
    are at least 63 tokens and, for every n_tok, on the elements of all the case's launches pooled (one flipped element of 128 would be 0.8 % of a
    single-token launch).  Measured on an MI355X: at most 0.18 % in a launch of 63 tokens or more, 1.30 % (5 of 384) in one of a single token."""
    g = torch.Generator().manual_seed(500 + 10 * n_tok + tok_off)
    S = tok_off + n_tok
    cos, sin = _rope(S + 128)
    wq, wk = _randbf(g, 128, scale=0.1, shift=1.0), _randbf(g, 128, scale=0.1, shift=1.0)
    c64, s64 = _f64(cos)[tok_off:S], _f64(sin)[tok_off:S]
    flipped = total = 0
    for H in (1, 3):
        x = _randbf(g, n_tok, 3, H, 128)
        xq, xk = _f64(x[:, 0]).transpose(1, 0, 2), _f64(x[:, 1]).transpose(1, 0, 2)       # [H, n_tok, 128]
        pk = R64.qkv_post(xk, _f64(wk), c64, s64, EPS, 1.0, parts=True)
        bk = _qk_bound(_f64(wk), c64, s64, 1.0, pk)
        for qs in (1.0, 0.1275):
            pq = R64.qkv_post(xq, _f64(wq), c64, s64, EPS, qs, parts=True)
            bq = _qk_bound(_f64(wq), c64, s64, qs, pq)
            for reorder in (False, True):
                Q, K, Vt = _qkv_case(x, n_tok, tok_off, H, qs, reorder, wq, wk, cos, sin, S_extra=64 if reorder else 0)
                for name, got, parts, bound in (("Q", _f64(Q), pq, bq), ("K", _f64(K), pk, bk)):
                    err = np.abs(got - parts[0])
                    share = float((got != parts[0]).mean())
                    print("qkv_post n_tok=%d tok_off=%d H=%d q_scale=%g %s: max err / bound %.3f, %.4f %% not bit-equal"
                          % (n_tok, tok_off, H, qs, name, float((err / bound).max()), 100 * share))
                    assert (err <= bound).all(), "%s: %d elements outside the counted bound" % (name, int((err > bound).sum()))
                    flipped, total = flipped + int((got != parts[0]).sum()), total + got.size
                    if n_tok >= 63:
                        assert share < 0.02, "%s: %.3f %% of the elements differ from the float64 reference" % (name, 100 * share)
        _, _, Vt2 = _qkv_case(x, n_tok, tok_off, H, 1.0, False, wq, wk, cos, sin, skip_qk=1)
        _, _, Vt1 = _qkv_case(x, n_tok, tok_off, H, 1.0, False, wq, wk, cos, sin)
        assert np.array_equal(_bits(Vt1), _bits(Vt2)), "skip_qk: Vt must equal the plain call's"
    assert flipped < 0.02 * total, "%.3f %% of the case's Q / K elements differ from the float64 reference" % (100.0 * flipped / total)


def test_qkv_post_zero_head_and_large_magnitude():
    """Judged by the counted bound only (_qk_bound).  Token 0: q of head 0 all zeros -- sum of squares 0, rstd = eps^-1/2, every output 0.  Token 70:
    |x| in [2^59, 2^60] in q and k -- the sum of 128 squares is at most 2^127, inside float32 (the reference's RMSNorm squares in float32 as well, so
    2^60 is the largest magnitude at which a head still norms there); x rstd is O(1) and the outputs are ordinary numbers."""
    n_tok, tok_off, H = 71, 8, 3
    g = torch.Generator().manual_seed(77)
    x = _randbf(g, n_tok, 3, H, 128)
    x[0, 0, 0] = 0
    big = (2.0 ** 60) * (0.5 + 0.5 * torch.rand(3, H, 128, generator=g)) * torch.where(torch.rand(3, H, 128, generator=g) < 0.5, -1.0, 1.0)
    x[70] = big.to(BF)
    cos, sin = _rope(tok_off + n_tok)
    wq, wk = _randbf(g, 128, scale=0.1, shift=1.0), _randbf(g, 128, scale=0.1, shift=1.0)
    c64, s64 = _f64(cos)[tok_off:], _f64(sin)[tok_off:]
    Q, K, _ = _qkv_case(x, n_tok, tok_off, H, 0.1275, True, wq, wk, cos, sin)
    for name, got, xi, w, qs in (("Q", _f64(Q), x[:, 0], wq, 0.1275), ("K", _f64(K), x[:, 1], wk, 1.0)):
        parts = R64.qkv_post(_f64(xi).transpose(1, 0, 2), _f64(w), c64, s64, EPS, qs, parts=True)
        err, bound = np.abs(got - parts[0]), _qk_bound(_f64(w), c64, s64, qs, parts)
        assert np.isfinite(got).all(), name + ": the sum of squares overflowed"
        print("qkv_post special tokens %s: max err / bound %.3f; |out| of the 2^60 token up to %.3f" % (name, float((err / bound).max()), float(np.abs(got[:, 70]).max())))
        assert (err <= bound).all(), name
        assert np.abs(got[:, 70]).max() > 0.05
    assert (_f64(Q)[0, 0] == 0).all()


@pytest.mark.parametrize("sub", [0, 1])
def test_qkv_post_grouped_head_layouts(sub):
    """heads_per_group = 2 over H = 4 heads, and sub_heads = 1 under it: head h = 2 gi + hi lives at gi gs + hi hs, with sub_heads = 1 at gi gs + hi gs2
    (hs then multiplies hi % 1 = 0), every stride larger than dense.  Expected buffers are built from the plain call's heads: bit-equal, and the
    sentinel everywhere else."""
    n_tok, tok_off, H = 71, 8, 4
    g = torch.Generator().manual_seed(88 + sub)
    x = _randbf(g, n_tok, 3, H, 128)
    cos, sin = _rope(tok_off + n_tok)
    wq, wk = _randbf(g, 128, scale=0.1, shift=1.0), _randbf(g, 128, scale=0.1, shift=1.0)
    Q, K, Vt = _qkv_case(x, n_tok, tok_off, H, 0.1275, False, wq, wk, cos, sin)
    S_pad = 128 + 8                                        # V^T row stride: >= tok_off + n_tok, a multiple of 8 only
    hs_qk, hs_v = S_pad * 128 + 256, 128 * S_pad + 64
    gs2_qk, gs2_v = hs_qk + 512, hs_v + 128
    gs_qk, gs_v = 2 * gs2_qk + 1024, 2 * gs2_v + 256
    off = lambda h, gs, gs2, hs: (h // 2) * gs + ((h % 2) * gs2 if sub else (h % 2) * hs)
    nq, nv = 2 * gs_qk + 4096, 2 * gs_v + 4096
    qkv = x.reshape(n_tok, 3 * H * 128).contiguous()
    rc, Qg, Kg, Vg = _k_qkv_post(qkv, 3 * H * 128, (0, H * 128, 2 * H * 128), wq, wk, cos, sin, _sent_bf(nq), _sent_bf(nq), _sent_bf(nv), hs_qk, hs_v,
                                 S_pad, n_tok, tok_off, H, q_scale=0.1275, hpg=2, gs_qk=gs_qk, gs_v=gs_v, sub=sub, gs2_qk=gs2_qk, gs2_v=gs2_v)
    assert rc == 0
    eq, ek, ev = _sent_bf(nq), _sent_bf(nq), _sent_bf(nv)
    for h in range(H):
        o = off(h, gs_qk, gs2_qk, hs_qk) + tok_off * 128
        eq[o: o + n_tok * 128] = Q[h].reshape(-1)
        ek[o: o + n_tok * 128] = K[h].reshape(-1)
        o = off(h, gs_v, gs2_v, hs_v)
        for d in range(128):
            ev[o + d * S_pad + tok_off: o + d * S_pad + tok_off + n_tok] = Vt[h, d, tok_off: tok_off + n_tok]
    for name, got, exp in (("Q", Qg, eq), ("K", Kg, ek), ("Vt", Vg, ev)):
        assert np.array_equal(_bits(got), _bits(exp)), "grouped layout (sub_heads=%d): %s differs from the plain call's heads at their grouped places" % (sub, name)


# ------------------------------------------------------------------------------------------------ gemv
def _silu_ambiguous(x):
    """inputs whose silu lies so close to a bf16 rounding boundary that the kernel's float32 silu (relative error below 8 x 2^-23, see
    test_gemv_k_passes) may round to the other neighbour than the float64 one"""
    s = R64.silu(x)
    e = 8 * 2.0 ** -23 * np.abs(s)
    return R64.bf16(s - e) != R64.bf16(s + e)


@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("K", [8, 504, 512, 520, 3072])
def test_gemv_k_passes(K, M):
    """One wave per output; a lane takes 8 consecutive k per pass and a pass covers 512: K = 8 one lane, 504 a partly filled pass, 512 exactly one,
    520 a second pass with one lane, 3072 six (production).  N 1 / 5 / 1001 (ragged last block of four waves), rows of x, W and y as dense and
    padded, bias null and given, silu_in / silu_out each, both, neither.
    Summation depth, from the kernel: a lane adds 8 products per pass sequentially into one float32 (a product of two bf16 is exact in float32, so
    an FMA or a multiply + add is one rounding either way), passes = ceil(K / 512), then 6 shuffle levels: n = 8 passes + 6, gamma = n u / (1 - n u).
        d    = gamma sum|x_k w_k| + u |v|  (the bias add)  [+ silu_in: sum over the _silu_ambiguous inputs of ulp(x'_k) |w_k|]
        |out - v| <= d + ulp(|v| + d) / 2                                       v = the float64 dot product + bias, unrounded
    silu_out: y = bf16(v32) as above, z = silu(y) through v / (1 + __expf(-v)): silu is 1.1-Lipschitz, and the float32 formula is within 8 x 2^-23
    relative -- __expf is listed at 1 ulp in the HIP math API documentation of ROCm (floating-point intrinsics table), its argument is exact, the add
    is half an ulp, the division at most 2.5 (the OpenCL-profile bound the device library keeps without -fhip-fp32-correctly-rounded-divide-sqrt):
    (1 + 0.5 + 2.5) 2^-23 = 4 x 2^-23, doubled for slack; the documentation, not a measurement, is the source --
        |out - silu(v)| <= 1.1 (d + ulp(|v| + d) / 2) + 8 x 2^-23 |silu(v)| + ulp(...) / 2                   (two bf16 half-ulps in all)."""
    g = torch.Generator().manual_seed(600 + K + M)
    N = 1001
    x = _randbf(g, M, K)
    W = _randbf(g, N, K, scale=1.0 / 16)
    bias = _randbf(g, N)
    xp = torch.full((M, K + 8), 3.0e38, dtype=BF); xp[:, :K] = x
    Wp = torch.full((N, K + 64), 3.0e38, dtype=BF); Wp[:, :K] = W
    run = _Gemv(x=x, xp=xp, W=W, Wp=Wp, bias=bias)
    passes = (K + 511) // 512
    n = 8 * passes + 6
    gamma = n * U / (1 - n * U)
    xs, Ws, bs = _f64(x), _f64(W), _f64(bias)
    worst = 0.0
    for si, so, wb in itertools.product((False, True), (False, True), (False, True)):
        _, v, S = R64.gemv(xs, Ws, bs if wb else None, si, False, parts=True)
        d = gamma * S + U * np.abs(v)
        if si:
            xr = R64.bf16(R64.silu(xs))
            d = d + (_silu_ambiguous(xs) * _ulp(xr)) @ np.abs(Ws).T
        bound = d + 0.5 * _ulp(np.abs(v) + d)
        ref = v
        if so:
            ref = R64.silu(v)
            dz = 1.1 * bound + 8 * 2.0 ** -23 * np.abs(ref)
            bound = dz + 0.5 * _ulp(np.abs(ref) + dz)
        for Nn, pad in itertools.product((1, 5, 1001), (False, True)):
            ldy = Nn + 24
            rc, y = run("xp" if pad else "x", K + 8 if pad else K, "Wp" if pad else "W", K + 64 if pad else K, "bias" if wb else None,
                        _sent_bf(M + 1, ldy), ldy, M, Nn, K, si, so)
            what = "gemv M=%d N=%d K=%d silu_in=%d silu_out=%d bias=%d pad=%d" % (M, Nn, K, si, so, wb, pad)
            assert rc == 0, what
            wr = np.zeros((M + 1, ldy), dtype=bool); wr[:M, :Nn] = True
            _assert_sentinel(y, wr, what)
            err = np.abs(_f64(y[:M, :Nn]) - ref[:, :Nn])
            worst = max(worst, float((err / bound[:, :Nn]).max()))
            assert (err <= bound[:, :Nn]).all(), "%s: %d outputs outside the counted bound (worst %.3f of it)" % (what, int((err > bound[:, :Nn]).sum()), float((err / bound[:, :Nn]).max()))
    print("gemv M=%d K=%d: depth %d, worst err / bound %.3f" % (M, K, n, worst))


def test_gemv_refusals():
    """Refused before any launch: M = 9 and M = 0; with more than one row, rows of x or y that overlap (ldx < K, ldy < N); with more than one output,
    ldw < K; and -- through a one-entry plan, which reaches the launcher without utx_gemv_bf16's own checks -- null x / W / y."""
    z = torch.zeros(16, 512, dtype=BF)
    run = _Gemv(x=z, W=z)
    for kw in (dict(M=9), dict(M=0), dict(M=2, ldx=504), dict(M=2, ldy=8), dict(M=2, ldw=504)):
        a = dict(M=1, ldx=512, ldw=512, ldy=16)
        a.update(kw)
        rc, y = run("x", a["ldx"], "W", a["ldw"], None, _sent_bf(16, 16), a["ldy"], a["M"], 16, 512, 0, 0)
        assert rc == -2 and (_bits(y) == SENT16).all(), kw
    for null in ("x", "W", "y"):
        rc, y = run("x", 512, "W", 512, None, _sent_bf(16, 16), 16, 2, 16, 512, 0, 0, via_plan=True, null=(null,))
        assert rc == -2 and (_bits(y) == SENT16).all(), null


# ------------------------------------------------------------------------------------------------ sched_step
def _sched_expected(x, v, ds, n_noise, cond):
    """float32 x + dsigma v, the product and the sum rounded separately (no contraction), rounded to bf16; then the re-pin"""
    out = x.clone()
    t = torch.tensor(ds, dtype=torch.float32) * v[:n_noise].float()
    out[:n_noise] = (x[:n_noise].float() + t).to(BF)
    if cond is not None:
        out[n_noise:] = cond[: x.numel() - n_noise]
    return out


def _sched_check(x, v, cond, n_noise, ds, tail=64):
    n_total = x.numel()
    xb = torch.cat([x, _sent_bf(tail)])
    rc, got = _k_sched(xb, v, cond, n_noise, n_total, ds)
    what = "sched_step n_total=%d n_noise=%d cond=%s dsigma=%g" % (n_total, n_noise, cond is not None, ds)
    assert rc == 0, what
    assert (_bits(got[n_total:]) == SENT16).all(), what + ": wrote behind n_total"
    exp = _sched_expected(x, v, ds, n_noise, cond)
    assert np.array_equal(_bits(got[:n_total]), _bits(exp)), what + ": %d elements differ from the float32 evaluation" % int((_bits(got[:n_total]) != _bits(exp)).sum())
    # the float32 evaluation itself against float64: half a bf16 ulp + 2^-23 relative (a double-rounding tie, not a disagreement)
    e = R64.sched_step(_f64(x), _f64(v), ds, n_noise, exact=True)
    dv = np.abs(R64.f32(ds) * _f64(v)[:n_noise])
    assert (np.abs(_f64(exp[:n_noise]) - e) <= 0.5 * _ulp(e) + 2.0 ** -23 * np.maximum(np.abs(e), dv)).all(), what


@pytest.mark.parametrize("ds", [-0.0371, 0.0, 1.0])
def test_sched_step_small(ds):
    """96 x 64 elements, n_noise 0 / 8 / all, cond given and null (the tail must then be left as it was), dsigma -0.0371 / 0 / 1.
    Bit-exact against the float32 evaluation x + dsigma v without contraction (one multiply, one add, one bf16 rounding: there is nothing to
    count), which itself lies within half a bf16 ulp + 2^-23 relative of the float64 value e: the two float32 roundings are u |dsigma v| + u |e|
    <= 2^-23 max(|e|, |dsigma v|) -- relative to e itself wherever x and dsigma v do not cancel, and relative to the product where they do (there the
    product's rounding alone can exceed any multiple of |e|)."""
    g = torch.Generator().manual_seed(700)
    n = 96 * 64
    x, v, cond = _randbf(g, n), _randbf(g, n), _randbf(g, n)
    for n_noise, c in itertools.product((0, 8, n), (cond, None)):
        _sched_check(x, v, c, n_noise, ds)


def test_sched_step_grid_stride_second_trip():
    """The grid is capped at 2048 blocks of 256 threads, one 8-element chunk per thread and trip: 2048 x 256 x 8 + 8 x 1000 elements (8.4 MB) make
    the loop take a second trip -- once all noise with cond null, once with the noise / condition boundary inside the second trip.  Same bit-exact
    rule as test_sched_step_small."""
    g = torch.Generator().manual_seed(701)
    first = 2048 * 256 * 8
    n = first + 8 * 1000
    x, v = _randbf(g, n), _randbf(g, n)
    cond = _randbf(g, 8 * 1000)
    _sched_check(x, v, None, n, -0.0371)
    _sched_check(x, v, cond, first + 8 * 400, -0.0371)


def test_sched_step_refusals():
    """n_noise_elems outside 0 .. n_total_elems would index cond (or x and v) outside the operand: refused before any launch, as are sizes that are no
    whole 16-byte chunks."""
    x = torch.zeros(1024, dtype=BF)
    for n_noise, n_total in ((-8, 1024), (1032, 1024), (1 << 40, 1024), (4, 1024), (0, 1020), (0, 0)):
        rc, got = _k_sched(_sent_bf(1024), x, x, n_noise, n_total, 1.0)
        assert rc == -2 and (_bits(got) == SENT16).all(), (n_noise, n_total)


# ------------------------------------------------------------------------------------------------ add3
@pytest.mark.parametrize("n", [1, 255, 256, 257, 3072])
def test_add3(n):
    """bf16(bf16(a + b) + c), b null: bf16(a + c); one thread per element, 256 per block: n = 1, one short of / exactly / one past a block, production.
    Bit-exact against the float64 reference (each sum of two bf16 of comparable size is exact in float32: one rounding per stage on both sides).
    The kernel is reached through a one-entry plan (utx_plan_add_add3), as the product reaches it."""
    g = torch.Generator().manual_seed(800 + n)
    a, b, c = _randbf(g, n), _randbf(g, n), _randbf(g, n)
    for bb in (b, None):
        rc, out = _k_add3(a, bb, c, _sent_bf(n + 64), n)
        assert rc == 0
        assert (_bits(out[n:]) == SENT16).all(), "add3 wrote behind n"
        ref = R64.add3(_f64(a), None if bb is None else _f64(bb), _f64(c))
        assert np.array_equal(_f64(out[:n]), ref), "add3 n=%d b=%s: %d elements differ" % (n, bb is not None, int((_f64(out[:n]) != ref).sum()))

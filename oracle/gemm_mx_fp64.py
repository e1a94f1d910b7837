"""float64 reference (TEST INFRASTRUCTURE ONLY) of the two MX fp8 GEMM kernels -- utx_gemm_desc.mx8 = 1 (gemm_bf16_kernel<128,128,2,2,false,true>, row-major scales) and
mx8 = 2 (gemm256_w4_kernel<GATED, false, true>, tile-packed scales, optional fp8 output q_out) -- with the input sets of tests/test_gemm_mx_edges_gpu.py and a float32
emulation that can be told to make one mistake (tests/test_gemm_mx_ref_cpu.py).

The GEMM contract is not restated: operands are quantised by oracle/mx8_ref.quantize (the one definition of the format), dequantised in float64 -- e4m3 x 2^(byte - 127)
is exact there -- and handed to oracle/gemm_fp64.gemm; the bf16 LoRA segment, alpha, bias, GELU, gate / res and n_split go through unchanged.

The interval is that module's, e = (K + K2 + 4) 2^-23 (|alpha| sum|a b| + |bias|) with K the fp8 element count.  It bounds any order of float32 partial sums at a unit
doubled for truncated internal sums, and it needs NO new term for MX: every product of two e4m3 values is exact in float32 and the block scales are powers of two, so only
the summation and the epilogue's bf16 roundings can differ.  No GPU number went into it.

fp8 output (q_out).  The GELU columns leave as e4m3 bytes + one E8M0 byte per 32 columns, defined as quantize(bf16 GELU output).  qout_accept builds the acceptance rule
from the bf16 interval [lo, hi] of those columns: the scale byte is monotone in the block's amax and, under a fixed scale, the e4m3 value is monotone in the element, so
  scale byte   between the bytes mx8_ref gives for amax = max(min |.| over [lo, hi]) and amax = max(max(|lo|, |hi|)) of the block (one byte almost everywhere);
  element      decoded under the byte the kernel chose, between the quantisations of lo and hi under that byte.
Where every element of a block has lo == hi this is equality with quantize(ref.out).

Operands (make_inputs).  Every scale byte must matter and the products of one output element must keep one sign (oracle/gemm_fp64.py says why).  With u[kb] an integer per
32-block in [-span, span] and r[m], c[n] integers in [-3, 3]:
    A = |N(0, 1/2)| 2^(u[kb] + r[m]),   B = sign[n] |N(0, 1)| 3 / K 2^(-u[kb] + c[n]),   bias = sign[n] |N(0, 1)| 2^c[n],
rounded to bf16, then quantised.  u cancels in every product, so every 32-block contributes a like share of sum|a b| (tests/test_gemm_mx_ref_cpu.py asserts at least
1 / (8 K / 32) for every output element and at least four distinct scale bytes per row) while the bytes of neighbouring blocks, rows and K-tiles differ: a scale read from the
wrong block, row, K-tile or row block is off by a power of two on a full share of the sum.  span 6 by default, 40 and 100 in one case each (A blocks near 2^+-100, B blocks at
the opposite end: normal products from E8M0 bytes near both ends of their range); one case zeroes a block of A and one of B in some rows (those blocks are exempt from the
share assertion, and from nothing else), one makes a block's amax an exact power of two.  One restriction: a GELU column of negative sign draws c[n] from [-3, -1], which
keeps its y above -8.  Below about -9.9 the float32 expression x / (1 + exp(-2u)) leaves float32's range (exp overflows, the result is -0) while the float64 GELU is still a
nonzero bf16 value: that is the range of the number format, not an error of a kernel, and the relative interval of gemm_fp64 rightly has no room for it.  LoRA operands are the zero-mean ones of gemm_fp64.make_inputs.
"""
import zlib

import numpy as np
import torch

from oracle import gemm_fp64 as G
from oracle import mx8_ref
from oracle.dit_glue_fp64 import F64, bf16

Q_SENT, S_SENT, A_POISON = 0x7F, 0xFF, 0x7F      # e4m3 NaN / E8M0 NaN: bytes no quantiser produces (|q| <= 448 = 0x7E, scale byte <= 254)
_E4M3 = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(torch.float64).numpy()


# ------------------------------------------------------------------------------------------------ the format: wrappers, never a second definition
def _t32(x):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x, dtype=np.float32)))


def quantize(x):
    """[R, K] of bf16 values (any float dtype) -> (q uint8 [R, K], s uint8 [R, K/32]) by mx8_ref.quantize"""
    q, s = mx8_ref.quantize(_t32(x))
    return q.numpy().copy(), s.numpy().copy()


def scale_byte(amax):
    """the E8M0 byte mx8_ref gives a block whose largest magnitude is amax (array of float32-representable values)"""
    return (mx8_ref.scale_exponent(_t32(amax)) + 127).numpy().astype(np.uint8)


def elements_under(x, byte):
    """decoded e4m3 value (float64, without the scale) of x [..., n] quantised under the scale bytes byte [...]"""
    e = torch.from_numpy(np.ascontiguousarray(np.asarray(byte, dtype=np.int32))) - 127
    return _E4M3[mx8_ref.elements(_t32(x), e).numpy()]


def dequantize(q, s):
    """(q uint8 [R, K], s uint8 [R, K/32]) -> float64 [R, K], exact"""
    q, s = np.asarray(q), np.asarray(s)
    R, K = q.shape
    v = _E4M3[q].reshape(R, K // 32, 32) * np.exp2(s.astype(F64) - 127.0)[..., None]
    return v.reshape(R, K)


def pack_scales(s, row_blocks=None, slabs=None, fill=S_SENT):
    """row-major scale bytes s [R, K/32] -> uint8 [slabs >= K/128][row_blocks >= ceil(R / 128)][512]: dword [kt][rb][l][im] holds, in byte j, the scale of block 4 kt + j
    of row 128 rb + 32 im + l (include/unitex_hip.h, utx_quant_mx8_packed).  Everything that is not a scale of s -- rows >= R of the last row block included -- holds `fill`."""
    s = np.asarray(s, dtype=np.uint8)
    R, KB = s.shape
    assert KB % 4 == 0
    nb = (R + 127) // 128
    row_blocks, slabs = (nb if row_blocks is None else row_blocks), (KB // 4 if slabs is None else slabs)
    assert row_blocks >= nb and slabs >= KB // 4
    full = np.full((nb * 128, KB), fill, dtype=np.uint8)
    full[:R] = s
    out = np.full((slabs, row_blocks, 512), fill, dtype=np.uint8)
    d = full.reshape(nb, 4, 32, KB // 4, 4)                        # rb, im, l, kt, j
    out[: KB // 4, :nb] = d.transpose(3, 0, 2, 1, 4).reshape(KB // 4, nb, 512)
    return out


def unpack_scales(data, rows, K, kt0=0):
    """the inverse: packed uint8 [slabs][row_blocks][512] -> row-major [rows, K/32] of K-tiles kt0 .. kt0 + K/128 - 1"""
    data = np.asarray(data, dtype=np.uint8)
    nb, nkt = (rows + 127) // 128, K // 128
    d = data[kt0: kt0 + nkt, :nb].reshape(nkt, nb, 32, 4, 4)        # kt, rb, l, im, j
    return np.ascontiguousarray(d.transpose(1, 3, 2, 0, 4).reshape(nb * 128, K // 32)[:rows])


# ------------------------------------------------------------------------------------------------ acceptance of the fp8 output
def qout_accept(q_bytes, scale_bytes, ref):
    """q_bytes uint8 [M, W], scale_bytes uint8 [M, W/32], ref: Ref of the W GELU columns -> (bool [M, W/32] scale byte accepted, bool [M, W] element accepted)"""
    q_bytes, scale_bytes = np.asarray(q_bytes, dtype=np.uint8), np.asarray(scale_bytes, dtype=np.uint8)
    M, W = q_bytes.shape
    lo, hi = ref.lo.reshape(M, W // 32, 32), ref.hi.reshape(M, W // 32, 32)
    straddle = (lo <= 0) & (hi >= 0)
    amin = np.where(straddle, 0.0, np.minimum(np.abs(lo), np.abs(hi))).max(-1)
    amax = np.maximum(np.abs(lo), np.abs(hi)).max(-1)
    ok_s = (scale_bytes >= scale_byte(amin)) & (scale_bytes <= scale_byte(amax))
    got = _E4M3[q_bytes].reshape(M, W // 32, 32)
    with np.errstate(invalid="ignore"):
        ok_q = (got >= elements_under(lo, scale_bytes)) & (got <= elements_under(hi, scale_bytes))
    return ok_s, ok_q.reshape(M, W)


def qout_check(q_buf, s_buf, M, W, kt0, ref, what):
    """q_buf uint8 [R >= M, >= W] and s_buf uint8 [R, 4 x slabs] (the packed scale buffer unpacked over ALL its slabs and row blocks) as a q_out launch left them, both
    preset with Q_SENT / S_SENT: sentinels intact outside rows < M x (columns < W | K-tiles kt0 .. kt0 + W/128 - 1), the rest accepted by qout_accept.  -> message or None"""
    q_buf, s_buf = np.asarray(q_buf), np.asarray(s_buf)
    inq = np.zeros(q_buf.shape, dtype=bool); inq[:M, :W] = True
    ins = np.zeros(s_buf.shape, dtype=bool); ins[:M, 4 * kt0: 4 * kt0 + W // 32] = True
    for name, buf, inside, sent in (("q_out", q_buf, inq, Q_SENT), ("qs_out (unpacked)", s_buf, ins, S_SENT)):
        wrong = np.argwhere(~inside & (buf != sent))
        if wrong.size:
            return "%s: %s written outside its region at %d places, first (row, column) = %s of %s" % (what, name, len(wrong), tuple(wrong[0]), buf.shape)
        left = np.argwhere(inside & (buf == sent))
        if left.size:
            return "%s: %d bytes of %s never written, first (row, column) = %s" % (what, len(left), name, tuple(left[0]))
    ok_s, ok_q = qout_accept(q_buf[:M, :W], s_buf[:M, 4 * kt0: 4 * kt0 + W // 32], ref)
    if not ok_s.all():
        m, b = (int(v) for v in np.argwhere(~ok_s)[0])
        return "%s: %d of %d scale bytes outside their range, first row %d block %d (256-tile row %d + %d): got %d" % (
            what, int((~ok_s).sum()), ok_s.size, m, b, m // 256, m % 256, int(s_buf[m, 4 * kt0 + b]))
    if not ok_q.all():
        m, n = (int(v) for v in np.argwhere(~ok_q)[0])
        return "%s: %d of %d fp8 elements outside their interval, first (m, n) = (%d, %d) [256-tile (%d, %d) + (%d, %d)]: byte 0x%02x under scale %d, bf16 interval [%r, %r]" % (
            what, int((~ok_q).sum()), ok_q.size, m, n, m // 256, n // 256, m % 256, n % 256, int(q_buf[m, n]), int(s_buf[m, 4 * kt0 + n // 32]),
            float(ref.lo[m, n]), float(ref.hi[m, n]))
    return None


def gelu_part(ref, gelu_from):
    return G.Ref(*(np.ascontiguousarray(x[:, gelu_from:]) for x in ref))


# ------------------------------------------------------------------------------------------------ the cases of tests/test_gemm_mx_edges_gpu.py
def _case(name, mx8, M, N, K, span=6, special=None, pad_sa=0, pad_sb=0, b_slice=None, **kw):
    """a gemm_fp64 case plus: mx8 (1 row-major / 2 packed scales), span of the block exponents, special (None / "zero_block" / "pow2_block"), pad_sa / pad_sb (scale bytes a
    row-major scale row is wider than K/32), b_slice = (r0, r1, rows): B is rows r0..r1 of a `rows`-row weight whose packed scales are sliced (PackedScales.row_slice)"""
    c = G._case(name, "mx%d" % mx8, M, N, K, **kw)
    c.update(mx8=mx8, span=span, special=special, pad_sa=pad_sa, pad_sb=pad_sb, b_slice=b_slice)
    return c


# mx8 = 1, the 128 x 128 kernel: the shapes of gemm_fp64.CASES_128 with K in fp8 elements (128 one K-tile, 256 / 384 the ring at both parities)
CASES_MX1 = [
    _case("mx1_m1_n8", 1, 1, 8, 128, pad_c=16),
    _case("mx1_m7_gelu0", 1, 7, 136, 256, gelu_from=0),
    _case("mx1_m127_gelu132_lda_lds", 1, 127, 264, 384, gelu_from=132, pad_a=64, pad_sa=4, pad_sb=8),
    _case("mx1_m128_lora_alpha_nobias", 1, 128, 128, 128, K2=64, lora_seg_n=128, lora_n_limit=128, alpha=0.37, bias=False),
    _case("mx1_m129_lora3seg", 1, 129, 384, 256, K2=128, lora_seg_n=128, lora_n_limit=256, nseg=3, pad_c=8),
    _case("mx1_m200_loraseg_split_gelu128", 1, 200, 384, 384, K2=64, lora_seg_n=128, lora_n_limit=128, nseg=3, gelu_from=128, n_split=128, pad_c=24, pad_c1=40),
    _case("mx1_m600_gated_inplace", 1, 600, 264, 128, gate="inplace", pad_c=8),
    _case("mx1_m200_gated_separate", 1, 200, 136, 256, gate="separate", pad_c=16, pad_res=40),
    _case("mx1_m200_span100", 1, 200, 264, 256, span=100),
    _case("mx1_m129_zero_blocks", 1, 129, 136, 384, special="zero_block"),
]
# mx8 = 2, the one-wave-per-SIMD kernel: M = 64 leaves two waves without a valid row, 300 / 600 a ragged last tile row; K 128 one K-tile, then even and odd counts
CASES_MX2 = [
    _case("mx2_m1", 2, 1, 256, 128, pad_c=8),
    _case("mx2_m64_alpha_nobias", 2, 64, 512, 256, alpha=0.37, bias=False),
    _case("mx2_m129", 2, 129, 768, 384),
    _case("mx2_m256_gelu_split", 2, 256, 512, 640, gelu_from=256, n_split=256, pad_c=8, pad_c1=24),
    _case("mx2_m257_pow2", 2, 257, 768, 256, special="pow2_block", pad_a=64),
    _case("mx2_m300_gated", 2, 300, 256, 384, gate="inplace", pad_c=16),
    _case("mx2_m600_grid1", 2, 600, 512, 256, pers_grid=1),
    _case("mx2_m600_gelu_split_grid2", 2, 600, 512, 384, gelu_from=256, n_split=256, pers_grid=2),
    _case("mx2_m600_gated_grid3", 2, 600, 512, 640, gate="inplace", pers_grid=3),
    _case("mx2_m200_span40_bslice", 2, 200, 512, 256, span=40, b_slice=(256, 768, 1024)),
    _case("mx2_m200_span100", 2, 200, 256, 256, span=100),
    _case("mx2_m129_zero_blocks", 2, 129, 256, 384, special="zero_block"),
]
# split tail: six tiles on a grid of four -> T = 2 tail tiles cut into S ranges of whole 128-element K-tiles (the launcher sees K / 128 range units for MX)
CASES_MXSPLIT = [
    _case("mxsk_s%d_k%d_%s" % (S, K, "gated" if gated else "plain"), 2, 600, 512, K, gate="inplace" if gated else None, pers_grid=4, streamk=S)
    for S in (2, 3) for K in (384, 640) for gated in (False, True)
]
# both kernels on the same operands: the same bits
CASE_BOTH = _case("mx12_m300_gelu_split", 2, 300, 512, 384, gelu_from=256, n_split=256)
# fp8 output of the GELU columns (mx8 = 2): gelu_from = n_split = 256 of N = 512, K = 256; the launches vary q_out_kt0 and the persistent grid
CASES_QOUT = [_case("mxq_m%d" % M, 2, M, 512, 256, gelu_from=256, n_split=256) for M in (300, 129, 600)]
CASES = CASES_MX1 + CASES_MX2 + CASES_MXSPLIT + [CASE_BOTH] + CASES_QOUT


def _block_exponents(rng, KB, span):
    """u[kb]: the first blocks on a grid of step 3 without repetition (their scale bytes cannot coincide whatever binade a block's amax falls in), the rest anywhere"""
    if span >= 100:          # both ends of the E8M0 range and nothing between: u within 9 of -span or of +span
        grid = np.concatenate([-span + 3 * np.arange(4), span - 3 * np.arange(4)])
        return np.concatenate([rng.permutation(grid), rng.choice(grid, max(KB - 8, 0))])[:KB].astype(F64)
    grid = np.arange(-span, span + 1, 3)
    n0 = min(KB, len(grid))
    return np.concatenate([rng.permutation(grid)[:n0], rng.integers(-span, span + 1, KB - n0)]).astype(F64)


def make_inputs(case, seed=20262):
    """the operands of one case from a fixed seed and the case's name: Aq / As / Bq / Bs (uint8: e4m3 bytes, row-major E8M0 bytes), A / B (float64, dequantised -- what the
    reference multiplies), bias / A2 / B2 / gate / res (float64 arrays of bf16 values or None), zero_a / zero_b (bool [rows, K/32]: blocks zeroed on purpose)"""
    rng = np.random.default_rng([seed, zlib.crc32(case["name"].encode())])
    M, N, K, K2 = case["M"], case["N"], case["K"], case["K2"]
    KB = K // 32
    u = np.repeat(_block_exponents(rng, KB, case["span"]), 32)[None, :]
    r, c = rng.integers(-3, 4, (M, 1)).astype(F64), rng.integers(-3, 4, (N, 1)).astype(F64)
    sign = rng.choice([-1.0, 1.0], (N, 1))
    gelu_neg = (np.arange(N)[:, None] >= (N if case["gelu_from"] is None else case["gelu_from"])) & (sign < 0)
    c = np.where(gelu_neg, rng.integers(-3, 0, (N, 1)).astype(F64), c)
    A = bf16(np.abs(rng.normal(0, 0.5, (M, K))) * np.exp2(u + r))
    B = bf16(sign * np.abs(rng.normal(0, 1, (N, K))) * 3.0 / K * np.exp2(-u + c))
    bias = bf16(sign[:, 0] * np.abs(rng.normal(0, 1, N)) * np.exp2(c[:, 0])) if case["bias"] else None
    zero_a, zero_b = np.zeros((M, KB), dtype=bool), np.zeros((N, KB), dtype=bool)
    if case["special"] == "zero_block":
        zero_a[::5, 1] = True
        zero_b[::7, KB - 2] = True
        A[np.repeat(zero_a, 32, 1)] = 0.0
        B[np.repeat(zero_b, 32, 1)] = 0.0
    if case["special"] == "pow2_block":          # block 0 of A and the last block of B: the largest magnitude is exactly a power of two
        A[:, 5] = np.exp2(np.ceil(np.log2(np.abs(A[:, :32]).max(1))))
        B[:, K - 3] = sign[:, 0] * np.exp2(np.ceil(np.log2(np.abs(B[:, K - 32:]).max(1))))
    Aq, As = quantize(A)
    Bq, Bs = quantize(B)
    inp = dict(Aq=Aq, As=As, Bq=Bq, Bs=Bs, A=dequantize(Aq, As), B=dequantize(Bq, Bs), bias=bias, A2=None, B2=None, gate=None, res=None, zero_a=zero_a, zero_b=zero_b)
    if K2:
        inp["A2"] = bf16(rng.normal(0, 0.5, (M, case["nseg"] * K2)) / 8)
        inp["B2"] = bf16(rng.normal(0, 1 / np.sqrt(K2), (N, K2)) / 4)
    if case["gate"]:
        inp["gate"], inp["res"] = bf16(rng.normal(0, 1, N)), bf16(rng.normal(0, 1, (M, N)))
    return inp


def reference(case, inp):
    return G.reference(case, inp)


def block_shares(inp):
    """[K/32, M, N]: the share of sum|a b| each 32-block carries for every output element"""
    A, B = np.abs(inp["A"]), np.abs(inp["B"])
    KB = A.shape[1] // 32
    S = np.stack([A[:, 32 * b: 32 * b + 32] @ B[:, 32 * b: 32 * b + 32].T for b in range(KB)])
    return S / S.sum(0)


# ------------------------------------------------------------------------------------------------ float32 emulation of the kernels, with defects
DEFECTS = ("drop_last_k_tile", "a_scale_next_block", "b_scale_stuck_at_kt0", "a_scale_row_block0", "packed_l_im_swapped", "a_scale_for_b", "lora_skipped",
           "qout_from_unrounded_y", "qout_kt0_ignored", "qout_amax_over_8", "qout_rows_ge_M_written")
QOUT_SLABS = 3


def emulate(case, inp, defect=None, q_out_kt0=None):
    """what the kernels compute, in numpy float32: per K-tile of 128 fp8 elements and per 32-block the dot product of the e4m3 values (exact products) times
    2^(a byte + b byte - 254), accumulated in float32; then the bf16 LoRA segment and the epilogue of gemm_fp64.emulate.  q_out_kt0 given (a CASES_QOUT case): the GELU columns
    leave as quantize(bf16(GELU)) instead.  defect: one of DEFECTS.
    -> dict(out [M, N] float64 (SENT where nothing was written), q uint8 [R, W] / qs uint8 [R, 4 QOUT_SLABS] with R = M rounded up to 128 (None without q_out))"""
    assert defect is None or defect in DEFECTS
    f = np.float32
    Av, Bv = _E4M3[inp["Aq"]].astype(f), _E4M3[inp["Bq"]].astype(f)
    As, Bs = inp["As"].astype(np.int64), inp["Bs"].astype(np.int64)
    (M, K), N = Av.shape, Bv.shape[0]
    KB = K // 32
    kb = np.arange(KB)
    sa, sb = As, Bs
    if defect == "a_scale_next_block":
        sa = As[:, (kb // 4) * 4 + (kb + 1) % 4]
    elif defect == "b_scale_stuck_at_kt0":
        sb = Bs[:, kb % 4]
    elif defect == "a_scale_row_block0":
        sa = As[np.minimum(np.arange(M) % 128, M - 1)]
    elif defect == "packed_l_im_swapped":
        m = np.arange(M)
        l, im = m % 32, (m % 128) // 32
        sa = As[np.minimum((m // 128) * 128 + 4 * l + im, M - 1)]
    elif defect == "a_scale_for_b":
        sb = As[np.arange(N) % M]
    acc = np.zeros((M, N), dtype=f)
    with np.errstate(over="ignore", invalid="ignore"):
        for b in range(KB - (4 if defect == "drop_last_k_tile" else 0)):
            dot = Av[:, 32 * b: 32 * b + 32] @ Bv[:, 32 * b: 32 * b + 32].T
            acc += dot * np.ldexp(f(1), (sa[:, b, None] + sb[None, :, b] - 254).astype(np.int32)).astype(f)
    if defect != "lora_skipped":
        G.emulate_lora(acc, case, inp)
    if q_out_kt0 is None:
        return dict(out=G.emulate_epilogue(acc, case, inp), q=None, qs=None)
    gf, R = case["gelu_from"], (M + 127) // 128 * 128
    assert gf == case["n_split"] and not case["gate"]
    W = N - gf
    out = np.full((M, N), G.SENT, dtype=F64)
    out[:, :gf] = G.emulate_epilogue(acc[:, :gf], dict(case, gelu_from=None), dict(inp, bias=None if inp["bias"] is None else inp["bias"][:gf]))
    b = np.zeros(W, dtype=f) if inp["bias"] is None else inp["bias"][gf:].astype(f)
    g32 = G.gelu_f32(G._rbf32(acc[:, gf:] * f(case["alpha"]) + b))
    src = g32 if defect == "qout_from_unrounded_y" else G._rbf32(g32)
    if defect == "qout_amax_over_8":        # a lane's 8 columns decide their own scale; the block's byte is its first lane's
        t = torch.from_numpy(src).view(M, W // 8, 8)
        e8 = mx8_ref.scale_exponent(t.abs().amax(-1))
        qv = mx8_ref.elements(t, e8).view(M, W).numpy()
        qs = (e8.view(M, W // 32, 4)[:, :, 0] + 127).numpy().astype(np.uint8)
    else:
        qv, qs = quantize(src)
    rows = R if defect == "qout_rows_ge_M_written" else M
    src_rows = np.minimum(np.arange(rows), M - 1)
    kt0 = 0 if defect == "qout_kt0_ignored" else q_out_kt0
    qbuf, sbuf = np.full((R, W), Q_SENT, dtype=np.uint8), np.full((R, 4 * QOUT_SLABS), S_SENT, dtype=np.uint8)
    qbuf[:rows] = qv[src_rows]
    sbuf[:rows, 4 * kt0: 4 * kt0 + W // 32] = qs[src_rows]
    return dict(out=out, q=qbuf, qs=sbuf)

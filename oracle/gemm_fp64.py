"""float64 reference (TEST INFRASTRUCTURE ONLY) of the bf16 GEMM contract in the header of unitex_amd/csrc/gemm.hip, with a COUNTED acceptance
interval per output element, the input sets of tests/test_gemm_edges_gpu.py, and a float32 emulation of the kernels that can be told to make one
mistake (tests/test_gemm_ref_cpu.py runs it through the same acceptance check: correct it must pass, with a defect it must not).

numpy on the CPU.  Arrays hold bf16-representable values; the float64 value is rounded to bf16 (oracle/dit_glue_fp64.bf16: straight from float64,
ties to even) exactly where the header puts a tensor boundary -- y, after GELU, gate * y, the residual sum -- and nowhere else.  alpha is taken at
its float32 value (the descriptor carries a C float).  Nothing here knows how a kernel spreads its work over lanes or tiles.

The interval.  y64 = f32(alpha) (A B^T + A2[:, seg] B2^T) + bias in float64, and
    e = (K + K2 + 4) 2^-23 (|alpha| (|A| |B|^T + |A2| |B2|^T) + |bias|)
bounds what ANY order of float32 partial sums can lose: one unit per product-and-add of the K + K2 terms, four more for alpha, the bias and the
margin of a split K range summed a second time.  The unit 2^-23 is twice round-to-nearest's on purpose: how the matrix unit rounds inside one
instruction is not documented, and with the doubled unit the bound also holds for truncated internal sums.  No GPU number went into it.
    plain      bf16(y64 - e) <= out <= bf16(y64 + e)
    GELU       float64 GELU-tanh of both end candidates of y, widened by the counted error of the kernels' x * rcp(1 + exp(-2u)) (GELU_REL), then bf16
    gated      res + bf16(gate * y) for both end candidates, 2^-23 |sum| for the one float32 add (none where the sum is a float32 number: _add_slack),
               then bf16; out between the smaller and the larger
The end candidates of y are neighbouring bf16 values (e is far below a bf16 ulp at every size used here), so "both ends" is every candidate.

Operand scales (make_inputs).  The share of elements whose interval holds more than one bf16 value is 2 e / ulp(y) on average, i.e. about
2 (K + K2 + 4) 2^-23 * 192 * sum|a b| / |y|: with zero-mean operands (A ~ N(0, 1/2), B ~ N(0, 1 / sqrt(K)), bias ~ N(0, 1)) sum|a b| / |y| grows like
0.64 sqrt(K) and the share, computed with this module on the CPU, is 3.7 % at K = 64, 8.1 % at 128, 12.9 % at 192, 24.6 % at 320, 36 % at 512: too blunt.
The inputs therefore keep the products of one output element of one sign: A >= 0 with a magnitude per row, B = sign[n] * magnitude[n] * |N(0, 1)| * 3 / K,
bias of the column's sign.  y still takes both signs and every magnitude between 0.1 and 5 (the GELU's curved part), rows and columns are distinguishable, and
the share is 1.4 % at most over the cases below (tests/test_gemm_ref_cpu.py prints it per case and holds it under 5 %).
The LoRA operands are zero-mean (A2 ~ N(0, 1/2) / 8, B2 ~ N(0, 1 / sqrt(K2)) / 4): their segment moves y by a few bf16 ulps, which is what makes a skipped or
misplaced segment visible.
"""
import zlib
from collections import namedtuple

import numpy as np

from oracle.dit_glue_fp64 import F64, bf16, f32

U23 = 2.0 ** -23
SENT16 = 0x4B5A                      # bit pattern of a finite bf16 (about 1.4e7) that no input set produces: the fill of preallocated outputs
SENT = float(np.array([SENT16 << 16], dtype=np.uint32).view(np.float32)[0])
K0 = f32(0.7978845608028654)         # the kernels' float constants, at their float32 value
K1 = f32(0.044715)
# v / (1 + __expf(-v)): 8 x 2^-23 relative -- the constant of the SiLU bound in tests/test_dit_glue_edges_gpu.py (test_gemv_k_passes: __expf 1 ulp by the HIP math API
# tables, the add half an ulp, the reciprocal / division at most 2.5, doubled).  GELU differs in two places, both counted from gelu_tanh() in gemm.hip: the
# exponent's argument -2u carries the five float32 roundings of u = k0 (x + k1 x x x), 5 x 2^-24 <= 3 x 2^-23 relative, which exp turns into |2u| times that; and the
# final product x * s is one more rounding (2^-24, counted as one unit).
INTRINSIC_REL = 8 * U23


def gelu_rel(y):
    """relative error bound of the kernels' float32 GELU expression at the bf16 input y"""
    u2 = np.abs(2.0 * K0 * (y + K1 * y * y * y))
    return INTRINSIC_REL + U23 + 3 * u2 * U23


def gelu_tanh(x):
    """0.5 x (1 + tanh u) = x / (1 + exp(-2u)), u = k0 (x + k1 x^3), float64"""
    x = np.asarray(x, dtype=F64)
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-2.0 * K0 * (x + K1 * x * x * x)))


def _add_slack(s):
    """allowance for the one float32 add res + bf16(gate * y): 2^-23 |s|, and nothing where the sum of the two bf16 values is itself a float32 number -- an IEEE add
    returns it exactly, so there is no error to allow for.  (That is nearly everywhere; without it every sum that lands on a bf16 tie -- one in five, two bf16 addends
    leave few bits -- would count as a two-valued interval although round-to-nearest-even decides it.)"""
    with np.errstate(over="ignore"):
        exact = s.astype(np.float32).astype(F64) == s
    return np.where(exact, 0.0, U23 * np.abs(s))


Ref = namedtuple("Ref", "out lo hi")          # each [M, N] float64 holding bf16 values; columns >= n_split belong to C1


def _lora_segments(N, K2, lora_seg_n, lora_n_limit):
    """(column slice, A2 column slice) of every LoRA segment: columns < lora_n_limit, segment s = n // lora_seg_n reads A2[:, s K2 : (s + 1) K2]"""
    seg = N if lora_seg_n is None else lora_seg_n
    lim = N if lora_n_limit is None else min(lora_n_limit, N)
    return [(slice(n0, min(n0 + seg, lim)), slice((n0 // seg) * K2, (n0 // seg + 1) * K2)) for n0 in range(0, lim, seg)]


def gemm(A, B, bias=None, A2=None, B2=None, lora_seg_n=None, lora_n_limit=None, alpha=1.0, gelu_from=None, gate=None, res=None, n_split=None):
    """-> Ref(out, lo, hi): the contract's value and the acceptance interval, [M, N] each.  n_split only says where C1 starts (split_cols)."""
    A, B = np.asarray(A, dtype=F64), np.asarray(B, dtype=F64)
    (M, K), N = A.shape, B.shape[0]
    acc, S = A @ B.T, np.abs(A) @ np.abs(B).T
    K2 = 0
    if A2 is not None:
        A2, B2 = np.asarray(A2, dtype=F64), np.asarray(B2, dtype=F64)
        K2 = B2.shape[1]
        for cols, ks in _lora_segments(N, K2, lora_seg_n, lora_n_limit):
            acc[:, cols] += A2[:, ks] @ B2[cols].T
            S[:, cols] += np.abs(A2[:, ks]) @ np.abs(B2[cols]).T
    assert n_split is None or 0 < n_split <= N
    a = f32(alpha)
    b = np.zeros(N) if bias is None else np.asarray(bias, dtype=F64)
    y64 = a * acc + b
    e = (K + K2 + 4) * U23 * (abs(a) * S + np.abs(b))
    out, lo, hi = bf16(y64), bf16(y64 - e), bf16(y64 + e)
    gf = N if gelu_from is None else gelu_from
    if gf < N:
        g = np.s_[:, gf:]
        ends = [(gelu_tanh(v[g]), gelu_rel(v[g])) for v in (lo, hi)]
        out[g] = bf16(gelu_tanh(out[g]))
        lo[g] = bf16(np.minimum(*[v - r * np.abs(v) for v, r in ends]))
        hi[g] = bf16(np.maximum(*[v + r * np.abs(v) for v, r in ends]))
    if gate is not None:
        gt, r = np.asarray(gate, dtype=F64), np.asarray(res, dtype=F64)
        s0, s1 = r + bf16(gt * lo), r + bf16(gt * hi)
        mn, mx = np.minimum(s0, s1), np.maximum(s0, s1)
        out = bf16(r + bf16(gt * out))
        lo, hi = bf16(mn - _add_slack(mn)), bf16(mx + _add_slack(mx))
    return Ref(out, lo, hi)


def accepted(got, ref):
    """bool [M, N]: got inside the interval (a NaN is outside)"""
    got = np.asarray(got, dtype=F64)
    return (got >= ref.lo) & (got <= ref.hi)


def multi_valued_share(ref):
    """share of the elements whose interval holds more than one bf16 value"""
    return float((ref.lo != ref.hi).mean())


def first_offender(got, ref, what):
    """None when every element is accepted, else a message naming the first offending (m, n), its tile coordinates and its interval"""
    ok = accepted(got, ref)
    if ok.all():
        return None
    m, n = (int(v) for v in np.argwhere(~ok)[0])
    return ("%s: %d of %d elements outside the interval; first at (m, n) = (%d, %d) [128-tile (%d, %d) + (%d, %d); 256-tile (%d, %d) + (%d, %d)]: got %r, reference %r, "
            "accepted [%r, %r]" % (what, int((~ok).sum()), ok.size, m, n, m // 128, n // 128, m % 128, n % 128, m // 256, n // 256, m % 256, n % 256,
                                   float(np.asarray(got, dtype=F64)[m, n]), float(ref.out[m, n]), float(ref.lo[m, n]), float(ref.hi[m, n])))


# ------------------------------------------------------------------------------------------------ the cases of tests/test_gemm_edges_gpu.py
def _case(name, kernel, M, N, K, K2=0, lora_seg_n=None, lora_n_limit=None, nseg=1, alpha=1.0, bias=True, gelu_from=None, gate=None, n_split=None,
          pad_a=0, pad_c=0, pad_c1=0, pad_res=0, pers_grid=0, group_m=0, streamk=None):
    """gate: None / "inplace" (res is C) / "separate" (res its own tensor, leading dimension N + pad_res).  pad_*: columns beyond the logical width of a row."""
    return dict(name=name, kernel=kernel, M=M, N=N, K=K, K2=K2, lora_seg_n=lora_seg_n, lora_n_limit=lora_n_limit, nseg=nseg, alpha=alpha, bias=bias,
                gelu_from=gelu_from, gate=gate, n_split=n_split, pad_a=pad_a, pad_c=pad_c, pad_c1=pad_c1, pad_res=pad_res, pers_grid=pers_grid,
                group_m=group_m, streamk=streamk)


# 128 x 128 kernel (UTX_GEMM_TILE=128).  M: 1 (every staged row clamped to row 0), 7, 127 / 128 / 129 around a tile, 200, 600 (five tile rows: the last GROUP_M group
# holds one).  N: 8 (one 16-byte chunk), 128, 136 (a tail of 8 columns), 264, 384.  K 64 / 128 / 192: one K-tile, then the two-stage ring left at either parity.
CASES_128 = [
    _case("t128_m1_n8", "128", 1, 8, 64, pad_c=16),
    _case("t128_m7_gelu0", "128", 7, 136, 128, gelu_from=0),
    _case("t128_m127_gelu132_lda", "128", 127, 264, 192, gelu_from=132, pad_a=64),
    _case("t128_m128_lora_alpha_nobias", "128", 128, 128, 64, K2=64, lora_seg_n=128, lora_n_limit=128, alpha=0.37, bias=False),
    _case("t128_m129_lora3seg_alpha", "128", 129, 384, 128, K2=128, lora_seg_n=128, lora_n_limit=256, nseg=3, alpha=0.37, pad_c=8),
    _case("t128_m200_loramid_split_gelu128", "128", 200, 384, 192, K2=64, lora_seg_n=128, lora_n_limit=128, nseg=3, gelu_from=128, n_split=128, pad_c=24, pad_c1=40),
    _case("t128_m600_gated_inplace", "128", 600, 264, 64, gate="inplace", pad_c=8),
    _case("t128_m200_gated_separate", "128", 200, 136, 128, gate="separate", pad_c=16, pad_res=40),
    _case("t128_m129_gelu136", "128", 129, 264, 192, gelu_from=136, pad_c=8),
    _case("t128_m600_group2", "128", 600, 136, 64, group_m=2),
]
# one-wave-per-SIMD kernel (UTX_GEMM_TILE=2564).  M = 64 leaves two of the four waves without a valid row, 300 / 600 a ragged last tile row; K 64 one K-tile, then
# even and odd K-tile counts for the two-K-tiles-per-trip stream; lora_n_limit 256 of N 768 alternates tiles with and without the LoRA segment.
CASES_W4 = [
    _case("w4_m1", "w4", 1, 256, 64, pad_c=8),
    _case("w4_m64_alpha_nobias", "w4", 64, 512, 128, alpha=0.37, bias=False),
    _case("w4_m129_lora", "w4", 129, 768, 192, K2=64, lora_seg_n=256, lora_n_limit=256, nseg=3),
    _case("w4_m256_gelu_split", "w4", 256, 512, 320, gelu_from=256, n_split=256, pad_c=8, pad_c1=24),
    _case("w4_m257_lora_alpha", "w4", 257, 768, 128, K2=128, lora_seg_n=256, lora_n_limit=256, nseg=3, alpha=0.37),
    _case("w4_m300_gated", "w4", 300, 256, 192, gate="inplace", pad_c=16),
    _case("w4_m600_gated_grid1", "w4", 600, 512, 320, gate="inplace", pers_grid=1),
    _case("w4_m600_gelu_split_grid2", "w4", 600, 512, 192, gelu_from=256, n_split=256, pers_grid=2),
    _case("w4_m600_lora_grid3", "w4", 600, 512, 128, K2=64, lora_seg_n=256, lora_n_limit=512, nseg=2, pers_grid=3),
    _case("w4_m600_lora_alternating_grid1", "w4", 600, 768, 64, K2=128, lora_seg_n=256, lora_n_limit=256, nseg=3, pers_grid=1),
]
# split tail: six tiles on a grid of four -> T = 2 tail tiles, cut into S ranges; plain and gated (the two fix-up instances)
CASES_SPLIT = [
    _case("sk_s%d_k%d_%d_%s" % (S, K, K2, "gated" if gated else "plain"), "w4", 600, 512, K, K2=K2, lora_seg_n=256 if K2 else None, lora_n_limit=512 if K2 else None,
          nseg=2 if K2 else 1, gate="inplace" if gated else None, pers_grid=4, streamk=S)
    for S, K, K2 in ((4, 192, 64), (3, 320, 0), (2, 128, 128)) for gated in (False, True)
]
CASES = CASES_128 + CASES_W4 + CASES_SPLIT


def make_inputs(case, seed=20261):
    """the operands of one case: float64 arrays of bf16 values (A, B, bias, A2, B2, gate, res; None where the case has none), from a fixed seed and the case's name"""
    rng = np.random.default_rng([seed, zlib.crc32(case["name"].encode())])
    M, N, K, K2 = case["M"], case["N"], case["K"], case["K2"]
    sign = rng.choice([-1.0, 1.0], (N, 1))
    inp = dict(A=bf16(rng.uniform(0.5, 1.5, (M, 1)) * np.abs(rng.normal(0, 0.5, (M, K)))),
               B=bf16(sign * rng.uniform(0.3, 1.5, (N, 1)) * np.abs(rng.normal(0, 1, (N, K))) * 3.0 / K),
               bias=bf16(sign[:, 0] * np.abs(rng.normal(0, 1, N))) if case["bias"] else None, A2=None, B2=None, gate=None, res=None)
    if K2:
        inp["A2"] = bf16(rng.normal(0, 0.5, (M, case["nseg"] * K2)) / 8)
        inp["B2"] = bf16(rng.normal(0, 1 / np.sqrt(K2), (N, K2)) / 4)
    if case["gate"]:
        inp["gate"], inp["res"] = bf16(rng.normal(0, 1, N)), bf16(rng.normal(0, 1, (M, N)))
    return inp


def reference(case, inp):
    return gemm(inp["A"], inp["B"], inp["bias"], inp["A2"], inp["B2"], case["lora_seg_n"], case["lora_n_limit"], case["alpha"], case["gelu_from"],
                inp["gate"], inp["res"], case["n_split"])


def split_cols(x, n_split):
    """[M, N] -> (C part, C1 part or None)"""
    return (x, None) if n_split is None or n_split >= x.shape[1] else (x[:, :n_split], x[:, n_split:])


# ------------------------------------------------------------------------------------------------ float32 emulation of the kernels, with defects
DEFECTS = ("drop_last_k_tile", "skip_lora_seg1", "a2_seg0_for_seg1", "alpha_on_bias", "round_acc_before_bias", "gelu_4_late", "gate_y_unrounded",
           "n_tail_group_unwritten")


def _rbf32(x):
    """float32 -> float32 holding the nearest bf16"""
    return bf16(np.asarray(x, dtype=np.float32).astype(F64)).astype(np.float32)


def gelu_f32(x):
    """the kernels' GELU expression on float32 x, not yet rounded to bf16"""
    f = np.float32
    with np.errstate(over="ignore"):
        return x * (f(1) / (f(1) + np.exp(f(-2) * (f(K0) * (x + f(K1) * x * x * x)))))


def emulate_lora(acc, case, inp, defect=None):
    """adds the bf16 LoRA segments to the float32 accumulators acc [M, N] in place, K2 in tiles of 64"""
    f, N, K2 = np.float32, acc.shape[1], case["K2"]
    if K2:
        A2, B2 = inp["A2"].astype(f), inp["B2"].astype(f)
        for s, (cols, ks) in enumerate(_lora_segments(N, K2, case["lora_seg_n"], case["lora_n_limit"])):
            if s == 1 and defect == "skip_lora_seg1":
                continue
            if s == 1 and defect == "a2_seg0_for_seg1":
                ks = slice(0, K2)
            for kt in range(K2 // 64):
                acc[:, cols] += A2[:, ks][:, 64 * kt: 64 * kt + 64] @ B2[cols][:, 64 * kt: 64 * kt + 64].T
    return acc


def emulate_epilogue(acc, case, inp, defect=None):
    """float32 accumulators -> [M, N] float64 of bf16 values: y = bf16(alpha * acc + bias), GELU by the kernels' expression, bf16(gate * y), bf16(res + .)"""
    f, N = np.float32, acc.shape[1]
    alpha = f(case["alpha"])
    b = np.zeros(N, dtype=f) if inp["bias"] is None else inp["bias"].astype(f)
    if defect == "alpha_on_bias":
        y = _rbf32((acc + b) * alpha)
    elif defect == "round_acc_before_bias":
        y = _rbf32(_rbf32(acc * alpha) + b)
    else:
        y = _rbf32(acc * alpha + b)
    gf = N if case["gelu_from"] is None else case["gelu_from"]
    gf += 4 if defect == "gelu_4_late" else 0
    if gf < N:
        y[:, gf:] = _rbf32(gelu_f32(y[:, gf:]))
    if case["gate"]:
        t = inp["gate"].astype(f) * y              # a product of two bf16 values: exact in float32
        y = _rbf32(inp["res"].astype(f) + (t if defect == "gate_y_unrounded" else _rbf32(t)))
    out = y.astype(F64)
    if defect == "n_tail_group_unwritten":
        out[:, N - 8:] = SENT
    return out


def emulate(case, inp, defect=None):
    """what the kernels compute, in numpy float32: K-tiles of 64 accumulated in float32, y = bf16(alpha * acc + bias), GELU by the kernels' expression, bf16(gate * y),
    bf16(res + .).  defect: one of DEFECTS, the mistake of that name; None: none.  -> [M, N] float64 of bf16 values (SENT where nothing was written)."""
    assert defect is None or defect in DEFECTS
    f = np.float32
    A, B = inp["A"].astype(f), inp["B"].astype(f)
    (M, K), N = A.shape, B.shape[0]
    acc = np.zeros((M, N), dtype=f)
    for kt in range(K // 64 - (1 if defect == "drop_last_k_tile" else 0)):
        acc += A[:, 64 * kt: 64 * kt + 64] @ B[:, 64 * kt: 64 * kt + 64].T
    return emulate_epilogue(emulate_lora(acc, case, inp, defect), case, inp, defect)

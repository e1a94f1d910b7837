"""float64 reference (TEST INFRASTRUCTURE ONLY) of the MX fp8 attention contract in include/unitex_hip.h (utx_attn_fwd_fp8*), with a COUNTED acceptance interval per
output element, the input sets of tests/test_attention_fp8_edges_gpu.py, and a float32 emulation of csrc/attention_fp8.hip that can be told to make one mistake
(tests/test_attention_fp8_ref_cpu.py runs it through the same acceptance check: correct it must pass, with a defect it must not).  The sibling of oracle/attention_fp64.py:
bf16, SENT16, split_plan, split_rows, split_term, accepted, first_offender, the target map and the key-multiplicity rule are that module's and are not restated here.

Operands.  Quantised on the host by oracle/mx8_ref.quantize (Q and K as [H * S_pad, 128], V^T as [H * 128, S_pad], its scales permuted to [H][S_pad / 32][32][4]) and uploaded
as bytes.  e4m3 x 2^(byte - 127) is exact in float64, so the reference works on exactly what the MFMAs see and operand quantisation is NOT part of the interval.
    out[i, h, :] = sum_j W_ij v_j,   W = softmax_2 of q_i . k_j + kb [tile(j) carries the key multiplicity],   keys >= S_kv absent;  rounded ONCE to bf16.

The interval.  bf16(ref - E) <= out <= bf16(ref + E),   E = (1 + 2^-7) E_p + (1 + 2^-4 + 2^-7) (E_w + r A [+ split_term]),   A = sum_j W_ij |v_jd|.
Units U = 2^-23 (doubled, as in the sibling oracles).  n = S_kv, nt = ceil(n / 64).  Every count below was read in csrc/attention_fp8.hip; no GPU number is in any of them.
  E_w = sum_j W_ij e_ij (|v_jd| + |ref|),   e_ij = ln 2 * N_s U (sum_d |q_id k_jd| + |kb| + M_i) + N_e 2 U,   M_i = max_j |score_ij|      (the form of attention_fp64.py)
      N_s = 128 + 1 + 2 nt:  128 product-and-adds of the four-MFMA chain started from negm (e4m3 x e4m3 products under power-of-two scales are exact in fp32; the block
            scales are exact), `sa += key_bias_log2`, and per re-centre `sa -= d` against the rounded `m_run += d`.  A re-centre happens at most once per TILE here
            (the check `ps0 <= 256 && ps1 <= 256` stands behind both blocks of a tile), not once per block as in attention_glds.hip.
      N_e = 1 + nt v_exp_f32 (1 ulp by the ISA reference's VOP1 table, doubled): the probability and one alpha = 2^-d per re-centre.
  E_p, P to e4m3 -- the term the bf16 kernel does not have.  `l_run += ps0 + ps1` sums the UNROUNDED fp32 probabilities, so it is the numerator's alone.  The conversion is
      v_cvt_pk_fp8_f32 (__builtin_amdgcn_cvt_pk_fp8_f32 in A8_EXPB / A8_EXPQ).  Rounding mode, where it was read: the SAME builtin converts the elements in quant_vt_mx8_kernel
      (attention_fp8.hip) and in the utx_quant_mx8 kernels, whose bytes tests/test_fp8_gpu.py, tests/test_attention_fp8_gpu.py and tests/test_attention_fp8_edges_gpu.py pin,
      byte for byte and including subnormal results and ties, to torch's float8_e4m3fn cast in oracle/mx8_ref.elements: round to nearest even, gradual underflow, no flush
      of subnormals (the ISA document was not at hand; the pinned bytes are the source, and quant_edge_rows adds subnormal, tie, +-448 and -0 blocks to them).  So, with p = 2^(s - m_run)
      the value that is converted (p <= 256 by the sum check, below e4m3's 448):
            p >= 2^-6 (normal, 3 mantissa bits)   loses at most 2^-4 of itself (half of the spacing 2^-3 at the bottom of a binade)
            p <  2^-6 (subnormal, spacing 2^-9)   loses at most min(p, 2^-10):  p <= 2^-10 becomes 0 (2^-10 itself is a tie and goes to the even 0), 2^-10 < p < 1.5 * 2^-9 becomes 2^-9.
      (The header said "p < 2^-9 flush to zero"; what flushes is p <= 2^-10.)  m_run only grows and is the rounded maximum of the scores seen so far, in a key range of a split
      the range's own, so one unit of p is at most 2^M_i / Z_i = W_i,max of the normalised weights (the rounding of m_run is inside the factor 1 + 2^-7):
            E_p[i, d] = sum_j |v_jd| max(2^-4 W_ij, min(W_ij, 2^-10 W_i,max))
  r A, everything behind P:  (n + nt) U the fp32 accumulation of P V (one add per key -- e4m3 x e4m3 x 2^k is exact --, one `oacc *= alpha` per re-centre), (n + nt + 1) U the
      row sum l (one add per key, one `l_run * alpha` per re-centre, the cross-half add), 2 U `1.0f / l_tot` and `oacc * inv`.
  split_term (attention_fp64.split_term) on the rows of the key-split tail round: the partial rows, part_lse and attn_merge_kernel are the bf16 kernel's.
  second order:  E_p is ONE rounding per probability and has no product with itself; it multiplies every other relative term (each below 2^-7 in sum): factor 1 + 2^-4 on those,
      and 2^-7 for their own squares.

Input sets (make_inputs).  The bf16 oracle's addressed rows spread half of a row's weight over all n keys: exactly the mass the e4m3 grid may drop.  Here:
  K   effective rows k''_j = g + (8 - g . e_b) e_b, g = (f[j % L] + 0.5 N(0, 1)) 2^w[j // 32, d // 32]: f the vector of the key's FAMILY {j, j + L, ..} (family_period: at most five keys,
      in other 32-key blocks from S_kv = 129 on and in other tiles from L = 64 on -- a target's companions are its family, so one direction of q serves all five and the
      cross-talk onto the other keys stays near 128^-1/2 of the score), w in {0, 1} on one channel block that moves with the key block (neighbouring 32-key blocks and tiles:
      different bytes), e_b the unit direction of the key's 32-key block.  What is stored is K = k'' 2^u[h][d // 32], u a rotation of (-6, -2, 2, 6), and Q = q'' 2^-u: the
      block exponents cancel in every product (as in oracle/gemm_mx_fp64.py) and the four scale bytes of one row differ, for Q and for K.
  addressed rows   q'' = sum over the target t(i) and its companions of c_m k''_m, c solved on the DEQUANTISED K (a Gram system of at most 5 x 5) so that the target scores S_i
      and the k companions S_i - log2 k (weights 1/2 and 1/(2 k): 1/8 each at k = 4), S_i the smallest score that leaves every other key >= 22 units below it;
      re-solved twice after quantising Q.  t is attention_fp64._targets: key 0 and S_kv - 1 from every wave slice, tile edges, all 32 positions of one block, all keys in order.
  block rows (every 8th)   q'' = s e_b, s chosen so that every key outside the block is >= 22 units below: even weight over one 32-key block, all 32 probabilities normal e4m3.
  ramp rows   K'' = 0.05 N(0, 1) + linspace(0, ramp) u, q'' = 0.1275 N(0, 1) + u.  The sum check is 2^8 per lane of 16 keys: a ramp of 3 stays below it (16 x 2^3 = 128, never
      re-centres), 6 re-centres a few times (the issue expected none: that was the bf16 kernel's 2^13), 45 again and again.  The emulation counts the re-centres.
  V   one sign per (head, channel): A = |ref|; |v| = (0.5 + U[0, 1)) 2^z[j // 32, d // 32], z = (3 kb + 2 cb + h) % 5 - 2: vs bytes differ between neighbouring key and channel blocks.
  pad   K8 rows in [S_kv, S_pad): 4 x an addressed target row.  V8^T columns there: the opposite sign of their channel at the block's own magnitude.  Q8 rows >= S_q: 0x7E under
      the scale byte 0xF0.  All finite, no 0x7F / 0xFF element byte, no 0xFF scale byte.
"""
import math
import zlib

import numpy as np
import torch

from oracle import attention_fp64 as A
from oracle import mx8_ref
from oracle.attention_fp64 import KVB, LN2, F64, U23, bf16

BLOCK_DIR = 8.0
GAP = 22.0                 # what the solve leaves between the five chosen keys and the rest (the condition asserted on the dequantised operands is 20)
U_EXP = (-6, -2, 2, 6)
E4 = torch.float8_e4m3fn


def _case(name, H, Sq, Sk, kb=0.0, period=0, ramp=0.0, tailsplit=1, data=None, kernel="g"):
    return dict(name=name, kernel=kernel, H=H, Sq=Sq, Sk=Sk, kb=kb, period=period, ramp=ramp, tailsplit=tailsplit, data=data or name, blk_rows=0)


SHAPES = [(1, 1, 1), (2, 33, 40), (1, 63, 63), (3, 64, 64), (2, 65, 65), (1, 100, 127), (2, 129, 129), (1, 192, 192), (3, 300, 520), (2, 257, 300), (1, 40, 1000)]
CASES_G = [_case("f8_h%d_q%d_k%d" % s, *s) for s in SHAPES]
CASES_KB = [_case("f8_kb3_h%d_q%d_k%d" % s, *s, kb=3.0) for s in ((2, 65, 65), (3, 300, 520), (2, 257, 300))]
CASES_PER = [_case("f8_per%d_k%d" % (p, n), 2, 150, n, kb=3.0, period=p) for p, n in A.PERIODIC]
CASES_RAMP = [_case("f8_ramp%d" % r, 2, 256, 1536, ramp=float(r)) for r in (3, 6, 45)]
CASES = CASES_G + CASES_KB + CASES_PER + CASES_RAMP


def split_cases(ncu):
    """attention_fp64.split_cases(ncu) under this module's names (same shapes, periods, key bias, short last range, TAILSPLIT = 0 on the same data)"""
    out = []
    for c in A.split_cases(ncu):
        d = dict(c)
        d["name"], d["data"] = "f8_" + c["name"], "f8_" + c["data"]
        out.append(d)
    return out


def units(n):
    """(N_s, N_e, r) of the module docstring"""
    nt = (n + KVB - 1) // KVB
    return 128 + 1 + 2 * nt, 1 + nt, U23 * ((n + nt) + (n + nt + 1) + 2)


# ------------------------------------------------------------------------------------------------ bytes <-> values
def decode(b):
    """e4m3 bytes (numpy uint8) -> float32 values"""
    return torch.from_numpy(np.ascontiguousarray(b)).view(E4).to(torch.float32).numpy()


def _pow2(e):
    return np.ldexp(np.float32(1.0), np.asarray(e, dtype=np.int32))


def _quant(x):
    """float64 [R, K] of bf16 values -> (bytes [R, K], scale bytes [R, K / 32], dequantised float64 [R, K])"""
    q, s = mx8_ref.quantize(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)))
    return q.numpy(), s.numpy(), mx8_ref.dequantize(q, s).numpy().astype(F64)


def vs_permute(s, H):
    """row-major V^T scales [H * 128, S_pad / 32] -> the kernel's [H][S_pad / 32][d % 32][d / 32]"""
    return np.ascontiguousarray(s.reshape(H, 4, 32, -1).transpose(0, 3, 2, 1))


# ------------------------------------------------------------------------------------------------ reference and interval
def attention64(q, k, v, kb=0.0, period=0, reverse=False):
    """one head in float64 on dequantised operands -> (ref, A, E_p, E_w + r A, W, M, flush part of E_p, 2^-4 part of E_p, smin, smax)"""
    n = k.shape[0]
    b = A._bias(n, kb, period)
    if reverse:
        k, v, b = k[::-1], v[::-1], b[::-1]
    s = q @ k.T + b
    M = np.abs(s).max(-1)
    W = np.exp2(s - s.max(-1, keepdims=True))
    W /= W.sum(-1, keepdims=True)
    av = np.abs(v)
    ref, Aabs = W @ v, W @ av
    ns, ne, r = units(n)
    e = LN2 * ns * U23 * ((np.abs(q) @ np.abs(k).T) + abs(kb) + M[:, None]) + ne * 2 * U23
    We = W * e
    Er = We @ av + np.abs(ref) * We.sum(-1, keepdims=True) + r * Aabs
    fl = np.minimum(W, 2.0 ** -10 * W.max(-1, keepdims=True))
    Ep = np.maximum(2.0 ** -4 * W, fl) @ av
    return ref, Aabs, Ep, Er, W, M, fl @ av, 2.0 ** -4 * Aabs, float(s.min()), float(s.max())


def reference(case, inp, rows_split=None):
    """-> (attention_fp64.Ref over all heads, share of the elements whose flush term exceeds their 2^-4 term, smallest gap in base-2 units between the five chosen keys of an
    addressed row / the block of a block row and every other key)"""
    H, Sq, n = case["H"], case["Sq"], case["Sk"]
    out, lo, hi, Es, As = (np.empty((H, Sq, 128)) for _ in range(5))
    wt = np.full((H, Sq), np.nan)
    smin, smax, nfl = np.inf, -np.inf, 0
    for h in range(H):
        ref, Aabs, Ep, Er, W, M, fl, t4, s0, s1 = attention64(inp["qd"][h], inp["kd"][h, :n], inp["vd"][h, :n], case["kb"], case["period"])
        if rows_split is not None and rows_split[h].any():
            Er = Er + np.where(rows_split[h][:, None], A.split_term(Aabs, M, n, case["kb"]), 0.0)
        E = (1 + 2.0 ** -7) * Ep + (1 + 2.0 ** -4 + 2.0 ** -7) * Er
        out[h], lo[h], hi[h], Es[h], As[h] = bf16(ref), bf16(ref - E), bf16(ref + E), E, Aabs
        t = inp["tgt"][h]
        has = t >= 0
        wt[h, has] = W[np.nonzero(has)[0], t[has]]
        smin, smax, nfl = min(smin, s0), max(smax, s1), nfl + int((fl > t4).sum())
    return A.Ref(out, lo, hi, Es, As, wt, smin, smax), nfl / float(H * Sq * 128)


def rest_gap(case, inp):
    """smallest distance, in base-2 units of the float64 scores on the dequantised operands, between a row's maximum and its keys outside the chosen ones (addressed rows: target
    and companions; block rows: the block); inf where no row has a rest"""
    n, gap = case["Sk"], np.inf
    for h in range(case["H"]):
        s = inp["qd"][h] @ inp["kd"][h, :n].T + A._bias(n, case["kb"], case["period"])
        mx = s.max(-1)
        keep = np.zeros(s.shape, dtype=bool)
        for i in range(case["Sq"]):
            if inp["kind"][h, i] == "a":
                keep[i, inp["chosen"][h, i]] = True
            elif inp["kind"][h, i] == "b":
                keep[i, 32 * inp["blk"][h, i]: 32 * inp["blk"][h, i] + 32] = True
            else:
                keep[i] = True
        rest = np.where(keep, -np.inf, s).max(-1)
        gap = min(gap, float((mx - rest).min()))
    return gap


# ------------------------------------------------------------------------------------------------ input sets
def family_period(n):
    """keys j, j + L, j + 2 L, ... form a family (at most five members): L = ceil(n / 5), at least 32 from n = 129 on (every member in another 32-key block; another tile from L = 64)"""
    L = (n + 4) // 5
    return max(L, 32) if n >= 129 else max(L, 1)


def _companions(t, n):
    """the other members of the target's family (at most four)"""
    L = family_period(n)
    return [j for j in range(t % L, n, L) if j != t][:4]


def make_inputs(case, seed=20268):
    """the operands of one case: bytes q8 [H, S_pad, 128], qs [H, S_pad, 4], k8, ks, v8t [H, 128, S_pad], vs [H, S_pad / 32, 32, 4] (numpy uint8, as uploaded) and their exact
    float64 values qd [H, S_q, 128], kd / vd [H, S_pad, 128] (vd is V, not V^T); per row tgt, kind ('a' addressed, 'b' block, 'r' ramp, 'p' plain), blk, chosen [H, S_q, 5]"""
    rng = np.random.default_rng([seed, zlib.crc32(case["data"].encode())])
    H, Sq, n, kb, period = case["H"], case["Sq"], case["Sk"], case["kb"], case["period"]
    npad = (n + 63) // 64 * 64
    nb32 = npad // 32
    uex = np.array([np.roll(U_EXP, h) for h in range(H)], dtype=F64)                         # [H, 4]
    usc = np.repeat(np.exp2(uex), 32, axis=1)[:, None, :]                                     # [H, 1, 128]
    # V
    sign = rng.choice([-1.0, 1.0], (H, 1, 128))
    z = (3 * np.arange(nb32)[None, :, None] + 2 * np.arange(4)[None, None, :] + np.arange(H)[:, None, None]) % 5 - 2.0
    zs = np.repeat(np.repeat(np.exp2(z), 32, axis=1), 32, axis=2)                             # [H, npad, 128]
    v = sign * (0.5 + rng.random((H, npad, 128))) * zs
    v[:, n:] = -sign * 1.5 * zs[:, n:]
    v = A._q16(v)
    # K''
    tgt = np.full((H, Sq), -1, dtype=np.int64)
    blk = np.full((H, Sq), -1, dtype=np.int64)
    chosen = np.full((H, Sq, 5), -1, dtype=np.int64)
    kind = np.full((H, Sq), "p")
    w = np.zeros((H, nb32, 4))
    for b in range(nb32):
        if (3 * b) % 5 < 4:                                                                   # the raised channel block moves with the key block (cycle of five, one of them flat)
            w[:, b, (3 * b) % 5] = 1.0
    ws = np.repeat(np.repeat(np.exp2(w), 32, axis=1), 32, axis=2)
    if case["ramp"] > 0:
        u = A._unit(rng.normal(size=(H, 1, 128)))
        k2 = 0.05 * rng.normal(size=(H, npad, 128)) * ws
        k2[:, :n] += np.linspace(0.0, case["ramp"], n)[None, :, None] * u
        k2[:, n:] = 4.0 * k2[:, n - 1: n]
        q2 = 0.1275 * rng.normal(size=(H, Sq, 128)) + u
        kind[:] = "r"
    else:
        e = A._unit(rng.normal(size=(H, nb32, 128)))
        eb = np.repeat(e, 32, axis=1)
        fam = rng.normal(size=(H, family_period(n), 128))
        g0 = (fam[:, np.arange(npad) % family_period(n)] + 0.5 * rng.normal(size=(H, npad, 128))) * ws
        k2 = g0 + (BLOCK_DIR - (g0 * eb).sum(-1, keepdims=True)) * eb
        q2 = 0.1275 * rng.normal(size=(H, Sq, 128))
        if n > 1:
            nfull = n // 32
            tgt, blk = A._targets(H, Sq, n, min(max(nfull - 1, 0), ((n + 31) // 32) // 2))
        else:
            k2[:, n:] = 4.0 * q2[:, :1] / np.abs(q2[:, :1]).max()
    k = A._q16(k2 * usc)
    if case["ramp"] == 0 and n > 1:                                                          # pad rows: exactly 4 x the (bf16) target row
        for h in range(H):
            for p in range(n, npad):
                t = tgt[h, (p - n) % Sq]
                k[h, p] = 4.0 * k[h, t if t >= 0 else n - 1]
    k8, ks, kd = _quant(k.reshape(H * npad, 128))
    kd = kd.reshape(H, npad, 128)
    kd2 = kd / usc                                                                            # the effective rows, dequantised (powers of two: exact)
    bias = A._bias(n, kb, period)

    def quant_q(q2_):
        q8_, qs_, qd_ = _quant(A._q16(q2_ / usc).reshape(H * Sq, 128))
        return q8_.reshape(H, Sq, 128), qs_.reshape(H, Sq, 4), qd_.reshape(H, Sq, 128)

    if case["ramp"] == 0 and n > 1:
        sols = []
        for h in range(H):
            K = kd2[h, :n]
            rows = np.nonzero(tgt[h] >= 0)[0]
            comp = {int(i): _companions(int(tgt[h, i]), n) for i in rows}
            for nc in sorted({len(c) + 1 for c in comp.values()}):                             # families of one size together: one batched Gram solve
                a = np.array([i for i in rows if len(comp[int(i)]) + 1 == nc], dtype=np.int64)
                ch = np.array([[tgt[h, i]] + comp[int(i)] for i in a], dtype=np.int64)        # [rows, nc]
                chosen[h, a, :nc] = ch
                K5 = K[ch]                                                                    # [rows, nc, 128]
                Gi = np.linalg.inv(K5 @ K5.transpose(0, 2, 1))
                off = np.concatenate([[0.0], np.full(nc - 1, math.log2(max(nc - 1, 1)))])     # the companions share the other half of the weight
                c1, c2 = Gi.sum(-1), (Gi @ (off[None, :] + bias[ch])[..., None])[..., 0]      # coefficients = S c1 - c2
                a1 = np.einsum("rm,rmd->rd", c1, K5) @ K.T                                    # score of every key per unit of S
                a2 = np.einsum("rm,rmd->rd", c2, K5) @ K.T - bias[None, :]
                a1[np.arange(len(a))[:, None], ch] = -np.inf
                need = np.where(np.isfinite(a1), (GAP - a2) / np.maximum(1.0 - np.maximum(a1, -1e30), 1e-3), 0.0)
                S = np.maximum(need.max(-1), 24.0)
                q2[h, a] = np.einsum("rm,rmd->rd", S[:, None] * c1 - c2, K5)
                kind[h, a] = "a"
                sols.append((h, a, ch, Gi, S, off))
            bq = np.nonzero(blk[h] >= 0)[0]
            eb_h = e[h, blk[h, bq]]
            sc = eb_h @ K.T                                                                   # [rows, n] per unit of s
            inb = (np.arange(n)[None, :] // 32) == blk[h, bq][:, None]
            lo_in = np.where(inb, sc, np.inf).min(-1)
            hi_out = np.where(inb, -np.inf, sc + 0.0).max(-1) if n > 32 else np.full(len(bq), -np.inf)
            hi_b = np.where(inb, -np.inf, bias[None, :]).max(-1) - np.where(inb, bias[None, :], np.inf).min(-1) if n > 32 else np.zeros(len(bq))
            s_in = np.where(np.isfinite(hi_out), (GAP + np.maximum(hi_b, 0.0)) / np.maximum(lo_in - hi_out, 0.25), 3.0)
            q2[h, bq] = np.maximum(s_in, 3.0)[:, None] * eb_h
            kind[h, bq] = "b"
        for _ in range(2):                                                                    # re-solve on the dequantised Q: the residual of the five scores goes back through the Gram system
            _, _, qd = quant_q(q2)
            for h, a, ch, Gi, S, off in sols:
                K5 = kd2[h][ch]
                have = np.einsum("rd,rmd->rm", qd[h, a] * usc[h], K5) + bias[ch]
                want = S[:, None] - off[None, :]
                q2[h, a] += np.einsum("rm,rmd->rd", (Gi @ (want - have)[..., None])[..., 0], K5)
    q8s, qss, qd = quant_q(q2)
    q8 = np.full((H, npad, 128), 0x7E, dtype=np.uint8)
    qs = np.full((H, npad, 4), 0xF0, dtype=np.uint8)
    q8[:, :Sq], qs[:, :Sq] = q8s, qss
    v8, vsr, vdt = _quant(np.ascontiguousarray(v.transpose(0, 2, 1)).reshape(H * 128, npad))
    return dict(q8=q8, qs=qs, k8=k8.reshape(H, npad, 128), ks=ks.reshape(H, npad, 4), v8t=v8.reshape(H, 128, npad), vs=vs_permute(vsr, H),
                qd=qd, kd=kd, vd=np.ascontiguousarray(vdt.reshape(H, 128, npad).transpose(0, 2, 1)), tgt=tgt, kind=kind, blk=blk, chosen=chosen)


def byte_counts(case, inp):
    """distinct scale bytes: (smallest count within one valid Q row, within one valid K row, over the rows of K for channel block 0 -- per head, the smallest --, over V^T's key blocks
    for channel 0, over V^T's four channel blocks of key block 0) and whether every pair of neighbouring 32-key blocks (b, b + 1) and tiles (b, b + 2) differs in the most frequent
    four-byte scale row of K (ramp cases exempt: their rows follow the ramp) and in vs"""
    H, Sq, n = case["H"], case["Sq"], case["Sk"]
    qrow = min(len(set(r.tolist())) for r in inp["qs"][:, :Sq].reshape(-1, 4))
    krow = min(len(set(r.tolist())) for r in inp["ks"][:, :n].reshape(-1, 4))
    kcol = min(len(set(inp["ks"][h, :n, 0].tolist())) for h in range(H))
    vkb = min(len(set(inp["vs"][h, :, 0, 0].tolist())) for h in range(H))
    vcb = min(len(set(inp["vs"][h, 0, 0, :].tolist())) for h in range(H))
    nb = (n + 31) // 32

    def modal(rows):
        t, c = np.unique(rows, axis=0, return_counts=True)
        return tuple(t[np.argmax(c)].tolist())
    kblk = [[modal(inp["ks"][h, 32 * b: min(32 * b + 32, n)]) for b in range(nb)] for h in range(H)]
    neigh = case["ramp"] > 0 or all(kblk[h][b] != kblk[h][b + d] for h in range(H) for d in (1, 2) for b in range(nb - d))
    neigh = neigh and all(not np.array_equal(inp["vs"][h, b], inp["vs"][h, b + d]) for h in range(H) for d in (1, 2) for b in range(inp["vs"].shape[1] - d))
    return qrow, krow, kcol, vkb, vcb, neigh


# ------------------------------------------------------------------------------------------------ float32 emulation of attention_fp8.hip, with defects
DEFECTS = ("ragged_mask_without_16_lh",        # 1  lim = S - 64 t for both lane halves
           "pad_keys_unmasked",                # 2
           "key_bias_on_tile_1",               # 3
           "periodic_bias_on_local_tile",      # 4  t % period instead of (tb + t) % period inside a key split
           "p_groups_swapped",                 # 5  8-key groups 1 and 2 of every 32-key block swapped in P, not in V
           "no_o_rescale",                     # 6
           "pv_under_this_tiles_v_scales",     # 7  vsc where vsc_pv belongs: PV(t - 1) under tile t's V scales
           "block1_under_block0_k_scales",     # 8  ksc0 for both 32-key blocks of a tile
           "upper_half_qs_not_shifted",        # 9  lanes 32-63 supply byte 0 / 2 of qs: channel blocks 1 and 3 under the scales of 0 and 2
           "vs_read_transposed",               # 10 vs read as [d / 32][d % 32]
           "split_scales_not_advanced",        # 11 ksb / vsb of a key range start at the sequence's first key
           "prefetched_scales_stuck_at_tile_0",    # 12
           "drop_last_full_tile",              # 13
           "merge_drops_last_range",           # 14
           "wave_rows_32_off")                 # 15


def _e4(x):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(E4).to(torch.float32).numpy()


def _core(q, Ke, kse, Ve, vse, Sk, tb, kb, period, defect, stats):
    """the kernel's loop over the Sk keys of one key range: q [B, R, 128] dequantised float32 (R a multiple of 32), Ke / Ve [B, T, 128] decoded e4m3 elements of K and V (T whole
    tiles), kse [B, T, 4] / vse [B, T / 32, 128] the scale exponents AS THE KERNEL READS THEM for this range -> (O unnormalised, l, m)"""
    f = np.float32
    B, R, _ = q.shape
    nt = (Sk + KVB - 1) // KVB
    T = Ke.shape[1]
    kse, vse = kse[:, :T].copy(), vse[:, : T // 32].copy()
    if defect == "block1_under_block0_k_scales":
        k4 = kse.reshape(B, T // 64, 2, 32, 4)
        k4[:, :, 1] = k4[:, :, 0]
    if defect == "prefetched_scales_stuck_at_tile_0":
        kse = np.tile(kse[:, :64], (1, T // 64, 1))
        vse = np.tile(vse[:, :2], (1, T // 64, 1))
    if defect == "vs_read_transposed":
        d = np.arange(128)
        vse = vse[:, :, (d // 4) + 32 * (d % 4)]
    if defect == "pv_under_this_tiles_v_scales" and T > 64:
        v4 = vse.reshape(B, T // 64, 2, 128).copy()
        v4[:, :-1] = v4[:, 1:].copy()
        vse = v4.reshape(B, T // 32, 128)
    K = Ke * _pow2(np.repeat(kse, 32, axis=-1))
    V = Ve * _pow2(np.repeat(vse, 32, axis=1))
    if defect == "drop_last_full_tile" and Sk % KVB == 0:
        nt -= 1
    m, l, O = np.zeros((B, R), f), np.zeros((B, R), f), np.zeros((B, R, 128), f)
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(nt):
            ragged = t == nt - 1 and Sk % KVB != 0
            tg = tb + t
            if period > 0:
                kbias = (t if defect == "periodic_bias_on_local_tile" else tg) % period == 0
            else:
                kbias = tg == (1 if defect == "key_bias_on_tile_1" else 0)
            j = t * KVB + np.arange(KVB)
            lh = (j % 32) // 16
            valid = (j - (16 * lh if defect == "ragged_mask_without_16_lh" else 0)) < Sk
            if defect == "pad_keys_unmasked":
                valid[:] = True
            sa = np.matmul(q, K[:, j].transpose(0, 2, 1)) - m[..., None]
            if kbias and kb != 0:
                sa = sa + f(kb)
            if ragged:
                sa = np.where(valid[None, None, :], sa, f(-np.inf))
            P = np.exp2(sa)
            lane = P.reshape(B, R, 4, 16).sum(-1)
            over = np.repeat((~(lane <= 256.0)).any(-1).reshape(B, R // 32, 32).any(-1), 32, axis=1)
            if t == 0 or ragged:
                over[:] = True
            else:
                stats["recentres"] = stats.get("recentres", 0) + int(over.sum()) // 32
            if over.any():
                mx = sa.max(-1)
                d = mx if t == 0 else np.maximum(mx, f(0))
                alpha = np.ones_like(d) if t == 0 else np.exp2(-d)
                d, alpha = np.where(over, d, f(0)), np.where(over, alpha, f(1))
                m, l = m + d, l * alpha
                if defect != "no_o_rescale":
                    O = O * alpha[..., None]
                P = np.exp2(sa - d[..., None])
            l = l + P.sum(-1)
            P8 = _e4(P)
            if defect == "p_groups_swapped":
                P8 = P8.reshape(B, R, 2, 4, 8)[:, :, :, [0, 2, 1, 3]].reshape(B, R, 64)
            O = O + np.matmul(P8, V[:, j])
    return O, l, m


def emulate(case, inp, plan=None, defect=None, stats=None):
    """what utx_attn_fwd_fp8 computes, in numpy float32: 64-key tiles, the per-tile sum check at 256 per lane (16 keys of a block) with wave-wide re-centring, l from the unrounded
    probabilities, P through the float8_e4m3fn cast, PV of the dequantised V; the tail items of `plan` through the key split with bf16 partial rows and the log-sum-exp merge.
    -> [H, S_q, 128] float64 of bf16 values (SENT where nothing was written).  stats: a dict that receives the number of re-centres that the sum check asked for"""
    assert defect is None or defect in DEFECTS
    stats = {} if stats is None else stats
    f = np.float32
    H, Sq, n, kb, period = case["H"], case["Sq"], case["Sk"], case["kb"], case["period"]
    R = (Sq + 31) // 32 * 32
    qse = inp["qs"][:, :Sq].astype(np.int32) - 127
    if defect == "upper_half_qs_not_shifted":
        qse = qse[..., [0, 0, 2, 2]]
    q = decode(inp["q8"][:, :Sq]) * _pow2(np.repeat(qse, 32, axis=-1))
    q = np.concatenate([q, np.repeat(q[:, -1:], R - Sq, axis=1)], 1)           # rows past S_q repeat the last query (the kernel clamps the row index)
    Ke, Ve = decode(inp["k8"]), np.ascontiguousarray(decode(inp["v8t"]).transpose(0, 2, 1))
    kse = inp["ks"].astype(np.int32) - 127
    vse = np.ascontiguousarray(inp["vs"].astype(np.int32).transpose(0, 1, 3, 2)).reshape(H, -1, 128) - 127      # [H, key block, d = 32 (d / 32) + d % 32]
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        O, l, _ = _core(q, Ke, kse, Ve, vse, n, 0, kb, period, defect, stats)
        out = A._rb(O * (f(1) / l)[..., None])[:, :Sq].astype(F64)
        if plan is not None and plan[2] > 1:
            nqb, ns, tps = (Sq + 255) // 256, plan[2], plan[3]
            for w in range(plan[1], plan[0]):
                h, r0 = w // nqb, (w % nqb) * 256
                r1 = min(r0 + 256, R)
                parts = []
                for s in range(ns):
                    k0 = s * tps * KVB
                    sk = min(n - k0, tps * KVB)
                    k1 = k0 + (sk + 63) // 64 * 64
                    s0 = 0 if defect == "split_scales_not_advanced" else k0
                    Os, ls, ms = _core(q[h: h + 1, r0:r1], Ke[h: h + 1, k0:k1], kse[h: h + 1, s0: s0 + k1 - k0], Ve[h: h + 1, k0:k1], vse[h: h + 1, s0 // 32: (s0 + k1 - k0) // 32],
                                       sk, s * tps, kb, period, defect, {})
                    parts.append((A._rb(Os[0] * (f(1) / ls[0])[:, None]), ms[0] + np.log2(ls[0])))
                if defect == "merge_drops_last_range":
                    parts = parts[:-1]
                M = np.max([p[1] for p in parts], 0)
                acc, Wt = np.zeros((r1 - r0, 128), f), np.zeros(r1 - r0, f)
                for On, lse in parts:
                    wgt = np.exp2(lse - M)
                    Wt = Wt + wgt
                    acc = acc + wgt[:, None] * On
                out[h, r0: min(r1, Sq)] = A._rb(acc * (f(1) / Wt)[:, None])[: min(r1, Sq) - r0].astype(F64)
    if defect == "wave_rows_32_off":
        moved = out[:, 32:64].copy()
        out[:, 32:64] = A.SENT
        out[:, 64:96] = moved[:, : max(0, min(96, Sq) - 64)]
    return out


# ------------------------------------------------------------------------------------------------ the quantisers at their edges (section 5 of the GPU test)
def quant_edge_rows(R, K, seed):
    """float32 [R, K] of bf16 values whose 32-blocks walk the quantisers' edges: all zero, amax exactly 2^k, amax just below 2^k, bf16 subnormals (the exponent clamps at -127),
    amax about 2^120 (the upper clamp), -0, elements that hit +-448 exactly after scaling; everything else N(0, 1) 2^(-3 .. 3)"""
    rng = np.random.default_rng([seed, R, K])
    x = (rng.normal(size=(R, K // 32, 32)) * np.exp2(rng.integers(-3, 4, (R, K // 32, 1)))).astype(np.float32)
    kinds = ("zero", "pow2", "below_pow2", "subnormal", "huge", "negzero", "hit448")
    for r in range(R):
        for b in range(K // 32):
            kind = kinds[(r + 3 * b) % 11] if (r + 3 * b) % 11 < len(kinds) else None
            blk = x[r, b]
            if kind == "zero":
                blk[:] = 0.0
            elif kind == "pow2":
                blk[:] = np.clip(blk, -1.0, 1.0); blk[(r + b) % 32] = -4.0
            elif kind == "below_pow2":
                blk[:] = np.clip(blk, -1.0, 1.0); blk[(r + b) % 32] = 3.984375          # bf16 just below 4
            elif kind == "subnormal":
                blk[:] = (rng.integers(-127, 128, 32) * 2.0 ** -133).astype(np.float32)   # multiples of the smallest bf16 subnormal
            elif kind == "huge":
                blk[:] = blk * np.float32(2.0 ** 118); blk[(r + b) % 32] = np.float32(1.5 * 2.0 ** 120)
            elif kind == "negzero":
                blk[::2] = -0.0
            elif kind == "hit448":
                blk[:] = np.clip(blk, -1.0, 1.0); blk[0], blk[1], blk[2] = 448.0, -448.0, 256.0   # amax 448 -> e = 0: +-448 exactly
    x = x.reshape(R, K)
    return torch.from_numpy(x).to(torch.bfloat16)

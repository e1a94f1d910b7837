"""float64 reference (TEST INFRASTRUCTURE ONLY) of the bf16 attention contract in include/unitex_hip.h (utx_attn_fwd_bf16*), with a COUNTED acceptance interval
per output element, the input sets of tests/test_attention_edges_gpu.py, and a float32 emulation of the kernels that can be told to make one mistake
(tests/test_attention_ref_cpu.py runs it through the same acceptance check: correct it must pass, with a defect it must not).

numpy on the CPU.  Arrays hold bf16-representable values.  The contract:
    out[i, h, :] = sum_j w_ij v_j / sum_j w_ij,      w_ij = 2^(c q_i . k_j + kb [tile(j) carries the key multiplicity])
    c = f32(f32(scale) * f32(log2 e)) (attention.hip: `p.scale_log2 = scale * 1.4426950408889634f`), c = 1 for scale == 0 (Q pre-scaled upstream)
    tile(j) = j // 64 carries the multiplicity when it is tile 0 or, with key_bias_period = n > 0, when tile(j) % n == 0;  keys >= S_kv are absent.
The float64 value is rounded ONCE to bf16 (oracle/dit_glue_fp64.bf16).  Nothing in reference() knows tiles, waves, rings or key splits.

The interval.  With normalised weights W_ij = w_ij / sum_j w_ij, ref = sum_j W_ij v_jd and A = sum_j W_ij |v_jd|:
    bf16(ref - E) <= out <= bf16(ref + E),      E = (1 + 2^-7) (E_w + r A)
Every unit below is U = 2^-23, TWICE round-to-nearest's, as in oracle/gemm_fp64.py: how the matrix unit rounds inside one instruction is not documented, and with
the doubled unit the bound also holds for truncated internal sums.  No GPU number went into any term.  n = S_kv, nt = ceil(n / 64) tiles, 2 nt blocks.
  E_w, the error of the weights.  A relative error e_ij of w_ij moves the quotient by sum_j W_ij e_ij (v_jd - ref) to first order, so
        E_w = sum_j W_ij e_ij (|v_jd| + |ref|),      e_ij = ln 2 * N_s U (|c| sum_d |q_id k_jd| + |kb| + M_i) + N_e 2 U,      M_i = max_j |score_ij|
      N_s, the score's roundings (ln 2 turns an error of a base-2 exponent into a relative error of the probability), read in attention_glds.hip:
        128   one per product-and-add of the QK^T chain of 8 MFMAs x 16 terms; the chain starts from the register block holding -m_run (AG_MM(sa0, .., negm)),
              so the running maximum enters through the same adds and every partial sum is bounded by |c| sum|q k| + |m_run|, |m_run| <= M_i
          1   `sa_[r] -= d_` of AG_SLOW (a block-1 score that saw `other_[r] -= d_` and then its own slow path is recomputed from the MFMAs: one, not two)
          1   `sa[r] += kbv` on a key-multiplicity tile
          1   kbv = key_bias_log2 / c2 of the scale > 0 instances (one division, against |kb|)
          1   `sa_[r] * c2` of the scale > 0 instances (AG_EXPB, PRESC = 0); counted for the pre-scaled ones too
       4 nt   a re-centre (at most one per block) rounds `m_run += d_` while the block's own scores were moved by the unrounded d_, and the scale > 0 instances
              round `-d_ * c2` before alpha: two units against M_i each time, as an error of every weight summed before that block against those behind it
      N_e = 1 + 2 nt v_exp_f32: the probability itself and one alpha = 2^(-d) per re-centre (alpha multiplies O and l alike, so only its disagreement with the new
              block's probabilities counts).  v_exp_f32 and v_log_f32 are documented as 1 ulp (AMD Instinct CDNA3 / CDNA4 ISA reference, VOP1 opcode table:
              "V_EXP_F32 ... 1ULP accuracy", "V_LOG_F32 ... 1ULP accuracy"); doubled: 2 U each.
      The 4 x 64 kernel (attention_q64.hip) never re-centres and centres on the exact maximum of the first block: its N_s and N_e are smaller.
  r, everything behind the probabilities:
      2^-8         P to bf16: `(__bf16)pv_` in AG_EXPB compiles to v_cvt_pk_bf16_f32 on gfx950, and tools/gen_attn_q64.py emits the same instruction for the 4 x 64 stream:
                   round to nearest even in BOTH kernels, none truncates.  bf16 carries 8 significant bits, so round-to-nearest loses up to HALF of the spacing 2^-7, i.e. 2^-8
                   of the value (a probability just above a power of two; 2^-9 is that error relative to the TOP of the binade, and truncation would be 2^-7).
                   l sums the unrounded fp32 probabilities (`sc0_ += pv_[0]`), so this term is the numerator's alone.
      (n + 2 nt) U  fp32 accumulation of P V in the MFMA accumulators: one add per key (the products of two bf16 values are exact), one `oacc *= alpha_` per re-centre
      (n + 2 nt + 1) U  the row sum l: one add per key over sc0_, sc1_, ps, l_run, one `l_run * alpha_` per re-centre, the cross-half add of the epilogue; a relative
                   error of l is weighted by |ref| <= A
      2 U          `1.0f / l_tot` and `oacc * inv`
  rows that went through the key-split tail round (split_rows of reference()) add, with L_i = M_i + log2 n + |kb| >= |lse|,
      A (2^-8 + 2 (ln 2 * 6 U L_i + 2 U) + 36 U)
      2^-8         the partial rows are stored normalised in bf16 (AG_STORE_ROW(p.part_o ..)); sum_i W_i |O_i| <= A over the ranges
      6 U L_i      lse = (m_run [* c2]) + v_log_f32(l_tot): 2 for the logarithm (1 ulp, doubled), 1 for `* c2`, 1 for the add; `part_lse - M` in attn_merge_kernel: 2 (|lse - M| <= 2 L_i)
      2 U          v_exp_f32 of the merge weight; both as errors of a weight (numerator and denominator: the factor 2)
      36 U         attn_merge_kernel's own arithmetic at up to 16 ranges: `acc += wgt * O` (a product and an add per range), `W += wgt`, `1.0f / W`, `acc * inv`
  (1 + 2^-7)       the second-order products of the terms above, each of which is below 2^-7.
Probabilities below the fp32 normal range (2^-126 of the row's largest) are flushed or denormal; their share of any sum is below every term above.

Input sets (make_inputs).  Every defect of DEFECTS must move some element by many times E:
  V   channel d of head h has ONE sign, so A = |ref| and the interval is relative; |v_jd| = 0.25 + U[0, 1) + c[j // 32, d], c in {0, 1}: keys and 32-key blocks differ.
  K   N(0, 1) with the component along a unit direction e_b of the key's 32-key block set to 4 (what the block rows aim at).
  addressed rows   q_i = g_i (k_t(i) + 0.05 N(0, 1)), g_i solved (Newton on the float64 log-odds) so that key t(i) holds half of the row's weight.  t sends queries of every
      32-query wave slice to key 0 and key S_kv - 1, walks the first and last key of every 64-key tile and every position of one 32-key block (the kappa permutation)
      eight per slice, and walks all keys in order with the rest, so that H * S_q rows cover every key where there are that many rows (coverage() reports it).
  block rows   every 8th query aims at e_b of one 32-key block (cycling over the blocks): its weight spreads evenly over that block's keys.
  ramp rows (cases with ramp > 0)   K = 0.05 N(0, 1) + linspace(0, ramp) u, q = N(0, 1) + 8 u: base-2 scores grow along the keys by about `ramp` units in all (Ref.smin / smax
      hold the float64 range).  6 stays inside the 8 x 32 kernel's sum check (2^13 per lane); 45 re-centres it again and again and is inside the 4 x 64 kernel's 2^96 headroom;
      110 and 150 leave that headroom (the repair pass) in the even heads; the odd heads aim 1.5 u at the same keys and stay inside it.
  pad   K rows and V^T columns between S_kv and the next multiple of 64 are part of the set: K pad rows are 4 k_t of addressed rows (unmasked they would dominate those rows),
      V^T pad columns hold +-64 (finite, as the header requires).
One key only (S_kv = 1) leaves nothing to address: its row is plain N(0, 1).
"""
import math
import zlib
from collections import namedtuple

import numpy as np

from oracle.dit_glue_fp64 import F64, bf16
from oracle.gemm_fp64 import SENT, SENT16, U23   # noqa: F401  (the sentinel of preallocated outputs is the GEMM oracle's)

LN2 = math.log(2.0)
LOG2E_F32 = np.float32(1.4426950408889634)
SCALE = 1.0 / math.sqrt(128.0)
BLOCK_DIR = 4.0                      # component of every key along its 32-key block's direction
NOISE = 0.05
KVB = 64

Ref = namedtuple("Ref", "out lo hi E A wt smin smax")      # out / lo / hi / E / A [H, S_q, 128]; wt [H, S_q] weight of the target key (NaN: no target)


def c_of(scale):
    """the factor of q . k in the base-2 exponent: the kernels' float32 product, 1 for pre-scaled Q"""
    return 1.0 if scale == 0 else F64(np.float32(scale) * LOG2E_F32)


def _bias(n, kb, period):
    t = np.arange(n) // KVB
    on = (t % period == 0) if period > 0 else (t == 0)
    return np.where(on, float(kb), 0.0)


def split_plan(H, Sq, S, ncu, tailsplit=True):
    """utx_attn_plan restated (attention_glds.hip, utx_attn_split_plan_impl): {workgroups, workgroups in full rounds, key ranges per tail workgroup, tiles per range}.
    tests/test_attention_ref_cpu.py pins it against the library's."""
    nqb = (Sq + 255) // 256
    nwg = nqb * H
    nfull = (nwg // ncu) * ncu
    r = nwg - nfull
    nt_all = (S + KVB - 1) // KVB
    best_ns, best = 1, 0.92
    if tailsplit and nfull > 0 and r > 0:
        for ns in range(2, 17):
            if r * ns > 2048 or (nt_all + ns - 1) // ns < 12:
                break
            cost = float((r * ns + ncu - 1) // ncu) * (1.0 / ns + 0.02)
            if cost < best:
                best, best_ns = cost, ns
    if best_ns == 1:
        return [nwg, nfull, 1, nt_all]
    tps = (nt_all + best_ns - 1) // best_ns
    return [nwg, nfull, (nt_all + tps - 1) // tps, tps]


def split_rows(case, plan):
    """bool [H, S_q]: the rows of the tail items (256-query work items nfull .. nwg - 1, item = head * nqb + query block) of a launch that splits"""
    H, Sq = case["H"], case["Sq"]
    rows = np.zeros((H, Sq), dtype=bool)
    if plan[2] > 1:
        nqb = (Sq + 255) // 256
        for w in range(plan[1], plan[0]):
            rows[w // nqb, (w % nqb) * 256: (w % nqb) * 256 + 256] = True
    return rows


def units(n, scaled=True):
    """(N_s, N_e, r) of the module docstring for n keys"""
    nt = (n + KVB - 1) // KVB
    return 128 + 4 + 4 * nt, 1 + 2 * nt, 2.0 ** -8 + U23 * ((n + 2 * nt) + (n + 2 * nt + 1) + 2)


def attention64(q, k, v, scale, kb=0.0, period=0, reverse=False):
    """one head in float64: q [S_q, 128], k / v [S_kv, 128] -> (ref, A, E_w + r A without the split term, W [S_q, S_kv], M [S_q], smin, smax)"""
    q, k, v = (np.asarray(a, dtype=F64) for a in (q, k, v))
    n = k.shape[0]
    c = c_of(scale)
    b = _bias(n, kb, period)
    if reverse:
        k, v, b = k[::-1], v[::-1], b[::-1]
    s = c * (q @ k.T) + b
    M = np.abs(s).max(-1)
    W = np.exp2(s - s.max(-1, keepdims=True))
    W /= W.sum(-1, keepdims=True)
    ref, A = W @ v, W @ np.abs(v)
    ns, ne, r = units(n)
    e = LN2 * ns * U23 * (abs(c) * (np.abs(q) @ np.abs(k).T) + abs(kb) + M[:, None]) + ne * 2 * U23
    We = W * e
    E = We @ np.abs(v) + np.abs(ref) * We.sum(-1, keepdims=True) + r * A
    return ref, A, E, W, M, float(s.min()), float(s.max())


def split_term(A, M, n, kb):
    L = M + math.log2(max(n, 2)) + abs(kb)
    return A * (2.0 ** -8 + 2 * (LN2 * 6 * U23 * L + 2 * U23) + 36 * U23)[..., None]


def reference(case, inp, scale, rows_split=None):
    """-> Ref over all heads.  rows_split: bool [H, S_q], the rows that the launch sends through the key-split tail round (split_rows)"""
    H, Sq, n = case["H"], case["Sq"], case["Sk"]
    out, lo, hi, Es, As = (np.empty((H, Sq, 128)) for _ in range(5))
    wt = np.full((H, Sq), np.nan)
    smin, smax = np.inf, -np.inf
    for h in range(H):
        ref, A, E, W, M, s0, s1 = attention64(inp["q"][h], inp["k"][h, :n], inp["v"][h, :n], scale, case["kb"], case["period"])
        if rows_split is not None and rows_split[h].any():
            E = E + np.where(rows_split[h][:, None], split_term(A, M, n, case["kb"]), 0.0)
        E = E * (1 + 2.0 ** -7)
        out[h], lo[h], hi[h], Es[h], As[h] = bf16(ref), bf16(ref - E), bf16(ref + E), E, A
        t = inp["tgt"][h]
        has = t >= 0
        wt[h, has] = W[np.nonzero(has)[0], t[has]]
        smin, smax = min(smin, s0), max(smax, s1)
    return Ref(out, lo, hi, Es, As, wt, smin, smax)


def accepted(got, ref):
    """bool [H, S_q, 128]: got inside the interval (a NaN is outside)"""
    got = np.asarray(got, dtype=F64)
    return (got >= ref.lo) & (got <= ref.hi)


def rel_width(ref):
    """(median, maximum) of E / |ref|"""
    x = ref.E / np.maximum(np.abs(ref.out), 1e-300)
    return float(np.median(x)), float(x.max())


def first_offender(got, ref, inp, what, plan=None):
    """None when every element is accepted, else a message naming the worst element (head, query, channel), its row's target key with tile / block / lane half / split range,
    got / lo / hi and the number of failing elements"""
    got = np.asarray(got, dtype=F64)
    ok = accepted(got, ref)
    if ok.all():
        return None
    with np.errstate(invalid="ignore"):
        miss = np.where(ok, 0.0, np.maximum(ref.lo - got, got - ref.hi) / np.maximum(ref.E, 1e-300))
    miss = np.where(np.isnan(miss) | (~ok & ~np.isfinite(got)), np.inf, miss)
    h, i, d = (int(x) for x in np.unravel_index(np.argmax(miss), miss.shape))
    t = int(inp["tgt"][h, i])
    where = "row kind %s" % inp["kind"][h, i]
    if t >= 0:
        where += ", target key %d = tile %d, block %d, 8-key group %d (lane half %d), key %d of it" % (t, t // 64, (t % 64) // 32, (t % 32) // 8, (t // 8) & 1, t % 8)
        if plan is not None and plan[2] > 1:
            where += ", split range %d of %d" % (t // (64 * plan[3]), plan[2])
    return ("%s: %d of %d elements outside the interval; worst (by E) at (head, query, channel) = (%d, %d, %d) [query block %d, wave slice %d, row %d of it; %s]: got %r, "
            "reference %r, accepted [%r, %r], E %.3g" % (what, int((~ok).sum()), ok.size, h, i, d, i // 256, (i % 256) // 32, i % 32, where, float(got[h, i, d]),
                                                          float(ref.out[h, i, d]), float(ref.lo[h, i, d]), float(ref.hi[h, i, d]), float(ref.E[h, i, d])))


# ------------------------------------------------------------------------------------------------ the cases of tests/test_attention_edges_gpu.py
def _case(name, kernel, H, Sq, Sk, kb=0.0, period=0, ramp=0.0, blk_rows=0, tailsplit=1, data=None):
    """data: the name that seeds the operands (two cases with the same data share them).  kernel: "g" the 8 x 32 kernel (UTX_ATTN_Q64=0), "blk" its block-strided instance, "q64" the 4 x 64 kernel, "split" a launch with a key-split tail round"""
    return dict(name=name, kernel=kernel, H=H, Sq=Sq, Sk=Sk, kb=kb, period=period, ramp=ramp, blk_rows=blk_rows, tailsplit=tailsplit, data=data or name)


# 8 x 32 kernel.  S_kv: 1; 40 and 63 (the first tile is the ragged one); 64; 65 (one key behind a whole tile); 127 / 129 / 192 around the two-tile ring; 520 a ragged tile
# behind the fast loop; 300 with more queries than keys; 1000.  S_q: 1, 33 / 63 / 64 / 65 around a wave and two, 100, 255 / 257 around a query block, 300, 520 (three blocks).
SHAPES_G = [(1, 1, 1), (2, 33, 40), (1, 63, 63), (3, 64, 64), (2, 65, 65), (1, 100, 127), (2, 255, 129), (1, 257, 192), (3, 300, 520), (2, 520, 300), (1, 40, 1000)]
CASES_G = [_case("g_h%d_q%d_k%d" % s, "g", *s) for s in SHAPES_G]
CASES_G_KB = [_case("g_kb3_h%d_q%d_k%d" % s, "g", *s, kb=3.0) for s in ((2, 65, 65), (3, 300, 520), (2, 520, 300))]
# periodic key multiplicity (FAST + KBP and the general loop): period 1 (every tile), 2, 3 (does not divide the 9 tiles of S_kv = 520, whose last is ragged), 5 (> the 4 tiles)
PERIODIC = [(1, 192), (2, 320), (3, 520), (5, 256)]
CASES_G_PER = [_case("g_per%d_k%d" % (p, n), "g", 2, 200, n, kb=3.0, period=p) for p, n in PERIODIC]
# ramp 6 is the existing growing-maximum test's; 45 is the one that makes the 8 x 32 kernel re-centre (6 base-2 units stay below its sum check)
CASES_G_RAMP = [_case("g_ramp6", "g", 2, 256, 1536, ramp=6.0), _case("g_ramp45", "g", 2, 256, 1536, ramp=45.0)]
CASES_BLK = [_case("blk%d_k%d_%s" % (b, n, "kb3" if kb else "plain"), "blk", 2, n, n, kb=kb, blk_rows=b) for b in (64, 128) for n in (256, 384) for kb in (0.0, 3.0)]
NSLOT = 3                            # ring depth of the 4 x 64 stream (AQ2_NSLOT of attention_q64_asm.inc; the CPU test reads the file and compares)
SHAPES_Q64 = [(1, 64, 64), (3, 128, 128), (2, 1, 192), (2, 100, 256), (1, 320, 320), (2, 448, 64 * (NSLOT + 1)), (2, 520, 256)]
CASES_Q64 = [_case("q64_h%d_q%d_k%d" % s, "q64", *s) for s in SHAPES_Q64]
CASES_Q64_KB = [_case("q64_kb3_h%d_q%d_k%d" % s, "q64", *s, kb=3.0) for s in ((3, 128, 128), (2, 520, 256))]
CASES_Q64_RAMP = [_case("q64_ramp%d" % r, "q64", 2, 200, 1024, ramp=float(r)) for r in (45, 110, 150)]


def short_last_range_sk(H, Sq, ncu):
    """the smallest S_kv (whole tiles) whose plan has at least three key ranges, the last of them with fewer tiles than the others"""
    for nt in range(24, 200):
        p = split_plan(H, Sq, 64 * nt, ncu)
        if p[2] >= 3 and nt % p[3]:
            return 64 * nt
    raise AssertionError("no such shape")


def split_cases(ncu):
    """the smallest launches with more workgroups than CUs: H = ncu / 2 + 1 heads of two query blocks -> two tail items (the last head).  At ncu = 256 (MI355X): H = 129,
    (129, 300, 1472) = 23 tiles in ranges of 12 + 11; (129, 300, 1500) a ragged tile in the last range; key_bias_period 4 (divides the 12 tiles of a range) and 5 (does not); (129, 300, 2176) = 34 tiles in ranges of 12 + 12 + 10."""
    H, Sq = ncu // 2 + 1, 300
    sk3 = short_last_range_sk(H, Sq, ncu)
    return [_case("split_k1472", "split", H, Sq, 1472), _case("split_k1500_ragged", "split", H, Sq, 1500), _case("split_k1472_per4", "split", H, Sq, 1472, kb=3.0, period=4),
            _case("split_k1472_per5", "split", H, Sq, 1472, kb=3.0, period=5),      # 12 tiles per range: a period that does not divide the range, so tb + t and t disagree
            _case("split_k1472_kb3", "split", H, Sq, 1472, kb=3.0), _case("split_k%d_short_last_range" % sk3, "split", H, Sq, sk3),
            _case("nosplit_k1472", "split", H, Sq, 1472, tailsplit=0, data="split_k1472"), _case("nosplit_k1500_ragged", "split", H, Sq, 1500, tailsplit=0, data="split_k1500_ragged")]


CASES = CASES_G + CASES_G_KB + CASES_G_PER + CASES_G_RAMP + CASES_BLK + CASES_Q64 + CASES_Q64_KB + CASES_Q64_RAMP


def _q16(x):
    """float -> nearest bf16 as float64, the quick way (for inputs; bf16() above is the exact one for results)"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((b + 0x7fff + ((b >> 16) & 1)) & np.uint32(0xffff0000)).view(np.float32).astype(F64)


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


def _targets(H, Sq, n, cb):
    """the map t [H, S_q] (-1: a block row) and the block of every block row [H, S_q] (-1: none)"""
    tgt, blk = np.full((H, Sq), -1, dtype=np.int64), np.full((H, Sq), -1, dtype=np.int64)
    nblk = (n + 31) // 32
    edges = []
    for t in range((n + 63) // 64):
        edges += [64 * t, min(64 * t + 63, n - 1)]
    edges += list(range(32 * cb, min(32 * cb + 32, n)))
    ce = ck = cblk = sl = 0
    for h in range(H):
        for s0 in range(0, Sq, 32):
            rows = [i for i in range(s0, min(s0 + 32, Sq))]
            want = [0, n - 1]
            for _ in range(8):
                want.append(edges[ce % len(edges)]); ce += 1
            addressed = [i for i in rows if i % 8 != 7]
            if len(addressed) == 1 and sl % 2:      # one-row slices take key 0 and key S_kv - 1 in turn
                want = want[1:]
            for j, i in enumerate(addressed):
                if j < len(want):
                    tgt[h, i] = want[j]
                else:
                    tgt[h, i] = ck % n; ck += 1
            for i in rows:
                if i % 8 == 7:
                    blk[h, i] = cblk % nblk; cblk += 1
            sl += 1
    return tgt, blk


def make_inputs(case, scale, seed=20262):
    """the operands of one case under one softmax_scale (0: Q pre-scaled): float64 arrays of bf16 values q [H, S_q, 128], k / v [H, S_pad, 128] (v is V, not V^T; rows >= S_kv
    are the pad region), and per row tgt (target key or -1), kind ('a' addressed, 'b' block, 'r' ramp, 'p' plain)"""
    rng = np.random.default_rng([seed, zlib.crc32(case["data"].encode())])
    H, Sq, n, kb, period = case["H"], case["Sq"], case["Sk"], case["kb"], case["period"]
    c = c_of(scale)
    npad = (n + 63) // 64 * 64
    nb32 = npad // 32
    sign = rng.choice([-1.0, 1.0], (H, 1, 128))
    v = sign * (0.25 + rng.random((H, npad, 128), dtype=np.float32) + np.repeat(rng.integers(0, 2, (H, nb32, 128)).astype(np.float32), 32, axis=1))
    v[:, n:] = 64.0 * rng.choice([-1.0, 1.0], (H, npad - n, 128))
    v = _q16(v)
    tgt = np.full((H, Sq), -1, dtype=np.int64)
    kind = np.full((H, Sq), "p")
    k = np.zeros((H, npad, 128))
    if case["ramp"] > 0:
        u = _unit(rng.normal(size=(H, 1, 128)))
        k[:, :n] = 0.05 * rng.normal(size=(H, n, 128)) + np.linspace(0.0, case["ramp"], n)[None, :, None] * u
        # ramps that leave the 4 x 64 kernel's headroom do so in the even heads only (odd heads: 1.5 u, at most about 5 x 0.1275 x ramp < 96 units): repaired and untouched blocks side by side
        coef = np.where((np.arange(H) % 2 == 1) & (case["ramp"] >= 100), 1.5, 8.0)[:, None, None]
        q = (rng.normal(size=(H, Sq, 128)) + coef * u) * (SCALE * float(LOG2E_F32) if scale == 0 else 1.0)
        kind[:] = "r"
        k[:, n:] = 4.0 * k[:, n - 1: n]
        return dict(q=_q16(q), k=_q16(k), v=v, tgt=tgt, kind=kind)
    e = _unit(rng.normal(size=(H, nb32, 128)))
    eb = np.repeat(e, 32, axis=1)[:, :n]
    g0 = rng.standard_normal((H, n, 128), dtype=np.float32).astype(F64)
    k[:, :n] = _q16(g0 + (BLOCK_DIR - (g0 * eb).sum(-1, keepdims=True)) * eb)
    q = rng.standard_normal((H, Sq, 128), dtype=np.float32).astype(F64) * (SCALE * float(LOG2E_F32) if scale == 0 else 1.0)
    if n > 1:
        nfull = n // 32
        cb = min(max(nfull - 1, 0), ((n + 31) // 32) // 2)
        tgt, blk = _targets(H, Sq, n, cb)
        bias = _bias(n, kb, period)
        s_in = (math.log2(n) + 3.0) / (c * BLOCK_DIR)
        for h in range(H):
            a = np.nonzero(tgt[h] >= 0)[0]
            t = tgt[h, a]
            base = k[h, t] + NOISE * rng.normal(size=(len(a), 128))
            beta = (c * (base @ k[h, :n].T)).astype(np.float32)                 # score per unit of g (float32 is plenty for the solve; reference() judges the result)
            ar = np.arange(len(a))
            bt = beta[ar, t].copy()
            g = ((math.log2(n) + 1.0) / bt).astype(np.float32)
            b32 = bias.astype(np.float32)
            for _ in range(4):                                                  # Newton on the log-odds of the target key, in base 2
                s = g[:, None] * beta + b32
                st = s[ar, t].copy()
                s[ar, t] = -np.inf
                mx = s.max(-1, keepdims=True)
                w = np.exp2(s - mx)
                z = w.sum(-1)
                f = st - (mx[:, 0] + np.log2(z))
                df = bt - (w * beta).sum(-1) / z
                g = np.clip(g - f / df, 0.25 * g, 4.0 * g)
            g = g.astype(F64)
            q[h, a] = g[:, None] * base
            kind[h, a] = "a"
            b = np.nonzero(blk[h] >= 0)[0]
            q[h, b] = s_in * e[h, blk[h, b]]
            kind[h, b] = "b"
        for h in range(H):
            for p in range(n, npad):
                t = tgt[h, (p - n) % Sq]
                k[h, p] = 4.0 * k[h, t if t >= 0 else n - 1]
    else:
        k[:, n:] = 4.0 * _q16(q[:, :1] / np.abs(q[:, :1]).max())
    return dict(q=_q16(q), k=_q16(k), v=v, tgt=tgt, kind=kind)


def coverage(inp, n):
    """share of the keys 0 .. n - 1 that some addressed row aims at"""
    t = inp["tgt"][inp["tgt"] >= 0]
    return len(np.unique(t)) / float(n)


# ------------------------------------------------------------------------------------------------ float32 emulation of the kernels, with defects
DEFECTS = ("ragged_mask_one_group_short",      # (a) lim = Sk - 64 t without the 8 lh term
           "pad_keys_unmasked",                # (b)
           "key_bias_on_tile_1",               # (c) instead of tile 0
           "periodic_bias_on_local_tile",      # (d) t % period instead of (tb + t) % period inside a key split
           "p_groups_swapped",                 # (e) 8-key groups 1 and 2 of every 32-key block swapped in P, not in V
           "no_o_rescale",                     # (f) O not multiplied by alpha on a re-centre
           "merge_drops_last_range",           # (g)
           "merge_weights_base_e",             # (h) e^(lse - M) instead of 2^(lse - M)
           "wave_rows_32_off",                 # (i) wave 1 of a workgroup writes its 32 rows 32 rows further down
           "drop_last_full_tile")              # (j) the last tile is dropped when S_kv is a multiple of 64


def _rb(x):
    """float32 -> float32 holding the nearest bf16 (ties to even)"""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((b + 0x7fff + ((b >> 16) & 1)) & np.uint32(0xffff0000)).view(np.float32)


def _core(q, K, V, Sk, tb, c2, presc, kb, period, defect):
    """the 8 x 32 kernel's loop over the Sk keys of K / V (padded to whole tiles; tile 0 of them is tile tb of the sequence) for q [B, R, 128], R a multiple of 32 (waves)
    -> (O unnormalised, l, m) in float32.  The sum check is on the row sum of a 32-key block (the kernel checks each lane half's 16 keys: it re-centres no earlier)."""
    f = np.float32
    B, R, _ = q.shape
    nt = (Sk + KVB - 1) // KVB
    if defect == "drop_last_full_tile" and Sk % KVB == 0:
        nt -= 1
    m, l, O = np.zeros((B, R), f), np.zeros((B, R), f), np.zeros((B, R, 128), f)
    kbv = f(kb) if presc else f(f(kb) / c2)
    ex = (lambda x: np.exp2(x)) if presc else (lambda x: np.exp2(x * c2))
    with np.errstate(over="ignore", invalid="ignore"):
        for t in range(nt):
            ragged = t == nt - 1 and Sk % KVB != 0
            tg = tb + t
            if period > 0:
                kbias = (t if defect == "periodic_bias_on_local_tile" else tg) % period == 0
            else:
                kbias = tg == (1 if defect == "key_bias_on_tile_1" else 0)
            kbias = kbias and kb != 0
            for b in (0, 1):
                j = t * KVB + 32 * b + np.arange(32)
                valid = (j - (8 * ((j // 8) & 1) if defect == "ragged_mask_one_group_short" else 0)) < Sk
                if defect == "pad_keys_unmasked":
                    valid[:] = True
                first = t == 0 and b == 0
                sa = np.matmul(q, K[:, j].transpose(0, 2, 1)) - m[..., None]
                if kbias:
                    sa = sa + kbv
                P = ex(sa)
                ps = P.sum(-1)
                slow = np.ones((B, R), bool) if first or ragged else np.repeat((~(ps <= 8192.0)).reshape(B, R // 32, 32).any(-1), 32, axis=1)
                if slow.any():
                    sam = np.where(valid[None, None, :], sa, f(-np.inf)) if ragged else sa
                    mx = sam.max(-1)
                    d = mx if first else np.maximum(mx, f(0))
                    alpha = np.ones_like(d) if first else (np.exp2(-d) if presc else np.exp2(-d * c2))
                    d, alpha = np.where(slow, d, f(0)), np.where(slow, alpha, f(1))
                    m, l = m + d, l * alpha
                    if defect != "no_o_rescale":
                        O = O * alpha[..., None]
                    P = ex(sam - d[..., None])
                    ps = P.sum(-1)
                l = l + ps
                Pb = _rb(P)
                if defect == "p_groups_swapped":
                    Pb = np.concatenate([Pb[..., :8], Pb[..., 16:24], Pb[..., 8:16], Pb[..., 24:]], -1)
                O = O + np.matmul(Pb, V[:, j])
    return O, l, m


def emulate(case, inp, scale, plan=None, defect=None):
    """what the kernels compute, in numpy float32: 64-key tiles in two 32-key blocks, online softmax with a deferred maximum, fp32 l from the unrounded probabilities, bf16 P,
    fp32 PV; the work items nfull .. nwg - 1 of `plan` (utx_attn_plan's output) through the key split with bf16 partial rows and the log-sum-exp merge.
    defect: one of DEFECTS, the mistake of that name.  -> [H, S_q, 128] float64 of bf16 values (SENT where nothing was written)"""
    assert defect is None or defect in DEFECTS
    f = np.float32
    H, Sq, n, kb, period = case["H"], case["Sq"], case["Sk"], case["kb"], case["period"]
    presc = scale == 0
    c2 = f(1) if presc else np.float32(scale) * LOG2E_F32
    R = (Sq + 31) // 32 * 32
    q = inp["q"].astype(f)
    q = np.concatenate([q, np.repeat(q[:, -1:], R - Sq, axis=1)], 1)           # rows past S_q repeat the last query (the kernels clamp the row index)
    K, V = inp["k"].astype(f), inp["v"].astype(f)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        O, l, _ = _core(q, K, V, n, 0, c2, presc, kb, period, defect)
        out = _rb(O * (f(1) / l)[..., None])[:, :Sq].astype(F64)
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
                    Os, ls, ms = _core(q[h: h + 1, r0:r1], K[h: h + 1, k0:k1], V[h: h + 1, k0:k1], sk, s * tps, c2, presc, kb, period, defect)
                    parts.append((_rb(Os[0] * (f(1) / ls[0])[:, None]), (ms[0] if presc else ms[0] * c2) + np.log2(ls[0])))
                if defect == "merge_drops_last_range":
                    parts = parts[:-1]
                M = np.max([p[1] for p in parts], 0)
                acc, Wt = np.zeros((r1 - r0, 128), f), np.zeros(r1 - r0, f)
                for On, lse in parts:
                    wgt = np.exp(lse - M) if defect == "merge_weights_base_e" else np.exp2(lse - M)
                    Wt = Wt + wgt
                    acc = acc + wgt[:, None] * On
                out[h, r0: min(r1, Sq)] = _rb(acc * (f(1) / Wt)[:, None])[: min(r1, Sq) - r0].astype(F64)
    if defect == "wave_rows_32_off":
        moved = out[:, 32:64].copy()
        out[:, 32:64] = SENT
        out[:, 64:96] = moved[:, : max(0, min(96, Sq) - 64)]
    return out

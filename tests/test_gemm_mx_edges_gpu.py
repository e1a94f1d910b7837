"""The two MX fp8 GEMM kernels (gemm_bf16_kernel<128,128,2,2,false,true>, utx_gemm_desc.mx8 = 1; gemm256_w4_kernel<GATED, false, true> + gemm_w4_fixup_kernel, mx8 = 2,
with its fp8 output q_out) against the float64 reference oracle/gemm_mx_fp64.py at their tile and scale edges: every output element inside the COUNTED interval
e = (K + K2 + 4) 2^-23 (|alpha| sum|a b| + |bias|) of oracle/gemm_fp64.py around the float64 value of the dequantised operands, pushed through the epilogue's bf16 roundings
(no number from a GPU went into it; tests/test_gemm_mx_ref_cpu.py shows on the CPU that at most 3.06 % of the intervals hold more than one bf16 value, that every 32-block's
scale carries a full share of every sum, and that eleven kernel mistakes fall outside the checks made here).

Operands are quantised on the host by the oracle (the device quantisers have their own tests) and uploaded as bytes.  Every buffer is larger than its matrix: A has rows up to
the next multiple of 256 holding 0x7F (e4m3 NaN), scale buffers hold 0xFF (E8M0 NaN) wherever the quantiser writes nothing -- padding columns of a row-major row, rows >= M
of the last packed row block, one spare row block and one spare K-tile slab -- and none of it may reach a written output.  Outputs are preallocated with a sentinel, two rows
and (where the case says so) some columns larger than the contract writes.  Every option a test sets is put back in a `finally`."""
import numpy as np
import pytest
import torch

from oracle import gemm_fp64 as G
from oracle import gemm_mx_fp64 as X
from tests.support.gemm_gpu import _bits, _options, _sent

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
_CACHE = {}


def _ops():
    from unitex_amd.flux import ops
    return ops


def _case_data(case):
    """(inputs, reference): built once per case, shared by every launch of it, never modified"""
    if case["name"] not in _CACHE:
        inp = X.make_inputs(case)
        _CACHE[case["name"]] = (inp, X.reference(case, inp))
    return _CACHE[case["name"]]


def _bf(a, pad=0, fill=3.0e38):
    t = torch.from_numpy(np.asarray(a, dtype=np.float32)).to(BF)
    if t.dim() == 1 or not pad:
        return t.cuda()
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=BF)
    buf[:, : t.shape[1]] = t
    return buf.cuda()[:, : t.shape[1]]


def _bytes(a, pad_cols, fill, rows=None):
    """uint8 [R, C] -> the [R, C] view of a CUDA uint8 buffer of `rows` (default: R rounded up to 256) x (C + pad_cols) bytes holding `fill` everywhere else"""
    a = np.asarray(a, dtype=np.uint8)
    R, C = a.shape
    buf = torch.full(((R + 255) // 256 * 256 if rows is None else rows, C + pad_cols), fill, dtype=torch.uint8)
    buf[:R, :C] = torch.from_numpy(a)
    return buf.cuda()[:R, :C]


def _packed(s, rows=None):
    """row-major scale bytes -> PackedScales on the GPU with one spare row block and one spare K-tile slab, 0xFF wherever the quantiser writes nothing"""
    from unitex_amd.flux import mx8
    R, KB = s.shape
    data = X.pack_scales(s, row_blocks=(R + 127) // 128 + 1, slabs=KB // 4 + 1, fill=X.S_SENT)
    return mx8.PackedScales(torch.from_numpy(data).cuda(), R, KB * 32)


def _operands(case, inp, mx8):
    """(A bytes, B bytes, a_scale, b_scale) of one launch in the scale layout of kernel mx8"""
    K = case["K"]
    aq = _bytes(inp["Aq"], case["pad_a"], X.A_POISON)
    bq = _bytes(inp["Bq"], 0, X.A_POISON, rows=case["N"])
    if mx8 == 1:
        return aq, bq, _bytes(inp["As"], case["pad_sa"], X.S_SENT), _bytes(inp["Bs"], case["pad_sb"], X.S_SENT, rows=case["N"])
    if case["b_slice"]:
        r0, r1, rows = case["b_slice"]
        full = np.full((rows, K // 32), X.S_SENT, dtype=np.uint8)
        full[r0:r1] = inp["Bs"]
        b_s = _packed(full).row_slice(r0, r1)
    else:
        b_s = _packed(inp["Bs"])
    return aq, bq, _packed(inp["As"]), b_s


def _plan(case, mx8, sk=False):
    return _ops().gemm_plan(case["M"], case["N"], K=case["K"], K2=case["K2"], n_split=case["n_split"], gelu_from=case["gelu_from"], lora_seg_n=case["lora_seg_n"],
                            lora_n_limit=case["lora_n_limit"], sk=sk, mx8=mx8)


def _launch(case, inp, mx8=None, sk_work=None, q_out=None):
    """one utx_gemm_bf16 on MX operands through ops.gemm -> (C buffer, C1 buffer or None) on the CPU, each two rows and pad_c / pad_c1 columns larger than what is written"""
    ops = _ops()
    mx8 = case["mx8"] if mx8 is None else mx8
    M, N = case["M"], case["N"]
    nc = N if case["n_split"] is None else case["n_split"]
    cbuf = _sent(M + 2, nc + case["pad_c"])
    c1buf = None if nc == N else _sent(M + 2, N - nc + case["pad_c1"])
    kw = dict(alpha=case["alpha"], gelu_from=case["gelu_from"], n_split=case["n_split"])
    if case["gate"] == "inplace":
        cbuf[:M, :N] = torch.from_numpy(inp["res"].astype(np.float32)).to(BF)
    cbuf = cbuf.cuda()
    if case["gate"]:
        kw.update(gate=_bf(inp["gate"]), res=cbuf[:M, :N] if case["gate"] == "inplace" else _bf(inp["res"], case["pad_res"]))
    if case["K2"]:
        kw.update(A2=_bf(inp["A2"]), B2=_bf(inp["B2"]), lora_seg_n=case["lora_seg_n"], lora_n_limit=case["lora_n_limit"])
    if c1buf is not None:
        c1buf = c1buf.cuda()
        kw.update(C1=c1buf[:M, : N - nc])
    aq, bq, a_s, b_s = _operands(case, inp, mx8)
    ops.gemm(aq, bq, bias=None if inp["bias"] is None else _bf(inp["bias"]), out=cbuf[:M, :nc], a_scale=a_s, b_scale=b_s, sk_work=sk_work, q_out=q_out, **kw)
    torch.cuda.synchronize()
    return cbuf.cpu(), (None if c1buf is None else c1buf.cpu())


def _got(case, bufs):
    M, N = case["M"], case["N"]
    nc = N if case["n_split"] is None else case["n_split"]
    parts = [bufs[0][:M, :nc]] + ([] if bufs[1] is None else [bufs[1][:M, : N - nc]])
    return torch.cat(parts, 1).double().numpy()


def _check(case, bufs, ref, what, c1_untouched=False):
    """sentinel gone inside M x N and intact outside, every element inside its interval (tests/test_gemm_edges_gpu._check); c1_untouched: C1 keeps its sentinel everywhere
    and only the columns of C are compared"""
    M, N = case["M"], case["N"]
    nc = N if case["n_split"] is None else case["n_split"]
    for name, buf, w in (("C", bufs[0], nc), ("C1", bufs[1], N - nc)):
        if buf is None:
            continue
        raw = _bits(buf)
        inside = np.zeros(raw.shape, dtype=bool)
        if not (c1_untouched and name == "C1"):
            inside[:M, :w] = True
        wrong = np.argwhere(~inside & (raw != G.SENT16))
        assert wrong.size == 0, "%s: %s written outside its region at %d places, first (row, column) = %s of a %s buffer" % (what, name, len(wrong), tuple(wrong[0]), raw.shape)
        left = np.argwhere(inside & (raw == G.SENT16))
        assert left.size == 0, "%s: %d elements of %s never written, first (m, n) = %s" % (what, len(left), name, tuple(left[0]))
    if c1_untouched:
        msg = G.first_offender(bufs[0][:M, :nc].double().numpy(), G.Ref(*(x[:, :nc] for x in ref)), what)
    else:
        msg = G.first_offender(_got(case, bufs), ref, what)
    assert msg is None, msg


def _same_bits(a, b, what):
    for x, y in zip(a, b):
        if x is not None:
            d = np.argwhere(_bits(x) != _bits(y))
            assert d.size == 0, "%s: %d elements differ in bits, first (m, n) = %s" % (what, len(d), tuple(d[0]))


# ------------------------------------------------------------------------------------------------ the scale layout
def test_pack_scales_is_the_layout_of_packed_scales_and_of_the_device_quantiser():
    from unitex_amd.flux import mx8
    ops = _ops()
    rng = np.random.default_rng(11)
    for R, K in ((1, 128), (129, 384), (300, 640)):
        s = rng.integers(0, 255, (R, K // 32)).astype(np.uint8)
        assert (_packed(s).rowmajor().cpu().numpy() == s).all(), "pack_scales against PackedScales.rowmajor, %d x %d" % (R, K)
        x = torch.from_numpy((rng.normal(0, 1, (R, K)) * np.exp2(rng.integers(-20, 20, (R, K // 32)).repeat(32, 1))).astype(np.float32)).to(BF)
        q_ref, s_ref = X.quantize(x.float().numpy())
        q, sp = mx8.quantize_act(x.cuda(), ops.get_ctx(0), packed=True)
        torch.cuda.synchronize()
        assert (q.cpu().numpy() == q_ref).all()
        assert (sp.data.cpu().numpy() == X.pack_scales(s_ref, fill=0)).all(), "utx_quant_mx8_packed against pack_scales (rows >= M not written), %d x %d" % (R, K)
        assert (X.unpack_scales(sp.data.cpu().numpy(), R, K) == s_ref).all()


# ------------------------------------------------------------------------------------------------ mx8 = 1
@pytest.mark.parametrize("case", X.CASES_MX1, ids=lambda c: c["name"])
def test_mx1_tile128_edges(case):
    inp, ref = _case_data(case)
    with _options():
        assert _plan(case, 1)["kernel"] == "128x128"
        bufs = _launch(case, inp)
    _check(case, bufs, ref, case["name"])


# ------------------------------------------------------------------------------------------------ mx8 = 2
@pytest.mark.parametrize("case", X.CASES_MX2, ids=lambda c: c["name"])
def test_mx2_w4_edges(case):
    inp, ref = _case_data(case)
    with _options(PERS_GRID=case["pers_grid"]):
        p = _plan(case, 2)
        assert (p["kernel"], p["tiles"], p["tail_tiles"]) == ("w4", (case["M"] + 255) // 256 * (case["N"] // 256), 0), p
        bufs = _launch(case, inp)
        again = _launch(case, inp) if case["name"] == "mx2_m600_gated_grid3" else None
    _check(case, bufs, ref, case["name"])
    if again is not None:
        _same_bits(bufs, again, case["name"] + ": a second launch")


@pytest.mark.parametrize("case", X.CASES_MXSPLIT, ids=lambda c: c["name"])
def test_mx2_split_tail(case):
    """six tiles on a grid of four: tiles 0..3 are the whole round (tile rows 0 and 1), tiles 4 and 5 (rows 512..599) are cut into S ranges of whole K-tiles of 128 fp8
    elements and finished by the fix-up kernel"""
    ops = _ops()
    inp, ref = _case_data(case)
    S = case["streamk"]
    ws = ops.streamk_workspace("cuda:0")
    with _options(PERS_GRID=4, STREAMK=1000 + S):
        p = _plan(case, 2, sk=True)
        assert (p["kernel"], p["tiles"], p["tail_tiles"], p["ranges"]) == ("w4", 6, 2, S), p
        a = _launch(case, inp, sk_work=ws)
        b = _launch(case, inp, sk_work=ws)
    with _options(PERS_GRID=4, STREAMK=0):
        assert _plan(case, 2, sk=True)["tail_tiles"] == 0
        whole = _launch(case, inp, sk_work=ws)
    _check(case, a, ref, "%s split" % case["name"])
    _check(case, whole, ref, "%s STREAMK=0" % case["name"])
    _same_bits(a, b, case["name"] + ": two split launches")
    _same_bits([a[0][:512]], [whole[0][:512]], case["name"] + ": the whole round's four tiles against the unsplit launch")


def test_both_mx_kernels_give_the_same_bits():
    """both kernels accumulate every output element over ascending K with the same instruction: 300 x 512 x 384 with GELU + split, split tail off"""
    case = X.CASE_BOTH
    inp, ref = _case_data(case)
    with _options(STREAMK=0):
        tiled, w4 = _launch(case, inp, mx8=1), _launch(case, inp, mx8=2)
    _check(case, tiled, ref, case["name"] + " mx8 = 1")
    _check(case, w4, ref, case["name"] + " mx8 = 2")
    _same_bits(tiled, w4, case["name"] + ": mx8 = 1 against mx8 = 2")


# ------------------------------------------------------------------------------------------------ fp8 output of the GELU columns
def _qout_buffers(M, W):
    """(q bytes [rows up to the next multiple of 256, + 2][W + 64], packed scales [QOUT_SLABS + 1][ceil(M / 128) + 1][512]) preset with their sentinels, on the GPU"""
    q = torch.full(((M + 255) // 256 * 256 + 2, W + 64), X.Q_SENT, dtype=torch.uint8).cuda()
    qs = torch.full((X.QOUT_SLABS + 1, (M + 127) // 128 + 1, 512), X.S_SENT, dtype=torch.uint8).cuda()
    return q, qs


@pytest.mark.parametrize("name,grid,kt0", [("mxq_m300", 0, 0), ("mxq_m300", 0, 1), ("mxq_m129", 1, 1), ("mxq_m600", 1, 0), ("mxq_m600", 2, 1)])
def test_mx2_q_out(name, grid, kt0):
    """q_out: columns < gelu_from of C inside the interval, C1 untouched, bytes and scales accepted by qout_accept, sentinels intact in rows >= M, padding columns, the spare
    row block and the other K-tile slabs; and the bits of the same launch without q_out followed by utx_quant_mx8_packed"""
    from unitex_amd.flux import mx8
    ops = _ops()
    case = next(c for c in X.CASES_QOUT if c["name"] == name)
    inp, ref = _case_data(case)
    M, gf = case["M"], case["gelu_from"]
    W = case["N"] - gf
    what = "%s PERS_GRID=%d q_out_kt0=%d" % (name, grid, kt0)
    q, qs = _qout_buffers(M, W)
    with _options(PERS_GRID=grid):
        assert _plan(case, 2)["kernel"] == "w4"
        bufs = _launch(case, inp, q_out=(q[:M, :W], qs, kt0))
        plain = _launch(case, inp)
        q2, qs2 = _qout_buffers(M, W)
        c1 = plain[1].cuda()
        mx8.quantize_act(c1[:M, :W], ops.get_ctx(0), out=(q2[:M, :W], mx8.PackedScales(qs2[kt0:], M, W)))
        torch.cuda.synchronize()
    _check(case, bufs, ref, what, c1_untouched=True)
    _check(case, plain, ref, what + " (without q_out)")
    rb = qs.shape[1]
    s_all = X.unpack_scales(qs.cpu().numpy(), rb * 128, 128 * qs.shape[0])
    msg = X.qout_check(q.cpu().numpy(), s_all, M, W, kt0, X.gelu_part(ref, gf), what)
    assert msg is None, msg
    assert torch.equal(q.cpu(), q2.cpu()), what + ": q_out bytes differ from the bf16 epilogue followed by utx_quant_mx8_packed"
    assert torch.equal(qs.cpu(), qs2.cpu()), what + ": packed q_out scales differ from the bf16 epilogue followed by utx_quant_mx8_packed"


def test_q_out_refusals_leave_every_output_untouched():
    """q_out with row-major scales (mx8 = 1), with a gate, with gelu_from off a 128 multiple, with too few scale row blocks: -2 each, nothing launched"""
    ops = _ops()
    case = X.CASES_QOUT[0]
    inp, _ = _case_data(case)
    M, N, gf = case["M"], case["N"], case["gelu_from"]
    aq1, bq1, as1, bs1 = _operands(case, inp, 1)
    aq, bq, a_s, b_s = _operands(case, inp, 2)
    gate, res = _bf(np.ones(N)), _bf(np.zeros((M, N)))

    def attempt(what, A, B, sa, sb, qs_rb=None, **kw):
        q, qs = _qout_buffers(M, N - gf)
        if qs_rb is not None:
            qs = torch.full((X.QOUT_SLABS + 1, qs_rb, 512), X.S_SENT, dtype=torch.uint8).cuda()
        c, c1 = _sent(M, N).cuda(), _sent(M, N - gf).cuda()
        kw = dict(dict(out=c[:, :gf], gelu_from=gf, n_split=gf, C1=c1), **kw)
        with pytest.raises(RuntimeError, match=r"utx_gemm_bf16 failed \(code -2"):
            ops.gemm(A, B, bias=_bf(inp["bias"]), a_scale=sa, b_scale=sb, q_out=(q[:M, : N - gf], qs, 0), **kw)
        torch.cuda.synchronize()
        assert (_bits(c.cpu()) == G.SENT16).all() and (_bits(c1.cpu()) == G.SENT16).all(), what + ": a refused launch wrote to C / C1"
        assert bool((q == X.Q_SENT).all()) and bool((qs == X.S_SENT).all()), what + ": a refused launch wrote to q_out / qs_out"

    with _options():
        attempt("mx8 = 1", aq1, bq1, as1, bs1)
        attempt("gate", aq, bq, a_s, b_s, gate=gate, res=res)
        attempt("gelu_from % 128", aq, bq, a_s, b_s, gelu_from=gf + 64)
        attempt("qs_out_rb too small", aq, bq, a_s, b_s, qs_rb=(M + 127) // 128 - 1)

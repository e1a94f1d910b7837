"""The two bf16 GEMM kernels (gemm_bf16_kernel<128,128> in gemm.hip; gemm256_w4_kernel + gemm_w4_fixup_kernel in gemm_w4.hip) against the float64 reference
oracle/gemm_fp64.py at their launch-geometry edges, every output element inside a COUNTED interval (see that module: e = (K + K2 + 4) 2^-23 (|alpha| sum|a b| + |bias|)
around the float64 value, pushed through the epilogue's bf16 roundings; no number from a GPU went into it, and tests/test_gemm_ref_cpu.py shows on the CPU that
at most 1.41 % of the intervals hold more than one bf16 value and that eight kernel mistakes fall outside them).

Cases, operands and references come from the oracle module (one copy, shared with the CPU test).  The one-wave-per-SIMD kernel is reached with a handful of
tiles through UTX_GEMM_TILE=2564 / UTX_GEMM_PERS_GRID / UTX_GEMM_STREAMK=1000+S; every option a test sets is put back in a `finally`.  Outputs are preallocated
with a sentinel, two rows and (where the case says so) some columns larger than the contract writes: the sentinel must be gone inside M x N and intact outside."""
import numpy as np
import pytest
import torch

from oracle import dit_ref
from oracle import gemm_fp64 as G
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
        inp = G.make_inputs(case)
        _CACHE[case["name"]] = (inp, G.reference(case, inp))
    return _CACHE[case["name"]]


def _bf(a, pad=0, fill=3.0e38):
    """numpy [R, C] of bf16 values -> the [R, C] view of a CUDA bf16 tensor whose rows are `pad` elements longer (the padding holds a value that would wreck a sum)"""
    t = torch.from_numpy(np.asarray(a, dtype=np.float32)).to(BF)
    if t.dim() == 1 or not pad:
        return t.cuda()
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=BF)
    buf[:, : t.shape[1]] = t
    return buf.cuda()[:, : t.shape[1]]


def _plan(case, sk=False):
    return _ops().gemm_plan(case["M"], case["N"], K=case["K"], K2=case["K2"], n_split=case["n_split"], gelu_from=case["gelu_from"],
                            lora_seg_n=case["lora_seg_n"], lora_n_limit=case["lora_n_limit"], sk=sk)


def _launch(case, inp, sk_work=None):
    """one utx_gemm_bf16 through ops.gemm -> (C buffer, C1 buffer or None) on the CPU, each two rows and pad_c / pad_c1 columns larger than what is written"""
    ops = _ops()
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
    ops.gemm(_bf(inp["A"], case["pad_a"]), _bf(inp["B"]), bias=None if inp["bias"] is None else _bf(inp["bias"]), out=cbuf[:M, :nc], sk_work=sk_work, **kw)
    torch.cuda.synchronize()
    return cbuf.cpu(), (None if c1buf is None else c1buf.cpu())


def _got(case, bufs):
    """the [M, N] output as float64, columns >= n_split from C1"""
    M, N = case["M"], case["N"]
    nc = N if case["n_split"] is None else case["n_split"]
    parts = [bufs[0][:M, :nc]] + ([] if bufs[1] is None else [bufs[1][:M, : N - nc]])
    return torch.cat(parts, 1).double().numpy()


def _check(case, bufs, ref, what):
    M, N = case["M"], case["N"]
    nc = N if case["n_split"] is None else case["n_split"]
    for name, buf, w in (("C", bufs[0], nc), ("C1", bufs[1], N - nc)):
        if buf is None:
            continue
        raw = _bits(buf)
        inside = np.zeros(raw.shape, dtype=bool)
        inside[:M, :w] = True
        wrong = np.argwhere(~inside & (raw != G.SENT16))
        assert wrong.size == 0, "%s: %s written outside its %d x %d region at %d places, first (row, column) = %s of a %s buffer" % (
            what, name, M, w, len(wrong), tuple(wrong[0]), raw.shape)
        left = np.argwhere(inside & (raw == G.SENT16))
        assert left.size == 0, "%s: %d elements of %s never written, first (m, n) = %s" % (what, len(left), name, tuple(left[0]))
    msg = G.first_offender(_got(case, bufs), ref, what)
    assert msg is None, msg


def _same_bits(a, b, what):
    for x, y in zip(a, b):
        if x is not None:
            d = np.argwhere(_bits(x) != _bits(y))
            assert d.size == 0, "%s: %d elements differ in bits, first (m, n) = %s" % (what, len(d), tuple(d[0]))


# ------------------------------------------------------------------------------------------------ 128 x 128 kernel
@pytest.mark.parametrize("case", G.CASES_128, ids=lambda c: c["name"])
def test_tile128_edges(case):
    inp, ref = _case_data(case)
    with _options(TILE=128, GROUP_M=case["group_m"]):
        assert _plan(case)["kernel"] == "128x128"
        bufs = _launch(case, inp)
    _check(case, bufs, ref, case["name"])


# ------------------------------------------------------------------------------------------------ one-wave-per-SIMD kernel
@pytest.mark.parametrize("case", G.CASES_W4, ids=lambda c: c["name"])
def test_w4_edges_under_both_k_loops(case):
    """every case under the generated K loop (UTX_GEMM_FASTK=1) and the plain one (0): the same bits, inside the interval"""
    inp, ref = _case_data(case)
    outs = {}
    for fastk in (1, 0):
        with _options(TILE=2564, FASTK=fastk, PERS_GRID=case["pers_grid"]):
            assert _plan(case)["kernel"] == "w4"
            outs[fastk] = _launch(case, inp)
            if fastk == 1 and case["name"] == "w4_m600_lora_grid3":
                _same_bits(outs[1], _launch(case, inp), case["name"] + ": a second launch")
        _check(case, outs[fastk], ref, "%s FASTK=%d" % (case["name"], fastk))
    _same_bits(outs[1], outs[0], case["name"] + ": FASTK=1 against FASTK=0")


@pytest.mark.parametrize("case", G.CASES_SPLIT, ids=lambda c: c["name"])
def test_w4_split_tail(case):
    """six tiles on a grid of four: tiles 0..3 are the whole round (tile rows 0 and 1 -- the default GROUP_M of a narrow output is 2, so the first group of the tile order
    is two tile rows x two tile columns), tiles 4 and 5 (rows 512..599) are cut into S ranges and finished by the fix-up kernel"""
    ops = _ops()
    inp, ref = _case_data(case)
    S = case["streamk"]
    ws = ops.streamk_workspace("cuda:0")
    with _options(TILE=2564, PERS_GRID=4, STREAMK=1000 + S):
        p = _plan(case, sk=True)
        assert (p["kernel"], p["tiles"], p["tail_tiles"], p["ranges"]) == ("w4", 6, 2, S), p
        a = _launch(case, inp, sk_work=ws)
        b = _launch(case, inp, sk_work=ws)
    with _options(TILE=2564, PERS_GRID=4, STREAMK=0):
        assert _plan(case, sk=True)["tail_tiles"] == 0
        whole = _launch(case, inp, sk_work=ws)
    _check(case, a, ref, "%s split" % case["name"])
    _check(case, whole, ref, "%s STREAMK=0" % case["name"])
    _same_bits(a, b, case["name"] + ": two split launches")
    _same_bits([a[0][:512]], [whole[0][:512]], case["name"] + ": the whole round's four tiles against the unsplit launch")


# ------------------------------------------------------------------------------------------------ fused q / k epilogue at a small shape
def test_w4_fused_qk_post_small():
    """utx_gemm_desc.qk_cols at M = 300 (a ragged second tile row), tok_off = 64, N = 768 with 512 q / k columns: bit-identical to GEMM -> utx_qkv_post under
    one and two persistent workgroups and both K loops; rows of Q / K outside [tok_off, tok_off + M) stay untouched"""
    ops = _ops()
    M, tok_off, H, K = 300, 64, 2, 256
    D = H * 128
    g = torch.Generator().manual_seed(300)
    x = (torch.randn(M, K, generator=g) / 2).to(BF).cuda()
    W = (torch.randn(3 * D, K, generator=g) / K ** 0.5).to(BF).cuda()
    bias = torch.randn(3 * D, generator=g).to(BF).cuda()
    wq = (1 + 0.1 * torch.randn(128, generator=g)).to(BF).cuda()
    wk = (1 + 0.1 * torch.randn(128, generator=g)).to(BF).cuda()
    S = tok_off + M
    S_pad = (S + 63) // 64 * 64
    ids = torch.stack([torch.zeros(S), torch.arange(S) // 19, torch.arange(S) % 19], 1).float()
    cos, sin = [t.cuda().contiguous() for t in dit_ref.rope_tables(ids)]
    qs = 0.1275

    def run(fused):
        qkv = torch.full((M, 3 * D), 3.0, dtype=BF, device="cuda")
        Qh = torch.zeros(H, S_pad, 128, dtype=BF, device="cuda"); Kh = torch.zeros_like(Qh); Vt = torch.zeros(H, 128, S_pad, dtype=BF, device="cuda")
        qk = dict(cols=2 * D, tok_off=tok_off, eps=1e-6, q_scale=qs, wq=wq, wk=wk, cos=cos, sin=sin, Qh=Qh, Kh=Kh) if fused else None
        ops.gemm(x, W, bias=bias, out=qkv, qk_post=qk)
        ops.qkv_post(qkv, 0, D, 2 * D, wq, wk, cos, sin, Qh, Kh, Vt, M, tok_off, H, q_scale=qs, skip_qk=fused)
        torch.cuda.synchronize()
        if fused:
            assert bool((qkv[:, : 2 * D] == 3.0).all()), "the fused epilogue must not write the q / k columns of C"
        return [t.cpu() for t in (Qh, Kh, Vt)]

    for grid in (1, 2):
        for fastk in (1, 0):
            with _options(TILE=2564, PERS_GRID=grid, FASTK=fastk):
                assert ops.gemm_plan(M, 3 * D, K=K)["kernel"] == "w4"
                plain, fused = run(False), run(True)
            what = "PERS_GRID=%d FASTK=%d" % (grid, fastk)
            for name, a, b in zip(("Q", "K", "Vt"), plain, fused):
                d = np.argwhere(_bits(a) != _bits(b))
                assert d.size == 0, "%s: %s differs between GEMM -> qkv_post and the fused epilogue in %d elements, first %s" % (what, name, len(d), tuple(d[0]))
            for name, t in zip(("Q", "K"), fused):
                assert float(t[:, :tok_off].abs().max()) == 0.0 and float(t[:, S:].abs().max()) == 0.0, "%s: %s rows outside the token window written" % (what, name)
                assert float(t[:, tok_off:S].float().abs().max()) > 0.05


# ------------------------------------------------------------------------------------------------ refusals
def test_gemm_refuses_column_boundaries_no_kernel_can_honour():
    """gelu_from = 130 falls inside the 4 columns a lane of either kernel owns (the epilogue decides GELU per such group: columns 130 and 131 would leave without it),
    lora_n_limit = 200 inside a 128-column tile (the K loop takes the LoRA segment per tile: columns 200..255 would get it too).  utx_gemm_bf16 answers -2 under every
    kernel selector and launches nothing -- the output keeps its sentinel -- as utx_gemm_plan does (tests/test_gemm_plan_cpu.py); the same call at the next boundary
    a kernel can honour then succeeds."""
    ops = _ops()
    case = dict(G.CASES_128[2], name="refusal", M=200, N=384, K=64, K2=64, lora_seg_n=128, lora_n_limit=256, nseg=3, gelu_from=132, pad_a=0)
    inp = G.make_inputs(case)
    for tile in (0, 128, 2564):
        for bad in (dict(gelu_from=130), dict(lora_n_limit=200)):
            with _options(TILE=tile):
                with pytest.raises(ValueError):
                    _plan(dict(case, **bad))
                out = _sent(case["M"], case["N"]).cuda()
                with pytest.raises(RuntimeError, match=r"utx_gemm_bf16 failed \(code -2"):
                    ops.gemm(_bf(inp["A"]), _bf(inp["B"]), bias=_bf(inp["bias"]), out=out, A2=_bf(inp["A2"]), B2=_bf(inp["B2"]), lora_seg_n=128,
                             **dict(dict(lora_n_limit=256, gelu_from=132), **bad))
                torch.cuda.synchronize()
                assert (_bits(out.cpu()) == G.SENT16).all(), "a refused launch wrote to the output (UTX_GEMM_TILE=%d, %s)" % (tile, bad)
    with _options(TILE=128):
        bufs = _launch(case, inp)
    _check(case, bufs, G.reference(case, inp), "after the refused launches")

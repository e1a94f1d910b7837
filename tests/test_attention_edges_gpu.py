"""The bf16 attention kernels -- the 8 x 32 kernel of attention_glds.hip in its general, FAST, FAST + KBP and BLK instances with its key-split tail round and attn_merge_kernel,
the 4 x 64 stream of attention_q64.hip with its repair pass -- against the float64 reference oracle/attention_fp64.py at their launch-geometry edges, every output element
inside a COUNTED interval (see that module: E = E_w + r A around the float64 value with r counted from the kernel text, no number from a GPU in it;
tests/test_attention_ref_cpu.py shows on the CPU that the interval is a few 2^-8 of the value wide and that ten kernel mistakes fall outside it).

Cases, operands and references come from the oracle module (one copy, shared with the CPU test).  The operands include the pad region: K rows and V^T columns between S_kv and
the next multiple of 64 hold values that would wreck any row they leaked into.  Every option a test sets is put back in a `finally`.  Outputs are preallocated with a sentinel,
eight rows and 64 columns larger than the contract writes: the sentinel must be gone inside S_q x H * 128 and intact outside."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import attention_fp64 as A

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
_DEFAULTS = (("UTX_ATTN_Q64", 1), ("UTX_ATTN_PEEL", 1), ("UTX_ATTN_TAILSPLIT", 1))
_CACHE = {}


def _ops():
    from unitex_amd.flux import ops
    return ops


@contextlib.contextmanager
def _options(**kw):
    """UTX_ATTN_<name> = value inside the block; every attention option back at its default behind it, whatever happened"""
    from unitex_amd import _lib
    try:
        for k, v in kw.items():
            _lib.set_option("UTX_ATTN_" + k, int(v))
        yield
    finally:
        for k, v in _DEFAULTS:
            _lib.set_option(k, v)


def _ncu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _lib_plan(case):
    out = (C.c_int * 4)()
    assert _ops().get_ctx(0).lib.utx_attn_plan(case["H"], case["Sq"], case["Sk"], _ncu(), out) == 0
    return list(out)


def _case_data(case, scale, plan=None):
    """(inputs, reference): built once per (operands, scale, split or not), shared by every launch, never modified.  The conditions on the inputs that
    tests/test_attention_ref_cpu.py asserts for its copies are asserted here for the ones that go to the GPU."""
    split = plan is not None and plan[2] > 1
    key = (case["data"], case["kb"], case["period"], scale, split)
    if key not in _CACHE:
        inp = _CACHE.get(("inp",) + key[:4]) or A.make_inputs(case, scale)
        _CACHE[("inp",) + key[:4]] = inp
        ref = A.reference(case, inp, scale, A.split_rows(case, plan) if split else None)
        wt = ref.wt[~np.isnan(ref.wt)]
        if case["ramp"] == 0 and case["Sk"] > 1:
            assert wt.size and wt.min() >= 0.3 and wt.max() <= 0.7, "%s: target weights [%g, %g]" % (case["name"], wt.min(), wt.max())
        _CACHE[key] = (inp, ref)
    return _CACHE[key]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(BF)


def _operands(case, inp):
    """Q [H, S_q up to 64, 128] (rows past S_q hold a value no kernel may read into a result), K [H, S_pad, 128] and V^T [H, 128, S_pad] with the oracle's pad region"""
    H, Sq = case["H"], case["Sq"]
    Qh = torch.full((H, (Sq + 63) // 64 * 64, 128), 3.0e38, dtype=BF)
    Qh[:, :Sq] = _t(inp["q"])
    return Qh.cuda(), _t(inp["k"]).cuda(), _t(inp["v"]).transpose(1, 2).contiguous().cuda()


def _out(case):
    return torch.full((case["Sq"] + 8, case["H"] * 128 + 64), A.SENT16, dtype=torch.int16).view(BF).cuda()


def _workspace(case):
    ctx = _ops().get_ctx(0)
    nbytes = int(ctx.lib.utx_attn_workspace_bytes(ctx.handle, case["H"], case["Sq"], case["Sk"]))
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda"), nbytes


def _launch(case, dev, scale, work=None):
    """one utx_attn_fwd_bf16_ws with caller-owned scratch -> the whole output buffer on the CPU"""
    ctx = _ops().get_ctx(0)
    Qh, Kh, Vt = dev
    out = _out(case)
    wk, nbytes = work if work is not None else _workspace(case)
    ctx.check(ctx.lib.utx_attn_fwd_bf16_ws(ctx.handle, Qh.data_ptr(), Kh.data_ptr(), Vt.data_ptr(), out.data_ptr(), Qh.stride(0), 128, Kh.stride(0), 128, Vt.stride(0), Vt.stride(1),
                                           out.stride(0), case["H"], case["Sq"], case["Sk"], float(scale), case["kb"], case["period"], wk.data_ptr(), nbytes, ctx.stream()))
    torch.cuda.synchronize()
    return out.cpu()


def _launch_blk(case, dev, scale):
    """the same operands laid out as the sequence-parallel receive buffer [block][q | k | v][head][blk_rows x 128] through utx_attn_fwd_bf16_blk"""
    ctx = _ops().get_ctx(0)
    Qh, Kh, Vt = dev
    H, S, R = case["H"], case["Sk"], case["blk_rows"]
    P, E = S // R, R * 128
    buf = torch.empty(P, 3, H, E, dtype=BF, device="cuda")
    buf[:, 0] = Qh.view(H, P, E).transpose(0, 1)
    buf[:, 1] = Kh.view(H, P, E).transpose(0, 1)
    buf[:, 2] = Vt.view(H, 128, P, R).permute(2, 0, 1, 3).reshape(P, H, E)
    out = _out(case)
    wk, nbytes = _workspace(case)
    bs = 3 * H * E
    ctx.check(ctx.lib.utx_attn_fwd_bf16_blk(ctx.handle, buf[0, 0].data_ptr(), buf[0, 1].data_ptr(), buf[0, 2].data_ptr(), out.data_ptr(), E, 128, E, 128, E, R, out.stride(0),
                                            H, S, S, float(scale), case["kb"], case["period"], wk.data_ptr(), nbytes, R, bs, bs, bs, ctx.stream()))
    torch.cuda.synchronize()
    return out.cpu()


def _bits(t):
    return t.contiguous().view(torch.int16).numpy()


def _check(case, buf, inp, ref, what, plan=None):
    H, Sq = case["H"], case["Sq"]
    raw = _bits(buf)
    inside = np.zeros(raw.shape, dtype=bool)
    inside[:Sq, : H * 128] = True
    wrong = np.argwhere(~inside & (raw != A.SENT16))
    assert wrong.size == 0, "%s: written outside the %d x %d output at %d places, first (row, column) = %s of a %s buffer" % (what, Sq, H * 128, len(wrong), tuple(wrong[0]), raw.shape)
    left = np.argwhere(inside & (raw == A.SENT16))
    assert left.size == 0, "%s: %d elements never written, first (query, column) = %s" % (what, len(left), tuple(left[0]))
    got = buf[:Sq, : H * 128].double().numpy().reshape(Sq, H, 128).transpose(1, 0, 2)
    msg = A.first_offender(got, ref, inp, what, plan)
    assert msg is None, msg


# ------------------------------------------------------------------------------------------------ 8 x 32 kernel
@pytest.mark.parametrize("case", A.CASES_G + A.CASES_G_KB + A.CASES_G_PER + A.CASES_G_RAMP, ids=lambda c: c["name"])
def test_8x32_edges_under_every_instance(case):
    """softmax_scale = 1 / sqrt(128): the general loop; softmax_scale = 0: FAST (FAST + KBP with a key_bias_period); softmax_scale = 0 with UTX_ATTN_PEEL=0: the general loop
    on pre-scaled Q.  None of these launches splits (a handful of workgroups)."""
    assert _lib_plan(case)[2] == 1
    for scale, peel in ((A.SCALE, 1), (0.0, 1), (0.0, 0)):
        inp, ref = _case_data(case, scale)
        with _options(Q64=0, PEEL=peel):
            buf = _launch(case, _operands(case, inp), scale)
        _check(case, buf, inp, ref, "%s scale=%.4f UTX_ATTN_PEEL=%d (8 x 32)" % (case["name"], scale, peel))


@pytest.mark.parametrize("case", A.CASES_BLK, ids=lambda c: c["name"])
def test_block_strided_instance(case):
    for scale in (0.0, A.SCALE):
        inp, ref = _case_data(case, scale)
        buf = _launch_blk(case, _operands(case, inp), scale)
        _check(case, buf, inp, ref, "%s scale=%.4f (BLK, blocks of %d rows)" % (case["name"], scale, case["blk_rows"]))


# ------------------------------------------------------------------------------------------------ 4 x 64 kernel
def _q64_qualifies(case, dev, work):
    """the documented conditions of include/unitex_hip.h: softmax_scale == 0 (the caller passes it), S_kv a multiple of 64, contiguous operands, no key_bias_period, scratch of
    utx_attn_workspace_bytes present"""
    assert case["Sk"] % 64 == 0 and case["Sk"] >= 64 and case["period"] == 0
    assert all(t.is_contiguous() for t in dev) and work[1] > 0 and work[0].numel() >= work[1]


@pytest.mark.parametrize("case", A.CASES_Q64 + A.CASES_Q64_KB + A.CASES_Q64_RAMP, ids=lambda c: c["name"])
def test_4x64_edges_and_repair_pass(case):
    """UTX_ATTN_Q64=1, pre-scaled Q.  The ramp cases: 45 stays inside the stream's 2^96 headroom; 110 and 150 leave it in some 64-query groups, whose 256-query block the
    repair pass rewrites with the 8 x 32 kernel -- the interval holds on repaired and on untouched rows alike (the reference does not know which are which)."""
    inp, ref = _case_data(case, 0.0)
    dev, work = _operands(case, inp), _workspace(case)
    _q64_qualifies(case, dev, work)
    assert _lib_plan(case)[2] == 1
    with _options(Q64=1):
        buf = _launch(case, dev, 0.0, work)
        flags = work[0][: work[1]].cpu().numpy()[-int((case["H"] * ((case["Sq"] + 255) // 256 * 4) + 255) // 256 * 256):]
    print("%s: base-2 scores [%.1f, %.1f], %d flagged 64-query groups" % (case["name"], ref.smin, ref.smax, int(flags.sum())))
    if case["ramp"] >= 110:
        assert 0 < int(flags.sum()) < case["H"] * ((case["Sq"] + 63) // 64), "%s is meant to leave the 4 x 64 kernel's headroom in some 64-query groups and not in others" % case["name"]
    elif case["ramp"] == 0:
        assert not flags.any()
    _check(case, buf, inp, ref, "%s (4 x 64)" % case["name"])


# ------------------------------------------------------------------------------------------------ key-split tail round
def _split_cases():
    """ids only: the shapes follow the CU count, which is read when the test runs"""
    return [c["name"].replace("k2176", "kN") for c in A.split_cases(256)]


@pytest.mark.parametrize("idx", range(len(A.split_cases(256))), ids=_split_cases())
def test_key_split_tail_round(idx):
    """H = ncu / 2 + 1 heads of two query blocks: one full round and two tail items (the last head), cut along the keys and merged.  Both kernels where the 4 x 64 kernel takes the
    shape; every head against the interval, the tail items with the split term; with UTX_ATTN_TAILSPLIT=0 the same operands against the interval without it."""
    case = A.split_cases(_ncu())[idx]
    split = bool(case["tailsplit"])
    with _options(TAILSPLIT=case["tailsplit"]):
        plan = _lib_plan(case)
        print("%s: H = %d, S_q = %d, S_kv = %d, utx_attn_plan -> %s" % (case["name"], case["H"], case["Sq"], case["Sk"], plan))
        assert plan == A.split_plan(case["H"], case["Sq"], case["Sk"], _ncu(), split)
        assert (plan[2] > 1) == split and plan[0] > plan[1] > 0, "%s: the plan %s is not the one this case is about" % (case["name"], plan)
        if "short_last_range" in case["name"]:
            assert plan[2] >= 3 and ((case["Sk"] + 63) // 64) % plan[3] != 0
        inp, ref = _case_data(case, 0.0, plan)
        dev, work = _operands(case, inp), _workspace(case)
        assert (work[1] > 0) or not split
        kernels = [0] + ([1] if case["Sk"] % 64 == 0 and case["period"] == 0 else [])
        for q64 in kernels:
            from unitex_amd import _lib
            _lib.set_option("UTX_ATTN_Q64", q64)
            buf = _launch(case, dev, 0.0, work)
            _check(case, buf, inp, ref, "%s UTX_ATTN_Q64=%d plan %s" % (case["name"], q64, plan), plan)

"""The MX fp8 attention kernel (csrc/attention_fp8.hip: general loop, peeled loop, key-split tail round through attn_merge_kernel) against the float64 reference
oracle/attention_fp8_fp64.py at its launch-geometry edges, every output element inside a COUNTED interval (see that module; tests/test_attention_fp8_ref_cpu.py shows on the CPU
that the interval is 2^-4 of the value wide and that fifteen kernel mistakes fall outside it).  Operands are quantised on the host and uploaded as bytes; neighbouring 32-blocks,
tiles and rows carry different E8M0 bytes; the pad region and the Q rows past S_q hold hostile finite values.  Outputs are preallocated with a sentinel, eight rows and 64 columns
larger than the contract writes.  Every option a test sets is put back in a `finally`.  Behind it: the launcher's refusals and the two quantisers of the operands at their edges."""
import contextlib
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import attention_fp64 as A
from oracle import attention_fp8_fp64 as F
from oracle import mx8_ref

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
_DEFAULTS = (("UTX_ATTN8_PEEL", 1), ("UTX_ATTN_TAILSPLIT", 1))
_CACHE = {}


def _ops():
    from unitex_amd.flux import ops
    return ops


@contextlib.contextmanager
def _options(**kw):
    """UTX_<name> = value inside the block; both options back at their defaults behind it, whatever happened"""
    from unitex_amd import _lib
    try:
        for k, v in kw.items():
            _lib.set_option("UTX_" + k, int(v))
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


def _case_data(case, plan=None):
    """(inputs, device operands, reference): built once per (operands, key bias, split or not), shared by every launch, never modified"""
    split = plan is not None and plan[2] > 1
    key = (case["data"], case["kb"], case["period"], split)
    if key not in _CACHE:
        ikey = ("inp", case["data"], case["kb"], case["period"])
        if ikey not in _CACHE:
            inp = F.make_inputs(case)
            _CACHE[ikey] = (inp, tuple(torch.from_numpy(inp[k]).cuda() for k in ("q8", "qs", "k8", "ks", "v8t", "vs")))
        inp, dev = _CACHE[ikey]
        ref, share = F.reference(case, inp, A.split_rows(case, plan) if split else None)
        wt = ref.wt[~np.isnan(ref.wt)]
        if case["ramp"] == 0 and case["Sk"] > 1:
            assert wt.size and wt.min() >= 0.25 and wt.max() <= 0.75 and share <= 0.05, "%s: target weights [%g, %g], flush share %g" % (case["name"], wt.min(), wt.max(), share)
        _CACHE[key] = (inp, dev, ref)
    return _CACHE[key]


def _out(case):
    return torch.full((case["Sq"] + 8, case["H"] * 128 + 64), A.SENT16, dtype=torch.int16).view(BF).cuda()


def _workspace(case):
    ctx = _ops().get_ctx(0)
    nbytes = int(ctx.lib.utx_attn_workspace_bytes(ctx.handle, case["H"], case["Sq"], case["Sk"]))
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda"), nbytes


def _rc(case, dev, out, work=None, nbytes=0, fn="utx_attn_fwd_fp8_ws", **over):
    """one launch -> the library's return code.  over: arguments replaced (pointers by name, H / Sq / Sk / S_pad / o_ss / period)"""
    ctx = _ops().get_ctx(0)
    a = dict(q8=dev[0].data_ptr(), qs=dev[1].data_ptr(), k8=dev[2].data_ptr(), ks=dev[3].data_ptr(), v8t=dev[4].data_ptr(), vs=dev[5].data_ptr(), o=out.data_ptr(),
             o_ss=out.stride(0), H=case["H"], Sq=case["Sq"], Sk=case["Sk"], S_pad=dev[2].shape[1], kb=float(case["kb"]), period=case["period"])
    a.update(over)
    args = [ctx.handle] + [C.c_void_p(a[k]) for k in ("q8", "qs", "k8", "ks", "v8t", "vs", "o")] + [a["o_ss"], a["H"], a["Sq"], a["Sk"], a["S_pad"], a["kb"], a["period"]]
    if fn == "utx_attn_fwd_fp8_ws":
        args += [C.c_void_p(work.data_ptr() if work is not None else 0), nbytes]
    rc = getattr(ctx.lib, fn)(*args, ctx.stream())
    torch.cuda.synchronize()
    return rc


def _launch(case, dev, work=None, **kw):
    """one utx_attn_fwd_fp8_ws with caller-owned scratch -> the whole output buffer on the CPU"""
    out = _out(case)
    wk, nbytes = work if work is not None else _workspace(case)
    rc = _rc(case, dev, out, wk, nbytes, **kw)
    assert rc == 0, "%s: return code %d" % (case["name"], rc)
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


# ------------------------------------------------------------------------------------------------ general and peeled loop
@pytest.mark.parametrize("case", F.CASES, ids=lambda c: c["name"])
def test_edges_under_the_peeled_and_the_general_loop(case):
    """UTX_ATTN8_PEEL = 1 (tile 0 and a ragged last tile in the general body, the rest in the fast body; a key_bias_period falls back to the general loop) and 0: both inside the
    interval and equal in bits.  None of these launches splits (a handful of workgroups)."""
    assert _lib_plan(case)[2] == 1
    inp, dev, ref = _case_data(case)
    bufs = []
    for peel in (1, 0):
        with _options(ATTN8_PEEL=peel):
            bufs.append(_launch(case, dev))
        _check(case, bufs[-1], inp, ref, "%s UTX_ATTN8_PEEL=%d" % (case["name"], peel))
    assert np.array_equal(_bits(bufs[0]), _bits(bufs[1])), "%s: the peeled and the general loop differ in bits" % case["name"]


# ------------------------------------------------------------------------------------------------ key-split tail round
def _split_ids():
    """ids only: the shapes follow the CU count, which is read when the test runs"""
    return [c["name"].replace("k2176", "kN") for c in F.split_cases(256)]


@pytest.mark.parametrize("idx", range(len(F.split_cases(256))), ids=_split_ids())
def test_key_split_tail_round(idx):
    """H = ncu / 2 + 1 heads of two query blocks: one full round and two tail items (the last head), cut along the keys and merged; every head against the interval, the tail items
    with the split term; with UTX_ATTN_TAILSPLIT=0 the same operands against the interval without it.  With scratch null or one byte short of what the split needs the launch stays
    unsplit: the bits of the UTX_ATTN_TAILSPLIT=0 launch, inside the plain interval."""
    case = F.split_cases(_ncu())[idx]
    split = bool(case["tailsplit"])
    with _options(ATTN_TAILSPLIT=case["tailsplit"]):
        plan = _lib_plan(case)
        print("%s: H = %d, S_q = %d, S_kv = %d, utx_attn_plan -> %s" % (case["name"], case["H"], case["Sq"], case["Sk"], plan))
        assert plan == A.split_plan(case["H"], case["Sq"], case["Sk"], _ncu(), split)
        assert (plan[2] > 1) == split and plan[0] > plan[1] > 0, "%s: the plan %s is not the one this case is about" % (case["name"], plan)
        if "short_last_range" in case["name"]:
            assert plan[2] >= 3 and ((case["Sk"] + 63) // 64) % plan[3] != 0
        inp, dev, ref = _case_data(case, plan)
        work = _workspace(case)
        assert (work[1] > 0) or not split
        buf = _launch(case, dev, work)
        _check(case, buf, inp, ref, "%s plan %s" % (case["name"], plan), plan)
    if split and case["name"] in ("f8_split_k1472", "f8_split_k1500_ragged"):
        need = (plan[0] - plan[1]) * plan[2] * 256 * (128 * 2 + 4)               # partial rows (bf16) + one float per row
        assert work[1] >= need
        _, _, plain = _case_data(case)
        with _options(ATTN_TAILSPLIT=0):
            unsplit = _launch(case, dev, work)
        _check(case, unsplit, inp, plain, "%s UTX_ATTN_TAILSPLIT=0" % case["name"])
        assert not np.array_equal(_bits(unsplit), _bits(buf)), "the split launch has the bits of the unsplit one: the tail round was not split"
        for what, wk in (("null scratch", (None, 0)), ("scratch one byte short", (work[0], need - 1))):
            out = _out(case)
            assert _rc(case, dev, out, wk[0], wk[1]) == 0
            _check(case, out.cpu(), inp, plain, "%s %s" % (case["name"], what))
            assert np.array_equal(_bits(out.cpu()), _bits(unsplit)), "%s: %s did not keep the launch unsplit" % (case["name"], what)
        out = _out(case)
        assert _rc(case, dev, out, work[0], need) == 0
        assert np.array_equal(_bits(out.cpu()), _bits(buf)), "scratch of exactly the split's own size must split"
        # the context-scratch entry: equal bits with the caller-owned launch
        out = _out(case)
        assert _rc(case, dev, out, fn="utx_attn_fwd_fp8") == 0
        assert np.array_equal(_bits(out.cpu()), _bits(buf)), "%s: utx_attn_fwd_fp8 and utx_attn_fwd_fp8_ws differ in bits" % case["name"]


# ------------------------------------------------------------------------------------------------ refusals
def test_refused_launches_return_minus_2_and_write_nothing():
    case = next(c for c in F.CASES if c["name"] == "f8_h2_q65_k65")
    inp, dev, _ = _case_data(case)
    work = _workspace(case)
    S_pad = dev[2].shape[1]
    assert S_pad == 128
    refusals = [("S_q > S_kv", dict(Sq=66, Sk=65)), ("S_pad < S_kv", dict(S_pad=64)), ("S_pad not a multiple of 64", dict(S_pad=96)), ("o_ss not a multiple of 4", dict(o_ss=322)),
                ("negative key_bias_period", dict(period=-1)), ("H = 0", dict(H=0))]
    refusals += [("%s off 16 bytes" % k, {k: dev[i].data_ptr() + 8}) for k, i in (("q8", 0), ("k8", 2), ("v8t", 4))]
    refusals += [("%s off 4 bytes" % k, {k: dev[i].data_ptr() + 2}) for k, i in (("qs", 1), ("ks", 3), ("vs", 5))]
    refusals += [("null %s" % k, {k: 0}) for k in ("q8", "qs", "k8", "ks", "v8t", "vs", "o")]
    ctx = _ops().get_ctx(0)
    for what, over in refusals:
        out = _out(case)
        for fn in ("utx_attn_fwd_fp8_ws", "utx_attn_fwd_fp8"):
            rc = _rc(case, dev, out, work[0], work[1], fn=fn, **over)
            assert rc == -2, "%s through %s: return code %d" % (what, fn, rc)
        assert (_bits(out.cpu()) == A.SENT16).all(), "%s: the refused launch wrote" % what
    ctx.lib.utx_last_error(ctx.handle)
    out = _out(case)                                      # and the context still launches
    assert _rc(case, dev, out, work[0], work[1]) == 0 and not (_bits(out.cpu())[:65, :256] == A.SENT16).any()


# ------------------------------------------------------------------------------------------------ the quantisers of the operands at their edges
def _sent8(*shape):
    return torch.full(shape, 0xA5, dtype=torch.uint8, device="cuda")


@pytest.mark.parametrize("H,S_pad", [(1, 64), (3, 128), (1, 576), (3, 576)])
def test_quant_vt_mx8_byte_for_byte_at_its_edges(H, S_pad):
    """utx_quant_vt_mx8 against mx8_ref.quantize + the scale permutation: all-zero blocks, amax exactly 2^k and just below, bf16 subnormals (exponent clamped at -127), amax near
    2^120, -0, elements that hit +-448; outputs sentinel-filled and 64 bytes longer than written"""
    ctx = _ops().get_ctx(0)
    vt = F.quant_edge_rows(H * 128, S_pad, 7)
    rq, rs = mx8_ref.quantize(vt)
    v8, vs = _sent8(H * 128 * S_pad + 64), _sent8(H * (S_pad // 32) * 128 + 64)
    ctx.check(ctx.lib.utx_quant_vt_mx8(ctx.handle, vt.cuda().data_ptr(), v8.data_ptr(), vs.data_ptr(), H, S_pad, ctx.stream()))
    torch.cuda.synchronize()
    v8, vs = v8.cpu(), vs.cpu()
    assert (v8[H * 128 * S_pad:] == 0xA5).all() and (vs[H * (S_pad // 32) * 128:] == 0xA5).all(), "written past the end"
    got_s = vs[: H * (S_pad // 32) * 128].view(H, S_pad // 32, 32, 4).permute(0, 3, 2, 1).reshape(H * 128, S_pad // 32)
    bad = torch.nonzero(got_s != rs)
    assert bad.numel() == 0, "scale bytes differ at %d places, first (row, key block) = %s: got %d, expected %d" % (len(bad), bad[0].tolist(), got_s[tuple(bad[0])], rs[tuple(bad[0])])
    got = v8[: H * 128 * S_pad].view(H * 128, S_pad)
    bad = torch.nonzero(got != rq)
    assert bad.numel() == 0, "element bytes differ at %d places, first (row, key) = %s: got 0x%02x, expected 0x%02x" % (len(bad), bad[0].tolist(), got[tuple(bad[0])], rq[tuple(bad[0])])
    assert (rs == 0).any() and (rq == 0x7E).any() and (rq == 0xFE).any() and (rq == 0x80).any(), "the edge blocks are meant to reach byte 0, +-448 and -0"


@pytest.mark.parametrize("H", [1, 3])
def test_quant_qk_mx8_byte_for_byte_at_its_edges(H):
    ops = _ops()
    x = F.quant_edge_rows(H * 64, 128, 11)
    rq, rs = mx8_ref.quantize(x)
    q8, sc = _sent8(H * 64 + 1, 128), _sent8(H * 64 + 1, 4)
    ops.quant_qk_mx8(x.view(H, 64, 128).cuda(), out=(q8[: H * 64].view(H, 64, 128), sc[: H * 64].view(H, 64, 4)))
    torch.cuda.synchronize()
    q8, sc = q8.cpu(), sc.cpu()
    assert (q8[H * 64:] == 0xA5).all() and (sc[H * 64:] == 0xA5).all(), "written past the end"
    assert torch.equal(sc[: H * 64], rs), "scale bytes differ at (row, block) %s" % torch.nonzero(sc[: H * 64] != rs)[:4].tolist()
    assert torch.equal(q8[: H * 64], rq), "element bytes differ at (row, channel) %s" % torch.nonzero(q8[: H * 64] != rq)[:4].tolist()

"""The step-plan table (unitex_amd/flux/step_plan.py) without a device or the library: for every device kind the eager launch and the utx_plan_add_* call
hand the SAME values in the SAME order to the C ABI (the eager call adds the context handle in front and the stream behind, the plan call the plan
handle in front); the walker flattens two-stream sections; an unknown kind is refused where the op is made."""
import types

import pytest
import torch

from unitex_amd._lib import GemmDesc, GemvDesc, LnModDesc, QkvPostDesc
from unitex_amd.flux import step_plan
from unitex_amd.flux.step_plan import DEVICE, Op, walk


class _RecordingLib:
    """every attribute is a function that stores its name and arguments and returns 0"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def fn(*args):
            self.calls.append((name, args))
            return 0
        return fn


def _both(op):
    """-> (name, args) of the eager call and of the plan call for one op"""
    lib = _RecordingLib()
    dit = types.SimpleNamespace(lib=lib, ctx=types.SimpleNamespace(handle="CTX"), attn_events=None, gemm_events=None)
    launch, add = DEVICE[op.kind]
    assert launch(dit, op.args, "STREAM") == 0 and add(lib, "PLAN", op.args) == 0
    assert len(lib.calls) == 2
    return lib.calls


@pytest.mark.parametrize("kind,desc,launch_name,add_name", [("gemm", GemmDesc, "utx_gemm_bf16", "utx_plan_add_gemm"), ("gemv", GemvDesc, "utx_gemv_bf16", "utx_plan_add_gemv"),
                                                            ("ln_mod", LnModDesc, "utx_ln_mod", "utx_plan_add_ln_mod"),
                                                            ("qkv_post", QkvPostDesc, "utx_qkv_post", "utx_plan_add_qkv_post")])
def test_descriptor_kinds_pass_the_same_struct_to_both_calls(kind, desc, launch_name, add_name):
    d = desc()
    (n1, a1), (n2, a2) = _both(Op(kind, d))
    assert (n1, n2) == (launch_name, add_name)
    assert a1[0] == "CTX" and a1[2] == "STREAM" and len(a1) == 3 and a2[0] == "PLAN" and len(a2) == 2
    assert a1[1]._obj is d and a2[1]._obj is d


ATTN = (0x1000, 0x2000, 0x3000, 0x4000, 8192, 128, 8192, 128, 8192, 64, 256, 2, 48, 64, 0.0, 1.5, 3)
ATTN8 = (0x1000, 0x1100, 0x2000, 0x2100, 0x3000, 0x3100, 0x4000, 256, 2, 48, 64, 64, 1.5, 3)


@pytest.mark.parametrize("kind,args,launch_name,add_name", [
    ("attn", ATTN + (0x5000, 4096), "utx_attn_fwd_bf16_ws", "utx_plan_add_attn"), ("attn", ATTN + (None, 0), "utx_attn_fwd_bf16_ws", "utx_plan_add_attn"),
    ("attn8", ATTN8 + (0x5000, 4096), "utx_attn_fwd_fp8_ws", "utx_plan_add_attn_fp8_ws"), ("attn8", ATTN8 + (None, 0), "utx_attn_fwd_fp8_ws", "utx_plan_add_attn_fp8_ws"),
    ("quant_vt", (0x1000, 0x2000, 0x3000, 2, 64), "utx_quant_vt_mx8", "utx_plan_add_quant_vt_mx8")])
def test_pointer_kinds_pass_the_same_scalars_in_the_same_order(kind, args, launch_name, add_name):
    (n1, a1), (n2, a2) = _both(Op(kind, args))
    assert (n1, n2) == (launch_name, add_name)
    assert a1 == ("CTX",) + args + ("STREAM",) and a2 == ("PLAN",) + args


@pytest.mark.parametrize("packed,launch_name", [(0, "utx_quant_mx8"), (1, "utx_quant_mx8_packed")])
def test_quant_mx8_names_its_layout_by_entry_point_when_eager_and_by_flag_in_the_plan(packed, launch_name):
    scalars = (0x1000, 256, 0x2000, 256, 0x3000, 3 if packed else 8, 96, 256)
    (n1, a1), (n2, a2) = _both(Op("quant_mx8", scalars + (packed,)))
    assert (n1, n2) == (launch_name, "utx_plan_add_quant_mx8")
    assert a1 == ("CTX",) + scalars + ("STREAM",) and a2 == ("PLAN",) + scalars + (packed,)


def test_quant_mx8_op_decides_the_scale_layout_where_the_op_is_made():
    x, q = torch.zeros(96, 256, dtype=torch.bfloat16), torch.zeros(96, 512, dtype=torch.uint8)
    rm = torch.zeros(96, 8, dtype=torch.uint8)
    pk = types.SimpleNamespace(data=torch.zeros(2, 1, 512, dtype=torch.uint8), row_blocks=1)
    a = step_plan.quant_mx8_op(x, q[:, :256], rm).args
    assert [v.value for v in (a[0], a[2], a[4])] == [x.data_ptr(), q.data_ptr(), rm.data_ptr()] and (a[1], a[3]) == (256, 512) and a[5:] == (8, 96, 256, 0)
    a = step_plan.quant_mx8_op(x, q[:, :256], pk).args
    assert a[4].value == pk.data.data_ptr() and a[5:] == (1, 96, 256, 1)


@pytest.mark.parametrize("guidance", [True, False])
def test_temb_sum_adds_eagerly_with_torch_and_as_add3_in_the_plan(guidance):
    g = torch.Generator().manual_seed(0)
    e_t, e_g, e_p = (torch.randn(1, 64, generator=g).to(torch.bfloat16) for _ in range(3))
    temb = torch.zeros(1, 64, dtype=torch.bfloat16)
    op = Op("temb_sum", (e_t, e_g if guidance else None, e_p, temb))
    lib = _RecordingLib()
    assert not DEVICE["temb_sum"][0](types.SimpleNamespace(lib=lib), op.args, "STREAM") and not lib.calls      # the library exports no eager add3
    assert torch.equal(temb, ((e_t + e_g) if guidance else e_t) + e_p)
    assert DEVICE["temb_sum"][1](lib, "PLAN", op.args) == 0
    (name, a), = lib.calls
    assert name == "utx_plan_add_add3" and a[0] == "PLAN" and a[5] == 64
    assert [v.value for v in a[1:5]] == [e_t.data_ptr(), e_g.data_ptr() if guidance else None, e_p.data_ptr(), temb.data_ptr()]


def test_walk_flattens_two_stream_sections_and_marks_the_side_ops():
    ops = [Op("gemv", GemvDesc()) for _ in range(5)]
    plan = [ops[0], Op("par", ([ops[1], ops[2]], [ops[3]], None, None)), Op("sp_start"), ops[4]]
    got = list(walk(plan))
    assert [(id(o), s) for o, s in got] == [(id(ops[0]), 0), (id(ops[1]), 0), (id(ops[2]), 0), (id(ops[3]), 1), (id(plan[2]), 0), (id(ops[4]), 0)]
    assert all(o.kind != "par" for o, _ in got)


def test_an_unknown_kind_is_refused_where_the_op_is_made():
    with pytest.raises(ValueError, match="quant_qk"):
        Op("quant_qk", (1, 2, 3))
    assert set(DEVICE) | set(step_plan.HOST_KINDS) == {"gemm", "gemv", "ln_mod", "qkv_post", "attn", "attn8", "quant_mx8", "quant_vt", "temb_sum", "par", "sp_start", "sp_attn"}


def test_timed_without_an_event_list_is_the_bare_call():
    assert step_plan.timed(None, (), lambda: 7) == 7

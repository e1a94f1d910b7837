"""The entries of a FluxDiT step plan: one record type, one table of kinds, one walker, one event bracket.

A plan is a list of Op(kind, args).  The args of an op are final where it is appended (FluxDiT._build): exactly what its C entry point takes -- a filled
descriptor struct, or the pointers / strides / sizes in the ABI's order -- so the eager launch and the utx_plan_add_* call of a kind are the two functions
of ONE table row over the same tuple.  The tensors behind the pointers are kept alive by the plan's workspace dict and the model's weights.
Host kinds ("par": (main ops, side ops, fork event, join event); "sp_start"; "sp_attn") are handled by FluxDiT's two interpreters (run_plan,
compile_plan) and nowhere else.  Debugging tools add a kind of their own as one more row of DEVICE.  Plain Python: importing this touches no device."""
from collections import namedtuple
from ctypes import byref

import torch

from .._lib import ptr

HOST_KINDS = ("par", "sp_start", "sp_attn")


class Op(namedtuple("Op", "kind args")):
    __slots__ = ()

    def __new__(cls, kind, args=None):
        if kind not in DEVICE and kind not in HOST_KINDS:
            raise ValueError("unknown step-plan kind %r" % (kind,))
        return super().__new__(cls, kind, args)


def quant_mx8_op(x, q, s):
    """MX fp8 quantiser of the [M, K] activation x into bytes q and scales s: row-major [M, K / 32], or tile-packed (mx8.PackedScales) -- decided here, once"""
    packed = hasattr(s, "row_blocks")
    return Op("quant_mx8", (ptr(x), x.stride(0), ptr(q), q.stride(0), ptr(s.data if packed else s), s.row_blocks if packed else s.stride(0),
                            x.shape[0], x.shape[1], int(packed)))


def walk(plan):
    """(op, side) of every device and sequence-parallel op of a plan, the two-stream sections flattened: side = 1 for the ops of a section's second stream"""
    for op in plan:
        if op.kind == "par":
            for side in (0, 1):
                for o in op.args[side]:
                    yield o, side
        else:
            yield op, 0


def timed(events, payload, call):
    """call() between two HIP events on the current stream when `events` is a list (bench.py's per-kernel timing): it receives (start, end) + payload"""
    if events is None:
        return call()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    rc = call()
    b.record()
    events.append((a, b) + payload)
    return rc


def _desc(launch, add):
    """a kind whose args are one descriptor struct: <launch>(ctx, &desc, stream) / <add>(plan, &desc)"""
    return (lambda dit, d, st: getattr(dit.lib, launch)(dit.ctx.handle, byref(d), st)), (lambda lib, cplan, d: getattr(lib, add)(cplan, byref(d)))


def _temb_sum(dit, a, st):
    # conditioning = (timesteps_emb + guidance_emb) + pooled_projections, bf16 adds [3p]; torch's current stream (the library exports the add only as a plan entry)
    e_t, e_g, e_p, temb = a
    torch.add(e_t if e_g is None else e_t + e_g, e_p, out=temb)


# kind -> (launch(dit, args, stream) -> rc, add(lib, cplan, args) -> rc)
DEVICE = {
    "gemm": _desc("utx_gemm_bf16", "utx_plan_add_gemm"), "gemv": _desc("utx_gemv_bf16", "utx_plan_add_gemv"),
    "ln_mod": _desc("utx_ln_mod", "utx_plan_add_ln_mod"), "qkv_post": _desc("utx_qkv_post", "utx_plan_add_qkv_post"),
    # (Q, K, V^T, out, their strides, H, S_q, S_kv, scale, key bias, key bias period, scratch, scratch bytes)
    "attn": (lambda dit, a, st: timed(dit.attn_events, (), lambda: dit.lib.utx_attn_fwd_bf16_ws(dit.ctx.handle, *a, st)),
             lambda lib, cplan, a: lib.utx_plan_add_attn(cplan, *a)),
    # (Q8, Q scales, K8, K scales, V8, V scales, out, out row stride, H, S_q, S_kv, S_pad, key bias, key bias period, scratch, scratch bytes)
    "attn8": (lambda dit, a, st: timed(dit.attn_events, (), lambda: dit.lib.utx_attn_fwd_fp8_ws(dit.ctx.handle, *a, st)),
              lambda lib, cplan, a: lib.utx_plan_add_attn_fp8_ws(cplan, *a)),
    # (x, ldx, q, ldq, scales, lds or row blocks, M, K, packed): quant_mx8_op
    "quant_mx8": (lambda dit, a, st: (dit.lib.utx_quant_mx8_packed if a[8] else dit.lib.utx_quant_mx8)(dit.ctx.handle, *a[:8], st),
                  lambda lib, cplan, a: lib.utx_plan_add_quant_mx8(cplan, *a)),
    # (V^T, V8, scales, H, S_pad)
    "quant_vt": (lambda dit, a, st: dit.lib.utx_quant_vt_mx8(dit.ctx.handle, *a, st),
                 lambda lib, cplan, a: lib.utx_plan_add_quant_vt_mx8(cplan, *a)),
    # (e_t, e_g or None, e_p, temb) tensors
    "temb_sum": (_temb_sum, lambda lib, cplan, a: lib.utx_plan_add_add3(cplan, ptr(a[0]), ptr(a[1]), ptr(a[2]), ptr(a[3]), a[3].numel())),
}

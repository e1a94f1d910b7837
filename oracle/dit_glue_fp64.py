"""float64 reference (TEST INFRASTRUCTURE ONLY) of the small kernels between the GEMMs and attention in a DiT step:
ln_mod, qkv_post, gemv, sched_step, add3 (unitex_amd/csrc/dit_elementwise.hip, gemv_bf16_kernel in gemm.hip).

numpy on the CPU.  Every function takes arrays holding bf16-representable values (float32 tables for cos / sin), computes in float64 and rounds
to bf16 (round to nearest even, straight from float64: no float32 step in between) exactly where the kernels' header comments put a tensor
boundary, and nowhere else.  Scalars that the descriptors carry as C floats (eps, q_scale, dsigma) are taken at their float32 value.  Nothing
here knows how a kernel spreads its work over lanes.  oracle/dit_ref.py is the float32 restatement; tests/test_dit_glue_ref_cpu.py pins this
module against it.
"""
import numpy as np

F64 = np.float64


def bf16(x):
    """float64 -> nearest bf16 (ties to even), returned as float64.  The float32 step is only a carrier: where it lands exactly on a bf16 tie
    that the float64 value was not on, the side the float64 value lies on decides."""
    x = np.asarray(x, dtype=F64)
    with np.errstate(over="ignore"):
        f = x.astype(np.float32)
    b = f.view(np.uint32).astype(np.uint64)
    down = b & 0xffff0000
    rne = (b + 0x7fff + ((b >> 16) & 1)) & 0xffff0000
    d = np.abs(x) - np.abs(f.astype(F64))
    tie = ((b & 0xffff) == 0x8000) & np.isfinite(f)
    r = np.where(tie & (d > 0), down + 0x10000, np.where(tie & (d < 0), down, rne))
    r = np.where(np.isnan(f), b, r)
    return r.astype(np.uint32).view(np.float32).astype(F64)


def f32(v):
    return F64(np.float32(v))


def silu(x):
    x = np.asarray(x, dtype=F64)
    with np.errstate(over="ignore"):
        return x / (1.0 + np.exp(-x))


def ln_mod(x, shift, scale, eps=1e-6, parts=False):
    """x [n, D], shift / scale [D] -> bf16(bf16(bf16(LN(x)) * bf16(1 + scale)) + shift).  parts: also the unrounded LN value t, bf16(1 + scale),
    mean and variance (what a test needs to count an error bound)."""
    x, shift, scale = (np.asarray(a, dtype=F64) for a in (x, shift, scale))
    mean = x.mean(-1, keepdims=True)
    var = ((x - mean) ** 2).mean(-1, keepdims=True)
    t = (x - mean) / np.sqrt(var + f32(eps))
    g = bf16(1.0 + scale)
    out = bf16(bf16(bf16(t) * g) + shift)
    return (out, t, g, mean, var) if parts else out


def qkv_post(x, w, cos, sin, eps=1e-6, q_scale=1.0, parts=False):
    """x [..., S, 128] (one of q / k, heads in front), w [128], cos / sin [S, 64] float32 tables -> RMSNorm over the 128 channels (eps inside
    the square root), bf16(bf16(x * rstd) * w), then the interleaved-pair rotation and q_scale in float64 with ONE bf16 rounding.
    parts: also the unrounded x * rstd and the unrounded rotated value."""
    x, w, cos, sin = (np.asarray(a, dtype=F64) for a in (x, w, cos, sin))
    t = x / np.sqrt((x * x).mean(-1, keepdims=True) + f32(eps))
    a = bf16(bf16(t) * w)
    a0, a1 = a[..., 0::2], a[..., 1::2]
    r = np.stack([a0 * cos - a1 * sin, a1 * cos + a0 * sin], -1).reshape(a.shape) * f32(q_scale)
    return (bf16(r), t, r) if parts else bf16(r)


def gemv(x, W, bias=None, silu_in=False, silu_out=False, parts=False):
    """x [M, K], W [N, K], bias [N] or None -> act_out(bf16(act_in(x) @ W^T + bias)), act_in = bf16(silu), act_out = bf16(silu).
    parts: also the unrounded dot product + bias and sum_k |act_in(x)_k W_k|."""
    x, W = np.asarray(x, dtype=F64), np.asarray(W, dtype=F64)
    if silu_in:
        x = bf16(silu(x))
    v = x @ W.T + (0.0 if bias is None else np.asarray(bias, dtype=F64))
    y = bf16(v)
    if silu_out:
        y = bf16(silu(y))
    return (y, v, np.abs(x) @ np.abs(W).T) if parts else y


def sched_step(x, v, dsigma, n_noise=None, cond=None, exact=False):
    """flat x, v -> x[:n_noise] = bf16(x + dsigma * v), x[n_noise:] = cond (left alone when cond is None).  exact: the noise part unrounded."""
    x = np.array(x, dtype=F64)
    n = x.size if n_noise is None else n_noise
    e = x[:n] + f32(dsigma) * np.asarray(v, dtype=F64)[:n]
    if exact:
        return e
    x[:n] = bf16(e)
    if cond is not None:
        x[n:] = np.asarray(cond, dtype=F64)[: x.size - n]
    return x


def add3(a, b, c):
    """bf16(bf16(a + b) + c); b None: bf16(a + c)."""
    t = np.asarray(a, dtype=F64)
    if b is not None:
        t = bf16(t + np.asarray(b, dtype=F64))
    return bf16(t + np.asarray(c, dtype=F64))

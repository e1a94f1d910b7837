"""The HIP AutoencoderKL's kernels at the shapes the 1024 x 6144 strip drives them with, against float64 references.

tests/test_vae_gpu.py checks every layer on at most 16 x 24 pixels; paths that only run at production size (the row-blocked mid
attention, the stream-K score / PV GEMMs, 1 024 GroupNorm statistics blocks, implicit-GEMM convolutions with M = 6.3 M rows) are
checked here.  Inputs are synthetic, seeded and generated on the GPU, rounded to bf16 before either side sees them, so the
reference works on exactly the values the kernel reads.  References are float64 torch ops (on the GPU for the large tensors);
a one-layer AutoencoderKL({"t.weight": ..., "t.bias": ...}) drives _conv / _norm / _attn directly, as in test_vae_gpu.py.

Rounding: bf16 has 8 significant bits, so rounding a value v to bf16 moves it by at most ulp(v) / 2 <= 2^-8 |v| (normal range;
equality at the bottom of a binade); ulp(v) below is the bf16 spacing at |v|.  Each bound is stated and derived where it is asserted."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
F64 = torch.float64
DEV = "cuda:0"


def _gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def _one_layer(params):
    from unitex_amd.flux.vae_hip import AutoencoderKL
    return AutoencoderKL({k: v.cpu() for k, v in params.items()}, device=DEV)     # the product loads state dicts from the host


def _ulp(v):
    """bf16 spacing at |v| (float64 tensor): 2^(e - 8) for |v| in [2^(e-1), 2^e); 2^-133 (the subnormal spacing) at and below 2^-126"""
    _, e = torch.frexp(v.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(v), e - 8)


def _bf16_candidates(v):
    """the two bf16 values around float64 v: the nearest, and its neighbour on v's other side (the nearest itself when v is a bf16 value)"""
    n = v.to(BF)
    nd = n.to(F64)
    toward = torch.where(nd < v, torch.full_like(n, float("inf")), torch.full_like(n, float("-inf")))
    other = torch.where(nd == v, n, torch.nextafter(n, toward))
    return n.to(F64), other.to(F64)


def _free():
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------------------------------------------------------ GroupNorm

def _gn_ref(x, gamma, beta):
    """float64 GroupNorm(32, eps 1e-6) + affine of bf16 x [npix, C]: two-pass group statistics (no cancellation)"""
    npix, C = x.shape
    xd = x.to(F64).view(npix, 32, C // 32)
    m = xd.mean(dim=(0, 2))
    var = (xd - m[None, :, None]).square_().mean(dim=(0, 2))
    z = (xd - m[None, :, None]).mul_(torch.rsqrt(var + 1e-6)[None, :, None]).view(npix, C)
    del xd
    return z.mul_(gamma.to(F64)).add_(beta.to(F64))


def _gn_check(y, x, gamma, beta, silu, tag):
    """y within 1 bf16 ulp of the float64 reference, + 1e-6 absolute.
    silu = 0: the kernel evaluates the normalisation and affine in fp32 (relative error ~1e-7 on O(1) terms, 2^-24 |mean| removed by
    centring on the pilot) and rounds once to bf16: <= ulp(ref) / 2 + the fp32 error, well inside ulp(ref) + 1e-6.
    silu = 1: like the reference, the GroupNorm value t is rounded to bf16, SiLU applied, and rounded again.  The kernel's fp32 t may land on
    either side of a bf16 rounding boundary of the exact t, so its bf16 t is one of the two bf16 neighbours of the exact t; the reference
    is taken at both, and y must be within 1 ulp + 1e-6 of one of them (SiLU's slope at -5 turns one ulp of t into ~5 ulps of the output,
    so a single reference would fail on boundary cases that are correct)."""
    ref = _gn_ref(x, gamma, beta).view(-1)
    yd = y.view(-1).to(F64)
    if not silu:
        excess = (yd - ref).abs_().sub_(_ulp(ref))
    else:
        excess = None
        for t in _bf16_candidates(ref):
            r = torch.nn.functional.silu(t).to(BF).to(F64)
            e = (yd - r).abs_().sub_(_ulp(r))
            excess = e if excess is None else torch.minimum(excess, e)
            del r, t
    del ref
    worst = excess.max().item()
    bad = int((excess > 1e-6).sum().item())
    print("[gn %s] worst |y - ref| - ulp(ref) = %.3g, %d elements beyond 1 ulp + 1e-6" % (tag, worst, bad))
    return worst, bad


GN_CHANNELS = list(range(128, 2049, 128))


@pytest.mark.parametrize("silu", [0, 1])
@pytest.mark.parametrize("npix", [1237, 300007])
@pytest.mark.parametrize("C", GN_CHANNELS)
def test_group_norm_every_channel_count(C, npix, silu):
    """every C the launcher accepts (C % 128 == 0, <= 2048): one ragged statistics block (1 237 pixels) and many (300 007).  For C / 8 not
    dividing 256 (C = 384, 640, 768, ...) the statistics pass used to read part of its pixels twice: mean and variance off by up to 78 %."""
    g = _gen(C * 7 + npix + silu)
    x = (torch.randn(npix, C, generator=g, device=DEV) * 1.5 + 0.3).to(BF)
    gamma = (1 + 0.1 * torch.randn(C, generator=g, device=DEV)).to(BF)
    beta = (0.1 * torch.randn(C, generator=g, device=DEV)).to(BF)
    vae = _one_layer({"t.weight": gamma, "t.bias": beta})
    y = vae._norm(x, "t", bool(silu))
    worst, bad = _gn_check(y, x, gamma, beta, silu, "C=%d npix=%d silu=%d" % (C, npix, silu))
    del x, y
    _free()
    assert bad == 0, "C=%d npix=%d silu=%d: %d elements beyond 1 bf16 ulp + 1e-6 (worst excess %.3g)" % (C, npix, silu, bad, worst)


# mean / sigma of the 32 groups: the five ratios, one constant group (var = 0: the eps path), one of alternating +-3072 (m = 0, sigma = 3072)
GN_RATIOS = (0, 8, 64, 256, 1024)


def _offset_groups(npix, C, seed):
    cpg = C // 32
    g = _gen(seed)
    sig = torch.tensor([2.0 ** ((i % 3) - 1) for i in range(32)], device=DEV)
    ratio = torch.tensor([float(GN_RATIOS[i % 5]) for i in range(32)], device=DEV)
    sign = torch.tensor([(-1.0) ** (i // 5) for i in range(32)], device=DEV)
    x = torch.randn(npix, 32, cpg, generator=g, device=DEV)
    x.mul_(sig[None, :, None]).add_((sign * ratio * sig)[None, :, None])
    x[:, 30, :] = 5.0                                                      # constant
    alt = torch.where(torch.arange(npix, device=DEV) % 2 == 0, 3072.0, -3072.0)
    x[:, 31, :] = alt[:, None]                                             # alternating +-3072
    kind = ["ratio%d" % GN_RATIOS[i % 5] for i in range(30)] + ["constant", "alternating"]
    return x.view(npix, C).to(BF), kind


@pytest.mark.parametrize("npix,C", [(6291456, 128), (6291456, 256), (1572864, 128), (1572864, 256), (1572864, 512),
                                    (393216, 256), (393216, 512), (98304, 512)])
def test_group_norm_production_offset_groups(npix, C):
    """every GroupNorm size of the strip's encode and decode, with groups whose mean is 0 / 8 / 64 / 256 / 1024 sigma, a constant group and an
    alternating +-3072 one.  Sums of x and x^2 in fp32 lose the variance once mean^2 / var approaches 2^24 / n-per-thread (mean / sigma = 1024:
    rstd off by ~14 %); the kernel sums x - P around a per-group pilot P.  Bound: as test_group_norm_every_channel_count, silu = 0."""
    x, kind = _offset_groups(npix, C, npix + C)
    g = _gen(C)
    gamma = (1 + 0.1 * torch.randn(C, generator=g, device=DEV)).to(BF)
    beta = (0.1 * torch.randn(C, generator=g, device=DEV)).to(BF)
    vae = _one_layer({"t.weight": gamma, "t.bias": beta})
    y = vae._norm(x, "t", False)
    ref = _gn_ref(x, gamma, beta)
    excess = ((y.to(F64) - ref).abs_() - _ulp(ref)).view(npix, 32, C // 32).amax(dim=(0, 2)).cpu()
    del ref, y, x
    _free()
    per_kind = {}
    for i, k in enumerate(kind):
        per_kind[k] = max(per_kind.get(k, -1.0), excess[i].item())
    print("[gn offsets npix=%d C=%d] worst |y - ref| - ulp(ref) per group kind: %s" % (npix, C, ", ".join("%s %.3g" % kv for kv in per_kind.items())))
    assert max(per_kind.values()) <= 1e-6, per_kind


# ------------------------------------------------------------------------------------------------------------------ softmax

def _softmax_rows(s, nrow, ncol):
    from unitex_amd._lib import ptr
    from unitex_amd.flux import ops
    ctx = ops.get_ctx(0)
    ctx.check(ctx.lib.utx_softmax_rows(ctx.handle, ptr(s), nrow, s.stride(0), ncol, ctx.stream()))


def _softmax_check(p, s_in):
    """p = the kernel's bf16 softmax of bf16 rows s_in.  Kernel: exp(x - max) in fp32 (a few fp32 ulps), the row sum in fp32 (<= 400
    terms per thread, then a tree: relative error < 2.5e-5 at 98 304 columns), one product with the reciprocal, and one rounding to bf16
    (<= 2^-8 relative): every element within 2^-8 ref, with 2^-126 absolute for the values bf16 flushes (exp of -100 is 3.7e-44).  The
    row sum of the rounded values: each term within 2^-8 of its own value, so the sum within 2^-8 (+ the fp32 part) of 1: assert 2^-8."""
    ref = torch.softmax(s_in.to(F64), dim=-1)
    pd = p.to(F64)
    excess = ((pd - ref).abs() - (2.0 ** -8 * ref + 2.0 ** -126)).max().item()
    rowsum = (pd.sum(dim=-1) - 1).abs().max().item()
    return excess, rowsum


def _score_rows(nrow, ncol, seed):
    """row r % 4: 0 Gaussian (sigma 3, the spread of the VAE's score GEMM); 1 the same with one dominant key (+40); 2 all keys equal;
    3 key 0 at 0 and the rest at -100 (their exp underflows fp32 and bf16)"""
    g = _gen(seed)
    s = torch.randn(nrow, ncol, generator=g, device=DEV) * 3
    r = torch.arange(nrow, device=DEV)
    dom = torch.randint(0, ncol, (nrow,), generator=g, device=DEV)
    s[r % 4 == 1, dom[r % 4 == 1]] = 40.0
    s[r % 4 == 2] = 1.5
    s[r % 4 == 3] = -100.0
    s[r % 4 == 3, 0] = 0.0
    return s.to(BF)


@pytest.mark.parametrize("nrow,ncol,ld", [(256, 8, 8), (300, 2056, 2056), (257, 2056, 2560), (128, 24576, 24576), (1536, 98304, 98304),
                                          (64, 98304, 98312)])
def test_softmax_rows_production(nrow, ncol, ld):
    """row softmax at the mid attention's widths (S = 24 576 for the 512 x 3072 strip, 98 304 for 1024 x 6144; 1 536 rows = the last score
    block at S = 98 304) and on column sub-views (ld > ncol: the columns past ncol are not touched)"""
    s_in = _score_rows(nrow, ncol, nrow + ncol)
    buf = torch.full((nrow, ld), 7.0, dtype=BF, device=DEV)
    buf[:, :ncol] = s_in
    d = buf[:, :ncol]
    _softmax_rows(d, nrow, ncol)
    excess, rowsum = _softmax_check(d, s_in)
    print("[softmax %d x %d ld %d] worst |p - ref| - (2^-8 ref + 2^-126) = %.3g, max |row sum - 1| = %.3g" % (nrow, ncol, ld, excess, rowsum))
    assert excess <= 0 and rowsum <= 2.0 ** -8
    eq = d[2::4]
    assert torch.equal(eq, torch.full_like(eq, 1.0 / ncol)), "all-equal rows: expected 1/ncol rounded to bf16 exactly"
    if ld > ncol:
        assert bool((buf[:, ncol:] == 7.0).all()), "softmax wrote past ncol"
    del buf, d, s_in
    _free()


# ------------------------------------------------------------------------------------------------------------------ convolutions

def _sample_pixels(Ho, Wo, seed):
    """the corners, 64 pixels on each edge row / column, m = b - 1, b, b + 1 around 12 multiples b of 256 (the M-tile boundaries of both the
    128- and the 256-row GEMM tiles), the whole last 256-row tile, and 1 024 random pixels"""
    M = Ho * Wo
    g = _gen(seed)
    idx = [0, Wo - 1, M - Wo, M - 1]
    xs = torch.linspace(0, Wo - 1, 64, device=DEV).long()
    ys = torch.linspace(0, Ho - 1, 64, device=DEV).long()
    idx = torch.tensor(idx, device=DEV)
    parts = [idx, xs, (Ho - 1) * Wo + xs, ys * Wo, ys * Wo + Wo - 1]
    b = (torch.linspace(1, M // 256 - 1, 12, device=DEV).long() * 256)
    parts += [b - 1, b, b + 1, torch.arange(max(0, M - 256), M, device=DEV), torch.randint(0, M, (1024,), generator=g, device=DEV)]
    return torch.unique(torch.cat(parts).clamp(0, M - 1))


def _gather_taps(x, H, W, m, Wo, mode):
    """the 3 x 3 input neighbourhoods of output pixels m: [len(m), 9, Cin] float64; zero outside the (padded / upsampled) input"""
    oy, ox = m // Wo, m % Wo
    ky = torch.arange(3, device=DEV).repeat_interleave(3)
    kx = torch.arange(3, device=DEV).repeat(3)
    if mode == "down":            # F.pad(x, (0, 1, 0, 1)) then a valid stride-2 3 x 3: rows / columns H, W are the zero pad
        iy, ix = 2 * oy[:, None] + ky, 2 * ox[:, None] + kx
        ok = (iy < H) & (ix < W)
    elif mode == "up":            # nearest 2x, then a pad-1 3 x 3 over the 2H x 2W image: source pixel = upsampled pixel // 2
        uy, ux = oy[:, None] + ky - 1, ox[:, None] + kx - 1
        ok = (uy >= 0) & (uy < 2 * H) & (ux >= 0) & (ux < 2 * W)
        iy, ix = uy.div(2, rounding_mode="floor"), ux.div(2, rounding_mode="floor")
    else:
        iy, ix = oy[:, None] + ky - 1, ox[:, None] + kx - 1
        ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
    src = (iy.clamp(0, H - 1) * W + ix.clamp(0, W - 1))
    a = x[src].to(F64)                                    # [n, 9, Cin]
    return a * ok[..., None]


def _conv_bound_check(y, ref, absum, K, tag, res=None):
    """|y - ref| <= 2^-8 |ref| + K 2^-24 sum|a w| (+ |bias|): the bf16 rounding of the output plus the standard fp32 summation bound of a
    K-term dot product.  With a residual r the epilogue stores bf16(r + bf16(c)): two roundings, |y - (r + ref)| <= (2^-8 + 2^-16) (|ref| +
    |r + ref|) + 2 K 2^-24 sum|a w|."""
    E = K * 2.0 ** -24 * absum
    if res is None:
        bound = 2.0 ** -8 * ref.abs() + E
        err = (y - ref).abs()
    else:
        z = res + ref
        bound = (2.0 ** -8 + 2.0 ** -16) * (ref.abs() + z.abs()) + 2 * E
        err = (y - z).abs()
    ratio = (err / bound).max().item()
    print("[conv %s] max |y - ref| / bound = %.3g (max|ref| %.3g)" % (tag, ratio, ref.abs().max().item()))
    return ratio


# (tag, Cin, Cout, H, W of the input, mode, residual?, 1 x 1 shortcut from Cin?)
CONV_CASES = [
    ("enc conv_in 3->128", 3, 128, 1024, 6144, "s1", False, False),
    ("enc 128->128 res", 128, 128, 1024, 6144, "s1", True, False),
    ("enc down 128", 128, 128, 1024, 6144, "down", False, False),
    ("enc down 256", 256, 256, 512, 3072, "down", False, False),
    ("enc down 512", 512, 512, 256, 1536, "down", False, False),
    ("enc 128->256 +shortcut", 128, 256, 512, 3072, "s1", False, True),
    ("enc 256->512 +shortcut", 256, 512, 256, 1536, "s1", False, True),
    ("enc 256->256", 256, 256, 512, 3072, "s1", False, False),
    ("enc 512->512", 512, 512, 128, 768, "s1", False, False),
    ("enc conv_out 512->32", 512, 32, 128, 768, "s1", False, False),
    ("dec conv_in 16->512", 16, 512, 128, 768, "s1", False, False),
    ("dec 512->512 res", 512, 512, 128, 768, "s1", True, False),
    ("dec 512->512 @256x1536 res", 512, 512, 256, 1536, "s1", True, False),
    ("dec up 512 -> 256x1536", 512, 512, 128, 768, "up", False, False),
    ("dec up 512 -> 512x3072", 512, 512, 256, 1536, "up", False, False),
    ("dec up 256 -> 1024x6144", 256, 256, 512, 3072, "up", False, False),
    ("dec 512->256 +shortcut", 512, 256, 512, 3072, "s1", False, True),
    ("dec 256->128 +shortcut", 256, 128, 1024, 6144, "s1", False, True),
    ("dec 128->128", 128, 128, 1024, 6144, "s1", False, False),
    ("dec conv_out 128->3", 128, 3, 1024, 6144, "s1", False, False),
]


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0].replace(" ", "_") for c in CONV_CASES])
def test_conv_production_geometry(case):
    """every 3 x 3 convolution of the strip's encode (1024 x 6144 image) and decode (latent 128 x 768) at its own geometry, with the 1 x 1
    shortcut GEMMs of the channel-changing resnets and the residual epilogue; float64 reference on sampled output pixels, all channels"""
    from unitex_amd.flux import ops
    tag, cin, cout, H, W, mode, use_res, shortcut = case
    g = _gen(cin * 1000 + cout + H)
    name = "t.conv_out" if cout % 8 else "t"
    w = (torch.randn(cout, cin, 3, 3, generator=g, device=DEV) / math.sqrt(9 * cin)).to(BF)
    b = (0.1 * torch.randn(cout, generator=g, device=DEV)).to(BF)
    x = torch.randn(H * W, cin, generator=g, device=DEV).to(BF)
    vae = _one_layer({name + ".weight": w, name + ".bias": b})
    Ho, Wo = (H // 2, W // 2) if mode == "down" else ((2 * H, 2 * W) if mode == "up" else (H, W))
    r = torch.randn(Ho * Wo, cout, generator=g, device=DEV).to(BF) if use_res else None
    y, ho, wo = vae._conv(x, H, W, name, stride=2 if mode == "down" else 1, up=1 if mode == "up" else 0, res=r)
    assert (ho, wo) == (Ho, Wo)
    m = _sample_pixels(Ho, Wo, cin + cout)
    a = _gather_taps(x, H, W, m, Wo, mode)                           # [n, 9, cin]
    wt = w.to(F64).permute(2, 3, 1, 0).reshape(9, cin, cout)         # [tap, cin, cout]
    ref = torch.einsum("ntc,tco->no", a, wt) + b.to(F64)
    absum = torch.einsum("ntc,tco->no", a.abs(), wt.abs()) + b.to(F64).abs()
    ratio = _conv_bound_check(y[m, :cout].to(F64), ref, absum, 9 * cin, tag, None if r is None else r[m].to(F64))
    assert ratio <= 1.0, "%s: sampled outputs beyond the bf16 + fp32-summation bound (x %.3g)" % (tag, ratio)
    if shortcut:                                                     # the resnet's 1 x 1 conv_shortcut on the block input: a plain GEMM, K = cin
        ws = (torch.randn(cout, cin, generator=g, device=DEV) / math.sqrt(cin)).to(BF)
        bs = (0.1 * torch.randn(cout, generator=g, device=DEV)).to(BF)
        ys = ops.gemm(x, ws, bias=bs)
        xs = x[m].to(F64)
        ref = xs @ ws.to(F64).t() + bs.to(F64)
        absum = xs.abs() @ ws.to(F64).abs().t() + bs.to(F64).abs()
        ratio = _conv_bound_check(ys[m].to(F64), ref, absum, cin, tag + " shortcut")
        assert ratio <= 1.0, "%s shortcut: beyond the bound (x %.3g)" % (tag, ratio)
    del x, y, r, a, vae
    _free()


# ------------------------------------------------------------------------------------------------------------------ mid attention

def _attn_layer(S, seed, C=512):
    """x [S, C] and a one-layer attention block whose score GEMM gives scores of sigma ~3 (q, k elements of variance 3: 512 * 3 * 3 / 512 = 9)"""
    g = _gen(seed)
    s3, s1 = math.sqrt(3.0 / C), math.sqrt(1.0 / C)
    p = {"t.group_norm.weight": 1 + 0.1 * torch.randn(C, generator=g, device=DEV), "t.group_norm.bias": 0.1 * torch.randn(C, generator=g, device=DEV)}
    for n, sc in (("to_q", s3), ("to_k", s3), ("to_v", s1), ("to_out.0", s1)):
        p["t.%s.weight" % n] = torch.randn(C, C, generator=g, device=DEV) * sc
        p["t.%s.bias" % n] = 0.1 * torch.randn(C, generator=g, device=DEV)
    p = {k: v.to(BF) for k, v in p.items()}
    x = torch.randn(S, C, generator=g, device=DEV).to(BF)
    return _one_layer(p), p, x


def test_attn_row_blocking_bit_identical():
    """S = 4 096 as one block of scores, as 16 blocks of 256 query rows, and as 5 blocks of 768 + 256: softmax and P V are row-wise, so the
    blocked results are the same bits (the claim _attn's row blocking rests on)"""
    vae, _, x = _attn_layer(4096, 11)
    outs = []
    for qb in (None, 256, 768):
        if qb is not None:
            vae.attn_score_elems = qb * 4096       # instance attribute: the class default stays as it is
        outs.append(vae._attn(x, "t"))
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def _attn_rows(S, QB, seed):
    """first / last 8 rows of every score block, so both sides of every block boundary, and 256 random rows"""
    rows = []
    for r0 in range(0, S, QB):
        r1 = min(S, r0 + QB)
        rows += list(range(r0, r0 + 8)) + list(range(r1 - 8, r1))
    r = torch.tensor(rows, device=DEV)
    return torch.unique(torch.cat([r, torch.randint(0, S, (256,), generator=_gen(seed), device=DEV)]))


def _rb(t):
    return t.to(BF).to(F64)


@pytest.mark.parametrize("S", [40960, 98304])
def test_attn_production_row_blocks(S):
    """S = 40 960 (two score blocks, the second ragged) and S = 98 304, the 1024 x 6144 strip (10 blocks, the last of 1 536 rows), at the
    default score budget.  Sampled rows against
    (1) an emulating float64 reference from the product's own q, k, V^T (the same deterministic ops.gemm calls _attn makes), rounded to bf16
        where the product rounds: scores after alpha, P, a = P V + b_v, the out-projection, and the residual sum.  Bound per element:
        2 ulp(ref) + 2^-8 rms(ref row) -- the product's fp32 accumulations may put a score, a probability or an output on the other side of
        a bf16 rounding boundary (1 ulp each), and those single-ulp moves average over 512 / S terms into the row's scale;
    (2) a plain float64 evaluation of the block (GroupNorm, projections, softmax over all S keys, out-projection, residual) with no
        rounding: the distance is printed and asserted loosely (<= 0.02 max|ref|, the full-width bf16 DiT's figure is 0.012); it is what
        materialising scores and probabilities in bf16 costs at production length."""
    from unitex_amd.flux import ops
    vae, p, x = _attn_layer(S, S)
    QB = max(256, min(S, (vae.attn_score_elems // S) // 256 * 256))
    assert (S + QB - 1) // QB == {40960: 2, 98304: 10}[S]
    y = vae._attn(x, "t")
    rows = _attn_rows(S, QB, S + 1)
    C = x.shape[1]
    alpha = 1.0 / math.sqrt(C)
    # (1) emulating reference
    h = vae._norm(x, "t.group_norm", False)
    w = vae.w
    q = ops.gemm(h, w["t.to_q.weight"], bias=w["t.to_q.bias"])
    k = ops.gemm(h, w["t.to_k.weight"], bias=w["t.to_k.bias"]).to(F64)
    vt = ops.gemm(w["t.to_v.weight"], h).to(F64)
    wo, bo, bv = w["t.to_out.0.weight"].to(F64), w["t.to_out.0.bias"].to(F64), w["t.to_v.bias"].to(F64)
    yr = y[rows].to(F64)
    xr = x[rows].to(F64)
    worst = 0.0
    emu = torch.empty_like(yr)
    for c0 in range(0, rows.numel(), 64):
        rr = rows[c0:c0 + 64]
        s = _rb(q[rr].to(F64) @ k.t() * alpha)
        pr = _rb(torch.softmax(s, dim=-1))
        a = _rb(pr @ vt.t() + bv)
        emu[c0:c0 + 64] = _rb(xr[c0:c0 + 64] + _rb(a @ wo.t() + bo))
        del s, pr, a
    bound = 2 * _ulp(emu) + 2.0 ** -8 * emu.square().mean(dim=1, keepdim=True).sqrt()
    worst = ((yr - emu).abs() / bound).max().item()
    del q, k, vt, h
    _free()
    # (2) plain float64
    g64 = _gn_ref(x, p["t.group_norm.weight"], p["t.group_norm.bias"])
    lin = lambda t, n: t @ p["t.%s.weight" % n].to(F64).t() + p["t.%s.bias" % n].to(F64)
    k64, v64 = lin(g64, "to_k"), lin(g64, "to_v")
    q64 = lin(g64[rows], "to_q")
    del g64
    ref = torch.empty_like(yr)
    for c0 in range(0, rows.numel(), 64):
        pr = torch.softmax(q64[c0:c0 + 64] @ k64.t() * alpha, dim=-1)
        ref[c0:c0 + 64] = xr[c0:c0 + 64] + lin(pr @ v64, "to_out.0")
        del pr
    dist = (yr - ref).abs().max().item()
    scale = ref.abs().max().item()
    mean_d = (yr - ref).abs().mean().item()
    print("[attn S=%d, %d blocks of %d] emulating: max |y - ref| / bound = %.3g; plain fp64: max|d| %.4g = %.4g of max|ref| %.3g, mean|d| %.4g "
          "(%d rows)" % (S, (S + QB - 1) // QB, QB, worst, dist, dist / scale, scale, mean_d, rows.numel()))
    del k64, v64, q64, y, x
    _free()
    assert worst <= 1.0, "S=%d: sampled rows beyond 2 ulp + 2^-8 rms of the emulating reference (x %.3g)" % (S, worst)
    assert dist <= 0.02 * scale


# ------------------------------------------------------------------------------------------------------------------ decode

def test_decode_reference_operating_point():
    """decode of a 64 x 384 latent (512 x 3072 image, mid attention S = 24 576) against oracle/vae_ref in fp32 on the GPU, same synthetic
    weights; the uint8 contract of test_e2e_tolerance_gpu.py: >= 99 % of the pixels within 2 LSB, >= 99.9 % within 4, none beyond 8"""
    import numpy as np

    from oracle import pipeline_ref, vae_ref
    from unitex_amd.flux.pipeline import PBRFluxPipeline
    from unitex_amd.flux.synthetic import synthetic_vae_state_dict
    from unitex_amd.flux.vae_hip import AutoencoderKL
    sd = synthetic_vae_state_dict(1)
    z = torch.randn(1, 16, 64, 384, generator=_gen(5), device=DEV).to(BF)
    vae = AutoencoderKL(sd, device=DEV)
    img = vae.decode(z)
    got = np.asarray(PBRFluxPipeline._postprocess(img)[0])[None]
    del vae, img
    _free()
    # plain fp32: no reduced-precision matmul, and torch's own im2col convolution rather than MIOpen's (whose first-use kernel builds for
    # ~25 layer shapes took minutes)
    saved = (torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32, torch.backends.cudnn.enabled)
    torch.backends.cuda.matmul.allow_tf32 = torch.backends.cudnn.allow_tf32 = torch.backends.cudnn.enabled = False
    try:
        ref_vae = vae_ref.AutoencoderKL.from_state_dict(sd).to(DEV)
        with torch.no_grad():
            ref_img = ref_vae.decode(z.float()).cpu()
    finally:
        torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32, torch.backends.cudnn.enabled = saved
    del ref_vae
    _free()
    ref = pipeline_ref.postprocess_u8(ref_img, True)[None]
    du = np.abs(got.astype(np.int32) - ref.astype(np.int32))
    hist = {k: float((du <= k).mean()) for k in (0, 1, 2, 4, 8)}
    print("[decode 512 x 3072] uint8 vs fp32 oracle: ==0 %.4f, <=1 %.4f, <=2 %.4f, <=4 %.4f, <=8 %.4f, max %d LSB (image std %.1f LSB)"
          % (hist[0], hist[1], hist[2], hist[4], hist[8], int(du.max()), float(ref.std())))
    assert ref.std() > 4.0
    assert hist[2] >= 0.99 and hist[4] >= 0.999 and du.max() <= 8

"""Numpy mirror (TEST INFRASTRUCTURE ONLY) of unitex_amd/csrc/shade_device.h: each per-pixel primitive of the geometry and shading kernels once --
barycentric interpolation, length and normalise, the grid_sample lookups (bilinear with zero padding or reflection, nearest), nvdiffrast's wrap
lookup and the overlay / blending epilogue of the two bakes.  Every function takes `dtype`: np.float32 evaluates the device expression in the device's order, every operation rounded on its own (numpy
contracts nothing), np.float64 is the yardstick the counted bounds are measured from.

The order of the roundings is the point.  torch's scalar and device grid_sample kernels unnormalise as ((g + 1) * size - 1) / 2, every operation
rounded; a fused (g + 1) * (size / 2) - 0.5 lands on another float often enough to move a bilinear sample by several ulps (the count is in
oracle/gbuffer_ref.py, MAP_BOUND).  The restatements that pin the kernels bit for bit share this one spelling."""
import numpy as np

F32, F64 = np.float32, np.float64


# ---- barycentric interpolation
def bary_w(rast, dtype=F32):  # sd_bary_w
    """rast [...,4] -> (u, v, w = (1 - u) - v), each [...,1] in `dtype`"""
    r = np.asarray(rast, F32)
    u, v = r[..., 0:1].astype(dtype), r[..., 1:2].astype(dtype)
    return u, v, (dtype(1.0) - u) - v


def interp_corners(attr, corners, u, v, w):  # sd_interp1
    """(a0*u + a1*v) + a2*w with a_k = attr[corners[...,k]] ([...,C]) and the weights [...,1], in attr's dtype"""
    return (attr[corners[..., 0]] * u + attr[corners[..., 1]] * v) + attr[corners[..., 2]] * w


def interp(attr, rast, faces, dtype=F32):  # sd_interp / utx_interpolate
    """(a0*u + a1*v) + a2*((1-u)-v) in `dtype`, zeros where empty; attr [V,C] -> ([...,C], coverage [...])"""
    attr = np.asarray(attr, dtype)
    tid = np.asarray(rast, F32)[..., 3].astype(np.int64) - 1
    cov = tid >= 0
    f = np.asarray(faces)[np.where(cov, tid, 0)]
    u, v, w = bary_w(rast, dtype)
    out = interp_corners(attr, f, u, v, w)
    return np.where(cov[..., None], out, dtype(0.0)).astype(dtype), cov


# ---- length and normalise
def len3(p, dtype=None):  # sd_length3
    """sqrt((x*x + y*y) + z*z) -> [...,1]; dtype None keeps p's own"""
    p = np.asarray(p) if dtype is None else np.asarray(p, dtype)
    return np.sqrt((p[..., 0:1] * p[..., 0:1] + p[..., 1:2] * p[..., 1:2]) + p[..., 2:3] * p[..., 2:3])


def unit(p, length=None, dtype=None):  # sd_normalize3
    """F.normalize(eps=1e-12): p / max(|p|, 1e-12); `length` [...,1] is |p| where the caller has it already"""
    p = np.asarray(p) if dtype is None else np.asarray(p, dtype)
    return p / np.maximum(len3(p) if length is None else length, p.dtype.type(1e-12))


# ---- grid_sample(align_corners=False) on an image [H,W,C] at pixel coordinates
def grid_unnormalize(g, size, dtype=F32):  # grid_unnormalize
    return ((np.asarray(g, dtype) + dtype(1.0)) * dtype(size) - dtype(1.0)) * dtype(0.5)


def reflect_index(g, size, dtype=F32):  # grid_reflect_index
    """padding_mode='reflection': unnormalise, reflect about [-0.5, size - 0.5], clip to [0, size - 1]; the parity of the flips in `dtype`, fmax / fmin as fmaxf / fminf"""
    span = dtype(size)
    with np.errstate(over="ignore", invalid="ignore"):
        x = np.abs(grid_unnormalize(g, size, dtype) + dtype(0.5))
        extra = np.fmod(x, span)
        even = np.fmod(np.floor(x / span), dtype(2.0)) == 0
        x = np.where(even, extra - dtype(0.5), (span - extra) - dtype(0.5)).astype(dtype)
    return np.fmin(dtype(size - 1), np.fmax(x, dtype(0)))


def grid_tap(img, y, x, dtype=F32):  # grid_tap
    """img [H,W,C] at the integer-valued (y, x): zero outside the image"""
    H, W = img.shape[:2]
    inside = (x >= 0) & (x < W) & (y >= 0) & (y < H)
    t = img[np.clip(y, 0, H - 1).astype(np.int64), np.clip(x, 0, W - 1).astype(np.int64)].astype(dtype)
    return np.where(inside[..., None], t, dtype(0.0))


def grid_blend(img, ix, iy, dtype=F32):  # grid_taps + grid_blend
    """the four taps around the pixel coordinate (ix, iy), ((a w0 + b w1) + c w2) + d w3; the bilinear and the reflection lookup both end here"""
    x0, y0 = np.floor(ix), np.floor(iy)
    tx, ty = (ix - x0).astype(dtype)[..., None], (iy - y0).astype(dtype)[..., None]
    one = dtype(1.0)
    w = ((one - tx) * (one - ty), tx * (one - ty), (one - tx) * ty, tx * ty)
    tap = lambda y, x: grid_tap(img, y, x, dtype)
    return ((tap(y0, x0) * w[0] + tap(y0, x0 + 1) * w[1]) + tap(y0 + 1, x0) * w[2]) + tap(y0 + 1, x0 + 1) * w[3]


def grid_nearest(img, ix, iy, dtype=F32):  # grid_nearest
    """one tap at rint: halves go to even, as torch's round"""
    return grid_tap(img, np.rint(iy), np.rint(ix), dtype)


# ---- nvdiffrast's linear lookup with the wrap boundary
def sample_wrap(img, gx, gy, dtype=F32):  # wrap_taps + wrap_blend
    """img [H,W,C] at the NDC (gx, gy) -> [...,C]: uv = ndc * 0.5 + 0.5, u -= floor(u), u * W - 0.5, indices wrapped, lerp(a, b, t) = a + (b - a) * t
    along u, then along v; a non-finite coordinate samples zero"""
    H, W = img.shape[:2]
    gx, gy = np.asarray(gx, dtype), np.asarray(gy, dtype)
    fin = np.isfinite(gx) & np.isfinite(gy)
    u = np.where(fin, gx, dtype(0)) * dtype(0.5) + dtype(0.5)
    v = np.where(fin, gy, dtype(0)) * dtype(0.5) + dtype(0.5)
    u, v = u - np.floor(u), v - np.floor(v)
    u, v = u * dtype(W) - dtype(0.5), v * dtype(H) - dtype(0.5)
    fu0, fv0 = np.floor(u), np.floor(v)
    fu, fv = (u - fu0)[..., None], (v - fv0)[..., None]
    iu0, iv0 = fu0.astype(np.int64), fv0.astype(np.int64)
    iu1, iv1 = iu0 + 1, iv0 + 1
    iu0, iv0 = np.where(iu0 < 0, iu0 + W, iu0), np.where(iv0 < 0, iv0 + H, iv0)
    iu1, iv1 = np.where(iu1 >= W, iu1 - W, iu1), np.where(iv1 >= H, iv1 - H, iv1)
    t = lambda y, x: img[y, x].astype(dtype)
    lerp = lambda a, b, w: (a + (b - a) * w).astype(dtype)
    out = lerp(lerp(t(iv0, iu0), t(iv0, iu1), fu), lerp(t(iv1, iu0), t(iv1, iu1), fu), fv)
    return np.where(fin[..., None], out, dtype(0)).astype(dtype)


# ---- the fronts
def sample(tex, uv, mode, dtype=F32):  # sample_view / the map lookup of utx_screen_gbuffer
    """one map [H,W,C] at uv [...,2] in [-1,1]: 'bilinear' | 'nearest' (grid_sample, zero padding) | 'nvdiffrast' (wrap)"""
    H, W = tex.shape[:2]
    gx, gy = uv[..., 0], uv[..., 1]
    if mode == "nvdiffrast":
        return sample_wrap(tex, gx, gy, dtype)
    ix, iy = grid_unnormalize(gx, W, dtype), grid_unnormalize(gy, H, dtype)
    if mode == "nearest":
        return grid_nearest(tex, ix, iy, dtype)
    assert mode == "bilinear", mode
    return grid_blend(tex, ix, iy, dtype)


def sample_planar(img, gx, gy, padding="zeros", dtype=F32):  # the lookups of utx_vertex_project
    """the planar form: img [C,H,W] at the NDC (gx, gy) [N] -> [C,N], bilinear with padding 'zeros' | 'reflection'"""
    index = reflect_index if padding == "reflection" else grid_unnormalize
    hwc = np.moveaxis(img, 0, -1)
    return np.moveaxis(grid_blend(hwc, index(gx, img.shape[2], dtype), index(gy, img.shape[1], dtype), dtype), -1, 0)


# ---- the overlay / blending epilogue of the two bakes
def bake_epilogue(acc, wacc, base, overlay_confidence, blending, blending_confidence, dtype=F32):  # sd_bake_epilogue
    """-> (overlay, blended): acc / wacc where wacc > overlay_confidence; then, where wacc <= blending_confidence, 'soft': (base * (conf - wacc) + overlay) / conf,
    'hard': base.  The thresholds are float32 values in either dtype: a float32 tensor is compared with a Python number in float32"""
    acc, wacc, base = np.asarray(acc, dtype), np.asarray(wacc, dtype), np.asarray(base, dtype)
    oc, bc = dtype(F32(overlay_confidence)), dtype(F32(blending_confidence))
    with np.errstate(divide="ignore", invalid="ignore"):
        over = np.where(wacc > oc, acc / wacc, acc)
        out = over
        if blending == "soft":
            out = np.where(wacc <= bc, (base * (bc - wacc) + over) / bc, over)
        elif blending == "hard":
            out = np.where(wacc <= bc, base, over)
    return over.astype(dtype), out.astype(dtype)

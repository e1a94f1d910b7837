"""Image-based PBR shading and tangent-space normal maps (TEST INFRASTRUCTURE ONLY): the fp64 numpy restatement (the oracle of tests/test_pbr_gpu.py and
tests/test_normal_map_gpu.py) of the cube lookup rule of include/unitex_hip.h, of the reference's lat-long conversion, its two prefilters
(c_src/cubemap.cu:110-139, 246-298), the split-sum estimator of utx_dfg_lut and PBRModel.forward (texture/pbr/pbr.py:110-130), proven in
tests/test_pbr_cpu.py against the reference's own PBRModel.forward (fixture G15, tests/golden/make_golden_pbr_shade.py: the reference's arithmetic around
the lookups; dr.texture there is this module's lookup); and of bsdf_prepare_shading_normal (two-sided, OpenGL convention; the rule in
include/unitex_hip.h), proven in tests/test_normal_map_cpu.py against the reference's own torch code (fixture G16, tests/golden/make_golden_normal_map.py)
and chained to pbr_forward, with the error bounds the GPU tests hold the kernels to; the fixture loaders.

Bounds of the shading normal, in units of u = 2^-24 (half an ulp of a value in [1, 2), as in test_pbr_gpu.test_g15_forward_and_fused_shade), absolute, first
order, every rounding taken in the same direction.  c = |cross(st, sn)|, r = |st p.x - b p.y + sn max(p.z, 0)|, both of the fp64 restatement:
  a normalised vector (dot 3, sqrt 1, divide 1)                                   5 u         (vv: one more for eye - pos, 6 u)
  cross(st, sn), per component two products of factors good to 5 u and a sum      23 u, as a vector 40 u
  b = cross / |cross|                                                              40 u / c + 5 u
  s_raw (|p| <= 1: 5 u on st and sn, |p.y| times b's, 3 products, 2 sums)          40 u (1 + |p.y| / c)
  s = s_raw / |s_raw|                                                              ds = 40 u (1 + |p.y| / c) / r + 5 u
  t = clamp(dot(vv, s) / 0.1)   (ds + 6 u + 3 u for the dot, times 10, the divide)  dt = 10 (ds + 10 u) + 2 u, and 0 where the fp64 dot / 0.1 lies
                                                                                   farther than dt outside [0, 1]: both sides clamp to the same 0 or 1
  out = g + t (s - g)                                                              (1 + |g|) dt + ds + 6 u max(1, |g|)
  r = 0 exactly (p.x = p.y = max(p.z, 0) = 0, or the frame itself is zero): the three products are exact zeros on both sides, s = 0, t = 0, out = g: ds = dt = 0
An ill-conditioned pixel (tangent nearly parallel to the normal, a perturbation near zero) gets the wider bound its own c and r give it, no pixel is
left out.  Through the shading (lights of N^2 faces with texel contrast C and maximum M, an R^2 table with contrast <= 1, kd <= 1, roughness exact):
  dn = d(out) / |out| + 5 u on the unit normal;  a direction error d moves a face coordinate by <= 2 sqrt(3) d, N / 2 texels per unit, two axes, C per
  texel: K d with K = 2 * 2 sqrt(3) * (N / 2) * C;  a lookup that snaps on one side only (rule 2 of the cube lookup) jumps by <= N 2^-21 C per axis
  diffuse  = kd * light_diffuse[n]:                       K dn + 2 N 2^-21 C
  specular = (ks FG.x + FG.y) * light_specular[wi]:       wi = 2 (wo.n) n - wo moves by 4 dn, the coefficient is <= 1.5: 1.5 (4 K dn + 2 N 2^-21 C);
             FG[c = wo.n] moves by R dn per entry, the coefficient by 1.5 R dn, times M
plus, against another evaluation of the whole chain, the 16 ulp of each output's maximum that G15 grants PBRModel.forward itself."""
import os

import numpy as np

from .pixel_ref import unit

GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
F32 = np.float32
U = 2.0 ** -24


def load_g15():
    return np.load(os.path.join(GOLD, "g15_pbr_shade.npz"), allow_pickle=False)


def load_fg_lut():
    return np.load(os.path.join(GOLD, "g15_fg_lut.npz"), allow_pickle=False)["fg_lut"]


# ---------------------------------------------------------------------------------------------------------------- cube geometry
def cube_to_dir(s, fx, fy):
    one = np.ones_like(fx)
    v = [(one, -fy, -fx), (-one, -fy, fx), (fx, one, fy), (fx, -one, -fy), (fx, -fy, one), (-fx, -fy, -one)][s]
    return np.stack(v, -1)


def texel_dirs(N):
    """unit texel-centre directions [6,N,N,3] and pixel_area [N,N] (cubemap.cu:17-46), fp64"""
    g = 2.0 * ((np.arange(N) + 0.5) / N) - 1.0
    gy, gx = np.meshgrid(g, g, indexing="ij")
    d = np.stack([cube_to_dir(s, gx, gy) for s in range(6)])
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    H = N // 2
    a = np.abs(np.arange(N) - H)
    da = np.arctan((a + 1) / H) - np.arctan(a / H)
    return d, da[:, None] * da[None, :]


def _face(d):
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    ax, ay, az = np.abs(x), np.abs(y), np.abs(z)
    mx = (ax >= ay) & (ax >= az)
    my = ~mx & (ay >= az)
    s = np.where(mx, np.where(x >= 0, 0, 1), np.where(my, np.where(y >= 0, 2, 3), np.where(z >= 0, 4, 5)))
    cx = np.choose(s, [-z, z, x, x, x, -x])
    cy = np.choose(s, [-y, -y, z, -z, -y, -y])
    cz = np.choose(s, [ax, ax, ay, ay, az, az])
    return s, cx, cy, cz


def _out_tap(N, s, x, y):
    """flat texel index of the tap (x, y) of face s seen from the face its own direction selects (rule 4), in integers"""
    a, b = 2 * x + 1 - N, 2 * y + 1 - N
    n = np.full_like(a, N)
    v = np.stack([np.choose(s, [n, -n, a, a, a, -a]), np.choose(s, [-b, -b, n, -n, -b, -b]), np.choose(s, [-a, a, b, -b, n, -n])], -1)
    s2, cx, cy, cz = _face(v)
    ix = np.clip((cx + cz) * N // (2 * cz), 0, N - 1)
    iy = np.clip((cy + cz) * N // (2 * cz), 0, N - 1)
    return (s2 * N + iy) * N + ix


def _cube_tap(flat, N, s, x, y):
    ox, oy = (x < 0) | (x >= N), (y < 0) | (y >= N)
    cx, cy = np.clip(x, 0, N - 1), np.clip(y, 0, N - 1)
    single = flat[_out_tap(N, s, x, y)]
    corner = ((flat[_out_tap(N, s, cx, y)] + flat[_out_tap(N, s, x, cy)]) + flat[(s * N + cy) * N + cx]) / 3.0
    return np.where((ox & oy)[..., None], corner, single)


def _snap(t, thr):
    b = np.floor(t)
    f = t - b
    up = f > 1.0 - thr
    return (b + up).astype(np.int64), np.where((f < thr) | up, 0.0, f)


def cube_lookup(cube, dirs):
    """the library's cube lookup rule in fp64: cube [6,N,N,C], dirs [...,3] -> [...,C]"""
    cube, d = np.asarray(cube, np.float64), np.asarray(dirs, np.float64)
    N = cube.shape[1]
    flat = cube.reshape(-1, cube.shape[-1])
    s, cx, cy, cz = _face(d)
    ok = cz > 0
    fx, fy = np.where(ok, cx / np.where(ok, cz, 1.0), 0.0), np.where(ok, cy / np.where(ok, cz, 1.0), 0.0)
    thr = min(N * 2.0 ** -21, 0.25)
    x0, wx = _snap((fx + 1.0) * (0.5 * N) - 0.5, thr)
    y0, wy = _snap((fy + 1.0) * (0.5 * N) - 0.5, thr)
    t00, t01 = _cube_tap(flat, N, s, x0, y0), _cube_tap(flat, N, s, x0 + 1, y0)
    t10, t11 = _cube_tap(flat, N, s, x0, y0 + 1), _cube_tap(flat, N, s, x0 + 1, y0 + 1)
    top = t00 + wx[..., None] * (t01 - t00)
    bot = t10 + wx[..., None] * (t11 - t10)
    return top + wy[..., None] * (bot - top)


def lut_lookup(lut, xy):
    """dr.texture(filter 'linear', boundary 'clamp') of a [R,R,C] table at xy [...,2] = (x, y) in [0, 1], fp64"""
    lut, xy = np.asarray(lut, np.float64), np.asarray(xy, np.float64)
    R = lut.shape[0]
    tx, ty = xy[..., 0] * R - 0.5, xy[..., 1] * R - 0.5
    bx, by = np.floor(tx), np.floor(ty)
    wx, wy = (tx - bx)[..., None], (ty - by)[..., None]
    c = lambda v: np.clip(v.astype(np.int64), 0, R - 1)
    t00, t01, t10, t11 = lut[c(by), c(bx)], lut[c(by), c(bx + 1)], lut[c(by + 1), c(bx)], lut[c(by + 1), c(bx + 1)]
    top, bot = t00 + wx * (t01 - t00), t10 + wx * (t11 - t10)
    return top + wy * (bot - top)


def latlong_to_cubemap(lat, N):
    """pbr.py:28-49 with dr.texture = bilinear, wrap addressing in both axes; returns (cubemap [6,N,N,3], pixel x coordinate before wrapping)"""
    lat = np.asarray(lat, np.float64)
    Hi, Wi = lat.shape[:2]
    v, _ = texel_dirs(N)
    tu = np.arctan2(v[..., 0], -v[..., 2]) / (2 * np.pi) + 0.5
    tv = np.arccos(np.clip(v[..., 1], -1, 1)) / np.pi
    px, py = tu * Wi - 0.5, tv * Hi - 0.5
    bx, by = np.floor(px), np.floor(py)
    wx, wy = (px - bx)[..., None], (py - by)[..., None]
    ix = lambda t: np.mod(t.astype(np.int64), Wi)
    iy = lambda t: np.mod(t.astype(np.int64), Hi)
    top = lat[iy(by), ix(bx)] * (1 - wx) + lat[iy(by), ix(bx + 1)] * wx
    bot = lat[iy(by + 1), ix(bx)] * (1 - wx) + lat[iy(by + 1), ix(bx + 1)] * wx
    return top * (1 - wy) + bot * wy, px


def diffuse_prefilter(cube):
    """(fp64 sums [6,N,N,3], sums of the absolute terms) of DiffuseCubemapFwdKernel"""
    cube = np.asarray(cube, np.float64)
    N = cube.shape[1]
    d, area = texel_dirs(N)
    L, c = d.reshape(-1, 3), cube.reshape(-1, 3)
    w = np.clip(L @ L.T, 0.0, 0.999) * (np.broadcast_to(area, (6, N, N)).reshape(-1) / 3.141592)[None, :]
    return (w @ c).reshape(cube.shape), (w @ np.abs(c)).reshape(cube.shape)


def specular_weights(N, roughness, cutoff):
    """(accept mask [n,n], weights [n,n], L.V [n,n]) of SpecularCubemapFwdKernel in fp64, n = 6 N^2, row = output"""
    d, area = texel_dirs(N)
    L = d.reshape(-1, 3)
    dot = L @ L.T
    acc = dot >= cutoff
    h = L[None, :, :] + L[:, None, :]
    h = h / np.maximum(np.linalg.norm(h, axis=-1, keepdims=True), 1e-300)
    vh = np.clip(np.einsum("ijk,ik->ij", h, L), 0.0, 1.0)
    a2 = float(roughness) ** 4
    dd = (vh * a2 - vh) * vh + 1.0
    w = np.maximum(dot, 0.0) * (a2 / (dd * dd * np.pi)) * np.broadcast_to(area, (6, N, N)).reshape(-1)[None, :] / 4.0
    return acc, np.where(acc, w, 0.0), dot


def specular_cutoff(N, roughness, cutoff=0.99, margin=1e-5):
    """the lobe cosine the specular tests use: ndf_cutoff's, moved down in steps of 3 margins until no texel pair has |L.V - c| < margin in fp64
    (then fp32 and fp64 accept the same set: a fp32 dot product of unit vectors is good to 4e-7); asserted, not assumed"""
    from unitex_amd.texturetools.pbr import ndf_cutoff
    d, _ = texel_dirs(N)
    L = d.reshape(-1, 3)
    dot = L @ L.T
    c = ndf_cutoff(roughness, cutoff)
    for _ in range(200):
        if np.abs(dot - c).min() >= margin:
            break
        c -= 3 * margin
    assert np.abs(dot - c).min() >= margin
    return float(F32(c)) if np.abs(dot - float(F32(c))).min() >= margin else c


def specular_prefilter(cube, roughness, cutoff):
    """(fp64 result [6,N,N,3], error scale sum|c w| / sum w, accepted count per output)"""
    cube = np.asarray(cube, np.float64)
    acc, w, _ = specular_weights(cube.shape[1], roughness, cutoff)
    c = cube.reshape(-1, 3)
    ws = w.sum(1, keepdims=True)
    return ((w @ c) / ws).reshape(cube.shape), ((w @ np.abs(c)) / ws).reshape(cube.shape), acc.sum(1).reshape(cube.shape[:3])


def dfg_lut(R, n):
    """utx_dfg_lut's estimator in fp64 (same Hammersley set, same formulas): [R,R,2], row = roughness, column = cos"""
    k = np.arange(n, dtype=np.uint32)
    rev = np.zeros(n, np.uint64)
    for b in range(32):
        rev |= ((k.astype(np.uint64) >> np.uint64(b)) & np.uint64(1)) << np.uint64(31 - b)
    x, y = k / n, rev.astype(np.float64) * 2.0 ** -32
    cp, sp = np.cos(2 * np.pi * x), np.sin(2 * np.pi * x)
    out = np.empty((R, R, 2))
    c = ((np.arange(R) + 0.5) / R)[:, None]
    vx, vz = np.sqrt(1 - c * c), c
    for j in range(R):
        rough = (j + 0.5) / R
        a = rough * rough
        a2 = a * a
        den = (1 - y) + a2 * y
        ct, st = np.sqrt((1 - y) / den)[None, :], np.sqrt(a2 * y / den)[None, :]
        vh = vx * (st * cp[None, :]) + vz * ct
        lz = 2 * vh * ct - vz
        ok = (lz > 0) & (vh > 0) & (ct > 0)
        lzs = np.where(ok, lz, 1.0)
        vis = 0.5 / (lzs * np.sqrt(vz * vz * (1 - a2) + a2) + vz * np.sqrt(lzs * lzs * (1 - a2) + a2))
        gv = np.where(ok, vis * 4 * lzs * vh / np.where(ok, ct, 1.0), 0.0)
        fc = (1 - vh) ** 5
        out[j, :, 0], out[j, :, 1] = ((1 - fc) * gv).sum(1) / n, (fc * gv).sum(1) / n
    return out


def pbr_forward(view_position, world_position, world_normal, map_Kd, map_Ks, light_diffuse, light_specular, fg_lut, lookups=False):
    """PBRModel.forward (pbr.py:110-130) in fp64 -> (diffuse, specular)"""
    f = lambda a: np.asarray(a, np.float64)
    nrm = unit(f(world_normal))
    wo = unit(f(view_position) - f(world_position))
    dn = (wo * nrm).sum(-1, keepdims=True)
    wi = unit(2 * dn * nrm - wo)
    c = np.clip(dn, 0.0, 1.0)
    albedo, rough, metal = f(map_Kd)[..., :3], f(map_Ks)[..., 1:2], f(map_Ks)[..., 2:3]
    kd = albedo * (1 - metal) + 0.0 * metal
    ks = (0.04 * (1 - metal) + albedo * metal) * (1 - 0.5) + 0.0 * 0.5
    ld, ls = cube_lookup(light_diffuse, nrm), cube_lookup(light_specular, wi)
    fg = lut_lookup(fg_lut, np.concatenate([c, rough], -1))
    out = kd * ld, (ks * fg[..., 0:1] + fg[..., 1:2]) * ls
    return out + (nrm, wi, np.concatenate([c, rough], -1), ld, ls, fg) if lookups else out



# ---------------------------------------------------------------------------------------------------------------- tangent-space normal maps
_cache = {}


def load_g16():
    if "f" not in _cache:
        _cache["f"] = dict(np.load(os.path.join(GOLD, "g16_normal_map.npz"), allow_pickle=False))
    return _cache["f"]


def shading_normal(view_pos, pos, p, smooth_nrm, smooth_tng, geom_nrm, parts=False):
    """bsdf_prepare_shading_normal(two_sided_shading=True, opengl=True) in fp64 -> out [...,3] (, the intermediates the bounds need)"""
    f = lambda a: np.asarray(a, np.float64)
    view_pos, pos, p, g = f(view_pos), f(pos), f(p), f(geom_nrm)
    sn, st, vv = unit(f(smooth_nrm)), unit(f(smooth_tng)), unit(view_pos - pos)
    c = np.cross(st, sn)
    b = unit(c)
    s_raw = st * p[..., 0:1] - b * p[..., 1:2] + sn * np.maximum(p[..., 2:3], 0.0)
    s = unit(s_raw)
    front = (g * vv).sum(-1, keepdims=True) > 0
    s, g = np.where(front, s, -s), np.where(front, g, -g)
    t_raw = (vv * s).sum(-1, keepdims=True) / 0.1
    out = g + np.clip(t_raw, 0.0, 1.0) * (s - g)
    if parts:
        return out, dict(c=np.linalg.norm(c, axis=-1), r=np.linalg.norm(s_raw, axis=-1), t_raw=t_raw[..., 0], gl=np.linalg.norm(g, axis=-1), py=np.abs(p[..., 1]),
                         gdot=(f(geom_nrm) * vv).sum(-1))
    return out


def shading_normal_bound(parts):
    """per-pixel absolute bound on a fp32 evaluation of the rule against the fp64 one (module docstring)"""
    tiny = 1e-300
    ds = 40 * U * (1 + parts["py"] / np.maximum(parts["c"], tiny)) / np.maximum(parts["r"], tiny) + 5 * U
    ds = np.where(parts["r"] == 0, 0.0, ds)
    dt = 10 * (ds + 10 * U) + 2 * U
    dt = np.where((parts["t_raw"] <= -dt) | (parts["t_raw"] >= 1 + dt) | (parts["r"] == 0), 0.0, dt)
    return (1 + parts["gl"]) * dt + ds + 6 * U * np.maximum(1.0, parts["gl"])


def shade_bounds(d_out, out, N, contrast, light_max, R):
    """(diffuse, specular) per-pixel bounds from the bound d_out on the un-normalised shading normal `out` (module docstring), without the 16 ulp"""
    dn = d_out / np.maximum(np.linalg.norm(out, axis=-1), 1e-300) + 5 * U
    K = 2 * 2 * np.sqrt(3.0) * (N / 2) * contrast
    snap = 2 * N * 2.0 ** -21 * contrast
    return K * dn + snap, 1.5 * (4 * K * dn + snap) + 1.5 * R * dn * light_max


def g16_oracle():
    """the restatement on G16's dense inputs, once: out, parts, bound, diffuse, specular, their bounds"""
    if "o" not in _cache:
        f = load_g16()
        out, parts = shading_normal(f["view_position"], f["world_position"], f["perturbed_nrm"], f["smooth_nrm"], f["smooth_tng"], f["geom_nrm"], parts=True)
        bound = shading_normal_bound(parts)
        d, s = pbr_forward(f["view_position"], f["world_position"], out, f["map_Kd"], f["map_Ks"], f["light_diffuse"], f["light_specular"], f["fg_lut"])
        bd, bs = shade_bounds(bound, out, 8, 2.0, 4.0, 16)
        ulp = lambda x: float(np.spacing(F32(np.abs(x).max())))
        _cache["o"] = dict(out=out, parts=parts, bound=bound, diffuse=d, specular=s, bound_diffuse=bd + 16 * ulp(d), bound_specular=bs + 16 * ulp(s))
    return _cache["o"]

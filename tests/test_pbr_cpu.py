"""Image-based PBR shading, CPU side: the fp64 numpy restatement (the oracle of tests/test_pbr_gpu.py) of the cube lookup rule of
include/unitex_hip.h, of the reference's lat-long conversion, its two prefilters (c_src/cubemap.cu:110-139, 246-298), the split-sum estimator of
utx_dfg_lut and PBRModel.forward (texture/pbr/pbr.py:110-130), proven here against the reference's own PBRModel.forward (fixture G15,
tests/golden/make_golden_pbr_shade.py: the reference's arithmetic around the lookups; dr.texture there is this module's lookup); the fixture loaders,
read_hdr and ndf_cutoff."""
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
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


def _normalize(v):
    return v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-12)


def pbr_forward(view_position, world_position, world_normal, map_Kd, map_Ks, light_diffuse, light_specular, fg_lut, lookups=False):
    """PBRModel.forward (pbr.py:110-130) in fp64 -> (diffuse, specular)"""
    f = lambda a: np.asarray(a, np.float64)
    nrm = _normalize(f(world_normal))
    wo = _normalize(f(view_position) - f(world_position))
    dn = (wo * nrm).sum(-1, keepdims=True)
    wi = _normalize(2 * dn * nrm - wo)
    c = np.clip(dn, 0.0, 1.0)
    albedo, rough, metal = f(map_Kd)[..., :3], f(map_Ks)[..., 1:2], f(map_Ks)[..., 2:3]
    kd = albedo * (1 - metal) + 0.0 * metal
    ks = (0.04 * (1 - metal) + albedo * metal) * (1 - 0.5) + 0.0 * 0.5
    ld, ls = cube_lookup(light_diffuse, nrm), cube_lookup(light_specular, wi)
    fg = lut_lookup(fg_lut, np.concatenate([c, rough], -1))
    out = kd * ld, (ks * fg[..., 0:1] + fg[..., 1:2]) * ls
    return out + (nrm, wi, np.concatenate([c, rough], -1), ld, ls, fg) if lookups else out


# ---------------------------------------------------------------------------------------------------------------- tests
def test_fixture_loaders():
    f = load_g15()
    assert f["world_position"].shape == (32, 32, 3) and f["world_normal"].shape == (32, 32, 3) and f["diffuse"].shape == (32, 32, 3)
    assert f["light_diffuse"].shape == (6, 8, 8, 3) and f["light_specular"].shape == (6, 8, 8, 3) and f["fg_lut"].shape == (16, 16, 2)
    ks = f["map_Ks"]
    assert (ks[..., 1] == 0).any() and (ks[..., 1] == 1).any() and (ks[..., 2] == 0).any() and (ks[..., 2] == 1).any()
    n = f["world_normal"]
    wo = f["view_position"].reshape(1, 1, 3) - f["world_position"]
    assert ((n * wo).sum(-1) < 0).any() and np.abs(np.linalg.norm(n, axis=-1) - 1).max() > 0.1, "back-facing and un-normalised normals"
    lut = load_fg_lut()
    assert lut.shape == (256, 256, 2) and lut.dtype == np.float32 and np.isfinite(lut).all()


def test_oracle_reproduces_the_references_forward():
    """G15's diffuse / specular are the reference's own PBRModel.forward in fp32 torch; the fp64 restatement agrees to 1e-6 relative (of each output's maximum).
    Measured: diffuse 8.8e-8, specular 9.2e-7.  What is left is the reference's own rounding: it carries the reflection vector in fp32 (2.3e-7 from the fp64 one),
    and a direction error d moves a bilinear lookup on an 8^2 face by about N / 2 * d * (texel contrast); on the lookups the reference itself made (stored in
    the fixture) the arithmetic around them agrees to 7.2e-8.  A first fixture with lights uniform in [0, 4) (twice the contrast) reached 1.10e-6 from that
    rounding alone, which is why the generator bounds the contrast by half the maximum and says so (tests/golden/make_golden_pbr_shade.py)."""
    f = load_g15()
    d, s, nrm, wi, cr, _, _, _ = pbr_forward(f["view_position"], f["world_position"], f["world_normal"], f["map_Kd"], f["map_Ks"], f["light_diffuse"],
                                            f["light_specular"], f["fg_lut"], lookups=True)
    # the lookup coordinates are the reference's to fp32 rounding: two normalisations (nrm: 4 u), the reflection and a third (wi: 8 u, in units of 2^-24)
    for got, name, bound in ((nrm, "diffuse_coord", 4 * U), (wi, "specular_coord", 8 * U), (cr, "fg_coord", 4 * U)):
        print(name, "max difference", np.abs(got - f[name]).max())
        assert np.abs(got - f[name]).max() <= bound, name
    # the arithmetic around the lookups, on the lookups the reference made
    al, m = f["map_Kd"].astype(np.float64), f["map_Ks"][..., 2:3].astype(np.float64)
    fg, ld, ls = (f[k].astype(np.float64) for k in ("fg_lookup", "diffuse_lookup", "specular_lookup"))
    for got, name in (((al * (1 - m)) * ld, "diffuse"), (((0.04 * (1 - m) + al * m) * 0.5 * fg[..., 0:1] + fg[..., 1:2]) * ls, "specular")):
        err = np.abs(got - f[name]).max() / np.abs(f[name]).max()
        print(name, "around the stored lookups: max relative difference", err)
        assert err <= 1e-6, name
    for got, name in ((d, "diffuse"), (s, "specular")):
        err = np.abs(got - f[name]).max() / np.abs(f[name]).max()
        print(name, "max relative difference", err)
        assert err <= 1e-6, name


def _write_hdr(path, rgbe, rle):
    h, w = rgbe.shape[:2]
    body = b""
    for y in range(h):
        if rle:
            body += bytes([2, 2, w >> 8, w & 255])
            for c in range(4):
                row, x = rgbe[y, :, c], 0
                while x < w:
                    run = 1
                    while x + run < w and run < 127 and row[x + run] == row[x]:
                        run += 1
                    if run >= 3:
                        body += bytes([128 + run, int(row[x])])
                    else:
                        run = min(5, w - x)
                        body += bytes([run]) + row[x:x + run].tobytes()
                    x += run
        else:
            body += rgbe[y].tobytes()
    open(path, "wb").write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n-Y %d +X %d\n" % (h, w) + body)


@pytest.mark.parametrize("rle", [False, True])
def test_read_hdr_round_trip(tmp_path, rle):
    from unitex_amd.texturetools.pbr import read_hdr
    rng = np.random.default_rng(3)
    rgbe = rng.integers(0, 256, (5, 12, 4)).astype(np.uint8)
    rgbe[..., 3] = rng.integers(120, 136, (5, 12))
    rgbe[1, 2:9] = rgbe[1, 2]          # a run for the RLE writer
    rgbe[0, 0, 3] = 0                  # exponent 0 = black
    p = str(tmp_path / "t.hdr")
    _write_hdr(p, rgbe, rle)
    want = rgbe[..., :3].astype(np.float64) * np.where(rgbe[..., 3:] > 0, 2.0 ** (rgbe[..., 3:].astype(np.float64) - 136), 0.0)
    got = read_hdr(p)
    assert got.dtype == np.float32 and got.shape == (5, 12, 3) and np.array_equal(got, want.astype(np.float32))
    open(str(tmp_path / "bad.hdr"), "wb").write(b"P6\n")
    with pytest.raises(ValueError):
        read_hdr(str(tmp_path / "bad.hdr"))


def test_ndf_cutoff():
    """the cosine search of __ndfBounds: the lobe narrows with the roughness, the returned cosine is a sample of the grid and holds the asked mass"""
    from unitex_amd.texturetools.pbr import ndf_cutoff
    c008, c05 = ndf_cutoff(0.08, 0.99), ndf_cutoff(0.5, 0.99)
    assert 0.0 < c05 < c008 < 1.0
    grid = np.cos(np.linspace(0, np.pi / 2.0, 1000000))
    for r, c in ((0.08, c008), (0.5, c05)):
        i = int(np.argmin(np.abs(grid - c)))
        assert grid[i] == c
        a2 = r ** 4
        D = np.cumsum(a2 / ((((grid * a2 - grid) * grid + 1.0) ** 2) * np.pi))
        assert D[i] >= 0.99 * D[-1] > D[i - 1]
    assert ndf_cutoff(0.5, 0.5) > c05


def test_cube_rule_is_continuous_and_exact_at_centres():
    """the fp64 rule itself: texel centres return their texel, the value is continuous across every edge and corner"""
    rng = np.random.default_rng(5)
    N = 4
    cube = rng.uniform(0, 1, (6, N, N, 3))
    d, _ = texel_dirs(N)
    assert np.array_equal(cube_lookup(cube, d), cube)
    pts = rng.uniform(-1, 1, (4000, 3))
    pts[:1500, 0] = np.sign(pts[:1500, 0])
    pts[:1500, 1] = np.sign(pts[:1500, 1])                       # on an edge between an x and a y face
    pts[:300, 2] = np.sign(pts[:300, 2])                         # at a corner
    perm = np.stack([np.roll(pts, k, axis=1) for k in range(3)]).reshape(-1, 3)
    eps = 1e-9
    for axis in range(3):
        e = np.zeros(3)
        e[axis] = eps
        assert np.abs(cube_lookup(cube, perm * (1 + e)) - cube_lookup(cube, perm * (1 - e))).max() < 1e-6


def test_specular_cutoff_has_its_margin():
    for r in (0.5, 0.08):
        c = specular_cutoff(16, r)
        _, _, dot = specular_weights(16, r, c)
        assert np.abs(dot - c).min() >= 1e-5
    acc, _, _ = specular_weights(16, 0.08, specular_cutoff(16, 0.08))
    assert (acc.sum(1) == 1).any(), "at roughness 0.08 some lobes hold a single texel"


def test_cubemap_table_matches_the_oracle():
    """utx_cubemap_table is host code: directions and pixel_area are the fp64 values rounded once; odd N is refused; the tile bound is conservative"""
    from unitex_amd.texturetools import ops
    for N in (8, 16, 34):
        c = 0.97
        tex, tiles = ops.cubemap_tables(N, c, "cpu")
        d, area = texel_dirs(N)
        assert np.array_equal(tex[..., :3].numpy(), d.astype(F32)) and np.array_equal(tex[..., 3].numpy(), np.broadcast_to(area, (6, N, N)).astype(F32))
        nt = (N + 15) // 16
        L = d.reshape(-1, 3)
        for t in range(6 * nt * nt):
            s, ty, tx = t // (nt * nt), (t // nt) % nt, t % nt
            inside = d[s, ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16].reshape(-1, 3)
            reach = ((L @ inside.T) >= c).any(1)
            axis, thr = tiles.reshape(-1, 4)[t, :3].numpy().astype(np.float64), float(tiles.reshape(-1, 4)[t, 3])
            assert ((L @ axis)[reach] >= thr + 5e-6).all()
    with pytest.raises(ValueError):
        ops.cubemap_tables(7, None, "cpu")

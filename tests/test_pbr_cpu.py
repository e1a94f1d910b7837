"""Image-based PBR shading, CPU side: the fp64 numpy restatement of oracle/pbr_ref.py (the oracle of tests/test_pbr_gpu.py: the cube lookup rule, the
lat-long conversion, the two prefilters, utx_dfg_lut's estimator and PBRModel.forward) proven against the reference's own PBRModel.forward (fixture G15,
tests/golden/make_golden_pbr_shade.py: the reference's arithmetic around the lookups; dr.texture there is the oracle's lookup); the fixture loaders,
read_hdr and ndf_cutoff."""
import numpy as np
import pytest

from oracle.pbr_ref import F32, U, cube_lookup, load_fg_lut, load_g15, pbr_forward, specular_cutoff, specular_weights, texel_dirs


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

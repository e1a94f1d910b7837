"""GPU tests of the geometry sampling for the field stage (csrc/sampling.hip through the C ABI): exact farthest-point sampling, the equal-steps edge
sampler and the surface sampler against the numpy restatements of oracle/sampling_ref.py (pinned in tests/test_sampling_cpu.py to the reference's run, fixture G14, to the
Random123 vectors and to a hand-worked example), and RGBTextureFullPipelineBase.sampling_on_mesh end to end.  Everything float is compared BIT FOR BIT
unless a test says why not."""
import os
import types

import numpy as np
import pytest
import torch

from oracle import sampling_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32


def _cu(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda().contiguous()


def _bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _fps_case(name):
    """-> pos [N,3] f32, M, mask | None, start"""
    rng = np.random.default_rng(sum(name.encode()))
    rnd = lambda n: rng.uniform(-1, 1, (n, 3)).astype(F32)
    if name == "single":
        return rnd(1), 1, None, 0
    if name.startswith("exhaust"):            # around one wave row of quads (256 points) and around one workgroup's 512 quads (2048 points): M = N empties the set
        n = int(name[7:])
        return rnd(n), n, None, 0
    if name == "ragged":                      # several workgroups, N = 1 mod 4
        return rnd(70001), 300, None, 0
    if name == "lattice":                     # exact ties everywhere: the tie rule's test
        g = np.stack(np.meshgrid(np.arange(9), np.arange(9), np.arange(9), indexing="ij"), -1).reshape(-1, 3).astype(F32)
        return g, 729, None, 0
    if name == "masked":                      # 50 % mask, more picks than candidates: the tail is -1
        return rnd(4096), 2500, (rng.random(4096) < 0.5).astype(np.uint8), 0
    if name == "start_last":
        return rnd(1000), 20, None, 999
    if name == "start_auto":                  # start = -1 with the first 100 points masked out
        m = np.ones(1000, np.uint8)
        m[:100] = 0
        return rnd(1000), 20, m, -1
    if name == "start_masked":                # a start that is no candidate counts as -1
        m = np.ones(1000, np.uint8)
        m[:100] = 0
        return rnd(1000), 20, m, 50
    if name == "nan":
        p = rnd(1000)
        p[317, 1] = np.nan
        p[5, 0] = np.inf
        return p, 1000, None, 0
    if name == "duplicates":                  # coincident points are picked last, with d2 = 0, each index once
        p = rnd(300)
        return np.concatenate([p, p[:100]]), 400, None, 0
    if name == "many_groups":
        return rnd(300000), 64, None, 0
    # several workgroups and a start that is not the lowest candidate: every workgroup has to agree on the first pick without reading what another one writes
    if name == "many_groups_start_last":
        return rnd(300000), 64, None, 299999
    if name == "many_groups_start_mid":       # the start's owner is neither the first nor the last workgroup
        return rnd(300000), 64, None, 123457
    if name == "many_groups_start_masked":    # a masked-out start, and a non-finite one, count as -1: the lowest candidate is index 100
        m = np.ones(300000, np.uint8)
        m[:100] = 0
        m[299999] = 0
        return rnd(300000), 64, m, 299999
    if name == "many_groups_start_nan":
        p = rnd(300000)
        p[299999, 2] = np.nan
        return p, 64, None, 299999
    raise KeyError(name)


FPS_CASES = ["single", "exhaust255", "exhaust256", "exhaust257", "exhaust2047", "exhaust2048", "exhaust2049", "ragged", "lattice", "masked", "start_last",
             "start_auto", "start_masked", "nan", "duplicates", "many_groups", "many_groups_start_last",
             "many_groups_start_mid", "many_groups_start_masked", "many_groups_start_nan"]


@pytest.mark.parametrize("name", FPS_CASES)
def test_fps_equals_the_restatement_index_for_index(name):
    from unitex_amd.texturetools import ops
    pos, M, mask, start = _fps_case(name)
    want_idx, want_d2 = R.fps_ref(pos, M, mask, start)
    dpos, dmask = _cu(pos), (_cu(mask) if mask is not None else None)
    idx, d2 = ops.fps(dpos, M, mask=dmask, start=start, want_d2=True)
    idx, d2 = idx.cpu().numpy(), d2.cpu().numpy()
    print("%s: N = %d, M = %d, picked %d" % (name, len(pos), M, int((idx >= 0).sum())))
    assert np.array_equal(idx, want_idx), "first difference at pick %d" % int(np.flatnonzero(idx != want_idx)[0])
    assert np.array_equal(_bits(d2), _bits(want_d2))
    picked = idx[idx >= 0]
    assert len(np.unique(picked)) == len(picked)
    if name == "masked":
        assert (idx[int(mask.sum()):] == -1).all() and (d2[int(mask.sum()):] == -1).all() and mask[picked].all()
    if name == "nan":
        assert len(picked) == 998 and 317 not in picked and 5 not in picked
    if name == "duplicates":
        assert (d2[300:] == 0).all() and (d2[1:300] > 0).all()
    # a second run is byte-identical, and the index-only call gives the same picks
    idx2, d22 = ops.fps(dpos, M, mask=dmask, start=start, want_d2=True)
    assert torch.equal(idx2.cpu(), torch.from_numpy(idx)) and np.array_equal(_bits(d22.cpu().numpy()), _bits(d2))
    assert np.array_equal(ops.fps(dpos, M, mask=dmask, start=start).cpu().numpy(), idx)


def test_fps_front_end_takes_numpy_and_refuses_bad_arguments():
    from unitex_amd.texturetools import ops
    from unitex_amd.texturetools.sampling import farthest_point_sampling
    pos = _fps_case("start_last")[0]
    want = R.fps_ref(pos, 20, None, 0)
    got = farthest_point_sampling(pos, 20, return_d2=True)
    assert isinstance(got[0], np.ndarray) and np.array_equal(got[0], want[0]) and np.array_equal(_bits(got[1]), _bits(want[1]))
    assert np.array_equal(farthest_point_sampling(_cu(pos), 20).cpu().numpy(), want[0])
    off = _cu(np.concatenate([np.zeros((1, 3), F32), pos]))[1:]            # a view whose storage is not 16-byte aligned
    assert off.data_ptr() % 16 != 0 and np.array_equal(ops.fps(off, 20).cpu().numpy(), want[0])
    for M, start, msg in ((0, 0, "n_samples"), (-3, 0, "n_samples"), (4, 1000, "start"), (4, -2, "start")):
        with pytest.raises(ValueError, match=msg):
            ops.fps(_cu(pos), M, start=start)
    ctx = ops.get_ctx(0)
    wb = ctx.lib.utx_fps_workspace_bytes(1000)
    work, out, dpos = torch.empty(wb, dtype=torch.uint8, device="cuda"), torch.empty(4, dtype=torch.int32, device="cuda"), _cu(pos)
    rc = ctx.lib.utx_fps(ctx.handle, ops.ptr(dpos), None, 1000, 4, 1000, ops.ptr(out), None, ops.ptr(work), wb, ctx.stream())
    assert rc == -2 and b"utx_fps" in ctx.lib.utx_last_error(ctx.handle)


def test_edge_sampling_on_the_staircase_equals_the_reference_run():
    from unitex_amd.texturetools import sampling
    g = R.g14()
    v, f = _cu(g["stair_verts"]), _cu(g["stair_faces"])
    edges, nonman, sharp = sampling.select_sharp_edges(v, f, None, 15.0)
    assert np.array_equal(edges.cpu().numpy(), g["stair_edges"])
    assert np.array_equal(nonman.cpu().numpy(), g["stair_nonmanifold_15"]) and np.array_equal(sharp.cpu().numpy(), g["stair_sharp_15"])
    samples, edge_index, edge_t = sampling.select_and_sample_on_edges(v, f, normals=None, method="equal_steps", angle_threhold_deg=15.0, N=1000)
    assert samples.shape == (1000, 3) and edge_index.dtype == torch.int64 and edge_t.shape == (1000, 1)
    assert np.array_equal(edge_index.cpu().numpy(), g["stair_edge_index"])
    assert np.array_equal(_bits(edge_t.cpu().numpy()[:, 0]), _bits(g["stair_edge_t"]))
    assert np.array_equal(_bits(samples.cpu().numpy()), _bits(g["stair_samples"]))
    # N = 1 is linspace's first end: the start of the first selected edge (w = 0 -> its second vertex)
    s1, e1, t1 = sampling.select_and_sample_on_edges(v, f, N=1)
    want = R.sample_edges_ref(g["stair_verts"], *R.edge_tables(g["stair_verts"], g["stair_edges"], g["stair_nonmanifold_15"] | g["stair_sharp_15"]), 1)
    assert np.array_equal(_bits(s1.cpu().numpy()), _bits(want[0])) and e1.item() == want[1][0] and t1.item() == 0.0


def _torus_edge_samples(N=5000):
    from unitex_amd.texturetools import sampling
    g = R.g14()
    v, e = g["torus_verts"], g["torus_edges"]
    mask = g["torus_nonmanifold_5"] | g["torus_sharp_5"]
    samples, edge_index, edge_t = sampling.sample_on_edges_equal_steps(_cu(v), _cu(e, torch.int64), _cu(mask), N=N)
    return v, e, mask, samples.cpu().numpy().astype(np.float64), edge_index.cpu().numpy()


def test_edge_sampling_on_the_torus_lies_within_1e_6_of_the_reported_segments():
    """Prefix rounding of 4560 inexact lengths depends on the summation order, so the check is float64 geometry, no sample exempt: every sample within 1e-6
    of the segment of the edge it reports.

    This is the test of the kernel's clamp of w to [0, 1].  With the reference's unclamped w = (t - start[e]) / length[e] (measured on the MI355X and,
    identically, with the numpy restatement): 4999 of 5000 samples within 1.5e-7 of their segment, one 6.754e-6 beyond its edge's end point, on the edge's
    line, with w = 1.0002354 -- the selected lengths sum to 185.51, where one float32 step is 1.53e-5, and start[e + 1] is the ROUNDED running sum, so a t
    just below it can exceed start[e] + length[e] by up to half that step.  What is left with the clamp is the float32 rounding of w * v0 + (1 - w) * v1 on
    coordinates of magnitude about 1: a few 1e-7."""
    v, e, mask, samples, edge_index = _torus_edge_samples()
    a, b = v[e[edge_index, 0]].astype(np.float64), v[e[edge_index, 1]].astype(np.float64)
    ab = b - a
    u = ((samples - a) * ab).sum(1) / (ab * ab).sum(1)
    dist = np.linalg.norm(samples - (a + np.clip(u, 0.0, 1.0)[:, None] * ab), axis=1)
    line = np.linalg.norm(samples - (a + u[:, None] * ab), axis=1)
    print("torus edges: max distance to the reported segment %.3e (to its line %.3e), %d of %d samples beyond 1e-6" % (dist.max(), line.max(), int((dist > 1e-6).sum()), len(dist)))
    assert dist.max() <= 1e-6


def test_edge_sampling_on_the_torus_reports_selected_edges_in_equal_steps():
    N = 5000
    v, e, mask, samples, edge_index = _torus_edge_samples(N)
    assert mask[edge_index].all()
    length = np.linalg.norm(v[e[:, 1]].astype(np.float64) - v[e[:, 0]].astype(np.float64), axis=1)[mask]
    expect = length / length.sum() * (N - 1)
    count = np.bincount(edge_index, minlength=len(e))[mask]
    print("torus edges: max |count - expected| %.4f" % np.abs(count - expect).max())
    assert np.abs(count - expect).max() <= 1.0
    assert (np.diff(edge_index) >= 0).all()


def _zero_area_mesh():
    g = R.g14()
    v, f = g["stair_verts"], g["stair_faces"]
    f = np.concatenate([f[:11], np.array([[3, 3, 9]], np.int32), f[11:]])          # face 11 is degenerate: weight 0
    return v, f


@pytest.mark.parametrize("case", ["torus4096", "one", "zero_area"])
def test_surface_sampling_equals_the_restatement(case):
    from unitex_amd.texturetools import ops
    g = R.g14()
    if case == "zero_area":
        (v, f), N, seed = _zero_area_mesh(), 3000, 7
    else:
        v, f, N, seed = g["torus_verts"], g["torus_faces"], (4096 if case == "torus4096" else 1), (666 if case == "torus4096" else (5 << 32) | 9)
    cum = R.face_weights_cum(v, f)
    want = R.sample_surface_ref(v, f, cum, N, seed)
    got = [t.cpu().numpy() for t in ops.sample_surface(_cu(v), _cu(f), _cu(cum), N, seed)]
    assert np.array_equal(got[1], want[1])
    assert np.array_equal(_bits(got[2]), _bits(want[2])) and np.array_equal(_bits(got[0]), _bits(want[0]))
    if case == "zero_area":
        assert cum[11] == cum[10] and 11 not in got[1] and len(np.unique(got[1])) == len(f) - 1
    again = ops.sample_surface(_cu(v), _cu(f), _cu(cum), N, seed)[0].cpu().numpy()
    assert np.array_equal(_bits(again), _bits(got[0]))
    if case == "torus4096":         # another seed is another stream; the front end draws from the same one
        from unitex_amd.texturetools.sampling import sample_surface
        assert not np.array_equal(ops.sample_surface(_cu(v), _cu(f), _cu(cum), N, seed + 1)[1].cpu().numpy(), got[1])
        s, fi, uvw = sample_surface(_cu(v), _cu(f, torch.int64), None, N=N, seed=seed)
        assert fi.dtype == torch.int64 and np.array_equal(_bits(uvw.cpu().numpy()), _bits(want[2]))
        assert (fi.cpu().numpy() != want[1]).mean() < 0.01          # weights computed on the device may round a boundary the other way; (u, v) cannot differ


def _sampling_on_mesh(tmp_path, verts, faces, **kw):
    from unitex_amd.pipeline import RGBTextureFullPipelineBase
    from unitex_amd.texturetools import meshes
    obj = str(tmp_path / "mesh.obj")
    meshes.save_obj(obj, verts, faces)
    RGBTextureFullPipelineBase.sampling_on_mesh(types.SimpleNamespace(inverse_renderer=None), str(tmp_path), obj, **kw)
    names = ("sharp_pcd", "coarse_pcd", "sharp_pcd_fps", "coarse_pcd_fps")
    assert all(os.path.isfile(str(tmp_path / (n + ".ply"))) for n in names)
    return {n: meshes.load_ply(str(tmp_path / (n + ".ply")), faces_required=False)[0] for n in names}


def test_sampling_on_mesh_writes_the_four_clouds(tmp_path):
    g = R.g14()
    out = _sampling_on_mesh(tmp_path, g["torus_verts"], g["torus_faces"], N=2000, N_fps=256, angle=5.0)
    assert out["sharp_pcd"].shape == (2000, 3) and out["coarse_pcd"].shape == (2000, 3)
    for key in ("sharp_pcd", "coarse_pcd"):
        thin, full = out[key + "_fps"], out[key]
        assert thin.shape == (256, 3) and np.isfinite(thin).all()
        rows = {r.tobytes() for r in full}
        assert all(r.tobytes() in rows for r in thin)
        assert np.array_equal(thin[0], full[0])              # the defined start: index 0
        assert len({r.tobytes() for r in thin}) == 256
    # the thinned surface cloud spreads: its closest pair is farther apart than the closest pair of the first 256 samples
    def closest(p):
        d = np.linalg.norm(p[:, None].astype(np.float64) - p[None].astype(np.float64), axis=-1)
        return d[np.triu_indices(len(p), 1)].min()
    assert closest(out["coarse_pcd_fps"]) > 4 * closest(out["coarse_pcd"][:256])


def test_sampling_on_mesh_without_sharp_edges_falls_back_to_ones(tmp_path):
    from unitex_amd.texturetools.meshes import closed_sphere
    v, f = closed_sphere(48, 24)
    out = _sampling_on_mesh(tmp_path, v, f, N=2000, N_fps=256, angle=60.0)
    assert out["sharp_pcd"].shape == (0, 3)
    assert out["sharp_pcd_fps"].shape == (256, 3) and (out["sharp_pcd_fps"] == 1.0).all()
    assert out["coarse_pcd_fps"].shape == (256, 3) and np.abs(np.linalg.norm(out["coarse_pcd"], axis=1) - 1).max() < 0.02

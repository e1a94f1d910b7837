"""Geometry sampling for the field stage, the part that needs no GPU: the edge selection against the reference's own run (fixture G14,
tests/golden/make_golden_sampling.py), the PLY point-cloud writer, and the numpy restatements of oracle/sampling_ref.py, each pinned HERE before
tests/test_sampling_gpu.py leans on it: the equal-steps sampler to G14's captured samples bit for bit, Philox4x32-10 to the Random123 known-answer
vectors, the farthest-point sampling to an example worked by hand."""
import numpy as np
import pytest
import torch

from oracle.sampling_ref import F32, edge_tables, face_weights_cum, fps_ref, g14, philox4x32_10, sample_edges_ref, sample_surface_ref


# ---- tests ----
@pytest.mark.parametrize("mesh", ["stair", "torus"])
@pytest.mark.parametrize("deg", [15, 5])
def test_select_sharp_edges_equals_the_reference_run(mesh, deg):
    from unitex_amd.texturetools.sampling import select_sharp_edges
    g = g14()
    v, f = torch.from_numpy(g[mesh + "_verts"]), torch.from_numpy(g[mesh + "_faces"])
    edges, nonman, sharp = select_sharp_edges(v, f, None, angle_threhold_deg=float(deg))
    assert edges.dtype == torch.int64 and nonman.dtype == torch.bool and sharp.dtype == torch.bool
    assert np.array_equal(edges.numpy(), g[mesh + "_edges"])
    assert np.array_equal(nonman.numpy(), g["%s_nonmanifold_%d" % (mesh, deg)])
    assert np.array_equal(sharp.numpy(), g["%s_sharp_%d" % (mesh, deg)])
    # given normals take the same path
    fl = f.long()
    n = torch.nn.functional.normalize(torch.linalg.cross(v[fl[:, 1]] - v[fl[:, 0]], v[fl[:, 2]] - v[fl[:, 0]], dim=-1), dim=-1)
    e2, n2, s2 = select_sharp_edges(v, f, n, angle_threhold_deg=float(deg))
    assert torch.equal(e2, edges) and torch.equal(n2, nonman) and torch.equal(s2, sharp)


def test_fixture_meshes_hold_what_they_were_built_for():
    g = g14()
    e, v = g["stair_edges"], g["stair_verts"]
    assert np.array_equal(v * 64, np.round(v * 64))
    assert g["stair_nonmanifold_15"].sum() == 8 and g["stair_sharp_15"].sum() == 16 and len(e) == 40      # 16 coplanar interior edges come out not sharp
    order = np.lexsort((e[:, 1], e[:, 0]))
    assert np.array_equal(order, np.arange(len(e))) and np.all(e[:, 0] < e[:, 1])
    assert g["torus_sharp_15"].sum() == 0 and g["torus_sharp_5"].sum() > 0 and g["torus_nonmanifold_5"].sum() == 0


def test_equal_steps_restatement_equals_the_reference_run_bit_for_bit():
    g = g14()
    v, e = g["stair_verts"], g["stair_edges"]
    mask = g["stair_nonmanifold_15"] | g["stair_sharp_15"]
    sel, ids, start, length, total = edge_tables(v, e, mask)
    assert total == 10.0 and set(length.tolist()) == {0.25, 0.5, 0.75}
    samples, edge_index, edge_t = sample_edges_ref(v, sel, ids, start, length, total, 1000)
    assert np.array_equal(edge_index, g["stair_edge_index"])
    assert np.array_equal(edge_t.view(np.uint32), g["stair_edge_t"].view(np.uint32))
    assert np.array_equal(samples.view(np.uint32), g["stair_samples"].view(np.uint32))
    assert mask[edge_index].all() and edge_index[0] == ids[0] and edge_index[-1] == ids[-1]


def test_philox_restatement_reproduces_the_known_answer_vectors():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        got = philox4x32_10(np.array(ctr, np.uint32), np.array(key, np.uint32))
        assert tuple(int(x) for x in got) == want, [hex(int(x)) for x in got]
    # vectorised over samples = one at a time
    ctr = np.zeros((5, 4), np.uint32)
    ctr[:, 0] = np.arange(5)
    key = np.broadcast_to(np.array([666, 0], np.uint32), (5, 2))
    many = philox4x32_10(ctr, key)
    assert all(np.array_equal(many[i], philox4x32_10(ctr[i], key[i])) for i in range(5))


def test_surface_restatement_stays_on_the_faces_it_reports():
    g = g14()
    v, f = g["torus_verts"], g["torus_faces"]
    cum = face_weights_cum(v, f)
    samples, face, uvw = sample_surface_ref(v, f, cum, 2000, 666)
    assert uvw.min() >= 0 and np.abs(uvw.sum(1) - 1).max() < 1e-6 and face.min() >= 0 and face.max() < len(f)
    want = (v[f[face]].astype(np.float64) * uvw[..., None].astype(np.float64)).sum(1)
    assert np.abs(samples - want).max() < 1e-6
    share = np.bincount(face, minlength=len(f)) / 2000.0          # area-weighted: the picks follow the weights (loose: 2000 draws over 9216 faces, summed in 16 bands)
    w = np.diff(np.concatenate([[0.0], cum.astype(np.float64)])) / float(cum[-1])
    assert np.abs(share.reshape(16, -1).sum(1) - w.reshape(16, -1).sum(1)).max() < 0.03


@pytest.mark.parametrize("colors", [False, True])
def test_save_ply_round_trips_through_load_ply(tmp_path, colors):
    from unitex_amd.texturetools import meshes
    rng = np.random.default_rng(3)
    v = rng.standard_normal((257, 3)).astype(F32)
    c = rng.integers(0, 256, (257, 3)).astype(np.uint8) if colors else None
    p = str(tmp_path / "cloud.ply")
    meshes.save_ply(p, v, c)
    got_v, got_f, got_uv = meshes.load_ply(p, faces_required=False)
    assert np.array_equal(got_v.view(np.uint32), v.view(np.uint32)) and got_f.shape == (0, 3) and got_uv is None
    blob = open(p, "rb").read()
    head, body = blob[:blob.index(b"end_header\n") + 11], blob[blob.index(b"end_header\n") + 11:]
    assert head.startswith(b"ply\nformat binary_little_endian 1.0\n") and b"element vertex 257\n" in head and b"element face" not in head
    assert len(body) == 257 * (15 if colors else 12)
    if colors:
        rec = np.frombuffer(body, dtype=np.dtype([("p", "<f4", (3,)), ("c", "u1", (3,))]))
        assert np.array_equal(rec["c"], c) and np.array_equal(rec["p"], v)
    with pytest.raises(ValueError):          # a point cloud is still no mesh
        meshes.load_mesh(p)
    meshes.save_ply(p, np.zeros((0, 3), F32))
    assert meshes.load_ply(p, faces_required=False)[0].shape == (0, 3)
    with pytest.raises(ValueError):
        meshes.save_ply(p, v, np.zeros((3, 3), np.uint8))


def test_fps_restatement_on_a_hand_checked_example():
    # six points on a line: x = 0, 10, 4, 4 (a duplicate), 20 (masked out), 7
    pos = np.zeros((6, 3), F32)
    pos[:, 0] = [0, 10, 4, 4, 20, 7]
    mask = np.array([1, 1, 1, 1, 0, 1], np.uint8)
    # start 0 -> farthest is x = 10 (100) -> x = 4 twice at 16, the lower index wins -> x = 7 at min(49, 9, 9) = 9 -> the duplicate at 0 -> nothing left
    idx, d2 = fps_ref(pos, 6, mask, start=0)
    assert idx.tolist() == [0, 1, 2, 5, 3, -1]
    assert d2.tolist() == [np.inf, 100.0, 16.0, 9.0, 0.0, -1.0]
    # start = -1: the lowest candidate; a masked start counts as -1; an unmasked run reaches x = 20 first
    assert fps_ref(pos, 2, np.array([0, 0, 1, 1, 0, 1], np.uint8), start=-1)[0].tolist() == [2, 5]
    assert fps_ref(pos, 2, mask, start=4)[0].tolist() == [0, 1]
    assert fps_ref(pos, 3, None, start=0)[0].tolist() == [0, 4, 1]
    bad = pos.copy()
    bad[1, 2] = np.nan
    assert fps_ref(bad, 6, mask, start=0)[0].tolist() == [0, 5, 2, 3, -1, -1]


def test_the_probability_method_is_refused_with_a_message():
    from unitex_amd.texturetools.sampling import select_and_sample_on_edges
    g = g14()
    with pytest.raises(NotImplementedError, match="equal_steps"):
        select_and_sample_on_edges(torch.from_numpy(g["stair_verts"]), torch.from_numpy(g["stair_faces"]), method="probability", N=10)


def test_fps_size_query_and_host_refusals_need_no_device():
    import ctypes as C
    from unitex_amd import _lib
    lib = _lib.load_library()
    assert lib.utx_fps_workspace_bytes(0) == 0 and lib.utx_fps_workspace_bytes(1) >= 16
    sizes = [lib.utx_fps_workspace_bytes(n) for n in (1, 255, 257, 70001, 1 << 22)]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] >= 4 << 22
    buf = (C.c_char * 8192)()
    base = (C.addressof(buf) + 255) & ~255
    pos, out = C.c_void_p(base), C.c_void_p(base + 1024)
    work, wb = C.c_void_p(base + 2048), lib.utx_fps_workspace_bytes(8)
    for N, M, start in ((8, 0, 0), (8, -1, 0), (8, 4, 8), (8, 4, -2), (0, 4, 0), (1 << 31, 4, 0)):      # refused before anything is launched
        assert lib.utx_fps(None, pos, None, N, M, start, out, None, work, wb, None) == -2, (N, M, start)
    assert lib.utx_fps(None, pos, None, 8, 4, 0, out, None, work, wb - 1, None) == -2
    assert lib.utx_fps(None, C.c_void_p(base + 4), None, 8, 4, 0, out, None, work, wb, None) == -2

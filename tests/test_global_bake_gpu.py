"""The scattered-sample UV bake on the GPU (csrc/global_bake.hip, NVDiffRendererInverse.global_inverse_rendering, remapping_uv_texture_v2), through the C ABI
and the Python surface, against the reference's own run (fixture G25) and the float64 restatement (tests/support/global_bake_ref.py).

Bounds (derived in the restatement's docstring; u = 2^-24, nothing measured):
  tex_to_pos / tex_to_pos_cam   4 u (|a0 u| + |a1 v| + |a2 w|) + u |a2| (1 + |w|) per channel, plus 4.5 u (|u| + |v| + |w|) for the per-vertex normalisation
  nearest stage                 the same sample as the float64 brute force wherever second - best > 8 u second; at most 0.5 % of the texels may be undecided
  propagation                   the neighbour lists are the kernel's INPUT, so the sets filled at each step and the number of steps are exact; a colour
                                filled at step s lies within s (4 k + 2 (12 / c_min + 5) + 2) u of the float64 evaluation on the same lists (colours in
                                [0, 1], positive cosines, c_min the smallest cosine used): each fill adds its own roundings to the largest error among the
                                colours it reads, which a convex combination passes on undiminished, hence the factor s along the fill chain."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests.support import global_bake_ref as R

pytestmark = pytest.mark.gpu


def _cuda(a, dtype=None):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).cuda().contiguous()


@pytest.fixture(scope="module")
def ops():
    from unitex_amd.texturetools import ops
    return ops


@pytest.fixture(scope="module")
def renderer():
    from unitex_amd.texturetools.renderer_inverse import NVDiffRendererInverse
    fix = R.g25()
    r = NVDiffRendererInverse(device="cuda").update_from_arrays(fix["verts"], fix["faces"], fix["uvs"])
    r.pbr_mesh.set_vertex_normals(fix["v_nrm"])
    return r


@pytest.fixture(scope="module")
def restated():
    return {name: R.restate_case(name) for name in R.CASES}


@pytest.mark.parametrize("name", list(R.CASES))
def test_view_samples_c_abi(ops, restated, name):
    fix, tag, _, kw, gold = R.case_arrays(name)
    uv = _cuda(fix["uvs"] * np.float32(2) - np.float32(1))
    t2p, cam, mask = ops.view_samples(_cuda(fix["rast_" + tag]), _cuda(fix["faces"]), uv, _cuda(fix["v_pos_cam_" + tag]), _cuda(fix["v_nrm_cam_" + tag]),
                                      kw.get("image_mask_exclude_boundary", True), kw.get("normal_angle_degree_threshold"),
                                      kw.get("ray_angle_degree_threshold"), None if "image_mask" not in kw else _cuda(kw["image_mask"]))
    assert np.array_equal(mask.cpu().numpy().astype(bool), gold["mask"]), "sample mask against G25"
    ref = restated[name]
    assert np.array_equal(mask.cpu().numpy().astype(bool), ref["mask"])
    _, _, _, detail = R.view_samples(fix["rast_" + tag], fix["faces"], fix["uvs"] * np.float32(2) - np.float32(1), fix["v_pos_cam_" + tag], fix["v_nrm_cam_" + tag])
    bu, bc = R.view_samples_bounds(detail)
    for got, key, bound in ((t2p, "tex_to_pos", bu), (cam, "tex_to_pos_cam", bc)):
        err = np.abs(got.cpu().numpy().astype(np.float64) - ref[key])
        print(name, key, "worst error / bound %.3f" % (err / bound).max())
        assert (err <= bound).all()
    assert (cam.cpu().numpy()[~detail["cov"]] == 0).all() and (t2p.cpu().numpy()[~detail["cov"]] == 0).all()


def test_view_samples_wraps_round_the_edge(ops):
    fix = R.g25()
    rast = np.roll(fix["rast_p"], 24, axis=2)
    uv = fix["uvs"] * np.float32(2) - np.float32(1)
    want = R.view_samples(rast, fix["faces"], uv, fix["v_pos_cam_p"], fix["v_nrm_cam_p"])[2]
    wrong = R.view_samples(rast, fix["faces"], uv, fix["v_pos_cam_p"], fix["v_nrm_cam_p"], mistakes={"no_wrap"})[2]
    got = ops.view_samples(_cuda(rast), _cuda(fix["faces"]), _cuda(uv), _cuda(fix["v_pos_cam_p"]), _cuda(fix["v_nrm_cam_p"]))[2].cpu().numpy().astype(bool)
    assert np.array_equal(got, want) and not np.array_equal(got, wrong)


def test_c_abi_refusals(ops):
    from unitex_amd._lib import ptr
    from unitex_amd.flux.ops import get_ctx
    ctx = get_ctx(torch.cuda.current_device())
    f = torch.zeros(64, device="cuda")
    i = torch.zeros(64, dtype=torch.int32, device="cuda")
    b = torch.full((64,), 7, dtype=torch.uint8, device="cuda")
    b2 = b.clone()
    step = lambda k=2, Cc=1, M=4, col_out=None, pend_out=None: ctx.lib.utx_knn_inpaint_step(
        ctx.handle, ptr(i), ptr(f), ptr(f), ptr(f), ptr(b), M, k, Cc, ptr(f.clone() if col_out is None else col_out), ptr(b2 if pend_out is None else pend_out),
        ptr(i[60:]), None)
    assert step(k=33) == -2 and step(k=0) == -2 and step(Cc=17) == -2 and step(Cc=0) == -2 and step(M=-1) == -2
    assert step(col_out=f) == -2 and step(pend_out=b) == -2
    assert ctx.lib.utx_knn_inpaint_step(ctx.handle, None, ptr(f), ptr(f), ptr(f), ptr(b), 4, 2, 1, ptr(f.clone()), ptr(b2), ptr(i), None) == -2
    assert step(M=0) == 0
    vs = lambda rast=f, B=1, F=1, out=b2: ctx.lib.utx_view_samples(ctx.handle, ptr(rast) if rast is not None else None, ptr(i), F, ptr(f), ptr(f), ptr(f), 4, B, 2, 2,
                                                                  1, 0, 0.0, 0, 0.0, None, ptr(f.clone()), ptr(f.clone()), ptr(out), None)
    assert vs(rast=None) == -2 and vs(F=0) == -2 and vs(B=-1) == -2 and vs(rast=f[1:]) == -2
    assert vs(B=0) == 0
    torch.cuda.synchronize()
    assert (b2 == 7).all(), "a refused call wrote its output"


@pytest.mark.parametrize("name", ["p_plain", "o_nrm"])
def test_nearest_stage(ops, restated, name):
    ref = restated[name]
    best, d_best, d_second = ref["nearest"]
    decided = (d_second - d_best) > R.nearest_margin(d_second)
    assert (~decided).sum() <= 0.005 * len(decided)
    z = lambda a: _cuda(np.concatenate([a, np.zeros_like(a[:, :1])], -1).astype(np.float32))
    ids = np.arange(len(ref["samples_u"]), dtype=np.float32)[:, None]
    got = ops.knn_gather(z(ref["samples_u"].astype(np.float32)), z(ref["predicts_u"]), 1, src_attr=_cuda(ids)).cpu().numpy()[:, 0].astype(np.int64)
    assert np.array_equal(got[decided], best[decided])


def _cloud(M, seed):
    """M points on a patch of the unit sphere (normals = positions, so every cosine is positive), one duplicated position, and an island of three
    points far away; known colours in [0, 1]; pending: the part of the patch with x < -0.15, one of the duplicates, and the whole island (stuck: its lists never hold two
    known points... at k = 10 and 32 they do reach the patch, so the island is filled late or never, as the count decides)"""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-0.5, 0.5, (M, 2))
    pos = np.concatenate([a, np.sqrt(1.0 - (a ** 2).sum(1))[:, None]], 1)
    pos[M - 3:] = pos[M - 3:] * [1, 1, -1]      # the island: the opposite cap
    pos[1] = pos[0]
    pos = pos.astype(np.float32)
    nrm = pos.copy()
    nrm[M - 3:] *= np.float32([1, 1, -1])       # keep the island's cosines against the patch positive
    pend = a[:, 0] < -0.15      # one contiguous region (about a third): the fill advances into it step by step
    pend[0], pend[1] = False, True
    pend[M - 3:] = True
    return pos, nrm, pend


@pytest.mark.parametrize("M,k,Cc", [(256, 2, 1), (257, 2, 9), (255, 10, 1), (256, 10, 3), (257, 10, 9), (255, 10, 3), (255, 32, 9), (256, 32, 1), (257, 32, 3)])
def test_propagation(ops, M, k, Cc):
    """exact fill sets and step count, colours within s e_fill (module docstring), the stuck island, the step cap and the duplicate"""
    pos, nrm, pend = _cloud(M, 1000 * k + M)
    rng = np.random.default_rng(M + k + Cc)
    col = (rng.integers(0, 256, (M, Cc)) / 255.0).astype(np.float32)
    col[pend] = 0
    tp = _cuda(pos)
    _, idx, d2 = ops.knn_gather(tp, tp, k, want_index=True)
    idx_n, d2_n = idx.cpu().numpy(), d2.cpu().numpy()
    assert (idx_n >= 0).all() and (d2_n[:2, :2] == 0).all(), "the duplicate leads both lists at distance 0"
    ref_col, ref_pend, ref_steps, ref_trace, cmins = R.inpaint(idx_n, d2_n, nrm, col, pend)
    trace = []
    got_col, got_pend, steps = ops.knn_inpaint(idx, d2, _cuda(nrm), _cuda(col), _cuda(pend.astype(np.uint8)), trace=trace)
    assert steps == ref_steps
    prev = pend.copy()
    for s, (t, fill) in enumerate(zip(trace, ref_trace), 1):
        now = t.cpu().numpy().astype(bool)
        assert np.array_equal(prev & ~now, fill), "the set filled at step %d" % s
        prev = now
    assert np.array_equal(got_pend.cpu().numpy().astype(bool), ref_pend)
    y = got_col.cpu().numpy().astype(np.float64)
    assert np.array_equal(np.isnan(y), np.isnan(ref_col))
    bound = np.zeros(M)
    for s, (fill, cmin) in enumerate(zip(ref_trace, cmins), 1):
        bound[fill] = R.fill_bound(k, s, cmin)
    fin = ~np.isnan(ref_col).any(1)
    err = np.abs(y - ref_col).max(1)
    if fin.any() and bound[fin].max() > 0:
        print("M %d k %d C %d: %d steps, worst error / bound %.3f" % (M, k, Cc, steps, (err[fin & (bound > 0)] / bound[fin & (bound > 0)]).max()))
    assert (err[fin] <= bound[fin]).all()
    assert (y[ref_pend] == 0).all(), "a texel that never qualifies keeps colour 0"
    if k == 2:
        assert steps == 0, "k - 1 = 1: a pending texel counts itself, nothing qualifies"
    else:
        assert steps >= 1 and np.isnan(y[1]).all() and (R.finish(y)[1] == 0).all(), "the duplicate: NaN, then colour 0"
        c1, p1, s1 = ops.knn_inpaint(idx, d2, _cuda(nrm), _cuda(col), _cuda(pend.astype(np.uint8)), n_iters_max=1)
        r1 = R.inpaint(idx_n, d2_n, nrm, col, pend, n_iters_max=1)
        assert s1 == 1 and np.array_equal(p1.cpu().numpy().astype(bool), r1[1]) and (steps == 1 or p1.sum() > got_pend.sum())


def test_stuck_island(ops):
    """k = 3: an island of three pending points far from everything: each list is the island itself, so no point ever has fewer than 2 pending entries"""
    pos, nrm, pend = _cloud(256, 5)
    tp = _cuda(pos)
    _, idx, d2 = ops.knn_gather(tp, tp, 3, want_index=True)
    col = np.where(pend[:, None], 0, 0.5).astype(np.float32)
    y, p, steps = ops.knn_inpaint(idx, d2, _cuda(nrm), _cuda(col), _cuda(pend.astype(np.uint8)))
    assert p.cpu().numpy()[-3:].all() and (y.cpu().numpy()[-3:] == 0).all()
    assert np.array_equal(p.cpu().numpy().astype(bool), R.inpaint(idx.cpu().numpy(), d2.cpu().numpy(), nrm, col, pend)[1])


def _own_lists(ops, samples_x, k, name):
    """(the kernel's own neighbour lists (idx, d2) of the covered texels, the rows on which they are not the lists the reference searched).  The two may
    differ only between points that are equally far in float32: |d2 - d2_k| <= 8 u d2_k in float64, asserted for every odd entry"""
    p = samples_x[:, :3].contiguous()
    _, idx, d2 = ops.knn_gather(p, p, k, want_index=True)
    knn = (idx.cpu().numpy().astype(np.int64), d2.cpu().numpy())
    pn = p.cpu().numpy()
    ridx, rd = R.knn_self(pn, k + 1)
    differ = (np.sort(knn[0], 1) != np.sort(ridx[:, :k], 1)).any(1)
    p64 = pn.astype(np.float64)
    for i in np.nonzero(differ)[0]:
        odd = np.setxor1d(knn[0][i], ridx[i, :k])
        dd = ((p64[odd] - p64[i]) ** 2).sum(1)
        assert (np.abs(dd - rd[i, k - 1] ** 2) <= 8 * R.U * rd[i, k - 1] ** 2 + 1e-300).all(), "a neighbour list differs beyond a float32 tie"
    print(name, "lists that differ from the float64 search (ties):", int(differ.sum()), "of", len(differ))
    return knn, differ


@pytest.mark.parametrize("name", ["p_ray", "o_nrm", "p_mask", "p_tex"])
def test_propagation_on_the_reference_lists_against_g25(ops, restated, name):
    """utx_knn_inpaint_step and its loop on the lists the REFERENCE searched (scipy's, leaf size 10: equal distances in its order), from the state in front of
    the propagation: the steps are G25's, the NaN texels are G25's, and every filled colour lies within twice s (e_fill + REF_EXTRA + 3 u) of G25's atlas --
    both sides within that of the float64 evaluation; the 3 u: the kernel takes squared distances, so the reference's float32 distance is squared and
    rooted again (1.5 u on each reciprocal, twice in the ratio).  No texel is left out but the NaN ones and what the nearest stage leaves undecided."""
    fix, tag, _, kw, gold = R.case_arrays(name)
    ref = restated[name]
    k = kw.get("n_neighbors", 10)
    cov = gold["map_alpha"] > 0
    idx, d = ref["knn"][0], np.sqrt(ref["knn"][1]).astype(np.float32)
    d2 = (d * d).astype(np.float32)
    y, pend, steps = ops.knn_inpaint(_cuda(idx.astype(np.int32)), _cuda(d2), _cuda(gold["world_to_tex"][cov][:, 3:]), _cuda(ref["y0"].astype(np.float32)),
                                     _cuda(ref["pending0"].astype(np.uint8)), n_iters_max=kw.get("n_iters_max", 1000))
    assert steps == gold["steps"] == ref["steps"]
    y = y.cpu().numpy().astype(np.float64)
    nan = np.isnan(y).any(-1)
    assert np.array_equal(nan, gold["nan"] > 0)
    bound, ok, _ = R.propagation_rows(name, ref, nan)
    filled = np.zeros(len(y), bool)
    for s, fill in enumerate(ref["trace"], 1):
        bound[fill] += s * 3 * R.U
        filled |= fill
    assert np.array_equal(pend.cpu().numpy().astype(bool), ref["pending0"] & ~filled)
    err = np.abs(R.finish(y) - gold["map_attr"][cov]).max(-1)
    print(name, "filled texels held to G25: %d of %d, worst error / (2 bound) %.3f" % ((ok & filled).sum(), filled.sum(),
                                                                                      (err[ok & filled] / (2 * bound[ok & filled])).max()))
    assert (ok & filled).sum() >= 0.9 * filled.sum()
    assert (err[ok] <= 2 * bound[ok]).all()


def _kw(kw):
    out = {}
    for k_, v in kw.items():
        out[k_] = torch.from_numpy(np.asarray(v)) if isinstance(v, np.ndarray) else v
    return out


@pytest.mark.parametrize("name", list(R.CASES))
def test_global_inverse_rendering_against_g25(ops, renderer, name):
    fix, tag, perspective, kw, gold = R.case_arrays(name)
    out = renderer.global_inverse_rendering(torch.from_numpy(fix["images"]), fix["c2ws_" + tag], fix["intr_" + tag], 48, 64, grid_interpolate_mode="nearest",
                                            perspective=perspective, **_kw(kw))
    assert set(out) == {"map_attr", "map_alpha", "map_mask", "samples_u", "samples_v", "predicts_u", "predicts_v", "samples_x", "samples_y", "tex_to_pos",
                        "tex_to_pos_cam", "world_to_tex"}
    got = {k_: (v.cpu().numpy() if v is not None else None) for k_, v in out.items()}
    got["mask"], got["steps"] = renderer.last["view_mask"].cpu().numpy(), renderer.last["inpaint_steps"]
    assert got["samples_u"].shape[0] == gold["n_samples"] and out["map_mask"].dtype == torch.bool
    assert np.array_equal(got["world_to_tex"], gold["world_to_tex"])
    knn = differ = None
    if kw.get("inpainting_occlusion", True):
        knn, differ = _own_lists(ops, out["samples_x"], kw.get("n_neighbors", 10), name)
    ref = R.restate_case(name, knn=knn, knn_nrm=None if knn is None else got["samples_x"][:, 3:])
    # the renderer builds the per-vertex camera arrays itself: their counted error joins the interpolation's
    fails = R.compare_case(name, got, ref=ref, strict_steps=differ is None or not differ.any(), list_rows_differ=differ, vertex_err=R.VERTEX_ERR_OWN_ARRAYS)
    assert not fails, "\n".join(fails)


def test_remapping_uv_texture_v2(ops, renderer):
    """the atlas against G25 on the covered texels: equal where the nearest stage set the colour (most of the atlas: a wrong permute or channel order cannot
    pass), within twice the counted bound where the propagation filled it and the neighbour lists are the reference's (atlas_against_g25; the kernel and
    its loop are held to G25 on the reference's own lists in test_propagation_on_the_reference_lists_against_g25); and against the composition of the
    renderer's call and pull_push"""
    from unitex_amd.texturetools.remapping_uv import remapping_uv_texture_v2
    fix = R.g25()
    images = torch.from_numpy(fix["images"]).permute(0, 3, 1, 2).contiguous()
    for name, tag, perspective, thr in (("p_ray", "p", True, "ray_angle_degree_threshold"), ("o_nrm", "o", False, "normal_angle_degree_threshold")):
        gold = R.case_arrays(name)[4]
        cov = gold["map_alpha"] > 0
        atlas = remapping_uv_texture_v2(renderer, fix["c2ws_" + tag], fix["intr_" + tag], images, render_size=48, texture_size=64, angle_degree_threshold=60.0,
                                        perspective=perspective)
        assert tuple(atlas.shape) == (64, 64, 4) and atlas.dtype == torch.float32
        assert np.array_equal(atlas[..., 3].cpu().numpy(), cov.astype(np.float32))
        inner = renderer.global_inverse_rendering(torch.from_numpy(fix["images"]), fix["c2ws_" + tag], fix["intr_" + tag], 48, 64, grid_interpolate_mode="nearest",
                                                  perspective=perspective, **{thr: 60.0})
        knn, differ = _own_lists(ops, inner["samples_x"], 10, name)
        ref = R.restate_case(name, knn=knn, knn_nrm=inner["samples_x"][:, 3:].cpu().numpy())
        fails = R.atlas_against_g25(name, atlas.cpu().numpy(), ref, differ, min_filled_rows=0)      # outpainting keeps the covered texels
        assert not fails, "\n".join(fails)
        bare = remapping_uv_texture_v2(renderer, fix["c2ws_" + tag], fix["intr_" + tag], images, render_size=48, texture_size=64, angle_degree_threshold=60.0,
                                       perspective=perspective, use_outpainting=False)
        assert torch.equal(bare[..., :3], inner["map_attr"][..., :3]) and torch.equal(bare[..., 3:], inner["map_alpha"])
        want = ops.pull_push(inner["map_attr"][..., :3].contiguous(), inner["map_alpha"][..., 0].to(torch.uint8).contiguous())
        assert torch.equal(atlas[..., :3], want)
        assert not torch.equal(atlas[..., :3], bare[..., :3]), "the outpainting filled nothing"
    for bad in (dict(use_cv_outpainting=True), dict(visualize=True), dict(visualize_detail=True), dict(grid_interpolate_mode="linear"),
                dict(grid_interpolate_mode="barycentric")):
        with pytest.raises(NotImplementedError):
            remapping_uv_texture_v2(renderer, fix["c2ws_p"], fix["intr_p"], images, render_size=48, texture_size=64, **bad)


def test_remapping_uv_texture_v2_downsamples_above_768(renderer):
    """render_size 770: the images are resampled to 768 x 768 and the views rendered at 768; a constant image makes every seen texel that constant"""
    from unitex_amd.texturetools.remapping_uv import remapping_uv_texture_v2
    fix = R.g25()
    colour = torch.tensor([0.25, 0.5, 0.75, 1.0])
    images = colour[None, :, None, None].expand(3, 4, 770, 770).contiguous()
    atlas = remapping_uv_texture_v2(renderer, fix["c2ws_p"], fix["intr_p"], images, render_size=770, texture_size=64, angle_degree_threshold=None,
                                    use_outpainting=False)
    assert tuple(atlas.shape) == (64, 64, 4) and tuple(renderer.last["view_mask"].shape) == (3, 768, 768)
    seen = np.unpackbits(fix["map_mask_p_plain"], axis=-1)[..., :64].astype(bool)
    assert seen.any() and (atlas[..., :3].cpu()[torch.from_numpy(seen)] == colour[:3]).all()
    with pytest.raises(ValueError):
        remapping_uv_texture_v2(renderer, fix["c2ws_p"], fix["intr_p"], images, render_size=768, texture_size=64)


def test_refusals(renderer):
    fix = R.g25()
    call = lambda **k: renderer.global_inverse_rendering(torch.from_numpy(fix["images"]), fix["c2ws_p"], fix["intr_p"], 48, 64, **k)
    for mode in ("linear", "barycentric"):
        with pytest.raises(NotImplementedError, match="'nearest'"):
            call(grid_interpolate_mode=mode)
    with pytest.raises(NotImplementedError, match="'nearest'"):
        call()      # the reference's default is kept, and refused
    with pytest.raises(ValueError):
        call(grid_interpolate_mode="cubic")
    with pytest.raises(TypeError):
        call(grid_interpolate_mode="nearest", antialias=True)
    with pytest.raises(ValueError):
        call(grid_interpolate_mode="nearest", texture_attr=torch.zeros(64, 64, 4))
    with pytest.raises(ValueError):
        call(grid_interpolate_mode="nearest", n_neighbors=33)


def test_wrappers_equal_simple_rendering(renderer):
    fix = R.g25()
    c2ws, intr = fix["c2ws_p"], fix["intr_p"]
    geo = renderer.geometry_rendering(c2ws, intr, 48)
    want = renderer.simple_rendering(c2ws, intr, 48, render_z_depth=True, render_distance=True, render_world_normal=True, render_camera_normal=True,
                                     render_world_position=True, render_camera_position=True, render_ray_direction=True, render_cos_ray_normal=True, render_uv=True)
    assert set(geo) == set(want) and all(torch.equal(geo[k_], want[k_]) for k_ in want)
    v_rgb = torch.from_numpy(np.random.default_rng(3).uniform(0, 1, (fix["verts"].shape[0], 3)).astype(np.float32))
    vr = renderer.vertex_rendering(v_rgb, c2ws, intr, 48, background=0.5)
    want = renderer.simple_rendering(c2ws, intr, 48, v_attr=v_rgb, render_v_attr=True, background=0.5)
    assert torch.equal(vr["rgb"], want["v_attr"]) and set(vr) == set(want) | {"rgb"}
    kd = torch.from_numpy(fix["texture"][..., :3].copy())
    ur = renderer.uv_rendering(kd, c2ws, intr, 48)
    want = renderer.simple_rendering(c2ws, intr, 48, map_attr=kd, render_uv=True, render_map_attr=True)
    assert torch.equal(ur["rgb"], want["map_attr"]) and torch.equal(ur["uv"], want["uv"]) and set(ur) == set(want) | {"rgb"}
    assert "rgb" not in renderer.uv_rendering(kd, c2ws, intr, 48, render_rgb=False)
    for fn, args in ((renderer.geometry_rendering, ()), (renderer.vertex_rendering, (v_rgb,)), (renderer.uv_rendering, (kd,))):
        for flag in ("render_all_point_cloud", "render_visible_point_cloud"):
            with pytest.raises(NotImplementedError):
                fn(*args, c2ws, intr, 48, **{flag: True})
        with pytest.raises(TypeError):
            fn(*args, c2ws, intr, 48, no_such_flag=1)

"""Restatement (TEST INFRASTRUCTURE ONLY), written for this project, of the scattered-sample UV bake (utx_view_samples, the nearest stage, utx_knn_inpaint_step
and the loop of ops.knn_inpaint; the reference: render/nvdiffrast/renderer_base.py:562-743) in numpy, shared by tests/test_global_bake_cpu.py and
tests/test_global_bake_gpu.py, with the counted bounds.  Every function evaluates in the kernel's operation order in the dtype it is given: float64 is the
yardstick, float32 reproduces the kernel's own roundings (each numpy float32 operation is one correctly rounded operation, as under -ffp-contract=off).

`mistakes` (a set of names) turns on deliberate kernel mistakes, one each, so that the tests can show that their comparisons reject them:
  no_wrap            the boundary test treats pixels outside the image as uncovered instead of wrapping round
  normalize_after    the position direction is interpolated un-normalised and normalised afterwards
  lt_k               a texel qualifies with fewer than k pending neighbours instead of k - 1
  in_place           the sweep updates in place (Gauss-Seidel) instead of Jacobi
  self_dropped       the +inf -> FLT_MAX self weight is left out of the L1 sum (so a duplicate no longer overflows it)
  pending_included   pending neighbours are not masked out of the two sums
  ray_as_normal      the ray threshold tests the normal's z instead of the dot product

Counted bounds (u = 2^-24, all relative to the magnitudes named):
  interpolation of one channel, (a0 u + a1 v) + a2 w with w = (1 - u) - v: each product 1 rounding, the two sums 1 each (<= 3 u of the terms' magnitudes,
      4 u with the second-order terms); w carries 2 roundings that are ABSOLUTE, not relative to w (1 - u is rounded near 1): |dw| <= u (1 + |w|) / 2 each:
      |err| <= 4 u (|a0 u| + |a1 v| + |a2 w|) + u |a2| (1 + |w|)            -> interp_bound
  a per-vertex normalised direction: 3 products, 2 sums, sqrt, division: each component within 4.5 u of the float64 one (|component| <= 1), which adds
      4.5 u (|u| + |v| + |w|) through the interpolation                -> interp_bound(..., attr_err=4.5 u)
  one propagation fill with k neighbours (step_bound): the weights are ratios of like-signed sums when every cosine is positive; r_j: sqrt + division (1.5 u
      relative on top of d2's own error, which cancels in the ratio only approximately: d2 is an INPUT here, identical on both sides); the L1 sum k roundings;
      s_j one division; the cosine: 2 x (3 products + 2 sums) for the lengths, 2 sqrt, 1 product, dot (3 + 2), a division: <= 12 u relative of |n_j||n_i|, and
      as a fraction of the cosine itself 12 u / |c_j|; w_j one product; the two sums k roundings each; the final division 1.  With c_min the smallest |cosine|
      among the known neighbours and all cosines positive:
          relative error of a filled colour against the float64 evaluation ON THE SAME INPUTS <= (2 k + 2 (12 / c_min + 5) + 2) u =: e_fill
      and an input error delta on the neighbours' colours passes through the convex combination undiminished: err_s <= max_j err_{s-1}(j) + e_fill max|y|.
      Along a fill chain of s steps: err <= s e_fill max|y| (colours lie in [0, 1] after the nearest stage, so max|y| <= 1).  A product w y below the normal
      range loses at most 2^-149 absolutely, against a weight sum of at least 2^-126 for the distances of any atlas (r / FLT_MAX with r >= 1e-3): 2^-23 k
      relative to the result in the worst case; counted as 2 k u more.                                         -> fill_bound(k, step, c_min)
  the nearest stage: utx_knn's d2 = (dx dx + dy dy) + dz dz with dz = 0: two subtractions (1 u each, relative to |dx|, i.e. 2 u on the square), two products,
      one sum: |d2_f32 - d2_f64| <= 4 u d2 (1 + O(u)) -> a texel is DECIDED when (second - best) > 8 u second    -> nearest_margin
"""
import numpy as np

U = 2.0 ** -24
FLT_MAX = float(np.finfo(np.float32).max)
MISTAKES = ("no_wrap", "normalize_after", "lt_k", "in_place", "self_dropped", "pending_included", "ray_as_normal")


def _tri_rows(rast, faces):
    tid = rast[..., 3].astype(np.int64) - 1
    cov = (rast[..., 3] > 0) & (tid >= 0) & (tid < faces.shape[0])
    return cov, faces[np.where(cov, tid, 0)].astype(np.int64)


def interp(a0, a1, a2, u, v, dtype):
    """(a0 u + a1 v) + a2 w, w = (1 - u) - v: sd_interp1; a* [..., C], u / v [...]"""
    u, v = u.astype(dtype)[..., None], v.astype(dtype)[..., None]
    w = (dtype(1.0) - u) - v
    return (a0.astype(dtype) * u + a1.astype(dtype) * v) + a2.astype(dtype) * w


def interp_bound(a0, a1, a2, u, v, attr_err=0.0):
    """the counted bound of one interpolated channel against float64 (module docstring); attr_err: the absolute error the attribute itself carries"""
    u, v = u.astype(np.float64)[..., None], v.astype(np.float64)[..., None]
    w = 1.0 - u - v
    mag = np.abs(a0 * u) + np.abs(a1 * v) + np.abs(a2 * w)
    return 4 * U * mag + U * np.abs(a2) * (1 + np.abs(w)) + attr_err * (np.abs(u) + np.abs(v) + np.abs(w)) * (1 + 8 * U) + 2.0 ** -140


def normalize(p, dtype):
    """F.normalize(eps=1e-12) in sd_normalize3's order: p / max(sqrt((x x + y y) + z z), 1e-12)"""
    p = p.astype(dtype)
    n = np.sqrt((p[..., 0] * p[..., 0] + p[..., 1] * p[..., 1]) + p[..., 2] * p[..., 2])
    return p / np.maximum(n, dtype(1e-12))[..., None]


def cos_threshold(degrees):
    return np.float32(np.cos(np.radians(float(degrees))))


def view_samples(rast, faces, v_uv, v_pos_cam, v_nrm_cam, exclude_boundary=True, normal_deg=None, ray_deg=None, image_mask=None, dtype=np.float64,
                 mistakes=()):
    """utx_view_samples: rast [B,H,W,4], faces [F,3], v_uv [V,2], v_pos_cam / v_nrm_cam [B,V,3] -> (tex_to_pos [B,H,W,2], tex_to_pos_cam [B,H,W,6], mask bool,
    detail) ; detail holds what the bounds need (the three vertices' attributes and the weights)"""
    B = rast.shape[0]
    cov, rows = _tri_rows(rast, faces)
    u, v = rast[..., 0], rast[..., 1]
    b = np.arange(B)[:, None, None]
    uv3 = [v_uv[rows[..., c]] for c in range(3)]
    tex_to_pos = interp(*uv3, u, v, dtype) * cov[..., None]
    if "normalize_after" in mistakes:
        d3 = [v_pos_cam[b, rows[..., c]].astype(dtype) for c in range(3)]
        d = normalize(interp(*d3, u, v, dtype), dtype)
    else:
        d3 = [normalize(v_pos_cam[b, rows[..., c]], dtype) for c in range(3)]
        d = interp(*d3, u, v, dtype)
    n3 = [v_nrm_cam[b, rows[..., c]] for c in range(3)]
    n = interp(*n3, u, v, dtype)
    cam = np.concatenate([d, n], axis=-1) * cov[..., None]
    mask = cov.copy()
    if exclude_boundary:
        if "no_wrap" in mistakes:
            p = np.pad(cov, ((0, 0), (1, 1), (1, 1)))
            mask &= p[:, :-2, 1:-1] & p[:, 2:, 1:-1] & p[:, 1:-1, :-2] & p[:, 1:-1, 2:]
        else:
            mask &= np.roll(cov, 1, 1) & np.roll(cov, -1, 1) & np.roll(cov, 1, 2) & np.roll(cov, -1, 2)
    dot = (cam[..., 0] * cam[..., 3] + cam[..., 1] * cam[..., 4]) + cam[..., 2] * cam[..., 5]
    if normal_deg is not None:
        mask &= cam[..., 5] > dtype(cos_threshold(normal_deg))
    if ray_deg is not None:
        mask &= (cam[..., 5] if "ray_as_normal" in mistakes else dot) > dtype(cos_threshold(ray_deg))
    if image_mask is not None:
        mask &= np.asarray(image_mask).reshape(mask.shape) != 0
    return tex_to_pos, cam, mask, dict(cov=cov, uv3=uv3, d3=d3, n3=n3, u=u, v=v, dot=dot)


# The per-vertex camera arrays, when the two sides do not share them (the renderer builds its own with utx_transform_points / utx_camera_normals, the fixture
# holds torch's): a camera-space position component is r0 x + r1 y + r2 z + t, 4 terms, |err| <= 4 u (|x| + |y| + |z| + |t|) <= 24 u for vertices in
# [-1, 1]^3 and cameras within 3 of the origin; as a direction, divided by a length of at least 1.6 (orbit radius 2.8, vertices within 1.2 of the origin), twice
# that relative error: 30 u per side, 60 u between two sides.  A rotated normal is 3 terms, <= 3 sqrt(3) u, its normalisation 4.5 u: 10 u per side, 20 u between.
VERTEX_ERR_OWN_ARRAYS = (60 * U, 20 * U)


def view_samples_bounds(detail, vertex_err=(0.0, 0.0)):
    """(bound of tex_to_pos [B,H,W,2], bound of tex_to_pos_cam [B,H,W,6]) against the float64 evaluation, from its `detail`; vertex_err: the absolute error of
    the per-vertex (direction, normal) the two sides were given, 0 when they share the arrays"""
    f = lambda t: [np.asarray(x, np.float64) for x in t]
    bu = interp_bound(*f(detail["uv3"]), detail["u"], detail["v"])
    bd = interp_bound(*f(detail["d3"]), detail["u"], detail["v"], attr_err=4.5 * U + vertex_err[0])
    bn = interp_bound(*f(detail["n3"]), detail["u"], detail["v"], attr_err=vertex_err[1])
    return bu, np.concatenate([bd, bn], axis=-1)


def nearest(samples_u, predicts_u, chunk=512):
    """float64 brute force 2-D nearest sample: (index of the best [Np], best d2, second-best d2); ties -> lower index (argmin)"""
    s, p = np.asarray(samples_u, np.float64), np.asarray(predicts_u, np.float64)
    best, d_best, d_second = np.zeros(len(p), np.int64), np.zeros(len(p)), np.full(len(p), np.inf)
    for i in range(0, len(p), chunk):
        d = ((p[i:i + chunk, None, :] - s[None]) ** 2).sum(-1)
        j = d.argmin(1)
        best[i:i + chunk], d_best[i:i + chunk] = j, d[np.arange(len(j)), j]
        if len(s) > 1:
            d[np.arange(len(j)), j] = np.inf
            d_second[i:i + chunk] = d.min(1)
    return best, d_best, d_second


def nearest_margin(d_second):
    """a texel is decided when second - best exceeds this (module docstring)"""
    return 8 * U * d_second + 2.0 ** -140


def knn_self(pos, k):
    """(idx [M,k], d [M,k]) of the k nearest points of the set to each of its points, float64, ascending; scipy's cKDTree if importable"""
    pos = np.asarray(pos, np.float64)
    try:
        from scipy.spatial import cKDTree
        d, idx = cKDTree(pos, leafsize=10).query(pos, k=k)      # the leaf size of the reference: it decides the order among equal distances
        return idx.reshape(len(pos), k).astype(np.int64), d.reshape(len(pos), k)
    except ImportError:
        d2 = ((pos[:, None, :] - pos[None]) ** 2).sum(-1)
        idx = np.argsort(d2, axis=1, kind="stable")[:, :k]
        return idx, np.sqrt(np.take_along_axis(d2, idx, 1))


def weights(d2, nrm, idx, dtype=np.float64, mistakes=()):
    """w [M,k] of utx_knn_inpaint_step, from SQUARED distances d2 [M,k]"""
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        r = dtype(1.0) / np.sqrt(d2.astype(dtype))
        fmax = dtype(FLT_MAX)
        r = np.where(np.isnan(r), dtype(0.0), np.clip(r, -fmax, fmax))
        l1 = np.zeros(len(r), dtype)
        for j in range(r.shape[1]):
            t = np.abs(r[:, j])
            if "self_dropped" in mistakes:
                t = np.where(t == fmax, dtype(0.0), t)
            l1 = l1 + t
            if dtype is np.float64:      # float32's overflow, which the reference's arithmetic rests on: past FLT_MAX + half an ulp (2^103) the sum is +inf
                l1 = np.where(l1 >= FLT_MAX + 2.0 ** 103, np.inf, l1)
        s = r / np.maximum(l1, dtype(1e-12))[:, None]
        n = nrm.astype(dtype)
        ln = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        nj = n[idx]
        dot = (nj[..., 0] * n[:, None, 0] + nj[..., 1] * n[:, None, 1]) + nj[..., 2] * n[:, None, 2]
        c = dot / np.maximum(ln[idx] * ln[:, None], dtype(1e-8))
        return (s * c).astype(dtype), c


def inpaint_step(idx, w, col, pending, mistakes=()):
    """one sweep: (col, pending, filled bool [M]); w from weights()"""
    M, k = idx.shape
    dtype = col.dtype.type
    pend = pending.astype(bool)
    fill = pend & (pend[idx].sum(1) < (k if "lt_k" in mistakes else k - 1))
    out, pend_out = col.copy(), pend.copy()
    src, src_pend = (out, pend_out) if "in_place" in mistakes else (col, pend)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for i in np.nonzero(fill)[0]:
            acc, ws = np.zeros(col.shape[1], dtype), dtype(0.0)
            for j in range(k):
                q = idx[i, j]
                mw = w[i, j] if "pending_included" in mistakes else (w[i, j] * dtype(0.0) if src_pend[q] else w[i, j])
                ws = ws + mw
                acc = acc + mw * src[q]
            out[i] = acc / ws
            pend_out[i] = False
    return out, pend_out, fill


def inpaint(idx, d2, nrm, col, pending, n_iters_max=1000, dtype=np.float64, mistakes=()):
    """ops.knn_inpaint: -> (col [M,C], pending bool [M], steps, trace = the list of each step's filled sets, c_min = each step's smallest |cosine| used)"""
    idx = np.asarray(idx, np.int64)
    w, c = weights(np.asarray(d2), np.asarray(nrm), idx, dtype, mistakes)
    col, pend = np.asarray(col).astype(dtype), np.asarray(pending).astype(bool)
    trace, cmins = [], []
    while len(trace) < n_iters_max:
        known = ~pend[idx]
        nxt, pend_nxt, fill = inpaint_step(idx, w, col, pend, mistakes)
        if not fill.any():
            break
        cmins.append(float(np.abs(c[fill])[known[fill]].min()) if known[fill].any() else 0.0)
        col, pend = nxt, pend_nxt
        trace.append(fill)
    return col, pend, len(trace), trace, cmins


def fill_bound(k, step, c_min):
    """the counted bound on a colour filled at `step` (1-based) against float64 on the same lists, colours in [0, 1] (module docstring)"""
    e_fill = (2 * k + 2 * (12.0 / max(c_min, 1e-30) + 5) + 2 + 2 * k) * U
    return step * e_fill


def finish(col):
    """nan_to_num(nan=0).clamp(0, 1)"""
    return np.clip(np.nan_to_num(col, nan=0.0, posinf=FLT_MAX, neginf=-FLT_MAX), 0.0, 1.0)


def bake(rast, rast2d, faces, v_uv, v_pos_cam, v_nrm_cam, v_pos, v_nrm, face_mask, image_attr, exclude_boundary=True, normal_deg=None, ray_deg=None,
         image_mask=None, texture_attr=None, texture_mask=None, inpainting=True, k=10, n_iters_max=1000, dtype=np.float64, mistakes=(), knn=None,
         knn_pos=None, knn_nrm=None):
    """global_inverse_rendering with grid_interpolate_mode='nearest' -> dict (the reference's keys, plus 'mask' = the sample mask, 'steps', 'trace').
    The neighbour lists are an INPUT of the propagation: knn = (idx, d2) as given (the GPU's own, in the GPU tests), else the float64 search over knn_pos
    [M,3] (the float32 positions the reference searched), else over the positions interpolated here; knn_nrm [M,3]: the normals the propagation reads, when
    the other side's own (float32) are to be shared."""
    tex_to_pos, cam, mask, _ = view_samples(rast, faces, v_uv, v_pos_cam, v_nrm_cam, exclude_boundary, normal_deg, ray_deg, image_mask, dtype, mistakes)
    cov2, rows2 = _tri_rows(rast2d[None], faces)
    cov2, rows2 = cov2[0], rows2[0]
    tid = rast2d[..., 3].astype(np.int64) - 1
    pm = cov2 & face_mask.astype(bool).any(0)[np.where(cov2, tid, 0)]
    if texture_mask is not None:
        pm &= ~texture_mask[..., 0].astype(bool)
    Ht, Wt = rast2d.shape[:2]
    gx, gy = (np.arange(Wt, dtype=np.float32) + np.float32(0.5)) / np.float32(Wt) * np.float32(2) - np.float32(1), \
        (np.arange(Ht, dtype=np.float32) + np.float32(0.5)) / np.float32(Ht) * np.float32(2) - np.float32(1)
    tt = np.stack(np.broadcast_arrays(gx[None, :], gy[:, None]), -1)
    samples_u, samples_v, predicts_u = tex_to_pos[mask], image_attr[mask], tt[pm]
    best, d_best, d_second = nearest(samples_u, predicts_u)
    predicts_v = samples_v[best]
    map_attr = np.zeros((Ht, Wt, image_attr.shape[-1]), dtype)
    map_attr[pm] = predicts_v
    map_mask = pm & ~np.isnan(map_attr).any(-1)
    map_attr = finish(map_attr)
    if texture_mask is not None:
        map_attr = np.where(texture_mask.astype(bool), texture_attr.astype(dtype), map_attr)
        map_mask = cov2 & (map_mask | texture_mask[..., 0].astype(bool))
    a6 = np.concatenate([v_pos, v_nrm], -1)
    w2t = interp(*[a6[rows2[..., c]] for c in range(3)], rast2d[..., 0], rast2d[..., 1], dtype) * cov2[..., None]
    out = dict(mask=mask, tex_to_pos=tex_to_pos, tex_to_pos_cam=cam, samples_u=samples_u, samples_v=samples_v, predicts_u=predicts_u, predicts_v=predicts_v,
               predicts_mask=pm, nearest=(best, d_best, d_second), map_mask=map_mask, map_alpha=cov2.astype(np.float32), world_to_tex=w2t, steps=0, trace=[])
    if inpainting:
        sx = w2t[cov2]
        if knn is None:
            idx, d = knn_self(sx[:, :3].astype(np.float32) if knn_pos is None else knn_pos, k)
            knn = (idx, d * d)
        y0 = map_attr[cov2].copy()
        y, _, steps, trace, cmins = inpaint(knn[0], knn[1], sx[:, 3:] if knn_nrm is None else knn_nrm, y0, ~map_mask[cov2], n_iters_max, dtype, mistakes)
        out.update(samples_x=sx, samples_y=y, steps=steps, trace=trace, cmins=cmins, knn=knn, y0=y0, pending0=~map_mask[cov2])
        map_attr = np.zeros_like(map_attr)
        map_attr[cov2] = y
        map_attr = finish(map_attr)
    out["map_attr"] = map_attr
    return out


# ---- the fixture (tests/golden/g25_global_inverse.npz, written by tests/golden/make_golden_global_inverse.py) and the comparisons both test modules make

import os

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "golden", "g25_global_inverse.npz")
CASES = {      # name -> (camera set, perspective, keywords of global_inverse_rendering)
    "p_ray": ("p", True, dict(ray_angle_degree_threshold=60.0)),
    "p_plain": ("p", True, dict(inpainting_occlusion=False)),
    "o_nrm": ("o", False, dict(normal_angle_degree_threshold=60.0)),
    "p_mask": ("p", True, dict(image_mask=True, image_mask_exclude_boundary=False, n_neighbors=4, n_iters_max=2)),
    "p_tex": ("p", True, dict(texture=True)),
}
_FIX = {}


def g25():
    if not _FIX:
        with np.load(GOLD, allow_pickle=False) as f:
            _FIX.update({k: f[k] for k in f.files})
        _FIX["images"] = _FIX["images_u8"].astype(np.float32) / np.float32(255.0)
        _FIX["texture"] = _FIX["texture_u8"].astype(np.float32) / np.float32(255.0)
    return _FIX


def case_arrays(name):
    """(fix, tag, perspective, kw with the fixture's arrays put in, golden dict) of one case"""
    fix = g25()
    tag, perspective, kw = CASES[name]
    kw = dict(kw)
    if kw.pop("image_mask", False):
        kw["image_mask"] = fix["image_mask"]
    if kw.pop("texture", False):
        kw["texture_attr"], kw["texture_mask"] = fix["texture"], fix["texture_mask"]
    R, T = int(fix["render_size"]), int(fix["texture_size"])
    gold = dict(mask=np.unpackbits(fix["mask_" + name], axis=-1)[..., :R].astype(bool), map_attr=fix["map_attr_" + name],
                map_mask=np.unpackbits(fix["map_mask_" + name], axis=-1)[..., :T].astype(bool), map_alpha=fix["map_alpha"], steps=int(fix["steps_" + name]),
                n_samples=int(fix["n_samples_" + name]), nan=fix.get("nan_" + name), tex_to_pos=fix["tex_to_pos_" + tag],
                tex_to_pos_cam=fix["tex_to_pos_cam_" + tag], world_to_tex=fix["world_to_tex"])
    return fix, tag, perspective, kw, gold


def restate_case(name, dtype=np.float64, mistakes=(), knn=None, knn_nrm=None):
    fix, tag, _, kw, _ = case_arrays(name)
    return bake(fix["rast_" + tag], fix["rast2d"], fix["faces"], fix["uvs"] * np.float32(2) - np.float32(1), fix["v_pos_cam_" + tag], fix["v_nrm_cam_" + tag],
                fix["verts"], fix["v_nrm"], fix["face_mask_" + tag], fix["images"], exclude_boundary=kw.get("image_mask_exclude_boundary", True),
                normal_deg=kw.get("normal_angle_degree_threshold"), ray_deg=kw.get("ray_angle_degree_threshold"), image_mask=kw.get("image_mask"),
                texture_attr=kw.get("texture_attr"), texture_mask=kw.get("texture_mask"), inpainting=kw.get("inpainting_occlusion", True),
                k=kw.get("n_neighbors", 10), n_iters_max=kw.get("n_iters_max", 1000), dtype=dtype, mistakes=mistakes, knn=knn,
                knn_pos=fix["world_to_tex"][fix["map_alpha"] > 0][:, :3], knn_nrm=knn_nrm)


# the reference's own roundings on top of fill_bound, per step: scipy's float64 distance rounded to float32 (0.5 u on r_j, twice in the ratio) and torch's
# cosine_similarity, whose operation order differs from the kernel's within the same count: 2 u more per step
REF_EXTRA = 2 * U


def propagation_rows(name, ref, nan_got, list_rows_differ=None):
    """Over the covered texels of one case with propagation: (bound [M], rows held to the restatement `ref`, rows held to G25's atlas).
    bound: per texel filled at step s, s (e_fill + REF_EXTRA), 0 on the texels the nearest stage set (their colours are copies).  Left out of both row
    sets: NaN texels, the texels whose nearest sample is undecided and what is filled from them; left out of the G25 rows as well: list_rows_differ (bool
    [M], the texels whose neighbour list is not the one the reference searched) and, to a fixed point whatever the order of the fills, what is filled
    from them -- with another list a neighbour may have been filled EARLIER in the reference's run than here."""
    _, _, _, kw, gold = case_arrays(name)
    cov = gold["map_alpha"] > 0
    pm = ref["predicts_mask"]
    _, d_best, d_second = ref["nearest"]
    decided = (d_second - d_best) > nearest_margin(d_second)
    M = int(cov.sum())
    bound = np.zeros(M)
    for s, (fill, cmin) in enumerate(zip(ref["trace"], ref["cmins"]), 1):
        bound[fill] = fill_bound(kw.get("n_neighbors", 10), s, cmin) + s * REF_EXTRA
    und = np.zeros(M, bool)
    und[pm[cov]] = ~decided
    ok_rows = ~und & ~np.isnan(ref["samples_y"]).any(-1) & ~nan_got
    tainted = und.copy()
    for fill in ref["trace"]:
        tainted[fill] |= tainted[ref["knn"][0][fill]].any(1)
    ok_rows &= ~tainted
    ok_g25 = ok_rows
    if list_rows_differ is not None:
        tainted = tainted | list_rows_differ
        filled = np.zeros(M, bool)
        for fill in ref["trace"]:
            filled |= fill
        while True:
            more = tainted | (filled & tainted[ref["knn"][0]].any(1))
            if np.array_equal(more, tainted):
                break
            tainted = more
        ok_g25 = ok_rows & ~tainted
    return bound, ok_rows, ok_g25


def atlas_against_g25(name, atlas_rgb, ref, list_rows_differ=None, min_filled_rows=1):
    """an atlas [Ht,Wt,>=3] (its first three channels) against G25's map_attr of the case on the covered texels, within twice the counted bound (both sides lie
    within `bound` of the float64 evaluation; 0 on the texels the nearest stage set: equality) -> list of failures.  At least min_filled_rows texels filled
    by the propagation must be among the rows compared, so that the comparison cannot run empty."""
    _, _, _, _, gold = case_arrays(name)
    cov = gold["map_alpha"] > 0
    bound, _, ok = propagation_rows(name, ref, np.isnan(ref["samples_y"]).any(-1), list_rows_differ)
    err = np.abs(np.asarray(atlas_rgb, np.float64)[cov][:, :3] - gold["map_attr"][cov][:, :3]).max(-1)
    fails = []
    if (ok & (bound > 0)).sum() < min_filled_rows:
        fails.append("only %d filled texels are held to G25" % (ok & (bound > 0)).sum())
    if not (err[ok] <= 2 * bound[ok]).all():
        fails.append("atlas against G25: %d of %d texels past twice the counted bound (worst error %.3g)" % ((err[ok] > 2 * bound[ok]).sum(), ok.sum(), err[ok].max()))
    return fails


def compare_case(name, got, ref=None, strict_steps=True, list_rows_differ=None, vertex_err=(0.0, 0.0)):
    """The comparisons of one case: `got` (a dict with the reference's keys plus 'mask' and 'steps'; arrays as numpy) against G25 and against the float64
    restatement `ref` (restate_case(name); made here when None).  list_rows_differ (bool [M]): the covered texels whose neighbour list is not the one the
    reference searched (equal distances, ordered differently): they, and what is filled from them, are compared with the restatement only, not with G25's
    atlas.  Returns the list of failures (empty = pass)."""
    fix, tag, _, kw, gold = case_arrays(name)
    ref = restate_case(name) if ref is None else ref
    fails = []
    if not np.array_equal(np.asarray(got["mask"]).astype(bool), gold["mask"]):
        fails.append("sample mask differs from G25 on %d pixels" % (np.asarray(got["mask"]).astype(bool) != gold["mask"]).sum())
    _, _, _, detail = view_samples(fix["rast_" + tag], fix["faces"], fix["uvs"] * np.float32(2) - np.float32(1), fix["v_pos_cam_" + tag], fix["v_nrm_cam_" + tag])
    bu, bc = view_samples_bounds(detail)
    bc_got = view_samples_bounds(detail, vertex_err)[1]
    for key, bound, bound_got in (("tex_to_pos", bu, bu), ("tex_to_pos_cam", bc, bc_got)):
        err = np.abs(np.asarray(got[key], np.float64) - ref[key])
        if not (err <= bound_got).all():
            fails.append("%s: %d values past the counted bound (worst %.3g x)" % (key, (err > bound_got).sum(), (err / bound_got).max()))
        err = np.abs(gold[key].astype(np.float64) - ref[key])
        if not (err <= bound).all():
            fails.append("%s of G25 against the restatement: %d values past the bound" % (key, (err > bound).sum()))
    if not np.array_equal(np.asarray(got["map_mask"]).reshape(gold["map_mask"].shape).astype(bool), gold["map_mask"]):
        fails.append("map_mask differs from G25")
    if not np.array_equal(np.asarray(got["map_alpha"]).reshape(gold["map_alpha"].shape) > 0, gold["map_alpha"] > 0):
        fails.append("map_alpha differs from G25")
    # the nearest stage: the same sample as the float64 brute force wherever it is decided
    best, d_best, d_second = ref["nearest"]
    decided = (d_second - d_best) > nearest_margin(d_second)
    if (~decided).sum() > 0.005 * max(len(decided), 1):
        fails.append("%d of %d predicted texels are undecided (cap 0.5 %%)" % ((~decided).sum(), len(decided)))
    pv = np.asarray(got["predicts_v"])
    if pv.shape != ref["predicts_v"].shape or not np.array_equal(pv[decided], ref["predicts_v"][decided]):
        fails.append("predicts_v differs from the float64 nearest sample on decided texels")
    cov = gold["map_alpha"] > 0
    pm = ref["predicts_mask"]
    dec_map = np.zeros(pm.shape, bool)
    dec_map[pm] = decided
    if not np.array_equal(gold["map_attr"][dec_map & gold["map_mask"]], np.asarray(got["map_attr"])[dec_map & gold["map_mask"]]):
        fails.append("map_attr differs from G25 on decided predicted texels")
    if kw.get("inpainting_occlusion", True):
        if strict_steps and int(got["steps"]) != gold["steps"]:
            fails.append("steps %d, G25 took %d" % (int(got["steps"]), gold["steps"]))
        if int(got["steps"]) != ref["steps"]:
            fails.append("steps %d, the restatement took %d" % (int(got["steps"]), ref["steps"]))
        y = np.asarray(got["samples_y"], np.float64)
        nan_got = np.isnan(y).any(-1)
        if gold["nan"] is not None and not np.array_equal(nan_got, gold["nan"] > 0):
            fails.append("NaN texels differ from G25 (%d against %d)" % (nan_got.sum(), (gold["nan"] > 0).sum()))
        bound, ok_rows, ok_g25 = propagation_rows(name, ref, nan_got, list_rows_differ)
        err = np.abs(y - ref["samples_y"]).max(-1)
        if not (err[ok_rows] <= bound[ok_rows] + 0).all():
            fails.append("samples_y: %d texels past the counted bound (worst %.3g x)" % ((err[ok_rows] > bound[ok_rows]).sum(),
                                                                                       (err[ok_rows] / np.maximum(bound[ok_rows], 1e-300)).max()))
        ok_rows = ok_g25
        ma = np.asarray(got["map_attr"], np.float64)[cov]
        err = np.abs(ma - gold["map_attr"][cov]).max(-1)
        if not (err[ok_rows] <= 2 * bound[ok_rows]).all():      # both sides within `bound` of the float64 evaluation
            fails.append("map_attr against G25: %d texels past twice the counted bound" % (err[ok_rows] > 2 * bound[ok_rows]).sum())
    else:
        if got.get("samples_y") is not None:
            fails.append("samples_y without inpainting_occlusion")
    return fails

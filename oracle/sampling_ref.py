"""Geometry sampling for the field stage (TEST INFRASTRUCTURE ONLY): the numpy restatements that tests/test_sampling_gpu.py and
tests/test_spatial_sampling_gpu.py hold the HIP kernels of csrc/sampling.hip to.  Each is pinned on the CPU before a GPU test leans on it.  tests/test_sampling_cpu.py:
the equal-steps sampler to fixture G14's captured samples (tests/golden/make_golden_sampling.py) bit for bit, Philox4x32-10 to the Random123 known-answer vectors, the
farthest-point sampling to an example worked by hand.  tests/test_spatial_sampling_cpu.py: the near-surface offsets and the material lookup to fixture G22, the texture lookup to grid_sample."""
import os

import numpy as np

from .pixel_ref import grid_blend, interp_corners, reflect_index

U = 2.0 ** -24
GOLD = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
F32 = np.float32


def g14():
    return np.load(os.path.join(GOLD, "g14_geometry_sampling.npz"))


# ---- numpy restatements (float32 throughout; numpy rounds every product and sum on its own, as the kernels do without contraction) ----
def prefix_f32(x):
    """running sum accumulated in float64, rounded to float32 per element (torch.cumsum on the CPU)"""
    return np.cumsum(np.asarray(x, np.float64)).astype(F32)


def edge_tables(verts, edges, mask):
    """selected edges -> (sel [E,2], ids [E], start [E], length [E], total) as sample_on_edges_v2 builds them"""
    ids = np.flatnonzero(mask)
    sel = edges[ids]
    d = verts[sel[:, 1]] - verts[sel[:, 0]]
    length = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F32)
    cum = prefix_f32(length)
    start = np.concatenate([np.zeros(1, F32), cum[:-1]])
    return sel, ids, start, length, cum[-1]


def linspace_f32(total, N):
    """torch's formula: step = total / (N - 1); lower half 0 + step * i, upper half total - step * (N - 1 - i)"""
    total = F32(total)
    if N == 1:
        return np.zeros(1, F32)
    i = np.arange(N)
    step = F32(total / F32(N - 1))
    return np.where(i < N // 2, F32(0) + step * i.astype(F32), total - step * (N - 1 - i).astype(F32)).astype(F32)


def sample_edges_ref(verts, sel, ids, start, length, total, N):
    t = linspace_f32(total, N)
    e = np.searchsorted(start[1:], t, side="left")
    with np.errstate(all="ignore"):
        w = ((t - start[e]) / length[e]).astype(F32)
    w = np.where(np.isfinite(w), w, F32(0.5)).astype(F32)
    w = np.minimum(np.maximum(w, F32(0)), F32(1))          # the kernel keeps a sample on the edge it reports; no-op wherever the prefix sums are exact (G14's staircase)
    v0, v1 = verts[sel[e, 0]], verts[sel[e, 1]]
    samples = w[:, None] * v0 + (F32(1) - w)[:, None] * v1
    return samples.astype(F32), ids[e].astype(np.int32), w


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] uint32 -> [..., 4] uint32 (Salmon et al., SC'11)"""
    c = [np.asarray(counter[..., j], np.uint64) for j in range(4)]
    k = [np.asarray(key[..., j], np.uint64) for j in range(2)]
    lo32 = np.uint64(0xffffffff)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & lo32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & lo32]
        k = [(k[0] + np.uint64(0x9E3779B9)) & lo32, (k[1] + np.uint64(0xBB67AE85)) & lo32]
    return np.stack(c, -1).astype(np.uint32)


def sample_surface_ref(verts, faces, cum, N, seed):
    u01 = uniforms(N, seed, 0)
    pick = u01[:, 0] * cum[-1]
    face = np.minimum(np.searchsorted(cum, pick, side="left"), len(cum) - 1)
    u, v = u01[:, 1].copy(), u01[:, 2].copy()
    fold = (u + v) > F32(1)
    u[fold] -= F32(1)
    v[fold] -= F32(1)
    u, v = np.abs(u), np.abs(v)
    w = F32(1) - (u + v)
    a, b, c = verts[faces[face, 0]], verts[faces[face, 1]], verts[faces[face, 2]]
    samples = (a * u[:, None] + b * v[:, None]) + c * w[:, None]
    return samples.astype(F32), face.astype(np.int32), np.stack([u, v, w], -1).astype(F32)


def face_weights_cum(verts, faces):
    a, b, c = verts[faces[:, 0]].astype(np.float64), verts[faces[:, 1]].astype(np.float64), verts[faces[:, 2]].astype(np.float64)
    return prefix_f32(np.linalg.norm(np.cross(b - a, c - a), axis=1).astype(F32))


def fps_ref(pos, M, mask=None, start=0):
    """utx_fps's semantics: mind = +inf for candidates; masked-out and non-finite points never are; each pick takes the candidate with the largest mind, ties to
    the lower index, and leaves the set; d2 = (dx*dx + dy*dy) + dz*dz in float32; out of candidates: -1 / -1.  start >= 0 is the first pick (a start that is no
    candidate counts as -1), start = -1 the lowest candidate index."""
    pos = np.asarray(pos, F32)
    N = len(pos)
    valid = np.isfinite(pos).all(1)
    if mask is not None:
        valid &= np.asarray(mask).astype(bool)
    mind = np.where(valid, F32(np.inf), F32(-1)).astype(F32)
    out_idx, out_d2 = np.full(M, -1, np.int32), np.full(M, -1, F32)
    for k in range(M):
        if not (mind >= 0).any():
            break
        p = start if (k == 0 and start >= 0 and mind[start] >= 0) else int(np.argmax(mind))      # argmax: the first (lowest-index) maximum; non-candidates are -1
        out_idx[k], out_d2[k] = p, mind[p]
        mind[p] = -1
        with np.errstate(all="ignore"):
            d = pos - pos[p]
            d2 = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F32)
        cand = mind >= 0
        mind[cand] = np.minimum(mind[cand], d2[cand])
    return out_idx, out_d2


# ---- the random stream and the arithmetic of sample_spatial / sample_near_surface ----
def uniforms(N, seed, stream_id):
    """Philox4x32-10, key (seed_lo, seed_hi), counter (i, stream_id, 0, 0): words 0..2 -> (x >> 8) * 2^-24 -> [N,3] f32"""
    ctr = np.zeros((N, 4), np.uint32)
    ctr[:, 0] = np.arange(N)
    ctr[:, 1] = stream_id
    key = np.broadcast_to(np.array([seed & 0xffffffff, (seed >> 32) & 0xffffffff], np.uint32), (N, 2))
    return ((philox4x32_10(ctr, key)[:, :3] >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)).astype(F32)


def vertex_normals_unit(verts, faces):
    """spatial_sampling.py:70-76: the normalised sum of the UNIT face normals (torch ops in float32; compared with a tolerance where it is compared at all)"""
    import torch
    v, f = torch.from_numpy(np.asarray(verts, F32)), torch.from_numpy(np.asarray(faces).astype(np.int64))
    areas = torch.linalg.cross(v[f[:, 1]] - v[f[:, 0]], v[f[:, 2]] - v[f[:, 0]], dim=-1)
    normals = torch.nn.functional.normalize(areas, dim=-1)
    vn = torch.zeros((v.shape[0], 3, 3), dtype=v.dtype)
    vn.scatter_add_(0, f.unsqueeze(-1).expand(f.shape[0], 3, 3), normals.unsqueeze(1).expand(f.shape[0], 3, 3))
    return torch.nn.functional.normalize(vn.sum(dim=1), dim=-1).numpy()


def near_surface_offsets(base, faces, face_index, uvw, vnormal, r, threshold):
    """spatial_sampling.py:87-89 in float32: n = (vn0 u + vn1 v) + vn2 w;  base + (threshold * (r * 2 - 1)) * n"""
    n = vertex_attr(vnormal, faces, face_index, uvw)
    return (np.asarray(base, F32) + (F32(threshold) * (np.asarray(r, F32) * F32(2) - F32(1))) * n).astype(F32), n.astype(F32)


# ---- PBRMesh.__call__: the three kinds of attribute ----
def vertex_attr(attr, faces, face_index, uvw):
    """(attr[f0] u + attr[f1] v) + attr[f2] w in float32, f = faces[face_index]"""
    uvw = np.asarray(uvw, F32)
    return interp_corners(np.asarray(attr, F32), np.asarray(faces)[face_index], uvw[:, 0:1], uvw[:, 1:2], uvw[:, 2:3]).astype(F32)


def texture_attr(tex, uvs_2d, faces_2d, face_index, uvw, dtype=np.float64):
    """uv = (uv0 u + uv1 v) + uv2 w in float32 (as the kernel forms it), then grid_sample's reflection lookup in `dtype` with the uv itself as the grid
    coordinate (pixel_ref.reflect_index + grid_blend; np.float32: the kernel's own bits) -> values [N,C], the uv, and the coordinate pair (ix, iy)"""
    uv = vertex_attr(uvs_2d, faces_2d, face_index, uvw)
    tex = np.asarray(tex, dtype)
    H, W = tex.shape[:2]
    ix, iy = reflect_index(uv[:, 0], W, dtype), reflect_index(uv[:, 1], H, dtype)
    return grid_blend(tex, ix, iy, dtype), uv, ix, iy


# ---- fixture G22 (tests/golden/make_golden_spatial_sampling.py) ----
def g22():
    return np.load(os.path.join(GOLD, "g22_spatial_sampling.npz"))


def tex_bound(tex):
    """G18's bilinear bound (14 M + 4 (W + H) R) u -- M the largest texel, R the texels' range -- with the reflection fold added: the fold is a subtraction, a
    quotient and a sum more on a coordinate of up to twice the size, another 4 (W + H) R u"""
    t = np.asarray(tex, np.float64) / 255.0
    H, W = t.shape[:2]
    return (14.0 * np.abs(t).max() + 8.0 * (W + H) * (t.max() - t.min())) * U


# ---- the inputs of the bit-for-bit texture-lookup tests (tests/test_spatial_sampling_{cpu,gpu}.py)
REFLECT_SIZES = ((1, 1), (1, 4), (3, 2))          # (H, W)
REFLECT_HUGE = 1e12                                # a flip count past int32: the GPU is compared with the restatement there, torch is not asked


def reflect_case(H, W, N=257):
    """-> (textures {C: [H,W,C] f32} for C = 1, 3, 4, with negative texels, faces_2d [N,3], uvs_2d [N,2], face_index [N], uvw [N,3]): sample i reads uvs_2d[i] through
    the face (i, i, i) with weights (1, 0, 0).  Per axis of S texels: the texel centres, the outer half-pixel rim (it clips onto the border texel: ix == S - 1, the
    absent tap), the edges, two points moved one to four spans (of 2) out on either side (odd and even flips), +-REFLECT_HUGE, the rest uniform in [-7, 7]"""
    rng = np.random.default_rng(22 + 100 * H + W)
    tex = {C: (rng.uniform(0.1, 1.0, (H, W, C)) * np.where(np.arange(C) % 2 == 0, -1.0, 1.0)).astype(F32) for C in (1, 3, 4)}          # even channels negative

    def axis(S, shift):
        g = [(2 * i + 1) / S - 1 for i in range(S)] + [-1 + 0.5 / S, 1 - 0.5 / S, -1 + 0.25 / S, 1 - 0.25 / S, -1.0, 1.0, REFLECT_HUGE, -REFLECT_HUGE]
        g += [b + s * 2 * k for b in (0.3, -0.55) for k in (1, 2, 3, 4) for s in (1, -1)]
        return np.roll(np.concatenate([np.array(g, F32), rng.uniform(-7.0, 7.0, N - len(g)).astype(F32)]), shift)
    idx = np.arange(N, dtype=np.int32)
    return tex, np.stack([idx, idx, idx], -1), np.stack([axis(W, 0), axis(H, 40)], -1), idx, np.tile(np.array([1, 0, 0], F32), (N, 1))

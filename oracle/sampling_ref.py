"""Geometry sampling for the field stage (TEST INFRASTRUCTURE ONLY): the numpy restatements that tests/test_sampling_gpu.py holds the HIP kernels to.
Each is pinned in tests/test_sampling_cpu.py before the GPU test leans on it: the equal-steps sampler to fixture G14's captured samples
(tests/golden/make_golden_sampling.py) bit for bit, Philox4x32-10 to the Random123 known-answer vectors, the farthest-point sampling to an example
worked by hand."""
import os

import numpy as np

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
    ctr = np.zeros((N, 4), np.uint32)
    ctr[:, 0] = np.arange(N)
    key = np.broadcast_to(np.array([seed & 0xffffffff, (seed >> 32) & 0xffffffff], np.uint32), (N, 2))
    r = philox4x32_10(ctr, key)
    u01 = (r >> np.uint32(8)).astype(F32) * F32(2.0 ** -24)
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

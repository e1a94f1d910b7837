"""Geometry sampling for the field stage (reference: TextureTools/texturetools/geometry/sampling/ -- edge_sampling.py, surface_sampling.py, __init__.py:19-73
geomerty_sampling -- and the farthest-point thinning of pipeline.py:387-407 / 507-514, which the reference takes from fpsample [3p]).

The edge selection is index bookkeeping and runs as torch ops on whatever device the mesh is on (CPU included); the samplers and the farthest-point
sampling are HIP kernels (csrc/sampling.hip) and need the GPU.  Two things are builder-defined, because the reference's own cannot be reproduced:
  * sample_surface's random stream -- the reference draws from the CUDA generator; here sample i reads Philox4x32-10 with key (seed_lo, seed_hi) and
    counter (i, 0, 0, 0), each word x giving (x >> 8) * 2^-24;
  * the first farthest point -- fpsample's start is not pinned (the package is absent); here it is index 0 unless the caller names another.
Prefix sums (edge lengths, face weights) accumulate in float64 and round to float32 per element, as torch.cumsum does on the CPU."""
import math
import os
from time import perf_counter

import numpy as np
import torch


def select_sharp_edges(vertices, faces, normals=None, angle_threhold_deg=15.0):
    """vertices [V,3] f32, faces [F,3] int, normals [F,3] f32 (optional; else normalised face cross products) ->
    edges_unique [E,2] int64 (each row ascending, rows in lexicographic order), mask_nonmanifold [E] bool (the edge does not have exactly two faces),
    mask_sharp [E] bool (two faces whose normals' cosine_similarity is NOT above cos(angle_threhold_deg)).  edge_sampling.py:6-46."""
    assert 0.0 <= angle_threhold_deg <= 180.0, "angle_threhold_deg should be in [0.0, 180.0], but %s" % angle_threhold_deg
    faces = faces.long()
    F, V = faces.shape[0], int(vertices.shape[0])
    corners = torch.stack([faces, faces.roll(-1, dims=1)], dim=-1).reshape(-1, 2)          # (0,1), (1,2), (2,0) of every face, face-major
    lo, hi = corners.min(dim=1).values, corners.max(dim=1).values
    keys, inverse, counts = torch.unique(lo * V + hi, return_inverse=True, return_counts=True)      # ascending keys = lexicographic (lo, hi)
    edges_unique = torch.stack([keys // V, keys % V], dim=1)
    two = counts == 2
    # the two faces of every two-face edge: half-edges grouped by edge, in face order
    order = torch.argsort(inverse, stable=True)
    first = torch.cumsum(counts, dim=0) - counts
    e2 = torch.where(two)[0]
    f0, f1 = order[first[e2]] // 3, order[first[e2] + 1] // 3
    if normals is None:
        areas = torch.linalg.cross(vertices[faces[:, 1]] - vertices[faces[:, 0]], vertices[faces[:, 2]] - vertices[faces[:, 0]], dim=-1)
        normals = torch.nn.functional.normalize(areas, dim=-1)
    cos = torch.nn.functional.cosine_similarity(normals[f0], normals[f1], dim=-1)
    smooth = cos > math.cos(math.radians(angle_threhold_deg))
    mask_sharp = two.clone()
    mask_sharp[e2[smooth]] = False
    return edges_unique, torch.logical_not(two), mask_sharp


def _prefix_f32(x):
    return torch.cumsum(x.double(), dim=0).float()


def sample_on_edges_equal_steps(vertices, edges, edges_mask=None, N=10_000_000):
    """sample_on_edges_v2 (edge_sampling.py:84-119): N equally spaced samples along the (selected) edges laid end to end.
    -> samples [N,3] f32, edge_index [N] int64 into `edges`, edge_t [N,1] f32.  edge_t is clamped to [0, 1] (the reference's is not: rounded running lengths
    let it pass 1 by a few 1e-4, which puts the sample beyond the end of the edge it reports; with exact running lengths the two agree bit for bit)."""
    from . import ops
    ids = torch.where(edges_mask)[0] if edges_mask is not None else torch.arange(edges.shape[0], device=edges.device)
    assert ids.numel() > 0, "edges selected by edges_mask are empty"
    sel = edges[ids]
    v = vertices.float()
    length = torch.norm(v[sel[:, 1]] - v[sel[:, 0]], dim=-1)
    cum = _prefix_f32(length)
    start = torch.cat([cum.new_zeros(1), cum[:-1]])
    samples, edge_index, edge_t = ops.sample_edges_equal_steps(v.contiguous(), sel.to(torch.int32).contiguous(), start.contiguous(), length.contiguous(),
                                                               float(cum[-1]), N, edge_ids=ids.to(torch.int32).contiguous())
    return samples, edge_index.long(), edge_t.unsqueeze(-1)


def select_and_sample_on_edges(vertices, faces, normals=None, method="equal_steps", angle_threhold_deg=15.0, N=10_000_000, seed=666):
    """edge_sampling.py:122-158.  (None, None, None) when the mesh has no sharp and no non-manifold edge."""
    assert method in ["probability", "equal_steps"]
    if method == "probability":
        raise NotImplementedError("method 'probability' (sample_on_edges_v1: torch.multinomial on the CUDA generator, a stream no other device reproduces) "
                                  "is not built; use method='equal_steps', the one the pipeline calls")
    edges, mask_nonmanifold, mask_sharp = select_sharp_edges(vertices, faces, normals=normals, angle_threhold_deg=angle_threhold_deg)
    edges_mask = torch.logical_or(mask_nonmanifold, mask_sharp)
    if edges_mask.sum() == 0:
        print("no sharp edges or nonmanifold edges on mesh")
        return None, None, None
    return sample_on_edges_equal_steps(vertices, edges, edges_mask, N=N)


def sample_surface(vertices, faces, areas=None, N=10_000_000, seed=666):
    """surface_sampling.py:5-35 on the defined Philox stream (module docstring).  areas [F,3]: the faces' cross products (computed when None).
    -> samples [N,3] f32, face_index [N] int64, face_uvw [N,3] f32."""
    from . import ops
    faces = faces.long()
    v = vertices.float()
    if areas is None:
        areas = torch.linalg.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]], dim=-1)
    cum = _prefix_f32(torch.norm(areas, p=2, dim=-1))
    samples, face_index, uvw = ops.sample_surface(v.contiguous(), faces.to(torch.int32).contiguous(), cum.contiguous(), N, 666 if seed is None else seed)
    return samples, face_index.long(), uvw


def farthest_point_sampling(points, n_samples, mask=None, start_idx=0, return_d2=False, device="cuda:0"):
    """exact farthest-point sampling of points [N,3] (tensor on the GPU, or numpy array: moved to `device`, results come back as numpy).
    -> idx [n_samples] int32; return_d2: also each pick's squared distance to the points picked before it (+inf for the first).
    Masked-out points and points with a non-finite coordinate are never picked; ties go to the lower index; no index twice; when the candidates run out,
    the rest is -1.  start_idx: the first pick (fpsample's is not pinned; ours is index 0), -1 = the lowest valid index."""
    from . import ops
    as_numpy = isinstance(points, np.ndarray)
    if as_numpy:
        points = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).to(device)
        mask = torch.from_numpy(np.ascontiguousarray(mask).astype(np.uint8)).to(device) if mask is not None else None
    out = ops.fps(points.float().contiguous(), n_samples, mask=mask, start=start_idx, want_d2=return_d2)
    if as_numpy:
        return tuple(o.cpu().numpy() for o in out) if return_d2 else out.cpu().numpy()
    return out


def geometry_sampling(input_mesh_path, sharp_path, coarse_path, scale=1.0, N=10_000_000, angle_threhold_deg=15.0, method="equal_steps",
                      merge_close_vertices=False, device="cuda:0"):
    """geomerty_sampling (geometry/sampling/__init__.py:19-73): N surface samples -> coarse_path, N samples on the sharp and non-manifold edges ->
    sharp_path (an empty cloud when the mesh has none), both binary PLY.  merge_close_vertices: vertices at bit-equal positions become one,
    so an edge shared across a UV seam or between STL corners counts both its faces.  This is EXACT-position merging (-0.0 equals 0.0): the reference calls
    trimesh.merge_vertices [3p], which also merges positions that agree only after rounding to its tolerance; vertices that close but not equal stay apart here."""
    from . import meshes
    time_log = dict()
    t0 = perf_counter()
    if input_mesh_path.lower().endswith(".obj"):
        verts, faces = meshes.load_obj(input_mesh_path)[:2]          # position indices: per-corner UVs do not split the geometry
    else:
        verts, faces = meshes.load_mesh(input_mesh_path)[:2]
    if merge_close_vertices:
        _, first, inv = np.unique(np.ascontiguousarray(verts + np.float32(0.0)).view(np.uint32).reshape(-1, 3), axis=0, return_index=True, return_inverse=True)
        order = np.argsort(first)                    # keep the file's vertex order
        rank = np.empty_like(order)
        rank[order] = np.arange(len(order))
        verts, faces = verts[first[order]], rank[inv.reshape(-1)][faces]
    vertices = torch.from_numpy(np.ascontiguousarray(verts, dtype=np.float32)).to(device)
    if scale is not None and scale != 1.0:
        vertices = vertices * scale
    faces = torch.from_numpy(np.ascontiguousarray(faces).astype(np.int64)).to(device)
    areas = torch.linalg.cross(vertices[faces[:, 1]] - vertices[faces[:, 0]], vertices[faces[:, 2]] - vertices[faces[:, 0]], dim=-1)
    normals = torch.nn.functional.normalize(areas, dim=-1)
    time_log["load whole mesh"] = perf_counter() - t0

    t0 = perf_counter()
    surface_points = sample_surface(vertices, faces, areas=areas, N=N, seed=666)[0]
    time_log["sample on surface"] = perf_counter() - t0

    t0 = perf_counter()
    edge_points = select_and_sample_on_edges(vertices, faces, normals=normals, method=method, angle_threhold_deg=angle_threhold_deg, N=N, seed=666)[0]
    time_log["select and sample on sharp edges"] = perf_counter() - t0

    t0 = perf_counter()
    for path, pts in ((sharp_path, edge_points), (coarse_path, surface_points)):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        meshes.save_ply(path, pts.cpu().numpy() if pts is not None else np.zeros((0, 3), np.float32))
    time_log["export point cloud"] = perf_counter() - t0
    return time_log

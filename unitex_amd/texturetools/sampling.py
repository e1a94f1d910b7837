"""Geometry sampling for the field stage (reference: TextureTools/texturetools/geometry/sampling/ -- edge_sampling.py, surface_sampling.py, __init__.py:19-73
geomerty_sampling -- and the farthest-point thinning of pipeline.py:387-407 / 507-514, which the reference takes from fpsample [3p]).

The edge selection is index bookkeeping and runs as torch ops on whatever device the mesh is on (CPU included); the samplers and the farthest-point
sampling are HIP kernels (csrc/sampling.hip) and need the GPU.  Two things are builder-defined, because the reference's own cannot be reproduced:
  * sample_surface's random stream -- the reference draws from the CUDA generator; here sample i reads Philox4x32-10 with key (seed_lo, seed_hi) and
    counter (i, 0, 0, 0), each word x giving (x >> 8) * 2^-24;
  * the first farthest point -- fpsample's start is not pinned (the package is absent); here it is index 0 unless the caller names another.
Prefix sums (edge lengths, face weights) accumulate in float64 and round to float32 per element, as torch.cumsum does on the CPU.
The second half of the file is the rest of that package: spatial_sampling.py (sample_spatial, sample_near_surface, on ops.closest_point in place of cuBVH [3p]),
uv_sampling.py with PBRMesh.__call__ (sample_pbr_mesh, pbr_attributes) and texture_sampling of __init__.py:76-121."""
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


# ---- spatial sampling (geometry/sampling/spatial_sampling.py) and material sampling (uv_sampling.py, PBRMesh.__call__, texture_sampling) ----
# Three readings of the reference are kept as they stand, on purpose:
#   * sample_spatial draws from [0, 1)^3 (torch.rand), whatever the mesh's bounding box is;
#   * sample_near_surface's vertex normals are the normalised sum of the UNIT face normals (its own scatter_add), not the area weighting used elsewhere;
#   * PBRMesh.__call__ hands the interpolated uv to grid_sample as the grid coordinate itself -- the map from [0, 1] to [-1, 1] is trimesh_to_pbr_mesh's, done once
#     when a mesh is converted (pbr_mesh_from_textured below), not the lookup's.
# The random stream is sample_surface's with another stream id: counter (i, 1, 0, 0) for sample_spatial, (i, 2, 0, 0) for the near-surface deltas.
def _bvh_for(vertices, faces, bvh):
    from . import ops
    if bvh is not None:
        return bvh
    return ops.BVH(vertices.float().contiguous(), faces.to(torch.int32).contiguous())


def _project(bvh, samples):
    from . import ops
    out = ops.closest_point(bvh, samples, want=("face", "uvw"))
    return samples, out["face"].long(), out["uvw"]


def sample_spatial(vertices, faces, bvh=None, N=10_000_000, seed=666):
    """spatial_sampling.py:11-37: N uniform points and their projection onto the mesh.  The points are drawn from [0, 1)^3, exactly as the reference's
    torch.rand((N, 3)) -- NOT from the mesh's bounding box; that quirk is kept.  bvh: an ops.BVH of (vertices, faces), built when None (the reference takes a
    cuBVH [3p]).  -> samples [N,3] f32, face_index [N] int64, face_uvw [N,3] f32 (the nearest face and the weights of its corners, ops.closest_point)."""
    from . import ops
    bvh = _bvh_for(vertices, faces, bvh)
    with torch.cuda.device(vertices.device):
        samples = ops.sample_offsets(N, 666 if seed is None else seed, 1)
    return _project(bvh, samples)


def unit_normal_vertex_normals(vertices, faces, normals=None):
    """spatial_sampling.py:70-76: per vertex the normalised sum of the UNIT normals of its faces (torch ops)"""
    faces = faces.long()
    if normals is None:
        areas = torch.linalg.cross(vertices[faces[:, 1]] - vertices[faces[:, 0]], vertices[faces[:, 2]] - vertices[faces[:, 0]], dim=-1)
        normals = torch.nn.functional.normalize(areas, dim=-1)
    vn = torch.zeros((vertices.shape[0], 3, 3), dtype=vertices.dtype, device=vertices.device)
    vn.scatter_add_(0, faces.unsqueeze(-1).expand(faces.shape[0], 3, 3), normals.unsqueeze(1).expand(faces.shape[0], 3, 3))
    return torch.nn.functional.normalize(vn.sum(dim=1), dim=-1)


def sample_near_surface(vertices, faces, areas=None, normals=None, bvh=None, N=10_000_000, N_radio=1.1, seed=666, distance_threhold=1.0, depth=8):
    """spatial_sampling.py:40-91, line by line: int(N * N_radio) surface samples (sample_surface, stream 0) cut to N, each moved along the interpolated vertex
    normal (unit_normal_vertex_normals; the interpolated normal is not renormalised) by threshold * (2 r - 1) per component, r from stream 2 and
    threshold = distance_threhold * 2 / 2^depth; then projected back onto the mesh.  -> samples [N,3] f32, face_index [N] int64, face_uvw [N,3] f32."""
    from . import ops
    seed = 666 if seed is None else seed
    threshold = distance_threhold * (2.0 / (2 ** depth))
    v = vertices.float()
    faces = faces.long()
    if areas is None:
        areas = torch.linalg.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]], dim=-1)
    if normals is None:
        normals = torch.nn.functional.normalize(areas, dim=-1)
    vnormal = unit_normal_vertex_normals(v, faces, normals)
    bvh = _bvh_for(v, faces, bvh)
    base, face_index, face_uvw = sample_surface(v, faces, areas=areas, N=int(N * N_radio), seed=seed)
    base, face_index, face_uvw = base[:N], face_index[:N], face_uvw[:N]          # maybe fewer than N, as in the reference
    n = base.shape[0]
    samples = ops.sample_offsets(n, seed, 2, base=base.contiguous(), faces=faces.to(torch.int32).contiguous(), face_index=face_index.to(torch.int32).contiguous(),
                                 uvw=face_uvw.contiguous(), vnormal=vnormal.contiguous(), threshold=threshold)
    return _project(bvh, samples)


PBR_DEFAULT = {"albedo": (0.0, 0.0, 0.0), "metallic": (0.0,), "roughness": (1.0,), "bump": (0.0, 0.0, 0.0)}          # PBRDefault, mesh/structure_v2.py:18-22
PBR_KEYS = ("albedo", "metallic", "roughness", "bump")


def pbr_mesh_from_textured(mesh, device="cuda:0"):
    """a TexturedMesh (or anything with .vertices .faces .uv .texture and optional .metallic_roughness .bump) -> the dict of arrays sample_pbr_mesh takes, as
    trimesh_to_pbr_mesh builds a PBRMesh (mesh/structure_v2.py:282-303): uvs_2d = uv * 2 - 1, faces_2d = faces, images / 255 with the bottom row first,
    metallic = the blue and roughness = the green channel of the metallic-roughness image."""
    def img(a):
        return torch.from_numpy(np.array(a)).to(device).float().div(255.0).flip(0).contiguous()
    out = {"vertices": torch.from_numpy(np.ascontiguousarray(mesh.vertices, dtype=np.float32)).to(device),
           "faces": torch.from_numpy(np.ascontiguousarray(mesh.faces).astype(np.int64)).to(device)}
    if getattr(mesh, "uv", None) is not None:
        out["uvs_2d"] = torch.from_numpy(np.ascontiguousarray(mesh.uv, dtype=np.float32)).to(device).mul(2.0).sub(1.0)
        out["faces_2d"] = out["faces"]
    if getattr(mesh, "texture", None) is not None:
        out["albedo"] = img(mesh.texture)
    if getattr(mesh, "metallic_roughness", None) is not None:
        mr = img(mesh.metallic_roughness)
        out["metallic"], out["roughness"] = mr[..., [2]].contiguous(), mr[..., [1]].contiguous()
    if getattr(mesh, "bump", None) is not None:
        out["bump"] = img(mesh.bump)
    return out


def pbr_attributes(mesh, face_index, face_uvw):
    """PBRMesh.__call__ (mesh/structure_v2.py:105-135) on a dict of arrays: vertices, faces and optionally uvs_2d, faces_2d, albedo, metallic, roughness, bump --
    each attribute a constant [C], a per-vertex array [V,C] or a texture [H,W,C]; a missing one takes PBRDefault's value.  One launch (ops.sample_attrs).
    -> dict name -> [N,C] f32."""
    from . import ops
    dev = face_index.device
    attrs = {}
    for k in PBR_KEYS:
        a = mesh.get(k)
        attrs[k] = torch.tensor(PBR_DEFAULT[k], dtype=torch.float32, device=dev) if a is None else a.to(dev).float().contiguous()
    i32 = lambda t: t.to(dev).to(torch.int32).contiguous() if t is not None else None
    uvs, faces_2d = mesh.get("uvs_2d"), mesh.get("faces_2d")
    if uvs is None or faces_2d is None:          # a uv table without its index (or the reverse) serves no lookup: PBRMesh reads them only for a texture, and only together
        uvs = faces_2d = None
    return ops.sample_attrs(attrs, face_index.to(torch.int32).contiguous(), face_uvw.float().contiguous(), faces=i32(mesh["faces"]), faces_2d=i32(faces_2d),
                            uvs_2d=uvs.to(dev).float().contiguous() if uvs is not None else None)


def sample_pbr_mesh(pbr_mesh, N=10_000_000, seed=666):
    """uv_sampling.py:9-26: N surface samples (sample_surface) and the material at each.  pbr_mesh: a dict of arrays (pbr_attributes) or a TexturedMesh
    (converted by pbr_mesh_from_textured).  A list of meshes (the reference's PBRScene) is not built.
    -> samples [N,3] f32, face_index [N] int64, face_attr {albedo [N,3], metallic [N,1], roughness [N,1], bump [N,3]}."""
    if isinstance(pbr_mesh, (list, tuple)):
        raise NotImplementedError("sample_pbr_mesh takes one mesh; a list of meshes (PBRScene) is not built")
    if not isinstance(pbr_mesh, dict):
        pbr_mesh = pbr_mesh_from_textured(pbr_mesh)
    v, faces = pbr_mesh["vertices"].float(), pbr_mesh["faces"].long()
    samples, face_index, face_uvw = sample_surface(v, faces, areas=pbr_mesh.get("areas"), N=N, seed=seed)
    return samples, face_index, pbr_attributes(pbr_mesh, face_index, face_uvw)


def albedo_to_u8(albedo):
    """round(clamp(albedo, 0, 1) * 255) as uint8 -- this build's rule for the colours of a point cloud"""
    return torch.round(albedo.clamp(0.0, 1.0) * 255.0).to(torch.uint8)


def texture_sampling(input_mesh_path, output_mesh_path, N=10_000_000, device="cuda:0"):
    """texture_sampling (geometry/sampling/__init__.py:76-121): a coloured point cloud of a textured mesh, N surface samples with the albedo at each, written as
    binary PLY.  The mesh is read by meshes.load_glb and its material by meshes.load_material_textures.  Colours are round(clamp(albedo, 0, 1) * 255): the
    reference hands the float albedo to trimesh.Trimesh(vertex_colors=...), whose conversion to uint8 is third-party and unpinned."""
    from types import SimpleNamespace
    from . import meshes
    time_log = dict()
    t0 = perf_counter()
    verts, faces, uvs, texture = meshes.load_glb(input_mesh_path)
    if meshes._glb_chunks(input_mesh_path)[0].get("materials"):
        tex = meshes.load_material_textures(input_mesh_path)
    else:                                        # a file without a material is an untextured mesh: PBRDefault's values throughout
        tex = {"metallic_roughness": None, "normal": None}
    time_log["load scene"] = perf_counter() - t0
    t0 = perf_counter()
    mesh = pbr_mesh_from_textured(SimpleNamespace(vertices=verts, faces=faces, uv=uvs, texture=texture, metallic_roughness=tex["metallic_roughness"],
                                                  bump=tex["normal"]), device=device)
    time_log["move mesh to gpu"] = perf_counter() - t0
    t0 = perf_counter()
    samples, face_index, face_attr = sample_pbr_mesh(mesh, N=N, seed=666)
    time_log["sample on mesh"] = perf_counter() - t0
    t0 = perf_counter()
    samples_np, colors = samples.cpu().numpy(), albedo_to_u8(face_attr["albedo"]).cpu().numpy()
    time_log["move samples to cpu"] = perf_counter() - t0
    t0 = perf_counter()
    os.makedirs(os.path.dirname(os.path.abspath(output_mesh_path)), exist_ok=True)
    meshes.save_ply(output_mesh_path, samples_np, colors_u8=colors)
    time_log["export point cloud"] = perf_counter() - t0
    return time_log

"""Ray casting on the LBVH: the reference's texturetools/raytracing package (RayTracing, ray_tracing) and its raytracing/check_visibility.py (self_rt, cross_rt,
sphere_rt, sphere_rt_nvdiffrast) with the reference's names and shapes, on this library's HIP kernels (csrc/raycast.hip through ops.BVH).

Deviations from the reference, on purpose:
- Every backend name that is accepted ('aprmis', 'slang', 'optix', 'triro') maps to ONE closest hit: the smallest t >= 0, both triangle sides, ties to the smallest
  face id.  The Slang walk's quirks (a negative t accepted, the last triangle met wins) are NOT kept here; ops.BVH.trace keeps them, id only, for the bit-equal
  visibility masks of the back-projection.  'nvdiffrast' (the raster-as-ray-tracer backend) raises NotImplementedError.
- front is this library's rule, dot(d, (v1 - v0) x (v2 - v0)) < 0: the reference's OptiX backend is a third-party library and its Slang backend returns None, so the
  reference does not pin it.
- A miss has loc = 0, uv = 0, front = False (the reference's Slang buffers start as zeros), tri_idx = -1.
- self_rt draws its directions from a defined stream (Philox4x32-10, Marsaglia's method: ops.sphere_directions), not torch.randn + normalize, in one fused launch
  that materialises no ray; chunk_size is accepted and ignored -- there is nothing to chunk.
- cross_rt: a segment is blocked iff a triangle is hit with 0 <= t < 1 on the UNNORMALISED segment outer -> point; the reference compares |loc - o| < |p - o|, which
  agrees away from rounding ties.  A miss counts as not blocked; the reference compares against whatever loc a miss carries."""
import math

import torch

_BACKENDS = ("aprmis", "slang", "optix", "triro")
DEFAULT_RAY_TRACING_BACKEND = "aprmis"


def _ops():
    from . import ops
    return ops


def _check_mesh(vertices, faces):
    if not torch.is_tensor(vertices) or not vertices.is_floating_point() or vertices.dim() != 2 or vertices.shape[1] != 3:
        raise ValueError("RayTracing: vertices must be a floating-point [V, 3] tensor, got %s" % _describe(vertices))
    if not torch.is_tensor(faces) or faces.is_floating_point() or faces.dtype == torch.bool or faces.dim() != 2 or faces.shape[1] != 3 or faces.shape[0] < 1:
        raise ValueError("RayTracing: faces must be an integer [F >= 1, 3] tensor, got %s" % _describe(faces))
    if vertices.device != faces.device:
        raise ValueError("RayTracing: vertices are on %s, faces on %s" % (vertices.device, faces.device))
    if vertices.device.type != "cuda":
        raise ValueError("RayTracing: the mesh must live on the GPU, got %s" % (vertices.device,))


def _describe(x):
    return "%s %s" % (x.dtype, tuple(x.shape)) if torch.is_tensor(x) else type(x).__name__


def _check_rows(what, x, min_dims=1):
    if not torch.is_tensor(x) or not x.is_floating_point():
        raise ValueError("%s must be a floating-point tensor, got %s" % (what, _describe(x)))
    if x.dim() < min_dims or x.shape[-1] != 3:
        raise ValueError("%s is %s, expected [..., 3]%s" % (what, tuple(x.shape), "" if min_dims == 1 else " with at least %d dimensions" % min_dims))


def _same_device(what, a, b):
    if a.device != b.device:
        raise ValueError("%s are on different devices: %s and %s" % (what, a.device, b.device))


def _check_n_rays(n_rays, hi):
    if isinstance(n_rays, bool) or not isinstance(n_rays, int) or not 1 <= n_rays <= hi:
        raise ValueError("n_rays must be an integer in 1 .. %d, got %r" % (hi, n_rays))


class RayTracing:
    """RayTracing of the reference on ops.BVH.  vertices [V,3] float, faces [F,3] integer (int64 as in the reference, or int32)."""

    def __init__(self, vertices, faces, backend=DEFAULT_RAY_TRACING_BACKEND, **kwargs):
        if backend in ("nvdiffrast", "nvdiff"):
            raise NotImplementedError("backend %r (a rasteriser standing in for a ray tracer) is not built; use 'aprmis'" % (backend,))
        if backend not in _BACKENDS:
            raise NotImplementedError("backend %r is not supported (one of %s)" % (backend, ", ".join(_BACKENDS)))
        self.backend = backend
        self.bvh = None
        self.update_raw(vertices, faces)

    def update_raw(self, vertices, faces):
        _check_mesh(vertices, faces)
        self.V, self.F = vertices.shape[0], faces.shape[0]
        self.bvh = _ops().BVH(vertices.to(torch.float32).contiguous(), faces.to(torch.int32).contiguous())

    def intersects_closest(self, rays_o, rays_d, stream_compaction=False):
        """(hit bool [...], front bool [...], tri_idx int64 [...] (-1: miss), loc f32 [..., 3], uv f32 [..., 2]) for rays_o, rays_d [..., 3], broadcast against each
        other.  stream_compaction=False is accepted because check_visibility.py passes it; True is not built."""
        if stream_compaction:
            raise NotImplementedError("intersects_closest: stream_compaction=True is not built")
        _check_rows("intersects_closest: rays_o", rays_o)
        _check_rows("intersects_closest: rays_d", rays_d)
        _same_device("intersects_closest: rays_o and rays_d", rays_o, rays_d)
        try:
            rays_o, rays_d = torch.broadcast_tensors(rays_o, rays_d)
        except RuntimeError:
            raise ValueError("intersects_closest: rays_o %s and rays_d %s do not broadcast" % (tuple(rays_o.shape), tuple(rays_d.shape)))
        batch = rays_o.shape[:-1]
        out = self.bvh.intersect(rays_o.reshape(-1, 3), rays_d.reshape(-1, 3), want=("tid", "loc", "uv", "front"))
        tid = out["tid"].to(torch.int64)
        return ((tid >= 0).reshape(batch), out["front"].bool().reshape(batch), tid.reshape(batch), out["loc"].reshape(*batch, 3), out["uv"].reshape(*batch, 2))


def ray_tracing(vertices, faces, rays_o, rays_d, backend=DEFAULT_RAY_TRACING_BACKEND):
    return RayTracing(vertices, faces, backend=backend).intersects_closest(rays_o, rays_d)


def _tree(bvh):
    """the ops.BVH of a RayTracing, or the ops.BVH itself"""
    if isinstance(bvh, RayTracing):
        return bvh.bvh
    if hasattr(bvh, "points_enclosed") and hasattr(bvh, "occluded") and hasattr(bvh, "intersect"):
        return bvh
    raise ValueError("bvh must be a RayTracing or an ops.BVH, got %s" % type(bvh).__name__)


def _seed(seed):
    return int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)


def self_rt(bvh, points, n_rays=32, chunk_size=1_000_000, seed=666, dirs=None):
    """inner-point mask, bool of points' batch shape: a point is inner iff every one of its n_rays (1 .. 1024) random rays hits the mesh.  seed=None draws a fresh
    seed from torch's generator.  chunk_size is accepted and ignored (one fused launch, no ray is materialised).  dirs [..., n_rays, 3] (beyond the reference:
    recorded draws, for tests) is read in place of the stream."""
    _check_n_rays(n_rays, 1024)
    _check_rows("self_rt: points", points)
    tree = _tree(bvh)
    batch = points.shape[:-1]
    if dirs is not None:
        if not torch.is_tensor(dirs) or tuple(dirs.shape) != tuple(batch) + (n_rays, 3):
            raise ValueError("self_rt: dirs is %s, expected %s" % (_describe(dirs), tuple(batch) + (n_rays, 3)))
        dirs = dirs.reshape(-1, n_rays, 3)
    return tree.points_enclosed(points.reshape(-1, 3), n_rays, _seed(seed), dirs=dirs).bool().reshape(batch)


def cross_rt(bvh, points, outer_points, chunk_size=32, exhaustive_mode=True):
    """bool mask: a point is kept iff EVERY segment from an outer point to it is blocked by the mesh.  exhaustive_mode: points [..., 3] x outer_points [M, 3] -> mask
    of points' batch shape; otherwise paired points, outer_points [..., M, 3] (broadcast against each other) -> mask [...].  The outer points are taken chunk_size at a
    time and a point that some outer point sees is dropped from the later chunks, as the reference does."""
    if isinstance(chunk_size, bool) or not isinstance(chunk_size, int) or chunk_size < 1:
        raise ValueError("cross_rt: chunk_size must be an integer >= 1, got %r" % (chunk_size,))
    _check_rows("cross_rt: points", points, 1 if exhaustive_mode else 2)
    _check_rows("cross_rt: outer_points", outer_points, 1 if exhaustive_mode else 2)
    _same_device("cross_rt: points and outer_points", points, outer_points)
    tree = _tree(bvh)
    if exhaustive_mode:
        batch = points.shape[:-1]
        P, O = points.reshape(-1, 3), outer_points.reshape(-1, 3)
        N, M = P.shape[0], O.shape[0]
    else:
        try:
            points, outer_points = torch.broadcast_tensors(points, outer_points)
        except RuntimeError:
            raise ValueError("cross_rt: points %s and outer_points %s do not broadcast" % (tuple(points.shape), tuple(outer_points.shape)))
        batch = points.shape[:-2]
        M = points.shape[-2]
        P, O = points.reshape(-1, M, 3), outer_points.reshape(-1, M, 3)
        N = P.shape[0]
    idx = torch.arange(N, dtype=torch.int64, device=points.device)
    for i in range(0, M, chunk_size):
        if idx.numel() == 0:
            break
        if exhaustive_mode:
            o = O[i:i + chunk_size]
            p, o = torch.broadcast_tensors(P[idx].unsqueeze(1), o.unsqueeze(0))
        else:
            p, o = P[idx, i:i + chunk_size], O[idx, i:i + chunk_size]
        c = p.shape[1]
        blocked = tree.occluded(o.reshape(-1, 3), p.reshape(-1, 3)).reshape(-1, c).bool().all(dim=-1)
        idx = idx[blocked]
    mask = torch.zeros(N, dtype=torch.bool, device=points.device)
    mask[idx] = True
    return mask.reshape(batch)


def _sphere_rays(tree, n, sample_offset, seed, dirs=None):
    radius = math.sqrt(3) * (1.0 + sample_offset)
    if dirs is None:
        d = tree.sphere_directions(1, n, _seed(seed))[0]
    else:
        _check_rows("sphere directions", dirs)
        if tuple(dirs.shape) != (n, 3):
            raise ValueError("sphere directions are %s, expected %s" % (tuple(dirs.shape), (n, 3)))
        d = dirs
    return radius * d, d.neg()


def sphere_rt(bvh, n_rays=1_000, sample_offset=0.0, seed=666, dirs=None):
    """ids (int64, misses removed) of the faces hit first by n_rays rays from the sphere of radius sqrt(3) (1 + sample_offset) towards the origin.  The directions
    are the stream's for point 0 (ops.sphere_directions(1, n_rays, seed)) or dirs [n_rays, 3] (beyond the reference: recorded draws, for tests)."""
    _check_n_rays(n_rays, 2 ** 31 - 1)
    tree = _tree(bvh)
    o, d = _sphere_rays(tree, n_rays, sample_offset, seed, dirs)
    tid = tree.intersect(o, d, want=("tid",))["tid"].to(torch.int64)
    return tid[tid >= 0]


def sphere_rt_nvdiffrast(bvh, n_cameras=6, sample_offset=0.0):
    """the reference's 4 or 6 axis rays towards the origin (or n_cameras random ones, seed 666) -> ids of the faces hit (int64, misses removed)"""
    _check_n_rays(n_cameras, 2 ** 31 - 1)
    tree = _tree(bvh)
    radius = math.sqrt(3) * (1.0 + sample_offset)
    if n_cameras in (4, 6):
        axes = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, -1.0]][:n_cameras]
        a = torch.tensor(axes, dtype=torch.float32, device=tree.verts.device)
        o, d = radius * a, a.neg()
    else:
        o, d = _sphere_rays(tree, n_cameras, sample_offset, 666)
    tid = tree.intersect(o, d, want=("tid",))["tid"].to(torch.int64)
    return tid[tid >= 0]


def outer_face_mask(bvh, n_rays=1_000, sample_offset=0.0, seed=666):
    """bool [F]: the faces sphere_rt's rays hit first -- the mask callers build from its ids, scattered by the intersect launch itself"""
    _check_n_rays(n_rays, 2 ** 31 - 1)
    tree = _tree(bvh)
    o, d = _sphere_rays(tree, n_rays, sample_offset, seed)
    mask = torch.zeros(tree.faces.shape[0], dtype=torch.uint8, device=tree.verts.device)
    tree.intersect(o, d, want=(), face_mask=mask)
    return mask.bool()

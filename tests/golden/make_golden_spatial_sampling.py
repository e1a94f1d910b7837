#!/usr/bin/env python
"""Generate the spatial / material sampling fixture under tests/golden/ from the REFERENCE's own Python, through the stub machinery of make_golden.py
(imported from there, unchanged):

    python tests/golden/make_golden_spatial_sampling.py            # writes tests/golden/g22_spatial_sampling.npz

  G22 (a)  PBRMesh.__call__ (TextureTools/texturetools/mesh/structure_v2.py:105-135) on G19's scene (the two-chart cylinder and its plate): an albedo texture
           (8 x 8 in one call, 5 x 7 in another; stored as uint8 k, the value is k / 255), a per-vertex roughness, a constant metallic and no bump (PBRDefault's),
           at 64 fixed (face_idx, uvw) -- corners, edge points and interior points.  uvs_2d is G19's uv * 3 - 1.5, handed over as PBRMesh takes it: the lookup uses
           it as grid_sample's grid coordinate as it stands, so coordinates fall outside [-1, 1] (asserted) and the reflection padding is exercised.
  G22 (b)  sample_near_surface (geometry/sampling/spatial_sampling.py:40-91) on the 80-face icosphere, N = 257, depth 4.  Seams, for the duration of the call:
           * module `cubvh` [3p, absent] is a stub whose unsigned_distance records the samples it is handed and answers with a float64 brute force
             (oracle/closest_point_ref.py::brute_f64_face: distance and face by the plane-foot formula, and whether the face is the only one within 1024 u * scale of that distance);
           * torch.Generator(device='cuda') is a dummy, and torch.rand(..., device='cuda') hands back the fixture's own uniform numbers (Philox stream 2) on the CPU;
           * sample_surface is replaced by one that returns the stored surface samples (oracle/sampling_ref.py's restatement, int(N * 1.1) of them).
           Everything else -- threshold, vertex normals, the cut to N, the interpolated normal, the offset -- is the reference's own code on CPU tensors.
           Stored: the offset samples the reference handed to unsigned_distance, its vertex normals, the faces the float64 brute force named and which of them are alone (outside a convex edge both faces of the
           edge are nearest, and which one a brute force names is rounding).
Data only."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from make_golden import REF, install_stubs  # noqa: E402

N_NEAR, SEED, DEPTH, THRESHOLD, N_RADIO = 257, 666, 4, 1.0, 1.1


def _picks(F):
    """64 fixed (face_idx, uvw): the three corners, points on each edge, and interior points, over faces spread through the mesh"""
    w = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0.5, 0.5, 0), (0, 0.25, 0.75), (0.625, 0, 0.375), (0.25, 0.25, 0.5), (0.125, 0.75, 0.125)]
    face = np.array([(7 * i + 3 * (i // 8)) % F for i in range(64)], np.int64)
    uvw = np.array([w[i % 8] for i in range(64)], np.float32)
    return face, uvw


def g22(out):
    from oracle import sampling_ref as SR
    from oracle import closest_point_ref as CR
    fix = {}
    # ---- (a) PBRMesh.__call__
    S2 = importlib.import_module("TextureTools.texturetools.mesh.structure_v2")
    g19 = np.load(os.path.join(HERE, "g19_uv_project.npz"))
    verts, faces, uvs = g19["verts"], g19["faces"], g19["uvs"]
    uvs_2d = (uvs * np.float32(3.0) - np.float32(1.5)).astype(np.float32)
    rng = np.random.default_rng(22)
    tex8, tex57 = rng.integers(0, 256, (8, 8, 3), dtype=np.uint8), rng.integers(0, 256, (5, 7, 3), dtype=np.uint8)
    rough = (rng.integers(0, 256, (len(verts), 1)).astype(np.float32) / np.float32(255)).astype(np.float32)
    metallic = np.array([0.25], np.float32)
    face_idx, uvw = _picks(len(faces))
    fix.update(a_verts=verts, a_faces=faces, a_uvs_2d=uvs_2d, a_tex8=tex8, a_tex57=tex57, a_roughness=rough, a_metallic=metallic, a_face_idx=face_idx.astype(np.int32), a_uvw=uvw)
    for tag, tex in (("8", tex8), ("57", tex57)):
        albedo = torch.from_numpy(tex.astype(np.float32) / np.float32(255))
        m = S2.PBRMesh(torch.from_numpy(verts), torch.from_numpy(faces).long(), uvs_2d=torch.from_numpy(uvs_2d), faces_2d=torch.from_numpy(faces).long(),
                       albedo=albedo, metallic=torch.from_numpy(metallic), roughness=torch.from_numpy(rough), bump=None)
        o = m(torch.from_numpy(face_idx), torch.from_numpy(uvw))
        assert o["albedo"].shape == (64, 3) and o["metallic"].shape == (64, 1) and o["roughness"].shape == (64, 1) and o["bump"].shape == (64, 3)
        for k, val in o.items():
            fix["a_out%s_%s" % (tag, k)] = np.ascontiguousarray(val.numpy(), dtype=np.float32)
    grid = (uvs_2d[faces[face_idx]] * uvw[:, :, None]).sum(1)
    assert (np.abs(grid) > 1).any() and (grid < -1).any() and (grid > 1).any(), "no grid coordinate outside [-1, 1]: reflection is not exercised"
    print("G22(a): grid coordinates in [%.3f, %.3f], %d of 64 outside [-1, 1]" % (grid.min(), grid.max(), int((np.abs(grid) > 1).any(1).sum())))

    # ---- (b) sample_near_surface
    v, f = CR.icosphere(1)
    n_surf = int(N_NEAR * N_RADIO)
    base, bface, buvw = SR.sample_surface_ref(v, f, SR.face_weights_cum(v, f), n_surf, SEED)
    r = SR.uniforms(N_NEAR, SEED, 2)
    handed, named = [], []

    class cuBVH:
        def __init__(self, vertices=None, triangles=None):
            self.v, self.f = vertices.numpy(), triangles.numpy()

        def unsigned_distance(self, samples, return_uvw=False):
            handed.append(samples.numpy().copy())
            d64, face, alone = CR.brute_f64_face(samples.numpy(), self.v, self.f, 1024 * CR.U * CR.scene_scale(samples.numpy(), self.v))
            named.append((face, alone))
            fv = self.v.astype(np.float64)[self.f[face]]
            w = np.stack([np.linalg.norm(samples.numpy() - fv[:, k], axis=1) for k in range(3)], -1)          # placeholder weights (the distances to the corners):
            return torch.from_numpy(d64), torch.from_numpy(face.astype(np.int64)), torch.from_numpy(w.astype(np.float32))      # the fixture stores faces only
    sys.modules["cubvh"] = types.SimpleNamespace(cuBVH=cuBVH)
    sp = importlib.import_module("TextureTools.texturetools.geometry.sampling.spatial_sampling")
    sp.cuBVH = cuBVH
    orig = (torch.Generator, torch.rand, sp.sample_surface)

    class _Gen:
        def __init__(self, device=None):
            pass

        def manual_seed(self, s):
            assert s == SEED
            return self

    def rand(shape, dtype=None, device=None, generator=None):
        assert tuple(shape) == (N_NEAR, 3) and dtype == torch.float32 and str(device) == "cuda"
        return torch.from_numpy(r.copy())

    def sample_surface(vertices, faces, areas, N, seed):
        assert N == n_surf and seed == SEED
        return torch.from_numpy(base), torch.from_numpy(bface.astype(np.int64)), torch.from_numpy(buvw)
    torch.Generator, torch.rand, sp.sample_surface = _Gen, rand, sample_surface
    try:
        samples, face_index, face_uvw = sp.sample_near_surface(torch.from_numpy(v), torch.from_numpy(f).long(), N=N_NEAR, N_radio=N_RADIO, seed=SEED,
                                                              distance_threhold=THRESHOLD, depth=DEPTH)
    finally:
        torch.Generator, torch.rand, sp.sample_surface = orig
    assert len(handed) == 1 and np.array_equal(handed[0], samples.numpy()) and samples.shape == (N_NEAR, 3)
    # the vertex normals, by the reference's own lines (spatial_sampling.py:68-76) on the same tensors
    vt, ft = torch.from_numpy(v), torch.from_numpy(f).long()
    areas = torch.linalg.cross(vt[ft[:, 1], :] - vt[ft[:, 0], :], vt[ft[:, 2], :] - vt[ft[:, 0], :], dim=-1)
    normals = torch.nn.functional.normalize(areas, dim=-1)
    vn = torch.zeros((vt.shape[0], 3, 3), dtype=vt.dtype)
    vn.scatter_add_(0, ft.unsqueeze(-1).expand(ft.shape[0], 3, 3), normals.unsqueeze(1).expand(ft.shape[0], 3, 3))
    vn = torch.nn.functional.normalize(vn.sum(dim=1), dim=-1)
    fix.update(b_verts=v, b_faces=f, b_uniforms=r, b_base=base, b_base_face=bface.astype(np.int32), b_base_uvw=buvw, b_vertex_normals=vn.numpy(),
               b_samples=samples.numpy(), b_face=face_index.numpy().astype(np.int32), b_face_alone=named[0][1],
               b_params=np.array([N_NEAR, SEED, DEPTH, n_surf], np.int64), b_threshold=np.array([THRESHOLD * (2.0 / 2 ** DEPTH)], np.float64))
    assert np.array_equal(named[0][0], face_index.numpy()) and 0.5 < named[0][1].mean() < 1.0, named[0][1].mean()
    print("G22(b): %d of %d samples have one nearest face alone; the others lie outside a convex edge or vertex, where its faces tie" % (named[0][1].sum(), N_NEAR))
    moved = np.linalg.norm(samples.numpy() - base[:N_NEAR], axis=1)
    assert moved.max() > 0 and moved.max() <= THRESHOLD * (2.0 / 2 ** DEPTH) * np.sqrt(3) * 1.001
    path = os.path.join(out, "g22_spatial_sampling.npz")
    np.savez_compressed(path, **fix)
    print("G22: %d arrays, %d bytes" % (len(fix), os.path.getsize(path)))


def main(out=HERE):
    sys.path.insert(0, REF)
    install_stubs()
    torch.set_num_threads(4)
    g22(out)
    print("wrote g22_spatial_sampling")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE)

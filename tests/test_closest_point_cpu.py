"""CPU pins of oracle/closest_point_ref.py, before the GPU tests lean on it: the float32 restatement of tri_closest against the float64 brute force (another
formula) within the bound its docstring counts, the properties the C ABI promises (weights, ties), and the Philox words of streams 1 and 2 against a
pure-Python Philox4x32-10."""
import numpy as np
import pytest

from oracle import closest_point_ref as R, sampling_ref as S

F32 = np.float32


@pytest.mark.parametrize("name", R.MESHES)
def test_restatement_is_within_the_counted_bound_of_the_float64_brute_force(name):
    v, f = R.mesh(name)
    pts = R.queries(name, 257)
    dist, d2, face, uvw, q = R.closest_point_f32(pts, v, f)
    d64 = R.brute_f64(pts, v, f)
    fin = np.isfinite(pts).all(1)
    assert (face[~fin] == -1).all() and np.isinf(dist[~fin]).all() and (uvw[~fin] == 0).all() and (q[~fin] == 0).all()
    assert (face[fin] >= 0).all()
    tol = R.BOUND_U * R.U * R.scene_scale(pts, v)
    p64, v64 = pts[fin].astype(np.float64), v.astype(np.float64)
    err = np.abs(dist[fin].astype(np.float64) - d64[fin])
    err_face = np.abs(R.face_dist_f64(pts[fin], v, f, face[fin]) - d64[fin])
    fv = v64[f[face[fin]]]
    err_q = np.abs(np.linalg.norm(p64 - (uvw[fin].astype(np.float64)[:, :, None] * fv).sum(1), axis=1) - d64[fin])
    print("%s: largest multiples of u * scale: dist %.2f, returned face %.2f, sum uvw v %.2f (bound %g)" % (name, err.max() / tol * R.BOUND_U,
          err_face.max() / tol * R.BOUND_U, err_q.max() / tol * R.BOUND_U, R.BOUND_U))
    assert err.max() <= tol and err_face.max() <= tol and err_q.max() <= tol
    assert (uvw >= 0).all() and np.abs(uvw[fin].astype(np.float64).sum(1) - 1.0).max() <= 4 * R.U


def test_exact_ties_go_to_the_smallest_face_id():
    """on the dyadic grid every operation of tri_closest is exact: a vertex is at distance 0 from every face around it, an edge midpoint from both faces of the edge"""
    v, f = R.mesh("grid")
    e = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    pts = np.concatenate([v, (v[e[:, 0]] + v[e[:, 1]]) * F32(0.5), v + F32([0, 0, 0.375])])
    dist, d2, face, uvw, q = R.closest_point_f32(pts, v, f)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    all_d2 = R.tri_closest_f32(pts[:, None, :], a[None], b[None], c[None])[0]
    assert (d2 == all_d2.min(1)).all()
    ties = (all_d2 == all_d2.min(1, keepdims=True)).sum(1)
    assert ties.max() == 6 and (ties[:25] >= 1).all()
    assert (face == np.argmax(all_d2 == all_d2.min(1, keepdims=True), axis=1)).all()
    assert (d2[:len(v)] == 0).all() and (q[:len(v)] == v).all()
    assert (dist[-25:] == F32(0.375)).all()


def test_degenerate_faces_are_finite_and_right():
    """a face with a repeated corner is its edge; a face of three equal corners is a point; three collinear corners are the longest segment"""
    p = np.array([[0.25, 1.0, 0.0], [3.0, 0.0, 0.0], [-1.0, -1.0, 0.0], [0.5, 0.0, 0.5]], F32)
    for a, b, c in (([0, 0, 0], [1, 0, 0], [1, 0, 0]), ([0, 0, 0], [0, 0, 0], [1, 0, 0]), ([0, 0, 0], [1, 0, 0], [0.5, 0, 0]), ([1, 0, 0], [0, 0, 0], [0.5, 0, 0]),
                    ([0.5, 0, 0], [0.5, 0, 0], [0.5, 0, 0]), ([0.5, 0, 0], [0, 0, 0], [1, 0, 0])):
        a, b, c = (np.array(x, F32) for x in (a, b, c))
        d2, u, v, w = R.tri_closest_f32(p, a, b, c)
        assert np.isfinite(d2).all() and (u >= 0).all() and (v >= 0).all() and (w >= 0).all()
        want = R.tri_dist_f64(p, a, b, c)
        assert np.abs(np.sqrt(d2.astype(np.float64)) - want).max() <= 16 * R.U * 4, (a, b, c)


def _philox_py(ctr, key):
    M0, M1, W0, W1, m = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xffffffff
    c, k = list(ctr), list(key)
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & m, (p0 >> 32) ^ c[3] ^ k[1], p0 & m]
        k = [(k[0] + W0) & m, (k[1] + W1) & m]
    return c


def test_philox_known_answers_and_the_words_of_streams_1_and_2():
    assert _philox_py([0, 0, 0, 0], [0, 0]) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]          # Random123's kat_vectors
    assert _philox_py([0xffffffff] * 4, [0xffffffff] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    for seed in (666, 0x123456789abcdef0):
        for sid in (1, 2):
            u = S.uniforms(300, seed, sid)
            for i in (0, 1, 63, 64, 255, 256, 299):
                w = _philox_py([i, sid, 0, 0], [seed & 0xffffffff, seed >> 32])
                assert [float(x) for x in u[i]] == [(x >> 8) * 2.0 ** -24 for x in w[:3]]
            assert (u >= 0).all() and (u < 1).all()
    assert not (S.uniforms(64, 666, 1) == S.uniforms(64, 666, 2)).all()

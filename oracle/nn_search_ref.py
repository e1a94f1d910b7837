"""Checkers and constructed inputs for the two uniform-grid nearest-neighbour searches (csrc/knn.hip utx_knn, csrc/texture_post.hip utx_nn_fill).
numpy only; test infrastructure, never shipped compute.

The float32 contract stays geom_ref.knn_brute: d2 = (dx*dx + dy*dy) + dz*dz in float32, ascending, ties to the lower source index.  This module adds
  * brute64 / check64: a float64 neighbour check that does not use the float32 expression,
  * ring_search: a restatement of the kernels' ring walk (cell rule, clamp, ring order, stop test) in which planted mistakes can be switched on,
  * margin_worst_case: how much narrower than r cells the float32 cell rule lets the gap between a cell and ring r + 1 become,
  * mvpaint64 / mvpaint_bound: the MVPaint weighting in float64 over a given neighbour list, with a counted error bound,
  * the input families A-H shared by tests/test_nn_search_ref_cpu.py and tests/test_nn_search_edges_gpu.py: constructed, nothing drawn at random.
"""
import numpy as np

from . import geom_ref as G

F = np.float32
U = 2.0 ** -24                       # unit roundoff of float32
FMAX = np.finfo(np.float32).max
MARGIN = F(0.99999)                  # the kernels' stop factor
GRIDS = (64, 128, 256)               # KNN_G is 128; nn_grid() returns one of the three
# roundings of d2 = (dx*dx + dy*dy) + dz*dz relative to the exact squared distance of the float32 inputs, per term: the subtraction (1, and the term
# squares it: 2), the product (1), the first addition (1), the second addition (1) = 5 for the x and y terms, 4 for the z term.
C_D2 = 5
UNDERFLOW = 4 * 2.0 ** -149
MISTAKES = frozenset(["stop_r_plus_1", "stop_have_1", "tie_high", "le_insert", "no_clamp", "xrow_first_cell", "skip_far_face", "ring_half"])


def _p3(a):
    return np.ascontiguousarray(np.asarray(a, F).reshape(-1, 3))


def d2_f32(s, q):
    """the kernels' float32 expression, one rounding per numpy operation (no fused multiply-add)"""
    dx, dy, dz = s[..., 0] - q[..., 0], s[..., 1] - q[..., 1], s[..., 2] - q[..., 2]
    return (dx * dx + dy * dy) + dz * dz


def cell_f32(v, grid, clamp=True):
    """knn_cell1 / nn_cell1: floor((v + 1) * (G / 2)) in float32, clamped into [0, G - 1]"""
    c = np.floor((np.asarray(v, F) + F(1.0)) * F(grid * 0.5)).astype(np.int64)
    return np.clip(c, 0, grid - 1) if clamp else c


# ---- float64 check ---------------------------------------------------------------------------------------------------------------------------------
def brute64(src, dst, k, src_mask=None):
    """k nearest sources by the float64 squared distance of the float32 inputs, sorted by (d2, index).  idx [M,k] (-1 padded), d2 [M,k] (inf padded)."""
    s, q = _p3(src).astype(np.float64), _p3(dst).astype(np.float64)
    ids = np.arange(len(s)) if src_mask is None else np.flatnonzero(np.asarray(src_mask).reshape(-1))
    M, kk = len(q), min(k, len(ids))
    idx = np.full((M, k), -1, np.int64); d2o = np.full((M, k), np.inf)
    for a in range(0, M, 512):
        d = ((s[ids][None] - q[a:a + 512, None]) ** 2).sum(-1)
        o = np.lexsort((np.broadcast_to(ids[None], d.shape), d), axis=1)[:, :kk]
        idx[a:a + 512, :kk] = ids[o]; d2o[a:a + 512, :kk] = np.take_along_axis(d, o, 1)
    return idx, d2o


def check64(src, dst, idx, k, src_mask=None):
    """The neighbour list `idx` [M,k] against float64, independent of the float32 expression: every row holds min(k, n_src) distinct valid sources,
    then -1, and its j-th neighbour has float64 d2 <= (true j-th smallest float64 d2) * (1 + c u) / (1 - c u) + UNDERFLOW, c = C_D2 = 5 (the float32 d2
    of any source is within (1 +- c u) of its float64 d2, and the list is sorted by the float32 d2).  UNDERFLOW = 4 * 2^-149: the relative count holds
    for normal numbers only; a product dx*dx below 2^-126 is rounded to a multiple of 2^-149 (gradual underflow: absolute error <= 2^-150 each, three
    products on either side of the comparison, sums of subnormals are exact).  Family A's coordinates one subnormal step from 0.0 reach it: their
    squares are 0 in float32.  Returns None, or a string that says what is wrong."""
    s, q = _p3(src).astype(np.float64), _p3(dst).astype(np.float64)
    idx = np.asarray(idx).reshape(len(q), k).astype(np.int64)
    valid = np.ones(len(s), bool) if src_mask is None else np.asarray(src_mask).reshape(-1).astype(bool)
    kk = min(k, int(valid.sum()))
    if (idx[:, kk:] != -1).any() or (idx[:, :kk] < 0).any() or (idx[:, :kk] >= len(s)).any():
        return "a row does not hold min(k, n_src) = %d sources followed by -1" % kk
    if kk == 0:
        return None
    if not valid[idx[:, :kk]].all():
        return "a masked-out source was returned"
    if kk > 1 and (np.diff(np.sort(idx[:, :kk], 1), axis=1) == 0).any():
        return "a source appears twice in one row"
    got = ((s[idx[:, :kk]] - q[:, None]) ** 2).sum(-1)
    true = brute64(src, dst, k, src_mask)[1][:, :kk]
    lim = true * ((1 + C_D2 * U) / (1 - C_D2 * U)) + UNDERFLOW
    bad = np.argwhere(got > lim)
    if len(bad):
        t, j = bad[0]
        return "query %d neighbour %d: float64 d2 %.17g above the bound %.17g (true %.17g)" % (t, j, got[t, j], lim[t, j], true[t, j])
    return None


# ---- the ring search, restated ---------------------------------------------------------------------------------------------------------------------
def _insert(bd, bi, kk, d2, j, le, hi):
    """the kernels' sorted insertion; le: `<=` for `<` (planted), hi: ties to the higher index (planted)"""
    def before(d, jj, b, bj):
        if le:
            return d <= b
        return d < b or (d == b and (jj > bj if hi else jj < bj))
    have = len(bd)
    if have == kk and not before(d2, j, bd[-1], bi[-1]):
        return
    if have < kk:
        bd.append(d2); bi.append(j)
    q = len(bd) - 1
    while q > 0 and before(d2, j, bd[q - 1], bi[q - 1]):
        bd[q], bi[q] = bd[q - 1], bi[q - 1]; q -= 1
    bd[q], bi[q] = d2, j


def ring_search(src, dst, k, src_mask=None, grid=128, margin=MARGIN, cell=cell_f32, mistakes=()):
    """The kernels' search: sources binned by `cell` and sorted by cell id (ascending index inside a cell, as the stable radix sort leaves them); a query
    walks the rings r = 0 .. G - 1 of its own cell, the cells of a ring in ascending (z, y, x); after ring r it stops when it holds min(k, n_src)
    neighbours and the worst has d2 < fl(fl(fl(r) * cs)^2 * margin), cs = fl(2 / G).  k = 1 is the search of utx_nn_fill (its merged x-row pass reads
    the same candidates in the same order).  mistakes: names from MISTAKES, each a way the kernels could be wrong.  Returns idx [M,k] i64, d2 [M,k] f32."""
    mistakes = frozenset(mistakes)
    assert mistakes <= MISTAKES, mistakes - MISTAKES
    s, q = _p3(src), _p3(dst)
    ids = np.arange(len(s)) if src_mask is None else np.flatnonzero(np.asarray(src_mask).reshape(-1))
    clamp = "no_clamp" not in mistakes
    le, hi = "le_insert" in mistakes, "tie_high" in mistakes
    kk = min(k, len(ids))                                   # the kernels count the valid sources, found or not
    sc = cell(s[ids], grid, clamp).reshape(-1, 3)
    ok = ((sc >= 0) & (sc < grid)).all(1)                   # a cell outside the table is never visited
    ids, sc = ids[ok], sc[ok]
    cid = (sc[:, 2] * grid + sc[:, 1]) * grid + sc[:, 0]
    o = np.lexsort((ids, cid))
    ids, sc, ps = ids[o], sc[o], s[ids[o]]
    cs = F(2.0) / F(grid)
    rmax = grid // 2 if "ring_half" in mistakes else grid
    idx = np.full((len(q), k), -1, np.int64); d2o = np.full((len(q), k), np.inf, F)
    for t in range(len(q)):
        if kk == 0:
            break
        qc = cell(q[t], grid, clamp)
        rel = sc - qc
        cheb = np.abs(rel).max(1) if len(sc) else np.zeros(0, np.int64)
        keep = np.ones(len(sc), bool)
        if "skip_far_face" in mistakes:
            keep &= ~((rel[:, 2] == cheb) & (cheb > 0))
        if "xrow_first_cell" in mistakes and len(sc):
            # nn_fill's merged x-row pass [start of the first non-empty cell, end of the LAST one): planted, it ends with the first cell
            shell = ((np.abs(rel[:, 2]) == cheb) | (np.abs(rel[:, 1]) == cheb)) & (cheb > 0)
            key = (cheb * grid + sc[:, 2]) * grid + sc[:, 1]
            u, inv = np.unique(key, return_inverse=True)
            mn = np.full(len(u), grid); np.minimum.at(mn, inv[shell], sc[shell, 0])
            keep &= ~shell | (sc[:, 0] == mn[inv])
        d2 = d2_f32(ps, q[t])
        order = np.flatnonzero(keep)
        order = order[np.argsort(cheb[order], kind="stable")]
        ring = cheb[order]
        bd, bi, pos = [], [], 0
        for r in range(rmax):
            end = pos + int(np.searchsorted(ring[pos:], r, side="right"))
            if end > pos:
                c = order[pos:end]
                if le or end - pos <= 4:
                    for i in c:
                        _insert(bd, bi, kk, d2[i], int(ids[i]), le, hi)
                else:
                    ad = np.concatenate([np.asarray(bd, F), d2[c]]); ai = np.concatenate([np.asarray(bi, np.int64), ids[c]])
                    oo = np.lexsort((-ai if hi else ai, ad))[:kk]
                    bd, bi = list(ad[oo]), [int(v) for v in ai[oo]]
                pos = end
            rr = F(r + 1 if "stop_r_plus_1" in mistakes else r) * cs
            thr = F(F(rr * rr) * F(margin))
            full = len(bd) >= 1 if "stop_have_1" in mistakes else len(bd) == kk
            if full and bd[-1] < thr:
                break
        idx[t, :len(bi)] = bi; d2o[t, :len(bd)] = bd
    return idx, d2o


# ---- the stop rule's margin ------------------------------------------------------------------------------------------------------------------------
def _f32_from_key(key):
    """float32 from a key that orders all floats like the integers (negative floats below the positive ones)"""
    key = np.int64(key)
    bits = key if key >= 0 else np.int64(-(key + 1)) | np.int64(0x80000000)
    return np.array([bits], np.uint64).astype(np.uint32).view(F)[0]


def _key_of(v):
    b = np.int64(np.array([v], F).view(np.uint32)[0])
    return b if b < 0x80000000 else -(b - 0x80000000) - 1


def cell_threshold(i, grid, cell=cell_f32):
    """the smallest float32 whose (unclamped) cell is >= i, found by bisection over the float order: the float at the rounding midpoint below the
    face b = -1 + i cs when v + 1 rounds up across it, the face itself otherwise.  Checked against its two neighbours."""
    lo, hi = _key_of(F(-4.0)), _key_of(F(4.0))
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if cell(_f32_from_key(mid), grid, False) >= i:
            hi = mid
        else:
            lo = mid
    t = _f32_from_key(hi)
    assert cell(t, grid, False) >= i > cell(_f32_from_key(hi - 1), grid, False) and cell(_f32_from_key(hi + 1), grid, False) >= i
    return t


_THR = {}


def _thresholds(grid, cell=cell_f32):
    if (grid, cell) not in _THR:
        _THR[(grid, cell)] = [cell_threshold(i, grid, cell) for i in range(grid + 1)]
    return _THR[(grid, cell)]


def margin_worst_case(grid, cell=cell_f32, detail=False, rings=None):
    """min over the cells c and over r in (1, 2, 3, G/2) of (gap / (r cs))^2, gap = the smallest true distance (float64) between a value binned into
    cell c and a value binned into a cell >= c + r + 1: that is thr(c + r + 1) - pred(thr(c + 1)), thr(i) = cell_threshold(i).  A point the walk has
    not seen after ring r differs from the query's cell by >= r + 1 on some axis, so its true squared distance is >= gap^2; clamping only moves points
    further out.  detail: (ratio, r, c)."""
    thr = [np.float64(v) for v in _thresholds(grid, cell)]
    below = [np.float64(np.nextafter(F(v), F(-np.inf))) for v in thr]
    cs = 2.0 / grid
    worst = (np.inf, None, None)
    for r in rings or (1, 2, 3, grid // 2):
        for c in range(0, grid - r - 1):
            ratio = ((thr[c + r + 1] - below[c + 1]) / (r * cs)) ** 2
            if ratio < worst[0]:
                worst = (ratio, r, c)
    return worst if detail else worst[0]


# ---- MVPaint weighting in float64 ------------------------------------------------------------------------------------------------------------------
def mvpaint64(idx, d2, attr, src_nrm, dst_nrm):
    """The reference's rule over a given neighbour list (idx [M,k], -1 padded; d2 [M,k] float32 as the search returned it):
        inv = nan_to_num(1 / d2, nan=0)       in float32, so 1/0 = inf becomes the largest finite float32
        w   = inv / max(sum |inv|, 1e-12) * cos(n_src, n_dst)        (norms clamped at 1e-8)
        out = sum(w a) / sum(w), and a non-finite result is 0.
    inv is the float32 value (one rounding, counted in the bound); everything after it is float64.  A float32 L1 sum that overflows (two or more
    coincident sources) makes every weight 0 and the row 0, as in float32.  Returns (out [M,C], bound [M,C]): the bound is
        (E_S + |out| E_W) / (|sum w| - E_W) + u |out|,   E_S = g sum |a_q| W_q,   E_W = g sum W_q,   W_q = inv_q / L1 * sum_i |n_i m_i| / (|n| |m|),
    g = (c_w + c') u.  c_w = k + 13 roundings of a weight: 1/d2 (1), the L1 sum (k - 1), the division by it (1), the dot product (3, taken absolutely
    through sum |n_i m_i| because it can cancel), each norm (3 under the square root: 1.5, the root: 1; two norms: 5), their product (1), the division (1),
    the product with the cosine (1), and 1 for second-order terms.  c' = k + 1: the product w a (1), at most k - 1 additions of the sum, and the final
    division is the u |out| term.  Where |sum w| <= E_W the row is ill-conditioned and the bound is +inf: it is inside the bound, no row is left out."""
    idx = np.asarray(idx).astype(np.int64); M, k = idx.shape
    a = np.asarray(attr, F).reshape(-1, np.asarray(attr).shape[-1]).astype(np.float64)
    have = idx >= 0
    j = np.maximum(idx, 0)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        inv = (F(1.0) / np.asarray(d2, F).reshape(M, k)).astype(F)
    inv = np.where(np.isnan(inv) | ~have, F(0), np.minimum(inv, FMAX)).astype(np.float64)
    l1 = np.abs(inv).sum(1)
    overflow = l1 >= float(FMAX) * (1 + 2.0 ** -25)
    n = np.asarray(src_nrm, F).reshape(-1, 3).astype(np.float64)[j]; m = np.asarray(dst_nrm, F).reshape(-1, 3).astype(np.float64)[:, None]
    den = np.maximum(np.sqrt((n * n).sum(-1)), 1e-8) * np.maximum(np.sqrt((m * m).sum(-1)), 1e-8)
    L = np.where(overflow[:, None], 0.0, inv / np.maximum(np.minimum(l1, float(FMAX)), 1e-12)[:, None]) * have
    w = L * (n * m).sum(-1) / den
    W = L * np.abs(n * m).sum(-1) / den
    S = (w[..., None] * a[j]).sum(1); ws = w.sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = S / ws[:, None]
    out = np.where(np.isfinite(out) & (np.abs(out) <= float(FMAX)), out, 0.0)
    g = ((k + 13) + (k + 1)) * U
    ES = g * (W[..., None] * np.abs(a[j])).sum(1); EW = g * W.sum(1)
    room = np.abs(ws) - EW
    with np.errstate(divide="ignore", invalid="ignore"):
        bound = np.where(room[:, None] > 0, (ES + np.abs(out) * EW[:, None]) / room[:, None] + U * np.abs(out) + 1e-45, np.inf)
    exact0 = (ws == 0) & (W.sum(1) == 0)                  # every weight exactly 0 (zero-length normals, overflowed L1): 0/0 -> 0, nothing to round
    bound[exact0] = 0.0
    return out, bound


# ---- brute force at the queries only ---------------------------------------------------------------------------------------------------------------
def nn_fill_index(pos, winner, rast2d):
    """utx_nn_fill's nn_index by brute force at the queries only (geom_ref.nn_fill_brute is O(T^2)): float32 d2, ties to the lowest texel index."""
    p = _p3(pos); w = np.asarray(winner).reshape(-1); rw = np.asarray(rast2d, F).reshape(-1, 4)[:, 3]
    src = np.flatnonzero(w >= 0); dst = np.flatnonzero((w < 0) & (rw > 0))
    idx = np.full(len(p), -1, np.int32)
    if len(src) and len(dst):
        ps = p[src]
        for a in range(0, len(dst), 16):
            d = d2_f32(ps[None], p[dst[a:a + 16], None])
            idx[dst[a:a + 16]] = src[np.argmin(d, axis=1)]       # argmin keeps the first of equal minima = the lowest index
    return idx


def as_atlas(src, dst, C=3, width=16, pad=3):
    """a source / query set as an atlas for utx_nn_fill: sources are seen texels (winner 0), queries covered unseen ones (winner -1, rast.w 1), texel
    index = source index, then `pad` uncovered texels (winner -1, rast.w 0; must stay -1), then the queries.  The atlas holds distinct exact values."""
    s, q = _p3(src), _p3(dst)
    n = len(s) + pad + len(q)
    H = (n + width - 1) // width; T = H * width
    pos = np.zeros((T, 3), F); win = np.full(T, -1, np.int8); rast = np.zeros((T, 4), F)
    pos[:len(s)] = s; win[:len(s)] = 0; rast[:len(s), 3] = 1
    a = len(s) + pad
    pos[a:a + len(q)] = q; rast[a:a + len(q), 3] = 1
    rast[len(s):a, 3] = [0.0, -1.0, -0.0][:pad] if pad <= 3 else 0.0
    atlas = (np.arange(T * C, dtype=np.int64).reshape(T, C) % 8191).astype(F) * F(0.125)
    return dict(pos=pos.reshape(H, width, 3), winner=win.reshape(H, width), rast2d=rast.reshape(H, width, 4), atlas=atlas.reshape(H, width, C),
                queries=np.arange(a, a + len(q)))


# ---- the input families ----------------------------------------------------------------------------------------------------------------------------
def _case(name, src, dst, **kw):
    return dict(name=name, src=_p3(src), dst=_p3(dst), **kw)


def face_values(grid):
    """family A's coordinates: the faces i in {0, 1, G/4, G/2 - 1, G/2, G/2 + 1, G - 1, G}, their float neighbours, b +- 2^-25, +-0.0 and +-1"""
    cs = 2.0 / grid
    v = [F(-0.0), F(0.0), F(-1.0), F(1.0)]
    for i in (0, 1, grid // 4, grid // 2 - 1, grid // 2, grid // 2 + 1, grid - 1, grid):
        b = F(-1.0 + i * cs)
        v += [b, np.nextafter(b, F(np.inf)), np.nextafter(b, F(-np.inf)), F(np.float64(b) + 2.0 ** -25), F(np.float64(b) - 2.0 ** -25)]
    v = np.array(v, F)
    return v[np.unique(v.view(np.uint32), return_index=True)[1]]            # by bit pattern: -0.0 and +0.0 both stay


def family_a(grid):
    """cell faces: every value of face_values on each axis (the other two at fixed off-face values) and on all three at once, as sources and as
    queries; a second query set is moved one cell on the other axes so that the neighbours straddle the faces"""
    v = face_values(grid); cs = F(2.0 / grid)
    pts = []
    for ax in range(3):
        p = np.empty((len(v), 3), F); p[:] = [F(0.3), F(-0.2), F(0.1)]; p[:, ax] = v
        pts.append(p)
    pts.append(np.stack([v, v, v], 1)); pts.append(np.stack([v, v[::-1], v], 1))
    src = np.concatenate(pts)
    dst = np.concatenate([src, src + np.array([cs, -cs, cs], F) * F(0.75)])
    return [_case("A/G%d" % grid, src, dst)]


def ring_stop_points(grid, r):
    """family B's x coordinates for one grid and ring: (q, xa, xb, D2), at the cell c where margin_worst_case finds ring r's narrowest gap.  The query is
    the largest float binned into cell c; B is the smallest float binned into cell c + r + 1, in ring r + 1: a float where the computed cell is one
    above the true cell (v + 1 rounds up across the face), so B is nearer than r cells.  A lies in cell c + r, the outermost cell of ring r on B's
    side, with dx^2 just under (r cs)^2 (1 - 2e-5)."""
    _, _, c = margin_worst_case(grid, detail=True, rings=(r,))
    thr = _thresholds(grid)
    q = np.nextafter(thr[c + 1], F(-np.inf))
    xb = thr[c + r + 1]
    D = r * 2.0 / grid
    xa = F(np.float64(q) + D * np.sqrt(1 - 2.2e-5))
    assert cell_f32(xa, grid) == c + r and cell_f32(xb, grid) == c + r + 1 and cell_f32(q, grid) == c
    assert np.float64(xb) - np.float64(q) < D, "B is in ring r + 1 and nearer than r cells"
    return q, xa, xb, D * D


def _tune(x, q, y0, target):
    """a float32 y near y0 with fl(fl(fl(x - q)^2 + fl(y - y0)^2) + 0) as close to `target` as the float32 grid of y allows; returns (y, d2)"""
    dx = F(x - q); base = F(dx * dx)
    if target <= base:
        return y0, base
    best = None
    y = F(np.float64(y0) + np.sqrt(np.float64(target) - np.float64(base)))
    for _ in range(3):
        y = np.nextafter(y, F(-np.inf))
    for _ in range(7):
        dy = F(y - y0); d2 = F(base + F(dy * dy))
        if best is None or abs(np.float64(d2) - np.float64(target)) < abs(np.float64(best[1]) - np.float64(target)):
            best = (y, d2)
        y = np.nextafter(y, F(np.inf))
    return best


def family_b(grid, r, k=1, steps=None, dense=None, max_rows=None):
    """ring stop: one scenario per float32 d2 of candidate A in [(r cs)^2 (1 - 2e-5), (r cs)^2 (1 + 2e-5)], float by float (`steps` keeps every
    steps-th; the cases record how many targets there are and how many distinct d2 the construction reached), twice: B with a lower and with a higher
    index than A.  B is in ring r + 1 with the largest d2 below A's that its coordinates allow, or at its nearest where it cannot be nearer than A.
    k > 1 adds k - 1 fillers next to the query.  Each scenario has its own (y, z) row.  Isolated rows are r + 3 cells apart: no scenario sees
    another's points before its own A and B, whatever k; at r = G/2 only 2 x 2 rows fit into the cube.  Dense rows (the default at r = G/2, k = 1)
    are 5 cells apart, which keeps a row's own A and B its two nearest candidates of their kind but not its fillers.  One case per launch, of at most max_rows scenarios."""
    dense = (r > 3 and k == 1) if dense is None else dense
    assert not (dense and k > 1), "fillers need isolated rows"
    q, xa, xb, D2 = ring_stop_points(grid, r)
    lo, hi = F(D2 * (1 - 2e-5)), F(D2 * (1 + 2e-5))
    targets = []
    t = lo
    while t <= hi:
        targets.append(t); t = np.nextafter(t, F(np.inf))
    targets = targets[::steps] if steps else targets
    cs = 2.0 / grid
    pitch = 5 if dense else r + 3
    per_axis = (grid - 3) // pitch + 1                      # rows at cell 1.5 + pitch * a, the last at most at G - 1.5
    rows = [(F(-1 + (1.5 + pitch * a) * cs), F(-1 + (1.5 + pitch * b) * cs)) for a in range(per_axis) for b in range(per_axis)]
    rows = rows[:max_rows] if max_rows else rows
    scen = []
    seen = set()
    for tg in targets:
        for b_low in (True, False):
            scen.append((tg, b_low))
    cases = []
    for c0 in range(0, len(scen), len(rows)):
        src, dst = [], []
        for (tg, b_low), (y0, z0) in zip(scen[c0:c0 + len(rows)], rows):
            ya, d2a = _tune(xa, q, y0, tg)
            yb, d2b = _tune(xb, q, y0, np.nextafter(d2a, F(-np.inf)))
            seen.add(float(d2a))
            A, B = [xa, ya, z0], [xb, yb, z0]
            fill = [[F(np.float64(q) - (i + 1) * cs * 2.0 ** -6), y0, z0] for i in range(k - 1)]
            src += ([B, A] if b_low else [A, B]) + fill
            dst.append([q, y0, z0])
        cases.append(_case("B/G%d/r%d/k%d/%d" % (grid, r, k, len(cases)), src, dst, distinct_d2=len(seen), targets=len(targets)))
    return cases


def lattice_ties(grid=128):
    """family C: on a 2^-6 lattice, exact ties of 6 (axis), 8 (corner), 12 (edge) sources, and 6 + 24 sources at 5 and (3, 4, 0) lattice steps: the
    same d2 = 25 * 2^-12 from rings 4 and 5 of a 128 grid.  Indices run against the cell order, so the lowest index of a tie is in the cell the walk
    reads last.  Queries: the lattice centre (ties), centre + one step (a source: d2 = 0), and a centre moved off the lattice."""
    h = 2.0 ** -6
    ctr = np.array([5, -9, 3]) * h
    off = set()
    for ax in range(3):
        for sg in (-1, 1):
            e = [0, 0, 0]; e[ax] = sg; off.add(tuple(e)); e5 = [0, 0, 0]; e5[ax] = 5 * sg; off.add(tuple(e5))
    for sx in (-1, 1):
        for sy in (-1, 1):
            for sz in (-1, 1):
                off.add((2 * sx, 2 * sy, 2 * sz))
            for ax in range(3):
                e = [3 * sx, 3 * sy]; e.insert(ax, 0); off.add(tuple(e))
                for a, b in ((3, 4), (4, 3)):
                    e = [a * sx, b * sy]; e.insert(ax, 0); off.add(tuple(e))
    src = (ctr + np.array(sorted(off)) * h).astype(F)
    cell = cell_f32(src, grid)
    order = np.lexsort((cell[:, 0], cell[:, 1], cell[:, 2]))[::-1]           # index 0 = the last cell of the walk
    src = src[order]
    dst = np.array([ctr, ctr + [h, 0, 0], ctr + [0, 0, 5 * h], ctr + [h / 4, -h / 8, h / 2], ctr + [0, 3 * h, 4 * h]], F)
    return [_case("C/ties/G%d" % grid, src, dst)]


def duplicates():
    """family C: 40 identical copies of one point (more than k = 32) between two other points; queries on the copies, beside them, and some twenty cells away"""
    p = np.array([0.25, -0.5, 0.125], F)
    src = np.concatenate([[p + F(2.0 ** -9)], np.tile(p, (40, 1)), [p - F(2.0 ** -9)]]).astype(F)
    dst = np.array([p, p + F(2.0 ** -10), [0.15, -0.4, 0.05]], F)
    return [_case("C/dups", src, dst)]


def k_edges(k):
    """family D: n_src in {0, 1, k - 1, k, k + 1}, once by src_mask over 40 points and once with N itself that small (N = 0 is not a launch)"""
    h = 2.0 ** -5
    pts = np.array([[(i % 4) * h - 0.4, ((i // 4) % 4) * h * 1.5 + 0.1, (i // 16) * h * 0.75 - 0.2] for i in range(40)], F)
    dst = np.array([[-0.37, 0.13, -0.18], [-0.1, 0.4, 0.1], pts[7], [-0.2, 0.0, 0.0]], F)
    out = []
    for n in sorted(set([0, 1, k - 1, k, k + 1])):
        m = np.zeros(40, bool); m[(np.arange(n) * 7) % 40] = True            # 7 is coprime to 40: n distinct points, out of index order
        out.append(_case("D/k%d/mask%d" % (k, n), pts, dst, src_mask=m))
        if n >= 1:
            out.append(_case("D/k%d/N%d" % (k, n), pts[np.flatnonzero(m)], dst))
    return out


def one_cell(grid=128, n=5000, far=8):
    """family D: n sources inside one cell (a 2^-12 sub-lattice of the cell at the cube's low corner); queries in the cell, in the next cell and, `far`
    of them (each walks all G^3 cells: ring G - 1), at the opposite corner"""
    h = 2.0 ** -12
    i = np.arange(n)
    src = np.stack([-1 + (1 + i % 20) * h, -1 + (1 + (i // 20) % 20) * h, -1 + (1 + i // 400) * h], 1).astype(F)
    assert (cell_f32(src, 256) == 0).all()
    cs = 2.0 / grid
    near = np.array([[-1 + 3.5 * h, -1 + 7.25 * h, -1 + 2 * h], [-1 + 1.5 * cs, -1 + 0.5 * cs, -1 + 0.25 * cs]], F)
    fq = np.array([[1 - (1 + j) * h, 1 - (1 + j % 3) * h, 1 - (1 + j % 2) * h] for j in range(far)], F)
    return [_case("D/onecell/G%d" % grid, src, np.concatenate([near, fq]))]


def outside(which):
    """family E: |v| up to 8 mixed with inside points; which in ('src', 'dst', 'both')"""
    h = 0.0625
    base = np.array([[((i * 5) % 17 - 8) * h, ((i * 3) % 13 - 6) * h * 1.25, ((i * 7) % 11 - 5) * h * 1.5] for i in range(120)], F)
    far = np.array([[8, 0.1, -0.2], [-8, 8, 0.3], [1.5, -1.25, 7.75], [-1.0000001, 1.0000001, 0], [3, 3, 3], [-2.5, 0.5, 0.5], [1.001, -0.999, 0.999],
                    [0.2, 6.5, -0.1], [-7, -7, -7], [1, 1, 1], [-1, -1, -1], [2, -1, 0.5]], F)
    ins = base * F(0.9) + F(0.013)
    src = np.concatenate([base, far]) if which in ("src", "both") else base
    dst = np.concatenate([ins, far * F(0.97), far]) if which in ("dst", "both") else ins
    return [_case("E/" + which, src, dst)]


def launch_geometry():
    """family F: M in {1, 127, 128, 129} x N in {1, 255, 256, 257} on a constructed lattice (point 0 at the centre: with N = 1 no query is more than 64 rings away)"""
    def lat(n, a, b, c, o):
        i = np.arange(n)
        return np.stack([((i * a + 30) % 61 - 30) / 32.0 + o, ((i * b + 26) % 53 - 26) / 28.0, ((i * c + 23) % 47 - 23) / 25.0 - o], 1).astype(F)
    return [_case("F/M%d/N%d" % (M, N), lat(N, 7, 11, 13, 0.0), lat(M, 5, 3, 17, 2.0 ** -7)) for M in (1, 127, 128, 129) for N in (1, 255, 256, 257)]


def xrow_gap(grid):
    """family G: sources along one x-row of cells with empty cells between them, the nearest in the LAST non-empty cell of the row pass, which is a
    shell row of the query's ring 2 (the query is two cells away in y); a lower-index decoy farther off in the first cell"""
    cs = 2.0 / grid
    cx = lambda i: -1 + (i + 0.5) * cs
    y, z = cx(grid // 2 + 2), cx(grid // 2)
    src = np.array([[cx(grid // 2 - 2), y, z], [cx(grid // 2 - 1) - 0.4 * cs, y, z], [cx(grid // 2 + 2) - 0.45 * cs, y - 0.45 * cs, z]], F)
    dst = np.array([[cx(grid // 2 + 1) + 0.3 * cs, cx(grid // 2) + 0.4 * cs, z]], F)
    return [_case("G/xrow/G%d" % grid, src, dst)]


def two_cell(grid):
    """family G: the nearest source in an interior row of ring 2 (|dy|, |dz| < 2): the walk reaches it through the two-cell branch (x = cx - r, cx + r);
    farther sources sit in shell rows of rings 1 and 2"""
    cs = 2.0 / grid
    cx = lambda i: -1 + (i + 0.5) * cs
    c = grid // 4
    dst = np.array([[cx(c) + 0.45 * cs, cx(c), cx(c)]], F)
    src = np.array([[cx(c), cx(c + 2), cx(c - 1)], [cx(c + 2) - 0.45 * cs, cx(c) + 0.1 * cs, cx(c + 1) - 0.4 * cs], [cx(c - 2), cx(c + 1), cx(c)],
                    [cx(c + 1), cx(c - 2), cx(c + 2)]], F)
    return [_case("G/twocell/G%d" % grid, src, dst)]


def big_atlas(H, W, C=3):
    """family G: an H x W atlas on a curved sheet, everything seen except <= 500 covered unseen texels: a 15 x 15 hole (its middle is several cells from
    the nearest seen texel) and every 997th texel; 7 uncovered unseen texels (rast.w <= 0) that must stay -1"""
    i, j = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    x = ((2 * j + 1) / W - 1).astype(F) * F(0.98); y = ((2 * i + 1) / H - 1).astype(F) * F(0.98)
    pos = np.stack([x, y, (x * y * F(0.5) + x * x * F(0.25) - F(0.1)).astype(F)], -1).astype(F)
    win = np.zeros((H, W), np.int8); rast = np.zeros((H, W, 4), F); rast[..., 3] = 1
    win[H // 3:H // 3 + 15, W // 2:W // 2 + 15] = -1
    flat = win.reshape(-1); flat[5::997] = -1
    rw = rast.reshape(-1, 4); unc = np.arange(11, H * W, (H * W) // 7)[:7]; flat[unc] = -1; rw[unc, 3] = [0, -1, 0, -0.0, 0, -2, 0]
    assert ((flat < 0) & (rw[:, 3] > 0)).sum() <= 500
    T = H * W
    atlas = ((np.arange(T, dtype=np.int64)[:, None] * 3 + np.arange(C)) % 65521).astype(F) * F(0.25)
    return dict(pos=pos, winner=win, rast2d=rast, atlas=atlas.reshape(H, W, C))


def normals(kind, n_src, n_dst):
    """family H's normals: 'parallel', 'opposed' (alternating +-: weights cancel), 'zero' (zero-length), 'mixed'"""
    e = np.array([0.0, 0.6, 0.8], F)
    i = np.arange(n_src)
    if kind == "parallel":
        sn = np.tile(e * F(2), (n_src, 1))
    elif kind == "opposed":
        sn = np.where((i % 2 == 0)[:, None], e, -e)
    elif kind == "zero":
        sn = np.where((i % 3 == 0)[:, None], np.zeros(3, F), e)
    else:
        sn = np.stack([((i * 3) % 7 - 3) / 4.0, ((i * 5) % 11 - 5) / 6.0, ((i * 2) % 5 - 2) / 3.0 + 0.05], 1)
    dn = np.tile(e, (n_dst, 1))
    if kind == "zero":
        dn[::2] = 0
    return np.asarray(sn, F), np.asarray(dn, F)


def knn_cases(k):
    """every family's cases for utx_knn (KNN_G = 128) at one k, except B (family_b) and the 5000-source cell (one_cell)"""
    out = []
    for g in GRIDS:
        out += family_a(g)
    out += lattice_ties(128) + duplicates() + k_edges(k)
    for w in ("src", "dst", "both"):
        out += outside(w)
    return out

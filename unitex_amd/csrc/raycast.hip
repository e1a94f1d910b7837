// Ray queries on the LBVH (gfx950): what RayTracing.intersects_closest of the reference promises (raytracing/__init__.py: hit, front, tri_idx, loc, uv) and
// what raytracing/check_visibility.py builds from it (self_rt, cross_rt, sphere_rt).  Four kernels on the utx_bvh handle, each ONE launch with no workspace,
// no host wait and no atomics but the optional visited-nodes counter:
//   raycast_intersect_kernel   closest hit of arbitrary rays: the close_* family of bvh_device.h (utx_visible_faces_rays' walk, unchanged), then the winner
//                              evaluated once more with the same arithmetic for t, u, v
//   raycast_occluded_kernel    any hit with 0 <= t < 1 along d = to - from; leaves at the first one, boxes pruned at limit 1
//   points_enclosed_kernel     the fused self_rt: a group of lanes per point, each lane walks its share of the point's rays (any hit, t >= 0), the group
//                              leaves at the first completed miss
//   sphere_directions_kernel   the direction stream of points_enclosed, written out
// Depth rule of utx_visible_faces_rays: the packed (stackless) walk up to UTX_BVH_PACKED_MAX_DEPTH, the stack walk beyond it or when forced; a tree too deep
// for CLOSE_STACK is refused.  Compiled with -ffp-contract=off and without packed fp32: t, u, v, loc, front and the directions are restated bit for bit in
// numpy (tests/support/raycast_ref.py).
//
// Why every walk ends, whatever the ray holds (a zero direction, NaN, infinities): the ray's numbers only decide whether a subtree is ENTERED.  The packed walk
// moves along link (into a subtree) or esc (past it), which enumerate the nodes in preorder -- no node twice, at most 2F - 1 steps; the stack walk pushes the
// two children of a node it popped, each node at most once.  A NaN makes close_box accept every box (fminf / fmaxf drop it) and close_tri refuse every
// triangle (each of its comparisons is false), so such a ray visits the whole tree once and misses; d = (0, 0, 0) gives P = 0, det = 0: a miss as well.
#include "common.h"
#include "kernels.h"
#include "bvh_device.h"
#include "philox_device.h"

// ---- any hit with t < tmax (t >= 0 is close_tri's): the walks of bvh_closest_packed / bvh_closest_stack with a fixed limit, left at the first hit.  close_box
// tests against [0, tmax], its far side widened, so a box that starts at tmax is still entered: the strict comparison is made on the triangle's own t.
__device__ __forceinline__ bool bvh_any_packed(const float4* __restrict__ nodes, const float4* __restrict__ tris, const CloseRay& r, float tmax, unsigned& nv) {
    int nd = 0;
    while (nd >= 0) {
        const float4 a = nodes[2 * (long)nd], b = nodes[2 * (long)nd + 1];
        const float bb[6] = {a.x, a.y, a.z, a.w, b.x, b.y};
        const int link = __float_as_int(b.z), esc = __float_as_int(b.w);
        ++nv;
        if (!close_box(r, tmax, bb)) { nd = esc; continue; }
        if (link > 0) { nd = link; continue; }
        const int prim = ~link;
        const float4 t0 = tris[3 * (long)prim], t1 = tris[3 * (long)prim + 1], t2 = tris[3 * (long)prim + 2];
        const float v0[3] = {t0.x, t0.y, t0.z}, v1[3] = {t1.x, t1.y, t1.z}, v2[3] = {t2.x, t2.y, t2.z};
        float t;
        if (close_tri(r, v0, v1, v2, t) && t < tmax) return true;
        nd = esc;
    }
    return false;
}
__device__ __forceinline__ bool bvh_any_stack(const int* __restrict__ info, const float* __restrict__ aabb, const float* __restrict__ vert,
                                              const int* __restrict__ faces, const CloseRay& r, float tmax, unsigned& nv) {
    int stack[CLOSE_STACK];
    int count = 0;
    stack[count++] = 0;
    while (count > 0) {
        const int nd = stack[--count];
        float bb[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) bb[k] = aabb[6 * (long)nd + k];
        ++nv;
        if (!close_box(r, tmax, bb)) continue;
        const int L = info[3 * (long)nd], R = info[3 * (long)nd + 1];
        if (L != 0 || R != 0) {
            if (count + 2 <= CLOSE_STACK) { stack[count++] = L; stack[count++] = R; }      // never refused: the launcher keeps depth + 2 <= CLOSE_STACK
        } else {
            const int prim = info[3 * (long)nd + 2];
            const int* f = faces + 3 * (long)prim;
            float t;
            if (close_tri(r, vert + 3 * (long)f[0], vert + 3 * (long)f[1], vert + 3 * (long)f[2], t) && t < tmax) return true;
        }
    }
    return false;
}

// the tree in both forms, as the kernels take it
struct RcTree {
    const float4* nodes; const float4* tris;
    const int* info; const float* aabb; const float* vert; const int* faces;
};
template <bool PACKED>
__device__ __forceinline__ bool rc_any(const RcTree& tr, const CloseRay& r, float tmax, unsigned& nv) {
    return PACKED ? bvh_any_packed(tr.nodes, tr.tris, r, tmax, nv) : bvh_any_stack(tr.info, tr.aabb, tr.vert, tr.faces, r, tmax, nv);
}
// diagnostics (tools/bench_raycast.py: nodes visited per ray): wave sum, one atomic per wave
__device__ __forceinline__ void rc_count(unsigned long long* visited, unsigned nv) {
    if (!visited) return;
    for (int o = 32; o > 0; o >>= 1) nv += __shfl_xor(nv, o, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(visited, (unsigned long long)nv);
}

// ---- (a) closest hit.  One thread per ray, in the caller's order.  Every output may be null.  face_mask [F] (the scatter of utx_visible_faces_rays: plain byte
// stores of the value 1, so their order does not matter) is NOT cleared here: the caller zeroes it, or accumulates over several launches.
template <bool PACKED>
__global__ __launch_bounds__(256) void raycast_intersect_kernel(const RcTree tr, const float* __restrict__ ro, const float* __restrict__ rd, long R, int* __restrict__ tid,
                                                                float* __restrict__ t_out, float* __restrict__ loc, float* __restrict__ uv,
                                                                unsigned char* __restrict__ front, unsigned char* face_mask, unsigned long long* visited) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned nv = 0;
    if (i < R) {
        const float o[3] = {ro[3 * i], ro[3 * i + 1], ro[3 * i + 2]};
        const float d[3] = {rd[3 * i], rd[3 * i + 1], rd[3 * i + 2]};
        const CloseRay r = close_ray(o, d);
        const int hit = PACKED ? bvh_closest_packed(tr.nodes, tr.tris, r, nv) : bvh_closest_stack(tr.info, tr.aabb, tr.vert, tr.faces, r, nv);
        float t = __int_as_float(0x7f800000), u = 0.f, v = 0.f, q[3] = {0.f, 0.f, 0.f};
        unsigned char fr = 0;
        if (hit >= 0) {      // the winner once more: the same function on the same numbers, so t is the walk's own
            float v0[3], v1[3], v2[3];
            if (PACKED) {
                const float4 a = tr.tris[3 * (long)hit], b = tr.tris[3 * (long)hit + 1], c = tr.tris[3 * (long)hit + 2];
                v0[0] = a.x; v0[1] = a.y; v0[2] = a.z; v1[0] = b.x; v1[1] = b.y; v1[2] = b.z; v2[0] = c.x; v2[1] = c.y; v2[2] = c.z;
            } else {
                const int* f = tr.faces + 3 * (long)hit;
#pragma unroll
                for (int k = 0; k < 3; ++k) { v0[k] = tr.vert[3 * (long)f[0] + k]; v1[k] = tr.vert[3 * (long)f[1] + k]; v2[k] = tr.vert[3 * (long)f[2] + k]; }
            }
            (void)close_tri_uv(r, v0, v1, v2, t, u, v);
            const float E1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]};
            const float E2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
            float n[3]; cross3(E1, E2, n);
            fr = dot3(d, n) < 0.f ? 1 : 0;
#pragma unroll
            for (int k = 0; k < 3; ++k) { const float s = t * d[k]; q[k] = o[k] + s; }
            if (face_mask) face_mask[hit] = 1;
        }
        if (tid) tid[i] = hit;
        if (t_out) t_out[i] = t;
        if (loc) { loc[3 * i] = q[0]; loc[3 * i + 1] = q[1]; loc[3 * i + 2] = q[2]; }
        if (uv) { uv[2 * i] = u; uv[2 * i + 1] = v; }
        if (front) front[i] = fr;
    }
    rc_count(visited, nv);
}

// ---- (b) segments: blocked iff some triangle is hit with 0 <= t < 1 along d = to - from (not normalised: Moeller-Trumbore's t scales with 1 / |d|)
template <bool PACKED>
__global__ __launch_bounds__(256) void raycast_occluded_kernel(const RcTree tr, const float* __restrict__ from, const float* __restrict__ to, long R,
                                                               unsigned char* __restrict__ blocked, unsigned long long* visited) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned nv = 0;
    if (i < R) {
        const float o[3] = {from[3 * i], from[3 * i + 1], from[3 * i + 2]};
        const float d[3] = {to[3 * i] - o[0], to[3 * i + 1] - o[1], to[3 * i + 2] - o[2]};
        blocked[i] = rc_any<PACKED>(tr, close_ray(o, d), 1.0f, nv) ? 1 : 0;
    }
    rc_count(visited, nv);
}

// ---- the direction stream: ray `ray` of point `point` on stream `sid`.  Marsaglia (1972): (x1, x2) uniform in the square, rejected while s = x1^2 + x2^2 >= 1;
// d = (2 x1 sqrt(1 - s), 2 x2 sqrt(1 - s), 1 - 2 s) is uniform on the sphere.  Philox counter (point, ray, attempt, sid), words 0 and 1 of each draw,
// u = (word >> 8) 2^-24.  Products, sums and the correctly rounded square root only: numpy float32 repeats every bit.  64 attempts, then (0, 0, 1)
// (probability (1 - pi / 4)^64, about 1e-43).
__device__ __forceinline__ void sphere_direction(unsigned point, unsigned ray, unsigned k0, unsigned k1, unsigned sid, float d[3]) {
    const float sc = 1.0f / 16777216.0f;
    for (unsigned attempt = 0; attempt < 64u; ++attempt) {
        unsigned w[4];
        philox4x32_10(point, ray, attempt, sid, k0, k1, w);
        const float x1 = 2.0f * ((float)(w[0] >> 8) * sc) - 1.0f, x2 = 2.0f * ((float)(w[1] >> 8) * sc) - 1.0f;
        const float s = x1 * x1 + x2 * x2;
        if (s < 1.0f) {
            const float q = sqrtf(1.0f - s);      // hipcc's default: correctly rounded (__fsqrt_rn is NOT: it is the native instruction unless OCML's rounded operations are on)
            d[0] = (2.0f * x1) * q; d[1] = (2.0f * x2) * q; d[2] = 1.0f - 2.0f * s;
            return;
        }
    }
    d[0] = 0.f; d[1] = 0.f; d[2] = 1.f;
}

__global__ __launch_bounds__(256) void sphere_directions_kernel(long total, long n_rays, unsigned k0, unsigned k1, unsigned sid, float* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    float d[3];
    sphere_direction((unsigned)(i / n_rays), (unsigned)(i % n_rays), k0, k1, sid, d);
    out[3 * i] = d[0]; out[3 * i + 1] = d[1]; out[3 * i + 2] = d[2];
}

// ---- (c) points enclosed: inner iff every one of the point's n_rays rays has a hit with t >= 0.  G = min(64, next power of two >= n_rays) lanes serve a
// point (G divides the wave, so a group never straddles two waves); lane j of the group walks the rays j, j + G, j + 2 G, ...  After each such outer step a wave
// ballot tells every group whether one of its lanes has completed a miss: the point is decided, the group takes no further rays (early = false: it goes on, and
// hits [N] is the exact number of rays that hit).  The ray a lane takes depends on (point, ray index) alone, never on the launch geometry.
// dirs [N][n_rays][3], if given, is read instead of the generator.
template <bool PACKED>
__global__ __launch_bounds__(256) void points_enclosed_kernel(const RcTree tr, const float* __restrict__ points, long N, int n_rays, int G, unsigned k0, unsigned k1,
                                                              unsigned sid, const float* __restrict__ dirs, int early, unsigned char* __restrict__ inner,
                                                              int* __restrict__ hits, unsigned long long* visited) {
    const long gt = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long p = gt / G;
    const int lane = threadIdx.x & 63, gl = lane & (G - 1);
    const unsigned long long gmask = (G == 64 ? ~0ull : ((1ull << G) - 1ull)) << (lane - gl);
    const bool valid = p < N;
    float o[3] = {0.f, 0.f, 0.f};
    if (valid) { o[0] = points[3 * p]; o[1] = points[3 * p + 1]; o[2] = points[3 * p + 2]; }
    unsigned nv = 0;
    int cnt = 0;
    bool miss = false, decided = !valid;
    const int steps = (n_rays + G - 1) / G;      // the same for every lane: the ballots below are reached by the whole wave
    for (int s = 0; s < steps; ++s) {
        const int ray = s * G + gl;
        if (!decided && ray < n_rays) {
            float d[3];
            if (dirs) { const float* dp = dirs + 3 * (p * n_rays + ray); d[0] = dp[0]; d[1] = dp[1]; d[2] = dp[2]; }
            else sphere_direction((unsigned)p, (unsigned)ray, k0, k1, sid, d);
            if (rc_any<PACKED>(tr, close_ray(o, d), __int_as_float(0x7f800000), nv)) ++cnt; else miss = true;
        }
        if (early) {
            if (__ballot(miss) & gmask) decided = true;
            if (__ballot(!decided) == 0ull) break;      // wave-uniform
        }
    }
    const bool any_miss = (__ballot(miss) & gmask) != 0ull;
    for (int off = 1; off < G; off <<= 1) cnt += __shfl_xor(cnt, off, 64);      // the group is an aligned power of two of lanes: the butterfly stays inside it
    if (valid && gl == 0) {
        inner[p] = any_miss ? 0 : 1;
        if (hits) hits[p] = cnt;
    }
    rc_count(visited, nv);
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
// which walk: 1 packed, 0 stack, < 0 the error (-7: the build's depth never arrived; -2: too deep for the stack walk)
static int rc_walk(utx_bvh* b, int force_stack) {
    const int depth = utx_bvh_depth_impl(b);
    if (depth < 0) return -7;
    const bool packed = depth <= UTX_BVH_PACKED_MAX_DEPTH && !force_stack;
    if (!packed && depth + 2 > CLOSE_STACK) return -2;
    return packed ? 1 : 0;
}
static RcTree rc_tree(const utx_bvh* b) { return RcTree{b->nodes, b->tris, b->info, b->aabb, b->verts, b->faces}; }

extern "C" int utx_bvh_intersect_impl(utx_bvh* b, const float* ro, const float* rd, long R, int* tid, float* t, float* loc, float* uv, unsigned char* front,
                                      unsigned char* face_mask, unsigned long long* visited, int flags, hipStream_t stream) {
    if (!b || b->F < 1 || R < 0 || R >= (1l << 31) || (flags & ~1)) return -2;
    if (R == 0) return 0;
    if (!ro || !rd) return -2;
    const int walk = rc_walk(b, flags & 1);
    if (walk < 0) return walk;
    const dim3 g((unsigned)((R + 255) / 256)), blk(256);
    if (walk) hipLaunchKernelGGL(raycast_intersect_kernel<true>, g, blk, 0, stream, rc_tree(b), ro, rd, R, tid, t, loc, uv, front, face_mask, visited);
    else hipLaunchKernelGGL(raycast_intersect_kernel<false>, g, blk, 0, stream, rc_tree(b), ro, rd, R, tid, t, loc, uv, front, face_mask, visited);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

extern "C" int utx_bvh_occluded_impl(utx_bvh* b, const float* from, const float* to, long R, unsigned char* blocked, unsigned long long* visited, int flags,
                                     hipStream_t stream) {
    if (!b || b->F < 1 || R < 0 || R >= (1l << 31) || (flags & ~1)) return -2;
    if (R == 0) return 0;
    if (!from || !to || !blocked) return -2;
    const int walk = rc_walk(b, flags & 1);
    if (walk < 0) return walk;
    const dim3 g((unsigned)((R + 255) / 256)), blk(256);
    if (walk) hipLaunchKernelGGL(raycast_occluded_kernel<true>, g, blk, 0, stream, rc_tree(b), from, to, R, blocked, visited);
    else hipLaunchKernelGGL(raycast_occluded_kernel<false>, g, blk, 0, stream, rc_tree(b), from, to, R, blocked, visited);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

extern "C" int utx_points_enclosed_impl(utx_bvh* b, const float* points, long N, int n_rays, unsigned long long seed, unsigned stream_id, const float* dirs,
                                        unsigned char* inner, int* hits, unsigned long long* visited, int flags, hipStream_t stream) {
    if (!b || b->F < 1 || N < 0 || N >= (1l << 31) || n_rays < 1 || n_rays > 1024 || (flags & ~3)) return -2;
    if (N == 0) return 0;
    if (!points || !inner) return -2;
    const int walk = rc_walk(b, flags & 1);
    if (walk < 0) return walk;
    int G = 1;
    while (G < n_rays && G < 64) G <<= 1;
    const dim3 g((unsigned)((N * G + 255) / 256)), blk(256);      // N < 2^31, G <= 64: at most 2^29 blocks
    const unsigned k0 = (unsigned)seed, k1 = (unsigned)(seed >> 32);
    const int early = (flags & 2) ? 0 : 1;
    if (walk) hipLaunchKernelGGL(points_enclosed_kernel<true>, g, blk, 0, stream, rc_tree(b), points, N, n_rays, G, k0, k1, stream_id, dirs, early, inner, hits, visited);
    else hipLaunchKernelGGL(points_enclosed_kernel<false>, g, blk, 0, stream, rc_tree(b), points, N, n_rays, G, k0, k1, stream_id, dirs, early, inner, hits, visited);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

extern "C" int utx_launch_sphere_directions(long n_points, long n_rays, unsigned long long seed, unsigned stream_id, float* out, hipStream_t stream) {
    if (n_points < 0 || n_rays < 0 || n_points >= (1l << 31) || n_rays >= (1l << 31)) return -2;
    const long total = n_points * n_rays;      // both < 2^31: no overflow
    if (total >= (1l << 31)) return -2;
    if (total == 0) return 0;
    if (!out) return -2;
    hipLaunchKernelGGL(sphere_directions_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, total, n_rays, (unsigned)seed, (unsigned)(seed >> 32),
                       stream_id, out);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// Device-side LBVH traversal shared by bvh.hip (utx_bvh_trace) and backproject.hip (fused visibility).
// Reproduces intersect_test2.slang:14-146 of the reference including its quirks; see bvh.hip / oracle header.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ bool aabb_hit(const float* ro, const float* rd, float tmin, float tmax, const float* bb) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float d = rd[i];
        if (d == 0.f) d = 0.000001f;
        const float inv = 1.0f / d;
        float t0 = (bb[i] - ro[i]) * inv;
        float t1 = (bb[3 + i] - ro[i]) * inv;
        if (inv < 0.0f) { const float t = t1; t1 = t0; t0 = t; }
        tmin = t0 > tmin ? t0 : tmin;
        tmax = t1 < tmax ? t1 : tmax;
        if (tmax < tmin) return false;
    }
    return true;
}
__device__ __forceinline__ float dot3(const float* a, const float* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
__device__ __forceinline__ void cross3(const float* a, const float* b, float* o) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ bool tri_hit(const float* ro, const float* rd, const float* v0, const float* v1, const float* v2, float& t_out) {
    const float eps = 1e-9f;
    const float E1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]};
    const float E2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
    float P[3]; cross3(rd, E2, P);
    const float det = dot3(E1, P);
    if (det > -eps && det < eps) return false;
    const float inv = 1.0f / det;
    const float T[3] = {ro[0] - v0[0], ro[1] - v0[1], ro[2] - v0[2]};
    const float u = dot3(T, P) * inv;
    if (u < 0 || u > 1) return false;
    float Q[3]; cross3(T, E1, Q);
    const float v = dot3(rd, Q) * inv;
    if (v < 0 || u + v > 1) return false;
    t_out = dot3(E2, Q) * inv;
    return true;
}

__device__ __forceinline__ int bvh_trace_one(const int* __restrict__ info, const float* __restrict__ aabb, const float* __restrict__ vert,
                             const int* __restrict__ faces, const float* ro, const float* rd_in) {
    const float nrm = sqrtf(dot3(rd_in, rd_in));
    const float rd[3] = {rd_in[0] / nrm, rd_in[1] / nrm, rd_in[2] / nrm};
    int stack[64];
    int count = 0;
    stack[count++] = 0;
    float closest = 1e9f;
    int hit_tid = -1;
    while (count > 0) {
        const int nd = stack[--count];
        float bb[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) bb[k] = aabb[6 * (long)nd + k];
        if (!aabb_hit(ro, rd, 0.f, closest, bb)) continue;
        const int L = info[3 * (long)nd], R = info[3 * (long)nd + 1];
        if (L != 0 && R != 0) {
            if (count + 2 <= 64) { stack[count++] = L; stack[count++] = R; }
        } else if (L == 0 && R == 0) {
            const int prim = info[3 * (long)nd + 2];
            const int* f = faces + 3 * (long)prim;
            float t;
            if (tri_hit(ro, rd, vert + 3 * (long)f[0], vert + 3 * (long)f[1], vert + 3 * (long)f[2], t)) {
                closest = t < closest ? t : closest;
                hit_tid = prim;
            }
        }
    }
    return hit_tid;
}


// ---- the same traversal over the PACKED tree (built by bvh_pack_kernel; used whenever the tree is shallow enough that the
// reference's 64-entry stack can never overflow, i.e. always in practice):
//   node  = two 16-byte words  {bb[0..3]} {bb[4], bb[5], link, esc}      (the reference reads 6 + 3 scalar dwords from two arrays)
//           link > 0: internal node, link = its SECOND child (the reference pushes first, second and pops the second first);
//           link < 0: leaf of primitive ~link.  esc = the node the reference would pop after this node's subtree is done:
//           the first child of the parent for a second child, the parent's esc for a first child, -1 at the root.
//   tri   = three 16-byte words {v0, 0} {v1, 0} {v2, 0}                  (the reference chases faces[] then three vertices)
// No stack, so no scratch memory and no dependent index load between "pop" and the next box test.  The order in which nodes and
// triangles are visited -- and with it the quirk that the LAST triangle hit wins, not the closest -- is the reference's exactly:
// miss -> esc; internal hit -> second child (whose esc is the first child); leaf -> test, esc.
__device__ __forceinline__ int bvh_trace_packed(const float4* __restrict__ nodes, const float4* __restrict__ tris, const float* ro,
                                                const float* rd_in, unsigned* visited) {
    const float nrm = sqrtf(dot3(rd_in, rd_in));
    const float rd[3] = {rd_in[0] / nrm, rd_in[1] / nrm, rd_in[2] / nrm};
    float closest = 1e9f;
    int hit_tid = -1;
    int nd = 0;
    unsigned nv = 0;
    while (nd >= 0) {
        const float4 a = nodes[2 * (long)nd], b = nodes[2 * (long)nd + 1];
        const float bb[6] = {a.x, a.y, a.z, a.w, b.x, b.y};
        const int link = __float_as_int(b.z), esc = __float_as_int(b.w);
        ++nv;
        if (!aabb_hit(ro, rd, 0.f, closest, bb)) { nd = esc; continue; }
        if (link > 0) { nd = link; continue; }
        const int prim = ~link;
        const float4 t0 = tris[3 * (long)prim], t1 = tris[3 * (long)prim + 1], t2 = tris[3 * (long)prim + 2];
        const float v0[3] = {t0.x, t0.y, t0.z}, v1[3] = {t1.x, t1.y, t1.z}, v2[3] = {t2.x, t2.y, t2.z};
        float t;
        if (tri_hit(ro, rd, v0, v1, v2, t)) {
            closest = t < closest ? t : closest;
            hit_tid = prim;
        }
        nd = esc;
    }
    if (visited) *visited = nv;
    return hit_tid;
}

// ---- the same traversal for a COHERENT PACKET: the 64 rays of a wave walk the packed tree together (backproject.hip: an 8 x 8 texel tile of one view --
// parallel rays from neighbouring surface points).  One node per step for the whole wave, fetched through the SCALAR cache (a uniform 32-byte
// s_load instead of 64 divergent 2 x 16-byte vector loads per step: the thread-per-ray walk is bound by exactly those -- 50 dependent divergent
// fetches per ray); each lane tests the box with its OWN ray and its OWN `closest`; the packet descends where any lane hits, and a lane takes part
// in a node iff it hit every ancestor -- the 64-bit masks travel with the packet's DFS stack (<= depth entries of {node, mask}, kept lane-distributed
// in LDS, 12 bytes per entry and wave, written and read wave-uniformly).  (A first version kept the stack lane-distributed in VGPRs -- entry i in lane i,
// v_writelane / v_readlane -- and hung the GPU: entries parked in lanes that are INACTIVE in the calling branch are lost whenever the compiler copies the
// register, because its copies are EXEC-masked.)
// Per lane the sequence of nodes it takes part in, and of triangles it tests, is EXACTLY the sequence of its own stackless walk above (the packet
// visits second child before first child, as the reference pops them; a lane that misses a node skips the subtree as `esc` would): the same
// `closest` at every test, the same last-hit-wins result -- bit-identical to bvh_trace_packed, ray by ray.  `first child` is not stored in a node:
// it is the escape link of the second child, so the push of (first child, mask) happens when the second child's words arrive.
typedef float bvh_f32x8 __attribute__((ext_vector_type(8)));
typedef float bvh_f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ bvh_f32x8 bvh_sload8(const void* p) {
    bvh_f32x8 r;
    asm volatile("s_load_dwordx8 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r) : "s"(p) : "memory");
    return r;
}
__device__ __forceinline__ bvh_f32x4 bvh_sload4(const void* p) {
    bvh_f32x4 r;
    asm volatile("s_load_dwordx4 %0, %1, 0x0\n\ts_waitcnt lgkmcnt(0)" : "=s"(r) : "s"(p) : "memory");
    return r;
}
__device__ __forceinline__ int bvh_trace_packet(const float4* __restrict__ nodes, const float4* __restrict__ tris, const float* ro, const float* rd_in,
                                                bool valid, int* stk /* this wave's 64 x 3 ints of LDS */, unsigned* visited) {
    const float nrm = sqrtf(dot3(rd_in, rd_in));
    const float rd[3] = {rd_in[0] / nrm, rd_in[1] / nrm, rd_in[2] / nrm};
    float closest = 1e9f;
    int hit_tid = -1;
    unsigned nv = 0;
    const unsigned lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
    const unsigned long long lbit = 1ull << lane;
    int sp = 0;                                        // the packet's stack: stk[3 sp + {0, 1, 2}] = {node, mask lo, mask hi}
    int cur = 0;
    unsigned long long cm = __ballot(valid);
    bool pend = false;                                 // the first child of the node just descended from is still to be pushed (with mask pm)
    unsigned long long pm = 0;
    while (cm != 0) {
        const bvh_f32x8 n8 = bvh_sload8((const char*)nodes + (long)cur * 32);
        const float bb[6] = {n8[0], n8[1], n8[2], n8[3], n8[4], n8[5]};
        const int link = __float_as_int(n8[6]), esc = __float_as_int(n8[7]);
        if (pend) {
            stk[3 * sp] = esc; stk[3 * sp + 1] = (int)(unsigned)pm; stk[3 * sp + 2] = (int)(unsigned)(pm >> 32);      // every active lane writes the same words
            ++sp;
            pend = false;
        }
        const bool act = (cm & lbit) != 0;
        if (act) ++nv;
        const bool h = act && aabb_hit(ro, rd, 0.f, closest, bb);
        const unsigned long long hm = __ballot(h);
        if (link > 0) {
            if (hm != 0) { cur = link; cm = hm; pm = hm; pend = true; continue; }
        } else if (hm != 0) {
            const int prim = ~link;
            const char* tp = (const char*)tris + (long)prim * 48;
            const bvh_f32x8 ta = bvh_sload8(tp);
            const bvh_f32x4 tb = bvh_sload4(tp + 32);
            if (h) {
                const float v0[3] = {ta[0], ta[1], ta[2]}, v1[3] = {ta[4], ta[5], ta[6]}, v2[3] = {tb[0], tb[1], tb[2]};
                float t;
                if (tri_hit(ro, rd, v0, v1, v2, t)) {
                    closest = t < closest ? t : closest;
                    hit_tid = prim;
                }
            }
        }
        if (sp == 0) break;
        --sp;
        cur = __builtin_amdgcn_readfirstlane(stk[3 * sp]);
        cm = (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane(stk[3 * sp + 1]) |
             ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane(stk[3 * sp + 2]) << 32);
    }
    if (visited) *visited = nv;
    return hit_tid;
}

// ---- CLOSEST hit (utx_visible_faces_rays): what Mesh.get_visible_faces of the reference gets from Embree through open3d's RaycastingScene
// (mesh/structure.py:801-844) -- the hit with the smallest t among those with t >= 0, no backface culling -- and none of the quirks above.  The direction
// is NOT normalised (t is in units of |rd|, as Embree's): the order of the hits along a ray does not depend on the scale.  Ties in t go to the smallest
// primitive id, so the result does not depend on the order in which the triangles are met.
// The ray: origin, direction and the reciprocal direction of the slab test, formed once per ray; a zero component is replaced by 1e-30 (1 / 1e-30 is finite, so
// (bb - ro) * inv is 0 or +-huge, never NaN).
struct CloseRay { float o[3], d[3], inv[3]; };
__device__ __forceinline__ CloseRay close_ray(const float* ro, const float* rd) {
    CloseRay r;
#pragma unroll
    for (int i = 0; i < 3; ++i) { r.o[i] = ro[i]; r.d[i] = rd[i]; r.inv[i] = 1.0f / (rd[i] == 0.f ? 1e-30f : rd[i]); }
    return r;
}
// slab test against [0, limit]; conservative: the far side is widened by 4e-7 (two ulp; Ize, "Robust BVH ray traversal", 2013), so that a box of no thickness
// (an axis-aligned triangle) and a hit on a box face are not lost to the rounding of the three products
__device__ __forceinline__ bool close_box(const CloseRay& r, float limit, const float* bb) {
    float tmin = 0.f, tmax = limit;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float t0 = (bb[i] - r.o[i]) * r.inv[i], t1 = (bb[3 + i] - r.o[i]) * r.inv[i];
        tmin = fmaxf(tmin, fminf(t0, t1));
        tmax = fminf(tmax, fmaxf(t0, t1) * 1.0000004f);
    }
    return tmin <= tmax;
}
// Moeller-Trumbore, both sides; t >= 0 only.  close_tri_uv also hands out the barycentrics (u weighs v1, v and v2) of a hit; close_tri is the same arithmetic
__device__ __forceinline__ bool close_tri_uv(const CloseRay& r, const float* v0, const float* v1, const float* v2, float& t_out, float& u_out, float& v_out) {
    const float E1[3] = {v1[0] - v0[0], v1[1] - v0[1], v1[2] - v0[2]};
    const float E2[3] = {v2[0] - v0[0], v2[1] - v0[1], v2[2] - v0[2]};
    float P[3]; cross3(r.d, E2, P);
    const float det = dot3(E1, P);
    if (det == 0.f) return false;
    const float inv = 1.0f / det;
    const float T[3] = {r.o[0] - v0[0], r.o[1] - v0[1], r.o[2] - v0[2]};
    const float u = dot3(T, P) * inv;
    if (!(u >= 0.f && u <= 1.f)) return false;
    float Q[3]; cross3(T, E1, Q);
    const float v = dot3(r.d, Q) * inv;
    if (!(v >= 0.f && u + v <= 1.f)) return false;
    const float t = dot3(E2, Q) * inv;
    if (!(t >= 0.f)) return false;
    t_out = t; u_out = u; v_out = v;
    return true;
}
__device__ __forceinline__ bool close_tri(const CloseRay& r, const float* v0, const float* v1, const float* v2, float& t_out) {
    float u, v;
    return close_tri_uv(r, v0, v1, v2, t_out, u, v);
}
__device__ __forceinline__ void close_take(float t, int prim, float& closest, int& hit) {
    if (t < closest || (t == closest && prim < hit)) { closest = t; hit = prim; }
}
// a subtree is skipped only if its box starts beyond the best hit by more than a part in a million: a triangle that TIES with the best hit is still tested
#define CLOSE_LIMIT(closest) ((closest) * 1.000001f)

// the packed walk (no stack: any depth would do; the launcher keeps the depth rule of the other traversals)
__device__ __forceinline__ int bvh_closest_packed(const float4* __restrict__ nodes, const float4* __restrict__ tris, const CloseRay& r, unsigned& nv) {
    float closest = __int_as_float(0x7f800000);
    int hit = -1, nd = 0;
    while (nd >= 0) {
        const float4 a = nodes[2 * (long)nd], b = nodes[2 * (long)nd + 1];
        const float bb[6] = {a.x, a.y, a.z, a.w, b.x, b.y};
        const int link = __float_as_int(b.z), esc = __float_as_int(b.w);
        ++nv;
        if (!close_box(r, CLOSE_LIMIT(closest), bb)) { nd = esc; continue; }
        if (link > 0) { nd = link; continue; }
        const int prim = ~link;
        const float4 t0 = tris[3 * (long)prim], t1 = tris[3 * (long)prim + 1], t2 = tris[3 * (long)prim + 2];
        const float v0[3] = {t0.x, t0.y, t0.z}, v1[3] = {t1.x, t1.y, t1.z}, v2[3] = {t2.x, t2.y, t2.z};
        float t;
        if (close_tri(r, v0, v1, v2, t)) close_take(t, prim, closest, hit);
        nd = esc;
    }
    return hit;
}
// the stack walk over the unpacked arrays, in the SAME order (first and second child pushed, the second popped first), with the same tests on the same
// numbers: its result equals the packed walk's.  The walk holds at most depth + 1 entries; the launcher (utx_visible_faces_rays_impl) refuses a tree with
// depth + 2 > CLOSE_STACK, so the guard in front of the push below never drops a subtree (a tree of 30 Morton bits + 32 index bits is at most 62 deep).
#define CLOSE_STACK 96
__device__ __forceinline__ int bvh_closest_stack(const int* __restrict__ info, const float* __restrict__ aabb, const float* __restrict__ vert,
                                                 const int* __restrict__ faces, const CloseRay& r, unsigned& nv) {
    int stack[CLOSE_STACK];
    int count = 0;
    stack[count++] = 0;
    float closest = __int_as_float(0x7f800000);
    int hit = -1;
    while (count > 0) {
        const int nd = stack[--count];
        float bb[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) bb[k] = aabb[6 * (long)nd + k];
        ++nv;
        if (!close_box(r, CLOSE_LIMIT(closest), bb)) continue;
        const int L = info[3 * (long)nd], R = info[3 * (long)nd + 1];
        if (L != 0 || R != 0) {
            if (count + 2 <= CLOSE_STACK) { stack[count++] = L; stack[count++] = R; }
        } else {
            const int prim = info[3 * (long)nd + 2];
            const int* f = faces + 3 * (long)prim;
            float t;
            if (close_tri(r, vert + 3 * (long)f[0], vert + 3 * (long)f[1], vert + 3 * (long)f[2], t)) close_take(t, prim, closest, hit);
        }
    }
    return hit;
}

#include <atomic>
struct utx_bvh {
    int F;
    int* info;       // [2F-1][3]
    float* aabb;     // [2F-1][6]
    const float* verts;  // borrowed (caller keeps them alive while the bvh is used)
    const int* faces;
    // build temporaries (kept: small)
    float* ebox;     // [F][6]
    unsigned* codes; unsigned* codes_sorted; int* idx; int* idx_sorted;
    int* parent;     // [2F-1]
    int* counter;    // [F-1]
    unsigned* extent;  // 6 ordered-uint min/max
    void* sort_tmp; size_t sort_tmp_bytes;
    float4* nodes;   // [2F-1][2] packed tree (bvh_trace_packed)
    float4* tris;    // [F][3]
    int* depth_dev;  // max number of ancestors of a leaf
    std::atomic<int> depth;   // host copy (-1: not read back yet -- utx_bvh_depth_impl waits for depth_ready once; atomic: a handle may see its first launches from two threads); the packed traversal is used when depth <= UTX_BVH_PACKED_MAX_DEPTH
    int* depth_host;           // pinned word the build copies depth_dev into
    hipEvent_t depth_ready;    // recorded behind that copy
    void* owned;               // the one hipMalloc of utx_bvh_build (null: the arrays live in the caller's workspace, utx_bvh_build_ws)
};
#define UTX_BVH_PACKED_MAX_DEPTH 60   // the reference's stack holds 64 entries and the walk keeps at most depth + 1 of them

// ---- NEAREST SURFACE POINT (utx_bvh_closest_point): what the reference takes from cuBVH.unsigned_distance(points, return_uvw=True) [3p, absent]
// (geometry/sampling/spatial_sampling.py:36,90).  A point query, no ray.
// tri_closest: the Voronoi-region form of Ericson, Real-Time Collision Detection, 5.1.5, in fp32 with every sum in a fixed order, so that a numpy float32
// restatement (oracle/closest_point_ref.py) repeats it bit for bit.  (u, v, w) weigh (v0, v1, v2); q = (u v0 + v v1) + w v2; d2 = |p - q|^2 summed like dot3.
// Beyond Ericson: a quotient whose denominator is not > 0 is 0 (a zero-length edge counts as its end point); the interior weights are clamped (v to [0, 1],
// w to [0, 1 - v], u = (1 - v) - w), so every weight is >= 0; and where the interior denominator va + vb + vc (|ab x ac|^2) is not > 0 -- a zero-area face, whose
// regions mean nothing -- the answer is the nearest of the three edge segments AB, AC, BC, the first of them on a tie.
struct TriClosest { float d2, u, v, w; };
__device__ __forceinline__ float cp_div(float n, float d) { return d > 0.f ? n / d : 0.f; }
__device__ __forceinline__ float cp_eval(const float* p, const float* a, const float* b, const float* c, float u, float v, float w) {
    float r[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) r[k] = p[k] - ((u * a[k] + v * b[k]) + w * c[k]);
    return dot3(r, r);
}
__device__ __forceinline__ float cp_seg_t(const float* xp, const float* e) { return fminf(fmaxf(cp_div(dot3(xp, e), dot3(e, e)), 0.f), 1.f); }
__device__ __forceinline__ TriClosest tri_closest(const float* p, const float* a, const float* b, const float* c) {
    float ab[3], ac[3], bc[3], ap[3], bp[3], cp[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { ab[k] = b[k] - a[k]; ac[k] = c[k] - a[k]; bc[k] = c[k] - b[k]; ap[k] = p[k] - a[k]; bp[k] = p[k] - b[k]; cp[k] = p[k] - c[k]; }
    const float d1 = dot3(ab, ap), d2 = dot3(ac, ap), d3 = dot3(ab, bp), d4 = dot3(ac, bp), d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    const float den = (va + vb) + vc;      // |ab x ac|^2 up to rounding
    TriClosest r;
    if (!(den > 0.f)) {      // no area (or not a number): Ericson's regions presuppose one -- the nearest of the three edge segments
        const float t0 = cp_seg_t(ap, ab), t1 = cp_seg_t(ap, ac), t2 = cp_seg_t(bp, bc);
        const float e0 = cp_eval(p, a, b, c, 1.f - t0, t0, 0.f), e1 = cp_eval(p, a, b, c, 1.f - t1, 0.f, t1), e2 = cp_eval(p, a, b, c, 0.f, 1.f - t2, t2);
        r.u = 1.f - t0; r.v = t0; r.w = 0.f;
        float e = e0;
        if (e1 < e) { e = e1; r.u = 1.f - t1; r.v = 0.f; r.w = t1; }
        if (e2 < e) { r.u = 0.f; r.v = 1.f - t2; r.w = t2; }
    }
    else if (d1 <= 0.f && d2 <= 0.f) { r.u = 1.f; r.v = 0.f; r.w = 0.f; }
    else if (d3 >= 0.f && d4 <= d3) { r.u = 0.f; r.v = 1.f; r.w = 0.f; }
    else if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) { r.v = cp_div(d1, d1 - d3); r.u = 1.f - r.v; r.w = 0.f; }
    else if (d6 >= 0.f && d5 <= d6) { r.u = 0.f; r.v = 0.f; r.w = 1.f; }
    else if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) { r.w = cp_div(d2, d2 - d6); r.u = 1.f - r.w; r.v = 0.f; }
    else if (va <= 0.f && d4 - d3 >= 0.f && d5 - d6 >= 0.f) { r.w = cp_div(d4 - d3, (d4 - d3) + (d5 - d6)); r.v = 1.f - r.w; r.u = 0.f; }
    else {
        const float inv = 1.0f / den;
        r.v = fminf(fmaxf(vb * inv, 0.f), 1.f);
        r.w = fminf(fmaxf(vc * inv, 0.f), 1.f - r.v);
        r.u = (1.f - r.v) - r.w;
    }
    r.d2 = cp_eval(p, a, b, c, r.u, r.v, r.w);
    return r;
}
// squared distance from p to a box: sum of max(0, lo - p, p - hi)^2, summed like dot3
__device__ __forceinline__ float cp_box_d2(const float* p, const float4& a, const float4& b) {
    const float ex[3] = {fmaxf(0.f, fmaxf(a.x - p[0], p[0] - a.w)), fmaxf(0.f, fmaxf(a.y - p[1], p[1] - b.x)), fmaxf(0.f, fmaxf(a.z - p[2], p[2] - b.y))};
    return dot3(ex, ex);
}
__device__ __forceinline__ void cp_take(const float* p, const float4* __restrict__ tris, int prim, float& best, int& face) {
    const float4 t0 = tris[3 * (long)prim], t1 = tris[3 * (long)prim + 1], t2 = tris[3 * (long)prim + 2];
    const float v0[3] = {t0.x, t0.y, t0.z}, v1[3] = {t1.x, t1.y, t1.z}, v2[3] = {t2.x, t2.y, t2.z};
    const float d2 = tri_closest(p, v0, v1, v2).d2;
    if (d2 < best || (d2 == best && prim < face)) { best = d2; face = prim; }
}
// a subtree is skipped only if its box lies beyond the best squared distance by more than a part in 1e5 (CLOSE_LIMIT's rule, on squares): a triangle that TIES
// with the best is still tested as long as the two roundings differ by less than that RELATIVE margin.  The limit of the rule: tri_closest's error is absolute, a few
// u * scale on q, so for a query within a few u * scale of the surface the computed d2 may lie far below the true one (down to 0) while the box distance of a
// tying face that does not contain p does not -- that face can then be skipped, and the walk may name another of the tying faces than the exhaustive loop does
// (the smallest id among those it met).  d2 is the same either way; the face id is order-independent only outside that band.
#define CP_LIMIT(best) ((best) * 1.00001f)
// The walk over the packed tree, no stack, no LDS, no cross-lane traffic.  First a greedy descent from the root into the child whose box is nearer (a node's first
// child is the esc of its second child), down to a leaf: that gives a finite `best` before the walk proper, which is bvh_closest_packed's esc-link walk with the
// box test above.  The result is the face with the smallest d2, ties to the smallest id, whatever the order of the visits.  seed = false skips the descent.
__device__ __forceinline__ int bvh_nearest_packed(const float4* __restrict__ nodes, const float4* __restrict__ tris, const float* p, bool seed, float& best, unsigned& nv) {
    best = __int_as_float(0x7f800000);
    int face = 0x7fffffff;
    if (seed) {
        int link = __float_as_int(nodes[1].z);      // of the node the descent stands on; at the root of a one-face tree it is a leaf's already
        ++nv;
        while (link > 0) {
            const float4 sa = nodes[2 * (long)link], sb = nodes[2 * (long)link + 1];
            const int first = __float_as_int(sb.w);
            const float4 fa = nodes[2 * (long)first], fb = nodes[2 * (long)first + 1];
            nv += 2;
            link = __float_as_int(cp_box_d2(p, fa, fb) <= cp_box_d2(p, sa, sb) ? fb.z : sb.z);
        }
        cp_take(p, tris, ~link, best, face);
    }
    int nd = 0;
    while (nd >= 0) {
        const float4 a = nodes[2 * (long)nd], b = nodes[2 * (long)nd + 1];
        const int link = __float_as_int(b.z), esc = __float_as_int(b.w);
        ++nv;
        if (cp_box_d2(p, a, b) > CP_LIMIT(best)) { nd = esc; continue; }
        if (link > 0) { nd = link; continue; }
        cp_take(p, tris, ~link, best, face);
        nd = esc;
    }
    return face == 0x7fffffff ? -1 : face;
}

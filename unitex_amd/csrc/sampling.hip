// Geometry sampling for the field stage (reference: pipeline.py:363-407 sampling_on_mesh -> TextureTools/texturetools/geometry/sampling/:
// edge_sampling.py:84-119 sample_on_edges_v2, surface_sampling.py:5-35 sample_surface; the thinning is fpsample [3p], absent) and the exact
// farthest-point sampling that thins those clouds and the atlas texels handed to a colour field (pipeline.py:507-514).  fp32 / integer work, no MFMA.
//
// FPS: one ordinary kernel launch per pick, enqueued from a plain host loop with no synchronisation in it.  Launch k
//   1. reduces the per-workgroup (value, index) partials that launch k - 1 left -- at most FPS_GMAX pairs, so EVERY workgroup does it redundantly and
//      nobody waits for anybody (no cooperative launch, no flag or counter one workgroup would spin on);
//   2. workgroup 0 records the pick;
//   3. every workgroup updates its slice of mind[] with the distance to the pick and writes its own partial for launch k + 1.
// The partials are double-buffered: a workgroup of launch k may write its partial while another one still reads those of launch k - 1.
//   d2 = (dx*dx + dy*dy) + dz*dz in float32 (knn.hip's convention); arg-max with ties towards the lower index.
// mind[i] < 0 marks a point outside the candidate set (masked out, non-finite, already picked, padding): distances are >= 0 or +inf, never NaN
// (the coordinates of a candidate are finite), so one float carries both.
// The numpy restatements the tests hold these kernels to are oracle/sampling_ref.py's.
#include "common.h"
#include "kernels.h"
#include "philox_device.h"
#include "shade_device.h"
#include <float.h>

#define FPS_THREADS 512
#define FPS_WAVES (FPS_THREADS / 64)
#define FPS_GMAX 512

struct FpsBest { float v; int i; };
// total order: larger value first, then lower index; (-1, -1) = "no candidate" loses against everything
__device__ __forceinline__ bool fps_better(float av, int ai, float bv, int bi) { return av > bv || (av == bv && (unsigned)ai < (unsigned)bi); }
__device__ __forceinline__ FpsBest fps_wave_best(FpsBest b) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(b.v, o, 64);
        const int oi = __shfl_xor(b.i, o, 64);
        if (fps_better(ov, oi, b.v, b.i)) { b.v = ov; b.i = oi; }
    }
    return b;
}
// every thread of the workgroup returns the workgroup's best; sv / si: FPS_WAVES entries of LDS (two calls in one kernel are separated by the barrier in front)
__device__ __forceinline__ FpsBest fps_block_best(FpsBest b, float* sv, int* si) {
    b = fps_wave_best(b);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = b.v; si[threadIdx.x >> 6] = b.i; }
    __syncthreads();
    b.v = sv[0]; b.i = si[0];
#pragma unroll
    for (int w = 1; w < FPS_WAVES; ++w)
        if (fps_better(sv[w], si[w], b.v, b.i)) { b.v = sv[w]; b.i = si[w]; }
    return b;
}
__device__ __forceinline__ bool fps_finite3(float x, float y, float z) { return fabsf(x) <= FLT_MAX && fabsf(y) <= FLT_MAX && fabsf(z) <= FLT_MAX; }

// quads [q0, q1) of workgroup w: contiguous slices of `per` quads (4 points each); nq = ceil(N / 4)
__global__ __launch_bounds__(FPS_THREADS) void fps_init_kernel(const float* __restrict__ pos, const unsigned char* __restrict__ mask, long N, long nq, long per,
                                                               float* __restrict__ mind, float* __restrict__ part_v, int* __restrict__ part_i) {
    __shared__ float sv[FPS_WAVES];
    __shared__ int si[FPS_WAVES];
    const long q0 = (long)blockIdx.x * per, q1 = q0 + per < nq ? q0 + per : nq;
    FpsBest b = {-1.0f, -1};
    for (long q = q0 + threadIdx.x; q < q1; q += FPS_THREADS) {
        f32x4 m;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const long i = 4 * q + j;
            float v = -1.0f;
            if (i < N && (!mask || mask[i]) && fps_finite3(pos[3 * i], pos[3 * i + 1], pos[3 * i + 2])) v = INFINITY;
            m[j] = v;
            if (v > b.v) { b.v = v; b.i = (int)i; }
        }
        *(f32x4*)(mind + 4 * q) = m;
    }
    b = fps_block_best(b, sv, si);
    if (threadIdx.x == 0) { part_v[blockIdx.x] = b.v; part_i[blockIdx.x] = b.i; }
}

__global__ __launch_bounds__(FPS_THREADS) void fps_step_kernel(const float* __restrict__ pos, const unsigned char* __restrict__ mask, long N, long nq, long per,
                                                               float* __restrict__ mind, float* __restrict__ part_v, int* __restrict__ part_i, int k, int M, int start,
                                                               int* __restrict__ out_idx, float* __restrict__ out_d2) {
    __shared__ float sv[FPS_WAVES];
    __shared__ int si[FPS_WAVES];
    const int G = gridDim.x;
    const float* pv = part_v + (k & 1) * FPS_GMAX;
    const int* pi = part_i + (k & 1) * FPS_GMAX;
    FpsBest b = {-1.0f, -1};
    for (int g = threadIdx.x; g < G; g += FPS_THREADS)
        if (fps_better(pv[g], pi[g], b.v, b.i)) { b.v = pv[g]; b.i = pi[g]; }
    b = fps_block_best(b, sv, si);
    // a start that is no candidate falls back to the lowest valid index.  Its candidacy is read from the INPUTS, which no launch writes: mind[start] is set
    // to -1 by the workgroup that owns it in this very launch, and a workgroup dispatched after that one would see another first pick than the rest
    if (k == 0 && start >= 0 && (!mask || mask[start]) && fps_finite3(pos[3 * (long)start], pos[3 * (long)start + 1], pos[3 * (long)start + 2])) {
        b.v = INFINITY; b.i = start;
    }
    const int p = b.i;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        out_idx[k] = p;
        if (out_d2) out_d2[k] = b.v;          // +inf for the first pick, -1 once the candidates have run out
    }
    if (k == M - 1) return;
    FpsBest nb = {-1.0f, -1};
    if (p >= 0) {
        const float px = pos[3 * (long)p], py = pos[3 * (long)p + 1], pz = pos[3 * (long)p + 2];
        const long q0 = (long)blockIdx.x * per, q1 = q0 + per < nq ? q0 + per : nq;
        for (long q = q0 + threadIdx.x; q < q1; q += FPS_THREADS) {
            f32x4 m = *(const f32x4*)(mind + 4 * q);
            if (!(m[0] >= 0.0f || m[1] >= 0.0f || m[2] >= 0.0f || m[3] >= 0.0f)) continue;
            float c[12];
            if (4 * q + 3 < N) {            // 48 contiguous, 16-byte aligned bytes
                const f32x4* s = (const f32x4*)(pos + 12 * q);
                const f32x4 a0 = s[0], a1 = s[1], a2 = s[2];
#pragma unroll
                for (int j = 0; j < 4; ++j) { c[j] = a0[j]; c[4 + j] = a1[j]; c[8 + j] = a2[j]; }
            } else {
#pragma unroll
                for (int j = 0; j < 12; ++j) c[j] = (12 * q + j < 3 * N) ? pos[12 * q + j] : 0.0f;
            }
            bool changed = false;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const long i = 4 * q + j;
                float v = m[j];
                if (v >= 0.0f) {
                    if (i == p) { v = -1.0f; changed = true; }
                    else {
                        const float dx = c[3 * j] - px, dy = c[3 * j + 1] - py, dz = c[3 * j + 2] - pz;
                        const float d2 = (dx * dx + dy * dy) + dz * dz;
                        if (d2 < v) { v = d2; changed = true; }
                    }
                    m[j] = v;
                    if (v > nb.v) { nb.v = v; nb.i = (int)i; }
                }
            }
            if (changed) *(f32x4*)(mind + 4 * q) = m;
        }
    }
    nb = fps_block_best(nb, sv, si);
    if (threadIdx.x == 0) { part_v[((k + 1) & 1) * FPS_GMAX + blockIdx.x] = nb.v; part_i[((k + 1) & 1) * FPS_GMAX + blockIdx.x] = nb.i; }
}

static inline size_t fps_mind_bytes(long N) { return ((size_t)((N + 3) / 4) * 16 + 255) & ~(size_t)255; }
extern "C" size_t utx_fps_workspace_bytes_impl(long N) {
    if (N <= 0) return 0;
    return fps_mind_bytes(N) + (size_t)2 * FPS_GMAX * 8;
}

extern "C" int utx_launch_fps(const float* pos, const unsigned char* mask, long N, int M, int start, int* out_idx, float* out_d2, void* work, size_t work_bytes,
                              hipStream_t stream) {
    if (N <= 0 || N >= (1l << 31) || M <= 0 || start < -1 || start >= N) return -2;
    if (((uintptr_t)pos & 15) || ((uintptr_t)work & 15) || work_bytes < utx_fps_workspace_bytes_impl(N)) return -2;
    float* mind = (float*)work;
    float* part_v = (float*)((char*)work + fps_mind_bytes(N));
    int* part_i = (int*)(part_v + 2 * FPS_GMAX);
    const long nq = (N + 3) / 4;
    int ncu = utx_ncu();
    if (ncu > FPS_GMAX) ncu = FPS_GMAX;
    long G = (nq + FPS_THREADS - 1) / FPS_THREADS;      // one workgroup per CU, fewer when not every thread would get a quad
    if (G > ncu) G = ncu;
    const long per = (nq + G - 1) / G;
    G = (nq + per - 1) / per;
    hipLaunchKernelGGL(fps_init_kernel, dim3((unsigned)G), dim3(FPS_THREADS), 0, stream, pos, mask, N, nq, per, mind, part_v, part_i);
    for (int k = 0; k < M; ++k)
        hipLaunchKernelGGL(fps_step_kernel, dim3((unsigned)G), dim3(FPS_THREADS), 0, stream, pos, mask, N, nq, per, mind, part_v, part_i, k, M, start,
                           out_idx, out_d2);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---- sample_on_edges_v2 (edge_sampling.py:102-119): N equal steps along the concatenated selected edges.
// t_i = linspace(0, total, N)[i] with torch's formula (step = total / (N - 1); lower half 0 + step * i, upper half total - step * (N - 1 - i));
// edge = searchsorted(start[1:], t) (lower bound); w = (t - start[e]) / length[e], non-finite -> 0.5, then clamped to [0, 1] (see below); point = w * v0 + (1 - w) * v1.
__global__ __launch_bounds__(256) void sample_edges_kernel(const float* __restrict__ verts, const int* __restrict__ edges, const int* __restrict__ edge_ids,
                                                           const float* __restrict__ start, const float* __restrict__ length, int E, float total, long N,
                                                           float* __restrict__ samples, int* __restrict__ edge_index, float* __restrict__ edge_t) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const float step = total / (float)(N - 1);
    const float t = N == 1 ? 0.0f : (i < N / 2 ? 0.0f + step * (float)i : total - step * (float)(N - 1 - i));      // linspace(.., 1) is its first end
    int lo = 0, hi = E - 1;                 // first j in [0, E - 1) with start[1 + j] >= t, else E - 1
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (start[1 + mid] < t) lo = mid + 1; else hi = mid;
    }
    const int e = lo;
    float w = (t - start[e]) / length[e];
    if (!(fabsf(w) <= FLT_MAX)) w = 0.5f;
    w = fminf(fmaxf(w, 0.0f), 1.0f);        // start[e + 1] is the ROUNDED running sum: t may pass start[e] + length[e] by half a float32 step of it; the sample stays on its edge
    const int a = edges[2 * e], b = edges[2 * e + 1];
    const float u = 1.0f - w;
#pragma unroll
    for (int c = 0; c < 3; ++c) samples[3 * i + c] = w * verts[3 * (long)a + c] + u * verts[3 * (long)b + c];
    if (edge_index) edge_index[i] = edge_ids ? edge_ids[e] : e;
    if (edge_t) edge_t[i] = w;
}

extern "C" int utx_launch_sample_edges(const float* verts, const int* edges, const int* edge_ids, const float* start, const float* length, int E, float total, long N,
                                       float* samples, int* edge_index, float* edge_t, hipStream_t stream) {
    if (E <= 0 || N <= 0 || N >= (1l << 31)) return -2;
    hipLaunchKernelGGL(sample_edges_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, verts, edges, edge_ids, start, length, E, total, N, samples, edge_index,
                       edge_t);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---- sample_surface (surface_sampling.py:24-35) on a defined random stream: Philox4x32-10 (philox_device.h), key (seed_lo, seed_hi),
// counter (i, 0, 0, 0) for sample i; a word x becomes (x >> 8) * 2^-24 in [0, 1).  Word 0 picks the face, words 1 and 2 are (u, v).
__global__ __launch_bounds__(256) void sample_surface_kernel(const float* __restrict__ verts, const int* __restrict__ faces, const float* __restrict__ cum, int F, long N,
                                                             unsigned seed_lo, unsigned seed_hi, float* __restrict__ samples, int* __restrict__ face_index,
                                                             float* __restrict__ uvw) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    unsigned r[4];
    philox4x32_10((unsigned)i, 0u, 0u, 0u, seed_lo, seed_hi, r);
    const float sc = 1.0f / 16777216.0f;
    const float pick = ((float)(r[0] >> 8) * sc) * cum[F - 1];
    int lo = 0, hi = F - 1;                 // searchsorted(cum, pick), lower bound, clamped to F - 1
    while (lo < hi) {
        const int mid = lo + (hi - lo) / 2;
        if (cum[mid] < pick) lo = mid + 1; else hi = mid;
    }
    float u = (float)(r[1] >> 8) * sc, v = (float)(r[2] >> 8) * sc;
    if (u + v > 1.0f) { u -= 1.0f; v -= 1.0f; }
    u = fabsf(u); v = fabsf(v);
    const float w = 1.0f - (u + v);
    const int a = faces[3 * (long)lo], b = faces[3 * (long)lo + 1], c = faces[3 * (long)lo + 2];
#pragma unroll
    for (int d = 0; d < 3; ++d) samples[3 * i + d] = (verts[3 * (long)a + d] * u + verts[3 * (long)b + d] * v) + verts[3 * (long)c + d] * w;
    if (face_index) face_index[i] = lo;
    if (uvw) { uvw[3 * i] = u; uvw[3 * i + 1] = v; uvw[3 * i + 2] = w; }
}

extern "C" int utx_launch_sample_surface(const float* verts, const int* faces, const float* cum, int F, long N, unsigned long long seed, float* samples, int* face_index,
                                         float* uvw, hipStream_t stream) {
    if (F <= 0 || N <= 0 || N >= (1l << 31)) return -2;
    hipLaunchKernelGGL(sample_surface_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, verts, faces, cum, F, N, (unsigned)(seed & 0xffffffffull),
                       (unsigned)(seed >> 32), samples, face_index, uvw);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---- sample_spatial / sample_near_surface (spatial_sampling.py:11-37, :40-91): the random offsets, on the defined stream of sample_surface with another stream id:
// counter (i, stream_id, 0, 0), stream_id 1 for sample_spatial's points and 2 for the near-surface deltas (0 is sample_surface's); words 0..2 -> r in [0, 1)^3.
//   base == null: out = r                                  (sample_spatial: torch.rand((N, 3)) -- the unit cube, whatever the mesh's box is)
//   else:  n = (vn[f0] * u + vn[f1] * v) + vn[f2] * w       (the interpolated vertex normal, not renormalised)
//          out = base + (threshold * (r * 2 - 1)) * n       (spatial_sampling.py:87-89, in the reference's order)
// uniforms (optional, [N][3]): read instead of the Philox words -- for tests that hand the kernel a fixture's recorded draws.
__global__ __launch_bounds__(256) void sample_offsets_kernel(const float* __restrict__ base, const int* __restrict__ faces, int F, const int* __restrict__ face_index,
                                                             const float* __restrict__ uvw, const float* __restrict__ vnormal, const float* __restrict__ uniforms, long N,
                                                             unsigned seed_lo, unsigned seed_hi, unsigned stream_id, float threshold, float* __restrict__ out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float r[3];
    if (uniforms) { r[0] = uniforms[3 * i]; r[1] = uniforms[3 * i + 1]; r[2] = uniforms[3 * i + 2]; }
    else {
        unsigned x[4];
        philox4x32_10((unsigned)i, stream_id, 0u, 0u, seed_lo, seed_hi, x);
        const float sc = 1.0f / 16777216.0f;
#pragma unroll
        for (int d = 0; d < 3; ++d) r[d] = (float)(x[d] >> 8) * sc;
    }
    if (!base) {
#pragma unroll
        for (int d = 0; d < 3; ++d) out[3 * i + d] = r[d];
        return;
    }
    const int f = face_index[i];
    if (f < 0 || f >= F) {      // no face, no normal: the sample stays where it is
#pragma unroll
        for (int d = 0; d < 3; ++d) out[3 * i + d] = base[3 * i + d];
        return;
    }
    const int a = faces[3 * (long)f], b = faces[3 * (long)f + 1], c = faces[3 * (long)f + 2];
    const float u = uvw[3 * i], v = uvw[3 * i + 1], w = uvw[3 * i + 2];
    float n[3];
    sd_interp<3>(vnormal + 3 * (long)a, vnormal + 3 * (long)b, vnormal + 3 * (long)c, u, v, w, n);
#pragma unroll
    for (int d = 0; d < 3; ++d) out[3 * i + d] = base[3 * i + d] + (threshold * (r[d] * 2.0f - 1.0f)) * n[d];
}

extern "C" int utx_launch_sample_offsets(const float* base, const int* faces, int F, const int* face_index, const float* uvw, const float* vnormal, const float* uniforms,
                                         long N, unsigned long long seed, int stream_id, float threshold, float* out, hipStream_t stream) {
    if (N < 0 || N >= (1l << 31) || stream_id < 1) return -2;
    if (N == 0) return 0;
    if (!out || (base && (!faces || F <= 0 || !face_index || !uvw || !vnormal))) return -2;
    hipLaunchKernelGGL(sample_offsets_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, base, faces, F, face_index, uvw, vnormal, uniforms, N,
                       (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), (unsigned)stream_id, threshold, out);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---- PBRMesh.__call__ (mesh/structure_v2.py:105-135): up to four attributes at N surface samples (face_index, uvw) in one launch.  An attribute is
//   a constant [C]                          -> copied;
//   a per-vertex array [V][C]               -> (attr[f0] * u + attr[f1] * v) + attr[f2] * w            (torch's sum over the three corners);
//   a texture [H][W][C], C <= 4             -> uv = (uvs_2d[g0] * u + uvs_2d[g1] * v) + uvs_2d[g2] * w with g = faces_2d[f], then grid_sample as the reference calls
//                                              it: THE UV ITSELF IS THE GRID COORDINATE (no map of [0, 1] to [-1, 1]), bilinear, align_corners=False,
//                                              padding_mode='reflection'.
// The interpolations are sd_interp's and the lookup is grid_reflect_taps / grid_tap / grid_blend of shade_device.h; oracle/sampling_ref.py restates them.
struct SampleAttr { const float* src; float* out; int kind, C, H, W; };
struct SampleAttrs { SampleAttr a[UTX_SAMPLE_ATTRS_MAX]; int n; };
__global__ __launch_bounds__(256) void sample_attrs_kernel(const int* __restrict__ faces, const int* __restrict__ faces_2d, const float* __restrict__ uvs_2d, int F,
                                                           const int* __restrict__ face_index, const float* __restrict__ uvw, long N, SampleAttrs P) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    const int f = face_index[i];
    const bool ok = f >= 0 && f < F;
    const float u = uvw[3 * i], v = uvw[3 * i + 1], w = uvw[3 * i + 2];
    float g[2] = {0.f, 0.f};
    if (ok && faces_2d && uvs_2d) {      // the launcher admits the two only together, and a texture only with both
        const long g0 = faces_2d[3 * (long)f], g1 = faces_2d[3 * (long)f + 1], g2 = faces_2d[3 * (long)f + 2];
        sd_interp<2>(uvs_2d + 2 * g0, uvs_2d + 2 * g1, uvs_2d + 2 * g2, u, v, w, g);
    }
    for (int k = 0; k < P.n; ++k) {
        const SampleAttr A = P.a[k];
        float* o = A.out + i * A.C;
        if (A.kind == 0) {
            for (int c = 0; c < A.C; ++c) o[c] = A.src[c];
        } else if (!ok) {      // a sample with no face: zeros
            for (int c = 0; c < A.C; ++c) o[c] = 0.f;
        } else if (A.kind == 1) {
            const long a0 = faces[3 * (long)f], a1 = faces[3 * (long)f + 1], a2 = faces[3 * (long)f + 2];
            for (int c = 0; c < A.C; ++c) o[c] = sd_interp1(A.src[a0 * A.C + c], A.src[a1 * A.C + c], A.src[a2 * A.C + c], u, v, w);
        } else {
            long t[4]; float tw[4];
            grid_reflect_taps(A.H, A.W, g[0], g[1], t, tw);
            for (int c = 0; c < A.C; ++c) {
                const float* ch = A.src + c;
                o[c] = grid_blend(grid_tap(ch, A.C, t[0]), grid_tap(ch, A.C, t[1]), grid_tap(ch, A.C, t[2]), grid_tap(ch, A.C, t[3]), tw);
            }
        }
    }
}

extern "C" int utx_launch_sample_attrs(const int* faces, const int* faces_2d, const float* uvs_2d, int F, const int* face_index, const float* uvw, long N, int n_attr,
                                       const float* const* src_host, const int* dims_host, float* const* out_host, hipStream_t stream) {
    if (N < 0 || N >= (1l << 31) || F <= 0 || n_attr < 1 || n_attr > UTX_SAMPLE_ATTRS_MAX || !src_host || !dims_host || !out_host) return -2;
    if ((faces_2d == nullptr) != (uvs_2d == nullptr)) return -2;      // the uv table and its index go together
    SampleAttrs P;
    P.n = n_attr;
    for (int k = 0; k < n_attr; ++k) {
        SampleAttr& A = P.a[k];
        A.src = src_host[k]; A.out = out_host[k];
        A.kind = dims_host[4 * k]; A.C = dims_host[4 * k + 1]; A.H = dims_host[4 * k + 2]; A.W = dims_host[4 * k + 3];
        if (!A.src || (!A.out && N > 0) || A.kind < 0 || A.kind > 2 || A.C < 1 || A.C > UTX_SAMPLE_ATTR_CHANNELS_MAX) return -2;
        if (A.kind == 1 && !faces) return -2;
        if (A.kind == 2 && (A.C > 4 || A.H < 1 || A.W < 1 || !faces_2d || !uvs_2d)) return -2;
    }
    if (N == 0) return 0;
    if (!face_index || !uvw) return -2;
    hipLaunchKernelGGL(sample_attrs_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, faces, faces_2d, uvs_2d, F, face_index, uvw, N, P);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

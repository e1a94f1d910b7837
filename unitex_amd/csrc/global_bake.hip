// Scattered-sample UV bake (NVDiffRendererBase.global_inverse_rendering of the reference, render/nvdiffrast/renderer_base.py:562-743): fp32, wave64,
// plain C++.
//   utx_view_samples      the per-pixel sample pass (:624-654): every pixel of every view as a sample at its own UV, with its mask, in one launch
//   utx_knn_inpaint_step  one Jacobi sweep of the surface-space propagation (:702-722) over the M covered texels, on the neighbour lists of utx_knn
// Built with -ffp-contract=off: every product and sum below is rounded on its own, in the order written, which is the order the restatement
// (tests/support/global_bake_ref.py) and the counted bounds assume.
#include "common.h"
#include "kernels.h"
#include "shade_device.h"
#include <cfloat>

// ---- the sample pass
// One thread per pixel of rast [B][H][W][4].  A covered pixel (triangle id + 1 > 0) on triangle (i0, i1, i2) with the raster's weights (u, v, w):
//   tex_to_pos     = interp of v_uv [V][2] (the vertex UVs in [-1, 1])
//   tex_to_pos_cam = interp of (normalize(v_pos_cam[b][i]), v_nrm_cam[b][i]): the vertices' camera-space positions are normalised PER VERTEX
//                    (F.normalize, sd_normalize3) and then interpolated; v_nrm_cam comes normalised (utx_camera_normals)
// an uncovered pixel holds zeros (dr.interpolate).  mask = covered
//   && (exclude_boundary: the four neighbours covered, wrapping round the image edge as torch.roll does)
//   && (use_normal: tex_to_pos_cam[5] > cos_normal) && (use_ray: dot(tex_to_pos_cam[0:3], tex_to_pos_cam[3:6]) > cos_ray) && (image_mask: non-zero)
struct ViewSamplesParams {
    const float4* rast; const int* tri; const float* v_uv; const float* v_pos_cam; const float* v_nrm_cam; const unsigned char* image_mask;
    float2* tex_to_pos; float* tex_to_pos_cam; unsigned char* mask;
    long F, V, total;
    int H, W, exclude_boundary, use_normal, use_ray;
    float cos_normal, cos_ray;
};

__global__ __launch_bounds__(256) void view_samples_kernel(const ViewSamplesParams p) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.total) return;
    const long hw = (long)p.H * p.W;
    const long b = i / hw, pix = i % hw;
    const int y = (int)(pix / p.W), x = (int)(pix % p.W);
    const float4 r = p.rast[i];
    const int id = (int)r.w - 1;
    const bool covered = r.w > 0.0f && id >= 0 && id < p.F;
    float uv[2] = {0.0f, 0.0f}, cam[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (covered) {
        const long i0 = p.tri[3 * (long)id + 0], i1 = p.tri[3 * (long)id + 1], i2 = p.tri[3 * (long)id + 2];
        const float u = r.x, v = r.y, w = sd_bary_w(u, v);
        sd_interp<2>(p.v_uv + 2 * i0, p.v_uv + 2 * i1, p.v_uv + 2 * i2, u, v, w, uv);
        const float* pc = p.v_pos_cam + 3 * b * p.V;
        float d0[3], d1[3], d2[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) { d0[c] = pc[3 * i0 + c]; d1[c] = pc[3 * i1 + c]; d2[c] = pc[3 * i2 + c]; }
        sd_normalize3(d0); sd_normalize3(d1); sd_normalize3(d2);
        sd_interp<3>(d0, d1, d2, u, v, w, cam);
        const float* nc = p.v_nrm_cam + 3 * b * p.V;
        sd_interp<3>(nc + 3 * i0, nc + 3 * i1, nc + 3 * i2, u, v, w, cam + 3);
    }
    bool m = covered;
    if (m && p.exclude_boundary) {
        const float4* rb = p.rast + b * hw;
        const int yu = y == 0 ? p.H - 1 : y - 1, yd = y == p.H - 1 ? 0 : y + 1, xl = x == 0 ? p.W - 1 : x - 1, xr = x == p.W - 1 ? 0 : x + 1;
        m = rb[(long)yu * p.W + x].w > 0.0f && rb[(long)yd * p.W + x].w > 0.0f && rb[(long)y * p.W + xl].w > 0.0f && rb[(long)y * p.W + xr].w > 0.0f;
    }
    if (m && p.use_normal) m = cam[5] > p.cos_normal;
    if (m && p.use_ray) m = sd_dot3(cam, cam + 3) > p.cos_ray;
    if (m && p.image_mask) m = p.image_mask[i] != 0;
    p.tex_to_pos[i] = make_float2(uv[0], uv[1]);
#pragma unroll
    for (int c = 0; c < 6; ++c) p.tex_to_pos_cam[6 * i + c] = cam[c];
    p.mask[i] = (unsigned char)m;
}

// arguments checked by utx_view_samples (capi.cpp).  B * H * W == 0 launches nothing.
extern "C" int utx_launch_view_samples(const float* rast, const int* faces, int F, const float* v_uv, const float* v_pos_cam, const float* v_nrm_cam, int V, int B,
                                       int H, int W, int exclude_boundary, int use_normal, float cos_normal, int use_ray, float cos_ray,
                                       const unsigned char* image_mask, float* tex_to_pos, float* tex_to_pos_cam, unsigned char* mask, hipStream_t stream) {
    ViewSamplesParams p;
    p.rast = (const float4*)rast; p.tri = faces; p.v_uv = v_uv; p.v_pos_cam = v_pos_cam; p.v_nrm_cam = v_nrm_cam; p.image_mask = image_mask;
    p.tex_to_pos = (float2*)tex_to_pos; p.tex_to_pos_cam = tex_to_pos_cam; p.mask = mask;
    p.F = F; p.V = V; p.total = (long)B * H * W;
    p.H = H; p.W = W; p.exclude_boundary = exclude_boundary; p.use_normal = use_normal; p.use_ray = use_ray;
    p.cos_normal = cos_normal; p.cos_ray = cos_ray;
    if (p.total == 0) return 0;
    hipLaunchKernelGGL(view_samples_kernel, dim3((unsigned)((p.total + 255) / 256)), dim3(256), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---- the propagation step
// One thread per covered texel i of M; idx / d2 [M][k]: its k nearest covered texels in 3-D and their squared distances (utx_knn on the set itself, so
// entry 0 is normally i at distance 0); nrm [M][3]; col [M][C]; pend [M] (non-zero: no colour yet).  Reads the *_in pair, writes every row of the *_out pair.
// A pending texel whose list holds fewer than k - 1 pending entries (itself included when the list holds it) is filled:
//   r_j   = nan_to_num(1 / sqrt(d2_j)): +inf (the self distance 0) becomes FLT_MAX, a NaN 0
//   s_j   = r_j / max(sum_j |r_j|, 1e-12)            F.normalize(p=1); the sum runs in list order
//   c_j   = dot(n_j, n_i) / max(|n_j| |n_i|, 1e-8)   cosine_similarity
//   w_j   = s_j c_j,  m_j = 1 for a known neighbour, 0 for a pending one
//   col_i = sum_j (m_j w_j) col_j / sum_j (m_j w_j)  both sums in list order
// and becomes known.  Nothing is guarded: a second zero distance makes the L1 sum overflow to +inf, every s_j is 0 and col_i is 0 / 0 = NaN, which later
// fills read as a colour (the host's closing nan_to_num removes it).  An entry outside [0, M) (utx_knn's -1 when fewer than k texels exist) is not read:
// it counts as known with weight 0.  The counter takes the texels filled by this launch, one ballot and one atomic per wave.
#define GB_CMAX 16
// nan_to_num(1 / sqrt(d2), nan=0): +-inf become +-FLT_MAX
__device__ __forceinline__ float gb_recip(float d2) {
    const float r = 1.0f / sqrtf(d2);
    return r != r ? 0.0f : fminf(fmaxf(r, -FLT_MAX), FLT_MAX);
}
__global__ __launch_bounds__(256) void knn_inpaint_step_kernel(const int* idx, const float* d2, const float* nrm, const float* col_in,
                                                               const unsigned char* pend_in, long M, int k, int C, float* col_out,
                                                               unsigned char* pend_out, int* counter) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    bool filled = false;
    if (i < M) {
        const int* nb = idx + i * k;
        bool pending = pend_in[i] != 0;
        if (pending) {
            int n_pending = 0;
            for (int j = 0; j < k; ++j) {
                const int q = nb[j];
                if (q >= 0 && q < M && pend_in[q] != 0) ++n_pending;
            }
            filled = n_pending < k - 1;
        }
        if (filled) {
            float l1 = 0.0f;
            for (int j = 0; j < k; ++j) {
                const int q = nb[j];
                if (q >= 0 && q < M) l1 = l1 + fabsf(gb_recip(d2[i * k + j]));
            }
            const float denom = fmaxf(l1, 1e-12f);
            const float ni[3] = {nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]};
            const float li = sd_length3(ni);
            float acc[GB_CMAX];
#pragma unroll
            for (int c = 0; c < GB_CMAX; ++c) acc[c] = 0.0f;
            float wsum = 0.0f;
            for (int j = 0; j < k; ++j) {
                const int q = nb[j];
                if (q < 0 || q >= M) continue;
                const float nj[3] = {nrm[3 * (long)q], nrm[3 * (long)q + 1], nrm[3 * (long)q + 2]};
                const float cj = sd_dot3(nj, ni) / fmaxf(sd_length3(nj) * li, 1e-8f);
                const float wj = (gb_recip(d2[i * k + j]) / denom) * cj;      // recomputed, not kept: a per-thread array indexed by j would live in scratch
                const float mw = pend_in[q] != 0 ? wj * 0.0f : wj;
                wsum = wsum + mw;
#pragma unroll
                for (int c = 0; c < GB_CMAX; ++c)
                    if (c < C) acc[c] = acc[c] + mw * col_in[(long)q * C + c];
            }
#pragma unroll
            for (int c = 0; c < GB_CMAX; ++c)
                if (c < C) col_out[i * C + c] = acc[c] / wsum;
            pending = false;
        } else {
            for (int c = 0; c < C; ++c) col_out[i * C + c] = col_in[i * C + c];
        }
        pend_out[i] = (unsigned char)pending;
    }
    wave_count_add(counter, filled);
}

// arguments checked by utx_knn_inpaint_step (capi.cpp); zeroes *counter, then one launch.  M == 0 launches nothing (and leaves the counter alone).
extern "C" int utx_launch_knn_inpaint_step(const int* idx, const float* d2, const float* nrm, const float* col_in, const unsigned char* pend_in, long M, int k,
                                           int C, float* col_out, unsigned char* pend_out, int* counter, hipStream_t stream) {
    if (M == 0) return 0;
    if (hipMemsetAsync(counter, 0, sizeof(int), stream) != hipSuccess) return -4;
    hipLaunchKernelGGL(knn_inpaint_step_kernel, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, stream, idx, d2, nrm, col_in, pend_in, M, k, C, col_out,
                       pend_out, counter);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// Blended multi-view UV texture bake (texture/reprojection/mesh_remapping.py of the reference, the atlas half): fp32, wave64, plain C++.
//   utx_uv_bake           project_uv_texture's accumulation over the views (:479-505), one thread per atlas texel, views in index order, optionally
//                         followed by the overlay / blending / inpainting-mask epilogue of remapping_uv_texture (:205-228) in the same launch
//   utx_uv_dilation_step  one _uv_dilation_v2 step of uv_dilation (texture/reprojection/uv_dilation.py:33-50, :80-92), or its closing clamp
// Built with -ffp-contract=off: every product and sum below is rounded on its own, in the order written, which is the order the restatement
// (oracle/uv_bake_ref.py) and the counted bounds assume.
#include "common.h"
#include "kernels.h"
#include "shade_device.h"

// ---- accumulation
// Per (view b, texel): what utx_uv_project computes for a [B][R][R][6] map = (rgba of the view's image, cos term, edge alpha) with the bilinear
// lookup and no background -- vis, uv, cov, uv_alpha and the six samples, from the same device functions (sd_uv_view, sd_view_coverage, grid_taps /
// grid_tap / grid_blend) -- and then, in the reference's written order (:489, :503),
//   a   = use_alpha ? uv_alpha : 1
//   w   = ((weights[b] * ((c * c) * (c * c))) * a) * (1 - e)
//   col = (a * rgba + (1 - a) * map_Kd) * w
// acc = sum_b col, wacc = sum_b w.  The six channels are never stored: the image stays planar [B][4][R][R] (a tap of channel c is one float of plane c),
// the weight maps stay [B][R][R][2].  A texel whose uv lands off the view's coverage takes texel [0][0] of the view's six channels (bg_kind NONE of
// utx_uv_project), which counts only with use_alpha = 0.
struct UvBakeParams {
    const float4* rast2d; const int* tri; const unsigned char* face_mask; const float* v_ndc; const float* images; const float2* wmap;
    const float* rast_view; const float4* map_Kd; const float* weights; float4* acc; float* wacc; float4* blended; unsigned char* inpaint;
    long F, V, total;
    int B, R, use_alpha, blending;
    float overlay_conf, blending_conf, inpainting_conf;
};

template <bool EPILOGUE>
__global__ __launch_bounds__(256) void uv_bake_kernel(const UvBakeParams p) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.total) return;
    const float4 r = p.rast2d[i];
    const float4 kd4 = p.map_Kd[i];
    const float kd[4] = {kd4.x, kd4.y, kd4.z, kd4.w};
    float acc[4] = {0.f, 0.f, 0.f, 0.f}, wa = 0.f;
    const long plane = (long)p.R * p.R;
    for (int b = 0; b < p.B; ++b) {
        const SdUvView s = sd_uv_view(r, p.tri, p.F, p.face_mask + b * p.F, p.v_ndc + 2 * p.V * b);
        const bool cov = sd_view_coverage(p.rast_view + 4 * plane * b, p.R, p.R, s.g[0], s.g[1]);
        const float* img = p.images + 4 * plane * b;
        const float2* wm = p.wmap + plane * b;
        float rgba[4], c, e;
        if (!cov) {
#pragma unroll
            for (int k = 0; k < 4; ++k) rgba[k] = img[plane * k];
            const float2 q = wm[0];
            c = q.x; e = q.y;
        } else {
            long o[4]; float gw[4];
            grid_taps(p.R, p.R, s.g[0], s.g[1], o, gw);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float* pl = img + plane * k;
                rgba[k] = grid_blend(grid_tap(pl, 1, o[0]), grid_tap(pl, 1, o[1]), grid_tap(pl, 1, o[2]), grid_tap(pl, 1, o[3]), gw);
            }
            float2 q[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = o[k] < 0 ? make_float2(0.f, 0.f) : wm[o[k]];
            c = grid_blend(q[0].x, q[1].x, q[2].x, q[3].x, gw);
            e = grid_blend(q[0].y, q[1].y, q[2].y, q[3].y, gw);
        }
        const float a = p.use_alpha ? ((s.vis && cov) ? 1.0f : 0.0f) : 1.0f;
        const float ia = 1.0f - a;
        const float w = ((p.weights[b] * ((c * c) * (c * c))) * a) * (1.0f - e);
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = acc[k] + (a * rgba[k] + ia * kd[k]) * w;
        wa = wa + w;
    }
    if (p.acc) p.acc[i] = make_float4(acc[0], acc[1], acc[2], acc[3]);
    p.wacc[i] = wa;
    if constexpr (EPILOGUE) {
        sd_bake_epilogue<4>(acc, wa, kd, p.overlay_conf, p.blending, p.blending_conf);
        p.blended[i] = make_float4(acc[0], acc[1], acc[2], acc[3]);
        p.inpaint[i] = (unsigned char)(wa <= p.inpainting_conf && r.w > 0.0f);
    }
}
// arguments checked by utx_uv_bake (capi.cpp); blended == nullptr: no epilogue.  Th * Tw == 0 launches nothing.
extern "C" int utx_launch_uv_bake(const float* rast2d, const int* faces, int F, const unsigned char* face_mask, const float* v_ndc, int V, int B, int Th, int Tw,
                                  const float* images, const float* wmap, const float* rast_view, int R, const float* map_Kd, const float* weights, int use_alpha,
                                  float* acc, float* wacc, float overlay_conf, int blending, float blending_conf, float inpainting_conf, float* blended,
                                  unsigned char* inpaint, hipStream_t stream) {
    UvBakeParams p;
    p.total = (long)Th * Tw;
    if (p.total == 0) return 0;
    p.rast2d = (const float4*)rast2d; p.tri = faces; p.face_mask = face_mask; p.v_ndc = v_ndc; p.images = images; p.wmap = (const float2*)wmap;
    p.rast_view = rast_view; p.map_Kd = (const float4*)map_Kd; p.weights = weights; p.acc = (float4*)acc; p.wacc = wacc; p.blended = (float4*)blended;
    p.inpaint = inpaint; p.F = F; p.V = V; p.B = B; p.R = R; p.use_alpha = use_alpha; p.blending = blending;
    p.overlay_conf = overlay_conf; p.blending_conf = blending_conf; p.inpainting_conf = inpainting_conf;
    const unsigned nb = (unsigned)((p.total + 255) / 256);
    if (blended) hipLaunchKernelGGL(uv_bake_kernel<true>, dim3(nb), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(uv_bake_kernel<false>, dim3(nb), dim3(256), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---- texel-space dilation
// One thread per texel of [H][W][C].  A tap reads as colour * mask (valid: the colour, invalid: colour * 0, which is what the reference's
// `map_Kd * _map_mask` leaves there, a NaN included); a tap outside the image is not visited and the divisor stays 9 (avg_pool2d with its default
// count_include_pad).  S: the nine taps summed row by row, M: the same of the mask.  Where M / 9 != mask the texel becomes (S / 9) / (M / 9), elsewhere it
// keeps its colour -- an invalid texel with no valid neighbour keeps its ORIGINAL colour here (the reference carries 0 and puts the original back in
// its last line, uv_dilation.py:49).  mask_out = M > 0; the counter takes the texels with mask_out = 0, one ballot and one atomic per wave.
__global__ __launch_bounds__(256) void uv_dilation_step_kernel(const float* col_in, const unsigned char* mask_in, int H, int W, int C, float* col_out,
                                                               unsigned char* mask_out, int* counter) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long total = (long)H * W;
    bool open = false;
    if (i < total) {
        const int x = (int)(i % W), y = (int)(i / W);
        long o[9];
        bool m[9];
        float M = 0.0f;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            const int xx = x + k % 3 - 1, yy = y + k / 3 - 1;
            o[k] = (xx < 0 || xx >= W || yy < 0 || yy >= H) ? -1 : (long)yy * W + xx;
            m[k] = o[k] >= 0 && mask_in[o[k]] != 0;
            if (o[k] >= 0) M = M + (m[k] ? 1.0f : 0.0f);
        }
        const float me = m[4] ? 1.0f : 0.0f;
        const float md = M / 9.0f;
        const bool boundary = (md - me) != 0.0f;
        for (int c = 0; c < C; ++c) {
            float v = col_in[i * C + c];
            if (boundary) {
                float S = 0.0f;
#pragma unroll
                for (int k = 0; k < 9; ++k) {
                    if (o[k] >= 0) {
                        const float t = col_in[o[k] * C + c];
                        S = S + (m[k] ? t : t * 0.0f);
                    }
                }
                v = (S / 9.0f) / md;
            }
            col_out[i * C + c] = v;
        }
        mask_out[i] = (unsigned char)(M > 0.0f);
        open = !(M > 0.0f);
    }
    wave_count_add(counter, open);
}
// uv_dilation's last line once the loop has ended: the whole map clamped to [0, 1] (torch.clamp: min(max(x, 0), 1), a NaN stays)
__global__ __launch_bounds__(256) void uv_dilation_clamp_kernel(const float* col_in, long n, float* col_out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = col_in[i];
    col_out[i] = v != v ? v : fminf(fmaxf(v, 0.0f), 1.0f);
}
// arguments checked by utx_uv_dilation_step (capi.cpp).  UTX_UVD_STEP: zeroes *counter, then one launch; UTX_UVD_CLAMP: one launch, mask and counter unread.
// H * W == 0 launches nothing.
extern "C" int utx_launch_uv_dilation_step(const float* col_in, const unsigned char* mask_in, int H, int W, int C, int mode, float* col_out, unsigned char* mask_out,
                                           int* counter, hipStream_t stream) {
    const long total = (long)H * W;
    if (total == 0) return 0;
    if (mode == UTX_UVD_CLAMP) {
        const long n = total * C;
        hipLaunchKernelGGL(uv_dilation_clamp_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, col_in, n, col_out);
        return hipGetLastError() == hipSuccess ? 0 : -4;
    }
    if (hipMemsetAsync(counter, 0, sizeof(int), stream) != hipSuccess) return -4;
    hipLaunchKernelGGL(uv_dilation_step_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, col_in, mask_in, H, W, C, col_out, mask_out, counter);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

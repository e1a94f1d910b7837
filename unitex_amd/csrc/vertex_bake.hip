// Vertex-colour bake from views (texture/reprojection/mesh_remapping.py of the reference): fp32, wave64, plain C++.
//   utx_view_weight_maps     the two per-pixel weight channels of project_vertex_color (:544-555): (cos term, dilated edge alpha)
//   utx_vertex_project       project_vertex_color's per-view loop (:559-594), one thread per vertex, views in index order, optionally followed by the
//                            overlay / blending / inpainting-mask epilogue of remapping_vertex_color (:326-343) in the same launch
//   utx_vertex_inpaint_step  one Jacobi step of inpainting_vertex_color (:617-622) on a CSR vertex adjacency
// Built with -ffp-contract=off: every product and sum below is rounded on its own, in the order written, which is the order the restatement
// (oracle/vertex_bake_ref.py) and the counted bounds assume.
#include "common.h"
#include "kernels.h"
#include "shade_device.h"

// ---- weight maps
// float32(pi / 2): what `torch.arccos(x) - torch.pi / 2` and `/ (torch.pi / 2)` use on a float32 tensor (the Python double is cast to the tensor's type)
#define VB_HALF_PI 1.57079637050628662109375f
// float32(math.radians(10) / (math.pi / 2)) = float32(1 / 9): the comparison of a float32 tensor with a Python double is made in float32
#define VB_GRAD_THR 0.111111111938953399658203125f

__device__ __forceinline__ float vb_clampf(float x, float lo, float hi) { return fminf(fmaxf(x, lo), hi); }
// ((arccos(clamp(cos, -1, 0)) - pi/2) / (pi/2)).clamp(0, 1)
__device__ __forceinline__ float vb_arccos01(float c) { return vb_clampf((acosf(vb_clampf(c, -1.0f, 0.0f)) - VB_HALF_PI) / VB_HALF_PI, 0.0f, 1.0f); }

// one thread per pixel of [B][H][W]: channel 0 of out and the undilated alpha, which goes to channel 1 (r == 0) or to the scratch `alpha` (r > 0).
// torch.gradient's stencil: (f[i+1] - f[i-1]) / 2 inside, f[1] - f[0] and f[n-1] - f[n-2] at the borders (H, W >= 2).  The four neighbours' arccos
// are recomputed here (5 acosf per pixel): no second full-size float scratch, and the kernel stays bound by its one read and one write per pixel.
__global__ __launch_bounds__(256) void vb_weight_alpha_kernel(const float* cosn, const float* cam_nrm, int B, int H, int W, float2* out, unsigned char* alpha,
                                                              float* arccos_out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long npix = (long)B * H * W;
    if (i >= npix) return;
    const int x = (int)(i % W), y = (int)((i / W) % H);
    const long xm = x > 0 ? i - 1 : i, xp = x < W - 1 ? i + 1 : i;
    const long ym = y > 0 ? i - W : i, yp = y < H - 1 ? i + W : i;
    const float sx = (x > 0 && x < W - 1) ? 2.0f : 1.0f, sy = (y > 0 && y < H - 1) ? 2.0f : 1.0f;
    const float c = cosn[i];
    const float dx = (vb_arccos01(cosn[xp]) - vb_arccos01(cosn[xm])) / sx;
    const float dy = (vb_arccos01(cosn[yp]) - vb_arccos01(cosn[ym])) / sy;
    const float a = sqrtf(dy * dy + dx * dx) > VB_GRAD_THR ? 1.0f : 0.0f;
    const float c0 = cam_nrm ? vb_clampf(cam_nrm[3 * i + 2], 0.0f, 1.0f) : vb_clampf(c, -1.0f, 0.0f);
    if (alpha) { alpha[i] = (unsigned char)(a != 0.0f); out[i].x = c0; }
    else out[i] = make_float2(c0, a);
    if (arccos_out) arccos_out[i] = vb_arccos01(c);
}
// the (2r + 1)^2 maximum of the 0 / 1 alpha, zero outside the image (max_pool2d(k, 1, k // 2) of a non-negative map), into channel 1
__global__ __launch_bounds__(256) void vb_weight_dilate_kernel(const unsigned char* alpha, int B, int H, int W, int r, float2* out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long npix = (long)B * H * W;
    if (i >= npix) return;
    const int x = (int)(i % W), y = (int)((i / W) % H);
    const int x0 = x - r < 0 ? 0 : x - r, x1 = x + r > W - 1 ? W - 1 : x + r;
    const int y0 = y - r < 0 ? 0 : y - r, y1 = y + r > H - 1 ? H - 1 : y + r;
    const unsigned char* base = alpha + (i - x - (long)y * W);
    bool hit = false;
    for (int yy = y0; yy <= y1 && !hit; ++yy)
        for (int xx = x0; xx <= x1 && !hit; ++xx) hit = base[(long)yy * W + xx] != 0;
    out[i].y = hit ? 1.0f : 0.0f;
}
// arguments checked by utx_view_weight_maps (capi.cpp); B * H * W == 0 launches nothing
extern "C" int utx_launch_view_weight_maps(const float* cosn, const float* cam_nrm, int B, int H, int W, int r, void* tmp, float* out, float* arccos_out,
                                           hipStream_t stream) {
    const long npix = (long)B * H * W;
    if (npix == 0) return 0;
    const unsigned nb = (unsigned)((npix + 255) / 256);
    unsigned char* alpha = r > 0 ? (unsigned char*)tmp : nullptr;
    hipLaunchKernelGGL(vb_weight_alpha_kernel, dim3(nb), dim3(256), 0, stream, cosn, cam_nrm, B, H, W, (float2*)out, alpha, arccos_out);
    if (r > 0) hipLaunchKernelGGL(vb_weight_dilate_kernel, dim3(nb), dim3(256), 0, stream, alpha, B, H, W, r, (float2*)out);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---- projection: the image through grid_sample's reflection lookup, the weight map through its zero-padding one (both of shade_device.h)
struct VbProjectParams {
    const float* v_pos; const unsigned char* visible; const float* xform; const float* proj; const float* images; const float2* wmap;
    const float* v_rgb; const float* weights; float* acc; float* wacc; float* blended; unsigned char* inpaint;
    int V, B, Hi, Wi, H, W, use_alpha, blending;
    float overlay_conf, blending_conf, inpainting_conf;
};
// row j of a row-major 4 x 4 applied to (x, y, z, w): the sum in index order, every product rounded (v_homo @ M^T of the reference)
__device__ __forceinline__ float vb_row4(const float* m, float x, float y, float z, float w) { return ((m[0] * x + m[1] * y) + m[2] * z) + m[3] * w; }

// EPILOGUE: also the overlay / blending / mask stage of remapping_vertex_color
template <bool EPILOGUE>
__global__ __launch_bounds__(256) void vb_vertex_project_kernel(const VbProjectParams p) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= p.V) return;
    const float px = p.v_pos[3 * (long)v], py = p.v_pos[3 * (long)v + 1], pz = p.v_pos[3 * (long)v + 2];
    const float rgb[3] = {p.v_rgb[3 * (long)v], p.v_rgb[3 * (long)v + 1], p.v_rgb[3 * (long)v + 2]};
    float acc[3] = {0.f, 0.f, 0.f}, wa = 0.f;
    const long plane = (long)p.Hi * p.Wi;
    for (int b = 0; b < p.B; ++b) {
        if (!p.visible[(long)b * p.V + v]) continue;
        const float* T = p.xform + 16 * b;
        const float* P = p.proj + 16 * b;
        const float hx = vb_row4(T, px, py, pz, 1.0f), hy = vb_row4(T + 4, px, py, pz, 1.0f), hz = vb_row4(T + 8, px, py, pz, 1.0f),
                    hw = vb_row4(T + 12, px, py, pz, 1.0f);
        const float cw = vb_row4(P + 12, hx, hy, hz, hw);
        const float nx = vb_row4(P, hx, hy, hz, hw) / cw, ny = vb_row4(P + 4, hx, hy, hz, hw) / cw;
        float c[3] = {rgb[0], rgb[1], rgb[2]}, w = 0.0f;
        if (nx > -1.0f && nx < 1.0f && ny > -1.0f && ny < 1.0f) {      // strictly inside; a NaN fails
            long o[4]; float gw[4];
            grid_reflect_taps(p.Hi, p.Wi, nx, ny, o, gw);
            const float* img = p.images + 4 * plane * b;
            float s[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const float* pl = img + plane * k;
                s[k] = grid_blend(grid_tap(pl, 1, o[0]), grid_tap(pl, 1, o[1]), grid_tap(pl, 1, o[2]), grid_tap(pl, 1, o[3]), gw);
            }
            grid_taps(p.H, p.W, nx, ny, o, gw);
            const float2* wm = p.wmap + (long)p.H * p.W * b;
            float2 q[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = o[k] < 0 ? make_float2(0.f, 0.f) : wm[o[k]];
            const float cs = grid_blend(q[0].x, q[1].x, q[2].x, q[3].x, gw), al = grid_blend(q[0].y, q[1].y, q[2].y, q[3].y, gw);
            const float a = p.use_alpha ? s[3] : 1.0f;
            const float ia = 1.0f - a;
#pragma unroll
            for (int k = 0; k < 3; ++k) c[k] = s[k] * a + rgb[k] * ia;
            const float cs2 = cs * cs;
            w = (p.weights[b] * (cs2 * cs2)) * (1.0f - al);
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[k] = acc[k] + w * c[k];
        wa = wa + w;
    }
    if (p.acc) { p.acc[3 * (long)v] = acc[0]; p.acc[3 * (long)v + 1] = acc[1]; p.acc[3 * (long)v + 2] = acc[2]; }
    p.wacc[v] = wa;
    if constexpr (EPILOGUE) {
        sd_bake_epilogue<3>(acc, wa, rgb, p.overlay_conf, p.blending, p.blending_conf);
        p.blended[3 * (long)v] = acc[0]; p.blended[3 * (long)v + 1] = acc[1]; p.blended[3 * (long)v + 2] = acc[2];
        p.inpaint[v] = (unsigned char)(wa <= p.inpainting_conf);
    }
}
// arguments checked by utx_vertex_project / utx_vertex_project_blend (capi.cpp); blended == nullptr: no epilogue.  V == 0 launches nothing.
extern "C" int utx_launch_vertex_project(const float* v_pos, int V, const unsigned char* visible, int B, const float* xform, const float* proj, const float* images,
                                         int Hi, int Wi, const float* wmap, int H, int W, const float* v_rgb, const float* weights, int use_alpha, float* acc,
                                         float* wacc, float overlay_conf, int blending, float blending_conf, float inpainting_conf, float* blended,
                                         unsigned char* inpaint, hipStream_t stream) {
    if (V == 0) return 0;
    VbProjectParams p;
    p.v_pos = v_pos; p.visible = visible; p.xform = xform; p.proj = proj; p.images = images; p.wmap = (const float2*)wmap; p.v_rgb = v_rgb;
    p.weights = weights; p.acc = acc; p.wacc = wacc; p.blended = blended; p.inpaint = inpaint;
    p.V = V; p.B = B; p.Hi = Hi; p.Wi = Wi; p.H = H; p.W = W; p.use_alpha = use_alpha; p.blending = blending;
    p.overlay_conf = overlay_conf; p.blending_conf = blending_conf; p.inpainting_conf = inpainting_conf;
    const unsigned nb = (unsigned)(((long)V + 255) / 256);
    if (blended) hipLaunchKernelGGL(vb_vertex_project_kernel<true>, dim3(nb), dim3(256), 0, stream, p);
    else hipLaunchKernelGGL(vb_vertex_project_kernel<false>, dim3(nb), dim3(256), 0, stream, p);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---- inpainting
// one thread per vertex of idx [n]: the reference's L[i, j] = deg[i] on both the colour sum and the mask sum (the factor is redundant and kept),
// neighbours in CSR order; reads (rgb_in, mask_in), writes row idx[k] of (rgb_out, mask_out) only, so the two buffer pairs must agree on every other
// row.  counter: the number of vertices of idx that are valid after this step, one atomic per wave.
__global__ __launch_bounds__(256) void vb_inpaint_step_kernel(const int* rowptr, const int* col, const int* idx, int n, const float* rgb_in,
                                                              const unsigned char* mask_in, float* rgb_out, unsigned char* mask_out, int* counter) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    bool valid = false;
    if (k < n) {
        const long v = idx[k];
        const int e0 = rowptr[v], e1 = rowptr[v + 1];
        const float deg = (float)(e1 - e0);
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, sm = 0.f;
        for (int e = e0; e < e1; ++e) {
            const long j = col[e];
            if (mask_in[j]) {
                s0 = s0 + rgb_in[3 * j]; s1 = s1 + rgb_in[3 * j + 1]; s2 = s2 + rgb_in[3 * j + 2];
                sm = sm + 1.0f;
            }
        }
        const float den = deg * sm;
        valid = den > 0.0f;
        if (valid) { rgb_out[3 * v] = (deg * s0) / den; rgb_out[3 * v + 1] = (deg * s1) / den; rgb_out[3 * v + 2] = (deg * s2) / den; }
        else { rgb_out[3 * v] = rgb_in[3 * v]; rgb_out[3 * v + 1] = rgb_in[3 * v + 1]; rgb_out[3 * v + 2] = rgb_in[3 * v + 2]; }
        mask_out[v] = (unsigned char)valid;
    }
    wave_count_add(counter, valid);
}
// arguments checked by utx_vertex_inpaint_step (capi.cpp); zeroes *counter, then one launch.  n == 0 launches nothing (and leaves the counter alone).
extern "C" int utx_launch_vertex_inpaint_step(const int* rowptr, const int* col, const int* idx, int n, const float* rgb_in, const unsigned char* mask_in,
                                              float* rgb_out, unsigned char* mask_out, int* counter, hipStream_t stream) {
    if (n == 0) return 0;
    if (hipMemsetAsync(counter, 0, sizeof(int), stream) != hipSuccess) return -4;
    hipLaunchKernelGGL(vb_inpaint_step_kernel, dim3((unsigned)(((long)n + 255) / 256)), dim3(256), 0, stream, rowptr, col, idx, n, rgb_in, mask_in, rgb_out,
                       mask_out, counter);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

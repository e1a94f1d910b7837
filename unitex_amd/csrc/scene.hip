// Environment renderer (gfx950): the per-pixel paths of the reference's NVDiffRendererScene (TextureTools/texturetools/render/nvdiffrast/renderer_scene.py):
// a camera batch looking into a cubemap and / or a lat-long panorama (perspective_rendering, :288-317), cubemap -> panorama (cubemap_to_latlong, :148-172)
// and the bake of M perspective views into one panorama (perspective_inverse_rendering_torch, :373-430).  All data fp32, wave64, one thread per pixel /
// texel, stream-ordered, no host synchronisation, no atomics: every sum has one fixed order, so results are run-to-run identical.
// These are latency- and bandwidth-bound gathers; what is reused is the direction: one ray feeds every requested output, one texel feeds all M views.
// Compiled with -ffp-contract=off: the lookups are the shared ones of cube_device.h (cube rule) and shade_device.h (sd_tex_taps / sd_bilerp: linear with
// wrap addressing in both axes, dr.texture's default boundary mode; grid_taps / grid_blend: grid_sample, bilinear, zero padding, align_corners=False).
#include <math.h>
#include "common.h"
#include "kernels.h"
#include "shade_device.h"
#include "cube_device.h"

#define SCENE_PI 3.14159265358979323846

// ---------------------------------------------------------------------------------------------------------------- camera ray of a pixel
// c2ws_to_ray_matrices(perspective=True) (camera/conversion.py:238-259) followed by F.normalize: the pixel centre in NDC, unprojected at depth 1 through
// the inverse of intr_to_proj's matrix (rows (2fx, 0, 2cx - 1, 0) and, flipped for nvdiffrast, (0, -2fy, -(2cy - 1), 0); w' = -z), written out:
//   p = ((nx + (2cx - 1)) / (2fx), ((2cy - 1) - ny) / (2fy), -1);  world = ((R0 p.x + R1 p.y) + R2 p.z) + t;  d = world - t;  d / max(|d|, 1e-12)
// c2w: [4][4] row-major, k: [3][3] normalised intrinsics
__device__ __forceinline__ void scene_ray(const float* c2w, const float* k, int H, int W, int x, int y, float d[3]) {
    const float nx = (((float)x + 0.5f) / (float)W) * 2.0f - 1.0f, ny = (((float)y + 0.5f) / (float)H) * 2.0f - 1.0f;
    const float px = (nx + (2.0f * k[2] - 1.0f)) / (2.0f * k[0]);
    const float py = ((2.0f * k[5] - 1.0f) - ny) / (2.0f * k[4]);
    const float pz = -1.0f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float t = c2w[4 * i + 3];
        d[i] = (((c2w[4 * i] * px + c2w[4 * i + 1] * py) + c2w[4 * i + 2] * pz) + t) - t;
    }
    sd_normalize3(d);
}

// (atan2(dx, -dz) / 2pi + 0.5, acos(clamp(dy)) / pi): the panorama coordinate of a direction (:309-311)
__device__ __forceinline__ void scene_dir_uv(const float d[3], float& u, float& v) {
    u = atan2f(d[0], -d[2]) / (float)(2.0 * SCENE_PI) + 0.5f;
    v = acosf(fminf(fmaxf(d[1], -1.0f), 1.0f)) / (float)SCENE_PI;
}

// linear lookup with wrap addressing in both axes of a [Hi][Wi][CH] panorama at (u, v): sd_tex3_wrap's taps and blend on CH channels
template <int CH>
__device__ __forceinline__ void scene_latlong_lookup(const float* lat, int Hi, int Wi, float u, float v, float o[CH]) {
    const SdTexTaps t = sd_tex_taps(Hi, Wi, u, v);
    const float *t00 = lat + CH * t.o00, *t01 = lat + CH * t.o01, *t10 = lat + CH * t.o10, *t11 = lat + CH * t.o11;
#pragma unroll
    for (int k = 0; k < CH; ++k) o[k] = sd_bilerp(t00[k], t01[k], t10[k], t11[k], t.fx, t.fy);
}

// ---------------------------------------------------------------------------------------------------------------- perspective_rendering
template <int CH>
__global__ __launch_bounds__(256) void scene_render_kernel(const float* c2ws, const float* intr, int intr_stride, int H, int W, long npix, const float* cube, int N,
                                                           const float* lat, int Hi, int Wi, float* rays_d, float* cube_attr, float* uv, float* lat_attr) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const long hw = (long)H * W;
    const int b = (int)(i / hw), y = (int)((i % hw) / W), x = (int)(i % W);
    float d[3];
    scene_ray(c2ws + 16 * (long)b, intr + (long)intr_stride * b, H, W, x, y, d);
    if (rays_d) { rays_d[3 * i] = d[0]; rays_d[3 * i + 1] = d[1]; rays_d[3 * i + 2] = d[2]; }
    if (cube_attr) {
        float o[CH];
        pbr_cube_lookup<CH>(cube, N, d[0], d[1], d[2], o);
#pragma unroll
        for (int k = 0; k < CH; ++k) cube_attr[CH * i + k] = o[k];
    }
    if (uv || lat_attr) {
        float u, v;
        scene_dir_uv(d, u, v);
        if (uv) { uv[2 * i] = u; uv[2 * i + 1] = v; }
        if (lat_attr) {
            float o[CH];
            scene_latlong_lookup<CH>(lat, Hi, Wi, u, v, o);
#pragma unroll
            for (int k = 0; k < CH; ++k) lat_attr[CH * i + k] = o[k];
        }
    }
}

extern "C" int utx_launch_scene_render(const float* c2ws, const float* intr, int intr_stride, int B, int H, int W, const float* cube, int N, const float* lat, int Hi,
                                       int Wi, int C, float* rays_d, float* cube_attr, float* uv, float* lat_attr, hipStream_t stream) {
    if (B <= 0 || H <= 0 || W <= 0 || (intr_stride != 0 && intr_stride != 9)) return -2;
    if (!rays_d && !cube_attr && !uv && !lat_attr) return -2;
    if (cube_attr && (!cube || N <= 0 || (N & 1) || N > 8192)) return -2;
    if (lat_attr && (!lat || Hi <= 0 || Wi <= 0)) return -2;
    if ((cube_attr || lat_attr) && (C < 1 || C > 4)) return -2;
    const long npix = (long)B * H * W;
    if (npix > 256L * 0x7fffffffL) return -2;
    const dim3 grid((unsigned)((npix + 255) / 256));
#define SCENE_RENDER(CH)                                                                                                                                    \
    hipLaunchKernelGGL(scene_render_kernel<CH>, grid, dim3(256), 0, stream, c2ws, intr, intr_stride, H, W, npix, cube, N, lat, Hi, Wi, rays_d, cube_attr, uv, \
                       lat_attr)
    switch ((cube_attr || lat_attr) ? C : 3) {
        case 1: SCENE_RENDER(1); break;
        case 2: SCENE_RENDER(2); break;
        case 3: SCENE_RENDER(3); break;
        default: SCENE_RENDER(4); break;
    }
#undef SCENE_RENDER
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---------------------------------------------------------------------------------------------------------------- the panorama's direction grid
// texel (x, y) of a [Ht][Wt] panorama: gx, gy = the texel-centre grid in (-1, 1), psi = gx pi, theta = gy pi / 2 + pi / 2,
// direction (sin theta sin psi, cos theta, -sin theta cos psi) (:159-170, :402-413).  Angles and direction in fp64, rounded once.
__device__ __forceinline__ void scene_texel_dir(int Ht, int Wt, int x, int y, float d[3]) {
    const double gx = 2.0 * ((x + 0.5) / Wt) - 1.0, gy = 2.0 * ((y + 0.5) / Ht) - 1.0;
    const double psi = gx * SCENE_PI, theta = gy * (SCENE_PI / 2.0) + SCENE_PI / 2.0;
    const double st = sin(theta);
    d[0] = (float)(st * sin(psi)); d[1] = (float)cos(theta); d[2] = (float)(-st * cos(psi));
}

// ---------------------------------------------------------------------------------------------------------------- cubemap_to_latlong
template <int CH>
__global__ __launch_bounds__(256) void cubemap_to_latlong_kernel(const float* cube, int N, int Ht, int Wt, float* out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)Ht * Wt) return;
    float d[3], o[CH];
    scene_texel_dir(Ht, Wt, (int)(i % Wt), (int)(i / Wt), d);
    pbr_cube_lookup<CH>(cube, N, d[0], d[1], d[2], o);
#pragma unroll
    for (int k = 0; k < CH; ++k) out[CH * i + k] = o[k];
}

extern "C" int utx_launch_cubemap_to_latlong(const float* cube, int N, int C, int Ht, int Wt, float* out, hipStream_t stream) {
    if (N <= 0 || (N & 1) || N > 8192 || C < 1 || C > 4 || Ht <= 0 || Wt <= 0) return -2;
    const dim3 grid((unsigned)(((long)Ht * Wt + 255) / 256));
    switch (C) {
        case 1: hipLaunchKernelGGL(cubemap_to_latlong_kernel<1>, grid, dim3(256), 0, stream, cube, N, Ht, Wt, out); break;
        case 2: hipLaunchKernelGGL(cubemap_to_latlong_kernel<2>, grid, dim3(256), 0, stream, cube, N, Ht, Wt, out); break;
        case 3: hipLaunchKernelGGL(cubemap_to_latlong_kernel<3>, grid, dim3(256), 0, stream, cube, N, Ht, Wt, out); break;
        default: hipLaunchKernelGGL(cubemap_to_latlong_kernel<4>, grid, dim3(256), 0, stream, cube, N, Ht, Wt, out); break;
    }
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---------------------------------------------------------------------------------------------------------------- perspective_inverse_rendering_torch
// One thread per panorama texel walks the M views in index order.  Per view (:414-428): the texel's unit direction, taken as the POINT (rd, 1) (the reference
// projects a point of the unit sphere, so the camera's translation counts), through w2c and then the projection, each a row-major [4][4] of the host's, each
// row as ((m0 x + m1 y) + m2 z) + m3 w;  uv = clip.xy / clip.w, depth = clip.w, alpha = (-1 <= uv <= 1 on both axes) and depth > 0;  grid_sample of view m's
// image at uv;  sum += sample * alpha (a view that does not see the texel adds an exact zero: it is skipped), count += alpha.
// out = sum / count, 0 where that is not finite (no view: 0 / 0), clamped to [0, 1].  CH = 0: no image, only uv and uv_alpha.
__device__ __forceinline__ float scene_row4(const float* m, const float v[4]) { return ((m[0] * v[0] + m[1] * v[1]) + m[2] * v[2]) + m[3] * v[3]; }

template <int CH>
__global__ __launch_bounds__(256) void scene_bake_latlong_kernel(const float* w2cs, const float* projs, const float* images, int M, int H, int W, int Ht, int Wt,
                                                                 float* uv, float* uv_alpha, float* out) {
    const long n = (long)Ht * Wt;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float rd[3];
    scene_texel_dir(Ht, Wt, (int)(i % Wt), (int)(i / Wt), rd);
    const float p[4] = {rd[0], rd[1], rd[2], 1.0f};
    constexpr int NA = CH > 0 ? CH : 1;
    float acc[NA], cnt = 0.0f;
#pragma unroll
    for (int k = 0; k < NA; ++k) acc[k] = 0.0f;
    for (int m = 0; m < M; ++m) {
        const float* w2c = w2cs + 16 * (long)m;
        const float* pr = projs + 16 * (long)m;
        const float cam[4] = {scene_row4(w2c, p), scene_row4(w2c + 4, p), scene_row4(w2c + 8, p), scene_row4(w2c + 12, p)};
        const float cx = scene_row4(pr, cam), cy = scene_row4(pr + 4, cam), depth = scene_row4(pr + 12, cam);
        const float gx = cx / depth, gy = cy / depth;
        const bool in = gx >= -1.0f && gx <= 1.0f && gy >= -1.0f && gy <= 1.0f && depth > 0.0f;
        const long o = (long)m * n + i;
        if (uv) { uv[2 * o] = gx; uv[2 * o + 1] = gy; }
        if (uv_alpha) uv_alpha[o] = in ? 1.0f : 0.0f;
        if constexpr (CH > 0) {
            if (in) {
                long t[4]; float w[4];
                grid_taps(H, W, gx, gy, t, w);
                const float* img = images + (long)m * H * W * CH;
#pragma unroll
                for (int k = 0; k < CH; ++k)
                    acc[k] += grid_blend(grid_tap(img + k, CH, t[0]), grid_tap(img + k, CH, t[1]), grid_tap(img + k, CH, t[2]), grid_tap(img + k, CH, t[3]), w);
                cnt += 1.0f;
            }
        }
    }
    if constexpr (CH > 0) {
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const float r = acc[k] / cnt;
            out[CH * i + k] = isfinite(r) ? fminf(fmaxf(r, 0.0f), 1.0f) : 0.0f;
        }
    }
}

extern "C" int utx_launch_scene_bake_latlong(const float* w2cs, const float* projs, const float* images, int M, int H, int W, int C, int Ht, int Wt, float* uv,
                                             float* uv_alpha, float* out, hipStream_t stream) {
    if (M <= 0 || Ht <= 0 || Wt <= 0 || (!uv && !uv_alpha && !out)) return -2;
    if (out && (!images || H <= 0 || W <= 0 || C < 1 || C > 4)) return -2;
    const dim3 grid((unsigned)(((long)Ht * Wt + 255) / 256));
#define SCENE_BAKE(CH) hipLaunchKernelGGL(scene_bake_latlong_kernel<CH>, grid, dim3(256), 0, stream, w2cs, projs, images, M, H, W, Ht, Wt, uv, uv_alpha, out)
    switch (out ? C : 0) {
        case 0: SCENE_BAKE(0); break;
        case 1: SCENE_BAKE(1); break;
        case 2: SCENE_BAKE(2); break;
        case 3: SCENE_BAKE(3); break;
        default: SCENE_BAKE(4); break;
    }
#undef SCENE_BAKE
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// Atlas-space geometry buffers (gfx950): NVDiffRendererBase.simple_inverse_rendering of the reference
// (TextureTools/texturetools/render/nvdiffrast/renderer_base.py:352-489) with alpha = coverage (no dr.antialias), every requested buffer of
// every camera in ONE launch.
//
// One thread per texel of the UV raster, x fastest.  The thread reads its raster record (u, v, z/w, id + 1) and the triangle's three vertex
// indices once, forms w = (1 - u) - v once, and then loops over the views itself: per view two gathers of three vertices (camera-space position and
// normal), the interpolation of utx_interpolate (gbuffer_device.h: the same routine utx_gbuffer_shade calls, (a0*u + a1*v) + a2*w) and the
// table below.  torch.lerp(bg, x, alpha) with alpha in {0, 1} returns x or bg exactly, so it is a select.
//
//   buffer               covered texel                                         background
//   world_normal         normalize(interp(v_nrm))                              -1     (:401-407)
//   world_position       interp(v_pos)                                         -1     (:419-429)
//   camera_normal[b]     normalize(interp(v_nrm_cam[b]))                       -1     (:409-417)
//   camera_position[b]   interp(v_pos_cam[b])                                   0     (:445-455)
//   distance[b]          sqrt((x*x + y*y) + z*z) of camera_position             0     (:456-461)
//   z_depth[b]           camera_position.z                                      0     (:462-467)
//   ray_direction[b]     normalize(camera_position)                            -1     (:468-473)
//   cos_ray_normal[b]    (cn.x*rd.x + cn.y*rd.y) + cn.z*rd.z, both as above    -1     (:475-489)
//   normalize(x) = x / max(|x|, 1e-12), |x| = sqrt((x*x + y*y) + z*z)
//
// HBM-bound: 16 B read and up to 29 + 48 B written per texel and view; the vertex gathers hit L2 (neighbouring texels share a triangle).  Plain
// vector loads and stores only: no atomics, no LDS, no scratch, no inline assembly.  Built with -ffp-contract=off (every operation one
// correctly rounded fp32 operation) and without packed fp32 (csrc/build.py NO_PK), which is what UTX_TU_NO_PACKED_FP32 tells the shared header.
#define UTX_TU_NO_PACKED_FP32
#include "common.h"
#include "kernels.h"
#include "gbuffer_device.h"

struct UvGbufferOut {
    unsigned char* mask;
    float *alpha, *world_normal, *world_position, *camera_normal, *camera_position, *distance, *z_depth, *ray_direction, *cos_ray_normal;
};

__device__ __forceinline__ void uvgb_store3(float* base, long texel, const float v[3]) {
    float* o = base + 3 * texel;
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
}

__global__ __launch_bounds__(256) void uv_gbuffer_kernel(const float4* __restrict__ rast, const int* __restrict__ tri, const float* __restrict__ v_pos,
                                                         const float* __restrict__ v_nrm, const float* __restrict__ v_pos_cam,
                                                         const float* __restrict__ v_nrm_cam, long V, int B, long npix, UvGbufferOut o) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const float4 r = rast[i];
    const int id = (int)r.w - 1;
    const bool covered = id >= 0;
    const float u = r.x, v = r.y, w = (1.0f - u) - v;
    long i0 = 0, i1 = 0, i2 = 0;
    if (covered) { i0 = tri[3 * id + 0]; i1 = tri[3 * id + 1]; i2 = tri[3 * id + 2]; }
    if (o.mask) o.mask[i] = covered ? 1 : 0;
    if (o.alpha) o.alpha[i] = covered ? 1.0f : 0.0f;
    if (o.world_normal) {
        float n[3] = {-1.0f, -1.0f, -1.0f};
        if (covered) {
            float p[3];
            gb_interp3(v_nrm + 3 * i0, v_nrm + 3 * i1, v_nrm + 3 * i2, u, v, w, p);
            gb_normalize3(p, gb_length3(p), n);
        }
        uvgb_store3(o.world_normal, i, n);
    }
    if (o.world_position) {
        float p[3] = {-1.0f, -1.0f, -1.0f};
        if (covered) gb_interp3(v_pos + 3 * i0, v_pos + 3 * i1, v_pos + 3 * i2, u, v, w, p);
        uvgb_store3(o.world_position, i, p);
    }
    const bool want_cn = o.camera_normal || o.cos_ray_normal;
    const bool want_cp = o.camera_position || o.distance || o.z_depth || o.ray_direction || o.cos_ray_normal;
    for (int b = 0; b < B; ++b) {
        const long t = (long)b * npix + i;
        float cn[3] = {-1.0f, -1.0f, -1.0f}, cp[3] = {0.0f, 0.0f, 0.0f}, rd[3] = {-1.0f, -1.0f, -1.0f};
        float dist = 0.0f, cosv = -1.0f;
        if (covered) {
            if (want_cn) {
                float p[3];
                const float* a = v_nrm_cam + 3 * V * b;
                gb_interp3(a + 3 * i0, a + 3 * i1, a + 3 * i2, u, v, w, p);
                gb_normalize3(p, gb_length3(p), cn);
            }
            if (want_cp) {
                const float* a = v_pos_cam + 3 * V * b;
                gb_interp3(a + 3 * i0, a + 3 * i1, a + 3 * i2, u, v, w, cp);
                dist = gb_length3(cp);
                gb_normalize3(cp, dist, rd);
            }
            if (o.cos_ray_normal) cosv = gb_dot3(cn[0], rd[0], cn[1], rd[1], cn[2], rd[2]);
        }
        if (o.camera_normal) uvgb_store3(o.camera_normal, t, cn);
        if (o.camera_position) uvgb_store3(o.camera_position, t, cp);
        if (o.distance) o.distance[t] = dist;
        if (o.z_depth) o.z_depth[t] = cp[2];
        if (o.ray_direction) uvgb_store3(o.ray_direction, t, rd);
        if (o.cos_ray_normal) o.cos_ray_normal[t] = cosv;
    }
}

// outs_host[k] is the buffer of bit k of `want` (unitex_hip.h UTX_UVGB_*); pointers of buffers that were not requested are never read
extern "C" int utx_launch_uv_gbuffer(const float* rast, const int* tri, const float* v_pos, const float* v_nrm, const float* v_pos_cam,
                                     const float* v_nrm_cam, int V, int B, int H2D, int W2D, unsigned want, void* const* outs_host,
                                     hipStream_t stream) {
    if (H2D <= 0 || W2D <= 0 || B < 0 || V <= 0 || !outs_host) return -2;
    const long npix = (long)H2D * W2D;
    auto out = [&](int bit) -> void* { return (want >> bit) & 1u ? outs_host[bit] : nullptr; };
    UvGbufferOut o;
    o.mask = (unsigned char*)out(0);
    o.alpha = (float*)out(1);
    o.world_normal = (float*)out(2);
    o.world_position = (float*)out(3);
    o.camera_normal = (float*)out(4);
    o.camera_position = (float*)out(5);
    o.distance = (float*)out(6);
    o.z_depth = (float*)out(7);
    o.ray_direction = (float*)out(8);
    o.cos_ray_normal = (float*)out(9);
    hipLaunchKernelGGL(uv_gbuffer_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, (const float4*)rast, tri, v_pos, v_nrm,
                       v_pos_cam, v_nrm_cam, (long)V, B, npix, o);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// Geometry buffers (gfx950).  Entry points:
//   utx_gbuffer_shade, utx_gbuffer_range, utx_camera_normals   the screen-space buffers of the orbit video
//   utx_uv_gbuffer                                             the atlas-space buffers of simple_inverse_rendering
//   utx_screen_gbuffer                                         the screen-space buffers of a camera batch (simple_rendering)
//   utx_uv_project                                             simple_inverse_rendering's projection of the camera views into the atlas
// All interpolate with shade_device.h's sd_interp, utx_interpolate's (a0*u + a1*v) + a2*w, and normalise with its F.normalize, so a covered pixel's
// value is bit-identical to interpolate_kernel's wherever it is computed.
//
// HBM-bound.  Plain vector loads and stores, no LDS, no scratch, no inline assembly; atomics only in the range reduction.  Built with -ffp-contract=off
// (every operation one correctly rounded fp32 operation) and without packed fp32 (csrc/build.py NO_PK): the sums of products below are exactly what hipcc
// would otherwise turn into the cross-half packed pair that tests/test_asm_hazards_cpu.py bans from every listing.
#include "common.h"
#include "kernels.h"
#include "shade_device.h"

// ---- geometry-buffer shading of the orbit video (VideoExporter.export_orbit_video(video_type=...) -> export_video,
// video/export_nvdiffrast_video.py:37-139, on simple_rendering, render/nvdiffrast/renderer_base.py:153-241, with alpha = coverage):
// one thread per pixel interpolates the triangle's three vertex attributes, then, per MODE,
//   NORMAL    v = n / max(sqrt((nx*nx + ny*ny) + nz*nz), 1e-12), background -1   (world_normal :160-166; camera_normal :168-176 with the
//             per-view, per-vertex re-normalised camera_normals_kernel output as attribute)
//   POSITION  v = p, background -1 (world_position :178-188) or 0 (camera_position :228-235: `fill`)
//   DEPTH     v = the one interpolated channel (clip w), background 0, repeated to three (z_depth :153-158, export_video :107-108)
//   DISTANCE  v = sqrt((px*px + py*py) + pz*pz) of the interpolated camera-space position, background 0, repeated (:236-241)
// then export_video :120-131 in its order: covered pixels (v - lo) / (hi - lo) if scale2 = {lo, hi} is given; v * 0.5 + 0.5 if ndc;
// v * alpha + bg * (1 - alpha) if composite; RGBA float frame (alpha fourth) and clamp(0, 1) * 255 truncated to uint8.
// torch.lerp(fill, v, alpha) with alpha in {0, 1} returns v or fill exactly, so it is a select here.
enum { GB_NORMAL = 0, GB_POSITION = 1, GB_DEPTH = 2, GB_DISTANCE = 3 };

template <int MODE>
__device__ __forceinline__ bool gbuffer_value(const float4 r, const int* tri, const float* attr, int stride, float fill, float v3[3]) {
    const int id = (int)r.w - 1;
    if (id < 0) { v3[0] = v3[1] = v3[2] = fill; return false; }
    const float u = r.x, v = r.y, w = sd_bary_w(u, v);
    const float* a0 = attr + (long)stride * tri[3 * id + 0];
    const float* a1 = attr + (long)stride * tri[3 * id + 1];
    const float* a2 = attr + (long)stride * tri[3 * id + 2];
    if constexpr (MODE == GB_DEPTH) {
        v3[0] = v3[1] = v3[2] = sd_interp1(a0[0], a1[0], a2[0], u, v, w);
    } else {
        float p[3];
        sd_interp<3>(a0, a1, a2, u, v, w, p);
        if constexpr (MODE == GB_NORMAL) {
            sd_normalize3(p, sd_length3(p), v3);
        } else if constexpr (MODE == GB_DISTANCE) {
            v3[0] = v3[1] = v3[2] = sd_length3(p);
        } else {
            v3[0] = p[0]; v3[1] = p[1]; v3[2] = p[2];
        }
    }
    return true;
}

template <int MODE>
__global__ __launch_bounds__(256) void gbuffer_shade_kernel(const float4* rast, const int* tri, const float* attr, int stride, float fill,
                                                            const float* scale2, int ndc, int composite, float bg0, float bg1, float bg2,
                                                            long npix, unsigned char* out_u8, float4* out_rgba) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    float c[3];
    const bool covered = gbuffer_value<MODE>(rast[i], tri, attr, stride, fill, c);
    const float a = covered ? 1.0f : 0.0f;
    if (scale2 && covered) {
        const float lo = scale2[0], hi = scale2[1];
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = (c[k] - lo) / (hi - lo);
    }
    const float bg[3] = {bg0, bg1, bg2};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (ndc) c[k] = c[k] * 0.5f + 0.5f;
        if (composite) c[k] = c[k] * a + bg[k] * (1.0f - a);
        out_u8[3 * i + k] = sd_to_u8(c[k]);
    }
    if (out_rgba) out_rgba[i] = make_float4(c[0], c[1], c[2], a);
}

// mode of the ABI (unitex_hip.h UTX_GBUF_*) -> kernel arm, background fill of the buffer, vertex stride is the caller's
extern "C" int utx_launch_gbuffer_shade(int mode, const float* rast, const int* tri, const float* attr, int stride, const float* scale2,
                                        int ndc, int composite, const float* bg3_host, long npix, void* out_u8, float* out_rgba,
                                        hipStream_t stream) {
    if (npix <= 0 || stride <= 0 || !bg3_host) return -2;
    const dim3 g((unsigned)((npix + 255) / 256)), b(256);
#define GB_LAUNCH(M, FILL) hipLaunchKernelGGL(gbuffer_shade_kernel<M>, g, b, 0, stream, (const float4*)rast, tri, attr, stride, FILL, scale2, \
                                              ndc, composite, bg3_host[0], bg3_host[1], bg3_host[2], npix, (unsigned char*)out_u8, (float4*)out_rgba)
    switch (mode) {
        case 0: case 1: GB_LAUNCH(GB_NORMAL, -1.0f); break;     // world_normal, camera_normal
        case 2: GB_LAUNCH(GB_POSITION, -1.0f); break;           // world_position
        case 3: GB_LAUNCH(GB_POSITION, 0.0f); break;            // camera_position
        case 4: GB_LAUNCH(GB_DEPTH, 0.0f); break;               // z_depth
        case 5: GB_LAUNCH(GB_DISTANCE, 0.0f); break;            // distance
        default: return -2;
    }
#undef GB_LAUNCH
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// (lo, hi) of the buffer over the covered pixels of one frame (export_video :120-125 rgb_sel.min() / .max(), taken on the first frame only):
// per-wave shuffle reduction, one atomic pair per wave.  Floats are ordered through their bit patterns (non-negative: as signed ints,
// negative: reversed as unsigned), so the result is the exact min / max whatever the order.  empty stays 1 if no pixel is covered.
__global__ void gbuffer_range_init_kernel(float* scale2, int* empty) {
    scale2[0] = __int_as_float(0x7f800000); scale2[1] = __int_as_float(0xff800000); *empty = 1;
}

__device__ __forceinline__ void atomic_min_float(float* addr, float v) {
    if (v >= 0.f) atomicMin((int*)addr, __float_as_int(v)); else atomicMax((unsigned int*)addr, __float_as_uint(v));
}
__device__ __forceinline__ void atomic_max_float(float* addr, float v) {
    if (v >= 0.f) atomicMax((int*)addr, __float_as_int(v)); else atomicMin((unsigned int*)addr, __float_as_uint(v));
}

template <int MODE>
__global__ __launch_bounds__(256) void gbuffer_range_kernel(const float4* rast, const int* tri, const float* attr, int stride, long npix,
                                                            float* scale2, int* empty) {
    float lo = __int_as_float(0x7f800000), hi = __int_as_float(0xff800000);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += (long)gridDim.x * blockDim.x) {
        float c[3];
        if (gbuffer_value<MODE>(rast[i], tri, attr, stride, 0.f, c))
            for (int k = 0; k < 3; ++k) { lo = fminf(lo, c[k]); hi = fmaxf(hi, c[k]); }
    }
    for (int off = warpSize / 2; off > 0; off >>= 1) {
        lo = fminf(lo, __shfl_down(lo, off));
        hi = fmaxf(hi, __shfl_down(hi, off));
    }
    if ((threadIdx.x & (warpSize - 1)) == 0 && lo <= hi) {
        atomic_min_float(scale2, lo + 0.0f);      // + 0.0f canonicalises -0
        atomic_max_float(scale2 + 1, hi + 0.0f);
        atomicAnd(empty, 0);
    }
}

extern "C" int utx_launch_gbuffer_range(int mode, const float* rast, const int* tri, const float* attr, int stride, long npix, float* scale2,
                                        int* empty, hipStream_t stream) {
    if (npix <= 0 || stride <= 0) return -2;
    long nb = (npix + 255) / 256; if (nb > 1024) nb = 1024;
    const dim3 g((unsigned)nb), b(256);
    hipLaunchKernelGGL(gbuffer_range_init_kernel, dim3(1), dim3(1), 0, stream, scale2, empty);
#define GB_RANGE(M) hipLaunchKernelGGL(gbuffer_range_kernel<M>, g, b, 0, stream, (const float4*)rast, tri, attr, stride, npix, scale2, empty)
    switch (mode) {
        case 0: case 1: GB_RANGE(GB_NORMAL); break;
        case 2: case 3: GB_RANGE(GB_POSITION); break;
        case 4: GB_RANGE(GB_DEPTH); break;
        case 5: GB_RANGE(GB_DISTANCE); break;
        default: return -2;
    }
#undef GB_RANGE
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// per-view, per-vertex camera-space normals of render_camera_normal (renderer_base.py:169-170): out[n][v] = normalize(nrm[v] @ c2ws[n][:3,:3]),
// out_j = (n0*R0j + n1*R1j) + n2*R2j, F.normalize eps 1e-12
__global__ __launch_bounds__(256) void camera_normals_kernel(const float* nrm, int V, const float* c2ws, float* out) {
    const int v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= V) return;
    const float* m = c2ws + 16 * blockIdx.y;
    const float n[3] = {nrm[3 * v], nrm[3 * v + 1], nrm[3 * v + 2]};
    float c[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const float col[3] = {m[j], m[4 + j], m[8 + j]};
        c[j] = sd_dot3(n, col);
    }
    sd_normalize3(c);
    float* o = out + 3 * ((long)blockIdx.y * V + v);
    o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
}

extern "C" int utx_launch_camera_normals(const float* nrm, int V, const float* c2ws, int n_views, float* out, hipStream_t stream) {
    if (V <= 0 || n_views <= 0) return -2;
    hipLaunchKernelGGL(camera_normals_kernel, dim3((V + 255) / 256, n_views), dim3(256), 0, stream, nrm, V, c2ws, out);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---- the per-pixel geometry of the atlas (utx_uv_gbuffer: simple_inverse_rendering, render/nvdiffrast/renderer_base.py:352-489) and of the screen
// (utx_screen_gbuffer: simple_rendering, :101-350), both with alpha = coverage (dr.antialias is not wired here: antialias.hip runs after the screen kernel, on request).  A pixel is a texel of the UV raster or a pixel of
// one view's raster; its record is (u, v, z/w, id + 1), w = (1 - u) - v is formed once.  torch.lerp(bg, x, alpha) with alpha in {0, 1} returns x or
// bg exactly, so it is a select.
//
//   buffer               covered pixel                                         background   (atlas, screen)
//   world_normal         normalize(interp(v_nrm))                              -1     (:401-407, :172-178)
//   world_position       interp(v_pos)                                         -1     (:419-429, :190-200)
//   camera_normal[b]     normalize(interp(v_nrm_cam[b]))                       -1     (:409-417, :180-188)
//   camera_position[b]   interp(v_pos_cam[b])                                   0     (:445-455, :241-248)
//   distance[b]          sqrt((x*x + y*y) + z*z) of camera_position             0     (:456-461, :249-254)
//   ray_direction[b]     normalize(camera_position)                            -1     (:468-473, :255-260)
//   cos_ray_normal[b]    (cn.x*rd.x + cn.y*rd.y) + cn.z*rd.z, both as above    -1     (:475-489, :262-274)
//   z_depth[b]           atlas: camera_position.z; screen: interp(clip_w[b])    0     (:462-467, :165-170) -- each kernel's own, see there
//   normalize(x) = x / max(|x|, 1e-12), |x| = sqrt((x*x + y*y) + z*z)
// distance on the screen: with render_camera_position set the reference takes the norm of the ALREADY MASKED position (:245, :250), without it of
// the raw one and masks afterwards (:251); with alpha = mask both give |p| on a covered pixel and 0 on the background, which is what is written.
//
// The two kernels stay two launches: the atlas has ONE raster for all views, so its thread reads the record and the triangle once, writes the world
// buffers once and loops over the views; the screen has a raster per view, one thread per (view, pixel).  A shared launch geometry would re-read the
// atlas record B times.
struct GeomOut {      // the buffers both kernels write; a null pointer = not requested
    unsigned char* mask;
    float *alpha, *world_normal, *world_position, *camera_normal, *camera_position, *distance, *z_depth, *ray_direction, *cos_ray_normal;
};
enum { GEOM_OUT_COUNT = 10 };

struct GeomPixel { bool covered; long i0, i1, i2; float u, v, w; };      // a raster record: coverage, the triangle's vertices, the barycentrics

__device__ __forceinline__ GeomPixel geom_pixel(const float4 r, const int* __restrict__ tri) {
    const int id = (int)r.w - 1;
    GeomPixel p = {id >= 0, 0, 0, 0, r.x, r.y, sd_bary_w(r.x, r.y)};
    if (p.covered) { p.i0 = tri[3 * id + 0]; p.i1 = tri[3 * id + 1]; p.i2 = tri[3 * id + 2]; }
    return p;
}

__device__ __forceinline__ void geom_store3(float* base, long pixel, const float v[3]) {
    float* o = base + 3 * pixel;
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
}

// mask, alpha and the world buffers of the pixel at index i
__device__ __forceinline__ void geom_world(const GeomPixel& p, const float* __restrict__ v_pos, const float* __restrict__ v_nrm, const GeomOut& o, long i) {
    if (o.mask) o.mask[i] = p.covered ? 1 : 0;
    if (o.alpha) o.alpha[i] = p.covered ? 1.0f : 0.0f;
    if (o.world_normal) {
        float n[3] = {-1.0f, -1.0f, -1.0f};
        if (p.covered) {
            float x[3];
            sd_interp<3>(v_nrm + 3 * p.i0, v_nrm + 3 * p.i1, v_nrm + 3 * p.i2, p.u, p.v, p.w, x);
            sd_normalize3(x, sd_length3(x), n);
        }
        geom_store3(o.world_normal, i, n);
    }
    if (o.world_position) {
        float x[3] = {-1.0f, -1.0f, -1.0f};
        if (p.covered) sd_interp<3>(v_pos + 3 * p.i0, v_pos + 3 * p.i1, v_pos + 3 * p.i2, p.u, p.v, p.w, x);
        geom_store3(o.world_position, i, x);
    }
}

// the camera buffers of ONE view (v_pos_cam / v_nrm_cam: that view's [V][3]) at index t, all but z_depth.  cp returns the interpolated camera
// position (0 on the background); cp_for_caller: the caller reads it even if no buffer here does.
__device__ __forceinline__ void geom_view(const GeomPixel& p, const float* __restrict__ v_pos_cam, const float* __restrict__ v_nrm_cam, const GeomOut& o,
                                          long t, bool cp_for_caller, float cp[3]) {
    const bool want_cn = o.camera_normal || o.cos_ray_normal;
    const bool want_cp = o.camera_position || o.distance || o.ray_direction || o.cos_ray_normal || cp_for_caller;
    float cn[3] = {-1.0f, -1.0f, -1.0f}, rd[3] = {-1.0f, -1.0f, -1.0f};
    float dist = 0.0f, cosv = -1.0f;
    cp[0] = cp[1] = cp[2] = 0.0f;
    if (p.covered) {
        if (want_cn) {
            float x[3];
            sd_interp<3>(v_nrm_cam + 3 * p.i0, v_nrm_cam + 3 * p.i1, v_nrm_cam + 3 * p.i2, p.u, p.v, p.w, x);
            sd_normalize3(x, sd_length3(x), cn);
        }
        if (want_cp) {
            sd_interp<3>(v_pos_cam + 3 * p.i0, v_pos_cam + 3 * p.i1, v_pos_cam + 3 * p.i2, p.u, p.v, p.w, cp);
            dist = sd_length3(cp);
            sd_normalize3(cp, dist, rd);
        }
        if (o.cos_ray_normal) cosv = sd_dot3(cn, rd);
    }
    if (o.camera_normal) geom_store3(o.camera_normal, t, cn);
    if (o.camera_position) geom_store3(o.camera_position, t, cp);
    if (o.distance) o.distance[t] = dist;
    if (o.ray_direction) geom_store3(o.ray_direction, t, rd);
    if (o.cos_ray_normal) o.cos_ray_normal[t] = cosv;
}

// the buffer of the bit `mask` of `want`, or null: outs_host[k] belongs to bit k, and the entry of a buffer that was not requested is never read
static void* wanted(unsigned want, void* const* outs_host, unsigned mask) { return (want & mask) ? outs_host[__builtin_ctz(mask)] : nullptr; }

// bits[k]: the ABI's bit (UTX_UVGB_* / UTX_SGB_*, which order theirs differently) of the k-th member of GeomOut
static GeomOut geom_out(unsigned want, void* const* outs_host, const unsigned (&bits)[GEOM_OUT_COUNT]) {
    void* p[GEOM_OUT_COUNT];
    for (int k = 0; k < GEOM_OUT_COUNT; ++k) p[k] = wanted(want, outs_host, bits[k]);
    return {(unsigned char*)p[0], (float*)p[1], (float*)p[2], (float*)p[3], (float*)p[4], (float*)p[5], (float*)p[6], (float*)p[7], (float*)p[8], (float*)p[9]};
}

// ---- atlas-space geometry buffers, every requested buffer of every camera in ONE launch.  One thread per texel of the UV raster, x fastest; per view
// two gathers of three vertices (camera-space position and normal) and the table above.  z_depth is the camera z of the interpolated position.
// 16 B read and up to 29 + 48 B written per texel and view; the vertex gathers hit L2 (neighbouring texels share a triangle).
__global__ __launch_bounds__(256) void uv_gbuffer_kernel(const float4* __restrict__ rast, const int* __restrict__ tri, const float* __restrict__ v_pos,
                                                         const float* __restrict__ v_nrm, const float* __restrict__ v_pos_cam,
                                                         const float* __restrict__ v_nrm_cam, long V, int B, long npix, GeomOut o) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const GeomPixel p = geom_pixel(rast[i], tri);
    geom_world(p, v_pos, v_nrm, o, i);
    for (int b = 0; b < B; ++b) {
        const long t = (long)b * npix + i;
        float cp[3];
        geom_view(p, v_pos_cam + 3 * V * b, v_nrm_cam + 3 * V * b, o, t, o.z_depth != nullptr, cp);
        if (o.z_depth) o.z_depth[t] = cp[2];
    }
}

extern "C" int utx_launch_uv_gbuffer(const float* rast, const int* tri, const float* v_pos, const float* v_nrm, const float* v_pos_cam,
                                     const float* v_nrm_cam, int V, int B, int H2D, int W2D, unsigned want, void* const* outs_host,
                                     hipStream_t stream) {
    if (H2D <= 0 || W2D <= 0 || B < 0 || V <= 0 || !outs_host) return -2;
    const long npix = (long)H2D * W2D;
    const GeomOut o = geom_out(want, outs_host, {UTX_UVGB_MASK, UTX_UVGB_ALPHA, UTX_UVGB_WORLD_NORMAL, UTX_UVGB_WORLD_POSITION, UTX_UVGB_CAMERA_NORMAL,
                                                 UTX_UVGB_CAMERA_POSITION, UTX_UVGB_DISTANCE, UTX_UVGB_Z_DEPTH, UTX_UVGB_RAY_DIRECTION, UTX_UVGB_COS_RAY_NORMAL});
    hipLaunchKernelGGL(uv_gbuffer_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, (const float4*)rast, tri, v_pos, v_nrm,
                       v_pos_cam, v_nrm_cam, (long)V, B, npix, o);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---- screen-space buffers of a camera batch, every requested buffer of every camera in ONE launch.  One thread per pixel of rast [B][H][W][4], x
// fastest: 16 B read and up to 77 B + the three buffers below written.  z_depth is the interpolated clip w, NOT camera z as on the atlas.
//
//   buffer            covered pixel                                          background
//   v_attr            interp(v_attr), Ca channels                            rule   (:276-287)
//   uv                interp(v_uv), in [-1, 1]                               -1     (:289-303)
//   map_attr          the maps sampled at uv, concatenated along channels    rule   (:305-336)
// rule (:278-284, :327-333): without a background the value stays as computed on EVERY pixel -- dr.interpolate's 0 for v_attr, the maps' sample at the
// background's uv = (-1, -1) for map_attr; with one (a scalar, a [C] vector or a dense [B][H][W][C] image) covered pixels keep the value and the rest
// take the background.
// FILTER of map_attr (grid_interpolate_mode): 0 'bilinear' / 1 'nearest' = F.grid_sample(align_corners=False, zero padding), 2 'nvdiffrast' =
// dr.texture(uv * 0.5 + 0.5, filter_mode='linear') with its wrap boundary: shade_device.h's grid_taps / grid_nearest / wrap_taps, the taps of the
// back-projection sampler, computed once per map and pixel and blended per channel.
enum { SGB_BG_NONE = 0, SGB_BG_SCALAR = 1, SGB_BG_VECTOR = 2, SGB_BG_DENSE = 3 };

struct ScreenGbufferArgs {
    const float4* rast; const int* tri;
    const float *v_pos, *v_nrm, *v_uv, *v_attr, *clip_w, *v_pos_cam, *v_nrm_cam;
    const float* map[UTX_SGB_MAX_MAPS];
    int map_h[UTX_SGB_MAX_MAPS], map_w[UTX_SGB_MAX_MAPS], map_c[UTX_SGB_MAX_MAPS];
    int n_maps, Ca, Cm, bg_kind;
    float bg_scalar;
    const float *bg_v_attr, *bg_map_attr;
    long V, npix, total;      // vertices, pixels of one view, pixels of all views
    GeomOut o;
    float *o_v_attr, *uv, *map_attr;
};

// channel c of the background of a pixel, kind != SGB_BG_NONE: the scalar, the [C] vector's or the dense [pixels][C] image's
__device__ __forceinline__ float sgb_background(int kind, float scalar, const float* bg, long pixel, int C, int c) {
    return kind == SGB_BG_SCALAR ? scalar : kind == SGB_BG_VECTOR ? bg[c] : bg[pixel * C + c];
}

// C channels of one map [Ht][Wt][C] at the NDC (gx, gy)
template <int FILTER>
__device__ __forceinline__ void sgb_sample_map(const float* tex, int Ht, int Wt, int C, float gx, float gy, float* out) {
    if constexpr (FILTER == 0) {
        long o[4]; float w[4];
        grid_taps(Ht, Wt, gx, gy, o, w);
        for (int c = 0; c < C; ++c)
            out[c] = grid_blend(grid_tap(tex + c, (long)C, o[0]), grid_tap(tex + c, (long)C, o[1]), grid_tap(tex + c, (long)C, o[2]), grid_tap(tex + c, (long)C, o[3]), w);
    } else if constexpr (FILTER == 1) {
        const long o = grid_nearest(Ht, Wt, gx, gy);
        for (int c = 0; c < C; ++c) out[c] = grid_tap(tex + c, (long)C, o);
    } else {
        long o00, o10, o01, o11; float fu, fv;
        const bool finite = wrap_taps(Ht, Wt, gx, gy, o00, o10, o01, o11, fu, fv);
        for (int c = 0; c < C; ++c)
            out[c] = finite ? wrap_blend(tex[o00 * C + c], tex[o10 * C + c], tex[o01 * C + c], tex[o11 * C + c], fu, fv) : 0.0f;
    }
}

template <int FILTER>
__global__ __launch_bounds__(256) void screen_gbuffer_kernel(ScreenGbufferArgs a) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.total) return;
    const long b = i / a.npix;
    const GeomPixel p = geom_pixel(a.rast[i], a.tri);
    const bool covered = p.covered;
    const float u = p.u, v = p.v, w = p.w;
    geom_world(p, a.v_pos, a.v_nrm, a.o, i);
    if (a.o.z_depth) {
        const float* cw = a.clip_w + a.V * b;
        a.o.z_depth[i] = covered ? sd_interp1(cw[p.i0], cw[p.i1], cw[p.i2], u, v, w) : 0.0f;
    }
    float cp[3];
    geom_view(p, a.v_pos_cam + 3 * a.V * b, a.v_nrm_cam + 3 * a.V * b, a.o, i, false, cp);
    if (a.o_v_attr) {
        float* o = a.o_v_attr + i * a.Ca;
        const float *p0 = a.v_attr + p.i0 * a.Ca, *p1 = a.v_attr + p.i1 * a.Ca, *p2 = a.v_attr + p.i2 * a.Ca;
        for (int c = 0; c < a.Ca; ++c) {
            if (covered) o[c] = sd_interp1(p0[c], p1[c], p2[c], u, v, w);
            else o[c] = a.bg_kind == SGB_BG_NONE ? 0.0f : sgb_background(a.bg_kind, a.bg_scalar, a.bg_v_attr, i, a.Ca, c);
        }
    }
    if (a.uv || a.map_attr) {
        float g[2] = {-1.0f, -1.0f};
        if (covered) sd_interp<2>(a.v_uv + 2 * p.i0, a.v_uv + 2 * p.i1, a.v_uv + 2 * p.i2, u, v, w, g);
        if (a.uv) { a.uv[2 * i] = g[0]; a.uv[2 * i + 1] = g[1]; }
        if (a.map_attr) {
            float* o = a.map_attr + i * a.Cm;
            if (!covered && a.bg_kind != SGB_BG_NONE) {
                for (int c = 0; c < a.Cm; ++c) o[c] = sgb_background(a.bg_kind, a.bg_scalar, a.bg_map_attr, i, a.Cm, c);
            } else {
#pragma unroll
                for (int m = 0; m < UTX_SGB_MAX_MAPS; ++m) {
                    if (m < a.n_maps) {
                        sgb_sample_map<FILTER>(a.map[m], a.map_h[m], a.map_w[m], a.map_c[m], g[0], g[1], o);
                        o += a.map_c[m];
                    }
                }
            }
        }
    }
}

// FILTER is a template argument of the kernels that sample a map: `filter` (0, 1 or 2, checked by the caller) -> the instance, one thread per pixel
#define LAUNCH_BY_FILTER(KERNEL, filter, args, stream) do { \
        const dim3 g_((unsigned)(((args).total + 255) / 256)), b_(256); \
        if ((filter) == 0) hipLaunchKernelGGL(KERNEL<0>, g_, b_, 0, stream, args); \
        else if ((filter) == 1) hipLaunchKernelGGL(KERNEL<1>, g_, b_, 0, stream, args); \
        else hipLaunchKernelGGL(KERNEL<2>, g_, b_, 0, stream, args); \
    } while (0)

// the arguments were checked by utx_screen_gbuffer (capi.cpp); B * H * W == 0 or want == 0 launches nothing
extern "C" int utx_launch_screen_gbuffer(const float* rast, const int* tri, const float* v_pos, const float* v_nrm, const float* v_uv, const float* v_attr,
                                         int Ca, const float* clip_w, const float* v_pos_cam, const float* v_nrm_cam, int V, int B, int H, int W,
                                         int n_maps, const float* const* maps_host, const int* map_dims_host, int filter, int bg_kind, float bg_scalar,
                                         const float* bg_v_attr, const float* bg_map_attr, unsigned want, void* const* outs_host, hipStream_t stream) {
    if (B < 0 || H < 0 || W < 0 || n_maps < 0 || n_maps > UTX_SGB_MAX_MAPS || filter < 0 || filter > 2) return -2;
    ScreenGbufferArgs a = {};
    a.npix = (long)H * W;
    a.total = a.npix * B;
    if (a.total == 0 || want == 0) return 0;
    a.rast = (const float4*)rast; a.tri = tri;
    a.v_pos = v_pos; a.v_nrm = v_nrm; a.v_uv = v_uv; a.v_attr = v_attr; a.clip_w = clip_w; a.v_pos_cam = v_pos_cam; a.v_nrm_cam = v_nrm_cam;
    a.V = V; a.Ca = Ca; a.bg_kind = bg_kind; a.bg_scalar = bg_scalar; a.bg_v_attr = bg_v_attr; a.bg_map_attr = bg_map_attr;
    a.o = geom_out(want, outs_host, {UTX_SGB_MASK, UTX_SGB_ALPHA, UTX_SGB_WORLD_NORMAL, UTX_SGB_WORLD_POSITION, UTX_SGB_CAMERA_NORMAL, UTX_SGB_CAMERA_POSITION,
                                     UTX_SGB_DISTANCE, UTX_SGB_Z_DEPTH, UTX_SGB_RAY_DIRECTION, UTX_SGB_COS_RAY_NORMAL});
    a.o_v_attr = (float*)wanted(want, outs_host, UTX_SGB_V_ATTR);
    a.uv = (float*)wanted(want, outs_host, UTX_SGB_UV);
    a.map_attr = (float*)wanted(want, outs_host, UTX_SGB_MAP_ATTR);
    if (a.map_attr) {
        a.n_maps = n_maps;
        for (int m = 0; m < n_maps; ++m) {
            a.map[m] = maps_host[m];
            a.map_h[m] = map_dims_host[3 * m]; a.map_w[m] = map_dims_host[3 * m + 1]; a.map_c[m] = map_dims_host[3 * m + 2];
            a.Cm += a.map_c[m];
        }
    }
    LAUNCH_BY_FILTER(screen_gbuffer_kernel, filter, a, stream);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---- atlas-space view projection: render_uv / render_map_attr of NVDiffRendererBase.simple_inverse_rendering (render/nvdiffrast/renderer_base.py:504-559)
// with alpha = coverage (dr.antialias is not wired here), every texel of every view in ONE launch.
//
// One thread per (view, texel) of the atlas raster rast2d [H2D][W2D][4], x fastest.  With tri = rast2d.w - 1:
//   vis       tri >= 0 and face_mask[b][tri]                     (:513-520: the raster with the faces the view does not see taken out)
//   uv        vis ? interp(v_ndc[b]) : (-1, -1)                  (:527-536; v_ndc = the view's NDC xy per vertex, utx_transform_points)
//   uv_alpha  vis                                                (:524)
// and with a map [Bm][Hm][Wm][C] (Bm = 1: shared, Bm = B: one image per view) and rast_map [B][Hm][Wm][4], the views rasterised at the map's size (:544):
//   s         the map sampled at uv with FILTER (sgb_sample_map above: the lookups of utx_screen_gbuffer); for an invisible texel that is the
//             sample at (-1, -1), as in the reference
//   cov       grid_sample(nearest, zero padding) of the view's coverage rast_map.w > 0 at uv (:545-546): only .w is read, straight from the raster
//   uv_alpha  cov < 1 ? 0 : uv_alpha                             (:547)
//   map_attr  with a background: uv_alpha ? s : bg (:548-554, a lerp with a weight of 0 or 1);  without: cov < 1 ? map[b or 0][0][0][:] : s  (:556)
// uv itself is not gated by cov.  The atlas record is read once per view; no [B][H][W][4] raster of the visible faces is ever written.
struct UvProjectArgs {
    const float4* rast2d; const int* tri; const unsigned char* face_mask; const float* v_ndc;
    const float* map; const float* rast_map; const float* bg;
    long F, V, npix, total;
    int Bm, Hm, Wm, C, bg_kind;
    float bg_scalar;
    float *uv, *uv_alpha, *map_attr;
};

template <int FILTER>
__global__ __launch_bounds__(256) void uv_project_kernel(UvProjectArgs a) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.total) return;
    const long b = i / a.npix;
    const SdUvView s = sd_uv_view(a.rast2d[i - b * a.npix], a.tri, a.F, a.face_mask + b * a.F, a.v_ndc + 2 * a.V * b);
    const float* g = s.g;
    a.uv[2 * i] = g[0]; a.uv[2 * i + 1] = g[1];
    bool alpha = s.vis;
    if (a.map_attr) {
        const long msize = (long)a.Hm * a.Wm;
        const float* m = a.map + (a.Bm > 1 ? b : 0) * msize * a.C;
        const bool cov = sd_view_coverage(a.rast_map + 4 * b * msize, a.Hm, a.Wm, g[0], g[1]);
        alpha = alpha && cov;
        float* out = a.map_attr + i * a.C;
        if (a.bg_kind != SGB_BG_NONE && !alpha) {
            for (int c = 0; c < a.C; ++c) out[c] = sgb_background(a.bg_kind, a.bg_scalar, a.bg, i, a.C, c);
        } else if (a.bg_kind == SGB_BG_NONE && !cov) {
            for (int c = 0; c < a.C; ++c) out[c] = m[c];
        } else {
            sgb_sample_map<FILTER>(m, a.Hm, a.Wm, a.C, g[0], g[1], out);
        }
    }
    a.uv_alpha[i] = alpha ? 1.0f : 0.0f;
}

// the arguments were checked by utx_uv_project (capi.cpp); map == nullptr: uv and uv_alpha only
extern "C" int utx_launch_uv_project(const float* rast2d, const int* tri, int F, const unsigned char* face_mask, const float* v_ndc, int V, int B, int H2D, int W2D,
                                     const float* map, int Bm, int Hm, int Wm, int C, const float* rast_map, int filter, int bg_kind, float bg_scalar,
                                     const float* bg, float* uv, float* uv_alpha, float* map_attr, hipStream_t stream) {
    if (B <= 0 || H2D <= 0 || W2D <= 0 || F <= 0 || V <= 0 || filter < 0 || filter > 2) return -2;
    UvProjectArgs a = {};
    a.rast2d = (const float4*)rast2d; a.tri = tri; a.face_mask = face_mask; a.v_ndc = v_ndc;
    a.F = F; a.V = V; a.npix = (long)H2D * W2D; a.total = a.npix * B;
    a.uv = uv; a.uv_alpha = uv_alpha;
    if (map) {
        a.map = map; a.rast_map = rast_map; a.bg = bg; a.Bm = Bm; a.Hm = Hm; a.Wm = Wm; a.C = C; a.bg_kind = bg_kind; a.bg_scalar = bg_scalar;
        a.map_attr = map_attr;
    }
    LAUNCH_BY_FILTER(uv_project_kernel, filter, a, stream);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}
#undef LAUNCH_BY_FILTER

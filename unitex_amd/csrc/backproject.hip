// Fused UV back-projection (gfx950): per (view, texel) colour gather + ray visibility, the visibility
// hole-filling, and the priority composite.
//
// Replaces NVDiffRendererInverse.uv_to_pcd (TextureTools/texturetools/render/nvdiffrast/
// renderer_inverse.py:262-343) and the composite loop of bake_mv_to_uv_reproject_blur (:591-602).
// The reference materialises ~10 tensors of shape [6,2048,2048,3] f32 (302 MB each) on the way
// (rays_o, rays_d, ndc, sampled image, masked_select copies ...); here one pass reads the 16-byte UV
// raster record per texel, recomputes position / ray / NDC in registers, bilinearly samples the view
// (4 taps x float4, L2/MALL resident: 6 x 512^2 x 16 B = 25 MB), walks the LBVH and writes 12 B colour
// + 2 flag bytes per (view, texel).  HBM-bound gather: no LDS, coalesced texel-major reads/writes.
// Same float expressions, in the same order, as oracle/geom_ref.c::utxref_backproject (-ffp-contract=off).
#include "common.h"
#include "kernels.h"
#include "bvh_device.h"
#include "shade_device.h"

// The two lookups of a view image (grid_sample with zero padding, nvdiffrast's linear lookup with wrap) are shade_device.h's sample_view.
// the NDC of a texel in view `nd` [V][2]: the triangle's three vertex NDCs at the texel's barycentrics, as utx_interpolate would
__device__ __forceinline__ void texel_ndc(const float* nd, int f0, int f1, int f2, float u, float v, float w, float g[2]) {
    sd_interp<2>(nd + 2 * (long)f0, nd + 2 * (long)f1, nd + 2 * (long)f2, u, v, w, g);
}

// MODE 1: stackless thread-per-ray walk over the packed tree (bvh_device.h); MODE 0: the reference's 64-entry stack walk, kept for trees deeper than
// UTX_BVH_PACKED_MAX_DEPTH (where the reference's stack overflow quirk could matter) and for A/B tests; MODE 2 (round 4, the default): a wave owns an
// 8 x 8 TEXEL TILE of one view and its 64 parallel rays walk the packed tree as ONE PACKET (bvh_trace_packet: nodes through the scalar cache, per-lane
// box / triangle tests, bit-identical results); 256 threads = a 16 x 16 block of texels, tiles without a covered texel skip the walk.
// PERSP (renderer_inverse.py:279-281, perspective=True): every ray of view v starts at the camera centre eyes[v] = c2w[v][:3, 3] and points at the texel's
// surface point, d = (pos - eye) / max(|pos - eye|, 1e-12); the orthographic arm (one direction per view, origin 2 sqrt(3) behind the point) is unchanged.
// SAMPLE (renderer_inverse.py:290-305, grid_interpolate_mode): 0 = grid_sample(bilinear, zero padding, align_corners=False); 1 = dr.texture(uv = ndc * 0.5 + 0.5,
// filter_mode='linear') with nvdiffrast's default wrap boundary (its indexTextureLinear + bilerp restated above); a non-finite coordinate samples zero.
// VIS (utx_backproject_vis, the 9-channel bake): visibility only -- p.images is the alpha plane [n][H][W] f32, p.color is not touched; the alpha expression, the ray
// and the walk are the ones of the colour kernel, so rayvis / alphaok come out bit-identical.
template <int MODE, bool PERSP, int SAMPLE, bool VIS = false>
__global__ __launch_bounds__(256) void backproject_kernel(utx_backproject_desc p, const float* eyes, const int* info, const float* aabb, const float4* nodes,
                                                          const float4* tris) {
    __shared__ int pstack[MODE == 2 ? 4 * 192 : 1];      // MODE 2: the packets' DFS stacks, 64 x {node, mask lo, mask hi} per wave
    const long T = (long)p.T_h * p.T_w;
    long t;
    bool inside = true;
    if constexpr (MODE == 2) {
        const int tiles_x = (p.T_w + 15) / 16;
        const int by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
        const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
        const int x = bx * 16 + (wv & 1) * 8 + (ln & 7), y = by * 16 + (wv >> 1) * 8 + (ln >> 3);
        inside = x < p.T_w && y < p.T_h;
        t = inside ? (long)y * p.T_w + x : 0;
    } else {
        t = (long)blockIdx.x * blockDim.x + threadIdx.x;
        if (t >= T) return;
    }
    const int vw = p.view_begin + blockIdx.y;
    const float4 r = inside ? ((const float4*)p.rast2d)[t] : make_float4(0.f, 0.f, 0.f, 0.f);
    const int id = (int)r.w - 1;
    float* oc = VIS ? nullptr : (float*)p.color + ((long)vw * T + t) * 3;
    unsigned char* rv = (unsigned char*)p.rayvis + (long)vw * T + t;
    unsigned char* ao = (unsigned char*)p.alphaok + (long)vw * T + t;
    if constexpr (MODE == 2) {
        if (__ballot(id >= 0) == 0) {      // nothing of this tile is covered
            if (inside) { if constexpr (!VIS) { oc[0] = 0.f; oc[1] = 0.f; oc[2] = 0.f; } *rv = 0; *ao = 0; }
            return;
        }
        if (id < 0) {      // an uncovered texel of a covered tile stays in the wave (the packet walk is wave-wide) with its ray switched off
            if (inside) { if constexpr (!VIS) { oc[0] = 0.f; oc[1] = 0.f; oc[2] = 0.f; } *rv = 0; *ao = 0; }
            return;      // (the packet walk below ballots over the lanes that are still here)
        }
    } else if (id < 0) { if constexpr (!VIS) { oc[0] = 0.f; oc[1] = 0.f; oc[2] = 0.f; } *rv = 0; *ao = 0; return; }
    const float* vert = (const float*)p.verts;
    const int* faces = (const int*)p.faces;
    const float u = r.x, v = r.y, w = sd_bary_w(u, v);
    const int f0 = faces[3 * (long)id], f1 = faces[3 * (long)id + 1], f2 = faces[3 * (long)id + 2];
    float pos[3];
    sd_interp<3>(vert + 3 * (long)f0, vert + 3 * (long)f1, vert + 3 * (long)f2, u, v, w, pos);
    float ro[3], d[3];
    if constexpr (PERSP) {
        const float* e = eyes + 3 * vw;
        ro[0] = e[0]; ro[1] = e[1]; ro[2] = e[2];
        const float dv[3] = {pos[0] - e[0], pos[1] - e[1], pos[2] - e[2]};
        float dn = sd_length3(dv); if (dn < 1e-12f) dn = 1e-12f;      // a compare, as the oracle's: a NaN length stays NaN (sd_normalize3's fmaxf would floor it)
        d[0] = dv[0] / dn; d[1] = dv[1] / dn; d[2] = dv[2] / dn;
    } else {
        const float* d_in = (const float*)p.dirs + 3 * vw;
        const float two_sqrt3 = p.two_sqrt3;
        ro[0] = pos[0] - two_sqrt3 * d_in[0]; ro[1] = pos[1] - two_sqrt3 * d_in[1]; ro[2] = pos[2] - two_sqrt3 * d_in[2];
        float dn = sqrtf(dot3(d_in, d_in)); if (dn < 1e-12f) dn = 1e-12f;
        d[0] = d_in[0] / dn; d[1] = d_in[1] / dn; d[2] = d_in[2] / dn;
    }
    const float* n = (const float*)p.fnormal + 3 * (long)id;
    float ld = sqrtf(dot3(d, d)); if (ld < 1e-8f) ld = 1e-8f;
    const float nn[3] = {n[0], n[1], n[2]};
    float ln = sqrtf(dot3(nn, nn)); if (ln < 1e-8f) ln = 1e-8f;
    const float cs = dot3(d, nn) / (ld * ln);
    const float* nd = (const float*)p.vndc + (long)vw * p.V * 2;
    float g[2];
    texel_ndc(nd, f0, f1, f2, u, v, w, g);
    const int H = p.H, W = p.W;
    float sa;
    if constexpr (VIS) {
        sa = sample_view<SAMPLE>((const float*)p.images + (long)vw * H * W, 1, H, W, g[0], g[1]);
    } else {
        const float4 s = sample_view<SAMPLE>((const float4*)p.images + (long)vw * H * W, 1, H, W, g[0], g[1]);
        oc[0] = s.x; oc[1] = s.y; oc[2] = s.z;
        sa = s.w;
    }
    *ao = sa > 0.999f ? 1 : 0;
    const int hit = MODE == 2 ? bvh_trace_packet(nodes, tris, ro, d, true, pstack + (threadIdx.x >> 6) * 192, nullptr)
                  : MODE == 1 ? bvh_trace_packed(nodes, tris, ro, d, nullptr) : bvh_trace_one(info, aabb, vert, faces, ro, d);
    *rv = (hit == id && hit != -1 && cs < p.cos_thresh) ? 1 : 0;
}

template <bool PERSP, int SAMPLE, bool VIS = false>
static void launch_backproject(const utx_backproject_desc& p, const float* eyes, const utx_bvh* bvh, int depth, hipStream_t stream) {
    const long T = (long)p.T_h * p.T_w;
    dim3 grid((unsigned)((T + 255) / 256), p.view_count);
    if (depth <= UTX_BVH_PACKED_MAX_DEPTH && !g_utx_opt.bvh_stack_walk && g_utx_opt.bvh_packet) {
        dim3 gridp((unsigned)(((p.T_w + 15) / 16) * ((p.T_h + 15) / 16)), p.view_count);
        hipLaunchKernelGGL((backproject_kernel<2, PERSP, SAMPLE, VIS>), gridp, dim3(256), 0, stream, p, eyes, bvh->info, bvh->aabb, bvh->nodes, bvh->tris);
    } else if (depth <= UTX_BVH_PACKED_MAX_DEPTH && !g_utx_opt.bvh_stack_walk)
        hipLaunchKernelGGL((backproject_kernel<1, PERSP, SAMPLE, VIS>), grid, dim3(256), 0, stream, p, eyes, bvh->info, bvh->aabb, bvh->nodes, bvh->tris);
    else
        hipLaunchKernelGGL((backproject_kernel<0, PERSP, SAMPLE, VIS>), grid, dim3(256), 0, stream, p, eyes, bvh->info, bvh->aabb, bvh->nodes, bvh->tris);
}

// eyes == nullptr: orthographic rays along p.dirs; otherwise [n_views][3] camera centres (perspective), p.dirs / p.two_sqrt3 unused.
// sample: 0 = grid_sample (zero padding), 1 = nvdiffrast linear filtering with wrap
template <bool VIS>
static int dispatch_backproject(const utx_backproject_desc& p, const float* eyes, int sample, const utx_bvh* bvh, hipStream_t stream) {
    const int depth = utx_bvh_depth_impl(const_cast<utx_bvh*>(bvh));      // first use after a build: waits for the build's depth word
    if (depth < 0) return -7;
    if (sample == 0) {
        if (eyes) launch_backproject<true, 0, VIS>(p, eyes, bvh, depth, stream);
        else launch_backproject<false, 0, VIS>(p, nullptr, bvh, depth, stream);
    } else {
        if (eyes) launch_backproject<true, 1, VIS>(p, eyes, bvh, depth, stream);
        else launch_backproject<false, 1, VIS>(p, nullptr, bvh, depth, stream);
    }
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

extern "C" int utx_launch_backproject(const utx_backproject_desc* hp, const float* eyes, int sample, const utx_bvh* bvh, hipStream_t stream) {
    const utx_backproject_desc p = *hp;
    if (!bvh || p.T_h <= 0 || p.T_w <= 0 || p.view_count <= 0 || (sample != 0 && sample != 1)) return -2;
    if (sample == 1 && (p.H <= 0 || p.W <= 0)) return -2;      // the wrap needs a non-empty view
    return dispatch_backproject<false>(p, eyes, sample, bvh, stream);
}

// visibility only (the 9-channel bake): p.images = alpha [n][H][W] f32, p.color unused.  Same traversal choice, same options.
extern "C" int utx_launch_backproject_vis(const utx_backproject_desc* hp, const float* eyes, int sample, const utx_bvh* bvh, hipStream_t stream) {
    const utx_backproject_desc p = *hp;
    if (!bvh || p.T_h <= 0 || p.T_w <= 0 || p.view_count <= 0 || p.H <= 0 || p.W <= 0 || (sample != 0 && sample != 1)) return -2;
    return dispatch_backproject<true>(p, eyes, sample, bvh, stream);
}

// ---------------------------------------------------------------------------------------------
// visibility hole filling (renderer_inverse.py:327-343, kernel_mode 7 => k = 3 then k = 5; A13):
//   k=3: m |= (9 * #set 8-neighbours - m) >= 3          k=5: m |= (25 * #set rim(16) - #set core(9)) >= 135
// zero padding outside the atlas.  pass 0: k=3 (src -> dst); pass 1: k=5 + AND coverage + AND alpha.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void dilate_kernel(const unsigned char* src, unsigned char* dst, int n_views, int Hh, int Ww,
                                                     int pass, const float4* rast2d, const unsigned char* alphaok) {
    const long T = (long)Hh * Ww;
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int vw = blockIdx.y;
    if (t >= T) return;
    const int y = (int)(t / Ww), x = (int)(t % Ww);
    const unsigned char* m = src + (long)vw * T;
    auto at = [&](int yy, int xx) -> int { return (yy < 0 || yy >= Hh || xx < 0 || xx >= Ww) ? 0 : (int)m[(long)yy * Ww + xx]; };
    int self = at(y, x), out;
    if (pass == 0) {
        int s = 0;
        for (int dy = -1; dy <= 1; ++dy) for (int dx = -1; dx <= 1; ++dx) if (dy || dx) s += at(y + dy, x + dx);
        out = (self || (9 * s - self) >= 3) ? 1 : 0;
    } else {
        int rim = 0, core = 0;
        for (int dy = -2; dy <= 2; ++dy) for (int dx = -2; dx <= 2; ++dx) {
            const int vv = at(y + dy, x + dx);
            if (dy == -2 || dy == 2 || dx == -2 || dx == 2) rim += vv; else core += vv;
        }
        out = (self || (25 * rim - core) >= 135) ? 1 : 0;
        const bool cov = rast2d[t].w > 0.f;
        out = (out && cov && alphaok[(long)vw * T + t]) ? 1 : 0;
    }
    dst[(long)vw * T + t] = (unsigned char)out;
}

extern "C" int utx_launch_dilate_visibility(const void* rayvis, const void* alphaok, const void* rast2d, int n_views, int Hh, int Ww,
                                            void* tmp, void* vis_out, hipStream_t stream) {
    if (n_views <= 0 || Hh <= 0 || Ww <= 0) return -2;
    const long T = (long)Hh * Ww;
    dim3 grid((unsigned)((T + 255) / 256), n_views);
    hipLaunchKernelGGL(dilate_kernel, grid, dim3(256), 0, stream, (const unsigned char*)rayvis, (unsigned char*)tmp, n_views, Hh, Ww, 0,
                       (const float4*)rast2d, (const unsigned char*)alphaok);
    hipLaunchKernelGGL(dilate_kernel, grid, dim3(256), 0, stream, (const unsigned char*)tmp, (unsigned char*)vis_out, n_views, Hh, Ww, 1,
                       (const float4*)rast2d, (const unsigned char*)alphaok);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---------------------------------------------------------------------------------------------
// priority composite (renderer_inverse.py:595-602): first view in `order` that sees the texel wins.
// A per-texel scan over <= 8 views -- no atomics needed.  winner = -1 where no view sees the texel.
// ---------------------------------------------------------------------------------------------
struct OrderArg { int v[8]; int n; };

// order [n_order <= 8] of view indices -> the kernel argument
static OrderArg order_arg(const int* order, int n_order) {
    OrderArg o; o.n = n_order;
    for (int i = 0; i < 8; ++i) o.v[i] = i < n_order ? order[i] : 0;
    return o;
}

__device__ __forceinline__ int first_visible(const unsigned char* vis, const OrderArg& ord, long T, long t) {
    for (int i = 0; i < ord.n; ++i) { const int vw = ord.v[i]; if (vis[(long)vw * T + t]) return vw; }
    return -1;
}

__global__ __launch_bounds__(256) void composite_kernel(const float* colors, const unsigned char* vis, OrderArg ord, long T,
                                                        float* atlas, signed char* winner) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    const int wv = first_visible(vis, ord, T, t);
    float c0 = 0.f, c1 = 0.f, c2 = 0.f;
    if (wv >= 0) { const float* c = colors + ((long)wv * T + t) * 3; c0 = c[0]; c1 = c[1]; c2 = c[2]; }
    atlas[3 * t] = c0; atlas[3 * t + 1] = c1; atlas[3 * t + 2] = c2;
    winner[t] = (signed char)wv;
}

extern "C" int utx_launch_composite(const float* colors, const void* vis, const int* order, int n_order, long T, float* atlas,
                                    void* winner, hipStream_t stream) {
    if (n_order <= 0 || n_order > 8 || T <= 0) return -2;
    const OrderArg o = order_arg(order, n_order);
    hipLaunchKernelGGL(composite_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, stream, colors, (const unsigned char*)vis, o, T,
                       atlas, (signed char*)winner);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// the same scan without colours (the 9-channel bake): vis [n_views][T] u8 + order -> winner [T] int8
__global__ __launch_bounds__(256) void composite_winner_kernel(const unsigned char* vis, OrderArg ord, long T, signed char* winner) {
    const long t = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= T) return;
    winner[t] = (signed char)first_visible(vis, ord, T, t);
}

extern "C" int utx_launch_composite_winner(const void* vis, int n_views, const int* order, int n_order, long T, void* winner, hipStream_t stream) {
    if (n_order <= 0 || n_order > 8 || T <= 0 || n_views <= 0) return -2;
    const OrderArg o = order_arg(order, n_order);
    for (int i = 0; i < n_order; ++i) if (o.v[i] < 0 || o.v[i] >= n_views) return -2;
    hipLaunchKernelGGL(composite_winner_kernel, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, stream, (const unsigned char*)vis, o, T, (signed char*)winner);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---------------------------------------------------------------------------------------------
// winner gather (the 9-channel bake): colour is sampled ONLY from the view that won the texel, after visibility, winner and seam -- none of which
// reads colour -- are known.  One thread per (texel, channel) of atlas [T][C]: consecutive lanes write consecutive floats (a thread per texel would
// store 4 C bytes at a stride of 4 C), and the C lanes of a texel read the same raster record, face and NDC (one request, broadcast) and adjacent
// floats of each tap.  NDC as backproject_kernel computes it; taps, weights and summation order as its SAMPLE arms, per channel, so for C = 3 the atlas
// equals utx_composite(utx_backproject) bit for bit.  images [n][H][W][C] f32; texels without a winner are written as zeros.
// ---------------------------------------------------------------------------------------------
template <int SAMPLE>
__global__ __launch_bounds__(256) void gather_winner_kernel(const float4* rast2d, const int* faces, const float* vndc, const float* images, const signed char* winner,
                                                            long T, int V, int n_views, int H, int W, int C, float* atlas) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T * C) return;
    const long t = i / C;
    const int ch = (int)(i - t * C);
    const int vw = winner[t];
    float o = 0.f;
    const float4 r = rast2d[t];
    const int id = (int)r.w - 1;
    if (vw >= 0 && vw < n_views && id >= 0) {
        const float u = r.x, v = r.y, w = sd_bary_w(u, v);
        const int f0 = faces[3 * (long)id], f1 = faces[3 * (long)id + 1], f2 = faces[3 * (long)id + 2];
        float g[2];
        texel_ndc(vndc + (long)vw * V * 2, f0, f1, f2, u, v, w, g);
        o = sample_view<SAMPLE>(images + (long)vw * H * W * C + ch, C, H, W, g[0], g[1]);
    }
    atlas[i] = o;
}

extern "C" int utx_launch_gather_winner(const float* rast2d, const int* faces, const float* vndc, const float* images, const void* winner, long T, int V, int n_views,
                                        int H, int W, int C, int sample, float* atlas, hipStream_t stream) {
    if (T <= 0 || V <= 0 || n_views <= 0 || n_views > 127 || H <= 0 || W <= 0 || C < 1 || C > 16 || (sample != 0 && sample != 1)) return -2;
    const long n = T * C;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (sample == 0) hipLaunchKernelGGL(gather_winner_kernel<0>, grid, dim3(256), 0, stream, (const float4*)rast2d, faces, vndc, images, (const signed char*)winner, T, V, n_views, H, W, C, atlas);
    else hipLaunchKernelGGL(gather_winner_kernel<1>, grid, dim3(256), 0, stream, (const float4*)rast2d, faces, vndc, images, (const signed char*)winner, T, V, n_views, H, W, C, atlas);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// Per-pixel device primitives of the geometry and shading kernels (raster.hip, gbuffer.hip, pbr.hip, backproject.hip, vertex_bake.hip, uv_bake.hip,
// sampling.hip): the barycentric interpolation of utx_interpolate, the wrap-addressed bilinear texture fetch of utx_texture_shade, the grid_sample
// (zero padding: grid_taps; reflection padding: grid_reflect_index / grid_reflect_taps) and nvdiffrast lookups of an image at an NDC coordinate, length /
// normalisation with F.normalize's eps, the overlay / blending epilogue of the two bakes (sd_bake_epilogue), and the float -> uint8 conversion.
// These kernels are held to bit-exact parity with the oracle and with each other, so each expression is written ONCE, here, with its sums in one fixed order.  Every translation unit that includes this header is compiled with
// -ffp-contract=off: each operation below is one correctly rounded fp32 operation and a value is bit-identical wherever it is computed.
#pragma once
#include <hip/hip_runtime.h>

// ---- barycentric interpolation: the raster record holds (u, v) = the weights of vertices 0 and 1
__device__ __forceinline__ float sd_bary_w(float u, float v) { return (1.0f - u) - v; }

// one channel of a per-vertex attribute (a0, a1, a2 = its values at the triangle's three vertices): utx_interpolate's expression and order
__device__ __forceinline__ float sd_interp1(float a0, float a1, float a2, float u, float v, float w) { return (a0 * u + a1 * v) + a2 * w; }

// N adjacent channels; a0, a1, a2 point at the attribute of the three vertices
template <int N>
__device__ __forceinline__ void sd_interp(const float* a0, const float* a1, const float* a2, float u, float v, float w, float* o) {
#pragma unroll
    for (int c = 0; c < N; ++c) o[c] = sd_interp1(a0[c], a1[c], a2[c], u, v, w);
}

// ---- length and normalisation
__device__ __forceinline__ float sd_dot3(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// sqrt((x*x + y*y) + z*z): torch.norm(p=2) / the length under F.normalize
__device__ __forceinline__ float sd_length3(const float p[3]) { return sqrtf(sd_dot3(p, p)); }

// F.normalize(eps=1e-12): p / max(|p|, 1e-12) with len = |p| (a NaN length takes the floor: fmaxf); o may be p
__device__ __forceinline__ void sd_normalize3(const float p[3], float len, float o[3]) {
    const float d = fmaxf(len, 1e-12f);
    o[0] = p[0] / d; o[1] = p[1] / d; o[2] = p[2] / d;
}
__device__ __forceinline__ void sd_normalize3(float v[3]) { sd_normalize3(v, sd_length3(v), v); }

// ---- bilinear texture fetch, dr.texture(filter 'linear', wrap addressing, texel centres at +0.5)
__device__ __forceinline__ int sd_wrapi(long i, int n) { i %= n; return (int)(i < 0 ? i + n : i); }

// the blend of the four texels around a sample, along x first: t00 (1 - fx) + t01 fx (fp32 in the shade kernels, fp64 in the lat-long resampling)
template <class T>
__device__ __forceinline__ T sd_bilerp(T t00, T t01, T t10, T t11, T fx, T fy) {
    const T top = t00 * ((T)1 - fx) + t01 * fx;
    const T bot = t10 * ((T)1 - fx) + t11 * fx;
    return top * ((T)1 - fy) + bot * fy;
}

// the sample (tu, tv) of a [Ht][Wt] texture: the four wrapped texel offsets (in texels) and the two blend fractions
struct SdTexTaps { long o00, o01, o10, o11; float fx, fy; };
__device__ __forceinline__ SdTexTaps sd_tex_taps(int Ht, int Wt, float tu, float tv) {
    const float x = tu * (float)Wt - 0.5f, y = tv * (float)Ht - 0.5f;
    const float x0 = floorf(x), y0 = floorf(y);
    const int ix0 = sd_wrapi((long)(int)x0, Wt), ix1 = sd_wrapi((long)(int)x0 + 1, Wt);
    const int iy0 = sd_wrapi((long)(int)y0, Ht), iy1 = sd_wrapi((long)(int)y0 + 1, Ht);
    return {(long)iy0 * Wt + ix0, (long)iy0 * Wt + ix1, (long)iy1 * Wt + ix0, (long)iy1 * Wt + ix1, x - x0, y - y0};
}
__device__ __forceinline__ void sd_tex3_blend(const float* t00, const float* t01, const float* t10, const float* t11, float fx, float fy, float o[3]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) o[k] = sd_bilerp(t00[k], t01[k], t10[k], t11[k], fx, fy);
}

// tex [Ht][Wt][3] fp32 at (tu, tv), row index growing with v
__device__ __forceinline__ void sd_tex3_wrap(const float* tex, int Ht, int Wt, float tu, float tv, float o[3]) {
    const SdTexTaps t = sd_tex_taps(Ht, Wt, tu, tv);
    sd_tex3_blend(tex + 3 * t.o00, tex + 3 * t.o01, tex + 3 * t.o10, tex + 3 * t.o11, t.fx, t.fy, o);
}
// the constant texture k of that size, sent through the same arithmetic so that it is bit-identical to a texture filled with k
__device__ __forceinline__ void sd_tex3_wrap_const(const float k[3], int Ht, int Wt, float tu, float tv, float o[3]) {
    const SdTexTaps t = sd_tex_taps(Ht, Wt, tu, tv);
    sd_tex3_blend(k, k, k, k, t.fx, t.fy, o);
}

// ---- the lookups of an image at an NDC coordinate in [-1, 1] (the views of the back-projection, the maps of utx_screen_gbuffer).
// The two lookups of a view image.  Each has ONE function for its taps and weights and ONE blend, templated on the tap type: float4 for the colour
// kernel (rgb + alpha, one 16-byte load per tap), float for the alpha plane and for one channel of a [H][W][C] image (taps `stride` = C floats apart).
//
// grid_sample(bilinear, zero padding, align_corners=False): the four tap offsets in pixels (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1), -1 for a
// tap outside the view (it reads as zero), and their weights
__device__ __forceinline__ float grid_unnormalize(float g, int size) { return ((g + 1.0f) * (float)size - 1.0f) * 0.5f; }
// the taps and weights around the pixel coordinate (ix, iy): both paddings end here
__device__ __forceinline__ void grid_taps_at(int H, int W, float ix, float iy, long o[4], float w[4]) {
    const float fx = floorf(ix), fy = floorf(iy);
    const int x0 = (int)fx, y0 = (int)fy;
    const float tx = ix - fx, ty = iy - fy;
    w[0] = (1.0f - tx) * (1.0f - ty); w[1] = tx * (1.0f - ty); w[2] = (1.0f - tx) * ty; w[3] = tx * ty;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int x = x0 + (k & 1), y = y0 + (k >> 1);
        o[k] = (x < 0 || x >= W || y < 0 || y >= H) ? -1 : (long)y * W + x;
    }
}
__device__ __forceinline__ void grid_taps(int H, int W, float gx, float gy, long o[4], float w[4]) { grid_taps_at(H, W, grid_unnormalize(gx, W), grid_unnormalize(gy, H), o, w); }
// grid_sample(bilinear, padding_mode='reflection', align_corners=False) of one axis, as torch's GridSampler.h computes the source index: unnormalise, reflect
// about [-0.5, size - 0.5] (|x + 0.5|, fmod by the span, an odd number of flips mirrors), back by -0.5, clip to [0, size - 1]: the outer half-pixel rim lands
// ON the border texel.  The parity of the flips is taken in floating point: defined for every finite g (a count past 2^24 is even; overflow and NaN end on texel 0).
__device__ __forceinline__ float grid_reflect_index(float g, int size) {
    const float span = (float)size, in = fabsf(grid_unnormalize(g, size) + 0.5f), extra = fmodf(in, span);
    const float r = fmodf(floorf(in / span), 2.0f) == 0.0f ? extra - 0.5f : (span - extra) - 0.5f;
    return fminf((float)(size - 1), fmaxf(r, 0.0f));
}
// its taps: grid_taps' outputs, so grid_tap and grid_blend serve both paddings.  x0 + 1 == W (or y0 + 1 == H) happens on the last texel only, with weight
// exactly 0: the tap is -1 and reads as zero (torch masks it out), so it adds +0.0 -- the sum's bits are those of skipping it unless the partial sum is -0.0
__device__ __forceinline__ void grid_reflect_taps(int H, int W, float gx, float gy, long o[4], float w[4]) { grid_taps_at(H, W, grid_reflect_index(gx, W), grid_reflect_index(gy, H), o, w); }
// grid_sample(nearest, zero padding, align_corners=False): the offset of the one tap, the pixel nearest to the sample with halves rounded to even
// (rintf, as torch's round), -1 outside the image
__device__ __forceinline__ long grid_nearest(int H, int W, float gx, float gy) {
    const float fx = rintf(grid_unnormalize(gx, W)), fy = rintf(grid_unnormalize(gy, H));
    if (!(fx >= 0.0f && fx < (float)W && fy >= 0.0f && fy < (float)H)) return -1;      // (a NaN coordinate is outside)
    return (long)(int)fy * W + (int)fx;
}
template <class T>
__device__ __forceinline__ T grid_tap(const T* img, long stride, long o) { return o < 0 ? T{} : img[o * stride]; }
template <class T>
__device__ __forceinline__ T grid_blend(T a, T b, T c, T e, const float w[4]) { return ((a * w[0] + b * w[1]) + c * w[2]) + e * w[3]; }

// nvdiffrast's 2-D linear lookup with the wrap boundary (indexTextureLinear + bilerp, restated): uv = ndc * 0.5 + 0.5 (two roundings, as
// ndc_2d.mul(0.5).add(0.5)), u -= floor(u), u = u * W - 0.5, i0 = floor(u), i1 = i0 + 1, f = u - i0, indices wrapped into [0, W) (the same along v with H),
// out = lerp(lerp(t00, t10, fu), lerp(t01, t11, fu), fv) with lerp(a, b, t) = a + t * (b - a).  For a finite u, u - floor(u) lies in [0, 1], so i0 lies in
// [-1, W - 1] and i1 in [0, W]: after the wrap every tap is inside the view.
// wrap_taps: the four tap offsets (in pixels) and the two lerp fractions; false for a non-finite coordinate (it samples zero)
__device__ __forceinline__ bool wrap_taps(int H, int W, float gx, float gy, long& o00, long& o10, long& o01, long& o11, float& fu, float& fv) {
    if (!isfinite(gx) || !isfinite(gy)) return false;
    float su = gx * 0.5f + 0.5f, sv = gy * 0.5f + 0.5f;
    su = su - floorf(su); sv = sv - floorf(sv);
    su = su * (float)W - 0.5f; sv = sv * (float)H - 0.5f;
    const float fu0 = floorf(su), fv0 = floorf(sv);
    int iu0 = (int)fu0, iv0 = (int)fv0, iu1 = iu0 + 1, iv1 = iv0 + 1;
    fu = su - fu0; fv = sv - fv0;
    if (iu0 < 0) iu0 += W;
    if (iv0 < 0) iv0 += H;
    if (iu1 >= W) iu1 -= W;
    if (iv1 >= H) iv1 -= H;
    o00 = (long)iv0 * W + iu0; o10 = (long)iv0 * W + iu1; o01 = (long)iv1 * W + iu0; o11 = (long)iv1 * W + iu1;
    return true;
}
template <class T>
__device__ __forceinline__ T lerp_nv(T a, T b, float t) { return a + (b - a) * t; }
template <class T>
__device__ __forceinline__ T wrap_blend(T t00, T t10, T t01, T t11, float fu, float fv) { return lerp_nv(lerp_nv(t00, t10, fu), lerp_nv(t01, t11, fu), fv); }

// SAMPLE 0: grid_sample, 1: the wrap lookup, of img [H][W] texels of type T, `stride` T's apart, at the NDC (gx, gy)
template <int SAMPLE, class T>
__device__ __forceinline__ T sample_view(const T* img, long stride, int H, int W, float gx, float gy) {
    if constexpr (SAMPLE == 0) {
        long o[4]; float w[4];
        grid_taps(H, W, gx, gy, o, w);
        return grid_blend(grid_tap(img, stride, o[0]), grid_tap(img, stride, o[1]), grid_tap(img, stride, o[2]), grid_tap(img, stride, o[3]), w);
    } else {
        long o00, o10, o01, o11; float fu, fv;
        if (!wrap_taps(H, W, gx, gy, o00, o10, o01, o11, fu, fv)) return T{};
        return wrap_blend(img[o00 * stride], img[o10 * stride], img[o01 * stride], img[o11 * stride], fu, fv);
    }
}

// ---- one texel of the atlas raster as one view sees it (utx_uv_project and utx_uv_bake; render/nvdiffrast/renderer_base.py:513-547 of the reference)
// r: the texel's record of the atlas raster (u, v, z/w, triangle id + 1); face_mask, v_ndc: the view's rows of [B][F] and [B][V][2].
//   vis   the texel lies on a face the view sees
//   g     vis ? the view's NDC of the texel's surface point : (-1, -1)
struct SdUvView { bool vis; float g[2]; };
__device__ __forceinline__ SdUvView sd_uv_view(float4 r, const int* tri, long F, const unsigned char* face_mask, const float* v_ndc) {
    SdUvView o;
    const int id = (int)r.w - 1;
    o.vis = id >= 0 && id < F && face_mask[id] != 0;
    o.g[0] = -1.0f; o.g[1] = -1.0f;
    if (o.vis) {
        const float u = r.x, v = r.y, w = sd_bary_w(u, v);
        sd_interp<2>(v_ndc + 2 * (long)tri[3 * id + 0], v_ndc + 2 * (long)tri[3 * id + 1], v_ndc + 2 * (long)tri[3 * id + 2], u, v, w, o.g);
    }
    return o;
}
// grid_sample(nearest, zero padding) of the view's coverage rast_map.w > 0 at (gx, gy); rast_map: the view's [Hm][Wm][4] raster, only .w is read
__device__ __forceinline__ bool sd_view_coverage(const float* rast_map, int Hm, int Wm, float gx, float gy) {
    const long o = grid_nearest(Hm, Wm, gx, gy);
    return o >= 0 && rast_map[4 * o + 3] > 0.0f;
}

// ---- the overlay / blending epilogue of the two bakes (remapping_vertex_color :326-337, remapping_uv_texture :205-217 of the reference), in place on acc:
// acc / wa where wa > overlay_conf; then, where wa <= blending_conf, blending 1 (soft): (base * (conf - wa) + acc) / conf, 2 (hard): base, 0: nothing
template <int N>
__device__ __forceinline__ void sd_bake_epilogue(float* acc, float wa, const float* base, float overlay_conf, int blending, float blending_conf) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const float a = wa > overlay_conf ? acc[k] / wa : acc[k];
        acc[k] = !(blending && wa <= blending_conf) ? a : blending == 1 ? (base[k] * (blending_conf - wa) + a) / blending_conf : base[k];
    }
}

// ---- float frame -> uint8: clamp(0, 1) * 255, truncated (astype(uint8))
__device__ __forceinline__ unsigned char sd_to_u8(float c) { return (unsigned char)(fminf(fmaxf(c, 0.f), 1.f) * 255.0f); }

// Per-pixel device primitives of the geometry and shading kernels (raster.hip, gbuffer.hip, pbr.hip, backproject.hip): the barycentric
// interpolation of utx_interpolate, the wrap-addressed bilinear texture fetch of utx_texture_shade, length / normalisation with F.normalize's
// eps, and the float -> uint8 conversion.  These kernels are held to bit-exact parity with the oracle and with each other, so each expression
// is written ONCE, here, with its sums in one fixed order.  Every translation unit that includes this header is compiled with
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

// ---- float frame -> uint8: clamp(0, 1) * 255, truncated (astype(uint8))
__device__ __forceinline__ unsigned char sd_to_u8(float c) { return (unsigned char)(fminf(fmaxf(c, 0.f), 1.f) * 255.0f); }

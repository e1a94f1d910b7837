// Device routines shared by the screen-space geometry buffers (raster.hip: gbuffer_shade_kernel, gbuffer_range_kernel, camera_normals_kernel)
// and the atlas-space ones (uv_gbuffer.hip): the interpolation of utx_interpolate, (a0*u + a1*v) + a2*w, and F.normalize with its eps, each
// with its sums in one fixed order.  Both translation units are compiled with -ffp-contract=off, so every operation below is one correctly
// rounded fp32 operation and the value is bit-identical to interpolate_kernel's wherever it is computed.
#pragma once
#include <hip/hip_runtime.h>

// keeps each product a scalar of its own: left alone, hipcc pairs two products of a sum into one packed multiply and adds its halves with a
// cross-half packed add, the instruction pair tests/test_asm_hazards_cpu.py bans from every listing (unitex_amd/csrc/build.py, NO_PK).  No code is emitted.
// Why not NO_PK on raster.hip, the project's usual answer: the flag is per translation unit and would regenerate the rasteriser, utx_interpolate and
// texture_shade_kernel, whose listings are clean today and whose speed and bit-exact results other tests and the rgb turntable rest on.  The audit
// reads every listing on every run, so a compiler that stops honouring the barrier is caught there, and NO_PK for the file remains the fallback.
// A translation unit that IS built with NO_PK defines UTX_TU_NO_PACKED_FP32 before including this header: no packed fp32 can form there, so the
// barrier is not needed and gb_scalar is the identity (uv_gbuffer.hip: no inline assembly of any kind in that file).
#ifdef UTX_TU_NO_PACKED_FP32
__device__ __forceinline__ float gb_scalar(float x) { return x; }
#else
__device__ __forceinline__ float gb_scalar(float x) { asm volatile("" : "+v"(x)); return x; }
#endif

__device__ __forceinline__ float gb_dot3(float x0, float y0, float x1, float y1, float x2, float y2) {
    return (gb_scalar(x0 * y0) + gb_scalar(x1 * y1)) + gb_scalar(x2 * y2);
}

// three channels of a per-vertex attribute at the barycentrics (u, v, w = (1 - u) - v) of a covered pixel; a0, a1, a2 point at the attribute of
// the triangle's three vertices: utx_interpolate's expression and order
__device__ __forceinline__ void gb_interp3(const float* a0, const float* a1, const float* a2, float u, float v, float w, float p[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) p[c] = gb_dot3(a0[c], u, a1[c], v, a2[c], w);
}

// sqrt((x*x + y*y) + z*z): torch.norm(p=2) / the length under F.normalize, sums in this order
__device__ __forceinline__ float gb_length3(const float p[3]) { return sqrtf(gb_dot3(p[0], p[0], p[1], p[1], p[2], p[2])); }

// F.normalize(eps=1e-12): p / max(|p|, 1e-12)
__device__ __forceinline__ void gb_normalize3(const float p[3], float len, float o[3]) {
    const float d = fmaxf(len, 1e-12f);
    o[0] = p[0] / d; o[1] = p[1] / d; o[2] = p[2] / d;
}

// Sliced optimal-transport colour transfer on the device (D. Coeurjolly's OTColorTransfer as the reference's image/color_transfer_ot.py CTSOT states it): fp32,
// wave64, plain C++.  Two entry points (DESIGN 8 "Colour transfer"):
//   utx_color_transfer_ot   the whole solver loop on one stream: per step and batch a projection onto the batch's direction, two rocPRIM radix sorts, the
//                           displacement of equally ranked projections scattered into the running advect, and once per step the update; no read-back
//   utx_bilateral_filter    the regulariser: a joint bilateral filter with a circular window of up to UTX_BILATERAL_RADIUS_MAX, through an LDS tile
// Built with -ffp-contract=off: every product and sum below is rounded on its own, in the order written, which is the order the float32 restatement
// (tests/support/color_transfer_ref.py) follows; the OT loop is pinned BIT FOR BIT by the reference's own output (tests/golden/g26_color_transfer_ot.npz).
//
// The OT loop.  cur = src.  For step s and batch b with d = dirs[s B + b]:
//   p(x) = ((x0 d0 + x1 d1) + x2 d2) + x3 d3 over the C channels; ps = p(cur[i]), pt = p(dst[i])
//   key(f) = bits(f) with the sign bit set for a non-negative f and all bits inverted for a negative one: unsigned order = the total order of the
//            float32 bit patterns, -0 before +0
//   (ks, id) = the source keys with their pixel ids, sorted; kt = the target keys, sorted.  The radix sort is STABLE: equal keys keep ascending pixel ids,
//            the library's rule where numpy's argsort leaves the order of ties open
//   advect[id[r]][c] = advect[id[r]][c] + (f(kt[r]) - f(ks[r])) * d[c]      in batch order; ids are a permutation, so no two threads share a row
// and after the last batch cur[i][c] = cur[i][c] + advect[i][c] / float(B) (a true division), advect = 0.
#include "common.h"
#include "kernels.h"
#include <cstring>
#include <string.h>
#include <rocprim/rocprim.hpp>

__device__ __forceinline__ unsigned ct_key(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ct_unkey(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

template <int C>
__device__ __forceinline__ float ct_project(const float* row, const float* d) {
    float p = row[0] * d[0];
#pragma unroll
    for (int c = 1; c < C; ++c) p = p + row[c] * d[c];
    return p;
}
// one thread per pixel: both projections as keys, and the identity permutation the pair sort carries
template <int C>
__global__ __launch_bounds__(256) void ct_project_kernel(const float* cur, const float* dst, const float* dir, long N, unsigned* ks, unsigned* kt, unsigned* id) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float d[C];
#pragma unroll
    for (int c = 0; c < C; ++c) d[c] = dir[c];
    ks[i] = ct_key(ct_project<C>(cur + i * C, d));
    kt[i] = ct_key(ct_project<C>(dst + i * C, d));
    id[i] = (unsigned)i;
}
// one thread per rank
template <int C>
__global__ __launch_bounds__(256) void ct_advect_kernel(const unsigned* ks, const unsigned* kt, const unsigned* id, const float* dir, long N, float* advect) {
    const long r = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= N) return;
    const float a = ct_unkey(kt[r]) - ct_unkey(ks[r]);
    const unsigned i = id[r];
    if (i >= (unsigned long)N) return;      // cannot happen with a permutation; keeps a store inside the buffer whatever the sort returned
    float* row = advect + (long)i * C;
#pragma unroll
    for (int c = 0; c < C; ++c) row[c] = row[c] + a * dir[c];
}
// one thread per value
__global__ __launch_bounds__(256) void ct_update_kernel(float* cur, float* advect, long n, float batch) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    cur[i] = cur[i] + advect[i] / batch;
    advect[i] = 0.0f;
}

static inline size_t ct_align(size_t v) { return (v + 255) & ~(size_t)255; }
static size_t ct_sort_bytes(long N) {
    size_t a = 0, b = 0;
    (void)rocprim::radix_sort_pairs(nullptr, a, (unsigned*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr, (unsigned*)nullptr, (size_t)N, 0, 32, (hipStream_t)0);
    (void)rocprim::radix_sort_keys(nullptr, b, (unsigned*)nullptr, (unsigned*)nullptr, (size_t)N, 0, 32, (hipStream_t)0);
    return a > b ? a : b;
}
// six arrays of N words (keys, sorted keys, ids, sorted ids), the advect image, rocPRIM's temporary storage; every part on a 256-byte boundary
extern "C" size_t utx_color_transfer_ot_workspace_bytes_impl(long N, int C) {
    if (N < 1 || N >= UTX_COLOR_TRANSFER_N_MAX || C < 1 || C > 4) return 0;
    return 6 * ct_align((size_t)N * 4) + ct_align((size_t)N * C * 4) + ct_align(ct_sort_bytes(N)) + 256;
}

// arguments checked by utx_color_transfer_ot (capi.cpp): N in 1 .. 2^30 - 1, C in 1 .. 4, steps >= 0, batch >= 1, out apart from src and dst
extern "C" int utx_launch_color_transfer_ot(const float* src, const float* dst, const float* dirs, long N, int C, int steps, int batch, float* out, void* work,
                                            size_t work_bytes, hipStream_t stream) {
    if (hipMemcpyAsync(out, src, (size_t)N * C * 4, hipMemcpyDeviceToDevice, stream) != hipSuccess) return -7;
    if (steps == 0) return 0;
    if (work_bytes < utx_color_transfer_ot_workspace_bytes_impl(N, C)) return -2;
    const size_t words = ct_align((size_t)N * 4);
    char* w = (char*)(((uintptr_t)work + 255) & ~(uintptr_t)255);
    unsigned* ks = (unsigned*)w; unsigned* ks_s = (unsigned*)(w + words);
    unsigned* kt = (unsigned*)(w + 2 * words); unsigned* kt_s = (unsigned*)(w + 3 * words);
    unsigned* id = (unsigned*)(w + 4 * words); unsigned* id_s = (unsigned*)(w + 5 * words);
    float* advect = (float*)(w + 6 * words);
    void* tmp = w + 6 * words + ct_align((size_t)N * C * 4);
    size_t tmp_bytes = ct_sort_bytes(N);
    if (hipMemsetAsync(advect, 0, (size_t)N * C * 4, stream) != hipSuccess) return -7;
    const dim3 grid((unsigned)((N + 255) / 256)), block(256);
    const long n = N * C;
    for (int s = 0; s < steps; ++s) {
        for (int b = 0; b < batch; ++b) {
            const float* d = dirs + ((long)s * batch + b) * C;
            switch (C) {
                case 1: hipLaunchKernelGGL(ct_project_kernel<1>, grid, block, 0, stream, (const float*)out, dst, d, N, ks, kt, id); break;
                case 2: hipLaunchKernelGGL(ct_project_kernel<2>, grid, block, 0, stream, (const float*)out, dst, d, N, ks, kt, id); break;
                case 3: hipLaunchKernelGGL(ct_project_kernel<3>, grid, block, 0, stream, (const float*)out, dst, d, N, ks, kt, id); break;
                default: hipLaunchKernelGGL(ct_project_kernel<4>, grid, block, 0, stream, (const float*)out, dst, d, N, ks, kt, id); break;
            }
            if (rocprim::radix_sort_pairs(tmp, tmp_bytes, ks, ks_s, id, id_s, (size_t)N, 0, 32, stream) != hipSuccess) return -7;
            if (rocprim::radix_sort_keys(tmp, tmp_bytes, kt, kt_s, (size_t)N, 0, 32, stream) != hipSuccess) return -7;
            switch (C) {
                case 1: hipLaunchKernelGGL(ct_advect_kernel<1>, grid, block, 0, stream, (const unsigned*)ks_s, (const unsigned*)kt_s, (const unsigned*)id_s, d, N, advect); break;
                case 2: hipLaunchKernelGGL(ct_advect_kernel<2>, grid, block, 0, stream, (const unsigned*)ks_s, (const unsigned*)kt_s, (const unsigned*)id_s, d, N, advect); break;
                case 3: hipLaunchKernelGGL(ct_advect_kernel<3>, grid, block, 0, stream, (const unsigned*)ks_s, (const unsigned*)kt_s, (const unsigned*)id_s, d, N, advect); break;
                default: hipLaunchKernelGGL(ct_advect_kernel<4>, grid, block, 0, stream, (const unsigned*)ks_s, (const unsigned*)kt_s, (const unsigned*)id_s, d, N, advect); break;
            }
        }
        hipLaunchKernelGGL(ct_update_kernel, dim3((unsigned)((n + 255) / 256)), block, 0, stream, out, advect, n, (float)batch);
    }
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---- joint bilateral filter
// The rule is this library's, on OpenCV's documented parameters of cv2.bilateralFilter(img, d = 0, sigmaColor, sigmaSpace) [3p]: radius r (the caller's
// max(1, rint(1.5 sigmaSpace))), the circular support dx^2 + dy^2 <= r^2, space weights from the caller's table ws[|dy|][|dx|] ((r + 1)^2 floats), colour weight
// expf(((sum_c |v_c(q) - v_c(p)|)^2) * coef) with coef = -1 / (2 sigmaColor^2), reflect-101 borders applied repeatedly (an axis of length 1 maps to index 0).
// Per pixel, q row-major over the window (dy outer, dx inner, ascending), one running sum per channel and one for the weights:
//   L1 = (|D0| + |D1|) + |D2|;  w = ws * expf((L1 * L1) * coef);  num_c = num_c + w * v_c(q);  den = den + w;  out_c = num_c / den
// The centre tap has w = 1, so den >= 1.
#define BIL_TILE 16      // 16 x 16 pixels per 256-thread block: a wave is four rows of 16

__device__ __forceinline__ int bil_reflect101(int p, int n) {
    if (n == 1) return 0;
    const int period = 2 * (n - 1);
    p %= period;
    if (p < 0) p += period;
    return p < n ? p : period - p;
}
// One thread per pixel.  The block stages its tile plus a halo of r, C planes of S^2 floats with S = 16 + 2 r, and the space table in LDS (one dynamic array:
// at r = 24 and C = 3, 64^2 x 12 + 25^2 x 4 = 51652 bytes), so every tap comes from LDS: lanes of a row read consecutive words.
template <int C>
__global__ __launch_bounds__(256) void bilateral_kernel(const float* img, int H, int W, int r, const float* ws, float coef, float* out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char bil_smem[];
    const int S = BIL_TILE + 2 * r, n = S * S, T = r + 1;
    float* sV = (float*)bil_smem;
    float* sW = sV + (size_t)C * n;
    const int tx = threadIdx.x & (BIL_TILE - 1), ty = threadIdx.x >> 4;
    const int x0 = blockIdx.x * BIL_TILE, y0 = blockIdx.y * BIL_TILE;
    for (int i = threadIdx.x; i < n; i += 256) {
        const int gx = bil_reflect101(x0 - r + i % S, W), gy = bil_reflect101(y0 - r + i / S, H);
        const float* px = img + ((long)gy * W + gx) * C;
#pragma unroll
        for (int c = 0; c < C; ++c) sV[c * n + i] = px[c];
    }
    for (int i = threadIdx.x; i < T * T; i += 256) sW[i] = ws[i];
    __syncthreads();
    const int x = x0 + tx, y = y0 + ty;
    if (x >= W || y >= H) return;
    const int lp = (ty + r) * S + tx + r;
    float v0[C], num[C], den = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) { v0[c] = sV[c * n + lp]; num[c] = 0.0f; }
    const int r2 = r * r;
    for (int dy = -r; dy <= r; ++dy) {
        const int ady = dy < 0 ? -dy : dy, rest = r2 - dy * dy;
        int hw = (int)sqrtf((float)rest);      // the row's half width: the largest hw with hw^2 <= r^2 - dy^2
        while (hw * hw > rest) --hw;
        while ((hw + 1) * (hw + 1) <= rest) ++hw;
        const float* wrow = sW + ady * T;
        const int lrow = lp + dy * S;
        for (int dx = -hw; dx <= hw; ++dx) {
            const int lq = lrow + dx;
            float v[C];
#pragma unroll
            for (int c = 0; c < C; ++c) v[c] = sV[c * n + lq];
            float l1 = fabsf(v[0] - v0[0]);
#pragma unroll
            for (int c = 1; c < C; ++c) l1 = l1 + fabsf(v[c] - v0[c]);
            const float w = wrow[dx < 0 ? -dx : dx] * expf((l1 * l1) * coef);
#pragma unroll
            for (int c = 0; c < C; ++c) num[c] = num[c] + w * v[c];
            den = den + w;
        }
    }
    float* o = out + ((long)y * W + x) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = num[c] / den;
}
extern "C" size_t utx_bilateral_lds_bytes_impl(int r, int C) {
    const size_t S = BIL_TILE + 2 * (size_t)r;
    return S * S * C * 4 + (size_t)(r + 1) * (r + 1) * 4;
}
// arguments checked by utx_bilateral_filter (capi.cpp): H, W >= 1, H W < 2^30, C 1 or 3, r in 1 .. UTX_BILATERAL_RADIUS_MAX
extern "C" int utx_launch_bilateral_filter(const float* img, int H, int W, int C, int r, const float* ws, float coef, float* out, hipStream_t stream) {
    const size_t lds = utx_bilateral_lds_bytes_impl(r, C);
    if (lds > 65536) return -2;      // what a launch gets without asking for more; UTX_BILATERAL_RADIUS_MAX keeps every accepted call below it
    const dim3 grid((unsigned)((W + BIL_TILE - 1) / BIL_TILE), (unsigned)((H + BIL_TILE - 1) / BIL_TILE));
    if (C == 1) hipLaunchKernelGGL(bilateral_kernel<1>, grid, dim3(256), lds, stream, img, H, W, r, ws, coef, out);
    else if (C == 3) hipLaunchKernelGGL(bilateral_kernel<3>, grid, dim3(256), lds, stream, img, H, W, r, ws, coef, out);
    else return -2;
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

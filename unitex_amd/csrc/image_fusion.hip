// Poisson image fusion (gradient-domain blending of src into dst under a mask; TextureTools/texturetools/image/image_fusion.py of the reference, which calls
// OpenCV's seamlessClone(NORMAL_CLONE) [3p] on the host).  The rule is this library's, written out in DESIGN 8 "Poisson image fusion" and restated in float64 in
// tests/support/image_fusion_ref.py.  fp32, wave64, plain C++, vector stores only; no atomics on the solution and no block waits for another, so a run is
// bit-reproducible.  Built with -ffp-contract=off.
//   utx_mask_morph     grey erosion / dilation of a uint8 mask by an n x n box, two separable passes
//   utx_mask_bbox      the tight bounding rectangle of mask > 0 (integer max reduction; the host reads the 16 bytes back to size the levels)
//   utx_image_fusion   fusion_rhs_kernel (one launch: the source zeroed outside the mask, the 3-fold 3 x 3 erosion, the gradients, the mixed divergence, all 3
//                      channels), a fixed number of multigrid V-cycles on the correction u = I - dst (three channels in the same launches), fusion_finish_kernel
#include "common.h"
#include "kernels.h"

typedef unsigned char u8;

// ---- morphology.  One thread per pixel and pass; the box covers the offsets -a .. k - 1 - a (a = k / 2); taps outside the image are left out.
__global__ __launch_bounds__(256) void morph_pass_kernel(const u8* in, u8* out, int H, int W, int k, int a, int erode, int horizontal) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)H * W) return;
    const int y = (int)(i / W), x = (int)(i % W);
    int v = erode ? 255 : 0;
    for (int d = -a; d <= k - 1 - a; ++d) {
        const int qx = horizontal ? x + d : x, qy = horizontal ? y : y + d;
        if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
        const int t = in[(long)qy * W + qx];
        v = erode ? min(v, t) : max(v, t);
    }
    out[i] = (u8)v;
}

extern "C" int utx_launch_mask_morph(const u8* mask_in, int H, int W, int n, u8* tmp, u8* mask_out, hipStream_t stream) {
    const int k = n > 0 ? n : -n, erode = n > 0;
    const unsigned blocks = (unsigned)(((long)H * W + 255) / 256);
    hipLaunchKernelGGL(morph_pass_kernel, dim3(blocks), dim3(256), 0, stream, mask_in, tmp, H, W, k, k / 2, erode, 1);
    hipLaunchKernelGGL(morph_pass_kernel, dim3(blocks), dim3(256), 0, stream, (const u8*)tmp, mask_out, H, W, k, k / 2, erode, 0);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---- bounding rectangle.  enc[4] starts at -1 and takes max(W - 1 - x), max(H - 1 - y), max(x), max(y) over mask > 0: integer maxima, so the order of the
// atomics does not matter.  bbox_finish_kernel turns them into (x1, y1, w, h), zeros for an empty mask.
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o, 64));
    return v;
}
__global__ __launch_bounds__(256) void bbox_kernel(const u8* mask, int H, int W, int* enc) {
    const long total = (long)H * W, stride = (long)gridDim.x * blockDim.x;
    int m0 = -1, m1 = -1, m2 = -1, m3 = -1;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        if (mask[i] == 0) continue;
        const int y = (int)(i / W), x = (int)(i % W);
        m0 = max(m0, W - 1 - x); m1 = max(m1, H - 1 - y); m2 = max(m2, x); m3 = max(m3, y);
    }
    m0 = wave_max_i(m0); m1 = wave_max_i(m1); m2 = wave_max_i(m2); m3 = wave_max_i(m3);
    if ((threadIdx.x & (UTX_WAVE - 1)) == 0 && m2 >= 0) {
        atomicMax(enc + 0, m0); atomicMax(enc + 1, m1); atomicMax(enc + 2, m2); atomicMax(enc + 3, m3);
    }
}
__global__ void bbox_finish_kernel(int* enc, int H, int W) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const int e0 = enc[0], e1 = enc[1], e2 = enc[2], e3 = enc[3];
    if (e2 < 0) { enc[0] = 0; enc[1] = 0; enc[2] = 0; enc[3] = 0; return; }
    const int x1 = W - 1 - e0, y1 = H - 1 - e1;
    enc[0] = x1; enc[1] = y1; enc[2] = e2 - x1 + 1; enc[3] = e3 - y1 + 1;
}

extern "C" int utx_launch_mask_bbox(const u8* mask, int H, int W, int* rect, hipStream_t stream) {
    if (hipMemsetAsync(rect, 0xFF, 4 * sizeof(int), stream) != hipSuccess) return -4;
    const long total = (long)H * W;
    const unsigned blocks = (unsigned)((total + 256 * 16 - 1) / (256 * 16));
    hipLaunchKernelGGL(bbox_kernel, dim3(blocks < 1 ? 1 : (blocks > 4096 ? 4096 : blocks)), dim3(256), 0, stream, mask, H, W, rect);
    hipLaunchKernelGGL(bbox_finish_kernel, dim3(1), dim3(64), 0, stream, rect, H, W);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---- the right-hand side.  One thread per interior pixel (ix, iy) of the rectangle R = (x1, y1, w, h), i.e. rectangle pixel (rx, ry) = (ix + 1, iy + 1).
//   g   = (mask > 0 ? src : 0) - dst                                      integers, exact
//   m   = the minimum of mask over the 7 x 7 window clipped to R, / 255   (three 3 x 3 erosions with the pixels outside R left out)
//   f   = (m(rx, ry) (g(rx+1) - g(rx)) - m(rx-1, ry) (g(rx) - g(rx-1))) + (m(rx, ry) (g(ry+1) - g(ry)) - m(rx, ry-1) (g(ry) - g(ry-1)))
// The solver holds 4 u - (sum of the four neighbours) = b, so b = -f; u starts at zero.  Planar: b, u [3][ny][nx].
struct FusionImage { const u8* src; const u8* dst; const u8* mask; int H, W, x1, y1, w, h; };

__global__ __launch_bounds__(256) void fusion_rhs_kernel(const FusionImage p, float* b, float* u) {
    const int nx = p.w - 2, ny = p.h - 2;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)nx * ny) return;
    const int iy = (int)(i / nx), ix = (int)(i % nx), rx = ix + 1, ry = iy + 1;
    int m0 = 255, ml = 255, mu = 255;
    for (int wy = ry - 4; wy <= ry + 3; ++wy) {
        if (wy < 0 || wy >= p.h) continue;
        for (int wx = rx - 4; wx <= rx + 3; ++wx) {
            if (wx < 0 || wx >= p.w) continue;
            const int t = p.mask[(long)(p.y1 + wy) * p.W + p.x1 + wx];
            if (wx >= rx - 3 && wy >= ry - 3) m0 = min(m0, t);
            if (wx <= rx + 2 && wy >= ry - 3) ml = min(ml, t);
            if (wx >= rx - 3 && wy <= ry + 2) mu = min(mu, t);
        }
    }
    const float f0 = (float)m0 / 255.0f, fl = (float)ml / 255.0f, fu = (float)mu / 255.0f;
    const long pc = (long)(p.y1 + ry) * p.W + p.x1 + rx;
    const long off[5] = {pc, pc + 1, pc - 1, pc + p.W, pc - p.W};      // centre, right, left, down, up: all inside R
    bool on[5];
#pragma unroll
    for (int k = 0; k < 5; ++k) on[k] = p.mask[off[k]] != 0;
    const long plane = (long)nx * ny;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float g[5];
#pragma unroll
        for (int k = 0; k < 5; ++k) g[k] = (float)((on[k] ? (int)p.src[3 * off[k] + c] : 0) - (int)p.dst[3 * off[k] + c]);
        const float f = (f0 * (g[1] - g[0]) - fl * (g[0] - g[2])) + (f0 * (g[3] - g[0]) - fu * (g[0] - g[4]));
        b[c * plane + i] = -f;
        u[c * plane + i] = 0.0f;
    }
}

// ---- geometric multigrid on  (4 + ex + ey) u - (left + right + up + down) = b  with zero values outside the grid.
// ex = ax on the last column, ey = ay on the last row, zero elsewhere.  On the finest level ax = ay = 0: the exact 5-point system, whose residual every cycle
// iterates on.  A coarse level keeps every second point (the odd indices), so its last point lies s / (1 + a) of its own spacing s from the rectangle's ring
// instead of s; the ghost value -a u_last beyond it puts the zero of the linear extension on the ring (a = 0 for a size 2^k - 1).  This only shapes the coarse
// correction: the result's accuracy is the fine level's.
#define MG_TX 64
#define MG_TY 16
#define MG_COARSE_SWEEPS 32
#define MG_MAX_LEVELS 32

// one red-black Gauss-Seidel sweep (red = even x + y first), uin -> uout.  A block loads its 64 x 16 tile with a halo of 2 into LDS, updates the red points of the
// tile and a halo of 1, then the black points of the tile: bit-identical to a sweep over the whole grid, since a red update reads black values only.
__global__ __launch_bounds__(256) void mg_smooth_kernel(const float* uin, float* uout, const float* b, int nx, int ny, float ax, float ay) {
    __shared__ float t[MG_TY + 4][MG_TX + 4 + 1];
    const long plane = (long)nx * ny * blockIdx.z;
    uin += plane; uout += plane; b += plane;
    const int x0 = blockIdx.x * MG_TX, y0 = blockIdx.y * MG_TY, tid = threadIdx.x;
    for (int i = tid; i < (MG_TY + 4) * (MG_TX + 4); i += 256) {
        const int ly = i / (MG_TX + 4), lx = i % (MG_TX + 4), gx = x0 + lx - 2, gy = y0 + ly - 2;
        t[ly][lx] = (gx >= 0 && gx < nx && gy >= 0 && gy < ny) ? uin[(long)gy * nx + gx] : 0.0f;
    }
    __syncthreads();
    for (int i = tid; i < (MG_TY + 2) * (MG_TX + 2); i += 256) {
        const int ly = 1 + i / (MG_TX + 2), lx = 1 + i % (MG_TX + 2), gx = x0 + lx - 2, gy = y0 + ly - 2;
        if (gx < 0 || gx >= nx || gy < 0 || gy >= ny || ((gx + gy) & 1) != 0) continue;
        const float d = (4.0f + (gx == nx - 1 ? ax : 0.0f)) + (gy == ny - 1 ? ay : 0.0f);
        t[ly][lx] = (b[(long)gy * nx + gx] + ((t[ly][lx - 1] + t[ly][lx + 1]) + (t[ly - 1][lx] + t[ly + 1][lx]))) / d;
    }
    __syncthreads();
    for (int i = tid; i < MG_TY * MG_TX; i += 256) {
        const int ly = 2 + i / MG_TX, lx = 2 + i % MG_TX, gx = x0 + lx - 2, gy = y0 + ly - 2;
        if (gx >= nx || gy >= ny || ((gx + gy) & 1) != 1) continue;
        const float d = (4.0f + (gx == nx - 1 ? ax : 0.0f)) + (gy == ny - 1 ? ay : 0.0f);
        t[ly][lx] = (b[(long)gy * nx + gx] + ((t[ly][lx - 1] + t[ly][lx + 1]) + (t[ly - 1][lx] + t[ly + 1][lx]))) / d;
    }
    __syncthreads();
    for (int i = tid; i < MG_TY * MG_TX; i += 256) {
        const int ly = 2 + i / MG_TX, lx = 2 + i % MG_TX, gx = x0 + lx - 2, gy = y0 + ly - 2;
        if (gx < nx && gy < ny) uout[(long)gy * nx + gx] = t[ly][lx];
    }
}

// the residual r = b - ((4 + ex + ey) u - neighbours) of the fine level, full-weighting restriction onto the coarse point (jx, jy) = fine (2 jx + 1, 2 jy + 1):
// bc = 4 * (1/16) (1 2 1; 2 4 2; 1 2 1) r  (the coarse operator is the same stencil at twice the spacing); a fine point outside the grid has r = 0.  uc = 0.
__device__ __forceinline__ float mg_at(const float* u, int nx, int ny, int x, int y) {
    return (x >= 0 && x < nx && y >= 0 && y < ny) ? u[(long)y * nx + x] : 0.0f;
}
__device__ __forceinline__ float mg_residual(const float* u, const float* b, int nx, int ny, float ax, float ay, int x, int y) {
    if (x >= nx || y >= ny) return 0.0f;
    const float d = (4.0f + (x == nx - 1 ? ax : 0.0f)) + (y == ny - 1 ? ay : 0.0f);
    const float nb = (mg_at(u, nx, ny, x - 1, y) + mg_at(u, nx, ny, x + 1, y)) + (mg_at(u, nx, ny, x, y - 1) + mg_at(u, nx, ny, x, y + 1));
    return b[(long)y * nx + x] - (d * u[(long)y * nx + x] - nb);
}
__global__ __launch_bounds__(256) void mg_restrict_kernel(const float* u, const float* b, int nx, int ny, float ax, float ay, float* bc, float* uc, int ncx, int ncy) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)ncx * ncy) return;
    const long plane = (long)nx * ny * blockIdx.z, cplane = (long)ncx * ncy * blockIdx.z;
    u += plane; b += plane;
    const int jy = (int)(i / ncx), jx = (int)(i % ncx), cx = 2 * jx + 1, cy = 2 * jy + 1;
    float r[3][3];
#pragma unroll
    for (int dy = 0; dy < 3; ++dy)
#pragma unroll
        for (int dx = 0; dx < 3; ++dx) r[dy][dx] = mg_residual(u, b, nx, ny, ax, ay, cx + dx - 1, cy + dy - 1);
    const float corners = (r[0][0] + r[0][2]) + (r[2][0] + r[2][2]), edges = (r[0][1] + r[2][1]) + (r[1][0] + r[1][2]);
    bc[cplane + i] = 0.25f * ((corners + 2.0f * edges) + 4.0f * r[1][1]);
    uc[cplane + i] = 0.0f;
}

// u += the bilinear interpolation of the coarse correction.  Coarse index -1 reads 0, index nc reads the ghost -a uc[nc - 1] (both axes: the product).
__device__ __forceinline__ float mg_coarse_at(const float* uc, int ncx, int ncy, float acx, float acy, int jx, int jy) {
    if (jx < 0 || jy < 0) return 0.0f;
    float s = 1.0f;
    if (jx >= ncx) { jx = ncx - 1; s = -acx; }
    if (jy >= ncy) { jy = ncy - 1; s = s * -acy; }
    return s * uc[(long)jy * ncx + jx];
}
__global__ __launch_bounds__(256) void mg_prolong_kernel(float* u, int nx, int ny, const float* uc, int ncx, int ncy, float acx, float acy) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)nx * ny) return;
    u += (long)nx * ny * blockIdx.z; uc += (long)ncx * ncy * blockIdx.z;
    const int y = (int)(i / nx), x = (int)(i % nx);
    const int jx0 = (x & 1) ? (x - 1) / 2 : x / 2 - 1, jx1 = (x & 1) ? (x - 1) / 2 : x / 2;
    const int jy0 = (y & 1) ? (y - 1) / 2 : y / 2 - 1, jy1 = (y & 1) ? (y - 1) / 2 : y / 2;
    const float e = 0.25f * ((mg_coarse_at(uc, ncx, ncy, acx, acy, jx0, jy0) + mg_coarse_at(uc, ncx, ncy, acx, acy, jx1, jy0)) +
                             (mg_coarse_at(uc, ncx, ncy, acx, acy, jx0, jy1) + mg_coarse_at(uc, ncx, ncy, acx, acy, jx1, jy1)));
    u[i] = u[i] + e;
}

// the coarsest level (its smaller side is 1 or 2 points, so a red-black sweep contracts by 0.57 at worst): MG_COARSE_SWEEPS sweeps in place by ONE workgroup per
// channel, the colours separated by __syncthreads().  A square-ish rectangle ends on a few unknowns; a long thin one on a strip that the workgroup walks through.
__global__ __launch_bounds__(256) void mg_coarse_kernel(float* u, const float* b, int nx, int ny, float ax, float ay) {
    const long n = (long)nx * ny;
    u += n * blockIdx.x; b += n * blockIdx.x;
    for (int sweep = 0; sweep < 2 * MG_COARSE_SWEEPS; ++sweep) {
        const int colour = sweep & 1;
        for (long i = threadIdx.x; i < n; i += 256) {
            const int y = (int)(i / nx), x = (int)(i % nx);
            if (((x + y) & 1) != colour) continue;
            const float d = (4.0f + (x == nx - 1 ? ax : 0.0f)) + (y == ny - 1 ? ay : 0.0f);
            const float nb = (mg_at(u, nx, ny, x - 1, y) + mg_at(u, nx, ny, x + 1, y)) + (mg_at(u, nx, ny, x, y - 1) + mg_at(u, nx, ny, x, y + 1));
            u[i] = (b[i] + nb) / d;
        }
        __syncthreads();
    }
}

// ---- the result.  One thread per pixel: inside R's interior v = dst + u, rounded half-even and clamped; everywhere else dst.  out_f (optional) takes v unrounded.
__global__ __launch_bounds__(256) void fusion_finish_kernel(const FusionImage p, const float* u, u8* out, float* out_f) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)p.H * p.W) return;
    const int y = (int)(i / p.W), x = (int)(i % p.W), ix = x - p.x1 - 1, iy = y - p.y1 - 1, nx = p.w - 2, ny = p.h - 2;
    const bool inside = u != nullptr && ix >= 0 && ix < nx && iy >= 0 && iy < ny;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const u8 d = p.dst[3 * i + c];
        float v = (float)d;
        u8 q = d;
        if (inside) {
            v = v + u[(long)c * nx * ny + (long)iy * nx + ix];
            q = (u8)fminf(fmaxf(rintf(v), 0.0f), 255.0f);
        }
        out[3 * i + c] = q;
        if (out_f) out_f[3 * i + c] = v;
    }
}

// ---- host: the levels and the cycle
struct MgLevel { int nx, ny; float ax, ay; float* u[2]; float* b; int cur; };

// level sizes of one axis: n, n / 2, n / 4 ...; a = s / gap - 1 with s the level's spacing and gap the distance of its last point to the ring, in fine cells
static int mg_axis(int n, int* sizes, float* a) {
    const double D = (double)n + 1.0;
    double s = 1.0;
    int L = 0;
    while (L < MG_MAX_LEVELS) {
        sizes[L] = n; a[L] = (float)(s / (D - s * n) - 1.0); ++L;
        if (n <= 2) break;
        n /= 2; s *= 2.0;
    }
    return L;
}
static int mg_levels(int w, int h, MgLevel* lv) {
    int sx[MG_MAX_LEVELS], sy[MG_MAX_LEVELS];
    float ax[MG_MAX_LEVELS], ay[MG_MAX_LEVELS];
    const int Lx = mg_axis(w - 2, sx, ax), Ly = mg_axis(h - 2, sy, ay), L = Lx < Ly ? Lx : Ly;
    for (int l = 0; l < L; ++l) { lv[l].nx = sx[l]; lv[l].ny = sy[l]; lv[l].ax = ax[l]; lv[l].ay = ay[l]; lv[l].cur = 0; }
    return L;
}

// 4 cycles up to max(w, h) = 512, 5 above: a cycle contracts the error by 0.053 at worst (measured), so 4 cycles leave 8e-6 of max|u| (|u| <= 2 * 255
// or so: 0.004 of a uint8 step, the size of the float32 rounding floor); the fifth is margin for the low-frequency corrections of the large rectangles
extern "C" int utx_image_fusion_cycles_impl(int w, int h) { return (w > h ? w : h) <= 512 ? 4 : 5; }

// per level three planar float arrays (u, its ping-pong twin, b) of 3 channels
extern "C" size_t utx_image_fusion_workspace_bytes_impl(int w, int h) {
    if (w < 3 || h < 3) return 0;
    MgLevel lv[MG_MAX_LEVELS];
    const int L = mg_levels(w, h, lv);
    size_t n = 0;
    for (int l = 0; l < L; ++l) n += (size_t)9 * lv[l].nx * lv[l].ny;
    return n * sizeof(float);
}

static inline unsigned blocks_for(long n) { return (unsigned)((n + 255) / 256); }

// arguments checked by utx_image_fusion (capi.cpp): the rectangle lies inside the image, the workspace holds utx_image_fusion_workspace_bytes_impl(w, h) bytes
extern "C" int utx_launch_image_fusion(const u8* src, const u8* dst, const u8* mask, int H, int W, int x1, int y1, int w, int h, int cycles, u8* out, float* out_f,
                                       void* work, hipStream_t stream) {
    FusionImage p;
    p.src = src; p.dst = dst; p.mask = mask; p.H = H; p.W = W; p.x1 = x1; p.y1 = y1; p.w = w; p.h = h;
    const unsigned img_blocks = blocks_for((long)H * W);
    if (w < 3 || h < 3) {      // no interior: the result is dst
        hipLaunchKernelGGL(fusion_finish_kernel, dim3(img_blocks), dim3(256), 0, stream, p, (const float*)nullptr, out, out_f);
        return hipGetLastError() == hipSuccess ? 0 : -4;
    }
    MgLevel lv[MG_MAX_LEVELS];
    const int L = mg_levels(w, h, lv);
    float* q = (float*)work;
    for (int l = 0; l < L; ++l) {
        const size_t n = (size_t)3 * lv[l].nx * lv[l].ny;
        lv[l].u[0] = q; lv[l].u[1] = q + n; lv[l].b = q + 2 * n; q += 3 * n;
    }
    if (cycles <= 0) cycles = utx_image_fusion_cycles_impl(w, h);
    hipLaunchKernelGGL(fusion_rhs_kernel, dim3(blocks_for((long)lv[0].nx * lv[0].ny)), dim3(256), 0, stream, p, lv[0].b, lv[0].u[0]);
    auto smooth = [&](MgLevel& v) {
        for (int s = 0; s < 2; ++s) {
            hipLaunchKernelGGL(mg_smooth_kernel, dim3((v.nx + MG_TX - 1) / MG_TX, (v.ny + MG_TY - 1) / MG_TY, 3), dim3(256), 0, stream,
                               (const float*)v.u[v.cur], v.u[v.cur ^ 1], (const float*)v.b, v.nx, v.ny, v.ax, v.ay);
            v.cur ^= 1;
        }
    };
    for (int c = 0; c < cycles; ++c) {
        for (int l = 0; l + 1 < L; ++l) {
            MgLevel& f = lv[l];
            MgLevel& g = lv[l + 1];
            smooth(f);
            g.cur = 0;
            hipLaunchKernelGGL(mg_restrict_kernel, dim3(blocks_for((long)g.nx * g.ny), 1, 3), dim3(256), 0, stream, (const float*)f.u[f.cur], (const float*)f.b,
                               f.nx, f.ny, f.ax, f.ay, g.b, g.u[0], g.nx, g.ny);
        }
        MgLevel& last = lv[L - 1];
        hipLaunchKernelGGL(mg_coarse_kernel, dim3(3), dim3(256), 0, stream, last.u[last.cur], (const float*)last.b, last.nx, last.ny, last.ax, last.ay);
        for (int l = L - 2; l >= 0; --l) {
            MgLevel& f = lv[l];
            MgLevel& g = lv[l + 1];
            hipLaunchKernelGGL(mg_prolong_kernel, dim3(blocks_for((long)f.nx * f.ny), 1, 3), dim3(256), 0, stream, f.u[f.cur], f.nx, f.ny,
                               (const float*)g.u[g.cur], g.nx, g.ny, g.ax, g.ay);
            smooth(f);
        }
        if (L == 1) break;      // a single level is solved by its sweeps: more cycles would repeat them on the converged values
    }
    hipLaunchKernelGGL(fusion_finish_kernel, dim3(img_blocks), dim3(256), 0, stream, p, (const float*)lv[0].u[lv[0].cur], out, out_f);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// Telea inpainting on the device (A. Telea, "An image inpainting technique based on the fast marching method", 2004): fp32, wave64, plain C++.  The reference
// hands uint8 images to OpenCV's cv2.inpaint(INPAINT_TELEA) [3p] on the host; OpenCV's heap order is not pinned by anything here, so the rule is this library's
// (DESIGN 8 "Telea inpainting"), the paper's weighted first-order estimate on an exact distance map:
//   utx_inpaint_distance    D2: the exact squared Euclidean distance of every hole pixel to the nearest pixel outside the hole (int32), 0 outside the hole
//   utx_inpaint_telea_step  one sweep of the propagation: every hole pixel whose read set is done computes its value from the previous sweep's state
//   utx_inpaint_finish      clamp to [0, 255], round half to even, uint8 store; optionally the unrounded float image
// Built with -ffp-contract=off: every product and sum below is rounded on its own, in the order written, which is the order the float32 restatement
// (tests/support/inpaint_ref.py) follows.
//
// The rule, with T = sqrt(float(D2)) correctly rounded and eps the radius (1 .. 8).  For a hole pixel p:
//   A(p) = { q in the image : |q - p|^2 <= eps^2 and D2(q) < D2(p) }      (a pixel outside the hole has D2 = 0 < D2(p); strict, on integers)
// and per channel, in float32, q enumerated ROW-MAJOR over the (2 eps + 1)^2 window (dy outer, dx inner, both ascending), r = p - q = (rx, ry):
//   len2 = float(rx rx + ry ry);  len = sqrt(len2);  dst = 1 / (len2 * len);  lev = 1 / (1 + |T(q) - T(p)|)
//   dir  = max(|rx * gTx + ry * gTy|, 1e-6);  w = (dst * lev) * dir
//   val  = I(q) + (gIx * rx + gIy * ry);  num = num + w * val;  den = den + w        (one running sum each, in the enumeration order)
//   v    = num / den
// gT = the difference of T at p: (T(+1) - T(-1)) * 0.5 where both neighbours are in the image, T(+1) - T(0) or T(0) - T(-1) at the image border, 0 on an axis of
// length 1.  gI at q, per axis, over the neighbours n of q that are in the image with D2(n) < D2(p): (I(+1) - I(-1)) * 0.5 with both, I(+1) - I(0) or
// I(0) - I(-1) with one, 0 with none.  Everything p reads has a strictly smaller D2, so the values are defined by induction on D2 and no schedule that honours
// that order can change a bit.  The READ SET of p is the disc and the 4-neighbours of the disc's pixels (gI reads them); p computes once every pixel of the read
// set with a smaller D2 is done.
#include "common.h"
#include "kernels.h"
#include <limits.h>

#define INP_TILE 16          // 16 x 16 pixels per 256-thread block: a wave is four rows of 16
#define INP_NONE INT_MAX     // D2 where no pixel lies outside the hole, and of the LDS entries outside the image: never smaller than any D2

// ---- distance
// pass 1, one thread per column: g = the vertical distance to the nearest pixel outside the hole in the column (a scan down, a scan up), INP_GINF if there is none
#define INP_GINF (1 << 30)
__global__ __launch_bounds__(64) void inpaint_column_scan_kernel(const unsigned char* hole, int H, int W, int* g) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= W) return;
    int d = INP_GINF;
#pragma unroll 8
    for (int y = 0; y < H; ++y) {
        const long i = (long)y * W + x;
        d = hole[i] == 0 ? 0 : (d < INP_GINF ? d + 1 : d);
        g[i] = d;
    }
    d = INP_GINF;
#pragma unroll 8
    for (int y = H - 1; y >= 0; --y) {
        const long i = (long)y * W + x;
        d = hole[i] == 0 ? 0 : (d < INP_GINF ? d + 1 : d);
        if (d < g[i]) g[i] = d;
    }
}
// pass 2, one thread per pixel: D2 = min over the row of dx^2 + g(x + dx)^2, walking outwards from dx = 0 and stopping once dx^2 alone reaches the best so far.
// H, W <= 16384 (checked by the C ABI): dx^2 + g^2 <= 2^29.
__global__ __launch_bounds__(256) void inpaint_row_min_kernel(const int* g, int H, int W, int* d2) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)H * W) return;
    const int x = (int)(i % W);
    const int* row = g + (i - x);
    const int g0 = row[x];
    int best = g0 >= INP_GINF ? INP_NONE : g0 * g0;
    for (int dx = 1; dx < W; ++dx) {
        const int dd = dx * dx;
        if (dd >= best) break;
        if (x - dx < 0 && x + dx >= W) break;
        if (x - dx >= 0) {
            const int gg = row[x - dx];
            if (gg < INP_GINF) best = min(best, dd + gg * gg);
        }
        if (x + dx < W) {
            const int gg = row[x + dx];
            if (gg < INP_GINF) best = min(best, dd + gg * gg);
        }
    }
    d2[i] = best;
}
extern "C" int utx_launch_inpaint_distance(const unsigned char* hole, int H, int W, int* tmp, int* d2, hipStream_t stream) {
    hipLaunchKernelGGL(inpaint_column_scan_kernel, dim3((unsigned)((W + 63) / 64)), dim3(64), 0, stream, hole, H, W, tmp);
    const long total = (long)H * W;
    hipLaunchKernelGGL(inpaint_row_min_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, stream, (const int*)tmp, H, W, d2);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---- propagation
struct InpaintStepParams {
    const float* col_in; const unsigned char* done_in; const int* d2; float* col_out; unsigned char* done_out; int* counter;
    int H, W, eps;
};
// is (dx, dy) in the read set of the centre: in the disc, or a 4-neighbour of a pixel of the disc
__device__ __forceinline__ bool inp_in_read_set(int dx, int dy, int e2) {
    const int ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy;
    if (ax * ax + ay * ay <= e2) return true;
    if (ax >= 1 && (ax - 1) * (ax - 1) + ay * ay <= e2) return true;
    return ay >= 1 && ax * ax + (ay - 1) * (ay - 1) <= e2;
}
// One thread per pixel, a 16 x 16 tile per block.  The block stages D2, T, the done flags and the colours of its tile plus a halo of eps + 1 (the read set) in
// LDS -- one dynamic array, carved [D2 int][T float][C colour planes float][done uint8], S = 16 + 2 (eps + 1) entries a side, at most 34^2 x 25 bytes = 28.9 KB --
// so every tap of the window and of the gradients comes from LDS.  A block with no pending pixel stages nothing.  Only hole pixels are written: a pixel outside
// the hole is the same in both buffers from the start (the caller initialises both) and never changes.  The counter takes the pixels computed in this sweep,
// one ballot and one vector atomic per wave.  No block waits for another.
template <int C>
__global__ __launch_bounds__(256) void inpaint_telea_step_kernel(const InpaintStepParams p) {
    extern __shared__ unsigned char inp_smem[];
    const int eps = p.eps, h = eps + 1, S = INP_TILE + 2 * h, n = S * S;
    int* sD2 = (int*)inp_smem;
    float* sT = (float*)(inp_smem + 4 * (size_t)n);
    float* sCol = (float*)(inp_smem + 8 * (size_t)n);
    unsigned char* sDone = inp_smem + (8 + 4 * C) * (size_t)n;
    const int tx = threadIdx.x & (INP_TILE - 1), ty = threadIdx.x >> 4;
    const int x0 = blockIdx.x * INP_TILE, y0 = blockIdx.y * INP_TILE;
    const int x = x0 + tx, y = y0 + ty;
    const bool in = x < p.W && y < p.H;
    const long idx = (long)y * p.W + x;
    const int myD2 = in ? p.d2[idx] : 0;
    const bool hole = myD2 > 0;
    const bool pending = hole && myD2 != INP_NONE && p.done_in[idx] == 0;
    if (!__syncthreads_or(pending)) {      // nothing to compute in this tile: the hole pixels carry their state into the other buffer
        if (hole) {
#pragma unroll
            for (int c = 0; c < C; ++c) p.col_out[idx * C + c] = p.col_in[idx * C + c];
            p.done_out[idx] = p.done_in[idx];
        }
        return;
    }
    for (int i = threadIdx.x; i < n; i += 256) {
        const int gx = x0 - h + i % S, gy = y0 - h + i / S;
        const bool inside = gx >= 0 && gx < p.W && gy >= 0 && gy < p.H;
        const long g = (long)gy * p.W + gx;
        const int d = inside ? p.d2[g] : INP_NONE;
        sD2[i] = d;
        sT[i] = sqrtf((float)d);
        sDone[i] = inside ? p.done_in[g] : (unsigned char)0;
#pragma unroll
        for (int c = 0; c < C; ++c) sCol[c * n + i] = inside ? p.col_in[g * C + c] : 0.0f;
    }
    __syncthreads();
    const int lp = (ty + h) * S + tx + h;      // this pixel's LDS entry
    const int e2 = eps * eps;
    bool ready = pending;
    if (pending) {
        for (int dy = -h; dy <= h && ready; ++dy)
            for (int dx = -h; dx <= h; ++dx) {
                if (!inp_in_read_set(dx, dy, e2)) continue;
                const int li = lp + dy * S + dx;
                if (sD2[li] < myD2 && sDone[li] == 0) { ready = false; break; }
            }
    }
    float v[C];
#pragma unroll
    for (int c = 0; c < C; ++c) v[c] = 0.0f;
    if (ready) {
        const float Tp = sT[lp];
        float gTx = 0.0f, gTy = 0.0f;
        if (x > 0 && x + 1 < p.W) gTx = (sT[lp + 1] - sT[lp - 1]) * 0.5f;
        else if (x + 1 < p.W) gTx = sT[lp + 1] - Tp;
        else if (x > 0) gTx = Tp - sT[lp - 1];
        if (y > 0 && y + 1 < p.H) gTy = (sT[lp + S] - sT[lp - S]) * 0.5f;
        else if (y + 1 < p.H) gTy = sT[lp + S] - Tp;
        else if (y > 0) gTy = Tp - sT[lp - S];
        float num[C], den = 0.0f;
#pragma unroll
        for (int c = 0; c < C; ++c) num[c] = 0.0f;
        // the summation order: dy = -eps .. eps outer, dx = -eps .. eps inner (row-major over the window), one running sum per channel and one for the weights
        for (int dy = -eps; dy <= eps; ++dy)
            for (int dx = -eps; dx <= eps; ++dx) {
                const int l2 = dx * dx + dy * dy;
                if (l2 > e2 || l2 == 0) continue;
                const int lq = lp + dy * S + dx;
                if (!(sD2[lq] < myD2)) continue;      // outside the image: INP_NONE, never smaller
                const float rx = (float)(-dx), ry = (float)(-dy);
                const float len2 = (float)l2;
                const float len = sqrtf(len2);
                const float dst = 1.0f / (len2 * len);
                const float lev = 1.0f / (1.0f + fabsf(sT[lq] - Tp));
                const float dir = fmaxf(fabsf(rx * gTx + ry * gTy), 1e-6f);
                const float w = (dst * lev) * dir;
                const bool xp = sD2[lq + 1] < myD2, xm = sD2[lq - 1] < myD2, yp = sD2[lq + S] < myD2, ym = sD2[lq - S] < myD2;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    const float* pl = sCol + c * n;
                    const float Iq = pl[lq];
                    float gIx = 0.0f, gIy = 0.0f;
                    if (xp && xm) gIx = (pl[lq + 1] - pl[lq - 1]) * 0.5f;
                    else if (xp) gIx = pl[lq + 1] - Iq;
                    else if (xm) gIx = Iq - pl[lq - 1];
                    if (yp && ym) gIy = (pl[lq + S] - pl[lq - S]) * 0.5f;
                    else if (yp) gIy = pl[lq + S] - Iq;
                    else if (ym) gIy = Iq - pl[lq - S];
                    const float val = Iq + (gIx * rx + gIy * ry);
                    num[c] = num[c] + w * val;
                }
                den = den + w;
            }
#pragma unroll
        for (int c = 0; c < C; ++c) v[c] = num[c] / den;
    }
    if (hole) {
#pragma unroll
        for (int c = 0; c < C; ++c) p.col_out[idx * C + c] = ready ? v[c] : sCol[c * n + lp];
        p.done_out[idx] = ready ? (unsigned char)1 : sDone[lp];
    }
    wave_count_add(p.counter, ready);
}
// arguments checked by utx_inpaint_telea_step (capi.cpp): H, W in 1 .. 16384, C in 1 .. 4, eps in 1 .. 8
extern "C" int utx_launch_inpaint_telea_step(const float* col_in, const unsigned char* done_in, const int* d2, int H, int W, int C, int eps, float* col_out,
                                             unsigned char* done_out, int* counter, hipStream_t stream) {
    InpaintStepParams p;
    p.col_in = col_in; p.done_in = done_in; p.d2 = d2; p.col_out = col_out; p.done_out = done_out; p.counter = counter; p.H = H; p.W = W; p.eps = eps;
    const int S = INP_TILE + 2 * (eps + 1);
    const size_t lds = (size_t)S * S * (8 + 4 * C + 1);
    const dim3 grid((unsigned)((W + INP_TILE - 1) / INP_TILE), (unsigned)((H + INP_TILE - 1) / INP_TILE));
    switch (C) {
        case 1: hipLaunchKernelGGL(inpaint_telea_step_kernel<1>, grid, dim3(256), lds, stream, p); break;
        case 2: hipLaunchKernelGGL(inpaint_telea_step_kernel<2>, grid, dim3(256), lds, stream, p); break;
        case 3: hipLaunchKernelGGL(inpaint_telea_step_kernel<3>, grid, dim3(256), lds, stream, p); break;
        case 4: hipLaunchKernelGGL(inpaint_telea_step_kernel<4>, grid, dim3(256), lds, stream, p); break;
        default: return -2;
    }
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---- finish
// out = uint8(rint(min(max(v, 0), 255))): rint rounds half to even in the default rounding mode.  out_f (optional) = v, unclamped and unrounded.
__global__ __launch_bounds__(256) void inpaint_finish_kernel(const float* col, long n, unsigned char* out, float* out_f) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float v = col[i];
    out[i] = (unsigned char)rintf(fminf(fmaxf(v, 0.0f), 255.0f));
    if (out_f) out_f[i] = v;
}
extern "C" int utx_launch_inpaint_finish(const float* col, int H, int W, int C, unsigned char* out, float* out_f, hipStream_t stream) {
    const long n = (long)H * W * C;
    hipLaunchKernelGGL(inpaint_finish_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, col, n, out, out_f);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

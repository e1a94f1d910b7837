// Silhouette antialiasing of screen-space buffers (gfx950): the forward pass of what the reference calls dr.antialias on every buffer of
// simple_rendering (render/nvdiffrast/renderer_base.py:143-336).  Entry points:
//   utx_antialias_analyze   geometry only: per pixel the four blend weights that its four pixel pairs land on it; runs once per rasterisation
//   utx_antialias_apply     the four-neighbour stencil of one buffer with those weights; runs once per buffer
// The rule is this project's own, after the published description (Laine et al. 2020, section 3.5); nvdiffrast [3p] is not on the machines and its
// samples are NOT pinned (DESIGN 8 "Silhouette antialiasing").  The kernels equal tests/support/antialias_ref.py's float32 restatement bit for bit.
//
// A pair is pixel p = (px, py) and q = p + (1, 0) (horizontal) or p + (0, 1) (vertical), both inside one view.  Every operation below is ONE float32
// operation, rounded once (-ffp-contract=off, no packed fp32; `/` is hipcc's correctly rounded division):
//  (a) ip = int(rast[p].w) - 1, iq = int(rast[q].w) - 1; ip == iq: nothing.
//  (b) far_p = ip < 0 || (iq >= 0 && rast[p].z > rast[q].z); t = far_p ? iq : ip; t outside [0, F) or a vertex index of t outside [0, V): nothing.
//  (c) per vertex k of t with (x, y, ., w) = pos[tri[t][k]]: not (|x|, |y|, |w| < inf and w > 0): nothing.  With cx = float(px) + 0.5, cy = float(py) + 0.5
//        sx = ((x / w) * 0.5 + 0.5) * float(W) - cx        sy = ((y / w) * 0.5 + 0.5) * float(H) - cy
//      (raster.hip's mapping: column c <-> x_ndc = (c + 0.5) / W * 2 - 1, row r <-> y_ndc = (r + 0.5) / H * 2 - 1);
//      horizontal pair: (X, Y) = (sx, sy); vertical pair: (X, Y) = (sy, sx).
//  (d) edge e = (a, b) = (k, (k + 1) % 3), e = 0, 1, 2 in this order: straddles if (Ya < 0) != (Yb < 0); d = (Xa * Yb - Xb * Ya) / (Yb - Ya);
//      candidate if d >= 0 && d <= 1 (false for NaN).  Chosen: the smallest d if t == ip, the largest if t == iq; a later edge replaces an earlier
//      one only when strictly smaller / larger.  No candidate: nothing.
//  (e) c = (k + 2) % 3; own = (Xb - Xa) * (Yc - Ya) - (Yb - Ya) * (Xc - Xa); not (own < 0 || own > 0): nothing.  o = opp[t][e]: the edge is a silhouette
//      edge if o < 0, o >= V, or pos[o] fails the test of (c); otherwise, with o projected as in (c), wing = (Xb - Xa) * (Yo - Ya) - (Yb - Ya) * (Xo - Xa),
//      and the surface CONTINUES (nothing) exactly if (own > 0 && wing < 0) || (own < 0 && wing > 0); a zero, equally signed or NaN wing is a silhouette.
//  (f) d < 0.5: p gets the weight 0.5 - d towards q;  d > 0.5: q gets d - 0.5 towards p;  d == 0.5: nothing.
// weights[p] = (w_left, w_right, w_up, w_down): what the pairs (p - (1,0), p), (p, p + (1,0)), (p - (0,1), p), (p, p + (0,1)) land on p; 0 where nothing lands
// or the neighbour lies outside the image.  Every pair is evaluated by both of its pixels: no atomics, no workspace, no ordering.
// apply, per channel:  k_n = w_n != 0 ? w_n * (color[n] - color[p]) : +0;   out[p] = (((color[p] + k_left) + k_right) + k_up) + k_down.
//
// HBM-bound: 16 B read + 16 B written per pixel in the analysis (the neighbours' records and the few silhouette triangles hit L2), a stencil per buffer.
// Plain vector loads and stores, no LDS, no scratch (the three edges are unrolled so no array is indexed by a register), no inline assembly, no atomics.
#include "common.h"
#include "kernels.h"

struct AaGeom {
    const float* rast; const float* pos; const int* tri; const int* opp;
    long pos_view_stride, npix, total;
    int F, V, H, W;
};

__device__ __forceinline__ bool aa_project(const float4 v, float Wf, float Hf, float cx, float cy, bool vertical, float& X, float& Y) {
    if (!(fabsf(v.x) < INFINITY) || !(fabsf(v.y) < INFINITY) || !(fabsf(v.w) < INFINITY) || !(v.w > 0.0f)) return false;
    const float sx = ((v.x / v.w) * 0.5f + 0.5f) * Wf - cx;
    const float sy = ((v.y / v.w) * 0.5f + 0.5f) * Hf - cy;
    X = vertical ? sy : sx;
    Y = vertical ? sx : sy;
    return true;
}

// the crossing d of the silhouette edge of the pair whose first pixel is (px, py), or -1 where the pair contributes nothing
__device__ float aa_pair(const AaGeom& g, const float4* __restrict__ pos, int px, int py, bool vertical, float zp, int ip, float zq, int iq) {
    if (ip == iq) return -1.0f;
    const bool far_p = ip < 0 || (iq >= 0 && zp > zq);
    const int t = far_p ? iq : ip;
    if (t < 0 || t >= g.F) return -1.0f;
    const int i0 = g.tri[3 * (long)t], i1 = g.tri[3 * (long)t + 1], i2 = g.tri[3 * (long)t + 2];
    if (i0 < 0 || i0 >= g.V || i1 < 0 || i1 >= g.V || i2 < 0 || i2 >= g.V) return -1.0f;
    const float Wf = (float)g.W, Hf = (float)g.H, cx = (float)px + 0.5f, cy = (float)py + 0.5f;
    float X0, Y0, X1, Y1, X2, Y2;
    if (!aa_project(pos[i0], Wf, Hf, cx, cy, vertical, X0, Y0) || !aa_project(pos[i1], Wf, Hf, cx, cy, vertical, X1, Y1) ||
        !aa_project(pos[i2], Wf, Hf, cx, cy, vertical, X2, Y2)) return -1.0f;
    float bd = -1.0f, Xa = 0.0f, Ya = 0.0f, Xb = 0.0f, Yb = 0.0f, Xc = 0.0f, Yc = 0.0f;
    int be = -1;
#define AA_EDGE(E, XA, YA, XB, YB, XC, YC) \
    if ((YA < 0.0f) != (YB < 0.0f)) { \
        const float d = (XA * YB - XB * YA) / (YB - YA); \
        if (d >= 0.0f && d <= 1.0f && (be < 0 || (far_p ? d > bd : d < bd))) { \
            bd = d; be = E; Xa = XA; Ya = YA; Xb = XB; Yb = YB; Xc = XC; Yc = YC; \
        } \
    }
    AA_EDGE(0, X0, Y0, X1, Y1, X2, Y2)
    AA_EDGE(1, X1, Y1, X2, Y2, X0, Y0)
    AA_EDGE(2, X2, Y2, X0, Y0, X1, Y1)
#undef AA_EDGE
    if (be < 0) return -1.0f;
    const float ex = Xb - Xa, ey = Yb - Ya;
    const float own = ex * (Yc - Ya) - ey * (Xc - Xa);
    if (!(own < 0.0f || own > 0.0f)) return -1.0f;
    const int o = g.opp[3 * (long)t + be];
    if (o >= 0 && o < g.V) {
        float Xo, Yo;
        if (aa_project(pos[o], Wf, Hf, cx, cy, vertical, Xo, Yo)) {
            const float wing = ex * (Yo - Ya) - ey * (Xo - Xa);
            if ((own > 0.0f && wing < 0.0f) || (own < 0.0f && wing > 0.0f)) return -1.0f;      // the surface continues across the edge
        }
    }
    return bd;
}

// (z, id) of the record at pixel index j
__device__ __forceinline__ void aa_record(const float* __restrict__ rast, long j, float& z, int& id) {
    const float2 r = *(const float2*)(rast + 4 * j + 2);
    z = r.x; id = (int)r.y - 1;
}

// one thread per pixel of rast [B][H][W][4], lanes along x
__global__ __launch_bounds__(256) void antialias_analyze_kernel(AaGeom g, float4* __restrict__ weights) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= g.total) return;
    const long b = i / g.npix, r = i - b * g.npix;
    const int py = (int)(r / g.W), px = (int)(r - (long)py * g.W);
    float zm, zn[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    int im, in[4];
    aa_record(g.rast, i, zm, im);
    in[0] = in[1] = in[2] = in[3] = im;      // a neighbour outside the image agrees: its pair does not exist
    if (px > 0) aa_record(g.rast, i - 1, zn[0], in[0]);
    if (px < g.W - 1) aa_record(g.rast, i + 1, zn[1], in[1]);
    if (py > 0) aa_record(g.rast, i - g.W, zn[2], in[2]);
    if (py < g.H - 1) aa_record(g.rast, i + g.W, zn[3], in[3]);
    float4 w = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (in[0] != im || in[1] != im || in[2] != im || in[3] != im) {      // all five agree: the overwhelming case leaves with four zeros
        const float4* pos = (const float4*)(g.pos + g.pos_view_stride * b);
        // left and up: this pixel is the pair's q and takes d - 0.5; right and down: it is p and takes 0.5 - d
        if (in[0] != im) { const float d = aa_pair(g, pos, px - 1, py, false, zn[0], in[0], zm, im); if (d > 0.5f) w.x = d - 0.5f; }
        if (in[1] != im) { const float d = aa_pair(g, pos, px, py, false, zm, im, zn[1], in[1]); if (d >= 0.0f && d < 0.5f) w.y = 0.5f - d; }
        if (in[2] != im) { const float d = aa_pair(g, pos, px, py - 1, true, zn[2], in[2], zm, im); if (d > 0.5f) w.z = d - 0.5f; }
        if (in[3] != im) { const float d = aa_pair(g, pos, px, py, true, zm, im, zn[3], in[3]); if (d >= 0.0f && d < 0.5f) w.w = 0.5f - d; }
    }
    weights[i] = w;
}

// the arguments were checked by utx_antialias_analyze (capi.cpp)
extern "C" int utx_launch_antialias_analyze(const float* rast, const float* pos, long pos_view_stride, const int* tri, const int* opp, int F, int V, int B, int H,
                                            int W, float* weights, hipStream_t stream) {
    if (F <= 0 || V <= 0 || B <= 0 || H <= 0 || W <= 0) return -2;
    AaGeom g = {};
    g.rast = rast; g.pos = pos; g.tri = tri; g.opp = opp; g.pos_view_stride = pos_view_stride;
    g.npix = (long)H * W; g.total = g.npix * B; g.F = F; g.V = V; g.H = H; g.W = W;
    const long nb = (g.total + 255) / 256;
    if (nb > 0x7fffffffL) return -2;
    hipLaunchKernelGGL(antialias_analyze_kernel, dim3((unsigned)nb), dim3(256), 0, stream, g, (float4*)weights);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// one thread per (pixel, channel) of color [B][H][W][C], channels fastest: neighbouring lanes read neighbouring addresses for every C
__global__ __launch_bounds__(256) void antialias_apply_kernel(const float* __restrict__ color, const float4* __restrict__ weights, long npix, int H, int W, int C,
                                                              long total, float* __restrict__ out) {
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= total) return;
    const long i = e / C;
    const float4 w = weights[i];
    const float c = color[e];
    const long row = (long)W * C;
    // utx_antialias_analyze writes a non-zero weight only where the neighbour lies inside the same view; checked again, so that weights of another origin
    // cannot make the stencil read outside the buffer
    const long r = i % npix;
    const int py = (int)(r / W), px = (int)(r - (long)py * W);
    const float kl = (w.x != 0.0f && px > 0) ? w.x * (color[e - C] - c) : 0.0f;
    const float kr = (w.y != 0.0f && px < W - 1) ? w.y * (color[e + C] - c) : 0.0f;
    const float ku = (w.z != 0.0f && py > 0) ? w.z * (color[e - row] - c) : 0.0f;
    const float kd = (w.w != 0.0f && py < H - 1) ? w.w * (color[e + row] - c) : 0.0f;
    out[e] = (((c + kl) + kr) + ku) + kd;
}

extern "C" int utx_launch_antialias_apply(const float* color, const float* weights, int B, int H, int W, int C, float* out, hipStream_t stream) {
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return -2;
    const long npix = (long)H * W, total = npix * B * C;
    const long nb = (total + 255) / 256;
    if (nb > 0x7fffffffL) return -2;
    hipLaunchKernelGGL(antialias_apply_kernel, dim3((unsigned)nb), dim3(256), 0, stream, color, (const float4*)weights, npix, H, W, C, total, out);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// The cube's faces and the cube lookup, stated once for pbr.hip (environment lights) and scene.hip (environment renderer).  The rule is the one at the head
// of pbr.hip and in include/unitex_hip.h.  Every translation unit that includes this header is compiled with -ffp-contract=off, as for shade_device.h:
// each operation is one correctly rounded fp32 operation, so a lookup is bit-identical wherever it is made.
// CH = channels per texel (cube [6][N][N][CH]); 3 unless stated, which is the arithmetic pbr.hip has always had.  The channels do not interact.
#pragma once
#include <math.h>
#include <hip/hip_runtime.h>

// ---------------------------------------------------------------------------------------------------------------- the cube's faces, stated once
// face s, in-face coordinates (a, b), depth d -> the vector (cube_to_dir before normalisation): fp64 with d = 1 for the tables and the lat-long resampling,
// integers in units of 1 / N with d = N for the taps that leave a face
template <class T>
__host__ __device__ inline void pbr_face_vec(int s, T a, T b, T d, T v[3]) {
    switch (s) {
        case 0: v[0] = d; v[1] = -b; v[2] = -a; break;
        case 1: v[0] = -d; v[1] = -b; v[2] = a; break;
        case 2: v[0] = a; v[1] = d; v[2] = b; break;
        case 3: v[0] = a; v[1] = -d; v[2] = -b; break;
        case 4: v[0] = a; v[1] = -b; v[2] = d; break;
        default: v[0] = -a; v[1] = -b; v[2] = -d; break;
    }
}

// vector -> its face (the component of largest magnitude, ties to x, then y) and the in-face numerators (cx, cy) over the denominator cz = that magnitude
// (dir_to_side of cubemap.cu:48-60): fp32 for a direction, integers for a tap's centre
__device__ __forceinline__ float pbr_abs(float x) { return fabsf(x); }
__device__ __forceinline__ int pbr_abs(int x) { return abs(x); }
template <class T>
__device__ __forceinline__ int pbr_vec_face(T v0, T v1, T v2, T& cx, T& cy, T& cz) {
    const T a0 = pbr_abs(v0), a1 = pbr_abs(v1), a2 = pbr_abs(v2);
    int s;
    if (a0 >= a1 && a0 >= a2) { s = v0 >= (T)0 ? 0 : 1; cx = s == 0 ? -v2 : v2; cy = -v1; cz = a0; }
    else if (a1 >= a2) { s = v1 >= (T)0 ? 2 : 3; cx = v0; cy = s == 2 ? v2 : -v2; cz = a1; }
    else { s = v2 >= (T)0 ? 4 : 5; cx = s == 4 ? v0 : -v0; cy = -v1; cz = a2; }
    return s;
}

// unit direction of (fx, fy) on face s
__host__ __device__ inline void pbr_cube_dir(int s, double fx, double fy, double v[3]) {
    pbr_face_vec(s, fx, fy, 1.0, v);
    const double l = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    v[0] /= l; v[1] /= l; v[2] /= l;
}

// ---------------------------------------------------------------------------------------------------------------- the lookup
// face and in-face coordinates of a direction, over the major magnitude
__device__ __forceinline__ int pbr_dir_face(float dx, float dy, float dz, float& fx, float& fy) {
    float cx, cy, cz;
    const int s = pbr_vec_face(dx, dy, dz, cx, cy, cz);
    if (cz > 0.f) { fx = cx / cz; fy = cy / cz; } else { fx = fy = 0.f; }
    return s;
}

// texel of a tap that left face s along one axis: its centre on the plane of s, in integer units of 1 / N ((a, b) odd, depth N), seen from the neighbour
__device__ __forceinline__ long pbr_out_tap(int N, int s, int x, int y) {
    int v[3], cx, cy, cz;
    pbr_face_vec(s, 2 * x + 1 - N, 2 * y + 1 - N, N, v);
    const int s2 = pbr_vec_face(v[0], v[1], v[2], cx, cy, cz);
    int ix = (int)(((long)(cx + cz) * N) / (2L * cz)), iy = (int)(((long)(cy + cz) * N) / (2L * cz));
    ix = min(max(ix, 0), N - 1); iy = min(max(iy, 0), N - 1);
    return ((long)s2 * N + iy) * N + ix;
}

template <int CH = 3>
__device__ __forceinline__ void pbr_cube_tap(const float* cube, int N, int s, int x, int y, float o[CH]) {
    const bool ox = x < 0 || x >= N, oy = y < 0 || y >= N;
    if (ox && oy) {
        const int cx = min(max(x, 0), N - 1), cy = min(max(y, 0), N - 1);
        const float* t1 = cube + CH * pbr_out_tap(N, s, cx, y);
        const float* t2 = cube + CH * pbr_out_tap(N, s, x, cy);
        const float* t3 = cube + CH * (((long)s * N + cy) * N + cx);
#pragma unroll
        for (int k = 0; k < CH; ++k) o[k] = ((t1[k] + t2[k]) + t3[k]) / 3.0f;
        return;
    }
    const float* t = cube + CH * ((ox || oy) ? pbr_out_tap(N, s, x, y) : ((long)s * N + y) * N + x);
#pragma unroll
    for (int k = 0; k < CH; ++k) o[k] = t[k];
}

__device__ __forceinline__ void pbr_snap(float t, float thr, int& base, float& frac) {
    const float b = floorf(t);
    base = (int)b; frac = t - b;
    if (frac < thr) frac = 0.f;
    else if (frac > 1.0f - thr) { frac = 0.f; base += 1; }
}

template <int CH = 3>
__device__ __forceinline__ void pbr_cube_lookup(const float* cube, int N, float dx, float dy, float dz, float o[CH]) {
    float fx, fy;
    const int s = pbr_dir_face(dx, dy, dz, fx, fy);
    const float tx = (fx + 1.0f) * (0.5f * (float)N) - 0.5f, ty = (fy + 1.0f) * (0.5f * (float)N) - 0.5f;
    const float thr = fminf((float)N * 4.76837158203125e-07f, 0.25f);      // N * 2^-21
    int x0, y0; float wx, wy;
    pbr_snap(tx, thr, x0, wx);
    pbr_snap(ty, thr, y0, wy);
    float t00[CH], t01[CH], t10[CH], t11[CH];
    pbr_cube_tap<CH>(cube, N, s, x0, y0, t00);
    pbr_cube_tap<CH>(cube, N, s, x0 + 1, y0, t01);
    pbr_cube_tap<CH>(cube, N, s, x0, y0 + 1, t10);
    pbr_cube_tap<CH>(cube, N, s, x0 + 1, y0 + 1, t11);
#pragma unroll
    for (int k = 0; k < CH; ++k) {
        const float top = t00[k] + wx * (t01[k] - t00[k]);
        const float bot = t10[k] + wx * (t11[k] - t10[k]);
        o[k] = top + wy * (bot - top);
    }
}

// Image-based PBR shading of the turntable (gfx950): the environment-light prefilters and the split-sum shading of the reference's PBRModel
// (TextureTools/texturetools/texture/pbr/pbr.py:18-49, 91-130; render/nvdiffrast/renderer_pbr.py:19-94; the prefilters of its renderutils
// plugin, texture/pbr/renderutils/ops.py:398-465 and c_src/cubemap.cu:12-139, 174-298).  All data fp32, wave64, stream-ordered, no host
// synchronisation, no inter-workgroup waiting.  Compiled with -ffp-contract=off (the shade kernel interpolates exactly as utx_interpolate
// does); the prefilter loops spell their fused multiply-adds out with fmaf.
//
// Cube face s and its in-face coordinates (fx, fy) in [-1, 1] follow cube_to_dir: 0 (1, -fy, -fx)  1 (-1, -fy, fx)  2 (fx, 1, fy)
// 3 (fx, -1, -fy)  4 (fx, -fy, 1)  5 (-fx, -fy, -1); texel (x, y) of an N^2 face has its centre at f = 2 (i + 0.5) / N - 1.
//
// Cube lookup rule (this project's own: nvdiffrast's boundary_mode='cube' is third-party and absent; include/unitex_hip.h states the same):
//   1. face = the component of largest magnitude, ties to x, then y (a zero vector looks up the centre of face 0); (fx, fy) = the other two
//      components over that magnitude, mapped as above;
//   2. texel coordinates t = (f + 1) * N / 2 - 0.5, base = floor(t), fraction = t - base; a fraction within N * 2^-21 of a texel centre (four
//      times the fp32 uncertainty of t itself) snaps to it, so a texel-centre direction returns that texel exactly;
//   3. the four taps (base + {0, 1})^2 blend as a + f (b - a), along x first;
//   4. a tap that left the face along ONE axis is taken from the texel that holds its own direction (the tap's centre on this face's plane)
//      on the neighbouring face: the edge texel of the same row, found in integers;
//   5. a tap that left along BOTH axes (its direction is equidistant from two neighbours) is the mean ((t1 + t2) + t3) / 3 of the three texels
//      that meet at that cube corner: its two single-axis neighbours and the face's own corner texel.
//   With 4 and 5 the value is continuous across every edge and corner.
#include <math.h>
#include "common.h"
#include "kernels.h"
#include "shade_device.h"
#include "cube_device.h"      // the cube's faces and the cube lookup, shared with scene.hip

// ---------------------------------------------------------------------------------------------------------------- host tables (fp64, rounded once)
// texels [6][N][N][4] = (unit direction of the texel centre, pixel_area(x, y, N) of cubemap.cu:17-30); tiles [6][nt][nt][4] with nt = ceil(N / 16):
// (unit axis a of the 16^2 texel tile, thr): every texel centre L of the tile with V.L >= costheta_cutoff has V.a >= thr for unit V
// (thr = cos(min(pi, acos(cutoff) + max angle(a, L))) - 1e-5, the margin covers fp32 dot products of unit vectors a hundred times over).
extern "C" int utx_cubemap_table_impl(int N, float costheta_cutoff, float* texels_host, float* tiles_host) {
    if (N < 2 || (N & 1) || N > 8192 || !texels_host) return -2;
    const int H = N / 2;
    for (int s = 0; s < 6; ++s)
        for (int y = 0; y < N; ++y)
            for (int x = 0; x < N; ++x) {
                double v[3];
                pbr_cube_dir(s, 2.0 * ((x + 0.5) / N) - 1.0, 2.0 * ((y + 0.5) / N) - 1.0, v);
                const int ax = abs(x - H), ay = abs(y - H);
                const double dx = atan((double)(ax + 1) / H) - atan((double)ax / H), dy = atan((double)(ay + 1) / H) - atan((double)ay / H);
                float* o = texels_host + 4 * (((size_t)s * N + y) * N + x);
                o[0] = (float)v[0]; o[1] = (float)v[1]; o[2] = (float)v[2]; o[3] = (float)(dx * dy);
            }
    if (!tiles_host) return 0;
    const int nt = (N + 15) / 16;
    const double cut = costheta_cutoff > 1.f ? 1.0 : costheta_cutoff < -1.f ? -1.0 : (double)costheta_cutoff;
    const double theta_c = acos(cut);
    for (int s = 0; s < 6; ++s)
        for (int ty = 0; ty < nt; ++ty)
            for (int tx = 0; tx < nt; ++tx) {
                const int x0 = tx * 16, y0 = ty * 16, x1 = x0 + 16 < N ? x0 + 16 : N, y1 = y0 + 16 < N ? y0 + 16 : N;
                double a[3];
                pbr_cube_dir(s, 2.0 * ((0.5 * (x0 + x1)) / N) - 1.0, 2.0 * ((0.5 * (y0 + y1)) / N) - 1.0, a);
                double cmin = 1.0;
                for (int y = y0; y < y1; ++y)
                    for (int x = x0; x < x1; ++x) {
                        const float* L = texels_host + 4 * (((size_t)s * N + y) * N + x);
                        const double c = a[0] * L[0] + a[1] * L[1] + a[2] * L[2];
                        if (c < cmin) cmin = c;
                    }
                const double ang = theta_c + acos(cmin < -1.0 ? -1.0 : cmin) + 1e-6;
                float* o = tiles_host + 4 * (((size_t)s * nt + ty) * nt + tx);
                o[0] = (float)a[0]; o[1] = (float)a[1]; o[2] = (float)a[2];
                o[3] = ang >= 3.14159265358979323846 ? -2.0f : (float)(cos(ang) - 1e-5);
            }
    return 0;
}

// ---------------------------------------------------------------------------------------------------------------- lat-long -> cube
// latlong_to_cubemap (pbr.py:28-49): v = normalize(cube_to_dir(s, gx, gy)), tu = atan2(vx, -vz) / 2pi + 0.5, tv = acos(clamp(vy)) / pi, bilinear fetch with
// wrap addressing in both axes (texel centres at +0.5).  The texture coordinates, the fractions and the blend are carried in fp64 and rounded once:
// a fp32 tu times Wi already moves the fraction by more than the result may differ from the fp64 statement (one-time work, 6 N^2 texels).
__global__ __launch_bounds__(256) void latlong_to_cubemap_kernel(const float* lat, int Hi, int Wi, int N, float* out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 6L * N * N) return;
    const int x = (int)(i % N), y = (int)((i / N) % N), s = (int)(i / ((long)N * N));
    const double fx = 2.0 * ((x + 0.5) / N) - 1.0, fy = 2.0 * ((y + 0.5) / N) - 1.0;
    double vd[3];
    pbr_cube_dir(s, fx, fy, vd);
    const double v0 = vd[0], v1 = vd[1], v2 = vd[2];
    const double kPi = 3.14159265358979323846;
    const double tu = atan2(v0, -v2) / (2.0 * kPi) + 0.5;
    const double tv = acos(fmin(fmax(v1, -1.0), 1.0)) / kPi;
    const double px = tu * Wi - 0.5, py = tv * Hi - 0.5;
    const double bx = floor(px), by = floor(py);
    const double wx = px - bx, wy = py - by;
    const int x0 = sd_wrapi((long)bx, Wi), x1 = sd_wrapi((long)bx + 1, Wi);
    const int y0 = sd_wrapi((long)by, Hi), y1 = sd_wrapi((long)by + 1, Hi);
    const float* t00 = lat + 3 * ((long)y0 * Wi + x0);
    const float* t01 = lat + 3 * ((long)y0 * Wi + x1);
    const float* t10 = lat + 3 * ((long)y1 * Wi + x0);
    const float* t11 = lat + 3 * ((long)y1 * Wi + x1);
    for (int k = 0; k < 3; ++k) out[3 * i + k] = (float)sd_bilerp((double)t00[k], (double)t01[k], (double)t10[k], (double)t11[k], wx, wy);
}

extern "C" int utx_launch_latlong_to_cubemap(const float* lat, int Hi, int Wi, int N, float* out, hipStream_t stream) {
    if (Hi <= 0 || Wi <= 0 || N <= 0 || N > 8192) return -2;
    const long n = 6L * N * N;
    hipLaunchKernelGGL(latlong_to_cubemap_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, lat, Hi, Wi, N, out);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---------------------------------------------------------------------------------------------------------------- diffuse prefilter
// DiffuseCubemapFwdKernel (cubemap.cu:110-139): out(n) = sum over ALL 6 N^2 texels of c * (clamp(n.L, 0, 0.999) * pixel_area / 3.141592).
// 6 N^2 outputs x 6 N^2 inputs of pure fp32 VALU work: the inputs sweep through LDS in tiles of 256 (direction + weight, colour), every lane reads the same
// entry (broadcast), each thread keeps DF_OUT outputs in registers so one pair of LDS reads feeds DF_OUT * 8 VALU operations.
// Reduction order (fixed, so results are run-to-run identical): inside a tile in texel order into a partial sum, the partial sums in tile order.
#define DF_TILE 256
#define DF_OUT 4

__global__ __launch_bounds__(256) void cubemap_diffuse_kernel(const float4* tab, const float* cube, int n, float* out) {
    __shared__ float4 sd[DF_TILE], sc[DF_TILE];
    const int tid = threadIdx.x;
    float nx[DF_OUT], ny[DF_OUT], nz[DF_OUT], acc[DF_OUT][3];
#pragma unroll
    for (int k = 0; k < DF_OUT; ++k) {
        const long o = (long)blockIdx.x * (256 * DF_OUT) + k * 256 + tid;
        const float4 t = tab[o < n ? o : n - 1];
        nx[k] = t.x; ny[k] = t.y; nz[k] = t.z;
        acc[k][0] = acc[k][1] = acc[k][2] = 0.f;
    }
    for (int j0 = 0; j0 < n; j0 += DF_TILE) {
        const int j = j0 + tid;
        float4 d = make_float4(0.f, 0.f, 0.f, 0.f), c = make_float4(0.f, 0.f, 0.f, 0.f);      // past the end: weight 0, colour 0 (adds exact zeros)
        if (j < n) {
            d = tab[j];
            d.w = d.w / 3.141592f;
            c = make_float4(cube[3 * (long)j], cube[3 * (long)j + 1], cube[3 * (long)j + 2], 0.f);
        }
        sd[tid] = d; sc[tid] = c;
        __syncthreads();
        float part[DF_OUT][3];
#pragma unroll
        for (int k = 0; k < DF_OUT; ++k) part[k][0] = part[k][1] = part[k][2] = 0.f;
#pragma unroll 4
        for (int i = 0; i < DF_TILE; ++i) {
            const float4 L = sd[i], col = sc[i];
#pragma unroll
            for (int k = 0; k < DF_OUT; ++k) {
                float cs = fmaf(nz[k], L.z, fmaf(ny[k], L.y, nx[k] * L.x));
                cs = fminf(fmaxf(cs, 0.0f), 0.999f);
                const float w = cs * L.w;
                part[k][0] = fmaf(col.x, w, part[k][0]);
                part[k][1] = fmaf(col.y, w, part[k][1]);
                part[k][2] = fmaf(col.z, w, part[k][2]);
            }
        }
#pragma unroll
        for (int k = 0; k < DF_OUT; ++k) { acc[k][0] += part[k][0]; acc[k][1] += part[k][1]; acc[k][2] += part[k][2]; }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < DF_OUT; ++k) {
        const long o = (long)blockIdx.x * (256 * DF_OUT) + k * 256 + tid;
        if (o < n) { out[3 * o] = acc[k][0]; out[3 * o + 1] = acc[k][1]; out[3 * o + 2] = acc[k][2]; }
    }
}

extern "C" int utx_launch_cubemap_diffuse(const float* cube, int N, const float* texels, float* out, hipStream_t stream) {
    if (N < 2 || (N & 1) || N > 8192) return -2;      // pixel_area halves N in integers
    const long n = 6L * N * N;
    hipLaunchKernelGGL(cubemap_diffuse_kernel, dim3((unsigned)((n + 256 * DF_OUT - 1) / (256 * DF_OUT))), dim3(256), 0, stream, (const float4*)texels, cube,
                       (int)n, out);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---------------------------------------------------------------------------------------------------------------- specular prefilter
// SpecularCubemapFwdKernel (cubemap.cu:174-179, 246-298) and the division of ops.py:465: over the texels with L.V >= costheta_cutoff,
//   w = max(L.V, 0) * ndfGGX(alpha^2, max(V.H, 0)) * pixel_area / 4,  H = safeNormalize(L + V);  out = sum(c w) / sum(w).
// The reference's bounds table only culls; here one workgroup owns one 16^2 tile of outputs and walks the 6 ceil(N/16)^2 input tiles, skipping a tile whose
// bounding cone (host table, conservative for its texel centres) cannot reach the lobe; inside a tile every texel takes the cutoff test itself, so the
// accepted set is the cutoff test's alone.  Neighbouring outputs accept the same tiles, so a wave stays together; all lanes read the same texel (broadcast).
// The weights are carried relative to the first accepted texel's (w / w_first, 1 for that texel itself): a ratio of sums does not see the common factor, a
// constant cubemap still returns exactly 1 (numerator and denominator add the same numbers in the same order) and a lobe of one texel returns that texel
// exactly (c * 1 / 1).  Fixed sweep order: tiles in (face, row, column) order, texels row-major inside a tile.
__global__ __launch_bounds__(256) void cubemap_specular_kernel(const float4* tab, const float4* tiles, const float* cube, int N, int nt, float alphaSqr,
                                                               float cutoff, float* out) {
    const int tid = threadIdx.x;
    const int bt = blockIdx.x, bs = bt / (nt * nt), bty = (bt / nt) % nt, btx = bt % nt;
    const int ox = btx * 16 + (tid & 15), oy = bty * 16 + (tid >> 4);
    const bool valid = ox < N && oy < N;
    const long o = ((long)bs * N + (valid ? oy : 0)) * N + (valid ? ox : 0);
    const float4 V = tab[o];
    float wsum = 0.f, col[3] = {0.f, 0.f, 0.f}, wref = 0.f;
    const int ntiles = 6 * nt * nt;
    for (int t = 0; t < ntiles; ++t) {
        const float4 tl = tiles[t];
        if (!(valid && (V.x * tl.x + V.y * tl.y) + V.z * tl.z >= tl.w)) continue;
        const int s = t / (nt * nt), y0 = ((t / nt) % nt) * 16, x0 = (t % nt) * 16;
        const int y1 = min(y0 + 16, N), x1 = min(x0 + 16, N);
        for (int y = y0; y < y1; ++y)
            for (int x = x0; x < x1; ++x) {
                const long j = ((long)s * N + y) * N + x;
                const float4 L = tab[j];
                const float d = (L.x * V.x + L.y * V.y) + L.z * V.z;
                if (!(d >= cutoff)) continue;
                float hx = L.x + V.x, hy = L.y + V.y, hz = L.z + V.z;
                const float hl = sqrtf((hx * hx + hy * hy) + hz * hz);
                if (hl > 0.f) { hx /= hl; hy /= hl; hz /= hl; } else { hx = hy = hz = 0.f; }
                const float wi = fmaxf(d, 0.f);
                const float vh = fminf(fmaxf((V.x * hx + V.y * hy) + V.z * hz, 0.f), 1.0f);
                const float dd = (vh * alphaSqr - vh) * vh + 1.0f;
                const float ndf = alphaSqr / ((dd * dd) * 3.14159265358979f);
                const float w = ((wi * ndf) * L.w) / 4.0f;
                if (!(w > 0.f)) continue;      // adds exact zeros in the reference
                float wr = 1.0f;
                if (wref == 0.f) wref = w; else wr = w / wref;
                col[0] = fmaf(cube[3 * j], wr, col[0]);
                col[1] = fmaf(cube[3 * j + 1], wr, col[1]);
                col[2] = fmaf(cube[3 * j + 2], wr, col[2]);
                wsum += wr;
            }
    }
    if (valid) { out[3 * o] = col[0] / wsum; out[3 * o + 1] = col[1] / wsum; out[3 * o + 2] = col[2] / wsum; }
}

extern "C" int utx_launch_cubemap_specular(const float* cube, int N, const float* texels, const float* tiles, float roughness, float costheta_cutoff,
                                           float* out, hipStream_t stream) {
    if (N < 2 || (N & 1) || N > 8192 || !(roughness > 0.f)) return -2;
    const int nt = (N + 15) / 16;
    const float alpha = roughness * roughness;
    hipLaunchKernelGGL(cubemap_specular_kernel, dim3(6 * nt * nt), dim3(256), 0, stream, (const float4*)texels, (const float4*)tiles, cube, N, nt,
                       alpha * alpha, costheta_cutoff, out);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---------------------------------------------------------------------------------------------------------------- split-sum DFG table
// out[j][i] = (scale, bias) at cos(theta) = (i + 0.5) / R (x, the column) and roughness = (j + 0.5) / R (y, the row), the layout PBRModel indexes its FG_LUT with.
// Estimator (Karis' split sum, GGX importance sampling over the Hammersley set (k / n, radical inverse base 2 of k), k = 0 .. n - 1), a = roughness^2:
//   V = (sqrt(1 - c^2), 0, c);  cos^2 th = (1 - y) / ((1 - y) + a^2 y), sin^2 th = a^2 y / ((1 - y) + a^2 y), phi = 2 pi x;  H = (sin th cos phi, sin th sin phi, cos th)
//   L = 2 (V.H) H - V;  if L.z > 0:  Vis = 0.5 / (N.L sqrt(N.V^2 (1 - a^2) + a^2) + N.V sqrt(N.L^2 (1 - a^2) + a^2))   (height-correlated Smith GGX, the G term the
//   reference's bsdf_256_256.bin was made with: DESIGN 8);  Gv = Vis * 4 N.L (V.H) / N.H;  Fc = (1 - V.H)^5
//   scale += (1 - Fc) Gv, bias += Fc Gv;  both / n.
// One thread per table entry; the samples add up in order inside blocks of 32 and the blocks in order (fixed).
__global__ __launch_bounds__(256) void dfg_lut_kernel(int R, int nsamples, float* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= R * R) return;
    const float c = ((float)(i % R) + 0.5f) / (float)R, rough = ((float)(i / R) + 0.5f) / (float)R;
    const float a = rough * rough, a2 = a * a;
    const float vx = sqrtf(1.0f - c * c), vz = c;
    const float lv = sqrtf(vz * vz * (1.0f - a2) + a2);
    float A = 0.f, B = 0.f;
    for (int k0 = 0; k0 < nsamples; k0 += 32) {
        float pa = 0.f, pb = 0.f;
        const int k1 = min(k0 + 32, nsamples);
        for (int q = k0; q < k1; ++q) {
            const float x = (float)q / (float)nsamples;
            const float y = (float)__brev((unsigned)q) * 2.3283064365386963e-10f;      // * 2^-32
            const float den = (1.0f - y) + a2 * y;
            const float ct = sqrtf((1.0f - y) / den), st = sqrtf((a2 * y) / den);
            float sp, cp;
            sincosf(6.2831853071795865f * x, &sp, &cp);
            const float hx = st * cp, hz = ct;
            const float vh = vx * hx + vz * hz;
            const float lz = 2.0f * vh * hz - vz;
            if (lz > 0.f && vh > 0.f && hz > 0.f) {
                const float vis = 0.5f / (lz * lv + vz * sqrtf(lz * lz * (1.0f - a2) + a2));
                const float gv = vis * 4.0f * lz * vh / hz;
                const float m = 1.0f - vh, m2 = m * m, fc = m2 * m2 * m;
                pa += (1.0f - fc) * gv;
                pb += fc * gv;
            }
        }
        A += pa; B += pb;
    }
    out[2 * i] = A / (float)nsamples;
    out[2 * i + 1] = B / (float)nsamples;
}

extern "C" int utx_launch_dfg_lut(int R, int nsamples, float* out, hipStream_t stream) {
    if (R <= 0 || R > 4096 || nsamples <= 0 || nsamples > (1 << 24)) return -2;
    hipLaunchKernelGGL(dfg_lut_kernel, dim3((R * R + 255) / 256), dim3(256), 0, stream, R, nsamples, out);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---------------------------------------------------------------------------------------------------------------- lookups
// FG_LUT lookup: dr.texture(filter 'linear', boundary 'clamp') of a [R][R][2] table at (x, y) in [0, 1]
__device__ __forceinline__ void pbr_lut_lookup(const float* lut, int R, float x, float y, float& fg0, float& fg1) {
    const float tx = x * (float)R - 0.5f, ty = y * (float)R - 0.5f;
    const float bx = floorf(tx), by = floorf(ty);
    const float wx = tx - bx, wy = ty - by;
    const int x0 = min(max((int)bx, 0), R - 1), x1 = min(max((int)bx + 1, 0), R - 1);
    const int y0 = min(max((int)by, 0), R - 1), y1 = min(max((int)by + 1, 0), R - 1);
    const float* t00 = lut + 2 * ((long)y0 * R + x0);
    const float* t01 = lut + 2 * ((long)y0 * R + x1);
    const float* t10 = lut + 2 * ((long)y1 * R + x0);
    const float* t11 = lut + 2 * ((long)y1 * R + x1);
    float r[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float top = t00[k] + wx * (t01[k] - t00[k]);
        const float bot = t10[k] + wx * (t11[k] - t10[k]);
        r[k] = top + wy * (bot - top);
    }
    fg0 = r[0]; fg1 = r[1];
}

__global__ __launch_bounds__(256) void cube_sample_kernel(const float* cube, int N, const float* dirs, long n, float* out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float o[3];
    pbr_cube_lookup(cube, N, dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2], o);
    out[3 * i] = o[0]; out[3 * i + 1] = o[1]; out[3 * i + 2] = o[2];
}

extern "C" int utx_launch_cube_sample(const float* cube, int N, const float* dirs, long n, float* out, hipStream_t stream) {
    if (N <= 0 || N > 8192 || n <= 0) return -2;
    hipLaunchKernelGGL(cube_sample_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, cube, N, dirs, n, out);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---------------------------------------------------------------------------------------------------------------- PBRModel.forward
// pbr.py:110-130 on one pixel, every sum in a fixed order:
//   nrm = n / max(|n|, 1e-12);  wo = normalize(eye - p);  wi = normalize(2 (wo.nrm) nrm - wo);  c = clamp(wo.nrm, 0, 1)
//   kd = albedo (1 - metallic) + 0 metallic;  ks = (0.04 (1 - metallic) + albedo metallic) (1 - 0.5) + 0 * 0.5      (the constant 0.5 "specular" term)
//   diffuse = kd * light_diffuse[nrm];  specular = (ks * FG[c, roughness].x + FG[c, roughness].y) * light_specular[wi]
struct PbrLights { const float* diff; int Nd; const float* spec; int Ns; const float* lut; int R; };

__device__ __forceinline__ void pbr_eval(const PbrLights& L, const float eye[3], const float p[3], const float n_in[3], const float albedo[3], float rough,
                                         float metal, float diffuse[3], float specular[3]) {
    float nrm[3] = {n_in[0], n_in[1], n_in[2]};
    sd_normalize3(nrm);
    float wo[3] = {eye[0] - p[0], eye[1] - p[1], eye[2] - p[2]};
    sd_normalize3(wo);
    const float dn = sd_dot3(wo, nrm);
    float wi[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) wi[k] = (2.0f * dn) * nrm[k] - wo[k];
    sd_normalize3(wi);
    const float c = fminf(fmaxf(dn, 0.0f), 1.0f);
    float ld[3], ls[3], fg0, fg1;
    pbr_cube_lookup(L.diff, L.Nd, nrm[0], nrm[1], nrm[2], ld);
    pbr_cube_lookup(L.spec, L.Ns, wi[0], wi[1], wi[2], ls);
    pbr_lut_lookup(L.lut, L.R, c, rough, fg0, fg1);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float kd = albedo[k] * (1.0f - metal) + 0.0f * metal;
        const float ks = (0.04f * (1.0f - metal) + albedo[k] * metal) * (1.0f - 0.5f) + 0.0f * 0.5f;
        diffuse[k] = kd * ld[k];
        specular[k] = (ks * fg0 + fg1) * ls[k];
    }
}

// dense form for callers that hold the buffers already (PBRModel.forward): eye [npix][3] or one [3] (eye_stride 0), Kd [npix][kd_stride >= 3], Ks [npix][3]
__global__ __launch_bounds__(256) void pbr_forward_kernel(PbrLights L, const float* eye, int eye_stride, const float* pos, const float* nrm, const float* kd,
                                                          int kd_stride, const float* ks, long npix, float* out_diffuse, float* out_specular) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const float* e = eye + (long)eye_stride * i;
    const float ev[3] = {e[0], e[1], e[2]}, p[3] = {pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]}, n[3] = {nrm[3 * i], nrm[3 * i + 1], nrm[3 * i + 2]};
    const float al[3] = {kd[(long)kd_stride * i], kd[(long)kd_stride * i + 1], kd[(long)kd_stride * i + 2]};
    float d[3], s[3];
    pbr_eval(L, ev, p, n, al, ks[3 * i + 1], ks[3 * i + 2], d, s);
#pragma unroll
    for (int k = 0; k < 3; ++k) { out_diffuse[3 * i + k] = d[k]; out_specular[3 * i + k] = s[k]; }
}

extern "C" int utx_launch_pbr_forward(const float* eye, int eye_stride, const float* pos, const float* nrm, const float* kd, int kd_stride, const float* ks,
                                      const float* light_diffuse, int Nd, const float* light_specular, int Ns, const float* lut, int R, long npix,
                                      float* out_diffuse, float* out_specular, hipStream_t stream) {
    if (npix <= 0 || Nd <= 0 || Ns <= 0 || R <= 0 || Nd > 8192 || Ns > 8192 || kd_stride < 3 || (eye_stride != 0 && eye_stride != 3)) return -2;
    const PbrLights L = {light_diffuse, Nd, light_specular, Ns, lut, R};
    hipLaunchKernelGGL(pbr_forward_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, L, eye, eye_stride, pos, nrm, kd, kd_stride, ks, npix,
                       out_diffuse, out_specular);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---------------------------------------------------------------------------------------------------------------- tangent-space normal map
// bsdf_prepare_shading_normal (texture/pbr/renderutils/bsdf.py:28-51) with two_sided_shading = True and opengl = True (glTF's convention) on one pixel,
// every sum in a fixed order; normalize is F.normalize (x / max(|x|, 1e-12), sd_normalize3):
//   sn = normalize(smooth_nrm);  st = normalize(smooth_tng);  vv = normalize(eye - pos);  b = normalize(cross(st, sn))
//   s = normalize((st p.x - b p.y) + sn max(p.z, 0))
//   dot(geom_nrm, vv) > 0 ? (s, g) = (s, geom_nrm) : (-s, -geom_nrm)
//   t = clamp(dot(vv, s) / 0.1, 0, 1);  out = g + t (s - g)
// out is not normalised (pbr_eval normalises its input).  A zero tangent, a tangent parallel to the normal, a zero perturbation and a negative p.z all
// stay finite: the 1e-12 floors turn a zero vector into a zero vector, and s = 0 gives t = 0, out = g.
__device__ __forceinline__ void pbr_shading_normal(const float eye[3], const float pos[3], const float p[3], const float smooth_nrm[3], const float smooth_tng[3],
                                                   const float geom_nrm[3], float out[3]) {
    float sn[3] = {smooth_nrm[0], smooth_nrm[1], smooth_nrm[2]}, st[3] = {smooth_tng[0], smooth_tng[1], smooth_tng[2]};
    float vv[3] = {eye[0] - pos[0], eye[1] - pos[1], eye[2] - pos[2]};
    sd_normalize3(sn);
    sd_normalize3(st);
    sd_normalize3(vv);
    float b[3] = {st[1] * sn[2] - st[2] * sn[1], st[2] * sn[0] - st[0] * sn[2], st[0] * sn[1] - st[1] * sn[0]};
    sd_normalize3(b);
    const float pz = fmaxf(p[2], 0.0f);
    float s[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) s[k] = (st[k] * p[0] - b[k] * p[1]) + sn[k] * pz;
    sd_normalize3(s);
    const bool front = sd_dot3(geom_nrm, vv) > 0.0f;
    float g[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { s[k] = front ? s[k] : -s[k]; g[k] = front ? geom_nrm[k] : -geom_nrm[k]; }
    const float t = fminf(fmaxf(sd_dot3(vv, s) / 0.1f, 0.0f), 1.0f);
#pragma unroll
    for (int k = 0; k < 3; ++k) out[k] = g[k] + t * (s[k] - g[k]);
}

// dense form, the counterpart of pbr_forward_kernel: eye [npix][3] or one [3] (eye_stride 0), everything else [npix][3]
__global__ __launch_bounds__(256) void pbr_shading_normal_kernel(const float* eye, int eye_stride, const float* pos, const float* pert, const float* snrm,
                                                                 const float* stng, const float* gnrm, long npix, float* out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const float* e = eye + (long)eye_stride * i;
    const float ev[3] = {e[0], e[1], e[2]}, p[3] = {pos[3 * i], pos[3 * i + 1], pos[3 * i + 2]}, pt[3] = {pert[3 * i], pert[3 * i + 1], pert[3 * i + 2]};
    const float n[3] = {snrm[3 * i], snrm[3 * i + 1], snrm[3 * i + 2]}, t[3] = {stng[3 * i], stng[3 * i + 1], stng[3 * i + 2]};
    const float g[3] = {gnrm[3 * i], gnrm[3 * i + 1], gnrm[3 * i + 2]};
    float o[3];
    pbr_shading_normal(ev, p, pt, n, t, g, o);
    out[3 * i] = o[0]; out[3 * i + 1] = o[1]; out[3 * i + 2] = o[2];
}

extern "C" int utx_launch_pbr_shading_normal(const float* eye, int eye_stride, const float* pos, const float* pert, const float* snrm, const float* stng,
                                             const float* gnrm, long npix, float* out, hipStream_t stream) {
    if (npix <= 0 || (eye_stride != 0 && eye_stride != 3)) return -2;
    hipLaunchKernelGGL(pbr_shading_normal_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, stream, eye, eye_stride, pos, pert, snrm, stng, gnrm, npix,
                       out);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

// ---------------------------------------------------------------------------------------------------------------- fused frame
// NVDiffRendererPBR.render_base + render_pbr (renderer_pbr.py:19-94) for one frame: position, normal and uv interpolate as utx_interpolate does (same
// operations, same order: sd_interp); Kd / Ks fetch as utx_texture_shade does (sd_tex3_wrap: bilinear, wrap, t00 (1 - fx) + t01 fx); PBRModel.forward; rgb = ld diffuse + ls specular;
// torch.lerp(bg, rgb, alpha) with alpha = coverage in {0, 1} is a select; uint8 = clamp * 255 truncated.  ks == nullptr: the reference's default
// [1, 1, 0] expanded to Kd's size (renderer_pbr.py:24-26): sd_tex3_wrap_const, bit-identical to that constant texture.
// NM = true (utx_pbr_shade_nm): the tangent interpolates as the normal does, the map fetches as Kd does and decodes as p = 2 texel - 1 (not normalised),
// pbr_shading_normal with the triangle's face normal as the geometric one replaces the interpolated normal in front of pbr_eval.  NM = false is
// utx_pbr_shade: none of that is compiled in and its arithmetic is what it was.
struct PbrNormalMap { const float* vtng; const float* fnrm; const float* nm; int Hn, Wn; };

template <bool NM>
__global__ __launch_bounds__(256) void pbr_shade_kernel(PbrLights L, PbrNormalMap M, const float4* rast, const int* tri, const float* vpos, const float* vnrm,
                                                        const float* vuv, const float* kd, int Hk, int Wk, const float* ks, int Hs, int Ws, float e0, float e1,
                                                        float e2, float lam_d, float lam_s, float bg0, float bg1, float bg2, long npix, unsigned char* out_u8,
                                                        float4* out_rgba) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npix) return;
    const float4 r = rast[i];
    const int id = (int)r.w - 1;
    float c[3] = {bg0, bg1, bg2};
    const float a = id >= 0 ? 1.0f : 0.0f;
    if (id >= 0) {
        const float u = r.x, v = r.y, w = sd_bary_w(u, v);
        const long i0 = tri[3 * id + 0], i1 = tri[3 * id + 1], i2 = tri[3 * id + 2];
        float p[3], n[3], uv[2];
        sd_interp<3>(vpos + 3 * i0, vpos + 3 * i1, vpos + 3 * i2, u, v, w, p);
        sd_interp<3>(vnrm + 3 * i0, vnrm + 3 * i1, vnrm + 3 * i2, u, v, w, n);
        sd_interp<2>(vuv + 2 * i0, vuv + 2 * i1, vuv + 2 * i2, u, v, w, uv);
        float al[3], arm[3];
        sd_tex3_wrap(kd, Hk, Wk, uv[0], uv[1], al);
        const float ks_default[3] = {1.0f, 1.0f, 0.0f};
        if (ks) sd_tex3_wrap(ks, Hs, Ws, uv[0], uv[1], arm);
        else sd_tex3_wrap_const(ks_default, Hk, Wk, uv[0], uv[1], arm);
        const float eye[3] = {e0, e1, e2};
        if constexpr (NM) {
            float tg[3], tx[3];
            sd_interp<3>(M.vtng + 3 * i0, M.vtng + 3 * i1, M.vtng + 3 * i2, u, v, w, tg);
            sd_tex3_wrap(M.nm, M.Hn, M.Wn, uv[0], uv[1], tx);
            const float pt[3] = {2.0f * tx[0] - 1.0f, 2.0f * tx[1] - 1.0f, 2.0f * tx[2] - 1.0f};
            const float g[3] = {M.fnrm[3 * (long)id], M.fnrm[3 * (long)id + 1], M.fnrm[3 * (long)id + 2]};
            const float sm[3] = {n[0], n[1], n[2]};
            pbr_shading_normal(eye, p, pt, sm, tg, g, n);
        }
        float d[3], s[3];
        pbr_eval(L, eye, p, n, al, arm[1], arm[2], d, s);
#pragma unroll
        for (int k = 0; k < 3; ++k) c[k] = lam_d * d[k] + lam_s * s[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) out_u8[3 * i + k] = sd_to_u8(c[k]);
    if (out_rgba) out_rgba[i] = make_float4(c[0], c[1], c[2], a);
}

static int pbr_shade_launch(const PbrNormalMap* M, const float* rast, const int* tri, const float* vpos, const float* vnrm, const float* vuv, const float* kd, int Hk,
                            int Wk, const float* ks, int Hs, int Ws, const float* eye3_host, const float* light_diffuse, int Nd, const float* light_specular,
                            int Ns, const float* lut, int R, float lambda_diffuse, float lambda_specular, const float* bg3_host, long npix, void* out_u8,
                            float* out_rgba, hipStream_t stream) {
    if (npix <= 0 || Hk <= 0 || Wk <= 0 || (ks && (Hs <= 0 || Ws <= 0)) || Nd <= 0 || Ns <= 0 || R <= 0 || Nd > 8192 || Ns > 8192 || !eye3_host || !bg3_host)
        return -2;
    const PbrLights L = {light_diffuse, Nd, light_specular, Ns, lut, R};
    const PbrNormalMap none = {nullptr, nullptr, nullptr, 0, 0};
    const dim3 grid((unsigned)((npix + 255) / 256));
    const auto kernel = M ? pbr_shade_kernel<true> : pbr_shade_kernel<false>;
    hipLaunchKernelGGL(kernel, grid, dim3(256), 0, stream, L, M ? *M : none, (const float4*)rast, tri, vpos, vnrm, vuv,
                       kd, Hk, Wk, ks, Hs, Ws, eye3_host[0], eye3_host[1], eye3_host[2], lambda_diffuse, lambda_specular, bg3_host[0], bg3_host[1], bg3_host[2], npix,
                       (unsigned char*)out_u8, (float4*)out_rgba);
    return hipGetLastError() == hipSuccess ? 0 : -4;
}

extern "C" int utx_launch_pbr_shade(const float* rast, const int* tri, const float* vpos, const float* vnrm, const float* vuv, const float* kd, int Hk, int Wk,
                                    const float* ks, int Hs, int Ws, const float* eye3_host, const float* light_diffuse, int Nd,
                                    const float* light_specular, int Ns, const float* lut, int R, float lambda_diffuse, float lambda_specular,
                                    const float* bg3_host, long npix, void* out_u8, float* out_rgba, hipStream_t stream) {
    return pbr_shade_launch(nullptr, rast, tri, vpos, vnrm, vuv, kd, Hk, Wk, ks, Hs, Ws, eye3_host, light_diffuse, Nd, light_specular, Ns, lut, R, lambda_diffuse,
                            lambda_specular, bg3_host, npix, out_u8, out_rgba, stream);
}

extern "C" int utx_launch_pbr_shade_nm(const float* rast, const int* tri, const float* vpos, const float* vnrm, const float* vtng, const float* fnrm, const float* vuv,
                                       const float* kd, int Hk, int Wk, const float* ks, int Hs, int Ws, const float* nm, int Hn, int Wn, const float* eye3_host,
                                       const float* light_diffuse, int Nd, const float* light_specular, int Ns, const float* lut, int R, float lambda_diffuse,
                                       float lambda_specular, const float* bg3_host, long npix, void* out_u8, float* out_rgba, hipStream_t stream) {
    if (!vtng || !fnrm || !nm || Hn <= 0 || Wn <= 0) return -2;
    const PbrNormalMap M = {vtng, fnrm, nm, Hn, Wn};
    return pbr_shade_launch(&M, rast, tri, vpos, vnrm, vuv, kd, Hk, Wk, ks, Hs, Ws, eye3_host, light_diffuse, Nd, light_specular, Ns, lut, R, lambda_diffuse,
                            lambda_specular, bg3_host, npix, out_u8, out_rgba, stream);
}

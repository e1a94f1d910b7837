// Internal launcher prototypes shared by the .hip files and capi.cpp.  The parameter structs ARE
// the public descriptors of include/unitex_hip.h (single source of truth for the layout).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/unitex_hip.h"
#ifndef UTX_BF16_T
#define UTX_BF16_T
typedef uint16_t bf16_t;
#endif

struct AttnParams {
    const bf16_t* q;
    const bf16_t* k;
    const bf16_t* vt;
    bf16_t* o;
    long q_hs, q_ss, k_hs, k_ss, vt_hs, vt_ds, o_ss;  // element strides
    int H, S, nqb;
    int Sq;            // query rows (0 = S): attention_glds.hip only
    int dbg;           // perf ablation only (UTX_ATTN_DEBUG; always 0 in the product library).  Its bits switched phases of the register-staged kernel off; no remaining kernel reads it
    float scale_log2;  // softmax_scale * log2(e)
    unsigned char* flags;  // per (head, 64-query group) overflow marks: written by the 4 x 64 kernel, read by the repair pass (else null)
    int flag_hs;           // flags per head
    // tail split (attention_glds.hip): work items [w_base, ...) of this launch, each cut into nsplit key ranges of
    // tiles_per_split 64-key tiles; a split writes its normalised partial output + log2-sum-exp instead of the final rows
    int w_base, nsplit, tiles_per_split;
    bf16_t* part_o;        // [items][nsplit][256][128] bf16
    float* part_lse;       // [items][nsplit][256] f32: running maximum + log2(row sum)
    // key multiplicity (text-token dedup, flux/transformer.py): the keys of tile 0 -- and of every tile whose index is a multiple of
    // key_bias_period when that is > 0 -- stand for 2^key_bias_log2 identical keys each: key_bias_log2 is added to their scores
    float key_bias_log2;
    int key_bias_period;
    // caller-owned scratch of the tail split (utx_attn_workspace_bytes); null / too small: the launch stays unsplit
    void* work;
    size_t work_bytes;
    // block-strided operands (attention_glds.hip, BLK): tokens in blocks of blk_rows (0 = contiguous) lying q_bs / k_bs / vt_bs elements apart
    int blk_rows;
    long q_bs, k_bs, vt_bs;
};
// MX fp8 attention (attention_fp8.hip; opt-in): e4m3 operands with E8M0 block scales
struct Attn8Params {
    const uint8_t *q8, *k8;      // [H][S_pad][128] e4m3
    const uint8_t* v8t;          // [H][128][S_pad] e4m3
    const uint32_t *qs, *ks;     // [H][S_pad]: four E8M0 bytes per row (32-channel blocks of d)
    const uint32_t* vs;          // [H][S_pad / 32][32]: dword of row d % 32 = the E8M0 bytes of channels d % 32 + {0, 32, 64, 96} for that block of 32 keys
    bf16_t* o;
    long o_ss;
    int H, S, Sq, S_pad, nqb;
    float key_bias_log2;
    int key_bias_period;
    // key-split tail round (round 6; the bf16 kernel's plan, work items and merge -- AttnParams above): filled by the launcher from `work`
    int w_base, nsplit, tiles_per_split;
    bf16_t* part_o;
    float* part_lse;
    void* work;            // caller-owned scratch (utx_attn_workspace_bytes); null / too small: the launch stays unsplit
    size_t work_bytes;
};
// Launch options.  Every field is result-preserving (kernel selection / scheduling A/B): read ONCE from the environment by
// the first utx_init (UTX_ATTN_*, UTX_GEMM_* variables of the same names), afterwards changed only through utx_set_option.
// The three `*_abl` fields switch timing ablations that compute WRONG results; they exist only in the UTX_ABLATION build
// (libunitex_hip_ablate.so, used by tools/ -- never by the product, the tests or bench.py).
// A field's default is written beside it; g_utx_opt (capi.cpp) is default-initialised.
struct UtxOptions {
    int attn_q64 = 1;         // 1 (default since round 6): launches the 4 x 64 kernel takes (attention_q64.hip: pre-scaled Q, whole 64-key tiles, contiguous operands, caller scratch) run it
                              // + its repair pass; 0: the 8 x 32 kernel everywhere (A/B; bit-identical wherever the 8 x 32 kernel does not re-centre behind the first block)
    int attn_tailsplit = 1;   // 1 (default): key-split tail round
    int gemm_group_m = 0;     // 0 = built-in GROUP_M
    int gemm_tile = 0;        // 0 auto, 128, 2564 (one wave per SIMD); any other value is refused with -2 (gemm.hip gemm_tile_known)
    int gemm_pers_grid = 0;   // one-wave-per-SIMD GEMM: number of workgroups of its persistent grid (0 = one per CU)
    int gemm_streamk = 1;     // 1 (default): one-wave-per-SIMD GEMM balances the K loops of its last, partly filled round over all CUs (needs utx_gemm_desc.sk_work)
    int bvh_stack_walk = 0;   // 1: the reference's stack walk over the unpacked tree instead of the stackless packed walk (A/B; same results)
    int attn_var_abl = 0, attn_debug_abl = 0, gemm_debug_abl = 0;      // gemm_debug_abl (UTX_GEMM_DEBUG): no remaining kernel reads it (its readers were the retired 256^2 kernels)
    int bvh_packet = 1;       // 1 (default): back-projection rays walk the tree as wave-wide packets over 8 x 8 texel tiles (bvh_trace_packet); 0: one thread per ray (A/B; same results)
    int attn_peel = 1;        // 1 (default since round 5): the pre-scaled 8 x 32 attention launch runs its fast loop (attention_glds.hip, FAST: first / ragged tile outside the loop, the tile's
                              // barrier between S2 and S3, next tile's first K fragments read under S3); 0: the general loop (the default until round 4).  Same bits either way.
    int attn8_peel = 1;       // 1 (default since round 5): MX fp8 attention with tile 0 / a ragged last tile outside the loop and the loop's exponentials in quarters under the PV MFMAs
                              // (attn_fwd_fp8_kernel<1>, attention_fp8.hip); 0: the general loop.  Same bits either way.
    int gemm_fastk = 1;       // one-wave-per-SIMD GEMM (bf16): 1 (default since round 6: +2.3 ... +3.7 % on the FLUX shapes, profiles/r06_gemm_fastk_check_v0.log) = the steady-state K loop runs the generated instruction stream (gemm_w4_loop_asm.inc), 0 = hipcc's loop (round 2-5).  Same bits.
    int nn_grid = 0;          // 0 (default): the NN fill's cell grid follows the atlas size; 64 | 128 | 256 force one (A/B and the grid-independence test; same results)
};
extern UtxOptions g_utx_opt;

typedef utx_gemm_desc GemmParams;
typedef utx_knn_desc KnnParams;
typedef utx_gemv_desc GemvParams;
typedef utx_qkv_post_desc QkvPostParams;
typedef utx_ln_mod_desc LnModParams;
typedef utx_sched_desc SchedParams;

extern "C" {
int utx_launch_attn_fwd(const void* q, const void* k, const void* vt, void* o,
                        long q_hs, long q_ss, long k_hs, long k_ss, long vt_hs, long vt_ds,
                        long o_ss, int H, int S, int Sq, float scale, float key_bias_log2, int key_bias_period, void* work, size_t work_bytes, hipStream_t stream);
void utx_attn_split_plan_impl(int H, int Sq, int S, int ncu, int out[4]);     // attention_glds.hip (pure): {workgroups, in full rounds, key ranges per tail workgroup, tiles per range}
size_t utx_attn_workspace_bytes_impl(int H, int Sq, int S, int ncu);      // [tail-split scratch | 4 x 64 kernel's headroom flags]
size_t utx_attn_split_bytes_impl(int H, int Sq, int S, int ncu);
size_t utx_attn_q64_flag_bytes(int H, int Sq, int S);                    // attention_q64.hip
int utx_attn_q64_takes(const AttnParams* p, int presc);                  // attention_q64.hip: shape, layout and scratch fit the 4 x 64 kernel
int utx_launch_attn_merge(const AttnParams* t, int n_items, hipStream_t stream);
int utx_launch_attn_fwd_glds(const AttnParams* p, int presc, hipStream_t stream);
int utx_launch_attn_fwd_fp8(const Attn8Params* p, hipStream_t stream);                                   // attention_fp8.hip
int utx_launch_quant_vt_mx8(const void* vt, void* v8, void* vs, int H, int S_pad, hipStream_t stream);   // attention_fp8.hip
int utx_launch_attn_fwd_blk(const void* q, const void* k, const void* vt, void* o, long q_hs, long q_ss, long k_hs, long k_ss, long vt_hs, long vt_ds,
                            long o_ss, int H, int S, int Sq, float scale, float key_bias_log2, int key_bias_period, void* work, size_t work_bytes,
                            int blk_rows, long q_bs, long k_bs, long vt_bs, hipStream_t stream);
int utx_launch_attn_fwd_q64(const AttnParams* p, int presc, hipStream_t stream);
int utx_launch_gemm_bf16(const GemmParams* p, hipStream_t stream);
size_t utx_gemm_streamk_workspace_bytes_impl(void);
int utx_gemm_plan_impl(const GemmParams* p, int ncu, int sk_has_work, int out[4]);           // gemm.hip: kernel choice + split of the last round (pure); -2: unknown UTX_GEMM_TILE
void utx_gemm_w4_split_plan(const GemmParams* p, int tiles, int grid, int has_work, int* T, int* S);   // gemm_w4.hip (pure)
int utx_launch_gemm_w4(GemmParams p, hipStream_t stream);     // gemm_w4.hip: persistent 256x256 kernel, one wave per SIMD
int utx_launch_gemv_bf16(const GemvParams* p, hipStream_t stream);
int utx_launch_quant_mx8(const void* x, long ldx, void* q, long ldq, void* s, long lds, int M, int K, hipStream_t stream);
int utx_launch_quant_mx8_packed(const void* x, long ldx, void* q, long ldq, void* s, long row_blocks, int M, int K, hipStream_t stream);
int utx_launch_qkv_post(const QkvPostParams* p, hipStream_t stream);
int utx_launch_sp_unpack_qkv(const void* recv, int P, int Hp, int S_loc, int text_rows, void* q, void* k, void* vt, hipStream_t stream);
int utx_launch_sp_unpack_o(const void* recv, int P, int Hp, int S_loc, void* out, long ld, long src_cols, hipStream_t stream);
size_t utx_group_norm_workspace_bytes_impl(void);
int utx_launch_group_norm(const void* x, long npix, int C, const void* gamma, const void* beta, float eps, int silu, void* y, void* work, hipStream_t stream);
int utx_launch_softmax_rows(void* s, long nrow, long ld, int ncol, hipStream_t stream);
int utx_launch_conv3x3_thin(const void* x, int H, int W, int Cin, const void* wt, const void* bias, int Cout, void* y, hipStream_t stream);
int utx_launch_ln_mod(const LnModParams* p, hipStream_t stream);
int utx_launch_sched_step(const SchedParams* p, hipStream_t stream);
int utx_launch_transform(const float* verts, int V, const float* mvp, int n_views, float* clip, float* ndc, hipStream_t stream);
int utx_launch_rasterize(const float* pos, const int* tri, int F, int H, int W, float* rast, void* work, hipStream_t stream);
int utx_launch_interpolate(const float* attr, int C, const float* rast, const int* tri, long npix, float* out, hipStream_t stream);
int utx_launch_condition_shade(const float* rast, const float* nrm, const float* pos, const float* bg3_host, long npix, void* out_normal, void* out_ccm, void* out_alpha, hipStream_t stream);
int utx_launch_face_normals(const float* verts, const int* faces, int F, float* out, hipStream_t stream);
int utx_launch_view_visibility(const float* attr6, const float* rast, const float* fnormal, const float* dirs, const float* eyes, int n, int H, int W,
                               float grad_thr, float cos_thr, int radius, void* tmp, void* vis, float* alpha, hipStream_t stream);
size_t utx_knn_workspace_bytes_impl(long N);
int utx_launch_knn(const KnnParams* p, void* work, size_t work_bytes, hipStream_t stream);
size_t utx_fps_workspace_bytes_impl(long N);      // sampling.hip
int utx_launch_fps(const float* pos, const unsigned char* mask, long N, int M, int start, int* out_idx, float* out_d2, void* work, size_t work_bytes, hipStream_t stream);
int utx_launch_sample_edges(const float* verts, const int* edges, const int* edge_ids, const float* start, const float* length, int E, float total, long N,
                            float* samples, int* edge_index, float* edge_t, hipStream_t stream);
int utx_launch_sample_surface(const float* verts, const int* faces, const float* cum, int F, long N, unsigned long long seed, float* samples, int* face_index,
                              float* uvw, hipStream_t stream);
int utx_launch_sample_offsets(const float* base, const int* faces, int F, const int* face_index, const float* uvw, const float* vnormal, const float* uniforms, long N,
                              unsigned long long seed, int stream_id, float threshold, float* out, hipStream_t stream);
int utx_launch_sample_attrs(const int* faces, const int* faces_2d, const float* uvs_2d, int F, const int* face_index, const float* uvw, long N, int n_attr,
                            const float* const* src_host, const int* dims_host, float* const* out_host, hipStream_t stream);
int utx_launch_texture_shade(const float* rast, const float* uv, const int* tri, const float* tex, int Ht, int Wt, const float* bg3_host, long npix, void* out, hipStream_t stream);
// gbuffer.hip
int utx_launch_gbuffer_shade(int mode, const float* rast, const int* tri, const float* attr, int stride, const float* scale2, int ndc, int composite, const float* bg3_host, long npix, void* out_u8, float* out_rgba, hipStream_t stream);
int utx_launch_gbuffer_range(int mode, const float* rast, const int* tri, const float* attr, int stride, long npix, float* scale2, int* empty, hipStream_t stream);
int utx_launch_camera_normals(const float* nrm, int V, const float* c2ws, int n_views, float* out, hipStream_t stream);
int utx_launch_uv_gbuffer(const float* rast, const int* tri, const float* v_pos, const float* v_nrm, const float* v_pos_cam, const float* v_nrm_cam, int V, int B, int H2D, int W2D,
                          unsigned want, void* const* outs_host, hipStream_t stream);
int utx_launch_screen_gbuffer(const float* rast, const int* tri, const float* v_pos, const float* v_nrm, const float* v_uv, const float* v_attr, int Ca, const float* clip_w,
                              const float* v_pos_cam, const float* v_nrm_cam, int V, int B, int H, int W, int n_maps, const float* const* maps_host, const int* map_dims_host,
                              int filter, int bg_kind, float bg_scalar, const float* bg_v_attr, const float* bg_map_attr, unsigned want, void* const* outs_host, hipStream_t stream);
int utx_launch_uv_project(const float* rast2d, const int* tri, int F, const unsigned char* face_mask, const float* v_ndc, int V, int B, int H2D, int W2D, const float* map,
                          int Bm, int Hm, int Wm, int C, const float* rast_map, int filter, int bg_kind, float bg_scalar, const float* bg, float* uv, float* uv_alpha,
                          float* map_attr, hipStream_t stream);
// pbr.hip
int utx_cubemap_table_impl(int N, float costheta_cutoff, float* texels_host, float* tiles_host);
int utx_launch_latlong_to_cubemap(const float* lat, int Hi, int Wi, int N, float* out, hipStream_t stream);
int utx_launch_cubemap_diffuse(const float* cube, int N, const float* texels, float* out, hipStream_t stream);
int utx_launch_cubemap_specular(const float* cube, int N, const float* texels, const float* tiles, float roughness, float costheta_cutoff, float* out, hipStream_t stream);
int utx_launch_dfg_lut(int R, int nsamples, float* out, hipStream_t stream);
int utx_launch_cube_sample(const float* cube, int N, const float* dirs, long n, float* out, hipStream_t stream);
int utx_launch_pbr_forward(const float* eye, int eye_stride, const float* pos, const float* nrm, const float* kd, int kd_stride, const float* ks, const float* light_diffuse, int Nd,
                           const float* light_specular, int Ns, const float* lut, int R, long npix, float* out_diffuse, float* out_specular, hipStream_t stream);
int utx_launch_pbr_shade(const float* rast, const int* tri, const float* vpos, const float* vnrm, const float* vuv, const float* kd, int Hk, int Wk, const float* ks, int Hs, int Ws,
                         const float* eye3_host, const float* light_diffuse, int Nd, const float* light_specular, int Ns, const float* lut, int R, float lambda_diffuse,
                         float lambda_specular, const float* bg3_host, long npix, void* out_u8, float* out_rgba, hipStream_t stream);
int utx_launch_pbr_shading_normal(const float* eye, int eye_stride, const float* pos, const float* pert, const float* snrm, const float* stng, const float* gnrm, long npix,
                                  float* out, hipStream_t stream);
int utx_launch_pbr_shade_nm(const float* rast, const int* tri, const float* vpos, const float* vnrm, const float* vtng, const float* fnrm, const float* vuv, const float* kd, int Hk,
                            int Wk, const float* ks, int Hs, int Ws, const float* nm, int Hn, int Wn, const float* eye3_host, const float* light_diffuse, int Nd,
                            const float* light_specular, int Ns, const float* lut, int R, float lambda_diffuse, float lambda_specular, const float* bg3_host, long npix,
                            void* out_u8, float* out_rgba, hipStream_t stream);
// scene.hip
int utx_launch_scene_render(const float* c2ws, const float* intr, int intr_stride, int B, int H, int W, const float* cube, int N, const float* lat, int Hi, int Wi, int C,
                            float* rays_d, float* cube_attr, float* uv, float* lat_attr, hipStream_t stream);
int utx_launch_cubemap_to_latlong(const float* cube, int N, int C, int Ht, int Wt, float* out, hipStream_t stream);
int utx_launch_scene_bake_latlong(const float* w2cs, const float* projs, const float* images, int M, int H, int W, int C, int Ht, int Wt, float* uv, float* uv_alpha,
                                  float* out, hipStream_t stream);
int utx_bvh_build_impl(const float* verts, int V, const int* faces, int F, utx_bvh** out, hipStream_t stream);
size_t utx_bvh_workspace_bytes_impl(int F);
int utx_bvh_build_ws_impl(const float* verts, int V, const int* faces, int F, void* work, size_t work_bytes, utx_bvh** out, hipStream_t stream);
void utx_bvh_free_impl(utx_bvh* b);
int utx_bvh_arrays_impl(utx_bvh* b, int** info, float** aabb, unsigned** codes_sorted, int** idx_sorted);
int utx_bvh_trace_impl(utx_bvh* b, const float* ro, const float* rd, long R, int* tid, unsigned long long* visited, int force_stack, hipStream_t stream);
int utx_bvh_depth_impl(utx_bvh* b);
int utx_visible_faces_rays_impl(utx_bvh* b, const float* verts, const int* faces, int F, const float* c2ws, int B, int perspective, int flags, unsigned char* mask,
                                unsigned long long* visited, hipStream_t stream);
int utx_bvh_closest_point_impl(utx_bvh* b, const float* points, long N, float* dist, int* face, float* uvw, float* closest, unsigned long long* visited, int flags,
                               hipStream_t stream);
int utx_launch_visible_faces_raster(const float* rast, int B, int H, int W, int F, unsigned char* mask, hipStream_t stream);
// raycast.hip
int utx_bvh_intersect_impl(utx_bvh* b, const float* ro, const float* rd, long R, int* tid, float* t, float* loc, float* uv, unsigned char* front, unsigned char* face_mask,
                           unsigned long long* visited, int flags, hipStream_t stream);
int utx_bvh_occluded_impl(utx_bvh* b, const float* from, const float* to, long R, unsigned char* blocked, unsigned long long* visited, int flags, hipStream_t stream);
int utx_points_enclosed_impl(utx_bvh* b, const float* points, long N, int n_rays, unsigned long long seed, unsigned stream_id, const float* dirs, unsigned char* inner,
                             int* hits, unsigned long long* visited, int flags, hipStream_t stream);
int utx_launch_sphere_directions(long n_points, long n_rays, unsigned long long seed, unsigned stream_id, float* out, hipStream_t stream);
int utx_launch_erode_faces(unsigned char* mask, const int* faces, int B, int F, int V, int depth, int* vstamp, hipStream_t stream);
int utx_launch_visible_vertices(const unsigned char* mask, const int* faces, int B, int F, int V, unsigned char* out, hipStream_t stream);
// vertex_bake.hip
int utx_launch_view_weight_maps(const float* cosn, const float* cam_nrm, int B, int H, int W, int r, void* tmp, float* out, float* arccos_out, hipStream_t stream);
int utx_launch_vertex_project(const float* v_pos, int V, const unsigned char* visible, int B, const float* xform, const float* proj, const float* images, int Hi, int Wi,
                              const float* wmap, int H, int W, const float* v_rgb, const float* weights, int use_alpha, float* acc, float* wacc, float overlay_conf,
                              int blending, float blending_conf, float inpainting_conf, float* blended, unsigned char* inpaint, hipStream_t stream);
int utx_launch_vertex_inpaint_step(const int* rowptr, const int* col, const int* idx, int n, const float* rgb_in, const unsigned char* mask_in, float* rgb_out,
                                   unsigned char* mask_out, int* counter, hipStream_t stream);
// uv_bake.hip
int utx_launch_uv_bake(const float* rast2d, const int* faces, int F, const unsigned char* face_mask, const float* v_ndc, int V, int B, int Th, int Tw,
                       const float* images, const float* wmap, const float* rast_view, int R, const float* map_Kd, const float* weights, int use_alpha,
                       float* acc, float* wacc, float overlay_conf, int blending, float blending_conf, float inpainting_conf, float* blended,
                       unsigned char* inpaint, hipStream_t stream);
int utx_launch_uv_dilation_step(const float* col_in, const unsigned char* mask_in, int H, int W, int C, int mode, float* col_out, unsigned char* mask_out,
                                int* counter, hipStream_t stream);
// global_bake.hip
int utx_launch_view_samples(const float* rast, const int* faces, int F, const float* v_uv, const float* v_pos_cam, const float* v_nrm_cam, int V, int B, int H, int W,
                            int exclude_boundary, int use_normal, float cos_normal, int use_ray, float cos_ray, const unsigned char* image_mask,
                            float* tex_to_pos, float* tex_to_pos_cam, unsigned char* mask, hipStream_t stream);
int utx_launch_knn_inpaint_step(const int* idx, const float* d2, const float* nrm, const float* col_in, const unsigned char* pend_in, long M, int k, int C,
                                float* col_out, unsigned char* pend_out, int* counter, hipStream_t stream);
// image_fusion.hip
int utx_launch_mask_morph(const unsigned char* mask_in, int H, int W, int n, unsigned char* tmp, unsigned char* mask_out, hipStream_t stream);
int utx_launch_mask_bbox(const unsigned char* mask, int H, int W, int* rect, hipStream_t stream);
int utx_image_fusion_cycles_impl(int w, int h);
size_t utx_image_fusion_workspace_bytes_impl(int w, int h);
int utx_launch_image_fusion(const unsigned char* src, const unsigned char* dst, const unsigned char* mask, int H, int W, int x1, int y1, int w, int h, int cycles,
                            unsigned char* out, float* out_f, void* work, hipStream_t stream);
// inpaint.hip
int utx_launch_inpaint_distance(const unsigned char* hole, int H, int W, int* tmp, int* d2, hipStream_t stream);
int utx_launch_inpaint_telea_step(const float* col_in, const unsigned char* done_in, const int* d2, int H, int W, int C, int eps, float* col_out,
                                  unsigned char* done_out, int* counter, hipStream_t stream);
int utx_launch_inpaint_finish(const float* col, int H, int W, int C, unsigned char* out, float* out_f, hipStream_t stream);
// color_transfer.hip
size_t utx_color_transfer_ot_workspace_bytes_impl(long N, int C);
int utx_launch_color_transfer_ot(const float* src, const float* dst, const float* dirs, long N, int C, int steps, int batch, float* out, void* work,
                                 size_t work_bytes, hipStream_t stream);
size_t utx_bilateral_lds_bytes_impl(int r, int C);
int utx_launch_bilateral_filter(const float* img, int H, int W, int C, int r, const float* ws, float coef, float* out, hipStream_t stream);
// antialias.hip
int utx_launch_antialias_analyze(const float* rast, const float* pos, long pos_view_stride, const int* tri, const int* opp, int F, int V, int B, int H, int W,
                                 float* weights, hipStream_t stream);
int utx_launch_antialias_apply(const float* color, const float* weights, int B, int H, int W, int C, float* out, hipStream_t stream);
int utx_launch_backproject(const utx_backproject_desc* p, const float* eyes, int sample, const utx_bvh* bvh, hipStream_t stream);
int utx_launch_backproject_vis(const utx_backproject_desc* p, const float* eyes, int sample, const utx_bvh* bvh, hipStream_t stream);
int utx_launch_composite_winner(const void* vis, int n_views, const int* order, int n_order, long T, void* winner, hipStream_t stream);
int utx_launch_gather_winner(const float* rast2d, const int* faces, const float* vndc, const float* images, const void* winner, long T, int V, int n_views, int H, int W, int C, int sample, float* atlas, hipStream_t stream);
int utx_launch_dilate_visibility(const void* rayvis, const void* alphaok, const void* rast2d, int n_views, int Hh, int Ww, void* tmp, void* vis_out, hipStream_t stream);
int utx_launch_composite(const float* colors, const void* vis, const int* order, int n_order, long T, float* atlas, void* winner, hipStream_t stream);
int utx_launch_seam_mask(const void* winner, const float* rast2d, int Hh, int Ww, void* tmp, void* seam, hipStream_t stream);
int utx_launch_seam_mask_sized(const void* winner, const float* rast2d, int Hh, int Ww, int k_boundary, int k_boundary_blur, void* tmp, void* seam, hipStream_t stream);
size_t utx_nn_fill_workspace_bytes_impl(long T);
int utx_launch_nn_fill(const float* pos, const void* winner, const float* rast2d, long T, int C, float* atlas, int* nn_index, void* work, size_t work_bytes, hipStream_t stream);
int utx_launch_lens_blur_seam(const float* src, const void* seam, int Hh, int Ww, int C, const float* k49_host, float* dst, hipStream_t stream);
int utx_launch_gaussian_blur_seam(const float* src, const void* seam, int Hh, int Ww, int C, int ksize, const float* w1_host, float* dst, hipStream_t stream);
size_t utx_pull_push_workspace_bytes_impl(int Hh, int Ww, int C);
int utx_launch_pull_push(const float* kd, const void* mask, int Hh, int Ww, int C, float* out, void* work, hipStream_t stream);
int utx_launch_chart_flood(const int* adj, const int* bucket, int F, int* chart, int* flag, hipStream_t stream);
int utx_launch_to_u8(const float* src, long n_rows, long row_elems, int flip, void* dst, hipStream_t stream);
}

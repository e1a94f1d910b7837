// C-ABI entry points of libunitex_hip.so (declared in include/unitex_hip.h).
// Thin: argument validation, error bookkeeping, launch.  No torch, no hidden syncs.
#include <cstdint>
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <stdlib.h>
#include <mutex>
#include <map>
#include <vector>
#include <utility>
#include "kernels.h"
#include "common.h"

UtxOptions g_utx_opt;      // defaults: the member initialisers in kernels.h

struct OptName { const char* name; int UtxOptions::*field; bool ablation; };
static const OptName kOptions[] = {
    {"UTX_ATTN_Q64", &UtxOptions::attn_q64, false},         {"UTX_ATTN_TAILSPLIT", &UtxOptions::attn_tailsplit, false},
    {"UTX_GEMM_GROUP_M", &UtxOptions::gemm_group_m, false}, {"UTX_GEMM_TILE", &UtxOptions::gemm_tile, false},
    {"UTX_GEMM_PERS_GRID", &UtxOptions::gemm_pers_grid, false}, {"UTX_GEMM_STREAMK", &UtxOptions::gemm_streamk, false},
    {"UTX_BVH_STACK_WALK", &UtxOptions::bvh_stack_walk, false}, {"UTX_BVH_PACKET", &UtxOptions::bvh_packet, false},
    {"UTX_ATTN_PEEL", &UtxOptions::attn_peel, false},             {"UTX_ATTN8_PEEL", &UtxOptions::attn8_peel, false},
    {"UTX_NN_GRID", &UtxOptions::nn_grid, false},                 {"UTX_GEMM_FASTK", &UtxOptions::gemm_fastk, false},
    {"UTX_ATTN_VAR", &UtxOptions::attn_var_abl, true},      {"UTX_ATTN_DEBUG", &UtxOptions::attn_debug_abl, true},
    {"UTX_GEMM_DEBUG", &UtxOptions::gemm_debug_abl, true},
};
#ifdef UTX_ABLATION
static const bool kAblationBuild = true;
#else
static const bool kAblationBuild = false;
#endif

// The environment is read exactly once, by whichever entry point touches the options first (utx_init, utx_set_option, utx_get_option,
// utx_gemm_plan): a utx_set_option made before the first utx_init must not be overwritten by a later read of the same UTX_* variable.
static void options_from_env_once() {
    static std::once_flag once;
    std::call_once(once, [] {
        for (const OptName& o : kOptions) {
            if (o.ablation && !kAblationBuild) continue;      // wrong-result switches do not exist in the product library
            const char* e = getenv(o.name);
            if (e && *e) g_utx_opt.*(o.field) = atoi(e);
        }
    });
}

struct utx_ctx {
    int device;
    std::string err;
    // scratch of the attention tail split for the entry points that take no workspace argument: owned by THIS context (not process-static), one buffer PER
    // STREAM (two streams of a context may run attention side by side) and GROW-ONLY: a buffer that was handed to a launch is never freed before utx_free
    // -- a replaced (smaller) buffer is parked in `retired`, so nothing that still holds its pointer (a launch in flight, a captured graph) can be left
    // dangling.  A CAPTURING stream gets no context scratch at all (the launch stays unsplit): a graph must not bake in a pointer whose other users
    // this library cannot order against the replays.  Callers that want the split under capture, or no allocation on the launch path, pass their own
    // buffer through utx_attn_fwd_bf16_ws (what FluxDiT does).
    std::mutex ws_mu;
    std::map<hipStream_t, std::pair<void*, size_t>> attn_ws;
    std::vector<void*> retired;
};

static void* ctx_attn_ws(utx_ctx* ctx, int H, int Sq, int S, hipStream_t stream, size_t* bytes) {
    *bytes = 0;
    if (!ctx) return nullptr;
    const size_t need = utx_attn_workspace_bytes_impl(H, Sq == S ? 0 : Sq, S, utx_ncu());
    if (need == 0) return nullptr;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(stream, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return nullptr;
    std::lock_guard<std::mutex> lock(ctx->ws_mu);
    std::pair<void*, size_t>& slot = ctx->attn_ws[stream];
    if (slot.second < need) {
        void* nb = nullptr;
        if (hipMalloc(&nb, need) != hipSuccess) { (void)hipGetLastError(); return nullptr; }      // no scratch: the launch stays unsplit
        if (slot.first) ctx->retired.push_back(slot.first);
        slot = {nb, need};
    }
    *bytes = slot.second;
    return slot.first;
}

static int fail(utx_ctx* ctx, int code, const char* what) {
    if (ctx) {
        char buf[256];
        snprintf(buf, sizeof(buf), "%s failed (code %d%s)", what, code,
                 code == -2 ? ": invalid argument / alignment" :
                 code == -3 ? ": hipFuncSetAttribute" :
                 code == -4 ? ": launch error" : "");
        ctx->err = buf;
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) { ctx->err += " hip: "; ctx->err += hipGetErrorString(e); }
    }
    return code;
}
#define UTX_CALL(ctx, name, expr) do { int rc_ = (expr); if (rc_ != 0) return fail(ctx, rc_, name); return 0; } while (0)

// argument checks that utx_uv_gbuffer, utx_screen_gbuffer and utx_uv_project share
static bool outs_present(unsigned want, void* const* outs_host, int count) {      // every requested bit has a buffer
    for (int k = 0; k < count; ++k)
        if (((want >> k) & 1u) && !outs_host[k]) return false;
    return true;
}
static bool bg_needs_pointer(int bg_kind) { return bg_kind == UTX_SGB_BG_VECTOR || bg_kind == UTX_SGB_BG_DENSE; }
static bool filter_and_bg_ok(int filter, int bg_kind) {
    return filter >= UTX_SGB_FILTER_BILINEAR && filter <= UTX_SGB_FILTER_NVDIFFRAST && bg_kind >= UTX_SGB_BG_NONE && bg_kind <= UTX_SGB_BG_DENSE;
}
// need_*_cam: the entry point's bits that read v_nrm_cam / v_pos_cam (its own: the two enumerations differ, and z_depth is camera z on the atlas only)
static bool cam_arrays_present(unsigned want, unsigned need_nrm_cam, unsigned need_pos_cam, const float* v_nrm_cam, const float* v_pos_cam) {
    return !((want & need_nrm_cam) && !v_nrm_cam) && !((want & need_pos_cam) && !v_pos_cam);
}

extern "C" {

int utx_version(void) { return UTX_VERSION; }

int utx_init(int device, utx_ctx** out) {
    if (!out) return -1;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return -5;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return -5;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return -6;  // MI355X only, by design
    options_from_env_once();
    utx_ctx* c = new utx_ctx();
    c->device = device;
    *out = c;
    return 0;
}

int utx_set_option(const char* name, int value) {
    if (!name) return -2;
    options_from_env_once();
    for (const OptName& o : kOptions)
        if (strcmp(name, o.name) == 0) {
            if (o.ablation && !kAblationBuild) return -7;
            g_utx_opt.*(o.field) = value;
            return 0;
        }
    return -2;
}

int utx_get_option(const char* name, int* value) {
    if (!name || !value) return -2;
    options_from_env_once();
    for (const OptName& o : kOptions)
        if (strcmp(name, o.name) == 0) {
            if (o.ablation && !kAblationBuild) return -7;
            *value = g_utx_opt.*(o.field);
            return 0;
        }
    return -2;
}

int utx_is_ablation_build(void) { return kAblationBuild ? 1 : 0; }

void utx_free(utx_ctx* ctx) {
    if (ctx) {
        for (auto& kv : ctx->attn_ws) if (kv.second.first) (void)hipFree(kv.second.first);
        for (void* p : ctx->retired) (void)hipFree(p);
    }
    delete ctx;
}

const char* utx_last_error(utx_ctx* ctx) { return ctx ? ctx->err.c_str() : "no context"; }

int utx_attn_fwd_bf16(utx_ctx* ctx, const void* q, const void* k, const void* vt, void* o,
                      long q_hs, long q_ss, long k_hs, long k_ss, long vt_hs, long vt_ds, long o_ss,
                      int H, int S, float softmax_scale, utx_stream stream) {
    if (!q || !k || !vt || !o) return fail(ctx, -2, "utx_attn_fwd_bf16");
    size_t wsb = 0; void* const ws = ctx_attn_ws(ctx, H, S, S, (hipStream_t)stream, &wsb);
    UTX_CALL(ctx, "utx_attn_fwd_bf16",
             utx_launch_attn_fwd(q, k, vt, o, q_hs, q_ss, k_hs, k_ss, vt_hs, vt_ds, o_ss, H, S, S,
                                 softmax_scale, 0.f, 0, ws, wsb, (hipStream_t)stream));
}

int utx_attn_fwd_bf16_kb(utx_ctx* ctx, const void* q, const void* k, const void* vt, void* o,
                         long q_hs, long q_ss, long k_hs, long k_ss, long vt_hs, long vt_ds, long o_ss,
                         int H, int S, float softmax_scale, float key_bias_log2, int key_bias_period, utx_stream stream) {
    if (!q || !k || !vt || !o) return fail(ctx, -2, "utx_attn_fwd_bf16_kb");
    size_t wsb = 0; void* const ws = ctx_attn_ws(ctx, H, S, S, (hipStream_t)stream, &wsb);
    UTX_CALL(ctx, "utx_attn_fwd_bf16_kb",
             utx_launch_attn_fwd(q, k, vt, o, q_hs, q_ss, k_hs, k_ss, vt_hs, vt_ds, o_ss, H, S, S,
                                 softmax_scale, key_bias_log2, key_bias_period, ws, wsb, (hipStream_t)stream));
}

int utx_attn_fwd_bf16_kbq(utx_ctx* ctx, const void* q, const void* k, const void* vt, void* o,
                          long q_hs, long q_ss, long k_hs, long k_ss, long vt_hs, long vt_ds, long o_ss,
                          int H, int S_q, int S_kv, float softmax_scale, float key_bias_log2, int key_bias_period, utx_stream stream) {
    if (!q || !k || !vt || !o) return fail(ctx, -2, "utx_attn_fwd_bf16_kbq");
    size_t wsb = 0; void* const ws = (S_q > 0) ? ctx_attn_ws(ctx, H, S_q, S_kv, (hipStream_t)stream, &wsb) : nullptr;
    UTX_CALL(ctx, "utx_attn_fwd_bf16_kbq",
             utx_launch_attn_fwd(q, k, vt, o, q_hs, q_ss, k_hs, k_ss, vt_hs, vt_ds, o_ss, H, S_kv, S_q,
                                 softmax_scale, key_bias_log2, key_bias_period, ws, wsb, (hipStream_t)stream));
}

int utx_attn_fwd_bf16_ws(utx_ctx* ctx, const void* q, const void* k, const void* vt, void* o,
                         long q_hs, long q_ss, long k_hs, long k_ss, long vt_hs, long vt_ds, long o_ss,
                         int H, int S_q, int S_kv, float softmax_scale, float key_bias_log2, int key_bias_period,
                         void* work, size_t work_bytes, utx_stream stream) {
    if (!q || !k || !vt || !o) return fail(ctx, -2, "utx_attn_fwd_bf16_ws");
    UTX_CALL(ctx, "utx_attn_fwd_bf16_ws",
             utx_launch_attn_fwd(q, k, vt, o, q_hs, q_ss, k_hs, k_ss, vt_hs, vt_ds, o_ss, H, S_kv, S_q,
                                 softmax_scale, key_bias_log2, key_bias_period, work, work_bytes, (hipStream_t)stream));
}

int utx_attn_fwd_bf16_blk(utx_ctx* ctx, const void* q, const void* k, const void* vt, void* o,
                          long q_hs, long q_ss, long k_hs, long k_ss, long vt_hs, long vt_ds, long o_ss,
                          int H, int S_q, int S_kv, float softmax_scale, float key_bias_log2, int key_bias_period,
                          void* work, size_t work_bytes, int blk_rows, long q_bs, long k_bs, long vt_bs, utx_stream stream) {
    if (!q || !k || !vt || !o || blk_rows <= 0) return fail(ctx, -2, "utx_attn_fwd_bf16_blk");
    UTX_CALL(ctx, "utx_attn_fwd_bf16_blk",
             utx_launch_attn_fwd_blk(q, k, vt, o, q_hs, q_ss, k_hs, k_ss, vt_hs, vt_ds, o_ss, H, S_kv, S_q,
                                     softmax_scale, key_bias_log2, key_bias_period, work, work_bytes, blk_rows, q_bs, k_bs, vt_bs, (hipStream_t)stream));
}

int utx_quant_vt_mx8(utx_ctx* ctx, const void* vt, void* v8, void* vs, int H, int S_pad, utx_stream stream) {
    if (!vt || !v8 || !vs) return fail(ctx, -2, "utx_quant_vt_mx8");
    UTX_CALL(ctx, "utx_quant_vt_mx8", utx_launch_quant_vt_mx8(vt, v8, vs, H, S_pad, (hipStream_t)stream));
}

int utx_attn_fwd_fp8(utx_ctx* ctx, const void* q8, const void* qs, const void* k8, const void* ks, const void* v8t, const void* vs, void* o, long o_ss,
                     int H, int S_q, int S_kv, int S_pad, float key_bias_log2, int key_bias_period, utx_stream stream) {
    if (!q8 || !qs || !k8 || !ks || !v8t || !vs || !o) return fail(ctx, -2, "utx_attn_fwd_fp8");
    Attn8Params p;
    p.q8 = (const uint8_t*)q8; p.k8 = (const uint8_t*)k8; p.v8t = (const uint8_t*)v8t;
    p.qs = (const uint32_t*)qs; p.ks = (const uint32_t*)ks; p.vs = (const uint32_t*)vs;
    p.o = (bf16_t*)o; p.o_ss = o_ss; p.H = H; p.S = S_kv; p.Sq = S_q; p.S_pad = S_pad; p.nqb = 0;
    p.key_bias_log2 = key_bias_log2; p.key_bias_period = key_bias_period;
    // the key-split tail round runs on the context's per-stream scratch (none while the stream is capturing: the launch then stays unsplit); utx_attn_fwd_fp8_ws takes the caller's
    p.work = (S_q > 0 && S_q <= S_kv) ? ctx_attn_ws(ctx, H, S_q, S_kv, (hipStream_t)stream, &p.work_bytes) : nullptr;
    if (!p.work) p.work_bytes = 0;
    UTX_CALL(ctx, "utx_attn_fwd_fp8", utx_launch_attn_fwd_fp8(&p, (hipStream_t)stream));
}

int utx_attn_fwd_fp8_ws(utx_ctx* ctx, const void* q8, const void* qs, const void* k8, const void* ks, const void* v8t, const void* vs, void* o, long o_ss,
                        int H, int S_q, int S_kv, int S_pad, float key_bias_log2, int key_bias_period, void* work, size_t work_bytes, utx_stream stream) {
    if (!q8 || !qs || !k8 || !ks || !v8t || !vs || !o) return fail(ctx, -2, "utx_attn_fwd_fp8_ws");
    Attn8Params p;
    p.q8 = (const uint8_t*)q8; p.k8 = (const uint8_t*)k8; p.v8t = (const uint8_t*)v8t;
    p.qs = (const uint32_t*)qs; p.ks = (const uint32_t*)ks; p.vs = (const uint32_t*)vs;
    p.o = (bf16_t*)o; p.o_ss = o_ss; p.H = H; p.S = S_kv; p.Sq = S_q; p.S_pad = S_pad; p.nqb = 0;
    p.key_bias_log2 = key_bias_log2; p.key_bias_period = key_bias_period;
    p.work = work; p.work_bytes = work ? work_bytes : 0;
    UTX_CALL(ctx, "utx_attn_fwd_fp8_ws", utx_launch_attn_fwd_fp8(&p, (hipStream_t)stream));
}

size_t utx_attn_workspace_bytes(utx_ctx* ctx, int H, int S_q, int S_kv) {
    (void)ctx;
    // S_q > S_kv is a plain case since round 6 (the sequence-parallel launch over de-duplicated text keys); refusing it here left exactly that launch without scratch -- unsplit
    // and on the 8 x 32 kernel -- while the launcher itself accepted it
    if (H <= 0 || S_kv <= 0 || S_q <= 0) return 0;
    return utx_attn_workspace_bytes_impl(H, S_q == S_kv ? 0 : S_q, S_kv, utx_ncu());
}

int utx_attn_plan(int H, int S_q, int S_kv, int n_cus, int out[4]) {
    if (!out || H <= 0 || S_kv <= 0 || S_q <= 0 || n_cus <= 0) return -2;
    options_from_env_once();
    utx_attn_split_plan_impl(H, S_q == S_kv ? 0 : S_q, S_kv, n_cus, out);
    return 0;
}

size_t utx_gemm_streamk_workspace_bytes(utx_ctx*) { return utx_gemm_streamk_workspace_bytes_impl(); }
int utx_gemm_plan(const utx_gemm_desc* d, int n_cus, int out[4]) {
    if (!d || !out || n_cus <= 0 || d->M <= 0 || d->N <= 0 || d->K <= 0) return -2;
    options_from_env_once();
    return utx_gemm_plan_impl(d, n_cus, d->sk_work != nullptr, out);
}
int utx_gemm_bf16(utx_ctx* ctx, const utx_gemm_desc* d, utx_stream stream) {
    if (!d || !d->A || !d->B || !d->C) return fail(ctx, -2, "utx_gemm_bf16");
    UTX_CALL(ctx, "utx_gemm_bf16", utx_launch_gemm_bf16(d, (hipStream_t)stream));
}

int utx_quant_mx8(utx_ctx* ctx, const void* x, long ldx, void* q, long ldq, void* sc, long lds, int M, int K, utx_stream stream) {
    if (!x || !q || !sc) return fail(ctx, -2, "utx_quant_mx8");
    UTX_CALL(ctx, "utx_quant_mx8", utx_launch_quant_mx8(x, ldx, q, ldq, sc, lds, M, K, (hipStream_t)stream));
}

int utx_quant_mx8_packed(utx_ctx* ctx, const void* x, long ldx, void* q, long ldq, void* sc, long row_blocks, int M, int K, utx_stream stream) {
    if (!x || !q || !sc) return fail(ctx, -2, "utx_quant_mx8_packed");
    UTX_CALL(ctx, "utx_quant_mx8_packed", utx_launch_quant_mx8_packed(x, ldx, q, ldq, sc, row_blocks, M, K, (hipStream_t)stream));
}

int utx_gemv_bf16(utx_ctx* ctx, const utx_gemv_desc* d, utx_stream stream) {
    if (!d || !d->x || !d->W || !d->y) return fail(ctx, -2, "utx_gemv_bf16");
    UTX_CALL(ctx, "utx_gemv_bf16", utx_launch_gemv_bf16(d, (hipStream_t)stream));
}

size_t utx_group_norm_workspace_bytes(void) { return utx_group_norm_workspace_bytes_impl(); }

int utx_group_norm(utx_ctx* ctx, const void* x, long npix, int C, const void* gamma, const void* beta, float eps, int silu,
                   void* y, void* work, utx_stream stream) {
    if (!x || !gamma || !beta || !y || !work) return fail(ctx, -2, "utx_group_norm");
    UTX_CALL(ctx, "utx_group_norm", utx_launch_group_norm(x, npix, C, gamma, beta, eps, silu, y, work, (hipStream_t)stream));
}

int utx_softmax_rows(utx_ctx* ctx, void* s, long nrow, long ld, int ncol, utx_stream stream) {
    if (!s) return fail(ctx, -2, "utx_softmax_rows");
    UTX_CALL(ctx, "utx_softmax_rows", utx_launch_softmax_rows(s, nrow, ld, ncol, (hipStream_t)stream));
}

int utx_conv3x3_thin(utx_ctx* ctx, const void* x, int H, int W, int Cin, const void* wt, const void* bias, int Cout, void* y,
                     utx_stream stream) {
    if (!x || !wt || !bias || !y) return fail(ctx, -2, "utx_conv3x3_thin");
    UTX_CALL(ctx, "utx_conv3x3_thin", utx_launch_conv3x3_thin(x, H, W, Cin, wt, bias, Cout, y, (hipStream_t)stream));
}

int utx_qkv_post(utx_ctx* ctx, const utx_qkv_post_desc* d, utx_stream stream) {
    if (!d || !d->qkv || !d->Qh || !d->Kh || !d->Vt || !d->cosb || !d->sinb || !d->wq || !d->wk)
        return fail(ctx, -2, "utx_qkv_post");
    UTX_CALL(ctx, "utx_qkv_post", utx_launch_qkv_post(d, (hipStream_t)stream));
}

int utx_sp_unpack_qkv(utx_ctx* ctx, const void* recv, int P, int Hp, int S_loc, void* q, void* k, void* vt, utx_stream stream) {
    if (!recv || !q || !k || !vt) return fail(ctx, -2, "utx_sp_unpack_qkv");
    UTX_CALL(ctx, "utx_sp_unpack_qkv", utx_launch_sp_unpack_qkv(recv, P, Hp, S_loc, 0, q, k, vt, (hipStream_t)stream));
}

int utx_sp_unpack_qkv_dedup(utx_ctx* ctx, const void* recv, int P, int Hp, int S_loc, int text_rows, void* q, void* k, void* vt, utx_stream stream) {
    if (!recv || !q || !k || !vt) return fail(ctx, -2, "utx_sp_unpack_qkv_dedup");
    UTX_CALL(ctx, "utx_sp_unpack_qkv_dedup", utx_launch_sp_unpack_qkv(recv, P, Hp, S_loc, text_rows, q, k, vt, (hipStream_t)stream));
}

int utx_sp_unpack_o(utx_ctx* ctx, const void* recv, int P, int Hp, int S_loc, void* out, long ld, utx_stream stream) {
    if (!recv || !out) return fail(ctx, -2, "utx_sp_unpack_o");
    UTX_CALL(ctx, "utx_sp_unpack_o", utx_launch_sp_unpack_o(recv, P, Hp, S_loc, out, ld, 0, (hipStream_t)stream));
}

int utx_sp_unpack_o_cols(utx_ctx* ctx, const void* recv, int P, int Hp, int S_loc, void* out, long ld, long src_cols, utx_stream stream) {
    if (!recv || !out || src_cols <= 0) return fail(ctx, -2, "utx_sp_unpack_o_cols");
    UTX_CALL(ctx, "utx_sp_unpack_o_cols", utx_launch_sp_unpack_o(recv, P, Hp, S_loc, out, ld, src_cols, (hipStream_t)stream));
}

int utx_ln_mod(utx_ctx* ctx, const utx_ln_mod_desc* d, utx_stream stream) {
    if (!d || !d->x || (!d->y && !d->q) || !d->shift || !d->scale) return fail(ctx, -2, "utx_ln_mod");
    UTX_CALL(ctx, "utx_ln_mod", utx_launch_ln_mod(d, (hipStream_t)stream));
}

int utx_sched_step(utx_ctx* ctx, const utx_sched_desc* d, utx_stream stream) {
    if (!d || !d->x || !d->v) return fail(ctx, -2, "utx_sched_step");
    UTX_CALL(ctx, "utx_sched_step", utx_launch_sched_step(d, (hipStream_t)stream));
}


// ---- geometry ----
int utx_transform_points(utx_ctx* ctx, const float* verts, int V, const float* mvp, int n_views, float* clip, float* ndc, utx_stream stream) {
    if (!verts || !mvp || !clip) return fail(ctx, -2, "utx_transform_points");
    UTX_CALL(ctx, "utx_transform_points", utx_launch_transform(verts, V, mvp, n_views, clip, ndc, (hipStream_t)stream));
}
long utx_rasterize_workspace_bytes(int F, int H, int W) { return 8L * H * W + 16 + 4L * F + 64; }
int utx_rasterize(utx_ctx* ctx, const float* pos, const int* tri, int F, int H, int W, float* rast, void* work, utx_stream stream) {
    if (!pos || !tri || !rast || !work) return fail(ctx, -2, "utx_rasterize");
    UTX_CALL(ctx, "utx_rasterize", utx_launch_rasterize(pos, tri, F, H, W, rast, work, (hipStream_t)stream));
}
int utx_interpolate(utx_ctx* ctx, const float* attr, int C, const float* rast, const int* tri, long npix, float* out, utx_stream stream) {
    if (!attr || !rast || !tri || !out) return fail(ctx, -2, "utx_interpolate");
    UTX_CALL(ctx, "utx_interpolate", utx_launch_interpolate(attr, C, rast, tri, npix, out, (hipStream_t)stream));
}
int utx_face_normals(utx_ctx* ctx, const float* verts, const int* faces, int F, float* out, utx_stream stream) {
    if (!verts || !faces || !out) return fail(ctx, -2, "utx_face_normals");
    UTX_CALL(ctx, "utx_face_normals", utx_launch_face_normals(verts, faces, F, out, (hipStream_t)stream));
}

int utx_texture_shade(utx_ctx* ctx, const float* rast, const float* uv, const int* tri, const float* tex, int Ht, int Wt,
                      const float* bg3_host, long npix, void* out, utx_stream stream) {
    if (!rast || !uv || !tri || !tex || !out) return fail(ctx, -2, "utx_texture_shade");
    UTX_CALL(ctx, "utx_texture_shade", utx_launch_texture_shade(rast, uv, tri, tex, Ht, Wt, bg3_host, npix, out, (hipStream_t)stream));
}

int utx_gbuffer_shade(utx_ctx* ctx, int mode, const float* rast, const int* tri, const float* attr, int attr_stride, const float* scale2_dev,
                      int flags, const float* bg3_host, long npix, void* out_u8, float* out_rgba_or_null, utx_stream stream) {
    if (!rast || !tri || !attr || !bg3_host || !out_u8) return fail(ctx, -2, "utx_gbuffer_shade");
    if (((uintptr_t)rast & 15) || ((uintptr_t)out_rgba_or_null & 15)) return fail(ctx, -2, "utx_gbuffer_shade");      // read / stored as float4
    if (mode < 0 || mode > UTX_GBUF_DISTANCE || npix <= 0 || (flags & ~(UTX_GBUF_NDC | UTX_GBUF_COMPOSITE))) return fail(ctx, -2, "utx_gbuffer_shade");
    if (attr_stride < (mode == UTX_GBUF_Z_DEPTH ? 1 : 3)) return fail(ctx, -2, "utx_gbuffer_shade");
    UTX_CALL(ctx, "utx_gbuffer_shade", utx_launch_gbuffer_shade(mode, rast, tri, attr, attr_stride, scale2_dev, (flags & UTX_GBUF_NDC) != 0,
                                                                (flags & UTX_GBUF_COMPOSITE) != 0, bg3_host, npix, out_u8, out_rgba_or_null, (hipStream_t)stream));
}
int utx_gbuffer_range(utx_ctx* ctx, int mode, const float* rast, const int* tri, const float* attr, int attr_stride, long npix,
                      float* scale2_dev, int* empty_flag_dev, utx_stream stream) {
    if (!rast || !tri || !attr || !scale2_dev || !empty_flag_dev) return fail(ctx, -2, "utx_gbuffer_range");
    if ((uintptr_t)rast & 15) return fail(ctx, -2, "utx_gbuffer_range");      // read as float4
    if (mode < 0 || mode > UTX_GBUF_DISTANCE || npix <= 0) return fail(ctx, -2, "utx_gbuffer_range");
    if (attr_stride < (mode == UTX_GBUF_Z_DEPTH ? 1 : 3)) return fail(ctx, -2, "utx_gbuffer_range");
    UTX_CALL(ctx, "utx_gbuffer_range", utx_launch_gbuffer_range(mode, rast, tri, attr, attr_stride, npix, scale2_dev, empty_flag_dev, (hipStream_t)stream));
}
int utx_uv_gbuffer(utx_ctx* ctx, const float* rast2d, const int* faces, const float* v_pos, const float* v_nrm, const float* v_pos_cam,
                   const float* v_nrm_cam, int V, int B, int H2D, int W2D, unsigned want, void* const* outs_host, utx_stream stream) {
    const unsigned need_nrm_cam = UTX_UVGB_CAMERA_NORMAL | UTX_UVGB_COS_RAY_NORMAL;
    const unsigned need_pos_cam = UTX_UVGB_CAMERA_POSITION | UTX_UVGB_DISTANCE | UTX_UVGB_Z_DEPTH | UTX_UVGB_RAY_DIRECTION | UTX_UVGB_COS_RAY_NORMAL;
    if (!rast2d || !faces || !outs_host || ((uintptr_t)rast2d & 15)) return fail(ctx, -2, "utx_uv_gbuffer");      // rast2d is read as float4
    if (H2D <= 0 || W2D <= 0 || V <= 0 || B < 0 || want == 0 || (want & ~(unsigned)UTX_UVGB_ALL)) return fail(ctx, -2, "utx_uv_gbuffer");
    if (!outs_present(want, outs_host, UTX_UVGB_COUNT)) return fail(ctx, -2, "utx_uv_gbuffer");
    if (((want & UTX_UVGB_WORLD_POSITION) && !v_pos) || ((want & UTX_UVGB_WORLD_NORMAL) && !v_nrm)) return fail(ctx, -2, "utx_uv_gbuffer");
    if (B > 0 && !cam_arrays_present(want, need_nrm_cam, need_pos_cam, v_nrm_cam, v_pos_cam)) return fail(ctx, -2, "utx_uv_gbuffer");
    UTX_CALL(ctx, "utx_uv_gbuffer", utx_launch_uv_gbuffer(rast2d, faces, v_pos, v_nrm, v_pos_cam, v_nrm_cam, V, B, H2D, W2D, want, outs_host,
                                                          (hipStream_t)stream));
}
int utx_screen_gbuffer(utx_ctx* ctx, const float* rast, const int* faces, const float* v_pos, const float* v_nrm, const float* v_uv,
                       const float* v_attr, int Ca, const float* clip_w, const float* v_pos_cam, const float* v_nrm_cam, int V, int B, int H, int W,
                       int n_maps, const float* const* maps_host, const int* map_dims_host, int filter, int bg_kind, float bg_scalar,
                       const float* bg_v_attr, const float* bg_map_attr, unsigned want, void* const* outs_host, utx_stream stream) {
    const char* const me = "utx_screen_gbuffer";
    const unsigned need_nrm_cam = UTX_SGB_CAMERA_NORMAL | UTX_SGB_COS_RAY_NORMAL;
    const unsigned need_pos_cam = UTX_SGB_CAMERA_POSITION | UTX_SGB_DISTANCE | UTX_SGB_RAY_DIRECTION | UTX_SGB_COS_RAY_NORMAL;
    if (!rast || !faces || !outs_host || ((uintptr_t)rast & 15)) return fail(ctx, -2, me);      // rast is read as float4
    if (H < 0 || W < 0 || V <= 0 || B < 0 || (want & ~(unsigned)UTX_SGB_ALL)) return fail(ctx, -2, me);
    if (!filter_and_bg_ok(filter, bg_kind) || !outs_present(want, outs_host, UTX_SGB_COUNT)) return fail(ctx, -2, me);
    if (B == 0 && (want & (need_nrm_cam | need_pos_cam | UTX_SGB_Z_DEPTH))) return fail(ctx, -2, me);      // a per-view array of no view has no address
    if (((want & UTX_SGB_WORLD_POSITION) && !v_pos) || ((want & UTX_SGB_WORLD_NORMAL) && !v_nrm)) return fail(ctx, -2, me);
    if (!cam_arrays_present(want, need_nrm_cam, need_pos_cam, v_nrm_cam, v_pos_cam) || ((want & UTX_SGB_Z_DEPTH) && !clip_w)) return fail(ctx, -2, me);
    if ((want & (UTX_SGB_UV | UTX_SGB_MAP_ATTR)) && !v_uv) return fail(ctx, -2, me);
    const bool bg_ptr = bg_needs_pointer(bg_kind);
    if (want & UTX_SGB_V_ATTR) {
        if (!v_attr || Ca <= 0 || (bg_ptr && !bg_v_attr)) return fail(ctx, -2, me);
    }
    if (want & UTX_SGB_MAP_ATTR) {
        if (n_maps < 1 || n_maps > UTX_SGB_MAX_MAPS || !maps_host || !map_dims_host || (bg_ptr && !bg_map_attr)) return fail(ctx, -2, me);
        for (int m = 0; m < n_maps; ++m)
            if (!maps_host[m] || map_dims_host[3 * m] <= 0 || map_dims_host[3 * m + 1] <= 0 || map_dims_host[3 * m + 2] <= 0) return fail(ctx, -2, me);
    }
    UTX_CALL(ctx, me, utx_launch_screen_gbuffer(rast, faces, v_pos, v_nrm, v_uv, v_attr, Ca, clip_w, v_pos_cam, v_nrm_cam, V, B, H, W,
                                                (want & UTX_SGB_MAP_ATTR) ? n_maps : 0, maps_host, map_dims_host, filter, bg_kind, bg_scalar, bg_v_attr,
                                                bg_map_attr, want, outs_host, (hipStream_t)stream));
}
int utx_uv_project(utx_ctx* ctx, const float* rast2d, const int* faces, int F, const unsigned char* face_mask, const float* v_ndc, int V, int B, int H2D,
                   int W2D, const float* map, int Bm, int Hm, int Wm, int C, const float* rast_map, int filter, int bg_kind, float bg_scalar,
                   const float* bg, float* uv, float* uv_alpha, float* map_attr, utx_stream stream) {
    const char* const me = "utx_uv_project";
    if (!rast2d || !faces || !face_mask || !v_ndc || !uv || !uv_alpha || ((uintptr_t)rast2d & 15)) return fail(ctx, -2, me);      // rast2d is read as float4
    if (F <= 0 || V <= 0 || B <= 0 || H2D <= 0 || W2D <= 0) return fail(ctx, -2, me);
    if (map) {
        if (!rast_map || !map_attr || (Bm != 1 && Bm != B) || Hm <= 0 || Wm <= 0 || C <= 0) return fail(ctx, -2, me);
        if (!filter_and_bg_ok(filter, bg_kind) || (bg_needs_pointer(bg_kind) && !bg)) return fail(ctx, -2, me);
    }
    UTX_CALL(ctx, me, utx_launch_uv_project(rast2d, faces, F, face_mask, v_ndc, V, B, H2D, W2D, map, Bm, Hm, Wm, C, rast_map, map ? filter : 0, bg_kind, bg_scalar, bg, uv,
                                            uv_alpha, map ? map_attr : nullptr, (hipStream_t)stream));
}
// ---- vertex-colour bake (vertex_bake.hip) ----
static bool misaligned(const void* p, unsigned mask) { return ((uintptr_t)p & mask) != 0; }
int utx_view_weight_maps(utx_ctx* ctx, const float* cos_ray_normal, const float* camera_normal, int B, int H, int W, int r, void* tmp, float* out,
                         float* arccos_out, utx_stream stream) {
    const char* const me = "utx_view_weight_maps";
    if (B < 0 || H < 0 || W < 0 || r < 0) return fail(ctx, -2, me);
    if ((long)B * H * W == 0) return 0;
    if (H < 2 || W < 2 || !cos_ray_normal || !out || (r > 0 && !tmp)) return fail(ctx, -2, me);      // torch.gradient needs two samples per axis
    if (misaligned(cos_ray_normal, 3) || misaligned(camera_normal, 3) || misaligned(out, 7) || misaligned(arccos_out, 3)) return fail(ctx, -2, me);
    UTX_CALL(ctx, me, utx_launch_view_weight_maps(cos_ray_normal, camera_normal, B, H, W, r, tmp, out, arccos_out, (hipStream_t)stream));
}
static int vertex_project_checked(utx_ctx* ctx, const char* me, bool epilogue, const float* v_pos, int V, const unsigned char* visible, int B, const float* xform,
                                  const float* proj, const float* images, int Hi, int Wi, const float* wmap, int H, int W, const float* v_rgb,
                                  const float* weights, int use_alpha, float* acc, float* wacc, float overlay_conf, int blending, float blending_conf,
                                  float inpainting_conf, float* blended, unsigned char* inpaint, utx_stream stream) {
    if (V < 0 || B < 0 || Hi < 0 || Wi < 0 || H < 0 || W < 0) return fail(ctx, -2, me);
    if (epilogue && (blending < UTX_VB_BLEND_NONE || blending > UTX_VB_BLEND_HARD)) return fail(ctx, -2, me);
    if (V == 0) return 0;
    if (!v_pos || !v_rgb || !wacc || (!epilogue && !acc) || (epilogue && (!blended || !inpaint))) return fail(ctx, -2, me);
    if (B > 0 && (!visible || !xform || !proj || !images || !wmap || !weights || Hi == 0 || Wi == 0 || H == 0 || W == 0)) return fail(ctx, -2, me);
    if (misaligned(v_pos, 3) || misaligned(xform, 3) || misaligned(proj, 3) || misaligned(images, 3) || misaligned(wmap, 7) || misaligned(v_rgb, 3) ||
        misaligned(weights, 3) || misaligned(acc, 3) || misaligned(wacc, 3) || misaligned(blended, 3)) return fail(ctx, -2, me);
    UTX_CALL(ctx, me, utx_launch_vertex_project(v_pos, V, visible, B, xform, proj, images, Hi, Wi, wmap, H, W, v_rgb, weights, use_alpha, acc, wacc, overlay_conf,
                                                blending, blending_conf, inpainting_conf, epilogue ? blended : nullptr, inpaint, (hipStream_t)stream));
}
int utx_vertex_project(utx_ctx* ctx, const float* v_pos, int V, const unsigned char* visible, int B, const float* xform, const float* proj, const float* images,
                       int Hi, int Wi, const float* wmap, int H, int W, const float* v_rgb, const float* weights, int use_alpha, float* v_rgb_acc,
                       float* v_weight_acc, utx_stream stream) {
    return vertex_project_checked(ctx, "utx_vertex_project", false, v_pos, V, visible, B, xform, proj, images, Hi, Wi, wmap, H, W, v_rgb, weights, use_alpha,
                                  v_rgb_acc, v_weight_acc, 0.f, 0, 0.f, 0.f, nullptr, nullptr, stream);
}
int utx_vertex_project_blend(utx_ctx* ctx, const float* v_pos, int V, const unsigned char* visible, int B, const float* xform, const float* proj,
                             const float* images, int Hi, int Wi, const float* wmap, int H, int W, const float* v_rgb, const float* weights, int use_alpha,
                             float* v_rgb_acc, float* v_weight_acc, float overlay_confidence, int blending, float blending_confidence,
                             float inpainting_confidence, float* blended, unsigned char* inpaint_mask, utx_stream stream) {
    return vertex_project_checked(ctx, "utx_vertex_project_blend", true, v_pos, V, visible, B, xform, proj, images, Hi, Wi, wmap, H, W, v_rgb, weights, use_alpha,
                                  v_rgb_acc, v_weight_acc, overlay_confidence, blending, blending_confidence, inpainting_confidence, blended, inpaint_mask, stream);
}
int utx_vertex_inpaint_step(utx_ctx* ctx, const int* rowptr, const int* col, const int* idx, int n, const float* rgb_in, const unsigned char* mask_in,
                            float* rgb_out, unsigned char* mask_out, int* counter, utx_stream stream) {
    const char* const me = "utx_vertex_inpaint_step";
    if (n < 0) return fail(ctx, -2, me);
    if (n == 0) return 0;
    if (!rowptr || !col || !idx || !rgb_in || !mask_in || !rgb_out || !mask_out || !counter) return fail(ctx, -2, me);
    if (rgb_in == rgb_out || mask_in == mask_out) return fail(ctx, -2, me);      // a step reads one pair and writes the other
    if (misaligned(rowptr, 3) || misaligned(col, 3) || misaligned(idx, 3) || misaligned(rgb_in, 3) || misaligned(rgb_out, 3) || misaligned(counter, 3))
        return fail(ctx, -2, me);
    UTX_CALL(ctx, me, utx_launch_vertex_inpaint_step(rowptr, col, idx, n, rgb_in, mask_in, rgb_out, mask_out, counter, (hipStream_t)stream));
}
// ---- blended UV texture bake (uv_bake.hip) ----
int utx_uv_bake(utx_ctx* ctx, const float* rast2d, const int* faces, int F, const unsigned char* face_mask, const float* v_ndc, int V, int B, int Th, int Tw,
                const float* images, const float* wmap, const float* rast_view, int R, const float* map_Kd, const float* weights, int use_alpha, float* acc,
                float* wacc, int epilogue, float overlay_confidence, int blending, float blending_confidence, float inpainting_confidence, float* blended,
                unsigned char* inpaint_mask, utx_stream stream) {
    const char* const me = "utx_uv_bake";
    if (Th < 0 || Tw < 0 || B <= 0 || R <= 0 || F <= 0 || V <= 0) return fail(ctx, -2, me);
    if (epilogue && (blending < UTX_VB_BLEND_NONE || blending > UTX_VB_BLEND_HARD)) return fail(ctx, -2, me);
    if ((long)Th * Tw == 0) return 0;
    if (!rast2d || !faces || !face_mask || !v_ndc || !images || !wmap || !rast_view || !map_Kd || !weights || !wacc) return fail(ctx, -2, me);
    if ((!epilogue && !acc) || (epilogue && (!blended || !inpaint_mask))) return fail(ctx, -2, me);
    if (misaligned(rast2d, 15) || misaligned(map_Kd, 15) || misaligned(acc, 15) || (epilogue && misaligned(blended, 15)) || misaligned(wmap, 7) ||
        misaligned(faces, 3) || misaligned(v_ndc, 3) || misaligned(images, 3) || misaligned(rast_view, 3) || misaligned(weights, 3) || misaligned(wacc, 3))
        return fail(ctx, -2, me);
    UTX_CALL(ctx, me, utx_launch_uv_bake(rast2d, faces, F, face_mask, v_ndc, V, B, Th, Tw, images, wmap, rast_view, R, map_Kd, weights, use_alpha, acc, wacc,
                                         overlay_confidence, blending, blending_confidence, inpainting_confidence, epilogue ? blended : nullptr, inpaint_mask,
                                         (hipStream_t)stream));
}
int utx_uv_dilation_step(utx_ctx* ctx, const float* col_in, const unsigned char* mask_in, int H, int W, int C, int mode, float* col_out, unsigned char* mask_out,
                         int* counter, utx_stream stream) {
    const char* const me = "utx_uv_dilation_step";
    if (H < 0 || W < 0 || C < 1 || C > 16 || (mode != UTX_UVD_STEP && mode != UTX_UVD_CLAMP)) return fail(ctx, -2, me);
    if ((long)H * W == 0) return 0;
    if (!col_in || !col_out || col_in == col_out || misaligned(col_in, 3) || misaligned(col_out, 3)) return fail(ctx, -2, me);
    if (mode == UTX_UVD_STEP && (!mask_in || !mask_out || !counter || mask_in == mask_out || misaligned(counter, 3))) return fail(ctx, -2, me);
    UTX_CALL(ctx, me, utx_launch_uv_dilation_step(col_in, mask_in, H, W, C, mode, col_out, mask_out, counter, (hipStream_t)stream));
}
// ---- scattered-sample UV bake (global_bake.hip) ----
int utx_view_samples(utx_ctx* ctx, const float* rast, const int* faces, int F, const float* v_uv, const float* v_pos_cam, const float* v_nrm_cam, int V, int B,
                     int H, int W, int exclude_boundary, int use_normal_threshold, float cos_normal, int use_ray_threshold, float cos_ray,
                     const unsigned char* image_mask, float* tex_to_pos, float* tex_to_pos_cam, unsigned char* mask, utx_stream stream) {
    const char* const me = "utx_view_samples";
    if (B < 0 || H < 0 || W < 0 || F <= 0 || V <= 0) return fail(ctx, -2, me);
    if ((long)B * H * W == 0) return 0;
    if (!rast || !faces || !v_uv || !v_pos_cam || !v_nrm_cam || !tex_to_pos || !tex_to_pos_cam || !mask) return fail(ctx, -2, me);
    if (misaligned(rast, 15) || misaligned(tex_to_pos, 7) || misaligned(faces, 3) || misaligned(v_uv, 3) || misaligned(v_pos_cam, 3) || misaligned(v_nrm_cam, 3) ||
        misaligned(tex_to_pos_cam, 3)) return fail(ctx, -2, me);
    UTX_CALL(ctx, me, utx_launch_view_samples(rast, faces, F, v_uv, v_pos_cam, v_nrm_cam, V, B, H, W, exclude_boundary != 0, use_normal_threshold != 0, cos_normal,
                                              use_ray_threshold != 0, cos_ray, image_mask, tex_to_pos, tex_to_pos_cam, mask, (hipStream_t)stream));
}
int utx_knn_inpaint_step(utx_ctx* ctx, const int* idx, const float* d2, const float* nrm, const float* col_in, const unsigned char* pending_in, long M, int k, int C,
                         float* col_out, unsigned char* pending_out, int* counter, utx_stream stream) {
    const char* const me = "utx_knn_inpaint_step";
    if (M < 0 || M > 0x7fffffffL || k < 1 || k > 32 || C < 1 || C > 16) return fail(ctx, -2, me);      // the neighbour ids are int32
    if (M == 0) return 0;
    if (!idx || !d2 || !nrm || !col_in || !pending_in || !col_out || !pending_out || !counter) return fail(ctx, -2, me);
    if (col_in == col_out || pending_in == pending_out) return fail(ctx, -2, me);      // a step reads one pair and writes the other
    if (misaligned(idx, 3) || misaligned(d2, 3) || misaligned(nrm, 3) || misaligned(col_in, 3) || misaligned(col_out, 3) || misaligned(counter, 3))
        return fail(ctx, -2, me);
    UTX_CALL(ctx, me, utx_launch_knn_inpaint_step(idx, d2, nrm, col_in, pending_in, M, k, C, col_out, pending_out, counter, (hipStream_t)stream));
}
// ---- Poisson image fusion (image_fusion.hip) ----
int utx_mask_morph(utx_ctx* ctx, const unsigned char* mask_in, int H, int W, int n, unsigned char* tmp, unsigned char* mask_out, utx_stream stream) {
    const char* const me = "utx_mask_morph";
    if (H <= 0 || W <= 0 || n == 0 || n > 31 || n < -31) return fail(ctx, -2, me);
    if (!mask_in || !tmp || !mask_out || tmp == mask_in || tmp == mask_out) return fail(ctx, -2, me);
    UTX_CALL(ctx, me, utx_launch_mask_morph(mask_in, H, W, n, tmp, mask_out, (hipStream_t)stream));
}
int utx_mask_bbox(utx_ctx* ctx, const unsigned char* mask, int H, int W, int* rect, utx_stream stream) {
    const char* const me = "utx_mask_bbox";
    if (H <= 0 || W <= 0 || !mask || !rect || misaligned(rect, 3)) return fail(ctx, -2, me);
    UTX_CALL(ctx, me, utx_launch_mask_bbox(mask, H, W, rect, (hipStream_t)stream));
}
int utx_image_fusion_cycles(int w, int h) { return utx_image_fusion_cycles_impl(w, h); }
long utx_image_fusion_workspace_bytes(int w, int h) { return (long)utx_image_fusion_workspace_bytes_impl(w, h); }
int utx_image_fusion(utx_ctx* ctx, const unsigned char* src, const unsigned char* dst, const unsigned char* mask, int H, int W, int x1, int y1, int w, int h,
                     int cycles, unsigned char* out, float* out_f, void* work, long work_bytes, utx_stream stream) {
    const char* const me = "utx_image_fusion";
    if (H <= 0 || W <= 0 || x1 < 0 || y1 < 0 || w < 0 || h < 0 || w > W - x1 || h > H - y1 || cycles < 0 || cycles > 64) return fail(ctx, -2, me);
    if (!src || !dst || !mask || !out || misaligned(out_f, 3)) return fail(ctx, -2, me);
    if (w >= 3 && h >= 3 && (!work || misaligned(work, 3) || work_bytes < (long)utx_image_fusion_workspace_bytes_impl(w, h))) return fail(ctx, -2, me);
    UTX_CALL(ctx, me, utx_launch_image_fusion(src, dst, mask, H, W, x1, y1, w, h, cycles, out, out_f, work, (hipStream_t)stream));
}
// ---- Telea inpainting (inpaint.hip) ----
int utx_inpaint_distance(utx_ctx* ctx, const unsigned char* hole, int H, int W, int* tmp, int* d2, utx_stream stream) {
    const char* const me = "utx_inpaint_distance";
    if (H <= 0 || W <= 0 || H > UTX_INPAINT_SIDE_MAX || W > UTX_INPAINT_SIDE_MAX) return fail(ctx, -2, me);
    if (!hole || !tmp || !d2 || tmp == d2 || misaligned(tmp, 3) || misaligned(d2, 3)) return fail(ctx, -2, me);
    UTX_CALL(ctx, me, utx_launch_inpaint_distance(hole, H, W, tmp, d2, (hipStream_t)stream));
}
int utx_inpaint_telea_step(utx_ctx* ctx, const float* col_in, const unsigned char* done_in, const int* d2, int H, int W, int C, int radius, float* col_out,
                           unsigned char* done_out, int* counter, utx_stream stream) {
    const char* const me = "utx_inpaint_telea_step";
    if (H <= 0 || W <= 0 || H > UTX_INPAINT_SIDE_MAX || W > UTX_INPAINT_SIDE_MAX || C < 1 || C > 4 || radius < 1 || radius > UTX_INPAINT_RADIUS_MAX)
        return fail(ctx, -2, me);
    if (!col_in || !done_in || !d2 || !col_out || !done_out || !counter) return fail(ctx, -2, me);
    if (col_in == col_out || done_in == done_out) return fail(ctx, -2, me);      // a sweep reads one pair and writes the other
    if (misaligned(col_in, 3) || misaligned(col_out, 3) || misaligned(d2, 3) || misaligned(counter, 3)) return fail(ctx, -2, me);
    UTX_CALL(ctx, me, utx_launch_inpaint_telea_step(col_in, done_in, d2, H, W, C, radius, col_out, done_out, counter, (hipStream_t)stream));
}
int utx_inpaint_finish(utx_ctx* ctx, const float* col, int H, int W, int C, unsigned char* out, float* out_f, utx_stream stream) {
    const char* const me = "utx_inpaint_finish";
    if (H <= 0 || W <= 0 || H > UTX_INPAINT_SIDE_MAX || W > UTX_INPAINT_SIDE_MAX || C < 1 || C > 4) return fail(ctx, -2, me);
    if (!col || !out || misaligned(col, 3) || misaligned(out_f, 3) || col == out_f) return fail(ctx, -2, me);
    UTX_CALL(ctx, me, utx_launch_inpaint_finish(col, H, W, C, out, out_f, (hipStream_t)stream));
}
// ---- sliced optimal-transport colour transfer and its bilateral regulariser (color_transfer.hip) ----
long utx_color_transfer_ot_workspace_bytes(long N, int C) { return (long)utx_color_transfer_ot_workspace_bytes_impl(N, C); }
int utx_color_transfer_ot(utx_ctx* ctx, const float* src, const float* dst, const float* dirs, long N, int C, int steps, int batch_size, float* out, void* work,
                          long work_bytes, utx_stream stream) {
    const char* const me = "utx_color_transfer_ot";
    if (N < 1 || N >= UTX_COLOR_TRANSFER_N_MAX || C < 1 || C > 4 || steps < 0 || batch_size < 1) return fail(ctx, -2, me);
    if (!src || !dst || !out || out == src || out == dst || misaligned(src, 3) || misaligned(dst, 3) || misaligned(out, 3)) return fail(ctx, -2, me);
    if (steps > 0 && (!dirs || misaligned(dirs, 3) || !work || work_bytes < (long)utx_color_transfer_ot_workspace_bytes_impl(N, C))) return fail(ctx, -2, me);
    UTX_CALL(ctx, me, utx_launch_color_transfer_ot(src, dst, dirs, N, C, steps, batch_size, out, work, (size_t)(steps > 0 ? work_bytes : 0), (hipStream_t)stream));
}
int utx_bilateral_lds_bytes(int radius, int C) {
    if (radius < 1 || radius > 1024 || C < 1 || C > 4) return -2;
    return (int)utx_bilateral_lds_bytes_impl(radius, C);
}
int utx_bilateral_filter(utx_ctx* ctx, const float* img, int H, int W, int C, int radius, const float* space_weights, float color_coef, float* out,
                         utx_stream stream) {
    const char* const me = "utx_bilateral_filter";
    if (H < 1 || W < 1 || H > UTX_BILATERAL_SIDE_MAX || W > UTX_BILATERAL_SIDE_MAX || (long)H * W >= UTX_COLOR_TRANSFER_N_MAX) return fail(ctx, -2, me);
    if ((C != 1 && C != 3) || radius < 1 || radius > UTX_BILATERAL_RADIUS_MAX || !(color_coef <= 0.0f)) return fail(ctx, -2, me);
    if (!img || !space_weights || !out || img == out || misaligned(img, 3) || misaligned(space_weights, 3) || misaligned(out, 3)) return fail(ctx, -2, me);
    UTX_CALL(ctx, me, utx_launch_bilateral_filter(img, H, W, C, radius, space_weights, color_coef, out, (hipStream_t)stream));
}
// ---- silhouette antialiasing of screen-space buffers (antialias.hip) ----
int utx_antialias_analyze(utx_ctx* ctx, const float* rast, const float* pos, long pos_view_stride, const int* tri, const int* opp, int F, int V, int B, int H, int W,
                          float* weights, utx_stream stream) {
    const char* const me = "utx_antialias_analyze";
    if (F <= 0 || V <= 0 || B <= 0 || H <= 0 || W <= 0 || (pos_view_stride != 0 && pos_view_stride != 4L * V)) return fail(ctx, -2, me);
    if (!rast || !pos || !tri || !opp || !weights || (const void*)rast == (const void*)weights) return fail(ctx, -2, me);
    if (misaligned(rast, 15) || misaligned(weights, 15) || misaligned(pos, 15) || misaligned(tri, 3) || misaligned(opp, 3)) return fail(ctx, -2, me);
    UTX_CALL(ctx, me, utx_launch_antialias_analyze(rast, pos, pos_view_stride, tri, opp, F, V, B, H, W, weights, (hipStream_t)stream));
}
int utx_antialias_apply(utx_ctx* ctx, const float* color, const float* weights, int B, int H, int W, int C, float* out, utx_stream stream) {
    const char* const me = "utx_antialias_apply";
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0) return fail(ctx, -2, me);
    if (!color || !weights || !out || out == color || out == weights) return fail(ctx, -2, me);
    if (misaligned(weights, 15) || misaligned(color, 3) || misaligned(out, 3)) return fail(ctx, -2, me);
    UTX_CALL(ctx, me, utx_launch_antialias_apply(color, weights, B, H, W, C, out, (hipStream_t)stream));
}
int utx_camera_normals(utx_ctx* ctx, const float* nrm, int V, const float* c2ws, int n_views, float* out, utx_stream stream) {
    if (!nrm || !c2ws || !out) return fail(ctx, -2, "utx_camera_normals");
    UTX_CALL(ctx, "utx_camera_normals", utx_launch_camera_normals(nrm, V, c2ws, n_views, out, (hipStream_t)stream));
}

// ---- image-based PBR shading (pbr.hip) ----
int utx_cubemap_table(int N, float costheta_cutoff, float* texels_host, float* tiles_host_or_null) {
    return utx_cubemap_table_impl(N, costheta_cutoff, texels_host, tiles_host_or_null);
}
int utx_latlong_to_cubemap(utx_ctx* ctx, const float* latlong, int Hi, int Wi, int N, float* out, utx_stream stream) {
    if (!latlong || !out) return fail(ctx, -2, "utx_latlong_to_cubemap");
    UTX_CALL(ctx, "utx_latlong_to_cubemap", utx_launch_latlong_to_cubemap(latlong, Hi, Wi, N, out, (hipStream_t)stream));
}
int utx_cubemap_diffuse(utx_ctx* ctx, const float* cube, int N, const float* texels_dev, float* out, utx_stream stream) {
    if (!cube || !texels_dev || !out || ((uintptr_t)texels_dev & 15)) return fail(ctx, -2, "utx_cubemap_diffuse");      // the table is read as float4
    UTX_CALL(ctx, "utx_cubemap_diffuse", utx_launch_cubemap_diffuse(cube, N, texels_dev, out, (hipStream_t)stream));
}
int utx_cubemap_specular(utx_ctx* ctx, const float* cube, int N, const float* texels_dev, const float* tiles_dev, float roughness, float costheta_cutoff,
                         float* out, utx_stream stream) {
    if (!cube || !texels_dev || !tiles_dev || !out || ((uintptr_t)texels_dev & 15) || ((uintptr_t)tiles_dev & 15)) return fail(ctx, -2, "utx_cubemap_specular");
    UTX_CALL(ctx, "utx_cubemap_specular", utx_launch_cubemap_specular(cube, N, texels_dev, tiles_dev, roughness, costheta_cutoff, out, (hipStream_t)stream));
}
int utx_dfg_lut(utx_ctx* ctx, int R, int n_samples, float* out, utx_stream stream) {
    if (!out) return fail(ctx, -2, "utx_dfg_lut");
    UTX_CALL(ctx, "utx_dfg_lut", utx_launch_dfg_lut(R, n_samples, out, (hipStream_t)stream));
}
int utx_cube_sample(utx_ctx* ctx, const float* cube, int N, const float* dirs, long n, float* out, utx_stream stream) {
    if (!cube || !dirs || !out) return fail(ctx, -2, "utx_cube_sample");
    UTX_CALL(ctx, "utx_cube_sample", utx_launch_cube_sample(cube, N, dirs, n, out, (hipStream_t)stream));
}
int utx_pbr_forward(utx_ctx* ctx, const float* view_pos, int view_stride, const float* world_pos, const float* world_nrm, const float* kd, int kd_stride,
                    const float* ks, const float* light_diffuse, int Nd, const float* light_specular, int Ns, const float* fg_lut, int R, long npix,
                    float* out_diffuse, float* out_specular, utx_stream stream) {
    if (!view_pos || !world_pos || !world_nrm || !kd || !ks || !light_diffuse || !light_specular || !fg_lut || !out_diffuse || !out_specular)
        return fail(ctx, -2, "utx_pbr_forward");
    UTX_CALL(ctx, "utx_pbr_forward", utx_launch_pbr_forward(view_pos, view_stride, world_pos, world_nrm, kd, kd_stride, ks, light_diffuse, Nd, light_specular, Ns,
                                                            fg_lut, R, npix, out_diffuse, out_specular, (hipStream_t)stream));
}
int utx_pbr_shade(utx_ctx* ctx, const float* rast, const int* tri, const float* v_pos, const float* v_nrm, const float* v_uv, const float* kd, int Hk, int Wk,
                  const float* ks_or_null, int Hs, int Ws, const float* eye3_host, const float* light_diffuse, int Nd, const float* light_specular, int Ns,
                  const float* fg_lut, int R, float lambda_diffuse, float lambda_specular, const float* bg3_host, long npix, void* out_u8,
                  float* out_rgba_or_null, utx_stream stream) {
    if (!rast || !tri || !v_pos || !v_nrm || !v_uv || !kd || !eye3_host || !light_diffuse || !light_specular || !fg_lut || !bg3_host || !out_u8)
        return fail(ctx, -2, "utx_pbr_shade");
    if (((uintptr_t)rast & 15) || ((uintptr_t)out_rgba_or_null & 15)) return fail(ctx, -2, "utx_pbr_shade");      // read / stored as float4
    UTX_CALL(ctx, "utx_pbr_shade", utx_launch_pbr_shade(rast, tri, v_pos, v_nrm, v_uv, kd, Hk, Wk, ks_or_null, Hs, Ws, eye3_host, light_diffuse, Nd, light_specular, Ns,
                                                        fg_lut, R, lambda_diffuse, lambda_specular, bg3_host, npix, out_u8, out_rgba_or_null, (hipStream_t)stream));
}
int utx_pbr_shading_normal(utx_ctx* ctx, const float* view_pos, int view_stride, const float* world_pos, const float* perturbed_nrm, const float* smooth_nrm,
                           const float* smooth_tng, const float* geom_nrm, long npix, float* out, utx_stream stream) {
    if (!view_pos || !world_pos || !perturbed_nrm || !smooth_nrm || !smooth_tng || !geom_nrm || !out) return fail(ctx, -2, "utx_pbr_shading_normal");
    UTX_CALL(ctx, "utx_pbr_shading_normal", utx_launch_pbr_shading_normal(view_pos, view_stride, world_pos, perturbed_nrm, smooth_nrm, smooth_tng, geom_nrm, npix, out,
                                                                          (hipStream_t)stream));
}
int utx_pbr_shade_nm(utx_ctx* ctx, const float* rast, const int* tri, const float* v_pos, const float* v_nrm, const float* v_tng, const float* f_nrm, const float* v_uv,
                     const float* kd, int Hk, int Wk, const float* ks_or_null, int Hs, int Ws, const float* nm, int Hn, int Wn, const float* eye3_host,
                     const float* light_diffuse, int Nd, const float* light_specular, int Ns, const float* fg_lut, int R, float lambda_diffuse, float lambda_specular,
                     const float* bg3_host, long npix, void* out_u8, float* out_rgba_or_null, utx_stream stream) {
    if (!rast || !tri || !v_pos || !v_nrm || !v_tng || !f_nrm || !v_uv || !kd || !nm || !eye3_host || !light_diffuse || !light_specular || !fg_lut || !bg3_host || !out_u8)
        return fail(ctx, -2, "utx_pbr_shade_nm");
    if (((uintptr_t)rast & 15) || ((uintptr_t)out_rgba_or_null & 15)) return fail(ctx, -2, "utx_pbr_shade_nm");      // read / stored as float4
    UTX_CALL(ctx, "utx_pbr_shade_nm", utx_launch_pbr_shade_nm(rast, tri, v_pos, v_nrm, v_tng, f_nrm, v_uv, kd, Hk, Wk, ks_or_null, Hs, Ws, nm, Hn, Wn, eye3_host,
                                                              light_diffuse, Nd, light_specular, Ns, fg_lut, R, lambda_diffuse, lambda_specular, bg3_host, npix, out_u8,
                                                              out_rgba_or_null, (hipStream_t)stream));
}

// ---- environment renderer (scene.hip) ----
int utx_scene_render(utx_ctx* ctx, const float* c2ws, const float* intrinsics, int intr_stride, int B, int H, int W, const float* cubemap_or_null, int N,
                     const float* latlong_or_null, int Hi, int Wi, int C, float* rays_d_or_null, float* cubemap_attr_or_null, float* uv_or_null,
                     float* latlong_attr_or_null, utx_stream stream) {
    if (!c2ws || !intrinsics) return fail(ctx, -2, "utx_scene_render");
    UTX_CALL(ctx, "utx_scene_render", utx_launch_scene_render(c2ws, intrinsics, intr_stride, B, H, W, cubemap_or_null, N, latlong_or_null, Hi, Wi, C, rays_d_or_null,
                                                              cubemap_attr_or_null, uv_or_null, latlong_attr_or_null, (hipStream_t)stream));
}
int utx_cubemap_to_latlong(utx_ctx* ctx, const float* cubemap, int N, int C, int Ht, int Wt, float* out, utx_stream stream) {
    if (!cubemap || !out) return fail(ctx, -2, "utx_cubemap_to_latlong");
    UTX_CALL(ctx, "utx_cubemap_to_latlong", utx_launch_cubemap_to_latlong(cubemap, N, C, Ht, Wt, out, (hipStream_t)stream));
}
int utx_scene_bake_latlong(utx_ctx* ctx, const float* w2cs, const float* projections, const float* images_or_null, int M, int H, int W, int C, int Ht, int Wt,
                           float* uv_or_null, float* uv_alpha_or_null, float* latlong_attr_or_null, utx_stream stream) {
    if (!w2cs || !projections) return fail(ctx, -2, "utx_scene_bake_latlong");
    UTX_CALL(ctx, "utx_scene_bake_latlong", utx_launch_scene_bake_latlong(w2cs, projections, images_or_null, M, H, W, C, Ht, Wt, uv_or_null, uv_alpha_or_null,
                                                                          latlong_attr_or_null, (hipStream_t)stream));
}

int utx_condition_shade(utx_ctx* ctx, const float* rast, const float* nrm, const float* pos, const float* bg3_host, long npix,
                        void* out_normal, void* out_ccm, void* out_alpha, utx_stream stream) {
    if (!rast || !nrm || !pos || !bg3_host || !out_normal || !out_ccm || !out_alpha) return fail(ctx, -2, "utx_condition_shade");
    UTX_CALL(ctx, "utx_condition_shade", utx_launch_condition_shade(rast, nrm, pos, bg3_host, npix, out_normal, out_ccm, out_alpha, (hipStream_t)stream));
}
int utx_bvh_build(utx_ctx* ctx, const float* verts, int V, const int* faces, int F, utx_bvh** out, utx_stream stream) {
    if (!verts || !faces || !out) return fail(ctx, -2, "utx_bvh_build");
    UTX_CALL(ctx, "utx_bvh_build", utx_bvh_build_impl(verts, V, faces, F, out, (hipStream_t)stream));
}
size_t utx_bvh_workspace_bytes(int F) { return utx_bvh_workspace_bytes_impl(F); }
int utx_bvh_build_ws(utx_ctx* ctx, const float* verts, int V, const int* faces, int F, void* work, size_t work_bytes, utx_bvh** out, utx_stream stream) {
    if (!verts || !faces || !out || !work) return fail(ctx, -2, "utx_bvh_build_ws");
    UTX_CALL(ctx, "utx_bvh_build_ws", utx_bvh_build_ws_impl(verts, V, faces, F, work, work_bytes, out, (hipStream_t)stream));
}
void utx_bvh_free(utx_bvh* bvh) { utx_bvh_free_impl(bvh); }
int utx_bvh_arrays(utx_bvh* bvh, int** info, float** aabb, unsigned** codes_sorted, int** idx_sorted) {
    return utx_bvh_arrays_impl(bvh, info, aabb, codes_sorted, idx_sorted);
}
int utx_bvh_trace(utx_ctx* ctx, utx_bvh* bvh, const float* ro, const float* rd, long R, int* tid, utx_stream stream) {
    if (!bvh || !ro || !rd || !tid) return fail(ctx, -2, "utx_bvh_trace");
    UTX_CALL(ctx, "utx_bvh_trace", utx_bvh_trace_impl(bvh, ro, rd, R, tid, nullptr, g_utx_opt.bvh_stack_walk, (hipStream_t)stream));
}
int utx_bvh_trace_count(utx_ctx* ctx, utx_bvh* bvh, const float* ro, const float* rd, long R, int* tid, unsigned long long* visited, utx_stream stream) {
    if (!bvh || !ro || !rd || !tid || !visited) return fail(ctx, -2, "utx_bvh_trace_count");
    UTX_CALL(ctx, "utx_bvh_trace_count", utx_bvh_trace_impl(bvh, ro, rd, R, tid, visited, 0, (hipStream_t)stream));
}
int utx_bvh_depth(utx_bvh* bvh) { return bvh ? utx_bvh_depth_impl(bvh) : -2; }
int utx_visible_faces_rays(utx_ctx* ctx, utx_bvh* bvh, const float* verts, const int* faces, int F, const float* c2ws, int B, int perspective, int flags,
                           unsigned char* mask, unsigned long long* visited, utx_stream stream) {
    const char* const me = "utx_visible_faces_rays";
    if (!bvh || !verts || !faces || !c2ws || !mask) return fail(ctx, -2, me);
    if (F <= 0 || B <= 0 || B > 65535 || (flags & ~(UTX_VF_STACK_WALK | UTX_VF_FACE_ORDER))) return fail(ctx, -2, me);
    UTX_CALL(ctx, me, utx_visible_faces_rays_impl(bvh, verts, faces, F, c2ws, B, perspective, flags, mask, visited, (hipStream_t)stream));
}
int utx_bvh_closest_point(utx_ctx* ctx, utx_bvh* bvh, const float* points, long N, float* dist, int* face, float* uvw, float* closest, unsigned long long* visited,
                          int flags, utx_stream stream) {
    const char* const me = "utx_bvh_closest_point";
    if (!bvh || N < 0 || N >= (1l << 31) || (flags & ~(UTX_CP_EXHAUSTIVE | UTX_CP_NO_SEED)) || (N > 0 && (!points || !dist))) return fail(ctx, -2, me);
    UTX_CALL(ctx, me, utx_bvh_closest_point_impl(bvh, points, N, dist, face, uvw, closest, visited, flags, (hipStream_t)stream));
}
int utx_bvh_intersect(utx_ctx* ctx, utx_bvh* bvh, const float* rays_o, const float* rays_d, long R, int* tid, float* t, float* loc, float* uv, unsigned char* front,
                      unsigned char* face_mask, unsigned long long* visited, int flags, utx_stream stream) {
    const char* const me = "utx_bvh_intersect";
    if (!bvh || R < 0 || R >= (1l << 31) || (flags & ~UTX_RC_STACK_WALK) || (R > 0 && (!rays_o || !rays_d))) return fail(ctx, -2, me);
    UTX_CALL(ctx, me, utx_bvh_intersect_impl(bvh, rays_o, rays_d, R, tid, t, loc, uv, front, face_mask, visited, flags, (hipStream_t)stream));
}
int utx_bvh_occluded(utx_ctx* ctx, utx_bvh* bvh, const float* from, const float* to, long R, unsigned char* blocked, unsigned long long* visited, int flags,
                     utx_stream stream) {
    const char* const me = "utx_bvh_occluded";
    if (!bvh || R < 0 || R >= (1l << 31) || (flags & ~UTX_RC_STACK_WALK) || (R > 0 && (!from || !to || !blocked))) return fail(ctx, -2, me);
    UTX_CALL(ctx, me, utx_bvh_occluded_impl(bvh, from, to, R, blocked, visited, flags, (hipStream_t)stream));
}
int utx_points_enclosed(utx_ctx* ctx, utx_bvh* bvh, const float* points, long N, int n_rays, unsigned long long seed, unsigned stream_id, const float* dirs_or_null,
                        unsigned char* inner, int* hits, unsigned long long* visited, int flags, utx_stream stream) {
    const char* const me = "utx_points_enclosed";
    if (!bvh || N < 0 || N >= (1l << 31) || n_rays < 1 || n_rays > 1024 || (flags & ~(UTX_RC_STACK_WALK | UTX_RC_NO_EARLY_EXIT)) || (N > 0 && (!points || !inner)))
        return fail(ctx, -2, me);
    UTX_CALL(ctx, me, utx_points_enclosed_impl(bvh, points, N, n_rays, seed, stream_id, dirs_or_null, inner, hits, visited, flags, (hipStream_t)stream));
}
int utx_sphere_directions(utx_ctx* ctx, long n_points, long n_rays, unsigned long long seed, unsigned stream_id, float* out, utx_stream stream) {
    UTX_CALL(ctx, "utx_sphere_directions", utx_launch_sphere_directions(n_points, n_rays, seed, stream_id, out, (hipStream_t)stream));
}
int utx_visible_faces_raster(utx_ctx* ctx, const float* rast, int B, int H, int W, int F, unsigned char* mask, utx_stream stream) {
    if (!rast || !mask || B <= 0 || H <= 0 || W <= 0 || F <= 0) return fail(ctx, -2, "utx_visible_faces_raster");
    UTX_CALL(ctx, "utx_visible_faces_raster", utx_launch_visible_faces_raster(rast, B, H, W, F, mask, (hipStream_t)stream));
}
int utx_erode_faces(utx_ctx* ctx, unsigned char* mask, const int* faces, int B, int F, int V, int depth, int* vstamp, utx_stream stream) {
    if (!mask || !faces || B <= 0 || B > 65535 || F <= 0 || V <= 0 || (depth > 0 && !vstamp)) return fail(ctx, -2, "utx_erode_faces");
    UTX_CALL(ctx, "utx_erode_faces", utx_launch_erode_faces(mask, faces, B, F, V, depth, vstamp, (hipStream_t)stream));
}
int utx_visible_vertices(utx_ctx* ctx, const unsigned char* mask, const int* faces, int B, int F, int V, unsigned char* out, utx_stream stream) {
    if (!mask || !faces || !out || B <= 0 || B > 65535 || F <= 0 || V <= 0) return fail(ctx, -2, "utx_visible_vertices");
    UTX_CALL(ctx, "utx_visible_vertices", utx_launch_visible_vertices(mask, faces, B, F, V, out, (hipStream_t)stream));
}
int utx_backproject(utx_ctx* ctx, const utx_backproject_desc* d, utx_bvh* bvh, utx_stream stream) {
    if (!d || !bvh || !d->rast2d || !d->verts || !d->faces || !d->fnormal || !d->vndc || !d->dirs || !d->images ||
        !d->color || !d->rayvis || !d->alphaok || d->view_begin < 0 || d->view_begin + d->view_count > d->n_views)
        return fail(ctx, -2, "utx_backproject");
    UTX_CALL(ctx, "utx_backproject", utx_launch_backproject(d, nullptr, 0, bvh, (hipStream_t)stream));
}
int utx_backproject_persp(utx_ctx* ctx, const utx_backproject_desc* d, const float* eyes, utx_bvh* bvh, utx_stream stream) {
    if (!d || !eyes || !bvh || !d->rast2d || !d->verts || !d->faces || !d->fnormal || !d->vndc || !d->images ||
        !d->color || !d->rayvis || !d->alphaok || d->view_begin < 0 || d->view_begin + d->view_count > d->n_views)
        return fail(ctx, -2, "utx_backproject_persp");
    UTX_CALL(ctx, "utx_backproject_persp", utx_launch_backproject(d, eyes, 0, bvh, (hipStream_t)stream));
}
int utx_backproject_sampled(utx_ctx* ctx, const utx_backproject_desc* d, const float* eyes, int sample_mode, utx_bvh* bvh, utx_stream stream) {
    if (!d || !bvh || !d->rast2d || !d->verts || !d->faces || !d->fnormal || !d->vndc || (!eyes && !d->dirs) || !d->images ||
        !d->color || !d->rayvis || !d->alphaok || d->view_begin < 0 || d->view_begin + d->view_count > d->n_views ||
        (sample_mode != 0 && sample_mode != 1) || d->H <= 0 || d->W <= 0)
        return fail(ctx, -2, "utx_backproject_sampled");
    UTX_CALL(ctx, "utx_backproject_sampled", utx_launch_backproject(d, eyes, sample_mode, bvh, (hipStream_t)stream));
}
int utx_dilate_visibility(utx_ctx* ctx, const void* rayvis, const void* alphaok, const float* rast2d, int n_views, int H, int W,
                          void* tmp, void* vis_out, utx_stream stream) {
    if (!rayvis || !alphaok || !rast2d || !tmp || !vis_out) return fail(ctx, -2, "utx_dilate_visibility");
    UTX_CALL(ctx, "utx_dilate_visibility", utx_launch_dilate_visibility(rayvis, alphaok, rast2d, n_views, H, W, tmp, vis_out, (hipStream_t)stream));
}
int utx_composite(utx_ctx* ctx, const float* colors, const void* vis, const int* order_host, int n_order, long T, float* atlas,
                  void* winner, utx_stream stream) {
    if (!colors || !vis || !order_host || !atlas || !winner) return fail(ctx, -2, "utx_composite");
    UTX_CALL(ctx, "utx_composite", utx_launch_composite(colors, vis, order_host, n_order, T, atlas, winner, (hipStream_t)stream));
}
int utx_seam_mask(utx_ctx* ctx, const void* winner, const float* rast2d, int H, int W, void* tmp, void* seam, utx_stream stream) {
    if (!winner || !rast2d || !tmp || !seam) return fail(ctx, -2, "utx_seam_mask");
    UTX_CALL(ctx, "utx_seam_mask", utx_launch_seam_mask(winner, rast2d, H, W, tmp, seam, (hipStream_t)stream));
}
int utx_seam_mask_sized(utx_ctx* ctx, const void* winner, const float* rast2d, int H, int W, int k_boundary, int k_boundary_blur, void* tmp, void* seam,
                        utx_stream stream) {
    if (!winner || !rast2d || !tmp || !seam || H <= 0 || W <= 0 || k_boundary < 0 || k_boundary_blur < 0 || k_boundary / 2 > 15 || k_boundary_blur / 2 > 15)
        return fail(ctx, -2, "utx_seam_mask_sized");
    UTX_CALL(ctx, "utx_seam_mask_sized", utx_launch_seam_mask_sized(winner, rast2d, H, W, k_boundary, k_boundary_blur, tmp, seam, (hipStream_t)stream));
}
int utx_view_visibility(utx_ctx* ctx, const float* attr6, const float* rast, const float* fnormal, const float* dirs, int n, int H, int W,
                        float grad_thr, float cos_thr, int radius, void* tmp, void* vis, float* alpha, utx_stream stream) {
    if (!attr6 || !rast || !fnormal || !dirs || !tmp || !vis) return fail(ctx, -2, "utx_view_visibility");
    UTX_CALL(ctx, "utx_view_visibility", utx_launch_view_visibility(attr6, rast, fnormal, dirs, nullptr, n, H, W, grad_thr, cos_thr, radius, tmp, vis, alpha, (hipStream_t)stream));
}
int utx_view_visibility_persp(utx_ctx* ctx, const float* attr6, const float* rast, const float* fnormal, const float* eyes, int n, int H, int W,
                              float grad_thr, float cos_thr, int radius, void* tmp, void* vis, float* alpha, utx_stream stream) {
    if (!attr6 || !rast || !fnormal || !eyes || !tmp || !vis) return fail(ctx, -2, "utx_view_visibility_persp");
    UTX_CALL(ctx, "utx_view_visibility_persp", utx_launch_view_visibility(attr6, rast, fnormal, nullptr, eyes, n, H, W, grad_thr, cos_thr, radius, tmp, vis, alpha, (hipStream_t)stream));
}
long utx_knn_workspace_bytes(long N) { return (long)utx_knn_workspace_bytes_impl(N); }
int utx_knn(utx_ctx* ctx, const utx_knn_desc* d, void* work, long work_bytes, utx_stream stream) {
    if (!d || !d->src_pos || !d->dst_pos || !work) return fail(ctx, -2, "utx_knn");
    UTX_CALL(ctx, "utx_knn", utx_launch_knn(d, work, (size_t)work_bytes, (hipStream_t)stream));
}
long utx_fps_workspace_bytes(long N) { return (long)utx_fps_workspace_bytes_impl(N); }
int utx_fps(utx_ctx* ctx, const float* pos, const void* mask, long N, int M, int start, int* out_idx, float* out_d2, void* work, long work_bytes,
            utx_stream stream) {
    if (!pos || !out_idx || !work || work_bytes < 0) return fail(ctx, -2, "utx_fps");
    UTX_CALL(ctx, "utx_fps", utx_launch_fps(pos, (const unsigned char*)mask, N, M, start, out_idx, out_d2, work, (size_t)work_bytes, (hipStream_t)stream));
}
int utx_sample_edges_equal_steps(utx_ctx* ctx, const float* verts, const int* edges, const int* edge_ids, const float* start, const float* length, int E,
                                 float total, long N, float* samples, int* edge_index, float* edge_t, utx_stream stream) {
    if (!verts || !edges || !start || !length || !samples) return fail(ctx, -2, "utx_sample_edges_equal_steps");
    UTX_CALL(ctx, "utx_sample_edges_equal_steps", utx_launch_sample_edges(verts, edges, edge_ids, start, length, E, total, N, samples, edge_index, edge_t, (hipStream_t)stream));
}
int utx_sample_surface(utx_ctx* ctx, const float* verts, const int* faces, const float* cum, int F, long N, unsigned long long seed, float* samples,
                       int* face_index, float* uvw, utx_stream stream) {
    if (!verts || !faces || !cum || !samples) return fail(ctx, -2, "utx_sample_surface");
    UTX_CALL(ctx, "utx_sample_surface", utx_launch_sample_surface(verts, faces, cum, F, N, seed, samples, face_index, uvw, (hipStream_t)stream));
}
int utx_sample_offsets(utx_ctx* ctx, const float* base, const int* faces, int F, const int* face_index, const float* uvw, const float* vnormal, const float* uniforms,
                       long N, unsigned long long seed, int stream_id, float threshold, float* out, utx_stream stream) {
    UTX_CALL(ctx, "utx_sample_offsets", utx_launch_sample_offsets(base, faces, F, face_index, uvw, vnormal, uniforms, N, seed, stream_id, threshold, out,
                                                                  (hipStream_t)stream));
}
int utx_sample_attrs(utx_ctx* ctx, const int* faces, const int* faces_2d, const float* uvs_2d, int F, const int* face_index, const float* uvw, long N, int n_attr,
                     const float* const* src_host, const int* dims_host, float* const* out_host, utx_stream stream) {
    UTX_CALL(ctx, "utx_sample_attrs", utx_launch_sample_attrs(faces, faces_2d, uvs_2d, F, face_index, uvw, N, n_attr, src_host, dims_host, out_host, (hipStream_t)stream));
}
long utx_nn_fill_workspace_bytes(long T) { return (long)utx_nn_fill_workspace_bytes_impl(T); }
int utx_nn_fill(utx_ctx* ctx, const float* pos, const void* winner, const float* rast2d, long T, float* atlas, int* nn_index,
                void* work, long work_bytes, utx_stream stream) {
    if (!pos || !winner || !rast2d || !atlas || !work) return fail(ctx, -2, "utx_nn_fill");
    UTX_CALL(ctx, "utx_nn_fill", utx_launch_nn_fill(pos, winner, rast2d, T, 3, atlas, nn_index, work, (size_t)work_bytes, (hipStream_t)stream));
}
int utx_lens_blur_seam(utx_ctx* ctx, const float* src, const void* seam, int H, int W, const float* k49_host, float* dst, utx_stream stream) {
    if (!src || !seam || !k49_host || !dst) return fail(ctx, -2, "utx_lens_blur_seam");
    UTX_CALL(ctx, "utx_lens_blur_seam", utx_launch_lens_blur_seam(src, seam, H, W, 3, k49_host, dst, (hipStream_t)stream));
}
int utx_gaussian_blur_seam(utx_ctx* ctx, const float* src, const void* seam, int H, int W, int ksize, const float* w1_host, float* dst, utx_stream stream) {
    if (!src || !seam || !w1_host || !dst || H <= 0 || W <= 0 || ksize < 1 || ksize > 31 || (ksize & 1) == 0 || ksize / 2 >= H || ksize / 2 >= W)
        return fail(ctx, -2, "utx_gaussian_blur_seam");
    UTX_CALL(ctx, "utx_gaussian_blur_seam", utx_launch_gaussian_blur_seam(src, seam, H, W, 3, ksize, w1_host, dst, (hipStream_t)stream));
}
long utx_pull_push_workspace_bytes(int H, int W) { return (long)utx_pull_push_workspace_bytes_impl(H, W, 3); }
int utx_pull_push(utx_ctx* ctx, const float* kd, const void* mask, int H, int W, float* out, void* work, utx_stream stream) {
    if (!kd || !mask || !out || !work) return fail(ctx, -2, "utx_pull_push");
    UTX_CALL(ctx, "utx_pull_push", utx_launch_pull_push(kd, mask, H, W, 3, out, work, (hipStream_t)stream));
}
/* ---- the C-channel (PBR stack) bake: visibility and winner without colour, one gather from the winning view, C-channel post-processing ---- */
int utx_backproject_vis(utx_ctx* ctx, const utx_backproject_desc* d, const float* eyes, int sample_mode, utx_bvh* bvh, utx_stream stream) {
    if (!d || !bvh || !d->rast2d || !d->verts || !d->faces || !d->fnormal || !d->vndc || (!eyes && !d->dirs) || !d->images ||
        !d->rayvis || !d->alphaok || d->view_begin < 0 || d->view_count <= 0 || d->view_begin + d->view_count > d->n_views ||
        (sample_mode != 0 && sample_mode != 1) || d->H <= 0 || d->W <= 0)
        return fail(ctx, -2, "utx_backproject_vis");
    UTX_CALL(ctx, "utx_backproject_vis", utx_launch_backproject_vis(d, eyes, sample_mode, bvh, (hipStream_t)stream));
}
int utx_composite_winner(utx_ctx* ctx, const void* vis, int n_views, const int* order_host, int n_order, long T, void* winner, utx_stream stream) {
    if (!vis || !order_host || !winner) return fail(ctx, -2, "utx_composite_winner");
    UTX_CALL(ctx, "utx_composite_winner", utx_launch_composite_winner(vis, n_views, order_host, n_order, T, winner, (hipStream_t)stream));
}
int utx_gather_winner(utx_ctx* ctx, const float* rast2d, const int* faces, const float* vndc, const float* images, const void* winner, long T, int V,
                      int n_views, int H, int W, int C, int sample_mode, float* atlas, utx_stream stream) {
    if (!rast2d || !faces || !vndc || !images || !winner || !atlas || C < 1 || C > 16) return fail(ctx, -2, "utx_gather_winner");
    UTX_CALL(ctx, "utx_gather_winner", utx_launch_gather_winner(rast2d, faces, vndc, images, winner, T, V, n_views, H, W, C, sample_mode, atlas, (hipStream_t)stream));
}
int utx_nn_fill_c(utx_ctx* ctx, const float* pos, const void* winner, const float* rast2d, long T, int C, float* atlas, int* nn_index,
                  void* work, long work_bytes, utx_stream stream) {
    if (!pos || !winner || !rast2d || !atlas || !nn_index || !work || C < 1 || C > 16) return fail(ctx, -2, "utx_nn_fill_c");
    UTX_CALL(ctx, "utx_nn_fill_c", utx_launch_nn_fill(pos, winner, rast2d, T, C, atlas, nn_index, work, (size_t)work_bytes, (hipStream_t)stream));
}
int utx_lens_blur_seam_c(utx_ctx* ctx, const float* src, const void* seam, int H, int W, int C, const float* k49_host, float* dst, utx_stream stream) {
    if (!src || !seam || !k49_host || !dst || C < 1 || C > 16) return fail(ctx, -2, "utx_lens_blur_seam_c");
    UTX_CALL(ctx, "utx_lens_blur_seam_c", utx_launch_lens_blur_seam(src, seam, H, W, C, k49_host, dst, (hipStream_t)stream));
}
int utx_gaussian_blur_seam_c(utx_ctx* ctx, const float* src, const void* seam, int H, int W, int C, int ksize, const float* w1_host, float* dst, utx_stream stream) {
    if (!src || !seam || !w1_host || !dst || C < 1 || C > 16 || H <= 0 || W <= 0 || ksize < 1 || ksize > 31 || (ksize & 1) == 0 || ksize / 2 >= H || ksize / 2 >= W)
        return fail(ctx, -2, "utx_gaussian_blur_seam_c");
    UTX_CALL(ctx, "utx_gaussian_blur_seam_c", utx_launch_gaussian_blur_seam(src, seam, H, W, C, ksize, w1_host, dst, (hipStream_t)stream));
}
long utx_pull_push_workspace_bytes_c(int H, int W, int C) { return (long)utx_pull_push_workspace_bytes_impl(H, W, C); }
int utx_pull_push_c(utx_ctx* ctx, const float* kd, const void* mask, int H, int W, int C, float* out, void* work, utx_stream stream) {
    if (!kd || !mask || !out || !work || C < 1 || C > 16) return fail(ctx, -2, "utx_pull_push_c");
    UTX_CALL(ctx, "utx_pull_push_c", utx_launch_pull_push(kd, mask, H, W, C, out, work, (hipStream_t)stream));
}
int utx_chart_flood(utx_ctx* ctx, const int* adj, const int* bucket, int F, int* chart, int* flag, utx_stream stream) {
    if (!adj || !bucket || !chart || !flag) return fail(ctx, -2, "utx_chart_flood");
    const int rc = utx_launch_chart_flood(adj, bucket, F, chart, flag, (hipStream_t)stream);
    if (rc < 0) return fail(ctx, rc, "utx_chart_flood");
    return rc;
}
int utx_to_u8(utx_ctx* ctx, const float* src, long n_rows, long row_elems, int flip, void* dst, utx_stream stream) {
    if (!src || !dst) return fail(ctx, -2, "utx_to_u8");
    UTX_CALL(ctx, "utx_to_u8", utx_launch_to_u8(src, n_rows, row_elems, flip, dst, (hipStream_t)stream));
}

}  // extern "C"

// Layout self-description, so the ctypes mirror in unitex_amd/_lib.py can be checked without a GPU.
extern "C" int utx_abi_sizes(int* out, int n) {
    const int v[] = {(int)sizeof(utx_gemm_desc), (int)sizeof(utx_gemv_desc), (int)sizeof(utx_qkv_post_desc),
                     (int)sizeof(utx_ln_mod_desc), (int)sizeof(utx_sched_desc), (int)sizeof(utx_backproject_desc),
                     (int)sizeof(utx_knn_desc), (int)sizeof(utx_dit_linear), (int)sizeof(utx_dit_double_block), (int)sizeof(utx_dit_single_block),
                     (int)sizeof(utx_dit_weights), (int)sizeof(utx_dit_config), (int)sizeof(utx_dit_workspace)};
    const int m = (int)(sizeof(v) / sizeof(v[0]));
    for (int i = 0; i < m && i < n; ++i) out[i] = v[i];
    return m;
}

/*
 * libunitex_hip.so -- C ABI of the MI355X (gfx950) hot path of UniTEX.
 *
 * Drop-in boundary for: CustomRGBTextureFullPipeline's FLUX-DiT denoise loop and the TextureTools
 * render / UV back-projection.  Every entry point below names the reference
 * interface it replaces (paths relative to /root/reference).
 *
 * Conventions
 *  - plain C: raw device pointers + sizes, no torch / C++ types.  All device memory is owned by the
 *    caller (PyTorch-ROCm allocations in the Python host); the library borrows pointers for the
 *    duration of a call and never frees or retains them, except opaque handles it allocates itself
 *    (utx_ctx, utx_bvh) that the caller releases with utx_free / utx_bvh_free.
 *  - every launch is stream-ordered on the caller's `stream` (a hipStream_t passed as void*), no
 *    hidden synchronisation unless stated.
 *  - return 0 on success, negative error code otherwise; utx_last_error(ctx) gives a message.
 *    The reference signals errors by Python exceptions/asserts (e.g.
 *    TextureTools/texturetools/render/nvdiffrast/renderer_inverse.py:171,256-261); the Python shim
 *    (unitex_amd/_lib.py) turns non-zero codes into RuntimeError.
 *  - bf16 tensors are passed as uint16_t storage.
 */
#ifndef UNITEX_HIP_H
#define UNITEX_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: exactly the functions declared in this header are exported (tests/test_abi.py compares `nm -D` with
 * this file); its internal launchers are not part of the ABI. */
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define UTX_VERSION 100

typedef struct utx_ctx utx_ctx;
typedef void* utx_stream;   /* hipStream_t */

int utx_version(void);
int utx_init(int device, utx_ctx** ctx);
void utx_free(utx_ctx* ctx);
const char* utx_last_error(utx_ctx* ctx);

/* Launch options (kernel selection / scheduling A/B).  Every one is RESULT-PRESERVING: identical bits, except that the two
 * tail-split switches (UTX_ATTN_TAILSPLIT, UTX_GEMM_STREAMK) change the fp32 summation order inside the tiles
 * they split -- the same result up to rounding, deterministic from launch to launch.  The first utx_init reads the environment
 * variables of the same names once; later changes go through utx_set_option only (no getenv on the launch path).  Names:
 * UTX_ATTN_Q64, UTX_ATTN_TAILSPLIT, UTX_GEMM_GROUP_M, UTX_GEMM_TILE (0, 128 or 2564: with any other value utx_gemm_bf16 and utx_gemm_plan return -2),
 * UTX_GEMM_STREAMK, UTX_GEMM_FASTK, UTX_GEMM_PERS_GRID, UTX_BVH_STACK_WALK, UTX_BVH_PACKET, UTX_ATTN_PEEL, UTX_ATTN8_PEEL, UTX_NN_GRID.  UTX_ATTN_Q64 (default 1: the
 * 4 x 64 attention kernel for the launches it takes) keeps the bits wherever the 8 x 32 kernel does not re-centre its running maximum behind the first 32 keys; where it does, the two
 * kernels return two roundings of the same softmax.  The timing-ablation switches that compute wrong
 * results (UTX_ATTN_VAR, UTX_ATTN_DEBUG, UTX_GEMM_DEBUG) exist only in the separately built libunitex_hip_ablate.so (tools/ only): in
 * this library they return -7 and the environment variables are ignored.  Returns -2 for an unknown name. */
int utx_set_option(const char* name, int value);
int utx_get_option(const char* name, int* value);
int utx_is_ablation_build(void);

/* ------------------------------------------------------------------------------------------------
 * FLUX DiT denoise step  (flux_piplines/texturing/pipeline.py:634-681; transformer blocks are
 * diffusers' FluxTransformer2DModel [3p], attention core restated in
 * flux_piplines/texturing/attention_processor.py:31-110)
 * ---------------------------------------------------------------------------------------------- */

/* Flash attention forward, bf16 in/out, fp32 softmax + accumulation, non-causal, head_dim 128.
 * Replaces F.scaled_dot_product_attention at attention_processor.py:89-91.
 *   q, k : element (h, s, d) at base + h*{q,k}_hs + s*{q,k}_ss + d; k rows must be readable (finite)
 *          up to the next multiple of 64 past S (keys >= S are masked, never used)
 *   vt   : V transposed, element (h, d, s) at base + h*vt_hs + d*vt_ds + s; every row must be readable
 *          (finite) up to the next multiple of 64 past S
 *   o    : element (s, h, d) at base + s*o_ss + h*128 + d
 * Strides in elements; q/k/vt base pointers 16-byte aligned; q_hs, k_hs, vt_hs, q_ss, k_ss, vt_ds multiples of 8,
 * o_ss multiple of 4.
 * softmax_scale > 0: the reference's scale (1/sqrt(128)); softmax_scale == 0: Q was pre-multiplied by
 * scale*log2(e) by utx_qkv_post (q_scale) and scores are used as base-2 exponents directly.
 * One call may issue up to five stream-ordered operations (a memset of the flag bytes, full rounds of workgroups, the key-split tail round, its merge, the repair pass).
 * Since round 6 the launches that qualify -- softmax_scale == 0, S a multiple of 64, contiguous operands, key_bias_period == 0, scratch present -- run the 4 x 64 kernel
 * (attention_q64.hip: one wave per SIMD, generated instruction stream) followed by its repair pass; all others the 8 x 32 kernel (attention_glds.hip).
 * The tail round needs scratch.  utx_attn_fwd_bf16_ws takes it from the caller (utx_attn_workspace_bytes: nothing is allocated on the
 * launch path, re-entrant per stream / buffer).  The entry points without a workspace argument use a buffer owned by the CONTEXT, grown
 * with hipMalloc by the first call that needs more (never while the stream is being captured: such a launch stays unsplit -- same
 * result up to one bf16 rounding of the tail rows); calls through one context must not run concurrently on different streams. */
int utx_attn_fwd_bf16(utx_ctx* ctx, const void* q, const void* k, const void* vt, void* o,
                      long q_hs, long q_ss, long k_hs, long k_ss, long vt_hs, long vt_ds, long o_ss,
                      int H, int S, float softmax_scale, utx_stream stream);
/* The same with KEY MULTIPLICITY: every key of tile 0 (keys 0..63) -- and, with key_bias_period = n > 0, of every 64-key tile
 * whose index is a multiple of n -- stands for 2^key_bias_log2 identical keys: key_bias_log2 is added to its base-2 scores, which
 * is exactly softmax over the repeated keys.  Used by the text-token dedup of unitex_amd/flux/transformer.py: the reference feeds
 * 512 all-zero text embeddings with all-zero position ids (flux_piplines/texturing/pipeline.py:538-543), i.e. 512 IDENTICAL tokens
 * at every layer (last bullet); 64 of them are carried, each counting 8-fold.  key_bias_log2 = 0 is utx_attn_fwd_bf16. */
int utx_attn_fwd_bf16_kb(utx_ctx* ctx, const void* q, const void* k, const void* vt, void* o,
                         long q_hs, long q_ss, long k_hs, long k_ss, long vt_hs, long vt_ds, long o_ss,
                         int H, int S, float softmax_scale, float key_bias_log2, int key_bias_period, utx_stream stream);
/* The same with a QUERY COUNT OF ITS OWN: rows 0 .. S_q-1 of q are the queries (o gets S_q rows), keys / values are all S_kv tokens; q and k / vt are separate arrays and
 * S_q may be smaller or (since round 6: the sequence-parallel launch over de-duplicated text keys, utx_sp_unpack_qkv_dedup) larger than S_kv.  S_q < S_kv is used by
 * the last transformer block: the pipeline discards the prediction of the condition tokens (flux_piplines/texturing/pipeline.py:645,660,684:
 * the condition tail of the latents is re-pinned before every transformer call and cut off at the end), so only the noise tokens need
 * a query in the block whose output nobody attends to any more (unitex_amd/flux/transformer.py, `set_output_rows`). */
int utx_attn_fwd_bf16_kbq(utx_ctx* ctx, const void* q, const void* k, const void* vt, void* o,
                          long q_hs, long q_ss, long k_hs, long k_ss, long vt_hs, long vt_ds, long o_ss,
                          int H, int S_q, int S_kv, float softmax_scale, float key_bias_log2, int key_bias_period, utx_stream stream);
/* The same with CALLER-OWNED scratch for the key-split tail round: work >= utx_attn_workspace_bytes(ctx, H, S_q, S_kv) bytes, 16-byte aligned, used only
 * by the launches of this call (stream-ordered); layout [key-split scratch | one flag byte per 64-query group (the 4 x 64 kernel's headroom record)].  work == NULL or too small:
 * the tail round is not split and the 8 x 32 kernel runs.  Both sizing calls follow the QUERY count and accept S_q > S_kv like the launch itself.  utx_attn_plan (pure host arithmetic,
 * no device): out = {workgroups, workgroups in full rounds of n_cus, key ranges per tail workgroup (1 = not split), 64-key tiles per range}. */
int utx_attn_fwd_bf16_ws(utx_ctx* ctx, const void* q, const void* k, const void* vt, void* o,
                         long q_hs, long q_ss, long k_hs, long k_ss, long vt_hs, long vt_ds, long o_ss,
                         int H, int S_q, int S_kv, float softmax_scale, float key_bias_log2, int key_bias_period,
                         void* work, size_t work_bytes, utx_stream stream);
size_t utx_attn_workspace_bytes(utx_ctx* ctx, int H, int S_q, int S_kv);

/* MX fp8 attention -- OPT-IN (BASELINE configs[4] "fp8 MFMA"; the reference has no fp8 path: the contract is this library's own and is a different numerics
 * contract from the bf16 kernel above, with its own stated tolerance: tests/test_attention_fp8_gpu.py, and per element the counted interval of
 * oracle/attention_fp8_fp64.py, tests/test_attention_fp8_edges_gpu.py).  Same joint attention as utx_attn_fwd_bf16_kbq
 * (attention_processor.py:31-110: softmax(Q K^T) V per head over the joint sequence; Q arrives pre-scaled by scale * log2(e), so scores are base-2 exponents)
 * with Q K^T and P V on the fp8 matrix pipe: Q8 / K8 [H][S_pad][128] e4m3 bytes + qs / ks [H][S_pad] dwords (four E8M0 bytes per row: the 32-channel blocks
 * of d) -- what utx_quant_mx8 makes of the head-major Q / K viewed as [H * S_pad, 128] with lds = 4; V8^T [H][128][S_pad] e4m3 + vs [H][S_pad / 32][32][4]
 * E8M0 bytes per (block of 32 keys, channel d % 32, d / 32) -- what utx_quant_vt_mx8 makes of V^T [H][128][S_pad] bf16.  P is quantised to e4m3 with the unit
 * scale inside the kernel, round to nearest even with gradual underflow (p <= 256 by the kernel's re-centring rule; p is taken relative to the running maximum, and
 * p <= 2^-10 becomes zero, 2^-10 < p < 1.5 * 2^-9 becomes 2^-9).  Output o [S_q][o_ss] bf16, head h in columns 128 h ..; S_q <= S_kv queries (the first S_q rows of
 * Q8), S_pad = rows allocated (multiple of 64).  The pad region need not be zero, only FINITE: K8 rows and V8^T columns in [S_kv, S_pad) are read and masked (no
 * 0x7F / 0xFF element byte and no 0xFF scale byte there: a NaN would survive 0 x v), Q8 / qs rows >= S_q are never read; key_bias_* as utx_attn_fwd_bf16_kb. */
int utx_quant_vt_mx8(utx_ctx* ctx, const void* vt, void* v8, void* vs, int H, int S_pad, utx_stream stream);
int utx_attn_fwd_fp8(utx_ctx* ctx, const void* q8, const void* qs, const void* k8, const void* ks, const void* v8t, const void* vs, void* o, long o_ss,
                     int H, int S_q, int S_kv, int S_pad, float key_bias_log2, int key_bias_period, utx_stream stream);
/* The same with CALLER-OWNED scratch for the key-split tail round (round 6: the bf16 kernel's plan, work items and merge): work >= utx_attn_workspace_bytes(ctx, H, S_q, S_kv)
 * bytes, 16-byte aligned; null / too small: the launch stays unsplit.  utx_attn_fwd_fp8 uses the context's per-stream scratch (none while the stream is capturing). */
int utx_attn_fwd_fp8_ws(utx_ctx* ctx, const void* q8, const void* qs, const void* k8, const void* ks, const void* v8t, const void* vs, void* o, long o_ss,
                        int H, int S_q, int S_kv, int S_pad, float key_bias_log2, int key_bias_period, void* work, size_t work_bytes, utx_stream stream);
int utx_attn_plan(int H, int S_q, int S_kv, int n_cus, int out[4]);
/* The same on BLOCK-STRIDED operands: the S_kv tokens (queries and keys alike) come in blocks of blk_rows (a multiple of 64 that divides S_kv); block b of Q / K /
 * V^T of a head starts q_bs / k_bs / vt_bs elements (multiples of 8) behind block b - 1, rows inside a block are q_ss / k_ss apart, V^T rows vt_ds (each holding the
 * blk_rows columns of its block).  This is the receive buffer of the sequence-parallel Q / K / V all-to-all, [source rank][q | k | v][head][S_loc x 128]
 * (unitex_amd/flux/ulysses.py), consumed where RCCL put it instead of behind a relayout pass; the output rows stay in token order (block-major), o_ss apart.
 * Same tiles in the same order as the contiguous call: bit-identical results.  Replaces nothing in the reference (it is single-GPU); beyond it, SURVEY 8e. */
int utx_attn_fwd_bf16_blk(utx_ctx* ctx, const void* q, const void* k, const void* vt, void* o,
                          long q_hs, long q_ss, long k_hs, long k_ss, long vt_hs, long vt_ds, long o_ss,
                          int H, int S_q, int S_kv, float softmax_scale, float key_bias_log2, int key_bias_period,
                          void* work, size_t work_bytes, int blk_rows, long q_bs, long k_bs, long vt_bs, utx_stream stream);

/* C = epi(alpha * (A B^T + A2 B2^T) + bias): bf16 GEMM, fp32 accumulate, fused epilogues.
 * Replaces every nn.Linear (+ peft LoRA branch, + GELU, + gated residual) inside the FLUX blocks
 * (attention_processor.py:42-45,60-63,101-106; pipeline.py:108-112 LoRA adapters;
 * trainer.py:282-295 LoRA targets). See unitex_amd/csrc/gemm.hip for the epilogue definitions. */
typedef struct utx_gemm_desc {
    const void* A; long lda;      /* [M,K]  bf16, K contiguous */
    const void* B; long ldb;      /* [N,K]  bf16 (torch Linear weight) */
    const void* A2; long lda2;    /* optional LoRA segment: [M, nseg*K2] = s * x A_lora^T */
    const void* B2; long ldb2;    /* [N,K2] LoRA up weight */
    int M, N, K, K2;              /* K, K2 multiples of 64; N multiple of 8 */
    int lora_n_limit;             /* output columns < limit take the LoRA segment; >= N or a multiple of 128 (else -2) */
    int lora_seg_n;               /* A2 column block for column n is (n / lora_seg_n) * K2 */
    float alpha;
    const void* bias;             /* [N] bf16 or NULL */
    int gelu_from;                /* columns >= gelu_from get GELU(tanh); N for none; below N a multiple of 4 (else -2) */
    const void* gate;             /* [N] bf16 or NULL: out = res + gate * y */
    const void* res; long ldres;  /* residual [M,N] bf16 (may alias C) */
    void* C; long ldc;
    int n_split; void* C1; long ldc1;  /* columns >= n_split go to C1[m, n - n_split]; N for none */
    int ntn;                      /* internal */
    /* implicit 3x3 convolution (conv_Wo > 0): A is an NHWC activation [Hi*Wi, Cin] (Cin = 1 << conv_cin_log2 >= 64),
     * B the weight [N, 9*Cin] with K order (ky, kx, cin), M = Ho*Wo output pixels, K = 9*Cin.  Tap (ky,kx) of output
     * pixel (oy,ox) reads input (oy*stride + ky - pad, ox*stride + kx - pad) of the (conv_up ? 2x nearest-upsampled
     * : plain) image; out-of-range taps read zero_page (>= 128 zero bytes).  Replaces torch Conv2d(3x3) (+ the
     * F.pad(0,1,0,1) stride-2 downsampler and the nearest-2x upsampler) of the FLUX VAE [3p]. */
    int conv_Hi, conv_Wi, conv_Wo, conv_cin_log2, conv_stride, conv_pad, conv_up;
    const void* zero_page;
    /* OCP MX fp8 base segment (mx8 = 1; BASELINE configs[4] "fp8 MFMA weights"): A [M,K] and B [N,K] hold e4m3 bytes (lda / ldb
     * in bytes, K a multiple of 128) and a_scale [M][K/32] / b_scale [N][K/32] one E8M0 byte per 32 elements along K (row strides
     * lds_a / lds_b bytes, multiples of 4); element value = e4m3 * 2^(scale - 127).  Accumulation in fp32 by
     * v_mfma_scale_f32_32x32x64_f8f6f4; the LoRA segment (A2 / B2) stays bf16; epilogues unchanged.  Quantise activations with
     * utx_quant_mx8; weights once at load (unitex_amd/flux/mx8.py).  Replaces the same nn.Linear as the bf16 form.
     * mx8 = 2: the same operands with TILE-PACKED scales (utx_quant_mx8_packed; lds_a / lds_b = row blocks of 128 per K-tile slab of a_scale /
     * b_scale) on the persistent one-wave-per-SIMD kernel: N and every column boundary (n_split, gelu_from) multiples of 256, no LoRA segment
     * (K2 = 0: merge the adapters into the weight before quantising), no fused q / k epilogue; anything else is refused (-2), never dropped. */
    const void* a_scale; long lds_a;
    const void* b_scale; long lds_b;
    int mx8;
    /* Fused q / k post-processing (qk_cols > 0; the "fused QKV + RMSNorm + RoPE" of the hot path; one-wave-per-SIMD kernel only -- a wave owns
     * a whole 128-column head there): output columns n < qk_cols are NOT written to C; each 128-column head slab gets what utx_qkv_post does
     * to q (columns < qk_cols / 2) or k (the rest): per-head RMSNorm with qk_wq / qk_wk, RoPE from qk_cos / qk_sin ([tok][64] fp32, token =
     * qk_tok_off + row), q scaled by qk_q_scale, head-major store to qk_Qh / qk_Kh ([H][S_pad][128], head stride qk_hs elements) -- same
     * arithmetic, same rounding points, same summation order, bit-identical to GEMM -> utx_qkv_post (attention_processor.py:42-87).  Columns
     * >= qk_cols (v, the MLP half of a single block) take the plain epilogue; v is transposed by utx_qkv_post with skip_qk = 1. */
    int qk_cols;                       /* 0 = off; else 2 * H * 128 */
    int qk_tok_off;
    float qk_eps, qk_q_scale;
    const void* qk_wq; const void* qk_wk;
    const float* qk_cos; const float* qk_sin;
    void* qk_Qh; void* qk_Kh; long qk_hs;
    /* Optional scratch for the balanced tail of the one-wave-per-SIMD kernel (UTX_GEMM_STREAMK, default on): when the 256 x 256 tiles do not
     * fill the last round of workgroups, the K loops of that round's tiles are cut into equal ranges over all CUs, the fp32 partial tiles
     * pass through sk_work and a second small kernel sums them in K order and runs the epilogue (deterministic; differs from the unsplit
     * result only by fp32 summation order).  Caller-owned, >= utx_gemm_streamk_workspace_bytes(), one buffer per stream that launches
     * GEMMs concurrently; NULL = never split. */
    void* sk_work; size_t sk_work_bytes;
    /* mx8 == 2 only, optional: the GELU part of the output (columns n >= gelu_from) leaves as OCP MX fp8 -- the A operand of the NEXT mx8 = 2 GEMM
     * (FLUX: GELU(ff.net.0) feeds ff.net.2; GELU(proj_mlp) feeds proj_out) -- instead of bf16: bytes q_out [M][ldq_out] at column n - gelu_from,
     * tile-packed scales qs_out (qs_out_rb row blocks per K-tile slab), K-tile q_out_kt0 + (n - gelu_from) / 128.  Bit-identical to the bf16
     * epilogue followed by utx_quant_mx8_packed (rounded to bf16, then quantised per block of 32 columns); C / C1 are not written for those
     * columns.  (N - gelu_from) % 128 == 0, ldq_out % 8 == 0.  The split tail round is not used by such a launch.  As with utx_quant_mx8_packed, rows >= M
     * are not written: neither their bytes in q_out nor their scales in the last row block of qs_out, nor any K-tile slab outside q_out_kt0 ..
     * q_out_kt0 + (N - gelu_from) / 128 - 1 or row block >= ceil(M / 128).  With row-major scales (mx8 = 1), a gate, gelu_from off a 128 multiple or
     * qs_out_rb < ceil(M / 128) the launch is refused (-2) and nothing is written (tests/test_gemm_mx_edges_gpu.py). */
    void* q_out; long ldq_out;
    void* qs_out; long qs_out_rb;
    int q_out_kt0;
} utx_gemm_desc;
int utx_gemm_bf16(utx_ctx* ctx, const utx_gemm_desc* d, utx_stream stream);
size_t utx_gemm_streamk_workspace_bytes(utx_ctx* ctx);   /* size of utx_gemm_desc.sk_work for this device (2 partial tiles per CU) */
/* What utx_gemm_bf16 would do with this descriptor on a device of n_cus compute units under the current launch options -- the library's own dispatch
 * arithmetic, no device needed (the host uses it to decide which projections can take the fused q / k epilogue, and bench.py to report the launch census):
 * out[0] = kernel (0 128x128 tiles, 1 one wave per SIMD; 2, 3 and 4 named retired kernels and are never returned), out[1] = output tiles of that kernel (128^2 for kernel 0, else 256^2), out[2] = tiles
 * of the last round that are cut along K (0: unsplit; needs d->sk_work != NULL), out[3] = K ranges per such tile.  Returns -2 for a bad argument and for a UTX_GEMM_TILE
 * value that names no kernel, as utx_gemm_bf16 does. */
int utx_gemm_plan(const utx_gemm_desc* d, int n_cus, int out[4]);

/* OCP MX fp8 quantisation of a bf16 matrix along its rows (the activation operand of an mx8 GEMM):
 *   per block of 32 consecutive elements: e = floor(log2(max|x|)) - 8 (clamped to [-127, 127]; -127 for an all-zero block),
 *   scale byte = e + 127, q = e4m3_rne(clamp(x * 2^-e, -448, 448)).
 * x [M][ldx] bf16 (K % 32 == 0, ldx % 8 == 0) -> q [M][ldq] bytes, s [M][lds] bytes (K/32 per row).  oracle/mx8_ref.py restates it. */
int utx_quant_mx8(utx_ctx* ctx, const void* x, long ldx, void* q, long ldq, void* s, long lds, int M, int K, utx_stream stream);
/* The same quantiser (identical q bytes and scale values) with the scales TILE-PACKED for utx_gemm_desc.mx8 == 2 (the one-wave-per-SIMD kernel,
 * unitex_amd/csrc/gemm_w4.hip): s is an array of dwords [K/128][row_blocks][32][4]; dword [kt][rb][l][im] holds the four E8M0 bytes of the
 * 32-element blocks 4 kt .. 4 kt + 3 of row 128 rb + 32 im + l (byte j = block 4 kt + j).  row_blocks >= ceil(M / 128); K % 128 == 0; s 16-byte
 * aligned, K/128 * row_blocks * 512 bytes.  Rows >= M of the last row block are not written.  A lane of the GEMM then fetches the scale dwords of
 * its four fragment rows for a K-tile with ONE 16-byte load (512 contiguous bytes per wave) instead of four strided dword gathers. */
int utx_quant_mx8_packed(utx_ctx* ctx, const void* x, long ldx, void* q, long ldq, void* s, long row_blocks, int M, int K, utx_stream stream);

/* y[m,n] = act_out(sum_k act_in(x[m,k]) W[n,k] + b[n]) for M <= 8 (embedders, AdaLN modulation). */
typedef struct utx_gemv_desc {
    const void* x; long ldx;
    const void* W; long ldw;
    const void* bias;
    void* y; long ldy;
    int M, N, K;
    int silu_in, silu_out;
} utx_gemv_desc;
int utx_gemv_bf16(utx_ctx* ctx, const utx_gemv_desc* d, utx_stream stream);

/* ---- FLUX AutoencoderKL pieces (diffusers [3p]; encode at flux_piplines/texturing/pipeline.py:226-238, decode at
 * :683-692).  Activations are NHWC bf16 [H*W, C].  Convolutions with Cin >= 64 are utx_gemm_bf16 in conv mode. */
/* GroupNorm(32 groups, C % 128 == 0) + affine (+ SiLU): work = utx_group_norm_workspace_bytes() bytes. */
size_t utx_group_norm_workspace_bytes(void);
int utx_group_norm(utx_ctx* ctx, const void* x, long npix, int C, const void* gamma, const void* beta, float eps, int silu,
                   void* y, void* work, utx_stream stream);
/* in-place row softmax of a bf16 matrix [nrow, ncol] (row stride ld elements; ncol, ld multiples of 8). */
int utx_softmax_rows(utx_ctx* ctx, void* s, long nrow, long ld, int ncol, utx_stream stream);
/* 3x3 / stride 1 / pad 1 convolution for thin inputs (Cin = 3 or 16): wt is [9*Cin][Cout] bf16 (tap-major). */
int utx_conv3x3_thin(utx_ctx* ctx, const void* x, int H, int W, int Cin, const void* wt, const void* bias, int Cout, void* y,
                     utx_stream stream);

/* per-head RMSNorm(q,k) + RoPE + head-major relayout + V transpose
 * (attention_processor.py:50-57,76-87). */
typedef struct utx_qkv_post_desc {
    const void* qkv; long ld;
    int q_col, k_col, v_col;
    const void* wq; const void* wk;          /* [128] bf16 RMSNorm weights */
    const float* cosb; const float* sinb;    /* [S_total][64] fp32 rotary tables */
    void* Qh; void* Kh; void* Vt;            /* [H][S_pad][128], [H][S_pad][128], [H][128][S_pad] */
    long hs_qk, hs_v, S_pad;
    int n_tok, tok_off, H;
    float eps;
    float q_scale;                           /* multiplies Q before its bf16 rounding (1 = reference layout;
                                                scale*log2(e) feeds utx_attn_fwd_bf16(softmax_scale = 0)) */
    /* grouped head addressing (sequence-parallel send layout, unitex_amd/flux/ulysses.py): with heads_per_group = g > 0 head h
     * lives at (h / g) * gs + (h % g) * hs instead of h * hs, i.e. the kernel writes straight into the all-to-all send buffer
     * [P][3][H/P][...] (one group per destination rank) and no pack pass exists.  0 = plain [H][...] layout. */
    int heads_per_group;
    long gs_qk, gs_v;
    int skip_qk;                             /* 1: q and k were produced by the GEMM's fused epilogue (utx_gemm_desc.qk_cols): only V is transposed */
    /* second level of the grouped addressing (0 = off): the g heads of a destination rank are cut into head groups of sub_heads heads whose
     * exchanges are pipelined with attention (send layout [group][P][3][sub_heads][...]): head hi = h % g of a rank lives at
     * (h / g) * gs + (hi / sub_heads) * gs2 + (hi % sub_heads) * hs.  g % sub_heads == 0. */
    int sub_heads;
    long gs2_qk, gs2_v;
} utx_qkv_post_desc;
int utx_qkv_post(utx_ctx* ctx, const utx_qkv_post_desc* d, utx_stream stream);

/* Sequence-parallel ("Ulysses") exchange, receive side (unitex_amd/flux/ulysses.py; no counterpart in the single-GPU reference,
 * flux_piplines/texturing/pipeline.py:633-681 -- this is SURVEY 8(e)'s parity-preserving split of the ONE joint sequence).
 * Both are pure 16-byte-vector copies (HBM-bound), one launch each; S = P * S_loc, S_loc % 64 == 0, E = S_loc * 128.
 *   utx_sp_unpack_qkv: recv [P src][3][Hp][E]  ->  q, k [Hp][S][128] (row = src*S_loc + tok),  vt [Hp][128][S]
 *                      (recv[src][0|1][hp] is [S_loc][128]; recv[src][2][hp] is [128][S_loc])
 *   utx_sp_unpack_qkv_dedup: the same for q; k [Hp][S_k][128] and vt [Hp][128][S_k] with S_k = text_rows + P (S_loc - text_rows): the first text_rows tokens of
 *                      EVERY source rank's block are the same rows (the caller's guarantee: the identical text tokens every rank carries, flux/transformer.py) and
 *                      are kept ONCE, from source rank 0, followed by the other tokens of rank 0 .. P-1 -- the key order of the single-GPU sequence, so that a rank's
 *                      attention launch (S_q = S queries over S_kv = S_k keys) is the single-GPU launch over H / P heads.  text_rows % 64 == 0, < S_loc
 *   utx_sp_unpack_o  : recv [P src][S_loc][Hp*128]  ->  out [S_loc][ld]: columns src*Hp*128 .. of row tok
 *   utx_sp_unpack_o_cols: the same for ONE head group of several (Hp = heads of the group): source rank src lands at column src * src_cols
 *                      of `out` (src_cols = all heads of a rank x 128; `out` points at the group's first column) */
int utx_sp_unpack_qkv(utx_ctx* ctx, const void* recv, int P, int Hp, int S_loc, void* q, void* k, void* vt, utx_stream stream);
int utx_sp_unpack_qkv_dedup(utx_ctx* ctx, const void* recv, int P, int Hp, int S_loc, int text_rows, void* q, void* k, void* vt, utx_stream stream);
int utx_sp_unpack_o(utx_ctx* ctx, const void* recv, int P, int Hp, int S_loc, void* out, long ld, utx_stream stream);
int utx_sp_unpack_o_cols(utx_ctx* ctx, const void* recv, int P, int Hp, int S_loc, void* out, long ld, long src_cols, utx_stream stream);

/* LayerNorm(no affine) + AdaLN modulation (AdaLayerNormZero/ZeroSingle/Continuous [3p]). */
typedef struct utx_ln_mod_desc {
    const void* x; long ldx;
    const void* shift; const void* scale;    /* [D] bf16 */
    void* y; long ldy;
    int n_tok, D;
    float eps;
    /* q != NULL (D % 128 == 0): the result leaves as OCP MX fp8 instead of bf16 -- exactly what utx_quant_mx8_packed makes of the bf16 result
     * (the value is rounded to bf16 first, then quantised per block of 32): bytes q [n_tok][ldq], tile-packed scales qs (qs_row_blocks row
     * blocks per K-tile slab, see utx_quant_mx8_packed).  The activation operand of an mx8 = 2 GEMM without the bf16 round trip through HBM;
     * y is not written. */
    void* q; long ldq;
    void* qs; long qs_row_blocks;
} utx_ln_mod_desc;
int utx_ln_mod(utx_ctx* ctx, const utx_ln_mod_desc* d, utx_stream stream);

/* Flow-match Euler step + condition re-pin (flux_piplines/texturing/pipeline.py:644-645,660). */
typedef struct utx_sched_desc {
    void* x; const void* v; const void* cond;
    long n_noise_elems, n_total_elems;
    float dsigma;
} utx_sched_desc;
int utx_sched_step(utx_ctx* ctx, const utx_sched_desc* d, utx_stream stream);


/* ------------------------------------------------------------------------------------------------
 * TextureTools render / UV back-projection
 * (TextureTools/texturetools/render/nvdiffrast/renderer_inverse.py:159-365,574-633,
 *  raytracing/rt_aprmis, texture/stitching/mip.py, image/lens_blur.py)
 * ---------------------------------------------------------------------------------------------- */

/* clip[n][v] = [x y z 1] . mvp[n]^T ; ndc (optional, may be NULL) = clip.xy / clip.w
 * (renderer_inverse.py:263-265).  verts [V][3], mvp [n][4][4] row-major, clip [n][V][4], ndc [n][V][2]. */
int utx_transform_points(utx_ctx* ctx, const float* verts, int V, const float* mvp, int n_views,
                         float* clip, float* ndc, utx_stream stream);

/* dr.rasterize replacement (renderer_inverse.py:183,273): pos [V][4] clip space, tri [F][3] int32,
 * rast [H][W][4] = (u, v, z/w, triangle_id + 1), 0 = empty.  work: utx_rasterize_workspace_bytes.
 * Accepted range: a triangle is drawn only if x, y, w of its three vertices are finite, every w > 0, and every snapped
 * coordinate s = floor((x / w * 0.5 + 0.5) * size * 256 + 0.5) has |s| <= 2^30; H, W <= 2^22.  Any other triangle is skipped
 * whole (no clipping).  Inside the range every int64 edge function and the area are exact (at most 4 * (2^30)^2 = 2^62).
 * A pixel whose z/w is NaN or outside [-1, 1] is not covered. */
long utx_rasterize_workspace_bytes(int F, int H, int W);
int utx_rasterize(utx_ctx* ctx, const float* pos, const int* tri, int F, int H, int W, float* rast,
                  void* work, utx_stream stream);

/* dr.interpolate replacement (renderer_inverse.py:188,277,288): attr [V][C] -> out [npix][C]. */
int utx_interpolate(utx_ctx* ctx, const float* attr, int C, const float* rast, const int* tri, long npix,
                    float* out, utx_stream stream);

/* geometry-condition shading of VideoExporter.export_condition (video/export_nvdiffrast_video.py:956-989):
 * rast [npix][4], interpolated vertex normals / positions [npix][3] -> uint8 normal / ccm images [npix][3]
 * and alpha [npix], composited on bg3_host (HOST array of 3 floats), uint8 by truncation. */
int utx_condition_shade(utx_ctx* ctx, const float* rast, const float* nrm, const float* pos, const float* bg3_host,
                        long npix, void* out_normal, void* out_ccm, void* out_alpha, utx_stream stream);

/* per-face unit normals of PBRMesh (mesh/structure_v2.py:49-50): verts [V][3], faces [F][3] -> out [F][3]. */
int utx_face_normals(utx_ctx* ctx, const float* verts, const int* faces, int F, float* out, utx_stream stream);

/* textured shading of the orbit video (video/export_nvdiffrast_video.py:141-256 -> renderer_base.py:289-336
 * uv_rendering): rast [npix][4], per-vertex uv [V][2] in [0,1], tex [Ht][Wt][3] fp32 in UV-raster orientation (row
 * grows with v) -> uint8 RGB [npix][3]: bilinear fetch (wrap), background bg3_host where empty, truncation to uint8. */
int utx_texture_shade(utx_ctx* ctx, const float* rast, const float* uv, const int* tri, const float* tex, int Ht, int Wt,
                      const float* bg3_host, long npix, void* out, utx_stream stream);

/* geometry-buffer shading of the orbit video, VideoExporter.export_orbit_video(video_type=...) (video/export_nvdiffrast_video.py:141-256 ->
 * export_video :37-139 -> simple_rendering, render/nvdiffrast/renderer_base.py:153-241; alpha = coverage, no dr.antialias).  One launch per
 * frame: rast [npix][4]; tri [F][3]; attr = the per-vertex attribute the mode interpolates, vertex v at attr + v * attr_stride (floats):
 *   UTX_GBUF_WORLD_NORMAL     v_nrm [V][3]                      interpolate, F.normalize, background -1          (:160-166)
 *   UTX_GBUF_CAMERA_NORMAL    utx_camera_normals of the view    the same arm                                     (:168-176)
 *   UTX_GBUF_WORLD_POSITION   v_pos [V][3]                      interpolate, background -1                       (:178-188)
 *   UTX_GBUF_CAMERA_POSITION  utx_transform_points(w2c), xyz    interpolate, background 0                        (:228-235)
 *   UTX_GBUF_Z_DEPTH          clip w (utx_transform_points)     one channel, background 0, repeated to three     (:153-158)
 *   UTX_GBUF_DISTANCE         utx_transform_points(w2c), xyz    L2 norm of the interpolated value, background 0  (:236-241)
 * The interpolation is utx_interpolate's, bit for bit.  Then export_video :120-131: scale2_dev (DEVICE {lo, hi}, or NULL) normalises the
 * covered pixels to (x - lo) / (hi - lo); UTX_GBUF_NDC maps x * 0.5 + 0.5; UTX_GBUF_COMPOSITE x * alpha + bg3_host * (1 - alpha) (bg3_host: HOST
 * array of 3 floats, always required).  out_u8 [npix][3] = clamp(0, 1) * 255 truncated; out_rgba_or_null [npix][4] fp32, alpha fourth
 * (16-byte aligned).  rast must be 16-byte aligned too.
 * Returns -2 for a mode outside 0..5, unknown flag bits, a null pointer, a rast / RGBA pointer off a 16-byte boundary, npix <= 0 or a
 * stride below the mode's channels. */
#define UTX_GBUF_WORLD_NORMAL 0
#define UTX_GBUF_CAMERA_NORMAL 1
#define UTX_GBUF_WORLD_POSITION 2
#define UTX_GBUF_CAMERA_POSITION 3
#define UTX_GBUF_Z_DEPTH 4
#define UTX_GBUF_DISTANCE 5
#define UTX_GBUF_NDC 1
#define UTX_GBUF_COMPOSITE 2
int utx_gbuffer_shade(utx_ctx* ctx, int mode, const float* rast, const int* tri, const float* attr, int attr_stride, const float* scale2_dev,
                      int flags, const float* bg3_host, long npix, void* out_u8, float* out_rgba_or_null, utx_stream stream);

/* (lo, hi) of a mode's buffer over the covered pixels of ONE frame -> scale2_dev[0..1] (export_video :120-125: min / max of the selected
 * pixels, which export_video takes on its first frame and reuses); *empty_flag_dev = 1 if the frame covers no pixel (scale2_dev is then
 * {+inf, -inf}), else 0.  Stream-ordered, no host synchronisation.  Same argument checks as utx_gbuffer_shade. */
int utx_gbuffer_range(utx_ctx* ctx, int mode, const float* rast, const int* tri, const float* attr, int attr_stride, long npix,
                      float* scale2_dev, int* empty_flag_dev, utx_stream stream);

/* per-view, per-vertex camera-space normals of render_camera_normal (renderer_base.py:169-170): nrm [V][3], c2ws [n_views][4][4] ->
 * out [n_views][V][3] = F.normalize(nrm @ c2ws[:3,:3]) with the fixed order (n0*R0j + n1*R1j) + n2*R2j. */
int utx_camera_normals(utx_ctx* ctx, const float* nrm, int V, const float* c2ws, int n_views, float* out, utx_stream stream);

/* Atlas-space geometry buffers: NVDiffRendererBase.simple_inverse_rendering (render/nvdiffrast/renderer_base.py:352-489) with alpha = coverage
 * (no dr.antialias).  ONE launch for a whole request: rast2d [H2D][W2D][4] is the UV raster (utx_rasterize of the uvs as clip xy; 16-byte
 * aligned); faces [F][3]; v_pos, v_nrm [V][3]; for B >= 0 cameras v_pos_cam [B][V][3] (xyz of utx_transform_points with M = w2c, packed to
 * three floats per vertex) and v_nrm_cam [B][V][3] (utx_camera_normals): the per-vertex arrays the reference hands to dr.interpolate.  `want`
 * is the OR of the requested buffers; outs_host is a HOST array of UTX_UVGB_COUNT device pointers, entry k belonging to bit k (entries of
 * buffers that were not requested are not read, and nothing is written through them).  m = rast.w > 0, lerp(bg, x, m) is a select:
 *   bit  buffer            layout                covered texel                                         bg
 *   0    MASK              u8  [H2D][W2D]        1                                                      0
 *   1    ALPHA             f32 [H2D][W2D][1]     1                                                      0
 *   2    WORLD_NORMAL      f32 [1][H2D][W2D][3]  normalize(interp(v_nrm))                              -1
 *   3    WORLD_POSITION    f32 [1][H2D][W2D][3]  interp(v_pos)                                         -1
 *   4    CAMERA_NORMAL     f32 [B][H2D][W2D][3]  normalize(interp(v_nrm_cam[b]))                       -1
 *   5    CAMERA_POSITION   f32 [B][H2D][W2D][3]  interp(v_pos_cam[b])                                   0
 *   6    DISTANCE          f32 [B][H2D][W2D][1]  |interp(v_pos_cam[b])|                                 0
 *   7    Z_DEPTH           f32 [B][H2D][W2D][1]  interp(v_pos_cam[b]).z                                 0
 *   8    RAY_DIRECTION     f32 [B][H2D][W2D][3]  normalize(interp(v_pos_cam[b]))                       -1
 *   9    COS_RAY_NORMAL    f32 [B][H2D][W2D][1]  dot(camera_normal[b], ray_direction[b])               -1
 * interp is utx_interpolate's expression, bit for bit; normalize(x) = x / max(|x|, 1e-12); |x| = sqrt((x*x + y*y) + z*z); the dot product is
 * (a.x*b.x + a.y*b.y) + a.z*b.z.  Stream-ordered, no workspace, no host synchronisation.
 * Returns -2 for a null rast2d / faces / outs_host, a rast2d off a 16-byte boundary, H2D, W2D or V <= 0, B < 0, want == 0 or with unknown bits,
 * a null output pointer of a requested buffer, a null v_pos / v_nrm that a requested buffer reads, and B > 0 with a camera-dependent buffer
 * requested but its per-view array null.  With B == 0 the camera-dependent buffers are empty and nothing is written to them. */
#define UTX_UVGB_MASK 1
#define UTX_UVGB_ALPHA 2
#define UTX_UVGB_WORLD_NORMAL 4
#define UTX_UVGB_WORLD_POSITION 8
#define UTX_UVGB_CAMERA_NORMAL 16
#define UTX_UVGB_CAMERA_POSITION 32
#define UTX_UVGB_DISTANCE 64
#define UTX_UVGB_Z_DEPTH 128
#define UTX_UVGB_RAY_DIRECTION 256
#define UTX_UVGB_COS_RAY_NORMAL 512
#define UTX_UVGB_COUNT 10
#define UTX_UVGB_ALL 1023
int utx_uv_gbuffer(utx_ctx* ctx, const float* rast2d, const int* faces, const float* v_pos, const float* v_nrm, const float* v_pos_cam,
                   const float* v_nrm_cam, int V, int B, int H2D, int W2D, unsigned want, void* const* outs_host, utx_stream stream);

/* Screen-space buffers of a camera batch: NVDiffRendererBase.simple_rendering (render/nvdiffrast/renderer_base.py:101-350) with alpha = coverage
 * (no dr.antialias).  ONE launch for a whole request: rast [B][H][W][4] holds the B views' rasters (utx_rasterize per view; 16-byte aligned);
 * faces [F][3]; per vertex v_pos, v_nrm [V][3], v_uv [V][2] in [-1, 1] (uv * 2 - 1), v_attr [V][Ca]; per view and vertex clip_w [B][V] (w of
 * utx_transform_points with M = mvp), v_pos_cam [B][V][3] (xyz of utx_transform_points with M = w2c) and v_nrm_cam [B][V][3]
 * (utx_camera_normals): the per-vertex arrays the reference hands to dr.interpolate.  maps_host is a HOST array of n_maps <= UTX_SGB_MAX_MAPS
 * device pointers to fp32 maps [Ht_i][Wt_i][C_i]; map_dims_host is a HOST array {Ht_0, Wt_0, C_0, Ht_1, ...}.  `want` is the OR of the requested
 * buffers; outs_host is a HOST array of UTX_SGB_COUNT device pointers, entry k belonging to bit k (entries of buffers that were not requested
 * are not read, and nothing is written through them).  m = rast.w > 0, lerp(bg, x, m) is a select:
 *   bit  buffer            layout              covered pixel                                   bg
 *   0    MASK              u8  [B][H][W]       1                                                0
 *   1    ALPHA             f32 [B][H][W][1]    1                                                0
 *   2    WORLD_NORMAL      f32 [B][H][W][3]    normalize(interp(v_nrm))                        -1
 *   3    CAMERA_NORMAL     f32 [B][H][W][3]    normalize(interp(v_nrm_cam[b]))                 -1
 *   4    WORLD_POSITION    f32 [B][H][W][3]    interp(v_pos)                                   -1
 *   5    CAMERA_POSITION   f32 [B][H][W][3]    interp(v_pos_cam[b])                             0
 *   6    DISTANCE          f32 [B][H][W][1]    |interp(v_pos_cam[b])|                           0
 *   7    RAY_DIRECTION     f32 [B][H][W][3]    normalize(interp(v_pos_cam[b]))                 -1
 *   8    Z_DEPTH           f32 [B][H][W][1]    interp(clip_w[b])  (clip w, not camera z)        0
 *   9    COS_RAY_NORMAL    f32 [B][H][W][1]    dot(camera_normal[b], ray_direction[b])         -1
 *   10   V_ATTR            f32 [B][H][W][Ca]   interp(v_attr)                                  rule
 *   11   UV                f32 [B][H][W][2]    interp(v_uv)                                    -1
 *   12   MAP_ATTR          f32 [B][H][W][sum C_i]  the maps sampled at uv, concatenated        rule
 * interp, normalize, |x| and the dot product as in utx_uv_gbuffer.  filter (UTX_SGB_FILTER_*): BILINEAR and NEAREST are F.grid_sample(map, uv,
 * align_corners=False, padding_mode='zeros') (nearest rounds halves to even), NVDIFFRAST is dr.texture(uv * 0.5 + 0.5, filter_mode='linear') with
 * its wrap boundary (the lookups of utx_backproject_sampled).  Background rule of V_ATTR and MAP_ATTR (bg_kind, UTX_SGB_BG_*): NONE leaves the
 * computed value on every pixel (0 for V_ATTR, the maps' sample at uv = (-1, -1) for MAP_ATTR); SCALAR fills uncovered pixels with bg_scalar,
 * VECTOR with bg_v_attr [Ca] / bg_map_attr [sum C_i], DENSE with the pixel's own entry of bg_v_attr [B][H][W][Ca] / bg_map_attr [B][H][W][sum C_i]
 * (device pointers; each is read only if its buffer is requested).  Stream-ordered, no workspace, no host synchronisation.
 * B * H * W == 0 or want == 0 does nothing and returns 0 -- except that B == 0 together with a buffer that reads a per-view vertex array (bits
 * 3, 5-9) is refused, such an array having no address.  Returns -2 for a null rast / faces / outs_host, a rast off a 16-byte boundary, V <= 0, a
 * negative B, H or W, unknown bits in want, a null output pointer of a requested buffer, a null vertex array that a requested buffer reads,
 * Ca <= 0 with V_ATTR, and with MAP_ATTR: n_maps < 1 or > UTX_SGB_MAX_MAPS, a null maps_host / map_dims_host / map pointer, a map with a side
 * or channel count <= 0; an unknown filter or bg_kind, and a VECTOR / DENSE background whose pointer for a requested buffer is null. */
#define UTX_SGB_MASK 1
#define UTX_SGB_ALPHA 2
#define UTX_SGB_WORLD_NORMAL 4
#define UTX_SGB_CAMERA_NORMAL 8
#define UTX_SGB_WORLD_POSITION 16
#define UTX_SGB_CAMERA_POSITION 32
#define UTX_SGB_DISTANCE 64
#define UTX_SGB_RAY_DIRECTION 128
#define UTX_SGB_Z_DEPTH 256
#define UTX_SGB_COS_RAY_NORMAL 512
#define UTX_SGB_V_ATTR 1024
#define UTX_SGB_UV 2048
#define UTX_SGB_MAP_ATTR 4096
#define UTX_SGB_COUNT 13
#define UTX_SGB_ALL 8191
#define UTX_SGB_MAX_MAPS 4
#define UTX_SGB_FILTER_BILINEAR 0
#define UTX_SGB_FILTER_NEAREST 1
#define UTX_SGB_FILTER_NVDIFFRAST 2
#define UTX_SGB_BG_NONE 0
#define UTX_SGB_BG_SCALAR 1
#define UTX_SGB_BG_VECTOR 2
#define UTX_SGB_BG_DENSE 3
int utx_screen_gbuffer(utx_ctx* ctx, const float* rast, const int* faces, const float* v_pos, const float* v_nrm, const float* v_uv,
                       const float* v_attr, int Ca, const float* clip_w, const float* v_pos_cam, const float* v_nrm_cam, int V, int B, int H, int W,
                       int n_maps, const float* const* maps_host, const int* map_dims_host, int filter, int bg_kind, float bg_scalar,
                       const float* bg_v_attr, const float* bg_map_attr, unsigned want, void* const* outs_host, utx_stream stream);

/* Atlas-space view projection: render_uv / render_map_attr of NVDiffRendererBase.simple_inverse_rendering (render/nvdiffrast/renderer_base.py:504-559)
 * with alpha = coverage.  ONE launch for every texel of every view.  rast2d [H2D][W2D][4] is the atlas raster (16-byte aligned), faces [F][3],
 * face_mask [B][F] uint8 (utx_visible_faces_*), v_ndc [B][V][2] the views' NDC xy per vertex (utx_transform_points).  Per (b, texel), tri = rast2d.w - 1:
 *   vis = tri >= 0 && face_mask[b][tri];  uv [B][H2D][W2D][2] = vis ? interp(v_ndc[b]) (utx_interpolate's order) : (-1, -1);  uv_alpha [B][H2D][W2D][1] = vis.
 * With map != null -- map [Bm][Hm][Wm][C] fp32, Bm = 1 (shared) or B (one image per view), C >= 1; rast_map [B][Hm][Wm][4], the views rasterised at the
 * map's own size, of which only .w is read -- also map_attr [B][H2D][W2D][C]:
 *   s = the map sampled at uv (filter: UTX_SGB_FILTER_*, the lookups of utx_screen_gbuffer; an invisible texel samples at (-1, -1));
 *   cov = the nearest, zero-padded lookup of rast_map.w > 0 at uv;  uv_alpha = cov < 1 ? 0 : uv_alpha;
 *   bg_kind NONE: map_attr = cov < 1 ? map[b or 0][0][0][:] : s;  SCALAR / VECTOR (bg [C]) / DENSE (bg [B][H2D][W2D][C]): map_attr = uv_alpha ? s : bg.
 * uv is not gated by cov.  With map == null the map arguments are not read and map_attr is not written.  Stream-ordered, no workspace.
 * Returns -2 for a null rast2d / faces / face_mask / v_ndc / uv / uv_alpha, a rast2d off a 16-byte boundary, F, V, B, H2D or W2D <= 0, and with a map:
 * a null rast_map / map_attr, Bm not in {1, B}, Hm, Wm or C <= 0, an unknown filter or bg_kind, a VECTOR / DENSE background with a null bg. */
int utx_uv_project(utx_ctx* ctx, const float* rast2d, const int* faces, int F, const unsigned char* face_mask, const float* v_ndc, int V, int B, int H2D,
                   int W2D, const float* map, int Bm, int Hm, int Wm, int C, const float* rast_map, int filter, int bg_kind, float bg_scalar,
                   const float* bg, float* uv, float* uv_alpha, float* map_attr, utx_stream stream);

/* Image-based PBR shading of the turntable: PBRModel (texture/pbr/pbr.py:18-49, 91-130), NVDiffRendererPBR.render_base / render_pbr
 * (render/nvdiffrast/renderer_pbr.py:19-94) and the environment-light prefilters of the renderutils plugin (texture/pbr/renderutils/ops.py:398-465,
 * c_src/cubemap.cu:12-139, 174-298).  Cubemaps are [6][N][N][3] fp32; face s and its in-face coordinates (fx, fy) in [-1, 1] follow cube_to_dir:
 * 0 (1, -fy, -fx)  1 (-1, -fy, fx)  2 (fx, 1, fy)  3 (fx, -1, -fy)  4 (fx, -fy, 1)  5 (-fx, -fy, -1); texel i has its centre at f = 2 (i + 0.5) / N - 1.
 * Everything is fp32 data, stream-ordered, without host synchronisation; a bad size returns -2.
 *
 * Cube lookup rule (utx_cube_sample, utx_pbr_forward, utx_pbr_shade, utx_pbr_shade_nm, utx_scene_render, utx_cubemap_to_latlong; this library's own -- nvdiffrast's boundary_mode='cube' is third-party):
 *   1. face = the component of largest magnitude, ties to x, then y (a zero vector looks up the centre of face 0); (fx, fy) = the other two
 *      components over that magnitude;
 *   2. t = (f + 1) * N / 2 - 0.5, base = floor(t), fraction = t - base; a fraction within N * 2^-21 of a texel centre snaps to it (four times
 *      the fp32 uncertainty of t), so a texel-centre direction returns that texel exactly;
 *   3. the four taps (base + {0, 1})^2 blend as a + f (b - a), along x first;
 *   4. a tap that left the face along one axis is taken from the texel that holds its own direction on the neighbouring face (the edge texel
 *      of the same row);
 *   5. a tap that left along both axes is the mean ((t1 + t2) + t3) / 3 of the three texels that meet at that cube corner.
 *   The value is continuous across edges and corners. */

/* HOST tables of a cubemap size, computed in fp64 and rounded once: texels_host [6][N][N][4] = (unit direction of the texel centre, pixel_area of
 * cubemap.cu:17-30); tiles_host_or_null [6][nt][nt][4], nt = ceil(N / 16) = (unit axis, cosine bound) of every 16^2 texel tile for the lobe
 * of costheta_cutoff (utx_cubemap_specular culls with it).  N must be even (pixel_area halves it in integers), 2 <= N <= 8192.  Upload both 16-byte aligned. */
int utx_cubemap_table(int N, float costheta_cutoff, float* texels_host, float* tiles_host_or_null);

/* latlong_to_cubemap (pbr.py:28-49): latlong [Hi][Wi][3] -> out [6][N][N][3]; tu = atan2(vx, -vz) / 2pi + 0.5, tv = acos(vy) / pi, bilinear fetch
 * with wrap addressing in both axes.  Coordinates and blend are carried in fp64 and rounded once. */
int utx_latlong_to_cubemap(utx_ctx* ctx, const float* latlong, int Hi, int Wi, int N, float* out, utx_stream stream);

/* diffuse prefilter (cubemap.cu:110-139): out(n) = sum over all 6 N^2 texels of c * clamp(n.L, 0, 0.999) * pixel_area / 3.141592 (the reference's
 * constants).  texels_dev: utx_cubemap_table's texels on the device.  Fixed reduction order (run-to-run identical).  Odd N is refused. */
int utx_cubemap_diffuse(utx_ctx* ctx, const float* cube, int N, const float* texels_dev, float* out, utx_stream stream);

/* specular prefilter (cubemap.cu:174-179, 246-298 and the division of ops.py:465): over the texels with L.V >= costheta_cutoff,
 * w = max(L.V, 0) * ndfGGX(roughness^4, max(V.H, 0)) * pixel_area / 4; out = sum(c w) / sum(w).  tiles_dev (built for the same cutoff) only culls: the
 * accepted set is the cutoff test's.  A cubemap of ones returns exactly 1.0f, a lobe of one texel that texel exactly (the weights are carried relative to the first accepted texel's). */
int utx_cubemap_specular(utx_ctx* ctx, const float* cube, int N, const float* texels_dev, const float* tiles_dev, float roughness, float costheta_cutoff,
                         float* out, utx_stream stream);

/* split-sum scale / bias table out [R][R][2] at cos(theta) = (column + 0.5) / R, roughness = (row + 0.5) / R: GGX importance sampling over the
 * n_samples-point Hammersley set, height-correlated Smith GGX visibility (alpha = roughness^2), Schlick's (1 - V.H)^5. */
int utx_dfg_lut(utx_ctx* ctx, int R, int n_samples, float* out, utx_stream stream);

/* the cube lookup alone: dirs [n][3] (any length) -> out [n][3]. */
int utx_cube_sample(utx_ctx* ctx, const float* cube, int N, const float* dirs, long n, float* out, utx_stream stream);

/* PBRModel.forward (pbr.py:110-130) on dense buffers: view_pos [npix][3] (view_stride 3) or one [3] (view_stride 0), world_pos / world_nrm
 * [npix][3], kd [npix][kd_stride >= 3], ks [npix][3] = (-, roughness, metallic), fg_lut [R][R][2] indexed (x = cos, y = roughness, clamp)
 * -> out_diffuse, out_specular [npix][3]. */
int utx_pbr_forward(utx_ctx* ctx, const float* view_pos, int view_stride, const float* world_pos, const float* world_nrm, const float* kd, int kd_stride,
                    const float* ks, const float* light_diffuse, int Nd, const float* light_specular, int Ns, const float* fg_lut, int R, long npix,
                    float* out_diffuse, float* out_specular, utx_stream stream);

/* one fused PBR frame (renderer_pbr.py:19-94): rast [npix][4]; position, normal and uv interpolate as utx_interpolate does, kd [Hk][Wk][3] and
 * ks_or_null [Hs][Ws][3] fetch as utx_texture_shade does (NULL = the reference's constant [1, 1, 0], bit-identical to that texture at kd's size);
 * PBRModel.forward; rgb = lambda_diffuse * diffuse + lambda_specular * specular; background bg3_host where empty (alpha = coverage);
 * out_u8 [npix][3] = clamp(0, 1) * 255 truncated; out_rgba_or_null [npix][4] fp32, alpha fourth.  eye3_host, bg3_host: HOST arrays of 3 floats.
 * rast and out_rgba_or_null must be 16-byte aligned.  The shading normal is the interpolated vertex normal; utx_pbr_shade_nm applies a normal map. */
int utx_pbr_shade(utx_ctx* ctx, const float* rast, const int* tri, const float* v_pos, const float* v_nrm, const float* v_uv, const float* kd, int Hk, int Wk,
                  const float* ks_or_null, int Hs, int Ws, const float* eye3_host, const float* light_diffuse, int Nd, const float* light_specular, int Ns,
                  const float* fg_lut, int R, float lambda_diffuse, float lambda_specular, const float* bg3_host, long npix, void* out_u8,
                  float* out_rgba_or_null, utx_stream stream);

/* tangent-space normal map: bsdf_prepare_shading_normal (texture/pbr/renderutils/bsdf.py:28-51) with two_sided_shading = True and opengl = True
 * (glTF's convention), on dense buffers: view_pos [npix][3] (view_stride 3) or one [3] (view_stride 0); world_pos, perturbed_nrm (the decoded map value,
 * not normalised), smooth_nrm, smooth_tng, geom_nrm [npix][3] -> out [npix][3].  fp32, every sum in a fixed order; normalize(x) = x / max(|x|, 1e-12):
 *   sn = normalize(smooth_nrm);  st = normalize(smooth_tng);  vv = normalize(view_pos - world_pos);  b = normalize(cross(st, sn))
 *   s  = normalize((st * p.x - b * p.y) + sn * max(p.z, 0))
 *   dot(geom_nrm, vv) > 0 ? (s, g) = (s, geom_nrm) : (s, g) = (-s, -geom_nrm)
 *   t  = clamp(dot(vv, s) / 0.1, 0, 1);  out = g + t * (s - g)
 * out is not normalised (utx_pbr_forward normalises its normal).  A zero tangent, a tangent parallel to the normal, a zero perturbation and a negative
 * p.z give finite values (the floors turn a zero vector into a zero vector; s = 0 gives out = g).  Mirrored UV charts (handedness -1) are not handled,
 * as in the reference: the bitangent is always cross(tangent, normal).
 * Returns -2 for a null pointer, npix <= 0 or a view_stride other than 0 and 3. */
int utx_pbr_shading_normal(utx_ctx* ctx, const float* view_pos, int view_stride, const float* world_pos, const float* perturbed_nrm, const float* smooth_nrm,
                           const float* smooth_tng, const float* geom_nrm, long npix, float* out, utx_stream stream);

/* utx_pbr_shade with a tangent-space normal map.  As utx_pbr_shade, plus: v_tng [V][3] (per-vertex tangents, interpolated exactly as v_nrm is), f_nrm [F][3]
 * (utx_face_normals' output, indexed by the pixel's triangle: the geometric normal) and nm [Hn][Wn][3] fp32 in UV-raster orientation, fetched as kd is and
 * decoded as p = 2 * texel - 1 without normalisation.  The rule of utx_pbr_shading_normal with (interpolated position, p, interpolated normal, interpolated
 * tangent, f_nrm[triangle]) gives the normal that PBRModel.forward shades with; everything after that is utx_pbr_shade's.
 * Returns -2 for a null pointer (ks_or_null and out_rgba_or_null excepted), a non-positive size, or rast / out_rgba_or_null off a 16-byte boundary. */
int utx_pbr_shade_nm(utx_ctx* ctx, const float* rast, const int* tri, const float* v_pos, const float* v_nrm, const float* v_tng, const float* f_nrm, const float* v_uv,
                     const float* kd, int Hk, int Wk, const float* ks_or_null, int Hs, int Ws, const float* nm, int Hn, int Wn, const float* eye3_host,
                     const float* light_diffuse, int Nd, const float* light_specular, int Ns, const float* fg_lut, int R, float lambda_diffuse, float lambda_specular,
                     const float* bg3_host, long npix, void* out_u8, float* out_rgba_or_null, utx_stream stream);

/* Environment renderer: the per-pixel paths of NVDiffRendererScene (render/nvdiffrast/renderer_scene.py).  Cubemaps are [6][N][N][C], panoramas
 * [Hi][Wi][C], 1 <= C <= 4, fp32.  A cubemap is read by the cube lookup rule above (N even, N <= 8192), a panorama linearly with wrap addressing in both
 * axes (texel centres at +0.5, blended as t00 (1 - fx) + t01 fx: utx_texture_shade's fetch), a view image as grid_sample(bilinear, zero padding,
 * align_corners=False).  One thread per pixel / texel, every sum in a fixed order: results are identical from run to run.
 *
 * utx_scene_render (perspective_rendering, :288-317): c2ws [B][4][4], intrinsics [B][3][3] (intr_stride 9) or one [3][3] (intr_stride 0), normalised.
 * Pixel (x, y) of camera b: n = 2 ((x, y) + 0.5) / (W, H) - 1;  p = ((n.x + (2cx - 1)) / (2fx), ((2cy - 1) - n.y) / (2fy), -1) (the point at depth 1 under
 * intr_to_proj's matrix, its second row flipped);  d = normalize((R p + t) - t) with normalize(v) = v / max(|v|, 1e-12).  Each requested output is written,
 * a NULL output is skipped (at least one is required):
 *   rays_d [B][H][W][3] = d;   cubemap_attr [B][H][W][C] = the cube lookup at d;   uv [B][H][W][2] = (atan2(d.x, -d.z) / 2pi + 0.5, acos(clamp(d.y)) / pi);
 *   latlong_attr [B][H][W][C] = the panorama at uv (computed whether or not uv itself is requested).
 * Returns -2 for a null c2ws / intrinsics, a size <= 0, intr_stride not in {0, 9}, no output at all, cubemap_attr without a cubemap (or N odd, N > 8192),
 * latlong_attr without a panorama, C outside 1 .. 4 when a lookup is requested. */
int utx_scene_render(utx_ctx* ctx, const float* c2ws, const float* intrinsics, int intr_stride, int B, int H, int W, const float* cubemap_or_null, int N,
                     const float* latlong_or_null, int Hi, int Wi, int C, float* rays_d_or_null, float* cubemap_attr_or_null, float* uv_or_null,
                     float* latlong_attr_or_null, utx_stream stream);

/* cubemap_to_latlong (:148-172): texel (x, y) of out [Ht][Wt][C]: g = 2 ((x, y) + 0.5) / (Wt, Ht) - 1, psi = g.x pi, theta = g.y pi / 2 + pi / 2,
 * d = (sin theta sin psi, cos theta, -sin theta cos psi), angles and direction in fp64 and rounded once; out = the cube lookup at d.
 * Not the inverse of utx_latlong_to_cubemap (neither is it in the reference).  Returns -2 for a null pointer, a size <= 0, N odd or > 8192, C outside 1 .. 4. */
int utx_cubemap_to_latlong(utx_ctx* ctx, const float* cubemap, int N, int C, int Ht, int Wt, float* out, utx_stream stream);

/* perspective_inverse_rendering_torch (:373-430): M views images [M][H][W][C] baked into one panorama [Ht][Wt][C].  w2cs, projections: [M][4][4] row-major,
 * the two matrices the reference applies one after the other (inverse of c2w; intr_to_proj), each row evaluated as ((m0 x + m1 y) + m2 z) + m3 w.
 * Per texel, d as in utx_cubemap_to_latlong, and per view in index order: clip = projection (w2c (d, 1)) -- the direction taken as a POINT of the unit
 * sphere, so the camera's translation counts, as in the reference;  uv = clip.xy / clip.w;  alpha = (-1 <= uv <= 1 on both axes) and clip.w > 0;
 * sum += alpha * grid_sample(images[m], uv), count += alpha.  latlong_attr = clamp(sum / count, 0, 1), exactly 0 where no view sees the texel.
 * Outputs (NULL = skipped, at least one required): uv [M][Ht][Wt][2], uv_alpha [M][Ht][Wt][1] (0 or 1), latlong_attr [Ht][Wt][C].
 * Returns -2 for a null matrix pointer, M, Ht or Wt <= 0, no output at all, latlong_attr without images (or H, W <= 0, C outside 1 .. 4). */
int utx_scene_bake_latlong(utx_ctx* ctx, const float* w2cs, const float* projections, const float* images_or_null, int M, int H, int W, int C, int Ht, int Wt,
                           float* uv_or_null, float* uv_alpha_or_null, float* latlong_attr_or_null, utx_stream stream);

/* LBVH ray-mesh intersector (raytracing/__init__.py:12-83 RayTracing / rt_aprmis APRMISRayTracing; the build the
 * reference runs per mesh: raytracing/rt_aprmis/bvhhelpers.py:20-84).  verts/faces are borrowed and must stay alive while
 * the handle is used.
 * utx_bvh_build: the handle owns its node arrays (ONE hipMalloc inside build, released by utx_bvh_free); the tree depth is
 *   known on return (one stream synchronisation).
 * utx_bvh_build_ws (what NVDiffRendererInverse.infer uses): every array lives in the caller's `work` (256-byte aligned,
 *   >= utx_bvh_workspace_bytes(F); it must outlive the handle) -- nothing is allocated, freed or waited for on the path:
 *   the build is enqueued and returns; the first launch that needs the tree depth (utx_bvh_trace*, utx_backproject,
 *   utx_bvh_depth) waits for it, later ones do not.  utx_bvh_free releases the handle only. */
typedef struct utx_bvh utx_bvh;
int utx_bvh_build(utx_ctx* ctx, const float* verts, int V, const int* faces, int F, utx_bvh** out, utx_stream stream);
size_t utx_bvh_workspace_bytes(int F);
int utx_bvh_build_ws(utx_ctx* ctx, const float* verts, int V, const int* faces, int F, void* work, size_t work_bytes, utx_bvh** out, utx_stream stream);
void utx_bvh_free(utx_bvh* bvh);
/* device pointers to the node arrays (tests / diagnostics): info [2F-1][3], aabb [2F-1][6], sorted Morton
 * codes [F], sorted element ids [F]; returns F. */
int utx_bvh_arrays(utx_bvh* bvh, int** info, float** aabb, unsigned** codes_sorted, int** idx_sorted);
/* intersects_closest (rt_aprmis/__init__.py:40-86): tid [R] int32, -1 = miss. */
int utx_bvh_trace(utx_ctx* ctx, utx_bvh* bvh, const float* rays_o, const float* rays_d, long R, int* tid, utx_stream stream);
/* the same trace + the number of tree nodes the rays visited, ADDED to *visited (device counter; measurement of SURVEY 8d's
 * nodes-visited-per-ray, bench.py); longest root-to-leaf path of the tree (the stackless packed traversal is used up to 60, the
 * reference's 64-entry stack walk above: intersect_test2.slang:63-146). */
int utx_bvh_trace_count(utx_ctx* ctx, utx_bvh* bvh, const float* rays_o, const float* rays_d, long R, int* tid,
                        unsigned long long* visited, utx_stream stream);
int utx_bvh_depth(utx_bvh* bvh);

/* Face and vertex visibility of a camera batch: Mesh.get_visible_faces / get_visible_vertices (mesh/structure.py:801-857),
 * NVDiffRendererBase.get_visible_faces / get_visible_vertices (render/nvdiffrast/renderer_base.py:65-99) and erode_face
 * (geometry/triangle_topology/topology.py:12-25).  Masks are uint8 (0 / 1), [B][F] per face and [B][V] per vertex; B <= 65535.
 * utx_visible_faces_rays: ONE launch for all B views behind a memset of mask.  One ray per (view, face) aimed at the face's centroid
 *   ((v0 + v1) + v2) / 3: perspective != 0 from o = c2w[:3,3] along centroid - o, otherwise from centroid + 2 sqrt(3) c2w[:3,2] along -c2w[:3,2]
 *   (c2ws [B][4][4], row-major).  The ray marks the face it hits FIRST -- the smallest t among the hits with t >= 0, ties to the smallest face id, no
 *   backface culling: Embree's closest hit, not the last-hit-wins traversal of utx_bvh_trace -- which need not be the face it was aimed at; a face is
 *   visible iff some ray of the view lands on it (the reference's scatter).  verts / faces are the arrays the tree was built from (F must equal the
 *   tree's).  The packed (stackless) walk is used up to the depth rule of utx_bvh_trace, the stack walk beyond it or with UTX_VF_STACK_WALK; both
 *   visit the nodes in one order and give equal masks.  Rays are issued in the tree's sorted leaf order (a wave's rays are neighbours in space);
 *   UTX_VF_FACE_ORDER issues them in face order (same mask; for the node count).  visited (may be null): device counter the number of visited nodes is
 *   ADDED to.
 * utx_visible_faces_raster: the faces whose id + 1 appears in rast [B][H][W][4].w (ids outside [1, F] are ignored); memset + one launch.
 * utx_erode_faces: in place, `depth` rounds of: a face stays set iff none of its vertices belongs to an unset face.  Two launches per round (a vertex
 *   scatter, a face gather); vstamp [B][V] int32 is the caller's scratch (zeroed here).  depth <= 0 does nothing.
 * utx_visible_vertices: out [B][V]: a vertex is set iff it belongs to a set face; memset + one launch.
 * All stream-ordered.  Return -2 for a null operand, F <= 0, V <= 0, B <= 0 or > 65535, H or W <= 0, unknown flags, a tree of another F, and a tree deeper than 94
 * levels on the stack walk (its stack holds 96 entries; an LBVH of 30 Morton bits and 32 index bits is at most 62 deep). */
#define UTX_VF_STACK_WALK 1
#define UTX_VF_FACE_ORDER 2
int utx_visible_faces_rays(utx_ctx* ctx, utx_bvh* bvh, const float* verts, const int* faces, int F, const float* c2ws, int B, int perspective, int flags,
                           unsigned char* mask, unsigned long long* visited, utx_stream stream);
int utx_visible_faces_raster(utx_ctx* ctx, const float* rast, int B, int H, int W, int F, unsigned char* mask, utx_stream stream);
int utx_erode_faces(utx_ctx* ctx, unsigned char* mask, const int* faces, int B, int F, int V, int depth, int* vstamp, utx_stream stream);
int utx_visible_vertices(utx_ctx* ctx, const unsigned char* mask, const int* faces, int B, int F, int V, unsigned char* out, utx_stream stream);

/* Nearest surface point: what the reference takes from cuBVH.unsigned_distance(points, return_uvw=True) [3p] (geometry/sampling/spatial_sampling.py:36,90).
 * points [N][3] f32 -> dist [N] f32 (the distance itself, sqrtf(d2)), face [N] i32, uvw [N][3] f32, closest [N][3] f32; face, uvw, closest and visited may be null.
 * Per triangle: tri_closest(p, v0, v1, v2) -> (d2, u, v, w), the Voronoi-region form of Ericson, Real-Time Collision Detection, 5.1.5, in fp32 with fixed
 *   summation order (csrc/bvh_device.h; oracle/closest_point_ref.py repeats it bit for bit): (u, v, w) weigh (v0, v1, v2), closest = (u v0 + v v1) + w v2,
 *   d2 = |p - closest|^2 summed (x^2 + y^2) + z^2; every weight is >= 0; a quotient with a denominator not > 0 is 0 (a zero-length edge is its end point);
 *   a zero-area face (interior denominator va + vb + vc not > 0) gives the nearest point of its three edge segments AB, AC, BC, the first on a tie.
 * Per query: the face with the smallest d2, ties to the smallest face id -- independent of the order in which the triangles are met.  A subtree is skipped
 *   only if its box's squared distance sum(max(0, lo - p, p - hi)^2) exceeds best * 1.00001f, so a tying triangle is still tested while the two
 *   roundings differ by less than that relative margin: for a query within a few ulp * scale of the surface the computed d2 can fall to 0 and a tying face whose box
 *   does not hold p may be skipped -- d2 is unaffected, the face named is then the smallest id among the tying faces met.  A query with a non-finite
 *   coordinate gives face -1, dist +inf, zero uvw and closest.  Coordinates are assumed small enough that their squares and the products of two squares stay
 *   finite in fp32 (|x| below about 1e9).
 * One launch, one thread per query in the caller's order, on the packed tree without a stack (a greedy descent into the nearer child seeds `best`, then the
 *   escape-link walk of utx_visible_faces_rays): no workspace, no atomics but the optional counter, no host wait, any tree depth.
 * flags: UTX_CP_EXHAUSTIVE loops over all F triangles instead (same per-triangle function and tie rule: the test twin and the cost baseline);
 *   UTX_CP_NO_SEED walks without the greedy descent (same result; for the node count).  visited: device counter the number of visited nodes is ADDED to.
 * N == 0 returns 0 at once; -2 for a null tree, points or dist, N < 0, N >= 2^31, unknown flags. */
#define UTX_CP_EXHAUSTIVE 1
#define UTX_CP_NO_SEED 2
int utx_bvh_closest_point(utx_ctx* ctx, utx_bvh* bvh, const float* points, long N, float* dist, int* face, float* uvw, float* closest,
                          unsigned long long* visited, int flags, utx_stream stream);

/* Ray queries on the tree: RayTracing.intersects_closest of the reference (raytracing/__init__.py: hit, front, tri_idx, loc, uv) for arbitrary rays, and the
 * queries raytracing/check_visibility.py builds from it (self_rt, cross_rt, sphere_rt).  Each is ONE launch, no workspace, no host wait, no atomics but the
 * optional counter `visited` (device word the number of visited nodes is ADDED to; may be null).  Walks and depth rule of utx_visible_faces_rays: the packed
 * walk up to a depth of 60, the stack walk beyond it or with UTX_RC_STACK_WALK (equal results).  All fp32, stream-ordered; csrc/raycast.hip.
 * utx_bvh_intersect: rays_o, rays_d [R][3]; directions are NOT normalised, t is in units of |d|.  The hit with the smallest t >= 0 wins, both triangle sides
 *   count, ties in t go to the smallest face id, a zero direction component is replaced by 1e-30 in the box test -- the closest hit of utx_visible_faces_rays,
 *   so tid is what that function finds for the same ray, and none of utx_bvh_trace's quirks.  Outputs, each may be null: tid [R] i32 (-1: miss), t [R] (+inf: miss),
 *   loc [R][3] = o + t d (a rounded product, then a rounded sum), uv [R][2] = Moeller-Trumbore's (u, v) of the winner (u weighs v1, v weighs v2),
 *   front [R] u8 = 1 iff dot(d, (v1 - v0) x (v2 - v0)) < 0 (this library's rule: the reference's backends leave it unpinned), face_mask [F] u8: the byte of
 *   every hit face is set to 1 (not cleared here: the caller zeroes it, or accumulates).  A miss: loc = 0, uv = 0, front = 0.  A ray with d = (0, 0, 0) or a
 *   NaN in o or d is a miss (it may visit every node once; it never faults and always ends).
 * utx_bvh_occluded: segments from [R][3] -> to [R][3]; blocked [R] u8 = 1 iff some triangle is hit with 0 <= t < 1 along d = to - from (strict, no
 *   normalisation).  The walk leaves at the first such hit and enters no box beyond t = 1.  A zero-length segment is not blocked.
 * utx_points_enclosed: inner [N] u8 = 1 iff each of the n_rays (1 .. 1024) rays from points[i] has a hit with t >= 0 (any hit).  Ray j of point i has the
 *   direction sphere(i, j): Philox4x32-10, key (seed low word, seed high word), counter (i, j, attempt, stream_id); x1 = 2 u0 - 1, x2 = 2 u1 - 1 with
 *   u = (word >> 8) 2^-24 from words 0 and 1; while s = x1^2 + x2^2 >= 1 the next attempt (at most 64, then d = (0, 0, 1)); d = (2 x1 q, 2 x2 q, 1 - 2 s),
 *   q = sqrt(1 - s) correctly rounded (Marsaglia 1972) -- independent of the launch geometry, repeated bit for bit by numpy.  dirs_or_null [N][n_rays][3]: read
 *   instead of the generator.  min(64, next power of two >= n_rays) lanes serve a point and stop at the point's first completed miss;
 *   UTX_RC_NO_EARLY_EXIT walks every ray (same inner).  hits [N] i32 (may be null): the number of rays that hit, exact only with UTX_RC_NO_EARLY_EXIT.
 * utx_sphere_directions: out [n_points][n_rays][3] = sphere(i, j) of the same device function (n_points * n_rays < 2^31).
 * R == 0, N == 0 or an empty direction table return 0 at once.  -2 for a null tree or a null required operand (rays, segments, blocked, points, inner, out),
 *   a negative count, a count >= 2^31, n_rays outside 1 .. 1024, unknown flags, and a tree deeper than 94 levels on the stack walk. */
#define UTX_RC_STACK_WALK 1
#define UTX_RC_NO_EARLY_EXIT 2
int utx_bvh_intersect(utx_ctx* ctx, utx_bvh* bvh, const float* rays_o, const float* rays_d, long R, int* tid, float* t, float* loc, float* uv, unsigned char* front,
                      unsigned char* face_mask, unsigned long long* visited, int flags, utx_stream stream);
int utx_bvh_occluded(utx_ctx* ctx, utx_bvh* bvh, const float* from, const float* to, long R, unsigned char* blocked, unsigned long long* visited, int flags,
                     utx_stream stream);
int utx_points_enclosed(utx_ctx* ctx, utx_bvh* bvh, const float* points, long N, int n_rays, unsigned long long seed, unsigned stream_id, const float* dirs_or_null,
                        unsigned char* inner, int* hits, unsigned long long* visited, int flags, utx_stream stream);
int utx_sphere_directions(utx_ctx* ctx, long n_points, long n_rays, unsigned long long seed, unsigned stream_id, float* out, utx_stream stream);

/* Vertex-colour bake from views: project_vertex_color / remapping_vertex_color / inpainting_vertex_color of the reference
 * (texture/reprojection/mesh_remapping.py:508-627, :273-350).  All fp32, stream-ordered, row-major.
 * utx_view_weight_maps: cos_ray_normal [B][H][W] (utx_screen_gbuffer) -> out [B][H][W][2] = (cos term, edge alpha).  cos term: clamp(cos, -1, 0), or with
 *   camera_normal [B][H][W][3] given (orthographic cameras; else null) clamp(camera_normal.z, 0, 1).  Edge alpha: a = ((acos(clamp(cos, -1, 0)) - pi/2) /
 *   (pi/2)).clamp(0, 1); torch.gradient's stencil along y and x (central difference over 2 inside, one-sided at the borders, hence H, W >= 2);
 *   sqrt(dy^2 + dx^2) > float32(radians(10) / (pi/2)), strictly; then the (2 r + 1)^2 maximum with zeros outside the image.  One launch for r = 0; for r > 0
 *   a second launch dilates out of tmp (B * H * W bytes, the caller's; may be null for r = 0).  arccos_out (may be null): `a` [B][H][W].
 * utx_vertex_project: one thread per vertex, the views b = 0 .. B-1 in index order.  For a view with visible [b][v] != 0 (uint8 [B][V]): h = xform[b] (x, y, z, 1),
 *   clip = proj[b] h (both [B][4][4], products summed in index order), ndc = clip.xy / clip.w.  Only with both ndc strictly inside (-1, 1): rgba = images
 *   [B][4][Hi][Wi] sampled as grid_sample(bilinear, padding_mode='reflection', align_corners=False) -- unnormalise, reflect about [-0.5, size - 0.5], then clip
 *   to [0, size - 1] --, (cos, alpha) = wmap [B][H][W][2] sampled as grid_sample(bilinear, zeros, align_corners=False), a = use_alpha ? rgba.a : 1,
 *   c = rgb a + v_rgb (1 - a), w = weights[b] (cos^2)^2 (1 - alpha); otherwise c = v_rgb, w = 0.  v_rgb_acc += w c, v_weight_acc += w.
 *   Outputs v_rgb_acc [V][3], v_weight_acc [V].
 * utx_vertex_project_blend: the same launch followed, per vertex, by remapping_vertex_color's epilogue into blended [V][3]: acc / w where w > overlay_confidence;
 *   blending UTX_VB_BLEND_SOFT: (v_rgb (blending_confidence - w) + acc) / blending_confidence where w <= blending_confidence, UTX_VB_BLEND_HARD: v_rgb there,
 *   UTX_VB_BLEND_NONE: nothing; inpaint_mask [V] uint8 = (w <= inpainting_confidence).  v_rgb_acc may be null here.
 * utx_vertex_inpaint_step: one Jacobi step on the CSR adjacency rowptr [V + 1] / col (neighbours ascending): for each of the n vertices i of idx, with
 *   deg = rowptr[i + 1] - rowptr[i], S = sum over the neighbours j with mask_in[j] of rgb_in[j] (CSR order) and M their number: if deg M > 0,
 *   rgb_out[i] = (deg S) / (deg M) and mask_out[i] = 1, else rgb_out[i] = rgb_in[i] and mask_out[i] = 0.  Rows outside idx are not written: the two buffer pairs
 *   must agree on them.  *counter (device int32, zeroed here) receives the number of vertices of idx with mask_out = 1.  One launch; no block waits for another.
 * A zero-size problem (B H W = 0, V = 0, n = 0) returns 0 without a launch.  -2: a negative size, H or W of 1, r < 0, a null or misaligned operand (wmap / out:
 * 8 bytes, every other array: its element), an unknown blending, rgb_in == rgb_out or mask_in == mask_out; outputs untouched. */
#define UTX_VB_BLEND_NONE 0
#define UTX_VB_BLEND_SOFT 1
#define UTX_VB_BLEND_HARD 2
int utx_view_weight_maps(utx_ctx* ctx, const float* cos_ray_normal, const float* camera_normal, int B, int H, int W, int r, void* tmp, float* out,
                         float* arccos_out, utx_stream stream);
int utx_vertex_project(utx_ctx* ctx, const float* v_pos, int V, const unsigned char* visible, int B, const float* xform, const float* proj, const float* images,
                       int Hi, int Wi, const float* wmap, int H, int W, const float* v_rgb, const float* weights, int use_alpha, float* v_rgb_acc,
                       float* v_weight_acc, utx_stream stream);
int utx_vertex_project_blend(utx_ctx* ctx, const float* v_pos, int V, const unsigned char* visible, int B, const float* xform, const float* proj,
                             const float* images, int Hi, int Wi, const float* wmap, int H, int W, const float* v_rgb, const float* weights, int use_alpha,
                             float* v_rgb_acc, float* v_weight_acc, float overlay_confidence, int blending, float blending_confidence,
                             float inpainting_confidence, float* blended, unsigned char* inpaint_mask, utx_stream stream);
int utx_vertex_inpaint_step(utx_ctx* ctx, const int* rowptr, const int* col, const int* idx, int n, const float* rgb_in, const unsigned char* mask_in,
                            float* rgb_out, unsigned char* mask_out, int* counter, utx_stream stream);

/* Blended multi-view UV texture bake: project_uv_texture / remapping_uv_texture of the reference (texture/reprojection/mesh_remapping.py:430-505, :145-270) and
 * uv_dilation (texture/reprojection/uv_dilation.py:33-50, :80-92).  All fp32, stream-ordered, row-major, no atomics on colour, no workspace.
 * utx_uv_bake: one thread per texel of the atlas raster rast2d [Th][Tw][4], the views b = 0 .. B-1 in index order.  Per view: vis, uv, the coverage lookup cov and
 *   uv_alpha = vis && cov exactly as utx_uv_project defines them (faces [F][3], face_mask uint8 [B][F], v_ndc [B][V][2], rast_view [B][R][R][4] = the views rasterised
 *   at R, only .w is read); rgba = images [B][4][R][R] (planar) and (c, e) = wmap [B][R][R][2] (utx_view_weight_maps) sampled at uv as grid_sample(bilinear, zeros,
 *   align_corners=False), or texel [0][0] of the view's six channels where cov fails; a = use_alpha ? uv_alpha : 1; w = weights[b] ((c c) (c c)) a (1 - e);
 *   col = (a rgba + (1 - a) map_Kd) w with map_Kd [Th][Tw][4].  acc [Th][Tw][4] = sum of col, wacc [Th][Tw] = sum of w.
 *   epilogue != 0: the same launch also writes blended [Th][Tw][4] -- acc / wacc where wacc > overlay_confidence; then, where wacc <= blending_confidence,
 *   UTX_VB_BLEND_SOFT: (map_Kd (blending_confidence - wacc) + acc) / blending_confidence, UTX_VB_BLEND_HARD: map_Kd, UTX_VB_BLEND_NONE: nothing -- and
 *   inpaint_mask [Th][Tw] uint8 = (wacc <= inpainting_confidence && rast2d.w > 0); acc may be null then.  epilogue == 0: blended and inpaint_mask are not used.
 * utx_uv_dilation_step, mode UTX_UVD_STEP: one _uv_dilation_v2 step on col_in [H][W][C] (1 <= C <= 16) and mask_in uint8 [H][W] (1 = valid) into col_out / mask_out.
 *   A tap reads as colour * mask (the premultiplication of uv_dilation.py:41, made on every read); taps outside the image count as zero and the divisor is 9
 *   everywhere.  S = the nine colour taps summed row by row, M = the nine mask taps.  Where M / 9 != mask: col_out = (S / 9) / (M / 9) (an invalid texel with a
 *   valid neighbour, and a valid texel with an invalid or out-of-image neighbour, which is averaged again); elsewhere col_out = col_in, so an invalid texel out of
 *   reach keeps its own colour.  mask_out = M > 0.  *counter (device int32, zeroed here) receives the number of texels with mask_out = 0.
 *   mode UTX_UVD_CLAMP: col_out = clamp(col_in, 0, 1) over the whole map (uv_dilation's last line); mask_in, mask_out and counter are not used and may be null.
 * A zero-size problem (Th Tw = 0, H W = 0) returns 0 without a launch.  -2: a negative size; B, R, F or V <= 0; C outside 1..16; a null or misaligned operand (rast2d,
 * map_Kd, acc, blended: 16 bytes, wmap: 8, every other array: its element); an unknown blending or mode; col_in == col_out or mask_in == mask_out; outputs untouched. */
#define UTX_UVD_STEP 0
#define UTX_UVD_CLAMP 1
int utx_uv_bake(utx_ctx* ctx, const float* rast2d, const int* faces, int F, const unsigned char* face_mask, const float* v_ndc, int V, int B, int Th, int Tw,
                const float* images, const float* wmap, const float* rast_view, int R, const float* map_Kd, const float* weights, int use_alpha, float* acc,
                float* wacc, int epilogue, float overlay_confidence, int blending, float blending_confidence, float inpainting_confidence, float* blended,
                unsigned char* inpaint_mask, utx_stream stream);
int utx_uv_dilation_step(utx_ctx* ctx, const float* col_in, const unsigned char* mask_in, int H, int W, int C, int mode, float* col_out, unsigned char* mask_out,
                         int* counter, utx_stream stream);

/* Scattered-sample UV bake: NVDiffRendererBase.global_inverse_rendering of the reference (render/nvdiffrast/renderer_base.py:562-743), the two stages that are
 * not already here.  All fp32, stream-ordered, row-major, no workspace.
 * utx_view_samples: one thread per pixel of rast [B][H][W][4] (one utx_rasterize per view).  For a covered pixel on triangle (i0, i1, i2) of faces [F][3] with the
 *   raster's weights: tex_to_pos [B][H][W][2] = the interpolation of v_uv [V][2] (vertex UVs in [-1, 1]); tex_to_pos_cam [B][H][W][6] = the interpolation of
 *   (v_pos_cam[b][i] / max(|v_pos_cam[b][i]|, 1e-12), v_nrm_cam[b][i]) with v_pos_cam / v_nrm_cam [B][V][3] (utx_transform_points with M = w2c; utx_camera_normals,
 *   which normalises): the position direction is normalised per VERTEX, before the interpolation, and nothing is normalised after it.  An uncovered pixel holds zeros.
 *   mask [B][H][W] uint8 = covered && (exclude_boundary: the pixels above, below, left and right are covered, the image wrapping round at its edges as torch.roll
 *   does) && (use_normal_threshold: tex_to_pos_cam[5] > cos_normal) && (use_ray_threshold: dot(tex_to_pos_cam[0:3], tex_to_pos_cam[3:6]) > cos_ray) &&
 *   (image_mask [B][H][W] uint8, optional: non-zero).
 * utx_knn_inpaint_step: one Jacobi sweep over M points (the covered texels) on their neighbour lists idx / d2 [M][k] (utx_knn with the set as source and query:
 *   ascending squared distance, so the point itself leads its list), nrm [M][3], col_in [M][C], pending_in [M] uint8 (non-zero: no colour yet).  A pending point
 *   whose list holds fewer than k - 1 pending entries takes col_out = sum_j (m_j w_j) col_in[j] / sum_j (m_j w_j) in list order, m_j = 0 for a pending neighbour
 *   and 1 otherwise, w_j = (r_j / max(sum_j |r_j|, 1e-12)) cos(nrm_j, nrm_i), r_j = 1 / sqrt(d2_j) with +inf replaced by FLT_MAX and NaN by 0
 *   (torch.nan_to_num), cos(a, b) = a.b / max(|a| |b|, 1e-8), and pending_out = 0; every other point copies its colour and flag.  Nothing guards the arithmetic:
 *   two zero distances in one list overflow the sum, the weights vanish and the point becomes NaN and known.  A list entry outside [0, M) is not read and weighs
 *   0.  *counter (device int32, zeroed here) receives the number of points filled.  One launch; no block waits for another.
 * A zero-size problem (B H W = 0, M = 0) returns 0 without a launch.  -2: a negative size; F or V <= 0; M > 2^31 - 1; k outside 1..32; C outside 1..16; a null or
 * misaligned operand (rast: 16 bytes, tex_to_pos: 8, every other array: its element); col_in == col_out or pending_in == pending_out; outputs untouched. */
int utx_view_samples(utx_ctx* ctx, const float* rast, const int* faces, int F, const float* v_uv, const float* v_pos_cam, const float* v_nrm_cam, int V, int B,
                     int H, int W, int exclude_boundary, int use_normal_threshold, float cos_normal, int use_ray_threshold, float cos_ray,
                     const unsigned char* image_mask, float* tex_to_pos, float* tex_to_pos_cam, unsigned char* mask, utx_stream stream);
int utx_knn_inpaint_step(utx_ctx* ctx, const int* idx, const float* d2, const float* nrm, const float* col_in, const unsigned char* pending_in, long M, int k, int C,
                         float* col_out, unsigned char* pending_out, int* counter, utx_stream stream);

/* Poisson image fusion: image_fusion of the reference (image/image_fusion.py:12-58), which hands uint8 images to OpenCV's seamlessClone(NORMAL_CLONE) [3p] on the
 * host.  The rule is this library's (DESIGN 8 "Poisson image fusion"); everything runs on the device in fp32, stream-ordered, row-major, bit-reproducible.
 * utx_mask_morph: mask_in / mask_out / tmp uint8 [H][W].  n > 0: grey erosion (minimum) over an n x n box, n < 0: grey dilation (maximum) over |n| x |n|; the box
 *   covers the offsets -(|n| / 2) .. |n| - 1 - |n| / 2 in both axes and taps outside the image are left out.  Two separable passes through tmp.  1 <= |n| <= 31.
 * utx_mask_bbox: rect (DEVICE int32 [4]) = (x1, y1, w, h), the tight bounding rectangle of mask > 0; four zeros for an empty mask.  The caller reads the 16 bytes
 *   back: the rectangle sizes the solver's levels on the host.
 * utx_image_fusion: src, dst, out uint8 [H][W][3], mask uint8 [H][W], the rectangle (x1, y1, w, h) inside the image (HOST integers).  w < 3 or h < 3: out = dst.
 *   Otherwise, inside the rectangle: s = src where mask > 0, else 0; m = mask / 255 eroded three times by a 3 x 3 box (pixels outside the rectangle left out);
 *   v = m grad(s) + (1 - m) grad(dst) with forward differences and m at (x, y); f = the backward divergence of v on the (w - 2) x (h - 2) interior; I has the
 *   5-point Laplacian f there and equals dst on the rectangle's one-pixel ring.  Solved for u = I - dst (zero boundary values, right-hand side div(m grad(s - dst)))
 *   by `cycles` multigrid V-cycles (0: utx_image_fusion_cycles(w, h), fixed per size; no data-dependent stop, no read-back); every cycle iterates on the residual of
 *   that exact system.  out = clamp(round_half_even(dst + u), 0, 255) on the interior and dst elsewhere; out_f float32 [H][W][3] (optional) = dst + u unrounded
 *   and unclamped on the interior, dst elsewhere.  work: utx_image_fusion_workspace_bytes(w, h) bytes (0 when there is no interior), 4-byte aligned.
 * -2, outputs untouched: H, W <= 0; n = 0 or |n| > 31; a null operand (out_f excepted); tmp equal to mask_in or mask_out; a rectangle with a negative member or
 * reaching outside the image; cycles outside 0 .. 64; with an interior, a null, misaligned or short workspace. */
int utx_mask_morph(utx_ctx* ctx, const unsigned char* mask_in, int H, int W, int n, unsigned char* tmp, unsigned char* mask_out, utx_stream stream);
int utx_mask_bbox(utx_ctx* ctx, const unsigned char* mask, int H, int W, int* rect, utx_stream stream);
int utx_image_fusion_cycles(int w, int h);
long utx_image_fusion_workspace_bytes(int w, int h);
int utx_image_fusion(utx_ctx* ctx, const unsigned char* src, const unsigned char* dst, const unsigned char* mask, int H, int W, int x1, int y1, int w, int h,
                     int cycles, unsigned char* out, float* out_f, void* work, long work_bytes, utx_stream stream);

/* Telea inpainting: what the reference's uv_dilation_cv / remapping_uv_texture(use_cv_inpainting=True) hand to OpenCV's cv2.inpaint(INPAINT_TELEA) [3p] on the host.
 * The rule is this library's (DESIGN 8 "Telea inpainting": Telea's 2004 estimate on an exact distance map, not OpenCV's heap order, which nothing here can pin);
 * everything runs on the device in fp32, stream-ordered, row-major, bit-reproducible.  H, W in 1 .. UTX_INPAINT_SIDE_MAX.
 * utx_inpaint_distance: hole uint8 [H][W] (non-zero: fill) -> d2 int32 [H][W]: the exact squared Euclidean distance of a hole pixel to the nearest in-image
 *   pixel outside the hole, 0 outside the hole, UTX_INPAINT_NONE everywhere when the whole image is a hole.  tmp: int32 [H][W] (the column scan).
 * utx_inpaint_telea_step: one sweep on col_in float [H][W][C] (1 <= C <= 4), done_in uint8 [H][W] (1: the pixel has its value; every pixel outside the hole) and
 *   d2 into col_out / done_out.  With T = sqrt(float(d2)) and eps = radius (1 .. UTX_INPAINT_RADIUS_MAX): a hole pixel p that is not done computes itself once
 *   every pixel of its read set -- the disc |q - p|^2 <= eps^2 and the 4-neighbours of the disc's pixels -- with d2 < d2(p) is done.  Per channel, q row-major
 *   over the (2 eps + 1)^2 window, in the image, inside the disc, with d2(q) < d2(p) (strict, on integers), r = p - q:
 *     w = ((1 / (|r|^2 |r|)) (1 / (1 + |T(q) - T(p)|))) max(|r . gT(p)|, 1e-6);  v = sum w (I(q) + gI(q) . r) / sum w
 *   gT: central difference of T where both neighbours are in the image, one-sided at the image border, 0 on an axis of length 1.  gI(q) per axis over the
 *   neighbours n of q in the image with d2(n) < d2(p): central with both, one-sided with one, 0 with none.  Every other hole pixel copies its colour and flag;
 *   pixels OUTSIDE the hole are not written: col_out / done_out must already hold col_in / done_in there (the caller initialises both buffers alike).  A pixel
 *   with d2 = UTX_INPAINT_NONE is never computed.  *counter (device int32) is INCREASED by the number of pixels computed in this sweep; the caller zeroes it,
 *   so it may be read back once every few sweeps.  One launch; no block waits for another; no workspace.
 * utx_inpaint_finish: out uint8 [H][W][C] = round_half_even(min(max(col, 0), 255)); out_f float [H][W][C] (optional) = col, unclamped and unrounded.
 * -2, outputs untouched: a null operand (out_f excepted) or one not aligned to its element; H or W outside 1 .. UTX_INPAINT_SIDE_MAX; C outside 1 .. 4; radius
 * outside 1 .. UTX_INPAINT_RADIUS_MAX (a caller's radius <= 0, OpenCV's clamp to 1, is normalised above the C ABI); tmp == d2; col_in == col_out or
 * done_in == done_out; col == out_f. */
#define UTX_INPAINT_RADIUS_MAX 8
#define UTX_INPAINT_SIDE_MAX 16384
#define UTX_INPAINT_NONE 2147483647
int utx_inpaint_distance(utx_ctx* ctx, const unsigned char* hole, int H, int W, int* tmp, int* d2, utx_stream stream);
int utx_inpaint_telea_step(utx_ctx* ctx, const float* col_in, const unsigned char* done_in, const int* d2, int H, int W, int C, int radius, float* col_out,
                           unsigned char* done_out, int* counter, utx_stream stream);
int utx_inpaint_finish(utx_ctx* ctx, const float* col, int H, int W, int C, unsigned char* out, float* out_f, utx_stream stream);

/* Sliced optimal-transport colour transfer: CTSOT of the reference (image/color_transfer_ot.py), which loops over numpy argsorts on the host and regularises with
 * OpenCV's cv2.bilateralFilter [3p].  DESIGN 8 "Colour transfer".  All fp32, stream-ordered, row-major, bit-reproducible; no read-back, no host synchronisation.
 * utx_color_transfer_ot: src, dst, out [N][C] (1 <= C <= 4, 1 <= N < UTX_COLOR_TRANSFER_N_MAX), dirs [steps * batch_size][C] (DEVICE; unit directions, one per
 *   step and batch in that order).  cur = src; per step, for each batch b in order with d = its direction: p(x) = ((x0 d0 + x1 d1) + x2 d2) + x3 d3, each product
 *   and sum rounded to float32; the projections of cur and of dst are sorted by the total order of their bit patterns (-0 before +0; equal source projections
 *   keep ascending pixel order: a stable radix sort); advect[i] = advect[i] + (pt_sorted[r] - ps_sorted[r]) * d for the pixel i of source rank r.  After the
 *   last batch cur = cur + advect / float(batch_size), advect = 0.  out = cur after the last step; steps = 0: out = src.  This is the reference's loop bit for
 *   bit wherever no two projections of a batch are equal (tests/golden/g26_color_transfer_ot.npz).  Non-finite values are not looked for.
 *   work: utx_color_transfer_ot_workspace_bytes(N, C) bytes (0 for arguments the call would refuse); not read when steps = 0.
 * utx_bilateral_filter: img, out [H][W][C], C 1 or 3.  The rule is this library's on OpenCV's documented parameters with d = 0: the circular support
 *   dx^2 + dy^2 <= radius^2 (the caller's max(1, rint(1.5 sigmaSpace)), 1 .. UTX_BILATERAL_RADIUS_MAX), space_weights (DEVICE, [radius + 1][radius + 1],
 *   indexed [|dy|][|dx|]: the caller's exp(-(dx^2 + dy^2) / (2 sigmaSpace^2))), colour weight expf((sum_c |v_c(q) - v_c(p)|)^2 * color_coef) with
 *   color_coef = -1 / (2 sigmaColor^2) <= 0, reflect-101 borders applied repeatedly (an axis of length 1 maps to index 0).  Taps row-major over the window, one
 *   running sum per channel and one of the weights w = space * colour: out = sum(w v) / sum(w).  One launch, a 16 x 16 tile with its halo in LDS:
 *   utx_bilateral_lds_bytes(radius, C) bytes, which UTX_BILATERAL_RADIUS_MAX keeps within the 65536 a launch gets without asking for more.
 * -2, outputs untouched: a null or misaligned operand (dirs and work only with steps > 0); out equal to an input; N, C, steps < 0, batch_size < 1, H, W
 *   (1 .. UTX_BILATERAL_SIDE_MAX, H W < UTX_COLOR_TRANSFER_N_MAX), radius or a positive or NaN color_coef outside the above; a short workspace. */
#define UTX_COLOR_TRANSFER_N_MAX 1073741824L
#define UTX_BILATERAL_RADIUS_MAX 27
#define UTX_BILATERAL_SIDE_MAX 32768
long utx_color_transfer_ot_workspace_bytes(long N, int C);
int utx_color_transfer_ot(utx_ctx* ctx, const float* src, const float* dst, const float* dirs, long N, int C, int steps, int batch_size, float* out, void* work,
                          long work_bytes, utx_stream stream);
int utx_bilateral_lds_bytes(int radius, int C);
int utx_bilateral_filter(utx_ctx* ctx, const float* img, int H, int W, int C, int radius, const float* space_weights, float color_coef, float* out,
                         utx_stream stream);

/* Silhouette antialiasing of screen-space buffers: the forward pass of what the reference calls dr.antialias on alpha and on every buffer of simple_rendering
 * (render/nvdiffrast/renderer_base.py:143-336).  DESIGN 8 "Silhouette antialiasing".  The rule is this library's, after Laine et al. 2020 section 3.5, and is
 * NOT pinned against nvdiffrast's samples [3p]; csrc/antialias.hip's header states it with its exact float32 operation order.  All fp32, stream-ordered,
 * row-major, bit-reproducible; no atomics, no workspace, no read-back.
 * utx_antialias_analyze: rast [B][H][W][4] (utx_rasterize's records (u, v, z/w, id + 1), one raster per view), pos the clip-space vertices the rasters were made
 *   from ([V][4] shared by the views with pos_view_stride = 0, [B][V][4] with pos_view_stride = 4 V), tri [F][3], opp [F][3] (the vertex of the face across edge
 *   e = (v_e, v_e+1) that is not on the edge, -1 on a border) -> weights [B][H][W][4] = (left, right, up, down): the share of the difference to that neighbour
 *   that the pixel takes, in [0, 0.5]; 0 where the pair of pixels shows one triangle, no silhouette edge of the nearer triangle crosses the segment between the
 *   two centres, the crossing is nearer to the other pixel, or the neighbour lies outside the view.  Indices of tri and opp outside [0, V), ids outside [0, F)
 *   and vertices with a non-finite x, y, w or w <= 0 are tolerated: the pair contributes nothing, or the edge counts as a silhouette (opp).
 * utx_antialias_apply: color, out [B][H][W][C], any C >= 1:  out = (((color + k_left) + k_right) + k_up) + k_down per channel, k_n = w_n (color[n] - color) where
 *   w_n != 0 and +0 elsewhere, in this order.  One set of weights serves every buffer of the rasterisation.
 * -2, outputs untouched: a null pointer; F, V, B, H, W or C < 1; a pos_view_stride other than 0 and 4 V; rast, weights or pos off a 16-byte boundary, any other
 *   operand off a 4-byte one; weights equal to rast; out equal to color or to weights. */
int utx_antialias_analyze(utx_ctx* ctx, const float* rast, const float* pos, long pos_view_stride, const int* tri, const int* opp, int F, int V, int B, int H, int W,
                          float* weights, utx_stream stream);
int utx_antialias_apply(utx_ctx* ctx, const float* color, const float* weights, int B, int H, int W, int C, float* out, utx_stream stream);

/* fused per-(view, texel) gather + visibility of uv_to_pcd (renderer_inverse.py:277-298,316-325) */
typedef struct utx_backproject_desc {
    const void* rast2d;                 /* [T][4] f32 UV-space raster */
    const void* verts; const void* faces; const void* fnormal;   /* [V][3] f32, [F][3] i32, [F][3] f32 */
    const void* vndc;                   /* [n_views][V][2] f32 */
    const void* dirs;                   /* [n_views][3] f32 = -c2w[:, :3, 2] (orthographic) */
    const void* images;                 /* [n_views][H][W][4] f32 (rgb + alpha) */
    void* color; void* rayvis; void* alphaok;   /* [n_views][T][3] f32, [n_views][T] u8, [n_views][T] u8 */
    int T_h, T_w, V, n_views, H, W;
    int view_begin, view_count;         /* views handled by this launch (per-GPU view sharding) */
    float cos_thresh, two_sqrt3;
} utx_backproject_desc;
int utx_backproject(utx_ctx* ctx, const utx_backproject_desc* d, utx_bvh* bvh, utx_stream stream);
/* the same with perspective rays (uv_to_pcd(perspective=True), renderer_inverse.py:279-281): every ray of view v starts at the camera
 * centre eyes[v] and points at the texel's surface point, d = (pos - eye) / max(|pos - eye|, 1e-12).  eyes [n_views][3] f32 = c2w[:, :3, 3];
 * d->dirs and d->two_sqrt3 are not read.  Colour, alpha and the facing threshold as in utx_backproject. */
int utx_backproject_persp(utx_ctx* ctx, const utx_backproject_desc* d, const float* eyes, utx_bvh* bvh, utx_stream stream);
/* the same with a choice of view sampling (uv_to_pcd(grid_interpolate_mode=...), renderer_inverse.py:290-305).  eyes NULL: orthographic rays along d->dirs
 * (as utx_backproject), else perspective rays from eyes [n_views][3] (as utx_backproject_persp).  sample_mode 0: grid_sample, bilinear, zero padding
 * ('torch'; the same kernels as the two entry points above); 1: nvdiffrast dr.texture(ndc * 0.5 + 0.5, filter_mode='linear') with its default wrap
 * boundary ('nvdiff'); a non-finite coordinate samples zero. */
int utx_backproject_sampled(utx_ctx* ctx, const utx_backproject_desc* d, const float* eyes, int sample_mode, utx_bvh* bvh, utx_stream stream);

/* visibility hole filling k=3,5 + AND coverage + AND alpha>0.999 (renderer_inverse.py:326-343).
 * rayvis/alphaok/vis_out/tmp: [n_views][H][W] u8. */
int utx_dilate_visibility(utx_ctx* ctx, const void* rayvis, const void* alphaok, const float* rast2d, int n_views,
                          int H, int W, void* tmp, void* vis_out, utx_stream stream);

/* first-come-wins priority composite (renderer_inverse.py:595-602).  order: HOST array of view ids.
 * colors [n][T][3] f32, vis [n][T] u8 -> atlas [T][3] f32, winner [T] int8 (-1 = unseen). */
int utx_composite(utx_ctx* ctx, const float* colors, const void* vis, const int* order_host, int n_order, long T,
                  float* atlas, void* winner, utx_stream stream);

/* seam mask (renderer_inverse.py:602-604): winner [H][W] int8 -> seam [H][W] u8; tmp [H][W] u8. */
int utx_seam_mask(utx_ctx* ctx, const void* winner, const float* rast2d, int H, int W, void* tmp, void* seam, utx_stream stream);
/* the same at other window sizes (bake_mv_to_uv_reproject_blur(kernel_size_boundary=k_boundary, kernel_size_boundary_blur=k_boundary_blur)):
 * boundary radius k_boundary / 2, dilation radius k_boundary_blur / 2, coverage erosion radius k_boundary_blur / 2 + 2; both radii <= 15.
 * tmp: 4 * H * W bytes. */
int utx_seam_mask_sized(utx_ctx* ctx, const void* winner, const float* rast2d, int H, int W, int k_boundary, int k_boundary_blur, void* tmp, void* seam,
                        utx_stream stream);

/* exact 3-D nearest-seen-texel fill of unseen covered texels, in place on atlas (renderer_inverse.py:606-615).
 * pos [T][3] f32; nn_index [T] int32 (optional): chosen source texel or -1. */
long utx_nn_fill_workspace_bytes(long T);
int utx_nn_fill(utx_ctx* ctx, const float* pos, const void* winner, const float* rast2d, long T, float* atlas,
                int* nn_index, void* work, long work_bytes, utx_stream stream);

/* view-space visibility with the gradient filter (mv_to_pcd, filt_gradient_points=True; renderer_inverse.py:189-209).
 * attr6 [n][H][W][6] f32 interpolated (position, vertex normal), rast [n][H][W][4], fnormal [F][3], dirs [n][3] ray directions.
 * tmp: 2*n*H*W bytes.  vis [n][H][W] u8, alpha [n][H][W] f32 (optional).  radius = 15 (the reference's 31-wide pool, along W). */
int utx_view_visibility(utx_ctx* ctx, const float* attr6, const float* rast, const float* fnormal, const float* dirs, int n, int H, int W,
                        float grad_thr, float cos_thr, int radius, void* tmp, void* vis, float* alpha, utx_stream stream);
/* the same with perspective rays (mv_to_pcd(perspective=True), renderer_inverse.py:187-190): the facing test of pixel p of view v uses
 * d = (attr6[p][0:3] - eyes[v]) / max(|attr6[p][0:3] - eyes[v]|, 1e-12).  eyes [n][3] f32 = c2w[:, :3, 3]. */
int utx_view_visibility_persp(utx_ctx* ctx, const float* attr6, const float* rast, const float* fnormal, const float* eyes, int n, int H, int W,
                              float grad_thr, float cos_thr, int radius, void* tmp, void* vis, float* alpha, utx_stream stream);

/* exact k-NN gather in 3-D (bake_mv_to_uv_kdtree, renderer_inverse.py:367-433; search = torch_kdtree [3p], pcd/knn/__init__.py:103-113).
 * Sources and queries are dense arrays with optional byte masks (view pixels / atlas texels); k <= 32.
 * mode 0: out_attr = mean of the k neighbours' attributes; mode 1: MVPaint weighting (needs normals).
 * out_idx / out_d2 ([M][k], optional): neighbour ids (ascending squared distance, ties -> lower id), -1 / inf when fewer exist. */
typedef struct utx_knn_desc {
    const float* src_pos; const float* src_attr; const float* src_nrm; const unsigned char* src_mask; long N;
    const float* dst_pos; const float* dst_nrm; const unsigned char* dst_mask; long M;
    int k, C, mode;
    float* out_attr; int* out_idx; float* out_d2;
} utx_knn_desc;
long utx_knn_workspace_bytes(long N);
int utx_knn(utx_ctx* ctx, const utx_knn_desc* d, void* work, long work_bytes, utx_stream stream);

/* ---- geometry sampling for the field stage (pipeline.py:363-407 sampling_on_mesh; TextureTools/texturetools/geometry/sampling/) ---- */

/* exact farthest-point sampling (replaces fpsample.bucket_fps_kdline_sampling [3p], pipeline.py:390,401, and the thinning of the atlas texels,
 * pipeline.py:507-514).  pos [N][3] f32 (16-byte aligned), mask [N] u8 (optional) -> out_idx [M] i32, out_d2 [M] f32 (optional): the pick's squared
 * distance to the set chosen before it, +inf for the first pick.  d2 = (dx*dx + dy*dy) + dz*dz in float32.  A point that is masked out or has a
 * non-finite coordinate is never a candidate; each pick is the candidate farthest from the chosen set, ties -> lower index, and leaves the candidate
 * set (coincident points are picked later with d2 = 0, no index twice); when the candidates run out the rest of out_idx and out_d2 is -1.
 * start >= 0: the first pick (a start that is no candidate counts as -1); start = -1: the lowest candidate index.
 * 0 < M, 0 < N < 2^31, -1 <= start < N, else -2.  One kernel launch per pick on `stream`, M + 1 launches, no synchronisation; work: utx_fps_workspace_bytes(N)
 * bytes, 16-byte aligned, owned by the call until the stream has run it. */
long utx_fps_workspace_bytes(long N);
int utx_fps(utx_ctx* ctx, const float* pos, const void* mask, long N, int M, int start, int* out_idx, float* out_d2, void* work, long work_bytes,
            utx_stream stream);
/* sample_on_edges_v2 (edge_sampling.py:102-119): N equally spaced samples along the selected edges laid end to end.  verts [V][3] f32, edges [E][2] i32
 * (the selected edges), edge_ids [E] i32 (optional: each one's index in the full edge list, else 0..E-1), start [E] f32 (length before each edge, start[0] = 0),
 * length [E] f32, total = their sum.  Sample i: t = linspace(0, total, N)[i] (torch's formula: step = total / (N - 1); lower half step * i, upper half
 * total - step * (N - 1 - i)); e = searchsorted(start[1:], t), lower bound; w = (t - start[e]) / length[e], 0.5 when non-finite; point = w * v0 + (1 - w) * v1.
 * One step beyond the reference: w is then clamped to [0, 1].  start[] holds ROUNDED running sums, so t can pass start[e] + length[e] by half a float32 step of the
 * running length and the unclamped point would lie past the end of the edge it reports; where the sums are exact the clamp changes nothing.
 * -> samples [N][3] f32, edge_index [N] i32 (optional), edge_t [N] f32 (optional). */
int utx_sample_edges_equal_steps(utx_ctx* ctx, const float* verts, const int* edges, const int* edge_ids, const float* start, const float* length, int E,
                                 float total, long N, float* samples, int* edge_index, float* edge_t, utx_stream stream);
/* sample_surface (surface_sampling.py:24-35).  cum [F] f32: running sum of the face weights |cross(v1 - v0, v2 - v0)|.  The reference draws from the CUDA
 * generator; here the stream is defined: Philox4x32-10, key (seed & 0xffffffff, seed >> 32), counter (i, 0, 0, 0) for sample i, a word x -> (x >> 8) * 2^-24.
 * Word 0: face = min(searchsorted(cum, u0 * cum[F - 1]), F - 1), lower bound; words 1, 2: (u, v), folded as the reference does (u + v > 1: both minus 1, then
 * absolute values), w = 1 - (u + v); point = (v0 * u + v1 * v) + v2 * w.  -> samples [N][3] f32, face_index [N] i32 (optional), uvw [N][3] f32 (optional). */
int utx_sample_surface(utx_ctx* ctx, const float* verts, const int* faces, const float* cum, int F, long N, unsigned long long seed, float* samples,
                       int* face_index, float* uvw, utx_stream stream);
/* The random offsets of sample_spatial / sample_near_surface (spatial_sampling.py:11-37, :40-91) on the same defined stream with another stream id: counter
 * (i, stream_id, 0, 0), stream_id 1 for sample_spatial's points, 2 for the near-surface deltas (0 is utx_sample_surface's, refused here); words 0..2 give r in [0, 1)^3.
 * base == null: out [N][3] = r (the unit cube, as the reference's torch.rand: whatever the mesh's box is).  Otherwise base [N][3] are surface samples with
 * face_index [N] i32 and uvw [N][3], vnormal [V][3] the vertex normals: n = (vn[f0] u + vn[f1] v) + vn[f2] w, not renormalised, and
 * out = base + (threshold * (r * 2 - 1)) * n per component; a face_index outside [0, F) leaves the sample where it is.  uniforms [N][3] (optional) replaces the
 * Philox words (tests feed recorded draws).  One launch.  N == 0 returns 0; -2 for N < 0, N >= 2^31, stream_id < 1, a null out or, with base, a null operand or F <= 0. */
int utx_sample_offsets(utx_ctx* ctx, const float* base, const int* faces, int F, const int* face_index, const float* uvw, const float* vnormal, const float* uniforms,
                       long N, unsigned long long seed, int stream_id, float threshold, float* out, utx_stream stream);
/* PBRMesh.__call__ (mesh/structure_v2.py:105-135): n_attr <= UTX_SAMPLE_ATTRS_MAX attributes at N surface samples (face_index [N] i32, uvw [N][3]) in one launch.
 * src_host / out_host: HOST arrays of n_attr device pointers; dims_host: HOST array [n_attr][4] = (kind, C, H, W); out k is [N][C].
 *   UTX_ATTR_CONSTANT  src [C]: copied.
 *   UTX_ATTR_VERTEX    src [V][C]: (src[f0] u + src[f1] v) + src[f2] w with f = faces[face_index].
 *   UTX_ATTR_TEXTURE   src [H][W][C], C <= 4: uv = (uvs_2d[g0] u + uvs_2d[g1] v) + uvs_2d[g2] w with g = faces_2d[face_index], then torch's grid_sample as the
 *                      reference calls it -- the uv itself is the grid coordinate (NOT mapped from [0, 1] to [-1, 1]), bilinear, align_corners=False,
 *                      padding_mode='reflection': x = ((uv.x + 1) W - 1) / 2, reflected about -0.5 and W - 0.5, clipped to [0, W - 1]; likewise y with H.
 * A face_index outside [0, F) gives zeros (constants are still copied).  C <= UTX_SAMPLE_ATTR_CHANNELS_MAX.  faces is needed by vertex attributes, faces_2d and
 * uvs_2d by textures; else they may be null -- faces_2d and uvs_2d only both or neither.  -2 for a bad count, kind, channel count or size, a missing operand, or one of
 * faces_2d / uvs_2d without the other.  Every refusal happens before any device call. */
#define UTX_SAMPLE_ATTRS_MAX 4
#define UTX_SAMPLE_ATTR_CHANNELS_MAX 16
#define UTX_ATTR_CONSTANT 0
#define UTX_ATTR_VERTEX 1
#define UTX_ATTR_TEXTURE 2
int utx_sample_attrs(utx_ctx* ctx, const int* faces, const int* faces_2d, const float* uvs_2d, int F, const int* face_index, const float* uvw, long N, int n_attr,
                     const float* const* src_host, const int* dims_host, float* const* out_host, utx_stream stream);

/* lens blur consumed on the seam only (image/lens_blur.py:260-280; renderer_inverse.py:620-624).
 * k49_host: HOST array, the collapsed real 7x7 kernel. src/dst [H][W][3] f32. */
int utx_lens_blur_seam(utx_ctx* ctx, const float* src, const void* seam, int H, int W, const float* k49_host, float* dst, utx_stream stream);
/* Gaussian blur consumed on the seam only (method='gaussian': torchvision gaussian_blur(img, (ksize, ksize)), sigma = 0.15 ksize + 0.35;
 * renderer_inverse.py:618-619).  ksize odd, 1..31, ksize / 2 < min(H, W) (reflect padding).  w1_host: HOST array of the ksize fp32 1-D weights.
 * src/dst [H][W][3] f32; the taps are summed in fp64. */
int utx_gaussian_blur_seam(utx_ctx* ctx, const float* src, const void* seam, int H, int W, int ksize, const float* w1_host, float* dst, utx_stream stream);

/* pull-push hole filling (texture/stitching/mip.py:51-95). kd/out [H][W][3] f32, mask [H][W] u8. */
long utx_pull_push_workspace_bytes(int H, int W);
int utx_pull_push(utx_ctx* ctx, const float* kd, const void* mask, int H, int W, float* out, void* work, utx_stream stream);

/* ---- C-channel (PBR stack) bake: renderer_inverse.py:635-726 with image_attrs of 9 channels (albedo, metallic-roughness, bump).  Visibility,
 * winner, seam and the nearest-neighbour search read no colour: they run once, and colour is gathered from the winning view only.  1 <= C <= 16
 * everywhere; all C-channel images are interleaved [..][C] f32 and every channel is processed on its own (the reference's blurs and pull-push are
 * depthwise) by the routine behind the 3-channel entry point, which passes C = 3: channels [3g, 3g+3) of a result equal the 3-channel entry point's
 * result on that group bit for bit. */

/* visibility-only back-projection: utx_backproject_sampled without the colour gather.  d->images is the view ALPHA plane [n_views][H][W] f32,
 * d->color is not read or written (may be NULL); eyes / sample_mode as in utx_backproject_sampled.  rayvis / alphaok are bit-identical to those of
 * utx_backproject_sampled on [n][H][W][4] images whose fourth channel is that plane, on every traversal mode. */
int utx_backproject_vis(utx_ctx* ctx, const utx_backproject_desc* d, const float* eyes, int sample_mode, utx_bvh* bvh, utx_stream stream);
/* utx_composite's priority scan without colours: vis [n_views][T] u8, order_host (HOST array, n_order <= 8 view ids < n_views) -> winner [T] int8. */
int utx_composite_winner(utx_ctx* ctx, const void* vis, int n_views, const int* order_host, int n_order, long T, void* winner, utx_stream stream);
/* atlas [T][C] = images [n_views][H][W][C] sampled at the texel's NDC in view winner[t] (vndc [n_views][V][2], rast2d [T][4], faces [F][3]), with the taps,
 * weights and summation order of utx_backproject_sampled(sample_mode); zeros where winner[t] < 0.  For C = 3 it equals utx_composite(utx_backproject). */
int utx_gather_winner(utx_ctx* ctx, const float* rast2d, const int* faces, const float* vndc, const float* images, const void* winner, long T, int V,
                      int n_views, int H, int W, int C, int sample_mode, float* atlas, utx_stream stream);
/* utx_nn_fill on atlas [T][C]: one search, C floats copied.  nn_index [T] int32 is REQUIRED here (the search's result, -1 = not filled);
 * work as for utx_nn_fill (utx_nn_fill_workspace_bytes(T)). */
int utx_nn_fill_c(utx_ctx* ctx, const float* pos, const void* winner, const float* rast2d, long T, int C, float* atlas, int* nn_index,
                  void* work, long work_bytes, utx_stream stream);
/* utx_lens_blur_seam / utx_gaussian_blur_seam on src / dst [H][W][C] f32. */
int utx_lens_blur_seam_c(utx_ctx* ctx, const float* src, const void* seam, int H, int W, int C, const float* k49_host, float* dst, utx_stream stream);
int utx_gaussian_blur_seam_c(utx_ctx* ctx, const float* src, const void* seam, int H, int W, int C, int ksize, const float* w1_host, float* dst, utx_stream stream);
/* utx_pull_push on kd / out [H][W][C] f32; utx_pull_push_workspace_bytes_c returns 0 for a C outside 1..16. */
long utx_pull_push_workspace_bytes_c(int H, int W, int C);
int utx_pull_push_c(utx_ctx* ctx, const float* kd, const void* mask, int H, int W, int C, float* out, void* work, utx_stream stream);

/* tensor_to_image (renderer_utils.py:62-83): clamp*255 -> u8 by truncation, optional vertical flip. */
int utx_to_u8(utx_ctx* ctx, const float* src, long n_rows, long row_elems, int flip, void* dst, utx_stream stream);

/* sizeof() of the descriptor structs above, in declaration order (ABI self-check for FFI mirrors). */

/* Chart labelling of the blank-mesh UV unwrap (pipeline.py:171-179 preprocess_blank_mesh -> uv_atlas.py:131-175: open3d / UVAtlas
 * [3p], replaced by a builder-defined chart unwrap, unitex_amd/texturetools/meshes.py `unwrap_charts`): connected components of
 * the face adjacency graph restricted to faces of equal `bucket`.  adj [F][3] = face across edge e or -1, bucket [F], chart [F]
 * out = smallest face index of the component (deterministic), flag = one device int of scratch.  Synchronises the stream
 * (convergence test).  Returns the number of sweeps (> 0) or a negative error. */
int utx_chart_flood(utx_ctx* ctx, const int* adj, const int* bucket, int F, int* chart, int* flag, utx_stream stream);

/* ---- utx_plan: one denoise step as a replayable list of launches (SURVEY 8b `utx_dit_step`) ------------------------------------------------
 * The host builds a step of the FLUX DiT once as a list of descriptors over fixed workspaces (unitex_amd/flux/transformer.py is the builder this
 * repo ships; any caller that can fill the descriptors can be one); utx_plan_add_* COPY them, utx_plan_run replays them on `stream` with the
 * same launchers as the single-call entry points above -- same kernels, same order, bit-identical -- in ONE C call per step, nothing allocated,
 * nothing synchronised (capturable into a HIP graph).  Inputs that change between steps (latents, timestep projection, conditioning) live in
 * the device buffers the descriptors point at.  Two-stream sections: utx_plan_fork; entries for the plan's side stream; utx_plan_main; entries for
 * the caller's stream; utx_plan_join (events recorded / awaited inside utx_plan_run).  utx_plan_add_add3: out = bf16(bf16(a + b) + c), n bf16
 * elements (b may be NULL) -- the conditioning-embedding sum of CombinedTimestepGuidanceTextProjEmbeddings [3p].
 * utx_plan_run returns 0 or the failing launcher's code (entry index in *failed_entry when not NULL). */
typedef struct utx_plan utx_plan;
int utx_plan_create(utx_ctx* ctx, utx_plan** out);
void utx_plan_free(utx_plan* plan);
int utx_plan_size(const utx_plan* plan);
int utx_plan_add_gemm(utx_plan* plan, const utx_gemm_desc* d);
int utx_plan_add_gemv(utx_plan* plan, const utx_gemv_desc* d);
int utx_plan_add_ln_mod(utx_plan* plan, const utx_ln_mod_desc* d);
int utx_plan_add_qkv_post(utx_plan* plan, const utx_qkv_post_desc* d);
int utx_plan_add_attn(utx_plan* plan, const void* q, const void* k, const void* vt, void* o, long q_hs, long q_ss, long k_hs, long k_ss, long vt_hs,
                      long vt_ds, long o_ss, int H, int S_q, int S_kv, float softmax_scale, float key_bias_log2, int key_bias_period, void* work,
                      size_t work_bytes);
int utx_plan_add_quant_mx8(utx_plan* plan, const void* x, long ldx, void* q, long ldq, void* s, long lds_or_row_blocks, int M, int K, int packed);
int utx_plan_add_add3(utx_plan* plan, const void* a, const void* b, const void* c, void* out, int n);
/* the opt-in MX fp8 attention as plan entries: arguments of utx_quant_vt_mx8 / utx_attn_fwd_fp8 (Q8 / K8 come from utx_plan_add_quant_mx8 over the
 * [H * S_pad, 128] row view: ldx = ldq = 128, lds = 4, packed = 0) */
int utx_plan_add_quant_vt_mx8(utx_plan* plan, const void* vt, void* v8, void* vs, int H, int S_pad);
int utx_plan_add_attn_fp8(utx_plan* plan, const void* q8, const void* qs, const void* k8, const void* ks, const void* v8t, const void* vs, void* o, long o_ss,
                          int H, int S_q, int S_kv, int S_pad, float key_bias_log2, int key_bias_period);
int utx_plan_add_attn_fp8_ws(utx_plan* plan, const void* q8, const void* qs, const void* k8, const void* ks, const void* v8t, const void* vs, void* o, long o_ss,
                             int H, int S_q, int S_kv, int S_pad, float key_bias_log2, int key_bias_period, void* work, size_t work_bytes);
int utx_plan_fork(utx_plan* plan);
int utx_plan_main(utx_plan* plan);
int utx_plan_join(utx_plan* plan);
int utx_plan_run(utx_plan* plan, utx_stream stream, int* failed_entry);
/* entries [begin, end) only (whole two-stream sections): a host that interleaves its own work with the step -- the sequence-parallel host issues its
 * all-to-alls between ranges -- replays each range with one call.  A launcher error inside a forked section still joins the side stream before returning. */
int utx_plan_run_range(utx_plan* plan, int begin, int end, utx_stream stream, int* failed_entry);
int utx_plan_assign_sk(utx_plan* plan, void* sk_work, size_t sk_work_bytes, int n_cus);   /* split-tail scratch for the caller-stream GEMMs when any has more 256^2 tiles than CUs */
int utx_plan_entry(const utx_plan* plan, int i, int* kind, int* side, void* buf, size_t cap);   /* read an entry back: kind 0 gemm 1 gemv 2 ln_mod 3 qkv_post 4 attn 5 quant 6 add3 7 fork 8 join */

/* ---- utx_dit_load / utx_dit_step: the FLUX.1-dev transformer step built in C -------------------------------------------------------------
 * Replaces FluxTransformer2DModel.forward as the reference calls it (flux_piplines/texturing/pipeline.py:646-656; block arithmetic = diffusers [3p]) for the
 * bf16 single-GPU path: utx_dit_load builds the SAME utx_plan unitex_amd/flux/transformer.py::FluxDiT builds (compared entry by entry, byte by byte, in
 * tests/test_dit_ops_gpu.py::test_c_built_dit_plan_equals_the_python_built_one) from plain structs.  The caller owns everything: weights PACKED as FluxDiT packs
 * them -- double block: qkv_x = [to_q; to_k; to_v] (9216 x 3072), qkv_c = [add_q; add_k; add_v]; single block: qkvm = [to_q; to_k; to_v; proj_mlp] (21504 x
 * 3072); `mod` = every AdaLN modulation Linear concatenated (mod_x / mod_c / mod / mod_out = row offset of a block's slice); LoRA (optional per linear,
 * un-merged, peft semantics): lora_A = s x A of the switched-on adapters concatenated along rank, one block of lora_rp (multiple of 64) rows per output
 * segment (lora_nseg: 3 for the fused q|k|v projections, else 1), lora_B [N_lora, lora_rp], lora_alpha -- and every workspace (bf16 unless noted; S = S_txt +
 * S_img, S_pad = S rounded up to 64, D = 128 heads): lat [S_img, in], enc [S_txt, joint], pooled [1, pooled], tproj / gproj [1, 256] (sinusoidal timestep /
 * guidance projections, filled by the caller per step), e1 / e_t / e_g / e_p / temb [1, D], mod [n_mod], h / xn / attn [S, D], qkv [S, 3D], cat [S, 5D], out
 * [S_img, in], cos / sin [S, 64] fp32 (RoPE tables), Qh / Kh [H, S_pad, 128], Vt [H, 128, S_pad] (zero-filled once: pad rows stay zero), T [S, 3 R] and Tc
 * [S_txt, 3 R] (LoRA temps, R = lora_rank_padded = the largest lora_rp), sk_work (utx_gemm_streamk_workspace_bytes) and attn_work (utx_attn_workspace_bytes)
 * optional.  n_out < S_img: last-block pruning (only the first n_out image rows of `out` are defined); key_bias_*: multiplicity of de-duplicated text keys;
 * two_streams: the text half of the double blocks on the plan's side stream.  A step: write lat / tproj (and enc / pooled / gproj / cos / sin when they change),
 * utx_dit_step(plan, stream) = utx_plan_run, read out.  fp8 = 1: the MX fp8 step (BASELINE configs[4] numerics) -- the linears that carry q / s / sp run
 * on fp8 operands (their LoRA is ignored: merged by the caller), shapes that fill the chip on the one-wave-per-SIMD kernel with tile-packed scales and, with
 * fp8_fuse_quant, activations written as fp8 by LayerNorm-modulation / the GELU epilogues; the rest on the 128^2-tile kernel behind a quantiser pass.  Not in
 * the C builder: sequence parallelism (the collectives are the host's). */
typedef struct utx_dit_linear {
    const void* w; const void* b;
    const void* lora_A; const void* lora_B;
    float lora_alpha; int lora_rp; int lora_nseg;
    /* fp8 mode (utx_dit_config.fp8), the five big image-stream linears only: the weight once more as OCP MX fp8 -- adapters MERGED in before quantising
     * (W + sum s B A, rounded to bf16, then utx_quant_mx8) -- q = e4m3 bytes [N, K], s = row-major E8M0 scales [N, lds_s >= K / 32], sp = the same scales
     * tile-packed (utx_quant_mx8_packed; sp_row_blocks = row blocks per K-tile slab; NULL when N % 256) */
    const void* q; const void* s; long lds_s; const void* sp; int sp_row_blocks;
} utx_dit_linear;
typedef struct utx_dit_double_block {
    utx_dit_linear qkv_x, qkv_c, out_x, out_c, ff1_x, ff2_x, ff1_c, ff2_c;
    const void* nq; const void* nk; const void* naq; const void* nak;      /* RMSNorm weights [128] */
    int mod_x, mod_c;
} utx_dit_double_block;
typedef struct utx_dit_single_block {
    utx_dit_linear qkvm, out;
    const void* nq; const void* nk;
    int mod;
} utx_dit_single_block;
typedef struct utx_dit_weights {
    utx_dit_linear x_embedder, context_embedder, proj_out, t_lin1, t_lin2, g_lin1, g_lin2, p_lin1, p_lin2, mod;
    const utx_dit_double_block* dbl; const utx_dit_single_block* sgl;
    int mod_out, n_mod;
} utx_dit_weights;
typedef struct utx_dit_config {
    int num_heads, num_double, num_single, in_channels, joint_dim, pooled_dim, mlp_ratio, guidance_embeds;
    int S_txt, S_img, n_out;
    float key_bias_log2; int key_bias_period;
    int two_streams, n_cus, lora_rank_padded;
    int fp8, fp8_fuse_quant;      /* MX fp8 linears (qkv_x / ff1_x / ff2_x of the double blocks, qkvm / out of the single blocks); producers write fp8 operands directly */
} utx_dit_config;
typedef struct utx_dit_workspace {
    void *lat, *enc, *pooled, *tproj, *gproj, *e1, *e_t, *e_g, *e_p, *temb, *mod, *h, *xn, *qkv, *cat, *attn, *out;
    float *cos, *sin;
    void *Qh, *Kh, *Vt, *T, *Tc;
    void* sk_work; size_t sk_work_bytes;
    void* attn_work; size_t attn_work_bytes;
    /* fp8 mode: activation scratch aq [S, 5D] e4m3 bytes, as_rm [S, 5D / 32] row-major scales (shapes on the 128^2-tile MX kernel), asp = tile-packed scales
     * [5D / 128][asp_row_blocks >= ceil(S / 128)][512]; aq2 [n_out, 5D] / asp2 the same for the rows a pruned last block keeps (n_out < S_img only) */
    void *aq, *as_rm, *asp; int asp_row_blocks;
    void *aq2, *asp2; int asp2_row_blocks;
} utx_dit_workspace;
int utx_dit_load(utx_ctx* ctx, const utx_dit_config* cfg, const utx_dit_weights* weights, const utx_dit_workspace* ws, utx_plan** out);
int utx_dit_step(utx_plan* plan, utx_stream stream, int* failed_entry);

/* HOST-side mesh preparation (no device work, no context): quadric-error-metric edge-collapse decimation to at most target_faces triangles.
 * Replaces open3d's simplify_quadric_decimation in preprocess_blank_mesh_o3d (uv_atlas.py:155-163; open3d / VTK [3p]) with the published
 * algorithm (Garland & Heckbert 1997): area-weighted face quadrics, boundary edges held by perpendicular constraint planes
 * (boundary_weight, 1.0 in the reference's legacy call), optimal placement, flip rejection.  verts [V][3] f32, faces [F][3] i32 ->
 * verts_out (capacity V), faces_out (capacity F), counts in *V_out / *F_out.  Deterministic.  A collapse is admissible when no surviving face flips, the
 * edge is not a non-manifold fan and the link condition holds (the common neighbours of its ends are exactly the apexes of its faces).  Returns 0, or 1 when
 * no admissible collapse was left above target_faces (the output is valid, *F_out > target_faces), negative on invalid arguments. */
int utx_mesh_decimate_qem(const float* verts, int V, const int* faces, int F, int target_faces, double boundary_weight,
                          float* verts_out, int* faces_out, int* V_out, int* F_out);

int utx_abi_sizes(int* out, int n);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif

// bf16 MFMA flash-attention forward for the FLUX joint [text; image] sequence (gfx950): the family's front door.
// This file holds the contract every bf16 attention kernel shares and the launcher that picks one; the device code is in
//   attention_glds.hip   the 8 x 32 kernel: 8 waves x 32 queries, K / V^T tiles staged by LDS-DMA (general, FAST, FAST + KBP and block-strided BLK instances)
//   attention_q64.hip    the 4 x 64 kernel: one wave per SIMD, generated hand-placed stream (+ its repair pass through the 8 x 32 kernel)
// (attention_fp8.hip, the opt-in MX fp8 kernel, has entry points of its own.)
//
// Replaces: torch SDPA call in NativeFluxAttnProcessor2_0.__call__
//   (/root/reference/flux_piplines/texturing/attention_processor.py:89-91): non-causal, no mask,
//   no dropout, head_dim 128, softmax scale 1/sqrt(128).
//
// Layout (produced by qkv_post in dit_elementwise.hip):
//   Q, K : [H][S_pad][128] bf16 (d contiguous)       -- strides passed explicitly
//   Vt   : [H][128][S_pad] bf16 (keys contiguous)    -- V pre-transposed so that the PV product's
//                                                       MFMA A-operand is a 16-byte LDS read
//   O    : [S][H*128] bf16 (token-major; feeds the out-projection GEMM directly)
//   K rows / Vt columns are readable up to the next multiple of 64 past S (ABI contract); KV tile = 64 keys.
//
// What the kernels share:
//   * S^T = K Q^T is computed "swapped" (MFMA A = K, B = Q) so each lane owns one query column and the
//     softmax row reductions are in-register (+ one cross-half exchange).  K rows inside each 32-key block
//     are read through a permutation kappa() chosen so that the C-layout of the 32x32x16 MFMA leaves, in each
//     lane, exactly the 8 consecutive keys the PV MFMA's B-operand wants: P goes to bf16 in registers and
//     straight into the second MFMA (no LDS round trip, no permlane).  O^T = Vt P^T accumulates in 4 x f32x16
//     per 32 queries.  kappa: MFMA row i = 8a + 4h' + c  ->  key 16(a>>1) + 8h' + 4(a&1) + c (within a 32-key block).
//   * the softmax VALU stream is minimised: score accumulators are INITIALISED to -m_run (the C-input of the first
//     QK^T MFMA of a block is a register block holding -m_run: the MFMA chain does the max subtraction and not even
//     the initialisation is per-tile VALU work); with Q pre-scaled by scale*log2(e) upstream (qkv_post) a probability
//     is ONE v_exp_f32; the running max only moves when it has to ("defer-max", guide T13).
//   * sum-checked softmax: tools/coissue_probe.hip shows that on this chip VALU work is NOT hidden under another
//     wave's MFMAs (cross-wave overlap ~0, same-wave ~0.5), so every softmax instruction costs wall time.  The common
//     path therefore has NO max reduction at all: a block is exponentiated against the running max as it stands and
//     only the row sum is checked: if any lane's partial sum exceeds 2^13 (some probability > 2^8 at the least), the
//     block is redone on the slow path -- QK^T again with the true max, O / l rescaled -- before anything of it was
//     accumulated.  Per tile and lane that removes 16 v_max3 + 2 v_max + a ds_bpermute round trip + 18 v_mov.  (The
//     4 x 64 kernel never re-centres: it marks the block and its repair pass redoes it, attention_q64.hip.)
//   Measured-negative in round 1 (profiles/r01_perf_ops_attn_variants.log): 4 waves x 2 workgroups / CU, QK(t+1)
//   software-pipelined under softmax(t), late-PV "ping-pong" between wave halves.
//
// Algorithmic FLOPs: 4 * S^2 * 128 per head (QK^T + PV, non-causal).
#include "common.h"
#include "kernels.h"
#include <stdlib.h>

// softmax_scale > 0: scores are multiplied by softmax_scale (natural-exp softmax, the reference's SDPA).
// softmax_scale == 0: Q was pre-multiplied by scale*log2(e) upstream (utx_qkv_post q_scale) -> scores are
// already base-2 exponents and a probability is a single v_exp_f32.
extern "C" int utx_launch_attn_fwd(const void* q, const void* k, const void* vt, void* o,
                                   long q_hs, long q_ss, long k_hs, long k_ss, long vt_hs, long vt_ds,
                                   long o_ss, int H, int S, int Sq, float scale, float key_bias_log2, int key_bias_period, void* work, size_t work_bytes,
                                   hipStream_t stream) {
    return utx_launch_attn_fwd_blk(q, k, vt, o, q_hs, q_ss, k_hs, k_ss, vt_hs, vt_ds, o_ss, H, S, Sq, scale, key_bias_log2, key_bias_period, work, work_bytes,
                                   0, 0, 0, 0, stream);
}

// blk_rows > 0: Q / K / V^T in blocks of blk_rows tokens q_bs / k_bs / vt_bs elements apart (attention_glds.hip BLK).
// The dispatch of the family: validate, then the 4 x 64 kernel if it takes the launch, else the 8 x 32 kernel, whose launcher picks the instance.
extern "C" int utx_launch_attn_fwd_blk(const void* q, const void* k, const void* vt, void* o,
                                       long q_hs, long q_ss, long k_hs, long k_ss, long vt_hs, long vt_ds,
                                       long o_ss, int H, int S, int Sq, float scale, float key_bias_log2, int key_bias_period, void* work, size_t work_bytes,
                                       int blk_rows, long q_bs, long k_bs, long vt_bs, hipStream_t stream) {
    // Sq > S is a plain case (round 6): queries and keys are separate arrays and nothing ties a query row to a key row -- the sequence-parallel launch whose keys carry the
    // ranks' identical text rows once (utx_sp_unpack_qkv_dedup) has P x 64 - 64 more queries than keys.  Block-strided operands share their blocks: Sq <= S there.
    if (S <= 0 || H <= 0 || scale < 0.f || key_bias_period < 0 || Sq < 0 || (Sq > S && blk_rows > 0) || blk_rows < 0) return -1;
    if (Sq == S) Sq = 0;
    if ((((uintptr_t)q) | ((uintptr_t)k) | ((uintptr_t)vt)) & 15) return -2;                       // 16-byte aligned bases (LDS-DMA / b128 loads)
    if ((vt_ds & 7) || (q_ss & 7) || (k_ss & 7) || (o_ss & 3) || (q_hs & 7) || (k_hs & 7) || (vt_hs & 7)) return -2;   // 16-byte rows
    AttnParams p;
    p.q = (const bf16_t*)q; p.k = (const bf16_t*)k; p.vt = (const bf16_t*)vt; p.o = (bf16_t*)o;
    p.q_hs = q_hs; p.q_ss = q_ss; p.k_hs = k_hs; p.k_ss = k_ss; p.vt_hs = vt_hs; p.vt_ds = vt_ds;
    p.o_ss = o_ss; p.H = H; p.S = S; p.nqb = 0; p.Sq = Sq;
    p.dbg = g_utx_opt.attn_debug_abl;   // always 0 in the product library (capi.cpp)
    p.scale_log2 = scale * 1.4426950408889634f;
    const bool presc = (scale == 0.f);
    p.flags = nullptr; p.flag_hs = 0;
    p.key_bias_log2 = key_bias_log2; p.key_bias_period = key_bias_period;
    p.work = work; p.work_bytes = work_bytes;
    p.blk_rows = blk_rows; p.q_bs = q_bs; p.k_bs = k_bs; p.vt_bs = vt_bs;
    // UTX_ATTN_Q64=1: the 4 x 64 kernel (attention_q64.hip: one wave per SIMD, hand-placed stream) + its repair pass, for the launches it takes (pre-scaled Q, whole 64-key
    // tiles, contiguous operands, no periodic key multiplicity, caller scratch with room for its flags)
    if (g_utx_opt.attn_q64 == 1 && utx_attn_q64_takes(&p, presc ? 1 : 0)) return utx_launch_attn_fwd_q64(&p, 1, stream);
    // everything else: the 8 x 32 kernel (attention_glds.hip) -- BLK for block-strided operands, FAST + KBP / FAST for pre-scaled Q under UTX_ATTN_PEEL, else the general loop
    return utx_launch_attn_fwd_glds(&p, presc ? 1 : 0, stream);
}

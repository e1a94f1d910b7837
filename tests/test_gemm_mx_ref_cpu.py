"""oracle/gemm_mx_fp64.py audited on the CPU: for every input set that tests/test_gemm_mx_edges_gpu.py sends to the GPU,
  (a) the float32 emulation of the MX kernels lies inside the counted interval at every element, its fp8 output passes qout_accept, and at most 5 % of the elements have an
      interval that holds more than one bf16 value (the cap of tests/test_gemm_ref_cpu.py; the reference alone must meet it);
  (b) the inputs have the property that makes the GPU test sharp: every 32-block carries at least 1 / (8 K / 32) of sum|a b| for every output element (blocks zeroed on
      purpose excepted) and every row carries at least four distinct scale bytes;
  (c) each of eleven mistakes an MX kernel can make falls outside the acceptance check at a case that exercises it.
Largest share of multi-valued intervals over all cases (printed by test_multi_valued_share_stays_small): 3.06 %, at mx2_m256_gelu_split (K = 640)."""
import numpy as np
import pytest

from oracle import gemm_fp64 as G
from oracle import gemm_mx_fp64 as X

_BY_NAME = {c["name"]: c for c in X.CASES}
_QOUT = {c["name"] for c in X.CASES_QOUT}
_CACHE = {}


def _case_data(name):
    """(case, inputs, reference) -- built once per case and shared, never modified"""
    if name not in _CACHE:
        case = _BY_NAME[name]
        inp = X.make_inputs(case)
        _CACHE[name] = (case, inp, X.reference(case, inp))
    return _CACHE[name]


def _verdict(case, inp, ref, defect=None, kt0=None):
    """None when the emulation (with `defect`) passes every check the GPU test makes of a launch, else the first complaint"""
    em = X.emulate(case, inp, defect, q_out_kt0=kt0)
    if kt0 is None:
        return G.first_offender(em["out"], ref, case["name"])
    gf = case["gelu_from"]
    c = G.first_offender(em["out"][:, :gf], G.Ref(*(x[:, :gf] for x in ref)), case["name"] + " columns < gelu_from")
    if c is None and not (em["out"][:, gf:] == G.SENT).all():
        c = "C1 written"
    return c or X.qout_check(em["q"], em["qs"], case["M"], case["N"] - gf, kt0, X.gelu_part(ref, gf), case["name"])


@pytest.mark.parametrize("name", sorted(_BY_NAME))
def test_correct_emulation_is_accepted(name):
    case, inp, ref = _case_data(name)
    assert ref.out.shape == (case["M"], case["N"]) and (ref.lo <= ref.out).all() and (ref.out <= ref.hi).all()
    msg = _verdict(case, inp, ref)
    assert msg is None, msg
    if name in _QOUT:
        for kt0 in (0, 1):
            msg = _verdict(case, inp, ref, kt0=kt0)
            assert msg is None, msg


def test_multi_valued_share_stays_small():
    worst = (0.0, None)
    for name in sorted(_BY_NAME):
        case, _, ref = _case_data(name)
        share = G.multi_valued_share(ref)
        print("%-40s K + K2 = %3d  multi-valued intervals %.2f %%" % (name, case["K"] + case["K2"], 100 * share))
        worst = max(worst, (share, name))
        assert share <= 0.05, "%s: %.2f %% of the intervals hold more than one bf16 value" % (name, 100 * share)
    print("largest share of multi-valued intervals: %.2f %% (%s)" % (100 * worst[0], worst[1]))


@pytest.mark.parametrize("name", sorted(_BY_NAME))
def test_every_block_scale_matters(name):
    case, inp, _ = _case_data(name)
    KB = case["K"] // 32
    sh = X.block_shares(inp)
    exempt = inp["zero_a"].T[:, :, None] | inp["zero_b"].T[:, None, :]
    smallest = float(np.where(exempt, 1.0, sh).min())
    rows = [len(set(r)) for r in inp["As"]] + [len(set(r)) for r in inp["Bs"]]
    print("%-40s smallest block share %.2f %% of sum|a b| (needed %.2f %%), distinct scale bytes per row %d..%d" % (
        name, 100 * smallest, 100 / (8.0 * KB), min(rows), max(rows)))
    assert smallest >= 1.0 / (8 * KB)
    assert min(rows) >= 4
    if case["special"] == "zero_block":
        assert inp["zero_a"].any() and inp["zero_b"].any() and (sh[exempt] == 0).all()
        assert (inp["As"][inp["zero_a"]] == 0).all() and (inp["Aq"].reshape(case["M"], KB, 32)[inp["zero_a"]] == 0).all()
    if case["special"] == "pow2_block":
        amax = np.abs(inp["A"][:, :32]).max(1)
        assert (np.exp2(np.round(np.log2(amax))) == amax).all()
    if case["span"] == 100:
        assert inp["As"].min() < 40 and inp["As"].max() > 210 and inp["Bs"].min() < 40 and inp["Bs"].max() > 210
        assert np.isfinite(X.reference(case, inp).out).all()


def test_every_listed_shape_and_option_is_among_the_cases():
    """the issue's lists, so that a case edited away is noticed here and not by a missing GPU run"""
    m1, m2 = X.CASES_MX1, X.CASES_MX2
    assert {(c["M"], c["N"]) for c in m1} >= {(1, 8), (7, 136), (127, 264), (128, 128), (129, 384), (200, 384), (600, 264), (200, 136)}
    assert {c["K"] for c in m1} == {128, 256, 384} and {c["K"] for c in m2} == {128, 256, 384, 640}
    assert any(c["gelu_from"] == 0 for c in m1) and any(c["gelu_from"] == 132 and c["pad_a"] == 64 and c["pad_sa"] and c["pad_sb"] for c in m1)
    assert any(c["K2"] == 64 and c["alpha"] == 0.37 and not c["bias"] for c in m1) and any(c["nseg"] == 3 and c["lora_n_limit"] == 256 and c["N"] == 384 for c in m1)
    assert any(c["n_split"] == 128 and c["gelu_from"] == 128 and c["K2"] for c in m1)
    assert any(c["gate"] == "inplace" and c["M"] == 600 for c in m1) and any(c["gate"] == "separate" and c["pad_res"] for c in m1)
    for cs in (m1, m2):
        assert any(c["span"] == 100 for c in cs) and any(c["special"] == "zero_block" for c in cs)
    assert any(c["special"] == "pow2_block" for c in X.CASES)
    assert {(c["M"], c["N"]) for c in m2} >= {(1, 256), (64, 512), (129, 768), (256, 512), (257, 768), (300, 256), (600, 512)}
    assert {(c["pers_grid"], c["gelu_from"], c["gate"]) for c in m2 if (c["M"], c["N"]) == (600, 512)} == {(1, None, None), (2, 256, None), (3, None, "inplace")}
    assert any(c["b_slice"] == (256, 768, 1024) for c in m2) and all(c["K2"] == 0 for c in m2)
    assert {(c["streamk"], c["K"], c["gate"]) for c in X.CASES_MXSPLIT} == {(S, K, g) for S in (2, 3) for K in (384, 640) for g in (None, "inplace")}
    assert all((c["M"], c["N"], c["pers_grid"]) == (600, 512, 4) for c in X.CASES_MXSPLIT)
    b = X.CASE_BOTH
    assert (b["M"], b["N"], b["K"], b["gelu_from"], b["n_split"]) == (300, 512, 384, 256, 256)
    assert {(c["M"], c["N"], c["K"], c["gelu_from"], c["n_split"]) for c in X.CASES_QOUT} == {(M, 512, 256, 256, 256) for M in (300, 129, 600)}
    assert len({c["name"] for c in X.CASES}) == len(X.CASES)


# the cases that exercise each defect (a_scale_row_block0 / packed_l_im_swapped need M > 128 resp. any M > 1; lora_skipped a LoRA segment; qout_* a q_out case)
_DEFECT_CASES = {
    "drop_last_k_tile": ("mx1_m1_n8", "mx1_m127_gelu132_lda_lds", "mx2_m256_gelu_split", "mxsk_s3_k640_plain"),
    "a_scale_next_block": ("mx1_m7_gelu0", "mx2_m129", "mx2_m200_span100", "mx2_m129_zero_blocks"),
    "b_scale_stuck_at_kt0": ("mx1_m200_gated_separate", "mx2_m64_alpha_nobias", "mxsk_s2_k384_gated"),
    "a_scale_row_block0": ("mx1_m129_lora3seg", "mx2_m257_pow2", "mx2_m600_grid1"),
    "packed_l_im_swapped": ("mx2_m64_alpha_nobias", "mx2_m300_gated", "mx2_m600_gated_grid3"),
    "a_scale_for_b": ("mx1_m200_span100", "mx2_m200_span40_bslice"),
    "lora_skipped": ("mx1_m128_lora_alpha_nobias", "mx1_m129_lora3seg", "mx1_m200_loraseg_split_gelu128"),
    "qout_from_unrounded_y": ("mxq_m300", "mxq_m600"),
    "qout_kt0_ignored": ("mxq_m300",),
    "qout_amax_over_8": ("mxq_m300", "mxq_m129"),
    "qout_rows_ge_M_written": ("mxq_m300", "mxq_m129", "mxq_m600"),
}


def test_the_defect_list_is_the_oracles():
    assert set(_DEFECT_CASES) == set(X.DEFECTS) and len(X.DEFECTS) == 11


@pytest.mark.parametrize("defect,name", [(d, n) for d in sorted(_DEFECT_CASES) for n in _DEFECT_CASES[d]])
def test_defect_is_rejected(defect, name):
    case, inp, ref = _case_data(name)
    msg = _verdict(case, inp, ref, defect, kt0=1 if name in _QOUT else None)
    print("%s at %s: %s" % (defect, name, msg))
    assert msg is not None, "%s: the acceptance check does not see the defect `%s`" % (name, defect)


def test_wrong_a_scale_block_puts_every_element_outside():
    """the sharpness the operand scheme was chosen for: with A's scales of each K-tile rotated by one block, every element of the case leaves its interval"""
    case, inp, ref = _case_data("mx2_m129")
    assert not G.accepted(X.emulate(case, inp, "a_scale_next_block")["out"], ref).any()


def test_pack_scales_round_trip_and_layout():
    rng = np.random.default_rng(5)
    for R, K in ((1, 128), (129, 384), (300, 640)):
        s = rng.integers(0, 255, (R, K // 32)).astype(np.uint8)
        p = X.pack_scales(s, row_blocks=(R + 127) // 128 + 1, slabs=K // 128 + 1)
        assert p.shape == (K // 128 + 1, (R + 127) // 128 + 1, 512)
        assert (X.unpack_scales(p, R, K) == s).all()
        assert (p[K // 128:] == X.S_SENT).all() and (p[:, (R + 127) // 128:] == X.S_SENT).all()
        assert int((p != X.S_SENT).sum()) <= s.size and int((p == X.S_SENT).sum()) >= p.size - s.size       # rows >= R of the last row block keep the fill
        m, b = R - 1, K // 32 - 1                                                                         # the header's sentence, on one byte
        assert p[b // 4, m // 128].reshape(32, 4, 4)[m % 32, (m % 128) // 32, b % 4] == s[m, b]
    q, sc = X.quantize(np.array([[1.0] * 32 + [0.0] * 32 + [448.0 * 2.0 ** 5] * 32 + [-3.0] * 32]))
    assert list(sc[0]) == [127 - 8, 0, 127 + 13 - 8, 127 + 1 - 8] and (X.dequantize(q, sc)[0, 96:] == -3.0).all() and (X.dequantize(q, sc)[0, :32] == 1.0).all()


def test_qout_accept_reduces_to_bit_equality_on_single_valued_blocks():
    case, inp, ref = _case_data("mxq_m129")
    g = X.gelu_part(ref, case["gelu_from"])
    q, s = X.quantize(g.out)
    ok_s, ok_q = X.qout_accept(q, s, g)
    assert ok_s.all() and ok_q.all()
    single = (g.lo == g.hi).reshape(case["M"], -1, 32).all(-1)
    assert single.mean() > 0.3
    m, b = (int(v) for v in np.argwhere(single)[0])
    for dq, ds in ((1, 0), (0, 1)):
        q2, s2 = q.copy(), s.copy()
        col = 32 * b + int(np.argmax(q[m, 32 * b: 32 * b + 32] & 0x7F))
        q2[m, col] ^= dq
        s2[m, b] += ds
        ok_s, ok_q = X.qout_accept(q2, s2, g)
        assert not (ok_s.all() and ok_q.all())


def test_gemm_plan_reports_the_mx_dispatch_in_k_tiles_of_128():
    """utx_gemm_plan with mx8: mx8 = 1 is the 128 x 128 kernel, mx8 = 2 the one-wave-per-SIMD kernel whatever the tile count; a forced split into S ranges exists only
    where K / 128 >= S, as in the launcher (which counts K in 128-element K-tiles for MX operands)"""
    from unitex_amd import _lib
    from unitex_amd.flux import ops
    try:
        assert ops.gemm_plan(600, 512, K=384, mx8=1)["kernel"] == "128x128"
        _lib.set_option("UTX_GEMM_PERS_GRID", 4)
        for S, K, want in ((2, 384, 2), (3, 384, 3), (3, 640, 3), (3, 256, 0), (2, 128, 0)):
            _lib.set_option("UTX_GEMM_STREAMK", 1000 + S)
            p = ops.gemm_plan(600, 512, K=K, mx8=2)
            assert (p["kernel"], p["tiles"], p["tail_tiles"], p["ranges"]) == ("w4", 6, 2 if want else 0, want), (S, K, p)
    finally:
        _lib.set_option("UTX_GEMM_PERS_GRID", 0)
        _lib.set_option("UTX_GEMM_STREAMK", 1)

"""oracle/gemm_fp64.py audited on the CPU: for every input set that tests/test_gemm_edges_gpu.py sends to the GPU,
  (a) a float32 restatement of the gemm.hip contract in torch lies inside the counted interval at every element, and at most 5 % of the elements have an
      interval that holds more than one bf16 value (the condition that keeps the GPU test sharp: the reference alone must meet it);
  (b) a float32 numpy emulation of the kernels passes the same acceptance check, and fails it with each of eight mistakes a GEMM kernel can make, at the
      case that is there for that mistake.
Largest share of multi-valued intervals over all cases (printed by test_multi_valued_share_stays_small): 1.41 %, at sk_s3_k320_0_plain (K = 320)."""
import numpy as np
import pytest
import torch

from oracle import gemm_fp64 as G

BF = torch.bfloat16
_BY_NAME = {c["name"]: c for c in G.CASES}
_CACHE = {}


def _case_data(name):
    """(case, inputs, reference) -- built once per case and shared, never modified"""
    if name not in _CACHE:
        case = _BY_NAME[name]
        inp = G.make_inputs(case)
        _CACHE[name] = (case, inp, G.reference(case, inp))
    return _CACHE[name]


def _t(a):
    return None if a is None else torch.from_numpy(np.asarray(a, dtype=np.float32))


def _torch_float32(case, inp):
    """the contract restated in torch on the CPU: float32 products, a bf16 rounding at each tensor boundary.  GELU in the sigmoid form x * sigmoid(2u) (the same function
    as 0.5 x (1 + tanh u); 1 + tanh u cancels in float32 for x < -3, which is the restatement's own error and not the contract's)"""
    A, B, bias, A2, B2, gate, res = (_t(inp[k]) for k in ("A", "B", "bias", "A2", "B2", "gate", "res"))
    N, K2 = B.shape[0], case["K2"]
    acc = A @ B.t()
    if K2:
        seg = N if case["lora_seg_n"] is None else case["lora_seg_n"]
        lim = N if case["lora_n_limit"] is None else case["lora_n_limit"]
        for n in range(0, lim, seg):
            s = n // seg
            acc[:, n: min(n + seg, lim)] += A2[:, s * K2: (s + 1) * K2] @ B2[n: min(n + seg, lim)].t()
    y = acc * case["alpha"]
    if bias is not None:
        y = y + bias
    y = y.to(BF).float()
    gf = case["gelu_from"]
    if gf is not None and gf < N:
        x = y[:, gf:]
        y[:, gf:] = (x * torch.sigmoid(2 * 0.7978845608028654 * (x + 0.044715 * x * x * x))).to(BF).float()
    if gate is not None:
        y = (res + (gate * y).to(BF).float()).to(BF).float()
    return y.double().numpy()


@pytest.mark.parametrize("name", sorted(_BY_NAME))
def test_torch_float32_restatement_lies_inside_the_interval(name):
    case, inp, ref = _case_data(name)
    assert ref.out.shape == (case["M"], case["N"]) and (ref.lo <= ref.out).all() and (ref.out <= ref.hi).all()
    msg = G.first_offender(_torch_float32(case, inp), ref, name)
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


def test_every_listed_shape_and_option_is_among_the_cases():
    """the issue's lists, so that a case edited away is noticed here and not by a missing GPU run"""
    c128, w4 = [c for c in G.CASES_128], [c for c in G.CASES_W4]
    assert {c["M"] for c in c128} >= {1, 7, 127, 128, 129, 200, 600} and {c["N"] for c in c128} >= {8, 128, 136, 264, 384}
    assert {c["K"] for c in c128} >= {64, 128, 192} and {c["K2"] for c in c128} >= {0, 64, 128}
    assert {c["gelu_from"] for c in c128} >= {0, 128, 132, 136, None}          # None: gelu_from = N
    assert any(c["lora_seg_n"] == 128 and c["lora_n_limit"] == 256 and c["N"] == 384 and c["nseg"] == 3 for c in c128)
    assert any(c["K2"] and 0 < c["lora_n_limit"] < c["N"] for c in c128)
    assert any(c["n_split"] == 128 and c["pad_c1"] != c["pad_c"] for c in c128)
    assert any(c["alpha"] == 0.37 and c["bias"] for c in c128) and any(c["alpha"] == 0.37 and not c["bias"] for c in c128)
    assert any(c["gate"] == "inplace" for c in c128) and any(c["gate"] == "separate" and c["pad_res"] != c["pad_c"] for c in c128)
    assert any(c["pad_a"] for c in c128) and any(c["pad_c"] for c in c128) and any(c["pad_c"] for c in w4)
    assert {c["M"] for c in w4} >= {1, 64, 129, 256, 257, 300, 600} and {c["N"] for c in w4} >= {256, 512, 768}
    assert {c["K"] for c in w4} >= {64, 128, 192, 320} and {c["K2"] for c in w4} >= {0, 64, 128}
    assert any(c["lora_seg_n"] == 256 and c["lora_n_limit"] == 256 and c["N"] == 768 for c in w4)
    assert {c["pers_grid"] for c in w4 if (c["M"], c["N"]) == (600, 512)} >= {1, 2, 3}
    assert any(c["gelu_from"] == 256 and c["n_split"] == 256 for c in w4) and any(c["gate"] == "inplace" for c in w4) and any(c["alpha"] == 0.37 for c in w4)
    assert {(c["streamk"], c["K"], c["K2"], c["gate"]) for c in G.CASES_SPLIT} == {(S, K, K2, g) for S, K, K2 in ((4, 192, 64), (3, 320, 0), (2, 128, 128))
                                                                                 for g in (None, "inplace")}
    assert all((c["M"], c["N"], c["pers_grid"]) == (600, 512, 4) for c in G.CASES_SPLIT)
    assert all(c["M"] * c["N"] * (c["K"] + c["K2"]) <= 600 * 768 * 512 for c in G.CASES)
    assert len({c["name"] for c in G.CASES}) == len(G.CASES)


@pytest.mark.parametrize("name", sorted(_BY_NAME))
def test_correct_emulation_is_accepted(name):
    case, inp, ref = _case_data(name)
    msg = G.first_offender(G.emulate(case, inp), ref, name + " (float32 emulation)")
    assert msg is None, msg


# the case that is there for each defect
_DEFECT_CASES = {
    "drop_last_k_tile": ("t128_m127_gelu132_lda", "w4_m256_gelu_split", "sk_s3_k320_0_plain"),
    "skip_lora_seg1": ("t128_m129_lora3seg_alpha", "w4_m600_lora_grid3"),
    "a2_seg0_for_seg1": ("t128_m129_lora3seg_alpha", "w4_m600_lora_grid3"),
    "alpha_on_bias": ("t128_m129_lora3seg_alpha", "w4_m257_lora_alpha"),
    "round_acc_before_bias": ("t128_m7_gelu0", "t128_m1_n8", "w4_m129_lora"),
    "gelu_4_late": ("t128_m127_gelu132_lda", "t128_m129_gelu136", "w4_m256_gelu_split"),
    "gate_y_unrounded": ("t128_m600_gated_inplace", "t128_m200_gated_separate", "w4_m300_gated", "sk_s2_k128_128_gated"),
    "n_tail_group_unwritten": ("t128_m7_gelu0", "t128_m1_n8", "t128_m127_gelu132_lda"),
}


def test_the_defect_list_is_the_oracles():
    assert set(_DEFECT_CASES) == set(G.DEFECTS) and len(G.DEFECTS) == 8


@pytest.mark.parametrize("defect,name", [(d, n) for d in sorted(_DEFECT_CASES) for n in _DEFECT_CASES[d]])
def test_defect_is_rejected(defect, name):
    case, inp, ref = _case_data(name)
    got = G.emulate(case, inp, defect)
    bad = ~G.accepted(got, ref)
    print("%s at %s: %d of %d elements rejected" % (defect, name, int(bad.sum()), bad.size))
    assert bad.any(), "%s: the acceptance check does not see the defect `%s`" % (name, defect)


def test_interval_arithmetic_on_a_hand_computed_element():
    """one element by hand: A = [1, 2], B = [[0.5, 0.25]] padded with zeros to K = 64, bias 0.125 -> y = 1.125 exactly (a bf16 value), e = 68 x 2^-23 x 1.125 far below
    half an ulp (2^-8): the interval is the single value; with gate 3 and res 1 the output is bf16(1 + bf16(3.375)) = 4.375"""
    A = np.zeros((1, 64)); A[0, :2] = (1, 2)
    B = np.zeros((8, 64)); B[0, :2] = (0.5, 0.25)
    bias = np.zeros(8); bias[0] = 0.125
    r = G.gemm(A, B, bias)
    assert r.out[0, 0] == r.lo[0, 0] == r.hi[0, 0] == 1.125 and (r.out[0, 1:] == 0).all() and (r.lo == r.hi).all()
    r = G.gemm(A, B, bias, gate=np.full(8, 3.0), res=np.ones((1, 8)))
    assert r.out[0, 0] == r.lo[0, 0] == r.hi[0, 0] == 4.375
    r = G.gemm(A, B, bias, gelu_from=0)
    exact = 1.125 * 0.5 * (1 + np.tanh(0.7978845608028654 * (1.125 + 0.044715 * 1.125 ** 3)))
    assert abs(r.out[0, 0] - exact) <= 2.0 ** -9 * exact and r.lo[0, 0] <= r.out[0, 0] <= r.hi[0, 0]
    assert not G.accepted(np.full((1, 8), G.SENT), r).any()

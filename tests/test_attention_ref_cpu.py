"""oracle/attention_fp64.py audited on the CPU: for every input set that tests/test_attention_edges_gpu.py sends to the GPU,
  (a) a float32 numpy emulation of the kernels' algorithm lies inside the counted interval at EVERY element, every addressed row keeps between 0.3 and 0.7 of its weight
      on its target key, and (ramp cases apart) the median of E / |ref| stays below 2^-6 -- a condition on the inputs that the reference alone must meet;
  (b) the emulation fails the same acceptance check with each of ten mistakes an attention kernel can make, at the cases that are there for that mistake;
  (c) the float64 reference summed over the keys in reversed order lies inside its own interval.
The key-split cases depend on the CU count: this module runs them at 8 CUs (H = 5: the same two tail items behind one full round, in seconds) and checks the plan
arithmetic of the 256-CU shapes that the case list states against the library's utx_attn_plan."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import attention_fp64 as A

NCU = 8
_SPLIT = A.split_cases(NCU)
_ALL = A.CASES + _SPLIT
_BY_NAME = {c["name"]: c for c in _ALL}
_CACHE = {}


def _scales(case):
    """the softmax_scale values a case runs under: the 8 x 32 cases both, everything else pre-scaled Q"""
    return (A.SCALE, 0.0) if case["kernel"] == "g" else (0.0,)


def _plan(case):
    return A.split_plan(case["H"], case["Sq"], case["Sk"], NCU, bool(case["tailsplit"])) if case["kernel"] == "split" else None


def _case_data(name, scale):
    """(case, inputs, plan, reference) -- built once and shared, never modified"""
    if (name, scale) not in _CACHE:
        case = _BY_NAME[name]
        inp, plan = A.make_inputs(case, scale), _plan(case)
        _CACHE[(name, scale)] = (case, inp, plan, A.reference(case, inp, scale, None if plan is None else A.split_rows(case, plan)))
    return _CACHE[(name, scale)]


_RUNS = [(c["name"], s) for c in _ALL for s in _scales(c)]


@pytest.mark.parametrize("name,scale", _RUNS)
def test_correct_emulation_is_accepted_and_the_inputs_are_sharp(name, scale):
    case, inp, plan, ref = _case_data(name, scale)
    assert ref.out.shape == (case["H"], case["Sq"], 128) and (ref.lo <= ref.out).all() and (ref.out <= ref.hi).all()
    med, mx = A.rel_width(ref)
    wt = ref.wt[~np.isnan(ref.wt)]
    print("%-30s scale %.4f  E / |ref| median 2^%.2f max 2^%.2f  target weight [%s]  keys aimed at %.0f %%  base-2 scores [%.1f, %.1f]  plan %s" % (
        name, scale, np.log2(med), np.log2(mx), "%.3f, %.3f" % (wt.min(), wt.max()) if wt.size else "no addressed rows", 100 * A.coverage(inp, case["Sk"]),
        ref.smin, ref.smax, plan))
    if case["ramp"] == 0 and case["Sk"] > 1:
        assert wt.size and wt.min() >= 0.3 and wt.max() <= 0.7, "%s: target weights [%g, %g]" % (name, wt.min(), wt.max())
        n_rows = int((inp["tgt"] >= 0).sum())
        if n_rows >= 2 * case["Sk"] + 64:
            assert A.coverage(inp, case["Sk"]) == 1.0, "%s: %d addressed rows leave keys that nobody aims at" % (name, n_rows)
    if case["ramp"] == 0:
        assert med < 2.0 ** -6, "%s: median E / |ref| = 2^%.2f" % (name, np.log2(med))
    msg = A.first_offender(A.emulate(case, inp, scale, plan), ref, inp, name + " (float32 emulation)", plan)
    assert msg is None, msg


def test_edge_keys_are_aimed_at_from_every_wave_slice():
    """key 0 and key S_kv - 1 from every 32-query wave slice with at least two addressed rows; the first and last key of every tile and all 32 positions of the chosen block somewhere"""
    for name in ("g_h3_q300_k520", "g_h2_q520_k300", "q64_h2_q448_k256", "blk128_k384_plain"):
        case, inp, _, _ = _case_data(name, 0.0)
        n, tgt = case["Sk"], inp["tgt"]
        for h in range(case["H"]):
            for s0 in range(0, case["Sq"], 32):
                t = set(tgt[h, s0: s0 + 32].tolist())
                if len(t - {-1}) >= 2:
                    assert 0 in t and n - 1 in t, (name, h, s0)
        aimed = set(tgt[tgt >= 0].tolist())
        for t in range((n + 63) // 64):
            assert 64 * t in aimed and min(64 * t + 63, n - 1) in aimed, (name, t)
        assert any(all(32 * b + p in aimed for p in range(32)) for b in range(n // 32)), name
        assert (inp["kind"] == "b").sum() >= case["H"] * (case["Sq"] // 8)


def test_pad_region_is_part_of_the_input_set():
    case, inp, _, _ = _case_data("g_h2_q33_k40", 0.0)
    assert inp["k"].shape == (2, 64, 128) and (np.abs(inp["v"][:, 40:]) == 64.0).all() and (np.abs(inp["k"][:, 40:]).max(-1) > 4.0).all()
    for key in ("q", "k", "v"):
        assert (A.bf16(inp[key]) == inp[key]).all(), key


def test_every_listed_shape_and_option_is_among_the_cases():
    """the issue's lists, so that a case edited away is noticed here and not by a missing GPU run"""
    shape = lambda cs: {(c["H"], c["Sq"], c["Sk"]) for c in cs}
    assert shape(A.CASES_G) == {(1, 1, 1), (2, 33, 40), (1, 63, 63), (3, 64, 64), (2, 65, 65), (1, 100, 127), (2, 255, 129), (1, 257, 192), (3, 300, 520), (2, 520, 300),
                                (1, 40, 1000)}
    assert shape(A.CASES_G_KB) == {(2, 65, 65), (3, 300, 520), (2, 520, 300)} and all(c["kb"] == 3.0 and c["period"] == 0 for c in A.CASES_G_KB)
    assert {(c["period"], c["Sk"]) for c in A.CASES_G_PER} == {(1, 192), (2, 320), (3, 520), (5, 256)} and all(c["kb"] == 3.0 for c in A.CASES_G_PER)
    assert any((c["H"], c["Sq"], c["Sk"], c["ramp"]) == (2, 256, 1536, 6.0) for c in A.CASES_G_RAMP)
    assert {(c["blk_rows"], c["Sk"], c["kb"]) for c in A.CASES_BLK} == {(b, n, kb) for b in (64, 128) for n in (256, 384) for kb in (0.0, 3.0)} and all(c["H"] == 2 for c in A.CASES_BLK)
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "unitex_amd", "csrc", "attention_q64_asm.inc")).read()
    assert int(re.search(r"#define AQ2_NSLOT (\d+)", text).group(1)) == A.NSLOT
    assert shape(A.CASES_Q64) == {(1, 64, 64), (3, 128, 128), (2, 1, 192), (2, 100, 256), (1, 320, 320), (2, 448, 64 * (A.NSLOT + 1)), (2, 520, 256)}
    assert all(c["kb"] == 3.0 for c in A.CASES_Q64_KB) and {(c["H"], c["Sq"], c["Sk"], c["ramp"]) for c in A.CASES_Q64_RAMP} == {(2, 200, 1024, r) for r in (45.0, 110.0, 150.0)}
    assert all(c["H"] * c["Sq"] * c["Sk"] <= 6e7 for c in A.CASES) and len({c["name"] for c in _ALL}) == len(_ALL)
    # the key-split shapes at the MI355X's 256 CUs, as the case list states them
    cs = {c["name"]: c for c in A.split_cases(256)}
    assert all((c["H"], c["Sq"]) == (129, 300) for c in cs.values())
    assert {c["Sk"] for c in cs.values()} == {1472, 1500, 2176} and cs["split_k1472_per4"]["period"] == 4 and cs["split_k1472_kb3"]["kb"] == 3.0
    assert A.split_plan(129, 300, 1472, 256) == [258, 256, 2, 12] and A.split_plan(129, 300, 1500, 256) == [258, 256, 2, 12]
    assert A.split_plan(129, 300, 2176, 256) == [258, 256, 3, 12]                  # 34 tiles: 12 + 12 + 10
    assert A.split_plan(129, 300, 1472, 256, tailsplit=False)[2] == 1
    for c in _SPLIT:
        assert (_plan(c)[2] > 1) == bool(c["tailsplit"]), c["name"]


def test_split_plan_is_the_librarys():
    from unitex_amd import _lib
    lib = _lib.load_library()
    out = (C.c_int * 4)()
    for H, Sq, S, ncu in [(129, 300, 1472, 256), (129, 300, 1500, 256), (129, 300, 2176, 256), (5, 300, 1472, 8), (5, 300, 2176, 8), (24, 2830, 2830, 256), (24, 4096, 4096, 256),
                          (3, 50688, 50688, 256), (2, 256, 1536, 256), (153, 300, 1472, 304), (41, 300, 9000, 80)]:
        assert lib.utx_attn_plan(H, Sq, S, ncu, C.byref(out)) == 0
        assert list(out) == A.split_plan(H, Sq, S, ncu), (H, Sq, S, ncu, list(out))


# the cases that are there for each defect: (name, softmax_scale)
_DEFECT_CASES = {
    "ragged_mask_one_group_short": (("g_h2_q33_k40", 0.0), ("g_h1_q63_k63", A.SCALE), ("g_h2_q65_k65", 0.0), ("g_h3_q300_k520", 0.0), ("split_k1500_ragged", 0.0)),
    "pad_keys_unmasked": (("g_h2_q33_k40", A.SCALE), ("g_h1_q100_k127", 0.0), ("g_h2_q520_k300", 0.0)),
    "key_bias_on_tile_1": (("g_kb3_h2_q65_k65", 0.0), ("g_kb3_h3_q300_k520", A.SCALE), ("q64_kb3_h2_q520_k256", 0.0), ("blk64_k256_kb3", 0.0), ("split_k1472_kb3", 0.0)),
    "periodic_bias_on_local_tile": (("split_k1472_per5", 0.0),),      # (period 4 divides the 12 tiles of a range: there the mistake changes nothing)
    "p_groups_swapped": (("g_h3_q64_k64", 0.0), ("g_h2_q33_k40", A.SCALE), ("q64_h2_q100_k256", 0.0)),
    "no_o_rescale": (("g_ramp45", 0.0), ("g_ramp45", A.SCALE), ("q64_ramp110", 0.0)),
    "merge_drops_last_range": (("split_k1472", 0.0), ("split_k%d_short_last_range" % A.short_last_range_sk(NCU // 2 + 1, 300, NCU), 0.0)),
    "merge_weights_base_e": (("split_k1472", 0.0), ("split_k1500_ragged", 0.0)),
    "wave_rows_32_off": (("g_h2_q65_k65", 0.0), ("g_h1_q100_k127", A.SCALE), ("q64_h1_q320_k320", 0.0)),
    "drop_last_full_tile": (("g_h3_q64_k64", 0.0), ("g_h1_q257_k192", A.SCALE), ("q64_h2_q448_k256", 0.0), ("split_k1472", 0.0)),
}


def test_the_defect_list_is_the_oracles():
    assert set(_DEFECT_CASES) == set(A.DEFECTS) and len(A.DEFECTS) == 10


@pytest.mark.parametrize("defect,name,scale", [(d, n, s) for d in A.DEFECTS for n, s in _DEFECT_CASES[d]])
def test_defect_is_rejected(defect, name, scale):
    case, inp, plan, ref = _case_data(name, scale)
    bad = ~A.accepted(A.emulate(case, inp, scale, plan, defect), ref)
    print("%s at %s (scale %.4f): %d of %d elements rejected" % (defect, name, scale, int(bad.sum()), bad.size))
    assert bad.any(), "%s: the acceptance check does not see the defect `%s`" % (name, defect)


@pytest.mark.parametrize("name", ["g_h2_q33_k40", "g_kb3_h3_q300_k520", "g_per3_k520", "g_ramp45", "q64_ramp150", "q64_h2_q448_k256"])
def test_reference_with_reversed_keys_lies_inside_its_interval(name):
    case, inp, _, ref = _case_data(name, 0.0)
    n = case["Sk"]
    for h in range(case["H"]):
        rev = A.attention64(inp["q"][h], inp["k"][h, :n], inp["v"][h, :n], 0.0, case["kb"], case["period"], reverse=True)[0]
        assert ((A.bf16(rev) >= ref.lo[h]) & (A.bf16(rev) <= ref.hi[h])).all(), (name, h)


def test_interval_arithmetic_on_a_hand_computed_row():
    """two keys, q . k = 1 and 0 in base-2 units: weights 2 / 3 and 1 / 3; v = 1.5 and 3 -> 2 exactly; with the multiplicity 2^1 on tile 0 both keys carry it: unchanged.
    E = (1 + 2^-7) (E_w + r A) with r just above 2^-8 (a handful of 2^-23 units at two keys): between 2^-8 and 2^-7 of the value"""
    q = np.zeros((1, 128)); q[0, 0] = 1.0
    k = np.zeros((2, 128)); k[0, 0] = 1.0
    v = np.zeros((2, 128)); v[0, :] = 1.5; v[1, :] = 3.0
    for kb in (0.0, 1.0):
        ref, Aabs, E, W, M, s0, s1 = A.attention64(q, k, v, 0.0, kb)
        assert abs(ref[0, 0] - 2.0) < 1e-15 and abs(W[0, 0] - 2.0 / 3) < 1e-15 and Aabs[0, 0] == ref[0, 0] and (s0, s1) == (kb, 1.0 + kb)
        assert 2.0 ** -8 < E[0, 0] / 2.0 < 2.0 ** -7
    assert A.c_of(0.0) == 1.0 and abs(A.c_of(A.SCALE) - 1.4426950408889634 / np.sqrt(128.0)) < 1e-8
    assert A._bias(200, 3.0, 0).tolist() == [3.0] * 64 + [0.0] * 136 and A._bias(260, 3.0, 2)[[0, 64, 128, 192, 256]].tolist() == [3.0, 0.0, 3.0, 0.0, 3.0]

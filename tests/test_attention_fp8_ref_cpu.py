"""oracle/attention_fp8_fp64.py audited on the CPU: for every input set that tests/test_attention_fp8_edges_gpu.py sends to the GPU,
  (a) a float32 numpy emulation of csrc/attention_fp8.hip (64-key tiles, the sum check at 256 per lane with wave-wide re-centring, l from the unrounded p, P through the
      float8_e4m3fn cast, PV of the dequantised V, the key split and its merge) lies inside the counted interval at EVERY element;
  (b) the conditions on the inputs hold on the reference alone: median E / |ref| <= 1.25 * 2^-4 outside the ramp cases, at most 5 % of the elements with a flush term above their
      2^-4 term, target weights in [0.25, 0.75], every unchosen key >= 20 base-2 units below its row's maximum, >= 3 distinct scale bytes of each kind, key coverage;
  (c) the emulation fails the same acceptance check with each of fifteen mistakes, at the cases that are there for that mistake.
The key-split cases depend on the CU count: this module runs them at 8 CUs (H = 5), like tests/test_attention_ref_cpu.py."""
import numpy as np
import pytest

from oracle import attention_fp64 as A
from oracle import attention_fp8_fp64 as F

NCU = 8
_SPLIT = F.split_cases(NCU)
_ALL = F.CASES + _SPLIT
_BY_NAME = {c["name"]: c for c in _ALL}
_CACHE = {}
CAP = 1.25 * 2.0 ** -4


def _plan(case):
    return A.split_plan(case["H"], case["Sq"], case["Sk"], NCU, bool(case["tailsplit"])) if case["kernel"] == "split" else None


def _case_data(name):
    """(case, inputs, plan, reference, flush share) -- built once and shared, never modified"""
    if name not in _CACHE:
        case = _BY_NAME[name]
        inp, plan = F.make_inputs(case), _plan(case)
        ref, share = F.reference(case, inp, None if plan is None else A.split_rows(case, plan))
        _CACHE[name] = (case, inp, plan, ref, share)
    return _CACHE[name]


@pytest.mark.parametrize("name", [c["name"] for c in _ALL])
def test_correct_emulation_is_accepted_and_the_inputs_are_sharp(name):
    case, inp, plan, ref, share = _case_data(name)
    H, Sq, n = case["H"], case["Sq"], case["Sk"]
    assert ref.out.shape == (H, Sq, 128) and (ref.lo <= ref.out).all() and (ref.out <= ref.hi).all()
    med, mx = A.rel_width(ref)
    wt = ref.wt[~np.isnan(ref.wt)]
    counts = F.byte_counts(case, inp)
    gap = F.rest_gap(case, inp)
    stats = {}
    got = F.emulate(case, inp, plan, None, stats)
    print("%-34s E / |ref| median %.4f = %.3f x 2^-4, max %.4f  flush-dominated elements %.3f %%  target weight [%s]  rest >= %.1f units below  keys aimed at %.0f %%  "
          "base-2 scores [%.1f, %.1f]  distinct bytes (qs row, ks row, ks column, vs key blocks, vs channel blocks) %s  re-centres asked by the sum check %d  plan %s" % (
              name, med, med * 16, mx, 100 * share, "%.3f, %.3f" % (wt.min(), wt.max()) if wt.size else "no addressed rows", gap, 100 * A.coverage(inp, n),
              ref.smin, ref.smax, counts[:5], stats.get("recentres", 0), plan))
    if case["ramp"] == 0:
        assert med <= CAP, "%s: median E / |ref| = %.4f" % (name, med)
    assert share <= 0.05, "%s: %.2f %% of the elements have a flush term above their 2^-4 term" % (name, 100 * share)
    if case["ramp"] == 0 and n > 1:
        assert wt.size and wt.min() >= 0.25 and wt.max() <= 0.75, "%s: target weights [%g, %g]" % (name, wt.min(), wt.max())
        assert gap >= 20.0, "%s: a key outside the chosen ones is only %.2f units below the maximum" % (name, gap)
        if int((inp["tgt"] >= 0).sum()) >= 2 * n + 64:
            assert A.coverage(inp, n) == 1.0, name
    # scale bytes: the four of a Q row and of a K row; V^T's over the key blocks (where there are three) and over the four channel blocks; neighbouring blocks and tiles differ
    qrow, krow, _, vkb, vcb, neigh = counts
    assert qrow >= 3 and krow >= 3 and vcb >= 3 and neigh, "%s: %s" % (name, counts)
    if (n + 63) // 64 * 2 >= 3:
        assert vkb >= 3, "%s: %s" % (name, counts)
    # the pad region and the rows past S_q are hostile and finite
    npad = inp["k8"].shape[1]
    for key in ("q8", "k8", "v8t"):
        assert not np.isin(inp[key], (0x7F, 0xFF)).any(), key
    for key in ("qs", "ks", "vs"):
        assert not (inp[key] == 0xFF).any(), key
    if npad > n:
        assert (np.abs(inp["kd"][:, n:]).max(-1) > 0).all() and (np.sign(inp["vd"][:, n:]) == -np.sign(inp["vd"][:, :1])).all()
    if npad > Sq:
        assert (inp["q8"][:, Sq:] == 0x7E).all() and (inp["qs"][:, Sq:] == 0xF0).all()
    if name == "f8_ramp3":
        assert stats.get("recentres", 0) == 0, "a ramp of 3 base-2 units must stay below the sum check"
    if name in ("f8_ramp6", "f8_ramp45"):
        assert stats["recentres"] > (0 if name == "f8_ramp6" else 100)
    msg = A.first_offender(got, ref, inp, name + " (float32 emulation)", plan)
    assert msg is None, msg


def test_edge_keys_are_aimed_at_from_every_wave_slice():
    for name in ("f8_h3_q300_k520", "f8_h2_q257_k300", "f8_h1_q192_k192"):
        case, inp, _, _, _ = _case_data(name)
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
        # companions: other 32-key blocks, and other tiles where the family period allows
        ch = inp["chosen"][inp["kind"] == "a"]
        have = ch[:, 1:] >= 0                                   # a family has four or five members
        assert have[:, :3].all() and (((ch[:, 1:] // 32) != (ch[:, :1] // 32)) | ~have).all()
        if F.family_period(n) >= 64:
            assert (((ch[:, 1:] // 64) != (ch[:, :1] // 64)) | ~have).all()


def test_every_listed_shape_and_option_is_among_the_cases():
    shape = lambda cs: {(c["H"], c["Sq"], c["Sk"]) for c in cs}
    assert shape(F.CASES_G) == {(1, 1, 1), (2, 33, 40), (1, 63, 63), (3, 64, 64), (2, 65, 65), (1, 100, 127), (2, 129, 129), (1, 192, 192), (3, 300, 520), (2, 257, 300), (1, 40, 1000)}
    assert len(F.CASES_KB) == 3 and all(c["kb"] == 3.0 and c["period"] == 0 for c in F.CASES_KB)
    assert {(c["period"], c["Sk"]) for c in F.CASES_PER} == {(1, 192), (2, 320), (3, 520), (5, 256)} and all(c["kb"] == 3.0 and c["Sq"] <= c["Sk"] for c in F.CASES_PER)
    assert {(c["H"], c["Sq"], c["Sk"], c["ramp"]) for c in F.CASES_RAMP} == {(2, 256, 1536, r) for r in (3.0, 6.0, 45.0)}
    assert all(c["Sq"] <= c["Sk"] for c in _ALL) and len({c["name"] for c in _ALL}) == len(_ALL)
    cs = {c["name"]: c for c in F.split_cases(256)}
    assert all((c["H"], c["Sq"]) == (129, 300) for c in cs.values()) and {c["Sk"] for c in cs.values()} == {1472, 1500, 2176}
    assert cs["f8_split_k1472_per4"]["period"] == 4 and cs["f8_split_k1472_per5"]["period"] == 5 and cs["f8_split_k1472_kb3"]["kb"] == 3.0
    assert cs["f8_nosplit_k1472"]["tailsplit"] == 0 and cs["f8_nosplit_k1472"]["data"] == cs["f8_split_k1472"]["data"]
    for c in _SPLIT:
        assert (_plan(c)[2] > 1) == bool(c["tailsplit"]), c["name"]


_SHORT = "f8_split_k%d_short_last_range" % A.short_last_range_sk(NCU // 2 + 1, 300, NCU)
_DEFECT_CASES = {
    "ragged_mask_without_16_lh": ("f8_h2_q33_k40", "f8_h1_q63_k63", "f8_h2_q65_k65", "f8_h3_q300_k520", "f8_split_k1500_ragged"),
    "pad_keys_unmasked": ("f8_h2_q33_k40", "f8_h1_q100_k127", "f8_h2_q257_k300"),
    "key_bias_on_tile_1": ("f8_kb3_h2_q65_k65", "f8_kb3_h3_q300_k520", "f8_split_k1472_kb3"),
    "periodic_bias_on_local_tile": ("f8_split_k1472_per5",),
    "p_groups_swapped": ("f8_h3_q64_k64", "f8_h2_q33_k40", "f8_h1_q40_k1000"),
    "no_o_rescale": ("f8_ramp45", "f8_ramp6"),
    "pv_under_this_tiles_v_scales": ("f8_h2_q65_k65", "f8_h2_q129_k129", "f8_h3_q300_k520"),
    "block1_under_block0_k_scales": ("f8_h2_q33_k40", "f8_h3_q64_k64", "f8_h3_q300_k520"),
    "upper_half_qs_not_shifted": ("f8_h2_q33_k40", "f8_h3_q64_k64", "f8_h2_q257_k300"),
    "vs_read_transposed": ("f8_h1_q1_k1", "f8_h3_q64_k64", "f8_h1_q192_k192"),
    "split_scales_not_advanced": ("f8_split_k1472", "f8_split_k1500_ragged"),
    "prefetched_scales_stuck_at_tile_0": ("f8_h2_q65_k65", "f8_h1_q192_k192", "f8_ramp45"),
    "drop_last_full_tile": ("f8_h3_q64_k64", "f8_h1_q192_k192", "f8_split_k1472"),
    "merge_drops_last_range": ("f8_split_k1472", _SHORT),
    "wave_rows_32_off": ("f8_h2_q65_k65", "f8_h1_q100_k127"),
}


def test_the_defect_list_is_the_oracles():
    assert set(_DEFECT_CASES) == set(F.DEFECTS) and len(F.DEFECTS) == 15


@pytest.mark.parametrize("defect,name", [(d, n) for d in F.DEFECTS for n in _DEFECT_CASES[d]])
def test_defect_is_rejected(defect, name):
    case, inp, plan, ref, _ = _case_data(name)
    bad = ~A.accepted(F.emulate(case, inp, plan, defect), ref)
    print("%s at %s: %d of %d elements rejected" % (defect, name, int(bad.sum()), bad.size))
    assert bad.any(), "%s: the acceptance check does not see the defect `%s`" % (name, defect)


@pytest.mark.parametrize("name", ["f8_h2_q33_k40", "f8_kb3_h3_q300_k520", "f8_per3_k520", "f8_ramp45"])
def test_reference_with_reversed_keys_lies_inside_its_interval(name):
    case, inp, _, ref, _ = _case_data(name)
    n = case["Sk"]
    for h in range(case["H"]):
        rev = F.attention64(inp["qd"][h], inp["kd"][h, :n], inp["vd"][h, :n], case["kb"], case["period"], reverse=True)[0]
        assert ((A.bf16(rev) >= ref.lo[h]) & (A.bf16(rev) <= ref.hi[h])).all(), (name, h)


def test_interval_arithmetic_on_hand_computed_rows():
    """two keys, q . k = 1 and 0: weights 2 / 3 and 1 / 3, v = 1.5 and 3 -> 2; E_p = 2^-4 * 2.  A third key 12 units down (weight ~ 2^-12 / 1.5 < 2^-10 W_max): its flush term is
    its whole weight, not 2^-4 of it.  One at 8 units down (2^-8 > 2^-10): min(W, 2^-10 W_max) = 2^-10 W_max, still above 2^-4 W."""
    q = np.zeros((1, 128)); q[0, 0] = 1.0
    k = np.zeros((2, 128)); k[0, 0] = 1.0
    v = np.zeros((2, 128)); v[0, :] = 1.5; v[1, :] = 3.0
    ref, Aabs, Ep, Er, W, M, fl, t4, s0, s1 = F.attention64(q, k, v)
    assert abs(ref[0, 0] - 2.0) < 1e-15 and abs(Ep[0, 0] - 2.0 ** -4 * 2.0) < 1e-15 and 0 < Er[0, 0] < 2.0 ** -12
    for down, want in ((12.0, lambda w, wm: w), (8.0, lambda w, wm: 2.0 ** -10 * wm)):
        k3 = np.zeros((3, 128)); k3[0, 0] = 1.0; k3[2, 0] = 1.0 - down
        v3 = np.concatenate([v, np.full((1, 128), 5.0)])
        ref, Aabs, Ep, Er, W, M, fl, t4, s0, s1 = F.attention64(q, k3, v3)
        assert abs(Ep[0, 0] - (2.0 ** -4 * (W[0, 0] * 1.5 + W[0, 1] * 3.0) + want(W[0, 2], W[0, 0]) * 5.0)) < 1e-15
    assert F.units(64) == (131, 2, A.U23 * (65 + 66 + 2)) and F.units(65)[:2] == (133, 3)
    # the conversion the interval is about: round to nearest even, gradual underflow, ties at 2^-10 to zero
    p = np.array([1.0625, 1.0626, 1.1875, 2.0 ** -10, 2.0 ** -10 * 1.001, 2.0 ** -9 * 1.49, 2.0 ** -9 * 1.5, 300.0], dtype=np.float32)
    assert F._e4(p).tolist() == [1.0, 1.125, 1.25, 0.0, 2.0 ** -9, 2.0 ** -9, 2.0 ** -8, 288.0]


def test_quantiser_edge_rows_hold_every_listed_block():
    x = F.quant_edge_rows(128, 64, 3).float()
    b = x.view(128, 2, 32)
    amax = b.abs().amax(-1)
    assert (amax == 0).any() and (amax == 4.0).any() and (amax == 3.984375).any() and ((amax > 0) & (amax < 2.0 ** -126)).any() and (amax >= 2.0 ** 120).any()
    assert (amax == 448.0).any() and (torch_signbit(x) & (x == 0)).any() and torch_isfinite(x)


def torch_signbit(x):
    import torch
    return torch.signbit(x)


def torch_isfinite(x):
    import torch
    return bool(torch.isfinite(x).all())

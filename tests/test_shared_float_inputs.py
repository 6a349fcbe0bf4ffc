"""CPU preconditions of test_gpu_shared_float.py (shared_float_cases.py), in the pattern of test_float_hops_inputs.py.  No GPU:
numpy, the float64 reference, and the library's two sizing helpers (the library loads without a GPU).

1. Every case meets the generator's conditions from the reference alone: spread attention (among the (query, hop) pairs with
   S >= 8 at least three quarters have 1 / sum p^2 >= 4, every hop index has one) and at most 1 % of the columns `near` a step.
2. The stated cases are there: every tile-edge length at every padded width, every batch size of every forced tile, the switches,
   the special memories; every case is ONE memory repeated.
3. qmann_hops_shared_float_lds_bytes / _tile against the formula and the cap: the largest accepted length is 38 368.
4. The comparison used on the GPU accepts a correct float32 read-out and REPORTS three faults of a shared-plane kernel: query t
   carrying query t - 1's read-out, the last row's weight dropped, a spare place of a short tile written into the guard.
"""
import numpy as np
import pytest

import float_hop_ref as ref
import float_hops_cases as fc
import shared_float_cases as sf
from conftest import load_pkg
from shared_float_cases import CASES, FAMILIES, build, reference_chain


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_meets_the_spread_and_near_conditions(name):
    case = build(name)
    share, per_hop, near = fc.conditions(case, reference_chain(name))
    print(f"{name}: 1/sum p^2 >= 4 in {100 * share:.1f} % of the (query, hop) pairs with S >= 8; near share {100 * near:.3f} %")
    assert case.max_slots <= 769 and case.B <= 19
    assert near <= fc.NEAR_SHARE, f"{name}: {100 * near:.2f} % of the columns are near a step"
    if case.exempt_spread:                       # +-127 everywhere: one-hot by construction, and it says so
        assert name == "sf_all_127"
        return
    if case.max_slots >= fc.SPREAD_MIN_SLOTS:    # (shorter memories have no pair the condition speaks of)
        assert share >= fc.SPREAD_SHARE, f"{name}: spread in {share:.2f} of the pairs"
        assert all(per_hop), f"{name}: a hop index without one spread query {per_hop}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_is_one_memory_repeated(name):
    case = build(name)
    S, B = case.max_slots, case.B
    mk, mv = sf.memory(case)
    assert np.array_equal(case.row_off, np.arange(B + 1) * S) and case.R == B * S
    assert np.array_equal(case.kb, np.tile(mk, (1, B, 1))) and np.array_equal(case.vb, np.tile(mv, (1, B, 1)))
    D, Dp = case.cfg["dim_emb"], case.kb.shape[2]
    assert Dp == fc.pad_dim(D) and not mk[:, :, D:].any() and not mv[:, :, D:].any(), "pad columns must be zero"
    assert len({case.u0[q].tobytes() for q in range(B)}) == B or name == "sf_all_127", "the questions differ"
    assert name not in fc.CASES                  # (check_outputs would take that module's chain for it)


def test_the_stated_cases_are_present():
    by = lambda fam: [build(n) for n in FAMILIES[fam]]
    for D in (60, 128, 200):
        T = fc.tile_rows(fc.pad_dim(D))
        got = {c.max_slots for c in by("tile_edges") if c.cfg["dim_emb"] == D}
        assert got >= {1, T - 1, T, T + 1, 4 * T + 1, 12 * T + 1} and got == set(fc.tile_edge_slots(fc.pad_dim(D)))
    assert {c.cfg["dim_emb"] for c in by("tile_edges")} == {20, 60, 128, 200}
    assert all(c.B == 5 for c in by("tile_edges"))
    batches = {c.B for c in by("batches") if c.cfg["dim_emb"] == 60}
    for qt in sf.TILES:
        assert {1, qt, qt + 1, 2 * qt + 3} <= batches
        assert qt == 1 or any(b % qt for b in batches), "a short last tile"
    assert {c.kb.shape[2] for c in by("batches") if c.B == 19} == {64, 128, 256}
    sw = {n: build(n).cfg for n in FAMILIES["switches"]}
    assert {c["softmax_variant"] for c in sw.values()} == {0, 1, 2}
    assert sw["sf_shift_pow2"]["softmax_shift_based"] and sw["sf_shift_exp"]["softmax_shift_based"]
    assert [np.sign(s) for s in sw["sf_scale_negative"]["att_scale"]] == [-1, 1, -1]
    assert sw["sf_binary_u"]["fmt_bin"] == (0, 0) and sw["sf_no_lin_map"]["en_lin_map"] is False and build("sf_no_lin_map").lin is None
    assert sw["sf_unscaled"].get("att_scale") is None
    for n in ("sf_relu_exp", "sf_relu_pow2", "sf_relu_plan"):       # the RELU changes something: a negative state enters a later hop
        assert sw[n]["en_non_lin"] and any((hp.u_next < 0).any() for hops in reference_chain(n) for hp in hops[:-1])
    draws = [c for n, c in sw.items() if n.startswith("sf_formats_")]
    assert len({(tuple(c["fmt"]), tuple(c["fmt_w"])) for c in draws}) == len(draws) >= 6
    assert any(len(set(c["fmt"])) > 1 or len(set(c["fmt_w"])) > 1 for c in draws), "per-hop formats"
    tied = build("sf_tied")
    assert tied.tied and tied.kb.shape[0] == 1 and sf.untied(tied).kb.shape[0] == 3


def test_special_memories():
    D = lambda c: c.cfg["dim_emb"]
    for n in ("sf_mz_sprinkled", "sf_mz_words"):
        case, ch = build(n), reference_chain(n)
        mk, mv = sf.memory(case)
        assert (mk[:, :, :D(case)] == 0x80).sum() >= 100 and (mv[:, :, :D(case)] == 0x80).sum() >= 100
        S, n_w = case.max_slots, 0
        for q in range(case.B):                  # 0x80 value bytes on rows that carry weight
            for h, hp in enumerate(ch[q]):
                rows = np.nonzero(hp.p >= 0.25 / S)[0]
                n_w += int((mv[h, rows, :D(case)] == 0x80).sum())
        assert n_w >= 100
    case, ch = build("sf_all_127"), reference_chain("sf_all_127")
    mk, mv = sf.memory(case)
    assert np.isin(mk[:, :, :D(case)], (0x7F, 0xFF)).all() and np.isin(mv[:, :, :D(case)], (0x7F, 0xFF)).all()
    assert (np.abs(ref.on_grid_codes(case.u0, case.cfg["fmt_w"][0])) == 127).all()
    case, ch = build("sf_equal_scores"), reference_chain("sf_equal_scores")
    for q in range(case.B):
        for hp in ch[q]:
            assert (hp.codes == hp.codes[0]).all() and np.allclose(hp.p, 1.0 / case.max_slots, rtol=1e-12)
    case, ch = build("sf_two_maxima"), reference_chain("sf_two_maxima")
    a, b = case.marks["pairs"][0]
    c0 = ch[0][0].codes
    assert c0[a] == c0[b] == c0.max() and (c0 == c0.max()).sum() == 2, "question 0: two equal maxima at hop 0"
    assert all(hp.codes[a] == hp.codes[b] for q in range(case.B) for hp in ch[q]), "a tie for every question"


# ---- 3. the sizing helpers ---------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    load_pkg()
    import qmann_amd.abi as abi
    return abi.lib


def test_lds_helper_follows_the_formula(lib):
    fixed = lib.qmann_hops_lds_bytes(0)
    assert fixed == 9344 and fixed % 16 == 0
    for S in (1, 3, 4, 5, 64, 769, 1000, 2752, 2753, 10000, sf.CAP_SLOTS, sf.CAP_SLOTS + 1, 100000):
        for qt in (1, 2, 4, 8):
            assert lib.qmann_hops_shared_float_lds_bytes(S, qt) == qt * (fixed + (4 * S + 15) // 16 * 16)
            assert sf.fits(S, qt) == (lib.qmann_hops_shared_float_lds_bytes(S, qt) <= 160 * 1024 - 1024)


def test_tile_helper_follows_the_cap(lib, monkeypatch):
    limit = 160 * 1024 - 1024
    assert lib.qmann_hops_shared_float_lds_bytes(sf.CAP_SLOTS, 1) <= limit < lib.qmann_hops_shared_float_lds_bytes(sf.CAP_SLOTS + 1, 1)
    many = 1 << 20                               # enough questions to give every compute unit a tile of 8
    try:
        for forced in (None, 1, 2, 4, 8):
            if forced:
                monkeypatch.setenv("QMANN_SHARED_QT", str(forced))
            else:
                monkeypatch.delenv("QMANN_SHARED_QT", raising=False)
            lib.qmann_tuning_reload()
            assert lib.qmann_hops_shared_float_tile(sf.CAP_SLOTS, many) == 1, "the largest accepted length is 38 368"
            assert lib.qmann_hops_shared_float_tile(sf.CAP_SLOTS + 1, many) == 0, "one more slot does not fit"
            assert lib.qmann_hops_shared_float_tile(0, many) == 0 and lib.qmann_hops_shared_float_tile(100, 0) == 0
            for S in (1, 200, 1000, 2752, 2753, 10000, 19184, 19185):
                fit = max(qt for qt in (1, 2, 4, 8) if sf.fits(S, qt))
                got = lib.qmann_hops_shared_float_tile(S, many)
                assert got in (1, 2, 4, 8) and got <= fit
                if forced:
                    assert got == min(forced, fit)
                else:
                    assert got == 1, "the launcher's own choice, by measurement (DESIGN.md section 5): one query per workgroup"
                assert lib.qmann_hops_shared_float_tile(S, 1) == (min(forced, fit) if forced else 1), "one question: one per workgroup"
        assert max(qt for qt in (1, 2, 4, 8) if sf.fits(10000, qt)) == 2 and sf.fits(2752, 8) and not sf.fits(2753, 8)
    finally:
        monkeypatch.delenv("QMANN_SHARED_QT", raising=False)
        lib.qmann_tuning_reload()


# ---- 4. the comparison routine ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sf_d60_s65", "sf_batch_19_d128", "sf_mz_words", "sf_relu_plan", "sf_formats_03"])
def test_comparison_accepts_a_correct_float32_read_out(name):
    case = build(name)
    stats = fc.check_outputs(case, sf.simulate(case))
    assert stats["cols"] > 0 and stats["differ"] <= stats["near"]


@pytest.mark.parametrize("fault,name,told", [("neighbour", "sf_batch_05", "o "), ("neighbour", "sf_batch_19_d200", "o "),
                                             ("last_row", "sf_d60_s65", "o "), ("last_row", "sf_d200_s193", "o "),
                                             ("spare", "sf_batch_03", "guard of u_out"), ("spare", "sf_d128_s33", "guard of u_out")])
def test_comparison_reports_each_fault(fault, name, told):
    case = build(name)
    with pytest.raises(AssertionError, match=told):
        fc.check_outputs(case, sf.simulate(case, fault=fault))

"""CPU preconditions of test_gpu_attended_float.py: conditions on the INPUTS of attended_float_cases.py, from the float64
reference (float_hop_ref.py) and the integer scores alone.  No kernel runs here."""
import numpy as np
import pytest

import attended_float_cases as af
import float_hops_cases as fc
from attended_cases import PAD_SLOT, want_rows
from attended_float_cases import KS, SHARED, STORY, build, family, reference_p


def _tied_across(p, k):
    """does the k-th place of the order tie with the (k + 1)-th (equal floats; two NaN tie as well)"""
    if p.size <= k:
        return False
    order = np.lexsort((np.arange(p.size), -p))
    a, b = p[order[k - 1]], p[order[k]]
    return bool(a == b or (np.isnan(a) and np.isnan(b)))


# ---- the tie families tie ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n in SHARED if family(n) == "mirrored"))
def test_mirrored_memories_cut_a_pair_at_every_odd_k(name):
    case = build(name)
    half = case.marks["mirrored"]
    mk, mv = af.sf.memory(case)
    assert np.array_equal(mk[:, :half], mk[:, half:]) and np.array_equal(mv[:, :half], mv[:, half:])
    for hops in reference_p(name):
        for p in hops:
            assert np.array_equal(p[:half], p[half:])
            for k in (1, 5):
                assert _tied_across(p, k), f"{name}: k = {k} cuts a pair"


@pytest.mark.parametrize("name", sorted(n for n in SHARED if family(n) in ("constant", "zero_scale")))
def test_constant_probabilities_answer_the_first_k_slots(name):
    case = build(name)
    S = case.max_slots
    for hops in reference_p(name):
        for p in hops:
            assert len(set(p.tolist())) == 1 and p[0] > 0
            for k in KS:
                assert _tied_across(p, k)
                slot, _ = want_rows(p[None, None, :], k)
                assert slot[0, 0].tolist() == list(range(min(k, S)))


@pytest.mark.parametrize("name", sorted(n for n in SHARED if family(n) == "underflow"))
def test_underflow_leaves_fewer_than_k_probabilities(name):
    for hops in reference_p(name):
        for p in hops:
            n = int((p > 0).sum())
            assert 1 <= n < 5 and not np.isnan(p).any(), "k = 5 and 16 fill up with zeros"
            for k in (5, 16):
                assert _tied_across(p, k)
                slot, _ = want_rows(p[None, None, :], k)
                zeros = [s for s in slot[0, 0].tolist() if p[s] == 0]
                assert zeros == sorted(zeros) and zeros == [s for s in range(p.size) if p[s] == 0][:k - n]


def test_a_nan_probability_is_reachable_in_float_attention():
    """the shift-based normaliser of the e^x base divides by llrint(log2(total)): 0 for a total below sqrt 2"""
    case = build("af_nan")
    assert case.cfg["n_hop"] == 1 and case.cfg["softmax_shift_based"] and case.cfg["softmax_variant"] == 0
    for hops in reference_p("af_nan"):
        p = hops[0]
        n_inf = int(np.isposinf(p).sum())
        assert 1 <= n_inf < 5 and int(np.isnan(p).sum()) == p.size - n_inf
        for k in (5, 16):
            assert _tied_across(p, k)
            slot, _ = want_rows(p[None, None, :], k)
            got = slot[0, 0].tolist()
            assert all(np.isposinf(p[s]) for s in got[:n_inf])
            assert got[n_inf:] == [s for s in range(p.size) if np.isnan(p[s])][:k - n_inf], "NaN below every number, lowest slot first"


# ---- the ordinary cases decide by value -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n in list(SHARED) + list(STORY) if af.ordinary(n)))
def test_ordinary_cases_have_distinct_first_places(name):
    share = af.distinct_share(name)
    assert share >= af.DISTINCT_SHARE, f"{name}: {share:.2f} of the rows have {af.DISTINCT_PLACES} distinct first places: replace the seed"


def test_the_exempt_cases_are_few_and_named():
    assert set(af.GRID_TIES) <= set(SHARED) and len(af.GRID_TIES) == 5
    assert all(af.distinct_share(n) < af.DISTINCT_SHARE for n in af.GRID_TIES), "a case that meets the share is an ordinary one"


# ---- coverage ------------------------------------------------------------------------------------------------------------------------
def test_slot_counts_batches_and_k_cover_the_edges():
    slots = {build(n).max_slots for n in SHARED}
    assert set(af.SLOT_COUNTS) <= slots and 4097 in slots and af.CAP_SLOTS in slots
    for D in (60, 128, 200):
        got = {build(n).max_slots for n in SHARED if family(n) == "tile_edges" and build(n).cfg["dim_emb"] == D}
        assert got == set(fc.tile_edge_slots(fc.pad_dim(D)))
    cap = build("af_cap")
    assert (cap.max_slots, cap.cfg["dim_emb"], cap.B) == (38368, 60, 2) and af.sf.fits(38368, 1) and not af.sf.fits(38369, 1)
    batches = {build(n).B for n in SHARED if family(n) == "batches"}
    for qt in af.TILES:
        assert {1, qt, qt + 1, 2 * qt + 3} <= batches
        assert (qt + 1) % qt == 1 % qt and (2 * qt + 3) % qt == 3 % qt      # short last tiles of one and of three (for qt > 3)
    assert KS == (1, 5, 16) and any(s < k for s in slots for k in KS), "k > S occurs"
    # the per-story call's own ground
    lens = [int(x) for n in STORY for x in np.diff(build(n).row_off)]
    assert 0 in lens and any(build(n).max_slots < np.diff(build(n).row_off).max() for n in STORY), "an empty story and a cut one"
    mixed = build("afs_mixed")
    assert len(set(np.diff(mixed.row_off).tolist())) >= 8
    assert build("af_tied").tied and build("afs_tied").tied
    assert any(v.get("scale_signs") for v in SHARED.values())
    bases = {(build(n).cfg.get("softmax_variant", 0), bool(build(n).cfg.get("softmax_shift_based"))) for n in SHARED}
    assert {(0, False), (1, False), (2, False), (0, True), (1, True)} <= bases


# ---- the yardstick's order -------------------------------------------------------------------------------------------------------------
def test_want_rows_orders_ties_and_nan_as_documented():
    nan, inf = np.float32("nan"), np.float32("inf")
    probs = np.array([[[0.25, nan, 0.5, 0.25, 0.0, inf, nan, 0.5, -0.0]]], np.float32)
    slot, p = want_rows(probs, 9)
    assert slot[0, 0].tolist() == [5, 2, 7, 0, 3, 4, 8, 1, 6], "larger first, equal floats (0.0 and -0.0 too) lower slot first, NaN last"
    assert np.array_equal(p[0, 0].view(np.uint32), probs[0, 0][slot[0, 0]].view(np.uint32))
    slot, p = want_rows(probs[:, :, :3], 5)
    assert slot[0, 0].tolist() == [2, 0, 1, PAD_SLOT, PAD_SLOT] and p[0, 0, 3:].tolist() == [0.0, 0.0]

"""CPU preconditions of test_gpu_shared_live.py (inputs and comparison: shared_live_cases.py).  The oracle alone runs here.

1. Every planted shared memory meets C1 .. C7 of shared_live_cases.py: live rows in every (query, hop), every p clear of the
   truncation steps of Q(p) by 1e-3, every live row and every hop visible in the output, three weight codes where the case is
   planted for them, live rows at the named positions, and no two queries of a tile of 8 with the same live rows at a hop.  What a
   case is FOR is asserted besides: survivor lists of 25 .. 28 rows, the three lengths round one scan tile, slices that cut
   between a pair's live rows and a short last slice.
2. The finding that asked for these cases, kept as a test: on shared_cases.CASES no memory longer than 257 slots has a live row.
3. The comparison routine accepts the oracle's own result and REPORTS four planted faults, with every tap and with u_out alone.
"""
import re
from pathlib import Path

import numpy as np
import pytest

import live_hops_cases as lc
import shared_live_cases as sl
from shared_live_cases import CASES, shared_live

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("name", sorted(CASES))
def test_case_meets_its_conditions(oracle, name):
    case = shared_live(name)
    st = sl.check_conditions(oracle, case)
    print(f"{name}: {case.S} slots x {case.cfg['dim_emb']}, {case.B} queries, {st['pairs']} (query, hop) pairs, live rows {st['live_min']} .. "
          f"{st['live_max']}, up to {st['codes']} different weight codes in a pair, {100 * st['o_nonzero']:.0f} % of the columns of o non-zero")
    assert st["pairs"] == case.B * case.H and st["live_min"] >= case.min_live and st["o_nonzero"] > 0.5
    assert case.S <= 4097 and case.B <= 19
    # the planted rows are the live rows: no pair shares one, and nothing else survives
    live = sl.live_sets(case, lc.reference(oracle, case.stories()))
    for (h, q), rows in case.hot.items():
        assert live[(q, h)] == frozenset(rows), f"{name} q{q} h{h}: live {sorted(live[(q, h)])}, planted {sorted(rows)}"


def test_many_live_fills_every_residue_of_the_four_row_fetch(oracle):
    """25 + (q mod 4) live rows of weight code 1 per pair: lists of 25, 26, 27 and 28 entries"""
    case = shared_live("many_live")
    st = case.stories()
    ref = lc.reference(oracle, st)
    seen = set()
    for q in range(case.B):
        for h in range(case.H):
            wc = lc.weight_codes(ref[q]["probs"][h], case.cfg["fmt"][h][1])
            assert np.count_nonzero(wc) == 25 + q % 4 and set(wc[wc > 0].tolist()) == {1}
            assert (np.abs(st.vals[h, st.slots(q)[0] + np.nonzero(wc)[0], :case.cfg["dim_emb"]]) >= 32).all()
            seen.add(np.count_nonzero(wc) % 4)
    assert seen == {0, 1, 2, 3}


def test_graded_cases_have_rows_of_different_weight(oracle):
    case = shared_live("graded_q25")
    ref = lc.reference(oracle, case.stories())
    for q in range(case.B):
        for h in range(case.H):
            wc = lc.weight_codes(ref[q]["probs"][h], 5)
            assert len(set(wc[wc > 0].tolist())) >= 3, (q, h, wc[wc > 0])
            s = np.sort(ref[q]["scores"][h][wc > 0])
            assert (np.diff(s) >= 0.25).all(), f"q{q} h{h}: live scores {s} are not a grid step apart"
    native = shared_live("q25_native")
    assert native.cfg["fmt_att"] == native.cfg["fmt"] == [lc.Q25] * 3 and native.cfg["fmt_bin"] == lc.Q25
    assert native.S * 1.0 <= 53 * (32 - 3)                # the bound of shared_live_cases.py's header for three hot rows


def test_short_scan_lengths_lie_round_one_scan_tile():
    """the tile is kWave / LPR * kUnrollDefault rows (hops_common.h); the constants are read back from the header"""
    text = (ROOT / "q-mann_amd" / "csrc" / "hops_common.h").read_text()
    assert int(re.search(r"constexpr int kWave = (\d+);", text).group(1)) == sl.K_WAVE
    assert int(re.search(r"constexpr int kUnrollDefault = (\d+);", text).group(1)) == sl.K_UNROLL_DEFAULT
    tile = sl.scan_tile_rows(sl.SHORT_D)
    assert tile == 64 // (128 // 16) * 4 == 32
    assert sorted(shared_live(n).S for n in CASES if n.startswith("short_scan")) == [tile - 1, tile, tile + 1]
    for n in CASES:
        if n.startswith("short_scan"):
            assert shared_live(n).B > max(q for q in shared_live(n).qts if q) >= 4      # several queries per tile, and a tail
    assert sl.scan_tile_rows(60) == 64 and sl.scan_tile_rows(256) == 16


@pytest.mark.parametrize("name", sorted(CASES))
def test_forced_slices_cut_between_live_rows(oracle, name):
    """every forced slice count of the split call separates the live rows of some (query, hop), and one of them leaves a short
    last slice (slices are multiples of 16 rows: a memory of a multiple of 16 rows has none)"""
    case = shared_live(name)
    ref = lc.reference(oracle, case.stories())
    short_last = False
    for n in case.slices:
        assert sl.slices_cut_between_live_rows(case, ref, n) is not None, f"{name}: {n} slices of {sl.slice_rows(case.S, n)} rows cut no pair's live rows"
        short_last |= case.S % sl.slice_rows(case.S, n) != 0
    assert short_last or case.S % 16 == 0


def test_tiles_case_leaves_tails():
    case = shared_live("tiles")
    assert case.qts == (1, 2, 4, 8) and case.B % 2 == 1 and case.B % 4 == 3 and case.B % 8 == 3
    assert shared_live("w7_off").envs == ({}, {"QMANN_NO_W7": "1"})
    assert shared_live("long_d60").S >= 4096 and {0, 4095, 4096} <= set(shared_live("long_d60").must)


# ---- 2. the gap ---------------------------------------------------------------------------------------------------------------------
NAMED = ("config4_q25", "config4_q52", "tiles", "tied", "en_mq_clamp", "wl6", "wl_mixed", "pow2", "exp_plan", "pow2_shift", "exp_shift_scaled",
         "scale_negative", "relu", "binary", "binary_relu", "no_lin_map", "one_hop", "eight_hops", "q70")


def test_the_old_shared_inputs_have_no_live_row_beyond_257_slots():
    """WHY THESE CASES EXIST.  On shared_cases.CASES -- the inputs of test_shared_hops_equal_the_oracle,
    test_shared_hops_equal_hops_i8_on_copies and test_split_equals_the_unsplit_call -- 706 of 1 132 (query, hop) pairs have no row
    with a non-zero weight code: every memory longer than 257 slots and every named case but the nine-slot `tied_short`.  Wherever
    a tile size, a softmax variant, a weight format or a tied plane is varied there, every kernel computed o = 0.  Whoever changes
    those inputs sees this assertion fail and can retire it; the old tests stay as they are."""
    import shared_cases as old
    pairs = dead = 0
    for name in sorted(old.CASES):
        case = old.shared_case(name)
        cfg = case["cfg"]
        live = []
        for _, t in old.oracle_taps(name):
            for h in range(cfg["n_hop"]):
                live.append(int(np.count_nonzero(lc.weight_codes(t["probs"][h], cfg["fmt"][h][1]))))
                assert live[-1] or not t["o"][h].any()
        pairs += len(live); dead += sum(n == 0 for n in live)
        if case["S"] > 257 or name in NAMED:
            assert not any(live), f"{name}: {sum(live)} live rows"
    print(f"shared_cases.CASES: {dead} of {pairs} (query, hop) pairs have no live row")
    assert (pairs, dead) == (1132, 706)


# ---- 3. the comparison ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_comparison_accepts_the_oracle_and_reports_planted_faults(oracle, name):
    case = shared_live(name)
    assert sl.check_outputs(oracle, case, sl.simulate(oracle, case)) == case.B
    sl.check_outputs(oracle, case, sl.simulate(oracle, case, taps=()), taps=())
    tried = []
    for fault in sl.FAULTS:
        if fault == "hop0_plane" and case.tied:
            continue
        for taps in (lc.ALL_TAPS, ()):
            raw = sl.simulate(oracle, case, taps=taps, fault=fault)
            if raw is None:
                break
            with pytest.raises(AssertionError):
                sl.check_outputs(oracle, case, raw, taps=taps)
        else:
            tried.append(fault)
    # what each case must be able to show: a list whose length is no multiple of four loses its last entry (every case but the one
    # with four live rows everywhere); neighbours with the same codes exchange o (the tied plants); rows of different codes swap
    # weights (the graded plants); hop 1 reads plane 0 (untied memories)
    assert ("drop_tail" in tried) == (name != "graded_q25")
    assert ("swap_weights" in tried) == (name in ("graded_q25", "q25_native"))
    assert "neighbours_o" in tried or name in ("many_live", "q25_native")
    assert ("hop0_plane" in tried) == (not case.tied)
    raw = sl.simulate(oracle, case)
    raw["u_out"][lc.GUARD - 1] ^= 0xFF                    # one byte written in front of u_out
    with pytest.raises(AssertionError, match="guard"):
        sl.check_outputs(oracle, case, raw)


def test_the_drop_tail_fault_takes_the_last_entry_of_a_ragged_list(oracle):
    """the fault acts on the highest live row of a list whose length is no multiple of four, and on nothing else"""
    for name in ("tiles", "many_live"):
        case = shared_live(name)
        st = case.stories()
        ref = lc.reference(oracle, st)
        q, vals = sl.fault_drop_tail(st, ref)
        changed = np.nonzero((vals != st.vals).any(axis=2))
        assert len(changed[0]) == 1
        h, row = int(changed[0][0]), int(changed[1][0]) - st.slots(q)[0]
        lv = lc.live_rows(st, ref, q, h)
        assert len(lv) % 4 != 0 and row == lv[-1]

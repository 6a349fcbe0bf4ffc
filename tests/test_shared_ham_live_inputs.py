"""CPU preconditions of test_gpu_shared_ham_live.py (inputs: shared_ham_live_cases.py; generator, conditions and comparison:
shared_live_cases.py).  The oracle alone runs here.

1. Every planted shared Hamming memory meets C1 .. C7 of shared_live_cases.py without exemption, its live rows are the planted rows
   and no others, and what a case is FOR is asserted besides: lanes per key row 1 .. 16, lengths round one scan tile (constants read
   back from the headers), survivor lists of 25 .. 28 rows, weight codes 20 / 7 / 2 / 1, one row on either side of V1's threshold,
   minus-zero bytes in hot keys, slices that cut between a pair's live rows and a short last slice.
2. plant_shared with the attention mode added leaves the fixed-point cases of shared_live_cases.py byte for byte as they were.
3. The finding that asked for these cases, kept as a test: the count of live rows on shared_ham_cases.CASES.
4. The comparison routine accepts the oracle's own result and REPORTS the four planted faults of shared_live_cases.FAULTS.
"""
import hashlib
import re
from pathlib import Path

import numpy as np
import pytest

import live_hops_cases as lc
import shared_ham_live_cases as hl
import shared_live_cases as sl
from shared_ham_live_cases import CASES, V0, V1, shared_ham_live

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "q-mann_amd" / "csrc"


def _ref(oracle, case):
    return lc.reference(oracle, case.stories())


# ---- 1. the conditions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_case_meets_its_conditions(oracle, name):
    case = shared_ham_live(name)
    st = sl.check_conditions(oracle, case)
    print(f"{name}: mode {case.cfg['attention_mode']}, {case.cfg['num_bit']} bits, {case.S} slots x {case.cfg['dim_emb']}, {case.B} queries, "
          f"{st['pairs']} (query, hop) pairs, live rows {st['live_min']} .. {st['live_max']}, up to {st['codes']} different weight codes in a pair, "
          f"{100 * st['o_nonzero']:.0f} % of the columns of o non-zero")
    assert st["pairs"] == case.B * case.H and st["live_min"] >= case.min_live >= 3 and st["o_nonzero"] > 0.5
    assert case.S <= 4097 and case.B <= 19
    assert case.cfg["attention_mode"] in (V0, V1) and case.cfg["attention_mode"] == CASES[name]["mode"] and case.cfg["num_bit"] == CASES[name]["num_bit"]
    # the planted rows are the live rows: no pair shares one, and nothing else survives
    live, want = sl.live_sets(case, _ref(oracle, case)), hl.planted_live(case)
    for pr, rows in want.items():
        assert live[pr] == rows, f"{name} q{pr[0]} h{pr[1]}: live {sorted(live[pr])}, planted {sorted(rows)}"


def test_every_option_runs_under_both_modes_and_every_row_width_is_there():
    for opt in hl.OPTIONS:
        assert {shared_ham_live(f"{opt}_v0").cfg["attention_mode"], shared_ham_live(f"{opt}_v1").cfg["attention_mode"]} == {V0, V1}
    assert shared_ham_live("binary_v1").cfg["fmt_bin"] == (0, 0) and shared_ham_live("eight_hops_v0").H == 8
    assert shared_ham_live("en_mq_v1").cfg["fmt_w"] != shared_ham_live("en_mq_v1").cfg["fmt_att"]
    assert shared_ham_live("tied_plane_v1").tied and shared_ham_live("tied_plane_v1").keys.shape[0] == 1
    text = (CSRC / "batch_hops_shared_ham.hip").read_text() + (CSRC / "batch_hops_shared_split_ham.hip").read_text()
    assert len(re.findall(r"LPRK = \(DP / 64\) \* NB \* 8 / 16", text)) == 2           # hl.lprk restates it
    seen = {}
    for name in CASES:
        c = shared_ham_live(name)
        seen.setdefault(hl.lprk(c.cfg["dim_emb"], c.cfg["num_bit"]), set()).add(c.cfg["attention_mode"])
    assert set(seen) == {1, 2, 4, 8, 16} and all(seen[k] == {V0, V1} for k in (4, 8))
    for k in (1, 2, 4, 8, 16):                            # the case planted for the width: a little over four scan tiles
        c = shared_ham_live(next(n for n in CASES if n.startswith(f"lprk{k}_")))
        tile = hl.scan_tile_rows(c.cfg["dim_emb"], c.cfg["num_bit"])
        assert hl.lprk(c.cfg["dim_emb"], c.cfg["num_bit"]) == k and tile == 256 // k and 4 * tile < c.S < 4 * tile + 16
        assert {0, c.S - 1, tile - 1, tile, 4 * tile - 1, 4 * tile, 15, 16} <= set(c.must)


def test_short_scan_lengths_lie_round_one_scan_tile():
    """the tile is kWave / LPRK * kUnrollDefault rows; the constants are read back from the header"""
    text = (CSRC / "hops_common.h").read_text()
    assert int(re.search(r"constexpr int kWave = (\d+);", text).group(1)) == hl.K_WAVE
    assert int(re.search(r"constexpr int kUnrollDefault = (\d+);", text).group(1)) == hl.K_UNROLL_DEFAULT
    for mode, (D, nb) in hl.SHORT.items():
        tile = hl.scan_tile_rows(D, nb)
        assert tile == 256 // (D * nb // 128)
        cases = [shared_ham_live(n) for n in CASES if n.startswith(f"short_scan_v{mode - 10}_")]
        assert sorted(c.S for c in cases) == [tile - 1, tile, tile + 1]
        for c in cases:
            assert c.cfg["attention_mode"] == mode and c.B > max(q for q in c.qts if q) >= 4            # several queries per tile, and a tail


def test_many_live_fills_every_residue_of_the_four_row_fetch(oracle):
    """25 + ((q + h) mod 4) live rows of weight code 1 per pair, through the histogram copy (V0) and the per-slot copy (V1)"""
    for name in ("many_live_v0", "many_live_v1"):
        case = shared_ham_live(name)
        st, ref, seen = case.stories(), _ref(oracle, case), set()
        for q in range(case.B):
            for h in range(case.H):
                wc = lc.weight_codes(ref[q]["probs"][h], case.cfg["fmt"][h][1])
                assert np.count_nonzero(wc) == 25 + (q + h) % 4 and set(wc[wc > 0].tolist()) == {1}
                assert (np.abs(st.vals[h, st.slots(q)[0] + np.nonzero(wc)[0], :case.cfg["dim_emb"]]) >= 32).all()
                seen.add(np.count_nonzero(wc) % 4)
        assert seen == {0, 1, 2, 3}


def test_graded_cases_have_four_weight_codes_in_every_pair(oracle):
    for name in ("graded_q25_v0", "graded_q25_v1"):
        case = shared_ham_live(name)
        assert case.c5
        ref = _ref(oracle, case)
        for q in range(case.B):
            for h in range(case.H):
                wc = lc.weight_codes(ref[q]["probs"][h], 5)
                assert sorted(wc[wc > 0].tolist()) == [1, 2, 7, 20], (name, q, h, wc[wc > 0])


def test_v1_threshold_has_a_row_on_either_side_of_the_step(oracle):
    """three tied rows, one row with 1 < p . 32 < 1.1 and one planted row with 0.8 < p . 32 < 1, which is not live: 36 and 39
    score codes under the top.  The kernel's code_lo, restated: floor((log(total / 32) - 1e-3) . 16) - 1 codes from the top, lies
    between them, two codes under the live row"""
    case = shared_ham_live("v1_threshold")
    assert case.cfg["attention_mode"] == V1 and case.cfg["num_bit"] == 4 and hl.DEAD[case.name] == 1
    assert case.cfg["softmax_variant"] == 0 and case.cfg.get("att_scale") is None                    # the shortcut is taken
    ref = _ref(oracle, case)
    for (h, q), rows in case.hot.items():
        x = ref[q]["probs"][h][rows].astype(np.float64) * 32
        assert len(rows) == 5 and x[0] == x[1] == x[2] > 8 and 1 < x[3] < 1.1 and 0.8 < x[4] < 1, (q, h, x)
        codes = np.rint((ref[q]["scores"][h][rows] - ref[q]["scores"][h].max()) * 16).astype(int).tolist()
        assert codes == [0, 0, 0, -36, -39], (q, h, codes)
        total = np.exp((ref[q]["scores"][h] - ref[q]["scores"][h].max()).astype(np.float64)).sum()
        assert int(np.floor((np.log(total / 32) - 1e-3) * 16)) - 1 == -38


def test_hot_keys_carry_minus_zero_bytes(oracle):
    """Q2.5 hop inputs under Q5.2 attention: a small negative column reads sign 1, magnitude 0; the hot key has the code -128 there,
    the byte 0x80, and still scores the top -- with a plus zero there it would not"""
    for name in ("en_mq_v0", "en_mq_v1", "tiles_v1"):
        case = shared_ham_live(name)
        ref = _ref(oracle, case)
        n = 0
        for (h, q), rows in case.hot.items():
            k = case.keys[0 if case.tied else h, rows[0], :case.cfg["dim_emb"]]
            n += int(np.count_nonzero(k == -128))
            assert ref[q]["scores"][h][rows[0]] == ref[q]["scores"][h].max()
        assert n > 0, name
        assert (lc.to_signmag(np.array([-128, 0, -1], np.int8)) == np.array([0x80, 0x00, 0x81], np.uint8)).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_forced_slices_cut_between_live_rows(oracle, name):
    """every forced slice count of the split call separates the live rows of some (query, hop), and one of them leaves a short
    last slice (slices are multiples of 16 rows: a memory of a multiple of 16 rows has none)"""
    case = shared_ham_live(name)
    ref = _ref(oracle, case)
    short_last = False
    for n in case.slices:
        assert sl.slices_cut_between_live_rows(case, ref, n) is not None, f"{name}: {n} slices of {sl.slice_rows(case.S, n)} rows cut no pair's live rows"
        short_last |= case.S % sl.slice_rows(case.S, n) != 0
    assert short_last or case.S % 16 == 0
    text = (CSRC / "batch_hops_shared_split_ham.hip").read_text()            # sl.slice_rows restates this file's slice_rows
    assert "const uint32_t per = (n_slots + want - 1) / want;\n    return (per + 15u) & ~15u;" in text


def test_tiles_cases_leave_tails():
    for name in ("tiles_v0", "tiles_v1"):
        case = shared_ham_live(name)
        assert case.qts == (1, 2, 4, 8) and case.B % 2 == 1 and case.B % 4 == 3 and case.B % 8 == 3
        assert all(len(set(hl.CASES[name]["deltas"](q, h))) == 1 + (q + h) % 2 for q in range(case.B) for h in range(case.H))
    assert shared_ham_live("long").S >= 4096 and {0, 4095, 4096} <= set(shared_ham_live("long").must)
    assert sum(1 for n in CASES if shared_ham_live(n).copies) >= 3


# ---- 2. the fixed-point cases are what they were ----------------------------------------------------------------------------------------
# sha256 of keys, vals and u0 of two cases of shared_live_cases.py, taken on the commit before plant_shared got `mode` and `num_bit`
BEFORE = {"w7_off": ("e2b6ac65f785f675", "fe531e59aaabd719", "50adcc84d1012bf9"),
          "scale_negative": ("156b1e31d3a1efa2", "89e9ef4e7c0819b6", "a747eede3a373f25")}


@pytest.mark.parametrize("name", sorted(BEFORE))
def test_fixed_point_plants_are_byte_for_byte_what_they_were(name):
    case = sl.shared_live(name)
    assert case.cfg["attention_mode"] == 2 and case.cfg["num_bit"] == 8
    got = tuple(hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16] for a in (case.keys, case.vals, case.u0))
    assert got == BEFORE[name]


# ---- 3. the gap -----------------------------------------------------------------------------------------------------------------------
AT_MOST = {"relu_v1": 1, "tied_v1": 1, "scale_negative_v1": 0, "exp_shift_scaled_v1": 0, "v1_one_bit": 0, "pow2_v1": 2, "no_lin_map_v1": 2,
           "en_mq_v1": 2, "binary_v0": 2, "exp_plan_v0": 2, "en_mq_v0": 2, "eight_hops_v0": 2}


def test_the_old_shared_ham_inputs_have_their_live_rows_at_hop_0_in_the_first_rows():
    """WHY THESE CASES EXIST.  On shared_ham_cases.CASES of at most 1 500 slots (78 cases; the two of 10 000 slots are not counted):
    several live rows at hop 0 come from the clustered plant, rows 0 .. 7 n_query - 1, built from u0 alone; at hops 1 and 2 they are
    what random codes leave; and the option cases of AT_MOST never have more live rows in a pair than stated there (relu_v1 and
    tied_v1: one or NONE; three cases none at all).  Whoever changes those inputs sees this fail and can retire it."""
    import shared_ham_cases as old
    hop0 = hop0_many = later = later_many = counted = 0
    beyond = []
    for name in sorted(old.CASES):
        if old.CASES[name]["S"] > 1500:
            continue
        counted += 1
        case = old.shared_ham_case(name)
        cfg, B, S = case["cfg"], case["n_query"], case["S"]
        most = 0
        for q, (_, t) in enumerate(old.oracle_taps(name)):
            for h in range(cfg["n_hop"]):
                lv = np.nonzero(lc.weight_codes(t["probs"][h], cfg["fmt"][h][1]))[0]
                most = max(most, len(lv))
                if S > 64 and h == 0:
                    hop0 += 1; hop0_many += len(lv) > 1
                    if len(lv) > 1 and case["clustered"] and lv.max() >= 7 * B:
                        beyond.append(name)
                elif S > 64:
                    later += 1; later_many += len(lv) > 1
        if name in AT_MOST:
            assert most <= AT_MOST[name], f"{name}: a pair with {most} live rows"
    print(f"shared_ham_cases.CASES, {counted} cases: above 64 slots {hop0_many} of {hop0} hop-0 pairs and {later_many} of {later} later pairs have several "
          f"live rows; clustered cases with such a hop-0 pair reaching beyond row 7 n_query: {sorted(set(beyond))}")
    assert counted == 78 and (hop0, hop0_many) == (344, 221) and (later, later_many) == (701, 322)
    assert sorted(set(beyond)) == ["scale_negative_v0"]


# ---- 4. the comparison ----------------------------------------------------------------------------------------------------------------
SWAPS = ("graded_q25_v0", "graded_q25_v1", "tiles_v0", "tiles_v1", "v1_threshold")     # the cases with rows of different codes in a pair
FOUR_LIVE = ("graded_q25_v0", "graded_q25_v1", "v1_threshold")                          # four live rows in every pair: no ragged list
NO_TWINS = ("many_live", "tiles")                                                       # no two neighbours with the same weight codes


@pytest.mark.parametrize("name", sorted(CASES))
def test_comparison_accepts_the_oracle_and_reports_planted_faults(oracle, name):
    case = shared_ham_live(name)
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
    assert ("drop_tail" in tried) == (name not in FOUR_LIVE)
    assert ("swap_weights" in tried) == (name in SWAPS)
    # (neighbours exchange o where they hold the same weight codes: not in `tiles`, whose odd queries hold an off-top row, nor in
    # `many_live`, whose neighbours hold 25 .. 28 rows)
    assert ("neighbours_o" in tried) == (not name.startswith(NO_TWINS))
    assert ("hop0_plane" in tried) == (not case.tied)
    raw = sl.simulate(oracle, case)
    raw["u_out"][lc.GUARD - 1] ^= 0xFF                    # one byte written in front of u_out
    with pytest.raises(AssertionError, match="guard"):
        sl.check_outputs(oracle, case, raw)


def test_every_fault_is_reported_under_v0_and_under_v1():
    """(what the parametrised test above asserts per case, summed: each fault of shared_live_cases.FAULTS has a V0 and a V1 case)"""
    modes = lambda names: {CASES[n]["mode"] for n in names}
    assert modes(n for n in CASES if n not in FOUR_LIVE) == modes(SWAPS) == modes(n for n in CASES if not n.startswith(NO_TWINS)) == {V0, V1}
    assert modes(n for n in CASES if not CASES[n].get("tied")) == {V0, V1}

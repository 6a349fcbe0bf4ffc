"""CPU preconditions of test_gpu_live_hops.py (inputs and comparison: live_hops_cases.py).  The oracle alone runs here.

1. Every case meets C1 .. C6 of live_hops_cases.py: live rows in every (query, hop), every p clear of the truncation steps of Q(p)
   by 1e-3, every live row and every hop visible in the output, distinct weight codes where the format has room for them, and
   live rows at the positions the case's kernel can get wrong.  The figures are printed per case.
2. The comparison routine accepts the oracle's own result and REPORTS four planted faults in the outputs, with every tap and
   with u_out alone (all the production kernels expose): one live row's term missing from o, two rows' weights swapped, hop 1
   reading hop 0's value plane, the row behind the cut used.  Each is tried in every case where it has something to act on.
3. The finding that asked for these cases, kept as a test: the memories of test_gpu_mid.py::test_mid_uniform_lengths[200] have
   no live row in any (query, hop) pair.
"""
import types

import numpy as np
import pytest

import live_hops_cases as lc


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_case_meets_its_conditions(oracle, name):
    case = lc.build(oracle, name)
    st = lc.check_conditions(oracle, case)
    print(f"{case.family} / {name}: {st['pairs']} (query, hop) pairs, live rows {st['live_min']} .. {st['live_max']}, up to {st['codes']} different "
          f"weight codes in a pair, {100 * st['o_nonzero']:.0f} % of the columns of o non-zero; no taps: {lc.form_of(case, False)}"
          + (f", taps: {lc.form_of(case, True)}" if case.taps_too else ""))
    assert st["live_min"] >= case.min_live and st["o_nonzero"] > 0.5


LEAN_LIVE = {1: (1, 1), 2: (3, 4), 4: (9, 16), 5: (17, 64)}


@pytest.mark.parametrize("name", sorted(n for n in lc.CASES if n.startswith("lean_frac")))
def test_lean_cases_take_one_and_several_fetch_rounds(oracle, name):
    """live rows per (query, hop) by fraction bits: 3 .. 4 at two, 9 .. 16 at four, more than 16 at five.  At ONE fraction bit a
    row is live from p = 1/2 on and two live rows would both sit on that step: one live row, p = 0.73"""
    case = lc.build(oracle, name)
    st = lc.check_conditions(oracle, case)
    lo, hi = LEAN_LIVE[case.cfg["fmt"][0][1]]
    assert lo <= st["live_min"] and st["live_max"] <= hi, st


def test_v1_threshold_case_has_a_row_on_each_side(oracle):
    """every (query, hop): a live row with 1 < p . 2^frac < 2 and a dead one with 1/2 < p . 2^frac < 1 -- one sign flip of one
    column apart, the closest two scores of this attention can lie to the shortcut threshold from either side"""
    case = lc.build(oracle, "ham_v1_threshold")
    for q, t in enumerate(lc.reference(oracle, case)):
        for h in range(case.H):
            x = t["probs"][h].astype(np.float64) * (1 << case.cfg["fmt"][h][1])
            assert ((x > 1) & (x < 2)).any() and ((x > 0.5) & (x < 1)).any(), (q, h, np.sort(x)[-6:])


@pytest.mark.parametrize("name", sorted(lc.PERSISTENT))
def test_persistent_cases(oracle, name):
    case = lc.build_persistent(oracle, name, 300)
    assert case.B == 300 and len(set(case.origin.tolist())) == 64
    st = lc.check_conditions(oracle, case)
    print(f"persistent / {name}: live rows {st['live_min']} .. {st['live_max']}, {100 * st['o_nonzero']:.0f} % of the columns of o non-zero; "
          f"no taps: {lc.form_of(case, False)}")
    ref = lc.reference(oracle, case)
    for q in range(case.B):                               # every copy shares its original's reference, and has its original's rows
        o = int(case.origin[q])
        assert ref[q] is ref[int(np.flatnonzero(case.origin == o)[0])]
    lc.check_outputs(case, ref, lc.simulate(oracle, case, taps=()), taps=())


@pytest.mark.parametrize("name", sorted(lc.CASES))
def test_comparison_accepts_the_oracle_and_reports_planted_faults(oracle, name):
    case = lc.build(oracle, name)
    ref = lc.reference(oracle, case)
    assert lc.check_outputs(case, ref, lc.simulate(oracle, case)) > 0
    lc.check_outputs(case, ref, lc.simulate(oracle, case, taps=()), taps=())
    tried = []
    for fault in lc.FAULTS:
        if lc.fault_applies(case, ref, fault) is None:
            continue
        tried.append(fault)
        for taps in (lc.ALL_TAPS, ()):
            with pytest.raises(AssertionError):
                lc.check_outputs(case, ref, lc.simulate(oracle, case, taps=taps, fault=fault), taps=taps)
    assert "drop_row" in tried and ("hop0_plane" in tried or case.H == 1)
    assert ("swap_weights" in tried) == (case.c5 or "swap_weights" in tried)
    assert ("behind_cut" in tried) == any(case.slots(q)[2] > case.max_slots for q in range(case.B))
    raw = lc.simulate(oracle, case)
    raw["u_out"][lc.GUARD - 1] ^= 0xFF                    # one byte written in front of u_out
    with pytest.raises(AssertionError, match="guard"):
        lc.check_outputs(case, ref, raw)


def test_the_form_of_every_family(oracle):
    """the kernel form each family is planted for (live_hops_cases.form_of: hops_host.h::hop_plan restated)"""
    want = {"mid_q52": "k_hops_mid", "cut_mid": "k_hops_mid", "cut_streaming": "k_hops_fixed (64 lanes)", "fixed_d128_256lanes": "k_hops_fixed (256 lanes)",
            "fixed_d60_1100": "k_hops_fixed (256 lanes)", "fixed_q25_1800_stop": "k_hops_fixed (stopping build)",
            "fixed_q25_1800_no_stop": "k_hops_fixed (256 lanes)", "small_d60": "k_hops_small", "small_d256": "k_hops_small",
            "lean_frac2_sparse0": "k_hops_lean (value tile)", "lean_frac5_sparse1": "k_hops_lean (sparse read-out)", "quad_short": "k_hops_quad",
            "quad_four_chunks": "k_hops_quad (four chunks)", "quad_split": "split: k_hops_quad + k_hops_lean", "ham_v0_planes": "k_hops_ham",
            "ham_appx_bytes": "k_hops_ham", "ham_v1_4bit_lean": "k_hops_lean", "ham_v0_2bit_quad": "k_hops_quad"}
    for name, form in want.items():
        assert lc.form_of(lc.build(oracle, name), False) == form, name
    assert lc.form_of(lc.build(oracle, "mid_q52"), True) == "k_hops_fixed (256 lanes)"
    assert lc.form_of(lc.build(oracle, "lean_frac2_sparse0"), True) == "k_hops_small"


def test_the_old_mid_inputs_have_no_live_row(oracle):
    """WHY THESE CASES EXIST.  test_gpu_mid.py::test_mid_uniform_lengths[200] -- 200 slots, key and query codes of sigma 30 and
    20 at Q5.2 -- has NO row with a non-zero weight code in any (query, hop) pair: the scores saturate, dozens of rows tie at
    the top code and p = 1 / n_ties falls under 2^-2.  The mid kernel's survivor list, value fetch and weighted sum run with
    o = 0 there.  Whoever changes the spreads of that test sees this assertion fail and can retire it; the old tests themselves
    stay as they are."""
    import test_gpu_mid as old
    cfg = old.cfg_of()
    H, D = cfg["n_hop"], cfg["dim_emb"]
    wts, keys, vals, u0, n_slots, row_off = old.make_batch(types.SimpleNamespace(model=None), cfg, 300, [200], 600 + 200)
    keys[:, ::11, 3] = 0                                  # (both_paths stores "minus zero" bytes there)
    m = oracle.make_model(cfg, wts)
    live = pairs = 0
    for q in range(40):
        r0, r1 = int(row_off[q]), int(row_off[q + 1])
        kf = np.stack([keys[h, r0:r1, :D] / np.float32(4) for h in range(H)]).astype(np.float32)
        vf = np.stack([vals[h, r0:r1, :D] / np.float32(4) for h in range(H)]).astype(np.float32)
        t = oracle.forward_mem(m, kf, vf, u0[q], taps=("probs", "o"))[1]
        for h in range(H):
            n = int(np.count_nonzero(lc.weight_codes(t["probs"][h], 2)))
            live += n; pairs += 1
            assert not t["o"][h].any() or n
    print(f"test_mid_uniform_lengths[200]: {live} live rows in {pairs} (query, hop) pairs")
    assert pairs == 120 and live == 0

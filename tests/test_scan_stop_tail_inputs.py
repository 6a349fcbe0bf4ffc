"""CPU preconditions of test_gpu_scan_stop_tail.py (inputs: scan_stop_tail_cases.py), in the pattern of test_scan_stop_inputs.py.
The oracle alone runs here.  The GPU test demands bit-equality with nothing excused, so every memory is shown to keep its
probabilities clear of the truncation steps of Q(p), and to put the bound's sum -- computed here in double from the oracle's
scores -- on the side of the threshold its name says.
"""
import numpy as np
import pytest

import scan_stop_cases as sc
import scan_stop_tail_cases as tc
from test_scan_stop_inputs import bound_prefix, clear_of_steps, near_step


@pytest.mark.parametrize("D", [128, 256])
def test_phase_memories_stop_inside_the_first_tiles(oracle, D):
    batch = tc.phase_batch(D)
    taps = sc.oracle_taps(oracle, batch)
    clear_of_steps(batch, taps, 1e-2)
    assert batch["max_slots"] >= 360                                         # the gate opens (test_scan_stop_inputs: 350 rows of room)
    tile = 64 // (D // 16) * 4
    counts = sorted({-(-S // tile) for S in tc.PHASE_S})
    print(f"D{D}: tile {tile} rows, tile counts {counts}, modulo 4: {sorted({c % 4 for c in counts})}, modulo 8: {sorted({c % 8 for c in counts})}")
    assert {c % 8 for c in counts} == set(range(8))                          # every residue of the four-wavefront loop (and of a two-wavefront one)
    assert any(S % tile == 0 for S in tc.PHASE_S) and any(S % tile for S in tc.PHASE_S)
    for q, ((name, keys, _, _), t) in enumerate(zip(batch["queries"], taps)):
        S = keys.shape[1]
        assert S >= 257 and 128.0 / S < 0.5                                  # p = 1 / S: weight code 0, half a step away from code 1
        for h in range(3):
            np.testing.assert_array_equal(np.rint(t["scores"][h] * 128), 127)
            assert sc.weight_codes(t["probs"][h], 7).max() == 0
            passed = np.nonzero(bound_prefix(batch, q, h) >= 128 * (1 + 2.0 ** -6))[0]
            assert passed[0] == 129                                          # 130 rows of e^0


@pytest.mark.parametrize("iwl", sorted(tc.SHORT_HOT))
def test_short_memories_must_not_stop(oracle, iwl):
    batch = tc.short_batch(iwl)
    taps = sc.oracle_taps(oracle, batch)
    frac, n_hot = 7 - iwl, tc.SHORT_HOT[iwl]
    thr = (1 << frac) * (1 + 2.0 ** -6)
    assert (1 << frac) * np.exp(127.0 / (1 << frac)) * (1 + 2.0 ** -6) <= batch["max_slots"]          # the gate opens
    for q, ((name, keys, _, _), t) in enumerate(zip(batch["queries"], taps)):
        S = keys.shape[1]
        hot = keys[0, :, 0] == 127
        assert hot.sum() == n_hot and (keys[0, ~hot, 0] == -127).all()
        if name.endswith("spread"):
            assert all(hot[a:a + 16].any() for a in range(0, S - 15, 16))    # every whole tile of the narrowest kind holds a hot row
        np.testing.assert_array_equal(np.rint(t["scores"][0] * (1 << frac)), np.where(hot, 127, -127))
        codes = sc.weight_codes(t["probs"][0], frac)
        assert (codes[hot] == 1).all() and (codes[~hot] == 0).all()
        assert not near_step(t["probs"][0], frac, 1e-2).any()                 # no probability within 1 % of a truncation step
        for h in range(3):
            assert not near_step(t["probs"][h], frac, 1e-3).any(), f"{name} hop {h}"
            end = bound_prefix(batch, q, h)[-1]
            assert end < thr, f"{name} hop {h}: the bound's sum ends at {end:.2f}"
        end = bound_prefix(batch, q)[-1]
        print(f"Q{iwl}.{frac} {name}: bound ends at {end:.2f} of {thr:.2f}, o[0] of hop 0 = {t['o'][0][0]:.4f}")
        if iwl == 0:
            assert end <= 60 + 340 * tc.A_Q07 + 1e-9 < 130
            assert not t["o"][0].any()                                       # Q0.7: weight code 1 reads out nothing (the case's docstring)
        else:
            assert thr / 2 < end <= 40 + 360 * tc.A_Q16 + 1e-9                # counted twice, it would pass thr
            assert t["o"][0].all()                                           # a wrong stop zeroes this: u changes in every column


def test_narrow_rows_beyond_the_mid_kernel(oracle):
    batch = tc.d60_tail_batch()
    taps = sc.oracle_taps(oracle, batch)
    clear_of_steps(batch, taps, 1e-5)
    assert batch["max_slots"] >= sc.FIRE                                     # the gate opens on max_slots
    assert sorted({-(-S // 64) for S in tc.D60_S}) == [17, 18, 19, 20]
    for q, ((name, keys, _, _), t) in enumerate(zip(batch["queries"], taps)):
        assert 1024 < keys.shape[1] <= batch["max_slots"]
        ends = [float(bound_prefix(batch, q, h)[-1]) for h in range(3)]
        live = [int((sc.weight_codes(t["probs"][h], 5) > 0).sum()) for h in range(3)]
        print(f"{name}: bound ends at {[round(e, 2) for e in ends]} of {sc.THR_Q25}, non-zero weight codes per hop {live}")


def test_hops_differ_within_one_launch(oracle):
    batch = tc.hops_differ_batch()
    (t,) = sc.oracle_taps(oracle, batch)
    clear_of_steps(batch, [t], 1e-3)
    keys = batch["queries"][0][1]
    for h in range(2):                                                       # u stays one-hot through hop 0: a row's score code is its key byte
        np.testing.assert_array_equal(np.rint(t["scores"][h] * 32).astype(np.int64), keys[h, :, 0])
    p0 = np.nonzero(bound_prefix(batch, 0, 0) >= sc.THR_Q25)[0]
    assert p0[0] == sc.FIRE - 1 and sc.weight_codes(t["probs"][0], 5).max() == 0 and not t["o"][0].any()
    end1 = bound_prefix(batch, 0, 1)[-1]
    pad = 1399 * np.exp(-254.0 / 32.0)
    assert abs(pad - 0.50) < 0.01 and abs(end1 - (1 + 1600 * sc.A + pad)) < 1e-6 and end1 < 32.0 < sc.THR_Q25
    codes = sc.weight_codes(t["probs"][1], 5)
    assert codes[tc.HOPS_DIFFER_TOP] == 1 and codes.sum() == 1
    assert t["o"][1].all()                                                   # what a stop in hop 1 would lose
    print(f"hop 0 passes thr at row {p0[0]}; hop 1's bound ends at {end1:.3f}, p . 32 of the top row = {32 / end1:.4f}")

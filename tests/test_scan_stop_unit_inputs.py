"""CPU preconditions of test_gpu_scan_stop_unit.py (inputs: scan_stop_unit_cases.py), in the pattern of
test_scan_stop_tail_inputs.py.  The oracle alone runs here.  The GPU test demands bit-equality with nothing excused, so every
memory is shown to keep its probabilities clear of the truncation steps of Q(p), to cover the lengths its name promises, and to
put the bound's sum -- computed here in double from the oracle's scores -- on the side of the threshold its name says.
"""
import numpy as np
import pytest

import scan_stop_cases as sc
import scan_stop_unit_cases as uc
from test_scan_stop_inputs import bound_prefix, clear_of_steps, near_step


def assert_covers_every_phase(lengths, row_bytes, both):
    U = uc.unit_rows(row_bytes)
    whole = {uc.n_units(S, row_bytes) % uc.PERIOD for S in lengths if S % U == 0}
    moved = {uc.n_units(S, row_bytes) % uc.PERIOD for S in lengths if S % U}
    print(f"{row_bytes}-byte rows: unit {U} rows, period {uc.PERIOD}, unit counts {sorted(uc.n_units(S, row_bytes) for S in lengths)}")
    every = set(range(uc.PERIOD))
    if both:
        assert whole == every and moved == every             # per residue one length of either kind
    else:
        assert whole | moved == every and whole and moved


def test_the_unit_is_half_a_tile():
    assert [uc.unit_rows(b) for b in (64, 128, 256)] == [32, 16, 8] and uc.PERIOD == 4 * uc.DEPTH


@pytest.mark.parametrize("D", [128, 256])
def test_phase_memories_cover_the_loop_and_read_out_nothing(oracle, D):
    batch = uc.phase_batch(D)
    taps = sc.oracle_taps(oracle, batch)
    clear_of_steps(batch, taps, 1e-2)
    lengths = [q[1].shape[1] for q in batch["queries"]]
    assert min(lengths) >= 257 and batch["max_slots"] >= 360                  # the four-wavefront block; the gate opens
    assert_covers_every_phase(lengths, D, both=True)
    for q, t in enumerate(taps):
        for h in range(3):
            np.testing.assert_array_equal(np.rint(t["scores"][h] * 128), 127)
            assert sc.weight_codes(t["probs"][h], 7).max() == 0
            assert not t["o"][h].any()                                       # the oracle's read-out is 0
            passed = np.nonzero(bound_prefix(batch, q, h) >= 128 * (1 + 2.0 ** -6))[0]
            assert passed[0] == 129                                          # 130 rows of e^0: inside the first units


@pytest.mark.parametrize("D", [128, 256])
def test_last_unit_memories_and_their_twins(oracle, D):
    batch = uc.last_unit_batch(D)
    taps = sc.oracle_taps(oracle, batch)
    clear_of_steps(batch, taps, 1e-2)
    assert 64 * np.exp(127.0 / 64) * (1 + 2.0 ** -6) <= batch["max_slots"]    # the gate opens
    U = uc.unit_rows(D)
    kinds = {bool(S % U) for S in uc.LAST_UNIT}
    assert kinds == {False, True}, "one length ends on a whole unit, one in a unit that is moved back"
    for q, ((name, keys, _, _), t) in enumerate(zip(batch["queries"], taps)):
        S = keys.shape[1]
        n_hot, n_cold = uc.LAST_UNIT[int(name[1:].split("_")[0])]
        hot = keys[0, :, 0] == 127
        assert (keys[0, ~hot, 0] == -127).all() and S > 256
        for h in range(2):
            np.testing.assert_array_equal(np.rint(t["scores"][h] * 64), np.where(hot, 127, -127))
            prefix = bound_prefix(batch, q, h)                               # (double)
            end = float(prefix[-1])
            codes = sc.weight_codes(t["probs"][h], 6)
            if name.endswith("stop"):
                assert hot.sum() == n_hot and S == n_hot + n_cold and hot[0] and hot[-1]
                assert end > uc.THR_Q16 * (1 + 0.015)
                # every hot row is needed: the sum passes thr with the memory's last row, in the last unit
                assert prefix[-2] < uc.THR_Q16 and end - 1.0 < uc.THR_Q16 - 1e-3
                assert np.nonzero(prefix >= uc.THR_Q16)[0][0] == S - 1
                assert codes.max() == 0 and not t["o"][h].any()
            elif name.endswith("twin"):
                assert hot.sum() == n_hot - 1 and S == n_hot + n_cold - 1
                assert 64.0 < end < uc.THR_Q16 - 1e-3                         # below thr by more than any float sum's error ...
                assert codes.max() == 0 and not t["o"][h].any()              # ... and yet no weight survives (the case's docstring)
            else:
                assert hot.sum() == n_hot - uc.LAST_UNIT_MISS and S == n_hot + n_cold - uc.LAST_UNIT_MISS
                assert end < 64.0 / 1.01
                assert (codes[hot] == 1).all() and (codes[~hot] == 0).all()
                assert t["o"][h].all()                                       # a wrong stop zeroes this: u changes in every column
        print(f"D{D} {name}: S {S}, bound ends at {float(bound_prefix(batch, q)[-1]):.5f} of {uc.THR_Q16}")


@pytest.mark.parametrize("D", [128, 256])
def test_fresh_look_memory(oracle, D):
    batch = uc.fresh_look_batch(D)
    (t,) = sc.oracle_taps(oracle, batch)
    clear_of_steps(batch, [t], 1e-2)
    U, S = uc.unit_rows(D), uc.FRESH_S
    keys = batch["queries"][0][1]
    assert 4 * np.exp(31.75 * uc.FRESH_SCALE) * (1 + 2.0 ** -6) <= batch["max_slots"] and S > 256      # the gate opens
    for h in range(2):                                                       # u stays one-hot through hop 0: a row's score code is its key byte
        np.testing.assert_array_equal(np.rint(t["scores"][h] * 4).astype(np.int64), keys[h, :, 0])
    # hop 0: hot rows in unit 0 alone, which is wavefront 0's first; its sum alone passes thr and nothing else comes near
    hot0 = np.nonzero(keys[0, :, 0] == 127)[0]
    assert {int(r) // U for r in hot0} == {0} and len(hot0) == U
    p0 = bound_prefix(batch, 0, 0)
    assert p0[U - 1] >= 1.5 * uc.THR_Q52                                      # crossed with room (8 or 16 against 4.06) ...
    rest = p0[-1] - p0[U - 1]                                                # ... and the other rows together come nowhere near
    assert rest < 1.0 and abs(rest - (S - U) * uc.FRESH_COLD) < 1e-6
    assert sc.weight_codes(t["probs"][0], 2).max() == 0 and not t["o"][0].any()
    # hop 1: must not stop, and what a stop would lose shows in every column
    end1 = float(bound_prefix(batch, 0, 1)[-1])
    assert abs(end1 - (2 + (S - 2) * uc.FRESH_COLD)) < 1e-6 and end1 < 0.75 * uc.THR_Q52       # (1e-6: the scale is a float, 0.1f)
    codes = sc.weight_codes(t["probs"][1], 2)
    assert codes[list(uc.FRESH_HOP1_HOT)].tolist() == [1, 1] and codes.sum() == 2
    assert not near_step(t["probs"][1], 2, 0.2).any()
    assert t["o"][1].all()
    assert {r // U % 4 for r in uc.FRESH_HOP1_HOT} != {0}                    # not wavefront 0's rows alone
    print(f"D{D}: hop 0 passes thr {uc.THR_Q52} at row {np.nonzero(p0 >= uc.THR_Q52)[0][0]} (unit 0 ends at {U - 1}), "
          f"hop 1's bound ends at {end1:.3f}, p . 4 = {4 / end1:.3f}")


def test_narrow_rows_cover_the_unit_residues(oracle):
    batch = uc.d60_unit_batch()
    taps = sc.oracle_taps(oracle, batch)
    clear_of_steps(batch, taps, 1e-5)
    assert batch["max_slots"] >= sc.FIRE                                     # the gate opens on max_slots
    lengths = [q[1].shape[1] for q in batch["queries"]]
    assert min(lengths) > 1024 and max(lengths) <= batch["max_slots"]        # beyond the mid kernel
    assert_covers_every_phase(lengths, 64, both=False)
    for q, ((name, *_), t) in enumerate(zip(batch["queries"], taps)):
        ends = [float(bound_prefix(batch, q, h)[-1]) for h in range(3)]
        live = [int((sc.weight_codes(t["probs"][h], 5) > 0).sum()) for h in range(3)]
        print(f"{name}: bound ends at {[round(e, 2) for e in ends]} of {sc.THR_Q25}, non-zero weight codes per hop {live}")

"""CPU preconditions of test_gpu_scan_stop.py (inputs: scan_stop_cases.py), in the pattern of test_shared_inputs.py.  The oracle
alone runs here.

1. The crafted memories are what their names say: the oracle's top weight code (1 at N = 1 600, 0 beyond, 8 in `never`), the
   normaliser total' on the intended side of 2^frac and of the kernel's threshold, and the prefix sum of the bound e^(x_r - Xb)
   -- computed here in double -- passing the threshold where the case wants it (or nowhere).
2. No oracle probability of a crafted memory lies within 1e-3 (relative) of a truncation step of Q(p), and none of any other
   memory within 1e-5 (test_gpu_batch.near_step: the one excuse a hop output has for differing from the oracle): the GPU test
   demands bit-equality with nothing excused.
3. The random memories cover both outcomes.  At Q2.5 both code sigmas, 6 and 30, leave no weight code above 0 in any hop (2 000
   rows of scores around 0 carry total' past 32 by themselves; at sigma 30 half the scores saturate at the top code besides):
   the scan stops.  Weights survive in the planted memory at Q2.5, where the launch takes the stopping kernel and must not
   stop in hop 0 (and in the crafted N = 1 600 and `never` memories).
"""
import math

import numpy as np
import pytest

import scan_stop_cases as sc


def near_step(p, frac, rel):
    """test_gpu_batch.near_step"""
    x = p.astype(np.float64) * (1 << frac)
    k = np.rint(x)
    return (np.abs(x - k) <= rel * np.maximum(1.0, np.abs(x))) & (k > 0)


def bound_prefix(batch, q, h=0):
    """double-precision prefix sums of e^(x_r - Xb) over the rows of query q, hop h, from the oracle's scores"""
    cfg = batch["cfg"]
    iwl, frac = cfg["fmt_att"][h]
    top = ((1 << (iwl + frac)) - 1) / float(1 << frac)
    s = 1.0 if cfg.get("att_scale") is None else float(np.float32(cfg["att_scale"][h]))
    x = batch["_taps"][q]["scores"][h].astype(np.float64) * s
    return np.cumsum(np.exp(x - max(top * s, -top * s)))


def clear_of_steps(batch, taps, rel):
    cfg = batch["cfg"]
    for (name, *_), t in zip(batch["queries"], taps):
        for h in range(cfg["n_hop"]):
            assert not near_step(t["probs"][h], cfg["fmt"][h][1], rel).any(), f"{name} hop {h}: a p on a truncation step"


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("D", [60, 128, 256])
def test_crafted_memories_are_what_they_claim(oracle, D, H):
    batch = sc.crafted_batch(D, H)
    taps = sc.oracle_taps(oracle, batch)
    clear_of_steps(batch, taps, 1e-3)
    assert sc.FIRE == 1720
    for q, ((name, keys, _, _), t) in enumerate(zip(batch["queries"], taps)):
        S = keys.shape[1]
        codes = np.rint(t["scores"][0] * 32).astype(np.int64)
        np.testing.assert_array_equal(codes, keys[0, :, 0])                 # a row's score code is its key byte
        top = int(sc.weight_codes(t["probs"][0], 5).max())
        total = float(np.exp((codes - codes.max()) / 32.0).sum())
        prefix = bound_prefix(batch, q)
        passed = np.nonzero(prefix >= sc.THR_Q25)[0]
        print(f"D{D} H{H} {name}: S {S}, total' {total:.3f}, top weight code {top}, bound ends at {prefix[-1]:.3f}, "
              f"passes thr at row {passed[0] if len(passed) else None}")
        if name == "never":
            assert top == sc.NEVER_TOP_CODE and abs(total - 3.86) < 0.01 and prefix[-1] < 4.0
            continue
        N = S - 1
        assert top == sc.CRAFTED_N[N]
        assert abs(total - (1.0 + N * sc.A)) < 1e-6
        if N == 1600:
            assert total < 32.0 and not len(passed)
        elif N == 1660:
            assert 32.0 < total < sc.THR_Q25 and not len(passed)
        elif N == 1700:
            assert len(passed) and passed[0] > S - 40                       # with the last rows (top row first: row 1 667 of 1 701)
        else:
            assert len(passed) and passed[0] <= sc.FIRE
            if name.endswith("fire") or name.endswith("late"):
                r = int(np.argmax(keys[0, :, 0]))
                assert passed[0] < r, "the maximum lies behind the prefix that passes the threshold"
        if H == 3 and top == 0:                                             # u stays one-hot: every hop sees the same scores
            for h in (1, 2):
                np.testing.assert_array_equal(t["scores"][h], t["scores"][0])


def test_cut_and_q07_memories(oracle):
    cut = sc.cut_batch()
    taps = sc.oracle_taps(oracle, cut)
    clear_of_steps(cut, taps, 1e-3)
    for (name, *_), t in zip(cut["queries"], taps):
        assert t["scores"][0].shape == (2000,)
        seen = name.endswith("first") or name.endswith("fire")
        assert (t["scores"][0].max() > 0) == seen, name
        assert sc.weight_codes(t["probs"][0], 5).max() == 0
    q07 = sc.q07_batch()
    taps = sc.oracle_taps(oracle, q07)
    clear_of_steps(q07, taps, 1e-3)
    assert 257 < 128 * math.exp(127 / 128) * (1 + 2.0 ** -6) <= q07["max_slots"]          # the gate opens; 257 rows alone would not open it
    for q, t in enumerate(taps):
        np.testing.assert_array_equal(np.rint(t["scores"][0] * 128), 127)
        assert sc.weight_codes(t["probs"][0], 7).max() == 0
        passed = np.nonzero(bound_prefix(q07, q) >= 128 * (1 + 2.0 ** -6))[0]
        assert passed[0] == 129                                              # 130 rows of e^0


@pytest.mark.parametrize("iwl", sc.RANDOM_IWL)
def test_random_memories_are_clear_of_steps_and_cover_both_outcomes(oracle, iwl):
    frac = 7 - iwl
    for sigma in sc.RANDOM_SIGMA:
        for scale in sorted(sc.SCALES):
            batch = sc.random_batch(iwl, sigma, scale)
            taps = sc.oracle_taps(oracle, batch)
            clear_of_steps(batch, taps, 1e-5)
            live = [[int((sc.weight_codes(t["probs"][h], frac) > 0).sum()) for h in range(3)] for t in taps]
            print(f"Q{iwl}.{frac} sigma {sigma} scale {scale}: non-zero weight codes per query and hop {live}")
            if iwl == 2:
                assert not np.any(live)
    if iwl == 2:
        batch = sc.planted_batch()
        taps = sc.oracle_taps(oracle, batch)
        clear_of_steps(batch, taps, 1e-5)
        for q, t in enumerate(taps):
            codes = sc.weight_codes(t["probs"][0], 5)
            print(f"planted q{q}: weight codes of hop 0 {sorted(codes[codes > 0].tolist())}, bound ends at {bound_prefix(batch, q)[-1]:.3f}")
            assert (codes > 0).sum() >= 1 and bound_prefix(batch, q)[-1] < 0.5 * sc.THR_Q25


def test_other_softmaxes_and_narrow_rows_are_clear_of_steps(oracle):
    for name in sorted(sc.OTHER_SOFTMAX):
        batch = sc.other_softmax_batch(name)
        clear_of_steps(batch, sc.oracle_taps(oracle, batch), 1e-5)
    batch = sc.d60_batch()
    taps = sc.oracle_taps(oracle, batch)
    clear_of_steps(batch, taps, 1e-5)
    assert not any((sc.weight_codes(t["probs"][h], 5) > 0).any() for t in taps for h in range(3))

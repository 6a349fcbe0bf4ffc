"""CPU preconditions of test_gpu_scan_stop_floor.py (inputs: scan_stop_floor_cases.py), in the pattern of
test_scan_stop_unit_inputs.py.  The oracle alone runs here.  Per query and hop the case names an intent, and the oracle's taps
must bear it out -- with the credit formula sum_P e^(x_r - Xb) + (S - |P|) f evaluated in double from the oracle's scores:

  survive  the hot row's weight code is 1 (every cold row's 0) and the read-out is non-zero in every column; the whole sum
           1 + (S - 1) f lies below 2^frac, hence 1.5 % below thr, and within ONE cold row of 2^frac: over-crediting by 3 % of
           thr passes thr, so the faulty stop is taken and shows;
  settled  every weight code is 0, the whole sum reaches thr and is within one cold row of it;
  alone    every weight code is 0 and S f -- no row read -- reaches thr with 0.4 % to spare;
  free     weights survive and the whole sum ends below 3/4 of thr (a hop that has nothing to do with the bound).
The distance to the step is printed in rows; it must be at most 1 % of the threshold.
"""
import math

import numpy as np
import pytest

import scan_stop_cases as sc
import scan_stop_floor_cases as fc
from test_scan_stop_inputs import bound_prefix, near_step


def check_intents(oracle, batch, gate_rows=None):
    cfg = batch["cfg"]
    H = cfg["n_hop"]
    taps = sc.oracle_taps(oracle, batch)
    scales = cfg.get("att_scale") or [None] * H
    assert batch["max_slots"] > 256, "the four-wavefront block, without which no stopping build is launched"
    if gate_rows is not None:
        assert gate_rows <= batch["max_slots"], "hops_host.h::scan_stop_gate stays shut"
    for q, ((name, keys, _, _), t, intents) in enumerate(zip(batch["queries"], taps, batch["intents"])):
        S = min(keys.shape[1], batch["max_slots"])
        for h, what in enumerate(intents):
            if what is None:
                continue
            att, frac = cfg["fmt_att"][h], cfg["fmt"][h][1]
            maxm = (1 << (att[0] + att[1])) - 1
            f, thr = fc.floor_f(att, scales[h]), fc.thr(frac)
            codes = np.rint(t["scores"][h] * (1 << att[1])).astype(np.int64)
            assert t["scores"][h].shape == (S,) and set(np.unique(codes)) <= {-maxm, maxm}, f"{name} hop {h}: a score off the ends"
            hot_code = -maxm if (scales[h] is not None and scales[h] < 0) else maxm
            hot = codes == hot_code
            w = sc.weight_codes(t["probs"][h], frac)
            assert not near_step(t["probs"][h], frac, 1e-5).any(), f"{name} hop {h}: a p on a truncation step"
            whole = float(bound_prefix(batch, q, h)[-1])                     # every row read: the sum itself (double)
            assert abs(whole - (hot.sum() + (S - hot.sum()) * f)) < 1e-6 * whole      # (the scale: one float product there, double here)
            one_pc_rows = 0.01 * thr / f
            if what == "survive":
                assert hot.sum() == 1 and (w[hot] == 1).all() and not w[~hot].any(), f"{name} hop {h}"
                assert t["o"][h].all(), f"{name} hop {h}: a column reads out nothing"
                assert S * f < thr and whole <= (1 << frac) < thr / 1.015
                rows = ((1 << frac) - whole) / f
                assert 0 <= rows < 1 and rows <= one_pc_rows
                assert whole + 0.03 * thr >= thr                             # a 3 % fault is decisive
            elif what == "settled":
                assert not w.any() and not t["o"][h].any(), f"{name} hop {h}"
                assert S * f < thr <= whole
                rows = (whole - thr) / f
                assert 0 <= rows < 1 and rows <= one_pc_rows
            elif what == "alone":
                assert not w.any() and not t["o"][h].any(), f"{name} hop {h}"
                assert S * f * (1 - 2.0 ** -11) >= thr * 1.004
                rows = (S * f - thr) / f                                     # (no step to be near: the decision is free)
            else:
                assert what == "free"
                assert w[hot].all() and not w[~hot].any() and t["o"][h].all() and whole < 0.75 * thr
                rows = (thr - whole) / f
            print(f"{name} hop {h} ({what}): S {S}, f {f:.6f}, S f {S * f:.4f}, whole sum {whole:.4f} of thr {thr}, "
                  f"{rows:.2f} rows from the step (1 % of thr: {one_pc_rows:.1f} rows)")
    return taps


def gate_rows(act_frac, att, scale=None):
    top = ((1 << (att[0] + att[1])) - 1) / float(1 << att[1])
    return (1 << act_frac) * math.exp(top * abs(1.0 if scale is None else scale)) * (1 + 2.0 ** -6)


def test_the_figures_of_the_headline_and_of_the_twins():
    """what DESIGN.md and the case file quote"""
    f25 = fc.floor_f(fc.Q25)
    assert abs(f25 - 3.571e-4) < 1e-7 and abs(10000 * f25 - 3.571) < 1e-3
    f16 = fc.floor_f(fc.Q16)
    assert abs(f16 - 0.018897) < 1e-6
    assert fc.survive_len(f16, 5) == 1641 and abs(1 + 1640 * f16 - 31.991) < 1e-3 and fc.settled_len(f16, 5) == 1668
    assert fc.floor_f(fc.Q16, -1.0) == f16 and fc.alone_len(fc.floor_f(fc.Q16, 0.5), 5) == 238
    assert math.ceil(32.5 / f25) == 91012                                    # "memories of 91 000 rows and more at Q2.5"


@pytest.mark.parametrize("D,scale", fc.WIDTH_CASES)
def test_width_twins(oracle, D, scale):
    batch = fc.width_batch(D, scale)
    check_intents(oracle, batch, gate_rows(5, fc.Q16, scale))
    lengths = {q[1].shape[1] for q in batch["queries"]}
    assert lengths == {1641, 1668} and min(lengths) > 1024                   # (D 60: beyond the mid kernel's 1 024 slots)
    U = fc.unit_rows(D)
    assert 1641 % U and 1668 % U                                            # both end in a unit that is moved back


def test_settled_by_the_floor_alone(oracle):
    batch = fc.alone_batch(128)
    check_intents(oracle, batch, gate_rows(5, fc.Q16, fc.ALONE_SCALE))
    assert [q[1].shape[1] for q in batch["queries"]] == [238, 226, 226, 226, 320]
    # credit for one unit too many (16 rows: 2.2) would settle the survivors
    f = fc.floor_f(fc.Q16, fc.ALONE_SCALE)
    assert 1 + 225 * f + fc.unit_rows(128) * f >= fc.thr(5)


def test_clipped_stories(oracle):
    batch = fc.clipped_batch()
    check_intents(oracle, batch, gate_rows(5, fc.Q16))
    f, thr = fc.floor_f(fc.Q16), fc.thr(5)
    assert batch["max_slots"] == 1641
    for name, keys, _, _ in batch["queries"][1:]:
        S_in = keys.shape[1]
        assert S_in > batch["max_slots"] and S_in * f >= thr * 1.01 > batch["max_slots"] * f      # unclipped: settled unread
        assert np.nonzero(keys[0, :, 0] == 127)[0].tolist()[0] < batch["max_slots"]             # the hot row is inside the clip


def test_two_hops(oracle):
    batch = fc.two_hop_batch(128)
    taps = check_intents(oracle, batch, gate_rows(5, fc.Q16, fc.TWO_HOP_SCALE[0]))
    for t in taps:
        assert sc.weight_codes(t["probs"][1], 5).max() in (4, 5)


def test_short_path(oracle):
    batch = fc.short_batch()
    check_intents(oracle, batch, gate_rows(2, fc.Q16, fc.SHORT_SCALE))
    lengths = [q[1].shape[1] for q in batch["queries"]]
    assert lengths[:3] == [31, 31, 32] and max(lengths[:3]) < 64             # scan_rows_short at 128-byte rows: fewer than 64 rows
    f = fc.floor_f(fc.Q16, fc.SHORT_SCALE)
    assert abs(fc.SHORT_COLD * f - fc.SHORT_SUM) < 1e-5
    assert 1 + 30 * f > fc.thr(2) - 31 * f                                   # the whole term against the lowered threshold: a stop


@pytest.mark.parametrize("which", sorted(fc.UNDERFLOW_SCALES))
def test_underflowing_floor(oracle, which):
    batch = fc.edge_batch(which)
    taps = check_intents(oracle, batch, gate_rows(2, fc.Q52, fc.EDGE_HOP0_SCALE))
    f = fc.floor_f(fc.Q52, fc.UNDERFLOW_SCALES[which])
    tiny = float(np.finfo(np.float32).tiny)
    assert (0 < f < tiny and np.float32(f) > 0) if which == "denormal" else np.float32(f) == 0
    for (name, *_), t in zip(batch["queries"], taps):
        w = sc.weight_codes(t["probs"][1], 2)
        assert w[list(fc.EDGE_HOT)].tolist() == [1, 1, 1] and w.sum() == 3 and t["o"][1].all()
        assert not near_step(t["probs"][1], 2, 0.2).any()                   # p = 1/3: p . 4 = 1.33


@pytest.mark.parametrize("which", sorted(fc.NONFINITE_SCALES))
def test_nonfinite_scale_opens_the_stopping_build(oracle, which):
    """hop 0 alone opens the gate (its own scale is finite); what hop 1 gives is left to the plain kernel (the GPU test)"""
    batch = fc.edge_batch(which)
    assert gate_rows(2, fc.Q52, fc.EDGE_HOP0_SCALE) <= batch["max_slots"] and batch["max_slots"] > 256
    assert not math.isfinite(batch["cfg"]["att_scale"][1])

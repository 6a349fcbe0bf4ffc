"""CPU precondition of test_gpu_attended_ham.py: the named cases of shared_ham_cases.py put the selection of the attended slots
where it can go wrong.  The oracle alone runs here (shared_ham_cases.oracle_taps), k in {1, 5, 16}:

  * ties straddle the cut -- the k-th probability in the order "larger first, lower slot first" equals the (k + 1)-th -- in a
    row of a V0 case and in a row of a V1 case, at k = 5 and at k = 16: the first-by-index rule decides those rows;
  * a zero probability reaches into the first 16 of a V0 row and of a V1 row (exp_plan's zero region, underflow): bins whose
    scores differ tie there;
  * a V1 case has a row with fewer than 5 non-zero weight codes and a row with at least 5: k = 5 is filled partly from below
    the threshold shortcut of the survivor search in the one and by survivors alone in the other; and no row of any case has 16
    survivors, so k = 16 always ranks slots the shortcut skips.

Existence is asserted, not counts: a later change of seeds may move the rows but cannot hollow the GPU test out."""
import functools

import numpy as np

from shared_ham_cases import CASES, oracle_taps, shared_ham_case

NAMED = sorted(n for n in CASES if not n.startswith("grid_"))
KS = (1, 5, 16)


@functools.lru_cache(maxsize=None)
def rows_of(name):
    """per (query, hop) of a case: (probabilities sorted as the attended slots are, number of non-zero weight codes)"""
    case = shared_ham_case(name)
    cfg = case["cfg"]
    out = []
    for _, t in oracle_taps(name):
        for h in range(cfg["n_hop"]):
            p = np.asarray(t["probs"][h], np.float32)
            order = np.lexsort((np.arange(len(p)), -p))
            live = int((np.floor(p.astype(np.float64) * (1 << cfg["fmt"][h][1])) != 0).sum())
            out.append((p[order], live))
    return out


def _mode(name):
    return CASES[name]["cfg"]["attention_mode"]


def _some_row(mode, pred):
    return [n for n in NAMED if _mode(n) == mode and any(pred(p, live) for p, live in rows_of(n))]


def test_the_named_cases_cover_both_modes():
    assert {_mode(n) for n in NAMED} == {10, 11}
    assert all(k <= 16 for k in KS)


def test_ties_straddle_the_cut():
    for mode in (10, 11):
        for k in (5, 16):
            names = _some_row(mode, lambda p, live: len(p) > k and p[k - 1] == p[k])
            assert names, f"mode {mode}: no row of any named case has its {k}-th and {k + 1}-th probabilities equal"


def test_zero_probabilities_reach_into_the_first_sixteen():
    for mode in (10, 11):
        names = _some_row(mode, lambda p, live: len(p) >= 16 and (p[:16] == 0.0).any() and p[0] > 0.0)
        assert names, f"mode {mode}: no row of any named case has a zero among its first 16"


def test_k_five_is_filled_by_survivors_in_one_row_and_from_below_the_shortcut_in_another():
    both = [n for n in NAMED if _mode(n) == 11 and any(live < 5 for _, live in rows_of(n)) and any(live >= 5 for _, live in rows_of(n))]
    assert both, "no V1 case with a row of fewer than 5 survivors and a row of at least 5"


def test_sixteen_always_reaches_below_the_survivors():
    for n in NAMED:
        most = max(live for _, live in rows_of(n))
        assert most < 16, f"{n}: a row with {most} non-zero weight codes"

"""CPU precondition of test_gpu_shared_ham.py: the seeded inputs of shared_ham_cases.py keep clear of the ONE excuse
run_hamming_case (test_gpu_batch.py) grants a hop output for differing from the oracle -- an oracle probability within 1e-5 of a
truncation step of Q(p).  The oracle alone runs here; with the excuse ruled out on these bytes the GPU test demands bit-equality
of every query with 0 excused and cannot raise a false alarm.  A seed that trips this is changed in shared_ham_cases.py
(SEED_BUMP / STORY_BUMP); the bound stays.

Per case, query and hop: either no oracle probability lies within 1e-5 of a truncation step, or the hop is ONE-HOT, which rules
the excuse out just as well and is asserted in full: the float64 softmax recomputed here from the oracle's exact integer scores
has a maximum >= 1 - 1e-9 (the others sum below 2^-25: any correct float softmax, whose exponential of 0 is 1, gives exactly
1.0f), the oracle's best weight is exactly 1.0f, and every other slot's weight code is 0."""
import numpy as np
import pytest

from shared_ham_cases import (CASES, MODEL_MODES, MODEL_N, MODEL_SOURCES, model_inputs, model_story_and_questions, oracle_taps,
                              shared_ham_case)
from test_gpu_batch import near_step


def _exp_plan(x):
    o = 0.597226 * x + 0.933989
    o = np.maximum(o, 0.141642 * x + 0.43981)
    o = np.maximum(o, 0.070265 * x + 0.10888)
    return np.maximum(o, 0.0)


def softmax64(codes, unit, cfg, h):
    """float64 softmax of exact integer score codes with the hop's base and scale layer (normalised: the one-hot clause is not
    for the shift-based forms, whose weights are not)"""
    x = codes.astype(np.float64) * unit
    if cfg.get("att_scale") is not None:
        x = x * float(np.float32(cfg["att_scale"][h]))
    x = x - x.max()
    base = cfg.get("softmax_variant", 0)
    e = np.exp(x) if base == 0 else (np.exp2(x) if base == 1 else _exp_plan(x))
    return e / e.sum()


def clear_or_one_hot(probs, codes, unit, cfg, h, what):
    """the precondition of one hop of one query; returns the number of non-zero weight codes"""
    frac = cfg["fmt"][h][1]
    kp = np.floor(probs.astype(np.float64) * (1 << frac)).astype(np.int64)
    if not near_step(probs, frac).any():
        return int((kp != 0).sum())
    assert not cfg.get("softmax_shift_based"), f"{what}: a p on a truncation step (shift-based softmax: no one-hot clause)"
    p64 = softmax64(codes, unit, cfg, h)
    best = int(np.argmax(p64))
    assert p64[best] >= 1.0 - 1e-9, f"{what}: a p on a truncation step and the hop is not one-hot (max {p64[best]!r})"
    assert probs[best] == np.float32(1.0), f"{what}: the oracle's best weight is {probs[best]!r}, not 1.0f"
    assert (np.delete(kp, best) == 0).all(), f"{what}: a second slot with a non-zero weight code"
    return 1


@pytest.mark.parametrize("name", sorted(CASES))
def test_no_probability_on_a_truncation_step(name):
    case = shared_ham_case(name)
    cfg = case["cfg"]
    most = 0
    for q, (_, t) in enumerate(oracle_taps(name)):
        for h in range(cfg["n_hop"]):
            codes = np.rint(t["scores"][h] / case["unit"]).astype(np.int64)
            np.testing.assert_array_equal(codes * case["unit"], t["scores"][h], err_msg="scores are integers in units of `unit`")
            most = max(most, clear_or_one_hot(t["probs"][h], codes, case["unit"], cfg, h, f"{name}: query {q} hop {h}"))
    if case["clustered"]:
        assert most >= 3, f"{name}: clustered, but no hop of any query has 3 non-zero weight codes (most: {most})"


def test_a_third_of_the_cases_are_clustered():
    n = sum(1 for c in CASES.values() if c["clustered"])
    assert 3 * n >= len(CASES), (n, len(CASES))


@pytest.mark.parametrize("N", MODEL_N)
@pytest.mark.parametrize("mode,num_bit", MODEL_MODES)
@pytest.mark.parametrize("which", MODEL_SOURCES)
def test_model_pairs_keep_clear_of_the_truncation_steps(oracle, which, mode, num_bit, N):
    """the (story, question) pairs test_gpu_shared_ham.py samples for the oracle, of both memorised stories: the same check"""
    from test_gpu_words import question_rows, words_to_bow
    cfg, wts, *_ = model_inputs(which, mode, num_bit)
    m = oracle.make_model(cfg, wts)
    for second in (False, True):
        story, q_sel, _, pick = model_story_and_questions(which, mode, num_bit, N, second)
        st = words_to_bow(story, cfg["dim_input"], True)
        qu = question_rows(q_sel[pick], cfg)
        for i, q in zip(pick, qu):
            _, t = oracle.forward(m, st, q, taps=("scores", "probs"))
            for h in range(cfg["n_hop"]):
                unit = 1.0 / (1 << cfg["fmt_att"][h][1]) if mode == 2 else (1.0 if mode == 10 else 1.0 / (1 << num_bit))
                codes = np.rint(t["scores"][h] / unit).astype(np.int64)
                clear_or_one_hot(t["probs"][h], codes, unit, cfg, h, f"{which} mode {mode} num_bit {num_bit} second {second}: pair {i} hop {h}")

"""CPU precondition of test_gpu_answer_i8.py: the seeded inputs of answer_i8_cases.py do what each case is for, and the numpy
reference there agrees with the oracle (itself pinned to the reference's C code).  No GPU, no library call: a seed that trips a
check here is changed in answer_i8_cases.py; the checks stay."""
import numpy as np
import pytest

from answer_i8_cases import CASES, OUTSIDE, case, highest_argmax, prob64, qm_code


@pytest.mark.parametrize("name", sorted(CASES))
def test_inputs_do_what_the_case_is_for(name):
    c = case(name)
    assert c.kmax < 1 << 23                                                  # int32 accumulators and float32 logits are exact
    assert np.array_equal(c.logits.astype(np.float64) * (1 << c.shift), (c.cu @ c.cw.T).astype(np.float64))
    # exact ties: the duplicated rows give equal codes in every query, and some query without a zero row has its maximum tied
    for a, b in c.pairs:
        assert np.array_equal(c.logits[:, a], c.logits[:, b])
    if c.V >= 2 and not c.zero_rows.all():
        live = ~c.zero_rows
        assert (c.n_at_max[live] >= 2).any(), "no query whose maximum is an exact tie"
    if c.V >= 67 and c.B >= 4 and c.D >= 17:                                  # each planted pair wins its query: the higher index
        for i, (a, b) in enumerate(c.pairs):
            assert c.pred[i] == max(a, b) and c.n_at_max[i] >= 2
    # rows of zeros: every logit equal, the highest index wins
    if c.B >= 6 or c.zero_rows.all():
        assert c.zero_rows.any()
        assert not c.u[c.zero_rows].any() and (c.pred[c.zero_rows] == c.V - 1).all()
    # labels outside the dictionary, both kinds; matches exist among the others
    if c.B >= 11:
        assert (c.labels == c.V + 3).any() and (c.labels == OUTSIDE).any()
        assert c.inside.any() and c.match > 0
    if c.B == 1:
        assert c.inside.all() != (c.labels == OUTSIDE).all()
    # off the grid and beyond the range, where promised -- and nowhere else
    x = c.u.astype(np.float64) * (1 << c.fu[1])
    off = x != np.trunc(x)
    M = (1 << sum(c.fu)) - 1
    if c.family == "offgrid":
        away = off & (np.abs(np.rint(x)) > np.abs(np.trunc(x)))               # rounding to nearest would give another code
        assert off.mean() > 0.3 and away.any() and (off & ~away).any()
        assert (np.abs(c.u) == float(1 << c.fu[0])).any() and (np.abs(x) > 2 * M).any()
        assert ((c.cu == M) & (np.abs(x) > M)).any() and ((c.cu == -M) & (np.abs(x) > M)).any()
        assert not np.array_equal(c.u, c.u_grid)
    else:
        assert not off.any() and np.abs(x).max() <= M and np.array_equal(c.u, c.u_grid)
    assert np.array_equal(qm_code(c.u_grid, c.fu), c.cu)


def test_logit_magnitudes_are_spread():
    """the softmax sees small and large exponents: |logit| beyond 50 somewhere, beyond 1e5 at scale 2^0, below 16 in every
    query of some case (where the relative bound on a probability is the whole criterion)"""
    top = {n: float(case(n).max_abs_logit.max()) for n in CASES}
    assert max(top.values()) > 50
    assert top["fmt_u7.0_w7.0"] > 1e5 and case("fmt_u7.0_w7.0").shift == 0
    assert case("fmt_u2.5_w1.6").shift == 11                                  # the bench's pair
    assert min(top.values()) < 16


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_agrees_with_the_oracle(oracle, name):
    """8 queries per case (the planted ties, a zero row, the last one): oracle.dense_fwd on the dequantised operands gives the
    reference's logits bit for bit, the arg-max of the oracle's e^x softmax is the reference's pred, and the float64 softmax is
    within rtol 1e-5 / atol 1e-7 of the oracle's"""
    c = case(name)
    qs = list(dict.fromkeys([0, 1, 2, 3, 5, c.B // 2, c.B - 2, c.B - 1]))
    qs = [q for q in qs if 0 <= q < c.B]
    for q in qs:
        lo = oracle.dense_fwd(c.w_float, c.u_grid[q], False, (8, 7), (8, 7))
        assert np.array_equal(lo, c.logits[q]), f"query {q}"
        po = oracle.softmax_fwd(lo, variant=0)
        assert oracle.argmax_hi(po) == c.pred[q] == highest_argmax(c.logits[q:q + 1])[0], f"query {q}"
        np.testing.assert_allclose(po, prob64(name, 0, q, np.arange(c.V)), rtol=1e-5, atol=1e-7, err_msg=f"query {q}")

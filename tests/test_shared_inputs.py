"""CPU precondition of test_gpu_shared.py: the seeded inputs of shared_cases.py keep clear of the ONE excuse run_case
(test_gpu_batch.py) grants a hop output for differing from the oracle -- an oracle probability within 1e-5 of a truncation step
of Q(p).  The oracle alone runs here (Oracle.forward_mem per query); with the excuse ruled out on these bytes, the GPU test
demands bit-equality of every query with 0 excused and cannot raise a false alarm.  A seed that trips this is changed in
shared_cases.py; the bound stays.

Memories of ONE slot cannot meet it as worded: their only probability is e / e = 1, which is a truncation step of every Q(p).
For them the test asserts what rules the excuse out just as well: every probability is 1.0 exactly (a quotient of equal floats,
the same in every correct softmax), so no float tolerance is involved and the weight code cannot differ."""
import numpy as np
import pytest

from shared_cases import CASES, oracle_taps, shared_case
from test_gpu_batch import near_step


@pytest.mark.parametrize("name", sorted(CASES))
def test_no_probability_on_a_truncation_step(name):
    case = shared_case(name)
    cfg = case["cfg"]
    for q, (_, t) in enumerate(oracle_taps(name)):
        for h in range(cfg["n_hop"]):
            if case["S"] == 1:
                assert np.array_equal(t["probs"][h], np.ones(1, np.float32)), f"{name}: query {q} hop {h}"
            else:
                assert not near_step(t["probs"][h], cfg["fmt"][h][1]).any(), f"{name}: query {q} hop {h} has a p on a truncation step"

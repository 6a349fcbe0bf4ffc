"""CPU precondition of test_gpu_shared_split.py for the memories beyond the LDS cap (shared_split_cases.py), in the pattern of
test_shared_inputs.py.  The oracle alone runs here.

1. No oracle probability lies within 1e-5 of a truncation step of Q(p) (test_gpu_batch.near_step): the one excuse a hop output
   has for differing from the oracle is ruled out on these bytes, so the GPU test demands bit-equality with 0 queries excused.
2. Every query has at least one hop whose NON-ZERO weight codes Q(p) fall into at least two different slices of the 7-way
   split: the survivors, and with them o and u', then depend on histogram counts that came from different workgroups -- the
   cross-workgroup merge is visible in the result.

A seed that trips either is changed in shared_split_cases.py; the bounds stay."""
import numpy as np
import pytest

from shared_split_cases import LONG_CASES, N_SLICES, long_case, long_oracle_taps, slice_len
from test_gpu_batch import near_step


@pytest.mark.parametrize("name", sorted(LONG_CASES))
def test_long_memories_are_clear_of_steps_and_span_slices(name):
    case = long_case(name)
    cfg, S = case["cfg"], case["S"]
    L = slice_len(S)
    assert -(-S // L) == N_SLICES
    for q, (_, t) in enumerate(long_oracle_taps(name)):
        spans = []
        for h in range(cfg["n_hop"]):
            p = t["probs"][h]
            frac = cfg["fmt"][h][1]
            assert p.shape == (S,)
            assert not near_step(p, frac).any(), f"{name}: query {q} hop {h} has a p on a truncation step"
            live = np.nonzero(np.floor(p.astype(np.float64) * (1 << frac)) > 0)[0]
            spans.append(len(set((live // L).tolist())))
            print(f"{name} q{q} h{h}: best p {p.max():.3g}, {len(live)} non-zero weight codes in {spans[-1]} slices")
        assert max(spans) >= 2, f"{name}: query {q}: non-zero weight codes in {spans} slices per hop"


def test_sizing_helpers_without_a_gpu():
    """the two host-side helpers launch nothing: the workspace is linear in the queries (score bytes at a pitch of 16, n_hop + 1
    KB of bins and state), the library's slices never cut below 256 rows, and both answer 0 where a call would launch nothing"""
    import ctypes as C
    from conftest import load_pkg
    load_pkg()
    import qmann_amd.abi as abi
    import qmann_amd.model as model
    net = model._net_from_cfg(long_case("long_pow2")["cfg"])
    ws = lambda S, B: abi.lib.qmann_hops_shared_split_ws_bytes(C.byref(net), S, B)
    for S in (1, 15, 16, 17, 10000, 160001, 1 << 24):
        per = (S + 15) // 16 * 16 + (net.n_hop + 1) * 1024
        assert [ws(S, B) for B in (0, 1, 2, 77)] == [0, per, 2 * per, 77 * per]
        for B in (1, 9, 8192):
            n = abi.lib.qmann_hops_shared_split_slices(S, 64, B)
            assert 1 <= n <= max(1, S // 256)
    assert abi.lib.qmann_hops_shared_split_slices(0, 64, 5) == 0 and abi.lib.qmann_hops_shared_split_slices(100, 64, 0) == 0
    assert abi.lib.qmann_hops_shared_split_ws_bytes(None, 100, 5) == 0

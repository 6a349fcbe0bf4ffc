"""CPU precondition of test_gpu_shared_split_ham.py for the packed memories beyond the LDS cap (shared_split_ham_cases.py), in the
pattern of test_shared_split_inputs.py.  The oracle alone runs here.

1. No oracle probability lies within 1e-5 of a truncation step of Q(p) (test_gpu_batch.near_step): the one excuse a hop output
   has for differing from the oracle is ruled out on these bytes, so the GPU test demands bit-equality with 0 queries excused.
2. Every query has at least one hop whose NON-ZERO weight codes Q(p) fall into at least two different slices of the 7-way
   split: the survivors, and with them o and u', then depend on scores (and, for V0, histogram counts) that came from different
   workgroups -- the cross-workgroup merge is visible in the result.
3. The sizing helpers of the split call, which launch nothing.

A seed that trips 1 or 2 is changed in shared_split_ham_cases.py; the bounds stay."""
import numpy as np
import pytest

from shared_split_ham_cases import LONG_CASES, N_SLICES, long_ham_case, long_oracle_taps, plant_rows, slice_len
from test_gpu_batch import near_step


@pytest.mark.parametrize("name", sorted(LONG_CASES))
def test_long_memories_are_clear_of_steps_and_span_slices(name):
    case = long_ham_case(name)
    cfg, S = case["cfg"], case["S"]
    L = slice_len(S)
    assert -(-S // L) == N_SLICES
    for q in range(case["n_query"]):                            # the 0-, 1- and 2-flip plants of a query: three different slices
        rows = plant_rows(S, q)
        assert len({r // L for r in rows[:3]}) == 3 and len(set(rows)) == 7 and max(rows) < S
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


def _net(name):
    from conftest import load_pkg
    load_pkg()
    import qmann_amd.model as model
    return model._net_from_cfg(long_ham_case(name)["cfg"])


def test_sizing_helpers_without_a_gpu():
    """the two host-side helpers launch nothing: the workspace is exactly linear in the queries (int16 scores at a pitch of 16,
    for V0 the bins of every hop rounded up to 4, 1 KB of state), the library's slices never cut below its floor of one step of a
    workgroup's four wavefronts (1024 / LPRK rows, at least 64), and both answer 0 where a call would launch nothing"""
    import ctypes as C
    nets = {name: _net(name) for name in ("long_v0", "long_v1")}
    import qmann_amd.abi as abi
    for name, net in nets.items():
        c = LONG_CASES[name]
        ws = lambda S, B: abi.lib.qmann_hops_shared_split_packed_ws_bytes(C.byref(net), S, B)
        bins = (c["num_bit"] * c["D"] + 1 + 3) // 4 * 4 if c["mode"] == 10 else 0
        lprk = net.dim_emb_pad // 64 * c["num_bit"] * 8 // 16
        floor = max(64, 1024 // lprk)
        for S in (1, 15, 16, 17, 10000, 200001, 1 << 24):
            per = 2 * ((S + 15) // 16 * 16) + 4 * net.n_hop * bins + 1024
            assert [ws(S, B) for B in (0, 1, 2, 77)] == [0, per, 2 * per, 77 * per], (name, S)
            for B in (1, 9, 8192):
                n = abi.lib.qmann_hops_shared_split_packed_slices(C.byref(net), S, B)
                assert 1 <= n <= max(1, S // floor), (name, S, B, n)
        slices = abi.lib.qmann_hops_shared_split_packed_slices
        assert slices(C.byref(net), 0, 5) == 0 and slices(C.byref(net), 100, 0) == 0 and slices(None, 100, 5) == 0
        assert slices(C.byref(net), (1 << 24) + 1, 5) == 0 and slices(C.byref(net), 100, 1 << 24) == 0
        assert ws(0, 5) == 0 and ws((1 << 24) + 1, 5) == 0
        assert abi.lib.qmann_hops_shared_split_packed_ws_bytes(None, 100, 5) == 0
    fixed = _net("long_v0")
    fixed.attention_mode = 2                                                  # a net the call refuses: nothing to size
    assert abi.lib.qmann_hops_shared_split_packed_ws_bytes(C.byref(fixed), 100, 5) == 0
    assert abi.lib.qmann_hops_shared_split_packed_slices(C.byref(fixed), 100, 5) == 0

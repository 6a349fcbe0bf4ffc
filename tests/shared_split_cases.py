"""The seeded inputs of the slot-split shared-plane tests (qmann_hops_shared_split_i8) -- ONE definition, read by the GPU test
(test_gpu_shared_split.py) and by the CPU precondition test (test_shared_split_inputs.py).  Not collected by pytest.

The cases of shared_cases.py are taken as they are (CASES: every one of them runs through the split call against the unsplit
one).  Added here: memories BEYOND the LDS cap of qmann_hops_shared_i8, which only the oracle can judge.

A long memory must make the merge of the slices' histograms visible: a uniform memory of 160 000 slots has every Q(p) = 0 and
would test nothing.  So the attention format is wide (Q5.2: a few rows can outweigh 160 000 others), the ordinary keys are small
(codes N(0, 1)), and for each query five rows aligned with its u0 -- sign(u0) . (6 + i) -- are planted at the edges of the
7-way split's slices: the first row, the last row of slice 0, the first of slice 1, a row inside slice 3, the last row (shifted
per query so that no two plants share a row).  test_shared_split_inputs.py asserts what the GPU test relies on."""
from __future__ import annotations

import functools

import numpy as np

from shared_cases import CASES, memory_floats, shared_case  # noqa: F401  (CASES / shared_case: re-exported for the GPU test)
from test_gpu_batch import cfg_synth, weights

N_SLICES = 7                                  # the split the plants are laid out for


def slice_len(S, n_slices=N_SLICES):
    """rows per slice as the library cuts: ceil(S / n_slices) rounded up to 16"""
    return (-(-S // n_slices) + 15) // 16 * 16


# name -> (S, n_query, seed, softmax base).  A seed whose draw fails test_shared_split_inputs.py is changed here; the bounds stay.
LONG_CASES = {
    "long_exp": dict(S=160001, n_query=3, seed=8102, base=0),
    "long_pow2": dict(S=153700, n_query=1, seed=8104, base=1),          # 2^x: the serial float total walks the workspace
}


def plant_rows(S, q):
    """the five planted rows of query q"""
    L = slice_len(S)
    return [0 + q, L - 1 + 16 * q, L - 16 * q, 3 * L + 5 + 16 * q, S - 1 - q]


@functools.lru_cache(maxsize=None)
def long_case(name):
    """-> the dict shared_cases.shared_case gives: cfg, weights, keys, vals (int8 codes [3][S][64]), u0 [n_query][60], S, n_query, tied"""
    c = LONG_CASES[name]
    S, B, seed = c["S"], c["n_query"], c["seed"]
    H, D, V, Dp = 3, 60, 40, 64
    cfg = dict(cfg_synth(D, V, 2, base=c["base"]), fmt_att=[(5, 2)] * H)
    rng = np.random.default_rng(seed)
    wts = weights(seed, H, D, V, 6.0 / 32.0, with_emb=False)
    keys = np.zeros((H, S, Dp), np.int8)
    vals = np.zeros((H, S, Dp), np.int8)
    keys[:, :, :D] = np.clip(np.rint(rng.normal(0, 1.0, (H, S, D))), -127, 127)
    vals[:, :, :D] = np.clip(np.rint(rng.normal(0, 6.0, (H, S, D))), -127, 127)
    u0c = np.clip(np.rint(rng.normal(0, 12.0, (B, D))), -127, 127)
    for q in range(B):
        for i, r in enumerate(plant_rows(S, q)):
            keys[:, r, :D] = (np.sign(u0c[q]) * (6 + i)).astype(np.int8)
    u0 = (u0c / 32.0).astype(np.float32)
    return dict(cfg=cfg, weights=wts, keys=keys, vals=vals, u0=u0, S=S, n_query=B, tied=False)


@functools.lru_cache(maxsize=None)
def long_oracle_taps(name):
    """Oracle.forward_mem of every query of a long case: a list of (pred, taps), computed once per process (seconds per query)"""
    from pyoracle import Oracle
    case = long_case(name)
    ora = Oracle()
    m = ora.make_model(case["cfg"], case["weights"])
    kf, vf = memory_floats(case)
    return [ora.forward_mem(m, kf, vf, case["u0"][q]) for q in range(case["n_query"])]

"""The seeded inputs of the slot-split shared-plane Hamming tests (qmann_hops_shared_split_packed) -- ONE definition, read by the
GPU test (test_gpu_shared_split_ham.py) and by the CPU precondition test (test_shared_split_ham_inputs.py).  Not collected by pytest.

The cases of shared_ham_cases.py are taken as they are (CASES: every one of them runs through the split call against the unsplit
one).  Added here: packed memories BEYOND the LDS cap of qmann_hops_shared_packed, which only the oracle can judge.

A uniform random memory is one-hot under a Hamming score and would show nothing of the slices' merge.  So the long cases use
Q2.5 (a weight survives from 1/32) and, per query, seven planted rows as shared_ham_cases builds its clustered rows: the
query's attention bytes with f = 0 .. 6 of the compared bits flipped.  They lie at the edges of the 7-way split's slices --
the first row, the first row of slice 1, a row inside slice 3, the last row of slice 0, the last row, and rows inside slices 5
and 2, in the order of f -- shifted per query so that no two plants share a row; the 0-, 1- and 2-flip rows of a query are in
slices 0, 1 and 3.  test_shared_split_ham_inputs.py asserts what the GPU test relies on."""
from __future__ import annotations

import functools

import numpy as np

from shared_ham_cases import CASES, V, _PAD, _cfg, att_bytes, oracle_taps, shared_ham_case  # noqa: F401  (re-exported for the GPU test)
from test_gpu_batch import weights

N_SLICES = 7                                  # the split the plants are laid out for


def slice_len(S, n_slices=N_SLICES):
    """rows per slice as the library cuts: ceil(S / n_slices) rounded up to 16"""
    return (-(-S // n_slices) + 15) // 16 * 16


# name -> mode, D, num_bit, S, n_query, seed, softmax base.  A seed whose draw fails test_shared_split_ham_inputs.py is changed
# here; the bounds stay.
LONG_CASES = {
    "long_v0": dict(mode=10, D=128, num_bit=1, S=90001, n_query=3, seed=8301, base=0),          # LPRK 1
    "long_v1": dict(mode=11, D=60, num_bit=8, S=80017, n_query=2, seed=8302, base=0),           # LPRK 4
    "long_v1_pow2": dict(mode=11, D=128, num_bit=4, S=80017, n_query=1, seed=8303, base=1),     # 2^x: the serial float total walks the workspace
}


def plant_rows(S, q):
    """the seven planted rows of query q; entry f carries f flipped bits"""
    L = slice_len(S)
    return [q, L + 16 * q, 3 * L + 5 + 16 * q, L - 1 - 16 * q, S - 1 - q, 5 * L + 9 + 16 * q, 2 * L + 3 + 16 * q]


@functools.lru_cache(maxsize=None)
def long_ham_case(name):
    """-> the dict shared_ham_cases.shared_ham_case gives: cfg, weights, key_bytes, key_floats, vals, u0, S, n_query, tied, unit"""
    c = LONG_CASES[name]
    mode, D, nb, S, B, seed = c["mode"], c["D"], c["num_bit"], c["S"], c["n_query"], c["seed"]
    H, Dp, sigma = 3, _PAD[D], 40.0
    cfg = _cfg(mode, D, nb, 2, H, c["base"])                           # Q2.5 throughout
    rng = np.random.default_rng(seed)
    wts = weights(seed, H, D, V, 1.0, with_emb=False)
    m0 = (1 << 7) - 1
    u0 = (np.clip(np.rint(rng.normal(0, sigma, (B, D))), -m0, m0) / 32.0).astype(np.float32)
    u0[:, ::7] = np.float32(m0 / 32.0) * np.sign(u0[:, ::7] + 0.1)
    vals = np.zeros((H, S, Dp), np.int8)
    vals[:, :, :D] = np.clip(np.rint(rng.normal(0, sigma, (H, S, D))), -127, 127)
    codes = np.zeros((H, S, Dp), np.int16)
    codes[:, :, :D] = np.clip(np.rint(rng.normal(0, sigma, (H, S, D))), -127, 127)
    codes[:, ::3, : D // 2] = np.clip(codes[:, ::3, : D // 2] * 3, -127, 127)     # magnitude ties, zeros and full-scale values
    codes[:, 1::5, ::4] = 0
    key_bytes = np.where(codes < 0, (-codes) | 0x80, codes).astype(np.uint8)
    del codes
    ub = att_bytes(u0, cfg["fmt_att"][0])                                         # [B][D]
    for p in range(H):
        for q in range(B):
            for f, r in enumerate(plant_rows(S, q)):
                row = ub[q].copy()
                for x in rng.choice(D * nb, size=f, replace=False):               # (column, plane) positions among the compared bits
                    row[x // nb] ^= np.uint8(0x80 >> (x % nb))
                row[row == 0x80] = 0                                              # (no minus zero: the oracle takes the float, whose sign it reads)
                key_bytes[p, r, :D] = row
    dec = np.where(key_bytes & 0x80, -(key_bytes & 0x7F).astype(np.float32), (key_bytes & 0x7F).astype(np.float32))
    key_floats = [(dec[h, :, :D] / np.float32(32.0)).astype(np.float32) for h in range(H)]
    return dict(cfg=cfg, weights=wts, key_bytes=key_bytes.view(np.int8), key_floats=key_floats, vals=vals, u0=u0, S=S, n_query=B,
                tied=False, clustered=True, unit=1.0 if mode == 10 else 1.0 / (1 << nb))


@functools.lru_cache(maxsize=None)
def long_oracle_taps(name):
    """Oracle.forward_mem of every query of a long case: a list of (pred, taps), computed once per process (seconds per query)"""
    from pyoracle import Oracle
    case = long_ham_case(name)
    cfg = case["cfg"]
    H, D = cfg["n_hop"], cfg["dim_emb"]
    ora = Oracle()
    m = ora.make_model(cfg, case["weights"])
    kf = np.stack(case["key_floats"])
    vf = np.stack([case["vals"][h, :, :D].astype(np.float32) / (1 << cfg["fmt"][h][1]) for h in range(H)])
    return [ora.forward_mem(m, kf, vf, case["u0"][q]) for q in range(case["n_query"])]

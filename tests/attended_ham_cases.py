"""The planted inputs of the attended-slots tests of the packed Hamming forms (qmann_hops_shared_top_packed and its split / model
forms) -- read by test_gpu_attended_ham.py.  Not collected by pytest (no test_ prefix).

The yardstick (attended_cases.want_rows / assert_rows) and the seeded cases (shared_ham_cases.py, shared_split_ham_cases.py) are
taken by import; added here are two memories that make ties certain:

  zero_ham_case     every key byte zero: every slot scores the same at every hop, every probability is the same float, and the
                    rows must come out 0 .. k-1;
  planted_ham_case  4 099 rows, ten of them identical to query 0's attention bytes (its best possible row under V0 and V1): they
                    tie for every query and hop, are the maximum for query 0 at hop 0, and lie on both sides of 64, 256, 2 048
                    and 4 096 -- the borders of a wavefront, of the workgroup's stride and of the chunks of the ordered walk."""
from __future__ import annotations

import functools

import numpy as np

from shared_ham_cases import V, _PAD, _cfg, att_bytes
from test_gpu_batch import weights

ZERO_S = [1, 5, 16, 17, 257, 2049, 4097]
PLANT_S = 4099
PLANT_ROWS = [63, 64, 255, 256, 2047, 2048, 4095, 4096, 4097, 4098]
MODES = ((10, 128, 4), (11, 128, 8))              # (attention mode, D, num_bit)
BASES = (0, 1, 2)


def _u0(rng, B, D):
    m0 = (1 << 7) - 1
    u0 = (np.clip(np.rint(rng.normal(0, 40.0, (B, D))), -m0, m0) / 32.0).astype(np.float32)        # Q2.5
    u0[:, ::7] = np.float32(m0 / 32.0) * np.sign(u0[:, ::7] + 0.1)
    return u0


@functools.lru_cache(maxsize=None)
def zero_ham_case(mode, D, nb, base, S):
    """-> the fields of shared_ham_cases.shared_ham_case the GPU test reads"""
    H, B, Dp = 3, 2, _PAD[D]
    rng = np.random.default_rng(8500 + 10 * S + base + mode)
    vals = np.zeros((H, S, Dp), np.int8)
    vals[:, :, :D] = np.clip(np.rint(rng.normal(0, 40.0, (H, S, D))), -127, 127)
    return dict(cfg=_cfg(mode, D, nb, 2, H, base), weights=weights(8500 + S, H, D, V, 1.0, with_emb=False),
                key_bytes=np.zeros((H, S, Dp), np.int8), vals=vals, u0=_u0(rng, B, D), S=S, n_query=B, tied=False)


@functools.lru_cache(maxsize=None)
def planted_ham_case(mode, D, nb, base):
    H, B, Dp, S = 3, 3, _PAD[D], PLANT_S
    cfg = _cfg(mode, D, nb, 2, H, base)
    rng = np.random.default_rng(8600 + base + mode)
    u0 = _u0(rng, B, D)
    vals = np.zeros((H, S, Dp), np.int8)
    vals[:, :, :D] = np.clip(np.rint(rng.normal(0, 40.0, (H, S, D))), -127, 127)
    codes = np.zeros((H, S, Dp), np.int16)
    codes[:, :, :D] = np.clip(np.rint(rng.normal(0, 40.0, (H, S, D))), -127, 127)
    key_bytes = np.where(codes < 0, (-codes) | 0x80, codes).astype(np.uint8)
    key_bytes[:, PLANT_ROWS, :D] = att_bytes(u0[0], cfg["fmt_att"][0])
    return dict(cfg=cfg, weights=weights(8600 + base, H, D, V, 1.0, with_emb=False), key_bytes=key_bytes.view(np.int8), vals=vals,
                u0=u0, S=S, n_query=B, tied=False)

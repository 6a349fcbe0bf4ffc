"""The yardstick and the planted inputs of the attended-slots tests (qmann_hops_shared_top_i8 and its split / model forms) --
read by test_gpu_attended.py.  Not collected by pytest (no test_ prefix).

The yardstick is the `probs` tap of the EXISTING call on the same inputs: per query and hop the k slots that come first in
"larger probability first, equal probabilities: lower slot first", padded past the memory's length with slot 0xFFFFFFFF, p 0."""
from __future__ import annotations

import functools

import numpy as np

from test_gpu_batch import cfg_synth, weights

PAD_SLOT = 0xFFFFFFFF


def want_rows(probs, k):
    """probs float32 [H][B][S] (the tap) -> (top_slot uint32 [B][H][k], top_p float32 [B][H][k])"""
    H, B, S = probs.shape
    slot = np.full((B, H, k), PAD_SLOT, np.uint32)
    p = np.zeros((B, H, k), np.float32)
    n = min(k, S)
    for h in range(H):
        for q in range(B):
            order = np.lexsort((np.arange(S), -probs[h, q]))
            want = order[:k]
            slot[q, h, :n] = want
            p[q, h, :n] = probs[h, q][want]
    return slot, p


def assert_rows(got_slot, got_p, probs, k, what):
    """got_slot int32 / got_p float32 device tensors [B][H][k] against the yardstick: indices exactly, probabilities by bit pattern"""
    w_slot, w_p = want_rows(probs, k)
    g_slot = got_slot.cpu().numpy().view(np.uint32)
    g_p = got_p.cpu().numpy()
    assert g_slot.shape == w_slot.shape and g_p.shape == w_p.shape, what
    np.testing.assert_array_equal(g_slot, w_slot, err_msg=f"{what}: top_slot, k={k}")
    np.testing.assert_array_equal(g_p.view(np.uint32), w_p.view(np.uint32), err_msg=f"{what}: top_p bits, k={k}")


# ---- planted ties ---------------------------------------------------------------------------------------------------------------
PLANT_S = 4099
PLANT_POS = [63, 64, 4095, 4096, 4097, 4098]      # code +127 in every column: score code +127 at hop 0 (saturated)
PLANT_NEG = [1, 3]                                # code -127: score code -127 at hop 0
ZERO_S = [1, 5, 16, 17, 64, 65, 257, 4097]


def _planted_cfg(base):
    return cfg_synth(60, 40, 2, base=base)


@functools.lru_cache(maxsize=None)
def planted_case(base):
    """-> the dict shared_cases.shared_case gives.  Keys all zero but for the planted rows, vals random codes (sigma 6), u0 every
    column at the top code of its grid, 3 queries.  At hop 0 every other row scores 0."""
    cfg = _planted_cfg(base)
    H, D, V, Dp, S, B = 3, 60, 40, 64, PLANT_S, 3
    rng = np.random.default_rng(8300 + base)
    keys = np.zeros((H, S, Dp), np.int8)
    vals = np.zeros((H, S, Dp), np.int8)
    vals[:, :, :D] = np.clip(np.rint(rng.normal(0, 6.0, (H, S, D))), -127, 127)
    keys[:, PLANT_POS, :D] = 127
    keys[:, PLANT_NEG, :D] = -127
    u0 = np.full((B, D), 127.0 / (1 << cfg["fmt_w"][0][1]), np.float32)
    return dict(cfg=cfg, weights=weights(8300 + base, H, D, V, 6.0 / 32.0, with_emb=False), keys=keys, vals=vals, u0=u0, S=S,
                n_query=B, tied=False)


@functools.lru_cache(maxsize=None)
def zero_case(S):
    """an all-zero memory of S slots: every score is 0 at every hop, every probability equal"""
    cfg = _planted_cfg(0)
    H, D, V, Dp, B = 3, 60, 40, 64, 2
    rng = np.random.default_rng(8400 + S)
    u0 = (np.clip(np.rint(rng.normal(0, 6.0, (B, D))), -127, 127) / 32.0).astype(np.float32)
    return dict(cfg=cfg, weights=weights(8400 + S, H, D, V, 6.0 / 32.0, with_emb=False), keys=np.zeros((H, S, Dp), np.int8),
                vals=np.zeros((H, S, Dp), np.int8), u0=u0, S=S, n_query=B, tied=False)

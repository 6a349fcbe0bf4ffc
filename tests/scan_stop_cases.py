"""Inputs of test_gpu_scan_stop.py and their CPU preconditions (test_scan_stop_inputs.py): memories on which the fixed-point hop
kernel's early end of the key scan (csrc/batch_hops.hip, step 1b) must or must not fire.

A BATCH is a dict: cfg, w_h (the linear maps), max_slots, and `queries`, a list of (name, keys, vals, u0) with keys / vals int8
CODES [H][S][D] and u0 float [D].  The kernel sums e^(x_r - Xb) over the rows it has retired and stops at thr = 2^frac (1 + 2^-6);
at Q2.5 a row of score code 0 adds A = e^(-127/32) and thr = 32.5, so zero rows alone reach it at row FIRE = 1 720.

Crafted memories (Q2.5): u0 is one-hot with code 32 (1.0) in column 0, so a row's score code is its key byte in column 0; the
linear map is the identity at code 32, so u stays one-hot from hop to hop while the read-out is 0; every value byte is 127, so a
surviving weight code changes u.  N rows of code 0 and ONE row of code 127 (`top`), whose weight is 1 / total',
total' = 1 + N A:
    N = 1 600: total' = 31.24, weight code 1 -- the read-out must NOT be zeroed
    N = 1 660: total' = 32.37, code 0, but below thr: the full path has to find the zero itself
    N = 1 700: total' = 33.13, code 0, thr passed only with the last rows (S = 1 701: inside the moved-back last tile)
    N = 3 000: thr passed early
with the top row first, last, and at row FIRE (N = 3 000: the first row behind the prefix that passes thr -- the maximum the
bound must not depend on; shorter memories: as far back as they reach) and, for N = 3 000, at row 2 048 as well.  `never`:
7 999 rows of code -127 and one of 127: total' = 3.86, top weight code 8, and the sum of the bound ends at 3.86 as well.
"""
import functools
import math

import numpy as np

A = math.exp(-127.0 / 32.0)
THR_Q25 = 32.0 * (1.0 + 2.0 ** -6)
FIRE = math.ceil(THR_Q25 / A)                     # 1 720
CRAFTED_N = {1600: 1, 1660: 0, 1700: 0, 3000: 0}  # N -> the oracle's top weight code
NEVER_TOP_CODE = 8


def cfg_synth(D, V, iwl=5, H=3, base=0, fmt_w=None):
    """test_gpu_batch.cfg_synth (kept here so that the CPU tests import no GPU module)"""
    frac = 7 - iwl
    fmt = [(iwl, frac)] * H
    return dict(n_hop=H, dim_emb=D, dim_input=V, attention_mode=2, softmax_variant=base, f_fixed=True,
                en_lin_map=True, fmt=fmt, fmt_w=fmt_w or list(fmt), fmt_att=list(fmt), fmt_bin=(iwl, frac))


def _one_hot_query(H, D, S, top_rows, low=0, hot_cols=1, u_code=32, frac=5):
    keys = np.zeros((H, S, D), np.int8)
    keys[:, :, :hot_cols] = low
    for r in top_rows:
        keys[:, r, :hot_cols] = 127
    vals = np.full((H, S, D), 127, np.int8)
    u0 = np.zeros(D, np.float32)
    u0[:hot_cols] = u_code / float(1 << frac)
    return keys, vals, u0


def crafted_positions(N):
    S = N + 1
    pos = {"first": 0, "last": S - 1, "fire": min(FIRE, S - 2)}
    if N == 3000:
        pos["late"] = 2048
    return pos


@functools.lru_cache(maxsize=None)
def crafted_batch(D, H):
    """every crafted memory as one ragged batch: stopping and non-stopping queries side by side"""
    cfg = cfg_synth(D, 16, 2, H=H)
    queries = []
    for N in sorted(CRAFTED_N):
        for where, r in crafted_positions(N).items():
            queries.append((f"N{N}_{where}",) + _one_hot_query(H, D, N + 1, [r]))
    queries.append(("never",) + _one_hot_query(H, D, 8000, [4000], low=-127))
    return dict(cfg=cfg, w_h=[np.eye(D, dtype=np.float32) for _ in range(H)], queries=queries,
                max_slots=max(q[1].shape[1] for q in queries))


@functools.lru_cache(maxsize=None)
def cut_batch():
    """max_slots below the stories' length: every story is cut to its first 2 000 rows (the top row first: seen; at FIRE: seen,
    behind the prefix that passes thr; last: cut away)"""
    b = dict(crafted_batch(128, 3))
    b.pop("_taps", None)
    b["queries"] = [q for q in b["queries"] if q[0].startswith("N3000")]
    b["max_slots"] = 2000
    return b


@functools.lru_cache(maxsize=None)
def q07_batch():
    """Q0.7, every score at +127 (two hot columns of 127 . 127 >> 7 = 126 each, clamped), so every row adds 1 and thr = 130 is
    passed after 130 rows: the smallest four-wavefront memory, 257 rows, where no wavefront retires a whole cadence of tiles
    and only the flush behind the scan sees the sum -- beside one of 360 rows, which the launch needs to take the stopping
    kernel at all (its gate asks for 128 e^(127/128) (1 + 2^-6) = 350 rows of room)."""
    D, H = 128, 3
    cfg = cfg_synth(D, 16, 0, H=H)
    qs = [(f"S{S}",) + _one_hot_query(H, D, S, range(S), low=127, hot_cols=2, u_code=127, frac=7) for S in (257, 360)]
    # (the identity at code 127 shrinks u by 1/128 per hop: scores stay large, total' stays above 128 for the first hop at least)
    return dict(cfg=cfg, w_h=[np.eye(D, dtype=np.float32) for _ in range(H)], queries=qs, max_slots=360)


SCALES = {"none": None, "plus": [0.5, 0.5, 0.5], "minus": [-0.5, -0.5, -0.5]}
RANDOM_IWL = (0, 1, 2, 5)
RANDOM_SIGMA = (6, 30)
# today's kernel by the gate (2^x, exp_plan, the shift softmax -- which needs a compressing scale layer, test_gpu_batch.SM_VARIANTS)
OTHER_SOFTMAX = {
    "pow2": dict(softmax_variant=1),
    "exp_plan": dict(softmax_variant=2),
    "exp_shift": dict(softmax_variant=0, softmax_shift_based=True, att_scale=[0.02, 0.015, 0.03]),
}


def _random(cfg, sigma, seed, S_list=(2000, 4096, 2000, 4096)):
    H, D = cfg["n_hop"], cfg["dim_emb"]
    frac = cfg["fmt"][0][1]
    rng = np.random.default_rng(seed)
    code = lambda shape: np.clip(np.rint(rng.normal(0, sigma, shape)), -127, 127)
    w_h = [(code((D, D)) / (1 << frac)).astype(np.float32) for _ in range(H)]
    queries = []
    for i, S in enumerate(S_list):
        keys, vals = code((H, S, D)).astype(np.int8), code((H, S, D)).astype(np.int8)
        queries.append((f"q{i}_S{S}", keys, vals, (code(D) / (1 << frac)).astype(np.float32)))
    return dict(cfg=cfg, w_h=w_h, queries=queries, max_slots=max(S_list))


@functools.lru_cache(maxsize=None)
def random_batch(iwl, sigma, scale):
    cfg = cfg_synth(128, 64, iwl)
    if SCALES[scale] is not None:
        cfg["att_scale"] = SCALES[scale]
    return _random(cfg, sigma, 7000 + 100 * iwl + sigma + 3 * sorted(SCALES).index(scale))


@functools.lru_cache(maxsize=None)
def other_softmax_batch(name):
    return _random(dict(cfg_synth(128, 64, 2), **OTHER_SOFTMAX[name]), 6, 7900 + sorted(OTHER_SOFTMAX).index(name))


@functools.lru_cache(maxsize=None)
def planted_batch():
    """Random memories at Q2.5 whose weights SURVIVE (random codes around 0 cannot do that at 2 000 rows: their scores alone
    carry total' past 32 -- both sigmas above end with every weight code 0): u0 is +0.25 in every column, the keys of hop 0
    lean negative (scores around code -96) except in five planted rows that lean positive and share the softmax between them.
    The launch takes the stopping kernel (the gate looks at formats and sizes only), whose bound stays far below thr in hop 0."""
    b = _random(cfg_synth(128, 64, 2), 6, 7950)
    rng = np.random.default_rng(7951)
    queries = []
    for name, keys, vals, u0 in b["queries"]:
        S = keys.shape[1]
        keys = np.clip(keys.astype(np.int64) - 3, -127, 127)
        for r in rng.choice(S, 5, replace=False):
            keys[0, r] = np.clip(keys[0, r] + 6, -127, 127)
        queries.append((name, keys.astype(np.int8), vals, np.full_like(u0, 0.25)))
    b["queries"] = queries
    return b


@functools.lru_cache(maxsize=None)
def d60_batch():
    """64-byte rows: beyond 1 024 slots the streaming kernel runs them (below, hops_mid.h)"""
    return _random(cfg_synth(60, 64, 2), 6, 7990, S_list=(1500, 3001, 2500))


def weights_of(batch):
    cfg = batch["cfg"]
    return {"w_h": batch["w_h"], "w_ans": np.zeros((cfg["dim_input"], cfg["dim_emb"]), np.float32)}


def oracle_taps(oracle, batch):
    """the oracle's taps of every query of the batch (each story cut to max_slots rows, as the kernels cut it); computed once
    per batch and process"""
    if "_taps" not in batch:
        cfg = batch["cfg"]
        H = cfg["n_hop"]
        m = oracle.make_model(cfg, weights_of(batch))
        out = []
        for _, keys, vals, u0 in batch["queries"]:
            n = min(keys.shape[1], batch["max_slots"])
            kf = np.stack([keys[h, :n].astype(np.float32) / (1 << cfg["fmt_att"][h][1]) for h in range(H)])
            vf = np.stack([vals[h, :n].astype(np.float32) / (1 << cfg["fmt"][h][1]) for h in range(H)])
            out.append(oracle.forward_mem(m, kf, vf, u0)[1])
        batch["_taps"] = out
    return batch["_taps"]


def weight_codes(p, frac):
    return np.floor(p.astype(np.float64) * (1 << frac)).astype(np.int64)

"""Inputs of test_gpu_scan_stop_floor.py and their CPU preconditions (test_scan_stop_floor_inputs.py): the stopping scan's
credit for the rows it has NOT read (csrc/batch_hops.hip::ScanStop).  Batches as in scan_stop_cases.py.

The bound.  Every unread row's clamped score is at least Xmin = min(x(+maxm), x(-maxm)), so with f = e^(Xmin - Xb)
    total' >= sum_{r in P} e^(x_r - Xb) + (S - |P|) f                  (P: the rows retired so far, S: the clipped length)
and the hop may end its scan once the right side reaches thr = 2^frac_act (1 + 2^-6) -- before a single row is read when S f
alone does.  Results do not depend on whether a hop stops, so every memory here is built to make a WRONG stop visible:

  one HOT row (score code at the end that gives the larger x: +maxm, or -maxm under a negative scale) among COLD rows at the
  other end.  Then total' = 1 + (S - 1) f exactly, the hot row's weight code is 1 while total' <= 2^frac_act, and the read-out
  1 . 127 >> frac is non-zero in every column.  survive_len() is the longest such memory; a build that credits 1.6 % too much
  ends its scan and zeroes what the oracle reads out.  settled_len() is the shortest memory whose full sum reaches thr (between
  the two either decision is right, and nothing is asserted about which was taken); alone_len() the shortest that S f settles.
"""
import functools
import math

import numpy as np

import scan_stop_cases as sc
import scan_stop_unit_cases as uc

ALONE_MARGIN = 1.005               # alone_len(): S f reaches thr with the kernel's own derating of f (2^-12) to spare
Q16, Q25, Q52 = (1, 6), (2, 5), (5, 2)


def thr(frac_act):
    return float(1 << frac_act) * (1.0 + 2.0 ** -6)


def floor_f(att, scale=None):
    """f = e^(Xmin - Xb) in double, the two ends of the score range scaled as the kernel scales them (one float product)"""
    top = np.float32(((1 << (att[0] + att[1])) - 1) / float(1 << att[1]))
    s = np.float32(1.0 if scale is None else scale)
    xp, xn = float(top * s), float(-top * s)
    return math.exp(min(xp, xn) - max(xp, xn))


def survive_len(f, frac_act):
    """the longest one-hot-row memory whose hot row keeps weight code 1: 1 + (S - 1) f <= 2^frac"""
    return 1 + int(math.floor(((1 << frac_act) - 1) / f))


def settled_len(f, frac_act):
    """the shortest one-hot-row memory whose whole sum reaches thr"""
    return 1 + int(math.ceil((thr(frac_act) - 1.0) / f))


def alone_len(f, frac_act):
    """the shortest memory the floor settles before any row is read"""
    return int(math.ceil(thr(frac_act) * ALONE_MARGIN / f))


def twin_query(H, D, S, hot_rows, att, sign=(1,)):
    """cold rows at score code -sign . maxm, hot rows at +sign . maxm (two columns that clamp each product), values at the top
    code, u0 at the top code of the input format (= the attention format); sign per hop (the last one repeats)"""
    keys = np.zeros((H, S, D), np.int8)
    for h in range(H):
        sg = sign[min(h, len(sign) - 1)]
        keys[h, :, :2] = -127 * sg
        keys[h, list(hot_rows), :2] = 127 * sg
    vals = np.full((H, S, D), 127, np.int8)
    u0 = np.zeros(D, np.float32)
    u0[:2] = 127.0 / (1 << att[1])
    return keys, vals, u0


def cfg_floor(D, H, act, att, scale=None):
    cfg = sc.cfg_synth(D, 16, act[0], H=H)
    cfg["fmt_att"] = [att] * H
    cfg["fmt_bin"] = att
    if scale is not None:
        cfg["att_scale"] = [float(s) for s in scale]
    return cfg


def _batch(cfg, queries, intents, max_slots):
    """intents: per query a tuple over hops of 'survive' | 'settled' | 'alone' | 'free' | None (test_scan_stop_floor_inputs.py)"""
    D, H = cfg["dim_emb"], cfg["n_hop"]
    return dict(cfg=cfg, w_h=[np.eye(D, dtype=np.float32) for _ in range(H)], queries=queries, intents=intents, max_slots=max_slots)


# ---- the twins at every row width, either sign of the scale ---------------------------------------------------------------
# Q1.6 attention, activation fraction 5: f = e^(-254/64) = 0.018897, thr = 32.5; the hot row survives up to S = 1 641 (total' =
# 31.991) and the whole sum reaches 32.5 from S = 1 668.  Two hops: the identity map and a query at the top code show hop 1 the
# same scores (the survivors' read-out of hop 0 lands in u, whose two live columns still clamp every product).
WIDTH_CASES = [(60, None), (128, None), (256, None), (128, -1.0)]      # (D, scale): Xmin is the score of +maxm under the last


@functools.lru_cache(maxsize=None)
def width_batch(D, scale=None):
    H, att, act = 2, Q16, Q25
    f = floor_f(att, scale)
    sg = (-1,) if (scale is not None and scale < 0) else (1,)
    S_live, S_dead = survive_len(f, act[1]), settled_len(f, act[1])
    qs, intents = [], []
    for name, S, hot, what in (("survives_mid", S_live, S_live // 2, "survive"), ("survives_first", S_live, 0, "survive"),
                               ("survives_last", S_live, S_live - 1, "survive"), ("settled_mid", S_dead, S_dead // 3, "settled"),
                               ("settled_last", S_dead, S_dead - 1, "settled")):
        qs.append((f"S{S}_{name}",) + twin_query(H, D, S, [hot], att, sg))
        intents.append((what,) * H)
    return _batch(cfg_floor(D, H, act, att, None if scale is None else [scale] * H), qs, intents, S_dead)


# ---- settled by the floor alone -------------------------------------------------------------------------------------------
# A scale layer of 0.5 in front of the softmax halves the score range: f = e^(-127/64) = 0.1375, and S f >= 32.5 from 237 rows.
ALONE_SCALE = 0.5
ALONE_LONG = 320                   # lifts max_slots above 256: the four-wavefront block, hence the stopping build


@functools.lru_cache(maxsize=None)
def alone_batch(D):
    H, att, act = 1, Q16, Q25
    f = floor_f(att, ALONE_SCALE)
    S_a, S_s = alone_len(f, act[1]), survive_len(f, act[1])
    qs = [(f"S{S_a}_alone",) + twin_query(H, D, S_a, [S_a // 2], att), (f"S{S_s}_survives_first",) + twin_query(H, D, S_s, [0], att),
          (f"S{S_s}_survives_mid",) + twin_query(H, D, S_s, [S_s // 2], att), (f"S{S_s}_survives_last",) + twin_query(H, D, S_s, [S_s - 1], att),
          (f"S{ALONE_LONG}_alone",) + twin_query(H, D, ALONE_LONG, [7], att)]
    return _batch(cfg_floor(D, H, act, att, [ALONE_SCALE] * H), qs, [("alone",), ("survive",), ("survive",), ("survive",), ("alone",)], ALONE_LONG)


# ---- clipped by max_slots -------------------------------------------------------------------------------------------------
# The stories are longer than max_slots = survive_len: the kernels cut each to its first 1 641 rows, among them the hot row, which
# survives.  Credit for the unclipped length (1 800 f = 34.0, 2 500 f = 47.2) would settle the hop before any row is read.
CLIP_S_IN = (1800, 2500)


@functools.lru_cache(maxsize=None)
def clipped_batch():
    H, D, att, act = 1, 128, Q16, Q25
    S_clip = survive_len(floor_f(att), act[1])
    qs = [(f"S{S_clip}_whole",) + twin_query(H, D, S_clip, [S_clip // 2], att)]
    for S_in in CLIP_S_IN:
        qs.append((f"S{S_in}_cut_hot_mid",) + twin_query(H, D, S_in, [S_clip // 2], att))
        qs.append((f"S{S_in}_cut_hot_last",) + twin_query(H, D, S_in, [S_clip - 1], att))
    return _batch(cfg_floor(D, H, act, att), qs, [("survive",)] * len(qs), S_clip)


# ---- two hops: the floor settles hop 0, hop 1 must not stop ---------------------------------------------------------------
# att_scale = (0.5, 1): hop 0 as in alone_batch (no row is read, o = 0, u stays); hop 1 without the narrowing: f = 0.0189,
# total' = 1 + (S - 1) f = 5.5 .. 7.0, far below 32.5, the hot row's weight code is 4 or 5.  A threshold, a word or a skip
# carried over from hop 0 loses that read-out.
TWO_HOP_SCALE = (0.5, 1.0)


@functools.lru_cache(maxsize=None)
def two_hop_batch(D):
    H, att, act = 2, Q16, Q25
    S_a = alone_len(floor_f(att, TWO_HOP_SCALE[0]), act[1])
    qs = [(f"S{S}_hot{hot}",) + twin_query(H, D, S, [hot], att) for S, hot in ((S_a, 3), (S_a, S_a - 1), (ALONE_LONG, 200))]
    return _batch(cfg_floor(D, H, act, att, TWO_HOP_SCALE), qs, [("alone", "free")] * len(qs), ALONE_LONG)


# ---- the short path inside a stopping launch ------------------------------------------------------------------------------
# Activation fraction 2 (thr = 4.0625) and a scale chosen so that SHORT_COLD cold rows add SHORT_SUM: the hot row of a memory of
# 31 rows -- fewer than the 64 rows (128-byte rows) below which the workgroup takes scan_rows_short -- keeps weight code 1 at
# total' = 3.994; one row more and the sum is 4.094.  A retire hook that adds the whole term against the lowered threshold
# (thr' = 4.0625 - 31 f = 0.97) ends that scan.  A long query beside them opens the stopping build.
SHORT_COLD, SHORT_SUM = 30, 2.994
SHORT_SCALE = float(np.float32(-math.log(SHORT_SUM / SHORT_COLD) / (2 * 127.0 / 64.0)))


@functools.lru_cache(maxsize=None)
def short_batch():
    H, D, att, act = 1, 128, Q16, Q52
    f = floor_f(att, SHORT_SCALE)
    S_s, S_d = survive_len(f, act[1]), settled_len(f, act[1])
    qs = [(f"S{S_s}_survives_first",) + twin_query(H, D, S_s, [0], att), (f"S{S_s}_survives_last",) + twin_query(H, D, S_s, [S_s - 1], att),
          (f"S{S_d}_settled",) + twin_query(H, D, S_d, [5], att), (f"S{ALONE_LONG}_alone",) + twin_query(H, D, ALONE_LONG, [100], att)]
    return _batch(cfg_floor(D, H, act, att, [SHORT_SCALE] * H), qs, [("survive",), ("survive",), ("settled",), ("alone",)], ALONE_LONG)


# ---- a floor that underflows; a scale that is no number -------------------------------------------------------------------
# Q5.2 throughout, two hops.  Hop 0 (scale 0.02: Xb = 0.635, f = 0.28) opens the gate and is settled by the floor alone.  Hop 1
# carries the scale under test:
#   1.5: e^(Xmin - Xb) = e^(-95.25) = 4.3e-42, a float denormal; 2.5: e^(-158.75), 0 in float -- the credit must vanish, and the
#        three hot rows (p = 1/3 each, weight code 1) read out;
#   NaN, +-inf: x is NaN or infinite, the bound's sum is NaN and never compares >= thr: the full path, whatever it gives.
EDGE_HOP0_SCALE = 0.02
UNDERFLOW_SCALES = {"denormal": 1.5, "zero": 2.5}
NONFINITE_SCALES = {"nan": float("nan"), "inf": float("inf"), "-inf": float("-inf")}
EDGE_SCALES = dict(UNDERFLOW_SCALES, **NONFINITE_SCALES)
EDGE_S = (300, 400)
EDGE_HOT = (1, 150, 299)


@functools.lru_cache(maxsize=None)
def edge_batch(which):
    H, D, att, act = 2, 128, Q52, Q52
    scale1 = EDGE_SCALES[which]
    sg = (1, -1) if scale1 < 0 else (1, 1)
    qs = [(f"S{S}",) + twin_query(H, D, S, EDGE_HOT, att, sg) for S in EDGE_S]
    return _batch(cfg_floor(D, H, act, att, (EDGE_HOP0_SCALE, scale1)), qs, [("alone", None)] * len(qs), max(EDGE_S))


def unit_rows(D):
    return uc.unit_rows(64 if D == 60 else D)

"""Inputs of test_gpu_scan_stop_tail.py and their CPU preconditions (test_scan_stop_tail_inputs.py): the smallest memories at
which the stopping scan's loop (csrc/hops_common.h::scan_rows with a hook: look after every tile, leave in front of the next
request) can go wrong.  Batches as in scan_stop_cases.py, whose helpers build them.

A tile is 32 rows at 128-byte rows, 16 at 256-byte rows, 64 at 64-byte rows; NW wavefronts take tiles in turn and the loop
handles two tiles per trip, so what matters of a length is its tile count modulo 2 NW (8 for the four wavefronts of a
stopping launch; the residues modulo 4 -- a two-wavefront workgroup -- come with them) and whether the last tile is whole.
"""
import functools
import math

import numpy as np

import scan_stop_cases as sc

# tile counts 9 .. 16 at 32-row tiles, 17 .. 32 at 16-row tiles, every residue modulo 8 at either size (305: 20 tiles of 16);
# 288, 384 and 512 end on a whole tile of either size, the others in a last tile that is moved back
PHASE_S = (257, 273, 288, 289, 300, 305, 321, 337, 353, 360, 384, 385, 417, 449, 481, 512)
SHORT_S = (257, 321, 400)
SHORT_PLACES = ("first", "last", "spread")
D60_S = (1025, 1089, 1153, 1217)
D60_MAX_SLOTS = sc.FIRE            # the gate looks at max_slots alone: 1 720 rows of room open it at Q2.5, whatever the stories hold
A_Q07 = math.exp(-254.0 / 128.0)   # what a row of score -127 adds to the bound (and to total' beside a row of +127) at Q0.7
A_Q16 = math.exp(-254.0 / 64.0)    # ... at Q1.6
SHORT_HOT = {0: 60, 1: 40}         # iwl -> rows of score +127


@functools.lru_cache(maxsize=None)
def phase_batch(D):
    """Q0.7, every row at +127 (scan_stop_cases.q07_batch): a row adds 1, the bound of 130 is passed inside the first tiles of
    every wavefront count, and each length leaves the loop from another of its exits"""
    H = 3
    qs = [(f"S{S}",) + sc._one_hot_query(H, D, S, range(S), low=127, hot_cols=2, u_code=127, frac=7) for S in PHASE_S]
    return dict(cfg=sc.cfg_synth(D, 16, 0, H=H), w_h=[np.eye(D, dtype=np.float32) for _ in range(H)], queries=qs,
                max_slots=max(PHASE_S))


def short_hot_rows(S, place, n_hot):
    if place == "first":
        return list(range(n_hot))
    if place == "last":
        return list(range(S - n_hot, S))
    return [(i * S) // n_hot for i in range(n_hot)]          # evenly: every 16-, 32- and 64-row tile holds some


@functools.lru_cache(maxsize=None)
def short_batch(iwl):
    """A memory that must NOT stop: n_hot rows at +127, the others at -127; the bound's sum equals total' and ends below thr.
    iwl = 0 (Q0.7, 60 hot rows): total' <= 60 + 340 A_Q07 = 106.8 < 130, the hot rows' weight code is 1 -- but at Q0.7 a weight
    code of 1 reads out NOTHING (1 . 127 >> 7 = 0 for the largest value code), so a wrong stop there would not show in u.
    iwl = 1 (Q1.6, 40 hot rows) is the same memory where it does show: total' <= 40 + 360 A_Q16 = 46.8 < thr = 65, weight code 1,
    1 . 127 >> 6 = 1 per hot row and column; a sum counted twice (>= 80) or left over from a hop before passes 65.  The gate
    needs 64 e^(127/64) (1 + 2^-6) = 473 rows of room at Q1.6, hence max_slots 480 there (350 at Q0.7: 400 do)."""
    H, D, frac, n_hot = 3, 128, 7 - iwl, SHORT_HOT[iwl]
    qs = []
    for S in SHORT_S:
        for place in SHORT_PLACES:
            qs.append((f"S{S}_{place}",) + sc._one_hot_query(H, D, S, short_hot_rows(S, place, n_hot), low=-127, hot_cols=2,
                                                             u_code=127, frac=frac))
    return dict(cfg=sc.cfg_synth(D, 16, iwl, H=H), w_h=[np.eye(D, dtype=np.float32) for _ in range(H)], queries=qs,
                max_slots=480 if iwl else max(SHORT_S))


@functools.lru_cache(maxsize=None)
def d60_tail_batch():
    """64-byte rows just beyond the mid kernel's 1 024 slots (scan_stop_cases.d60_batch's codes): 17 .. 20 tiles of 64 rows"""
    b = sc._random(sc.cfg_synth(60, 64, 2), 6, 7991, S_list=D60_S)
    b["max_slots"] = D60_MAX_SLOTS
    return b


HOPS_DIFFER_S, HOPS_DIFFER_TOP = 3000, 800


@functools.lru_cache(maxsize=None)
def hops_differ_batch():
    """One Q2.5 query (one-hot u, identity map: scan_stop_cases' crafted memories) whose hop 0 stops and whose hop 1 must not:
    hop 0's plane is 3 000 rows of score 0 (the bound passed at row 1 720, o = 0, u stays one-hot); hop 1's is 1 600 rows of
    score 0, one of +127 at row 800 and 1 399 rows of -127 behind them, which add 1 399 e^(-254/32) = 0.50 to
    total' = 1 + 1 600 A + 0.50 = 31.73: weight code 1 (p . 32 = 1.0086), and the bound ends at 31.73 < 32.5.  A stop word or a
    lane's sum that hop 0 left behind makes hop 1 stop and lose the top row's read-out."""
    H, D, S = 2, 128, HOPS_DIFFER_S
    keys = np.zeros((H, S, D), np.int8)
    keys[1, HOPS_DIFFER_TOP, 0] = 127
    keys[1, 1601:, 0] = -127
    vals = np.full((H, S, D), 127, np.int8)
    u0 = np.zeros(D, np.float32)
    u0[0] = 1.0
    return dict(cfg=sc.cfg_synth(D, 16, 2, H=H), w_h=[np.eye(D, dtype=np.float32) for _ in range(H)],
                queries=[("stops_in_hop0_only", keys, vals, u0)], max_slots=S)

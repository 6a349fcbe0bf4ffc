"""Inputs of test_gpu_scan_stop_unit.py and their CPU preconditions (test_scan_stop_unit_inputs.py): the stopping scan's loop
in its own unit (csrc/hops_common.h::scan_rows_stop, csrc/batch_hops.hip::ScanStop).  Batches as in scan_stop_cases.py, whose
helpers and scan_stop_tail_cases.py's build them.

The stopping scan requests, retires and decides on UNITS of UNIT_LOADS 16-byte loads per lane: unit_rows(row bytes) rows -- 16
at 128-byte rows, 8 at 256, 32 at 64 (half the tile of the plain scan).  Four wavefronts take units in turn, each keeps DEPTH
of them (one being retired, the others in flight), and one trip of the loop handles DEPTH units per wavefront: what matters of
a length is its unit count modulo 4 DEPTH and whether the last unit is whole or moved back to end at the last row.  The lanes
that retire a unit's rows add the rows' terms to the workgroup's sum, and THEN the wavefront looks at it, its own unit included.
"""
import functools
import math

import numpy as np

import scan_stop_cases as sc
import scan_stop_tail_cases as tc

UNIT_LOADS = 2                     # batch_hops.hip::ScanStop::kUnitLoads
DEPTH = 3                          # ... ::kDepth
NW = 4                             # wavefronts of a stopping launch
PERIOD = NW * DEPTH                # units one trip of the loop handles, over the workgroup


def unit_rows(row_bytes):
    return 64 // (row_bytes // 16) * UNIT_LOADS


def n_units(S, row_bytes):
    return -(-S // unit_rows(row_bytes))


def phase_lengths(row_bytes, s_min, both=True):
    """PERIOD consecutive unit counts, the lengths from s_min upwards.  both: per count one length that ends on a whole unit and
    one whose last unit is moved back (by 1 .. U - 1 rows, the amount changing with the count); else the two kinds in turn"""
    U = unit_rows(row_bytes)
    n0 = -(-(s_min + U - 1) // U)                            # (U n0 - (U - 1) >= s_min)
    out = []
    for n in range(n0, n0 + PERIOD):
        moved, whole = U * n - (1 + (5 * n) % (U - 1)), U * n
        out += [moved, whole] if both else [whole if n % 2 else moved]
    return out


# ---- every phase of the loop ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def phase_batch(D):
    """scan_stop_tail_cases.phase_batch's construction (Q0.7, every row at +127: a row adds 1, the bound of 130 rows is passed
    inside the first units) at lengths from 257 -- the launcher takes the four-wavefront block only above 256 slots -- whose
    unit counts hit every residue modulo PERIOD, whole and moved-back"""
    H = 3
    lengths = phase_lengths(D, 257)
    qs = [(f"S{S}",) + sc._one_hot_query(H, D, S, range(S), low=127, hot_cols=2, u_code=127, frac=7) for S in lengths]
    return dict(cfg=sc.cfg_synth(D, 16, 0, H=H), w_h=[np.eye(D, dtype=np.float32) for _ in range(H)], queries=qs,
                max_slots=max(max(lengths), 360))            # (the gate asks for 350 rows of room at Q0.7)


# ---- the bound passed with the very last unit, and memories that miss it ----------------------------------------------------
# Q1.6: thr = 64 (1 + 2^-6) = 65 exactly, a row of +127 adds 1 to the bound's sum (and to total'), a row of -127 adds
# A_Q16 = e^(-254/64) = 0.0189.  (hot, cold) below: hot + cold A_Q16 lies in (65.975, 65.998) -- above thr by the 1.5 % the
# proof leaves for the float sum, and less than one row above 65, so that the sum passes thr only when EVERY hot row has been
# added: with the last unit some wavefront retires (the last row is hot).
#   S = 273, 377: last unit moved back at either row width; 584: whole at 256-byte rows (73 x 8), moved back at 128-byte rows;
#   688: whole at both (43 x 16, 86 x 8).
LAST_UNIT = {273: (62, 211), 377: (60, 317), 584: (56, 528), 688: (54, 634)}
A_Q16 = tc.A_Q16
THR_Q16 = 65.0
LAST_UNIT_MISS = 3                 # hot rows the `miss` twin lacks


def spread_rows(S, n_hot):
    """n_hot rows spread evenly over S, the first and the last row among them"""
    return [(i * (S - 1)) // (n_hot - 1) for i in range(n_hot)]


def _q16_query(H, D, S, hot_rows):
    return sc._one_hot_query(H, D, S, hot_rows, low=-127, hot_cols=2, u_code=127, frac=6)


@functools.lru_cache(maxsize=None)
def last_unit_batch(D):
    """Per length of LAST_UNIT three memories:
      `stop`   hot rows spread from the first row to the last: the sum ends above 65 (1 + 0.015), the scan may stop, o = 0;
      `twin`   the same memory without its last (hot) row: one hot row fewer, the sum ends just BELOW 65 -- the bound is not
               reached by one row, the full path has to run.  Its total' lies between 64 and 65, so the weight code is 0 there
               too: a stop taken one row early would not show in u (a hot row adds at most 1, and a weight code of 1 needs
               total' <= 64: no memory one row short of 65.975 can have it);
      `miss`   LAST_UNIT_MISS hot rows fewer (the last, the first, one in the middle): total' = 62.98, every hot row's weight
               code is 1 and 1 . 127 >> 6 = 1 per hot row and column reads out: the nearest memory in which a wrong stop --
               a sum counted twice, a term of another hop or query -- changes u.
    Two hops: with the identity map and a query already at the top code, hop 1 sees hop 0's scores again."""
    H = 2
    qs = []
    for S, (n_hot, n_cold) in sorted(LAST_UNIT.items()):
        assert n_hot + n_cold == S
        hot = spread_rows(S, n_hot)
        qs.append((f"S{S}_stop",) + _q16_query(H, D, S, hot))
        qs.append((f"S{S}_twin",) + _q16_query(H, D, S - 1, hot[:-1]))
        keep = [r for i, r in enumerate(hot) if i not in (0, n_hot // 2, n_hot - 1)]
        shift = lambda r: r - 1 - (r > hot[n_hot // 2])      # rows 0 and hot[n_hot // 2] are taken out, the last one cut off
        qs.append((f"S{S}_miss",) + _q16_query(H, D, S - LAST_UNIT_MISS, [shift(r) for r in keep]))
    return dict(cfg=sc.cfg_synth(D, 16, 1, H=H), w_h=[np.eye(D, dtype=np.float32) for _ in range(H)], queries=qs,
                max_slots=max(LAST_UNIT))                    # (the gate asks for 473 rows of room at Q1.6)


# ---- the look is fresh ---------------------------------------------------------------------------------------------------
# Q5.2 with a scale layer of 0.1 in front of the softmax: thr = 4 (1 + 2^-6) = 4.0625, Xb = 3.175, a row of +127 adds 1 and a
# row of -127 e^(-6.35) = 0.00175; the gate asks for 4 e^3.175 (1 + 2^-6) = 97 rows of room.
FRESH_S = 400
FRESH_SCALE = 0.1
FRESH_COLD = math.exp(-254.0 / 4.0 * FRESH_SCALE)
FRESH_HOP1_HOT = (100, 300)
THR_Q52 = 4.0 * (1.0 + 2.0 ** -6)


@functools.lru_cache(maxsize=None)
def fresh_look_batch(D):
    """One query, two hops in one launch (one-hot u at code 4 = 1.0, identity map: u stays what it was while o = 0).
    Hop 0: the rows of unit 0 -- the first unit of wavefront 0 -- at +127, every other row at -127: wavefront 0's first unit
    alone carries the sum past thr (8 or 16 against 4.06; all the other rows together add 0.7), and the look behind its
    retiring shows it.  total' >= 8.7: every weight code 0, o = 0.
    Hop 1: two rows at +127 (units 6 / 12 and 18 / 37 of 16 / 8 rows), the others at -127: total' = the bound's sum = 2.70,
    below thr, weight code 1 for both (p . 4 = 1.48), and 1 . 127 >> 2 = 31 per row and column reads out.  A stop word
    carried over from hop 0, or a look at another hop's word, stops hop 1 and loses that read-out."""
    H, S = 2, FRESH_S
    U = unit_rows(D)
    keys = np.zeros((H, S, D), np.int8)
    keys[:, :, 0] = -127
    keys[0, :U, 0] = 127
    keys[1, list(FRESH_HOP1_HOT), 0] = 127
    vals = np.full((H, S, D), 127, np.int8)
    u0 = np.zeros(D, np.float32)
    u0[0] = 1.0
    cfg = sc.cfg_synth(D, 16, 5, H=H)
    cfg["att_scale"] = [FRESH_SCALE] * H
    return dict(cfg=cfg, w_h=[np.eye(D, dtype=np.float32) for _ in range(H)], queries=[("hop0_unit0_only", keys, vals, u0)],
                max_slots=S)


# ---- 64-byte rows --------------------------------------------------------------------------------------------------------
D60_S = tuple(phase_lengths(64, 1025, both=False))


@functools.lru_cache(maxsize=None)
def d60_unit_batch():
    """scan_stop_tail_cases.d60_tail_batch's codes (random, sigma 6, Q2.5, D = 60: 64-byte rows) just beyond the mid kernel's
    1 024 slots, at lengths whose unit counts (32-row units) hit every residue modulo PERIOD, whole and moved-back last units
    in turn"""
    b = sc._random(sc.cfg_synth(60, 64, 2), 6, 7992, S_list=D60_S)
    b["max_slots"] = max(max(D60_S), tc.D60_MAX_SLOTS)
    return b

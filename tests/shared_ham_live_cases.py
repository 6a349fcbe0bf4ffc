"""Planted SHARED memories for the shared-plane HAMMING hop kernels on packed codes (k_hops_shared_ham, its TOP build, and the
slot-split pair k_shared_split_scan_ham / k_shared_split_finish_ham), for test_shared_ham_live_inputs.py (CPU) and
test_gpu_shared_ham_live.py.  Not collected by pytest (no test_ prefix).

WHY.  These kernels fetch a value row only where its weight code Q(p) = floor(p . 2^frac) is not zero.  Their softmax and survivor
stages are COPIES (ham_common.h::ham_hist_softmax_survivors, ham_slot_softmax_survivors) of text k_hops_ham carries inline, so the
per-story suite (live_hops_cases.py) runs no line of them.  On shared_ham_cases.py several live rows exist at hop 0 only, in the
first 7 . n_query rows, and the V1 option cases carry at most one or two (test_shared_ham_live_inputs.py keeps the count).

HOW.  shared_live_cases.plant_shared with the attention mode: one memory of int8 key codes whose sign-magnitude bytes
QNet.pack_planes packs, planted hop-major on the oracle.  Cold rows are dense random codes (a V0 score near half the compared bits,
a V1 score near zero).  A hot row carries the hop input's own bytes (shared_live_cases._hot_key_ham): every compared bit agrees, the
top score; `deltas` count columns whose sign is turned, one score step each (V0: 1; V1: 2 . sum_{i=1}^{num_bit-1} 2^-(i+1)); a pair (flips,
fine) takes `fine` single score codes more through compared magnitude bits (`v1_threshold`).  Three tied rows give p = 1/3.  Hot rows of another query are ordinary rows, dozens of steps under the top, so the repairs of
plant_shared have next to nothing to do; a cold row that is loud is drawn again.
  Negative attention scale: the hot key agrees with u in NOTHING the mode counts (V0 score 0; V1 the most negative score), the cold
rows sit in the middle of the score range, and |scale| . (half the range) must keep e^gap above S: at 60 x 8 bits V0 has 240 bits of
gap, the scale 0.125 leaves e^30; V1 at 128 columns has 63, and takes the scales (-0.5, 0.5, -0.25), e^15 at the least.
  ReLU: the hop input has zero columns.  Its byte there is 0x00 and so is the hot key's; a column that is small and NEGATIVE on a
grid finer than the attention's reads sign 1, magnitude 0 -- the minus zero --, and the hot key carries the code -128 there, the float
-2^iwl_att, which the oracle reads as the same word.  (A key built by rounding u's codes has a PLUS zero there: V0 loses a bit, V1
counts the column negative, and rows meant to tie at the top do not.)  Under ReLU every sign of the hop input is plus, so V1 tells
two queries' inputs apart by the compared MAGNITUDE bits alone: at 4 bits those are the codes' bits 64, 32 and 16, which quiet
values (|u code| < 16) leave all zero -- every query's hot rows then top every other query's score too and nothing settles.
`relu_v1` takes loud values (sigma 60, none under 16) for that reason; the nearest foreign row is then 5.4 under the top.

CONDITIONS C1 .. C7 and the split condition are shared_live_cases.py's, asserted per case and without exemption in
test_shared_ham_live_inputs.py.  C5 (three different weight codes in a pair) is asked of the graded cases: e^0, e^-1, e^-2, e^-3 at
five fraction bits are the codes 20, 7, 2, 1.  The other cases hold tied rows on purpose (one code), as that file explains for its
own.  At Q5.2 a row one flip under two tied ones has p = 0.155 < 1/4, so cases that need an off-top live row take Q2.5 activations
under Q5.2 attention (shared_live_cases.Q25_ACT).  `v1_threshold` plants FIVE rows of which the last must NOT be live
(p . 32 = 0.88): DEAD names how many planted rows of a pair stay under the step.
"""
import functools

import shared_live_cases as sl
from live_hops_cases import TIED, pad_dim
from shared_live_cases import Q25_ACT, slice_rows

K_WAVE, K_UNROLL_DEFAULT = sl.K_WAVE, sl.K_UNROLL_DEFAULT


def lprk(D, num_bit):
    """lanes per key row, (Dp / 64) num_bit 8 / 16 (batch_hops_shared_ham.hip)"""
    return pad_dim(D) // 64 * num_bit * 8 // 16


def scan_tile_rows(D, num_bit):
    """rows of one tile of the plane scan, kWave / LPRK * kUnrollDefault: below it the kernels take scan_rows_short"""
    return K_WAVE // lprk(D, num_bit) * K_UNROLL_DEFAULT


def _edges(S, D, num_bit, n_slices=3):
    """both ends, both sides of the first and last scan-tile edge, of 16-row edges and of the edge of the split call's slices"""
    t, s = scan_tile_rows(D, num_bit), slice_rows(S, n_slices)
    last_t, last_16 = t * ((S - 1) // t), 16 * ((S - 1) // 16)
    rows = [0, S - 1, t - 1, t, last_t - 1, last_t, 15, 16, last_16 - 1, last_16, s - 1, s]
    return tuple(dict.fromkeys(r for r in rows if 0 <= r < S))


V0, V1 = 10, 11
GRADED4 = (0, 1, 2, 3)                            # sign flips under the top: weights e^0 .. e^-3 (V0), codes 20, 7, 2, 1 at Q2.5
DEAD = {"v1_threshold": 1}


def _case(mode, num_bit, S, D, B, edges=True, **kw):
    must = kw.pop("must", ())
    return dict(mode=mode, num_bit=num_bit, S=S, D=D, B=B, must=tuple(must) + (_edges(S, D, num_bit) if edges else ()), **kw)


CASES = {
    # 1. the tile sizes, forced: 19 queries leave a tail of 1 (tiles of 2) and 3 (4 and 8).  Where query + hop is odd the pair holds
    #    one of its three live rows a flip under the top (p . 32 = 13.5, 13.5, 4.97): neighbours in a tile then differ in their
    #    tables by score too, and so do a query's consecutive HOPS -- bins or scores of hop h - 1 give other weights
    "tiles_v0": _case(V0, 4, 1500, 128, 19, deltas=lambda q, h: (0, 0, 1) if (q + h) % 2 else TIED, qts=(1, 2, 4, 8), copies=True, **Q25_ACT),
    "tiles_v1": _case(V1, 8, 700, 128, 19, deltas=lambda q, h: (0, 0, 1) if (q + h) % 2 else TIED, qts=(1, 2, 4, 8), **Q25_ACT),
    # 2. one case per lanes-per-key-row 1, 2, 4, 8, 16: a little over four scan tiles of the shape
    "lprk1_v0": _case(V0, 1, 4 * 256 + 3, 128, 5),
    "lprk2_v1": _case(V1, 4, 4 * 128 + 3, 60, 5),
    "lprk4_v0": _case(V0, 4, 4 * 64 + 3, 128, 5),
    "lprk8_v1": _case(V1, 8, 4 * 32 + 3, 128, 5),
    "lprk16_v0": _case(V0, 8, 4 * 16 + 3, 256, 5),
    # 3. four graded rows per pair: weight codes 20, 7, 2, 1 (C5)
    "graded_q25_v0": _case(V0, 2, 1500, 128, 11, deltas=GRADED4, min_live=4, c5=True, **Q25_ACT),
    "graded_q25_v1": _case(V1, 8, 1000, 256, 5, deltas=GRADED4, min_live=4, c5=True, **Q25_ACT),
    # 4. 25 + ((q + h) mod 4) tied rows of code 1 and |value code| >= 32: every residue of the four-row fetch, through both copies;
    #    p . 32 = 1.28, 1.23, 1.19, 1.14, another one at every hop of a query
    "many_live_v0": _case(V0, 8, 1000, 128, 5, n_hot=lambda q, h: 25 + (q + h) % 4, min_live=25, **Q25_ACT),
    "many_live_v1": _case(V1, 4, 1000, 128, 5, n_hot=lambda q, h: 25 + (q + h) % 4, min_live=25, **Q25_ACT),
    # 5. V1's shortcut (ham_slot_softmax_survivors: a slot whose score code is under code_lo, or whose e^(x - max) is under
    #    total . 2^-frac, is dropped before the quotient).  At 4 bits a code is 1/16 and a sign flip 14 codes.  Beside three tied rows:
    #    one row 36 codes under the top (e^-2.25 = 0.1054) and one 39 under (e^-2.4375 = 0.0874); the total is 3.193, so p . 32 =
    #    1.056 and 0.876 -- live and not live, THREE codes apart.  The threshold total / 32 lies 36.9 codes under the top and code_lo
    #    38 under: the live row passes the shortcut by two codes, the dead one is cut by it
    "v1_threshold": _case(V1, 4, 300, 128, 6, deltas=(0, 0, 0, (2, 8), (2, 11)), min_live=4, **Q25_ACT),
    # 6. the launcher's own tile on a long memory, D = 60 in rows of 64
    "long": _case(V0, 8, 4097, 60, 9, must=(4095, 4096, 0), copies=True),
}
# 7. below, at and one above one scan tile of rows (scan_rows_short), V0 at 128 x 4 bits (64 rows) and V1 at 128 x 8 bits (32 rows)
SHORT = {V0: (128, 4), V1: (128, 8)}
for _m, (_D, _nb) in SHORT.items():
    _T = scan_tile_rows(_D, _nb)
    for _S in (_T - 1, _T, _T + 1):
        CASES[f"short_scan_v{_m - 10}_{_S}"] = _case(_m, _nb, _S, _D, 5, edges=False, must=(0, _S - 1, 15, 16) + ((_T - 1,) if _S > _T else ()),
                                                   qts=(2, 4), slices=(2, 7))
# 8. the options that shared_ham_cases.py runs with at most one or two live rows, each under V0 and under V1
MQ_W = [(6, 1), (5, 2), (4, 3)]                   # weight formats that differ from the attention's Q5.2 (EN_MQ)
OPTIONS = {
    "tied_plane": dict(S=300, D=60, B=6, tied=True, passes=4, qts=(None, 8), copies=True),
    "pow2": dict(S=257, D=128, B=6, cfg_extra=dict(softmax_variant=1)),
    "exp_plan": dict(S=300, D=128, B=6, cfg_extra=dict(softmax_variant=2)),
    "scale_negative": dict(S=300, D=60, B=5, cfg_extra=dict(att_scale=[-0.5, 0.25, -0.125])),
    "relu": dict(S=300, D=128, B=6, cfg_extra=dict(en_non_lin=True)),
    "no_lin_map": dict(S=300, D=128, B=6, cfg_extra=dict(en_lin_map=False)),
    "binary": dict(S=300, D=128, B=6, fmt_bin=(0, 0)),
    "eight_hops": dict(S=130, D=60, B=5, H=8),
    # Q2.5 activations: the hop inputs of hops 1 and 2 lie on a finer grid than the attention's, and their small negative columns
    # are minus zeros -- in u's bytes and in the hot keys (code -128)
    "en_mq": dict(S=300, D=128, B=7, fmt_w=MQ_W, **Q25_ACT),
}
for _n, _o in OPTIONS.items():
    for _m, _nb in ((V0, 4 if _n in ("pow2", "no_lin_map") else 8), (V1, 4 if _n in ("relu", "exp_plan") else 8)):
        _o2 = dict(_o)
        if _n == "scale_negative" and _m == V1:   # (the header: V1's score range at 128 columns is 63 wide on either side)
            _o2.update(D=128, cfg_extra=dict(att_scale=[-0.5, 0.5, -0.25]))
        if _n == "relu" and _m == V1:             # (the header: loud values, so that the top magnitude bits of max(u, 0) differ)
            _o2.update(sigma_v=60.0, v_min=16)
        CASES[f"{_n}_v{_m - 10}"] = _case(_m, _nb, _o2.pop("S"), _o2.pop("D"), _o2.pop("B"), **_o2)
TOP_K = (5, 16)


@functools.lru_cache(maxsize=None)
def shared_ham_live(name):
    """the planted case, built once per process"""
    return sl.plant_shared(sl._oracle(), name, **CASES[name])


def planted_live(case):
    """(query, hop) -> the planted rows that must be live: all of them, but for the last DEAD[name] of each pair"""
    n = DEAD.get(case.name, 0)
    return {(q, h): frozenset(rows[:len(rows) - n]) for (h, q), rows in case.hot.items()}

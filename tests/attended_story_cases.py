"""The yardstick and the seeded inputs of the attended-slots-per-story tests (qmann_hops_top_i8, qmann_model_forward_words_top)
-- read by test_gpu_attended_story.py.  Not collected by pytest (no test_ prefix).

The yardstick is the `probs` tap [n_hop][rows_total] of the EXISTING qmann_hops_i8 on the same inputs: sliced per story, cut to
max_slots and ordered by attended_cases.want_rows ("larger probability first, equal probabilities: lower slot first", padded
with slot 0xFFFFFFFF, p 0).

A case is a net configuration, a batch of stories of the listed lengths (keys / vals as integer codes [planes][rows][Dp], planes
= n_hop or 1 for tied hops), row_off, max_slots and the question embeddings u0.  Codes are drawn as run_case / run_hamming_case
in test_gpu_batch.py draw them.  For the Hamming family the library reads the same sign-magnitude bytes whatever grid they were
meant for, and the tap of the same bytes is the yardstick, so no operand grid needs modelling here."""
from __future__ import annotations

import functools

import numpy as np

from attended_cases import PAD_SLOT, want_rows
from test_gpu_batch import SM_VARIANTS, cfg_synth, weights

_PAD = {60: 64, 128: 128, 256: 256}
KS = (1, 5, 16)


def want_story_rows(probs, row_off, max_slots, k):
    """probs float32 [H][rows] (the tap) -> (top_slot uint32 [B][H][k], top_p float32 [B][H][k])"""
    H = probs.shape[0]
    B = len(row_off) - 1
    slot = np.full((B, H, k), PAD_SLOT, np.uint32)
    p = np.zeros((B, H, k), np.float32)
    for q in range(B):
        r0 = int(row_off[q])
        S = min(int(row_off[q + 1]) - r0, max_slots)
        s1, p1 = want_rows(probs[:, None, r0:r0 + S], k)
        slot[q], p[q] = s1[0], p1[0]
    return slot, p


def assert_story_rows(got_slot, got_p, probs, row_off, max_slots, k, what):
    """got_slot int32 / got_p float32 device tensors [B][H][k] against the yardstick: slots exactly, probabilities by bit pattern"""
    w_slot, w_p = want_story_rows(probs, row_off, max_slots, k)
    g_slot = got_slot.cpu().numpy().view(np.uint32)
    g_p = got_p.cpu().numpy()
    assert g_slot.shape == w_slot.shape and g_p.shape == w_p.shape, what
    np.testing.assert_array_equal(g_slot, w_slot, err_msg=f"{what}: top_slot, k={k}")
    np.testing.assert_array_equal(g_p.view(np.uint32), w_p.view(np.uint32), err_msg=f"{what}: top_p bits, k={k}")


# ---- configurations -----------------------------------------------------------------------------------------------------------------
def cfg_ham(mode, D, num_bit=8, iwl=5, mq=False):
    """run_hamming_case's configuration"""
    H, frac = 3, 7 - iwl
    fmt = [(iwl, frac)] * H
    cfg = dict(n_hop=H, dim_emb=D, dim_input=40, attention_mode=mode, softmax_variant=0, f_fixed=True, en_lin_map=True, fmt=fmt,
               fmt_w=list(fmt), fmt_att=list(fmt), fmt_bin=(iwl, frac), num_bit=num_bit)
    if mq:
        cfg["fmt_w"] = [(iwl + 1, frac - 1), (iwl, frac), (iwl - 1, frac + 1)]
    return cfg


def _ham_variant(name):
    extra = dict(SM_VARIANTS[name])
    if name == "exp_shift_scaled":
        extra["att_scale"] = [0.002, 0.001, 0.0015]       # (Hamming scores span hundreds of units: test_hops_softmax_variants)
    return extra


Q25 = dict(sigma_u=6.0, sigma_k=6.0, sigma_h=6.0 / 32.0)
BIN_RELU = dict(fmt_bin=(0, 0), en_non_lin=True)

# 1. the one-wavefront kernel: every story length class of it in one batch
WAVE_S = [0, 1, 2, 15, 16, 17, 33, 50, 63, 64]
WAVE = {
    "fixed_D60": dict(cfg=cfg_synth(60, 40, 5)),
    "fixed_D128_q25": dict(cfg=cfg_synth(128, 40, 2), **Q25),
    "fixed_D256": dict(cfg=cfg_synth(256, 40, 5)),
    "fixed_D60_en_mq": dict(cfg=cfg_synth(60, 30, 5, fmt_w=[(6, 1), (5, 2), (4, 3)]), sigma_u=90.0, sigma_k=60.0, sigma_h=4.0),
    "fixed_D128_wl6": dict(cfg=dict(cfg_synth(128, 40, 5), fmt_att=[(4, 2)] * 3, fmt=[(3, 2)] * 3, fmt_bin=(4, 2))),
    **{f"fixed_D60_{v}": dict(cfg=dict(cfg_synth(60, 40, 5), **SM_VARIANTS[v])) for v in sorted(SM_VARIANTS)},
    "fixed_D128_exp_plan": dict(cfg=dict(cfg_synth(128, 40, 5), **SM_VARIANTS["exp_plan"])),
    "fixed_D256_pow2_shift": dict(cfg=dict(cfg_synth(256, 40, 5), **SM_VARIANTS["pow2_shift"])),
    "fixed_D60_binary_relu": dict(cfg=dict(cfg_synth(60, 40, 5), **BIN_RELU)),
    "fixed_D128_binary_relu": dict(cfg=dict(cfg_synth(128, 40, 5), **BIN_RELU)),
    "appx_D60": dict(cfg=cfg_ham(3, 60)),
    "appx_D128": dict(cfg=cfg_ham(3, 128)),
    "appx_D256": dict(cfg=cfg_ham(3, 256)),
    "appx_D60_en_mq": dict(cfg=cfg_ham(3, 60, mq=True)),
    "appx_D128_en_mq": dict(cfg=cfg_ham(3, 128, mq=True)),
    "appx_D60_exp_plan": dict(cfg=dict(cfg_ham(3, 60), **_ham_variant("exp_plan"))),
    "appx_D128_scale_negative": dict(cfg=dict(cfg_ham(3, 128), **_ham_variant("scale_negative"))),
    "v0_D60_nb8": dict(cfg=cfg_ham(10, 60, 8)),
    "v0_D128_nb2": dict(cfg=cfg_ham(10, 128, 2)),
    "v0_D256_nb2": dict(cfg=cfg_ham(10, 256, 2)),
    "v0_D60_nb2_pow2_shift": dict(cfg=dict(cfg_ham(10, 60, 2), **_ham_variant("pow2_shift"))),
    "v0_D128_nb8_exp_shift_scaled": dict(cfg=dict(cfg_ham(10, 128, 8), **_ham_variant("exp_shift_scaled"))),
    "v1_D60_nb2": dict(cfg=cfg_ham(11, 60, 2)),
    "v1_D128_nb8": dict(cfg=cfg_ham(11, 128, 8)),
    "v1_D256_nb8": dict(cfg=cfg_ham(11, 256, 8)),
    "v1_D60_nb8_scale_pow2": dict(cfg=dict(cfg_ham(11, 60, 8), **_ham_variant("scale_pow2"))),
    "v1_D128_nb2_scale_negative": dict(cfg=dict(cfg_ham(11, 128, 2), **_ham_variant("scale_negative"))),
    "v1_D60_nb8_binary_relu": dict(cfg=dict(cfg_ham(11, 60, 8), **BIN_RELU)),
}
for _i, _c in enumerate(WAVE.values()):
    _c.update(S_list=WAVE_S, max_slots=64, seed=9100 + _i)

# 2. the streaming kernel, fixed-point: one wavefront per query up to 256 slots, four beyond (4097: a second chunk of the walk)
ONE_WAVE_S, FOUR_WAVES_S = [65, 66, 255, 256], [257, 300, 4097]
STREAM = {}
for _j, (_S, _ms) in enumerate(((ONE_WAVE_S, 256), (FOUR_WAVES_S, 4097))):
    _t = f"ms{_ms}"
    STREAM.update({
        f"D60_{_t}": dict(cfg=cfg_synth(60, 40, 5)),
        # Q2.5, e^x: hops_host.h::scan_stop_gate accepts a plain call of 4097 rows (1 720 suffice); the TOP call must ignore it
        f"D128_q25_{_t}": dict(cfg=cfg_synth(128, 40, 2), **Q25),
        f"D256_q25_{_t}": dict(cfg=cfg_synth(256, 40, 2), **Q25),
        f"D128_wl6_{_t}": dict(cfg=dict(cfg_synth(128, 40, 5), fmt_att=[(4, 2)] * 3, fmt=[(3, 2)] * 3, fmt_bin=(4, 2))),
        f"D128_exp_plan_{_t}": dict(cfg=dict(cfg_synth(128, 40, 5), **SM_VARIANTS["exp_plan"])),
        f"D60_pow2_shift_{_t}": dict(cfg=dict(cfg_synth(60, 40, 5), **SM_VARIANTS["pow2_shift"])),
        f"D60_scale_negative_{_t}": dict(cfg=dict(cfg_synth(60, 40, 5), **SM_VARIANTS["scale_negative"])),
        f"D256_binary_relu_{_t}": dict(cfg=dict(cfg_synth(256, 40, 5), **BIN_RELU)),
    })
    for _i, _n in enumerate(n for n in STREAM if n.endswith(_t)):
        STREAM[_n].update(S_list=_S, max_slots=_ms, seed=9300 + 20 * _j + _i)

# 4. stories longer than the caller's bound: (true length, max_slots)
CUT = {
    "fixed_80_64": dict(cfg=cfg_synth(60, 40, 5), S_list=[80, 64, 3, 80], max_slots=64, seed=9401),
    "appx_80_64": dict(cfg=cfg_ham(3, 128), S_list=[80, 64, 3, 80], max_slots=64, seed=9402),
    "v1_80_64": dict(cfg=cfg_ham(11, 60, 8), S_list=[80, 64, 3, 80], max_slots=64, seed=9403),
    "fixed_100_70": dict(cfg=cfg_synth(128, 40, 5), S_list=[100, 70, 3, 100], max_slots=70, seed=9404),
    "fixed_400_300": dict(cfg=cfg_synth(60, 40, 2), S_list=[400, 300, 3, 400], max_slots=300, seed=9405, **Q25),
}

# 5. tied hops: ONE plane
TIED = {
    "fixed_small": dict(cfg=cfg_synth(60, 40, 2), S_list=[0, 1, 9, 50, 64], max_slots=64, seed=9501, tied=True, **Q25),
    "v1_small": dict(cfg=cfg_ham(11, 128, 4), S_list=[0, 1, 9, 50, 64], max_slots=64, seed=9502, tied=True),
    "fixed_one_wave": dict(cfg=cfg_synth(128, 40, 5), S_list=[65, 200, 7], max_slots=256, seed=9503, tied=True),
    "fixed_four_waves": dict(cfg=cfg_synth(128, 40, 2), S_list=[257, 700, 7], max_slots=700, seed=9504, tied=True, **Q25),
}

CASES = {**{f"wave_{n}": c for n, c in WAVE.items()}, **{f"stream_{n}": c for n, c in STREAM.items()},
         **{f"cut_{n}": c for n, c in CUT.items()}, **{f"tied_{n}": c for n, c in TIED.items()}}


def _batch(cfg, wts, S_list, max_slots, keys, vals, u0, tied=False):
    row_off = np.concatenate([[0], np.cumsum(S_list)]).astype(np.int32)
    return dict(cfg=cfg, weights=wts, keys=keys, vals=vals, u0=u0, row_off=row_off, max_slots=max_slots, n_query=len(S_list), tied=tied)


@functools.lru_cache(maxsize=None)
def story_case(name):
    """-> dict(cfg, weights, keys, vals, u0, row_off, max_slots, n_query, tied): keys / vals int8 integer codes [planes][rows][Dp]
    (two's complement; the library wants sign-magnitude bytes: model.to_signmag), u0 float32 [n_query][D]"""
    c = CASES[name]
    cfg, S_list = c["cfg"], c["S_list"]
    H, D, V = cfg["n_hop"], cfg["dim_emb"], cfg["dim_input"]
    Dp, B, R = _PAD[D], len(S_list), max(int(sum(S_list)), 1)
    ham = cfg["attention_mode"] != 2
    sigma_k = c.get("sigma_k", 40.0 if ham else 30.0)
    rng = np.random.default_rng(c["seed"])
    wts = weights(c["seed"], H, D, V, c.get("sigma_h", 1.0), with_emb=False)
    P = 1 if c.get("tied") else H
    keys = np.zeros((P, R, Dp), np.int8)
    vals = np.zeros((P, R, Dp), np.int8)
    keys[:, :, :D] = np.clip(np.rint(rng.normal(0, sigma_k, (P, R, D))), -127, 127)
    vals[:, :, :D] = np.clip(np.rint(rng.normal(0, sigma_k, (P, R, D))), -127, 127)
    if ham:                                              # magnitude ties, zeros and full-scale values, as run_hamming_case plants them
        keys[:, ::3, : D // 2] = np.clip(keys[:, ::3, : D // 2].astype(np.int16) * 3, -127, 127)
        keys[:, 1::5, ::4] = 0
    for p in range(P):                                   # valid codes of the formats that read the plane (every hop's, when tied)
        hops = range(H) if c.get("tied") else [p]
        mv = min((1 << sum(cfg["fmt"][h])) - 1 for h in hops)
        vals[p] = np.clip(vals[p], -mv, mv)
        if not ham:
            mk = min((1 << sum(cfg["fmt_att"][h])) - 1 for h in hops)
            keys[p] = np.clip(keys[p], -mk, mk)
    w0 = cfg["fmt_w"][0]
    m0 = (1 << sum(w0)) - 1
    u0 = (np.clip(np.rint(rng.normal(0, c.get("sigma_u", 40.0 if ham else 20.0), (B, D))), -m0, m0) / (1 << w0[1])).astype(np.float32)
    return _batch(cfg, wts, S_list, c["max_slots"], keys, vals, u0, bool(c.get("tied")))


# ---- 3. planted ties and all-zero stories ---------------------------------------------------------------------------------------------
PLANT_POS = [5, 7, 63, 64, 255, 256, 4095, 4096, 4097, 4098]     # code +127 in every column where the story has the row
PLANT_NEG = [1, 3]                                                # code -127
PLANT_GROUPS = {"wave": ([20, 50, 64], 64), "one_wave": ([65, 200, 256], 256), "four_waves": ([257, 300, 4099], 4099)}
ZERO_GROUPS = {"wave": ([1, 5, 16, 17, 64], 64), "one_wave": ([1, 5, 16, 17, 64, 65], 256), "four_waves": ([1, 5, 16, 17, 64, 65, 257], 257)}


def planted_rows(S):
    """(rows at +127, rows at -127, every other row) of a planted story of S rows"""
    pos = [r for r in PLANT_POS if r < S]
    return pos, list(PLANT_NEG), [r for r in range(S) if r not in pos and r not in PLANT_NEG]


@functools.lru_cache(maxsize=None)
def planted_story_case(base, group):
    """per-story form of attended_cases.planted_case: keys all zero but for the planted rows of every story, vals random codes
    (sigma 6), u0 every column at the top code of its grid.  At hop 0 every other row scores 0."""
    S_list, max_slots = PLANT_GROUPS[group]
    cfg = cfg_synth(60, 40, 2, base=base)
    H, D, V, Dp = 3, 60, 40, 64
    R, B = sum(S_list), len(S_list)
    rng = np.random.default_rng(9600 + base)
    keys = np.zeros((H, R, Dp), np.int8)
    vals = np.zeros((H, R, Dp), np.int8)
    vals[:, :, :D] = np.clip(np.rint(rng.normal(0, 6.0, (H, R, D))), -127, 127)
    r0 = 0
    for S in S_list:
        pos, neg, _ = planted_rows(S)
        keys[:, [r0 + r for r in pos], :D] = 127
        keys[:, [r0 + r for r in neg], :D] = -127
        r0 += S
    u0 = np.full((B, D), 127.0 / (1 << cfg["fmt_w"][0][1]), np.float32)
    return _batch(cfg, weights(9600 + base, H, D, V, 6.0 / 32.0, with_emb=False), S_list, max_slots, keys, vals, u0)


@functools.lru_cache(maxsize=None)
def zero_story_case(group):
    """all-zero stories: every score is 0 at every hop, every probability of a story equal"""
    S_list, max_slots = ZERO_GROUPS[group]
    cfg = cfg_synth(60, 40, 2)
    H, D, V, Dp = 3, 60, 40, 64
    R, B = sum(S_list), len(S_list)
    rng = np.random.default_rng(9700 + max_slots)
    u0 = (np.clip(np.rint(rng.normal(0, 6.0, (B, D))), -127, 127) / 32.0).astype(np.float32)
    return _batch(cfg, weights(9700 + max_slots, H, D, V, 6.0 / 32.0, with_emb=False), S_list, max_slots, np.zeros((H, R, Dp), np.int8),
                  np.zeros((H, R, Dp), np.int8), u0)

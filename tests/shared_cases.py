"""The seeded inputs of the shared-plane tests (qmann_hops_shared_i8: one memory, many queries) -- ONE definition, read by the
GPU test (test_gpu_shared.py) and by the CPU precondition test (test_shared_inputs.py), so both see the same bytes.
Not collected by pytest (no test_ prefix).

A case is a net configuration, one memory of S slots (keys / vals as integer codes, [planes][S][Dp], planes = n_hop or 1 for
tied hops) and n_query question embeddings u0.  Codes are drawn as run_case in test_gpu_batch.py draws them: clip(round(N(0,
sigma))) cut to the valid codes of the format, u0 on hop 0's weight grid."""
from __future__ import annotations

import functools
import itertools

import numpy as np

from test_gpu_batch import cfg_synth, weights

_PAD = {60: 64, 64: 64, 128: 128, 256: 256}


def _case(cfg, S, n_query, seed, sigma_u=20.0, sigma_k=30.0, sigma_h=1.0, tied=False, extra=None):
    return dict(cfg=dict(cfg, **(extra or {})), S=S, n_query=n_query, seed=seed, sigma_u=sigma_u, sigma_k=sigma_k, sigma_h=sigma_h,
                tied=tied)


# grid cases whose first seed put an oracle probability on a truncation step of Q(p) (test_shared_inputs.py): seed + bump
SEED_BUMP = {(2, 60, 17): 15000}


def _grid():
    """S x D x n_query thinned to 36 combinations: every S, every D and every n_query appear, in varying company.
    Format Q2.5 with the code spread of bench.py's synth10k_d128_q25 (sigma 6): scores stay inside +-3.97, so even a memory of
    two slots has no weight within 1e-5 of 1 (with Q5.2 and wide codes a short memory's best slot takes p = 1 - 1e-9, which IS a
    truncation step, and saturated scores tie into p = 1/2, 1/4)."""
    S_list = [1, 2, 15, 16, 17, 63, 64, 65, 255, 257, 1000, 4097]
    out = {}
    for (i, S), (j, D), (k, nq) in itertools.product(enumerate(S_list), enumerate([60, 128, 256]), enumerate([1, 3, 5, 17])):
        if (i + j + k) % 4 == 0:
            out[f"grid_S{S}_D{D}_q{nq}"] = _case(cfg_synth(D, 40, 2), S, nq, 7000 + 100 * i + 10 * j + k + SEED_BUMP.get((S, D, nq), 0),
                                                 sigma_u=6.0, sigma_k=6.0, sigma_h=6.0 / 32.0)
    return out


CASES = {
    # BASELINE config 4's shape, 9 queries: a tail tile for every tile size in {2, 4, 8}; the two code spreads of
    # test_hops_full_size_memory_q25_as_specified and test_hops_full_size_memory
    "config4_q25": _case(cfg_synth(128, 256, 2), 10000, 9, 8001, sigma_u=6.0, sigma_k=6.0, sigma_h=6.0 / 32.0),
    "config4_q52": _case(cfg_synth(128, 256, 5), 10000, 9, 8002, sigma_u=12.0, sigma_k=20.0),
    # EN_MQ per-hop weight formats, the per-product clamp path forced (test_hops_en_mq_formats_and_clamp_path)
    "en_mq_clamp": _case(cfg_synth(60, 30, 5, fmt_w=[(6, 1), (5, 2), (4, 3)]), 300, 7, 8003, sigma_u=90.0, sigma_k=60.0, sigma_h=4.0),
    "q70": _case(cfg_synth(64, 30, 7), 200, 5, 8004, sigma_u=3.0, sigma_k=3.0),
    # word length 6 in the attention format of every hop (not the W7 form), 5 in the activations
    "wl6": _case(dict(cfg_synth(128, 40, 5), fmt_att=[(4, 2)] * 3, fmt=[(3, 2)] * 3, fmt_bin=(4, 2)), 500, 6, 8005),
    "wl_mixed": _case(dict(cfg_synth(60, 40, 5), fmt_att=[(5, 2), (3, 2), (2, 5)], fmt_w=[(4, 3), (2, 3), (5, 2)]), 130, 5, 8006),
    "pow2": _case(cfg_synth(128, 64, 5, base=1), 257, 6, 8007),
    "exp_plan": _case(cfg_synth(128, 40, 5, base=2), 300, 6, 8008),
    "pow2_shift": _case(cfg_synth(128, 40, 5), 300, 6, 8009, extra=dict(softmax_variant=1, softmax_shift_based=True)),
    "exp_shift_scaled": _case(cfg_synth(128, 40, 5), 300, 6, 8010,
                              extra=dict(softmax_variant=0, softmax_shift_based=True, att_scale=[0.02, 0.015, 0.03])),
    "scale_negative": _case(cfg_synth(60, 40, 5), 1000, 5, 8011, extra=dict(att_scale=[-0.5, 0.25, -0.125])),
    "relu": _case(cfg_synth(128, 40, 5), 300, 6, 8012, extra=dict(en_non_lin=True)),
    "binary": _case(cfg_synth(128, 40, 5), 300, 6, 8013, extra=dict(fmt_bin=(0, 0))),
    "binary_relu": _case(cfg_synth(60, 40, 5), 70, 6, 8014, extra=dict(fmt_bin=(0, 0), en_non_lin=True)),
    "no_lin_map": _case(cfg_synth(128, 40, 5), 300, 6, 8015, extra=dict(en_lin_map=False)),
    "one_hop": _case(cfg_synth(128, 40, 5, H=1), 300, 6, 8016),
    "eight_hops": _case(cfg_synth(60, 40, 5, H=8), 130, 5, 8017),
    "tied": _case(cfg_synth(128, 40, 5), 700, 11, 8018, tied=True),
    "tied_short": _case(cfg_synth(60, 40, 2), 9, 4, 8019, sigma_u=6.0, sigma_k=6.0, sigma_h=6.0 / 32.0, tied=True),
    # the tile sizes, forced: 19 queries leave a tail of 1 (tiles of 2), 3 (4 and 8)
    "tiles": _case(cfg_synth(128, 40, 5), 1500, 19, 8020),
    **_grid(),
}


@functools.lru_cache(maxsize=None)
def shared_case(name):
    """-> dict(cfg, weights, keys, vals, u0, S, n_query, tied): keys / vals int8 integer codes [planes][S][Dp] (two's complement;
    the library wants them as sign-magnitude bytes: model.to_signmag), u0 float32 [n_query][D]"""
    c = CASES[name]
    cfg, S, B = c["cfg"], c["S"], c["n_query"]
    H, D, V = cfg["n_hop"], cfg["dim_emb"], cfg["dim_input"]
    Dp = _PAD[D]
    rng = np.random.default_rng(c["seed"])
    wts = weights(c["seed"], H, D, V, c["sigma_h"], with_emb=False)
    P = 1 if c["tied"] else H
    keys = np.zeros((P, S, Dp), np.int8)
    vals = np.zeros((P, S, Dp), np.int8)
    keys[:, :, :D] = np.clip(np.rint(rng.normal(0, c["sigma_k"], (P, S, D))), -127, 127)
    vals[:, :, :D] = np.clip(np.rint(rng.normal(0, c["sigma_k"], (P, S, D))), -127, 127)
    for p in range(P):                                   # valid codes of the formats that read the plane (every hop's, when tied)
        hops = range(H) if c["tied"] else [p]
        mk = min((1 << sum(cfg["fmt_att"][h])) - 1 for h in hops)
        mv = min((1 << sum(cfg["fmt"][h])) - 1 for h in hops)
        keys[p] = np.clip(keys[p], -mk, mk)
        vals[p] = np.clip(vals[p], -mv, mv)
    u0 = (np.clip(np.rint(rng.normal(0, c["sigma_u"], (B, D))), -127, 127) / (1 << cfg["fmt_w"][0][1])).astype(np.float32)
    return dict(cfg=cfg, weights=wts, keys=keys, vals=vals, u0=u0, S=S, n_query=B, tied=c["tied"])


def memory_floats(case):
    """the memory as the oracle takes it: kf, vf float32 [n_hop][S][D] on the attention / activation grids"""
    cfg, keys, vals = case["cfg"], case["keys"], case["vals"]
    H, D = cfg["n_hop"], cfg["dim_emb"]
    plane = (lambda h: 0) if case["tied"] else (lambda h: h)
    kf = np.stack([keys[plane(h), :, :D].astype(np.float32) / (1 << cfg["fmt_att"][h][1]) for h in range(H)])
    vf = np.stack([vals[plane(h), :, :D].astype(np.float32) / (1 << cfg["fmt"][h][1]) for h in range(H)])
    return kf, vf


@functools.lru_cache(maxsize=None)
def oracle_taps(name):
    """Oracle.forward_mem of every query of a case against the one memory: a list of (pred, taps) -- computed once per process"""
    from pyoracle import Oracle
    case = shared_case(name)
    ora = Oracle()
    m = ora.make_model(case["cfg"], case["weights"])
    kf, vf = memory_floats(case)
    return [ora.forward_mem(m, kf, vf, case["u0"][q]) for q in range(case["n_query"])]

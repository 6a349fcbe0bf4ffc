"""The seeded inputs of the shared-plane Hamming tests (qmann_hops_shared_packed: one packed memory, many queries) -- ONE
definition, read by the GPU test (test_gpu_shared_ham.py) and by the CPU precondition test (test_shared_ham_inputs.py), so both
see the same bytes.  Not collected by pytest (no test_ prefix).

A case is a net configuration of mode 10 (V0) or 11 (V1), one memory of S slots (key BYTES sign-magnitude [planes][S][Dp], the
floats the oracle takes for them, value codes [planes][S][Dp]; planes = n_hop, or 1 for tied hops) and n_query question
embeddings u0.  Keys are built as run_hamming_case (test_gpu_batch.py) builds them: N(0, sigma) codes with magnitude ties,
zeros and full-scale codes; under EN_MQ weight formats they are floats on their hop's weight grid and the bytes follow
ham_key_bytes.

CLUSTERED memories: random Hamming scores make the softmax nearly one-hot -- the read-out then has a single survivor.  In a
clustered memory row r (r < 7 n_query) is the attention byte code of query (r // 7) % n_query with r % 7 of its compared bits
flipped, so that several slots survive Q(p); the remaining rows are random.  Those cases use Q2.5 (a weight survives from 1/32)."""
from __future__ import annotations

import functools
import itertools

import numpy as np

from test_gpu_batch import ham_key_bytes, weights

_PAD = {60: 64, 64: 64, 128: 128, 256: 256}
V = 40


def _cfg(mode, D, num_bit, iwl=5, H=3, base=0, mq=False):
    frac = 7 - iwl
    fmt = [(iwl, frac)] * H
    cfg = dict(n_hop=H, dim_emb=D, dim_input=V, attention_mode=mode, softmax_variant=base, f_fixed=True, en_lin_map=True,
               fmt=fmt, fmt_w=list(fmt), fmt_att=list(fmt), fmt_bin=(iwl, frac), num_bit=num_bit)
    if mq:
        cfg["fmt_w"] = [(iwl + 1, frac - 1), (iwl, frac), (iwl - 1, frac + 1)]
    return cfg


def _case(mode, D, num_bit, S, n_query, seed, iwl=5, H=3, base=0, mq=False, clustered=False, tied=False, sigma=40.0, extra=None):
    assert not (mq and (clustered or tied))
    return dict(cfg=dict(_cfg(mode, D, num_bit, 2 if clustered else iwl, H, base, mq), **(extra or {})), S=S, n_query=n_query,
                seed=seed, mq=mq, clustered=clustered, tied=tied, sigma=sigma)


# cases whose first seed put an oracle probability on a truncation step of Q(p) (test_shared_ham_inputs.py): seed + bump
SEED_BUMP = {"binary_v0": 2000, "eight_hops_v0": 24000, "en_mq_v0": 5000, "grid_D128_b1_S2_q3_m10": 3000,
             "grid_D128_b8_S257_q5_m10": 29000, "grid_D128_b8_S2_q17_m10": 22000, "grid_D128_b8_S32_q3_m10": 3000,
             "grid_D60_b8_S257_q17_m10": 4000, "grid_D60_b8_S63_q5_m10": 1000, "grid_D60_b8_S65_q1_m10": 1000, "pow2_v0": 1000,
             "relu_v0": 3000}
# Grid cases that no seed in sixty cleared: V0 scores are integers and e^x is steep, so the best of a few random rows is 12 to 20
# counts ahead of the second in some hop of some of 17 queries almost surely -- p = 1 - 1e-6 .. 1 - 1e-9, inside 1e-5 of the step
# at 1 and not one-hot.  They take a scale layer (1/8, 1/16, 1/16), which flattens the softmax; the scan, which is what the grid
# is for, does not see it.
GRID_SCALED = ("grid_D128_b8_S129_q17_m10", "grid_D256_b1_S2_q5_m10", "grid_D256_b2_S64_q17_m10", "grid_D60_b8_S2_q17_m10")

# (D, num_bit) -> lanes per key row LPRK = (Dp / 64) num_bit / 2 from 1 to 16; a wavefront's tile is 256 / LPRK rows
SHAPES = [(60, 8), (64, 2), (128, 1), (128, 4), (128, 8), (256, 1), (256, 2), (256, 8)]


def _grid():
    """(D, num_bit) x S x n_query thinned as shared_cases._grid() thins: every value appears, in varying company.  S: below, at
    and beyond one tile of rows of the shape, and several tiles with a clamped last one.  A single plane (num_bit 1) takes V0
    only here: its V1 scores are all zero, p = 1 / S, which is a truncation step at S = 2 (V1 with one bit: the named case)."""
    out = {}
    for (j, (D, nb)) in enumerate(SHAPES):
        tile = 256 // ((_PAD[D] // 64) * nb * 8 // 16)
        S_list = [1, 2, tile - 1, tile, tile + 1, 4 * tile + 1, 8 * tile + 1]
        for (i, S), (k, nq) in itertools.product(enumerate(S_list), enumerate([1, 3, 5, 17])):
            if (i + j + k) % 4:
                continue
            mode = 10 if nb == 1 else 10 + (i + k) % 2
            name = f"grid_D{D}_b{nb}_S{S}_q{nq}_m{mode}"
            out[name] = _case(mode, D, nb, S, nq, 9000 + 100 * j + 10 * i + k, clustered=S >= 3 and (j + k) % 2 == 0,
                              extra=dict(att_scale=[0.125, 0.0625, 0.0625]) if name in GRID_SCALED else None)
    return out


CASES = {
    # BASELINE config 5's shape, 9 queries: a tail tile for every tile size in {2, 4, 8}
    "config5_v0_b1": _case(10, 256, 1, 10000, 9, 9901, clustered=True),
    "config5_v1_b8": _case(11, 256, 8, 10000, 9, 9902, clustered=True, sigma=25.0),
    # the tile sizes, forced: 19 queries leave a tail of 1 (tiles of 2), 3 (4 and 8)
    "tiles_v0": _case(10, 128, 4, 1500, 19, 9903, clustered=True),
    "tiles_v1": _case(11, 128, 8, 700, 19, 9904, clustered=True),
    "tied_v0": _case(10, 128, 2, 700, 11, 9905, tied=True, clustered=True),
    "tied_v1": _case(11, 60, 8, 130, 4, 9906, tied=True),
    "pow2_v0": _case(10, 128, 4, 257, 6, 9907, base=1, clustered=True),
    "pow2_v1": _case(11, 128, 8, 300, 6, 9908, base=1),
    "exp_plan_v0": _case(10, 60, 8, 300, 6, 9909, base=2),
    "exp_plan_v1": _case(11, 128, 4, 300, 6, 9910, base=2, clustered=True),
    "pow2_shift_v0": _case(10, 128, 2, 300, 6, 9911, clustered=True, extra=dict(softmax_variant=1, softmax_shift_based=True)),
    # (shift-based e^x divides by an integer: the best slot's weight is exactly 1 / llrint(log2(total)) -- a truncation step
    # unless the total is large; small scales keep the softmax flat, as shared_cases.py does)
    "exp_shift_scaled_v1": _case(11, 128, 8, 300, 6, 9912,
                                 extra=dict(softmax_variant=0, softmax_shift_based=True, att_scale=[0.02, 0.015, 0.03])),
    "scale_negative_v0": _case(10, 60, 8, 1000, 5, 9913, clustered=True, extra=dict(att_scale=[-0.5, 0.25, -0.125])),
    "scale_negative_v1": _case(11, 256, 2, 300, 5, 9914, extra=dict(att_scale=[-0.5, 0.25, -0.125])),
    "relu_v0": _case(10, 128, 8, 300, 6, 9915, clustered=True, extra=dict(en_non_lin=True)),
    "relu_v1": _case(11, 128, 4, 300, 6, 9916, extra=dict(en_non_lin=True)),
    "binary_v0": _case(10, 128, 4, 300, 6, 9917, extra=dict(fmt_bin=(0, 0))),
    "binary_v1": _case(11, 60, 8, 70, 6, 9918, clustered=True, extra=dict(fmt_bin=(0, 0), en_non_lin=True)),
    "no_lin_map_v0": _case(10, 128, 2, 300, 6, 9919, clustered=True, extra=dict(en_lin_map=False)),
    "no_lin_map_v1": _case(11, 128, 8, 300, 6, 9920, extra=dict(en_lin_map=False)),
    "one_hop_v1": _case(11, 128, 8, 300, 6, 9921, H=1, clustered=True),
    "eight_hops_v0": _case(10, 60, 8, 130, 5, 9922, H=8),
    "en_mq_v0": _case(10, 128, 8, 300, 7, 9923, mq=True),
    "en_mq_v1": _case(11, 256, 8, 500, 7, 9924, mq=True),
    "en_mq_v1_b4": _case(11, 60, 4, 200, 5, 9925, mq=True, iwl=3),
    # V1 on a single plane: every score is zero, p = 1 / S
    "v1_one_bit": _case(11, 128, 1, 300, 5, 9926),
    **_grid(),
}


def att_bytes(u, att):
    """sign-magnitude attention bytes of float values (ham_common.h::ham_ubyte)"""
    return ham_key_bytes(np.asarray(u, np.float32), 10, "same", att, att).view(np.uint8)


@functools.lru_cache(maxsize=None)
def shared_ham_case(name):
    """-> dict(cfg, weights, key_bytes, key_floats, vals, u0, S, n_query, tied, unit): key_bytes int8 sign-magnitude
    [planes][S][Dp] (what qmann_pack_bitplanes packs), key_floats[h] float32 [S][D] (what the oracle takes), vals int8 integer
    codes [planes][S][Dp] (two's complement: model.to_signmag for the library), u0 float32 [n_query][D], unit: a score code's
    value (1 for V0, 2^-num_bit for V1)"""
    c = CASES[name]
    cfg, S, B = c["cfg"], c["S"], c["n_query"]
    H, D, nb, mode = cfg["n_hop"], cfg["dim_emb"], cfg["num_bit"], cfg["attention_mode"]
    Dp = _PAD[D]
    sigma = c["sigma"]
    seed = c["seed"] + SEED_BUMP.get(name, 0)
    rng = np.random.default_rng(seed)
    wts = weights(seed, H, D, V, 1.0, with_emb=False)
    P = 1 if c["tied"] else H
    w0 = cfg["fmt_w"][0]                             # u0 is an emb_q output: on the Q(w[0]) grid
    m0 = (1 << sum(w0)) - 1
    u0 = (np.clip(np.rint(rng.normal(0, sigma, (B, D))), -m0, m0) / (1 << w0[1])).astype(np.float32)
    u0[:, ::7] = np.float32(m0 / (1 << w0[1])) * np.sign(u0[:, ::7] + 0.1)
    vals = np.zeros((P, S, Dp), np.int8)
    vals[:, :, :D] = np.clip(np.rint(rng.normal(0, sigma, (P, S, D))), -127, 127)
    for p in range(P):                               # value codes must be codes of the activation format (every hop's, when tied)
        mv = min((1 << sum(cfg["fmt"][h])) - 1 for h in (range(H) if c["tied"] else [p]))
        vals[p] = np.clip(vals[p], -mv, mv)
    key_bytes = np.zeros((P, S, Dp), np.uint8)
    key_floats = []
    if c["mq"]:
        iwl = cfg["fmt_att"][0][0]
        edge = np.float32(1 << iwl)                  # 2^iwl_att: +edge saturates the operand word, -edge is its minus zero
        u0[:, 3::11] = -edge; u0[:, 5::13] = edge; u0[:, 6::17] = -edge - np.float32(0.5)
        for h in range(H):
            wk, att = cfg["fmt_w"][h], cfg["fmt_att"][h]
            mk = (1 << sum(wk)) - 1
            kf = np.zeros((S, Dp), np.float32)
            kf[:, :D] = np.clip(np.rint(rng.normal(0, sigma, (S, D))), -mk, mk) / np.float32(1 << wk[1])
            kf[::3, : D // 2] = np.clip(kf[::3, : D // 2] * 3, -mk / (1 << wk[1]), mk / (1 << wk[1]))
            kf[1::5, :D:4] = 0
            if wk[0] > att[0]:
                kf[2::7, 1:D:5] = -edge; kf[4::9, 2:D:6] = edge; kf[::4, 3:D:9] = np.float32(mk / (1 << wk[1]))
            key_bytes[h] = ham_key_bytes(kf, mode, "same", wk, att).view(np.uint8)
            key_bytes[h, :, D:] = 0
            key_floats.append(kf[:, :D].copy())
    else:
        codes = np.zeros((P, S, Dp), np.int16)
        codes[:, :, :D] = np.clip(np.rint(rng.normal(0, sigma, (P, S, D))), -127, 127)
        # magnitude ties, zeros and full-scale values
        codes[:, ::3, : D // 2] = np.clip(codes[:, ::3, : D // 2] * 3, -127, 127)
        codes[:, 1::5, ::4] = 0
        key_bytes[:] = np.where(codes < 0, (-codes) | 0x80, codes).astype(np.uint8)
        if c["clustered"]:
            ub = att_bytes(u0, cfg["fmt_att"][0])                       # [B][D]
            for p in range(P):
                for r in range(min(S, 7 * B)):
                    row = ub[(r // 7) % B].copy()
                    pos = rng.choice(D * nb, size=r % 7, replace=False)   # (column, plane) positions among the compared bits
                    for x in pos:
                        row[x // nb] ^= np.uint8(0x80 >> (x % nb))
                    row[row == 0x80] = 0                                # (no minus zero: the oracle takes the float, whose sign it reads)
                    key_bytes[p, r, :D] = row
        frac_att = cfg["fmt_att"][0][1]
        dec = np.where(key_bytes & 0x80, -(key_bytes & 0x7F).astype(np.float32), (key_bytes & 0x7F).astype(np.float32))
        for h in range(H):
            key_floats.append((dec[0 if c["tied"] else h, :, :D] / np.float32(1 << frac_att)).astype(np.float32))
    return dict(cfg=cfg, weights=wts, key_bytes=key_bytes.view(np.int8), key_floats=key_floats, vals=vals, u0=u0, S=S, n_query=B,
                tied=c["tied"], clustered=c["clustered"], unit=1.0 if mode == 10 else 1.0 / (1 << nb))


@functools.lru_cache(maxsize=None)
def oracle_taps(name):
    """Oracle.forward_mem of every query of a case against the one memory: a list of (pred, taps) -- computed once per process"""
    from pyoracle import Oracle
    case = shared_ham_case(name)
    cfg = case["cfg"]
    H, D = cfg["n_hop"], cfg["dim_emb"]
    ora = Oracle()
    m = ora.make_model(cfg, case["weights"])
    kf = np.stack(case["key_floats"])
    vf = np.stack([case["vals"][0 if case["tied"] else h, :, :D].astype(np.float32) / (1 << cfg["fmt"][h][1]) for h in range(H)])
    return [ora.forward_mem(m, kf, vf, case["u0"][q]) for q in range(case["n_query"])]


# ---- the model-level pairs (test_gpu_shared_ham.py section 3) -------------------------------------------------------------------
MODEL_SOURCES = ("trained_qa1", "random_joint20")
MODEL_MODES = ((2, 8), (10, 8), (10, 2), (11, 8), (11, 2))         # (attention mode, num_bit); num_bit plays no part in mode 2
MODEL_N = (1, 7, 4099)
# which story of the set is THE memory: offset into the stories sorted by length, longest first (0 = the longest).  A (source,
# mode, num_bit) whose sampled pairs put an oracle probability on a truncation step takes the next story: recorded here
STORY_BUMP = {("random_joint20", 2, 8): 11, ("random_joint20", 10, 8): 19}


@functools.lru_cache(maxsize=None)
def model_inputs(which, mode, num_bit):
    """-> cfg, weights, story words of the whole set, question words, n_sen, answers (tests/golden; the words of test_gpu_shared.py)"""
    import json
    from conftest import GOLD, load_pkg
    from test_gpu_words import weights as word_weights, words16
    load_pkg()
    import qmann_amd.model as model
    if which == "trained_qa1":
        g = np.load(GOLD / "babi_qa1_test1000_words.npz")
        rec = json.loads((GOLD / "trained_qa1" / "reference_run.json").read_text())
        Vd, W = int(g["dim_input"]), 8
        cfg = model.babi_cfg(Vd, attention_mode=mode, softmax_base=0, iwl=int(rec["argv"][3]), en_mq=True)
        wts = model.load_weights(GOLD / "trained_qa1", cfg)
    else:
        g = np.load(GOLD / "babi_joint20_test20000_words.npz")
        Vd, W = int(g["dim_input"]), 16
        cfg = model.babi_cfg(Vd, attention_mode=mode, en_mq=False)
        wts = word_weights(12, 3, 60, Vd)
    cfg["num_bit"] = num_bit
    sw, qw = words16(g["story_words"], W), words16(g["question_words"], W)
    ans = g["answer"].astype(np.int64)
    ans = np.where(ans == 0xFF, 0xFFFF, ans)
    return cfg, wts, sw, qw, g["n_sen"].astype(np.int64), ans


def model_story_and_questions(which, mode, num_bit, N, second=False):
    """THE memory (one of the set's longest stories; `second`: another one, for the replacing memorize) and the questions of N
    other stories, taken round the set where it has fewer -> story words [R][W], question words [N][Wq], answers [N], and the
    indices (<= 48, spread) of the pairs that go against the oracle"""
    cfg, wts, sw, qw, n_sen, ans = model_inputs(which, mode, num_bit)
    offs = np.concatenate([[0], np.cumsum(n_sen)])
    order = np.argsort(-n_sen, kind="stable")
    s = int(order[STORY_BUMP.get((which, mode, num_bit), 0) + (5 if second else 0)])
    story = sw[offs[s]:offs[s + 1]]
    others = (s + 1 + np.arange(N)) % len(n_sen)
    pick = np.unique(np.linspace(0, N - 1, min(N, 48)).astype(np.int64))
    return story, qw[others], ans[others], pick

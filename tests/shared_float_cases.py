"""Inputs of test_gpu_shared_float.py (qmann_hops_shared_float_i8, csrc/batch_hops_shared_float.hip), shared with the CPU
preconditions in test_shared_float_inputs.py.

A case is ONE memory of S slots and B questions.  It is built as a float_hops_cases.Case whose planes are the memory repeated B
times (row_off = arange(B + 1) . S, max_slots = S): exactly the call on copies that the shared-plane call promises to equal bit
for bit, and the form float_hops_cases.chain / conditions / check_outputs take unchanged.  The flat tap layouts of the two calls
coincide: [h][q][s] of the shared call is [h][q . S + s] of the call on copies.  `memory(case)` gives the one memory back.

THE GENERATOR'S CONDITIONS ARE THOSE OF float_hops_cases.py, from the float64 reference alone: the score scale of every hop is
tuned on the reference chain -- through att_scale, or for the cases without the scale layer through the amplitude and density of
the key codes -- so that among the (query, hop) pairs with S >= 8 at least three quarters have 1 / sum p^2 >= 4 and every hop
index has one, and `near` holds at most 1 % of the columns.  A seed that fails one is replaced and listed in SEEDS.  These are
conditions on the inputs, not tolerances on the kernel.

Batch sizes: for every forced tile QT in {1, 2, 4, 8} the batches 1, QT, QT + 1 and 2 QT + 3, so that full tiles, a short last
tile of one query and a short last tile of three each occur; the tile-edge cases take 5 questions (a short last tile under every
QT but 1) and the switch cases 11.
"""
import zlib
from functools import lru_cache

import numpy as np

import float_hop_ref as ref
import float_hops_cases as fc
from float_hops_cases import GUARD, Q43, Q52, Case, pad_dim, tile_edge_slots, tile_rows

TILES = (1, 2, 4, 8)
BATCHES = sorted({b for qt in TILES for b in (1, qt, qt + 1, 2 * qt + 3)})       # 1 2 3 4 5 7 8 9 11 19
SEEDS = {"sf_all_127": 1271}       # name -> seed, where the default (a hash of the name) failed a condition (here: ties between +-127
                                 # rows put 7 % of the columns on a step)
CAP_SLOTS = 38368                # the longest memory one query's LDS holds: 9 344 + 4 . 38 368 = 160 KiB - 1 KiB exactly


def _seed(name):
    return SEEDS.get(name, zlib.crc32(name.encode()))


def memory(case):
    """the one memory of a case: (keys, values) uint8 [P][S][Dp]"""
    S = case.max_slots
    return case.kb[:, :S], case.vb[:, :S]


def _make(name, family, D, S, B, H=3, fmt=None, fmt_w=None, fmt_att=None, fmt_bin=Q52, tune="layer", cfg_extra=None, en_lin_map=True,
          tied=False, special=None, sigma_u=3.0, scale_signs=None, exempt_spread=False):
    rng = np.random.default_rng(_seed(name))
    fmt = [tuple(f) for f in (fmt or [Q52] * H)]
    fmt_w = [tuple(f) for f in (fmt_w or [Q43] * H)]
    cfg = dict(n_hop=H, dim_emb=D, dim_input=4, attention_mode=1, softmax_variant=0, f_fixed=True, en_lin_map=en_lin_map,
               fmt=fmt, fmt_w=fmt_w, fmt_att=[tuple(f) for f in (fmt_att or fmt)], fmt_bin=tuple(fmt_bin))
    cfg.update(cfg_extra or {})
    Dp, P = pad_dim(D), 1 if tied else H
    mw = [ref.max_code(f) for f in fmt_w]
    kc = np.zeros((P, S, Dp), np.int64); vc = np.zeros((P, S, Dp), np.int64)
    for p in range(P):
        kc[p, :, :D] = fc._codes(rng, (S, D), max(1.0, 0.3 * mw[p]), mw[p])
        vc[p, :, :D] = fc._codes(rng, (S, D), max(1.0, 0.35 * mw[p]), mw[p])
    lin = wts_h = None
    if en_lin_map:
        lin = [fc._codes(rng, (D, D), 0.1 * (1 << fmt_w[h][1]), mw[h]) for h in range(H)]
        wts_h = [(lin[h].astype(np.float64) / (1 << fmt_w[h][1])).astype(np.float32) for h in range(H)]
    u0c = fc._codes(rng, (B, D), sigma_u, mw[0])
    if S == 1 and all(fmt_w[h][1] == fmt[h][1] + 1 for h in range(H)):     # a one-slot memory reads out its value row: keep it off the grid
        v = vc[:, 0, :D]
        vc[:, 0, :D] = np.where(v % 2 == 0, v + np.where(v >= 0, 1, -1), v)
    u0 = (u0c.astype(np.float64) / (1 << fmt_w[0][1])).astype(np.float32)
    wts = dict(w_h=wts_h, w_ans=np.zeros((4, D), np.float32))
    mk, mv = ref.encode(kc), ref.encode(vc)
    one = Case(name, family, cfg, lin, wts, mk, mv, np.array([0, S], np.uint32), u0, S, tied, exempt_spread)
    if special:                                             # planted on the memory itself (a one-story view of it)
        special(rng, one)
    case = Case(name, family, cfg, lin, wts, None, None, (np.arange(B + 1) * S).astype(np.uint32), u0, S, tied, exempt_spread, one.marks)

    def retile():
        case.kb, case.vb = np.tile(mk, (1, B, 1)), np.tile(mv, (1, B, 1))
    retile()

    # the score scale, hop by hop on the reference chain
    states = [case.u0[q] for q in range(B)]
    if tune == "layer":
        cfg["att_scale"] = [1.0] * H
    for h in range(H):
        if tune == "keys" and not (tied and h > 0):
            for li, (sg, dens) in enumerate(fc.KEY_LEVELS):
                r2 = np.random.default_rng([_seed(name), h, li])
                kc[case.plane(h), :, :D] = fc._codes(r2, (S, D), sg, mw[h], dens)
                mk[case.plane(h)] = ref.encode(kc[case.plane(h)])
                retile()
                if fc._story_sigma(case, h, states) <= 1.1 * fc.TARGET_SIGMA:
                    break
            else:
                raise AssertionError(f"{name}: no key level brings hop {h} to the target score scale")
        elif tune == "layer":
            sg = fc._story_sigma(case, h, states)
            s = fc.TARGET_SIGMA / sg if sg > 0 else 1.0
            cfg["att_scale"][h] = float(np.float32(s * (scale_signs[h] if scale_signs else 1)))
        states = [case.hop(q, h, states[q]).u_next_f32() for q in range(B)]
    return case


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
CASES = {}
FAMILIES = {}


def _add(name, family, **kw):
    assert name not in fc.CASES
    CASES[name] = dict(family=family, **kw)
    FAMILIES.setdefault(family, []).append(name)


# tile edges of both scans at every padded width: the short path, one tile, a moved-back tile, each break / continue of the
# double-buffered loops; 5 questions: a short last tile under every tile size but 1
for _D in (60, 128, 200):
    for _S in tile_edge_slots(pad_dim(_D)):
        _add(f"sf_d{_D}_s{_S}", "tile_edges", D=_D, S=_S, B=5)
_T = tile_rows(64)
for _S in (1, _T - 1, _T + 1, 4 * _T + 1):
    _add(f"sf_d20_s{_S}", "tile_edges", D=20, S=_S, B=5)
# every batch size of the module text, one tile of rows and one more
for _B in BATCHES:
    _add(f"sf_batch_{_B:02d}", "batches", D=60, S=_T + 1, B=_B)
_add("sf_batch_19_d128", "batches", D=128, S=4 * tile_rows(128) + 1, B=19)
_add("sf_batch_19_d200", "batches", D=200, S=tile_rows(256) + 1, B=19)
# the switches
for _b, _n in ((1, "pow2"), (2, "plan")):
    _add(f"sf_{_n}", "switches", D=60, S=150, B=11, cfg_extra=dict(softmax_variant=_b))
    _add(f"sf_relu_{_n}", "switches", D=60, S=70, B=11, cfg_extra=dict(en_non_lin=True, softmax_variant=_b))
_add("sf_relu_exp", "switches", D=128, S=70, B=11, cfg_extra=dict(en_non_lin=True))
_add("sf_shift_pow2", "switches", D=60, S=150, B=11, cfg_extra=dict(softmax_variant=1, softmax_shift_based=True))
_add("sf_shift_exp", "switches", D=128, S=150, B=11, cfg_extra=dict(softmax_variant=0, softmax_shift_based=True))
_add("sf_scale_negative", "switches", D=60, S=150, B=11, scale_signs=[-1, 1, -1])
_add("sf_binary_u", "switches", D=60, S=150, B=11, fmt_bin=(0, 0))
_add("sf_no_lin_map", "switches", D=128, S=150, B=11, en_lin_map=False)
_add("sf_unscaled", "switches", D=60, S=150, B=11, tune="keys")
for _i in (0, 1, 2, 3, 5, 7):
    _a, _w, _t, _bn = fc.rand_formats(_i)
    _add(f"sf_formats_{_i:02d}", "switches", D=(60, 128, 200)[_i % 3], S=70, B=11, fmt=_a, fmt_w=_w, fmt_att=_t, fmt_bin=_bn)
_add("sf_tied", "tied", D=100, S=129, B=7, tied=True)
# special memories
_add("sf_mz_sprinkled", "special", D=60, S=257, B=5, special=fc._mz_sprinkle)
_add("sf_mz_words", "special", D=200, S=65, B=5, special=fc._mz_words)
_add("sf_all_127", "special", D=200, S=40, B=5, tune="none", special=fc._all_127, exempt_spread=True)
_add("sf_equal_scores", "special", D=100, S=97, B=5, special=fc._equal_scores)
_add("sf_two_maxima", "special", D=60, S=130, B=5, special=fc._two_maxima)


@lru_cache(maxsize=None)
def build(name):
    spec = dict(CASES[name])
    return _make(name, spec.pop("family"), **spec)


@lru_cache(maxsize=None)
def reference_chain(name):
    return fc.chain(build(name))


def untied(case):
    """the tied case with its one plane handed over once per hop"""
    return fc.untied(case)


def fits(S, qt):
    """does a tile of qt queries of an S-slot memory fit the LDS limit (the sizing formula of the header, restated)"""
    return qt * (9344 + (4 * S + 15) // 16 * 16) <= 160 * 1024 - 1024


# ---- stand-in outputs with the faults the comparison must report --------------------------------------------------------------------
def simulate(case, fault=None):
    """float_hops_cases.simulate for a shared-plane kernel: what a correct kernel hands back (float32 read-out of the reference),
    or with `fault` one of
      "neighbour"   query t carries query t - 1's read-out (a tile's accumulators mixed up), hop 0, every t >= 1;
      "last_row"    the last row's weight dropped from every read-out (a short tile's end lost);
      "spare"       a spare place of a short last tile stored: one state vector written behind u_out, into the guard."""
    cfg = case.cfg
    H, D = cfg["n_hop"], cfg["dim_emb"]
    raw = fc.blank_outputs(case)
    out = {k: fc.payload(case, raw, k) for k in raw}
    prev_o = None
    for q in range(case.B):
        r0, S, _ = case.slots(q)
        u = case.u0[q]
        for h in range(H):
            hp = case.hop(q, h, u)
            fw, fa = cfg["fmt_w"][h], cfg["fmt"][h]
            C = ref.decode(case.vb[case.plane(h), r0:r0 + S])[:, :D].astype(np.float64) / (1 << fw[1])
            p = hp.p.copy()
            if fault == "last_row":
                p[-1] = 0.0
            o = p @ C
            if h == 0:
                if fault == "neighbour" and prev_o is not None:
                    o, prev_o = prev_o, o
                else:
                    prev_o = o
            o32 = o.astype(np.float32)
            u = (ref.update_codes(hp.lu, o32, fa).astype(np.float64) / (1 << fa[1])).astype(np.float32)
            out["codes"][h, r0:r0 + S] = hp.codes; out["scores"][h, r0:r0 + S] = hp.scores; out["probs"][h, r0:r0 + S] = hp.p
            out["o"][q, h] = o32; out["u"][q, h] = u
        out["u_out"][q] = ref.relu_if(u, bool(cfg.get("en_non_lin")))
    if fault == "spare":
        n = case.B * D * 4
        raw["u_out"][GUARD + n:GUARD + n + 4 * D] = out["u_out"][case.B - 1].view(np.uint8)
    return raw

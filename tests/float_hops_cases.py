"""Inputs and the comparison routine of test_gpu_float_hops.py (ATTENTION_MODE 1, csrc/batch_hops_float.hip), shared with the
CPU preconditions in test_float_hops_inputs.py.

THE GENERATOR'S CONDITION IS SPREAD ATTENTION.  With the inputs of test_gpu_batch.py::run_float_case nearly every softmax weight
is zero, and the dense float read-out is tested as a copy of one value row.  Here the score scale of every hop is CHOSEN -- by
the scale layer (att_scale), tuned hop by hop on the reference chain, or for the cases without that layer by the amplitude and
density of the key codes -- so that in every case, among the (query, hop) pairs with S >= 8, at least three quarters have an
effective number of slots 1 / sum p^2 >= 4 and every hop index has one.  No query is discarded to get there.  Second condition:
`near` (float_hop_ref.py: the columns where a correct float32 read-out may land on the other side of a truncation step) holds
at most 1 % of a case's columns.  Both are asserted in test_float_hops_inputs.py from the reference alone.

A story of ONE slot reads out its value row itself, which lies on the weight grid; every case here has activations one bit
coarser than the weights where such a story exists, and gives that row odd codes, so that the read-out sits half a step away
from the grid instead of on it.

Rows before row_off[0] are allowed by the ABI (a query's rows are found through row_off alone): the tile-edge cases start at a
non-zero row_off[0] and fill the rows in front with bytes that must never be read.
"""
import zlib
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

import float_hop_ref as ref

GUARD = 4096                     # bytes on both sides of every output
FILL = 0xA5
ALL_TAPS = ("codes", "scores", "probs", "o", "u")
SPREAD_MIN_SLOTS, SPREAD_NEFF, SPREAD_SHARE = 8, 4.0, 0.75
NEAR_SHARE = 0.01
TARGET_SIGMA = 0.7               # of a story's scores after the tuning: S e^(-sigma^2) effective slots, 4.9 of 8
Q52, Q43 = (5, 2), (4, 3)


def pad_dim(D):
    return 64 if D <= 64 else 128 if D <= 128 else 256


def tile_rows(Dp):
    """rows of one tile of both scans: 4 loads per lane, 64 / (Dp / 16) rows per load"""
    return 4 * 64 // (Dp // 16)


def tile_edge_slots(Dp):
    T = tile_rows(Dp)
    return [1, T - 1, T, T + 1, 2 * T - 1, 4 * T, 4 * T + 1, 5 * T - 1, 8 * T, 8 * T + 1, 9 * T - 1, 12 * T + 1]


@dataclass
class Case:
    name: str
    family: str
    cfg: dict
    lin: list                    # per hop integer codes [D][D] of H on the grid w[h] (None without the linear map)
    wts: dict                    # the float arrays QNet takes (w_h on its grid, w_ans)
    kb: np.ndarray               # uint8 [P][R][Dp] sign-magnitude, P = n_hop, or 1 for tied planes
    vb: np.ndarray
    row_off: np.ndarray          # uint32 [B + 1]
    u0: np.ndarray               # float32 [B][D] on the grid w[0]
    max_slots: int
    tied: bool = False
    exempt_spread: bool = False  # the +-127 case: one-hot by construction
    marks: dict = field(default_factory=dict)       # what a special case planted, for the CPU assertions

    @property
    def B(self):
        return len(self.row_off) - 1

    @property
    def R(self):
        return self.kb.shape[1]

    def slots(self, q):
        """(first row, slots the kernel reads, slots handed over)"""
        r0 = int(self.row_off[q]); s_in = int(self.row_off[q + 1]) - r0
        return r0, min(s_in, self.max_slots), s_in

    def plane(self, h):
        return 0 if self.tied else h

    def hop(self, q, h, u, **kw):
        r0, S, _ = self.slots(q)
        p = self.plane(h)
        return ref.hop(u, self.kb[p, r0:r0 + S], self.vb[p, r0:r0 + S], h, self.cfg, self.lin[h] if self.lin else None, **kw)


def chain(case):
    """the reference through its own u_next: [query][hop] -> float_hop_ref.Hop"""
    out = []
    for q in range(case.B):
        u, hops = case.u0[q], []
        for h in range(case.cfg["n_hop"]):
            hops.append(case.hop(q, h, u))
            u = hops[-1].u_next_f32()
        out.append(hops)
    return out


def conditions(case, ch=None):
    """(share of the (query, hop) pairs with S >= 8 whose 1 / sum p^2 >= 4, the same per hop index, share of near columns)"""
    ch = ch or chain(case)
    H = case.cfg["n_hop"]
    ok = [[] for _ in range(H)]
    near = cols = 0
    for q in range(case.B):
        S = case.slots(q)[1]
        for h in range(H):
            if S >= SPREAD_MIN_SLOTS:
                ok[h].append(ref.n_eff(ch[q][h].p) >= SPREAD_NEFF)
            if S > 0:
                near += int(ch[q][h].near.sum()); cols += ch[q][h].near.size
    flat = [x for per in ok for x in per]
    return (float(np.mean(flat)) if flat else 1.0), [bool(any(per)) for per in ok], near / max(cols, 1)


# ---- generator -----------------------------------------------------------------------------------------------------------------
# amplitude (sigma in codes) and density of the key codes for the cases WITHOUT the scale layer, strongest first
KEY_LEVELS = [(3.0, 1.0), (2.0, 1.0), (1.5, 1.0), (1.0, 1.0), (1.0, 0.5), (1.0, 0.25), (1.0, 0.12), (1.0, 0.06), (1.0, 0.03), (1.0, 0.015), (1.0, 0.008), (1.0, 0.004)]
SEEDS = {}                       # name -> seed, where the default (a hash of the name) failed a condition


def _seed(name):
    return SEEDS.get(name, zlib.crc32(name.encode()))


def _codes(rng, shape, sigma, m, density=1.0):
    c = np.clip(np.rint(rng.normal(0, sigma, shape)), -m, m).astype(np.int64)
    if density < 1.0:
        c = c * (rng.random(shape) < density)
    return c


def _story_sigma(case, h, states):
    """per-story standard deviation of the raw scores of hop h, pooled over the stories with S >= 8"""
    var = []
    for q in range(case.B):
        r0, S, _ = case.slots(q)
        if S < SPREAD_MIN_SLOTS:
            continue
        cfg1 = dict(case.cfg, att_scale=None, softmax_variant=0, softmax_shift_based=False)
        hp = ref.hop(states[q], case.kb[case.plane(h), r0:r0 + S], case.vb[case.plane(h), r0:r0 + S], h, cfg1, case.lin[h] if case.lin else None)
        var.append(float(np.var(hp.scores.astype(np.float64))))
    return float(np.sqrt(np.mean(var))) if var else 0.0


def _make(name, family, D, S_in, H=3, fmt=None, fmt_w=None, fmt_att=None, fmt_bin=Q52, tune="layer", cfg_extra=None, en_lin_map=True,
          max_slots=None, lead_rows=0, tied=False, special=None, sigma_u=3.0, scale_signs=None, exempt_spread=False):
    rng = np.random.default_rng(_seed(name))
    fmt = [tuple(f) for f in (fmt or [Q52] * H)]
    fmt_w = [tuple(f) for f in (fmt_w or [Q43] * H)]
    cfg = dict(n_hop=H, dim_emb=D, dim_input=4, attention_mode=1, softmax_variant=0, f_fixed=True, en_lin_map=en_lin_map,
               fmt=fmt, fmt_w=fmt_w, fmt_att=[tuple(f) for f in (fmt_att or fmt)], fmt_bin=tuple(fmt_bin))
    cfg.update(cfg_extra or {})
    Dp, B, P = pad_dim(D), len(S_in), 1 if tied else H
    row_off = (lead_rows + np.concatenate([[0], np.cumsum(S_in)])).astype(np.uint32)
    R = max(int(row_off[-1]), 1)
    mw = [ref.max_code(f) for f in fmt_w]
    kc = np.zeros((P, R, Dp), np.int64); vc = np.zeros((P, R, Dp), np.int64)
    for p in range(P):
        kc[p, :, :D] = _codes(rng, (R, D), max(1.0, 0.3 * mw[p]), mw[p])
        vc[p, :, :D] = _codes(rng, (R, D), max(1.0, 0.35 * mw[p]), mw[p])
    lin = wts_h = None
    if en_lin_map:
        lin = [_codes(rng, (D, D), 0.1 * (1 << fmt_w[h][1]), mw[h]) for h in range(H)]
        wts_h = [(lin[h].astype(np.float64) / (1 << fmt_w[h][1])).astype(np.float32) for h in range(H)]
    u0c = _codes(rng, (B, D), sigma_u, mw[0])
    if D < 4:
        u0c[u0c == 0] = 1
    for q in range(B):                                      # a one-slot story reads out its value row: keep it off the grid
        if S_in[q] == 1 and all(fmt_w[h][1] == fmt[h][1] + 1 for h in range(H)):
            r = int(row_off[q])
            v = vc[:, r, :D]
            vc[:, r, :D] = np.where(v % 2 == 0, v + np.where(v >= 0, 1, -1), v)
    case = Case(name, family, cfg, lin, dict(w_h=wts_h, w_ans=np.zeros((4, D), np.float32)), None, None, row_off,
                (u0c.astype(np.float64) / (1 << fmt_w[0][1])).astype(np.float32),
                int(max_slots if max_slots is not None else max(max(S_in), 1)), tied, exempt_spread)
    kb, vb = ref.encode(kc), ref.encode(vc)
    if lead_rows:                                           # rows no query owns
        kb[:, :lead_rows] = rng.integers(1, 256, (P, lead_rows, Dp)); vb[:, :lead_rows] = rng.integers(1, 256, (P, lead_rows, Dp))
    case.kb, case.vb = kb, vb
    if special:
        special(rng, case)

    # the score scale, hop by hop on the reference chain
    states = [case.u0[q] for q in range(B)]
    if tune == "layer":
        cfg["att_scale"] = [1.0] * H
    for h in range(H):
        if tune == "keys" and not (tied and h > 0):
            for li, (sg, dens) in enumerate(KEY_LEVELS):
                r2 = np.random.default_rng([_seed(name), h, li])
                kc[case.plane(h), :, :D] = _codes(r2, (R, D), sg, mw[h], dens)
                case.kb[case.plane(h), lead_rows:] = ref.encode(kc[case.plane(h), lead_rows:])
                if _story_sigma(case, h, states) <= 1.1 * TARGET_SIGMA:
                    break
            else:
                raise AssertionError(f"{name}: no key level brings hop {h} to the target score scale")
        elif tune == "layer":
            sg = _story_sigma(case, h, states)
            s = TARGET_SIGMA / sg if sg > 0 else 1.0
            cfg["att_scale"][h] = float(np.float32(s * (scale_signs[h] if scale_signs else 1)))
        states = [case.hop(q, h, states[q]).u_next_f32() for q in range(B)]
    return case


# ---- special plantings -------------------------------------------------------------------------------------------------------------
def _mz_sprinkle(rng, case, share=0.125):
    D = case.cfg["dim_emb"]
    for plane in (case.kb, case.vb):
        hit = rng.random(plane[:, :, :D].shape) < share
        plane[:, :, :D][hit] = 0x80
    case.marks["sprinkled"] = True


def _mz_whole_rows(rng, case):
    """in every story of 8 rows or more, one whole row of 0x80 in the keys (its score is 0) and another in the values"""
    D = case.cfg["dim_emb"]
    _mz_sprinkle(rng, case, 0.05)
    rows_k, rows_v = [], []
    for q in range(case.B):
        r0, S, _ = case.slots(q)
        if S >= 8:
            a, b = rng.choice(S, 2, replace=False)
            case.kb[:, r0 + a, :D] = 0x80; case.vb[:, r0 + b, :D] = 0x80
            rows_k.append(r0 + int(a)); rows_v.append(r0 + int(b))
    case.marks["whole_rows"] = (rows_k, rows_v)


def _mz_words(rng, case):
    """whole words of 0x80 between words of 0x7F and 0xFF (+127 / -127), and words that mix the three, in both planes: a carry
    out of one byte of the word-wide sign-magnitude conversion would land in its neighbour"""
    D = case.cfg["dim_emb"]
    words = np.array([[0x7F] * 4, [0x80] * 4, [0xFF] * 4, [0x80] * 4, [0x7F, 0x80, 0xFF, 0x80], [0x80, 0xFF, 0x80, 0x7F],
                      [0xFF, 0x80, 0x80, 0x7F], [0x80, 0x7F, 0xFF, 0xFF]], np.uint8)
    nw = D // 4
    for plane in (case.kb, case.vb):
        P, R, _ = plane.shape
        hit = rng.random((P, R)) < 0.5                       # half of the rows carry the pattern over their whole width
        start = rng.integers(0, len(words), (P, R))
        for p, r in zip(*np.nonzero(hit)):
            plane[p, r, :nw * 4] = words[(start[p, r] + np.arange(nw)) % len(words)].reshape(-1)
    case.marks["words"] = True


def _all_127(rng, case):
    D = case.cfg["dim_emb"]
    for plane in (case.kb, case.vb):
        plane[:, :, :D] = np.where(rng.random(plane[:, :, :D].shape) < 0.5, 0x7F, 0xFF)
    case.u0[:] = np.where(rng.random(case.u0.shape) < 0.5, 127, -127) / np.float32(1 << case.cfg["fmt_w"][0][1])


def _equal_scores(rng, case):
    """every key row of a story is the same row: all scores equal, p = 1 / S on every hop"""
    for q in range(case.B):
        r0, S, _ = case.slots(q)
        case.kb[:, r0:r0 + S] = case.kb[:, r0:r0 + 1]


def _two_maxima(rng, case):
    """two rows of every story share one key row, aligned with u0 so that their score is hop 0's maximum: a tie at the top"""
    D = case.cfg["dim_emb"]
    pairs = []
    for q in range(case.B):
        r0, S, _ = case.slots(q)
        a, b = sorted(int(x) for x in rng.choice(S, 2, replace=False))
        key = ref.encode(30 * np.sign(ref.on_grid_codes(case.u0[q], case.cfg["fmt_w"][0])))
        case.kb[:, r0 + a, :D] = key; case.kb[:, r0 + b, :D] = key
        pairs.append((a, b))
    case.marks["pairs"] = pairs


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
CASES = {}
FAMILIES = {}


def _add(name, family, **kw):
    CASES[name] = dict(family=family, **kw)
    FAMILIES.setdefault(family, []).append(name)


FORMAT_SEEDS = {4: 7804, 6: 7926}                # draw -> seed, where the default (7700 + draw) failed a condition


def rand_formats(draw, H=3):
    """(act, w, att) per hop and bin: word lengths 1 .. 7, frac 0 .. word length"""
    rng = np.random.default_rng(FORMAT_SEEDS.get(draw, 7700 + draw))

    def one():
        wl = int(rng.integers(1, 8)); fr = int(rng.integers(0, wl + 1))
        return (wl - fr, fr)
    return [one() for _ in range(H)], [one() for _ in range(H)], [one() for _ in range(H)], one()


# tile edges: the short path, the one-tile path, a moved-back tile, each break / continue of the double-buffered loops; an empty
# story between two others; rows in front of row_off[0]
for _D in (60, 100, 256):
    _s = tile_edge_slots(pad_dim(_D))
    _add(f"tiles_d{_D}", "tile_edges", D=_D, S_in=_s[:6] + [0] + _s[6:], lead_rows=5)
for _D in (1, 17, 60, 64, 100, 128, 200, 255, 256):
    _T = tile_rows(pad_dim(_D))
    _add(f"width_d{_D}", "widths", D=_D, S_in=[8, 23, 50, _T + 3, 4 * _T + 5, 2 * _T, 9, 5 * _T + 1])
_add("mz_sprinkled", "minus_zero", D=60, S_in=[8, 20, 63, 64, 65, 130, 257, 300], special=_mz_sprinkle)
_add("mz_whole_rows", "minus_zero", D=100, S_in=[8, 31, 32, 33, 70, 129, 161], special=_mz_whole_rows)
_add("mz_words", "minus_zero", D=256, S_in=[8, 15, 16, 17, 40, 65, 100], special=_mz_words)
# all operands +-127: scores of +-127 . 127 . D codes (< 2^24), one-hot by construction -- EXEMPT from the spread condition
_add("extreme_127", "extremes", D=256, S_in=[8, 40, 129, 16, 65], tune="none", special=_all_127, exempt_spread=True)
_add("equal_scores", "extremes", D=100, S_in=[97, 193, 389, 31], special=_equal_scores)        # (prime S: sum / S rarely on a step)
_add("two_maxima", "extremes", D=60, S_in=[50, 64, 65, 130, 20, 257], special=_two_maxima)
for _i in range(12):
    _a, _w, _t, _b = rand_formats(_i)
    _add(f"formats_{_i:02d}", "formats", D=(60, 128, 200)[_i % 3], S_in=[8, 19, 40, 70, 150, 33], fmt=_a, fmt_w=_w, fmt_att=_t, fmt_bin=_b)
_add("binary_mode", "formats", D=60, S_in=[8, 19, 40, 70, 150, 64], fmt_bin=(0, 0))
_add("no_lin_map", "formats", D=128, S_in=[8, 19, 40, 70, 150, 32], en_lin_map=False)
for _b, _n in ((0, "exp"), (1, "pow2"), (2, "plan")):
    _add(f"non_lin_{_n}", "formats", D=60, S_in=[8, 19, 40, 70, 150, 64], cfg_extra=dict(en_non_lin=True, softmax_variant=_b))
_add("shift_pow2", "formats", D=60, S_in=[8, 19, 40, 70, 150], cfg_extra=dict(softmax_variant=1, softmax_shift_based=True))
_add("shift_exp", "formats", D=128, S_in=[8, 19, 40, 70, 150], cfg_extra=dict(softmax_variant=0, softmax_shift_based=True))
_add("scale_negative", "formats", D=60, S_in=[8, 19, 40, 70, 150], scale_signs=[-1, 1, -1])
# the stock path with no scale layer at all: the score scale comes from the key codes
_add("unscaled_d60", "formats", D=60, S_in=[8, 19, 50, 64, 65, 150], tune="keys")
_add("unscaled_d256", "formats", D=256, S_in=[8, 16, 17, 50, 100], tune="keys")
# a story that max_slots cuts, max_slots below and above the tile (T = 64 rows at Dp = 64)
_add("cut_below_tile", "cut", D=60, S_in=[30, 50, 51, 80, 200, 8], max_slots=50)
_add("cut_above_tile", "cut", D=60, S_in=[64, 100, 101, 300, 65, 8], max_slots=100)
_add("tied_planes", "tied", D=100, S_in=[8, 31, 32, 33, 70, 129, 161], tied=True)
_add("taps", "taps", D=100, S_in=[8, 31, 32, 33, 70, 129])

TAP_COMBOS = [ALL_TAPS, ()] + [(t,) for t in ALL_TAPS]


@lru_cache(maxsize=None)
def build(name):
    spec = dict(CASES[name])
    return _make(name, spec.pop("family"), **spec)


@lru_cache(maxsize=None)
def reference_chain(name):
    return chain(build(name))


def untied(case):
    """the tied case with its one plane handed over once per hop: what the tied launch must equal bit for bit"""
    H = case.cfg["n_hop"]
    return Case(case.name + "_untied", case.family, case.cfg, case.lin, case.wts, np.repeat(case.kb, H, 0), np.repeat(case.vb, H, 0),
                case.row_off, case.u0, case.max_slots, False, case.exempt_spread, case.marks)


# ---- outputs inside guards, and the comparison -------------------------------------------------------------------------------
def out_shapes(case):
    H, D, B, R = case.cfg["n_hop"], case.cfg["dim_emb"], case.B, case.R
    return {"u_out": ((B, D), np.float32), "codes": ((H, R), np.int32), "scores": ((H, R), np.float32), "probs": ((H, R), np.float32),
            "o": ((B, H, D), np.float32), "u": ((B, H, D), np.float32)}


def payload(case, raw, name):
    shape, dt = out_shapes(case)[name]
    n = int(np.prod(shape)) * 4
    assert raw[name].size == n + 2 * GUARD
    return raw[name][GUARD:GUARD + n].view(dt).reshape(shape)


def blank_outputs(case, taps=ALL_TAPS):
    return {k: np.full(int(np.prod(out_shapes(case)[k][0])) * 4 + 2 * GUARD, FILL, np.uint8) for k in ("u_out",) + tuple(taps)}


def check_outputs(case, raw, taps=ALL_TAPS, label=""):
    """`raw`: name -> the WHOLE guard-filled byte buffer (numpy uint8) of u_out and of every tap in `taps`, as the call left it.
    Asserts everything test_gpu_float_hops.py promises; with every tap on, each hop's reference input is the tapped state of the
    hop before (u0 for hop 0), so a permitted difference on a `near` column cannot cascade.  Returns counts for the log."""
    cfg = case.cfg
    H, D, B, R = cfg["n_hop"], cfg["dim_emb"], case.B, case.R
    what = f"{case.name}{label}"
    fill4 = np.full(4, FILL, np.uint8)
    for k, buf in raw.items():
        n = buf.size - 2 * GUARD
        assert (buf[:GUARD] == FILL).all() and (buf[GUARD + n:] == FILL).all(), f"{what}: the guard of {k} was written"
    got = {k: payload(case, raw, k) for k in raw}
    assert set(got) == {"u_out", *taps}

    # rows no query reads -- in front of row_off[0], past a cut, behind the last story -- keep their fill in every per-row tap
    owned = np.zeros(R, bool)
    for q in range(B):
        r0, S, _ = case.slots(q)
        owned[r0:r0 + S] = True
    for k in ("codes", "scores", "probs"):
        if k in got:
            b = got[k].view(np.uint8).reshape(H, R, 4)
            assert (b[:, ~owned] == fill4).all(), f"{what}: {k} written on a row no query reads"
            assert not (b[:, owned] == fill4).all(axis=-1).any(), f"{what}: {k} left unwritten on a row that is read"

    stats = dict(cols=0, near=0, differ=0)
    if set(ALL_TAPS) <= set(got):
        known = reference_chain(case.name) if case.name in CASES else None
        for q in range(B):
            r0, S, _ = case.slots(q)
            u_in = case.u0[q]
            for h in range(H):
                fa = cfg["fmt"][h]
                ref.on_grid_codes(u_in, ref.src_fmt(cfg, h))                 # (asserts: on its grid, inside its format)
                hp = known[q][h] if known is not None and np.array_equal(u_in, case.u0[q] if h == 0 else known[q][h - 1].u_next_f32()) \
                    else case.hop(q, h, u_in)
                at = f"{what} q{q} h{h} (S={S})"
                np.testing.assert_array_equal(got["codes"][h, r0:r0 + S], hp.codes, err_msg=f"score codes {at}")
                np.testing.assert_array_equal(got["scores"][h, r0:r0 + S], hp.scores, err_msg=f"scores {at}")
                np.testing.assert_allclose(got["probs"][h, r0:r0 + S], hp.p, rtol=1e-5, atol=1e-7, err_msg=f"p {at}")
                err = np.abs(got["o"][q, h].astype(np.float64) - hp.o64)
                assert (err <= hp.bound).all(), f"o {at}: column {int(np.argmax(err - hp.bound))} off by {err.max():.3e}, bound {hp.bound[int(np.argmax(err - hp.bound))]:.3e}"
                gk = ref.on_grid_codes(got["u"][q, h], fa)
                a, b = hp.allowed()
                bad = (gk != a) & (gk != b)
                assert not bad.any(), (f"u {at}: columns {np.nonzero(bad)[0][:8].tolist()} got {gk[bad][:8].tolist()}, want {hp.u_next[bad][:8].tolist()}"
                                       f" (near: {hp.near[bad][:8].tolist()})")
                if S > 0:
                    stats["cols"] += D; stats["near"] += int(hp.near.sum()); stats["differ"] += int((gk != hp.u_next).sum())
                u_in = got["u"][q, h]
            np.testing.assert_array_equal(got["u_out"][q], ref.relu_if(got["u"][q, H - 1], bool(cfg.get("en_non_lin"))), err_msg=f"u_out {what} q{q}")
        # `near` as recomputed from the inputs the kernel actually had: a test that excuses everything cannot pass
        assert stats["near"] <= NEAR_SHARE * stats["cols"], f"{what}: {stats['near']} of {stats['cols']} columns are near a step"
    return stats


def simulate(case, taps=ALL_TAPS, fault=None):
    """What a correct kernel hands back, built from the reference with a float32 read-out -- or, with `fault`, what a kernel with
    one of the errors the comparison must catch hands back:
      "row_twice"  one value row of one story added twice (a moved-back tile counted again);
      "minus128"   a 0x80 value byte read as -128;
      "u_code"     one state code off by one on a column outside `near`;
      "guard"      one byte written in front of u_out."""
    cfg = case.cfg
    H, D = cfg["n_hop"], cfg["dim_emb"]
    raw = blank_outputs(case, taps)
    out = {k: payload(case, raw, k) for k in raw}
    dec = (lambda b: np.where(np.asarray(b) == 0x80, -128, ref.decode(b))) if fault == "minus128" else ref.decode
    pending = fault in ("row_twice", "u_code")
    for q in range(case.B):
        r0, S, _ = case.slots(q)
        u = case.u0[q]
        for h in range(H):
            hp = case.hop(q, h, u)
            fw, fa = cfg["fmt_w"][h], cfg["fmt"][h]
            C = dec(case.vb[case.plane(h), r0:r0 + S])[:, :D].astype(np.float64) / (1 << fw[1])
            o = hp.p @ C if S else np.zeros(D)
            if pending and fault == "row_twice" and S >= 8:
                r = int(np.argsort(hp.p)[S // 2])                            # a row of median weight
                o = o + hp.p[r] * C[r]
                pending = False
            o32 = o.astype(np.float32)
            uk = ref.update_codes(hp.lu, o32, fa)
            if pending and fault == "u_code" and S >= 8 and not hp.near.all():
                c = int(np.nonzero(~hp.near)[0][0])
                uk[c] += 1 if uk[c] < ref.max_code(fa) else -1
                pending = False
            u = (uk.astype(np.float64) / (1 << fa[1])).astype(np.float32)
            for k, v in (("codes", hp.codes), ("scores", hp.scores), ("probs", hp.p)):
                if k in out:
                    out[k][h, r0:r0 + S] = v
            if "o" in out:
                out["o"][q, h] = o32
            if "u" in out:
                out["u"][q, h] = u
        out["u_out"][q] = ref.relu_if(u, bool(cfg.get("en_non_lin")))
    assert not pending, "the fault found no place"
    if fault == "guard":
        raw["u_out"][GUARD - 1] ^= 0xFF
    return raw

"""Planted memories for the per-story hop kernels (k_hops_small, k_hops_lean, k_hops_quad and the split pair, k_hops_mid,
k_hops_fixed, k_hops_ham), the conditions they meet and the one comparison routine of test_live_hops_inputs.py (CPU) and
test_gpu_live_hops.py.

WHY.  These kernels read a value row only where its weight code Q(p) = floor(p . 2^frac) is not zero.  On the random memories of
test_gpu_mid.py, test_gpu_lean.py, test_gpu_quad.py and test_gpu_batch.py no row of a story of more than about 16 rows has one:
the scores saturate and tie (p = 1 / n_ties < 2^-frac), or the softmax is too flat.  Survivor selection, the value fetch and the
weighted sum then run with o = 0 (test_live_hops_inputs.py::test_the_old_mid_inputs_have_no_live_row records it).

HOW.  Memories are built hop by hop on the CPU oracle.  Cold rows have sparse keys near zero (Hamming modes: dense random codes),
so their scores stay far under the top.  A few HOT rows per (query, hop) get keys aligned with that hop's own input u_h, which
the generator takes from the oracle run on the memory planted so far: sign(u_h) . amplitude for fixed-point attention -- whole
for a score that saturates at the top code, thinned column by column for a score `delta` under the top --, u_h's own code
pattern for the Hamming modes.  Three tied rows give p = 1/3, which no power of two divides: clear of every step of Q(p).

CONDITIONS, asserted per case in test_live_hops_inputs.py from the oracle alone:
  C1  every (query, hop) with S >= 2 and frac >= 1 has at least `min_live` live rows.  min_live >= 2 everywhere but at ONE
      fraction bit: there Q(p) != 0 asks p >= 1/2, two live rows ask p = 1/2 twice, and 1/2 is a step (C2): the frac-1 case
      states min_live = 1 and says so;
  C2  no oracle p within 1e-3 (relative, in steps) of a truncation step of Q(p): a hundred times the 1e-5 the GPU softmax is
      granted, so every weight code is decided and the GPU tests excuse NOTHING;
  C3  the term Q(Q(p_r) . v_r) of every live row is non-zero in at least a quarter of the columns;
  C4  for every query and hop, the oracle with that hop's value plane zeroed gives another u_out;
  C5  every fixed-point case whose activation formats have frac >= 4 (Case.c5, derived from the formats) has a pair with three
      different non-zero weight codes, so weights swapped among rows would be seen.  With fewer fraction bits this cannot be had
      (at Q5.2 every live row has code 1 .. 3 and three of them share p >= 3/4), and the Hamming families are held to C1 .. C4
      only: their hot rows carry u_h's own pattern and tie;
  C6  the live rows of a case, taken together, cover the positions named in `positions` (a kernel's group, lane and chunk
      edges, both ends of a story, the neighbour's first row behind a hot last row, the row behind the cut).
"""
import zlib
from dataclasses import dataclass, field

import numpy as np

GUARD = 4096
FILL = 0xA5
ALL_TAPS = ("codes", "scores", "probs", "o", "u")
CLEAR_REL = 1e-3
Q52, Q25, Q07 = (5, 2), (2, 5), (0, 7)


def pad_dim(D):
    return 64 if D <= 64 else 128 if D <= 128 else 256


def to_signmag(codes):
    """int8 codes, |code| <= 127 -> sign-magnitude bytes"""
    out = np.abs(codes).view(np.uint8)
    out |= (codes.view(np.uint8) & 0x80)
    return out


def near_step(p, frac, rel):
    """test_gpu_batch.near_step"""
    x = p.astype(np.float64) * (1 << frac)
    k = np.rint(x)
    return (np.abs(x - k) <= rel * np.maximum(1.0, np.abs(x))) & (k > 0)


def weight_codes(p, frac):
    return np.floor(p.astype(np.float64) * (1 << frac)).astype(np.int64)


@dataclass
class Case:
    name: str
    family: str
    cfg: dict
    wts: dict
    keys: np.ndarray             # int8 CODES [H][R][Dp] on the attention grid of their hop
    vals: np.ndarray             # int8 codes [H][R][Dp] on the activation grid of their hop
    row_off: np.ndarray          # int64 [B + 1]
    u0: np.ndarray               # float32 [B][D] on the grid w[0]
    max_slots: int
    env: dict                    # QMANN_* switches the launch runs under
    packed: bool                 # qmann_hops_packed on bit planes instead of qmann_hops_i8
    min_live: int
    positions: tuple             # names of position_flags() that must all be set
    hot: dict = field(default_factory=dict)         # (query, hop) -> hot rows, counted from the story's first row
    origin: np.ndarray = None    # persistent cases: query -> the planted story it copies
    taps_too: bool = True        # also launched with taps (the general kernels)

    @property
    def B(self):
        return len(self.row_off) - 1

    @property
    def R(self):
        return self.keys.shape[1]

    @property
    def H(self):
        return self.cfg["n_hop"]

    @property
    def c5(self):
        """condition C5 applies: fixed-point attention and four or more fraction bits in every hop's activation format"""
        return self.cfg["attention_mode"] == 2 and min(f[1] for f in self.cfg["fmt"]) >= 4

    def slots(self, q):
        r0 = int(self.row_off[q]); s_in = int(self.row_off[q + 1]) - r0
        return r0, min(s_in, self.max_slots), s_in

    def floats(self, q, n=None, keys=None, vals=None):
        """(keys, vals) of query q as the oracle takes them, cut to n rows (default: what the kernels read)"""
        r0, S, _ = self.slots(q)
        n = S if n is None else n
        D, cfg = self.cfg["dim_emb"], self.cfg
        keys = self.keys if keys is None else keys
        vals = self.vals if vals is None else vals
        kf = np.stack([keys[h, r0:r0 + n, :D].astype(np.float32) / np.float32(1 << cfg["fmt_att"][h][1]) for h in range(self.H)])
        vf = np.stack([vals[h, r0:r0 + n, :D].astype(np.float32) / np.float32(1 << cfg["fmt"][h][1]) for h in range(self.H)])
        return kf, vf

    def unit(self):
        """the score that one score code stands for, per hop"""
        m, nb = self.cfg["attention_mode"], self.cfg.get("num_bit", 8)
        if m == 2:
            return [1.0 / (1 << f[1]) for f in self.cfg["fmt_att"]]
        return [{3: 1.0 / 1024.0, 10: 1.0, 11: 1.0 / (1 << nb)}[m]] * self.H


def form_of(case, taps):
    """The kernel form hops_host.h::hop_plan gives the launch, restated from the shape and the switches (the library exports no
    call that tells; qm_hops_will_split answers for the split alone and is no ABI symbol)."""
    cfg, env, ms = case.cfg, case.env, case.max_slots
    mode, Dp = cfg["attention_mode"], pad_dim(cfg["dim_emb"])
    fixed = mode == 2
    long_form = "k_hops_fixed" if fixed else "k_hops_ham"
    plain_softmax = cfg.get("softmax_variant", 0) == 0 and not cfg.get("softmax_shift_based")
    if taps or case.packed or Dp != 64 or ms > 64 or "QMANN_NO_LEAN" in env:
        if ms <= 64:
            return "k_hops_small"
        if fixed and not taps and Dp == 64 and ms <= 1024 and cfg.get("att_scale") is None and not cfg.get("softmax_shift_based") \
                and "QMANN_NO_MID" not in env:
            return "k_hops_mid"
        if fixed and not taps and ms > 256 and plain_softmax and "QMANN_NO_SCAN_STOP" not in env and scan_stop_opens(cfg, ms):    # (four-wavefront launches only)
            return "k_hops_fixed (stopping build)"
        return long_form + (" (256 lanes)" if fixed and ms > 256 else " (64 lanes)" if fixed else "")
    w7 = all(sum(f) == 7 for k in (("fmt_att",) if fixed else ()) + ("fmt_w", "fmt") for f in cfg[k]) and cfg["fmt_bin"][1] <= 7
    quad_ok = "QMANN_NO_QUAD" not in env and plain_softmax and w7 and case.R * 64 < 0x7FFF0000
    if not quad_ok or case.B <= int(env.get("QMANN_QUAD_MIN_QUERIES", 8192)):
        sparse = env.get("QMANN_LEAN_SPARSE")
        return "k_hops_lean" + ("" if sparse is None else " (sparse read-out)" if sparse == "1" else " (value tile)")
    if ms <= 16:
        return "k_hops_quad"
    if case.R // case.B > 16:
        return "k_hops_quad (four chunks)" if fixed and "QMANN_NO_QUAD_LONG" not in env else "k_hops_lean"
    return "split: k_hops_quad + k_hops_lean"


def scan_stop_opens(cfg, max_slots):
    """hops_host.h::scan_stop_gate for a call without taps and without the scale layer"""
    for h in range(cfg["n_hop"]):
        (ia, fa), frac = cfg["fmt_att"][h], cfg["fmt"][h][1]
        top = ((1 << (ia + fa)) - 1) / float(1 << fa)
        if (1 << frac) * np.exp(top) * (1.0 + 0.015625) <= max_slots:
            return True
    return False


# ---- the generator -------------------------------------------------------------------------------------------------------------
def _pick(cands, n, k):
    cands = list(dict.fromkeys(cands))
    assert len(cands) >= n, (cands, n)
    out, i = [], k
    while len(out) < n:
        if cands[i % len(cands)] not in out:
            out.append(cands[i % len(cands)])
        i += 1
    return out


def edge_rows(S, unit):
    """both ends of a story, both sides of every multiple of `unit`, and the first row of the last partial group"""
    g = unit * ((S - 1) // unit)
    c = [S - 1, 0, unit - 1, unit, g, S - 2, 2 * unit - 1, 2 * unit, g - 1, 3 * unit - 1, 3 * unit, S // 2, 4 * unit - 1, 4 * unit]
    return [r for r in c if 0 <= r < S]


def _model(oracle, case_cfg, wts, n_hop):
    cfg = dict(case_cfg, n_hop=n_hop)
    return oracle.make_model(cfg, wts)


def _att_input(cfg, u, h):
    return np.maximum(u, 0).astype(np.float32) if cfg.get("en_non_lin") and h > 0 else u


def _hot_key_fixed(oracle, cfg, h, u_att, amp, delta, cols=None):
    """delta = 0: sign(u_h) . amp in every column where u_h is not zero, a score that saturates at the top code.  delta > 0:
    columns are added, strong ones first and then single codes, as long as the oracle's score stays at or under top - delta.
    cols: the columns the key may use (default: all)"""
    (ia, fa), fb = cfg["fmt_att"][h], cfg["fmt_bin"]
    top = ((1 << (ia + fa)) - 1) / float(1 << fa)
    sgn = np.sign(u_att).astype(np.int64)
    if cols is not None:
        sgn = sgn * np.isin(np.arange(len(sgn)), cols)
    if delta <= 0:
        return sgn * amp
    score = lambda k: float(oracle.dot_mat_vec_fwd((k / float(1 << fa)).astype(np.float32)[None], u_att, False, True, (ia, fa), fb)[0])
    key = np.zeros_like(sgn)
    for a in sorted({amp, max(amp // 3, 1), 6, 2, 1}, reverse=True):
        for c in np.nonzero(sgn)[0]:
            if key[c] == 0:
                key[c] = sgn[c] * a
                if score(key) > top - delta:
                    key[c] = 0
    return key


def _hot_key_ham(cfg, h, u_att, delta):
    """u_h's own codes on the attention grid; delta > 0: the sign of round(delta) columns turned"""
    fa = cfg["fmt_att"][h][1]
    key = np.clip(np.rint(u_att.astype(np.float64) * (1 << fa)), -127, 127).astype(np.int64)
    turn = np.nonzero(key)[0][:int(round(delta * (4 if cfg["attention_mode"] == 3 else 1)))]
    key[turn] = -key[turn]
    return key


def cold_memory(rng, P, R, D, mode, fmt_att, fmt, sigma_cold, density, sigma_v):
    """P planes of R cold rows (plane p on the grids fmt_att[p] / fmt[p]): sparse keys near zero (Hamming modes: dense random
    codes) and dense random values -> keys, vals int8 codes [P][R][Dp]"""
    Dp = pad_dim(D)
    keys = np.zeros((P, R, Dp), np.int8); vals = np.zeros((P, R, Dp), np.int8)
    for h in range(P):
        mk, mv = (1 << sum(fmt_att[h])) - 1, (1 << sum(fmt[h])) - 1
        if mode == 2:
            k = np.rint(rng.normal(0, sigma_cold, (R, D))) * (rng.random((R, D)) < density * min(1.0, 60.0 / D))
        else:
            k = np.rint(rng.normal(0, 40, (R, D)))
        keys[h, :, :D] = np.clip(k, -min(mk, 127), min(mk, 127))
        vals[h, :, :D] = np.clip(np.rint(rng.normal(0, sigma_v, (R, D))), -min(mv, 127), min(mv, 127))
    return keys, vals


def linear_maps(rng, H, D, fmt_w, lin_density):
    """a signed permutation at 1.0 (or the format's top code), so that every hop's state reaches the output, plus sparse single
    codes -> w_h, float32 [D][D] per hop.  (A dense Gaussian map saturates the later hops' states.)"""
    lin = []
    for h in range(H):
        one = min(1 << fmt_w[h][1], (1 << sum(fmt_w[h])) - 1)
        m = np.sign(rng.normal(0, 1, (D, D))) * (rng.random((D, D)) < lin_density / np.sqrt(D))
        m[np.arange(D), rng.permutation(D)] = one * np.where(rng.random(D) < 0.5, -1, 1)
        lin.append(m)
    return [(lin[h] / float(1 << fmt_w[h][1])).astype(np.float32) for h in range(H)]


def first_states(rng, B, D, fmt_w0, sigma_u):
    """u0 float32 [B][D] on hop 0's weight grid, no column zero"""
    m0 = min((1 << sum(fmt_w0)) - 1, 127)
    u0c = np.clip(np.rint(rng.normal(0, sigma_u, (B, D))), -m0, m0)
    u0c[u0c == 0] = 1
    return (u0c / float(1 << fmt_w0[1])).astype(np.float32)


def loud_values(v, v_min, mv):
    """a hot row's value codes: none below v_min in magnitude, so that the row's term shows in every column"""
    v = v.astype(np.int64)
    v = np.where(np.abs(v) < v_min, np.where(v < 0, -v_min, v_min), v)
    return np.clip(v, -mv, mv)


NUDGES = (None, 3.0, 2.75, 3.25, 2.5, 3.5, 2.25, 2.0, 3.75, 1.75, 4.0, 1.5)


def plant(oracle, name, family, S_in, D=60, H=3, mode=2, fmt=Q52, fmt_att=None, fmt_w=None, fmt_bin=None, cfg_extra=None, max_slots=None,
          deltas=(0, 0, 0), unit=64, amp=60, sigma_cold=2.0, density=0.15, sigma_v=14.0, v_min=6, sigma_u=8.0, env=None, packed=False,
          min_live=2, positions=(), rows_fn=None, forced=None, num_bit=8, behind_cut=False, taps_too=True, lin_density=0.5, cold_anti=False):
    """One case.  `deltas`: one hot row per entry, its score that far under the top code (0: saturated, tied with the other
    zeros).  rows_fn(S) -> candidate hot rows, of which (query + hop) picks a rotating window; forced(q, h, S) -> rows that
    are hot besides.  behind_cut: stories longer than max_slots get a hot row at max_slots - 1 and, at max_slots, a row whose
    key is stronger still -- which the cut story does not hold."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    fmt = [tuple(fmt)] * H if isinstance(fmt[0], int) else [tuple(f) for f in fmt]
    fmt_att = [tuple(f) for f in (fmt_att or ([Q52] * H if fmt[0] == Q07 else fmt))]
    fmt_w = [tuple(f) for f in (fmt_w or fmt_att)]
    cfg = dict(n_hop=H, dim_emb=D, dim_input=4, attention_mode=mode, softmax_variant=0, f_fixed=True, en_lin_map=True, fmt=fmt,
               fmt_w=fmt_w, fmt_att=fmt_att, fmt_bin=tuple(fmt_bin or fmt_att[0]), num_bit=num_bit)
    cfg.update(cfg_extra or {})
    Dp, B = pad_dim(D), len(S_in)
    row_off = np.concatenate([[0], np.cumsum(S_in)]).astype(np.int64)
    R = max(int(row_off[-1]), 1)
    ms = int(max_slots if max_slots is not None else max(S_in))
    keys, vals = cold_memory(rng, len(fmt), R, D, mode, fmt_att, fmt, sigma_cold, density, sigma_v)
    wts = dict(w_ans=np.zeros((4, D), np.float32))
    if cfg["en_lin_map"]:
        wts["w_h"] = linear_maps(rng, H, D, fmt_w, lin_density)
    u0 = first_states(rng, B, D, fmt_w[0], sigma_u)
    case = Case(name, family, cfg, wts, keys, vals, row_off, u0, ms, dict(env or {}), packed, min_live, tuple(positions),
                taps_too=taps_too)
    model = _model(oracle, cfg, wts, H)
    rows_fn = rows_fn or (lambda S: edge_rows(S, unit))
    for q in range(B):
        r0, S, s_in = case.slots(q)
        if S == 0:
            continue
        u = u0[q]
        for h in range(H):
            u_att = _att_input(cfg, u, h)
            fa = fmt_att[h]
            full = min((1 << sum(fa)) - 1, 127)
            mv = min((1 << sum(fmt[h])) - 1, 127)
            hot_key = lambda dl: _hot_key_fixed(oracle, cfg, h, u_att, min(amp, full), dl) if mode == 2 else _hot_key_ham(cfg, h, u_att, dl)
            if cold_anti and mode == 2:                           # cold rows lean AGAINST u_h: their scores sit at the bottom code
                keys[h, r0:r0 + s_in, :D] = -np.sign(u_att) * full
            # (two tied rows give p = 1/2 and one row alone p = 1, both ON a step: a story of two rows gets scores one apart)
            dls = deltas if S > 2 and len(deltas) <= S else (0, 1.0) if S == 2 else deltas[:S]
            rows = list(dict.fromkeys(forced(q, h, S)))[:len(dls)] if forced else []
            if behind_cut and s_in > ms:
                rows = ([ms - 1] + rows)[:len(dls)]
            spread = [int(r) for r in np.random.default_rng([zlib.crc32(name.encode()), q, h]).permutation(S)]
            pool = [r for r in rows_fn(S) + spread if r not in rows]
            rows = rows + _pick(pool, len(dls) - len(rows), q + h)
            spare = [r for r in spread if r not in rows][0] if S > len(rows) else None
            for r, dl in zip(rows, dls):
                keys[h, r0 + r, :D] = hot_key(dl)
                vals[h, r0 + r, :D] = loud_values(vals[h, r0 + r, :D], v_min, mv)
            if behind_cut and s_in > ms:                  # the row behind the cut: every column at full strength, a loud value row
                keys[h, r0 + ms, :D] = np.sign(u_att) * full if mode == 2 else _hot_key_ham(cfg, h, u_att, 0)
                vals[h, r0 + ms, :D] = np.where(np.arange(D) % 2 == 0, mv, -mv)
            # a p on a truncation step: one more warm row moves the softmax total, and with it every p, by a percent or so
            for nudge in NUDGES:
                if nudge is not None:
                    if spare is None or mode != 2:
                        break
                    keys[h, r0 + spare, :D] = hot_key(nudge)
                kf, vf = case.floats(q)
                t = oracle.forward_mem(model, kf, vf, u0[q], taps=("probs", "u"))[1]
                if not near_step(t["probs"][h], fmt[h][1], 2 * CLEAR_REL).any():
                    break
            u = t["u"][h]
            case.hot[(q, h)] = sorted(rows)
    return case


def repeat_case(case, name, family, B, env=None, seed=0):
    """`B` queries, each a copy of one of the planted stories of `case`, in shuffled order: the batch of the persistent grids"""
    rng = np.random.default_rng(seed)
    origin = np.concatenate([rng.permutation(case.B) for _ in range((B + case.B - 1) // case.B)])[:B]
    n = np.array([case.row_off[o + 1] - case.row_off[o] for o in origin], np.int64)
    row_off = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    idx = np.concatenate([np.arange(case.row_off[o], case.row_off[o + 1]) for o in origin])
    out = Case(name, family, case.cfg, case.wts, np.ascontiguousarray(case.keys[:, idx]), np.ascontiguousarray(case.vals[:, idx]), row_off,
               case.u0[origin], case.max_slots, dict(env if env is not None else case.env), case.packed, case.min_live,
               case.positions, {}, origin, taps_too=False)
    return out


# ---- the reference and the conditions -----------------------------------------------------------------------------------------------
ORACLE_TAPS = ("scores", "probs", "o", "u")


def reference(oracle, case):
    """the oracle's taps per query (None for an empty story; a copy shares its original's), computed once per case"""
    if getattr(case, "_ref", None) is None:
        model = _model(oracle, case.cfg, case.wts, case.H)
        done, out = {}, []
        for q in range(case.B):
            key = q if case.origin is None else int(case.origin[q])
            if key not in done:
                kf, vf = case.floats(q)
                done[key] = oracle.forward_mem(model, kf, vf, case.u0[q], taps=ORACLE_TAPS)[1] if kf.shape[1] else None
            out.append(done[key])
        case._ref = out
    return case._ref


def live_rows(case, ref, q, h):
    return np.nonzero(weight_codes(ref[q]["probs"][h], case.cfg["fmt"][h][1]))[0]


def position_flags(case, ref, unit=64):
    """what the live rows of the case cover, by name"""
    f = dict.fromkeys(("row0", "last_row", "group_last", "group_first", "last_partial_group", "neighbour", "at_cut", "lane15_16", "lane31_32",
                       "lane63", "chunk_edges", "every_chunk", "second_group", "beyond_256", "every_query_of_a_quad", "short_last_quad",
                       "short_and_long_neighbours"), False)
    first_live, last_live = {}, {}
    for q in range(case.B):
        r0, S, s_in = case.slots(q)
        if ref[q] is None:
            continue
        for h in range(case.H):
            lv = set(int(r) for r in live_rows(case, ref, q, h))
            first_live[(q, h)] = 0 in lv; last_live[(q, h)] = (S - 1) in lv and S == s_in
            f["row0"] |= 0 in lv; f["last_row"] |= (S - 1) in lv
            f["group_last"] |= any(r % unit == unit - 1 and r + 1 < S for r in lv)
            f["group_first"] |= any(r % unit == 0 and r > 0 for r in lv)
            f["last_partial_group"] |= S % unit != 0 and S > unit and any(r >= unit * (S // unit) for r in lv)
            f["at_cut"] |= s_in > case.max_slots and (case.max_slots - 1) in lv
            f["lane15_16"] |= {15, 16} <= lv; f["lane31_32"] |= {31, 32} <= lv; f["lane63"] |= 63 in lv
            f["chunk_edges"] |= S > 48 and {15, 16, 31, 32, 47, 48} <= lv
            f["every_chunk"] |= S > 48 and all(any(r // 16 == c for r in lv) for c in range(4))
            f["second_group"] |= any(r >= unit for r in lv)
            f["beyond_256"] |= any(r >= 256 for r in lv)
    for (q, h), last in last_live.items():
        f["neighbour"] |= last and first_live.get((q + 1, h), False)
        if last and first_live.get((q + 1, h), False):
            a, b = case.slots(q)[1], case.slots(q + 1)[1]
            f["short_and_long_neighbours"] |= (a <= 16) != (b <= 16)
    live_q = [ref[q] is not None and all(len(live_rows(case, ref, q, h)) for h in range(case.H)) for q in range(case.B)]
    f["every_query_of_a_quad"] = case.B >= 4 and all(live_q[:4 * (case.B // 4)])
    f["short_last_quad"] = case.B % 4 == 3 and all(live_q[-3:])
    return f


def check_conditions(oracle, case, ref=None):
    """C1 .. C6 on the oracle alone; returns the figures the CPU test prints"""
    ref = ref or reference(oracle, case)
    cfg, H, D = case.cfg, case.H, case.cfg["dim_emb"]
    model = _model(oracle, cfg, case.wts, H)
    relu = bool(cfg.get("en_non_lin"))
    live_counts, nz, codes_seen = [], [], 0
    for q in range(case.B):
        if case.origin is not None and q >= 64:
            break
        r0, S, _ = case.slots(q)
        if ref[q] is None:
            continue
        t = ref[q]
        for h in range(H):
            ia, frac = cfg["fmt"][h]
            p = t["probs"][h]
            at = f"{case.name} q{q} h{h} (S={S})"
            assert not near_step(p, frac, CLEAR_REL).any(), f"C2 {at}: a p within {CLEAR_REL} of a truncation step"
            wc = weight_codes(p, frac)
            lv = np.nonzero(wc)[0]
            if S >= 2 and frac >= 1:
                assert len(lv) >= case.min_live, f"C1 {at}: {len(lv)} live rows, the case states {case.min_live}"
            live_counts.append(len(lv))
            codes_seen = max(codes_seen, len(set(wc[lv].tolist())))
            nz.append(float(np.mean(t["o"][h] != 0)))
            for r in lv:                                  # C3: the row's own term of the read-out
                v = case.vals[h, r0 + r, :D].astype(np.float32) / np.float32(1 << frac)
                term = np.array([oracle.L.qo_fixed_mul(float(p[r]), float(x), ia, frac, ia, frac) for x in v])
                assert np.count_nonzero(term) * 4 >= D, f"C3 {at}: row {r} (code {wc[r]}) shows in {np.count_nonzero(term)} of {D} columns"
            # C4: the hop's value plane zeroed
            vz = case.vals.copy(); vz[h, r0:r0 + S] = 0
            kf, vf = case.floats(q, vals=vz)
            u_z = oracle.forward_mem(model, kf, vf, case.u0[q], taps=("u",))[1]["u"][H - 1]
            want = t["u"][H - 1]
            if relu:
                u_z, want = np.maximum(u_z, 0), np.maximum(want, 0)
            assert not np.array_equal(u_z, want), f"C4 {at}: u_out does not see this hop's read-out"
    if case.c5:
        assert codes_seen >= 3, f"C5 {case.name}: at most {codes_seen} different non-zero weight codes in a pair"
    flags = position_flags(case, ref)
    for name in case.positions:
        assert flags[name], f"C6 {case.name}: no live row at `{name}`"
    return dict(live_min=min(live_counts), live_max=max(live_counts), o_nonzero=float(np.mean(nz)), codes=codes_seen, pairs=len(live_counts))


# ---- outputs inside guards, and the comparison ---------------------------------------------------------------------------------------
def out_shapes(case):
    H, D, B, R = case.H, case.cfg["dim_emb"], case.B, case.R
    return {"u_out": ((B, D), np.float32), "codes": ((H, R), np.int32), "scores": ((H, R), np.float32), "probs": ((H, R), np.float32),
            "o": ((B, H, D), np.float32), "u": ((B, H, D), np.float32)}


def payload(case, raw, name):
    shape, dt = out_shapes(case)[name]
    n = int(np.prod(shape)) * 4
    assert raw[name].size == n + 2 * GUARD
    return raw[name][GUARD:GUARD + n].view(dt).reshape(shape)


def blank_outputs(case, taps=ALL_TAPS):
    return {k: np.full(int(np.prod(out_shapes(case)[k][0])) * 4 + 2 * GUARD, FILL, np.uint8) for k in ("u_out",) + tuple(taps)}


def check_outputs(case, ref, raw, taps=ALL_TAPS, label=""):
    """`raw`: name -> the WHOLE guard-filled byte buffer of u_out and of every tap in `taps` as the call left it; `ref`: the
    oracle's taps per query.  Score codes equal; p within rtol 1e-5 / atol 1e-7; o and u of every hop and u_out bit-equal; the
    guards untouched.  Nothing is excused.  Returns the number of queries compared."""
    cfg, H, D = case.cfg, case.H, case.cfg["dim_emb"]
    what = f"{case.name}{label}"
    for k, buf in raw.items():
        n = buf.size - 2 * GUARD
        assert (buf[:GUARD] == FILL).all() and (buf[GUARD + n:] == FILL).all(), f"{what}: the guard of {k} was written"
    got = {k: payload(case, raw, k) for k in raw}
    assert set(got) == {"u_out", *taps}
    unit = case.unit()
    relu = bool(cfg.get("en_non_lin"))
    bad = []
    for q in range(case.B):
        r0, S, _ = case.slots(q)
        t = ref[q]
        if t is None:
            continue
        for h in range(H):
            at = f"{what} q{q} h{h} (S={S})"
            if "codes" in got:
                np.testing.assert_array_equal(got["codes"][h, r0:r0 + S], np.rint(t["scores"][h] / unit[h]).astype(np.int32), err_msg=f"score codes {at}")
            if "scores" in got:
                np.testing.assert_array_equal(got["scores"][h, r0:r0 + S], t["scores"][h], err_msg=f"scores {at}")
            if "probs" in got:
                np.testing.assert_allclose(got["probs"][h, r0:r0 + S], t["probs"][h], rtol=1e-5, atol=1e-7, err_msg=f"p {at}")
            if "o" in got:
                np.testing.assert_array_equal(got["o"][q, h], t["o"][h], err_msg=f"o {at}")
            if "u" in got:
                np.testing.assert_array_equal(got["u"][q, h], t["u"][h], err_msg=f"u {at}")
        want = np.maximum(t["u"][H - 1], 0) if relu else t["u"][H - 1]
        if not np.array_equal(got["u_out"][q], want):
            bad.append(q)
    assert not bad, f"{what}: u_out of {len(bad)} of {case.B} queries differs from the oracle's, first {bad[:6]} (slots {[case.slots(q)[1] for q in bad[:6]]})"
    return sum(t is not None for t in ref)


FAULTS = ("drop_row", "swap_weights", "hop0_plane", "behind_cut")


def fault_applies(case, ref, fault):
    """the first query (and hop) where the planted fault has something to act on, or None"""
    for q in range(case.B):
        if ref[q] is None:
            continue
        r0, S, s_in = case.slots(q)
        if fault == "behind_cut":
            if s_in > S:
                return q, 0
            continue
        for h in range(case.H):
            wc = weight_codes(ref[q]["probs"][h], case.cfg["fmt"][h][1])
            if fault == "drop_row" and wc.any():
                return q, h
            if fault == "swap_weights" and len(set(wc[wc > 0].tolist())) >= 2:
                return q, h
            if fault == "hop0_plane" and h == 1 and wc.any():
                return q, h
    return None


def simulate(oracle, case, taps=ALL_TAPS, fault=None):
    """What a correct kernel hands back (the oracle's own result inside guards) -- or, with `fault`, what a kernel hands back
    that, in one query,
      "drop_row"      leaves one live row's term out of o (the oracle with that value row zeroed);
      "swap_weights"  gives two live rows each other's weight (the oracle with their value rows swapped);
      "hop0_plane"    reads hop 1's values from hop 0's plane;
      "behind_cut"    scores and reads one row more than max_slots allows;
      a callable      reads other value planes (shared_live_cases.py has its faults in this form)."""
    ref = list(reference(oracle, case))
    if fault:
        if callable(fault):                               # (case, ref) -> (query, the value planes that query reads instead)
            q, vals = fault(case, ref)
            h = 0
        else:
            q, h = fault_applies(case, ref, fault)
            vals = case.vals.copy()
        r0, S, _ = case.slots(q)
        n = S
        wc = weight_codes(ref[q]["probs"][h], case.cfg["fmt"][h][1])
        lv = np.nonzero(wc)[0]
        if fault == "drop_row":
            vals[h, r0 + lv[len(lv) // 2]] = 0
        elif fault == "swap_weights":
            a = lv[0]; b = [r for r in lv if wc[r] != wc[a]][0]
            vals[h, [r0 + a, r0 + b]] = vals[h, [r0 + b, r0 + a]]
        elif fault == "hop0_plane":
            vals[1, r0:r0 + S] = case.vals[0, r0:r0 + S]
        elif fault == "behind_cut":
            n = S + 1
        kf, vf = case.floats(q, n=n, vals=vals)
        t = oracle.forward_mem(_model(oracle, case.cfg, case.wts, case.H), kf, vf, case.u0[q], taps=ORACLE_TAPS)[1]
        if fault == "behind_cut":
            t = {k: (v[:, :S] if k in ("scores", "probs") else v) for k, v in t.items()}
        ref[q] = t
    raw = blank_outputs(case, taps)
    out = {k: payload(case, raw, k) for k in raw}
    unit = case.unit()
    for q in range(case.B):
        r0, S, _ = case.slots(q)
        t = ref[q]
        if t is None:
            out["u_out"][q] = case.u0[q] * 0
            continue
        for h in range(case.H):
            for k, v in (("codes", np.rint(t["scores"][h] / unit[h])), ("scores", t["scores"][h]), ("probs", t["probs"][h])):
                if k in out:
                    out[k][h, r0:r0 + S] = v
            if "o" in out:
                out["o"][q, h] = t["o"][h]
            if "u" in out:
                out["u"][q, h] = t["u"][h]
        out["u_out"][q] = np.maximum(t["u"][case.H - 1], 0) if case.cfg.get("en_non_lin") else t["u"][case.H - 1]
    return raw


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
CASES = {}
FAMILIES = {}
# the value and spread knobs that go with an activation format (Q5.2 is plant()'s default)
PRESETS = {
    "q25": dict(fmt=Q25, sigma_v=40.0, v_min=40, sigma_u=20.0, cold_anti=True),        # wide values: code 1 reads out |v| >= 32 only
    "q07": dict(fmt=Q07, fmt_bin=Q25, sigma_v=60.0, v_min=64, sigma_u=30.0),           # attention stays Q5.2
    "short_words": dict(fmt=(3, 2), fmt_att=[(3, 2)] * 3, sigma_u=4.0, sigma_v=8.0, sigma_cold=1.0, density=0.05),
    "frac4": dict(fmt=(3, 4), fmt_att=[Q52] * 3, sigma_v=20.0, v_min=16),
    "frac5": dict(fmt=Q25, fmt_att=[Q52] * 3, sigma_v=40.0, v_min=32),
}


def _add(name, family, preset=None, **kw):
    CASES[name] = dict(family=family, **dict(PRESETS.get(preset, {}), **kw))
    FAMILIES.setdefault(family, []).append(name)


MID_S = [65, 66, 127, 128, 129, 200, 1023, 1024]
OPT_S = [65, 128, 129, 200, 1024]
MID_POS = ("row0", "last_row", "group_last", "group_first", "last_partial_group", "neighbour")
OPT_POS = ("row0", "last_row", "second_group")
GROUP_POS = ("row0", "last_row", "group_last", "group_first", "neighbour")
WIDE_POS = ("row0", "last_row", "beyond_256", "neighbour")
LANE_POS = ("row0", "last_row", "lane15_16", "lane31_32", "lane63")
QUAD_POS = ("row0", "last_row", "every_query_of_a_quad", "short_last_quad")
# hot rows' scores under the top code, one entry per hot row
TIED = (0, 0, 0)                 # p = 1/3 each
STAGGER = (0, 0.75, 1.5, 0, 2.25, 0.75)
OFF_TOP = (0, 0, 0.25)           # Q5.2: p = 0.36, 0.36, 0.28 -- three live rows of code 1, one of them NOT in the top score bin,
#                                  so a kernel that weighs the top bin alone is seen
Q07_LADDER = tuple(0.25 * (i % 5) for i in range(24))
FRAC4_LADDER = (0,) + (0.5,) * 2 + (1.25,) * 6
FRAC5_LADDER = (0,) * 2 + (0.5,) * 5 + (1.0,) * 11
CHUNK_LADDER = (0, 0.5, 1.25, 0, 0.5, 1.25)      # six rows, three weight codes at four fraction bits


def _ends(q, h, S):
    """hop 0: the last row of even stories and the first of odd ones -- a neighbour's row read as one's own would show"""
    return ([S - 1] if q % 2 == 0 else [0]) if h == 0 else []


# 1. the mid kernel
_add("mid_q52", "mid", S_in=MID_S * 2, positions=MID_POS, forced=_ends)
_add("mid_q25", "mid", "q25", S_in=[65, 66, 127, 128, 129, 200] * 2, deltas=STAGGER, positions=MID_POS, forced=_ends)
_add("mid_q07_act", "mid", "q07", S_in=MID_S, deltas=Q07_LADDER, positions=MID_POS, forced=_ends, min_live=20)
_add("mid_short_words", "mid", "short_words", S_in=MID_S, positions=MID_POS, forced=_ends)
for _n, _x in (("relu", dict(en_non_lin=True)), ("no_lin_map", dict(en_lin_map=False)), ("binary", dict(fmt_bin=(0, 0))),
               ("pow2", dict(softmax_variant=1)), ("exp_plan", dict(softmax_variant=2))):
    _add(f"mid_{_n}", "mid_options", S_in=OPT_S, cfg_extra=_x, positions=OPT_POS, forced=_ends)
_add("mid_one_hop", "mid_options", S_in=OPT_S, H=1, positions=OPT_POS, forced=_ends)
_add("mid_five_hops", "mid_options", S_in=OPT_S, H=5, positions=OPT_POS, forced=_ends)
# 2. the cut at the bound
CUT_S = [100, 101, 150, 400, 90, 130, 99, 164]
_add("cut_mid", "cut", S_in=CUT_S, max_slots=100, behind_cut=True, positions=("at_cut", "second_group"))
_add("cut_streaming", "cut", S_in=CUT_S, D=128, max_slots=100, behind_cut=True, positions=("at_cut", "second_group"))
# 3. the streaming kernel
for _D in (128, 256):
    _add(f"fixed_d{_D}_64lanes", "streaming", S_in=[65, 129, 256, 130], D=_D, deltas=OFF_TOP, positions=GROUP_POS, forced=_ends)
    _add(f"fixed_d{_D}_256lanes", "streaming", S_in=[257, 1100, 300], D=_D, unit=256, deltas=OFF_TOP, positions=WIDE_POS, forced=_ends)
_add("fixed_d60_1100", "streaming", S_in=[1100, 1025, 1100], unit=256, deltas=OFF_TOP, positions=WIDE_POS, forced=_ends)
# Q2.5 at 1 800 rows: scan_stop_gate opens (it looks at formats and sizes only) and the launch takes the stopping build.  The cold
# rows sit at the BOTTOM score code (the q25 preset), so the bound e^(x - Xb) summed over them stays far under its threshold: the
# case checks that the stopping build does NOT end a scan whose early rows are live, not that a stop happens behind them -- that
# is test_gpu_scan_stop.py's.  The taps launch is the same kernel with and without QMANN_NO_SCAN_STOP (taps close the gate), so
# it runs once, in the `stop` case.
for _n, _e in (("stop", {}), ("no_stop", {"QMANN_NO_SCAN_STOP": "1"})):
    _add(f"fixed_q25_1800_{_n}", "streaming_stop_gate", "q25", S_in=[1800, 1750], D=128, deltas=STAGGER, env=_e, positions=("row0",),
         rows_fn=lambda S: [3, 0, 40, 64, 100, 7, 63, 130], taps_too=_n == "stop")
# 4. one wavefront
LANES = lambda S: [r for r in (0, 15, 16, 31, 32, 63, S - 1, 1) if r < S]
LANE_TRIPLES = lambda q, h, S: [r for r in ((0, 15, 16), (31, 32, 63), (S - 1, 15, 16), (31, 32, 0))[(q + h) % 4] if r < S]
for _D, _e in ((128, {}), (256, {}), (60, {"QMANN_NO_LEAN": "1"})):
    _add(f"small_d{_D}", "small", S_in=[17, 33, 63, 64, 64, 33], D=_D, rows_fn=LANES, forced=LANE_TRIPLES, env=_e, positions=LANE_POS)
# 5. the lean kernel, both read-out forms, 1 / 2 / 4 / 5 fraction bits
for _sp in ("0", "1"):
    _e = {"QMANN_LEAN_SPARSE": _sp}
    _add(f"lean_frac1_sparse{_sp}", "lean", S_in=[17, 33, 50, 64], fmt=(6, 1), fmt_att=[Q52] * 3, deltas=(0, 1.0), env=_e, min_live=1, unit=16,
         positions=("row0", "last_row"))
    _add(f"lean_frac2_sparse{_sp}", "lean", S_in=[17, 33, 50, 63, 64, 40], rows_fn=LANES, forced=LANE_TRIPLES, env=_e, min_live=3, positions=LANE_POS)
    _add(f"lean_frac4_sparse{_sp}", "lean", "frac4", S_in=[17, 33, 50, 64], deltas=FRAC4_LADDER, env=_e, min_live=9, unit=16, positions=("row0", "last_row"))
    _add(f"lean_frac5_sparse{_sp}", "lean", "frac5", S_in=[33, 50, 64], deltas=FRAC5_LADDER, env=_e, min_live=17, unit=16, positions=("row0", "last_row"))
# 6. the quad kernel, its four-chunk form and the split
QUAD_ENV = {"QMANN_QUAD_MIN_QUERIES": "0"}
CHUNK_EDGES = [15, 16, 31, 32, 47, 48]
_add("quad_short", "quad", S_in=[16, 9, 2, 16, 5, 16, 12, 3, 16, 7, 10], env=QUAD_ENV, unit=4, positions=QUAD_POS + ("neighbour",), forced=_ends)
_add("quad_four_chunks", "quad", "frac4", S_in=[50] * 6 + [49], env=QUAD_ENV, deltas=CHUNK_LADDER, min_live=6,
     rows_fn=lambda S: CHUNK_EDGES + [0, S - 1, 14, 17, 33, 46], forced=lambda q, h, S: CHUNK_EDGES if (q + h) % 3 == 0 else [0, S - 1],
     positions=("row0", "last_row", "chunk_edges", "every_chunk"))
_add("quad_split", "quad", S_in=[5, 50, 9, 40, 16, 17, 3, 64, 12, 30, 2, 4, 8, 20, 6, 7, 10, 11, 13, 3, 5], env=QUAD_ENV, unit=16,
     positions=("row0", "last_row", "neighbour", "short_and_long_neighbours"), forced=_ends)
# 8. k_hops_ham on int8 keys and on planes; 9. the lean and quad forms of the Hamming modes (C1 .. C4: tied hot rows)
HAM = {"appx": dict(mode=3), "v0": dict(mode=10), "v0_2bit": dict(mode=10, num_bit=2), "v1_4bit": dict(mode=11, num_bit=4)}
for _n, _m in HAM.items():
    _D = 256 if _n == "appx" else 128
    _add(f"ham_{_n}_bytes", "ham", S_in=[65, 200, 1000, 130], D=_D, positions=GROUP_POS, forced=_ends, **_m)
    if _m["mode"] != 3:
        _add(f"ham_{_n}_planes", "ham", S_in=[65, 200, 1000, 130], D=_D, packed=True, positions=GROUP_POS, forced=_ends, **_m)
    _add(f"ham_{_n}_lean", "ham_short", S_in=[17, 33, 64, 40], rows_fn=LANES, positions=("row0", "last_row"), **_m)
    _add(f"ham_{_n}_quad", "ham_short", S_in=[16, 9, 3, 16, 5, 12, 2], env=QUAD_ENV, unit=4, positions=QUAD_POS, **_m)
# V1's shortcut threshold (batch_hops_ham.hip: a slot whose e^(x - max) is under total . 2^-frac is dropped before the quotient): beside
# three tied rows, one row two sign flips under them (p . 32 between 1 and 2: just above) and one three flips under (just below).
# (Q2.5 activations, but a Hamming case: C5 is not asked of it, see the module's header.)
_add("ham_v1_threshold", "ham", "q25", S_in=[65, 200, 130, 257], D=128, mode=11, num_bit=4, deltas=(0, 0, 0, 2, 3), min_live=4,
     positions=("row0", "last_row", "second_group"), forced=_ends)

_BUILT = {}


def build(oracle, name):
    if name not in _BUILT:
        spec = dict(CASES[name])
        _BUILT[name] = plant(oracle, name, spec.pop("family"), **spec)
    return _BUILT[name]


# 7. persistent grids: 64 planted stories repeated in shuffled order, more queries than can be resident at once
PERSISTENT = {"persistent_mid": dict(S_in=[65, 66, 67, 70, 72, 75, 78, 80] * 8, max_slots=80, positions=("row0", "last_row", "second_group")),
              # (a batch this large would take the four-chunk quad form: the switch keeps it on the lean kernel)
              "persistent_lean": dict(S_in=[17, 20, 33, 40, 50, 63, 64, 18] * 8, unit=16, positions=("row0", "last_row"),
                                      env={"QMANN_QUAD_MIN_QUERIES": "100000000"}),
              "persistent_quad_chunks": dict(S_in=[17, 18, 20, 24, 33, 17, 19, 50] * 8, unit=16, positions=("row0", "last_row"))}
# Queries one CU can hold at once, AT MOST: rt.h::qm_launch_persistent never launches more workgroups than are resident, and a CU
# holds at most 32 wavefronts whatever a kernel's registers and LDS allow.  k_hops_mid and k_hops_lean walk one query per
# wavefront, k_hops_quad four.  A batch of twice this per CU makes EVERY workgroup of the grid take a second round at least.
PERSISTENT_QUERIES_PER_CU = {"persistent_mid": 32, "persistent_lean": 32, "persistent_quad_chunks": 4 * 32}


def build_persistent(oracle, name, B):
    key = (name, B)
    if key not in _BUILT:
        if name not in _BUILT:
            _BUILT[name] = plant(oracle, name, "persistent", forced=_ends, **PERSISTENT[name])
        _BUILT[key] = repeat_case(_BUILT[name], name, "persistent", B)
    return _BUILT[key]

"""Planted SHARED memories for the fixed-point shared-plane hop kernels (k_hops_shared, its TOP build, and the slot-split pair
k_shared_split_scan / k_shared_split_finish), the conditions they meet and the comparison of test_shared_live_inputs.py (CPU)
and test_gpu_shared_live.py.  Not collected by pytest (no test_ prefix).

WHY.  These kernels fetch a value row only where its weight code Q(p) = floor(p . 2^frac) is not zero.  On the memories of
shared_cases.py no memory longer than 257 slots has such a row (test_shared_live_inputs.py keeps the count as a test), so the
survivor list, the four-row value fetch and its tail, each query's own slice of LDS during the read-out, the weighted sum, the
`o` tap and the term Qa(lu) + Qa(o) of the hop update ran there with o = 0.  live_hops_cases.py planted live rows for the
per-story kernels; this file does it for one memory that B queries read.

HOW.  One memory of S slots is built on the CPU oracle, HOP-MAJOR: for plane h every query's hop input u_{q,h} comes from the
oracle on the planes planted so far, then all queries' hot rows of plane h are planted, then plane h + 1.  No two (query, hop)
pairs share a row of a plane.  Cold rows: sparse keys near zero (live_hops_cases.cold_memory).  Hot rows: sign(u_{q,h}) . a in
every column, a the SMALLEST code whose own score reaches the top code -- the hot rows of query q' are then ordinary rows for
query q, a random walk far under the top.  Graded rows (a score `delta` under the top) come from live_hops_cases._hot_key_fixed.
The linear map is live_hops_cases.linear_maps (a signed permutation plus sparse single codes).  Where a hop's attention scale is
negative the hot rows are aligned AGAINST u.  Three repairs run per plane until it is clean: a foreign hot row that is live for
another query (or carries a quarter of the weight of that query's weakest hot row) is re-drawn on a random 60 % of the columns,
a cold row that does so gets a zero key, and a p on a truncation step gets one warm row of the query's own
(live_hops_cases.NUDGES).  A tied memory (one plane for every hop) is planted in repeated passes over the hops.
plant_shared also takes the Hamming modes (mode, num_bit: shared_ham_live_cases.py); the fixed-point cases below come out byte
for byte as without them (test_shared_ham_live_inputs.py holds their digests).

NATIVE Q2.5 ATTENTION.  The top score is 3.97, e^3.97 = 53, and a cold row scores about 0 (e^0 = 1).  A hot row among n_hot tied
ones survives Q2.5 only while 53 / (n_hot . 53 + S) >= 1/32, i.e. S <= 53 . (32 - n_hot): about 1 500 slots.  Longer memories
take Q5.2 attention (top 31.75) under Q2.5 activations; `q25_native` (the benchmark's format) stays at 700 slots.

CONDITIONS, asserted per case in test_shared_live_inputs.py from the oracle alone.  The memory is handed to
live_hops_cases.check_conditions as B stories that are copies of it (SharedLive.stories), so C1 .. C5 are that file's, unchanged:
  C1  every (query, hop) has at least `min_live` live rows;       C2  no oracle p within 1e-3 (relative) of a step of Q(p);
  C3  every live row's own term is non-zero in a quarter of the columns;   C4  zeroing a hop's values changes u_out;
  C5  a pair with three different non-zero weight codes -- asked of `graded_q25`, the case planted for it.  The other two cases with
      five fraction bits cannot have it: `many_live` exists for 25 .. 28 TIED rows of code 1, and in `q25_native` no p exceeds
      53 / (53 + 700), code 2 (live_hops_cases derives C5 from the formats; SharedLive.c5 states it per case);
  C6  every row of `must` is live for some (query, hop): both ends of the memory, both sides of scan-tile, 16-row and slice edges;
  C7  within every tile of 8 consecutive queries no two queries have the same live rows at the same hop.
No case is exempt from any of them.  Copies also give the per-story call (qmann_hops_i8) its input, bit for bit the same memory.
"""
import functools
import zlib
from dataclasses import dataclass, field

import numpy as np

import live_hops_cases as lc
from live_hops_cases import ALL_TAPS, CLEAR_REL, NUDGES, Q25, Q52, TIED, near_step, pad_dim, weight_codes

K_WAVE, K_UNROLL_DEFAULT = 64, 4                  # hops_common.h (test_shared_live_inputs.py reads them back from the header)


def scan_tile_rows(D):
    """rows of one tile of the key scan, kWave / LPR * kUnrollDefault with LPR = Dp / 16 lanes per row: below it k_hops_shared and
    k_shared_split_scan take scan_rows_short"""
    return K_WAVE // (pad_dim(D) // 16) * K_UNROLL_DEFAULT


def slice_rows(S, want):
    """batch_hops_shared_split.hip::slice_rows: rows per slice for `want` slices, a multiple of 16"""
    return ((S + want - 1) // want + 15) & ~15


@dataclass
class SharedLive:
    name: str
    cfg: dict
    wts: dict
    keys: np.ndarray             # int8 CODES [P][S][Dp], P = n_hop, or 1 for a tied memory
    vals: np.ndarray
    u0: np.ndarray               # float32 [B][D]
    tied: bool
    envs: tuple                  # the QMANN_* switch settings the unsplit call runs under, one dict each
    qts: tuple                   # QMANN_SHARED_QT values (None: the launcher's choice)
    slices: tuple                # forced slice counts of the split call
    min_live: int
    must: tuple                  # C6: rows that are live for some (query, hop)
    copies: bool                 # also run through qmann_hops_i8 on copies of the plane
    c5: bool                     # condition C5 is asked of this case
    hot: dict = field(default_factory=dict)         # (hop, query) -> hot rows

    @property
    def S(self):
        return self.keys.shape[1]

    @property
    def B(self):
        return self.u0.shape[0]

    @property
    def H(self):
        return self.cfg["n_hop"]

    def stories(self):
        """the memory as B per-story copies of it, query q owning rows q S .. (q + 1) S: what live_hops_cases' conditions, reference
        and comparison take, and what qmann_hops_i8 reads.  The shared calls' taps [H][B][S] have that file's layout [H][B . S]."""
        if getattr(self, "_stories", None) is None:
            rep = lambda a: np.ascontiguousarray(np.broadcast_to(a[:, None], (a.shape[0], self.B) + a.shape[1:]).reshape(a.shape[0], self.B * self.S, -1))
            k, v = rep(self.keys), rep(self.vals)
            if self.tied:
                k, v = np.repeat(k, self.H, axis=0), np.repeat(v, self.H, axis=0)
            self._stories = _Copies(self.name, "shared", self.cfg, self.wts, k, v, np.arange(self.B + 1, dtype=np.int64) * self.S, self.u0, self.S,
                                    {}, False, self.min_live, (), dict(self.hot))
            self._stories.c5 = self.c5
        return self._stories


class _Copies(lc.Case):
    c5 = False                   # (live_hops_cases.Case derives it from the formats; here the case states it)


def memory_floats(cfg, keys, vals, tied):
    """kf, vf float32 [n_hop][S][D] as the oracle takes them"""
    H, D = cfg["n_hop"], cfg["dim_emb"]
    pl = (lambda h: 0) if tied else (lambda h: h)
    kf = np.stack([keys[pl(h), :, :D].astype(np.float32) / np.float32(1 << cfg["fmt_att"][h][1]) for h in range(H)])
    vf = np.stack([vals[pl(h), :, :D].astype(np.float32) / np.float32(1 << cfg["fmt"][h][1]) for h in range(H)])
    return kf, vf


# ---- the generator -------------------------------------------------------------------------------------------------------------
def _score(oracle, cfg, h, key, u_att):
    (ia, fa), fb = cfg["fmt_att"][h], cfg["fmt_bin"]
    return float(oracle.dot_mat_vec_fwd((key / float(1 << fa)).astype(np.float32)[None], u_att, False, True, (ia, fa), fb)[0])


def _hot_key_ham(oracle, cfg, h, u_att, delta):
    """the Hamming modes' hot key, as int8 codes on the attention grid.  It is built on the BYTE the kernels compare -- the top
    byte of the oracle's own sign-magnitude word of u (qo_float2fixed at frac = 31 - iwl_att), so that a hop input on a finer grid
    than the attention's, a saturated column and a small negative column (sign set, magnitude 0: the word's minus zero) are what
    the oracle reads.  delta: the sign of round(delta) columns turned, each one step of the score under the top; a pair (flips,
    fine): `fine` score CODES besides, through compared magnitude bits of further columns (V0: one bit a code; V1: bit i of
    num_bit counts 2^(num_bit - 1 - i) codes of 2^-num_bit).  A hop with a negative attention scale gets the key that agrees with
    u in NOTHING the mode counts, so that its score is the lowest there is and its scaled score the largest: V0 -- every compared
    bit (the sign and the top num_bit - 1 magnitude bits) turned; V1 -- the sign turned and the magnitude kept (the column counts
    -sum 2^-(i+1) in full).  The byte 0x80 is the code -128, the float -2^iwl_att, which the oracle reads as minus zero too
    (test_gpu_batch.ham_key_bytes)."""
    ia, nb = cfg["fmt_att"][h][0], cfg["num_bit"]
    byte = (oracle.float2fixed(u_att, ia, 31 - ia).view(np.uint32) >> 24).astype(np.int64)
    flips, fine = delta if isinstance(delta, tuple) else (int(round(delta)), 0)
    byte[:flips] ^= 0x80
    col = flips                                           # `fine`: compared magnitude bits turned in the columns behind, heaviest first
    for i in range(1, nb):
        w = 1 if cfg["attention_mode"] == 10 else 1 << (nb - 1 - i)
        while fine >= w:
            byte[col] ^= 0x80 >> i
            col, fine = col + 1, fine - w
    sc = cfg.get("att_scale")
    if sc is not None and sc[h] < 0:
        byte ^= (0xFF << (8 - nb)) & 0xFF if cfg["attention_mode"] == 10 else 0x80
    return np.where(byte == 0x80, -128, np.where(byte & 0x80, -(byte & 0x7F), byte & 0x7F))


def _hot_key(oracle, cfg, h, u_att, delta, cols=None):
    """the key of a hot row for the hop input u_att: the smallest amplitude whose own score reaches the top code, on `cols`
    (default: every column); delta > 0: live_hops_cases._hot_key_fixed from that amplitude, `delta` under the top.  A hop with a
    negative attention scale gets the key aligned AGAINST u (its scaled score is then the largest).  Hamming modes: _hot_key_ham
    (`cols` plays no part: a key thinned by columns would leave its pair's tie)."""
    if cfg["attention_mode"] != 2:
        return _hot_key_ham(oracle, cfg, h, u_att, delta)
    ia, fa = cfg["fmt_att"][h]
    full = min((1 << (ia + fa)) - 1, 127)
    top = full / float(1 << fa)
    amp = next((a for a in range(1, full + 1) if _score(oracle, cfg, h, lc._hot_key_fixed(oracle, cfg, h, u_att, a, 0, cols), u_att) >= top), full)
    key = lc._hot_key_fixed(oracle, cfg, h, u_att, amp, delta, cols)
    sc = cfg.get("att_scale")
    return -key if sc is not None and sc[h] < 0 else key


def plant_shared(oracle, name, S, D, B, H=3, fmt=Q52, fmt_att=None, fmt_w=None, fmt_bin=None, cfg_extra=None, tied=False, deltas=TIED,
                 n_hot=None, must=(), sigma_cold=2.0, density=0.15, sigma_v=14.0, v_min=6, sigma_u=8.0, lin_density=0.5, min_live=3,
                 envs=({},), qts=(None, 4), slices=(2, 3, 7), passes=1, copies=False, c5=False, rounds=16, mode=2, num_bit=8):
    """One shared memory.  mode, num_bit: the attention (2: fixed point; 10 / 11: Hamming V0 / V1 on the top num_bit bits of the key
    bytes -- shared_ham_live_cases.py; `deltas` then count sign flips under the top, and the cold rows are dense random codes).
    deltas (or deltas(q), deltas(q, h)): one hot row per entry, its score that far under the top (n_hot(q) or n_hot(q, h): so many tied
    rows instead).
    must: rows dealt out to the (hop, query) pairs first.  passes: planting passes over the hops (a tied memory takes several)."""
    seed = zlib.crc32(name.encode())
    rng = np.random.default_rng(seed)
    fmt = [tuple(fmt)] * H if isinstance(fmt[0], int) else [tuple(f) for f in fmt]
    fmt_att = [tuple(f) for f in (fmt_att or fmt)]
    fmt_w = [tuple(f) for f in (fmt_w or fmt_att)]
    cfg = dict(n_hop=H, dim_emb=D, dim_input=4, attention_mode=mode, softmax_variant=0, f_fixed=True, en_lin_map=True, fmt=fmt,
               fmt_w=fmt_w, fmt_att=fmt_att, fmt_bin=tuple(fmt_bin or fmt_att[0]), num_bit=num_bit)
    cfg.update(cfg_extra or {})
    P = 1 if tied else H
    assert not tied or (len(set(fmt)) == 1 and len(set(fmt_att)) == 1), "a tied plane is read on one grid"
    keys, vals = lc.cold_memory(rng, P, S, D, mode, fmt_att, fmt, sigma_cold, density, sigma_v)
    wts = dict(w_ans=np.zeros((4, D), np.float32))
    if cfg["en_lin_map"]:
        wts["w_h"] = lc.linear_maps(rng, H, D, fmt_w, lin_density)
    u0 = lc.first_states(rng, B, D, fmt_w[0], sigma_u)
    pl = (lambda h: 0) if tied else (lambda h: h)
    mv = [min((1 << sum(f)) - 1, 127) for f in fmt]

    # rows: `must` dealt round the pairs, the rest from one shuffle per plane; no row of a plane serves two pairs
    pairs = [(h, q) for h in range(H) for q in range(B)]
    per = lambda f, q, h: f(q, h) if f.__code__.co_argcount == 2 else f(q)          # (a callable of the query, or of query and hop)
    dls = {(h, q): (0,) * per(n_hot, q, h) if n_hot else tuple(per(deltas, q, h) if callable(deltas) else deltas) for h, q in pairs}
    hot = {pr: [] for pr in pairs}
    for j, r in enumerate(dict.fromkeys(must)):
        for i in range(len(pairs)):
            pr = pairs[(j + i) % len(pairs)]
            if len(hot[pr]) < len(dls[pr]) and all(r not in hot[o] for o in pairs if pl(o[0]) == pl(pr[0])):
                hot[pr].append(int(r))
                break
    free = {p: [int(r) for r in np.random.default_rng([seed, p]).permutation(S) if r not in must] for p in range(P)}
    for pr in pairs:
        while len(hot[pr]) < len(dls[pr]):
            hot[pr].append(free[pl(pr[0])].pop())
    owner = {(pl(h), r): (h, q, i) for (h, q), rows in hot.items() for i, r in enumerate(rows)}
    assert len(owner) == sum(len(r) for r in hot.values()), f"{name}: two pairs share a row"
    warm, tries = {}, {}                                   # pair -> its nudge row / the nudges tried

    models = {}

    def evaluate(upto):
        """the oracle's taps of hops 0 .. upto per query on the memory as it stands, and every pair's attention input as far as
        those hops give it (an untied memory: planes behind `upto` are still cold and cost oracle time only)"""
        n = H if tied else max(1, min(upto + 1, H))
        if n not in models:
            models[n] = lc._model(oracle, cfg, wts, n)
        kf, vf = memory_floats(cfg, keys, vals, tied)
        t = [oracle.forward_mem(models[n], kf[:n], vf[:n], u0[q], taps=("scores", "probs", "u"))[1] for q in range(B)]
        u_att = {(h, q): lc._att_input(cfg, u0[q] if h == 0 else t[q]["u"][h - 1], h) for h, q in pairs if h <= n}
        return t, u_att

    def put(h, q, i, u_att, cols=None):
        r = hot[(h, q)][i]
        keys[pl(h), r, :D] = _hot_key(oracle, cfg, h, u_att[(h, q)], dls[(h, q)][i], cols)
        vals[pl(h), r, :D] = lc.loud_values(vals[pl(h), r, :D], v_min, mv[h])

    def dirty(h, t):
        """what keeps hop h from being clean: ("foreign", owner) -- another pair's hot row is live for a query, or carries a
        quarter of the weight of the query's own weakest hot row; ("cold", plane, row) -- a cold row does; ("step", query) -- a p
        of the query lies on a truncation step"""
        out = []
        for q in range(B):
            frac = fmt[h][1]
            p = t[q]["probs"][h]
            own = hot[(h, q)] + ([warm[(h, q)]] if (h, q) in warm else [])
            loud = (weight_codes(p, frac) > 0) | (p >= 0.25 * p[hot[(h, q)]].min())
            loud[own] = False
            for r in np.nonzero(loud)[0]:
                o = owner.get((pl(h), int(r)))
                out.append(("foreign", o) if o is not None else ("cold", (pl(h), int(r))))
            if near_step(p, frac, 2 * CLEAR_REL).any():
                out.append(("step", q))
        return out

    def settle(h):
        """repairs hop h; returns the evaluation of the clean memory, or None"""
        for _ in range(rounds):
            t, u_att = evaluate(h)
            todo = dirty(h, t)
            if not todo:
                return t, u_att
            for kind, x in dict.fromkeys(todo):
                if kind == "foreign":
                    oh, oq, oi = x
                    put(oh, oq, oi, u_att, cols=np.nonzero(rng.random(D) < 0.6)[0])
                elif kind == "cold" and mode == 2:
                    keys[x[0], x[1], :D] = 0
                elif kind == "cold":                            # (Hamming: a zero key is no cold one; another random row)
                    keys[x[0], x[1], :D] = np.clip(np.rint(rng.normal(0, 40, D)), -127, 127)
                else:
                    pr = (h, x)
                    if pr not in warm:
                        warm[pr] = free[pl(h)].pop()
                    tries[pr] = tries.get(pr, 0) + 1
                    keys[pl(h), warm[pr], :D] = _hot_key(oracle, cfg, h, u_att[pr], NUDGES[1 + (tries[pr] - 1) % (len(NUDGES) - 1)])
        return None

    for _ in range(passes):
        state = None
        for h in range(H):
            _, u_att = state if state and not tied else evaluate(h - 1)
            for q in range(B):
                for i in range(len(hot[(h, q)])):
                    put(h, q, i, u_att)
            state = settle(h)
            assert state, f"{name}: hop {h} does not come clean in {rounds} rounds"
        if not any(dirty(h, state[0]) for h in range(H)):               # (the last evaluation saw every hop)
            break
    return SharedLive(name, cfg, wts, keys, vals, u0, tied, tuple(dict(e) for e in envs), tuple(qts), tuple(slices), min_live,
                      tuple(dict.fromkeys(must)), copies, c5, hot)


# ---- the conditions ---------------------------------------------------------------------------------------------------------------
def live_sets(case, ref):
    """(query, hop) -> the frozenset of live rows"""
    st = case.stories()
    return {(q, h): frozenset(int(r) for r in lc.live_rows(st, ref, q, h)) for q in range(case.B) for h in range(case.H)}


def check_conditions(oracle, case):
    """C1 .. C5 through live_hops_cases.check_conditions on the copies, then C6 and C7; returns that routine's figures"""
    st = case.stories()
    ref = lc.reference(oracle, st)
    figures = lc.check_conditions(oracle, st, ref)
    live = live_sets(case, ref)
    covered = set().union(*live.values())
    assert set(case.must) <= covered, f"C6 {case.name}: no live row at {sorted(set(case.must) - covered)}"
    for q0 in range(0, case.B, 8):
        for h in range(case.H):
            sets = [live[(q, h)] for q in range(q0, min(q0 + 8, case.B))]
            assert len(set(sets)) == len(sets), f"C7 {case.name} hop {h}: two queries of the tile at {q0} have the same live rows"
    return figures


def slices_cut_between_live_rows(case, ref, n_slices):
    """a (query, hop) whose live rows lie in more than one slice of the split call, or None"""
    rows = slice_rows(case.S, n_slices)
    for pr, lv in live_sets(case, ref).items():
        if len({r // rows for r in lv}) > 1:
            return pr
    return None


# ---- planted faults of the comparison (live_hops_cases.simulate takes them as callables) ----------------------------------------------
def _codes(st, ref, q, h):
    return weight_codes(ref[q]["probs"][h], st.cfg["fmt"][h][1])


def fault_drop_tail(st, ref):
    """the LAST entry of a survivor list whose length is no multiple of four is left out (the tail of the four-row fetch)"""
    for q in range(st.B):
        for h in range(st.H):
            lv = np.nonzero(_codes(st, ref, q, h))[0]
            if len(lv) % 4:
                vals = st.vals.copy()
                vals[h, st.slots(q)[0] + lv[-1]] = 0
                return q, vals
    return None


def fault_swap_weights(st, ref):
    """two live rows of different codes carry each other's weight"""
    for q in range(st.B):
        for h in range(st.H):
            wc = _codes(st, ref, q, h)
            lv = np.nonzero(wc)[0]
            other = [r for r in lv if wc[r] != wc[lv[0]]] if len(lv) else []
            if other:
                r0, vals = st.slots(q)[0], st.vals.copy()
                vals[h, [r0 + lv[0], r0 + other[0]]] = vals[h, [r0 + other[0], r0 + lv[0]]]
                return q, vals
    return None


def fault_neighbours_o(st, ref):
    """query t carries query t - 1's o at hop 0 (the read-out ran on the neighbour's slice of LDS): the value rows of t's live rows
    are replaced by those of t - 1's, code by code -- applies where both have the same weight codes"""
    for t in range(1, st.B):
        a, b = _codes(st, ref, t - 1, 0), _codes(st, ref, t, 0)
        la, lb = np.nonzero(a)[0], np.nonzero(b)[0]
        la, lb = la[np.argsort(a[la], kind="stable")], lb[np.argsort(b[lb], kind="stable")]
        if len(la) and np.array_equal(a[la], b[lb]):
            vals = st.vals.copy()
            vals[0, st.slots(t)[0] + lb] = st.vals[0, st.slots(t - 1)[0] + la]
            return t, vals
    return None


def fault_hop0_plane(st, ref):
    """hop 1 reads hop 0's value plane (untied memories)"""
    if st.H < 2:
        return None
    r0, S, _ = st.slots(0)
    vals = st.vals.copy()
    vals[1, r0:r0 + S] = st.vals[0, r0:r0 + S]
    return 0, vals


FAULTS = {"drop_tail": fault_drop_tail, "swap_weights": fault_swap_weights, "neighbours_o": fault_neighbours_o, "hop0_plane": fault_hop0_plane}


def simulate(oracle, case, taps=ALL_TAPS, fault=None):
    """what a correct kernel hands back inside guards, or with a name of FAULTS what a kernel with that fault hands back; None
    where the fault has nothing to act on in this case"""
    st = case.stories()
    if fault is None:
        return lc.simulate(oracle, st, taps)
    hit = FAULTS[fault](st, lc.reference(oracle, st))
    return None if hit is None else lc.simulate(oracle, st, taps, fault=lambda c, r: hit)


def check_outputs(oracle, case, raw, taps=ALL_TAPS, label=""):
    """live_hops_cases.check_outputs on the copies: score codes and scores equal, p within rtol 1e-5 / atol 1e-7, o and u of every
    hop and u_out bit-equal to the oracle, the guards untouched, no query excused.  Returns the number of queries compared."""
    st = case.stories()
    n = lc.check_outputs(st, lc.reference(oracle, st), raw, taps, label)
    assert n == case.B
    return n


# ---- the cases ---------------------------------------------------------------------------------------------------------------------
Q25_ACT = dict(fmt=Q25, fmt_att=[Q52] * 3, fmt_bin=Q52, sigma_v=40.0, v_min=32)          # Q2.5 activations under Q5.2 attention
GRADED4 = (0, 0.25, 0.75, 1.5)                    # Q5.2 attention: scores one, two and three grid steps apart
SHORT_D = 128
_T = scan_tile_rows(SHORT_D)


def _edges(S, D, n_slices=3):
    """both ends, both sides of the first and last scan-tile edge, of 16-row edges and of the edge of the split call's slices"""
    t, s = scan_tile_rows(D), slice_rows(S, n_slices)
    last_t, last_16 = t * ((S - 1) // t), 16 * ((S - 1) // 16)
    rows = [0, S - 1, t - 1, t, last_t - 1, last_t, 15, 16, last_16 - 1, last_16, s - 1, s]
    return tuple(dict.fromkeys(r for r in rows if 0 <= r < S))


CASES = {
    # 1. the tile sizes, forced: 19 queries leave a tail of 1 (tiles of 2) and 3 (4 and 8).  Odd queries hold one of their three live
    #    rows a quarter under the top (p = 0.36, 0.36, 0.28): neighbours in a tile then differ in their tables by score code (ptab,
    #    kplut) too, not only in their live rows
    "tiles": dict(S=1500, D=128, B=19, deltas=lambda q: lc.OFF_TOP if q % 2 else TIED, must=_edges(1500, 128), qts=(1, 2, 4, 8), copies=True),
    # 2. the word-length-7 scan and the general one (QMANN_NO_W7)
    "w7_off": dict(S=300, D=128, B=6, must=_edges(300, 128), envs=({}, {"QMANN_NO_W7": "1"})),
    # 3. the launcher's own tile on a long memory (choose_qt's n_slots >= 4096 branch), D = 60 in rows of 64
    "long_d60": dict(S=4097, D=60, B=9, must=(4095, 4096, 0) + _edges(4097, 60), copies=True),
    "d256": dict(S=1000, D=256, B=5, must=_edges(1000, 256)),
    # 5. four graded rows per pair: three or more different weight codes (C5)
    "graded_q25": dict(S=4097, D=128, B=6, deltas=GRADED4, min_live=4, must=(0, 4096), c5=True, **Q25_ACT),
    # 6. the benchmark's format, native Q2.5 attention: S under the bound of the header
    "q25_native": dict(S=700, D=128, B=9, fmt=Q25, deltas=(0, 0.25, 0.5), min_live=3, sigma_v=40.0, v_min=40, sigma_u=20.0, must=(0, 699)),
    # 7. 25 + (q mod 4) tied rows of code 1 and |value code| >= 32: survivor lists of 25, 26, 27 and 28 rows, every residue of the
    #    four-row fetch.  p . 32 = 32/25 .. 32/28 = 1.28, 1.23, 1.19, 1.14: clear of a step
    "many_live": dict(S=1000, D=128, B=5, n_hot=lambda q: 25 + q % 4, min_live=25, must=(0, 999), **Q25_ACT),
    # 8. one plane for every hop
    "tied_plane": dict(S=700, D=128, B=11, tied=True, passes=4, must=_edges(700, 128), qts=(None, 8), copies=True),
    # 9. below one scan tile of rows (scan_rows_short), exactly one tile, one tile and a row; two and four queries per tile
    f"short_scan_{_T - 1}": dict(S=_T - 1, D=SHORT_D, B=5, must=(0, _T - 2, 15, 16), qts=(2, 4), slices=(2, 7)),
    f"short_scan_{_T}": dict(S=_T, D=SHORT_D, B=5, must=(0, _T - 1, 15, 16), qts=(2, 4), slices=(2, 7)),
    f"short_scan_{_T + 1}": dict(S=_T + 1, D=SHORT_D, B=5, must=(0, _T, 15, 16, _T - 1), qts=(2, 4), slices=(2, 7)),
    # 10. softmax and update variants
    "pow2": dict(S=257, D=128, B=6, cfg_extra=dict(softmax_variant=1), must=(0, 256)),
    "exp_plan": dict(S=300, D=128, B=6, cfg_extra=dict(softmax_variant=2), must=(0, 299)),
    # (scaled top scores 15.9, 15.9 and 7.9: e^7.9 = 2 800 against 300 cold rows still gives p = 0.32 to each of three tied rows)
    "scale_negative": dict(S=300, D=60, B=5, cfg_extra=dict(att_scale=[-0.5, 0.5, -0.25]), must=(0, 299)),
    "relu": dict(S=300, D=128, B=6, cfg_extra=dict(en_non_lin=True), must=(0, 299)),
    "eight_hops": dict(S=130, D=60, B=5, H=8, must=(0, 129)),
}
TOP_K = (5, 16)


@functools.lru_cache(maxsize=None)
def _oracle():
    from pyoracle import Oracle
    return Oracle()


@functools.lru_cache(maxsize=None)
def shared_live(name):
    """the planted case, built once per process"""
    return plant_shared(_oracle(), name, **CASES[name])

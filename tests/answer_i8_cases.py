"""Seeded inputs and the exact reference of the int8 answer layer (qmann_answer_i8), shared by test_answer_i8_inputs.py (CPU:
the inputs do what each case is for, the reference agrees with the oracle) and test_gpu_answer_i8.py.  Plain numpy, no GPU.

The reference is integer arithmetic:
  cu     = clip(trunc(u . 2^frac_u), -M, M), M = 2^(iwl_u + frac_u) - 1      qfmt.h::qm_code
  K      = cu @ cw.T                                                         |K| < 2^23: exact in int64, float64 and float32
  logits = K . 2^-(frac_u + frac_w)                                          exact in float32
  pred   = the highest index with K == max K                                 lib/layer_cuda.cu:1918-1939
  match, cost: over labels < V only
  probabilities: a float64 softmax of the exact logits to the base e (softmax_base 0) or 2 (softmax_base 1).  For the two-kernel
  form at the bases 1 and 2 the GPU tests take the oracle's softmax_fwd of that variant on the exact logits instead (its total is
  a float sum in index order, which the float64 total does not reproduce: up to V . 2^-24 apart).

Every case plants duplicated answer rows (exact ties: inside one 16-column block, 16 and 64 rows apart, row 0 = row V - 1) with a
query that makes each pair win, rows of u that are all zero (every logit equal: pred = V - 1), and labels outside the dictionary
(V + 3 and 0xFFFFFFFF) at every seventh query."""
import functools
import zlib
from types import SimpleNamespace

import numpy as np

OUTSIDE = 0xFFFFFFFF


def _case_table():
    c = {}

    def add(name, family, D, V, B, fu=(5, 2), fw=(1, 6), bases=(0, 1), **kw):
        c[name] = dict(name=name, family=family, D=D, V=V, B=B, fu=fu, fw=fw, bases=bases, **kw)

    # formats: every byte format of u against four weight fractions -- scale 2^0 .. 2^-14; Q2.5 x Q1.6 is the bench's pair
    for f in range(8):
        for g in (0, 3, 6, 7):
            add(f"fmt_u{7 - f}.{f}_w{7 - g}.{g}", "formats", 60, 70, 40, fu=(7 - f, f), fw=(7 - g, g), bases=(0, 1, 2))
    add("fmt_narrow_u2.2_w1.2", "formats", 60, 70, 40, fu=(2, 2), fw=(1, 2), bases=(0, 1, 2))
    # widths: the scalar-load branch (D % 4 != 0), every Dp (64, 128, 256), D == Dp
    for D in (1, 3, 17, 61, 63, 64, 65, 127, 129, 191, 193, 255, 256):
        add(f"width_{D}", "widths", D, 70, 21)
    # dictionaries: V < 4 (records do not fit the workspace), every 16-column block and 64-row tile edge, several slices
    for V in (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 127, 128, 129, 321):
        add(f"dict_{V}", "dictionaries", 60, V, 64, bases=(0, 1, 2))
    add("dict_4033", "dictionaries", 60, 4033, 64, bases=(0, 1, 2))        # 64 slices of one tile, the last holds ONE column
    add("dict_4097", "dictionaries", 60, 4097, 2000, bases=(0, 1, 2))      # 13 slices of five tiles, ragged
    # batches: the 16-query wavefront tile and the 64-query workgroup
    for B in (1, 15, 16, 17, 63, 64, 65):
        add(f"batch_{B}", "batches", 128, 130, B, bases=(0, 1, 2))
    add("batch_1_zero", "batches", 128, 130, 1, bases=(0, 1, 2), lone="zero")   # (a lone query cannot be both zero and not)
    # 513 query blocks: ONE slice walks two tiles; 32 805 queries > 2 048 . 16: a second trip of the combine kernel's loop
    add("one_slice_two_tiles", "big", 60, 65, 32805)
    # 8 229 > 8 192 workgroups: a second trip of k_answer<true>'s loop (two-kernel form)
    add("k_answer_second_trip", "big", 60, 65, 8229)
    # the same for k_answer<false> (V > 256), through qmann_answer_f32_serial
    add("k_answer_float_second_trip", "float", 60, 257, 8229, bases=(0, 1, 2))
    # u off the activation grid and beyond its range
    add("offgrid_q5.2", "offgrid", 60, 70, 40, fu=(5, 2))
    add("offgrid_q2.5", "offgrid", 61, 70, 40, fu=(2, 5))
    return c


CASES = _case_table()
I8_CASES = sorted(n for n, c in CASES.items() if c["family"] != "float")


def qm_code(u, fmt):
    """two's-complement code of Q(fmt)(u): truncation toward zero, symmetric saturation (int64)"""
    iwl, frac = fmt
    M = (1 << (iwl + frac)) - 1
    return np.clip(np.trunc(np.asarray(u, np.float64) * (1 << frac)), -M, M).astype(np.int64)


def tie_pairs(V):
    """(a, b): row b of the matrix is a copy of row a"""
    p = []
    if V >= 2:
        p.append((0, V - 1))
    if V >= 7:
        p.append((2, 5))
    if V >= 21:
        p.append((3, 19))
    if V >= 67:
        p.append((1, 65))
    return p


def _freeze(ns):
    for v in vars(ns).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ns


@functools.lru_cache(maxsize=None)
def case(name):
    """inputs and reference of one case; computed once per process, arrays read-only"""
    c = CASES[name]
    D, V, B, fu, fw = c["D"], c["V"], c["B"], c["fu"], c["fw"]
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    Mu, Mw = (1 << sum(fu)) - 1, (1 << sum(fw)) - 1
    cw = np.clip(np.rint(rng.normal(0, Mw / 3.0, (V, D))), -Mw, Mw).astype(np.int64)
    pairs = tie_pairs(V)
    for a, b in pairs:
        if D < 17:                                        # too few columns for the row's own direction to single it out:
            cw[a] = Mw * rng.choice([-1, 1], D)           # the duplicated rows are the longest ones
        cw[b] = cw[a]
    cu0 = np.clip(np.rint(rng.normal(0, Mu / 3.0, (B, D))), -Mu, Mu).astype(np.int64)
    q = np.arange(B)
    zero_rows = q % 11 == 5
    planted = np.zeros(B, bool)
    if c.get("lone") == "zero":
        zero_rows[:] = True
    else:
        for i, (a, _) in enumerate(pairs):
            if i < B:
                cu0[i] = Mu * np.sign(cw[a])             # the duplicated row and its copy win this query
                planted[i] = True
    cu0[zero_rows] = 0
    u = cu0 / float(1 << fu[1])
    if c["family"] == "offgrid":
        step = 1.0 / (1 << fu[1])
        free = ~(zero_rows | planted)
        kind = rng.integers(0, 3, (B, D))                 # 0: on the grid, 1: 0.4 steps toward zero, 2: away from zero
        sgn = np.where(cu0 >= 0, 1.0, -1.0)
        u = u + np.where(free[:, None], np.where(kind == 1, -0.4, np.where(kind == 2, 0.4, 0.0)) * step * sgn, 0.0)
        lim = float(1 << fu[0])
        sat = (rng.random((B, D)) < 0.05) & free[:, None]
        sat_val = rng.choice(np.array([lim, -lim, 1.5 * lim, -1.5 * lim, 3.0e4, -3.0e4]), (B, D))
        u = np.where(sat, sat_val, u)
    u = u.astype(np.float32)
    cu = qm_code(u, fu)
    u_grid = (cu / float(1 << fu[1])).astype(np.float32)
    K = (cu.astype(np.float64) @ cw.T.astype(np.float64)).astype(np.int64)          # exact: |K| < 2^23
    kmax = int(np.abs(K).max())
    shift = fu[1] + fw[1]
    logits = (K.astype(np.float64) / float(1 << shift)).astype(np.float32)
    best = K.max(1)
    pred = (V - 1 - np.argmax(K[:, ::-1] == best[:, None], axis=1)).astype(np.int64)
    n_at_max = (K == best[:, None]).sum(1)
    labels = rng.integers(0, V, B).astype(np.int64)
    labels[q % 5 == 1] = V - 1
    labels[q % 9 == 2] = pred[q % 9 == 2]
    labels[(q % 7 == 3) & ((q // 7) % 2 == 0)] = V + 3
    labels[(q % 7 == 3) & ((q // 7) % 2 == 1)] = OUTSIDE
    if c.get("lone") == "zero":
        labels[:] = OUTSIDE
    inside = labels < V
    w_i8 = np.zeros((V, 64 if D <= 64 else 128 if D <= 128 else 256), np.int8)
    w_i8[:, :D] = cw
    ns = SimpleNamespace(name=name, family=c["family"], D=D, V=V, B=B, fu=fu, fw=fw, bases=c["bases"], Dp=w_i8.shape[1],
                         u=u, u_grid=u_grid, cu=cu, cw=cw, w_i8=w_i8, w_float=(cw / float(1 << fw[1])).astype(np.float32),
                         logits=logits, shift=shift, kmax=kmax, pred=pred, n_at_max=n_at_max, pairs=tuple(pairs),
                         zero_rows=zero_rows, planted=planted, labels=labels.astype(np.uint32), inside=inside,
                         match=int((pred[inside] == labels[inside]).sum()), max_abs_logit=np.abs(logits).max(1))
    return _freeze(ns)


_LOG_BASE = {0: 1.0, 1: float(np.log(2.0))}


@functools.lru_cache(maxsize=None)
def _normaliser(name, base):
    lg = case(name).logits.astype(np.float64)
    mx = lg.max(1)
    tot = np.exp((lg - mx[:, None]) * _LOG_BASE[base]).sum(1)
    return mx, tot


def prob64(name, base, q, y):
    """float64 softmax probability of answers y for queries q (arrays or scalars); base 0: e^x, 1: 2^x"""
    mx, tot = _normaliser(name, base)
    return np.exp((case(name).logits[q, y].astype(np.float64) - mx[q]) * _LOG_BASE[base]) / tot[q]


def probs64(name, base):
    """the whole float64 softmax [B][V] (not kept)"""
    mx, tot = _normaliser(name, base)
    return np.exp((case(name).logits.astype(np.float64) - mx[:, None]) * _LOG_BASE[base]) / tot[:, None]


def cost64(name, base):
    """-sum of p[q][label q] over the labels inside the dictionary"""
    c = case(name)
    q = np.flatnonzero(c.inside)
    return -float(prob64(name, base, q, c.labels[q].astype(np.int64)).sum())


def oracle_probs(oracle, logits, base):
    """the oracle's softmax of variant `base` (0 e^x double total, 1 2^x and 2 exp_plan: float total in index order), row by row"""
    return np.stack([oracle.softmax_fwd(row, variant=base) for row in logits])


def highest_argmax(x):
    """per row the highest index that holds the row's maximum"""
    return x.shape[1] - 1 - np.argmax(x[:, ::-1] == x.max(1)[:, None], axis=1)

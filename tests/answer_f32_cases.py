"""Seeded inputs and references of the float answer layer (qmann_answer_f32, qmann_answer_f32_serial, qmann_answer_topk_f32:
csrc/batch_answer.hip::answer_f32_impl), shared by test_answer_f32_inputs.py (CPU: the inputs do what each case is for, the
references agree with the oracle) and test_gpu_answer_f32.py.  Plain numpy, no GPU, no library call.

References -- none is the code under test:
  R64   float64 softmax, base e (softmax_base 0) or 2 (1), of u.astype(f64) @ W.astype(f64).T: the fused bf16 form's reference
  Rser  the reference's own loop (lib/layer_cuda.cu:70-80) in numpy: columns 0 .. D-1, the product rounded to float32, then the
        add rounded to float32 -- the serial kernels' logits bit for bit.  Probabilities from them: a float64 softmax at base 0,
        the oracle's softmax_fwd of the variant at bases 1 and 2 (its float total in index order), as answer_i8_cases.oracle_probs
  pred  the highest index at the maximum

Which query may be excused from `pred == the reference's`: duplicated rows of W give equal probabilities in every arithmetic
that treats rows alike, and a zero row of u makes every logit zero, so such EXACT ties are never excused: the lower index of a
duplicated pair is taken out, and what remains decides.  A query is `decided` where the two best remaining reference
probabilities differ by more than 1e-6 (or nothing else remains); the others are excused, at most 10 % of a case.

Kernel of a shape (restated from the launcher, asserted against a table in the CPU test):
  fused   D <= 64, V <= 256, base 0 or 1: k_answer_mfma<T>, T the smallest of 2 3 4 5 8 12 15 16 with 16 T >= V
  serial  V <= 256 and (D . (lpq . vpt) + 16 . qpw . D) . 4 <= 78 KiB: k_answer_small<lpq, vpt, qb>; otherwise k_answer<false>

A seed that fails a condition of the CPU test is replaced in SEEDS (name -> seed) and stays listed there."""
import functools
import zlib
from types import SimpleNamespace

import numpy as np

from float_hops_cases import FILL, GUARD          # 4 096 bytes of 0xA5 on both sides of every output

OUTSIDE = 0xFFFFFFFF
LOG_BASE = {0: 1.0, 1: float(np.log(2.0))}
MAX_SWEEP_B = 140_000
SEEDS = {}                                        # name -> seed, where the default (a hash of the name) failed a condition


def seed_of(name):
    return SEEDS.get(name, zlib.crc32(name.encode()))


# ---- which kernel serves a shape --------------------------------------------------------------------------------------------------
def fused_tiles(V):
    t = (V + 15) // 16
    return next(x for x in (2, 3, 4, 5, 8, 12, 15, 16) if x >= t)


def takes_fused(D, V, base):
    return D <= 64 and V <= 256 and base != 2


def small_plan(D, V):
    """ans_small_plan: (lpq, vpt, qb, queries per wavefront, LDS bytes, fits)"""
    lpq = 16 if V <= 128 else 64
    qb = 2 if V <= 96 else (1 if V <= 128 else 4)
    vpt = (V + lpq - 1) // lpq
    vpt = 2 if vpt <= 2 else 4 if vpt <= 4 else 6 if vpt <= 6 else 8
    qpw = 64 // lpq * qb
    lds = (D * lpq * vpt + 16 * qpw * D) * 4
    return SimpleNamespace(lpq=lpq, vpt=4 if lpq == 64 else vpt, qb=qb, qpw=qpw, lds=lds, fits=V <= 256 and lds <= 78 * 1024)


def serial_kernel(D, V):
    p = small_plan(D, V)
    return f"k_answer_small<{p.lpq},{p.vpt},{p.qb}>" if p.fits else "k_answer<false>"


def fits_edge(V):
    """the largest D whose transposed matrix still fits (V <= 256)"""
    D = 1
    while small_plan(D + 1, V).fits:
        D += 1
    return D


def resident_groups(n_cu, waves, waves_per_simd, lds):
    """rt.h::qm_resident_groups"""
    per_cu = min(waves_per_simd * 4 // waves, (160 * 1024) // (lds + 256), 32 // waves)
    return n_cu * max(per_cu, 1)


def sweep_queries(call, D, V, n_cu):
    """queries one trip of the kernel's persistent loop covers on n_cu compute units"""
    if call == "fused":
        return 256 * resident_groups(n_cu, 16, 4, 3 * fused_tiles(V) * 16 * 144 + 256)
    p = small_plan(D, V)
    if not p.fits:
        return 8192
    return 16 * p.qpw * resident_groups(n_cu, 16, 8, p.lds)


# ---- the cases ----------------------------------------------------------------------------------------------------------------------
def _case_table():
    c = {}

    def add(name, family, D, V, B, calls=("fused", "serial"), bases=(0, 1, 2), **kw):
        c[name] = dict(name=name, family=family, D=D, V=V, B=B, calls=calls, bases=bases, **kw)

    # order: cancelling column pairs, the serial calls only -- one shape per serial kernel, an odd width, one beyond the fits edge
    for D, V in [(60, 30), (60, 64), (60, 96), (60, 128), (60, 200), (60, 300), (17, 70), (64, 200)]:
        add(f"order_D{D}_V{V}", "order", D, V, 40, calls=("serial",))
    # widths, fused: the vec4 branch with the low float4 alone (4, 12, 28, 36), an empty second K step (<= 32), D < 8, D = 1; 65
    # leaves the fused form
    for D in (1, 2, 3, 4, 5, 8, 12, 28, 31, 32, 33, 36, 59, 61, 63, 64, 65):
        add(f"width_fused_{D}", "widths", D, 70, 21)
    # widths, serial: D 1 and 3, both sides of every fits edge, D 200
    for D in (1, 3, 200):
        add(f"width_serial_{D}", "widths", D, 70, 21, calls=("serial",))
    for V in (32, 64, 96, 128, 256):
        e = fits_edge(V)
        for D in (e, e + 1):
            add(f"width_serial_V{V}_D{D}", "widths", D, V, 21, calls=("serial",))
    # dictionaries: the edges of every T class of the fused form and every vpt class of the serial one
    for V in (1, 2, 3, 16, 17, 32, 33, 48, 49, 64, 65, 80, 81, 96, 97, 128, 129, 192, 193, 240, 241, 256, 257):
        add(f"dict_{V}", "dictionaries", 60, V, 64)
    # batches: below one task, the 16-query task, the 256-query workgroup, 4 or 8 queries per wavefront, 64 or 128 per workgroup
    for V in (30, 200):
        for B in (1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129, 255, 256, 257):
            add(f"batch_V{V}_{B}", "batches", 60, V, B)
    for V in (70, 238):
        add(f"ties_labels_{V}", "ties_labels", 60, V, V + 42)
    add("magnitudes", "magnitudes", 60, 70, 64, calls=("fused",), bases=(0, 1))
    return c


CASES = _case_table()
FUSED_T_OF_SWEEP = {20: 2, 40: 3, 60: 4, 70: 5, 100: 8, 150: 12, 230: 15, 250: 16}
SWEEP = {}                                            # name -> (call, V, with probs)
for _V, _T in FUSED_T_OF_SWEEP.items():
    SWEEP[f"sweep_fused_T{_T}_V{_V}"] = ("fused", _V, _T == 16)
for _V in (30, 64, 96, 128, 200, 257):
    SWEEP[f"sweep_serial_V{_V}"] = ("serial", _V, _V == 200)
SWEEP_RANKED = (30, 200)
SWEEP_D = 60
# one trip of each kernel's loop on 256 compute units (an MI355X in SPX mode)
SWEEP_256 = {**{n: 65536 for n in SWEEP if n.startswith("sweep_fused")}, "sweep_serial_V30": 65536, "sweep_serial_V64": 65536,
             "sweep_serial_V96": 65536, "sweep_serial_V128": 32768, "sweep_serial_V200": 32768, "sweep_serial_V257": 8192}

ORDER_VARIANTS = ("reversed", "fma", "even_odd", "f64")


# ---- arithmetic ---------------------------------------------------------------------------------------------------------------------
def rser_logits(W, u, order=None):
    """the reference's loop: per column a float32 product, then a float32 add (numpy rounds each float32 operation once)"""
    W, u = np.asarray(W, np.float32), np.asarray(u, np.float32)
    acc = np.zeros((u.shape[0], W.shape[0]), np.float32)
    for c in (range(W.shape[1]) if order is None else order):
        t = u[:, c, None] * W[None, :, c]
        acc = acc + t
    return acc


def variant_logits(W, u, kind):
    """four WRONG evaluations of the serial loop (condition O1)"""
    D = W.shape[1]
    if kind == "reversed":
        return rser_logits(W, u, range(D - 1, -1, -1))
    if kind == "even_odd":
        return rser_logits(W, u, list(range(0, D, 2)) + list(range(1, D, 2)))
    W64, u64 = W.astype(np.float64), u.astype(np.float64)
    if kind == "f64":
        return (u64 @ W64.T).astype(np.float32)
    assert kind == "fma"                              # one rounding per multiply-add (the product is exact in float64)
    acc = np.zeros((u.shape[0], W.shape[0]), np.float32)
    for c in range(D):
        acc = (acc.astype(np.float64) + u64[:, c, None] * W64[None, :, c]).astype(np.float32)
    return acc


def pairwise_logits(W, u):
    """float32 products summed pairwise in float32 (condition M2: another correct float evaluation)"""
    t = u[:, None, :] * W[None, :, :]
    while t.shape[2] > 1:
        if t.shape[2] % 2:
            t = np.concatenate([t, np.zeros(t.shape[:2] + (1,), np.float32)], axis=2)
        t = t[:, :, 0::2] + t[:, :, 1::2]
    return t[:, :, 0]


def two_images(W):
    """W cut to its first two bf16 images (condition M1)"""
    W = np.ascontiguousarray(W, np.float32)
    b1 = (W.view(np.uint32) & 0xFFFF0000).view(np.float32)
    r1 = W - b1
    b2 = (r1.view(np.uint32) & 0xFFFF0000).view(np.float32)
    return b1 + b2


def logits64(W, u, pairs=()):
    L = u.astype(np.float64) @ W.astype(np.float64).T
    for a, b in pairs:                                # equal rows: equal logits (whatever order the BLAS sums a column in)
        L[:, b] = L[:, a]
    return L


def softmax64(L, base):
    z = (L.astype(np.float64) - L.max(1, keepdims=True)) * LOG_BASE[base]
    e = np.exp(z)
    return e / e.sum(1, keepdims=True)


def highest_argmax(x):
    return x.shape[1] - 1 - np.argmax(x[:, ::-1] == x.max(1)[:, None], axis=1)


def decide(c, p):
    """(decided [B] bool, pred [B]) of reference probabilities p: see the module docstring"""
    p = np.array(p, np.float64)
    for a, _ in c.pairs:
        p[:, a] = -1.0                                # the copy at the higher index stands for the pair
    pred = highest_argmax(p)
    if p.shape[1] - len(c.pairs) >= 2:
        top = np.sort(p, axis=1)[:, -2:]
        decided = (top[:, 1] - top[:, 0]) > 1e-6
    else:
        decided = np.ones(len(p), bool)
    decided = decided | c.zero_rows
    pred = np.where(c.zero_rows, c.V - 1, pred)
    return decided, pred


def cost_of(c, p, lo=0, hi=None):
    """-sum of p[q][label q] over the labels inside the dictionary, queries lo .. hi - 1"""
    hi = c.B if hi is None else hi
    q = np.arange(lo, hi)[c.inside[lo:hi]]
    return -float(np.asarray(p)[q, c.labels[q].astype(np.int64)].astype(np.float64).sum())


def _freeze(ns):
    for v in vars(ns).values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ns


# ---- inputs -------------------------------------------------------------------------------------------------------------------------
def _grid_u(rng, B, D):
    return (np.clip(np.rint(rng.normal(0, 20, (B, D))), -127, 127) / 4.0).astype(np.float32)          # Q5.2 codes


def _random_inputs(rng, D, V, B):
    """the tests' usual draw, W scaled down where a logit would pass 14: the fused form's relative bound holds to 16"""
    W = rng.normal(0, 0.1, (V, D)).astype(np.float32)
    u = _grid_u(rng, B, D)
    top = np.abs(logits64(W, u)).max()
    if top > 14.0:
        W = (W * np.float32(14.0 / top)).astype(np.float32)
    return W, u


def _labels(rng, B, V, pred):
    q = np.arange(B)
    labels = rng.integers(0, V, B).astype(np.int64)
    labels[q % 5 == 1] = V - 1
    labels[q % 9 == 2] = pred[q % 9 == 2]
    labels[(q % 7 == 3) & ((q // 7) % 2 == 0)] = V + 3
    labels[(q % 7 == 3) & ((q // 7) % 2 == 1)] = OUTSIDE
    return labels


TIE_PAIRS = ((5, 6), (9, 13), (18, 34), (1, 65))      # one group of four answers; neighbouring lane groups; 16 and 64 apart (tiles)


def _order_inputs(rng, D, V, B):
    h = D // 2
    even = rng.normal(0, 3000, (V, h)).astype(np.float32)
    k = rng.integers(-2, 3, (V, h))
    odd = (even.astype(np.float64) + k / 256.0).astype(np.float32)
    assert np.abs(odd.astype(np.float64) - even.astype(np.float64) - k / 256.0).max() < 2.0 ** -20   # (exact but for entries below 1)
    W = np.zeros((V, D), np.float32)
    W[:, 0:2 * h:2], W[:, 1:2 * h:2] = even, odd
    if D % 2:
        W[:, D - 1] = rng.normal(0, 3000, V).astype(np.float32)
    s = rng.choice([-1.0, 1.0], (B, h))
    cc = rng.integers(64, 128, (B, h))
    u = np.zeros((B, D), np.float32)                  # (odd D: the last column of u is zero)
    u[:, 0:2 * h:2], u[:, 1:2 * h:2] = s * cc / 4.0, -s * cc / 4.0
    return W, u


def _ties_inputs(rng, D, V, B):
    W, u = _random_inputs(rng, D, V, B)
    W = np.array(W)
    pairs = TIE_PAIRS + ((0, V - 1),)
    for a, b in pairs:
        W[b] = W[a]
    u = np.array(u)
    for i, (a, _) in enumerate(pairs):
        u[i] = 0.5 * np.sign(W[a])                    # the duplicated row and its copy win this query, at a logit of about 2.4
    u[np.arange(B) % 11 == 5] = 0.0
    return W, u, pairs


# every row of W is scaled (by a power of two) so that its largest |logit| lies in (A / 2, A].  A is as high as M2 lets it be: the
# float32 sums' error grows with it as the third image's weight does (at 15.5: M2 6e-6), and the low mantissa byte is drawn from
# 0xE1 .. 0xFF so that the third image weighs 0.9 . 2^-16 of an entry instead of 2^-17 on average
MAG_AMPLITUDE = 7.75
MAG_QUIET = 52                                        # columns from here on hold W . 2^-7: a code of +-127 at frac 0 stays a small term


def _magnitude_inputs(rng, D, V, B):
    m = (rng.integers(1 << 15, 1 << 16, (V, D)) << 8) | rng.integers(0xE0, 0x100, (V, D)) | 1        # 24 significant bits
    e = rng.integers(-20, 7, (V, D))
    W = (rng.choice([-1.0, 1.0], (V, D)) * m * np.exp2(e - 24.0)).astype(np.float32)
    assert ((W.view(np.uint32) & 1) == 1).all()
    Wb = W.view(np.uint32)
    Wb[0:10, 0:20] &= 0xFFFF0000                                                    # at most 8 significant bits: one image
    Wb[10:20, 20:40] &= 0xFFFFFF00                                                  # at most 16: two images
    W[:, MAG_QUIET:] *= np.float32(2.0 ** -7)
    q = np.arange(B)
    frac = q % 8
    amp = np.minimum(127, 1 << frac)
    codes = np.rint(rng.uniform(-1, 1, (B, D)) * amp[:, None]).astype(np.int64)
    codes[:, 0], codes[:, 1] = 1, -1                                                # +-1 and +-127 in every byte format
    codes[:, MAG_QUIET], codes[:, MAG_QUIET + 1] = 127, -127
    u = (codes / np.exp2(frac)[:, None]).astype(np.float32)
    top = np.abs(logits64(W, u)).max(0)
    W = (W * np.exp2(np.floor(np.log2(MAG_AMPLITUDE / top)))[:, None].astype(np.float32)).astype(np.float32)
    W[20:24, 40:44] = -0.0
    W[24:28, 44:48] = (rng.integers(1, 1 << 23, (4, 4)).astype(np.uint32) | (rng.integers(0, 2, (4, 4)).astype(np.uint32) << 31)).view(np.float32)
    return W, u, frac


def _finish(name, c, W, u, pairs=(), labels=None, rng=None, **extra):
    """references of a case small enough to keep whole"""
    D, V, B = c["D"], c["V"], c["B"]
    W, u = np.ascontiguousarray(W, np.float32), np.ascontiguousarray(u, np.float32)
    L64, Lser = logits64(W, u, pairs), rser_logits(W, u)
    zero_rows = ~u.any(1)
    ns = SimpleNamespace(name=name, family=c["family"], D=D, V=V, B=B, calls=c["calls"], bases=c["bases"], W=W, u=u, L64=L64,
                         Lser=Lser, pairs=tuple(pairs), zero_rows=zero_rows, max_abs_logit=float(np.abs(L64).max()), **extra)
    _, pred = decide(ns, softmax64(Lser, 0))
    labels = _labels(rng, B, V, pred) if labels is None else labels
    ns.labels = labels.astype(np.uint32)
    ns.inside = labels < V
    return _freeze(ns)


@functools.lru_cache(maxsize=None)
def case(name):
    """inputs and logits of one case; computed once per process, arrays read-only"""
    c = CASES[name]
    D, V, B, fam = c["D"], c["V"], c["B"], c["family"]
    rng = np.random.default_rng(seed_of(name))
    if fam == "order":
        W, u = _order_inputs(rng, D, V, B)
        return _finish(name, c, W, u, rng=rng)
    if fam == "ties_labels":
        W, u, pairs = _ties_inputs(rng, D, V, B)
        q = np.arange(B)
        labels = np.where(q < V, q % V, rng.integers(0, V, B)).astype(np.int64)      # every position of the select tree holds the label once
        late = (q >= V) & (q % 7 == 3)
        labels[late & ((q // 7) % 2 == 0)] = V + 3
        labels[late & ((q // 7) % 2 == 1)] = OUTSIDE
        return _finish(name, c, W, u, pairs=pairs, labels=labels)
    if fam == "magnitudes":
        W, u, frac = _magnitude_inputs(rng, D, V, B)
        return _finish(name, c, W, u, rng=rng, frac=frac)
    W, u = _random_inputs(rng, D, V, B)
    return _finish(name, c, W, u, rng=rng)


def probs_r64(c, base):
    return softmax64(c.L64, base)


_SER = {}


def probs_rser(oracle, c, base):
    """probabilities of the serial reference: float64 softmax at base 0, the oracle's softmax of the variant at 1 and 2"""
    key = (c.name, c.B, base)
    if key not in _SER:
        p = softmax64(c.Lser, 0) if base == 0 else np.stack([oracle.softmax_fwd(row, variant=base) for row in c.Lser])
        p.setflags(write=False)
        _SER[key] = p
    return _SER[key]


def sweep_b(name, n_cu):
    call, V, _ = SWEEP[name]
    return min(sweep_queries(call, SWEEP_D, V, n_cu) + 37, MAX_SWEEP_B)


@functools.lru_cache(maxsize=1)
def sweep_case(name, n_cu):
    """second_sweep: one trip of the kernel's loop + 37 queries.  Nothing of size B x V is kept: logits64 is recomputed on demand.
    Labels: inside the dictionary for the first 64 queries and those of the second trip (both served by the same lanes, whose
    partial cost and match carry over), 0xFFFFFFFF between -- a cost of a hundred terms, not of B atomic float additions.
    sample: the last 128 queries and 256 others, where Rser is computed."""
    call, V, with_probs = SWEEP[name] if name in SWEEP else ("ranked", int(name.rsplit("V", 1)[1]), False)
    D = SWEEP_D
    one = sweep_queries("serial" if call == "ranked" else call, D, V, n_cu)
    B = min(one + 37, MAX_SWEEP_B)
    rng = np.random.default_rng(seed_of(name))
    W, u = _random_inputs(rng, D, V, B)
    sample = np.concatenate([np.sort(rng.choice(B - 128, 256, replace=False)), np.arange(B - 128, B)])
    q = np.arange(B)
    ns = SimpleNamespace(name=name, family="second_sweep", call=call, D=D, V=V, B=B, one_sweep=one, with_probs=with_probs, W=W, u=u,
                         pairs=(), zero_rows=np.zeros(B, bool), sample=sample, Lser=rser_logits(W, u[sample]))
    L64 = logits64(W, u)
    ns.max_abs_logit = float(np.abs(L64).max())
    labels = rng.integers(0, V, B).astype(np.int64)
    labels[q % 9 == 2] = highest_argmax(L64)[q % 9 == 2]
    labels[(q >= 64) & (q < one)] = OUTSIDE
    labels[q % 7 == 3] = OUTSIDE
    ns.labels = labels.astype(np.uint32)
    ns.inside = labels < V
    ns.decided, ns.pred64, ns.cost64 = {}, {}, {}
    for base in (0, 1):                               # (exp_plan changes sm_exp alone, nothing a second trip touches: the small cases run it)
        p = softmax64(L64, base)
        ns.decided[base], ns.pred64[base] = decide(ns, p)
        ns.cost64[base] = cost_of(ns, p)
    return _freeze(ns)

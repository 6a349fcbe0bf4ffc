"""One hop of ATTENTION_MODE 1 (csrc/batch_hops_float.hip) in float64, numpy only.

The kernel's read-out o[c] = sum_r p[r] . C[r][c] is a float32 sum over every slot in an order of its own, so it cannot be
checked bit for bit.  This reference states what CAN be checked exactly and gives the rest a derived bound:

  scores   exact integers times 2^-(frac_w + frac_src): both operands sit on grids, no tolerance applies;
  p        stock e^x base: exp(x - max) / sum in float64.  The 2^x and exp_plan bases and the shift variant are DEFINED by the
           float32 steps of csrc/hops_common.h (sm_exp_plan, sm_quot, the serial float total), which are redone here in
           numpy float32;
  o64, m   o64[c] = sum_r p[r] . C[r][c] and m[c] = sum_r p[r] . |C[r][c]|, float64;
  lu       the linear map in integers, as hops_common.h::linmap_update documents it: each product Qw(Qw(H) . Qbin(u)) clamped,
           the row sum clamped to Qw, then shifted to the activation grid toward zero (BINARY_MODE: u binarised to +-1);
  u_next   integer codes clamp(lu_a + trunc(o64 . 2^frac_a));
  near     the columns where |o64 . 2^frac_a - nearest integer| <= bound[c] . 2^frac_a: truncation is toward zero, so the integers
           are the steps, and only there may a correct float32 read-out give the neighbouring code.

bound[c] = (1e-5 + (S + 8) . 2^-24) . m[c]:
  1e-5              the project's float tolerance on p (header of batch_hops_float.hip): every term may be off by that share;
  (S + 8) . 2^-24   the standard bound of a float32 sum of S terms taken in any order with one rounding per FMA (every partial
                    sum is at most m in magnitude); the 8 covers the lane folds and the four wavefront partials.
Where m[c] = 0 every term is an exact zero in any arithmetic: such a column is never `near`.

Memories are sign-magnitude bytes; 0x80 ("minus zero") decodes to 0.
"""
from dataclasses import dataclass

import numpy as np

P_RTOL = 1e-5


def decode(b):
    """sign-magnitude bytes -> integer codes (int64); 0x80 is 0"""
    u = np.asarray(b).view(np.uint8).astype(np.int64)
    return np.where(u & 0x80, -(u & 0x7F), u & 0x7F)


def encode(codes):
    """integer codes (|code| <= 127) -> sign-magnitude bytes (never 0x80)"""
    c = np.asarray(codes).astype(np.int64)
    assert np.abs(c).max(initial=0) <= 127
    return np.where(c < 0, (-c) | 0x80, c).astype(np.uint8)


def max_code(fmt):
    return (1 << (fmt[0] + fmt[1])) - 1


def code_of(x, fmt):
    """qfmt.h::qm_code on float32 grid values: trunc(x . 2^frac) toward zero, clamped at +-(2^(iwl+frac) - 1)"""
    m = max_code(fmt)
    return np.clip(np.trunc(np.asarray(x, np.float64) * (1 << fmt[1])), -m, m).astype(np.int64)


def on_grid_codes(u, fmt):
    """codes of a float32 vector that must sit ON the grid of fmt (asserted)"""
    x = np.asarray(u, np.float64) * (1 << fmt[1])
    k = np.rint(x)
    assert np.array_equal(x, k), "state is off its grid"
    assert np.abs(k).max(initial=0) <= max_code(fmt), "state exceeds its format"
    return k.astype(np.int64)


def src_fmt(cfg, h):
    """the grid the state entering hop h sits on: emb_q's (w[0]) for hop 0, sv[h-1]'s afterwards"""
    return tuple(cfg["fmt_w"][0]) if h == 0 else tuple(cfg["fmt"][h - 1])


def exp_plan(x):
    """hops_common.h::sm_exp_plan, float32"""
    x = x.astype(np.float32)
    f = np.float32
    o = f(0.597226) * x + f(0.933989)
    o = np.maximum(o, f(0.141642) * x + f(0.43981))
    o = np.maximum(o, f(0.070265) * x + f(0.10888))
    return np.maximum(o, f(0.0) * x + f(0.0)).astype(np.float32)


def serial_total_f32(e):
    """the CPU softmax's float total: S dependent float32 additions in slot order"""
    return np.add.accumulate(e.astype(np.float32), dtype=np.float32)[-1]


def softmax(scores, h, cfg):
    """p per slot (float64 array) from the float32 scores of hop h"""
    base = cfg.get("softmax_variant", 0)
    shift = bool(cfg.get("softmax_shift_based"))
    x = np.asarray(scores, np.float32)
    if cfg.get("att_scale") is not None:
        x = (x * np.float32(cfg["att_scale"][h])).astype(np.float32)         # the scale layer: one float product
    d = (x - x.max()).astype(np.float32)
    if base == 0 and not shift:
        e = np.exp(d.astype(np.float64))
        return e / e.sum()
    if base == 0:                                                            # e^x / llrint(log2(total)), total a double
        e = np.exp(d).astype(np.float32)
        total = e.astype(np.float64).sum()
        div = np.float32(np.rint(np.log2(np.float32(total))))
        return (e / div).astype(np.float64)
    if base == 2:
        e = exp_plan(d)
    else:
        e = np.exp2((d + np.float32(1.0)).astype(np.float32) if shift else d).astype(np.float32)
    return (e / serial_total_f32(e)).astype(np.float64)


def lin_map_codes(u, lin, h, cfg):
    """code of Qa(lu) on the activation grid of hop h.  lin: integer codes [D][D] of H on the grid w[h], or None."""
    fa, fw, fb = tuple(cfg["fmt"][h]), tuple(cfg["fmt_w"][h]), tuple(cfg["fmt_bin"])
    maxa, maxw = max_code(fa), max_code(fw)
    if not cfg.get("en_lin_map", True):
        return code_of(u, fa)
    if fb[0] + fb[1] == 0:
        ub = np.where(np.asarray(u) >= 0, 1, -1).astype(np.int64)
    else:
        ub = code_of(u, fb)
    hk = np.asarray(lin, np.int64)
    mag = np.minimum((np.abs(hk) * np.abs(ub)[None, :]) >> fb[1], maxw)      # Qw(Qw(H) . Qbin(u)) per product
    row = (np.sign(hk) * np.sign(ub)[None, :] * mag).sum(axis=1)
    kw = np.clip(row, -maxw, maxw)
    m = np.abs(kw)
    ma = m << (fa[1] - fw[1]) if fa[1] >= fw[1] else m >> (fw[1] - fa[1])     # to the activation grid, toward zero
    return np.sign(kw) * np.minimum(ma, maxa)


@dataclass
class Hop:
    codes: np.ndarray      # int64 [S]   score in units of 2^-(frac_w + frac_src)
    scores: np.ndarray     # float32 [S]
    p: np.ndarray          # float64 [S]
    o64: np.ndarray        # float64 [D]
    m: np.ndarray          # float64 [D]
    bound: np.ndarray      # float64 [D]
    lu: np.ndarray         # int64 [D]   code of Qa(lu)
    u_next: np.ndarray     # int64 [D]   codes on the activation grid of this hop
    near: np.ndarray       # bool [D]
    frac_a: int
    max_a: int

    def u_next_f32(self):
        return (self.u_next.astype(np.float64) / (1 << self.frac_a)).astype(np.float32)

    def allowed(self):
        """per column the two codes a correct float32 read-out may give: equal outside `near`; inside, the truncations on
        either side of the step"""
        x = self.o64 * (1 << self.frac_a)
        k = np.rint(x).astype(np.int64)
        lo = np.where(k > 0, k - 1, k)
        hi = np.where(k < 0, k + 1, k)
        maxa = self.max_a
        f = lambda t: np.clip(self.lu + np.clip(t, -maxa, maxa), -maxa, maxa)
        a, b = f(lo), f(hi)
        return np.where(self.near, a, self.u_next), np.where(self.near, b, self.u_next)


def update_codes(lu, o, fa):
    """u' = clamp(lu_a + Qa(o)) in codes"""
    maxa = max_code(fa)
    return np.clip(lu + code_of(o, fa), -maxa, maxa)


def hop(u, kb, vb, h, cfg, lin=None, value_decode=decode):
    """u float32 [D] on its grid; kb / vb uint8 [S][Dp] of hop h (S may be 0); lin: codes of H[h] or None"""
    D = cfg["dim_emb"]
    fa, fw, fs = tuple(cfg["fmt"][h]), tuple(cfg["fmt_w"][h]), src_fmt(cfg, h)
    S = kb.shape[0]
    ku = on_grid_codes(u, fs)
    if cfg.get("en_non_lin") and h > 0:
        ku = np.maximum(ku, 0)                                               # the attention reads RELU(sv[h-1])
    codes = decode(kb)[:, :D] @ ku
    assert np.abs(codes).max(initial=0) < (1 << 24)
    scores = (codes.astype(np.float64) / (1 << (fw[1] + fs[1]))).astype(np.float32)
    if S:
        p = softmax(scores, h, cfg)
        C = value_decode(vb)[:, :D].astype(np.float64) / (1 << fw[1])
        o64, m = p @ C, p @ np.abs(C)
    else:
        p = np.zeros(0)
        o64, m = np.zeros(D), np.zeros(D)
    bound = (P_RTOL + (S + 8) * 2.0 ** -24) * m
    lu = lin_map_codes(u, lin, h, cfg)
    x = o64 * (1 << fa[1])
    near = (np.abs(x - np.rint(x)) <= bound * (1 << fa[1])) & (m > 0)
    return Hop(codes, scores, p, o64, m, bound, lu, update_codes(lu, o64, fa), near, fa[1], max_code(fa))


def relu_if(u, on):
    return np.where(u > 0, u, np.float32(0.0)).astype(np.float32) if on else np.asarray(u, np.float32)


def n_eff(p):
    """(sum p)^2 / sum p^2: the effective number of slots, 1 / sum p^2 wherever p sums to 1 (every variant but the shift-based)"""
    p = np.asarray(p, np.float64)
    return float(p.sum() ** 2 / (p * p).sum()) if p.size else 0.0

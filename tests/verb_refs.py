"""Plain numpy restatements of the optional-layer verbs of boundary B, for the tests of verbs that no program of the
reference instantiates on its CPU branch (lib/layer.c prints "not implemented" for them), so neither the oracle's C nor
the reference's live C code covers them.  Each function states, in float32 and in the reference's evaluation order, what
the CUDA definition computes; the line numbers are those of the reference's lib/layer_cuda.cu and lib/layer_cuda.h.

Conventions: float32 in, float32 out; one product or sum per rounding (no fused multiply-add); a reduction is a serial
loop in index order.  Nothing here imports the product or the oracle.
"""
from __future__ import annotations

import numpy as np

F32 = np.float32
ACTS = ("NULL", "SIGMOID", "RELU")


def quant(x, iwl, frac):
    """CUDA_FLOAT_QUANT (lib/layer_cuda.h:207-253), f_mode 3: t = trunc(x . 2^frac) toward zero, saturated at
    +-(2^(iwl+frac) - 1), decoded as (float)t / 2^frac; iwl + frac == 0 binarises to +-1.  The macro computes in the type
    of its argument: a float32 array is multiplied in float32, a float64 array (the sigmoid expressions) in float64."""
    x = np.asarray(x)
    assert x.dtype in (np.float32, np.float64)
    if iwl + frac == 0:
        return np.where(x >= 0, F32(1), F32(-1)).astype(F32)
    m = (1 << (iwl + frac)) - 1
    maxf = F32(m) / F32(1 << frac)                       # CUDA_FIXED_MAX_FLOAT is a float
    t = np.trunc(x * x.dtype.type(1 << frac))
    t = np.where(x > maxf, m, np.where(x < -maxf, -m, t))
    return (t.astype(F32) / F32(1 << frac)).astype(F32) + F32(0)          # (+0: a "minus zero" word decodes to 0)


def sigmoid_f64(x):
    """the float64 sigmoid the float-mode SIGMOID is measured against"""
    return 1.0 / (1.0 + np.exp(-np.asarray(x, np.float64)))


def _sigmoid_expr(x):
    """1.0/(1.0+expf(-in)) (:1682, :1684): expf in float, the sum and the quotient in double"""
    return 1.0 / (1.0 + np.exp(-np.asarray(x, F32)).astype(np.float64))


def activation_fwd(x, act, f_fixed=False, fmt=(0, 0)):
    """cuda_activation_fwd (:4548-4584) -> _cuda_bypass / _cuda_sigmoid / _cuda_relu (:1664-1703).  The fixed-point
    sigmoid hands the DOUBLE expression to the quantiser (:1682): sigmoid(20) = 1 - 2e-9 is 0.75 in Q5.2, where its float
    rounding, 1.0, would stay 1.0."""
    assert act in ACTS
    x = np.asarray(x, F32)
    if act == "SIGMOID":
        v = _sigmoid_expr(x)
        if not f_fixed:
            v = v.astype(F32)
    elif act == "RELU":
        v = np.where(x > 0, x, F32(0)).astype(F32)
    else:
        v = x
    return quant(v, *fmt) if f_fixed else v.astype(F32)


def activation_bwd(out, grad_in, act, f_fixed=False, fmt=(0, 0)):
    """cuda_activation_bwd (:4587-4614) -> _cuda_bypass / _cuda_sigmoid_bwd / _cuda_relu_bwd (:1664-1674, :1705-1731):
    the gradient format is Q(1, iwl + frac - 1); the sigmoid derivative is (grad_in * out) in float, times
    (1.0 - out) in double, and that double goes into the quantiser (:1711)."""
    assert act in ACTS
    out, grad_in = np.asarray(out, F32), np.asarray(grad_in, F32)
    gf = (1, fmt[0] + fmt[1] - 1)
    if act == "SIGMOID":
        g = (grad_in * out).astype(F32).astype(np.float64) * (1.0 - out.astype(np.float64))
        if not f_fixed:
            g = g.astype(F32)
    elif act == "RELU":
        g = np.where(out > 0, grad_in, F32(0)).astype(F32)
    else:
        g = grad_in
    return quant(g, *gf) if f_fixed else g.astype(F32)


def scale_fwd(x, w):
    """cuda_scale_fwd (:4805-4827) -> _cuda_vec_const_mult (:1551-1558): out = in . w; f_fixed and the format are ignored"""
    return (np.asarray(x, F32) * F32(w)).astype(F32)


def scale_bwd(x, grad_in, w):
    """cuda_scale_bwd (:4830-4858): w_del = sum_i grad_in[i] . in[i], ASSIGNED, a serial float sum in index order
    (_cuda_vec_vec_mult_accum_scalar :1560-1579); grad_out = grad_in . w.  Returns (w_del, grad_out)."""
    x, grad_in = np.asarray(x, F32), np.asarray(grad_in, F32)
    s = F32(0)
    for t in (grad_in * x).astype(F32):
        s = F32(s + t)
    return s, (grad_in * F32(w)).astype(F32)


def scale_w_up(w, w_del, dim, batch_size, lr, lam):
    """cuda_scale_w_up (:4861-4905): _cuda_w_up (:1834-1849) with batch_size . dim as the divisor,
    w += lr / n . w_del + lr . lambda . w, and then the verb clears w_del (:4902).  Returns (w, w_del)."""
    w, w_del, lr, lam = F32(w), F32(w_del), F32(lr), F32(lam)
    n = F32(np.uint32(batch_size * dim))
    step = F32(F32(lr / n) * w_del)
    decay = F32(F32(lr * lam) * w)
    return F32(w + F32(step + decay)), F32(0)


def mult_e_fwd(a, b):
    """cuda_mult_e_vec_fwd / cuda_mult_e_mat_fwd (:4234-4263, :4373-4394) -> _cuda_vec_vec_mult (:1581-1586)"""
    return (np.asarray(a, F32) * np.asarray(b, F32)).astype(F32)


def mult_e_bwd(a, b, grad_in):
    """cuda_mult_e_vec_bwd / cuda_mult_e_mat_bwd (:4266-4299, :4397-4425): grad_out_a = grad_in . b, grad_out_b = grad_in . a"""
    g = np.asarray(grad_in, F32)
    return (g * np.asarray(b, F32)).astype(F32), (g * np.asarray(a, F32)).astype(F32)


# ---- inputs shared by the CPU check of the restatements and the GPU tests of the verbs -----------------------------
DIMS = (1, 7, 60, 257, 1000)
FIXED_FORMATS = ((5, 2), (2, 5), (0, 7))
SIGMOID_POINTS = 10000
# largest relative error of the library's float SIGMOID against the float64 sigmoid over SIGMOID_POINTS points in
# [-20, 20], as measured on an MI355X (tests/test_gpu_ops.py::test_activation_sigmoid_float_error prints it); the tests
# assert four times this
SIGMOID_REL_ERR_MEASURED = 9.78e-8
SIGMOID_EXCUSED_SHARE = 0.01


def act_inputs(dim, fmt=None, seed=0):
    """off-grid values around the format's range (float mode: around +-8), with values beyond the range, exact zeros,
    a tiny negative and on-grid values sprinkled in; the same array for every kind of activation"""
    lim = 2.0 ** fmt[0] if fmt else 8.0
    rng = np.random.default_rng(7700 + 131 * dim + 17 * seed + (fmt[0] * 8 + fmt[1] if fmt else 99))
    x = rng.normal(0, 0.6 * lim + 0.05, dim).astype(F32)
    x[::7] = F32(lim * 1.5)
    x[3::11] = F32(-lim * 2.0)
    x[1::5] = F32(0.0)
    x[2::13] = F32(-1e-5)
    if fmt:
        x[4::9] = quant(x[4::9], *fmt)
    return x


def sigmoid_points():
    return np.linspace(-20.0, 20.0, SIGMOID_POINTS).astype(F32)


def near_step(v64, fmt, bound):
    """where the float64 value v64 lies within the relative `bound` of a rounding step of the grid (then a result one
    code away is excused)"""
    y = np.asarray(v64, np.float64) * (1 << fmt[1])
    return np.abs(y - np.rint(y)) <= bound * np.maximum(np.abs(y), 1.0)


def bwd_inputs(dim, fmt=None, seed=0):
    """(out, grad_in) for the activation derivatives: outputs in [0, 1] with exact zeros and exact ones, gradients around
    the Q(1, wl - 1) range with a few beyond it"""
    rng = np.random.default_rng(8800 + 131 * dim + 17 * seed + (fmt[0] * 8 + fmt[1] if fmt else 99))
    out = rng.random(dim).astype(F32)
    out[::5] = F32(0.0)
    out[2::7] = F32(1.0)
    g = rng.normal(0, 0.7, dim).astype(F32)
    g[1::9] = F32(2.5)
    g[4::11] = F32(-3.0)
    return out, g

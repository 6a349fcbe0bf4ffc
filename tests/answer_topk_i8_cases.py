"""Inputs and the exact reference of the ranked int8 answer layer (qmann_answer_topk_i8), shared by test_answer_topk_i8_inputs.py
(CPU) and test_gpu_answer_topk_i8.py.  Plain numpy, no GPU.

The cases are answer_i8_cases.py's (by import: their planted ties and all-zero queries are what a ranking must get right) plus a
RAMP family of two: cw[v][0] = clip(v - 160, -127, 127), every other column 0, and queries +M, -M and 0 in column 0, cycled over
the batch.
  +M: the logit codes ascend with the index, so every tile brings new candidates, and end in a plateau of 34 tied answers (the
      clipped rows 287 .. 320 at V 321) that crosses 16-column blocks, 64-row tiles and slices;
  -M: the codes descend, so nothing passes after the first tile of a slice, and the 34 tied answers 0 .. 33 lead;
   0: every code equal, the ranking is V - 1, V - 2, ...
At V 4 033 a batch this small gets 64 slices of one tile, the last holding one column.

The reference: K = cu @ cw.T (the integer the matrix cores produce), ranked by a stable sort on (-K, -v): larger code first,
equal codes: higher index first.  Probabilities: the float64 softmax of the exact logits (answer_i8_cases.prob64's formula)."""
import functools
from types import SimpleNamespace

import numpy as np

from answer_i8_cases import CASES, I8_CASES, _LOG_BASE, _freeze, case, qm_code

TOP = 16                                    # QMANN_MAX_TOPK
KS = (1, 2, 5, 16)

RAMPS = {"ramp_321": dict(V=321, B=19), "ramp_4033": dict(V=4033, B=19)}
RAMP_D, RAMP_FU, RAMP_FW = 4, (5, 2), (1, 6)

FORMAT_PAIRS = ["fmt_u7.0_w7.0", "fmt_u0.7_w0.7", "fmt_u2.5_w1.6", "fmt_u5.2_w1.6", "fmt_u4.3_w4.3", "fmt_u0.7_w7.0",
                "fmt_u7.0_w0.7", "fmt_narrow_u2.2_w1.2"]          # scale 2^0 first, 2^-14 second
GPU_CASES = (sorted(n for n in I8_CASES if CASES[n]["family"] in ("widths", "dictionaries", "batches", "offgrid"))
             + ["one_slice_two_tiles"] + FORMAT_PAIRS + sorted(RAMPS))


def ramp_kind(B):
    """per query: +1 (the +M query), -1 (-M), 0 (all zero)"""
    return np.array([1, -1, 0])[np.arange(B) % 3]


@functools.lru_cache(maxsize=None)
def tcase(name):
    """a case with its integer logit codes K [B][V]; computed once per process, arrays read-only"""
    if name not in RAMPS:
        c = case(name)
        K = c.cu @ c.cw.T                                           # int64, exact
        assert np.array_equal(K.astype(np.float64) / float(1 << c.shift), c.logits.astype(np.float64))
        return _freeze(SimpleNamespace(name=name, D=c.D, V=c.V, B=c.B, Dp=c.Dp, fu=c.fu, fw=c.fw, bases=c.bases, u=c.u, cu=c.cu,
                                       cw=c.cw, w_i8=c.w_i8, K=K, logits=c.logits, shift=c.shift, pred=c.pred))
    V, B = RAMPS[name]["V"], RAMPS[name]["B"]
    Mu = (1 << sum(RAMP_FU)) - 1
    cw = np.zeros((V, RAMP_D), np.int64)
    cw[:, 0] = np.clip(np.arange(V) - 160, -127, 127)
    u = np.zeros((B, RAMP_D), np.float32)
    u[:, 0] = ramp_kind(B) * Mu / float(1 << RAMP_FU[1])
    cu = qm_code(u, RAMP_FU)
    K = cu @ cw.T
    shift = RAMP_FU[1] + RAMP_FW[1]
    w_i8 = np.zeros((V, 64), np.int8)
    w_i8[:, :RAMP_D] = cw
    best = K.max(1)
    pred = (V - 1 - np.argmax(K[:, ::-1] == best[:, None], axis=1)).astype(np.int64)
    return _freeze(SimpleNamespace(name=name, D=RAMP_D, V=V, B=B, Dp=64, fu=RAMP_FU, fw=RAMP_FW, bases=(0, 1, 2), u=u, cu=cu, cw=cw,
                                   w_i8=w_i8, K=K, logits=(K.astype(np.float64) / float(1 << shift)).astype(np.float32), shift=shift,
                                   pred=pred))


@functools.lru_cache(maxsize=None)
def ranking(name):
    """[B][min(16, V)] int64: per query the answers that come first in the order (-K, -v); cut to k by the caller"""
    K = tcase(name).K
    V = K.shape[1]
    order = np.argsort(-K[:, ::-1], axis=1, kind="stable")[:, :TOP]         # stable on -K over DESCENDING indices: (-K, -v)
    order = V - 1 - order
    order.setflags(write=False)
    return order


@functools.lru_cache(maxsize=None)
def _normaliser(name, base):
    lg = tcase(name).logits.astype(np.float64)
    mx = lg.max(1)
    return mx, np.exp((lg - mx[:, None]) * _LOG_BASE[base]).sum(1)


def top_prob64(name, base, idx):
    """float64 softmax probabilities of the answers idx [B][k]; base 0: e^x, 1: 2^x"""
    mx, tot = _normaliser(name, base)
    lg = np.take_along_axis(tcase(name).logits.astype(np.float64), idx, axis=1)
    return np.exp((lg - mx[:, None]) * _LOG_BASE[base]) / tot[:, None]


def float_ranking(p32, k):
    """what a ranking of rounded float32 probabilities gives: larger probability first, equal probabilities: higher index first"""
    V = p32.shape[1]
    return (V - 1 - np.argsort(-p32[:, ::-1].astype(np.float64), axis=1, kind="stable")[:, :k])


def takes_two_kernel_form(c, base, two_pass_switch=False):
    """where qmann_answer_i8 takes the two-kernel form whatever `probs` is"""
    return base == 2 or c.V < 4 or two_pass_switch

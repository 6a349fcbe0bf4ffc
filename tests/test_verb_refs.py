"""The numpy restatements of tests/verb_refs.py against float64 arithmetic, the oracle's quantiser and the reference's own
float activations (tests/golden/ref_activation.npz).  They are the yardstick of the GPU tests of verbs that neither the
oracle's C nor the reference's CPU branches cover, so they are checked here, without a GPU."""
import numpy as np
import pytest

import verb_refs as vr

F32, F64 = np.float32, np.float64
# the bound the GPU tests assert for the float SIGMOID: four times the error measured on the device
SIGMOID_BOUND = 4.0 * vr.SIGMOID_REL_ERR_MEASURED


def quant_f64(x, iwl, frac):
    """the format in exact arithmetic: truncate x . 2^frac toward zero, saturate, scale back"""
    m = (1 << (iwl + frac)) - 1
    t = np.clip(np.trunc(np.asarray(x, F64) * (1 << frac)), -m, m)
    return (t / (1 << frac)).astype(F32)


@pytest.mark.parametrize("fmt", [(5, 2), (2, 5), (0, 7), (6, 1), (1, 0), (3, 9)])
def test_quant_is_the_oracles_and_exact_truncation(oracle, fmt):
    rng = np.random.default_rng(fmt[0] * 16 + fmt[1])
    x = rng.normal(0, 2.0 ** fmt[0], 400).astype(F32)
    x[:6] = [0.0, -1e-6, 2.0 ** fmt[0], -(2.0 ** fmt[0]), 2.0 ** fmt[0] - 2.0 ** -fmt[1], 1e9]
    np.testing.assert_array_equal(vr.quant(x, *fmt), oracle.quant(x, *fmt))
    np.testing.assert_array_equal(vr.quant(x, *fmt), quant_f64(x, *fmt))
    np.testing.assert_array_equal(vr.quant(x.astype(F64), *fmt), quant_f64(x, *fmt))
    np.testing.assert_array_equal(vr.quant(np.array([0.0, -0.0, 3.0, -1e-9], F32), 0, 0), [1, 1, 1, -1])


def test_float_activations_are_the_references(gold):
    a = gold("ref_activation.npz")
    np.testing.assert_array_equal(vr.activation_fwd(a["x"], "NULL"), a["null"])
    np.testing.assert_array_equal(vr.activation_fwd(a["x"], "RELU"), a["relu"])
    # the reference's CPU branch takes double exp(), the CUDA kernel and this restatement expf(): one ulp apart at most
    np.testing.assert_allclose(vr.activation_fwd(a["x"], "SIGMOID"), a["sigmoid"], rtol=3e-7)


def test_the_sigmoid_bound_is_what_was_measured():
    """four times the measured error, and small against the 1e-5 of the float stages"""
    assert 0.0 < SIGMOID_BOUND < 1e-5
    pts = vr.sigmoid_points()
    assert pts.size == 10000 and pts[0] == -20.0 and pts[-1] == 20.0
    ref = vr.sigmoid_f64(pts)
    err = np.abs(vr.activation_fwd(pts, "SIGMOID").astype(F64) - ref) / ref
    assert err.max() <= SIGMOID_BOUND, err.max()


@pytest.mark.parametrize("fmt", [None] + list(vr.FIXED_FORMATS))
@pytest.mark.parametrize("dim", vr.DIMS)
def test_activation_fwd_against_float64(dim, fmt):
    x = vr.act_inputs(dim, fmt)
    assert x.size == dim and (dim < 7 or (np.any(x == 0) and np.any(np.abs(x) > 2.0 ** (fmt[0] if fmt else 3))))
    fixed = fmt is not None
    q = (lambda v: quant_f64(v, *fmt)) if fixed else (lambda v: np.asarray(v, F32))
    np.testing.assert_array_equal(vr.activation_fwd(x, "NULL", fixed, fmt or (0, 0)), q(x))
    np.testing.assert_array_equal(vr.activation_fwd(x, "RELU", fixed, fmt or (0, 0)), q(np.maximum(x.astype(F64), 0.0)))
    got, s64 = vr.activation_fwd(x, "SIGMOID", fixed, fmt or (0, 0)), vr.sigmoid_f64(x)
    if not fixed:
        assert np.max(np.abs(got - s64) / s64) <= SIGMOID_BOUND
    else:
        # equal wherever the float64 sigmoid is farther than the bound from a step of the grid; at most 1 % may differ
        bad = got != quant_f64(s64, *fmt)
        assert np.all(vr.near_step(s64, fmt, SIGMOID_BOUND)[bad])
        assert bad.sum() <= vr.SIGMOID_EXCUSED_SHARE * dim


@pytest.mark.parametrize("fmt", [None] + list(vr.FIXED_FORMATS))
@pytest.mark.parametrize("dim", vr.DIMS)
def test_activation_bwd_against_float64(dim, fmt):
    out, g = vr.bwd_inputs(dim, fmt)
    assert dim < 7 or (np.any(out == 0) and np.any(out == 1))
    fixed = fmt is not None
    gf = (1, fmt[0] + fmt[1] - 1) if fixed else None
    q = (lambda v: quant_f64(v, *gf)) if fixed else (lambda v: np.asarray(v, F32))
    np.testing.assert_array_equal(vr.activation_bwd(out, g, "NULL", fixed, fmt or (0, 0)), q(g))
    np.testing.assert_array_equal(vr.activation_bwd(out, g, "RELU", fixed, fmt or (0, 0)), q(np.where(out > 0, g, 0.0)))
    got = vr.activation_bwd(out, g, "SIGMOID", fixed, fmt or (0, 0))
    exact = g.astype(F64) * out.astype(F64) * (1.0 - out.astype(F64))
    if not fixed:
        # two roundings: the float product and the result
        np.testing.assert_allclose(got, exact, rtol=2.0 ** -23, atol=0)
    else:
        bad = got != q(exact)
        assert np.all(vr.near_step(exact, gf, 2.0 ** -23)[bad]) and bad.sum() <= 0.01 * dim
    assert np.all(got[out == 0] == 0) and np.all(got[out == 1] == 0)


@pytest.mark.parametrize("dim", vr.DIMS)
def test_scale_verbs_against_float64(dim):
    rng = np.random.default_rng(dim)
    x, g, w = rng.normal(0, 3, dim).astype(F32), rng.normal(0, 1, dim).astype(F32), F32(-0.37)
    np.testing.assert_array_equal(vr.scale_fwd(x, w), (x.astype(F64) * F64(w)).astype(F32))
    w_del, gout = vr.scale_bwd(x, g, w)
    np.testing.assert_array_equal(gout, (g.astype(F64) * F64(w)).astype(F32))
    t = g.astype(F64) * x.astype(F64)
    assert abs(F64(w_del) - t.sum()) <= (dim + 1) * 2.0 ** -24 * np.abs(t).sum()         # a serial float sum of dim terms
    if dim == 7:
        s = F32(0)
        for k in range(dim):
            s = F32(s + F32(g[k] * x[k]))
        assert w_del == s                                                              # index order, starting from 0
    w1, d1 = vr.scale_w_up(w, w_del, dim, 32, 0.3, 0.01)
    want = F64(w) + 0.3 / (32 * dim) * F64(w_del) + 0.3 * 0.01 * F64(w)
    assert d1 == 0 and abs(F64(w1) - want) <= 4 * 2.0 ** -24 * (abs(want) + abs(F64(w_del)))
    # the verb clears the gradient (lib/layer_cuda.cu:4902): a second update without a backward pass only decays
    w2, d2 = vr.scale_w_up(w1, d1, dim, 32, 0.3, 0.01)
    assert d2 == 0 and w2 == F32(w1 + F32(F32(F32(0.3) * F32(0.01)) * w1))


@pytest.mark.parametrize("shape", [(1,), (257,), (1, 1), (7, 13), (50, 60)])
def test_mult_e_against_float64(shape):
    rng = np.random.default_rng(len(shape) * 1000 + shape[0])
    a, b, g = (rng.normal(0, 2, shape).astype(F32) for _ in range(3))
    np.testing.assert_array_equal(vr.mult_e_fwd(a, b), (a.astype(F64) * b).astype(F32))
    ga, gb = vr.mult_e_bwd(a, b, g)
    np.testing.assert_array_equal(ga, (g.astype(F64) * b).astype(F32))
    np.testing.assert_array_equal(gb, (g.astype(F64) * a).astype(F32))

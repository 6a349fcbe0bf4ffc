"""qmann_answer_i8 (csrc/answer_i8.h: k_answer_i8_part + k_answer_i8_combine, the one-pass form; k_logits_mfma_i8 +
k_answer<true>, the two-kernel form) against the exact integer reference of answer_i8_cases.py, case by case: every byte format
pair, every width class and the scalar-load branch, dictionaries from 1 answer to 13 slices, the batch edges of the 16-query
tile and the 64-query workgroup, the second trips of the three grid-stride loops, u off the grid and beyond its range, labels
outside the dictionary, every refusal.  No query is excused anywhere.

Workspace discipline (every call here): logits_ws is a view of the first B . V floats behind a 256-byte prefix of ONE tensor
whose tail is 16 . B + 256 bytes -- more than the one-pass form's records of a V < 4 dictionary would overrun the documented
[n_query][V] floats by -- and prefix and tail must hold their fill afterwards.  The test touches no memory it does not own."""
import ctypes as C

import numpy as np
import pytest

from answer_i8_cases import (CASES, I8_CASES, OUTSIDE, case, cost64, highest_argmax, oracle_probs, prob64, probs64)
from conftest import load_pkg

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
PREFIX = 64                         # floats in front of the workspace (256 bytes: the workspace keeps the tensor's alignment)


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    load_pkg()
    import qmann_amd.abi as abi
    import qmann_amd.model as model

    class Env:
        pass
    e = Env()
    e.torch, e.model, e.abi, e.dev = torch, model, abi, torch.device("cuda:0")
    return e


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def make_net(env, c, base, with_weights=False):
    """a QNet whose last activation format is the case's; the float matrix only where the serial float layer is asked"""
    fmt = [tuple(c.fu)] * 3
    cfg = dict(n_hop=3, dim_emb=c.D, dim_input=c.V, attention_mode=2, softmax_variant=base, f_fixed=True, en_lin_map=False,
               fmt=fmt, fmt_w=list(fmt), fmt_att=list(fmt), fmt_bin=fmt[0])
    return env.model.QNet(cfg, {"w_ans": c.w_float if with_weights else np.zeros((1, 1), np.float32)}, device="cuda:0")


class Call:
    """one qmann_answer_i8 call on sentinel-filled outputs; results on the host, the guards checked"""

    def __init__(self, env, c, net, u, w_i8, labels=None, want_probs=False):
        torch = env.torch
        B, V = c.B, c.V
        tail = (16 * B + 256) // 4
        buf = torch.full((PREFIX + B * V + tail,), FILL, dtype=torch.int32, device=env.dev)
        ws = buf[PREFIX:PREFIX + B * V]
        assert ws.data_ptr() % 8 == 0
        pred = torch.full((B + 2,), FILL, dtype=torch.int32, device=env.dev)
        probs = torch.full((B * V + 2,), FILL, dtype=torch.int32, device=env.dev) if want_probs else None
        acc = torch.zeros(4, dtype=torch.int32, device=env.dev)                  # cost, match, two guards
        acc[2:] = FILL
        rc = env.abi.lib.qmann_answer_i8(C.byref(net.net), _p(w_i8), env.abi.Fmt(*c.fw), _p(u), _p(ws), _p(labels),
                                         _p(pred[1:]), _p(probs[1:]) if want_probs else None,
                                         _p(acc[:1]) if labels is not None else None, _p(acc[1:2]) if labels is not None else None,
                                         B, None)
        assert rc == env.abi.QMANN_OK, rc
        torch.cuda.synchronize()
        assert bool((buf[:PREFIX] == FILL).all()), "the workspace prefix was written"
        over = torch.nonzero(buf[PREFIX + B * V:] != FILL)
        assert over.numel() == 0, f"{over.numel()} words written past the [n_query][V] workspace, first at +{int(over[0])}"
        assert int(pred[0]) == FILL and int(pred[-1]) == FILL and bool((acc[2:] == FILL).all())
        self.pred = pred[1:-1].cpu().numpy().astype(np.int64)
        assert (self.pred != FILL).all(), "a prediction was not written"
        self.ws = ws.cpu().numpy().view(np.float32).reshape(B, V)
        if want_probs:
            assert int(probs[0]) == FILL and int(probs[-1]) == FILL
            self.probs = probs[1:-1].cpu().numpy().view(np.float32).reshape(B, V)
        self.cost = float(acc[:1].view(torch.float32).item())
        self.match = int(acc[1].item())


def device_inputs(env, c, u=None):
    torch = env.torch
    du = torch.from_numpy(np.array(c.u if u is None else u)).to(env.dev)
    dw = torch.from_numpy(np.array(c.w_i8)).to(env.dev)
    dl = torch.from_numpy(np.array(c.labels).view(np.int32)).to(env.dev)
    return du, dw, dl


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def reference_probs(oracle, name, base):
    """two-kernel form: float64 softmax at the e^x base, the oracle's softmax of the variant (float total in index order) at 2^x
    and exp_plan"""
    return probs64(name, 0) if base == 0 else oracle_probs(oracle, case(name).logits, base)


def takes_one_pass(c, base):
    return base != 2 and c.V >= 4


def cost_tolerance(B):
    """the softmax tolerance plus one rounding of the running float total per atomic add"""
    return dict(rel=1e-5 + B * 2.0 ** -24, abs=1e-6)


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", I8_CASES)
def test_two_kernel_form(env, oracle, name):
    """want_probs: logits bit-equal to the reference, pred and match equal, probabilities within rtol 1e-5 / atol 1e-7 of the
    reference softmax"""
    c = case(name)
    du, dw, dl = device_inputs(env, c)
    for base in c.bases:
        net = make_net(env, c, base)
        r = Call(env, c, net, du, dw, labels=dl, want_probs=True)
        assert same_bits(r.ws, c.logits), f"base {base}: logits"
        assert np.array_equal(r.pred, c.pred), f"base {base}: {(r.pred != c.pred).sum()} predictions differ"
        assert r.match == c.match
        np.testing.assert_allclose(r.probs, reference_probs(oracle, name, base), rtol=1e-5, atol=1e-7, err_msg=f"base {base}")


@pytest.mark.parametrize("name", I8_CASES)
def test_two_kernel_form_equals_the_serial_float_layer(env, name):
    """The header's contract: with want_probs the probabilities are those of qmann_answer_f32_serial on the dequantised matrix and
    the on-grid u, bit for bit (pred and match too).

    This holds at every magnitude only because k_answer<true> adds its double normaliser up in the order of the k_answer_small
    build that serves the shape in the float layer.  With its own strided order two cases missed, at the e^x base, in
    probabilities below 2^-126, by one step of 2^-149: dict_63 (1 of 4 032 entries) and k_answer_second_trip (4 of 534 885, all in
    query 4 046).  There two tied answers carry the total: 2 exactly in one order, 2 + 2^-51 in the other, and e / 2 of an odd
    denormal e is an exact rounding midpoint of the conversion to float."""
    c = case(name)
    du, dw, dl = device_inputs(env, c)
    du_grid = env.torch.from_numpy(np.array(c.u_grid)).to(env.dev)
    for base in c.bases:
        net = make_net(env, c, base, with_weights=True)
        r = Call(env, c, net, du, dw, labels=dl, want_probs=True)
        pred_f, probs_f, _, match_f = net.answer(du_grid, answer=dl, want_probs=True, serial=True)
        env.torch.cuda.synchronize()
        probs_f = probs_f.cpu().numpy()
        assert np.array_equal(pred_f.cpu().numpy(), r.pred) and int(match_f.item()) == r.match
        bad = np.argwhere(r.probs.view(np.uint32) != probs_f.view(np.uint32))
        assert len(bad) == 0, (f"base {base}: {len(bad)} of {probs_f.size} probabilities differ from the serial float layer, first "
                               f"[{bad[0][0]}][{bad[0][1]}]: {r.probs[tuple(bad[0])]!r} against {probs_f[tuple(bad[0])]!r}")


@pytest.mark.parametrize("name", I8_CASES)
def test_one_pass_form(env, oracle, name):
    """probs == NULL: pred and match equal the reference with and without labels; the batch's cost against the float64 softmax
    within 1e-5 + B . 2^-24 relative, 1e-6 absolute.  Where the library must take the two-kernel form instead -- exp_plan, and
    dictionaries of fewer than 4 answers, whose workspace is smaller than a record -- the workspace holds the exact logits
    afterwards and the cost is the two-kernel form's."""
    c = case(name)
    du, dw, dl = device_inputs(env, c)
    for base in c.bases:
        net = make_net(env, c, base)
        r = Call(env, c, net, du, dw, labels=dl)
        n = Call(env, c, net, du, dw)
        assert np.array_equal(r.pred, c.pred), f"base {base}: {(r.pred != c.pred).sum()} predictions differ"
        assert np.array_equal(n.pred, c.pred), f"base {base}, no labels: {(n.pred != c.pred).sum()} predictions differ"
        assert r.match == c.match and n.match == 0 and n.cost == 0.0
        if takes_one_pass(c, base):
            want = cost64(name, base)
            assert not same_bits(r.ws, c.logits)                           # (records, not logits)
        else:
            assert same_bits(r.ws, c.logits) and same_bits(n.ws, c.logits), f"base {base}: not routed to the two-kernel form"
            p = reference_probs(oracle, name, base)
            q = np.flatnonzero(c.inside)
            want = -float(p[q, c.labels[q].astype(np.int64)].astype(np.float64).sum())
        print(f"{name} base {base}: cost {r.cost!r}, reference {want!r}")
        assert r.cost == pytest.approx(want, **cost_tolerance(c.B)), f"base {base}"


def probe_pairs(c):
    """8 (query, answer) pairs: queries first and last of the batch and of a 64-query block, answers the prediction, 0, V - 1
    and a column of the ragged last tile"""
    qs = [q for q in dict.fromkeys([0, c.B - 1, 63, 64, c.B // 2, (c.B - 1) // 64 * 64]) if 0 <= q < c.B][:4]
    out = []
    for i in range(8):
        q = qs[i % len(qs)]
        ys = [int(c.pred[q]), 0, c.V - 1, (c.V - 1) // 64 * 64 + ((c.V - 1) % 64) // 2]
        out.append((q, ys[(i + i // len(qs)) % 4]))
    return out


ONE_PASS_ERRORS = {}


@pytest.mark.parametrize("name", [n for n in I8_CASES if CASES[n]["V"] >= 4])
def test_one_pass_probability_per_query(env, name):
    """Every label 0xFFFFFFFF but one: the cost after the call is -p[q][y] of the one-pass form itself.  Against the float64
    softmax at rtol 1e-5 / atol 1e-7, the header's promise, 8 pairs per case and base.

    Measured on an MI355X, largest relative error per format pair (u x w; the absolute error in brackets where it is above 1e-12):
      Q0.7 x Q0.7 5.8e-8 (2.8e-8), x Q1.6 1.0e-7 (1.3e-8), x Q4.3 5.2e-8, x Q7.0 0
      Q1.6 x Q0.7 4.6e-8 (2.1e-8), x Q1.6 6.9e-8 (4.5e-9), x Q4.3 6.6e-8, x Q7.0 0
      Q2.5 x Q0.7 7.4e-8 (8.9e-11), x Q1.6 6.4e-8 (6.9e-10), x Q4.3 0, x Q7.0 0        Q2.2 x Q1.2 3.9e-8
      Q3.4 x Q0.7 6.8e-8 (2.2e-11), x Q1.6 5.0e-8, x Q4.3 0, x Q7.0 0
      Q4.3 x Q0.7 5.1e-8, x Q1.6 3.6e-8, x Q4.3 0, x Q7.0 0
      Q5.2 x Q0.7 6.9e-8, x Q1.6 1.3e-7 (2.3e-8; 39 cases), x Q4.3 0, x Q7.0 0
      Q6.1 x Q0.7 9.6e-8, x Q1.6 5.6e-8, x Q4.3 0, x Q7.0 0
      Q7.0 x Q0.7 3.2e-8, x Q1.6 0, x Q4.3 0, x Q7.0 0
    (0: the probed probabilities are 0, 1/2 or 1 there -- logits of magnitude 10^3 and more -- and come out exactly.)"""
    c = case(name)
    du, dw, _ = device_inputs(env, c)
    worst_rel = worst_abs = 0.0
    for base in (0, 1):
        net = make_net(env, c, base)
        for q, y in probe_pairs(c):
            lab = np.full(c.B, OUTSIDE, np.uint32)
            lab[q] = y
            r = Call(env, c, net, du, dw, labels=env.torch.from_numpy(lab.view(np.int32)).to(env.dev))
            got, want = -r.cost, float(prob64(name, base, q, y))
            err = abs(got - want)
            worst_abs = max(worst_abs, err)
            if want > 1e-30:
                worst_rel = max(worst_rel, err / want)
            assert r.match == int(c.pred[q] == y)
            assert err <= 1e-7 + 1e-5 * want, f"base {base}, query {q}, answer {y}: {got!r} against {want!r} (max |logit| {c.max_abs_logit[q]})"
    key = (c.fu, c.fw)
    old = ONE_PASS_ERRORS.get(key, (0.0, 0.0))
    ONE_PASS_ERRORS[key] = (max(old[0], worst_rel), max(old[1], worst_abs))
    print(f"one-pass p[q][y], u Q{c.fu[0]}.{c.fu[1]} w Q{c.fw[0]}.{c.fw[1]} {name}: largest relative error {worst_rel:.3e}, absolute {worst_abs:.3e}"
          f"; the pair so far: {ONE_PASS_ERRORS[key][0]:.3e}, {ONE_PASS_ERRORS[key][1]:.3e}")


@pytest.mark.parametrize("name", [n for n in I8_CASES if CASES[n]["family"] == "offgrid"])
def test_off_grid_and_saturating_u(env, name):
    """the kernels quantise u with qm_code (truncation toward zero, symmetric saturation): both forms give for u exactly what they
    give for dequantise(qm_code(u)), and what the reference gives (test_two_kernel_form / test_one_pass_form on the same case)"""
    c = case(name)
    du, dw, dl = device_inputs(env, c)
    dg, _, _ = device_inputs(env, c, u=c.u_grid)
    for base in (0, 1):
        net = make_net(env, c, base)
        a, b = Call(env, c, net, du, dw, labels=dl, want_probs=True), Call(env, c, net, dg, dw, labels=dl, want_probs=True)
        assert same_bits(a.ws, b.ws) and same_bits(a.ws, c.logits)
        assert same_bits(a.probs, b.probs) and np.array_equal(a.pred, b.pred) and a.match == b.match == c.match
        a, b = Call(env, c, net, du, dw, labels=dl), Call(env, c, net, dg, dw, labels=dl)
        assert np.array_equal(a.pred, b.pred) and np.array_equal(a.pred, c.pred) and a.match == b.match == c.match
        assert a.cost == pytest.approx(b.cost, **cost_tolerance(c.B))          # (atomic adds in any order)
        for q, y in probe_pairs(c):                                            # one term: no order to differ by
            lab = np.full(c.B, OUTSIDE, np.uint32)
            lab[q] = y
            dlab = env.torch.from_numpy(lab.view(np.int32)).to(env.dev)
            assert Call(env, c, net, du, dw, labels=dlab).cost == Call(env, c, net, dg, dw, labels=dlab).cost


@pytest.mark.parametrize("name", ["dict_4033", "one_slice_two_tiles"])
def test_two_pass_switch(env, monkeypatch, name):
    """QMANN_ANSWER_TWO_PASS: pred and match equal both ways (and equal to the reference)"""
    c = case(name)
    du, dw, dl = device_inputs(env, c)
    net = make_net(env, c, 0)
    out = []
    for on in (False, True):
        monkeypatch.delenv("QMANN_ANSWER_TWO_PASS", raising=False)
        if on:
            monkeypatch.setenv("QMANN_ANSWER_TWO_PASS", "1")
        env.abi.lib.qmann_tuning_reload()
        out.append(Call(env, c, net, du, dw, labels=dl))
    one, two = out
    assert np.array_equal(one.pred, two.pred) and np.array_equal(one.pred, c.pred)
    assert one.match == two.match == c.match
    assert same_bits(two.ws, c.logits) and not same_bits(one.ws, c.logits)


@pytest.mark.parametrize("base", [0, 1, 2])
def test_float_layer_second_trip_of_the_workgroup_loop(env, oracle, base):
    """k_answer<false> (V > 256: one workgroup per query, the grid capped at 8 192) at 8 229 queries, through
    qmann_answer_f32_serial, with the criteria of test_gpu_batch.py::test_answer_layer_vs_oracle: probabilities within rtol 1e-5 /
    atol 1e-7 of the reference softmax, the arg-max the reference's rule on OUR probabilities, match and cost to follow.  (The
    operands lie on byte grids, so the serial float logits are exact and the reference is the integer one.)
    Labels: inside the dictionary for the 37 queries of the second trip and the first 19, 0xFFFFFFFF for the rest, so that the cost
    is a sum of 56 terms as it is of 37 there -- rel 1e-5 cannot hold for 8 229 atomic float additions in any order."""
    name = "k_answer_float_second_trip"
    c = case(name)
    net = make_net(env, c, base, with_weights=True)
    du, _, _ = device_inputs(env, c)
    q = np.arange(c.B)
    counted = (q < 19) | (q >= 8192)
    lab = np.where(counted, np.where(c.inside, c.labels, 0), OUTSIDE).astype(np.uint32)
    lab[8200] = int(c.pred[8200])                                             # (a match in the second trip)
    pred, probs, cost, match = net.answer(du, env.torch.from_numpy(lab.view(np.int32)).to(env.dev), want_probs=True, serial=True)
    env.torch.cuda.synchronize()
    pred, probs = pred.cpu().numpy(), probs.cpu().numpy()
    np.testing.assert_allclose(probs, reference_probs(oracle, name, base), rtol=1e-5, atol=1e-7)
    assert np.array_equal(pred, highest_argmax(probs))
    assert np.array_equal(pred, c.pred)
    assert (pred[c.zero_rows] == c.V - 1).all()
    qs = np.flatnonzero(counted)
    assert int(match.item()) == int((pred[qs] == lab[qs]).sum()) >= 1
    want_cost = -float(probs[qs, lab[qs].astype(np.int64)].astype(np.float64).sum())
    assert float(cost.item()) == pytest.approx(want_cost, rel=1e-5)


def test_refusals_launch_nothing(env):
    """every return code the header lists: sentinel-filled outputs unchanged after a synchronize, then a valid call writes them"""
    torch, abi = env.torch, env.abi
    c = case("fmt_u2.5_w1.6")
    B, V = c.B, c.V
    du, dw, dl = device_inputs(env, c)
    net = make_net(env, c, 0)
    ws = torch.full((B * V,), FILL, dtype=torch.int32, device=env.dev)
    pred = torch.full((B,), FILL, dtype=torch.int32, device=env.dev)
    probs = torch.full((B * V,), FILL, dtype=torch.int32, device=env.dev)
    acc = torch.full((2,), FILL, dtype=torch.int32, device=env.dev)

    def net_with(**fields):
        n = abi.Net.from_buffer_copy(net.net)
        for k, v in fields.items():
            if k == "act":
                n.act[n.n_hop - 1] = abi.Fmt(*v)
            else:
                setattr(n, k, v)
        return n

    def call(n=None, net_null=False, w=dw, w_fmt=c.fw, u=du, wsp=ws, pr=pred, pb=probs, nq=B):
        n = n if n is not None else net.net
        return abi.lib.qmann_answer_i8(None if net_null else C.byref(n), _p(w), abi.Fmt(*w_fmt), _p(u), _p(wsp), _p(dl), _p(pr),
                                       _p(pb), _p(acc[:1]), _p(acc[1:]), nq, None)

    assert call(net_null=True) == abi.QMANN_EINVAL
    assert call(w=None) == abi.QMANN_EINVAL and call(u=None) == abi.QMANN_EINVAL
    assert call(wsp=None) == abi.QMANN_EINVAL and call(pr=None) == abi.QMANN_EINVAL
    assert call(net_with(dim_emb=0)) == abi.QMANN_EINVAL and call(net_with(dim_input=0)) == abi.QMANN_EINVAL
    assert call(net_with(dim_emb_pad=96)) == abi.QMANN_EINVAL                 # no multiple of 64
    assert call(net_with(dim_emb=70)) == abi.QMANN_EINVAL                     # beyond dim_emb_pad = 64
    assert call(net_with(act=(8, 0))) == abi.QMANN_ERANGE and call(net_with(act=(0, 0))) == abi.QMANN_ERANGE
    assert call(w_fmt=(1, 7)) == abi.QMANN_ERANGE and call(w_fmt=(0, 0)) == abi.QMANN_ERANGE
    assert call(net_with(dim_input=40000)) == abi.QMANN_ERANGE                # a query's LDS beyond 128 KiB
    assert call(nq=1 << 24) == abi.QMANN_ERANGE
    assert call(nq=0) == abi.QMANN_OK
    assert call(net_with(dim_emb_pad=192)) == abi.QMANN_EUNSUPPORTED          # two-kernel form
    assert call(net_with(dim_emb_pad=192), pb=None) == abi.QMANN_EUNSUPPORTED  # one-pass form
    torch.cuda.synchronize()
    for t in (ws, pred, probs, acc):
        assert bool((t == FILL).all())
    acc.zero_()
    assert call() == abi.QMANN_OK
    torch.cuda.synchronize()
    assert np.array_equal(pred.cpu().numpy(), c.pred) and int(acc[1].item()) == c.match
    assert same_bits(ws.cpu().numpy().view(np.float32).reshape(B, V), c.logits) and not bool((probs == FILL).any())

"""qmann_answer_topk_i8 (csrc/batch_answer_i8.hip: the ranked builds of k_answer_i8_part and k_answer<true>, k_answer_i8_combine_topk)
against the integer reference of answer_topk_i8_cases.py.

top_idx is compared exactly at every softmax base a case lists; nothing is excused.  top_p: in the one-pass form (bases 0 and 1)
every entry against the float64 softmax of the exact logits with |got - want| <= 1e-7 + 1e-5 . want; in the two-kernel form
(exp_plan, QMANN_ANSWER_TWO_PASS, dictionaries of fewer than 4 answers) by bit pattern against qmann_answer_i8's probs gathered
at top_idx.  Every call here gets a workspace of exactly the helper's size in front of a canary region that must stay intact."""
import ctypes as C

import numpy as np
import pytest

from answer_topk_i8_cases import GPU_CASES, KS, ranking, takes_two_kernel_form, tcase, top_prob64
from conftest import load_pkg

pytestmark = pytest.mark.gpu

FILL = 0x5A5A5A5A
CANARY = 1024                                  # bytes behind the workspace


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


def make_net(env, c, base):
    fmt = [tuple(c.fu)] * 3
    cfg = dict(n_hop=3, dim_emb=c.D, dim_input=c.V, attention_mode=2, softmax_variant=base, f_fixed=True, en_lin_map=False,
               fmt=fmt, fmt_w=list(fmt), fmt_att=list(fmt), fmt_bin=fmt[0])
    return env.model.QNet(cfg, {"w_ans": np.zeros((1, 1), np.float32)}, device="cuda:0")


def device_inputs(env, c):
    torch = env.torch
    return torch.from_numpy(np.array(c.u)).to(env.dev), torch.from_numpy(np.array(c.w_i8)).to(env.dev)


def topk(env, c, net, du, dw, k, stream=None, out=None):
    """one call on sentinel-filled outputs with a workspace of exactly the helper's size; (top_idx int64, top_p float32) on the
    host, the guards and the canary checked"""
    torch = env.torch
    B = c.B
    need = int(env.abi.lib.qmann_answer_topk_i8_ws_bytes(C.byref(net.net), k, B))
    assert need > 0 and need % 8 == 0
    buf = torch.full(((need + CANARY) // 4,), FILL, dtype=torch.int32, device=env.dev)
    idx = torch.full((B * k + 2,), FILL, dtype=torch.int32, device=env.dev)
    tp = torch.full((B * k + 2,), FILL, dtype=torch.int32, device=env.dev)
    rc = env.abi.lib.qmann_answer_topk_i8(C.byref(net.net), _p(dw), env.abi.Fmt(*c.fw), _p(du), _p(buf), need, k, _p(idx[1:]),
                                          _p(tp[1:]), B, None)
    assert rc == env.abi.QMANN_OK, rc
    torch.cuda.synchronize()
    over = torch.nonzero(buf[need // 4:] != FILL)
    assert over.numel() == 0, f"{over.numel()} words written past the workspace of {need} bytes, first at +{int(over[0]) * 4}"
    for t in (idx, tp):
        assert int(t[0]) == FILL and int(t[-1]) == FILL
    return (idx[1:-1].cpu().numpy().astype(np.int64).reshape(B, k), tp[1:-1].cpu().numpy().view(np.float32).reshape(B, k))


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def check_case(env, name, bases=None, two_pass_switch=False):
    c = tcase(name)
    du, dw = device_inputs(env, c)
    ref = ranking(name)
    for base in (c.bases if bases is None else bases):
        net = make_net(env, c, base)
        two = takes_two_kernel_form(c, base, two_pass_switch)
        pred, probs, _, _, _ = net.answer_i8(du, dw, c.fw, want_probs=two)
        env.torch.cuda.synchronize()
        pred = pred.cpu().numpy().astype(np.int64)
        assert np.array_equal(pred, c.pred)
        probs = probs.cpu().numpy() if two else None
        for k in sorted({min(k, c.V) for k in KS}):
            top_idx, top_p = topk(env, c, net, du, dw, k)
            want = ref[:, :k]
            bad = np.flatnonzero((top_idx != want).any(1))
            assert len(bad) == 0, (f"{name} base {base} k {k}: {len(bad)} of {c.B} rows differ, first query {bad[0]}: "
                                   f"{top_idx[bad[0]].tolist()} against {want[bad[0]].tolist()}")
            assert np.array_equal(top_idx[:, 0], pred)
            if two:
                assert same_bits(top_p, np.take_along_axis(probs, top_idx, axis=1)), f"{name} base {base} k {k}: two-kernel probabilities"
            else:
                wp = top_prob64(name, base, want)
                err = np.abs(top_p.astype(np.float64) - wp)
                worst = np.unravel_index(np.argmax(err - 1e-5 * wp), err.shape)
                print(f"{name} base {base} k {k}: largest |got - want| {err.max():.3e}, largest relative "
                      f"{(err / np.maximum(wp, 1e-300))[wp > 1e-30].max(initial=0.0):.3e}")
                assert (err <= 1e-7 + 1e-5 * wp).all(), (f"{name} base {base} k {k}: query {worst[0]} pick {worst[1]}: "
                                                         f"{top_p[worst]!r} against {wp[worst]!r}")


@pytest.mark.parametrize("name", GPU_CASES)
def test_ranked_answers(env, name):
    """indices exact, probabilities by the form's criterion, the first entry qmann_answer_i8's pred; k 1, 2, 5, 16 cut to V"""
    check_case(env, name)


@pytest.mark.parametrize("name", ["dict_4033", "one_slice_two_tiles"])
def test_two_pass_switch(env, monkeypatch, name):
    """QMANN_ANSWER_TWO_PASS: the two-kernel form at the e^x and 2^x bases -- the same indices, probabilities bit-equal to
    qmann_answer_i8's"""
    monkeypatch.setenv("QMANN_ANSWER_TWO_PASS", "1")
    env.abi.lib.qmann_tuning_reload()
    check_case(env, name, bases=(0, 1), two_pass_switch=True)


def test_a_workspace_one_byte_short_is_refused(env):
    torch, abi = env.torch, env.abi
    for name, k in (("dict_321", 5), ("dict_65", 16), ("dict_3", 2)):
        c = tcase(name)
        du, dw = device_inputs(env, c)
        net = make_net(env, c, 0)
        need = int(abi.lib.qmann_answer_topk_i8_ws_bytes(C.byref(net.net), k, c.B))
        ws = torch.full((need // 4 + 2,), FILL, dtype=torch.int32, device=env.dev)
        idx = torch.full((c.B, k), FILL, dtype=torch.int32, device=env.dev)
        tp = torch.full((c.B, k), FILL, dtype=torch.int32, device=env.dev)
        call = lambda n: abi.lib.qmann_answer_topk_i8(C.byref(net.net), _p(dw), abi.Fmt(*c.fw), _p(du), _p(ws), n, k, _p(idx), _p(tp),
                                                      c.B, None)
        assert call(need - 1) == abi.QMANN_EINVAL and call(0) == abi.QMANN_EINVAL
        torch.cuda.synchronize()
        assert bool((ws == FILL).all()) and bool((idx == FILL).all()) and bool((tp == FILL).all())
        assert call(need) == abi.QMANN_OK
        torch.cuda.synchronize()
        assert np.array_equal(idx.cpu().numpy().astype(np.int64), ranking(name)[:, :k])


def test_python_layer(env):
    """QNet.answer_topk_i8 sizes its own workspace"""
    name, k = "dict_321", 5
    c = tcase(name)
    du, dw = device_inputs(env, c)
    top_idx, top_p = make_net(env, c, 0).answer_topk_i8(du, dw, c.fw, k)
    env.torch.cuda.synchronize()
    assert top_idx.dtype == env.torch.int32 and top_p.dtype == env.torch.float32 and tuple(top_idx.shape) == tuple(top_p.shape) == (c.B, k)
    assert np.array_equal(top_idx.cpu().numpy().astype(np.int64), ranking(name)[:, :k])


def test_graph_capture_and_replay(env):
    """dict_321, k 5: captured once on one stream, replayed twice; the outputs equal the eager call's"""
    torch, abi = env.torch, env.abi
    name, k = "dict_321", 5
    c = tcase(name)
    du, dw = device_inputs(env, c)
    net = make_net(env, c, 0)
    eager_idx, eager_p = topk(env, c, net, du, dw, k)
    need = int(abi.lib.qmann_answer_topk_i8_ws_bytes(C.byref(net.net), k, c.B))
    ws = torch.empty(need, dtype=torch.uint8, device=env.dev)
    idx = torch.full((c.B, k), FILL, dtype=torch.int32, device=env.dev)
    tp = torch.full((c.B, k), FILL, dtype=torch.int32, device=env.dev)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        rc = abi.lib.qmann_answer_topk_i8(C.byref(net.net), _p(dw), abi.Fmt(*c.fw), _p(du), _p(ws), need, k, _p(idx), _p(tp), c.B,
                                          C.c_void_p(s.cuda_stream))                # captured, not run
    assert rc == abi.QMANN_OK
    for _ in range(2):
        idx.fill_(FILL)
        tp.fill_(FILL)
        ws.zero_()
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(idx.cpu().numpy().astype(np.int64), eager_idx)
        assert same_bits(tp.cpu().numpy().view(np.float32), eager_p)

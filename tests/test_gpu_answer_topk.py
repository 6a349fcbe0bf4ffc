"""Ranked answers (qmann_answer_topk_f32, qmann_model_last_topk) against the serial-order answer layer.

The reference throughout is net.answer(u, want_probs=True, serial=True) on the same tensors -- qmann_answer_f32_serial's
probabilities -- ranked in numpy by (probability descending, index descending).  top_idx is compared exactly and top_p through
its bit patterns; nothing is excused."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_pkg

pytestmark = pytest.mark.gpu


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


def make_net(env, D, V, w_ans, frac=2):
    fmt = [(7 - frac, frac)] * 3
    cfg = dict(n_hop=3, dim_emb=D, dim_input=V, attention_mode=2, softmax_variant=0, f_fixed=True, en_lin_map=False,
               fmt=fmt, fmt_w=list(fmt), fmt_att=list(fmt), fmt_bin=fmt[0])
    return env.model.QNet(cfg, {"w_ans": w_ans}, device="cuda:0")


def grid_u(rng, B, D, sigma_u=20.0, frac=2):
    return (np.clip(np.rint(rng.normal(0, sigma_u, (B, D))), -127, 127) / (1 << frac)).astype(np.float32)   # on the activation grid


def serial(env, net, du):
    """(pred, probs) of qmann_answer_f32_serial"""
    pred, probs, _, _ = net.answer(du, want_probs=True, serial=True)
    env.torch.cuda.synchronize()
    return pred.cpu().numpy(), probs.cpu().numpy()


def ranked(probs, k):
    """the first k of every row in the order: larger probability first, equal probabilities: higher index first"""
    B, V = probs.shape
    idx = np.broadcast_to(np.arange(V), (B, V))
    order = np.lexsort((-idx, -probs.astype(np.float64)), axis=1)[:, :k]        # (last key is the primary one)
    return order.astype(np.int32), np.take_along_axis(probs, order, axis=1)


def check(env, net, du, probs, pred, k):
    top_idx, top_p = net.answer_topk(du, k)
    env.torch.cuda.synchronize()
    top_idx, top_p = top_idx.cpu().numpy(), top_p.cpu().numpy()
    want_idx, want_p = ranked(probs, k)
    assert top_idx.shape == top_p.shape == (probs.shape[0], k)
    assert np.array_equal(top_idx, want_idx)
    assert np.array_equal(top_p.view(np.uint32), want_p.view(np.uint32))
    assert np.array_equal(top_idx[:, 0], pred)
    return top_idx, top_p


# every serial dispatch branch: 16 lanes x {2, 4, 6, 8} logits (V <= 32, 64, 96, 128), 64 lanes x 4 (129 .. 256), one workgroup
# per query beyond (V > 256, or where the transposed matrix does not fit LDS: V 200 at D 256)
SHAPES = [(V, D) for V in (1, 2, 17, 33, 65, 97, 128, 129, 256, 257, 1000) for D in (17, 60)] + [(200, 256)]


@pytest.mark.parametrize("V,D", SHAPES)
def test_topk_equals_the_ranked_serial_probabilities(env, V, D):
    """B 1, 5, 67: ragged tails against 4, 8 and 16 queries per wavefront; k 1, 2, 5, 16 clipped to V; every softmax base.
    (One reference per (base, B), every k against it; the three bases share the net.)"""
    torch = env.torch
    rng = np.random.default_rng(V * 131 + D)
    net = make_net(env, D, V, rng.normal(0, 0.1, (V, D)).astype(np.float32))
    for base in (0, 1, 2):
        net.net.softmax_base = base
        for B in (1, 5, 67):
            du = torch.from_numpy(grid_u(rng, B, D)).to(env.dev)
            pred, probs = serial(env, net, du)
            for k in sorted({min(k, V) for k in (1, 2, 5, 16)}):
                check(env, net, du, probs, pred, k)


@pytest.mark.parametrize("V,D", [(33, 17), (97, 60), (200, 60), (200, 256), (1000, 60)])
def test_ties_go_to_the_higher_index(env, V, D):
    """every third row of w_ans equals the row before it: equal logits, equal probabilities, the higher index comes first;
    w_ans = 0: every probability equal, the ranking is V-1, V-2, ..."""
    torch = env.torch
    rng = np.random.default_rng(V + D)
    w = rng.normal(0, 0.1, (V, D)).astype(np.float32)
    w[2::3] = w[1:-1:3][:len(w[2::3])]
    B, k = 67, min(16, V)
    du = torch.from_numpy(grid_u(rng, B, D)).to(env.dev)
    for base in (0, 1, 2):
        net = make_net(env, D, V, w)
        net.net.softmax_base = base
        pred, probs = serial(env, net, du)
        assert np.array_equal(probs[:, 2::3], probs[:, 1:-1:3][:, :probs[:, 2::3].shape[1]])
        top_idx, top_p = check(env, net, du, probs, pred, k)
        pairs = 0
        for q in range(B):
            for j in range(k - 1):
                if top_idx[q, j] % 3 == 2:                       # the duplicate first, the row it copies right behind it
                    assert top_idx[q, j + 1] == top_idx[q, j] - 1 and top_p[q, j + 1] == top_p[q, j]
                    pairs += 1
        assert pairs > 0
        zero = make_net(env, D, V, np.zeros((V, D), np.float32))
        zero.net.softmax_base = base
        pred0, probs0 = serial(env, zero, du)
        top0, _ = check(env, zero, du, probs0, pred0, k)
        assert np.array_equal(top0, np.broadcast_to(V - 1 - np.arange(k), (B, k)))


@pytest.mark.parametrize("V", [80, 238, 1000])
@pytest.mark.parametrize("sigma_w,sigma_u", [(0.3, 40.0), (1.0, 60.0)])
def test_wide_spread_of_exponents_stays_bit_equal(env, V, sigma_w, sigma_u):
    """logits of magnitude 50 .. 300 (test_gpu_answer.py's large-logit case): many probabilities underflow to 0 and the terms of
    the normaliser span more than 29 binary orders, where a double total of floats depends on the order of the additions.
    Still bit-equal; the zeros are ranked by index; the first entry is the serial call's pred.
    (The e^x and 2^x bases, whose exponentials underflow; the piece-wise linear exp_plan base is left to the shape test above.)"""
    torch = env.torch
    D, B, k = 60, 67, 16
    rng = np.random.default_rng(9)
    net = make_net(env, D, V, rng.normal(0, sigma_w, (V, D)).astype(np.float32))
    du = torch.from_numpy(grid_u(rng, B, D, sigma_u=sigma_u)).to(env.dev)
    seen_zero = 0
    for base in (0, 1):
        net.net.softmax_base = base
        pred, probs = serial(env, net, du)
        pos = np.where(probs > 0, probs, np.inf).min(1)
        assert (pos * 2.0 ** 29 < probs.max(1)).mean() > 0.9        # the spread of the total's terms, row by row
        top_idx, top_p = check(env, net, du, probs, pred, k)
        for q in range(B):
            z = top_idx[q][top_p[q] == 0]
            if len(z):
                seen_zero += 1
                all_zero = np.flatnonzero(probs[q] == 0)[::-1]
                assert np.array_equal(z, all_zero[:len(z)])
    if (sigma_w, sigma_u) == (1.0, 60.0):
        assert seen_zero > 0                                        # (there the sixteenth logit lies > 104 below the best)


def test_refusals_launch_nothing(env):
    torch, abi = env.torch, env.abi
    D, B = 17, 5
    rng = np.random.default_rng(3)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
    for V in (5, 30):
        net = make_net(env, D, V, rng.normal(0, 0.1, (V, D)).astype(np.float32))
        du = torch.from_numpy(grid_u(rng, B, D)).to(env.dev)
        idx = torch.full((B, 16), 0x5A5A5A5A, dtype=torch.int32, device=env.dev)
        tp = torch.full((B, 16), -7.5, dtype=torch.float32, device=env.dev)

        def call(k, n=B, i=idx, t=tp, net_p=C.byref(net.net), w=net.w_ans, u=du):
            return abi.lib.qmann_answer_topk_f32(net_p, p(w), p(u), k, p(i), p(t), n, None)

        assert call(0) == abi.QMANN_EINVAL
        assert call(17) == abi.QMANN_EINVAL
        assert call(V + 1) == abi.QMANN_EINVAL
        assert call(1, i=None) == abi.QMANN_EINVAL and call(1, t=None) == abi.QMANN_EINVAL
        assert call(1, w=None) == abi.QMANN_EINVAL and call(1, u=None) == abi.QMANN_EINVAL and call(1, net_p=None) == abi.QMANN_EINVAL
        assert call(1, n=0) == abi.QMANN_OK and call(min(16, V), n=0) == abi.QMANN_OK
        assert call(1, n=1 << 24) == abi.QMANN_ERANGE                 # as qmann_answer_f32_serial answers it
        torch.cuda.synchronize()
        assert bool((idx == 0x5A5A5A5A).all()) and bool((tp == -7.5).all())
        assert call(min(16, V)) == abi.QMANN_OK                       # (and the same buffers are written by a valid call)
        torch.cuda.synchronize()
        assert bool((idx.view(-1)[:B * min(16, V)] < V).all())
    # a dictionary whose probabilities do not fit a workgroup's LDS: QMANN_ERANGE from the serial call and from this one
    V = 40000
    net = make_net(env, D, V, np.zeros((V, D), np.float32))
    du = torch.from_numpy(grid_u(rng, 1, D)).to(env.dev)
    idx = torch.full((1, 4), 0x5A5A5A5A, dtype=torch.int32, device=env.dev)
    tp = torch.full((1, 4), -7.5, dtype=torch.float32, device=env.dev)
    pred = torch.zeros(1, dtype=torch.int32, device=env.dev)
    assert abi.lib.qmann_answer_f32_serial(C.byref(net.net), p(net.w_ans), p(du), None, p(pred), None, None, None, 1, None) == abi.QMANN_ERANGE
    assert abi.lib.qmann_answer_topk_f32(C.byref(net.net), p(net.w_ans), p(du), 4, p(idx), p(tp), 1, None) == abi.QMANN_ERANGE
    torch.cuda.synchronize()
    assert bool((idx == 0x5A5A5A5A).all()) and bool((tp == -7.5).all())


# ---- the model call ----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def answer_exact(env, monkeypatch):
    """QMANN_ANSWER_EXACT: the forwards' own answer layer is the serial-order one, so their pred is the ranking's first entry always"""
    monkeypatch.setenv("QMANN_ANSWER_EXACT", "1")
    env.abi.lib.qmann_tuning_reload()
    yield
    monkeypatch.delenv("QMANN_ANSWER_EXACT", raising=False)
    env.abi.lib.qmann_tuning_reload()


def words(rng, rows, n_words, lo, hi, last=None):
    """uint16 word rows [rows][8]: n_words indices of [lo, hi), then `last[r]` (a story row's time index) where given"""
    out = np.full((rows, 8), 0xFFFF, np.uint16)
    out[:, :n_words] = rng.integers(lo, hi, (rows, n_words))
    if last is not None:
        out[:, n_words] = last
    return out


@pytest.mark.parametrize("mode,num_bit", [(2, 8), (11, 4)])
def test_model_last_topk_ranks_the_last_batch(env, answer_exact, mode, num_bit):
    """D 60, V 80, 3 hops: memorise 40 rows, ask 67 questions, rank 3; a smaller ask then ranks its 5 rows, not 67; the same after
    forward_words on 5 ragged stories.  Every ranking is that of the serial probabilities of last_u, its first entry the call's pred."""
    torch, model, abi = env.torch, env.model, env.abi
    D, V, H, k = 60, 80, 3, 3
    rng = np.random.default_rng(17 + mode)
    cfg = model.babi_cfg(V, attention_mode=mode, D=D, en_mq=False)
    cfg["num_bit"] = num_bit
    wts = {"w_q": rng.normal(0, 1.0, (D, V)).astype(np.float32),
           "w_a": [rng.normal(0, 1.0, (D, V)).astype(np.float32) for _ in range(H)],
           "w_c": [rng.normal(0, 1.0, (D, V)).astype(np.float32) for _ in range(H)],
           "w_h": [rng.normal(0, 1.0, (D, D)).astype(np.float32) for _ in range(H)],
           "w_ans": rng.normal(0, 0.1, (V, D)).astype(np.float32)}
    hm = model.HostModel(cfg, wts, device="cuda:0")
    net = model.QNet.from_model(cfg, hm)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(env.dev)
    p = lambda t: C.c_void_p(t.data_ptr())

    # before any batch: QMANN_EINVAL, nothing written
    idx = torch.full((67, k), 0x5A5A5A5A, dtype=torch.int32, device=env.dev)
    tp = torch.full((67, k), -7.5, dtype=torch.float32, device=env.dev)
    assert abi.lib.qmann_model_last_n_query(hm.h) == 0
    assert abi.lib.qmann_model_last_topk(hm.h, k, p(idx), p(tp), None) == abi.QMANN_EINVAL
    with pytest.raises(RuntimeError):
        hm.last_topk(k)
    torch.cuda.synchronize()
    assert bool((idx == 0x5A5A5A5A).all()) and bool((tp == -7.5).all())

    def same_as_serial(B, pred):
        top_idx, top_p = hm.last_topk(k)
        torch.cuda.synchronize()
        assert tuple(top_idx.shape) == tuple(top_p.shape) == (B, k) and abi.lib.qmann_model_last_n_query(hm.h) == B
        u = hm.last_u(B)
        assert float(u.abs().sum()) > 0
        _, probs = serial(env, net, u)
        want_idx, want_p = ranked(probs, k)
        assert np.array_equal(top_idx.cpu().numpy(), want_idx)
        assert np.array_equal(top_p.cpu().numpy().view(np.uint32), want_p.view(np.uint32))
        assert np.array_equal(top_idx[:, 0].cpu().numpy(), pred.cpu().numpy())

    story = words(rng, 40, 4, 1, 40, last=40 + np.arange(40))
    hm.memorize_words(up(story))
    pred, _, _ = hm.ask_words(up(words(rng, 67, 3, 1, 40)))
    same_as_serial(67, pred)

    # a second, smaller ask: 5 rows are ranked and written, not 67
    pred, _, _ = hm.ask_words(up(words(rng, 5, 3, 1, 40)))
    same_as_serial(5, pred)
    assert abi.lib.qmann_model_last_topk(hm.h, k, p(idx), p(tp), None) == abi.QMANN_OK
    torch.cuda.synchronize()
    assert bool((idx[:5] < V).all()) and bool((idx[5:] == 0x5A5A5A5A).all()) and bool((tp[5:] == -7.5).all())

    # forward_words on 5 ragged stories
    n_sen = np.array([1, 7, 3, 12, 2])
    off = np.concatenate([[0], np.cumsum(n_sen)])
    sw = words(rng, int(off[-1]), 4, 1, 40, last=np.concatenate([40 + np.arange(n) for n in n_sen]))
    pred, _, _ = hm.forward_words(up(sw), up(words(rng, 5, 3, 1, 40)), torch.from_numpy(off.astype(np.int32)).to(env.dev), int(n_sen.max()))
    same_as_serial(5, pred)

    # what the ranked call itself refuses comes back through the model call
    for bad in (0, 17, V + 1):
        assert abi.lib.qmann_model_last_topk(hm.h, bad, p(idx), p(tp), None) == abi.QMANN_EINVAL
    assert abi.lib.qmann_model_last_topk(hm.h, k, None, p(tp), None) == abi.QMANN_EINVAL
    hm.close()

"""Attended slots for float attention: qmann_hops_top_float_i8, qmann_hops_shared_top_float_i8 (csrc/batch_hops_top_float.hip,
csrc/hops_attended_float.h) and the model verbs qmann_model_forward_words_top_float / qmann_model_ask_words_top_float.

The yardstick is the `probs` tap of the EXISTING base call on the same inputs -- qmann_hops_i8 (mode 1) for the per-story call,
qmann_hops_shared_float_i8 for the shared call -- ordered by attended_cases.want_rows / attended_story_cases.want_story_rows.
Slots are compared exactly, top_p and u_out by bit pattern; nothing is excused.  u_out, top_slot and top_p of the hop calls sit
inside 4 KiB guards filled with 0xA5, compared with the payload: a row stored for a spare place of a short tile lands there.

1. every case of attended_float_cases.py through both calls, k = 1, 5, 16, the shared call under the launcher's tile and every
   forced tile that fits; 2. tied hops; 3. the model verbs; 4. the refusal order, outputs untouched; 5. the old verbs still
   refuse float attention; 6. the shared call captured in a graph and replayed.
"""
import ctypes as C

import numpy as np
import pytest

import attended_float_cases as af
import float_hops_cases as fc
import shared_float_cases as sf
from attended_cases import assert_rows, want_rows
from attended_float_cases import KS, SHARED, STORY, build
from attended_story_cases import assert_story_rows, want_story_rows
from conftest import load_pkg
from float_hops_cases import FILL, GUARD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    load_pkg()
    import qmann_amd.abi as abi
    import qmann_amd.model as model

    class Env:
        pass
    e = Env()
    e.torch, e.abi, e.model = torch, abi, model
    e.dev = torch.device("cuda:0")
    return e


@pytest.fixture
def force_qt(env, monkeypatch):
    """queries per workgroup forced through the tuning switch (conftest reloads the switches after the test)"""
    def _force(qt):
        if qt:
            monkeypatch.setenv("QMANN_SHARED_QT", str(qt))
        else:
            monkeypatch.delenv("QMANN_SHARED_QT", raising=False)
        env.abi.lib.qmann_tuning_reload()
    return _force


def _up(env, a):
    return env.torch.from_numpy(np.ascontiguousarray(a)).to(env.dev)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _guarded(env, n_bytes):
    return env.torch.full((n_bytes + 2 * GUARD,), FILL, dtype=env.torch.uint8, device=env.dev)


def _payload(raw, dtype, shape):
    a = raw.cpu().numpy()
    assert (a[:GUARD] == FILL).all() and (a[-GUARD:] == FILL).all(), "a store outside the output"
    return a[GUARD:-GUARD].view(dtype).reshape(shape)


class Run:
    """one case on the device: its planes, the two base calls with the `probs` tap, the two new calls"""

    def __init__(self, env, case, shared):
        self.env, self.case, self.shared = env, case, shared
        self.net = env.model.QNet(case.cfg, case.wts)
        self.H, self.D, self.B = case.cfg["n_hop"], case.cfg["dim_emb"], case.B
        self.dk, self.dv = _up(env, case.kb.view(np.int8)), _up(env, case.vb.view(np.int8))
        self.ro, self.u0 = _up(env, case.row_off.view(np.int32)), _up(env, case.u0)
        self.stride = 0 if case.tied else case.R * self.net.Dp
        if shared:
            mk, mv = sf.memory(case)
            self.mk, self.mv = _up(env, mk.view(np.int8)), _up(env, mv.view(np.int8))
            self.mstride = 0 if case.tied else case.max_slots * self.net.Dp

    def base_story(self):
        """(u_out [B][D], probs [H][rows]) of qmann_hops_i8 with taps"""
        u, taps = self.net.hops(self.dk, self.dv, self.ro, self.case.max_slots, self.u0, taps=True)
        self.env.torch.cuda.synchronize()
        return u.cpu().numpy(), taps.probs.cpu().numpy()

    def base_shared(self):
        """(u_out [B][D], probs [H][B][S]) of qmann_hops_shared_float_i8 with taps"""
        u, taps = self.net.hops_shared_float(self.mk, self.mv, self.case.max_slots, self.u0, taps=True)
        self.env.torch.cuda.synchronize()
        return u.cpu().numpy(), taps.probs.cpu().numpy()

    def top(self, k, shared):
        """the new call into guarded buffers: (u_out float32 [B][D], top_slot uint32 [B][H][k], top_p float32 [B][H][k])"""
        env, abi = self.env, self.env.abi
        B, H, D = self.B, self.H, self.D
        u, slot, tp = _guarded(env, B * D * 4), _guarded(env, B * H * k * 4), _guarded(env, B * H * k * 4)
        at = lambda t: C.c_void_p(t.data_ptr() + GUARD)
        if shared:
            rc = abi.lib.qmann_hops_shared_top_float_i8(C.byref(self.net.net), _p(self.mk), _p(self.mv), self.mstride, self.case.max_slots,
                                                        _p(self.u0), at(u), k, at(slot), at(tp), B, None)
        else:
            rc = abi.lib.qmann_hops_top_float_i8(C.byref(self.net.net), _p(self.dk), _p(self.dv), self.stride, _p(self.ro),
                                                 self.case.max_slots, _p(self.u0), at(u), k, at(slot), at(tp), B, None)
        assert rc == abi.QMANN_OK, f"{self.case.name}: returned {rc}"
        env.torch.cuda.synchronize()
        return _payload(u, np.float32, (B, D)), _payload(slot, np.uint32, (B, H, k)), _payload(tp, np.float32, (B, H, k))


def _same(got, want, what):
    g_u, g_slot, g_p = got
    w_u, w_slot, w_p = want
    np.testing.assert_array_equal(g_slot, w_slot, err_msg=f"{what}: top_slot")
    np.testing.assert_array_equal(g_p.view(np.uint32), w_p.view(np.uint32), err_msg=f"{what}: top_p bits")
    np.testing.assert_array_equal(g_u.view(np.uint32), w_u.view(np.uint32), err_msg=f"{what}: u_out bits")


def _tiles(env, case, force_qt):
    for qt in (None,) + sf.TILES:
        if qt and not sf.fits(case.max_slots, qt):
            continue
        force_qt(qt)
        ran = env.abi.lib.qmann_hops_shared_float_tile(case.max_slots, case.B)
        assert ran in sf.TILES and (not qt or ran == qt), "the switch took effect"
        yield f"tile {qt or 'chosen'}"


# ---- 1. every case, both calls ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n in SHARED if af.family(n) != "tied"))
def test_shared_cases_through_both_calls(env, force_qt, name):
    case = build(name)
    run = Run(env, case, True)
    force_qt(None)
    u_story, probs_story = run.base_story()
    u_shared, probs_shared = run.base_shared()
    assert np.array_equal(u_story.view(np.uint32), u_shared.view(np.uint32))
    if af.family(name) == "nan":
        assert np.isnan(probs_shared).any() and np.isposinf(probs_shared).any(), "the kernel reaches the NaN the reference shows"
    for k in KS:
        w_slot, w_p = want_story_rows(probs_story, case.row_off, case.max_slots, k)
        _same(run.top(k, False), (u_story, w_slot, w_p), f"{name} per story, k={k}")
    rows = {k: want_rows(probs_shared, k) for k in KS}
    for label in _tiles(env, case, force_qt):
        for k in KS:
            _same(run.top(k, True), (u_shared,) + rows[k], f"{name} shared, {label}, k={k}")


@pytest.mark.parametrize("name", sorted(n for n in STORY if af.family(n) != "tied"))
def test_story_cases(env, name):
    case = build(name)
    run = Run(env, case, False)
    u, probs = run.base_story()
    for k in KS:
        w_slot, w_p = want_story_rows(probs, case.row_off, case.max_slots, k)
        got = run.top(k, False)
        _same(got, (u, w_slot, w_p), f"{name}, k={k}")
        live = got[1][got[1] != 0xFFFFFFFF]
        assert live.size == 0 or int(live.max()) < case.max_slots, "a cut story lists no slot >= max_slots"
        for q in range(case.B):
            if case.slots(q)[1] == 0:
                assert (got[1][q] == 0xFFFFFFFF).all() and (got[2][q].view(np.uint32) == 0).all(), "an empty story is all padding"


# ---- 2. tied hops --------------------------------------------------------------------------------------------------------------------
def test_tied_hops_equal_the_call_on_copies_of_the_plane(env, force_qt):
    """hop_stride = 0: the base calls take no taps then, so the yardstick is the tap of the call on n_hop copies of the plane"""
    for name, shared in (("af_tied", True), ("afs_tied", False)):
        tied = build(name)
        three = fc.untied(tied)
        r1, r3 = Run(env, tied, shared), Run(env, three, shared)
        force_qt(None)
        u, probs = r3.base_story()
        for k in KS:
            w_slot, w_p = want_story_rows(probs, three.row_off, three.max_slots, k)
            _same(r1.top(k, False), (u, w_slot, w_p), f"{name} per story, k={k}")
        if shared:
            u_s, probs_s = r3.base_shared()
            for label in _tiles(env, tied, force_qt):
                for k in KS:
                    _same(r1.top(k, True), (u_s,) + want_rows(probs_s, k), f"{name} shared, {label}, k={k}")


# ---- 3. the model ----------------------------------------------------------------------------------------------------------------------
N_STORIES = 64


def _float_model(env):
    from test_gpu_attended_story import _qnet_of
    from test_gpu_shared import _model_inputs
    cfg, wts, sw, qw, n_sen, ans = _model_inputs("random_joint20", env)
    cfg = dict(cfg, attention_mode=1)
    hm = env.model.HostModel(cfg, wts, device="cuda:0")
    return cfg, wts, sw, qw, n_sen, ans, hm, _qnet_of(env, cfg, wts, hm)


def test_forward_words_top_float(env):
    torch, model = env.torch, env.model
    cfg, wts, sw, qw, n_sen, ans, hm, net = _float_model(env)
    n_sen = n_sen[:N_STORIES]
    row_off = np.concatenate([[0], np.cumsum(n_sen)]).astype(np.int32)
    R, K, MS = int(row_off[-1]), 5, int(n_sen.max())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(env.dev)
    d_sw, d_qw, d_ro = up(sw[:R]), up(qw[:N_STORIES]), torch.from_numpy(row_off).to(env.dev)
    d_ans = torch.from_numpy(ans[:N_STORIES].astype(np.int32)).to(env.dev)
    plain = model.HostModel(cfg, wts, device="cuda:0")
    pred2, cost2, match2 = plain.forward_words(d_sw, d_qw, d_ro, MS, d_ans)
    torch.cuda.synchronize()
    u2, rank2 = plain.last_u(N_STORIES), plain.last_topk(3)
    dk, dv, du0 = net.embed_idx(d_sw, d_qw)
    u_tap, taps = net.hops(dk, dv, d_ro, MS, du0, taps=True)
    torch.cuda.synchronize()
    pred, cost, match, slot, p = hm.forward_words_top_float(d_sw, d_qw, d_ro, MS, K, d_ans)
    torch.cuda.synchronize()
    assert_story_rows(slot, p, taps.probs.cpu().numpy(), row_off, MS, K, "forward_words_top_float")
    assert torch.equal(pred, pred2) and int(match.item()) == int(match2.item())
    assert torch.equal(hm.last_u(N_STORIES).view(torch.int32), u2.view(torch.int32)) and torch.equal(u2, u_tap)
    assert float(cost.item()) == pytest.approx(float(cost2.item()), rel=1e-4, abs=1e-3)      # float atomics: the order of the adds differs
    rank = hm.last_topk(3)
    torch.cuda.synchronize()
    assert torch.equal(rank[0], rank2[0]) and torch.equal(rank[1], rank2[1])
    assert float(u2.abs().sum()) > 0
    hm.close(); plain.close()


def test_ask_words_top_float(env):
    torch, model = env.torch, env.model
    cfg, wts, sw, qw, n_sen, ans, hm, net = _float_model(env)
    offs = np.concatenate([[0], np.cumsum(n_sen)])
    s = int(np.argmax(n_sen))
    N, K = 11, 5
    others = (s + 1 + np.arange(N)) % len(n_sen)
    story, q_sel, a_sel = sw[offs[s]:offs[s + 1]], qw[others], ans[others]
    R = story.shape[0]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(env.dev)
    d_story, d_q, d_ans = up(story), up(q_sel), torch.from_numpy(a_sel.astype(np.int32)).to(env.dev)
    hm.enable_float_asks()
    hm.memorize_words(d_story)
    plain = model.HostModel(cfg, wts, device="cuda:0")
    plain.enable_float_asks()
    plain.memorize_words(d_story)
    pred2, cost2, match2 = plain.ask_words(d_q, d_ans)
    torch.cuda.synchronize()
    u2, rank2 = plain.last_u(N), plain.last_topk(3)
    dk, dv, du0 = net.embed_idx(d_story, d_q)
    u_tap, taps = net.hops_shared_float(dk, dv, R, du0, taps=True)
    torch.cuda.synchronize()
    pred, cost, match, slot, p = hm.ask_words_top_float(d_q, K, d_ans)
    torch.cuda.synchronize()
    assert_rows(slot, p, taps.probs.cpu().numpy(), K, "ask_words_top_float")
    assert torch.equal(pred, pred2) and int(match.item()) == int(match2.item())
    assert torch.equal(hm.last_u(N).view(torch.int32), u2.view(torch.int32)) and torch.equal(u2, u_tap)
    assert float(cost.item()) == pytest.approx(float(cost2.item()), rel=1e-4, abs=1e-3)
    rank = hm.last_topk(3)
    torch.cuda.synchronize()
    assert torch.equal(rank[0], rank2[0]) and torch.equal(rank[1], rank2[1])
    hm.close(); plain.close()


def test_model_verbs_refuse_in_order_and_touch_nothing(env):
    torch, model, abi = env.torch, env.model, env.abi
    cfg, wts, sw, qw, n_sen, ans, hm, _ = _float_model(env)
    H, K, N = cfg["n_hop"], 2, 4
    offs = np.concatenate([[0], np.cumsum(n_sen)])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(env.dev)
    R = int(offs[N])
    d_sw, d_q = up(sw[:R]), up(qw[:N])
    d_ro = torch.from_numpy(offs[:N + 1].astype(np.int32)).to(env.dev)
    MS = int(n_sen[:N].max())
    pred = torch.full((N,), -7, dtype=torch.int32, device=env.dev)
    slot = torch.full((N, H, K), -7, dtype=torch.int32, device=env.dev)
    tp = torch.full((N, H, K), -7.0, dtype=torch.float32, device=env.dev)
    fwd, ask = abi.lib.qmann_model_forward_words_top_float, abi.lib.qmann_model_ask_words_top_float

    def forward(m, k=K, s=slot, t=tp, n=N, q=d_q):
        return fwd(m, _p(d_sw), R, d_sw.shape[1], _p(q), d_q.shape[1], _p(d_ro), MS, n, None, _p(pred), None, None, k, _p(s), _p(t), None)

    def asks(m, k=K, s=slot, t=tp, n=N, q=d_q):
        return ask(m, _p(q), d_q.shape[1], n, None, _p(pred), None, None, k, _p(s), _p(t), None)
    fx = model.HostModel(dict(cfg, attention_mode=2), wts, device="cuda:0")
    fx.memorize_words(d_sw)
    # the base verbs' answers first
    assert forward(None) == abi.QMANN_EINVAL and asks(None) == abi.QMANN_EINVAL
    assert forward(hm.h, k=0, n=0) == abi.QMANN_OK and forward(fx.h, k=0, n=0) == abi.QMANN_OK
    assert forward(hm.h, k=0, q=None) == abi.QMANN_EINVAL and forward(fx.h, q=None) == abi.QMANN_EINVAL
    assert asks(hm.h) == abi.QMANN_EINVAL, "nothing memorised: float asks are off"
    hm.enable_float_asks()
    assert asks(hm.h) == abi.QMANN_EINVAL, "nothing memorised yet"
    hm.memorize_words(d_sw)
    assert asks(hm.h, k=0, n=0) == abi.QMANN_OK and asks(fx.h, k=0, n=0) == abi.QMANN_OK
    assert asks(hm.h, k=0, q=None) == abi.QMANN_EINVAL
    # then the model's mode, ahead of k and the pointers
    assert forward(fx.h, k=0) == abi.QMANN_EUNSUPPORTED and asks(fx.h, k=0, s=None) == abi.QMANN_EUNSUPPORTED
    # then k and the two pointers
    for verb in (forward, asks):
        assert verb(hm.h, k=0) == abi.QMANN_EINVAL and verb(hm.h, k=abi.QMANN_MAX_TOP_SLOTS + 1) == abi.QMANN_EINVAL
        assert verb(hm.h, s=None) == abi.QMANN_EINVAL and verb(hm.h, t=None) == abi.QMANN_EINVAL
    torch.cuda.synchronize()
    assert (pred == -7).all() and (slot == -7).all() and (tp == -7.0).all(), "none of them launched anything"
    assert forward(hm.h) == abi.QMANN_OK and asks(hm.h) == abi.QMANN_OK
    torch.cuda.synchronize()
    assert (pred != -7).all() and (slot != -7).all()
    # 5. the old verbs still refuse a float model
    slot.fill_(-7)
    assert abi.lib.qmann_model_forward_words_top(hm.h, _p(d_sw), R, d_sw.shape[1], _p(d_q), d_q.shape[1], _p(d_ro), MS, N, None, _p(pred),
                                                 None, None, K, _p(slot), _p(tp), None) == abi.QMANN_EUNSUPPORTED
    for old in (abi.lib.qmann_model_ask_words_top, abi.lib.qmann_model_ask_words_top_packed):
        assert old(hm.h, _p(d_q), d_q.shape[1], N, None, _p(pred), None, None, K, _p(slot), _p(tp), None) == abi.QMANN_EUNSUPPORTED
    torch.cuda.synchronize()
    assert (slot == -7).all()
    hm.close(); fx.close()


# ---- 4. + 5. the hop calls' refusals ---------------------------------------------------------------------------------------------------
def test_hop_calls_refuse_in_order_and_touch_nothing(env):
    torch, abi, model = env.torch, env.abi, env.model
    case = build("af_batch_03")
    run = Run(env, case, True)
    net, S, B, H, K = run.net, case.max_slots, case.B, case.cfg["n_hop"], 3
    u_out = torch.full_like(run.u0, -77.0)
    slot = torch.full((B, H, K), -7, dtype=torch.int32, device=env.dev)
    tp = torch.full((B, H, K), -7.0, dtype=torch.float32, device=env.dev)

    def story(n=None, keys=run.dk, out=u_out, max_slots=S, n_query=B, k=K, s=slot, t=tp):
        return abi.lib.qmann_hops_top_float_i8(C.byref(n if n is not None else net.net), _p(keys), _p(run.dv), run.stride, _p(run.ro),
                                               max_slots, _p(run.u0), _p(out), k, _p(s), _p(t), n_query, None)

    def shared(n=None, keys=run.mk, out=u_out, max_slots=S, n_query=B, k=K, s=slot, t=tp):
        return abi.lib.qmann_hops_shared_top_float_i8(C.byref(n if n is not None else net.net), _p(keys), _p(run.mv), run.mstride, max_slots,
                                                      _p(run.u0), _p(out), k, _p(s), _p(t), n_query, None)

    def variant(**kw):
        n = model._net_from_cfg(case.cfg)
        for h in range(n.n_hop):
            n.lin_map[h] = net.net.lin_map[h]
        for key, v in kw.items():
            setattr(n, key, v)
        return n
    too_long = sf.CAP_SLOTS + 1
    wide = variant()
    wide.w[0] = abi.Fmt(5, 4)                                     # word length 9
    for call in (story, shared):
        # the base call's refusals first, whatever k and the pointers are
        assert call(keys=None, k=0) == abi.QMANN_EINVAL and call(out=None, s=None) == abi.QMANN_EINVAL
        assert call(variant(n_hop=0), k=0) == abi.QMANN_EINVAL
        assert call(variant(dim_emb_pad=96), k=0) == abi.QMANN_EUNSUPPORTED
        assert call(wide, k=0) == abi.QMANN_ERANGE
        assert call(variant(softmax_base=7), k=0) == abi.QMANN_EINVAL
        assert call(max_slots=too_long, k=0) == abi.QMANN_ERANGE
        assert call(n_query=0, k=0, s=None, t=None) == abi.QMANN_OK
        assert call(n_query=1 << 24, k=0) == abi.QMANN_ERANGE
        # then the attention mode, ahead of k and the pointers
        for mode in (2, 3, 10, 11):
            assert call(variant(attention_mode=mode), k=0, s=None) == abi.QMANN_EUNSUPPORTED, mode
        # then k and the two pointers
        assert call(k=0) == abi.QMANN_EINVAL and call(k=abi.QMANN_MAX_TOP_SLOTS + 1) == abi.QMANN_EINVAL
        assert call(s=None) == abi.QMANN_EINVAL and call(t=None) == abi.QMANN_EINVAL
    assert shared(max_slots=0, k=0) == abi.QMANN_EINVAL and shared(variant(attention_mode=2), max_slots=0) == abi.QMANN_EUNSUPPORTED
    torch.cuda.synchronize()
    assert (u_out == -77.0).all() and (slot == -7).all() and (tp == -7.0).all(), "none of them launched anything"
    assert story() == abi.QMANN_OK
    torch.cuda.synchronize()
    assert (slot != -7).all() and (u_out != -77.0).any()
    # the old calls keep refusing float attention
    slot.fill_(-7)
    assert abi.lib.qmann_hops_top_i8(C.byref(net.net), _p(run.dk), _p(run.dv), run.stride, _p(run.ro), S, _p(run.u0), _p(u_out), K,
                                     _p(slot), _p(tp), B, None) == abi.QMANN_EUNSUPPORTED
    assert abi.lib.qmann_hops_shared_top_i8(C.byref(net.net), _p(run.mk), _p(run.mv), run.mstride, S, _p(run.u0), _p(u_out), K, _p(slot),
                                            _p(tp), B, None) == abi.QMANN_EUNSUPPORTED
    torch.cuda.synchronize()
    assert (slot == -7).all()


# ---- 6. graph capture ------------------------------------------------------------------------------------------------------------------
def test_the_shared_call_replays_from_a_captured_graph(env):
    torch = env.torch
    case = build("af_batch_19")
    run = Run(env, case, True)
    K = 5
    eager = run.net.hops_shared_top_float(run.mk, run.mv, case.max_slots, run.u0, K)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=env.dev)
    net = env.model.QNet(case.cfg, case.wts, stream=s.cuda_stream)
    u0 = run.u0.clone()
    with torch.cuda.stream(s):
        net.hops_shared_top_float(run.mk, run.mv, case.max_slots, u0, K)          # warm-up
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        u, slot, p = net.hops_shared_top_float(run.mk, run.mv, case.max_slots, u0, K)      # captured, not run
    for t in (u, slot, p):
        t.zero_()
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(slot, eager[1]) and torch.equal(p.view(torch.int32), eager[2].view(torch.int32))
    assert torch.equal(u.view(torch.int32), eager[0].view(torch.int32)) and int((slot >= 0).sum()) > 0

"""Slot-split shared-plane hops: qmann_hops_shared_split_i8 / qmann_model_enable_split_asks (csrc/batch_hops_shared_split.hip).

1. bit-equality with qmann_hops_shared_i8 on every case of shared_cases.py, under the library's own slices and forced ones;
2. memories beyond the LDS cap against the CPU oracle with NO excused query (test_shared_split_inputs.py has ruled the excuse
   out on these bytes and shown that the slices' merge is visible in them);
3. return codes, nothing launched; 4. the model's opt-in; 5. replay of a split ask from a captured graph."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_pkg
from shared_split_cases import CASES, LONG_CASES, long_case, long_oracle_taps, shared_case

pytestmark = pytest.mark.gpu

LDS_LIMIT = 160 * 1024 - 1024
SLICES = (0, 1, 2, 3, 7)          # the library's choice; one slice; slices shorter than a scan tile, a last slice of 1 row, more than exist


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


def device_case(env, case):
    torch, model = env.torch, env.model
    net = model.QNet(case["cfg"], case["weights"], device="cuda:0")
    dk = torch.from_numpy(model.to_signmag(case["keys"])).to(env.dev)
    dv = torch.from_numpy(model.to_signmag(case["vals"])).to(env.dev)
    return net, dk, dv, torch.from_numpy(case["u0"]).to(env.dev)


def assert_same_run(torch, got, want, what):
    (u_g, t_g), (u_w, t_w) = got, want
    assert torch.equal(u_g, u_w), f"{what}: u_out"
    for f in ("score_codes", "scores", "probs", "o", "u"):
        assert torch.equal(getattr(t_g, f), getattr(t_w, f)), f"{what}: tap {f}"


# ---- 1. against the unsplit call --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_split_equals_the_unsplit_call(env, name):
    """u_out and every tap, torch.equal, for every slicing; without taps too"""
    torch = env.torch
    case = shared_case(name)
    S = case["S"]
    net, dk, dv, du0 = device_case(env, case)
    want = net.hops_shared(dk, dv, S, du0, taps=True)
    for n_slices in SLICES:
        got = net.hops_shared_split(dk, dv, S, du0, n_slices=n_slices, taps=True)
        plain = net.hops_shared_split(dk, dv, S, du0, n_slices=n_slices)
        torch.cuda.synchronize()
        assert_same_run(torch, got, want, f"{name}, n_slices={n_slices}")
        assert torch.equal(plain, want[0]), f"{name}, n_slices={n_slices}: u_out without taps"


@pytest.mark.parametrize("qt", [1, 2, 4, 8])
def test_split_with_forced_tiles(env, monkeypatch, qt):
    """19 queries: tails of 1 (tiles of 2) and 3 (4 and 8) queries, three slices of 512 rows (the last: 476)"""
    torch = env.torch
    case = shared_case("tiles")
    S = case["S"]
    net, dk, dv, du0 = device_case(env, case)
    monkeypatch.delenv("QMANN_SHARED_QT", raising=False)
    env.abi.lib.qmann_tuning_reload()
    want = net.hops_shared(dk, dv, S, du0, taps=True)
    monkeypatch.setenv("QMANN_SHARED_QT", str(qt))
    env.abi.lib.qmann_tuning_reload()
    got = net.hops_shared_split(dk, dv, S, du0, n_slices=3, taps=True)
    torch.cuda.synchronize()
    assert_same_run(torch, got, want, f"tiles of {qt}")


# ---- 2. beyond the LDS cap, against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LONG_CASES))
def test_long_memories_equal_the_oracle(env, name):
    torch, abi = env.torch, env.abi
    case = long_case(name)
    cfg, S, B = case["cfg"], case["S"], case["n_query"]
    H = cfg["n_hop"]
    assert abi.lib.qmann_hops_shared_lds_bytes(S, 1) > LDS_LIMIT
    net, dk, dv, du0 = device_case(env, case)
    u_ref = torch.full_like(du0, -77.0)
    rc = abi.lib.qmann_hops_shared_i8(C.byref(net.net), C.c_void_p(dk.data_ptr()), C.c_void_p(dv.data_ptr()), S * net.Dp, S,
                                      C.c_void_p(du0.data_ptr()), C.c_void_p(u_ref.data_ptr()), None, B, None)
    assert rc == abi.QMANN_ERANGE                                 # the unsplit call still refuses this length
    assert abi.lib.qmann_hops_shared_split_slices(S, net.Dp, B) > 1
    oracle = long_oracle_taps(name)
    for n_slices in (0, 7):
        u_taps, taps = net.hops_shared_split(dk, dv, S, du0, n_slices=n_slices, taps=True)
        u_plain = net.hops_shared_split(dk, dv, S, du0, n_slices=n_slices)
        torch.cuda.synchronize()
        g_codes, g_probs, g_scores = taps.score_codes.cpu().numpy(), taps.probs.cpu().numpy(), taps.scores.cpu().numpy()
        g_o, g_u = taps.o.cpu().numpy(), taps.u.cpu().numpy()
        g_taps, g_plain = u_taps.cpu().numpy(), u_plain.cpu().numpy()
        for q, (_, t) in enumerate(oracle):
            for h in range(H):
                what = f"{name}, n_slices={n_slices}, q{q} h{h}"
                want_codes = np.rint(t["scores"][h] * (1 << cfg["fmt_att"][h][1])).astype(np.int32)
                np.testing.assert_array_equal(g_codes[h, q], want_codes, err_msg=f"score codes {what}")
                np.testing.assert_array_equal(g_scores[h, q], t["scores"][h], err_msg=f"scores {what}")
                np.testing.assert_allclose(g_probs[h, q], t["probs"][h], rtol=1e-5, atol=1e-7, err_msg=f"probs {what}")
                np.testing.assert_array_equal(g_o[q, h], t["o"][h], err_msg=f"o {what}")
                np.testing.assert_array_equal(g_u[q, h], t["u"][h], err_msg=f"u {what}")
            np.testing.assert_array_equal(g_taps[q], t["u"][H - 1], err_msg=f"u_out with taps q{q}")
            np.testing.assert_array_equal(g_plain[q], t["u"][H - 1], err_msg=f"u_out without taps q{q}")
    assert (u_ref == -77.0).all()


# ---- 3. return codes ----------------------------------------------------------------------------------------------------------------
def test_return_codes(env):
    torch, abi, model = env.torch, env.abi, env.model
    case = shared_case("tied_short")
    S, B = case["S"], case["n_query"]
    net, dk, dv, du0 = device_case(env, case)
    u_out = torch.full_like(du0, -77.0)
    need = abi.lib.qmann_hops_shared_split_ws_bytes(C.byref(net.net), S, B)
    assert need == B * abi.lib.qmann_hops_shared_split_ws_bytes(C.byref(net.net), S, 1)
    assert need == B * (16 + (case["cfg"]["n_hop"] + 1) * 1024)                # 9 slots: a pitch of 16
    ws = torch.zeros(need + 16, dtype=torch.uint8, device=env.dev)
    assert ws.data_ptr() % 16 == 0
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(n=None, keys=dk, vals=dv, u0=du0, out=u_out, n_slots=S, n_query=B, n_slices=0, ws_ptr=ws.data_ptr(), ws_bytes=need):
        return abi.lib.qmann_hops_shared_split_i8(C.byref(n if n is not None else net.net), p(keys) if keys is not None else None,
                                                  p(vals) if vals is not None else None, 0, n_slots, p(u0) if u0 is not None else None,
                                                  p(out) if out is not None else None, None, n_query, n_slices,
                                                  C.c_void_p(ws_ptr) if ws_ptr else None, ws_bytes, None)

    def variant(**kw):
        n = model._net_from_cfg(case["cfg"])
        for h in range(n.n_hop):
            n.lin_map[h] = net.net.lin_map[h]
        for k, v in kw.items():
            setattr(n, k, v)
        return n
    for mode in (1, 3, 10, 11):
        assert call(variant(attention_mode=mode)) == abi.QMANN_EUNSUPPORTED
    assert call(variant(dim_emb_pad=96)) == abi.QMANN_EUNSUPPORTED
    assert call(n_slots=0) == abi.QMANN_EINVAL
    assert call(keys=None) == abi.QMANN_EINVAL and call(vals=None) == abi.QMANN_EINVAL
    assert call(u0=None) == abi.QMANN_EINVAL and call(out=None) == abi.QMANN_EINVAL
    assert abi.lib.qmann_hops_shared_split_i8(None, p(dk), p(dv), 0, S, p(du0), p(u_out), None, B, 0, p(ws), need, None) == abi.QMANN_EINVAL
    assert call(ws_ptr=0) == abi.QMANN_EINVAL
    assert call(ws_ptr=ws.data_ptr() + 8) == abi.QMANN_EINVAL
    assert call(ws_bytes=need - 1) == abi.QMANN_EINVAL
    wide = variant()
    wide.att[0] = abi.Fmt(5, 4)                                   # word length 9
    assert call(wide) == abi.QMANN_ERANGE
    assert call(n_slots=(1 << 24) + 1) == abi.QMANN_ERANGE
    assert call(n_query=1 << 24) == abi.QMANN_ERANGE
    assert call(n_query=0) == abi.QMANN_OK
    torch.cuda.synchronize()
    assert (u_out == -77.0).all()                                 # none of them launched anything
    assert call() == abi.QMANN_OK
    torch.cuda.synchronize()
    assert torch.equal(u_out, net.hops_shared(dk, dv, S, du0))
    # the helpers
    assert abi.lib.qmann_hops_shared_split_slices(0, 64, 1) == 0 and abi.lib.qmann_hops_shared_split_slices(9, 64, 4) == 1
    assert abi.lib.qmann_hops_shared_split_ws_bytes(None, S, B) == 0


# ---- 4. the model ---------------------------------------------------------------------------------------------------------------------
LONG_ROWS = 160001
V_, DD_, D_, H_ = 40, 30, 60, 3


def _model_cfg_weights(env):
    rng = np.random.default_rng(78)
    cfg = env.model.babi_cfg(V_, 2, 0, iwl=5, en_mq=True)
    wts = {"w_q": rng.normal(0, 1.0, (D_, V_)).astype(np.float32), "w_ans": rng.normal(0, 0.3, (V_, D_)).astype(np.float32),
           "w_a": [rng.normal(0, 1.0, (D_, V_)).astype(np.float32) for _ in range(H_)],
           "w_c": [rng.normal(0, 1.0, (D_, V_)).astype(np.float32) for _ in range(H_)],
           "w_h": [rng.normal(0, 1.0, (D_, D_)).astype(np.float32) for _ in range(H_)]}
    return cfg, wts


@pytest.fixture(scope="module")
def long_story(env):
    """160 001 rows of words, drawn as test_gpu_graph._words draws them; on the device, made once"""
    from test_gpu_graph import _words
    return env.torch.from_numpy(_words(np.random.default_rng(79), LONG_ROWS, V_, DD_, 8, True).view(np.int16)).to(env.dev)


def _questions(env, seed, B):
    from test_gpu_graph import _words
    r = np.random.default_rng(seed)
    return (env.torch.from_numpy(_words(r, B, V_, DD_, 8, False).view(np.int16)).to(env.dev),
            env.torch.from_numpy(r.integers(0, V_, B).astype(np.int32)).to(env.dev))


def _memorize_rc(env, hm, story, n_rows=None):
    return env.abi.lib.qmann_model_memorize_words(hm.h, C.c_void_p(story.data_ptr()), story.shape[0] if n_rows is None else n_rows,
                                                  story.shape[1], None)


def test_model_split_asks(env, long_story):
    torch, abi, model = env.torch, env.abi, env.model
    cfg, wts = _model_cfg_weights(env)
    hm = model.HostModel(cfg, wts, device="cuda:0")
    too_long = torch.full((200000, 8), -1, dtype=torch.int16, device=env.dev)      # (0xFFFF: no word)
    assert _memorize_rc(env, hm, too_long) == abi.QMANN_ERANGE                      # without the opt-in: as ever
    assert _memorize_rc(env, hm, long_story) == abi.QMANN_ERANGE
    share = abi.lib.qmann_hops_shared_split_ws_bytes(C.byref(hm.net_and_w_ans()[0]), LONG_ROWS, 1)
    assert share == 160016 + 4 * 1024
    qw, ans = _questions(env, 80, 5)
    runs = []
    hm.enable_split_asks(64 * share)                                               # ample
    hm.memorize_words(long_story)
    assert hm.memory_rows() == LONG_ROWS
    for budget in (None, 2 * share, share):                                        # one chunk; chunks of 2 + 2 + 1; five of 1
        if budget:
            hm.enable_split_asks(budget)
            assert hm.memory_rows() == LONG_ROWS                                   # (the memory still fits the budget: kept)
        pred, cost, match = hm.ask_words(qw, ans)
        torch.cuda.synchronize()
        runs.append((pred.clone(), hm.last_u(5), int(match.item())))
    for pred, u, match in runs[1:]:
        assert torch.equal(pred, runs[0][0]) and torch.equal(u, runs[0][1]) and match == runs[0][2]
    assert float(runs[0][1].abs().sum()) > 0
    # the model's ask is the hop call on its own memory: the same u from the public call on the same words
    net = model.QNet.from_model(cfg, hm)
    net.w_q, net.w_a, net.w_c = [torch.from_numpy(wts["w_q"]).to(env.dev),
                                 [torch.from_numpy(w).to(env.dev) for w in wts["w_a"]],
                                 [torch.from_numpy(w).to(env.dev) for w in wts["w_c"]]]
    net.make_tables()
    dk, dv, du0 = net.embed_idx(long_story, qw)
    u_pub = net.hops_shared_split(dk, dv, LONG_ROWS, du0, n_slices=7)
    torch.cuda.synchronize()
    assert torch.equal(u_pub, runs[0][1])
    # a budget below one query's share: memorize refuses, and the kept memory is forgotten
    hm.enable_split_asks(share - 1)
    assert hm.memory_rows() == 0
    assert _memorize_rc(env, hm, long_story) == abi.QMANN_ERANGE
    # 0 turns the mode off: today's refusal again
    hm.enable_split_asks(share)
    hm.memorize_words(long_story)
    hm.enable_split_asks(0)
    assert hm.memory_rows() == 0
    assert _memorize_rc(env, hm, long_story) == abi.QMANN_ERANGE and _memorize_rc(env, hm, too_long) == abi.QMANN_ERANGE
    hm.close()


def test_model_split_asks_leave_short_memories_as_they_are(env, long_story):
    torch, model = env.torch, env.model
    cfg, wts = _model_cfg_weights(env)
    story = long_story[:300].contiguous()
    qw, ans = _questions(env, 81, 37)
    hm, plain = model.HostModel(cfg, wts, device="cuda:0"), model.HostModel(cfg, wts, device="cuda:0")
    hm.enable_split_asks(1 << 20)
    hm.memorize_words(story); plain.memorize_words(story)
    p1, c1, m1 = hm.ask_words(qw, ans)
    p2, c2, m2 = plain.ask_words(qw, ans)
    torch.cuda.synchronize()
    assert torch.equal(p1, p2) and torch.equal(hm.last_u(37), plain.last_u(37)) and int(m1.item()) == int(m2.item())
    assert float(hm.last_u(37).abs().sum()) > 0
    hm.close(); plain.close()


def test_split_asks_refuse_other_attention_modes(env):
    abi, model = env.abi, env.model
    cfg, wts = _model_cfg_weights(env)
    for mode, nb in ((1, 8), (3, 8), (10, 4), (11, 4)):
        hm = model.HostModel(dict(cfg, attention_mode=mode, num_bit=nb), wts, device="cuda:0")
        assert abi.lib.qmann_model_enable_split_asks(hm.h, 1 << 20, None) == abi.QMANN_EUNSUPPORTED
        hm.close()
    assert abi.lib.qmann_model_enable_split_asks(None, 1 << 20, None) == abi.QMANN_EINVAL


# ---- 5. graph capture -------------------------------------------------------------------------------------------------------------------
def test_split_ask_replays_from_a_captured_graph(env, long_story):
    """pattern of test_forward_shared_words_replays_from_a_captured_graph: one eager ask grows the question workspace, the
    captured ask (chunks of 2 + 2 + 1 questions through the split call) replays on new questions in the graph's buffers and
    gives what an eager model gives"""
    torch, abi, model = env.torch, env.abi, env.model
    cfg, wts = _model_cfg_weights(env)
    B = 5
    s = torch.cuda.Stream(device=env.dev)
    hm = model.HostModel(cfg, wts, device="cuda:0", stream=s.cuda_stream)
    eager = model.HostModel(cfg, wts, device="cuda:0")
    share = abi.lib.qmann_hops_shared_split_ws_bytes(C.byref(hm.net_and_w_ans()[0]), LONG_ROWS, 1)
    eager.enable_split_asks(B * share)
    eager.memorize_words(long_story)
    qw, ans = _questions(env, 1, B)
    with torch.cuda.stream(s):
        hm.enable_split_asks(2 * share)
        hm.memorize_words(long_story)
        hm.ask_words(qw, ans)                                                     # warm-up: the question workspace takes its size
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        pred, cost, match = hm.ask_words(qw, ans)                                 # captured, not run
    for seed in (2, 3, 4):
        nqw, nans = _questions(env, seed, B)
        qw.copy_(nqw); ans.copy_(nans)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        p2, c2, m2 = eager.ask_words(nqw, nans)
        torch.cuda.synchronize()
        assert torch.equal(pred, p2), seed
        assert torch.equal(hm.last_u(B), eager.last_u(B)), seed
        assert int(match.item()) == int(m2.item()) and float(cost.item()) == pytest.approx(float(c2.item()), rel=1e-5)
    hm.close(); eager.close()

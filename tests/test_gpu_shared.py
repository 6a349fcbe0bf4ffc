"""One memory for many queries: qmann_hops_shared_i8 / qmann_model_forward_shared_words (csrc/batch_hops_shared.hip).

1. against the CPU oracle, query by query, with the criteria of run_case (test_gpu_batch.py) and NO excused query: the inputs
   are those of shared_cases.py, on which test_shared_inputs.py has ruled the p-on-a-truncation-step excuse out on the CPU;
2. against the per-query kernels: qmann_hops_i8 on n_query copies of the plane, bit for bit;
3. the model call against qmann_model_forward_words on copies of the story, and against the oracle;
4. return codes; 5. replay from a captured graph."""
import ctypes as C
import json

import numpy as np
import pytest

from conftest import GOLD, load_pkg
from shared_cases import CASES, oracle_taps, shared_case

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


def device_case(env, case):
    torch, model = env.torch, env.model
    net = model.QNet(case["cfg"], case["weights"], device="cuda:0")
    dk = torch.from_numpy(model.to_signmag(case["keys"])).to(env.dev)
    dv = torch.from_numpy(model.to_signmag(case["vals"])).to(env.dev)
    return net, dk, dv, torch.from_numpy(case["u0"]).to(env.dev)


# ---- 1. against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qt", [None, 2, 4, 8])
@pytest.mark.parametrize("name", sorted(CASES))
def test_shared_hops_equal_the_oracle(env, force_qt, name, qt):
    """score codes, o and u of every hop and the final state bit-equal, probabilities within north_star's tolerance, for every
    query; the final state both with taps and without.  qt: the tile size forced (None: the launcher's choice)"""
    force_qt(qt)
    case = shared_case(name)
    cfg, S, B = case["cfg"], case["S"], case["n_query"]
    H = cfg["n_hop"]
    if qt:                                                        # the switch took effect: this run is on tiles of qt queries
        assert env.abi.lib.qmann_hops_shared_tile(S, B) == qt
    net, dk, dv, du0 = device_case(env, case)
    u_taps, taps = net.hops_shared(dk, dv, S, du0, taps=True)
    u_plain = net.hops_shared(dk, dv, S, du0)
    env.torch.cuda.synchronize()
    g_codes, g_probs = taps.score_codes.cpu().numpy(), taps.probs.cpu().numpy()
    g_scores = taps.scores.cpu().numpy()
    g_o, g_u = taps.o.cpu().numpy(), taps.u.cpu().numpy()
    g_taps, g_plain = u_taps.cpu().numpy(), u_plain.cpu().numpy()
    assert g_codes.shape == (H, B, S) and g_o.shape == (B, H, cfg["dim_emb"])
    for q, (_, t) in enumerate(oracle_taps(name)):
        for h in range(H):
            want_codes = np.rint(t["scores"][h] * (1 << cfg["fmt_att"][h][1])).astype(np.int32)
            np.testing.assert_array_equal(g_codes[h, q], want_codes, err_msg=f"score codes q{q} h{h}")
            np.testing.assert_array_equal(g_scores[h, q], t["scores"][h], err_msg=f"scores q{q} h{h}")
            np.testing.assert_allclose(g_probs[h, q], t["probs"][h], rtol=1e-5, atol=1e-7, err_msg=f"probs q{q} h{h}")
            np.testing.assert_array_equal(g_o[q, h], t["o"][h], err_msg=f"o q{q} h{h}")
            np.testing.assert_array_equal(g_u[q, h], t["u"][h], err_msg=f"u q{q} h{h}")
        want_u = np.maximum(t["u"][H - 1], 0.0) if cfg.get("en_non_lin") else t["u"][H - 1]     # (u_out is what the answer layer reads)
        np.testing.assert_array_equal(g_taps[q], want_u, err_msg=f"u_out with taps q{q}")
        np.testing.assert_array_equal(g_plain[q], want_u, err_msg=f"u_out without taps q{q}")


# ---- 2. against the per-query kernels ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("qt", [None, 4])
@pytest.mark.parametrize("name", ["config4_q25", "tiles", "en_mq_clamp", "wl6", "tied", "tied_short", "eight_hops", "binary_relu",
                                  "grid_S17_D256_q5", "grid_S64_D60_q5", "grid_S1_D60_q1", "grid_S4097_D256_q17"])
def test_shared_hops_equal_hops_i8_on_copies(env, force_qt, name, qt):
    force_qt(qt)
    torch = env.torch
    case = shared_case(name)
    cfg, S, B = case["cfg"], case["S"], case["n_query"]
    H = cfg["n_hop"]
    net, dk, dv, du0 = device_case(env, case)
    u_s, t_s = net.hops_shared(dk, dv, S, du0, taps=True)
    u_s_plain = net.hops_shared(dk, dv, S, du0)
    # n_query copies of every hop's plane, query q owning rows q S .. (q + 1) S (a tied memory: the one plane for every hop)
    rep = lambda d: d.expand(H, S, net.Dp).unsqueeze(1).expand(H, B, S, net.Dp).reshape(H, B * S, net.Dp).contiguous()
    row_off = torch.arange(0, (B + 1) * S, S, dtype=torch.int32, device=env.dev)
    u_r, t_r = net.hops(rep(dk), rep(dv), row_off, S, du0, taps=True)
    u_r_plain = net.hops(rep(dk), rep(dv), row_off, S, du0)
    torch.cuda.synchronize()
    assert torch.equal(u_s, u_r) and torch.equal(u_s_plain, u_r_plain) and torch.equal(u_s, u_s_plain)
    assert torch.equal(t_s.score_codes, t_r.score_codes.reshape(H, B, S))
    assert torch.equal(t_s.scores, t_r.scores.reshape(H, B, S))
    assert torch.equal(t_s.probs, t_r.probs.reshape(H, B, S))
    assert torch.equal(t_s.o, t_r.o) and torch.equal(t_s.u, t_r.u)


@pytest.mark.parametrize("S,D,want", [(4500, 128, 4), (600, 60, 2)])
def test_the_launchers_own_tile_on_a_full_batch(env, force_qt, S, D, want):
    """enough queries to give every CU a tile: the launcher itself takes tiles of 4 (long memory) / 2 queries, with a short last
    tile, and the result is that of qmann_hops_i8 on copies of the plane"""
    from test_gpu_batch import cfg_synth, weights
    force_qt(None)
    torch, model = env.torch, env.model
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = want * cus + 1
    assert env.abi.lib.qmann_hops_shared_tile(S, B) == want
    H, rng = 3, np.random.default_rng(S)
    net = model.QNet(cfg_synth(D, 40, 2), weights(S, H, D, 40, 6.0 / 32.0, with_emb=False), device="cuda:0")
    plane = lambda: torch.from_numpy(model.to_signmag(np.pad(np.clip(np.rint(rng.normal(0, 6.0, (H, S, D))), -127, 127).astype(np.int8),
                                                             ((0, 0), (0, 0), (0, net.Dp - D))))).to(env.dev)
    dk, dv = plane(), plane()
    du0 = torch.from_numpy((np.clip(np.rint(rng.normal(0, 6.0, (B, D))), -127, 127) / 32.0).astype(np.float32)).to(env.dev)
    u_s = net.hops_shared(dk, dv, S, du0)
    rep = lambda d: d.unsqueeze(1).expand(H, B, S, net.Dp).reshape(H, B * S, net.Dp).contiguous()
    u_r = net.hops(rep(dk), rep(dv), torch.arange(0, (B + 1) * S, S, dtype=torch.int32, device=env.dev), S, du0)
    torch.cuda.synchronize()
    assert torch.equal(u_s, u_r) and float(u_s.abs().sum()) > 0


# ---- 3. model level -----------------------------------------------------------------------------------------------------------
def _model_inputs(which, env):
    from test_gpu_words import weights as word_weights, words16
    model = env.model
    if which == "trained_qa1":
        g = np.load(GOLD / "babi_qa1_test1000_words.npz")
        rec = json.loads((GOLD / "trained_qa1" / "reference_run.json").read_text())
        V, W = int(g["dim_input"]), 8
        cfg = model.babi_cfg(V, attention_mode=2, softmax_base=0, iwl=int(rec["argv"][3]), en_mq=True)
        wts = model.load_weights(GOLD / "trained_qa1", cfg)
    else:
        g = np.load(GOLD / "babi_joint20_test20000_words.npz")
        V, W = int(g["dim_input"]), 16
        cfg = model.babi_cfg(V, attention_mode=2, en_mq=False)
        wts = word_weights(12, 3, 60, V)
    sw, qw = words16(g["story_words"], W), words16(g["question_words"], W)
    ans = g["answer"].astype(np.int64)
    ans = np.where(ans == 0xFF, 0xFFFF, ans)
    return cfg, wts, sw, qw, g["n_sen"].astype(np.int64), ans


@pytest.mark.parametrize("N", [1, 7, 4099])
@pytest.mark.parametrize("which", ["trained_qa1", "random_joint20"])
def test_forward_shared_words_equals_forward_words_on_copies(env, oracle, which, N):
    """one story of the set is THE memory (its longest), the questions are those of N other stories (taken round the set where
    it has fewer); also on a replica built from the parameter blob, and a sample against the oracle"""
    from test_gpu_words import oracle_full
    torch, model = env.torch, env.model
    cfg, wts, sw, qw, n_sen, ans = _model_inputs(which, env)
    offs = np.concatenate([[0], np.cumsum(n_sen)])
    s = int(np.argmax(n_sen))
    story = sw[offs[s]:offs[s + 1]]
    R = story.shape[0]
    others = (s + 1 + np.arange(N)) % len(n_sen)
    q_sel, a_sel = qw[others], ans[others]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(env.dev)
    d_ans = torch.from_numpy(a_sel.astype(np.int32)).to(env.dev)

    hm = model.HostModel(cfg, wts, device="cuda:0")
    pred, cost, match = hm.forward_shared_words(up(story), up(q_sel), d_ans)
    torch.cuda.synchronize()
    p_s, u_s = pred.cpu().numpy(), hm.last_u(N).cpu().numpy()
    c_s, m_s = float(cost.item()), int(match.item())

    story_rep = np.tile(story, (N, 1))
    row_off = (np.arange(N + 1) * R).astype(np.int32)
    hm2 = model.HostModel(cfg, wts, device="cuda:0")
    pred2, cost2, match2 = hm2.forward_words(up(story_rep), up(q_sel), torch.from_numpy(row_off).to(env.dev), R, d_ans)
    torch.cuda.synchronize()
    assert np.array_equal(p_s, pred2.cpu().numpy())
    assert np.array_equal(u_s, hm2.last_u(N).cpu().numpy())
    assert m_s == int(match2.item()) == int((p_s == a_sel).sum())
    assert c_s == pytest.approx(float(cost2.item()), rel=1e-4, abs=1e-3)          # float atomics: the order of the adds differs
    assert np.abs(u_s).sum() > 0
    hm2.close()

    ptr, nbytes = hm.params()
    replica = model.HostModel.from_params(cfg, ptr, nbytes, device="cuda:0")
    pred3, _, match3 = replica.forward_shared_words(up(story), up(q_sel), d_ans)
    torch.cuda.synchronize()
    assert np.array_equal(p_s, pred3.cpu().numpy()) and np.array_equal(u_s, replica.last_u(N).cpu().numpy()) and int(match3.item()) == m_s
    replica.close(); hm.close()

    pick = np.unique(np.linspace(0, N - 1, min(N, 48)).astype(np.int64))
    oracle_full(oracle, cfg, wts, np.tile(story, (len(pick), 1)), q_sel[pick], np.full(len(pick), R, np.int64), p_s[pick], u_s[pick],
                max_excused=0)


def test_forward_shared_words_refuses_other_attention_modes(env):
    torch, model, abi = env.torch, env.model, env.abi
    cfg, wts, sw, qw, n_sen, _ = _model_inputs("random_joint20", env)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(env.dev)
    for mode in (1, 3, 10, 11):
        hm = model.HostModel(dict(cfg, attention_mode=mode), wts, device="cuda:0")
        pred = torch.full((4,), -7, dtype=torch.int32, device=env.dev)
        rc = abi.lib.qmann_model_forward_shared_words(hm.h, C.c_void_p(up(sw[:5]).data_ptr()), 5, sw.shape[1],
                                                      C.c_void_p(up(qw[:4]).data_ptr()), qw.shape[1], 4, None,
                                                      C.c_void_p(pred.data_ptr()), None, None, None)
        torch.cuda.synchronize()
        assert rc == abi.QMANN_EUNSUPPORTED and (pred == -7).all()
        hm.close()


# ---- 4. return codes ------------------------------------------------------------------------------------------------------------
def test_return_codes(env):
    torch, abi, model = env.torch, env.abi, env.model
    case = shared_case("tied_short")
    S, B = case["S"], case["n_query"]
    net, dk, dv, du0 = device_case(env, case)
    u_out = torch.full_like(du0, -77.0)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(n=None, keys=dk, vals=dv, u0=du0, out=u_out, n_slots=S, n_query=B):
        return abi.lib.qmann_hops_shared_i8(C.byref(n if n is not None else net.net), p(keys) if keys is not None else None,
                                            p(vals) if vals is not None else None, 0, n_slots, p(u0) if u0 is not None else None,
                                            p(out) if out is not None else None, None, n_query, None)

    def variant(**kw):
        n = model._net_from_cfg(case["cfg"])
        for h in range(n.n_hop):
            n.lin_map[h] = net.net.lin_map[h]
        for k, v in kw.items():
            setattr(n, k, v)
        return n
    for mode in (1, 3, 10, 11):
        assert call(variant(attention_mode=mode)) == abi.QMANN_EUNSUPPORTED
    assert call(n_slots=0) == abi.QMANN_EINVAL
    assert call(keys=None) == abi.QMANN_EINVAL and call(vals=None) == abi.QMANN_EINVAL
    assert call(u0=None) == abi.QMANN_EINVAL and call(out=None) == abi.QMANN_EINVAL
    assert abi.lib.qmann_hops_shared_i8(None, p(dk), p(dv), 0, S, p(du0), p(u_out), None, B, None) == abi.QMANN_EINVAL
    assert call(variant(dim_emb_pad=96)) == abi.QMANN_EUNSUPPORTED
    wide = variant()
    wide.att[0] = abi.Fmt(5, 4)                                   # word length 9
    assert call(wide) == abi.QMANN_ERANGE
    # a memory too long for LDS with ONE query per workgroup (the sizing helper says so; nothing is read or launched)
    limit = 160 * 1024 - 1024
    assert abi.lib.qmann_hops_shared_lds_bytes(10000, 4) == 4 * abi.lib.qmann_hops_lds_bytes(10000) <= limit
    too_long = 160000
    assert abi.lib.qmann_hops_shared_lds_bytes(too_long, 1) > limit
    assert call(n_slots=too_long) == abi.QMANN_ERANGE
    assert call(n_query=0) == abi.QMANN_OK
    assert call(n_query=1 << 24) == abi.QMANN_ERANGE
    torch.cuda.synchronize()
    assert (u_out == -77.0).all()                                 # none of them launched anything
    assert call() == abi.QMANN_OK
    torch.cuda.synchronize()
    assert torch.equal(u_out, net.hops_shared(dk, dv, S, du0))


# ---- 5. graph capture -----------------------------------------------------------------------------------------------------------
def test_forward_shared_words_replays_from_a_captured_graph(env):
    """pattern of test_gpu_graph.py: one eager call grows the workspace, the captured call replays with new inputs in the
    graph's buffers and gives what an eager model gives"""
    from test_gpu_graph import _words
    torch, model = env.torch, env.model
    dev = env.dev
    rng = np.random.default_rng(77)
    V, dd, D, H, B, R = 40, 30, 60, 3, 333, 23
    cfg = model.babi_cfg(V, 2, 0, iwl=5, en_mq=True)
    wts = {"w_q": rng.normal(0, 1.0, (D, V)).astype(np.float32), "w_ans": rng.normal(0, 0.3, (V, D)).astype(np.float32),
           "w_a": [rng.normal(0, 1.0, (D, V)).astype(np.float32) for _ in range(H)],
           "w_c": [rng.normal(0, 1.0, (D, V)).astype(np.float32) for _ in range(H)],
           "w_h": [rng.normal(0, 1.0, (D, D)).astype(np.float32) for _ in range(H)]}

    def batch(seed):
        r = np.random.default_rng(seed)
        return (torch.from_numpy(_words(r, R, V, dd, 8, True).view(np.int16)).to(dev),
                torch.from_numpy(_words(r, B, V, dd, 8, False).view(np.int16)).to(dev),
                torch.from_numpy(r.integers(0, V, B).astype(np.int32)).to(dev))
    s = torch.cuda.Stream(device=dev)
    hm = model.HostModel(cfg, wts, device="cuda:0", stream=s.cuda_stream)
    plain = model.HostModel(cfg, wts, device="cuda:0")
    sw, qw, ans = batch(1)
    with torch.cuda.stream(s):
        hm.forward_shared_words(sw, qw, ans)                                      # warm-up: the workspace takes its size
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        pred, cost, match = hm.forward_shared_words(sw, qw, ans)                  # captured, not run
    for seed in (2, 3, 4):
        nsw, nqw, nans = batch(seed)
        sw.copy_(nsw); qw.copy_(nqw); ans.copy_(nans)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        p2, c2, m2 = plain.forward_shared_words(nsw, nqw, nans)
        torch.cuda.synchronize()
        assert torch.equal(pred, p2), seed
        assert torch.equal(hm.last_u(B), plain.last_u(B)), seed
        assert int(match.item()) == int(m2.item()) and float(cost.item()) == pytest.approx(float(c2.item()), rel=1e-5)
    assert len({int(x) for x in pred.cpu().numpy()}) > 1                         # (not a degenerate constant prediction)

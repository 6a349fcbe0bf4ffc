"""One packed memory for many queries: qmann_hops_shared_packed (csrc/batch_hops_shared_ham.hip) and the model's memorise-once /
ask-many calls (qmann_model_memorize_words / qmann_model_ask_words).

1. against the CPU oracle, query by query, with the criteria of run_hamming_case (test_gpu_batch.py) and NO excused query: the
   inputs are those of shared_ham_cases.py, on which test_shared_ham_inputs.py has ruled the p-on-a-truncation-step excuse out
   on the CPU;
2. against the per-query kernel: qmann_hops_packed on n_query copies of the planes and values, bit for bit;
3. memorize / ask against qmann_model_forward_words on copies of the story, and against the oracle;
4. return codes; 5. replay of an ask from a captured graph."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_pkg
from shared_ham_cases import (CASES, MODEL_MODES, MODEL_N, MODEL_SOURCES, model_inputs, model_story_and_questions, oracle_taps,
                              shared_ham_case)

pytestmark = pytest.mark.gpu

LDS_LIMIT = 160 * 1024 - 1024


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
    """-> net, packed key planes, sign-magnitude values, u0 on the device"""
    torch, model = env.torch, env.model
    net = model.QNet(case["cfg"], case["weights"], device="cuda:0")
    planes = net.pack_planes(torch.from_numpy(case["key_bytes"]).to(env.dev), case["cfg"]["num_bit"])
    dv = torch.from_numpy(model.to_signmag(case["vals"])).to(env.dev)
    return net, planes, dv, torch.from_numpy(case["u0"]).to(env.dev)


def largest_tile_that_fits(env, net, S):
    fit = 8
    while fit > 1 and env.abi.lib.qmann_hops_shared_packed_lds_bytes(C.byref(net.net), S, fit) > LDS_LIMIT:
        fit //= 2
    return fit


# ---- 1. against the oracle ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qt", [None, 2, 4, 8])
@pytest.mark.parametrize("name", sorted(CASES))
def test_shared_packed_hops_equal_the_oracle(env, force_qt, name, qt):
    """scores and score codes bit-equal in the units of run_hamming_case, probabilities within north_star's tolerance, o and u
    of every hop and the final state bit-equal, for every query; the final state both with taps and without.
    qt: the tile size forced (None: the launcher's choice)"""
    force_qt(qt)
    case = shared_ham_case(name)
    cfg, S, B, unit = case["cfg"], case["S"], case["n_query"], case["unit"]
    H = cfg["n_hop"]
    net, planes, dv, du0 = device_case(env, case)
    if qt:                                  # the switch took effect: tiles of qt queries, or the largest tile that fits LDS
        assert env.abi.lib.qmann_hops_shared_packed_tile(C.byref(net.net), S, B) == min(qt, largest_tile_that_fits(env, net, S))
    u_taps, taps = net.hops_shared_packed(planes, dv, S, du0, taps=True)
    u_plain = net.hops_shared_packed(planes, dv, S, du0)
    env.torch.cuda.synchronize()
    g_codes, g_probs = taps.score_codes.cpu().numpy(), taps.probs.cpu().numpy()
    g_scores = taps.scores.cpu().numpy()
    g_o, g_u = taps.o.cpu().numpy(), taps.u.cpu().numpy()
    g_taps, g_plain = u_taps.cpu().numpy(), u_plain.cpu().numpy()
    assert g_codes.shape == (H, B, S) and g_o.shape == (B, H, cfg["dim_emb"])
    for q, (_, t) in enumerate(oracle_taps(name)):
        for h in range(H):
            np.testing.assert_array_equal(g_scores[h, q], t["scores"][h], err_msg=f"scores q{q} h{h}")
            np.testing.assert_array_equal(g_codes[h, q], np.rint(t["scores"][h] / unit).astype(np.int32), err_msg=f"score codes q{q} h{h}")
            np.testing.assert_allclose(g_probs[h, q], t["probs"][h], rtol=1e-5, atol=1e-7, err_msg=f"probs q{q} h{h}")
            np.testing.assert_array_equal(g_o[q, h], t["o"][h], err_msg=f"o q{q} h{h}")
            np.testing.assert_array_equal(g_u[q, h], t["u"][h], err_msg=f"u q{q} h{h}")
        want_u = np.maximum(t["u"][H - 1], 0.0) if cfg.get("en_non_lin") else t["u"][H - 1]     # (u_out is what the answer layer reads)
        np.testing.assert_array_equal(g_taps[q], want_u, err_msg=f"u_out with taps q{q}")
        np.testing.assert_array_equal(g_plain[q], want_u, err_msg=f"u_out without taps q{q}")


# ---- 2. against the per-query kernel ----------------------------------------------------------------------------------------
def packed_on_copies(env, net, planes, dv, S, du0, taps):
    """qmann_hops_packed with query q owning rows q S .. (q + 1) S of n_query copies of every hop's planes and values"""
    torch = env.torch
    H, B = net.H, du0.shape[0]
    G, nb = net.Dp // 64, planes.shape[-1]
    rk = planes.expand(H, S, G, nb).unsqueeze(1).expand(H, B, S, G, nb).reshape(H, B * S, G, nb).contiguous()
    rv = dv.expand(H, S, net.Dp).unsqueeze(1).expand(H, B, S, net.Dp).reshape(H, B * S, net.Dp).contiguous()
    row_off = torch.arange(0, (B + 1) * S, S, dtype=torch.int32, device=env.dev)
    return net.hops_packed(rk, rv, row_off, S, du0, taps=taps)


@pytest.mark.parametrize("qt", [None, 4])
@pytest.mark.parametrize("name", ["config5_v0_b1", "config5_v1_b8", "tiles_v0", "tiles_v1", "tied_v0", "tied_v1", "en_mq_v0", "en_mq_v1",
                                  "eight_hops_v0", "binary_v1", "exp_shift_scaled_v1", "scale_negative_v0", "v1_one_bit"])
def test_shared_packed_hops_equal_hops_packed_on_copies(env, force_qt, name, qt):
    """S > 64: both calls run the same per-slot stage; final state and every tap bit-equal"""
    force_qt(qt)
    torch = env.torch
    case = shared_ham_case(name)
    S, B, H = case["S"], case["n_query"], case["cfg"]["n_hop"]
    assert S > 64
    net, planes, dv, du0 = device_case(env, case)
    u_s, t_s = net.hops_shared_packed(planes, dv, S, du0, taps=True)
    u_s_plain = net.hops_shared_packed(planes, dv, S, du0)
    u_r, t_r = packed_on_copies(env, net, planes, dv, S, du0, True)
    u_r_plain = packed_on_copies(env, net, planes, dv, S, du0, False)
    torch.cuda.synchronize()
    assert torch.equal(u_s, u_r) and torch.equal(u_s_plain, u_r_plain) and torch.equal(u_s, u_s_plain)
    assert torch.equal(t_s.score_codes, t_r.score_codes.reshape(H, B, S))
    assert torch.equal(t_s.scores, t_r.scores.reshape(H, B, S))
    assert torch.equal(t_s.probs, t_r.probs.reshape(H, B, S))
    assert torch.equal(t_s.o, t_r.o) and torch.equal(t_s.u, t_r.u)
    assert float(u_s.abs().sum()) > 0


@pytest.mark.parametrize("S,D,nb,mode", [(4500, 128, 4, 10), (600, 64, 2, 11)])
def test_the_launchers_own_tile_on_a_full_batch(env, force_qt, S, D, nb, mode):
    """enough queries to give every CU a tile: the launcher itself takes its tile, with a short last tile, and the result is that
    of qmann_hops_packed on copies"""
    from shared_ham_cases import _cfg
    from test_gpu_batch import weights
    force_qt(None)
    torch, model, abi = env.torch, env.model, env.abi
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    H, rng = 3, np.random.default_rng(S)
    net = model.QNet(_cfg(mode, D, nb), weights(S, H, D, 40, 1.0, with_emb=False), device="cuda:0")
    want = abi.lib.qmann_hops_shared_packed_tile(C.byref(net.net), S, 8 * cus)          # (the tile of a batch that fills every CU)
    assert want in (1, 2, 4, 8)
    B = want * cus + 1
    assert abi.lib.qmann_hops_shared_packed_tile(C.byref(net.net), S, B) == want
    code = lambda *shape: np.clip(np.rint(rng.normal(0, 40.0, shape)), -127, 127).astype(np.int8)
    plane = lambda: torch.from_numpy(model.to_signmag(np.pad(code(H, S, D), ((0, 0), (0, 0), (0, net.Dp - D))))).to(env.dev)
    planes, dv = net.pack_planes(plane(), nb), plane()
    du0 = torch.from_numpy((code(B, D) / 4.0).astype(np.float32)).to(env.dev)
    u_s = net.hops_shared_packed(planes, dv, S, du0)
    u_r = packed_on_copies(env, net, planes, dv, S, du0, False)
    torch.cuda.synchronize()
    assert torch.equal(u_s, u_r) and float(u_s.abs().sum()) > 0


# ---- 3. model level -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", MODEL_N)
@pytest.mark.parametrize("mode,num_bit", MODEL_MODES)
@pytest.mark.parametrize("which", MODEL_SOURCES)
def test_memorize_once_ask_many_equals_forward_words_on_copies(env, oracle, which, mode, num_bit, N):
    """memorize_words once; ask_words on two different question batches with a forward_words call on OTHER stories between them
    (it must not disturb the memory); the same on a replica from the parameter blob; a second memorize replaces the first.
    Every ask equals forward_words on copies of the story; a sample of pairs goes against the oracle with nothing excused."""
    from test_gpu_words import oracle_full
    torch, model = env.torch, env.model
    cfg, wts, sw, qw, n_sen, ans = model_inputs(which, mode, num_bit)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(env.dev)
    hm = model.HostModel(cfg, wts, device="cuda:0")
    ref = model.HostModel(cfg, wts, device="cuda:0")
    assert hm.memory_rows() == 0

    def ask(m, q_sel, a_sel):
        pred, cost, match = m.ask_words(up(q_sel), torch.from_numpy(a_sel.astype(np.int32)).to(env.dev))
        torch.cuda.synchronize()
        return pred.cpu().numpy(), m.last_u(len(q_sel)).cpu().numpy(), float(cost.item()), int(match.item())

    def on_copies(story, q_sel, a_sel):
        n, R = len(q_sel), story.shape[0]
        row_off = torch.from_numpy((np.arange(n + 1) * R).astype(np.int32)).to(env.dev)
        pred, cost, match = ref.forward_words(up(np.tile(story, (n, 1))), up(q_sel), row_off, R, torch.from_numpy(a_sel.astype(np.int32)).to(env.dev))
        torch.cuda.synchronize()
        return pred.cpu().numpy(), ref.last_u(n).cpu().numpy(), float(cost.item()), int(match.item())

    def same(got, want, a_sel):
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
        assert got[3] == want[3] == int((got[0] == a_sel).sum())
        assert got[2] == pytest.approx(want[2], rel=1e-4, abs=1e-3)               # float atomics: the order of the adds differs
        assert np.abs(got[1]).sum() > 0

    story, q_sel, a_sel, pick = model_story_and_questions(which, mode, num_bit, N)
    hm.memorize_words(up(story))
    assert hm.memory_rows() == story.shape[0]
    first = ask(hm, q_sel, a_sel)
    same(first, on_copies(story, q_sel, a_sel), a_sel)
    # other stories through the per-batch workspace of the SAME model, then other questions on the kept memory
    lo = int(np.cumsum(n_sen)[9])
    hm.forward_words(up(sw[:lo]), up(qw[:10]), torch.from_numpy(np.concatenate([[0], np.cumsum(n_sen[:10])]).astype(np.int32)).to(env.dev),
                     int(n_sen[:10].max()))
    q2, a2 = q_sel[::-1].copy(), a_sel[::-1].copy()                          # (a copy: a reversed one-row view keeps its negative stride)
    q2 = np.roll(q2, 3, axis=0) if N > 3 else q2
    a2 = np.roll(a2, 3, axis=0) if N > 3 else a2
    same(ask(hm, q2, a2), on_copies(story, q2, a2), a2)

    ptr, nbytes = hm.params()
    replica = model.HostModel.from_params(cfg, ptr, nbytes, device="cuda:0")
    replica.memorize_words(up(story))
    rep = ask(replica, q_sel, a_sel)
    assert np.array_equal(rep[0], first[0]) and np.array_equal(rep[1], first[1]) and rep[3] == first[3]
    replica.close()

    oracle_full(oracle, cfg, wts, np.tile(story, (len(pick), 1)), q_sel[pick], np.full(len(pick), story.shape[0], np.int64),
                first[0][pick], first[1][pick], max_excused=0)

    story_b, q_b, a_b, pick_b = model_story_and_questions(which, mode, num_bit, N, second=True)
    assert not np.array_equal(story_b, story)
    hm.memorize_words(up(story_b))
    assert hm.memory_rows() == story_b.shape[0]
    second = ask(hm, q_b, a_b)
    same(second, on_copies(story_b, q_b, a_b), a_b)
    oracle_full(oracle, cfg, wts, np.tile(story_b, (len(pick_b), 1)), q_b[pick_b], np.full(len(pick_b), story_b.shape[0], np.int64),
                second[0][pick_b], second[1][pick_b], max_excused=0)
    hm.close(); ref.close()


# ---- 4. return codes ------------------------------------------------------------------------------------------------------------
def test_return_codes_of_the_hop_call(env):
    torch, abi, model = env.torch, env.abi, env.model
    case = shared_ham_case("tied_v1")
    S, B = case["S"], case["n_query"]
    net, planes, dv, du0 = device_case(env, case)
    Dp, nb = net.Dp, case["cfg"]["num_bit"]
    u_out = torch.full_like(du0, -77.0)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(n=None, keys=planes, vals=dv, u0=du0, out=u_out, n_slots=S, n_query=B, ks=0, vs=0, key_off=0):
        kp = C.c_void_p(keys.data_ptr() + key_off) if keys is not None else None
        return abi.lib.qmann_hops_shared_packed(C.byref(n if n is not None else net.net), kp, ks, p(vals), vs, n_slots, p(u0), p(out),
                                                None, n_query, None)

    def variant(**kw):
        n = model._net_from_cfg(case["cfg"])
        for h in range(n.n_hop):
            n.lin_map[h] = net.net.lin_map[h]
        for k, v in kw.items():
            setattr(n, k, v)
        return n
    for mode in (1, 2, 3, 12):
        assert call(variant(attention_mode=mode)) == abi.QMANN_EUNSUPPORTED
    for bits in (0, 3, 5, 6, 7):
        assert call(variant(num_bit=bits)) == abi.QMANN_EUNSUPPORTED
    assert call(variant(num_bit=1)) == abi.QMANN_EUNSUPPORTED                  # Dp = 64 with a single plane
    bad_att = variant()
    bad_att.att[1] = abi.Fmt(0, 7)                                             # no integer bit: check_ham_hop refuses
    assert call(bad_att) == abi.QMANN_EUNSUPPORTED
    short_att = variant()
    short_att.att[0] = abi.Fmt(3, 3)                                           # word length 6
    assert call(short_att) == abi.QMANN_EUNSUPPORTED
    assert call(variant(dim_emb_pad=96)) == abi.QMANN_EUNSUPPORTED
    assert call(keys=None) == abi.QMANN_EINVAL and call(vals=None) == abi.QMANN_EINVAL
    assert call(u0=None) == abi.QMANN_EINVAL and call(out=None) == abi.QMANN_EINVAL
    assert abi.lib.qmann_hops_shared_packed(None, p(planes), 0, p(dv), 0, S, p(du0), p(u_out), None, B, None) == abi.QMANN_EINVAL
    assert call(key_off=8) == abi.QMANN_EINVAL                                 # planes not 16-byte aligned
    assert call(n_slots=0) == abi.QMANN_EINVAL
    assert call(ks=S * (Dp // 64) * nb * 8, vs=0) == abi.QMANN_EINVAL          # strides that do not describe the same rows
    assert call(ks=0, vs=S * Dp) == abi.QMANN_EINVAL
    assert call(ks=S * (Dp // 64) * nb * 8 + 16, vs=S * Dp) == abi.QMANN_EINVAL
    # a memory too long for LDS with ONE query per workgroup (the sizing helper says so; nothing is read or launched)
    lds = lambda n_slots, qt: abi.lib.qmann_hops_shared_packed_lds_bytes(C.byref(net.net), n_slots, qt)
    assert lds(10000, 4) == 4 * lds(10000, 1) <= LDS_LIMIT
    too_long = 90000
    assert lds(too_long, 1) > LDS_LIMIT
    assert call(n_slots=too_long) == abi.QMANN_ERANGE
    assert abi.lib.qmann_hops_shared_packed_tile(C.byref(net.net), too_long, B) == 0
    assert call(n_query=0) == abi.QMANN_OK
    assert call(n_query=1 << 24) == abi.QMANN_ERANGE
    torch.cuda.synchronize()
    assert (u_out == -77.0).all()                                 # none of them launched anything
    assert call() == abi.QMANN_OK
    torch.cuda.synchronize()
    assert torch.equal(u_out, net.hops_shared_packed(planes, dv, S, du0))


def test_return_codes_of_memorize_and_ask(env):
    torch, model, abi = env.torch, env.model, env.abi
    cfg, wts, sw, qw, n_sen, _ = model_inputs("random_joint20", 10, 8)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(env.dev)
    d_sw, d_qw = up(sw[:5]), up(qw[:4])
    p = lambda t: C.c_void_p(t.data_ptr())
    pred = torch.full((4,), -7, dtype=torch.int32, device=env.dev)

    def memorize(hm, n_rows=5, words=d_sw):
        return abi.lib.qmann_model_memorize_words(hm.h, p(words) if words is not None else None, n_rows, sw.shape[1], None)

    def ask(hm, n_query=4, words=d_qw, out=pred):
        return abi.lib.qmann_model_ask_words(hm.h, p(words) if words is not None else None, qw.shape[1], n_query, None,
                                             p(out) if out is not None else None, None, None, None)
    for mode, bits in ((1, 8), (3, 8), (10, 3), (11, 7)):        # float and APPX attention; plane counts the packed call refuses
        hm = model.HostModel(dict(cfg, attention_mode=mode, num_bit=bits), wts, device="cuda:0")
        assert memorize(hm) == abi.QMANN_EUNSUPPORTED and hm.memory_rows() == 0
        assert ask(hm) == abi.QMANN_EINVAL                        # nothing memorised
        hm.close()
    hm = model.HostModel(dict(cfg, attention_mode=11, num_bit=1), wts, device="cuda:0")      # D = 60: 64 columns, a single plane
    assert memorize(hm) == abi.QMANN_EUNSUPPORTED
    hm.close()
    for mode in (2, 10):
        hm = model.HostModel(dict(cfg, attention_mode=mode), wts, device="cuda:0")
        assert ask(hm) == abi.QMANN_EINVAL                        # nothing memorised yet
        assert memorize(hm, n_rows=0) == abi.QMANN_EINVAL and memorize(hm, words=None) == abi.QMANN_EINVAL
        assert memorize(hm, n_rows=200000) == abi.QMANN_ERANGE    # too long for LDS: said at memorize, before anything is read
        assert hm.memory_rows() == 0
        assert abi.lib.qmann_model_memorize_words(None, p(d_sw), 5, sw.shape[1], None) == abi.QMANN_EINVAL
        torch.cuda.synchronize()
        assert (pred == -7).all()                                 # none of them launched anything that writes a prediction
        assert memorize(hm) == abi.QMANN_OK and hm.memory_rows() == 5
        assert ask(hm, words=None) == abi.QMANN_EINVAL and ask(hm, out=None) == abi.QMANN_EINVAL
        assert ask(hm, n_query=0) == abi.QMANN_OK
        torch.cuda.synchronize()
        assert (pred == -7).all()
        assert ask(hm) == abi.QMANN_OK
        torch.cuda.synchronize()
        assert (pred != -7).all()
        pred.fill_(-7)
        hm.close()


# ---- 5. graph capture -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,num_bit", [(10, 8), (11, 4), (2, 8)])
def test_ask_words_replays_from_a_captured_graph(env, mode, num_bit):
    """pattern of test_forward_shared_words_replays_from_a_captured_graph: one eager ask grows the question workspace, the
    captured ask replays with new questions in the graph's buffers and gives what an eager model gives"""
    from test_gpu_graph import _words
    torch, model = env.torch, env.model
    dev = env.dev
    rng = np.random.default_rng(78)
    V, dd, D, H, B, R = 40, 30, 60, 3, 333, 23
    cfg = model.babi_cfg(V, mode, 0, iwl=5, en_mq=True)
    cfg["num_bit"] = num_bit
    wts = {"w_q": rng.normal(0, 1.0, (D, V)).astype(np.float32), "w_ans": rng.normal(0, 0.3, (V, D)).astype(np.float32),
           "w_a": [rng.normal(0, 1.0, (D, V)).astype(np.float32) for _ in range(H)],
           "w_c": [rng.normal(0, 1.0, (D, V)).astype(np.float32) for _ in range(H)],
           "w_h": [rng.normal(0, 1.0, (D, D)).astype(np.float32) for _ in range(H)]}
    story = torch.from_numpy(_words(np.random.default_rng(1), R, V, dd, 8, True).view(np.int16)).to(dev)

    def batch(seed):
        r = np.random.default_rng(seed)
        return (torch.from_numpy(_words(r, B, V, dd, 8, False).view(np.int16)).to(dev),
                torch.from_numpy(r.integers(0, V, B).astype(np.int32)).to(dev))
    s = torch.cuda.Stream(device=dev)
    hm = model.HostModel(cfg, wts, device="cuda:0", stream=s.cuda_stream)
    plain = model.HostModel(cfg, wts, device="cuda:0")
    plain.memorize_words(story)
    qw, ans = batch(1)
    with torch.cuda.stream(s):
        hm.memorize_words(story)
        hm.ask_words(qw, ans)                                                     # warm-up: the workspace takes its size
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        pred, cost, match = hm.ask_words(qw, ans)                                 # captured, not run
    for seed in (2, 3, 4):
        nqw, nans = batch(seed)
        qw.copy_(nqw); ans.copy_(nans)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        p2, c2, m2 = plain.ask_words(nqw, nans)
        torch.cuda.synchronize()
        assert torch.equal(pred, p2), seed
        assert torch.equal(hm.last_u(B), plain.last_u(B)), seed
        assert int(match.item()) == int(m2.item()) and float(cost.item()) == pytest.approx(float(c2.item()), rel=1e-5)
    assert len({int(x) for x in pred.cpu().numpy()}) > 1                         # (not a degenerate constant prediction)

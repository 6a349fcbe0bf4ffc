"""Slot-split shared-plane Hamming hops on packed codes: qmann_hops_shared_split_packed / qmann_model_enable_split_asks_packed
(csrc/batch_hops_shared_split_ham.hip).

1. bit-equality with qmann_hops_shared_packed, and equality with the oracle with NO excused query, on every case of
   shared_ham_cases.py under the library's own slices and forced ones; the named cases under forced query tiles too;
2. memories beyond the LDS cap against the CPU oracle with NO excused query (test_shared_split_ham_inputs.py has ruled the
   excuse out on these bytes and shown that the slices' merge is visible in them);
3. the workspace: its contents before the call do not matter, nothing beyond the helper's size is touched, it can be reused;
4. return codes, nothing launched; 5. replay from a captured graph; 6. the model's opt-in."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_pkg
from shared_split_ham_cases import CASES, LONG_CASES, long_ham_case, long_oracle_taps, oracle_taps, shared_ham_case

pytestmark = pytest.mark.gpu

LDS_LIMIT = 160 * 1024 - 1024
NAMED = sorted(n for n in CASES if not n.startswith("grid_"))


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
    """queries per workgroup forced through the tuning switch, as test_gpu_shared_ham.py forces them (conftest reloads the
    switches after the test)"""
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


def assert_same_run(torch, got, want, what):
    (u_g, t_g), (u_w, t_w) = got, want
    assert torch.equal(u_g, u_w), f"{what}: u_out"
    for f in ("score_codes", "scores", "probs", "o", "u"):
        assert torch.equal(getattr(t_g, f), getattr(t_w, f)), f"{what}: tap {f}"


def assert_u_out_is_the_oracles(case, oracle, u_out, what):
    cfg = case["cfg"]
    H = cfg["n_hop"]
    got = u_out.cpu().numpy()
    for q, (_, t) in enumerate(oracle):
        want_u = np.maximum(t["u"][H - 1], 0.0) if cfg.get("en_non_lin") else t["u"][H - 1]     # (u_out is what the answer layer reads)
        np.testing.assert_array_equal(got[q], want_u, err_msg=f"{what}: u_out of query {q} against the oracle")


# ---- 1. against the unsplit call and the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_split_equals_the_unsplit_call_and_the_oracle(env, force_qt, name):
    """u_out and every tap, torch.equal, for the library's slices, 2, 7 and as many as there can be (16 rows each: below one
    tile of rows for every shape); without taps too; u_out against the oracle, nothing excused"""
    force_qt(None)
    torch = env.torch
    case = shared_ham_case(name)
    S = case["S"]
    net, planes, dv, du0 = device_case(env, case)
    want = net.hops_shared_packed(planes, dv, S, du0, taps=True)
    torch.cuda.synchronize()
    assert_u_out_is_the_oracles(case, oracle_taps(name), want[0], f"{name}, unsplit")
    for n_slices in (0, 2, 7, -(-S // 16)):
        got = net.hops_shared_split_packed(planes, dv, S, du0, n_slices=n_slices, taps=True)
        plain = net.hops_shared_split_packed(planes, dv, S, du0, n_slices=n_slices)
        torch.cuda.synchronize()
        assert_same_run(torch, got, want, f"{name}, n_slices={n_slices}")
        assert torch.equal(plain, want[0]), f"{name}, n_slices={n_slices}: u_out without taps"


@pytest.mark.parametrize("qt", [1, 2, 4, 8])
@pytest.mark.parametrize("name", NAMED)
def test_split_with_forced_tiles(env, force_qt, name, qt):
    """the named cases under every forced tile of the scan (short last tiles: 9 queries, 19, 11, 5, 7 ...), seven slices"""
    torch = env.torch
    case = shared_ham_case(name)
    S = case["S"]
    net, planes, dv, du0 = device_case(env, case)
    force_qt(None)
    want = net.hops_shared_packed(planes, dv, S, du0, taps=True)
    force_qt(qt)
    got = net.hops_shared_split_packed(planes, dv, S, du0, n_slices=7, taps=True)
    plain = net.hops_shared_split_packed(planes, dv, S, du0, n_slices=0)
    torch.cuda.synchronize()
    assert_same_run(torch, got, want, f"{name}, tiles of {qt}")
    assert torch.equal(plain, want[0]), f"{name}, tiles of {qt}, the library's slices, no taps"


# ---- 2. beyond the LDS cap, against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LONG_CASES))
def test_long_memories_equal_the_oracle(env, name):
    torch, abi = env.torch, env.abi
    case = long_ham_case(name)
    cfg, S, B, unit = case["cfg"], case["S"], case["n_query"], case["unit"]
    H = cfg["n_hop"]
    net, planes, dv, du0 = device_case(env, case)
    assert abi.lib.qmann_hops_shared_packed_lds_bytes(C.byref(net.net), S, 1) > LDS_LIMIT
    G, nb = net.Dp // 64, cfg["num_bit"]
    u_ref = torch.full_like(du0, -77.0)
    rc = abi.lib.qmann_hops_shared_packed(C.byref(net.net), C.c_void_p(planes.data_ptr()), S * G * nb * 8, C.c_void_p(dv.data_ptr()),
                                          S * net.Dp, S, C.c_void_p(du0.data_ptr()), C.c_void_p(u_ref.data_ptr()), None, B, None)
    assert rc == abi.QMANN_ERANGE                                 # the unsplit call still refuses this length
    assert abi.lib.qmann_hops_shared_split_packed_slices(C.byref(net.net), S, B) > 1
    oracle = long_oracle_taps(name)
    for n_slices in (0, 7):
        u_taps, taps = net.hops_shared_split_packed(planes, dv, S, du0, n_slices=n_slices, taps=True)
        u_plain = net.hops_shared_split_packed(planes, dv, S, du0, n_slices=n_slices)
        torch.cuda.synchronize()
        g_codes, g_probs, g_scores = taps.score_codes.cpu().numpy(), taps.probs.cpu().numpy(), taps.scores.cpu().numpy()
        g_o, g_u = taps.o.cpu().numpy(), taps.u.cpu().numpy()
        g_taps, g_plain = u_taps.cpu().numpy(), u_plain.cpu().numpy()
        for q, (_, t) in enumerate(oracle):
            for h in range(H):
                what = f"{name}, n_slices={n_slices}, q{q} h{h}"
                np.testing.assert_array_equal(g_scores[h, q], t["scores"][h], err_msg=f"scores {what}")
                np.testing.assert_array_equal(g_codes[h, q], np.rint(t["scores"][h] / unit).astype(np.int32), err_msg=f"score codes {what}")
                np.testing.assert_allclose(g_probs[h, q], t["probs"][h], rtol=1e-5, atol=1e-7, err_msg=f"probs {what}")
                np.testing.assert_array_equal(g_o[q, h], t["o"][h], err_msg=f"o {what}")
                np.testing.assert_array_equal(g_u[q, h], t["u"][h], err_msg=f"u {what}")
            np.testing.assert_array_equal(g_taps[q], t["u"][H - 1], err_msg=f"u_out with taps q{q}")
            np.testing.assert_array_equal(g_plain[q], t["u"][H - 1], err_msg=f"u_out without taps q{q}")
    assert (u_ref == -77.0).all()


# ---- 3. the workspace -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["tiles_v0", "tiles_v1", "pow2_v1"])
def test_workspace_contents_and_bounds(env, name):
    """a workspace full of 0xFF gives the same result; a workspace of exactly the helper's size inside a larger guard-filled
    buffer leaves the guard as it was; two calls back to back on one workspace are equal"""
    torch, abi = env.torch, env.abi
    case = shared_ham_case(name)
    S, B = case["S"], case["n_query"]
    net, planes, dv, du0 = device_case(env, case)
    want = net.hops_shared_packed(planes, dv, S, du0)
    need = abi.lib.qmann_hops_shared_split_packed_ws_bytes(C.byref(net.net), S, B)
    assert need > 0 and need % 16 == 0
    guard = 4096
    buf = torch.full((guard + need + guard,), 0xA5, dtype=torch.uint8, device=env.dev)
    assert buf.data_ptr() % 16 == 0
    ws = buf[guard:guard + need]
    for n_slices in (0, 7):
        ws.fill_(0xFF)
        first = net.hops_shared_split_packed(planes, dv, S, du0, n_slices=n_slices, ws=ws).clone()
        second = net.hops_shared_split_packed(planes, dv, S, du0, n_slices=n_slices, ws=ws).clone()      # on what the first left behind
        torch.cuda.synchronize()
        assert torch.equal(first, want) and torch.equal(second, want), f"{name}, n_slices={n_slices}"
        assert (buf[:guard] == 0xA5).all() and (buf[guard + need:] == 0xA5).all(), f"{name}, n_slices={n_slices}: the guard was written"


# ---- 4. return codes ------------------------------------------------------------------------------------------------------------------
def test_return_codes(env):
    torch, abi, model = env.torch, env.abi, env.model
    case = shared_ham_case("tied_v1")
    S, B = case["S"], case["n_query"]
    net, planes, dv, du0 = device_case(env, case)
    Dp, nb = net.Dp, case["cfg"]["num_bit"]
    u_out = torch.full_like(du0, -77.0)
    need = abi.lib.qmann_hops_shared_split_packed_ws_bytes(C.byref(net.net), S, B)
    assert need == B * abi.lib.qmann_hops_shared_split_packed_ws_bytes(C.byref(net.net), S, 1)
    assert need == B * (2 * 144 + 1024)                           # 130 slots: a pitch of 144 int16; V1: no bins
    ws = torch.zeros(need + 16, dtype=torch.uint8, device=env.dev)
    assert ws.data_ptr() % 16 == 0
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(n=None, keys=planes, vals=dv, u0=du0, out=u_out, n_slots=S, n_query=B, ks=0, vs=0, key_off=0, n_slices=0,
             ws_ptr=ws.data_ptr(), ws_bytes=need):
        kp = C.c_void_p(keys.data_ptr() + key_off) if keys is not None else None
        return abi.lib.qmann_hops_shared_split_packed(C.byref(n if n is not None else net.net), kp, ks, p(vals), vs, n_slots, p(u0),
                                                      p(out), None, n_query, n_slices, C.c_void_p(ws_ptr) if ws_ptr else None,
                                                      ws_bytes, None)

    def variant(**kw):
        n = model._net_from_cfg(case["cfg"])
        for h in range(n.n_hop):
            n.lin_map[h] = net.net.lin_map[h]
        for k, v in kw.items():
            setattr(n, k, v)
        return n
    # every refusal of qmann_hops_shared_packed (test_gpu_shared_ham.py) except the LDS one
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
    assert abi.lib.qmann_hops_shared_split_packed(None, p(planes), 0, p(dv), 0, S, p(du0), p(u_out), None, B, 0, p(ws), need, None) == abi.QMANN_EINVAL
    assert call(key_off=8) == abi.QMANN_EINVAL                                 # planes not 16-byte aligned
    assert call(n_slots=0) == abi.QMANN_EINVAL
    assert call(ks=S * (Dp // 64) * nb * 8, vs=0) == abi.QMANN_EINVAL          # strides that do not describe the same rows
    assert call(ks=0, vs=S * Dp) == abi.QMANN_EINVAL
    assert call(ks=S * (Dp // 64) * nb * 8 + 16, vs=S * Dp) == abi.QMANN_EINVAL
    assert call(n_query=1 << 24) == abi.QMANN_ERANGE
    assert call(n_query=0) == abi.QMANN_OK
    # the split call's own
    assert call(ws_ptr=0) == abi.QMANN_EINVAL
    assert call(ws_ptr=ws.data_ptr() + 8) == abi.QMANN_EINVAL
    assert call(ws_bytes=need - 1) == abi.QMANN_EINVAL
    assert call(n_slots=(1 << 24) + 1) == abi.QMANN_ERANGE
    torch.cuda.synchronize()
    assert (u_out == -77.0).all()                                 # none of them launched anything
    assert call() == abi.QMANN_OK
    torch.cuda.synchronize()
    assert torch.equal(u_out, net.hops_shared_packed(planes, dv, S, du0))
    # the helpers' zeros
    slices, ws_bytes = abi.lib.qmann_hops_shared_split_packed_slices, abi.lib.qmann_hops_shared_split_packed_ws_bytes
    assert slices(C.byref(net.net), 0, 1) == 0 and slices(C.byref(net.net), S, 0) == 0 and slices(None, S, B) == 0
    assert slices(C.byref(net.net), S, B) == 1                    # 130 slots: below the floor of 256 rows at LPRK 4
    assert ws_bytes(None, S, B) == 0 and ws_bytes(C.byref(net.net), S, 0) == 0 and ws_bytes(C.byref(net.net), 0, B) == 0
    assert ws_bytes(C.byref(variant(attention_mode=2)), S, B) == 0
    # the fixed-point split call still refuses the Hamming modes
    for mode in (10, 11):
        rc = abi.lib.qmann_hops_shared_split_i8(C.byref(variant(attention_mode=mode)), p(dv), p(dv), 0, S, p(du0), p(u_out), None, B, 0,
                                                p(ws), need, None)
        assert rc == abi.QMANN_EUNSUPPORTED


# ---- 5. graph capture -------------------------------------------------------------------------------------------------------------------
def _loaded_hip_runtime():
    """the HIP runtime this process already runs on (the one torch brought), opened by its path: the same library, not a second"""
    with open("/proc/self/maps") as f:
        paths = sorted({line.split()[-1] for line in f if "libamdhip64" in line})
    assert paths, "no HIP runtime loaded"
    return C.CDLL(paths[0])


def test_split_call_replays_from_a_captured_graph(env):
    """the call captured on a side stream (V0: the memset of the bins and two kernels per hop) is a straight chain of 1 + 2 n_hop
    nodes; replayed twice with new u0 in the graph's buffer it gives what the eager calls give"""
    torch, abi = env.torch, env.abi
    hip = _loaded_hip_runtime()
    case = shared_ham_case("tiles_v0")
    S, B, H = case["S"], case["n_query"], case["cfg"]["n_hop"]
    net, planes, dv, du0 = device_case(env, case)
    need = abi.lib.qmann_hops_shared_split_packed_ws_bytes(C.byref(net.net), S, B)
    ws = torch.empty(need, dtype=torch.uint8, device=env.dev)
    u_in, u_out = du0.clone(), torch.empty_like(du0)
    s = torch.cuda.Stream(device=env.dev)
    stream = C.c_void_p(s.cuda_stream)
    net.stream = s.cuda_stream
    net.hops_shared_split_packed(planes, dv, S, u_in, n_slices=7, u_out=u_out, ws=ws)           # warm-up (allocates nothing: ws, u_out given)
    s.synchronize()
    graph, gexec = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamBeginCapture(stream, 1) == 0                                            # (thread-local capture mode)
    net.hops_shared_split_packed(planes, dv, S, u_in, n_slices=7, u_out=u_out, ws=ws)           # captured, not run
    assert hip.hipStreamEndCapture(stream, C.byref(graph)) == 0 and graph.value
    net.stream = None
    # a straight chain: 1 + 2 n_hop nodes, one root, and edges that give every other node one predecessor and one successor at most
    n_nodes, n_edges, n_roots = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0)
    assert hip.hipGraphGetNodes(graph, None, C.byref(n_nodes)) == 0 and n_nodes.value == 1 + 2 * H
    assert hip.hipGraphGetRootNodes(graph, None, C.byref(n_roots)) == 0 and n_roots.value == 1
    assert hip.hipGraphGetEdges(graph, None, None, C.byref(n_edges)) == 0 and n_edges.value == 2 * H
    src, dst = (C.c_void_p * n_edges.value)(), (C.c_void_p * n_edges.value)()
    assert hip.hipGraphGetEdges(graph, src, dst, C.byref(n_edges)) == 0
    assert len(set(src)) == len(set(dst)) == 2 * H
    assert hip.hipGraphInstantiate(C.byref(gexec), graph, None, None, C.c_size_t(0)) == 0
    rng = np.random.default_rng(5)
    for rep in range(2):
        new = torch.from_numpy((np.clip(np.rint(rng.normal(0, 40.0, tuple(du0.shape))), -127, 127) / 32.0).astype(np.float32)).to(env.dev)
        u_in.copy_(new)
        u_out.fill_(-77.0)
        torch.cuda.synchronize()
        assert hip.hipGraphLaunch(gexec, stream) == 0
        s.synchronize()
        eager = net.hops_shared_split_packed(planes, dv, S, new, n_slices=7)
        unsplit = net.hops_shared_packed(planes, dv, S, new)
        torch.cuda.synchronize()
        assert torch.equal(u_out, eager) and torch.equal(u_out, unsplit), rep
        assert float(u_out.abs().sum()) > 0
    assert hip.hipGraphExecDestroy(gexec) == 0 and hip.hipGraphDestroy(graph) == 0


# ---- 6. the model -------------------------------------------------------------------------------------------------------------------------
LONG_ROWS = 80017
V_, DD_, D_, H_ = 40, 30, 60, 3


def _model_cfg_weights(env, mode, num_bit):
    rng = np.random.default_rng(78)
    cfg = env.model.babi_cfg(V_, mode, 0, iwl=5, en_mq=True)
    cfg["num_bit"] = num_bit
    wts = {"w_q": rng.normal(0, 1.0, (D_, V_)).astype(np.float32), "w_ans": rng.normal(0, 0.3, (V_, D_)).astype(np.float32),
           "w_a": [rng.normal(0, 1.0, (D_, V_)).astype(np.float32) for _ in range(H_)],
           "w_c": [rng.normal(0, 1.0, (D_, V_)).astype(np.float32) for _ in range(H_)],
           "w_h": [rng.normal(0, 1.0, (D_, D_)).astype(np.float32) for _ in range(H_)]}
    return cfg, wts


@pytest.fixture(scope="module")
def long_story(env):
    """80 017 rows of words, drawn as test_gpu_graph._words draws them; on the device, made once"""
    from test_gpu_graph import _words
    return env.torch.from_numpy(_words(np.random.default_rng(79), LONG_ROWS, V_, DD_, 8, True).view(np.int16)).to(env.dev)


def _questions(env, seed, B):
    from test_gpu_graph import _words
    r = np.random.default_rng(seed)
    return (env.torch.from_numpy(_words(r, B, V_, DD_, 8, False).view(np.int16)).to(env.dev),
            env.torch.from_numpy(r.integers(0, V_, B).astype(np.int32)).to(env.dev))


def _memorize_rc(env, hm, story):
    return env.abi.lib.qmann_model_memorize_words(hm.h, C.c_void_p(story.data_ptr()), story.shape[0], story.shape[1], None)


@pytest.mark.parametrize("mode,num_bit", [(11, 8), (10, 4)])
def test_model_split_asks_packed(env, long_story, mode, num_bit):
    torch, abi, model = env.torch, env.abi, env.model
    cfg, wts = _model_cfg_weights(env, mode, num_bit)
    hm = model.HostModel(cfg, wts, device="cuda:0")
    net_c = hm.net_and_w_ans()[0]
    assert abi.lib.qmann_hops_shared_packed_lds_bytes(C.byref(net_c), LONG_ROWS, 1) > LDS_LIMIT
    assert _memorize_rc(env, hm, long_story) == abi.QMANN_ERANGE                    # without the opt-in: as ever
    assert abi.lib.qmann_model_enable_split_asks(hm.h, 1 << 20, None) == abi.QMANN_EUNSUPPORTED     # the fixed-point opt-in: as ever
    assert _memorize_rc(env, hm, long_story) == abi.QMANN_ERANGE
    share = abi.lib.qmann_hops_shared_split_packed_ws_bytes(C.byref(net_c), LONG_ROWS, 1)
    bins = (num_bit * D_ + 1 + 3) // 4 * 4 if mode == 10 else 0
    assert share == 2 * 80032 + 4 * H_ * bins + 1024
    qw, ans = _questions(env, 80, 5)
    runs = []
    hm.enable_split_asks_packed(64 * share)                                        # ample
    hm.memorize_words(long_story)
    assert hm.memory_rows() == LONG_ROWS
    for budget in (None, 2 * share, share):                                        # one chunk; chunks of 2 + 2 + 1; five of 1
        if budget:
            hm.enable_split_asks_packed(budget)
            assert hm.memory_rows() == LONG_ROWS                                   # (the memory still fits the budget: kept)
        pred, cost, match = hm.ask_words(qw, ans)
        torch.cuda.synchronize()
        runs.append((pred.clone(), hm.last_u(5).clone(), int(match.item())))
    for pred, u, match in runs[1:]:
        assert torch.equal(pred, runs[0][0]) and torch.equal(u, runs[0][1]) and match == runs[0][2]
    assert float(runs[0][1].abs().sum()) > 0
    # the model's ask is the hop call on its own memory: the same u from the public calls on the same words
    net = model.QNet.from_model(cfg, hm)
    net.w_q, net.w_a, net.w_c = [torch.from_numpy(wts["w_q"]).to(env.dev),
                                 [torch.from_numpy(w).to(env.dev) for w in wts["w_a"]],
                                 [torch.from_numpy(w).to(env.dev) for w in wts["w_c"]]]
    net.make_tables()
    dk, dv, du0 = net.embed_idx(long_story, qw)
    u_pub = net.hops_shared_split_packed(net.pack_planes(dk, num_bit), dv, LONG_ROWS, du0, n_slices=7)
    torch.cuda.synchronize()
    assert torch.equal(u_pub, runs[0][1])
    # a budget below one query's share: memorize refuses, and the kept memory is forgotten
    hm.enable_split_asks_packed(share - 1)
    assert hm.memory_rows() == 0
    assert _memorize_rc(env, hm, long_story) == abi.QMANN_ERANGE
    # 0 turns the mode off: today's refusal again
    hm.enable_split_asks_packed(share)
    hm.memorize_words(long_story)
    hm.enable_split_asks_packed(0)
    assert hm.memory_rows() == 0
    assert _memorize_rc(env, hm, long_story) == abi.QMANN_ERANGE
    hm.close()


@pytest.mark.parametrize("mode,num_bit", [(11, 8), (10, 4)])
def test_model_split_asks_packed_leave_short_memories_as_they_are(env, long_story, mode, num_bit):
    torch, model = env.torch, env.model
    cfg, wts = _model_cfg_weights(env, mode, num_bit)
    story = long_story[:700].contiguous()
    qw, ans = _questions(env, 81, 37)
    hm, plain = model.HostModel(cfg, wts, device="cuda:0"), model.HostModel(cfg, wts, device="cuda:0")
    hm.enable_split_asks_packed(1 << 20)
    hm.memorize_words(story); plain.memorize_words(story)
    p1, c1, m1 = hm.ask_words(qw, ans)
    p2, c2, m2 = plain.ask_words(qw, ans)
    torch.cuda.synchronize()
    assert torch.equal(p1, p2) and torch.equal(hm.last_u(37), plain.last_u(37)) and int(m1.item()) == int(m2.item())
    assert float(hm.last_u(37).abs().sum()) > 0
    hm.close(); plain.close()


def test_packed_split_asks_refuse_other_models(env):
    abi, model = env.abi, env.model
    cfg, wts = _model_cfg_weights(env, 2, 8)
    for mode, nb in ((1, 8), (2, 8), (3, 8), (10, 3), (11, 1)):        # float, fixed-point, APPX; planes the packed call refuses
        hm = model.HostModel(dict(cfg, attention_mode=mode, num_bit=nb), wts, device="cuda:0")
        assert abi.lib.qmann_model_enable_split_asks_packed(hm.h, 1 << 20, None) == abi.QMANN_EUNSUPPORTED
        hm.close()
    assert abi.lib.qmann_model_enable_split_asks_packed(None, 1 << 20, None) == abi.QMANN_EINVAL

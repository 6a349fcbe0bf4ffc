"""Attended slots for the packed Hamming forms: qmann_hops_shared_top_packed / qmann_hops_shared_split_top_packed /
qmann_model_ask_words_top_packed (csrc/hops_attended_ham.h).

The yardstick everywhere is the `probs` tap of the EXISTING call on the same inputs (qmann_hops_shared_packed where it runs,
qmann_hops_shared_split_packed beyond the LDS cap), ordered by "larger probability first, equal probabilities: lower slot first"
(attended_cases.want_rows).  Nothing is excused: slots are compared exactly, probabilities by bit pattern, u_out with torch.equal
against the plain call WITHOUT taps.  test_attended_ham_inputs.py asserts on the CPU that the cases put the selection where it
can go wrong (ties across the cut, zeros in the first 16, k filled from below V1's threshold shortcut).

1. every case of shared_ham_cases.py, k in {1, 5, 16}; 2. forced tiles; 3. all-zero memories and planted identical rows, V0 and
V1, the three softmax bases; 4. the split call, memories beyond the LDS cap included; 5. return codes, nothing launched, the base
call's refusals first; 6. the model's ask, unsplit on bAbI stories and in chunks through the split call on a memory of 80 017
rows; 7. replay from a captured graph."""
import ctypes as C

import numpy as np
import pytest

from attended_cases import PAD_SLOT, assert_rows
from attended_ham_cases import BASES, MODES, PLANT_ROWS, PLANT_S, ZERO_S, planted_ham_case, zero_ham_case
from conftest import load_pkg
from shared_ham_cases import CASES, MODEL_SOURCES, MODEL_N, model_inputs, model_story_and_questions, shared_ham_case
from shared_split_ham_cases import LONG_CASES, long_ham_case

pytestmark = pytest.mark.gpu

KS = (1, 5, 16)
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


_REF = {}


def reference(env, key, case, split=False):
    """(the probs tap [H][B][S] as numpy, u_out of the plain call WITHOUT taps) of the EXISTING call on a case -- computed once per
    process under the launcher's own tile and left unchanged"""
    if key not in _REF:
        net, planes, dv, du0 = device_case(env, case)
        run = net.hops_shared_split_packed if split else net.hops_shared_packed
        _, taps = run(planes, dv, case["S"], du0, taps=True)
        u_plain = run(planes, dv, case["S"], du0)
        env.torch.cuda.synchronize()
        probs = taps.probs.cpu().numpy()
        probs.setflags(write=False)
        _REF[key] = (probs, u_plain.clone())
    return _REF[key]


# ---- 1. every shared Hamming case -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_top_equals_the_sorted_tap(env, force_qt, name):
    force_qt(None)
    case = shared_ham_case(name)
    probs, u_plain = reference(env, name, case)
    net, planes, dv, du0 = device_case(env, case)
    for k in KS:
        u, slot, p = net.hops_shared_top_packed(planes, dv, case["S"], du0, k)
        env.torch.cuda.synchronize()
        assert env.torch.equal(u, u_plain), f"{name}: u_out, k={k}"
        assert_rows(slot, p, probs, k, name)


# ---- 2. forced tiles ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qt", [1, 2, 4, 8])
@pytest.mark.parametrize("name", ["tiles_v0", "tiles_v1"])
def test_top_with_forced_tiles(env, force_qt, name, qt):
    case = shared_ham_case(name)
    force_qt(None)
    probs, u_plain = reference(env, name, case)
    force_qt(qt)
    net, planes, dv, du0 = device_case(env, case)
    assert env.abi.lib.qmann_hops_shared_packed_tile(C.byref(net.net), case["S"], case["n_query"]) == qt
    u, slot, p = net.hops_shared_top_packed(planes, dv, case["S"], du0, 16)
    env.torch.cuda.synchronize()
    assert env.torch.equal(u, u_plain)
    assert_rows(slot, p, probs, 16, f"{name}, tiles of {qt}")


# ---- 3. plants ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", ZERO_S)
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("mode,D,nb", MODES)
def test_all_zero_memory(env, force_qt, mode, D, nb, base, S):
    force_qt(None)
    case = zero_ham_case(mode, D, nb, base, S)
    probs, u_plain = reference(env, ("zero", mode, base, S), case)
    for h in range(probs.shape[0]):                                 # the plant did what it should: one float per query and hop
        for q in range(probs.shape[1]):
            assert (probs[h, q].view(np.uint32) == probs[h, q, 0].view(np.uint32)).all()
    net, planes, dv, du0 = device_case(env, case)
    for split in (False, True):
        for k in KS:
            if split:
                u, slot, p = net.hops_shared_split_top_packed(planes, dv, S, du0, k, n_slices=2)
            else:
                u, slot, p = net.hops_shared_top_packed(planes, dv, S, du0, k)
            env.torch.cuda.synchronize()
            n = min(k, S)
            got = slot.cpu().numpy().view(np.uint32)
            what = f"zero memory, mode {mode}, base {base}, S={S}, k={k}, split={split}"
            assert (got[:, :, :n] == np.arange(n, dtype=np.uint32)).all() and (got[:, :, n:] == PAD_SLOT).all(), what
            assert env.torch.equal(u, u_plain), what
            assert_rows(slot, p, probs, k, what)


def _assert_planted_tap(probs):
    """what the test below relies on, asserted on the EXISTING kernel's tap: the planted rows carry one float per query and hop,
    and for query 0 at hop 0 it is the row's maximum and above every other row"""
    others = np.setdiff1d(np.arange(PLANT_S), PLANT_ROWS)
    for h in range(probs.shape[0]):
        for q in range(probs.shape[1]):
            p = probs[h, q]
            assert (p[PLANT_ROWS].view(np.uint32) == p[PLANT_ROWS[0]].view(np.uint32)).all(), (h, q)
    p = probs[0, 0]
    assert p[PLANT_ROWS[0]] == p.max() and p[PLANT_ROWS[0]] > p[others].max()


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("mode,D,nb", MODES)
def test_planted_identical_rows(env, force_qt, mode, D, nb, base):
    force_qt(None)
    case = planted_ham_case(mode, D, nb, base)
    probs, u_plain = reference(env, ("planted", mode, base), case)
    _assert_planted_tap(probs)
    net, planes, dv, du0 = device_case(env, case)
    for split in (False, True):
        for k in (5, 16):
            if split:
                u, slot, p = net.hops_shared_split_top_packed(planes, dv, PLANT_S, du0, k, n_slices=7)
            else:
                u, slot, p = net.hops_shared_top_packed(planes, dv, PLANT_S, du0, k)
            env.torch.cuda.synchronize()
            what = f"planted, mode {mode}, base {base}, k={k}, split={split}"
            assert env.torch.equal(u, u_plain), what
            got = slot.cpu().numpy().view(np.uint32)
            n = min(k, len(PLANT_ROWS))
            assert got[0, 0, :n].tolist() == PLANT_ROWS[:n], what
            assert_rows(slot, p, probs, k, what)


# ---- 4. the split call ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_split_top_equals_the_unsplit_call(env, force_qt, name):
    force_qt(None)
    torch = env.torch
    case = shared_ham_case(name)
    S = case["S"]
    probs, u_plain = reference(env, name, case)
    net, planes, dv, du0 = device_case(env, case)
    for k in (5, 16):
        u1, slot1, p1 = net.hops_shared_top_packed(planes, dv, S, du0, k)
        for n_slices in (1, 2, 7, 0):
            u, slot, p = net.hops_shared_split_top_packed(planes, dv, S, du0, k, n_slices=n_slices)
            torch.cuda.synchronize()
            what = f"{name}, n_slices={n_slices}, k={k}"
            assert torch.equal(u, u_plain), what
            assert torch.equal(slot, slot1) and torch.equal(p.view(torch.int32), p1.view(torch.int32)), what
            assert_rows(slot, p, probs, k, what)


@pytest.mark.parametrize("name", sorted(LONG_CASES))
def test_split_top_beyond_the_lds_cap(env, force_qt, name):
    """only the split call runs these lengths; its own probs tap is the yardstick"""
    force_qt(None)
    torch = env.torch
    case = long_ham_case(name)
    S = case["S"]
    probs, u_plain = reference(env, name, case, split=True)
    net, planes, dv, du0 = device_case(env, case)
    assert env.abi.lib.qmann_hops_shared_packed_lds_bytes(C.byref(net.net), S, 1) > LDS_LIMIT
    for k, n_slices in ((5, 0), (16, 7), (1, 2)):
        u, slot, p = net.hops_shared_split_top_packed(planes, dv, S, du0, k, n_slices=n_slices)
        torch.cuda.synchronize()
        assert torch.equal(u, u_plain)
        assert_rows(slot, p, probs, k, f"{name}, n_slices={n_slices}")


# ---- 5. return codes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
def test_return_codes(env, force_qt, split):
    force_qt(None)
    torch, abi, model = env.torch, env.abi, env.model
    case = shared_ham_case("tied_v1")
    S, B, H, K = case["S"], case["n_query"], case["cfg"]["n_hop"], 5
    net, planes, dv, du0 = device_case(env, case)
    Dp, nb = net.Dp, case["cfg"]["num_bit"]
    u_out = torch.full_like(du0, -77.0)
    slot = torch.full((B, H, K), -7, dtype=torch.int32, device=env.dev)
    tp = torch.full((B, H, K), -7.0, dtype=torch.float32, device=env.dev)
    need = abi.lib.qmann_hops_shared_split_packed_ws_bytes(C.byref(net.net), S, B)
    ws = torch.zeros(need + 16, dtype=torch.uint8, device=env.dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(n=None, keys=planes, vals=dv, u0=du0, out=u_out, n_slots=S, n_query=B, ks=0, vs=0, key_off=0, k=K, top_slot=slot,
             top_p=tp, net_null=False, ws_ptr=ws.data_ptr(), ws_bytes=need):
        nref = None if net_null else C.byref(n if n is not None else net.net)
        kp = C.c_void_p(keys.data_ptr() + key_off) if keys is not None else None
        if split:
            return abi.lib.qmann_hops_shared_split_top_packed(nref, kp, ks, p(vals), vs, n_slots, p(u0), p(out), k, p(top_slot),
                                                              p(top_p), n_query, 0, C.c_void_p(ws_ptr) if ws_ptr else None,
                                                              ws_bytes, None)
        return abi.lib.qmann_hops_shared_top_packed(nref, kp, ks, p(vals), vs, n_slots, p(u0), p(out), k, p(top_slot), p(top_p),
                                                    n_query, None)

    def variant(**kw):
        n = model._net_from_cfg(case["cfg"])
        for h in range(n.n_hop):
            n.lin_map[h] = net.net.lin_map[h]
        for key, v in kw.items():
            setattr(n, key, v)
        return n
    # the new refusals
    assert call(k=0) == abi.QMANN_EINVAL and call(k=17) == abi.QMANN_EINVAL
    assert call(top_slot=None) == abi.QMANN_EINVAL and call(top_p=None) == abi.QMANN_EINVAL
    # every refusal of the base call (test_gpu_shared_ham.py / test_gpu_shared_split_ham.py); QMANN_ATT_FIXED is mode 2
    for mode in (1, 2, 3, 12):
        assert call(variant(attention_mode=mode)) == abi.QMANN_EUNSUPPORTED
    for bits in (0, 3, 5, 6, 7):
        assert call(variant(num_bit=bits)) == abi.QMANN_EUNSUPPORTED
    assert call(variant(num_bit=1)) == abi.QMANN_EUNSUPPORTED                  # Dp = 64 with a single plane
    bad_att = variant()
    bad_att.att[1] = abi.Fmt(0, 7)                                             # no integer bit: check_ham_hop refuses
    assert call(bad_att) == abi.QMANN_EUNSUPPORTED
    assert call(variant(dim_emb_pad=96)) == abi.QMANN_EUNSUPPORTED
    assert call(keys=None) == abi.QMANN_EINVAL and call(vals=None) == abi.QMANN_EINVAL
    assert call(u0=None) == abi.QMANN_EINVAL and call(out=None) == abi.QMANN_EINVAL
    assert call(net_null=True) == abi.QMANN_EINVAL
    assert call(key_off=8) == abi.QMANN_EINVAL                                 # planes not 16-byte aligned
    assert call(n_slots=0) == abi.QMANN_EINVAL
    assert call(ks=S * (Dp // 64) * nb * 8, vs=0) == abi.QMANN_EINVAL          # strides that do not describe the same rows
    assert call(ks=0, vs=S * Dp) == abi.QMANN_EINVAL
    assert call(n_query=1 << 24) == abi.QMANN_ERANGE
    if split:
        assert call(ws_ptr=0) == abi.QMANN_EINVAL
        assert call(ws_ptr=ws.data_ptr() + 8) == abi.QMANN_EINVAL
        assert call(ws_bytes=need - 1) == abi.QMANN_EINVAL
        assert call(n_slots=(1 << 24) + 1) == abi.QMANN_ERANGE
    else:
        assert abi.lib.qmann_hops_shared_packed_lds_bytes(C.byref(net.net), 90000, 1) > LDS_LIMIT
        assert call(n_slots=90000) == abi.QMANN_ERANGE
    assert call(n_query=0) == abi.QMANN_OK
    # the base call's answers come first: a fault of each kind in one call gives the base call's code
    assert call(variant(attention_mode=2), k=0) == abi.QMANN_EUNSUPPORTED
    assert call(n_query=1 << 24, k=17) == abi.QMANN_ERANGE and call(key_off=8, top_p=None) == abi.QMANN_EINVAL
    assert call(bad_att, top_slot=None) == abi.QMANN_EUNSUPPORTED
    assert call(n_query=0, k=0) == abi.QMANN_OK and call(n_query=0, top_slot=None) == abi.QMANN_OK
    if split:
        assert call(n_slots=(1 << 24) + 1, k=0) == abi.QMANN_ERANGE
    else:
        assert call(n_slots=90000, k=0) == abi.QMANN_ERANGE
    torch.cuda.synchronize()
    assert (u_out == -77.0).all() and (slot == -7).all() and (tp == -7.0).all()       # none of them launched anything
    # one good call; k = 16 is no error, nor would k > S be
    assert call() == abi.QMANN_OK
    torch.cuda.synchronize()
    probs, u_plain = reference(env, "tied_v1", case)
    assert torch.equal(u_out, u_plain)
    assert_rows(slot, tp, probs, K, "tied_v1")
    slot16 = torch.full((B, H, 16), -7, dtype=torch.int32, device=env.dev)
    tp16 = torch.full((B, H, 16), -7.0, dtype=torch.float32, device=env.dev)
    assert call(k=16, top_slot=slot16, top_p=tp16) == abi.QMANN_OK
    torch.cuda.synchronize()
    assert_rows(slot16, tp16, probs, 16, "tied_v1")


# ---- 6. the model ---------------------------------------------------------------------------------------------------------------------
def _qnet_of(env, cfg, wts, hm):
    torch, model = env.torch, env.model
    net = model.QNet.from_model(cfg, hm)
    net.w_q, net.w_a, net.w_c = [torch.from_numpy(wts["w_q"]).to(env.dev), [torch.from_numpy(w).to(env.dev) for w in wts["w_a"]],
                                 [torch.from_numpy(w).to(env.dev) for w in wts["w_c"]]]
    net.make_tables()
    return net


@pytest.mark.parametrize("N", MODEL_N)
@pytest.mark.parametrize("mode,num_bit", [(10, 8), (10, 2), (11, 8), (11, 2)])
@pytest.mark.parametrize("which", MODEL_SOURCES)
def test_ask_words_top_packed(env, force_qt, which, mode, num_bit, N):
    """the memory is one of the set's longest stories, the questions those of N other stories (shared_ham_cases.py).  Yardstick:
    the probs tap of QNet.hops_shared_packed on the model's own memory; pred, match, last_u and last_topk are those of ask_words"""
    force_qt(None)
    torch, model = env.torch, env.model
    cfg, wts, *_ = model_inputs(which, mode, num_bit)
    story, q_sel, a_sel, _ = model_story_and_questions(which, mode, num_bit, N)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(env.dev)
    d_story, d_q = up(story), up(q_sel)
    d_ans = torch.from_numpy(a_sel.astype(np.int32)).to(env.dev)
    S, K = story.shape[0], 5

    plain = model.HostModel(cfg, wts, device="cuda:0")
    plain.memorize_words(d_story)
    pred2, cost2, match2 = plain.ask_words(d_q, d_ans)
    torch.cuda.synchronize()
    u2, rank2 = plain.last_u(N), plain.last_topk(3)
    torch.cuda.synchronize()

    hm = model.HostModel(cfg, wts, device="cuda:0")
    net = _qnet_of(env, cfg, wts, hm)
    dk, dv, du0 = net.embed_idx(d_story, d_q)
    _, taps = net.hops_shared_packed(net.pack_planes(dk, num_bit), dv, S, du0, taps=True)
    torch.cuda.synchronize()
    probs = taps.probs.cpu().numpy()
    hm.memorize_words(d_story)
    pred, cost, match, slot, p = hm.ask_words_top_packed(d_q, K, d_ans)
    torch.cuda.synchronize()
    what = f"{which}, mode {mode}, {num_bit} bits, N={N}"
    assert torch.equal(pred, pred2) and int(match.item()) == int(match2.item()), what
    assert torch.equal(hm.last_u(N), u2), what
    assert float(cost.item()) == pytest.approx(float(cost2.item()), rel=1e-4, abs=1e-3)      # float atomics: the order of the adds differs
    assert_rows(slot, p, probs, K, what)
    rank = hm.last_topk(3)
    torch.cuda.synchronize()
    assert torch.equal(rank[0], rank2[0]) and torch.equal(rank[1], rank2[1]), what
    assert float(u2.abs().sum()) > 0
    hm.close(); plain.close()


@pytest.fixture(scope="module")
def long_story(env):
    """80 017 rows of words, the construction of test_gpu_shared_split_ham.py's long_story; on the device, made once"""
    from test_gpu_graph import _words
    from test_gpu_shared_split_ham import DD_, LONG_ROWS, V_
    return env.torch.from_numpy(_words(np.random.default_rng(79), LONG_ROWS, V_, DD_, 8, True).view(np.int16)).to(env.dev)


@pytest.mark.parametrize("mode,num_bit", [(11, 8), (10, 4)])
def test_ask_words_top_packed_in_chunks_beyond_the_lds_cap(env, force_qt, long_story, mode, num_bit):
    """a memory of 80 017 rows: only the split call can ask it, so every ask below goes through
    qmann_hops_shared_split_top_packed.  7 questions under budgets of 64 shares (one chunk), 2 shares (chunks of 2 + 2 + 2 + 1)
    and 1 share (seven chunks): each chunk must write its own block of both outputs.  Yardstick: the probs tap of
    hops_shared_split_packed on the same words; pred, last_u and last_topk are those of ask_words"""
    from test_gpu_shared_split_ham import LONG_ROWS, _model_cfg_weights, _questions
    force_qt(None)
    torch, abi, model = env.torch, env.abi, env.model
    cfg, wts = _model_cfg_weights(env, mode, num_bit)
    N, K = 7, 5
    qw, ans = _questions(env, 83, N)
    hm, plain = model.HostModel(cfg, wts, device="cuda:0"), model.HostModel(cfg, wts, device="cuda:0")
    net_c = hm.net_and_w_ans()[0]
    # without the opt-in the memory is refused: what is asked below cannot have taken the unsplit call
    assert abi.lib.qmann_model_memorize_words(hm.h, C.c_void_p(long_story.data_ptr()), LONG_ROWS, long_story.shape[1], None) == abi.QMANN_ERANGE
    assert abi.lib.qmann_hops_shared_packed_lds_bytes(C.byref(net_c), LONG_ROWS, 1) > LDS_LIMIT
    share = abi.lib.qmann_hops_shared_split_packed_ws_bytes(C.byref(net_c), LONG_ROWS, 1)

    plain.enable_split_asks_packed(64 * share)
    plain.memorize_words(long_story)
    pred2, cost2, match2 = plain.ask_words(qw, ans)
    torch.cuda.synchronize()
    u2, rank2 = plain.last_u(N), plain.last_topk(3)
    torch.cuda.synchronize()

    net = _qnet_of(env, cfg, wts, hm)
    dk, dv, du0 = net.embed_idx(long_story, qw)
    u_pub, taps = net.hops_shared_split_packed(net.pack_planes(dk, num_bit), dv, LONG_ROWS, du0, n_slices=7, taps=True)
    torch.cuda.synchronize()
    probs = taps.probs.cpu().numpy()
    assert torch.equal(u_pub, u2)
    rows = []
    for budget in (64 * share, 2 * share, share):
        hm.enable_split_asks_packed(budget)
        if hm.memory_rows() == 0:
            hm.memorize_words(long_story)
        assert hm.memory_rows() == LONG_ROWS
        pred, cost, match, slot, p = hm.ask_words_top_packed(qw, K, ans)
        torch.cuda.synchronize()
        what = f"mode {mode}: budget of {budget // share} shares"
        assert torch.equal(pred, pred2) and int(match.item()) == int(match2.item()), what
        assert torch.equal(hm.last_u(N), u2), what
        assert float(cost.item()) == pytest.approx(float(cost2.item()), rel=1e-4, abs=1e-3)      # float atomics: the order of the adds differs
        assert_rows(slot, p, probs, K, what)
        rank = hm.last_topk(3)
        torch.cuda.synchronize()
        assert torch.equal(rank[0], rank2[0]) and torch.equal(rank[1], rank2[1]), what
        rows.append(slot.cpu().numpy())
    assert len({r.tobytes() for r in rows[0]}) > 1                   # (the questions' blocks differ: a misplaced block would show)
    assert float(u2.abs().sum()) > 0
    hm.close(); plain.close()


def test_ask_words_top_packed_refusals(env):
    torch, abi, model = env.torch, env.abi, env.model
    cfg, wts, sw, qw, n_sen, _ = model_inputs("random_joint20", 11, 8)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(env.dev)
    d_story, d_q = up(sw[:5]), up(qw[:4])
    H, K = cfg["n_hop"], 5
    pred = torch.full((4,), -7, dtype=torch.int32, device=env.dev)
    slot = torch.full((4, H, K), -7, dtype=torch.int32, device=env.dev)
    tp = torch.full((4, H, K), -7.0, dtype=torch.float32, device=env.dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def ask(hm, k=K, top_slot=slot, top_p=tp, fn=abi.lib.qmann_model_ask_words_top_packed, words=d_q, out=pred, n_query=4):
        return fn(hm.h, p(words), d_q.shape[1], n_query, None, p(out), None, None, k, p(top_slot), p(top_p), None)
    fixed = model.HostModel(dict(cfg, attention_mode=2), wts, device="cuda:0")
    assert ask(fixed) == abi.QMANN_EINVAL                         # nothing memorised: qmann_model_ask_words' answer, first
    fixed.memorize_words(d_story)
    assert ask(fixed) == abi.QMANN_EUNSUPPORTED                   # a QMANN_ATT_FIXED model
    assert ask(fixed, k=0) == abi.QMANN_EUNSUPPORTED              # ... before a bad k
    fixed.close()
    hm = model.HostModel(cfg, wts, device="cuda:0")
    assert ask(hm) == abi.QMANN_EINVAL                            # nothing memorised
    hm.memorize_words(d_story)
    assert ask(hm, fn=abi.lib.qmann_model_ask_words_top) == abi.QMANN_EUNSUPPORTED      # the fixed-point form STILL refuses a Hamming model
    assert ask(hm, k=0) == abi.QMANN_EINVAL and ask(hm, k=17) == abi.QMANN_EINVAL
    assert ask(hm, top_slot=None) == abi.QMANN_EINVAL and ask(hm, top_p=None) == abi.QMANN_EINVAL
    assert ask(hm, words=None) == abi.QMANN_EINVAL and ask(hm, out=None, k=0) == abi.QMANN_EINVAL
    # n_query = 0 is answered as qmann_model_ask_words answers it, whatever k
    assert ask(hm, n_query=0, k=0, top_slot=None, top_p=None) == abi.QMANN_OK
    torch.cuda.synchronize()
    assert (pred == -7).all() and (slot == -7).all() and (tp == -7.0).all()
    assert ask(hm) == abi.QMANN_OK
    torch.cuda.synchronize()
    assert (pred != -7).all() and (slot != -7).all()
    hm.close()


# ---- 7. graph capture -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,num_bit", [(10, 8), (11, 4)])
def test_ask_words_top_packed_replays_from_a_captured_graph(env, force_qt, mode, num_bit):
    """pattern of test_ask_words_replays_from_a_captured_graph (test_gpu_shared_ham.py): one eager ask grows the question
    workspace, the captured ask (a single branch on one stream) replays on new questions in the graph's buffers and gives an eager
    model's rows"""
    from test_gpu_graph import _words
    force_qt(None)
    torch, model = env.torch, env.model
    dev = env.dev
    rng = np.random.default_rng(78)
    V, dd, D, H, B, R, K = 40, 30, 60, 3, 333, 23, 5
    cfg = model.babi_cfg(V, mode, 0, iwl=5, en_mq=True)
    cfg["num_bit"] = num_bit
    wts = {"w_q": rng.normal(0, 1.0, (D, V)).astype(np.float32), "w_ans": rng.normal(0, 0.3, (V, D)).astype(np.float32),
           "w_a": [rng.normal(0, 1.0, (D, V)).astype(np.float32) for _ in range(H)],
           "w_c": [rng.normal(0, 1.0, (D, V)).astype(np.float32) for _ in range(H)],
           "w_h": [rng.normal(0, 1.0, (D, D)).astype(np.float32) for _ in range(H)]}

    def questions(seed):
        r = np.random.default_rng(seed)
        return (torch.from_numpy(_words(r, B, V, dd, 8, False).view(np.int16)).to(dev),
                torch.from_numpy(r.integers(0, V, B).astype(np.int32)).to(dev))
    story = torch.from_numpy(_words(np.random.default_rng(1), R, V, dd, 8, True).view(np.int16)).to(dev)
    s = torch.cuda.Stream(device=dev)
    hm = model.HostModel(cfg, wts, device="cuda:0", stream=s.cuda_stream)
    eager = model.HostModel(cfg, wts, device="cuda:0")
    eager.memorize_words(story)
    qw, ans = questions(1)
    with torch.cuda.stream(s):
        hm.memorize_words(story)
        hm.ask_words_top_packed(qw, K, ans)                                       # warm-up: the question workspace takes its size
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        pred, cost, match, slot, p = hm.ask_words_top_packed(qw, K, ans)          # captured, not run
    for seed in (2, 3):
        nqw, nans = questions(seed)
        qw.copy_(nqw); ans.copy_(nans)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        p2, c2, m2, slot2, tp2 = eager.ask_words_top_packed(nqw, K, nans)
        torch.cuda.synchronize()
        assert torch.equal(pred, p2) and torch.equal(hm.last_u(B), eager.last_u(B)), seed
        assert torch.equal(slot, slot2) and torch.equal(p.view(torch.int32), tp2.view(torch.int32)), seed
        assert int(match.item()) == int(m2.item()) and float(cost.item()) == pytest.approx(float(c2.item()), rel=1e-5)
    assert len({int(x) for x in slot[:, 0, 0].cpu().numpy()}) > 1                 # (not one row for every question)
    hm.close(); eager.close()

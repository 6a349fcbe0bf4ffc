"""Attended slots: qmann_hops_shared_top_i8 / qmann_hops_shared_split_top_i8 / qmann_model_ask_words_top (csrc/hops_attended.h).

The yardstick everywhere is the `probs` tap of the EXISTING call on the same inputs, ordered by "larger probability first, equal
probabilities: lower slot first" (attended_cases.want_rows).  Nothing is excused: slots are compared exactly, probabilities by
bit pattern, u_out with torch.equal against the plain call.

1. every case of shared_cases.py, k in {1, 5, 16}; 2. forced tiles; 3. planted ties and all-zero memories; 4. the split call,
memories beyond the LDS cap included; 5. return codes, nothing launched, the base call's refusals first; 6. the model's ask,
unsplit on bAbI stories and in chunks through the split call on a memory of 160 001 rows; 7. replay from a captured graph."""
import ctypes as C

import numpy as np
import pytest

from attended_cases import PAD_SLOT, PLANT_NEG, PLANT_POS, PLANT_S, ZERO_S, assert_rows, planted_case, want_rows, zero_case
from conftest import load_pkg
from shared_cases import CASES, shared_case
from shared_split_cases import long_case

pytestmark = pytest.mark.gpu

KS = (1, 5, 16)


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


_REF = {}


def reference(env, key, case, split=False):
    """(taps as numpy: probs [H][B][S], score_codes; u_out of the plain call) of the EXISTING call on a case -- computed once per
    process under the launcher's own tile and left unchanged"""
    if key not in _REF:
        net, dk, dv, du0 = device_case(env, case)
        run = net.hops_shared_split if split else net.hops_shared
        _, taps = run(dk, dv, case["S"], du0, taps=True)
        u_plain = run(dk, dv, case["S"], du0)
        env.torch.cuda.synchronize()
        probs, codes = taps.probs.cpu().numpy(), taps.score_codes.cpu().numpy()
        probs.setflags(write=False)
        _REF[key] = (probs, codes, u_plain.clone())
    return _REF[key]


# ---- 1. every shared case ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_top_equals_the_sorted_tap(env, force_qt, name):
    force_qt(None)
    case = shared_case(name)
    probs, _, u_plain = reference(env, name, case)
    net, dk, dv, du0 = device_case(env, case)
    for k in KS:
        u, slot, p = net.hops_shared_top(dk, dv, case["S"], du0, k)
        env.torch.cuda.synchronize()
        assert env.torch.equal(u, u_plain), f"{name}: u_out, k={k}"
        assert_rows(slot, p, probs, k, name)


# ---- 2. forced tiles ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qt", [1, 2, 4, 8])
@pytest.mark.parametrize("name", ["tiles", "config4_q25"])
def test_top_with_forced_tiles(env, force_qt, name, qt):
    case = shared_case(name)
    force_qt(None)
    probs, _, u_plain = reference(env, name, case)
    force_qt(qt)
    assert env.abi.lib.qmann_hops_shared_tile(case["S"], case["n_query"]) == qt
    net, dk, dv, du0 = device_case(env, case)
    u, slot, p = net.hops_shared_top(dk, dv, case["S"], du0, 16)
    env.torch.cuda.synchronize()
    assert env.torch.equal(u, u_plain)
    assert_rows(slot, p, probs, 16, f"{name}, tiles of {qt}")


# ---- 3. planted ties ------------------------------------------------------------------------------------------------------------------
def _assert_planted_tap(probs, codes, base):
    """what the tests below rely on, asserted on the EXISTING kernel's tap at hop 0: the planted rows saturate at +-127, every
    other row scores 0; three probability levels (exp_plan: two, its zero region joins the zero rows and the negative ones)"""
    others = np.setdiff1d(np.arange(PLANT_S), PLANT_POS + PLANT_NEG)
    for q in range(probs.shape[1]):
        c, p = codes[0, q], probs[0, q]
        assert (c[PLANT_POS] == 127).all() and (c[PLANT_NEG] == -127).all() and (c[others] == 0).all()
        top, zero, neg = p[PLANT_POS[0]], p[others[0]], p[PLANT_NEG[0]]
        assert (p[PLANT_POS].view(np.uint32) == top.view(np.uint32)).all() and (p[others] == zero).all() and (p[PLANT_NEG] == neg).all()
        assert top == p.max() and top > zero
        if base == 2:
            assert zero == 0.0 and neg == 0.0                  # different bins, equal floats
        else:
            assert zero > neg


@pytest.mark.parametrize("base", [0, 1, 2])
def test_planted_ties(env, force_qt, base):
    force_qt(None)
    case = planted_case(base)
    probs, codes, u_plain = reference(env, ("planted", base), case)
    _assert_planted_tap(probs, codes, base)
    net, dk, dv, du0 = device_case(env, case)
    # exp_plan: rows 1 and 3 tie with their neighbours and come in index order; e^x and 2^x: they come after every zero row
    tail = list(range(10)) if base == 2 else [0, 2, 4, 5, 6, 7, 8, 9, 10, 11]
    for k, want0 in ((5, PLANT_POS[:5]), (16, PLANT_POS + tail)):
        u, slot, p = net.hops_shared_top(dk, dv, PLANT_S, du0, k)
        env.torch.cuda.synchronize()
        assert env.torch.equal(u, u_plain)
        got = slot.cpu().numpy().view(np.uint32)
        for q in range(case["n_query"]):
            assert got[q, 0].tolist() == want0, f"base {base}, k={k}, q{q}"
        assert_rows(slot, p, probs, k, f"planted, base {base}")


@pytest.mark.parametrize("S", ZERO_S)
def test_all_zero_memory(env, force_qt, S):
    force_qt(None)
    case = zero_case(S)
    probs, _, u_plain = reference(env, ("zero", S), case)
    assert (probs == probs[0, 0, 0]).all()
    net, dk, dv, du0 = device_case(env, case)
    for k in KS:
        u, slot, p = net.hops_shared_top(dk, dv, S, du0, k)
        env.torch.cuda.synchronize()
        n = min(k, S)
        got = slot.cpu().numpy().view(np.uint32)
        assert (got[:, :, :n] == np.arange(n, dtype=np.uint32)).all() and (got[:, :, n:] == PAD_SLOT).all()
        assert env.torch.equal(u, u_plain)
        assert_rows(slot, p, probs, k, f"zero memory S={S}")


# ---- 4. the split call ------------------------------------------------------------------------------------------------------------------
SPLIT_NAMES = ["config4_q25", "tiles", "en_mq_clamp", "wl6", "tied", "tied_short", "eight_hops", "binary_relu", "grid_S17_D256_q5",
               "grid_S64_D60_q5", "grid_S1_D60_q1", "grid_S4097_D256_q17", "exp_plan", "pow2_shift", "scale_negative"]


def _split_against_unsplit(env, key, case, ks):
    torch = env.torch
    probs, _, u_plain = reference(env, key, case)
    net, dk, dv, du0 = device_case(env, case)
    S = case["S"]
    for k in ks:
        u1, slot1, p1 = net.hops_shared_top(dk, dv, S, du0, k)
        for n_slices in (1, 2, 0):
            u, slot, p = net.hops_shared_split_top(dk, dv, S, du0, k, n_slices=n_slices)
            torch.cuda.synchronize()
            what = f"{key}, n_slices={n_slices}, k={k}"
            assert torch.equal(u, u_plain), what
            assert torch.equal(slot, slot1) and torch.equal(p.view(torch.int32), p1.view(torch.int32)), what
            assert_rows(slot, p, probs, k, what)


@pytest.mark.parametrize("name", SPLIT_NAMES)
def test_split_top_equals_the_unsplit_call(env, force_qt, name):
    force_qt(None)
    _split_against_unsplit(env, name, shared_case(name), (5, 16))


@pytest.mark.parametrize("base", [0, 1, 2])
def test_split_top_planted_ties(env, force_qt, base):
    force_qt(None)
    _split_against_unsplit(env, ("planted", base), planted_case(base), (5, 16))


@pytest.mark.parametrize("S", ZERO_S)
def test_split_top_all_zero_memory(env, force_qt, S):
    """every p equal: the walk ends at its first chunk, and k > S pads, with the score bytes read from the workspace"""
    force_qt(None)
    case = zero_case(S)
    _split_against_unsplit(env, ("zero", S), case, KS)
    net, dk, dv, du0 = device_case(env, case)
    for n_slices in (1, 2, 0):
        _, slot, _ = net.hops_shared_split_top(dk, dv, S, du0, 16, n_slices=n_slices)
        env.torch.cuda.synchronize()
        n = min(16, S)
        got = slot.cpu().numpy().view(np.uint32)
        assert (got[:, :, :n] == np.arange(n, dtype=np.uint32)).all() and (got[:, :, n:] == PAD_SLOT).all()


@pytest.mark.parametrize("name", ["long_exp", "long_pow2"])
def test_split_top_beyond_the_lds_cap(env, force_qt, name):
    """S > 150 000: only the split call runs; its own probs tap is the yardstick"""
    force_qt(None)
    torch = env.torch
    case = long_case(name)
    S = case["S"]
    probs, _, u_plain = reference(env, name, case, split=True)
    net, dk, dv, du0 = device_case(env, case)
    for k, n_slices in ((5, 0), (16, 7)):
        u, slot, p = net.hops_shared_split_top(dk, dv, S, du0, k, n_slices=n_slices)
        torch.cuda.synchronize()
        assert torch.equal(u, u_plain)
        assert_rows(slot, p, probs, k, f"{name}, n_slices={n_slices}")


# ---- 5. return codes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("split", [False, True])
def test_return_codes(env, force_qt, split):
    force_qt(None)
    torch, abi, model = env.torch, env.abi, env.model
    case = shared_case("tied_short")
    S, B, H, K = case["S"], case["n_query"], case["cfg"]["n_hop"], 5
    net, dk, dv, du0 = device_case(env, case)
    u_out = torch.full_like(du0, -77.0)
    slot = torch.full((B, H, K), -7, dtype=torch.int32, device=env.dev)
    tp = torch.full((B, H, K), -7.0, dtype=torch.float32, device=env.dev)
    need = abi.lib.qmann_hops_shared_split_ws_bytes(C.byref(net.net), S, B)
    ws = torch.zeros(need + 16, dtype=torch.uint8, device=env.dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(n=None, keys=dk, vals=dv, u0=du0, out=u_out, n_slots=S, n_query=B, k=K, top_slot=slot, top_p=tp, net_null=False,
             ws_ptr=ws.data_ptr(), ws_bytes=need):
        nref = None if net_null else C.byref(n if n is not None else net.net)
        if split:
            return abi.lib.qmann_hops_shared_split_top_i8(nref, p(keys), p(vals), 0, n_slots, p(u0), p(out), k, p(top_slot), p(top_p),
                                                          n_query, 0, C.c_void_p(ws_ptr) if ws_ptr else None, ws_bytes, None)
        return abi.lib.qmann_hops_shared_top_i8(nref, p(keys), p(vals), 0, n_slots, p(u0), p(out), k, p(top_slot), p(top_p), n_query, None)

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
    # every refusal of the base call
    for mode in (1, 3, 10, 11):
        assert call(variant(attention_mode=mode)) == abi.QMANN_EUNSUPPORTED
    assert call(variant(dim_emb_pad=96)) == abi.QMANN_EUNSUPPORTED
    assert call(n_slots=0) == abi.QMANN_EINVAL
    assert call(keys=None) == abi.QMANN_EINVAL and call(vals=None) == abi.QMANN_EINVAL
    assert call(u0=None) == abi.QMANN_EINVAL and call(out=None) == abi.QMANN_EINVAL
    assert call(net_null=True) == abi.QMANN_EINVAL
    wide = variant()
    wide.att[0] = abi.Fmt(5, 4)                                   # word length 9
    assert call(wide) == abi.QMANN_ERANGE
    assert call(n_query=1 << 24) == abi.QMANN_ERANGE
    if split:
        assert call(ws_ptr=0) == abi.QMANN_EINVAL
        assert call(ws_ptr=ws.data_ptr() + 8) == abi.QMANN_EINVAL
        assert call(ws_bytes=need - 1) == abi.QMANN_EINVAL
        assert call(n_slots=(1 << 24) + 1) == abi.QMANN_ERANGE
    else:
        assert abi.lib.qmann_hops_shared_lds_bytes(160000, 1) > 160 * 1024 - 1024
        assert call(n_slots=160000) == abi.QMANN_ERANGE
    assert call(n_query=0) == abi.QMANN_OK
    # the base call's answers come first (the header says so): a fault of each kind in one call gives the base call's code
    assert call(variant(attention_mode=1), k=0) == abi.QMANN_EUNSUPPORTED
    assert call(n_query=1 << 24, k=17) == abi.QMANN_ERANGE and call(wide, top_p=None) == abi.QMANN_ERANGE
    assert call(n_query=0, k=0) == abi.QMANN_OK and call(n_query=0, top_slot=None) == abi.QMANN_OK
    if not split:
        assert call(n_slots=160000, k=0) == abi.QMANN_ERANGE
    torch.cuda.synchronize()
    assert (u_out == -77.0).all() and (slot == -7).all() and (tp == -7.0).all()       # none of them launched anything
    # one good call; k = 16 > S = 9 is no error
    assert call() == abi.QMANN_OK
    torch.cuda.synchronize()
    probs, _, u_plain = reference(env, "tied_short", case)
    assert torch.equal(u_out, u_plain)
    assert_rows(slot, tp, probs, K, "tied_short")
    slot16 = torch.full((B, H, 16), -7, dtype=torch.int32, device=env.dev)
    tp16 = torch.full((B, H, 16), -7.0, dtype=torch.float32, device=env.dev)
    assert call(k=16, top_slot=slot16, top_p=tp16) == abi.QMANN_OK
    torch.cuda.synchronize()
    assert_rows(slot16, tp16, probs, 16, "tied_short")


# ---- 6. the model ---------------------------------------------------------------------------------------------------------------------
def _qnet_of(env, cfg, wts, hm):
    torch, model = env.torch, env.model
    net = model.QNet.from_model(cfg, hm)
    net.w_q, net.w_a, net.w_c = [torch.from_numpy(wts["w_q"]).to(env.dev), [torch.from_numpy(w).to(env.dev) for w in wts["w_a"]],
                                 [torch.from_numpy(w).to(env.dev) for w in wts["w_c"]]]
    net.make_tables()
    return net


@pytest.mark.parametrize("N", [1, 7, 4099])
@pytest.mark.parametrize("which", ["trained_qa1", "random_joint20"])
def test_ask_words_top(env, force_qt, which, N):
    """the memory is the set's longest story, the questions those of N other stories.  A story of this length fits LDS, so the
    ask is the unsplit call, also once split asks are enabled (they leave short memories as they are: the second round pins
    that the rows do not change with the opt-in); the chunked path is test_ask_words_top_in_chunks_beyond_the_lds_cap"""
    from test_gpu_shared import _model_inputs
    force_qt(None)
    torch, abi, model = env.torch, env.abi, env.model
    cfg, wts, sw, qw, n_sen, ans = _model_inputs(which, env)
    offs = np.concatenate([[0], np.cumsum(n_sen)])
    s = int(np.argmax(n_sen))
    story = sw[offs[s]:offs[s + 1]]
    S, K = story.shape[0], 5
    others = (s + 1 + np.arange(N)) % len(n_sen)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(env.dev)
    d_story, d_q = up(story), up(qw[others])
    d_ans = torch.from_numpy(ans[others].astype(np.int32)).to(env.dev)

    plain = model.HostModel(cfg, wts, device="cuda:0")
    plain.memorize_words(d_story)
    pred2, cost2, match2 = plain.ask_words(d_q, d_ans)
    torch.cuda.synchronize()
    u2, rank2 = plain.last_u(N), plain.last_topk(3)
    torch.cuda.synchronize()

    hm = model.HostModel(cfg, wts, device="cuda:0")
    net = _qnet_of(env, cfg, wts, hm)
    dk, dv, du0 = net.embed_idx(d_story, d_q)
    _, taps = net.hops_shared(dk, dv, S, du0, taps=True)
    torch.cuda.synchronize()
    probs = taps.probs.cpu().numpy()
    hm.memorize_words(d_story)
    share = abi.lib.qmann_hops_shared_split_ws_bytes(C.byref(hm.net_and_w_ans()[0]), S, 1)
    for budget in (0, 2 * share + 64):
        if budget:
            hm.enable_split_asks(budget)
            assert hm.memory_rows() == S
        pred, cost, match, slot, p = hm.ask_words_top(d_q, K, d_ans)
        torch.cuda.synchronize()
        what = f"{which}, N={N}, budget={budget}"
        assert torch.equal(pred, pred2) and int(match.item()) == int(match2.item()), what
        assert torch.equal(hm.last_u(N), u2), what
        assert float(cost.item()) == pytest.approx(float(cost2.item()), rel=1e-4, abs=1e-3)      # float atomics: the order of the adds differs
        assert_rows(slot, p, probs, K, what)
        rank = hm.last_topk(3)
        torch.cuda.synchronize()
        assert torch.equal(rank[0], rank2[0]) and torch.equal(rank[1], rank2[1]), what
    assert float(u2.abs().sum()) > 0
    hm.close(); plain.close()


LONG_ROWS = 160001


def test_ask_words_top_in_chunks_beyond_the_lds_cap(env, force_qt):
    """a memory of 160 001 rows (test_gpu_shared_split.py's model and story): only the split call can ask it, so every ask below
    goes through qmann_hops_shared_split_top_i8.  7 questions under budgets of 64 shares (one chunk), 2 shares (chunks of 2 + 2 +
    2 + 1) and 1 share (seven chunks): each chunk must write its own block of both outputs.  Yardstick: the probs tap of
    hops_shared_split on the same words; pred, last_u and last_topk are those of ask_words"""
    from test_gpu_graph import _words
    from test_gpu_shared_split import _model_cfg_weights, _questions
    force_qt(None)
    torch, abi, model = env.torch, env.abi, env.model
    cfg, wts = _model_cfg_weights(env)
    story = torch.from_numpy(_words(np.random.default_rng(79), LONG_ROWS, 40, 30, 8, True).view(np.int16)).to(env.dev)
    N, K = 7, 5
    qw, ans = _questions(env, 83, N)
    hm, plain = model.HostModel(cfg, wts, device="cuda:0"), model.HostModel(cfg, wts, device="cuda:0")
    # without the opt-in the memory is refused: what is asked below cannot have taken the unsplit call
    assert abi.lib.qmann_model_memorize_words(hm.h, C.c_void_p(story.data_ptr()), LONG_ROWS, story.shape[1], None) == abi.QMANN_ERANGE
    assert abi.lib.qmann_hops_shared_lds_bytes(LONG_ROWS, 1) > 160 * 1024 - 1024
    share = abi.lib.qmann_hops_shared_split_ws_bytes(C.byref(hm.net_and_w_ans()[0]), LONG_ROWS, 1)

    plain.enable_split_asks(64 * share)
    plain.memorize_words(story)
    pred2, cost2, match2 = plain.ask_words(qw, ans)
    torch.cuda.synchronize()
    u2, rank2 = plain.last_u(N), plain.last_topk(3)
    torch.cuda.synchronize()

    net = _qnet_of(env, cfg, wts, hm)
    dk, dv, du0 = net.embed_idx(story, qw)
    u_pub, taps = net.hops_shared_split(dk, dv, LONG_ROWS, du0, n_slices=7, taps=True)
    torch.cuda.synchronize()
    probs = taps.probs.cpu().numpy()
    assert torch.equal(u_pub, u2)
    rows = []
    for budget in (64 * share, 2 * share, share):
        hm.enable_split_asks(budget)
        if hm.memory_rows() == 0:
            hm.memorize_words(story)
        assert hm.memory_rows() == LONG_ROWS
        pred, cost, match, slot, p = hm.ask_words_top(qw, K, ans)
        torch.cuda.synchronize()
        what = f"budget of {budget // share} shares"
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


def test_ask_words_top_refusals(env):
    from test_gpu_shared import _model_inputs
    torch, abi, model = env.torch, env.abi, env.model
    cfg, wts, sw, qw, n_sen, _ = _model_inputs("random_joint20", env)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(env.dev)
    d_story, d_q = up(sw[:5]), up(qw[:4])
    H, K = cfg["n_hop"], 5
    pred = torch.full((4,), -7, dtype=torch.int32, device=env.dev)
    slot = torch.full((4, H, K), -7, dtype=torch.int32, device=env.dev)
    tp = torch.full((4, H, K), -7.0, dtype=torch.float32, device=env.dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def ask(hm, k=K, top_slot=slot, top_p=tp):
        return abi.lib.qmann_model_ask_words_top(hm.h, p(d_q), d_q.shape[1], 4, None, p(pred), None, None, k, p(top_slot), p(top_p), None)
    ham = model.HostModel(dict(cfg, attention_mode=11, num_bit=4), wts, device="cuda:0")
    ham.memorize_words(d_story)
    assert ask(ham) == abi.QMANN_EUNSUPPORTED
    ham.close()
    hm = model.HostModel(cfg, wts, device="cuda:0")
    assert ask(hm) == abi.QMANN_EINVAL                            # nothing memorised
    hm.memorize_words(d_story)
    assert ask(hm, k=0) == abi.QMANN_EINVAL and ask(hm, k=17) == abi.QMANN_EINVAL
    assert ask(hm, top_slot=None) == abi.QMANN_EINVAL and ask(hm, top_p=None) == abi.QMANN_EINVAL
    # n_query = 0 is answered as qmann_model_ask_words answers it, whatever k
    assert abi.lib.qmann_model_ask_words_top(hm.h, p(d_q), d_q.shape[1], 0, None, p(pred), None, None, 0, None, None, None) == abi.QMANN_OK
    torch.cuda.synchronize()
    assert (pred == -7).all() and (slot == -7).all() and (tp == -7.0).all()
    assert ask(hm) == abi.QMANN_OK
    torch.cuda.synchronize()
    assert (pred != -7).all() and (slot != -7).all()
    hm.close()


# ---- 7. graph capture -------------------------------------------------------------------------------------------------------------------
def test_ask_words_top_replays_from_a_captured_graph(env, force_qt):
    """pattern of test_forward_shared_words_replays_from_a_captured_graph: one eager ask grows the question workspace, the captured
    ask replays on new questions in the graph's buffers and gives an eager model's rows"""
    from test_gpu_graph import _words
    force_qt(None)
    torch, model = env.torch, env.model
    dev = env.dev
    rng = np.random.default_rng(77)
    V, dd, D, H, B, R, K = 40, 30, 60, 3, 333, 23, 5
    cfg = model.babi_cfg(V, 2, 0, iwl=5, en_mq=True)
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
        hm.ask_words_top(qw, K, ans)                                              # warm-up: the question workspace takes its size
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        pred, cost, match, slot, p = hm.ask_words_top(qw, K, ans)                 # captured, not run
    for seed in (2, 3, 4):
        nqw, nans = questions(seed)
        qw.copy_(nqw); ans.copy_(nans)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        p2, c2, m2, slot2, tp2 = eager.ask_words_top(nqw, K, nans)
        torch.cuda.synchronize()
        assert torch.equal(pred, p2) and torch.equal(hm.last_u(B), eager.last_u(B)), seed
        assert torch.equal(slot, slot2) and torch.equal(p.view(torch.int32), tp2.view(torch.int32)), seed
        assert int(match.item()) == int(m2.item()) and float(cost.item()) == pytest.approx(float(c2.item()), rel=1e-5)
    assert len({int(x) for x in slot[:, 0, 0].cpu().numpy()}) > 1                 # (not one row for every question)
    hm.close(); eager.close()

"""Attended slots per story: qmann_hops_top_i8 / qmann_model_forward_words_top (csrc/hops_attended_story.h).

The yardstick everywhere is the `probs` tap of the EXISTING qmann_hops_i8 on the same inputs, sliced per story, cut to max_slots
and ordered by "larger probability first, equal probabilities: lower slot first" (attended_cases.want_rows through
attended_story_cases.want_story_rows).  Nothing is excused: slots are compared exactly, probabilities by bit pattern, u_out with
torch.equal against the tapped call.

1. the one-wavefront kernel on ragged batches, every attention family; 2. the streaming fixed-point kernel at both of its block
sizes; 3. planted ties and all-zero stories; 4. stories cut by max_slots; 5. tied hops; 6. return codes, nothing launched, the
base call's answers first; 7. the model's forward; 8. replay from a captured graph."""
import ctypes as C

import numpy as np
import pytest

from attended_cases import PAD_SLOT
from attended_story_cases import (CASES, KS, PLANT_GROUPS, ZERO_GROUPS, assert_story_rows, planted_rows, planted_story_case, story_case,
                                  zero_story_case)
from conftest import load_pkg

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


def device_case(env, case, copies=False):
    """copies: a tied case's one plane repeated n_hop times (what the tapped call needs: taps are indexed by plane row)"""
    torch, model = env.torch, env.model
    net = model.QNet(case["cfg"], case["weights"], device="cuda:0")
    keys, vals = case["keys"], case["vals"]
    if copies and keys.shape[0] == 1:
        H = case["cfg"]["n_hop"]
        keys, vals = np.repeat(keys, H, axis=0), np.repeat(vals, H, axis=0)
    dk = torch.from_numpy(model.to_signmag(np.ascontiguousarray(keys))).to(env.dev)
    dv = torch.from_numpy(model.to_signmag(np.ascontiguousarray(vals))).to(env.dev)
    return net, dk, dv, torch.from_numpy(case["row_off"]).to(env.dev), torch.from_numpy(case["u0"]).to(env.dev)


_REF = {}


def reference(env, key, case):
    """(probs [H][rows] and score_codes of the taps as numpy; u_out of the tapped call) of the EXISTING call on a case -- computed
    once per process and left unchanged"""
    if key not in _REF:
        net, dk, dv, dro, du0 = device_case(env, case, copies=True)
        u_tap, taps = net.hops(dk, dv, dro, case["max_slots"], du0, taps=True)
        env.torch.cuda.synchronize()
        probs, codes = taps.probs.cpu().numpy(), taps.score_codes.cpu().numpy()
        probs.setflags(write=False)
        _REF[key] = (probs, codes, u_tap.clone())
    return _REF[key]


def _top_equals_the_sorted_tap(env, name, case, ks=KS):
    probs, _, u_tap = reference(env, name, case)
    net, dk, dv, dro, du0 = device_case(env, case)
    for k in ks:
        u, slot, p = net.hops_top(dk, dv, dro, case["max_slots"], du0, k)
        env.torch.cuda.synchronize()
        assert env.torch.equal(u, u_tap), f"{name}: u_out, k={k}"
        assert_story_rows(slot, p, probs, case["row_off"], case["max_slots"], k, name)
        got = slot.cpu().numpy().view(np.uint32)
        assert ((got < case["max_slots"]) | (got == PAD_SLOT)).all(), f"{name}: a slot beyond max_slots"


# ---- 1. the one-wavefront kernel, 2. the streaming kernel, 4. cut stories ------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n in CASES if n.startswith("wave_")))
def test_one_wavefront_kernel_ragged(env, name):
    case = story_case(name)
    assert case["max_slots"] == 64
    _top_equals_the_sorted_tap(env, name, case)


@pytest.mark.parametrize("name", sorted(n for n in CASES if n.startswith("stream_")))
def test_streaming_kernel_fixed_point(env, name):
    """one wavefront per query up to 256 slots, four beyond; the Q2.5 e^x cases at 4097 rows are those a plain call would run with
    the scan-stop kernel: u_out must still be the tapped call's (and the plain call's, which ends scans early only where the
    result is known)"""
    case = story_case(name)
    _top_equals_the_sorted_tap(env, name, case)
    if "_q25_ms4097" in name:
        net, dk, dv, dro, du0 = device_case(env, case)
        u_plain = net.hops(dk, dv, dro, case["max_slots"], du0)
        env.torch.cuda.synchronize()
        assert env.torch.equal(u_plain, reference(env, name, case)[2])


@pytest.mark.parametrize("name", sorted(n for n in CASES if n.startswith("cut_")))
def test_stories_cut_by_max_slots(env, name):
    """rows are those of the cut story; no slot >= max_slots appears (asserted for every case by the helper)"""
    case = story_case(name)
    assert int(np.diff(case["row_off"]).max()) > case["max_slots"]
    _top_equals_the_sorted_tap(env, name, case)


# ---- 3. planted ties and all-zero stories ----------------------------------------------------------------------------------------------
def _assert_planted_tap(case, probs, codes, base):
    """what the test below relies on, asserted on the EXISTING kernel's tap at hop 0, story by story: the planted rows saturate at
    +-127, every other row scores 0; three probability levels (exp_plan: two, its zero region joins the zero rows and the
    negative ones)"""
    for q in range(case["n_query"]):
        r0, r1 = int(case["row_off"][q]), int(case["row_off"][q + 1])
        pos, neg, others = planted_rows(r1 - r0)
        c, p = codes[0, r0:r1], probs[0, r0:r1]
        assert (c[pos] == 127).all() and (c[neg] == -127).all() and (c[others] == 0).all()
        top, zero, low = p[pos[0]], p[others[0]], p[neg[0]]
        assert (p[pos].view(np.uint32) == top.view(np.uint32)).all() and (p[others] == zero).all() and (p[neg] == low).all()
        assert top == p.max() and top > zero
        if base == 2:
            assert zero == 0.0 and low == 0.0                  # different bins, equal floats
        else:
            assert zero > low


@pytest.mark.parametrize("group", sorted(PLANT_GROUPS))
@pytest.mark.parametrize("base", [0, 1, 2])
def test_planted_ties(env, base, group):
    case = planted_story_case(base, group)
    key = ("planted", base, group)
    probs, codes, u_tap = reference(env, key, case)
    _assert_planted_tap(case, probs, codes, base)
    net, dk, dv, dro, du0 = device_case(env, case)
    for k in (5, 16):
        u, slot, p = net.hops_top(dk, dv, dro, case["max_slots"], du0, k)
        env.torch.cuda.synchronize()
        assert env.torch.equal(u, u_tap)
        got = slot.cpu().numpy().view(np.uint32)
        for q in range(case["n_query"]):
            pos, neg, others = planted_rows(int(case["row_off"][q + 1] - case["row_off"][q]))
            # exp_plan: rows 1 and 3 tie with the zero rows and come in index order; e^x and 2^x: they come after every zero row
            order = pos + (sorted(others + neg) if base == 2 else others + neg)
            assert got[q, 0].tolist() == order[:k], f"base {base}, {group}, k={k}, q{q}"
        assert_story_rows(slot, p, probs, case["row_off"], case["max_slots"], k, f"planted, base {base}, {group}")


@pytest.mark.parametrize("group", sorted(ZERO_GROUPS))
def test_all_zero_stories(env, group):
    case = zero_story_case(group)
    probs, _, u_tap = reference(env, ("zero", group), case)
    S_list = np.diff(case["row_off"])
    for q, S in enumerate(S_list):
        seg = probs[:, case["row_off"][q]:case["row_off"][q + 1]]
        assert (seg == seg[:, :1]).all()
    net, dk, dv, dro, du0 = device_case(env, case)
    for k in KS:
        u, slot, p = net.hops_top(dk, dv, dro, case["max_slots"], du0, k)
        env.torch.cuda.synchronize()
        got = slot.cpu().numpy().view(np.uint32)
        for q, S in enumerate(S_list):
            n = min(k, int(S))
            assert (got[q, :, :n] == np.arange(n, dtype=np.uint32)).all() and (got[q, :, n:] == PAD_SLOT).all(), f"S={S}, k={k}"
        assert env.torch.equal(u, u_tap)
        assert_story_rows(slot, p, probs, case["row_off"], case["max_slots"], k, f"zero stories, {group}")


# ---- 5. tied hops -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n in CASES if n.startswith("tied_")))
def test_tied_hops(env, name):
    """hop_stride = 0 on one plane == the call on n_hop copies of it == the yardstick of the copies"""
    torch = env.torch
    case = story_case(name)
    assert case["keys"].shape[0] == 1
    probs, _, u_tap = reference(env, name, case)
    net, dk, dv, dro, du0 = device_case(env, case)
    _, dk_c, dv_c, _, _ = device_case(env, case, copies=True)
    assert dk_c.shape[0] == case["cfg"]["n_hop"]
    for k in KS:
        u, slot, p = net.hops_top(dk, dv, dro, case["max_slots"], du0, k)
        u_c, slot_c, p_c = net.hops_top(dk_c, dv_c, dro, case["max_slots"], du0, k)
        torch.cuda.synchronize()
        assert torch.equal(u, u_c) and torch.equal(u, u_tap)
        assert torch.equal(slot, slot_c) and torch.equal(p.view(torch.int32), p_c.view(torch.int32))
        assert_story_rows(slot, p, probs, case["row_off"], case["max_slots"], k, name)


# ---- 6. return codes --------------------------------------------------------------------------------------------------------------------
def test_return_codes(env):
    torch, abi, model = env.torch, env.abi, env.model
    name = "wave_fixed_D60"
    case = story_case(name)
    B, H, K, MS = case["n_query"], case["cfg"]["n_hop"], 5, case["max_slots"]
    net, dk, dv, dro, du0 = device_case(env, case)
    rows = dk.shape[1]
    u_out = torch.full_like(du0, -77.0)
    slot = torch.full((B, H, K), -7, dtype=torch.int32, device=env.dev)
    tp = torch.full((B, H, K), -7.0, dtype=torch.float32, device=env.dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def call(n=None, keys=dk, vals=dv, ro=dro, u0=du0, out=u_out, max_slots=MS, n_query=B, k=K, top_slot=slot, top_p=tp, net_null=False):
        nref = None if net_null else C.byref(n if n is not None else net.net)
        return abi.lib.qmann_hops_top_i8(nref, p(keys), p(vals), rows * net.Dp, p(ro), max_slots, p(u0), p(out), k, p(top_slot), p(top_p),
                                         n_query, None)

    def base(n=None, keys=dk, vals=dv, ro=dro, u0=du0, out=u_out, max_slots=MS, n_query=B, net_null=False):
        nref = None if net_null else C.byref(n if n is not None else net.net)
        return abi.lib.qmann_hops_i8(nref, p(keys), p(vals), rows * net.Dp, p(ro), max_slots, p(u0), p(out), None, n_query, None)

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
    # float attention is not served at any length; the Hamming family beyond 64 slots
    assert call(variant(attention_mode=1)) == abi.QMANN_EUNSUPPORTED and call(variant(attention_mode=1), max_slots=300) == abi.QMANN_EUNSUPPORTED
    for mode in (3, 10, 11):
        assert call(variant(attention_mode=mode, num_bit=8), max_slots=65) == abi.QMANN_EUNSUPPORTED
        assert call(variant(attention_mode=mode, num_bit=8), max_slots=65, k=0) == abi.QMANN_EUNSUPPORTED      # ahead of a bad k
    assert call(variant(attention_mode=1), top_p=None) == abi.QMANN_EUNSUPPORTED
    # every refusal of the base call, alone and together with a bad k or a null output: the base call's code
    wide = variant()
    wide.att[0] = abi.Fmt(5, 4)                                   # word length 9
    assert abi.lib.qmann_hops_lds_bytes(200000) > 160 * 1024 - 1024
    faults = [dict(net_null=True), dict(keys=None), dict(vals=None), dict(ro=None), dict(u0=None), dict(out=None),
              dict(n=variant(dim_emb_pad=96)), dict(n=variant(attention_mode=7)), dict(n=variant(softmax_base=9)), dict(n=wide),
              dict(n=variant(n_hop=0)), dict(n_query=1 << 24), dict(max_slots=200000),
              dict(n=variant(attention_mode=10, num_bit=3)), dict(n=variant(attention_mode=3), max_slots=200000),
              dict(n=variant(attention_mode=1), max_slots=200000), dict(n=variant(attention_mode=1), max_slots=100000)]
    for f in faults:
        want = base(**f)
        assert want not in (abi.QMANN_OK,), f
        assert call(**f) == want, f
        assert call(k=0, **f) == want and call(k=17, **f) == want and call(top_slot=None, **f) == want and call(top_p=None, **f) == want, f
    # n_query = 0 is QMANN_OK whatever k, in every family
    assert call(n_query=0) == abi.QMANN_OK and call(n_query=0, k=0) == abi.QMANN_OK and call(n_query=0, top_slot=None) == abi.QMANN_OK
    assert call(variant(attention_mode=11, num_bit=8), n_query=0, k=17) == abi.QMANN_OK
    torch.cuda.synchronize()
    assert (u_out == -77.0).all() and (slot == -7).all() and (tp == -7.0).all()       # none of them launched anything
    # one good call; k = 16 exceeds most of the batch's stories and is no error
    assert call() == abi.QMANN_OK
    torch.cuda.synchronize()
    probs, _, u_tap = reference(env, name, case)
    assert torch.equal(u_out, u_tap)
    assert_story_rows(slot, tp, probs, case["row_off"], MS, K, name)
    slot16 = torch.full((B, H, 16), -7, dtype=torch.int32, device=env.dev)
    tp16 = torch.full((B, H, 16), -7.0, dtype=torch.float32, device=env.dev)
    assert call(k=16, top_slot=slot16, top_p=tp16) == abi.QMANN_OK
    torch.cuda.synchronize()
    assert_story_rows(slot16, tp16, probs, case["row_off"], MS, 16, name)


# ---- 7. the model -----------------------------------------------------------------------------------------------------------------------
def _qnet_of(env, cfg, wts, hm):
    torch, model = env.torch, env.model
    net = model.QNet.from_model(cfg, hm)
    net.w_q, net.w_a, net.w_c = [torch.from_numpy(wts["w_q"]).to(env.dev), [torch.from_numpy(w).to(env.dev) for w in wts["w_a"]],
                                 [torch.from_numpy(w).to(env.dev) for w in wts["w_c"]]]
    net.make_tables()
    return net


N_STORIES = 64


# (tied: equal matrices on every hop AND equal formats -- the trained fixture's formats differ per hop, so only the joint-20 model)
@pytest.mark.parametrize("which,mode,num_bit,tie", [("trained_qa1", 2, 8, False), ("trained_qa1", 11, 4, False),
                                                    ("random_joint20", 2, 8, False), ("random_joint20", 11, 4, False),
                                                    ("random_joint20", 2, 8, True), ("random_joint20", 11, 4, True)])
def test_forward_words_top(env, which, mode, num_bit, tie):
    """the first 64 stories of a fixture: rows against the yardstick built from QNet.embed_idx plus the tapped hop call; pred,
    cost, match and last_u those of forward_words on the same batch; last_topk works afterwards"""
    from test_gpu_shared import _model_inputs
    from test_gpu_words import tied
    torch, model = env.torch, env.model
    cfg, wts, sw, qw, n_sen, ans = _model_inputs(which, env)
    cfg = dict(cfg, attention_mode=mode, num_bit=num_bit)
    if tie:
        wts = tied(wts)
    n_sen = n_sen[:N_STORIES]
    row_off = np.concatenate([[0], np.cumsum(n_sen)]).astype(np.int32)
    R, K = int(row_off[-1]), 5
    MS = min(int(n_sen.max()), 64)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(env.dev)
    d_sw, d_qw, d_ro = up(sw[:R]), up(qw[:N_STORIES]), torch.from_numpy(row_off).to(env.dev)
    d_ans = torch.from_numpy(ans[:N_STORIES].astype(np.int32)).to(env.dev)

    plain = model.HostModel(cfg, wts, device="cuda:0")
    pred2, cost2, match2 = plain.forward_words(d_sw, d_qw, d_ro, MS, d_ans)
    torch.cuda.synchronize()
    u2, rank2 = plain.last_u(N_STORIES), plain.last_topk(3)
    torch.cuda.synchronize()

    hm = model.HostModel(cfg, wts, device="cuda:0")
    net = _qnet_of(env, cfg, wts, hm)
    dk, dv, du0 = net.embed_idx(d_sw, d_qw)
    u_tap, taps = net.hops(dk, dv, d_ro, MS, du0, taps=True)
    torch.cuda.synchronize()
    probs = taps.probs.cpu().numpy()
    pred, cost, match, slot, p = hm.forward_words_top(d_sw, d_qw, d_ro, MS, K, d_ans)
    torch.cuda.synchronize()
    what = f"{which}, mode {mode}, tied {tie}"
    assert_story_rows(slot, p, probs, row_off, MS, K, what)
    assert torch.equal(pred, pred2) and int(match.item()) == int(match2.item()), what
    assert torch.equal(hm.last_u(N_STORIES), u2) and torch.equal(u2, u_tap), what
    assert float(cost.item()) == pytest.approx(float(cost2.item()), rel=1e-4, abs=1e-3)      # float atomics: the order of the adds differs
    rank = hm.last_topk(3)
    torch.cuda.synchronize()
    assert torch.equal(rank[0], rank2[0]) and torch.equal(rank[1], rank2[1]), what
    assert float(u2.abs().sum()) > 0
    hm.close(); plain.close()


def test_forward_words_top_return_code_order(env):
    from test_gpu_shared import _model_inputs
    torch, abi, model = env.torch, env.abi, env.model
    cfg, wts, sw, qw, n_sen, _ = _model_inputs("random_joint20", env)
    B, K, H = 4, 5, cfg["n_hop"]
    row_off = np.concatenate([[0], np.cumsum(n_sen[:B])]).astype(np.int32)
    R = int(row_off[-1])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(env.dev)
    d_sw, d_qw, d_ro = up(sw[:R]), up(qw[:B]), torch.from_numpy(row_off).to(env.dev)
    pred = torch.full((B,), -7, dtype=torch.int32, device=env.dev)
    slot = torch.full((B, H, K), -7, dtype=torch.int32, device=env.dev)
    tp = torch.full((B, H, K), -7.0, dtype=torch.float32, device=env.dev)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None

    def fwd(hm, k=K, top_slot=slot, top_p=tp, max_slots=64, n_query=B, words=d_qw, ro=d_ro, out=pred, null_model=False):
        return abi.lib.qmann_model_forward_words_top(None if null_model else hm.h, p(d_sw), R, d_sw.shape[1], p(words), d_qw.shape[1], p(ro),
                                                     max_slots, n_query, None, p(out), None, None, k, p(top_slot), p(top_p), None)
    flt = model.HostModel(dict(cfg, attention_mode=1), wts, device="cuda:0")
    assert fwd(flt) == abi.QMANN_EUNSUPPORTED and fwd(flt, k=0) == abi.QMANN_EUNSUPPORTED              # ahead of a bad k
    assert fwd(flt, words=None) == abi.QMANN_EINVAL and fwd(flt, n_query=0, k=0) == abi.QMANN_OK      # forward_words' answers first
    flt.close()
    for mode in (3, 10, 11):
        ham = model.HostModel(dict(cfg, attention_mode=mode, num_bit=4), wts, device="cuda:0")
        assert fwd(ham, max_slots=65) == abi.QMANN_EUNSUPPORTED and fwd(ham, max_slots=65, top_p=None) == abi.QMANN_EUNSUPPORTED
        assert fwd(ham, k=17) == abi.QMANN_EINVAL
        ham.close()
    hm = model.HostModel(cfg, wts, device="cuda:0")
    assert fwd(hm, null_model=True) == abi.QMANN_EINVAL
    assert fwd(hm, words=None, k=0) == abi.QMANN_EINVAL and fwd(hm, ro=None) == abi.QMANN_EINVAL and fwd(hm, out=None) == abi.QMANN_EINVAL
    assert fwd(hm, n_query=0, k=0, top_slot=None) == abi.QMANN_OK
    assert fwd(hm, k=0) == abi.QMANN_EINVAL and fwd(hm, k=17) == abi.QMANN_EINVAL
    assert fwd(hm, top_slot=None) == abi.QMANN_EINVAL and fwd(hm, top_p=None) == abi.QMANN_EINVAL
    torch.cuda.synchronize()
    assert (pred == -7).all() and (slot == -7).all() and (tp == -7.0).all()
    assert fwd(hm, max_slots=65) == abi.QMANN_OK                  # a fixed-point model beyond 64 slots is served
    torch.cuda.synchronize()
    assert (pred != -7).all() and (slot != -7).all()
    hm.close()


# ---- 8. graph capture -------------------------------------------------------------------------------------------------------------------
def test_forward_words_top_replays_from_a_captured_graph(env):
    """one eager call grows the workspace, the captured call replays on new words of the same shape in the graph's buffers and
    gives an eager model's results"""
    from test_gpu_graph import _words
    torch, model = env.torch, env.model
    dev = env.dev
    rng = np.random.default_rng(78)
    V, dd, D, H, B, K = 40, 30, 60, 3, 333, 5
    cfg = model.babi_cfg(V, 2, 0, iwl=5, en_mq=True)
    wts = {"w_q": rng.normal(0, 1.0, (D, V)).astype(np.float32), "w_ans": rng.normal(0, 0.3, (V, D)).astype(np.float32),
           "w_a": [rng.normal(0, 1.0, (D, V)).astype(np.float32) for _ in range(H)],
           "w_c": [rng.normal(0, 1.0, (D, V)).astype(np.float32) for _ in range(H)],
           "w_h": [rng.normal(0, 1.0, (D, D)).astype(np.float32) for _ in range(H)]}
    n_sen = rng.integers(1, 51, B)
    row_off = np.concatenate([[0], np.cumsum(n_sen)]).astype(np.int32)
    R, MS = int(row_off[-1]), 50
    d_ro = torch.from_numpy(row_off).to(dev)

    def batch(seed):
        r = np.random.default_rng(seed)
        return (torch.from_numpy(_words(r, R, V, dd, 8, True).view(np.int16)).to(dev),
                torch.from_numpy(_words(r, B, V, dd, 8, False).view(np.int16)).to(dev),
                torch.from_numpy(r.integers(0, V, B).astype(np.int32)).to(dev))
    s = torch.cuda.Stream(device=dev)
    hm = model.HostModel(cfg, wts, device="cuda:0", stream=s.cuda_stream)
    eager = model.HostModel(cfg, wts, device="cuda:0")
    sw, qw, ans = batch(1)
    with torch.cuda.stream(s):
        hm.forward_words_top(sw, qw, d_ro, MS, K, ans)                            # warm-up: the workspace takes its size
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        pred, cost, match, slot, p = hm.forward_words_top(sw, qw, d_ro, MS, K, ans)      # captured, not run
    for seed in (2, 3, 4):
        nsw, nqw, nans = batch(seed)
        sw.copy_(nsw); qw.copy_(nqw); ans.copy_(nans)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        p2, c2, m2, slot2, tp2 = eager.forward_words_top(nsw, nqw, d_ro, MS, K, nans)
        torch.cuda.synchronize()
        assert torch.equal(pred, p2) and torch.equal(hm.last_u(B), eager.last_u(B)), seed
        assert torch.equal(slot, slot2) and torch.equal(p.view(torch.int32), tp2.view(torch.int32)), seed
        assert int(match.item()) == int(m2.item()) and float(cost.item()) == pytest.approx(float(c2.item()), rel=1e-5)
    assert len({int(x) for x in slot[:, 0, 0].cpu().numpy()}) > 1                 # (not one row for every story)
    hm.close(); eager.close()

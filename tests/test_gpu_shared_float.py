"""Float attention over one shared memory: qmann_hops_shared_float_i8 (csrc/batch_hops_shared_float.hip) and the model's
memorise / ask for float models (qmann_model_enable_float_asks).

Every output of a hop call sits inside 4 KiB guards filled with 0xA5 (float_hops_cases.GUARD / FILL).

1. bit-equality: for every case of shared_float_cases.py and every forced tile that fits, plus the launcher's choice, u_out and
   all five taps are bit-equal to qmann_hops_i8 (mode 1) on n_query copies of the planes -- with all taps, with none, with each
   alone; the guards are compared with the payload;
2. reference: the same outputs pass float_hops_cases.check_outputs against the float64 reference (scores equal, p within 1e-5,
   o within the derived bound, u equal outside `near`; each hop's reference input is the kernel's own tapped state);
3. tied hops; 4. refusals in their order; 5. the LDS cap; 6. - 8. the model, mode off / on / its refusals; 9. graph replay.
"""
import ctypes as C

import numpy as np
import pytest

import float_hops_cases as fc
import shared_float_cases as sf
from conftest import load_pkg
from float_hops_cases import ALL_TAPS, FILL, GUARD, TAP_COMBOS
from shared_float_cases import CASES, build

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


def _buffers(env, case, taps):
    shapes = fc.out_shapes(case)
    bufs = {k: env.torch.full((int(np.prod(shapes[k][0])) * 4 + 2 * GUARD,), FILL, dtype=env.torch.uint8, device=env.dev)
            for k in ("u_out",) + tuple(taps)}
    ptr = lambda k: bufs[k].data_ptr() + GUARD if k in bufs else 0
    return bufs, ptr, env.abi.Taps(ptr("codes"), ptr("scores"), ptr("probs"), ptr("o"), ptr("u"))


def _up(env, a):
    return env.torch.from_numpy(np.ascontiguousarray(a)).to(env.dev)


def launch_copies(env, case, taps=ALL_TAPS):
    """qmann_hops_i8 (mode 1) on the case's planes -- the memory repeated once per query; name -> whole guard-filled buffer"""
    torch, abi = env.torch, env.abi
    net = env.model.QNet(case.cfg, case.wts)
    dk, dv = _up(env, case.kb.view(np.int8)), _up(env, case.vb.view(np.int8))
    ro, u0 = _up(env, case.row_off.view(np.int32)), _up(env, case.u0)
    bufs, ptr, tp = _buffers(env, case, taps)
    rc = abi.lib.qmann_hops_i8(C.byref(net.net), C.c_void_p(dk.data_ptr()), C.c_void_p(dv.data_ptr()), case.R * net.Dp,
                               C.c_void_p(ro.data_ptr()), case.max_slots, C.c_void_p(u0.data_ptr()), C.c_void_p(ptr("u_out")),
                               C.byref(tp) if taps else None, case.B, None)
    assert rc == abi.QMANN_OK, f"{case.name}: qmann_hops_i8 returned {rc}"
    torch.cuda.synchronize()
    return {k: b.cpu().numpy() for k, b in bufs.items()}


def launch_shared(env, case, taps=ALL_TAPS):
    """qmann_hops_shared_float_i8 on the case's ONE memory; outputs in the layout of launch_copies"""
    torch, abi = env.torch, env.abi
    net = env.model.QNet(case.cfg, case.wts)
    mk, mv = sf.memory(case)
    assert net.Dp == mk.shape[2]
    dk, dv, u0 = _up(env, mk.view(np.int8)), _up(env, mv.view(np.int8)), _up(env, case.u0)
    bufs, ptr, tp = _buffers(env, case, taps)
    stride = 0 if case.tied else case.max_slots * net.Dp
    rc = abi.lib.qmann_hops_shared_float_i8(C.byref(net.net), C.c_void_p(dk.data_ptr()), C.c_void_p(dv.data_ptr()), stride,
                                            case.max_slots, C.c_void_p(u0.data_ptr()), C.c_void_p(ptr("u_out")),
                                            C.byref(tp) if taps else None, case.B, None)
    assert rc == abi.QMANN_OK, f"{case.name}: qmann_hops_shared_float_i8 returned {rc}"
    torch.cuda.synchronize()
    return {k: b.cpu().numpy() for k, b in bufs.items()}


def tiles_to_run(env, case, force_qt):
    """(label, tile that runs) for the launcher's choice and every forced tile that fits"""
    S, B = case.max_slots, case.B
    for qt in (None,) + sf.TILES:
        if qt and not sf.fits(S, qt):
            continue
        force_qt(qt)
        ran = env.abi.lib.qmann_hops_shared_float_tile(S, B)
        assert ran in sf.TILES and (not qt or ran == qt), "the switch took effect"
        yield (f" tile {qt or 'chosen'}", ran)


# ---- 1. + 2. bit-equality with the per-story call on copies, and the float64 reference --------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n in CASES if CASES[n]["family"] != "tied"))
def test_shared_float_equals_hops_i8_on_copies_and_the_reference(env, force_qt, name):
    case = build(name)
    want = {combo: launch_copies(env, case, combo) for combo in TAP_COMBOS}
    stats = fc.check_outputs(case, want[ALL_TAPS], label=" (per-story call)")
    ran = []
    for label, tile in tiles_to_run(env, case, force_qt):
        ran.append(tile)
        for combo in TAP_COMBOS:
            got = launch_shared(env, case, combo)
            assert set(got) == set(want[combo])
            for k in got:                                           # payload AND guards, byte for byte
                np.testing.assert_array_equal(got[k], want[combo][k], err_msg=f"{name}{label} taps={combo}: {k}")
            fc.check_outputs(case, got, taps=combo, label=f"{label} taps={combo}")
    assert set(ran) == {1} | {qt for qt in sf.TILES if sf.fits(case.max_slots, qt)}
    print(f"{name}: tiles {sorted(set(ran))}; {stats['differ']} of {stats['cols']} state columns differ from the float64 reference, "
          f"all among the {stats['near']} near a step")


def test_a_full_batch_with_the_launchers_own_tile_and_the_largest(env, force_qt):
    """more workgroups than compute units and a short last tile: the launcher's own choice (one query per workgroup, by the
    measurement in DESIGN.md section 5) and tiles of 8, each against qmann_hops_i8 on copies"""
    torch = env.torch
    base = build("sf_batch_05")
    S, D = base.max_slots, base.cfg["dim_emb"]
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    B = 8 * cus + 3
    rng = np.random.default_rng(B)
    u0 = (fc._codes(rng, (B, D), 3.0, 127).astype(np.float64) / 8).astype(np.float32)
    mk, mv = sf.memory(base)
    case = fc.Case("sf_full_batch", "batches", base.cfg, base.lin, base.wts, np.tile(mk, (1, B, 1)), np.tile(mv, (1, B, 1)),
                   (np.arange(B + 1) * S).astype(np.uint32), u0, S)
    want = launch_copies(env, case)
    for qt, tile in ((None, 1), (8, 8)):
        force_qt(qt)
        assert env.abi.lib.qmann_hops_shared_float_tile(S, B) == tile
        got = launch_shared(env, case)
        for k in got:
            np.testing.assert_array_equal(got[k], want[k], err_msg=f"{k}, tile {tile}")
    assert np.abs(fc.payload(case, got, "u_out")).sum() > 0


# ---- 3. tied hops -----------------------------------------------------------------------------------------------------------------
def test_tied_hops_with_taps_equal_three_copies_of_the_plane(env, force_qt):
    """hop_stride = 0 WITH taps (they are indexed by query, not by plane row) equals the launch on three copies of the plane, which
    equals the per-story call on copies and passes the whole comparison"""
    tied = build("sf_tied")
    three = sf.untied(tied)
    want = launch_copies(env, three)
    fc.check_outputs(three, want)
    for label, _ in tiles_to_run(env, tied, force_qt):
        for combo in TAP_COMBOS:
            a, b = launch_shared(env, tied, combo), launch_shared(env, three, combo)
            for k in a:
                np.testing.assert_array_equal(a[k], b[k], err_msg=f"tied{label} taps={combo}: {k}")
                np.testing.assert_array_equal(a[k], want[k], err_msg=f"tied{label} taps={combo}: {k} against the per-story call")


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------
def test_refusals_in_their_order(env):
    torch, abi, model = env.torch, env.abi, env.model
    case = build("sf_batch_03")
    S, B = case.max_slots, case.B
    net = model.QNet(case.cfg, case.wts)
    mk, mv = sf.memory(case)
    dk, dv, du0 = _up(env, mk.view(np.int8)), _up(env, mv.view(np.int8)), _up(env, case.u0)
    u_out = torch.full_like(du0, -77.0)
    p = lambda t: C.c_void_p(t.data_ptr())

    def call(n=None, keys=dk, vals=dv, u0=du0, out=u_out, n_slots=S, n_query=B):
        return abi.lib.qmann_hops_shared_float_i8(C.byref(n if n is not None else net.net), p(keys) if keys is not None else None,
                                                  p(vals) if vals is not None else None, S * net.Dp, n_slots,
                                                  p(u0) if u0 is not None else None, p(out) if out is not None else None, None, n_query, None)

    def variant(**kw):
        n = model._net_from_cfg(case.cfg)
        for h in range(n.n_hop):
            n.lin_map[h] = net.net.lin_map[h]
        for k, v in kw.items():
            setattr(n, k, v)
        return n
    too_long = sf.CAP_SLOTS + 1
    # 1. the shared checks' own refusals, ahead of everything else
    assert call(keys=None) == abi.QMANN_EINVAL and call(vals=None) == abi.QMANN_EINVAL
    assert call(u0=None) == abi.QMANN_EINVAL and call(out=None) == abi.QMANN_EINVAL
    assert abi.lib.qmann_hops_shared_float_i8(None, p(dk), p(dv), 0, S, p(du0), p(u_out), None, B, None) == abi.QMANN_EINVAL
    assert call(variant(n_hop=0), n_slots=0) == abi.QMANN_EINVAL
    assert call(variant(dim_emb_pad=96, attention_mode=2)) == abi.QMANN_EUNSUPPORTED
    wide = variant(attention_mode=2)
    wide.w[0] = abi.Fmt(5, 4)                                     # word length 9: fill_hop_args, ahead of the attention mode
    assert call(wide) == abi.QMANN_ERANGE
    assert call(variant(softmax_base=7, attention_mode=2)) == abi.QMANN_EINVAL
    # 2. the attention mode, ahead of the sizes
    for mode in (2, 3, 10, 11):
        assert call(variant(attention_mode=mode), n_slots=0) == abi.QMANN_EUNSUPPORTED
        assert call(variant(attention_mode=mode), n_slots=too_long, n_query=0) == abi.QMANN_EUNSUPPORTED
    # 3. n_slots = 0, ahead of the LDS size and the query counts
    assert call(n_slots=0, n_query=0) == abi.QMANN_EINVAL and call(n_slots=0, n_query=1 << 24) == abi.QMANN_EINVAL
    # 4. one query's LDS, ahead of n_query = 0
    assert call(n_slots=too_long) == abi.QMANN_ERANGE and call(n_slots=too_long, n_query=0) == abi.QMANN_ERANGE
    # 5. n_query = 0 is no error; 6. 2^24 queries or more
    assert call(n_query=0) == abi.QMANN_OK
    assert call(n_query=1 << 24) == abi.QMANN_ERANGE and call(n_query=(1 << 32) - 1) == abi.QMANN_ERANGE
    torch.cuda.synchronize()
    assert (u_out == -77.0).all(), "none of them launched anything"
    assert call() == abi.QMANN_OK
    torch.cuda.synchronize()
    assert torch.equal(u_out, net.hops_shared_float(dk, dv, S, du0))
    # qmann_hops_shared_i8 keeps refusing float attention
    assert abi.lib.qmann_hops_shared_i8(C.byref(net.net), p(dk), p(dv), S * net.Dp, S, p(du0), p(u_out), None, B, None) == abi.QMANN_EUNSUPPORTED


# ---- 5. the LDS cap -----------------------------------------------------------------------------------------------------------------
def test_the_largest_memory_runs_and_one_more_slot_is_refused(env, force_qt):
    torch, abi = env.torch, env.abi
    force_qt(None)
    S, D, B, H = sf.CAP_SLOTS, 60, 2, 1
    rng = np.random.default_rng(38368)
    cfg = dict(n_hop=H, dim_emb=D, dim_input=4, attention_mode=1, softmax_variant=0, f_fixed=True, en_lin_map=False,
               fmt=[fc.Q52], fmt_w=[fc.Q43], fmt_att=[fc.Q52], fmt_bin=fc.Q52, att_scale=[0.02])
    kc = np.zeros((H, S + 1, 64), np.int64); vc = np.zeros((H, S + 1, 64), np.int64)
    kc[:, :, :D] = fc._codes(rng, (H, S + 1, D), 3.0, 127); vc[:, :, :D] = fc._codes(rng, (H, S + 1, D), 30.0, 127)
    mk, mv = fc.ref.encode(kc), fc.ref.encode(vc)
    u0 = (fc._codes(rng, (B, D), 3.0, 127).astype(np.float64) / 8).astype(np.float32)
    wts = dict(w_h=None, w_ans=np.zeros((4, D), np.float32))
    case = fc.Case("sf_cap", "cap", cfg, None, wts, np.tile(mk[:, :S], (1, B, 1)), np.tile(mv[:, :S], (1, B, 1)),
                   (np.arange(B + 1) * S).astype(np.uint32), u0, S)
    assert abi.lib.qmann_hops_shared_float_tile(S, B) == 1 and abi.lib.qmann_hops_shared_float_tile(S + 1, B) == 0
    want, got = launch_copies(env, case), launch_shared(env, case)
    for k in got:
        np.testing.assert_array_equal(got[k], want[k], err_msg=k)
    probs = fc.payload(case, got, "probs")
    assert np.abs(fc.payload(case, got, "u_out")).sum() > 0 and (probs[0, S - 1] > 0) and (probs[0, 2 * S - 1] > 0), "the last slot carries weight"
    # one slot more
    net = env.model.QNet(cfg, wts)
    dk, dv, du0 = _up(env, mk.view(np.int8)), _up(env, mv.view(np.int8)), _up(env, u0)
    u_out = torch.full_like(du0, -77.0)
    p = lambda t: C.c_void_p(t.data_ptr())
    rc = abi.lib.qmann_hops_shared_float_i8(C.byref(net.net), p(dk), p(dv), (S + 1) * 64, S + 1, p(du0), p(u_out), None, B, None)
    torch.cuda.synchronize()
    assert rc == abi.QMANN_ERANGE and (u_out == -77.0).all()


# ---- 6. - 8. the model ----------------------------------------------------------------------------------------------------------------
def _float_model_inputs(env):
    """bAbI-shaped words as test_gpu_shared.py builds them (the joint-20 test set, random weights), for a float-attention model"""
    from test_gpu_shared import _model_inputs
    cfg, wts, sw, qw, n_sen, ans = _model_inputs("random_joint20", env)
    return dict(cfg, attention_mode=1), wts, sw, qw, n_sen, ans


def _story_and_questions(sw, qw, n_sen, ans, N):
    offs = np.concatenate([[0], np.cumsum(n_sen)])
    s = int(np.argmax(n_sen))
    others = (s + 1 + np.arange(N)) % len(n_sen)
    return sw[offs[s]:offs[s + 1]], qw[others], ans[others]


def test_model_mode_off_memorize_is_unsupported(env):
    torch, model, abi = env.torch, env.model, env.abi
    cfg, wts, sw, qw, n_sen, ans = _float_model_inputs(env)
    story, _, _ = _story_and_questions(sw, qw, n_sen, ans, 1)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(env.dev)
    hm = model.HostModel(cfg, wts, device="cuda:0")
    d_story = up(story)
    rc = abi.lib.qmann_model_memorize_words(hm.h, C.c_void_p(d_story.data_ptr()), story.shape[0], story.shape[1], None)
    assert rc == abi.QMANN_EUNSUPPORTED and hm.memory_rows() == 0
    hm.close()


@pytest.mark.parametrize("N", [1, 7, 4099])
def test_model_memorize_and_ask_equal_forward_words_on_copies(env, monkeypatch, N):
    """pred, match and last_u bit for bit; cost bit for bit where one atomic makes it (N = 1), else within the order of the answer
    layer's float atomics, which differs between two runs of ONE call as well.  Under QMANN_ANSWER_EXACT, so that pred is the
    ranking's first entry."""
    torch, model, abi = env.torch, env.model, env.abi
    monkeypatch.setenv("QMANN_ANSWER_EXACT", "1")
    abi.lib.qmann_tuning_reload()
    cfg, wts, sw, qw, n_sen, ans = _float_model_inputs(env)
    story, q_sel, a_sel = _story_and_questions(sw, qw, n_sen, ans, N)
    R = story.shape[0]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(env.dev)
    d_ans = torch.from_numpy(a_sel.astype(np.int32)).to(env.dev)

    hm = model.HostModel(cfg, wts, device="cuda:0")
    hm.enable_float_asks()
    hm.memorize_words(up(story))
    assert hm.memory_rows() == R
    pred, cost, match = hm.ask_words(up(q_sel), d_ans)
    torch.cuda.synchronize()
    p_s, u_s = pred.cpu().numpy(), hm.last_u(N).cpu().numpy()
    top_idx, top_p = hm.last_topk(3)
    torch.cuda.synchronize()
    assert np.array_equal(top_idx[:, 0].cpu().numpy(), p_s), "pred is the ranking's first entry"

    hm2 = model.HostModel(cfg, wts, device="cuda:0")
    pred2, cost2, match2 = hm2.forward_words(up(np.tile(story, (N, 1))), up(q_sel), torch.from_numpy((np.arange(N + 1) * R).astype(np.int32)).to(env.dev),
                                             R, d_ans)
    torch.cuda.synchronize()
    assert np.array_equal(p_s, pred2.cpu().numpy())
    assert np.array_equal(u_s.view(np.uint32), hm2.last_u(N).cpu().numpy().view(np.uint32))
    assert int(match.item()) == int(match2.item()) == int((p_s == a_sel).sum())
    if N == 1:
        assert float(cost.item()) == float(cost2.item())
    else:
        assert float(cost.item()) == pytest.approx(float(cost2.item()), rel=1e-5)
    assert np.abs(u_s).sum() > 0 and (N < 100 or len(set(p_s.tolist())) > 1)
    # a second ask of fewer questions on the same memory, after a forward in between on the same model
    hm.forward_words(up(story), up(q_sel[:1]), torch.tensor([0, R], dtype=torch.int32, device=env.dev), R)
    pred3, _, _ = hm.ask_words(up(q_sel[:max(N // 2, 1)]))
    torch.cuda.synchronize()
    assert np.array_equal(pred3.cpu().numpy(), p_s[:max(N // 2, 1)])
    hm.close(); hm2.close()


def test_model_refusals(env):
    torch, model, abi = env.torch, env.model, env.abi
    cfg, wts, sw, qw, n_sen, ans = _float_model_inputs(env)
    story, q_sel, _ = _story_and_questions(sw, qw, n_sen, ans, 4)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(env.dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    d_story, d_q = up(story), up(q_sel)
    hm = model.HostModel(cfg, wts, device="cuda:0")
    assert abi.lib.qmann_model_enable_float_asks(None, 1) == abi.QMANN_EINVAL
    hm.enable_float_asks()
    hm.memorize_words(d_story)
    # the attended-slots asks refuse a float model before anything is launched
    k = 2
    pred = torch.full((4,), -7, dtype=torch.int32, device=env.dev)
    slot = torch.full((4, cfg["n_hop"], k), -7, dtype=torch.int32, device=env.dev)
    tp = torch.full((4, cfg["n_hop"], k), -7.0, dtype=torch.float32, device=env.dev)
    for fn in (abi.lib.qmann_model_ask_words_top, abi.lib.qmann_model_ask_words_top_packed):
        assert fn(hm.h, p(d_q), q_sel.shape[1], 4, None, p(pred), None, None, k, p(slot), p(tp), None) == abi.QMANN_EUNSUPPORTED
    torch.cuda.synchronize()
    assert (pred == -7).all() and (slot == -7).all() and (tp == -7.0).all()
    # the other shared-memory calls keep refusing float models
    assert abi.lib.qmann_model_forward_shared_words(hm.h, p(d_story), story.shape[0], story.shape[1], p(d_q), q_sel.shape[1], 4, None,
                                                    p(pred), None, None, None) == abi.QMANN_EUNSUPPORTED
    assert abi.lib.qmann_model_enable_split_asks(hm.h, 1 << 20, None) == abi.QMANN_EUNSUPPORTED
    assert abi.lib.qmann_model_enable_split_asks_packed(hm.h, 1 << 20, None) == abi.QMANN_EUNSUPPORTED
    assert hm.memory_rows() == story.shape[0]
    # on = 0 forgets the memory and restores the refusal
    hm.enable_float_asks(False)
    assert hm.memory_rows() == 0
    assert abi.lib.qmann_model_ask_words(hm.h, p(d_q), q_sel.shape[1], 4, None, p(pred), None, None, None) == abi.QMANN_EINVAL
    assert abi.lib.qmann_model_memorize_words(hm.h, p(d_story), story.shape[0], story.shape[1], None) == abi.QMANN_EUNSUPPORTED
    torch.cuda.synchronize()
    assert (pred == -7).all()
    # too long a memory: QMANN_ERANGE at memorize, nothing memorised (the words are not read: the length is checked first)
    hm.enable_float_asks()
    too_long = sf.CAP_SLOTS + 1
    long_story = torch.full((too_long, story.shape[1]), -1, dtype=torch.int16, device=env.dev)
    assert abi.lib.qmann_model_memorize_words(hm.h, p(long_story), too_long, story.shape[1], None) == abi.QMANN_ERANGE
    assert hm.memory_rows() == 0
    hm.close()
    # a fixed-point model has no float asks
    fx = model.HostModel(dict(cfg, attention_mode=2), wts, device="cuda:0")
    assert abi.lib.qmann_model_enable_float_asks(fx.h, 1) == abi.QMANN_EUNSUPPORTED
    assert abi.lib.qmann_model_enable_float_asks(fx.h, 0) == abi.QMANN_EUNSUPPORTED
    fx.memorize_words(d_story)                                   # ... and memorises as before
    assert fx.memory_rows() == story.shape[0]
    fx.close()


# ---- 9. graph capture ----------------------------------------------------------------------------------------------------------------
def test_ask_words_replays_from_a_captured_graph(env):
    """pattern of test_gpu_graph.py: one eager ask grows the question workspace, the captured ask replays with new questions in the
    graph's buffer and gives the bytes of an eager model (in a process with the machines' four hardware queues)"""
    from test_gpu_graph import _words
    torch, model = env.torch, env.model
    dev = env.dev
    rng = np.random.default_rng(78)
    V, dd, D, H, B, R = 40, 30, 60, 3, 333, 23
    cfg = model.babi_cfg(V, 1, 0, iwl=5, en_mq=True)
    wts = {"w_q": rng.normal(0, 1.0, (D, V)).astype(np.float32), "w_ans": rng.normal(0, 0.3, (V, D)).astype(np.float32),
           "w_a": [rng.normal(0, 1.0, (D, V)).astype(np.float32) for _ in range(H)],
           "w_c": [rng.normal(0, 1.0, (D, V)).astype(np.float32) for _ in range(H)],
           "w_h": [rng.normal(0, 1.0, (D, D)).astype(np.float32) for _ in range(H)]}
    story = torch.from_numpy(_words(np.random.default_rng(1), R, V, dd, 8, True).view(np.int16)).to(dev)

    def questions(seed):
        r = np.random.default_rng(seed)
        return (torch.from_numpy(_words(r, B, V, dd, 8, False).view(np.int16)).to(dev),
                torch.from_numpy(r.integers(0, V, B).astype(np.int32)).to(dev))
    s = torch.cuda.Stream(device=dev)
    hm = model.HostModel(cfg, wts, device="cuda:0", stream=s.cuda_stream)
    plain = model.HostModel(cfg, wts, device="cuda:0")
    for m in (hm, plain):
        m.enable_float_asks()
    qw, ans = questions(1)
    with torch.cuda.stream(s):
        hm.memorize_words(story)
        hm.ask_words(qw, ans)                                                     # warm-up: the workspace takes its size
    s.synchronize()
    plain.memorize_words(story)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        pred, cost, match = hm.ask_words(qw, ans)                                 # captured, not run
    for seed in (2, 3, 4):
        nqw, nans = questions(seed)
        qw.copy_(nqw); ans.copy_(nans)
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        p2, c2, m2 = plain.ask_words(nqw, nans)
        torch.cuda.synchronize()
        assert torch.equal(pred, p2), seed
        assert torch.equal(hm.last_u(B).view(torch.int32), plain.last_u(B).view(torch.int32)), seed
        assert int(match.item()) == int(m2.item()) and float(cost.item()) == pytest.approx(float(c2.item()), rel=1e-5)
    assert len({int(x) for x in pred.cpu().numpy()}) > 1                         # (not a degenerate constant prediction)

"""The optional branches of the deferred queue's matcher (csrc/abi_defer.hip::match_query), driven verb by verb.

Every case runs the reference host's loop (tests/host_loop.py) on the 64-story bAbI fixture with the queue off, on and in
verify mode.  Queue off is compared with the oracle's composite forward of the same configuration (the first numerical
test of cuda_scale_fwd and cuda_activation_fwd inside a forward); queue on and verify are compared with queue off, and the
queue's statistics say which path ran.  Fixed-point and Hamming stages must be equal, float stages carry the stated
tolerance.
"""
import ctypes as C
import importlib.util

import numpy as np
import pytest

import verb_refs as vr
from conftest import ROOT, load_pkg
from host_loop import host_loop, make_state
from pyoracle import SM_CPU_POW2

pytestmark = pytest.mark.gpu

D, NQ, WSEED = 60, 40, 4321
ATT_SCALE = [-0.5, 0.25, -0.125]          # the values of the batched tests (tests/test_gpu_batch.py)
# mode 1: queries whose float read-out sits on a step of Qa(o), so that the hop state may differ by a code between two float
# implementations -- the cap of tests/test_gpu_batch.py::run_float_case, unchanged
FLOAT_EXCUSED = 1


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    load_pkg()
    import qmann_amd.abi as abi

    class Env:
        pass
    e = Env()
    e.torch, e.abi, e.lib = torch, abi, abi.lib
    e.dev = torch.device("cuda:0")
    e.up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(e.dev)
    e.ptr = lambda t: C.c_void_p(t.data_ptr())
    e.empty = lambda *s: torch.empty(s, dtype=torch.float32, device=e.dev)
    return e


@pytest.fixture(scope="module")
def data(gold):
    spec = importlib.util.spec_from_file_location("gen_golden", ROOT / "oracle" / "gen_golden.py")
    gg = importlib.util.module_from_spec(spec); spec.loader.exec_module(gg)
    b = gold("babi_qa1_test64.npz")

    class Data:
        pass
    d = Data()
    d.gg, d.V = gg, int(b["dim_input"])
    d.story, d.ques, d.ans = b["story"].astype(np.float32), b["question"].astype(np.float32), b["answer"].astype(np.float32)
    d.n_sen = b["n_sen"].astype(np.int64)
    d.offs = np.concatenate([[0], np.cumsum(d.n_sen)]).astype(np.int64)
    return d


def make_cfg(data, mode=2, iwl=5, n_hop=3, **extra):
    cfg = data.gg.babi_cfg(data.V, mode, 0, iwl=iwl, n_hop=n_hop, D=D)
    cfg.update(extra)
    return cfg


def loop(env, data, cfg, wts, defer, nq=NQ, ans=None, **kw):
    return host_loop(env, cfg, wts, data.story, data.ques, data.ans if ans is None else ans, data.n_sen, nq, defer, **kw)


def same_as_the_verbs(r, off, float_att=False):
    """queue on / verify against queue off: match, last prediction and the last query's buffers equal, cost within the rel 1e-5
    of test_deferred_queue_equals_the_verbs.  Float attention (mode 1): the batched kernel is another float implementation
    of scores, softmax and read-out, so up to FLOAT_EXCUSED queries may have a hop state one code away (the criterion of
    run_float_case); each such query moves the match count by at most 1 and the cost -- a sum of -p[label], p in [0, 1] --
    by at most 1.  The last query's buffers come from the verbs in either case and are equal."""
    if float_att:
        assert abs(r["match"] - off["match"]) <= FLOAT_EXCUSED
        if r["match"] == off["match"] and abs(r["cost"] - off["cost"]) <= 1e-5 * abs(off["cost"]):
            pass
        else:
            assert abs(r["cost"] - off["cost"]) <= FLOAT_EXCUSED * 1.0 + 1e-5 * abs(off["cost"])
    else:
        assert r["match"] == off["match"]
        assert r["cost"] == pytest.approx(off["cost"], rel=1e-5)
    assert r["last_pred"] == off["last_pred"]
    np.testing.assert_array_equal(r["last_u"], off["last_u"])
    np.testing.assert_array_equal(r["last_scores"], off["last_scores"])
    np.testing.assert_array_equal(r["last_p"], off["last_p"])
    for h in range(len(off["sv"])):
        np.testing.assert_array_equal(r["sv"][h], off["sv"][h], err_msg=f"sv hop {h}")
        np.testing.assert_array_equal(r["p"][h], off["p"][h], err_msg=f"p hop {h}")


def verbs_against_oracle(oracle, data, cfg, wts, off, order=None, ans=None, ce_mode=3):
    """queue off against oracle.forward with the same cfg: the match count over all queries (the oracle's predictions where
    its top-2 gap is above 1e-6; a closer call may fall either way), and the LAST query's hop states, per-hop probabilities
    and output probabilities.  Integer and Hamming stages equal, softmax outputs within 1e-5."""
    ans = data.ans if ans is None else ans
    order = list(range(NQ)) if order is None else list(order)
    m = oracle.make_model(cfg, wts)
    lo = hi = 0
    for i in order:
        a, b = int(data.offs[i]), int(data.offs[i + 1])
        pred, t = oracle.forward(m, data.story[a:b], data.ques[i], taps=("scores", "probs", "o", "u", "out_probs"))
        top2 = np.sort(t["out_probs"])[-2:]
        hit = int(pred == int(np.argmax(ans[i])))
        if top2[1] - top2[0] > 1e-6:
            lo += hit; hi += hit
        else:
            hi += 1
    H, float_att = cfg["n_hop"], cfg["attention_mode"] == 1
    slack = FLOAT_EXCUSED if float_att else 0
    print(f"oracle match in [{lo}, {hi}], verbs {off['match']}")
    assert lo - slack <= off["cnts"][ce_mode - 1] <= hi + slack
    frac = cfg["fmt"][0][1]
    for h in range(H):
        if not np.array_equal(off["sv"][h], t["u"][h]) and float_att:
            # run_float_case's criterion: only where the oracle's float read-out sits within 1e-3 code units of a step of Qa
            x = t["o"][h].astype(np.float64) * (1 << frac)
            bad = off["sv"][h] != t["u"][h]
            assert np.all(np.abs(x[bad] - np.rint(x[bad])) < 1e-3), f"hop {h}: state differs away from a step"
            assert FLOAT_EXCUSED >= 1
            return                                      # the later hops of this query follow another state
        np.testing.assert_array_equal(off["scores"][h], t["scores"][h], err_msg=f"scores hop {h}")
        np.testing.assert_allclose(off["p"][h], t["probs"][h], rtol=1e-5, atol=1e-7, err_msg=f"probs hop {h}")
        if float_att:
            np.testing.assert_allclose(off["o"][h], t["o"][h], rtol=1e-5, atol=2e-5, err_msg=f"o hop {h}")
        else:
            np.testing.assert_array_equal(off["o"][h], t["o"][h], err_msg=f"o hop {h}")
        np.testing.assert_array_equal(off["sv"][h], t["u"][h], err_msg=f"u hop {h}")
    err = np.abs(off["last_p"] - t["out_probs"]) / np.maximum(np.abs(t["out_probs"]), 1e-30)
    print(f"output softmax: largest relative error {err.max():.3g}")
    np.testing.assert_allclose(off["last_p"], t["out_probs"], rtol=1e-5, atol=1e-7)


def three_ways(env, oracle, data, cfg, wts, batched=True, with_oracle=True, **kw):
    """off / on / verify; returns the three results"""
    float_att = cfg["attention_mode"] == 1
    s0 = env.abi.defer_stats()
    off = loop(env, data, cfg, wts, 0, **kw)
    assert off["stats"]["queries_batched"] == s0["queries_batched"]
    if with_oracle:
        verbs_against_oracle(oracle, data, cfg, wts, off, order=kw.get("order"), ans=kw.get("ans"), ce_mode=kw.get("ce_mode", 3))
    on = loop(env, data, cfg, wts, 1, **kw)
    assert on["stats"]["queries_batched"] - off["stats"]["queries_batched"] == (NQ if batched else 0)
    ver = loop(env, data, cfg, wts, 2, **kw)
    assert ver["stats"]["queries_batched"] - on["stats"]["queries_batched"] == (NQ if batched else 0)
    assert ver["stats"]["verify_mismatch"] - off["stats"]["verify_mismatch"] <= (FLOAT_EXCUSED if float_att else 0)
    same_as_the_verbs(on, off, float_att)
    same_as_the_verbs(ver, off)                   # (verify mode: the accumulators are the verbs' own)
    return off, on, ver


CASES = {
    "scale": dict(att_scale=ATT_SCALE),
    "relu": dict(en_non_lin=True),
    "relu_no_lin_map": dict(en_non_lin=True, en_lin_map=False),
    "shift_scale_relu": dict(softmax_shift_based=True, att_scale=ATT_SCALE, en_non_lin=True),       # the `feat` build
    "pow2": dict(softmax_variant=SM_CPU_POW2),
    "one_hop": dict(n_hop=1),
    "two_hops": dict(n_hop=2),
    "appx_q2_5_relu": dict(mode=3, iwl=2, en_non_lin=True),
    "float_attention": dict(mode=1),
    "binary_operand_relu": dict(fmt_bin=(0, 0), en_non_lin=True),
}


@pytest.mark.parametrize("name", list(CASES))
def test_option_through_the_queue(env, oracle, data, name):
    opts = dict(CASES[name])
    cfg = make_cfg(data, mode=opts.pop("mode", 2), iwl=opts.pop("iwl", 5), n_hop=opts.pop("n_hop", 3), **opts)
    wts = data.gg.seeded_weights(WSEED, cfg["n_hop"], D, data.V, 1.0)
    kw = dict(softmax_base=1) if name == "pow2" else {}
    three_ways(env, oracle, data, cfg, wts, **kw)


def test_validation_phase_batches_into_the_valid_accumulators(env, oracle, data):
    """cross-entropy mode 2: the run batches, the VALID accumulators move and the test and train ones stay 0"""
    cfg = make_cfg(data)
    wts = data.gg.seeded_weights(WSEED, 3, D, data.V, 1.0)
    off, on, ver = three_ways(env, oracle, data, cfg, wts, ce_mode=2)
    for r in (off, on, ver):
        assert r["costs"][1] < 0.0 and r["cnts"][1] == off["cnts"][1]
        assert r["costs"][0] == 0.0 and r["costs"][2] == 0.0 and r["cnts"][0] == 0 and r["cnts"][2] == 0


def test_training_phase_never_batches(env, oracle, data):
    """cross-entropy mode 1 (a training step's forward): nothing batches, and the train accumulators are the verbs'"""
    cfg = make_cfg(data)
    wts = data.gg.seeded_weights(WSEED, 3, D, data.V, 1.0)
    off, on, ver = three_ways(env, oracle, data, cfg, wts, batched=False, ce_mode=1)
    for r in (on, ver):
        assert r["cnts"] == off["cnts"] and r["costs"] == off["costs"]
        assert r["costs"][0] < 0.0 and r["costs"][1] == 0.0 and r["costs"][2] == 0.0


def test_relu_layer_with_a_coarser_format_stays_with_the_verbs(env, oracle, data):
    """A host whose RELU layer is Q5.0 behind hops of Q5.2: the verb re-quantises RELU(sv), the batched hop does not, so the
    matcher refuses the pattern and the run stays with the verbs.  A float RELU leaves on-grid values alone: that one batches,
    and equals both the verbs and the oracle (whose RELU carries the hop's format)."""
    cfg = make_cfg(data, en_non_lin=True)
    wts = data.gg.seeded_weights(WSEED, 3, D, data.V, 1.0)
    off, _, _ = three_ways(env, oracle, data, cfg, wts, batched=False, with_oracle=False, relu_fmt=(5, 0))
    grid = off["nl"][0] * 1.0
    assert np.array_equal(grid, np.floor(grid)) and not np.array_equal(off["sv"][0] * 1.0, np.floor(off["sv"][0]))   # (it did re-quantise)
    three_ways(env, oracle, data, cfg, wts, batched=True, with_oracle=True, relu_fixed=False)
    three_ways(env, oracle, data, cfg, wts, batched=True, with_oracle=True, relu_fmt=(6, 3))      # a finer, wider grid: unchanged values


def test_scale_updated_between_two_phases(env, oracle, data):
    """att_scale[h] is read from the device scalar when the batched model is built, and the model is cached.  A host that
    trains the scalar between two forward phases (cuda_scale_bwd, cuda_scale_w_up) must get the new value in the second
    phase: cuda_scale_w_up is a write synchronisation point and drops the model.  A plain flush keeps it."""
    cfg = make_cfg(data, att_scale=ATT_SCALE)
    wts = data.gg.seeded_weights(WSEED, 3, D, data.V, 1.0)
    st = make_state(env, cfg, int(data.n_sen[:NQ].max()), wts=wts)
    first = loop(env, data, cfg, wts, 1, state=st)
    env.lib.qmann_abi_flush()
    again = loop(env, data, cfg, wts, 1, state=st)
    assert again["stats"]["models_built"] == first["stats"]["models_built"]           # same pointers, same signature: the cache
    assert again["stats"]["queries_batched"] - first["stats"]["queries_batched"] == NQ
    # one training step of hop 0's scalar
    dim = 16
    rng = np.random.default_rng(77)
    x, gin = rng.normal(0, 1, dim).astype(np.float32), rng.normal(0, 1, dim).astype(np.float32)
    dx, dg, dgo = env.up(x), env.up(gin), env.empty(dim)
    lr, lam = C.c_float(0.5), C.c_float(0.01)
    env.lib.cuda_scale_bwd(env.ptr(dx), env.ptr(dg), env.ptr(st["sc_w"][0]), env.ptr(st["sc_w_del"][0]), env.ptr(dgo), dim,
                           True, 5, 2, 3, False)
    env.lib.cuda_scale_w_up(env.ptr(st["sc_w"][0]), env.ptr(st["sc_w_del"][0]), dim, 32, C.byref(lr), C.byref(lam), True, 5, 2, 3, False)
    w_del, _ = vr.scale_bwd(x, gin, ATT_SCALE[0])
    w_new, _ = vr.scale_w_up(ATT_SCALE[0], w_del, dim, 32, 0.5, 0.01)
    assert float(st["sc_w"][0].cpu()[0]) == float(w_new) and float(w_new) != ATT_SCALE[0]
    second = loop(env, data, cfg, wts, 1, state=st)
    assert second["stats"]["models_built"] == again["stats"]["models_built"] + 1
    assert second["stats"]["queries_batched"] - again["stats"]["queries_batched"] == NQ
    plain = loop(env, data, cfg, wts, 0, state=st)
    same_as_the_verbs(second, plain)
    cfg2 = dict(cfg, att_scale=[float(w_new)] + ATT_SCALE[1:])
    verbs_against_oracle(oracle, data, cfg2, wts, plain)
    assert not np.array_equal(second["p"][0], first["p"][0])                          # (the new scalar does change hop 0's weights)


def test_irregular_answer_rows_go_back_to_the_verbs(env, oracle, data):
    """an all-zero answer row (query 11) and one with two ones (query 23): cross_entropy_run counts every entry == 1, which the
    batched answer layer (one label per query) cannot restate -- the piece runs verb by verb, results as with the queue off"""
    ans = data.ans.copy()
    ans[11] = 0.0
    ans[23, (int(np.argmax(ans[23])) + 1) % data.V] = 1.0
    cfg = make_cfg(data)
    wts = data.gg.seeded_weights(WSEED, 3, D, data.V, 1.0)
    three_ways(env, oracle, data, cfg, wts, batched=False, with_oracle=False, ans=ans)


def test_shuffled_pools_are_cut_into_contiguous_pieces(env, oracle, data):
    """queries issued in a permuted order: every query is still batched, in more than one call, and the results are those of
    the verbs issued in the same order"""
    order = np.random.default_rng(5).permutation(NQ)
    assert np.any(np.diff(order) != 1)
    cfg = make_cfg(data)
    wts = data.gg.seeded_weights(WSEED, 3, D, data.V, 1.0)
    off, on, _ = three_ways(env, oracle, data, cfg, wts, order=order)
    assert on["stats"]["batches"] - off["stats"]["batches"] > 1


def test_hops_with_different_score_verbs_do_not_batch(env, oracle, data):
    """hop 0 scores with cuda_dot_mat_vec_fwd_appx, hop 1 with cuda_dot_mat_vec_fwd: no batched model has that shape"""
    cfg = make_cfg(data, mode=3)
    wts = data.gg.seeded_weights(WSEED, 3, D, data.V, 1.0)
    three_ways(env, oracle, data, cfg, wts, batched=False, with_oracle=False, hop_verbs=["appx", "dot", "appx"])


def test_queue_cap_drains_in_mid_phase(env, oracle, data):
    """4 352 queries (the 64 fixture queries tiled 68 times, contiguous pools) of the shift + scale + RELU configuration, whose
    queries take 31 verbs each (the stock sequence takes 25), pass the queue's capacity of 2^17 verbs: the record is drained
    in the middle of the phase and again at the end.  Match count = 68 x the 64-query run's, cost within the rel 1e-4 that
    test_answer_mfma_i8_one_pass grants reordered float atomics, last query's buffers those of the 64-query run.
    (The one long case of this file: 135 000 verb calls from Python, about 0.2 s.)"""
    reps, n = 68, 64
    cfg = make_cfg(data, softmax_shift_based=True, att_scale=ATT_SCALE, en_non_lin=True)
    wts = data.gg.seeded_weights(WSEED, 3, D, data.V, 1.0)
    base = loop(env, data, cfg, wts, 0, nq=n)
    assert base["match"] > 0 and base["cost"] < -0.1                 # (a run whose accumulators have something to show)
    story, ques, ans = np.tile(data.story[:data.offs[n]], (reps, 1)), np.tile(data.ques[:n], (reps, 1)), np.tile(data.ans[:n], (reps, 1))
    n_sen = np.tile(data.n_sen[:n], reps)
    s0 = env.abi.defer_stats()
    on = host_loop(env, cfg, wts, story, ques, ans, n_sen, reps * n, 1)
    assert on["stats"]["ops_queued"] - s0["ops_queued"] == 31 * reps * n > (1 << 17)
    assert on["stats"]["queries_batched"] - s0["queries_batched"] == reps * n
    assert on["stats"]["batches"] - s0["batches"] == 2
    assert on["match"] == reps * base["match"]
    assert on["cost"] == pytest.approx(reps * base["cost"], rel=1e-4)
    assert on["last_pred"] == base["last_pred"]
    np.testing.assert_array_equal(on["last_u"], base["last_u"])
    np.testing.assert_array_equal(on["last_scores"], base["last_scores"])
    np.testing.assert_array_equal(on["last_p"], base["last_p"])

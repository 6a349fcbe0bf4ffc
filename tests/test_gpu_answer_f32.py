"""The float answer layer (csrc/batch_answer.hip::answer_f32_impl: the fused bf16 form k_answer_mfma<T>, the serial-order
k_answer_small builds and k_answer<false>, their ranked builds) against the references of answer_f32_cases.py, case by case: the
ORDER of the serial additions on inputs whose result is their rounding history, every width branch of the fused form and both
sides of every `fits` edge of the serial one, the edges of every T and vpt class, batches from one query across every task,
wavefront and workgroup edge, planted exact ties and a label on every position of the fused select tree, a matrix that needs all
three bf16 images, a second trip of every persistent loop, and the bookkeeping (accumulated cost / match, null outputs).

Criteria (the project's own):
  serial calls   probabilities within rtol 1e-5 / atol 1e-7 of Rser's; pred is the highest arg-max of the call's OWN probabilities
  fused call     probabilities within 1e-5 absolute of R64, and within rtol 1e-5 / atol 1e-7 (every case keeps |logit| <= 16)
  pred           the reference's wherever it is decided (answer_f32_cases.decide: exact ties are never excused)
  cost           rel 2e-5 / abs 1e-5 of the reference sum; match: the count recomputed from the call's own pred, at most the
                 number of excused queries from the reference's
Every output of every call lies between 4 096-byte guards of 0xA5, checked after the call.

Sensitivity: scratch builds with one arithmetic-only, in-bounds fault each, run once against this file on an MI355X (tests failed
of 124):
  fault (one per build)                                              failed   where
  fmaf in the serial loops (k_answer, k_answer_small)                    39    all 8 order cases (99.8 % of their probabilities, up
                                                                               to 8.6 % off), 30 shape cases, ties_labels_238
  the third bf16 image of W dropped (k_answer_mfma)                      82    76 shape cases (magnitudes among them), both tie
                                                                               cases, 2 fused sweeps, 2 bookkeeping cases
  `o > bi` turned round in the fused cross-group tie                      2    ties_labels_70, ties_labels_238 (nothing else plants a tie)
  `ry & 2` dropped from the fused label select                           85    73 shape cases, both tie cases, all 8 fused sweeps, 2
                                                                               bookkeeping cases
  cost_acc reset inside k_answer_mfma's task loop                         8    the 8 fused sweeps (nothing else takes a second trip)
  cost_acc reset inside k_answer_small's query loop                       7    the 5 k_answer_small sweeps, both ranked sweeps (their
                                                                               serial reference call)
No fault reads or writes outside an array; the shipped kernels pass every test.
"""
import ctypes as C

import numpy as np
import pytest

import answer_f32_cases as cs
from answer_f32_cases import CASES, FILL, GUARD, case
from conftest import load_pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available()
    load_pkg()
    import qmann_amd.abi as abi
    import qmann_amd.model as model

    class Env:
        pass
    e = Env()
    e.torch, e.model, e.abi, e.dev = torch, model, abi, torch.device("cuda:0")
    e.n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    return e


def make_net(env, c, base):
    fmt = [(5, 2)] * 3
    cfg = dict(n_hop=3, dim_emb=c.D, dim_input=c.V, attention_mode=2, softmax_variant=base, f_fixed=True, en_lin_map=False,
               fmt=fmt, fmt_w=list(fmt), fmt_att=list(fmt), fmt_bin=fmt[0])
    return env.model.QNet(cfg, {"w_ans": np.array(c.W)}, device="cuda:0")


class Guarded:
    """an output of `n` 32-bit words between two guards, everything filled with 0xA5"""

    def __init__(self, env, n):
        self.n = n
        self.buf = env.torch.full((4 * n + 2 * GUARD,), FILL, dtype=env.torch.uint8, device=env.dev)
        self.ptr = C.c_void_p(self.buf.data_ptr() + GUARD)

    def words(self):
        return self.buf[GUARD:GUARD + 4 * self.n]

    def check(self, what):
        assert bool((self.buf[:GUARD] == FILL).all()) and bool((self.buf[GUARD + 4 * self.n:] == FILL).all()), f"the guard of {what} was written"

    def host(self, dtype):
        return self.words().cpu().numpy().view(dtype)


def _dev(env, a):
    return env.torch.from_numpy(np.ascontiguousarray(a)).to(env.dev)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def answer(env, net, call, du, dl, B, V, want_probs=True, want_cost=True, want_match=True, cost0=0.0, match0=0):
    """one call of qmann_answer_f32 (`fused`) or qmann_answer_f32_serial on guarded outputs; cost and match start from the presets"""
    torch = env.torch
    pred, probs, acc_c, acc_m = Guarded(env, B), Guarded(env, B * V if want_probs else 0), Guarded(env, 1), Guarded(env, 1)
    acc_c.words().view(torch.float32)[0] = cost0
    acc_m.words().view(torch.int32)[0] = match0
    fn = env.abi.lib.qmann_answer_f32 if call == "fused" else env.abi.lib.qmann_answer_f32_serial
    rc = fn(C.byref(net.net), _p(net.w_ans), _p(du), _p(dl), pred.ptr, probs.ptr if want_probs else None,
            acc_c.ptr if want_cost else None, acc_m.ptr if want_match else None, B, None)
    assert rc == env.abi.QMANN_OK, rc
    torch.cuda.synchronize()
    for g, what in ((pred, "pred"), (probs, "probs"), (acc_c, "cost"), (acc_m, "match")):
        g.check(what)

    class R:
        pass
    r = R()
    r.pred = pred.host(np.uint32).astype(np.int64)
    r.cost, r.match = float(acc_c.host(np.float32)[0]), int(acc_m.host(np.int32)[0])
    r.probs = probs.host(np.float32).reshape(B, V) if want_probs else None
    if B:
        assert (r.pred < V).all(), "a prediction was not written"
        assert r.probs is None or (r.probs >= 0).all(), "a probability was not written"   # (the fill is a negative float)
    return r


def ranked_call(env, net, du, B, k):
    top_idx, top_p = Guarded(env, B * k), Guarded(env, B * k)
    rc = env.abi.lib.qmann_answer_topk_f32(C.byref(net.net), _p(net.w_ans), _p(du), k, top_idx.ptr, top_p.ptr, B, None)
    assert rc == env.abi.QMANN_OK, rc
    env.torch.cuda.synchronize()
    top_idx.check("top_idx"), top_p.check("top_p")
    return top_idx.host(np.uint32).astype(np.int64).reshape(B, k), top_p.host(np.float32).reshape(B, k)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32))


def check_bookkeeping(c, r, p_ref, decided, pred_ref, lo=0, hi=None, what=""):
    hi = c.B if hi is None else hi
    labels, inside = c.labels[lo:hi].astype(np.int64), c.inside[lo:hi]
    bad = np.flatnonzero(decided[lo:hi] & (r.pred != pred_ref[lo:hi]))
    assert len(bad) == 0, f"{what}: {len(bad)} decided predictions differ, first query {lo + bad[0]}: {r.pred[bad[0]]} against {pred_ref[lo + bad[0]]}"
    assert r.match == int((r.pred[inside] == labels[inside]).sum()), what
    want_match = int((pred_ref[lo:hi][inside] == labels[inside]).sum())
    assert abs(r.match - want_match) <= int((~decided[lo:hi]).sum()), what
    want = cs.cost_of(c, p_ref, lo, hi) if not np.isscalar(p_ref) else p_ref
    print(f"{what}: cost {r.cost!r}, reference {want!r}; match {r.match}, reference {want_match}")
    assert r.cost == pytest.approx(want, rel=2e-5, abs=1e-5), what


def check_call(oracle, c, r, call, base, lo=0, hi=None):
    """the criteria of the module docstring for one call on queries lo .. hi - 1 of the case"""
    hi = c.B if hi is None else hi
    what = f"{c.name} {call} base {base}" + (f" queries {lo}..{hi - 1}" if (lo, hi) != (0, c.B) else "")
    if call == "fused" and base != 2:                                        # (beyond D 64 or V 256 the serial kernels answer: right either way)
        p_ref = cs.probs_r64(c, base)
        err = np.abs(r.probs - p_ref[lo:hi]).max()
        print(f"{what}: largest absolute error of a probability {err:.2e} (max |logit| {c.max_abs_logit:.1f})")
        assert err <= 1e-5, what
        assert c.max_abs_logit <= 16.0
        np.testing.assert_allclose(r.probs, p_ref[lo:hi], rtol=1e-5, atol=1e-7, err_msg=what)
    else:
        p_ref = cs.probs_rser(oracle, c, base)
        np.testing.assert_allclose(r.probs, p_ref[lo:hi], rtol=1e-5, atol=1e-7, err_msg=what)
    if not cs.takes_fused(c.D, c.V, base) or call != "fused":
        assert np.array_equal(r.pred, cs.highest_argmax(r.probs)), f"{what}: pred is not the highest arg-max of the call's own probabilities"
        assert oracle.argmax_hi(r.probs[0]) == r.pred[0]
    decided, pred_ref = cs.decide(c, p_ref)
    check_bookkeeping(c, r, p_ref, decided, pred_ref, lo, hi, what)


def run_both_ways(env, oracle, c, net, call, base, du, dl, lo=0, hi=None):
    """with probabilities (checked against the reference) and the production call without: the same pred and match, the same cost
    but for the order of the atomic additions"""
    hi = c.B if hi is None else hi
    r = answer(env, net, call, du[lo:hi], dl[lo:hi], hi - lo, c.V)
    check_call(oracle, c, r, call, base, lo, hi)
    n = answer(env, net, call, du[lo:hi], dl[lo:hi], hi - lo, c.V, want_probs=False)
    assert np.array_equal(n.pred, r.pred) and n.match == r.match and n.cost == pytest.approx(r.cost, rel=1e-5, abs=1e-6)
    return r


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c["family"] == "order"))
def test_serial_order_of_additions(env, oracle, monkeypatch, name):
    """cancelling column pairs (partial sums to 2^17, logits within +-4): reversed columns, a fused multiply-add, even columns then
    odd or a float64 sum each move a probability of every query by 1e-2 (CPU: O1).  qmann_answer_f32_serial, qmann_answer_f32 under
    QMANN_ANSWER_EXACT (bit-equal to it) and qmann_answer_topk_f32 (k = 3: top_p bit-equal to the serial probabilities at
    top_idx, top_idx[:, 0] = pred, in ranked order)."""
    c = case(name)
    du, dl = _dev(env, c.u), _dev(env, c.labels.view(np.int32))
    for base in c.bases:
        net = make_net(env, c, base)
        r = run_both_ways(env, oracle, c, net, "serial", base, du, dl)
        monkeypatch.setenv("QMANN_ANSWER_EXACT", "1")
        env.abi.lib.qmann_tuning_reload()
        e = answer(env, net, "fused", du, dl, c.B, c.V)
        monkeypatch.delenv("QMANN_ANSWER_EXACT")
        env.abi.lib.qmann_tuning_reload()
        assert same_bits(e.probs, r.probs) and np.array_equal(e.pred, r.pred) and e.match == r.match, f"base {base}: QMANN_ANSWER_EXACT"
        assert e.cost == pytest.approx(r.cost, rel=1e-5, abs=1e-6)
        k = min(3, c.V)
        top_idx, top_p = ranked_call(env, net, du, c.B, k)
        assert (top_idx < c.V).all() and np.array_equal(top_idx[:, 0], r.pred), f"base {base}: ranked call"
        assert same_bits(top_p, np.take_along_axis(r.probs, top_idx, axis=1)), f"base {base}: ranked probabilities"
        assert (np.diff(top_p, axis=1) <= 0).all() and all(len(set(row)) == k for row in top_idx)


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c["family"] in ("widths", "dictionaries", "batches", "magnitudes")))
def test_shapes_and_magnitudes(env, oracle, name):
    """widths: every load branch of the fused form (vec4 with the low float4 alone, an empty second K step, D < 8, D = 1, and 65,
    where the call leaves the fused form), both sides of every `fits` edge of the serial form; dictionaries: the edges of every T
    and vpt class; batches: 1 query to 257 across the task, wavefront and workgroup edges; magnitudes: a matrix whose entries need
    all three bf16 images, -0.0, denormals, u of +-127 and +-1 in every byte format (CPU: M1, M2)."""
    c = case(name)
    du, dl = _dev(env, c.u), _dev(env, c.labels.view(np.int32))
    for base in c.bases:
        net = make_net(env, c, base)
        for call in c.calls:
            run_both_ways(env, oracle, c, net, call, base, du, dl)


@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c["family"] == "ties_labels"))
def test_ties_and_labels(env, oracle, name):
    """duplicated rows inside one group of four answers, 4, 16 and 64 apart and row 0 = row V - 1, each with a query that makes it
    win; zero rows of u; a label on every (tile, lane group, register) position; labels V + 3 and 0xFFFFFFFF.  Once whole, once in
    slices of 16 queries: a wrong label pick shows in a cost of 16 terms."""
    c = case(name)
    du, dl = _dev(env, c.u), _dev(env, c.labels.view(np.int32))
    for base in c.bases:
        net = make_net(env, c, base)
        for call in c.calls:
            r = run_both_ways(env, oracle, c, net, call, base, du, dl)
            for i, (_, b) in enumerate(c.pairs):
                assert r.pred[i] == b, f"{call} base {base}: the tie of query {i} went to {r.pred[i]}, not to {b}"
            assert (r.pred[c.zero_rows] == c.V - 1).all(), f"{call} base {base}: zero rows"
            for lo in range(0, c.B, 16):
                hi = min(lo + 16, c.B)
                s = answer(env, net, call, du[lo:hi], dl[lo:hi], hi - lo, c.V)
                check_call(oracle, c, s, call, base, lo, hi)
                assert np.array_equal(s.pred, r.pred[lo:hi])


def sweep_checks(env, oracle, c, net, call, base, du, dl, want_probs):
    r = answer(env, net, call, du, dl, c.B, c.V, want_probs=want_probs)
    what = f"{c.name} base {base} ({c.B} queries, one trip {c.one_sweep})"
    check_bookkeeping(c, r, c.cost64[base], c.decided[base], c.pred64[base], what=what)
    late = np.flatnonzero(c.inside & (np.arange(c.B) >= c.one_sweep))
    assert (r.pred[late] == c.labels[late]).any()                                            # (matches of the second trip are among the count)
    if want_probs:
        p = cs.softmax64(cs.logits64(c.W, c.u), base)
        err = np.abs(r.probs - p).max()
        print(f"{what}: largest absolute error of a probability {err:.2e}")
        assert err <= 1e-5
        if call == "fused":
            np.testing.assert_allclose(r.probs, p, rtol=1e-5, atol=1e-7)
        else:
            assert np.array_equal(r.pred, cs.highest_argmax(r.probs))
            p_ser = cs.softmax64(c.Lser, 0) if base == 0 else np.stack([oracle.softmax_fwd(row, variant=base) for row in c.Lser])
            np.testing.assert_allclose(r.probs[c.sample], p_ser, rtol=1e-5, atol=1e-7)
    return r


@pytest.mark.parametrize("name", sorted(cs.SWEEP))
def test_second_trip_of_the_persistent_loop(env, oracle, name):
    """one trip of the kernel's loop + 37 queries (one trip: restated from qm_resident_groups with the device's compute units):
    cost_acc and match_acc carry over, the fused form reads its W fragments again.  pred, cost, match everywhere against R64; the
    probabilities of k_answer_mfma<16> and k_answer_small<64,4,4> too (the latter against Rser on 384 sampled queries)."""
    call, V, want_probs = cs.SWEEP[name]
    c = cs.sweep_case(name, env.n_cu)
    assert c.B > c.one_sweep and (env.n_cu != 256 or c.one_sweep == cs.SWEEP_256[name])
    du, dl = _dev(env, c.u), _dev(env, c.labels.view(np.int32))
    for base in (0, 1):
        sweep_checks(env, oracle, c, make_net(env, c, base), call, base, du, dl, want_probs)


@pytest.mark.parametrize("V", cs.SWEEP_RANKED)
def test_second_trip_of_the_ranked_builds(env, oracle, V):
    """k_answer_small<16,2,2,true> and <64,4,4,true> beyond one trip: top_p bit-equal to the serial call's probabilities at top_idx,
    top_idx[:, 0] = pred"""
    c = cs.sweep_case(f"sweep_ranked_V{V}", env.n_cu)
    du, dl = _dev(env, c.u), _dev(env, c.labels.view(np.int32))
    net = make_net(env, c, 0)
    r = sweep_checks(env, oracle, c, net, "serial", 0, du, dl, True)
    top_idx, top_p = ranked_call(env, net, du, c.B, 3)
    assert (top_idx < V).all() and np.array_equal(top_idx[:, 0], r.pred)
    assert same_bits(top_p, np.take_along_axis(r.probs, top_idx, axis=1))


@pytest.mark.parametrize("call", ["fused", "serial"])
@pytest.mark.parametrize("name", ["batch_V30_65", "batch_V200_65", "dict_257"])
def test_bookkeeping(env, oracle, name, call):
    """cost and match are ACCUMULATED: presets of -3.5 and 11 come back as preset + the batch's figures; without labels they come
    back untouched; either may be null; no query touches nothing"""
    c = case(name)
    du, dl = _dev(env, c.u), _dev(env, c.labels.view(np.int32))
    net = make_net(env, c, 0)
    base_r = answer(env, net, call, du, dl, c.B, c.V)
    check_call(oracle, c, base_r, call, 0)
    assert base_r.match > 0 and base_r.cost < -0.1
    r = answer(env, net, call, du, dl, c.B, c.V, cost0=-3.5, match0=11)
    assert r.match == 11 + base_r.match and np.array_equal(r.pred, base_r.pred)
    assert r.cost + 3.5 == pytest.approx(base_r.cost, rel=2e-5, abs=1e-5)
    r = answer(env, net, call, du, None, c.B, c.V, cost0=-3.5, match0=11)                     # answer == NULL, cost and match given
    assert r.cost == -3.5 and r.match == 11 and np.array_equal(r.pred, base_r.pred) and same_bits(r.probs, base_r.probs)
    r = answer(env, net, call, du, dl, c.B, c.V, want_probs=False, want_cost=False, match0=11, cost0=-3.5)
    assert r.match == 11 + base_r.match and r.cost == -3.5 and np.array_equal(r.pred, base_r.pred)
    r = answer(env, net, call, du, dl, c.B, c.V, want_probs=False, want_match=False, match0=11, cost0=-3.5)
    assert r.match == 11 and r.cost + 3.5 == pytest.approx(base_r.cost, rel=2e-5, abs=1e-5) and np.array_equal(r.pred, base_r.pred)
    # n_query == 0: nothing is touched (the outputs of a whole batch stay filled)
    torch = env.torch
    pred, probs, acc = Guarded(env, c.B), Guarded(env, c.B * c.V), Guarded(env, 2)
    fn = env.abi.lib.qmann_answer_f32 if call == "fused" else env.abi.lib.qmann_answer_f32_serial
    assert fn(C.byref(net.net), _p(net.w_ans), _p(du), _p(dl), pred.ptr, probs.ptr, acc.ptr, C.c_void_p(acc.ptr.value + 4), 0, None) == env.abi.QMANN_OK
    torch.cuda.synchronize()
    for g in (pred, probs, acc):
        assert bool((g.buf == FILL).all())

"""The shared-plane HAMMING hop kernels on ONE packed memory whose read-out weights SURVIVE Q(p), against the CPU oracle:
k_hops_shared_ham (qmann_hops_shared_packed), its TOP build (qmann_hops_shared_top_packed) and the slot-split pair
k_shared_split_scan_ham / k_shared_split_finish_ham (qmann_hops_shared_split_packed, qmann_hops_shared_split_top_packed).  Cases:
shared_ham_live_cases.py; generator, conditions and comparison: shared_live_cases.py; the conditions are asserted on the CPU in
test_shared_ham_live_inputs.py.

The softmax and survivor stages of these kernels are copies (ham_common.h::ham_hist_softmax_survivors, ham_slot_softmax_survivors)
of what k_hops_ham carries inline, so test_gpu_live_hops.py runs no line of them, and on shared_ham_cases.py several live rows exist
at hop 0 only and in the first 7 n_query rows (the count: test_shared_ham_live_inputs.py).  Here every (query, hop) has planted live
rows of its own -- at both ends of the memory, on both sides of scan-tile, 16-row and slice edges --, no two queries of a tile have
the same ones, and every oracle p is clear of the truncation steps of Q(p) by 1e-3.

Per case, every output inside 4 KiB guards, through live_hops_cases.check_outputs on the memory's per-query copies:
  with taps      score codes and scores equal, p rtol 1e-5 / atol 1e-7, o and u of every hop and u_out bit-equal to the oracle;
  without taps   u_out bit-equal to the oracle's (so with and without taps agree bit for bit).
ZERO queries are excused.  The attended-slots builds give that u_out too, the rows attended_cases.assert_rows computes from the
base call's `probs` tap, and in front the pair's live rows in the ORACLE's order (larger p first, equal p: lower row first).

Sensitivity.  Four arithmetic-only faults (wrong numbers; no address formed from them, no loop bound moved) were planted in scratch
builds, one per build, never committed, and this file was run once against each on an MI355X.  "Old": the 542 tests of
test_gpu_shared_ham.py and test_gpu_shared_split_ham.py that compare hop calls (oracle, copies, launcher's tile, split, forced
tiles; not the model, graph, workspace and return-code tests).  Tests that FAIL, of this file's 152 / of the old 542:
  1  ham_slot_softmax_survivors (the copy): code_lo three score codes too high                              4 /  61
     (the four tests of `v1_threshold`, whose fourth live row lies two codes above code_lo; ONE or two codes too high drop no live
     row of any input -- the shortcut keeps that margin under the threshold e >= total . 2^-frac by construction -- and cannot be
     seen by a test.  The old inputs notice this fault too, wherever random V1 rows lie just above the threshold.)
  2  ham_hist_softmax_survivors (the copy): v0_kp[d] from the probability of count d - 1                   79 / 243
     (every V0 case in every call; no V1 case)
  3  k_shared_split_finish_ham reads hop h - 1's merged bins                                               25 /  95
     (22 attended-slots tests, whose ranking of the cold rows reads the bins, and the split tests of `tiles_v0`, `many_live_v0`
     and `scale_negative_v0`.  Three tied rows at the top and cold rows at e^-200 give the SAME weights from either hop's bins:
     that is why `tiles` and `many_live` vary their rows by query + hop.  The old files see it through test_split_*, which compare
     with the unsplit call.)
  4  k_hops_shared_ham: the read-out of query t of a tile takes query t - 1's live_kp                      22 / 184
     (the unsplit, attended-slots and copies tests of `tiles`, `graded_q25`, `many_live` and `v1_threshold`: live_kp holds weight
     codes in list order, so neighbours whose live rows all carry one code and are equally many have the same list.  The split
     kernels finish one query per workgroup and have no such fault.)
Every fault is caught by this file; faults 1, 2 and 4 are also caught by the old files on their random rows, so what this file
adds there is a KNOWN position and weight of every live row (tile, 16-row and slice edges, the memory's end, hops 1 and 2, the
option cases), not the first alarm.
"""
import ctypes as C

import numpy as np
import pytest

import live_hops_cases as lc
import shared_live_cases as sl
from attended_cases import assert_rows
from conftest import load_pkg
from live_hops_cases import ALL_TAPS, FILL, GUARD
from shared_ham_live_cases import CASES, TOP_K, shared_ham_live

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


def switches(env, monkeypatch, qt=None):
    """QMANN_SHARED_QT for one launch (conftest re-reads the switches after the test)"""
    monkeypatch.delenv("QMANN_SHARED_QT", raising=False)
    if qt:
        monkeypatch.setenv("QMANN_SHARED_QT", str(qt))
    env.abi.lib.qmann_tuning_reload()


class Device:
    """a case on the device: the net, the one memory (key bytes [P][S][Dp] packed into planes by QNet.pack_planes, sign-magnitude
    values) and the queries"""

    def __init__(self, env, case):
        torch = env.torch
        self.case, self.env = case, env
        self.net = env.model.QNet(case.cfg, case.wts)
        self.nb = case.cfg["num_bit"]
        assert self.net.Dp == case.keys.shape[2]
        self.up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(env.dev)
        self.planes = self.net.pack_planes(self.up(lc.to_signmag(case.keys.copy()).view(np.int8)), self.nb)
        self.vals = self.up(lc.to_signmag(case.vals.copy()).view(np.int8))
        self.u0 = self.up(case.u0)
        self.row_planes = (self.net.Dp // 64) * self.nb * 8               # bytes of one row's planes
        assert self.planes.numel() * 8 == case.keys.shape[0] * case.S * self.row_planes
        self.strides = (0, 0) if case.tied else (case.S * self.row_planes, case.S * self.net.Dp)

    def launch(self, call, taps=ALL_TAPS, n_slices=0, k=0):
        """call: "shared" | "split" | "top" | "split_top" | "copies" (qmann_hops_packed on the per-query copies).  Returns name ->
        the WHOLE guard-filled byte buffer of u_out, of every tap in `taps` and, with k, of top_slot and top_p [B][H][k]"""
        env, case, net = self.env, self.case, self.net
        torch, abi = env.torch, env.abi
        st = case.stories()
        shapes = dict(lc.out_shapes(st), top_slot=((case.B, case.H, k), np.int32), top_p=((case.B, case.H, k), np.float32))
        names = ("u_out",) + tuple(taps) + (("top_slot", "top_p") if k else ())
        bufs = {n: torch.full((int(np.prod(shapes[n][0])) * 4 + 2 * GUARD,), FILL, dtype=torch.uint8, device=env.dev) for n in names}
        ptr = lambda n: bufs[n].data_ptr() + GUARD if n in bufs else 0
        tp = abi.Taps(ptr("codes"), ptr("scores"), ptr("probs"), ptr("o"), ptr("u"))
        tpp = C.byref(tp) if taps else None
        p = lambda t: C.c_void_p(t.data_ptr())
        ks, vs = self.strides
        head = (C.byref(net.net), p(self.planes), ks, p(self.vals), vs, case.S, p(self.u0), C.c_void_p(ptr("u_out")))
        top = (k, C.c_void_p(ptr("top_slot")), C.c_void_p(ptr("top_p")))
        ws = None
        if call in ("split", "split_top"):
            nbytes = int(abi.lib.qmann_hops_shared_split_packed_ws_bytes(C.byref(net.net), case.S, case.B))
            assert nbytes > 0
            ws = torch.empty(nbytes, dtype=torch.uint8, device=env.dev)
        if call == "shared":
            rc = abi.lib.qmann_hops_shared_packed(*head, tpp, case.B, None)
        elif call == "split":
            rc = abi.lib.qmann_hops_shared_split_packed(*head, tpp, case.B, n_slices, p(ws), nbytes, None)
        elif call == "top":
            rc = abi.lib.qmann_hops_shared_top_packed(*head, *top, case.B, None)
        elif call == "split_top":
            rc = abi.lib.qmann_hops_shared_split_top_packed(*head, *top, case.B, n_slices, p(ws), nbytes, None)
        else:
            planes = net.pack_planes(self.up(lc.to_signmag(st.keys.copy()).view(np.int8)), self.nb)
            dv = self.up(lc.to_signmag(st.vals.copy()).view(np.int8))
            ro = self.up(st.row_off.astype(np.int32))
            rc = abi.lib.qmann_hops_packed(C.byref(net.net), p(planes), st.R * self.row_planes, p(dv), st.R * net.Dp, p(ro), case.S, p(self.u0),
                                           C.c_void_p(ptr("u_out")), tpp, case.B, None)
        assert rc == abi.QMANN_OK, f"{case.name}: {call} returned {rc}"
        torch.cuda.synchronize()
        return {n: b.cpu().numpy() for n, b in bufs.items()}


def check_both(oracle, dev, call, label, **kw):
    """the call with every tap and without any, each against the oracle; returns the taps run's buffers"""
    raw = dev.launch(call, **kw)
    sl.check_outputs(oracle, dev.case, raw, label=f" ({label}, taps)")
    sl.check_outputs(oracle, dev.case, dev.launch(call, taps=(), **kw), taps=(), label=f" ({label}, no taps)")
    return raw


# ---- 1. the unsplit call under its tile sizes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_shared_packed_hops_read_live_rows(env, oracle, monkeypatch, name):
    case = shared_ham_live(name)
    dev = Device(env, case)
    for qt in case.qts:
        switches(env, monkeypatch, qt)
        tile = env.abi.lib.qmann_hops_shared_packed_tile(C.byref(dev.net.net), case.S, case.B)
        assert tile == qt or not qt                         # the switch took effect (every case fits LDS with eight queries)
        check_both(oracle, dev, "shared", f"tiles of {tile}")
        print(f"{name}: tiles of {tile} queries: {case.B} queries equal the oracle in every tap and in u_out, 0 excused")


# ---- 2. the slot-split call -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_split_packed_hops_read_live_rows(env, oracle, monkeypatch, name):
    """forced slice counts that cut between the live rows of a pair and of which one leaves a short last slice
    (test_shared_ham_live_inputs.py), the library's own choice (0), and the largest forced tile of the case with the last count --
    each against the oracle, not against the unsplit call"""
    case = shared_ham_live(name)
    dev = Device(env, case)
    switches(env, monkeypatch)
    for n in (0,) + case.slices:
        check_both(oracle, dev, "split", f"{n} slices", n_slices=n)
    switches(env, monkeypatch, case.qts[-1])
    check_both(oracle, dev, "split", f"{case.slices[-1]} slices, tiles of {case.qts[-1]}", n_slices=case.slices[-1])
    print(f"{name}: split into {(0,) + case.slices} slices: {case.B} queries equal the oracle in every tap and in u_out, 0 excused")


# ---- 3. the attended-slots builds ---------------------------------------------------------------------------------------------------
def top_tensors(env, case, raw, k):
    view = lambda n, dt: env.torch.from_numpy(raw[n][GUARD:-GUARD].copy().view(dt).reshape(case.B, case.H, k))
    for n in ("top_slot", "top_p"):
        assert (raw[n][:GUARD] == FILL).all() and (raw[n][-GUARD:] == FILL).all(), f"{case.name}: the guard of {n} was written"
    return view("top_slot", np.int32), view("top_p", np.float32)


def leading_rows(ref, live, q, h, k):
    """the pair's live rows in the oracle's order -- larger p first, equal p: lower row first --, cut to k, and whether that order is
    DECIDED: neighbouring oracle values exactly equal, or more than 1e-5 (relative) apart"""
    p = ref[q]["probs"][h].astype(np.float64)
    rows = sorted(live[(q, h)], key=lambda r: (-p[r], r))
    decided = all(p[a] == p[b] or p[a] - p[b] > 1e-5 * p[a] for a, b in zip(rows, rows[1:]))
    return rows[:k], decided


@pytest.mark.parametrize("k", TOP_K)
@pytest.mark.parametrize("name", sorted(CASES))
def test_attended_slots_builds_read_live_rows(env, oracle, monkeypatch, name, k):
    case = shared_ham_live(name)
    dev = Device(env, case)
    switches(env, monkeypatch, case.qts[-1])
    base = dev.launch("shared")
    sl.check_outputs(oracle, case, base, label=" (base call)")
    probs = lc.payload(case.stories(), base, "probs").reshape(case.H, case.B, case.S)
    ref = lc.reference(oracle, case.stories())
    live = sl.live_sets(case, ref)
    ordered = 0
    for call, n in (("top", 0), ("split_top", case.slices[0]), ("split_top", case.slices[-1])):
        raw = dev.launch(call, taps=(), n_slices=n, k=k)
        what = f"{name}, {call}, k={k}, {n} slices"
        sl.check_outputs(oracle, case, {"u_out": raw["u_out"]}, taps=(), label=f" ({what})")        # u_out bit-equal to the oracle's
        slot_t, p_t = top_tensors(env, case, raw, k)
        assert_rows(slot_t, p_t, probs, k, what)
        slot = slot_t.numpy()
        for (q, h) in live:
            rows, decided = leading_rows(ref, live, q, h, k)
            got = slot[q, h, :len(rows)].tolist()
            if decided:
                assert got == rows, f"{what} q{q} h{h}: the leading attended slots {got} are not the live rows in the oracle's order {rows}"
                ordered += 1
            else:
                assert set(got) <= live[(q, h)], f"{what} q{q} h{h}: the leading attended slots {got} are not live rows {sorted(live[(q, h)])}"
    assert ordered >= 3 * case.B * case.H // 2, f"{name}: the oracle decides the order in {ordered} of {3 * case.B * case.H} rows only"


# ---- 4. the per-story call on copies of the planes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c.get("copies")))
def test_hops_packed_on_copies_is_bit_equal(env, oracle, monkeypatch, name):
    case = shared_ham_live(name)
    dev = Device(env, case)
    switches(env, monkeypatch, case.qts[-1])
    shared = dev.launch("shared")
    copies = check_both(oracle, dev, "copies", "qmann_hops_packed on copies")
    for n in ("u_out",) + ALL_TAPS:
        assert np.array_equal(shared[n], copies[n]), f"{name}: {n} of the shared call and of qmann_hops_packed on copies differ"

"""The fixed-point shared-plane hop kernels on ONE memory whose read-out weights SURVIVE Q(p), against the CPU oracle: k_hops_shared
(qmann_hops_shared_i8), its TOP build (qmann_hops_shared_top_i8) and the slot-split pair k_shared_split_scan /
k_shared_split_finish (qmann_hops_shared_split_i8, qmann_hops_shared_split_top_i8).  Cases, conditions and the comparison:
shared_live_cases.py; the conditions are asserted on the CPU in test_shared_live_inputs.py.

On the memories of shared_cases.py no memory longer than 257 slots has a row with a non-zero weight code (706 of 1 132 (query,
hop) pairs have none), so wherever test_gpu_shared.py and test_gpu_shared_split.py vary a tile size, a softmax variant, a weight
format or a tied plane, hist_softmax_survivors -> finish_hop ran with o = 0.  Here every (query, hop) has planted live rows of
its own -- at both ends of the memory, on both sides of scan-tile, 16-row and slice edges --, no two queries of a tile have the
same ones, and every oracle p is clear of the truncation steps of Q(p) by 1e-3.

Per case, every output inside 4 KiB guards, through live_hops_cases.check_outputs on the memory's per-query copies:
  with taps      score codes and scores equal, p rtol 1e-5 / atol 1e-7, o and u of every hop and u_out bit-equal to the oracle;
  without taps   u_out bit-equal to the oracle's (so with and without taps agree bit for bit).
ZERO queries are excused.  The attended-slots builds give that u_out too (attended_select runs on the query's LDS slice behind
finish_hop and must leave u_f alone) and the rows attended_cases.assert_rows computes from the base call's `probs` tap.

Sensitivity.  Three arithmetic-only faults (wrong numbers, no address or loop bound moved out of range) were planted in scratch
builds of batch_hops_shared.hip and batch_hops_shared_split.hip, one per build, never committed, and this file was run once
against each on an MI355X.  Tests that FAIL, of this file's 67:
  1  readout_sparse leaves out the last entry of a survivor list whose length is no multiple of four      63
     (all but the four tests of `graded_q25`, whose every pair has four live rows)
  2  k_hops_shared: query t of a tile searches its survivors with query t - 1's kplut                      10
     (the unsplit, attended-slots and copies tests of `tiles`, `graded_q25` and `q25_native`.  The table is indexed by score
     code, so neighbours whose live rows all sit at the top code have the SAME table: that is why the odd queries of `tiles`
     hold one live row a quarter under the top.  The split kernels finish one query per workgroup and have no such fault.)
  3  readout_sparse reads every hop's values from plane 0                                                 62
     (all but the five tests of `tied_plane`, which has one plane)
"""
import ctypes as C

import numpy as np
import pytest

import live_hops_cases as lc
import shared_live_cases as sl
from attended_cases import assert_rows
from conftest import load_pkg
from live_hops_cases import ALL_TAPS, FILL, GUARD
from shared_live_cases import CASES, TOP_K, shared_live

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


def switches(env, monkeypatch, settings, qt=None):
    """the QMANN_* switches of one launch (conftest re-reads them after the test)"""
    for k in ("QMANN_SHARED_QT", "QMANN_NO_W7"):
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(settings, **({"QMANN_SHARED_QT": str(qt)} if qt else {})).items():
        monkeypatch.setenv(k, v)
    env.abi.lib.qmann_tuning_reload()


class Device:
    """a case on the device: the net, the one memory (sign-magnitude bytes [P][S][Dp]) and the queries"""

    def __init__(self, env, case):
        torch = env.torch
        self.case, self.env = case, env
        self.net = env.model.QNet(case.cfg, case.wts)
        assert self.net.Dp == case.keys.shape[2]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(env.dev)
        self.keys, self.vals = up(lc.to_signmag(case.keys.copy()).view(np.int8)), up(lc.to_signmag(case.vals.copy()).view(np.int8))
        self.u0 = up(case.u0)
        self.hop_stride = 0 if case.tied else case.S * self.net.Dp

    def launch(self, call, taps=ALL_TAPS, n_slices=0, k=0):
        """call: "shared" | "split" | "top" | "split_top" | "copies" (qmann_hops_i8 on the per-query copies).  Returns name -> the
        WHOLE guard-filled byte buffer of u_out, of every tap in `taps` and, with k, of top_slot and top_p [B][H][k]"""
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
        head = (C.byref(net.net), p(self.keys), p(self.vals), self.hop_stride, case.S, p(self.u0), C.c_void_p(ptr("u_out")))
        ws = None
        if call in ("split", "split_top"):
            nbytes = int(abi.lib.qmann_hops_shared_split_ws_bytes(C.byref(net.net), case.S, case.B))
            ws = torch.empty(max(nbytes, 16), dtype=torch.uint8, device=env.dev)
        if call == "shared":
            rc = abi.lib.qmann_hops_shared_i8(*head, tpp, case.B, None)
        elif call == "split":
            rc = abi.lib.qmann_hops_shared_split_i8(*head, tpp, case.B, n_slices, p(ws), nbytes, None)
        elif call == "top":
            rc = abi.lib.qmann_hops_shared_top_i8(*head, k, C.c_void_p(ptr("top_slot")), C.c_void_p(ptr("top_p")), case.B, None)
        elif call == "split_top":
            rc = abi.lib.qmann_hops_shared_split_top_i8(*head, k, C.c_void_p(ptr("top_slot")), C.c_void_p(ptr("top_p")), case.B, n_slices,
                                                        p(ws), nbytes, None)
        else:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(env.dev)
            dk, dv = up(lc.to_signmag(st.keys.copy()).view(np.int8)), up(lc.to_signmag(st.vals.copy()).view(np.int8))
            ro = up(st.row_off.astype(np.int32))
            rc = abi.lib.qmann_hops_i8(C.byref(net.net), p(dk), p(dv), st.R * net.Dp, p(ro), case.S, p(self.u0), C.c_void_p(ptr("u_out")), tpp,
                                       case.B, None)
        assert rc == abi.QMANN_OK, f"{case.name}: {call} returned {rc}"
        torch.cuda.synchronize()
        return {n: b.cpu().numpy() for n, b in bufs.items()}


def check_both(oracle, dev, call, label, **kw):
    """the call with every tap and without any, each against the oracle; returns the taps run's buffers"""
    raw = dev.launch(call, **kw)
    sl.check_outputs(oracle, dev.case, raw, label=f" ({label}, taps)")
    sl.check_outputs(oracle, dev.case, dev.launch(call, taps=(), **kw), taps=(), label=f" ({label}, no taps)")
    return raw


# ---- 1. the unsplit call under its tile sizes and switches -----------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_shared_hops_read_live_rows(env, oracle, monkeypatch, name):
    case = shared_live(name)
    dev = Device(env, case)
    for settings in case.envs:
        for qt in case.qts:
            switches(env, monkeypatch, settings, qt)
            tile = env.abi.lib.qmann_hops_shared_tile(case.S, case.B)
            assert tile == qt or not qt                     # the switch took effect: this run is on tiles of qt queries
            check_both(oracle, dev, "shared", f"tiles of {tile}, {settings or 'no switch'}")
            print(f"{name}: tiles of {tile} queries, {settings or 'no switch'}: {case.B} queries equal the oracle in every tap and in u_out, 0 excused")


# ---- 2. the slot-split call -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(CASES))
def test_split_hops_read_live_rows(env, oracle, monkeypatch, name):
    """forced slice counts that cut between the live rows of a pair (test_shared_live_inputs.py), the library's own choice (0),
    and the largest forced tile of the case with the first count"""
    case = shared_live(name)
    dev = Device(env, case)
    switches(env, monkeypatch, {})
    for n in (0,) + case.slices:
        check_both(oracle, dev, "split", f"{n} slices", n_slices=n)
    switches(env, monkeypatch, {}, case.qts[-1])
    check_both(oracle, dev, "split", f"{case.slices[-1]} slices, tiles of {case.qts[-1]}", n_slices=case.slices[-1])
    print(f"{name}: split into {(0,) + case.slices} slices: {case.B} queries equal the oracle in every tap and in u_out, 0 excused")


# ---- 3. the attended-slots builds ---------------------------------------------------------------------------------------------------
def top_tensors(env, case, raw, k):
    view = lambda n, dt: env.torch.from_numpy(raw[n][GUARD:-GUARD].copy().view(dt).reshape(case.B, case.H, k))
    for n in ("top_slot", "top_p"):
        assert (raw[n][:GUARD] == FILL).all() and (raw[n][-GUARD:] == FILL).all(), f"{case.name}: the guard of {n} was written"
    return view("top_slot", np.int32), view("top_p", np.float32)


@pytest.mark.parametrize("k", TOP_K)
@pytest.mark.parametrize("name", sorted(CASES))
def test_attended_slots_builds_read_live_rows(env, oracle, monkeypatch, name, k):
    case = shared_live(name)
    dev = Device(env, case)
    switches(env, monkeypatch, {}, case.qts[-1])
    base = dev.launch("shared")
    sl.check_outputs(oracle, case, base, label=" (base call)")
    probs = lc.payload(case.stories(), base, "probs").reshape(case.H, case.B, case.S)
    for call, n in (("top", 0), ("split_top", case.slices[0]), ("split_top", case.slices[-1])):
        raw = dev.launch(call, taps=(), n_slices=n, k=k)
        what = f"{name}, {call}, k={k}, {n} slices"
        sl.check_outputs(oracle, case, {"u_out": raw["u_out"]}, taps=(), label=f" ({what})")
        assert_rows(*top_tensors(env, case, raw, k), probs, k, what)
    # the weights the rows carry are the live rows' where there are k or fewer of them in front
    live = sl.live_sets(case, lc.reference(oracle, case.stories()))
    slot = top_tensors(env, case, raw, k)[0].numpy()
    for (q, h), lv in live.items():
        n = min(k, len(lv))
        assert set(slot[q, h, :n].tolist()) <= lv, f"{name} q{q} h{h}: the first {n} attended slots {slot[q, h, :n]} are not live rows {sorted(lv)}"


# ---- 4. the per-story call on copies of the plane -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(n for n, c in CASES.items() if c.get("copies")))
def test_hops_i8_on_copies_is_bit_equal(env, oracle, monkeypatch, name):
    case = shared_live(name)
    dev = Device(env, case)
    switches(env, monkeypatch, {}, case.qts[-1])
    shared = dev.launch("shared")
    copies = check_both(oracle, dev, "copies", "qmann_hops_i8 on copies")
    for n in ("u_out",) + ALL_TAPS:
        assert np.array_equal(shared[n], copies[n]), f"{name}: {n} of the shared call and of qmann_hops_i8 on copies differ"

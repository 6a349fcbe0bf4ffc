"""The per-story hop kernels on memories whose read-out weights SURVIVE Q(p), against the CPU oracle (cases, conditions and the
comparison: live_hops_cases.py; the conditions are asserted on the CPU in test_live_hops_inputs.py).

On the random memories of test_gpu_mid.py, test_gpu_lean.py, test_gpu_quad.py and test_gpu_batch.py no row of a story longer than
about 16 rows has a non-zero weight code, so survivor selection, the value fetch and the weighted sum of k_hops_mid, k_hops_lean
(both read-out forms), k_hops_quad (both forms, and the split), k_hops_small, k_hops_fixed and k_hops_ham run there with o = 0.
Here every (query, hop) has planted live rows -- at both ends of the story, on both sides of the kernels' 64-row groups, 16-row
chunks and lanes 15 / 16, 31 / 32 and 63, in the last partial group, in the neighbour's first row behind a hot last row, and
just in front of and behind the max_slots cut -- and every oracle p is clear of the truncation steps of Q(p) by 1e-3.

Per case, every output inside 4 KiB guards:
  with taps (the general kernels)     score codes and scores equal, p rtol 1e-5 / atol 1e-7, o and u of every hop bit-equal;
  without taps (the production form)  u_out bit-equal to the oracle's (ReLU applied where the configuration has it).
ZERO queries are excused.  The form each launch takes is printed (live_hops_cases.form_of restates hops_host.h::hop_plan).

Sensitivity.  Six arithmetic-only faults (wrong numbers, no address or loop bound moved) were planted in scratch builds of the
library, one per build, never committed, and run on an MI355X.  Tests that FAIL, of this file's 53 and of the 42 /
140 / 118 / 405 of test_gpu_mid.py / test_gpu_lean.py / test_gpu_quad.py / test_gpu_batch.py:
                                                                            here   mid   lean   quad   batch
  1  k_hops_mid skips the survivors of its last partial group                 13    11      0      0       4
  2  k_hops_mid takes a survivor's value row at row - 1 (clamped to row 0)    13    20      0      0       7
  3  lean, sparse read-out, mode 2: the second fetch round is not added        2     0      8      8       6
  4  k_hops_fixed weights only the top score bin                               9     4      0      0       7
  5  every kernel reads every hop's values from hop 0's plane                 52    22      0      3     274
  6  k_hops_quad, mode 2: query 3 of a quad gets query 2's weights             4     0      1     38       2
(Row 4 is why the Q5.2 streaming cases hold one of their three live rows a quarter under the top score.)
Here: 1, 2 every mid case, the mid cut and the persistent mid grid; 3 the two sparse cases with more than four survivors; 4 every
case with a live row off the top bin; 5 all but the one-hop case; 6 the three quad cases and the persistent four-chunk grid.
The old files see each fault as well, through their Q2.5 / Q0.7 formats and their stories of up to 16 rows -- except that
test_gpu_lean.py, which holds the lean kernel against the general one, is blind to a fault both share (5: 0 of 140).
"""
import ctypes as C

import numpy as np
import pytest

import live_hops_cases as lc
from conftest import load_pkg
from live_hops_cases import ALL_TAPS, CASES, FILL, GUARD

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


def switches(env, monkeypatch, case):
    for k in ("QMANN_NO_LEAN", "QMANN_LEAN_SPARSE", "QMANN_QUAD_MIN_QUERIES", "QMANN_NO_SCAN_STOP", "QMANN_NO_MID", "QMANN_NO_QUAD",
              "QMANN_NO_QUAD_LONG"):
        monkeypatch.delenv(k, raising=False)
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    env.abi.lib.qmann_tuning_reload()                     # (read once per process; conftest re-reads them after the test)


def launch(env, case, taps=ALL_TAPS):
    """qmann_hops_i8 (or qmann_hops_packed) on the case; returns name -> the whole guard-filled buffer of u_out and of every tap"""
    torch, abi = env.torch, env.abi
    net = env.model.QNet(case.cfg, case.wts)
    assert net.Dp == case.keys.shape[2]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(env.dev)
    dk, dv = up(lc.to_signmag(case.keys).view(np.int8)), up(lc.to_signmag(case.vals).view(np.int8))
    ro, u0 = up(case.row_off.astype(np.int32)), up(case.u0)
    shapes = lc.out_shapes(case)
    bufs = {k: torch.full((int(np.prod(shapes[k][0])) * 4 + 2 * GUARD,), FILL, dtype=torch.uint8, device=env.dev) for k in ("u_out",) + tuple(taps)}
    ptr = lambda k: bufs[k].data_ptr() + GUARD if k in bufs else 0
    tp = abi.Taps(ptr("codes"), ptr("scores"), ptr("probs"), ptr("o"), ptr("u"))
    p = lambda t: C.c_void_p(t.data_ptr())
    if case.packed:
        nb = case.cfg["num_bit"]
        planes = net.pack_planes(dk, nb)
        rc = abi.lib.qmann_hops_packed(C.byref(net.net), p(planes), case.R * (net.Dp // 64) * nb * 8, p(dv), case.R * net.Dp, p(ro), case.max_slots,
                                       p(u0), C.c_void_p(ptr("u_out")), C.byref(tp) if taps else None, case.B, None)
    else:
        rc = abi.lib.qmann_hops_i8(C.byref(net.net), p(dk), p(dv), case.R * net.Dp, p(ro), case.max_slots, p(u0), C.c_void_p(ptr("u_out")),
                                   C.byref(tp) if taps else None, case.B, None)
    assert rc == abi.QMANN_OK, f"{case.name}: the hop call returned {rc}"
    torch.cuda.synchronize()
    return {k: b.cpu().numpy() for k, b in bufs.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_live_rows_against_the_oracle(env, oracle, monkeypatch, name):
    case = lc.build(oracle, name)
    ref = lc.reference(oracle, case)
    switches(env, monkeypatch, case)
    if case.taps_too:
        n = lc.check_outputs(case, ref, launch(env, case))
        print(f"{name}: taps, {lc.form_of(case, True)}: {n} queries equal the oracle in every tap, 0 excused")
    n = lc.check_outputs(case, ref, launch(env, case, taps=()), taps=(), label=" (no taps)")
    print(f"{name}: no taps, {lc.form_of(case, False)}: u_out of {n} queries equals the oracle's, 0 excused")


@pytest.mark.parametrize("name", sorted(lc.PERSISTENT))
def test_persistent_grid_walks_planted_stories(env, oracle, monkeypatch, name):
    """Twice as many queries as the device can hold at once, and 37 more: rt.h::qm_launch_persistent launches no more workgroups
    than are resident, a CU holds at most 32 wavefronts, and a wavefront of k_hops_mid or k_hops_lean walks one query, one of
    k_hops_quad four (live_hops_cases.PERSISTENT_QUERIES_PER_CU: an upper bound, so the real grid is no larger).  Every
    workgroup of the grid therefore takes a second round at least.  Each query is a copy of one of 64 planted stories, in
    shuffled order, and must give its original's oracle result."""
    cus = env.torch.cuda.get_device_properties(0).multi_processor_count
    case = lc.build_persistent(oracle, name, 2 * lc.PERSISTENT_QUERIES_PER_CU[name] * cus + 37)
    switches(env, monkeypatch, case)
    ref = lc.reference(oracle, case)
    n = lc.check_outputs(case, ref, launch(env, case, taps=()), taps=(), label=" (no taps)")
    print(f"{name}: {lc.form_of(case, False)}, {n} queries on {cus} CUs equal their originals' oracle results, 0 excused")

"""ATTENTION_MODE 1 (csrc/batch_hops_float.hip) with SPREAD softmax weights, against float_hop_ref.py.

test_gpu_batch.py::run_float_case feeds this kernel scores of a standard deviation in the hundreds: nearly every weight is zero
and the dense float read-out is tested as a copy of one value row.  The cases of float_hops_cases.py choose the score scale so
that the weights are spread (asserted on the CPU in test_float_hops_inputs.py), which puts weight on every row a moved-back tile
repeats, on every row group of the __shfl_xor fold, on every wavefront's partial and on every decoded byte.

Per case, through qmann_hops_i8 with every tap on and every output inside guard-filled buffers (float_hops_cases.check_outputs):
  scores, score codes   equal;
  p                     rtol 1e-5, atol 1e-7;
  o                     |o_gpu[c] - o64[c]| <= (1e-5 + (S + 8) 2^-24) . sum_r p[r] |C[r][c]|  (derived in float_hop_ref.py);
  u                     bit-equal outside `near`; inside, equal or the one code across that step -- and `near`, recomputed
                        from the inputs the kernel had, stays within 1 % of the columns;
  u_out                 relu_if(u[H-1]);
  guards                4 KiB on both sides of u_out and of every tap untouched; per-row taps of rows no query reads (in front of
                        row_off[0], past a cut) keep their fill.
Hop h's reference input is the kernel's own tapped u[h-1] (asserted to lie on its grid), so a permitted difference cannot cascade.
"""
import ctypes as C

import numpy as np
import pytest

import float_hops_cases as fc
from conftest import load_pkg
from float_hops_cases import ALL_TAPS, CASES, FILL, GUARD, build

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


def launch(env, case, taps=ALL_TAPS):
    """qmann_hops_i8 on the case; returns name -> the whole guard-filled buffer of u_out and of every tap asked for"""
    torch, abi = env.torch, env.abi
    net = env.model.QNet(case.cfg, case.wts)
    assert net.Dp == case.kb.shape[2]
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(env.dev)
    dk, dv = up(case.kb.view(np.int8)), up(case.vb.view(np.int8))
    ro, u0 = up(case.row_off.view(np.int32)), up(case.u0)
    shapes = fc.out_shapes(case)
    bufs = {k: torch.full((int(np.prod(shapes[k][0])) * 4 + 2 * GUARD,), FILL, dtype=torch.uint8, device=env.dev) for k in ("u_out",) + tuple(taps)}
    ptr = lambda k: bufs[k].data_ptr() + GUARD if k in bufs else 0
    tp = abi.Taps(ptr("codes"), ptr("scores"), ptr("probs"), ptr("o"), ptr("u"))
    stride = 0 if case.tied else case.R * net.Dp
    rc = abi.lib.qmann_hops_i8(C.byref(net.net), C.c_void_p(dk.data_ptr()), C.c_void_p(dv.data_ptr()), stride, C.c_void_p(ro.data_ptr()),
                               case.max_slots, C.c_void_p(u0.data_ptr()), C.c_void_p(ptr("u_out")), C.byref(tp) if taps else None,
                               case.B, None)
    assert rc == abi.QMANN_OK, f"{case.name}: qmann_hops_i8 returned {rc}"
    torch.cuda.synchronize()
    return {k: b.cpu().numpy() for k, b in bufs.items()}


@pytest.mark.parametrize("name", sorted(n for n in CASES if CASES[n]["family"] not in ("tied", "taps")))
def test_float_hops_spread_weights(env, name):
    case = build(name)
    raw = launch(env, case)
    stats = fc.check_outputs(case, raw)
    print(f"{name}: {stats['differ']} of {stats['cols']} state columns differ from the float64 reference, all among the {stats['near']} near a step")
    # the same call without taps (the same kernel, tap pointers null): the final state alone, inside its guards
    plain = launch(env, case, taps=())
    fc.check_outputs(case, plain, taps=(), label=" (no taps)")
    np.testing.assert_array_equal(fc.payload(case, plain, "u_out").view(np.uint32), fc.payload(case, raw, "u_out").view(np.uint32))


def test_float_hops_tied_planes(env):
    """hop_stride = 0: one plane serves every hop.  Taps need distinct planes, so the tied launch is held against the launch on
    three copies of the plane, which goes through the whole comparison."""
    tied = build("tied_planes")
    three = fc.untied(tied)
    raw = launch(env, three)
    stats = fc.check_outputs(three, raw)
    assert stats["cols"] > 0
    out = launch(env, tied, taps=())
    fc.check_outputs(tied, out, taps=())
    np.testing.assert_array_equal(fc.payload(tied, out, "u_out").view(np.uint32), fc.payload(three, raw, "u_out").view(np.uint32))


def test_float_hops_every_tap_combination(env):
    """all taps, each tap alone, none: u_out is the same in every combination, and a tap is the same alone as among the others"""
    case = build("taps")
    full = launch(env, case)
    fc.check_outputs(case, full)
    for combo in fc.TAP_COMBOS[1:]:
        raw = launch(env, case, taps=combo)
        fc.check_outputs(case, raw, taps=combo, label=f" taps={combo}")
        for k in ("u_out",) + tuple(combo):
            np.testing.assert_array_equal(raw[k], full[k], err_msg=f"{k} with taps={combo}")
    # QNet.hops, the call every other test of this kernel goes through, hands back the same arrays
    torch = env.torch
    net = env.model.QNet(case.cfg, case.wts)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(env.dev)
    u_out, t = net.hops(up(case.kb.view(np.int8)), up(case.vb.view(np.int8)), up(case.row_off.view(np.int32)), case.max_slots, up(case.u0), taps=True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(u_out.cpu().numpy(), fc.payload(case, full, "u_out"))
    np.testing.assert_array_equal(t.u.cpu().numpy(), fc.payload(case, full, "u"))
    np.testing.assert_array_equal(t.o.cpu().numpy(), fc.payload(case, full, "o"))


def test_float_launcher_refuses_by_its_own_lds_size(env):
    """The float kernel keeps a float p per slot where the fixed-point kernels keep a score byte: its launcher accepts max_slots
    while fixed + roundup16(4 . max_slots) <= 160 KiB - 1 KiB, fixed = qmann_hops_lds_bytes(0).  The refusals come back as codes
    with nothing launched."""
    torch, abi, model = env.torch, env.abi, env.model
    cap = 160 * 1024 - 1024
    fixed = abi.lib.qmann_hops_lds_bytes(0)
    assert fixed % 16 == 0 and abi.lib.qmann_hops_lds_bytes(16) == fixed + 16
    largest = (cap - fixed) // 16 * 16 // 4                      # 4 . largest is a multiple of 16: one more slot rounds up by 16
    assert fixed + (4 * largest + 15) // 16 * 16 <= cap < fixed + (4 * (largest + 1) + 15) // 16 * 16
    D, H = 128, 3
    cfg = dict(build("width_d128").cfg, att_scale=None)
    wts = build("width_d128").wts
    net_float = model.QNet(cfg, wts)
    net_fixed = model.QNet(dict(cfg, attention_mode=2), wts)
    dk = torch.zeros((H, 8, net_float.Dp), dtype=torch.int8, device=env.dev)
    ro = torch.tensor([0, 8], dtype=torch.int32, device=env.dev)
    u0 = torch.zeros((1, D), dtype=torch.float32, device=env.dev)
    u1 = torch.full((1, D), 7.0, dtype=torch.float32, device=env.dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    call = lambda net, ms: abi.lib.qmann_hops_i8(C.byref(net.net), p(dk), p(dk), 8 * net.Dp, p(ro), ms, p(u0), p(u1), None, 1, None)
    assert call(net_float, largest + 1) == abi.QMANN_ERANGE
    torch.cuda.synchronize()
    assert (u1 == 7.0).all(), "a refused call launches nothing"
    assert call(net_float, largest) == abi.QMANN_OK                # one 8-slot story of zeros under the largest reservation
    torch.cuda.synchronize()
    assert (u1 == 0.0).all()
    u1.fill_(7.0)
    assert call(net_fixed, largest + 1) == abi.QMANN_OK            # a score byte per slot: far inside the LDS
    torch.cuda.synchronize()
    assert (u1 == 0.0).all()

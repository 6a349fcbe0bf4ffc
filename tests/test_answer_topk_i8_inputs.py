"""Ranked int8 answers, CPU side: the inputs of answer_topk_i8_cases.py do what each is for, and qmann_answer_topk_i8's refusals --
codes and their order -- on the loaded library.  A refused call launches nothing, so no GPU is needed: the pointers are host
arrays that a refused call must not touch."""
import ctypes as C
import re

import numpy as np
import pytest

from answer_i8_cases import case, prob64
from answer_topk_i8_cases import (FORMAT_PAIRS, GPU_CASES, KS, RAMPS, float_ranking, ramp_kind, ranking, tcase, top_prob64)
from conftest import ROOT, load_pkg


@pytest.fixture(scope="module")
def abi():
    load_pkg()
    import qmann_amd.abi as a
    return a


def test_a_tie_straddles_position_k():
    """for every k of the GPU test some case has a query whose k-th and (k+1)-th answers carry the same code: the cut falls inside
    a tie and only the index rule decides which of them is listed"""
    for k in KS:
        found = []
        for name in GPU_CASES:
            c = tcase(name)
            if c.V <= k:
                continue
            Ks = -np.sort(-c.K, axis=1)
            if (Ks[:, k - 1] == Ks[:, k]).any():
                found.append(name)
        assert found, k
        if k in (5, 16):
            assert set(RAMPS) <= set(found)


def test_the_float_order_differs_from_the_logit_order_somewhere():
    """scale 2^0: logits hundreds apart, every probability but the first few underflows to 0 as a float, and a ranking of the
    rounded probabilities orders those by index where this call keeps ordering them by logit"""
    name = "fmt_u7.0_w7.0"
    assert name in FORMAT_PAIRS
    c = tcase(name)
    V = c.V
    allv = np.broadcast_to(np.arange(V), (c.B, V))
    differ = 0
    for base in (0, 1):
        p32 = top_prob64(name, base, allv).astype(np.float32)
        fr = float_ranking(p32, 16)
        lr = ranking(name)[:, :16]
        rows = (fr != lr).any(1)
        differ += int(rows.sum())
        # ... and where the first 16 probabilities are pairwise distinct the two orders coincide (on the first 15: the 16th may
        # still tie with an answer that is not listed)
        pl = np.take_along_axis(p32, lr, axis=1)
        distinct = (np.diff(pl, axis=1) < 0).all(1)
        assert np.array_equal(fr[distinct, :15], lr[distinct, :15])
    assert differ > 0


@pytest.mark.parametrize("name", sorted(RAMPS))
def test_the_ramps_are_monotone_with_plateaus(name):
    c = tcase(name)
    kind = ramp_kind(c.B)
    assert set(kind) == {1, -1, 0}
    V = c.V
    top_plateau = V - 287                                  # rows 287 .. V - 1 are clipped to +127
    for q in range(c.B):
        d = np.diff(c.K[q])
        if kind[q] == 1:
            assert (d >= 0).all() and (d[33:286] > 0).all()
            assert (c.K[q] == c.K[q].max()).sum() == top_plateau and c.K[q, 287] == c.K[q, V - 1] > c.K[q, 286]
            assert np.array_equal(ranking(name)[q], V - 1 - np.arange(16))
        elif kind[q] == -1:
            assert (d <= 0).all() and (d[33:286] < 0).all()
            assert (c.K[q] == c.K[q].max()).sum() == 34 and c.K[q, 0] == c.K[q, 33] > c.K[q, 34]
            assert np.array_equal(ranking(name)[q], 33 - np.arange(16))
        else:
            assert (c.K[q] == 0).all()
            assert np.array_equal(ranking(name)[q], V - 1 - np.arange(16))
    if name == "ramp_321":
        assert top_plateau == 34
        assert 287 // 64 != 320 // 64 and 287 // 16 != 303 // 16          # the plateau crosses tiles and 16-column blocks


@pytest.mark.parametrize("name", GPU_CASES)
def test_the_reference_starts_with_pred(name):
    c = tcase(name)
    r = ranking(name)
    assert r.shape == (c.B, min(16, c.V))
    assert np.array_equal(r[:, 0], c.pred)
    if name not in RAMPS:
        assert np.array_equal(r[:, 0], case(name).pred)
        q = np.arange(c.B)
        for base in (0, 1):                                 # the probabilities are answer_i8_cases.prob64's
            assert np.array_equal(top_prob64(name, base, r[:, :1])[:, 0], prob64(name, base, q, r[:, 0]))
    Ks = np.take_along_axis(c.K, r, axis=1)
    assert (np.diff(Ks, axis=1) <= 0).all()
    assert ((np.diff(Ks, axis=1) < 0) | (np.diff(r, axis=1) < 0)).all()      # equal codes: descending indices


def test_the_calls_are_declared_and_bound(abi):
    syms = abi.header_symbols("qmann_batch.h")
    assert "qmann_answer_topk_i8" in syms and "qmann_answer_topk_i8_ws_bytes" in syms
    vp, u32 = C.c_void_p, C.c_uint32
    f = abi.lib.qmann_answer_topk_i8
    assert f.restype is C.c_int
    assert list(f.argtypes) == [C.POINTER(abi.Net), vp, abi.Fmt, vp, vp, C.c_size_t, u32, vp, vp, u32, vp]
    h = abi.lib.qmann_answer_topk_i8_ws_bytes
    assert h.restype is C.c_size_t and list(h.argtypes) == [C.POINTER(abi.Net), u32, u32]
    import qmann_amd.model as model
    assert callable(getattr(model.QNet, "answer_topk_i8", None))
    text = (ROOT / "include" / "qmann_batch.h").read_text()
    assert not re.search(r"there is none for qmann_answer_i8's int8 matrices", text)


def make_net(abi, D=60, V=70, base=0, fu=(2, 5)):
    import qmann_amd.model as model
    fmt = [tuple(fu)] * 3
    cfg = dict(n_hop=3, dim_emb=D, dim_input=V, attention_mode=2, softmax_variant=base, f_fixed=True, en_lin_map=False,
               fmt=fmt, fmt_w=list(fmt), fmt_att=list(fmt), fmt_bin=fmt[0])
    return model._net_from_cfg(cfg)


def test_the_workspace_helper(abi):
    """the larger of float [n_query][V] rounded up to 8 bytes and the one-pass records: per slice and query 16 + 8 k bytes, the
    slices those of qmann_answer_i8 (512 workgroups of 64 queries wanted, at most one slice per 64-row tile)"""
    ws = lambda net, k, B: int(abi.lib.qmann_answer_topk_i8_ws_bytes(C.byref(net), k, B))
    assert ws(make_net(abi, V=4096, D=256), 5, 8192) == 8192 * 4096 * 4            # 4 slices of 56-byte records: the logits are larger
    assert ws(make_net(abi, V=70), 16, 40) == 40 * 2 * (16 + 8 * 16)               # two tiles, two slices: the records are larger
    assert ws(make_net(abi, V=70), 1, 40) == 40 * 70 * 4
    assert ws(make_net(abi, V=5), 5, 3) == 3 * (16 + 40)
    assert ws(make_net(abi, V=3), 3, 3) == 40                                       # 36 rounded up; no record form below 4 answers
    assert ws(make_net(abi, V=3, base=2), 1, 1) == 16
    assert ws(make_net(abi, V=70), 5, 0) == 0
    assert ws(make_net(abi, V=4033), 16, 64) == 64 * 4033 * 4                       # 64 slices x 144 bytes < 16 132
    # 0 for what the call would refuse
    assert abi.lib.qmann_answer_topk_i8_ws_bytes(None, 1, 1) == 0
    for k in (0, 17, 71):
        assert ws(make_net(abi, V=70), k, 8) == 0
    n = make_net(abi); n.dim_emb_pad = 96
    assert ws(n, 1, 8) == 0
    n = make_net(abi); n.dim_emb_pad = 192; n.dim_emb = 130
    assert ws(n, 1, 8) == 0
    n = make_net(abi); n.dim_emb = 0
    assert ws(n, 1, 8) == 0
    n = make_net(abi, V=40000)
    assert ws(n, 1, 8) == 0
    n = make_net(abi); n.act[2] = abi.Fmt(8, 0)
    assert ws(n, 1, 8) == 0


def test_refusal_codes_and_their_order(abi):
    """every refusal the header lists, and for each pair of neighbouring checks a call that fails both: the earlier one decides.
    The outputs are pre-filled and come back unchanged."""
    E, R, U, OK = abi.QMANN_EINVAL, abi.QMANN_ERANGE, abi.QMANN_EUNSUPPORTED, abi.QMANN_OK
    B, k = 8, 5
    net = make_net(abi)
    w = np.zeros((70, 64), np.int8)
    u = np.zeros((B, 60), np.float32)
    idx = np.full((B, 16), 0x5A5A5A5A, np.uint32)
    tp = np.full((B, 16), -7.5, np.float32)
    need = int(abi.lib.qmann_answer_topk_i8_ws_bytes(C.byref(net), k, B))
    assert need == B * 70 * 4
    wsbuf = np.full(need // 8 + 2, 0x5A5A5A5A5A5A5A5A, np.uint64)
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None

    def net_with(**fields):
        n = abi.Net.from_buffer_copy(net)
        for f, v in fields.items():
            if f == "act":
                n.act[n.n_hop - 1] = abi.Fmt(*v)
            else:
                setattr(n, f, v)
        return n

    def call(n=net, net_null=False, w_=w, w_fmt=(1, 6), u_=u, ws=wsbuf, ws_ptr=None, nbytes=need, k_=k, i=idx, t=tp, nq=B):
        wp = C.c_void_p(ws_ptr) if ws_ptr is not None else p(ws)
        return abi.lib.qmann_answer_topk_i8(None if net_null else C.byref(n), p(w_), abi.Fmt(*w_fmt), p(u_), wp, nbytes, k_, p(i),
                                            p(t), nq, None)

    # 1. qmann_answer_i8's refusals, its codes
    assert call(net_null=True) == E and call(w_=None) == E and call(u_=None) == E
    assert call(i=None) == E and call(t=None) == E
    assert call(net_with(dim_emb=0)) == E and call(net_with(dim_input=0)) == E
    assert call(net_with(dim_emb_pad=96)) == E and call(net_with(dim_emb=70)) == E
    assert call(net_with(act=(8, 0))) == R and call(net_with(act=(0, 0))) == R
    assert call(w_fmt=(1, 7)) == R and call(w_fmt=(0, 0)) == R
    assert call(net_with(dim_input=40000)) == R                              # a query's LDS beyond 128 KiB
    assert call(net_with(dim_emb=0, act=(8, 0))) == E                        # (within 1: dimensions before formats)
    # 1 before 2
    assert call(net_with(act=(8, 0)), k_=0) == R and call(w_fmt=(1, 7), k_=17) == R
    assert call(net_with(dim_input=40000), k_=0) == R
    # 2.
    assert call(k_=0) == E and call(k_=17) == E
    assert call(net_with(dim_input=4), k_=5) == E and call(net_with(dim_input=4), k_=4, nq=0) == OK
    # 2 before 4 and 5; 3 before 4, 5 and 6
    assert call(k_=0, nq=0) == E and call(k_=17, nq=1 << 24) == E
    assert call(ws=None) == E and call(nbytes=need - 1) == E and call(ws_ptr=wsbuf.ctypes.data + 4) == E
    assert call(ws=None, nq=0) == E
    assert call(nbytes=need - 1, nq=1 << 24) == E
    assert call(net_with(dim_emb_pad=192), ws=None) == E
    # 4., 5., 6.
    assert call(nq=0) == OK and call(nq=0, nbytes=0) == OK
    assert call(nq=1 << 24, nbytes=1 << 62) == R
    assert call(net_with(dim_emb_pad=192)) == U
    assert call(net_with(dim_emb_pad=192), nq=0) == OK                       # 4 before 6
    assert call(net_with(dim_emb_pad=192), nq=1 << 24) == R                  # 5 before 6
    assert (idx == 0x5A5A5A5A).all() and (tp == -7.5).all() and (wsbuf == 0x5A5A5A5A5A5A5A5A).all()

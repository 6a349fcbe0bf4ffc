"""qmann_answer_i8's refusals -- codes and their order, as include/qmann_batch.h lists them -- on the loaded library.  A refused
call launches nothing, so no GPU is needed: the pointers are host arrays that a refused call must not touch."""
import ctypes as C

import numpy as np
import pytest

from conftest import load_pkg


@pytest.fixture(scope="module")
def abi():
    load_pkg()
    import qmann_amd.abi as a
    return a


def make_net(abi, D=60, V=70, base=0, fu=(2, 5)):
    import qmann_amd.model as model
    fmt = [tuple(fu)] * 3
    cfg = dict(n_hop=3, dim_emb=D, dim_input=V, attention_mode=2, softmax_variant=base, f_fixed=True, en_lin_map=False,
               fmt=fmt, fmt_w=list(fmt), fmt_att=list(fmt), fmt_bin=fmt[0])
    return model._net_from_cfg(cfg)


def test_refusal_codes_and_their_order(abi):
    """every refusal the header lists, and for each pair of neighbouring checks a call that fails both: the earlier one decides.
    The outputs are pre-filled and come back unchanged.  The checks, in the header's order:
      1. QMANN_EINVAL for a null net, w_ans_i8, u, logits_ws or pred;
      2. QMANN_EINVAL for dim_emb = 0, dim_input = 0, dim_emb_pad no multiple of 64, dim_emb > dim_emb_pad;
      3. QMANN_ERANGE for a last-hop activation format or a w_fmt that is no byte format;
      4. QMANN_ERANGE for a query's LDS beyond 128 KiB;
      5. QMANN_OK for n_query = 0;
      6. QMANN_ERANGE for 2^24 queries or more;
      7. QMANN_EUNSUPPORTED for a dim_emb_pad other than 64, 128 or 256."""
    E, R, U, OK = abi.QMANN_EINVAL, abi.QMANN_ERANGE, abi.QMANN_EUNSUPPORTED, abi.QMANN_OK
    B = 8
    net = make_net(abi)
    assert (net.dim_emb, net.dim_emb_pad, net.dim_input) == (60, 64, 70)
    w = np.zeros((70, 64), np.int8)
    u = np.zeros((B, 60), np.float32)
    ws = np.full((B, 70), -7.5, np.float32)
    labels = np.zeros(B, np.uint32)
    pred = np.full(B, 0x5A5A5A5A, np.uint32)
    probs = np.full((B, 70), -7.5, np.float32)
    cost = np.full(1, -7.5, np.float32)
    match = np.full(1, 0x5A5A5A5A, np.uint32)
    p = lambda a: C.c_void_p(a.ctypes.data) if a is not None else None

    def net_with(**fields):
        n = abi.Net.from_buffer_copy(net)
        for f, v in fields.items():
            if f == "act":
                n.act[n.n_hop - 1] = abi.Fmt(*v)
            else:
                setattr(n, f, v)
        return n

    def call(n=net, net_null=False, w_=w, w_fmt=(1, 6), u_=u, ws_=ws, pred_=pred, probs_=None, nq=B):
        return abi.lib.qmann_answer_i8(None if net_null else C.byref(n), p(w_), abi.Fmt(*w_fmt), p(u_), p(ws_), p(labels), p(pred_),
                                       p(probs_), p(cost), p(match), nq, None)

    # 1.
    assert call(net_null=True) == E and call(w_=None) == E and call(u_=None) == E
    assert call(ws_=None) == E and call(pred_=None) == E
    # 1 before 3, 4, 5, 6 and 7 (1 and 2 share a code: a null pointer with a zero dimension answers it either way)
    assert call(net_with(dim_emb=0), w_=None) == E
    assert call(net_with(act=(8, 0)), u_=None) == E and call(net_with(dim_input=40000), ws_=None) == E
    assert call(pred_=None, nq=0) == E and call(pred_=None, nq=1 << 24) == E
    assert call(net_with(dim_emb_pad=192), w_=None) == E
    # 2.
    assert call(net_with(dim_emb=0)) == E and call(net_with(dim_input=0)) == E
    assert call(net_with(dim_emb_pad=96)) == E and call(net_with(dim_emb=70)) == E
    # 2 before 3, 4, 5 and 6
    assert call(net_with(dim_emb=0, act=(8, 0))) == E and call(net_with(dim_emb_pad=96), w_fmt=(1, 7)) == E
    assert call(net_with(dim_emb=70, dim_input=40000)) == E
    assert call(net_with(dim_input=0), nq=0) == E and call(net_with(dim_emb_pad=96), nq=1 << 24) == E
    # 3.
    assert call(net_with(act=(8, 0))) == R and call(net_with(act=(0, 0))) == R
    assert call(w_fmt=(1, 7)) == R and call(w_fmt=(0, 0)) == R
    # 3 before 4 (one code), 5 and 7
    assert call(net_with(act=(8, 0), dim_input=40000)) == R
    assert call(net_with(act=(8, 0)), nq=0) == R and call(w_fmt=(1, 7), nq=0) == R
    assert call(net_with(act=(8, 0), dim_emb_pad=192)) == R
    # 4.: a query's LDS beyond 128 KiB (60 rounded up to 4, plus 40 000, floats); 32 708 answers are the most that fit
    assert call(net_with(dim_input=40000)) == R
    assert call(net_with(dim_input=32709)) == R and call(net_with(dim_input=32708), nq=0) == OK
    # 4 before 5 and 7
    assert call(net_with(dim_input=40000), nq=0) == R
    assert call(net_with(dim_input=40000, dim_emb_pad=192)) == R
    # 5., 6., 7.
    assert call(nq=0) == OK and call(nq=0, probs_=probs) == OK
    assert call(nq=1 << 24) == R and call(nq=0xFFFFFFFF) == R
    for pr in (None, probs):
        assert call(net_with(dim_emb_pad=192), nq=8, probs_=pr) == U
        assert call(net_with(dim_emb_pad=320), nq=8, probs_=pr) == U
        assert call(net_with(dim_emb_pad=192), nq=0, probs_=pr) == OK                  # 5 before 7
        assert call(net_with(dim_emb_pad=192), nq=1 << 24, probs_=pr) == R             # 6 before 7
    assert (pred == 0x5A5A5A5A).all() and (probs == -7.5).all() and (ws == -7.5).all()
    assert (cost == -7.5).all() and (match == 0x5A5A5A5A).all() and not labels.any()


def test_a_batch_near_2_32_queries_is_refused_not_sized_with_zero_workgroups(abi):
    """the one-pass grid of a batch within 63 queries of 2^32 wrapped to 0 workgroups of 64, and the slice count divided by it:
    qmann_answer_topk_i8 and its workspace helper, which size the workspace ahead of the 2^24 refusal, trapped.  Now the helper
    answers the logits' size and the call its documented codes; qmann_answer_i8 (above) answered QMANN_ERANGE all along."""
    E, R = abi.QMANN_EINVAL, abi.QMANN_ERANGE
    net = make_net(abi)
    nq = 0xFFFFFFFF
    assert int(abi.lib.qmann_answer_topk_i8_ws_bytes(C.byref(net), 5, nq)) == (nq * 70 * 4 + 7) // 8 * 8
    w, u = np.zeros((70, 64), np.int8), np.zeros((8, 60), np.float32)
    idx, tp = np.full((8, 5), 0x5A5A5A5A, np.uint32), np.full((8, 5), -7.5, np.float32)
    ws = np.full(16, 0x5A5A5A5A5A5A5A5A, np.uint64)
    p = lambda a: C.c_void_p(a.ctypes.data)
    call = lambda nbytes: abi.lib.qmann_answer_topk_i8(C.byref(net), p(w), abi.Fmt(1, 6), p(u), p(ws), nbytes, 5, p(idx), p(tp), nq, None)
    assert call(128) == E and call(1 << 62) == R
    assert (idx == 0x5A5A5A5A).all() and (tp == -7.5).all() and (ws == 0x5A5A5A5A5A5A5A5A).all()

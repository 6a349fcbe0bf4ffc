"""The reference host's test / validation loop (MemN2N/MemN2N.c:2378-2702), verb by verb through the C-ABI in ctypes.

Per query it issues the forward verbs in the reference's order (:2626-2697) on FIXED layer buffers, as the host's layer
structs hold them, with the options the host program has: the attention mode (lib/layer.c:176-233), the linear map, the
attention scale layer (:2647-2649), the RELU layer behind sum_vec with its wiring (:2435-2437, :2471-2473, :2535-2537),
the shift-based softmax, the softmax base of the library, the cross-entropy phase and the number of hops.  The
accumulators are fetched once after the loop (:2701-2702).
"""
import ctypes as C

import numpy as np


def make_state(env, cfg, S, dev_wts=None, wts=None):
    """every device buffer of the host's layers for `cfg` (memories of up to S sentences).  A state that is passed to
    several host_loop() calls keeps the pointers, and with them the queue's signature of the run, the same."""
    up, empty, torch = env.up, env.empty, env.torch
    V, D, H = cfg["dim_input"], cfg["dim_emb"], cfg["n_hop"]
    st = {}
    st["wts"] = dev_wts if dev_wts is not None else {k: ([up(w) for w in v] if isinstance(v, list) else up(v))
                                                      for k, v in wts.items()}
    st["u0"] = empty(D)
    for name, shape in (("Mk", (S, D)), ("Mc", (S, D)), ("s", (S,)), ("sc_out", (S,)), ("p", (S,)), ("o", (D,)), ("lu", (D,)),
                        ("sv", (D,)), ("nl", (D,))):
        st[name] = [empty(*shape) for _ in range(H)]
    st["a"], st["ph"], st["mxs"], st["grad"] = empty(V), empty(V), empty(1), empty(V)
    st["cost"] = torch.zeros(3, device=env.dev)
    st["cnt"] = torch.zeros(3, dtype=torch.int32, device=env.dev)
    st["pred"] = torch.zeros(1, dtype=torch.int32, device=env.dev)
    st["junk"] = [empty(D) for _ in range(3)]
    st["S"] = S
    if cfg.get("att_scale") is not None:
        # one scale layer per hop: the scalar, its gradient, out and grad_out (cuda_scale_constructor's buffers), set up by
        # cuda_scale_init from the host's value
        st["sc_w"], st["sc_w_del"], st["sc_grad"] = [empty(1) for _ in range(H)], [empty(1) for _ in range(H)], [empty(S) for _ in range(H)]
        for h in range(H):
            w = C.c_float(float(np.float32(cfg["att_scale"][h])))
            env.lib.cuda_scale_init(env.ptr(st["sc_w"][h]), env.ptr(st["sc_w_del"][h]), env.ptr(st["sc_out"][h]),
                                    env.ptr(st["sc_grad"][h]), C.byref(w), S)
    return st


def host_loop(env, cfg, wts, story, ques, ans_onehot, n_sen, nq, defer, stray=None, dev_wts=None, *, ce_mode=3, order=None,
              relu_fixed=True, relu_fmt=None, hop_verbs=None, softmax_base=None, state=None):
    """MemN2N.c's test loop in ctypes: per query the verbs in the reference's order, accumulators fetched once at the end.

    cfg            the oracle's configuration dict: attention_mode 1 (float scores and read-out, fixed sum_vec), 2, or 3
                   (cuda_dot_mat_vec_fwd_appx, num_bit = 1 + iwl + frac); en_lin_map; att_scale (a list: a cuda_scale_fwd
                   between scores and softmax); en_non_lin (a RELU behind sum_vec); softmax_shift_based; n_hop
    stray          a query index after which an unrelated verb (a vector sum on scratch) is issued: the pattern breaks there
    ce_mode        the phase of cuda_cross_entropy_run: 1 train, 2 valid, 3 test
    order          the query indices in the order they are issued (default 0 .. nq-1); the pools stay where they are
    relu_fixed, relu_fmt   f_fixed and (iwl, frac) the RELU verb is called with (default: the hop's activation format)
    hop_verbs      per hop "dot" or "appx": the score verb of that hop, whatever the attention mode says
    softmax_base   qmann_abi_set_softmax_base for the duration of the loop (restored to 0)
    state          make_state()'s buffers, to keep every pointer over several calls
    Returns the match count, cost and last prediction of the `ce_mode` phase, all three phases' accumulators (`cnts`,
    `costs`), the LAST issued query's buffers (final state, output softmax, hop-0 scores; every hop's `sv`, `p`, `scores`,
    `o` and RELU output) and the queue's statistics."""
    lib, up, ptr = env.lib, env.up, env.ptr
    V, D, H = cfg["dim_input"], cfg["dim_emb"], cfg["n_hop"]
    mode = cfg.get("attention_mode", 2)
    lin, relu, shift = bool(cfg.get("en_lin_map", True)), bool(cfg.get("en_non_lin", False)), bool(cfg.get("softmax_shift_based", False))
    scale = cfg.get("att_scale") is not None
    order = list(range(nq)) if order is None else [int(i) for i in order]
    n_pool = max(order) + 1
    offs = np.concatenate([[0], np.cumsum(n_sen[:n_pool])]).astype(np.int64)
    S = int(n_sen[:n_pool].max())
    st = state if state is not None else make_state(env, cfg, S, dev_wts, wts)
    assert st["S"] >= S
    w = st["wts"]
    dwq, dwans, dwa, dwc, dwh = w["w_q"], w["w_ans"], w["w_a"], w["w_c"], w.get("w_h")
    dm, dq, da = up(story[:offs[n_pool]]), up(ques[:n_pool]), up(ans_onehot[:n_pool])
    u0, Mk, Mc, s, p, o, lu, sv, nl = (st[k] for k in ("u0", "Mk", "Mc", "s", "p", "o", "lu", "sv", "nl"))
    a, ph, mxs, grad, cost, cnt, pred, junk = (st[k] for k in ("a", "ph", "mxs", "grad", "cost", "cnt", "pred", "junk"))
    cost.zero_(); cnt.zero_()
    env.torch.cuda.synchronize()
    fptr = lambda t, i: C.c_void_p(t.data_ptr() + 4 * i)
    if softmax_base is not None:
        lib.qmann_abi_set_softmax_base(softmax_base)
    lib.qmann_abi_set_defer(defer)
    try:
        for i in order:
            ns = int(n_sen[i])
            X = C.c_void_p(dm.data_ptr() + 4 * V * int(offs[i])); q = C.c_void_p(dq.data_ptr() + 4 * V * i)
            y = C.c_void_p(da.data_ptr() + 4 * V * i)
            fw0 = cfg["fmt_w"][0]
            lib.cuda_dense_fwd(ptr(dwq), None, q, ptr(u0), None, V, D, b"NULL", True, *fw0, *fw0, 3, False)
            u_att = u_lin = u0                      # what the attention / the linear map of the next hop read
            for h in range(H):
                fw, fa, fm, fb = cfg["fmt_w"][h], cfg["fmt"][h], cfg["fmt_att"][h], cfg["fmt_bin"]
                verb = hop_verbs[h] if hop_verbs else ("appx" if mode == 3 else "dot")
                lib.cuda_dense_mat_fwd(ptr(dwa[h]), None, X, ptr(Mk[h]), None, V, D, ns, True, *fw, 3, False)
                lib.cuda_dense_mat_fwd(ptr(dwc[h]), None, X, ptr(Mc[h]), None, V, D, ns, True, *fw, 3, False)
                if verb == "appx":
                    lib.cuda_dot_mat_vec_fwd_appx(ptr(Mk[h]), ptr(u_att), ptr(s[h]), None, None, ns, D, True, *fm, 3,
                                                  1 + fm[0] + fm[1], False, False)
                elif mode == 2 or hop_verbs:
                    lib.cuda_dot_mat_vec_fwd(ptr(Mk[h]), ptr(u_att), ptr(s[h]), None, ns, D, False, True, *fm, *fb, 3, False)
                else:
                    lib.cuda_dot_mat_vec_fwd(ptr(Mk[h]), ptr(u_att), ptr(s[h]), None, ns, D, False, False, *fm, *fm, 3, False)
                sm_in = s[h]
                if scale:
                    lib.cuda_scale_fwd(ptr(s[h]), ptr(st["sc_w"][h]), ptr(st["sc_out"][h]), ns, True, *fm, 3, False)
                    sm_in = st["sc_out"][h]
                lib.cuda_softmax_fwd(ptr(p[h]), ptr(sm_in), None, None, ptr(mxs), ns, shift, False)
                if verb == "appx":
                    lib.cuda_dot_mat_vec_fwd_appx(ptr(Mc[h]), ptr(p[h]), ptr(o[h]), None, None, ns, D, True, *fa, 3,
                                                  1 + fa[0] + fa[1], True, False)
                else:
                    lib.cuda_dot_mat_vec_fwd(ptr(Mc[h]), ptr(p[h]), ptr(o[h]), None, ns, D, True, mode != 1, *fa, *fa, 3, False)
                A = u_lin
                if lin:
                    lib.cuda_dense_fwd(ptr(dwh[h]), None, ptr(u_lin), ptr(lu[h]), None, D, D, b"NULL", True, *fb, *fw, 3, False)
                    A = lu[h]
                lib.cuda_sum_vec_fwd(ptr(A), ptr(o[h]), ptr(sv[h]), D, True, *fa, 3, False)
                u_att = u_lin = sv[h]
                if relu:
                    lib.cuda_activation_fwd(ptr(sv[h]), ptr(nl[h]), b"RELU", D, relu_fixed, *(relu_fmt or fa), 3)
                    u_att = nl[h]
            lib.cuda_dense_fwd(ptr(dwans), None, ptr(u_att), ptr(a), None, D, V, b"NULL", False, 8, 7, 8, 7, 3, False)
            lib.cuda_softmax_fwd(ptr(ph), ptr(a), None, None, ptr(mxs), V, False, False)
            lib.cuda_cross_entropy_run(fptr(cost, 0), fptr(cost, 1), fptr(cost, 2), fptr(cnt, 0), fptr(cnt, 1), fptr(cnt, 2), ptr(pred),
                                       None, ptr(ph), y, None, None, ptr(grad), None, V, ce_mode)
            if stray is not None and i == stray:
                lib.cuda_sum_vec_fwd(ptr(junk[0]), ptr(junk[1]), ptr(junk[2]), D, False, 0, 0, 3, False)
        hc = (C.c_float * 3)(); hm = (C.c_uint * 3)()
        lib.cuda_cross_entropy_cost_load(fptr(cost, 0), fptr(cost, 1), fptr(cost, 2), hc, C.byref(hc, 4), C.byref(hc, 8))
        lib.cuda_cross_entropy_m_cnt_load(fptr(cnt, 0), fptr(cnt, 1), fptr(cnt, 2), hm, C.byref(hm, 4), C.byref(hm, 8))
        stats = env.abi.defer_stats()
    finally:
        lib.qmann_abi_set_defer(0)
        if softmax_base is not None:
            lib.qmann_abi_set_softmax_base(0)
    ns_last = int(n_sen[order[-1]])
    get = lambda t, n=None: t.cpu().numpy()[:n].copy()
    return dict(match=int(hm[ce_mode - 1]), cost=float(hc[ce_mode - 1]), cnts=[int(x) for x in hm], costs=[float(x) for x in hc],
                last_u=get(sv[H - 1]), last_p=get(ph), last_pred=int(pred.item()), last_scores=get(s[0], ns_last),
                sv=[get(t) for t in sv], p=[get(t, ns_last) for t in p], scores=[get(t, ns_last) for t in s],
                o=[get(t) for t in o], nl=[get(t) for t in nl] if relu else None, stats=stats)

"""The refusal order of the eleven shared-plane hop calls, pinned without a device.

Every refusal of these calls runs before their first HIP call, so the library answers them on a machine without a GPU.  Each call
has an ordered list of defects (one argument or net field made wrong) with the code it answers; the lists are the calls' own
order of checks.  A single defect must give its code, and two defects together must give the code of the one checked FIRST --
that is what "the order of the return codes" means to a caller, and what a shared prelude (csrc/hops_host.h) must not change.

No case launches: every case either refuses or has n_query = 0 ("OK, launch nothing").  The buffers are small fake addresses.
"""
import ctypes as C
import itertools

import pytest

from conftest import load_pkg

OK, EINVAL, ERANGE, EUNSUPPORTED = 0, -1, -2, -3
D, DP, H, N_SLOTS, N_QUERY = 60, 64, 3, 100, 4
LDS_TOO_LONG, SPLIT_TOO_LONG = 200000, (1 << 24) + 1
ADDR = {n: 0x10000 + 0x1000 * i for i, n in enumerate(("keys", "vals", "u0", "u_out", "top_slot", "top_p", "ws", "lin_map"))}


@pytest.fixture(scope="module")
def env():
    load_pkg()
    import qmann_amd.abi as abi
    import qmann_amd.model as model
    return abi, model


# ---- the defects: (label, overrides of the good call, code) ------------------------------------------------------------------
PRELUDE = [("null net", dict(null_net=True), EINVAL), ("null keys", dict(keys=0), EINVAL), ("null vals", dict(vals=0), EINVAL),
           ("null u0", dict(u0=0), EINVAL), ("null u_out", dict(u_out=0), EINVAL), ("n_hop = 0", dict(n_hop=0), EINVAL),
           ("dim_emb_pad = 96", dict(Dp=96), EUNSUPPORTED)]
QUERIES = [("n_query = 0", dict(n_query=0), OK), ("n_query = 1 << 24", dict(n_query=1 << 24), ERANGE)]
TOP = [("k = 0", dict(k=0), EINVAL), ("k = 17", dict(k=17), EINVAL), ("null top_slot", dict(top_slot=0), EINVAL),
       ("null top_p", dict(top_p=0), EINVAL)]
SOFTMAX_7 = ("softmax_base = 7", dict(softmax_base=7), EINVAL)
WORD_9 = ("a format of word length 9", dict(word9=True), ERANGE)
NO_SLOTS = ("n_slots = 0", dict(n_slots=0), EINVAL)
LDS_LONG = ("too long for LDS", dict(n_slots=LDS_TOO_LONG), ERANGE)
BAD_WS = [("null ws", dict(ws=0), EINVAL), ("ws at 8 mod 16", dict(ws=ADDR["ws"] + 8), EINVAL)]
SPLIT_LONG = ("n_slots > 1 << 24", dict(n_slots=SPLIT_TOO_LONG), ERANGE)
WS_SHORT = ("ws_bytes one short", dict(ws_short=True), EINVAL)
PACKED_HEAD = [("mode 2", dict(mode=2), EUNSUPPORTED), ("key stride wrong", dict(key_stride_off=8), EINVAL),
               ("key_planes at 8 mod 16", dict(keys=ADDR["keys"] + 8), EINVAL),
               ("att word length 6", dict(att6=True), EUNSUPPORTED)]            # (ham_common.h::check_ham_hop)
ONE_PLANE = ("Dp = 64, num_bit = 1", dict(num_bit=1), EUNSUPPORTED)


def fixed_list(top):
    return (PRELUDE + [("mode 1", dict(mode=1), EUNSUPPORTED), SOFTMAX_7, WORD_9, NO_SLOTS, LDS_LONG] + QUERIES + (TOP if top else []))


def float_list(top):
    # (the float calls fill HopArgs -- softmax base and formats -- BEFORE their mode check)
    return (PRELUDE + [SOFTMAX_7, WORD_9, ("mode 2", dict(mode=2), EUNSUPPORTED), NO_SLOTS, LDS_LONG] + QUERIES + (TOP if top else []))


def packed_list(top):
    return PRELUDE + PACKED_HEAD + [NO_SLOTS, LDS_LONG, ONE_PLANE] + QUERIES + (TOP if top else [])


def split_list(top):
    # (no LDS refusal: the slots are cut into slices)
    return (PRELUDE + [("mode 1", dict(mode=1), EUNSUPPORTED), WORD_9, NO_SLOTS] + BAD_WS + [SPLIT_LONG] + QUERIES + [WS_SHORT]
            + (TOP if top else []))


def split_packed_list(top):
    return PRELUDE + PACKED_HEAD + [NO_SLOTS, ONE_PLANE] + BAD_WS + [SPLIT_LONG] + QUERIES + [WS_SHORT] + (TOP if top else [])


# (call, the mode of a good net, its list)
CALLS = [("qmann_hops_shared_i8", 2, fixed_list(False)), ("qmann_hops_shared_top_i8", 2, fixed_list(True)),
         ("qmann_hops_shared_float_i8", 1, float_list(False)), ("qmann_hops_shared_top_float_i8", 1, float_list(True))]
for _mode in (10, 11):                                                           # Hamming V0 and V1
    CALLS += [("qmann_hops_shared_packed", _mode, packed_list(False)), ("qmann_hops_shared_top_packed", _mode, packed_list(True)),
              ("qmann_hops_shared_split_packed", _mode, split_packed_list(False)),
              ("qmann_hops_shared_split_top_packed", _mode, split_packed_list(True))]
CALLS += [("qmann_hops_shared_split_i8", 2, split_list(False)), ("qmann_hops_shared_split_top_i8", 2, split_list(True))]


def run(env, name, mode, overrides):
    """the good call of `name` with `overrides` applied -> its return code"""
    abi, model = env
    p = dict(mode=mode, softmax_base=0, word9=False, att6=False, n_hop=H, Dp=DP, num_bit=2, null_net=False, n_slots=N_SLOTS,
             n_query=N_QUERY, k=2, key_stride_off=0, ws_short=False, **ADDR)
    p.update(overrides)
    cfg = model.babi_cfg(30, attention_mode=p["mode"], softmax_base=p["softmax_base"], n_hop=H, D=D, en_mq=False)
    cfg["num_bit"] = p["num_bit"]
    if p["word9"]:
        cfg["fmt"] = [(5, 4)] + cfg["fmt"][1:]
    if p["att6"]:
        cfg["fmt_att"] = [(3, 3)] + cfg["fmt_att"][1:]
    net = model._net_from_cfg(cfg)
    assert net.dim_emb_pad == DP
    net.n_hop, net.dim_emb_pad = p["n_hop"], p["Dp"]
    for h in range(H):
        net.lin_map[h] = p["lin_map"] + 0x1000 * h
    packed, split, top = "packed" in name, "split" in name, "top" in name
    n_slots, n_query = p["n_slots"], p["n_query"]
    val_stride = n_slots * DP
    args = [None if p["null_net"] else C.byref(net), p["keys"] or None]
    if packed:
        args += [n_slots * (DP // 64) * p["num_bit"] * 8 + p["key_stride_off"], p["vals"] or None, val_stride]
    else:
        args += [p["vals"] or None, val_stride]
    args += [n_slots, p["u0"] or None, p["u_out"] or None]
    args += [p["k"], p["top_slot"] or None, p["top_p"] or None] if top else [None]          # (else: no taps)
    args += [n_query]
    if split:
        size = getattr(abi.lib, "qmann_hops_shared_split_packed_ws_bytes" if packed else "qmann_hops_shared_split_ws_bytes")
        nbytes = int(size(C.byref(net), n_slots, n_query))
        args += [0, p["ws"] or None, max(nbytes - 1, 0) if p["ws_short"] else nbytes]
    return getattr(abi.lib, name)(*args, None)


@pytest.mark.parametrize("name, mode, defects", CALLS, ids=[f"{c[0][11:]}-mode{c[1]}" for c in CALLS])
def test_refusals_and_their_order(env, name, mode, defects):
    # every single defect
    for label, over, code in defects:
        assert over.get("n_query") == 0 or code != OK
        assert run(env, name, mode, over) == code, label
    # two defects at once: the one checked first answers.  (Two defects of the same argument cannot be combined, and two with
    # the same code tell nothing about the order.)
    n_pairs = 0
    for (la, oa, ca), (lb, ob, cb) in itertools.combinations(defects, 2):
        if ca == cb or set(oa) & set(ob):
            continue
        assert run(env, name, mode, {**oa, **ob}) == ca, f"{la} + {lb}"
        n_pairs += 1
    assert n_pairs >= len(defects)


def test_the_cases_the_order_is_known_by(env):
    """a few of the pairs above by name: the ones the calls' documented order speaks of"""
    for name in ("qmann_hops_shared_i8", "qmann_hops_shared_top_i8"):
        assert run(env, name, 2, dict(n_slots=LDS_TOO_LONG, n_query=0)) == ERANGE
    for name in ("qmann_hops_shared_float_i8", "qmann_hops_shared_top_float_i8"):
        assert run(env, name, 2, dict(word9=True)) == ERANGE                   # formats before the mode
        assert run(env, name, 2, dict(softmax_base=7)) == EINVAL
        assert run(env, name, 2, dict(n_slots=0)) == EUNSUPPORTED                # the mode before the memory
        assert run(env, name, 2, dict(n_slots=LDS_TOO_LONG)) == EUNSUPPORTED
    for name, mode, _ in CALLS:
        if "top" in name:
            assert run(env, name, mode, dict(n_query=0, k=0)) == OK               # the top arguments come last
    for name in ("qmann_hops_shared_split_i8", "qmann_hops_shared_split_top_i8"):
        assert run(env, name, 2, dict(n_slots=LDS_TOO_LONG, n_query=0)) == OK     # the split calls have no LDS refusal

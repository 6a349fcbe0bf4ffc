"""The nine A/B switches of INTEGRATION.md section 5 that no other test sets: each runs the same call with the switch unset and
set (qmann_tuning_reload() between) at the smallest shape where the table there and the launcher say the switch changes the
kernel, and the outputs must be equal bit for bit ("none changes a result").  For the hop switches the library has no way to
report which kernel ran; every docstring names the launcher condition its shape relies on.  The byte-level side of the three
embedding switches is in test_gpu_embed_forms.py (where qmann_embed_story_idx_form does report the kernel)."""
import numpy as np
import pytest

from conftest import load_pkg
from test_gpu_words import random_stories, weights

pytestmark = pytest.mark.gpu

ALL = ("QMANN_NO_LEAN", "QMANN_NO_MID", "QMANN_NO_W7", "QMANN_NO_TIGHT", "QMANN_NO_QUAD_LONG", "QMANN_ANSWER_TWO_PASS",
       "QMANN_EMBED_VALU", "QMANN_EMBED_PER_HOP", "QMANN_EMBED_GENERAL_EPILOGUE", "QMANN_LEAN_SPARSE", "QMANN_QUAD_MIN_QUERIES")


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
    e.torch, e.abi, e.model, e.dev = torch, abi, model, torch.device("cuda:0")
    return e


def both_ways(env, monkeypatch, switch, call, fixed=None):
    """call() with `switch` unset, then set; `fixed`: other variables held at a value (None: unset) through both runs.
    (conftest re-reads the restored environment after the test.)"""
    out = []
    for on in (False, True):
        for k in ALL:
            monkeypatch.delenv(k, raising=False)
        for k, v in (fixed or {}).items():
            if v is not None:
                monkeypatch.setenv(k, v)
        if on:
            monkeypatch.setenv(switch, "1")
        env.abi.lib.qmann_tuning_reload()
        out.append(call())
        env.torch.cuda.synchronize()
    return out


def cfg_of(mode, D=60, H=3, base=0, nb=8, V=40, en_mq=False):
    fmt = [(5, 2)] * H
    fmt_w = [(6, 1), (5, 2), (4, 3)] if en_mq else list(fmt)
    return dict(n_hop=H, dim_emb=D, dim_input=V, attention_mode=mode, softmax_variant=base, f_fixed=True, en_lin_map=True,
                fmt=fmt, fmt_w=fmt_w, fmt_att=list(fmt), fmt_bin=(5, 2), num_bit=nb)


def memories(env, cfg, n_slots, seed, sigma_k=30.0, sigma_u=20.0):
    """random int8 memories for stories of n_slots[i] rows -> net, keys, vals, row_off, u0 on the device"""
    torch, model = env.torch, env.model
    H, D, V = cfg["n_hop"], cfg["dim_emb"], cfg["dim_input"]
    rng = np.random.default_rng(seed)
    wts = {"w_h": [rng.normal(0, 1.0, (D, D)).astype(np.float32) for _ in range(H)],
           "w_ans": rng.normal(0, 0.1, (V, D)).astype(np.float32)}
    net = model.QNet(cfg, wts, device="cuda:0")
    Dp = net.Dp
    n_slots = np.asarray(n_slots, np.int64)
    row_off = np.concatenate([[0], np.cumsum(n_slots)]).astype(np.int32)
    R = int(row_off[-1])
    keys = np.zeros((H, R, Dp), np.int8); vals = np.zeros((H, R, Dp), np.int8)
    keys[:, :, :D] = np.clip(np.rint(rng.normal(0, sigma_k, (H, R, D))), -127, 127)
    vals[:, :, :D] = np.clip(np.rint(rng.normal(0, sigma_k, (H, R, D))), -127, 127)
    keys[:, 1::5, ::4] = 0
    sk = model.to_signmag(keys)
    sk[:, ::11, 3] = np.int8(-128)                          # "minus zero" bytes are legal memory codes
    m0 = (1 << sum(cfg["fmt_w"][0])) - 1
    u0 = (np.clip(np.rint(rng.normal(0, sigma_u, (len(n_slots), D))), -m0, m0) / (1 << cfg["fmt_w"][0][1])).astype(np.float32)
    up = lambda a: torch.from_numpy(a).to(env.dev)
    return net, up(sk), up(model.to_signmag(vals)), up(row_off), up(u0)


def spread(S_list, B, seed):
    n = np.array([S_list[i % len(S_list)] for i in range(B)], np.int64)
    np.random.default_rng(seed).shuffle(n)
    return n


def assert_same(a, b, what):
    a, b = a.cpu().numpy(), b.cpu().numpy()
    bad = np.flatnonzero((a != b).reshape(a.shape[0], -1).any(1))
    assert bad.size == 0, f"{what}: {bad.size} of {a.shape[0]} rows differ with the switch set, first {bad[:5]}"
    assert np.abs(a).sum() > 0                              # (a case that computes nothing tests nothing)


@pytest.mark.parametrize("mode,nb", [(2, 8), (3, 8), (10, 8), (11, 8)])
def test_no_lean(env, monkeypatch, mode, nb):
    """hops_lean.h::lean_supported: Dp = 64, 64-byte key rows, max_slots <= 64, no taps -- the lean kernel, unless QMANN_NO_LEAN;
    then hop_plan gives HopForm::Small (the one-wavefront general kernel).  50 queries <= QMANN_QUAD_MIN_QUERIES keep the quad
    forms out of it either way."""
    n = spread([1, 2, 16, 17, 50, 64], 50, 1)
    net, k, v, ro, u0 = memories(env, cfg_of(mode, nb=nb), n, 8100 + mode)
    a, b = both_ways(env, monkeypatch, "QMANN_NO_LEAN", lambda: net.hops(k, v, ro, 64, u0))
    assert_same(a, b, f"mode {mode}")


@pytest.mark.parametrize("base", [0, 1, 2])
def test_no_mid(env, monkeypatch, base):
    """hops_lean.h::mid_supported: Dp = 64, 64 < max_slots <= 1 024, softmax base e^x / 2^x / exp_plan without the shift form or
    an attention scale, no taps; hop_plan takes HopForm::Mid for mode 2 only, and HopForm::General under QMANN_NO_MID."""
    n = spread([65, 300, 1024], 12, 2)
    net, k, v, ro, u0 = memories(env, cfg_of(2, base=base), n, 8200 + base, sigma_k=12.0)
    a, b = both_ways(env, monkeypatch, "QMANN_NO_MID", lambda: net.hops(k, v, ro, 1024, u0))
    assert_same(a, b, f"softmax base {base}")


@pytest.mark.parametrize("call", ["hops_i8", "shared", "shared_split"])
@pytest.mark.parametrize("D", [128, 60])
def test_no_w7(env, monkeypatch, call, D):
    """batch_hops.hip, batch_hops_shared.hip and batch_hops_shared_split.hip each take their W7 instantiation when every
    attention format has word length 7 (hops_common.h::all_w7 with kW7Att: the babi_cfg defaults, Q5.2) and QMANN_NO_W7 is
    unset.  qmann_hops_i8 reaches that line only for the general kernel: a 300-row memory at D = 128 (Dp = 128: neither
    lean_supported nor mid_supported); at D = 60 the same memory takes hops_mid.h and the pair is one more equality."""
    S, B = 300, 8
    net, k, v, ro, u0 = memories(env, cfg_of(2, D=D), [S] * B if call == "hops_i8" else [S], 8300 + D, sigma_k=12.0)
    if call != "hops_i8":
        u0 = env.torch.from_numpy((np.clip(np.rint(np.random.default_rng(8310 + D).normal(0, 20, (B, D))), -127, 127) / 4.0).astype(np.float32)).to(env.dev)
    run = {"hops_i8": lambda: net.hops(k, v, ro, S, u0), "shared": lambda: net.hops_shared(k, v, S, u0),
           "shared_split": lambda: net.hops_shared_split(k, v, S, u0, n_slices=3)}[call]
    a, b = both_ways(env, monkeypatch, "QMANN_NO_W7", run)
    assert_same(a, b, f"{call}, D = {D}")


@pytest.mark.parametrize("sparse", [None, "0", "1"])
@pytest.mark.parametrize("mode,nb", [(2, 8), (11, 8)])
def test_no_tight(env, monkeypatch, mode, nb, sparse):
    """hops_lean.h::launch_lean_w: the six-wave (80-register) build wherever it buys a resident workgroup, the four-wave build
    under QMANN_NO_TIGHT; the switch also enters the launcher's choice of the sparse read-out (50-slot value tiles cost the
    tight build a workgroup), so the pair runs with QMANN_LEAN_SPARSE left to the launcher, forced off and forced on.
    300 stories of 50 rows: lean_supported, and n_query <= QMANN_QUAD_MIN_QUERIES keeps HopForm::Lean."""
    net, k, v, ro, u0 = memories(env, cfg_of(mode, nb=nb), [50] * 300, 8400 + mode)
    a, b = both_ways(env, monkeypatch, "QMANN_NO_TIGHT", lambda: net.hops(k, v, ro, 50, u0), fixed={"QMANN_LEAN_SPARSE": sparse})
    assert_same(a, b, f"mode {mode}, QMANN_LEAN_SPARSE {sparse}")


def test_no_quad_long(env, monkeypatch):
    """hops_host.h::hop_plan: lean_supported and quad_supported (e^x softmax, word-length-7 formats, plane size known),
    n_query > QMANN_QUAD_MIN_QUERIES (set to 0 here so that 300 stories qualify, as test_gpu_quad.py does), max_slots > 16 and
    a mean story length above 16 rows: HopForm::QuadLong for mode 2, HopForm::Lean under QMANN_NO_QUAD_LONG."""
    n = spread([17, 18, 31, 32, 33, 47, 48, 49, 63, 64], 300, 5)
    assert n.mean() > 16
    net, k, v, ro, u0 = memories(env, cfg_of(2), n, 8500)
    a, b = both_ways(env, monkeypatch, "QMANN_NO_QUAD_LONG", lambda: net.hops(k, v, ro, 64, u0), fixed={"QMANN_QUAD_MIN_QUERIES": "0"})
    assert_same(a, b, "stories of 17 .. 64 rows")


@pytest.mark.parametrize("D,V,B,sig", [(60, 30, 5, 40), (256, 4096, 300, 12), (60, 4097, 2000, 1)])
def test_answer_two_pass(env, monkeypatch, D, V, B, sig):
    """batch_answer_i8.hip: qmann_answer_i8 without a probabilities output and with a true exponential runs in one pass unless
    QMANN_ANSWER_TWO_PASS.  Predictions and the match count are equal; the cost is held to the criterion of
    test_gpu_batch.py::test_answer_mfma_i8_one_pass (rel 1e-4, abs 1e-6): two float sums over the batch in different orders
    cannot agree bit for bit."""
    torch, model, abi = env.torch, env.model, env.abi
    rng = np.random.default_rng(D + V + B)
    cfg = cfg_of(2, D=D, V=V)
    w_fmt = (1, 6)
    w_codes = np.clip(np.rint(rng.normal(0, sig, (V, D))), -127, 127).astype(np.int32)
    w_codes[V // 3] = w_codes[V // 2]                        # two identical answers: a tie wherever they win
    w_float = (w_codes / 64.0).astype(np.float32)
    u = (np.clip(np.rint(rng.normal(0, sig, (B, D))), -127, 127) / 4.0).astype(np.float32)
    u[::7] = 0.0                                             # all logits equal: the last index wins
    wts = {"w_h": [np.zeros((D, D), np.float32) for _ in range(3)], "w_ans": w_float}
    net = model.QNet(cfg, wts)
    du = torch.from_numpy(u).to(env.dev)
    w_i8 = net.quantize_i8(torch.from_numpy(w_float).to(env.dev), w_fmt, abi.CODE_TWOS)
    ans_np = rng.integers(0, V, B)
    ans_np[::5] = V - 1
    ans = torch.from_numpy(ans_np.astype(np.int32)).to(env.dev)

    def call():
        pred, _, cost, match, _ = net.answer_i8(du, w_i8, w_fmt, answer=ans)
        return pred, cost, match
    (p1, c1, m1), (p2, c2, m2) = both_ways(env, monkeypatch, "QMANN_ANSWER_TWO_PASS", call)
    np.testing.assert_array_equal(p1.cpu().numpy(), p2.cpu().numpy())
    assert int(m1.item()) == int(m2.item())
    print(f"cost one pass {float(c1.item())!r}, two passes {float(c2.item())!r}")
    assert float(c1.item()) == pytest.approx(float(c2.item()), rel=1e-4, abs=1e-6)
    assert (p1.cpu().numpy()[::7] == V - 1).all()


@pytest.mark.parametrize("mode", [2, 11])
@pytest.mark.parametrize("switch", ["QMANN_EMBED_VALU", "QMANN_EMBED_PER_HOP", "QMANN_EMBED_GENERAL_EPILOGUE"])
def test_embedding_switches_through_the_host_model(env, monkeypatch, switch, mode):
    """The whole HostModel.forward_words on 400 random ragged stories at V = 238, D = 60 under EN_MQ: three hops on a 256-entry
    dictionary, 16 slots per row, take k_embed_story_mfma_hops; QMANN_EMBED_PER_HOP -> k_embed_story_mfma<4, 16>,
    QMANN_EMBED_VALU -> the gather-sum kernel, QMANN_EMBED_GENERAL_EPILOGUE -> ew_to_bytes in every epilogue (EN_MQ has a
    left-, an equal- and a right-shifted hop).  A new model per run: the model path reads the switches too."""
    torch, model = env.torch, env.model
    V, D, B = 238, 60, 400
    rng = np.random.default_rng(8600 + mode)
    sw, qw, n_sen = random_stories(rng, B, V, V - 12, 16, [0, 1, 2, 3, 4, 5, 9, 16, 17, 40, 64])
    cfg = cfg_of(mode, D=D, V=V, en_mq=True)
    wts = weights(8610 + mode, 3, D, V, 1.5)
    row_off = np.concatenate([[0], np.cumsum(n_sen)]).astype(np.int32)
    d_sw = torch.from_numpy(np.ascontiguousarray(sw).view(np.int16)).to(env.dev)
    d_qw = torch.from_numpy(np.ascontiguousarray(qw).view(np.int16)).to(env.dev)
    d_ro = torch.from_numpy(row_off).to(env.dev)

    def call():
        hm = model.HostModel(cfg, wts, device="cuda:0")
        pred, _, _ = hm.forward_words(d_sw, d_qw, d_ro, int(n_sen.max()))
        torch.cuda.synchronize()
        out = pred.clone(), hm.last_u(B)
        hm.close()
        return out
    (p1, u1), (p2, u2) = both_ways(env, monkeypatch, switch, call)
    assert_same(u1, u2, f"{switch}, mode {mode}: last_u")
    np.testing.assert_array_equal(p1.cpu().numpy(), p2.cpu().numpy())

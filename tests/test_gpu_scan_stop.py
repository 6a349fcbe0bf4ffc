"""The early end of the key scan in the fixed-point hop kernel (csrc/batch_hops.hip, step 1b) changes no result.

Every batch of scan_stop_cases.py goes through QNet.hops three times -- (a) without taps: the stopping kernel wherever its gate
opens, (b) with taps: the full scan, (d) without taps under QMANN_NO_SCAN_STOP: the plain kernel -- and the final u of all three
must equal (c) the oracle's, bit for bit, for every query, nothing excused: test_scan_stop_inputs.py shows on the CPU that no
oracle probability of these inputs lies near a truncation step of Q(p), and that the crafted memories put the normaliser where
their names say (weight code 1 just below the bound -- a scan that stops there is caught --, code 0 just above, the bound passed
early, late, in the last tile, or never; the maximum before, behind and far behind the prefix that passes it).
"""
import numpy as np
import pytest

import scan_stop_cases as sc
from conftest import load_pkg

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def env():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    load_pkg()
    import qmann_amd.model as model

    class Env:
        pass
    e = Env()
    e.torch, e.model, e.dev = torch, model, torch.device("cuda:0")
    return e


def check_batch(env, oracle, monkeypatch, batch):
    torch, model = env.torch, env.model
    cfg = batch["cfg"]
    H, D = cfg["n_hop"], cfg["dim_emb"]
    net = model.QNet(cfg, sc.weights_of(batch), device="cuda:0")
    Dp = net.Dp
    n_slots = [q[1].shape[1] for q in batch["queries"]]
    row_off = np.concatenate([[0], np.cumsum(n_slots)]).astype(np.int32)
    R = int(row_off[-1])
    keys = np.zeros((H, R, Dp), np.int8)
    vals = np.zeros((H, R, Dp), np.int8)
    for (_, k, v, _), a in zip(batch["queries"], row_off):
        keys[:, a:a + k.shape[1], :D] = k
        vals[:, a:a + k.shape[1], :D] = v
    u0 = torch.from_numpy(np.stack([q[3] for q in batch["queries"]])).to(env.dev)
    dk = torch.from_numpy(model.to_signmag(keys)).to(env.dev)
    dv = torch.from_numpy(model.to_signmag(vals)).to(env.dev)
    ro = torch.from_numpy(row_off).to(env.dev)
    u_fast = net.hops(dk, dv, ro, batch["max_slots"], u0)
    u_taps, _ = net.hops(dk, dv, ro, batch["max_slots"], u0, taps=True)
    try:
        monkeypatch.setenv("QMANN_NO_SCAN_STOP", "1")
        model.abi.lib.qmann_tuning_reload()
        u_plain = net.hops(dk, dv, ro, batch["max_slots"], u0)
        torch.cuda.synchronize()
    finally:
        monkeypatch.delenv("QMANN_NO_SCAN_STOP", raising=False)
        model.abi.lib.qmann_tuning_reload()
    g_fast, g_taps, g_plain = u_fast.cpu().numpy(), u_taps.cpu().numpy(), u_plain.cpu().numpy()
    bad = []
    for q, ((name, *_), t) in enumerate(zip(batch["queries"], sc.oracle_taps(oracle, batch))):
        want = t["u"][H - 1]
        for what, got in (("no taps", g_fast[q]), ("taps", g_taps[q]), ("QMANN_NO_SCAN_STOP", g_plain[q])):
            if not np.array_equal(got, want):
                bad.append(f"{name}: {what}: {int((got != want).sum())} of {D} columns differ from the oracle")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("H", [1, 3])
@pytest.mark.parametrize("D", [60, 128, 256])
def test_crafted_memories(env, oracle, monkeypatch, D, H):
    """a ragged batch of stopping and non-stopping queries at 64-, 128- and 256-byte rows; no story is a multiple of a tile"""
    check_batch(env, oracle, monkeypatch, sc.crafted_batch(D, H))


def test_max_slots_below_the_story_length(env, oracle, monkeypatch):
    check_batch(env, oracle, monkeypatch, sc.cut_batch())


def test_smallest_four_wavefront_memory_q07(env, oracle, monkeypatch):
    check_batch(env, oracle, monkeypatch, sc.q07_batch())


@pytest.mark.parametrize("sigma", sc.RANDOM_SIGMA)
@pytest.mark.parametrize("iwl", sc.RANDOM_IWL)
def test_random_memories(env, oracle, monkeypatch, iwl, sigma):
    for scale in sorted(sc.SCALES):
        check_batch(env, oracle, monkeypatch, sc.random_batch(iwl, sigma, scale))


def test_planted_survivors_and_narrow_rows(env, oracle, monkeypatch):
    check_batch(env, oracle, monkeypatch, sc.planted_batch())
    check_batch(env, oracle, monkeypatch, sc.d60_batch())


@pytest.mark.parametrize("name", sorted(sc.OTHER_SOFTMAX))
def test_other_softmaxes_keep_their_kernel_and_agree(env, oracle, monkeypatch, name):
    check_batch(env, oracle, monkeypatch, sc.other_softmax_batch(name))

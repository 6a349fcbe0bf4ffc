"""The stopping key scan in its own unit (csrc/hops_common.h::scan_rows_stop, csrc/batch_hops.hip::ScanStop): half-tile
requests, three units per wavefront, and a look that follows the adds of the unit the wavefront has just retired.

test_gpu_scan_stop.py's three-way check on every batch of scan_stop_unit_cases.py -- no taps (the stopping kernel), taps (the
full scan), QMANN_NO_SCAN_STOP (the plain kernel), each bit-equal to the oracle's final u for every query, nothing excused:
test_scan_stop_unit_inputs.py shows on the CPU that these inputs leave no excuse -- with every u_out inside a guard-filled
buffer whose guards must come back untouched.
"""
import numpy as np
import pytest

import scan_stop_cases as sc
import scan_stop_unit_cases as uc
from test_gpu_scan_stop import env  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu

GUARD = 1024                       # floats on either side of u_out
FILL = -7.25e11                    # no state of any format


def check_batch_guarded(env, oracle, monkeypatch, batch):
    """test_gpu_scan_stop.check_batch with every call's u_out in the middle of a buffer of FILL"""
    torch, model = env.torch, env.model
    cfg = batch["cfg"]
    H, D = cfg["n_hop"], cfg["dim_emb"]
    net = model.QNet(cfg, sc.weights_of(batch), device="cuda:0")
    Dp = net.Dp
    n_slots = [q[1].shape[1] for q in batch["queries"]]
    B = len(n_slots)
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

    def call(**kw):
        buf = torch.full((GUARD + B * D + GUARD,), FILL, dtype=torch.float32, device=env.dev)
        net.hops(dk, dv, ro, batch["max_slots"], u0, u_out=buf[GUARD:GUARD + B * D].view(B, D), **kw)
        return buf

    b_fast = call()
    b_taps = call(taps=True)
    try:
        monkeypatch.setenv("QMANN_NO_SCAN_STOP", "1")
        model.abi.lib.qmann_tuning_reload()
        b_plain = call()
        torch.cuda.synchronize()
    finally:
        monkeypatch.delenv("QMANN_NO_SCAN_STOP", raising=False)
        model.abi.lib.qmann_tuning_reload()
    bad = []
    want = [t["u"][H - 1] for t in sc.oracle_taps(oracle, batch)]
    for what, buf in (("no taps", b_fast), ("taps", b_taps), ("QMANN_NO_SCAN_STOP", b_plain)):
        raw = buf.cpu().numpy()
        if not ((raw[:GUARD] == np.float32(FILL)).all() and (raw[GUARD + B * D:] == np.float32(FILL)).all()):
            bad.append(f"{what}: the guard around u_out was written")
        got = raw[GUARD:GUARD + B * D].reshape(B, D)
        for q, (name, *_) in enumerate(batch["queries"]):
            if not np.array_equal(got[q], want[q]):
                bad.append(f"{name}: {what}: {int((got[q] != want[q]).sum())} of {D} columns differ from the oracle")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("D", [128, 256])
def test_every_phase_of_the_unit_loop(env, oracle, monkeypatch, D):
    """all-(+127) memories at Q0.7 from 257 rows: unit counts of every residue modulo 4 x depth, whole and moved-back last units"""
    check_batch_guarded(env, oracle, monkeypatch, uc.phase_batch(D))


@pytest.mark.parametrize("D", [128, 256])
def test_stop_on_the_last_unit_and_its_twins(env, oracle, monkeypatch, D):
    """Q1.6: the bound passed only with the memory's last row; one hot row fewer: not passed; three fewer: the read-out shows"""
    check_batch_guarded(env, oracle, monkeypatch, uc.last_unit_batch(D))


@pytest.mark.parametrize("D", [128, 256])
def test_fresh_look_stops_hop0_and_leaves_hop1_alone(env, oracle, monkeypatch, D):
    """hop 0 crosses with wavefront 0's first unit alone; hop 1 of the same launch must not stop"""
    check_batch_guarded(env, oracle, monkeypatch, uc.fresh_look_batch(D))


def test_narrow_rows_at_every_unit_residue(env, oracle, monkeypatch):
    check_batch_guarded(env, oracle, monkeypatch, uc.d60_unit_batch())

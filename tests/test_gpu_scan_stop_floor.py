"""The stopping key scan's credit for the rows it has not read (csrc/batch_hops.hip::ScanStop: the floor term f_dev, the net
term e_r - f_dev, the lowered threshold thr - S f_dev, and the hop that S f_dev settles before any row is read).

Results do not depend on whether a hop stops, so every memory of scan_stop_floor_cases.py is built to make a WRONG stop
visible (one hot row that keeps weight code 1 within one cold row of the step; test_scan_stop_floor_inputs.py shows it on the
CPU).  Each batch goes through QNet.hops three times -- no taps (the stopping kernel), taps (the full scan), QMANN_NO_SCAN_STOP
(the plain kernel; set through qmann_tuning_reload() inside this process) -- with every u_out in the middle of a guard-filled
buffer, and all three are compared bit for bit with the oracle's final u, nothing excused.  Where the scale of a hop is NaN or
infinite the oracle defines no outcome (its quantiser casts a NaN probability to an integer, which C leaves undefined): there
the stopping kernel must equal the plain kernel and the taps kernel byte for byte.

Sensitivity record.  Scratch builds of the library with ONE arithmetic fault each (a float constant only; none committed),
of the file's 13 cases:
    credit for the unclipped length            1 fails  (the clipped stories)
    f 3 % high                                 4 fail   (the twins at 64-, 128-, 256-byte rows and under the negative scale)
    f from the wrong end under a negative scale  1 fails  (the twins under a scale of -1)
    credit for S + one unit                    3 fail   (the twins at 64-byte rows, the floor-alone batch's survivors, the short path)
The unfaulted build passes all 13.
"""
import numpy as np
import pytest

import scan_stop_cases as sc
import scan_stop_floor_cases as fc
from test_gpu_scan_stop import env  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu

GUARD = 1024                       # floats on either side of u_out
FILL = -7.25e11                    # no state of any format


def run_three(env, monkeypatch, batch):
    """the three calls' whole buffers (guards included), as bytes-comparable arrays"""
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
    return {"no taps": b_fast.cpu().numpy(), "taps": b_taps.cpu().numpy(), "QMANN_NO_SCAN_STOP": b_plain.cpu().numpy()}


def guards_and_rows(batch, raw, what, bad):
    B, D = len(batch["queries"]), batch["cfg"]["dim_emb"]
    if not ((raw[:GUARD] == np.float32(FILL)).all() and (raw[GUARD + B * D:] == np.float32(FILL)).all()):
        bad.append(f"{what}: the guard around u_out was written")
    return raw[GUARD:GUARD + B * D].reshape(B, D)


def check_against_oracle(env, oracle, monkeypatch, batch):
    H, D = batch["cfg"]["n_hop"], batch["cfg"]["dim_emb"]
    want = [t["u"][H - 1] for t in sc.oracle_taps(oracle, batch)]
    bufs = run_three(env, monkeypatch, batch)
    bad = []
    for what, raw in bufs.items():
        got = guards_and_rows(batch, raw, what, bad)
        for q, (name, *_) in enumerate(batch["queries"]):
            if not np.array_equal(got[q], want[q]):
                bad.append(f"{name}: {what}: {int((got[q] != want[q]).sum())} of {D} columns differ from the oracle")
    assert not bad, "\n".join(bad)
    return bufs


def same_bytes(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("D,scale", fc.WIDTH_CASES)
def test_twins_at_every_row_width_and_either_sign_of_the_scale(env, oracle, monkeypatch, D, scale):
    """Q1.6, thr 32.5: the hot row survives at 1 641 rows, the sum settles the hop from 1 668; 64-, 128- and 256-byte rows, and
    a scale layer of -1 (Xmin is then the score of +maxm)"""
    check_against_oracle(env, oracle, monkeypatch, fc.width_batch(D, scale))


def test_settled_by_the_floor_alone_beside_a_survivor(env, oracle, monkeypatch):
    """scale 0.5: S f >= thr from 238 rows, no row is read; the twin of 226 rows keeps its hot row"""
    check_against_oracle(env, oracle, monkeypatch, fc.alone_batch(128))


def test_credit_is_for_the_clipped_length(env, oracle, monkeypatch):
    """stories of 1 800 and 2 500 rows cut to max_slots = 1 641: the hot row inside the clip survives"""
    check_against_oracle(env, oracle, monkeypatch, fc.clipped_batch())


def test_hop0_settled_unread_then_hop1_reads_out(env, oracle, monkeypatch):
    """att_scale (0.5, 1): the skipped scan of hop 0 leaves the hop loop's state clean for hop 1, which must not stop"""
    check_against_oracle(env, oracle, monkeypatch, fc.two_hop_batch(128))


def test_short_path_carries_the_net_term(env, oracle, monkeypatch):
    """31 rows (scan_rows_short) inside a stopping launch: the whole term against the lowered threshold would end the scan"""
    check_against_oracle(env, oracle, monkeypatch, fc.short_batch())


@pytest.mark.parametrize("which", sorted(fc.UNDERFLOW_SCALES))
def test_floor_that_underflows(env, oracle, monkeypatch, which):
    """Q5.2, hop 1's e^(Xmin - Xb) a float denormal or 0: the oracle's result, and the plain kernel's byte for byte"""
    bufs = check_against_oracle(env, oracle, monkeypatch, fc.edge_batch(which))
    assert same_bytes(bufs["no taps"], bufs["QMANN_NO_SCAN_STOP"])


@pytest.mark.parametrize("which", sorted(fc.NONFINITE_SCALES))
def test_scale_that_is_no_number(env, monkeypatch, which):
    """hop 1's scale NaN or infinite (hop 0 opens the gate): the full path, byte for byte what the plain and taps kernels give"""
    batch = fc.edge_batch(which)
    bufs = run_three(env, monkeypatch, batch)
    bad = []
    for what, raw in bufs.items():
        guards_and_rows(batch, raw, what, bad)
    assert not bad, "\n".join(bad)
    assert same_bytes(bufs["no taps"], bufs["QMANN_NO_SCAN_STOP"]) and same_bytes(bufs["no taps"], bufs["taps"])

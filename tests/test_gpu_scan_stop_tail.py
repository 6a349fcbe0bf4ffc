"""The stopping key scan at its edges (csrc/hops_common.h::scan_rows with a hook, csrc/batch_hops.hip::ScanStop): every
exit of the loop that looks after each tile, memories that must not stop although most of the bound is there, 64-byte rows just
beyond the mid kernel, and one launch whose hops decide differently.

test_gpu_scan_stop.py's three-way check on every batch of scan_stop_tail_cases.py: no taps (the stopping kernel), taps (the
full scan), QMANN_NO_SCAN_STOP (the plain kernel), each bit-equal to the oracle's final u for every query, nothing excused --
test_scan_stop_tail_inputs.py shows on the CPU that these inputs leave no excuse.
"""
import pytest

import scan_stop_tail_cases as tc
from test_gpu_scan_stop import check_batch, env  # noqa: F401  (env: the module's fixture)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("D", [128, 256])
def test_every_phase_of_the_loop(env, oracle, monkeypatch, D):
    """a ragged batch of all-(+127) memories at Q0.7: tile counts of every residue, whole and moved-back last tiles"""
    check_batch(env, oracle, monkeypatch, tc.phase_batch(D))


@pytest.mark.parametrize("iwl", sorted(tc.SHORT_HOT))
def test_short_memories_must_not_stop(env, oracle, monkeypatch, iwl):
    """hot rows first, last and spread over the tiles; at Q1.6 a stop on a sum counted twice or left over changes u"""
    check_batch(env, oracle, monkeypatch, tc.short_batch(iwl))


def test_narrow_rows_beyond_the_mid_kernel(env, oracle, monkeypatch):
    check_batch(env, oracle, monkeypatch, tc.d60_tail_batch())


def test_hops_differ_within_one_launch(env, oracle, monkeypatch):
    """hop 0 stops, hop 1 must not: nothing of hop 0's sum may be left in the stop word or in a lane"""
    check_batch(env, oracle, monkeypatch, tc.hops_differ_batch())

"""Ranked answers, CPU side: qmann_answer_topk_f32 (qmann_batch.h) and qmann_model_last_topk (qmann_model.h) are declared,
exported unmangled, bound with argtypes in abi, and reachable as QNet.answer_topk / HostModel.last_topk.  No compute calls."""
import ctypes as C
import re
import subprocess

import pytest

from conftest import ROOT, load_pkg


@pytest.fixture(scope="module")
def abi():
    load_pkg()
    import qmann_amd.abi as a
    return a


def test_both_calls_are_declared_in_the_headers(abi):
    assert "qmann_answer_topk_f32" in abi.header_symbols("qmann_batch.h")
    assert "qmann_model_last_topk" in abi.header_symbols("qmann_model.h")
    assert "qmann_model_last_n_query" in abi.header_symbols("qmann_model.h")
    text = (ROOT / "include" / "qmann_batch.h").read_text()
    assert re.search(r"^#define\s+QMANN_MAX_TOPK\s+16\s*$", text, flags=re.M)


def test_both_calls_are_exported_unmangled(abi):
    out = subprocess.run(["nm", "-D", "--defined-only", str(abi.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert "qmann_answer_topk_f32" in names and "qmann_model_last_topk" in names


def test_both_calls_are_bound_with_argtypes(abi):
    vp, u32 = C.c_void_p, C.c_uint32
    f = abi.lib.qmann_answer_topk_f32
    assert f.restype is C.c_int
    assert list(f.argtypes) == [C.POINTER(abi.Net), vp, vp, u32, vp, vp, u32, vp]
    g = abi.lib.qmann_model_last_topk
    assert g.restype is C.c_int
    assert list(g.argtypes) == [vp, u32, vp, vp, vp]
    n = abi.lib.qmann_model_last_n_query
    assert n.restype is u32 and list(n.argtypes) == [vp]
    assert n(None) == 0                                          # (pure host code: no model, no batch)


def test_the_python_layer_has_both(abi):
    import qmann_amd.model as model
    assert callable(getattr(model.QNet, "answer_topk", None))
    assert callable(getattr(model.HostModel, "last_topk", None))

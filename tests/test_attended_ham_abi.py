"""Attended slots for the packed Hamming forms, CPU side: qmann_hops_shared_top_packed / qmann_hops_shared_split_top_packed
(qmann_batch.h) and qmann_model_ask_words_top_packed (qmann_model.h) are declared, exported unmangled, bound with argtypes in
abi, and reachable as QNet.hops_shared_top_packed / QNet.hops_shared_split_top_packed / HostModel.ask_words_top_packed.  No
compute calls."""
import ctypes as C
import subprocess

import pytest

from conftest import load_pkg

BATCH = ("qmann_hops_shared_top_packed", "qmann_hops_shared_split_top_packed")
MODEL = "qmann_model_ask_words_top_packed"


@pytest.fixture(scope="module")
def abi():
    load_pkg()
    import qmann_amd.abi as a
    return a


def test_the_three_calls_are_declared_in_the_headers(abi):
    for name in BATCH:
        assert name in abi.header_symbols("qmann_batch.h")
    assert MODEL in abi.header_symbols("qmann_model.h")


def test_the_three_calls_are_exported_unmangled(abi):
    out = subprocess.run(["nm", "-D", "--defined-only", str(abi.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {*BATCH, MODEL} <= names


def test_the_three_calls_are_bound_with_argtypes(abi):
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    f = abi.lib.qmann_hops_shared_top_packed
    assert f.restype is C.c_int
    assert list(f.argtypes) == [C.POINTER(abi.Net), vp, sz, vp, sz, u32, vp, vp, u32, vp, vp, u32, vp]
    g = abi.lib.qmann_hops_shared_split_top_packed
    assert g.restype is C.c_int
    assert list(g.argtypes) == [C.POINTER(abi.Net), vp, sz, vp, sz, u32, vp, vp, u32, vp, vp, u32, u32, vp, sz, vp]
    a = abi.lib.qmann_model_ask_words_top_packed
    assert a.restype is C.c_int
    assert list(a.argtypes) == [vp, vp, u32, u32, vp, vp, vp, vp, u32, vp, vp, vp]
    assert a(None, None, 0, 0, None, None, None, None, 5, None, None, None) == abi.QMANN_EINVAL     # (pure host code: no model)


def test_the_python_layer_has_the_three(abi):
    import qmann_amd.model as model
    assert callable(getattr(model.QNet, "hops_shared_top_packed", None))
    assert callable(getattr(model.QNet, "hops_shared_split_top_packed", None))
    assert callable(getattr(model.HostModel, "ask_words_top_packed", None))

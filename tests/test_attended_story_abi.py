"""Attended slots per story, CPU side: qmann_hops_top_i8 (qmann_batch.h) and qmann_model_forward_words_top (qmann_model.h) are
declared, exported unmangled, bound with argtypes in abi, and reachable as QNet.hops_top / HostModel.forward_words_top.
No compute calls."""
import ctypes as C
import subprocess

import pytest

from conftest import load_pkg


@pytest.fixture(scope="module")
def abi():
    load_pkg()
    import qmann_amd.abi as a
    return a


def test_both_calls_are_declared_in_the_headers(abi):
    assert "qmann_hops_top_i8" in abi.header_symbols("qmann_batch.h")
    assert "qmann_model_forward_words_top" in abi.header_symbols("qmann_model.h")


def test_both_calls_are_exported_unmangled(abi):
    out = subprocess.run(["nm", "-D", "--defined-only", str(abi.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert {"qmann_hops_top_i8", "qmann_model_forward_words_top"} <= names


def test_both_calls_are_bound_with_argtypes(abi):
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    f = abi.lib.qmann_hops_top_i8
    assert f.restype is C.c_int
    assert list(f.argtypes) == [C.POINTER(abi.Net), vp, vp, sz, vp, u32, vp, vp, u32, vp, vp, u32, vp]
    g = abi.lib.qmann_model_forward_words_top
    assert g.restype is C.c_int
    assert list(g.argtypes) == [vp, vp, u32, u32, vp, u32, vp, u32, u32, vp, vp, vp, vp, u32, vp, vp, vp]
    # (pure host code: no model)
    assert g(None, None, 0, 0, None, 0, None, 0, 0, None, None, None, None, 5, None, None, None) == abi.QMANN_EINVAL


def test_the_python_layer_has_both(abi):
    import qmann_amd.model as model
    assert callable(getattr(model.QNet, "hops_top", None))
    assert callable(getattr(model.HostModel, "forward_words_top", None))

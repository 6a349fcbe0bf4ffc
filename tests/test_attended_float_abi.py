"""Attended slots for float attention, CPU side: qmann_hops_top_float_i8 and qmann_hops_shared_top_float_i8 (qmann_batch.h),
qmann_model_forward_words_top_float and qmann_model_ask_words_top_float (qmann_model.h) are declared, exported unmangled, bound
with argtypes in abi, and reachable as QNet.hops_top_float / hops_shared_top_float and HostModel.forward_words_top_float /
ask_words_top_float.  No compute calls."""
import ctypes as C
import subprocess

import pytest

from conftest import load_pkg

BATCH = ("qmann_hops_top_float_i8", "qmann_hops_shared_top_float_i8")
MODEL = ("qmann_model_forward_words_top_float", "qmann_model_ask_words_top_float")


@pytest.fixture(scope="module")
def abi():
    load_pkg()
    import qmann_amd.abi as a
    return a


def test_the_four_calls_are_declared_in_the_headers(abi):
    assert set(BATCH) <= set(abi.header_symbols("qmann_batch.h"))
    assert set(MODEL) <= set(abi.header_symbols("qmann_model.h"))


def test_the_four_calls_are_exported_unmangled(abi):
    out = subprocess.run(["nm", "-D", "--defined-only", str(abi.LIB_PATH)], capture_output=True, text=True, check=True).stdout
    names = {l.split()[-1] for l in out.splitlines() if " T " in l}
    assert set(BATCH + MODEL) <= names


def test_the_four_calls_are_bound_with_argtypes(abi):
    vp, u32, sz = C.c_void_p, C.c_uint32, C.c_size_t
    f = abi.lib.qmann_hops_top_float_i8
    assert f.restype is C.c_int
    assert list(f.argtypes) == [C.POINTER(abi.Net), vp, vp, sz, vp, u32, vp, vp, u32, vp, vp, u32, vp]
    f = abi.lib.qmann_hops_shared_top_float_i8
    assert f.restype is C.c_int
    assert list(f.argtypes) == [C.POINTER(abi.Net), vp, vp, sz, u32, vp, vp, u32, vp, vp, u32, vp]
    g = abi.lib.qmann_model_forward_words_top_float
    assert g.restype is C.c_int
    assert list(g.argtypes) == [vp, vp, u32, u32, vp, u32, vp, u32, u32, vp, vp, vp, vp, u32, vp, vp, vp]
    a = abi.lib.qmann_model_ask_words_top_float
    assert a.restype is C.c_int
    assert list(a.argtypes) == [vp, vp, u32, u32, vp, vp, vp, vp, u32, vp, vp, vp]


def test_a_null_model_is_einval(abi):
    """(pure host code: no model, no device)"""
    assert abi.lib.qmann_model_forward_words_top_float(None, None, 0, 0, None, 0, None, 0, 0, None, None, None, None, 5, None, None,
                                                       None) == abi.QMANN_EINVAL
    assert abi.lib.qmann_model_ask_words_top_float(None, None, 0, 3, None, None, None, None, 5, None, None, None) == abi.QMANN_EINVAL
    # a null net is the first refusal of both hop calls, whatever k
    assert abi.lib.qmann_hops_top_float_i8(None, None, None, 0, None, 0, None, None, 0, None, None, 0, None) == abi.QMANN_EINVAL
    assert abi.lib.qmann_hops_shared_top_float_i8(None, None, None, 0, 0, None, None, 0, None, None, 0, None) == abi.QMANN_EINVAL


def test_the_python_layer_has_all_four(abi):
    import qmann_amd.model as model
    for name in ("hops_top_float", "hops_shared_top_float"):
        assert callable(getattr(model.QNet, name, None)), name
    for name in ("forward_words_top_float", "ask_words_top_float"):
        assert callable(getattr(model.HostModel, name, None)), name

"""CPU-side checks of the classifier-from-data entry points (gp_ep_create_rbf, gp_ep_predict_rbf, gp_ep_predict_rbf_dev): exported,
bound, and a null handle is an argument error -- no compute, so no GPU."""
import ctypes

import pytest

import __graft_entry__ as entry
from gp_algos_amd import _lib

NAMES = ("gp_ep_create_rbf", "gp_ep_predict_rbf", "gp_ep_predict_rbf_dev")


@pytest.fixture(scope="module")
def lib():
    entry.build()
    return _lib.load()


def test_symbols_are_exported(lib):
    for name in NAMES:
        assert hasattr(lib, name), name


def test_symbols_are_in_the_binding_table():
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["gp_ep_create_rbf"][1]) == 8
    assert len(_lib.SIGNATURES["gp_ep_predict_rbf"][1]) == 7
    assert len(_lib.SIGNATURES["gp_ep_predict_rbf_dev"][1]) == 8


def test_null_handles_are_argument_errors(lib):
    x = (ctypes.c_double * 6)(0.0, 1.0, 2.0, 0.5, 1.5, 2.5)
    y = (ctypes.c_int32 * 3)(1, -1, 1)
    theta = (ctypes.c_double * 4)(1.0, 1.0, 1.0, 0.1)
    out = (ctypes.c_double * 3)()
    h = ctypes.c_void_p()
    assert lib.gp_ep_create_rbf(None, x, 3, 2, 3, y, theta, ctypes.byref(h)) == _lib.GP_EINVAL
    assert not h.value
    assert lib.gp_ep_predict_rbf(None, x, 3, 3, out, None, None) == _lib.GP_EINVAL
    assert lib.gp_ep_predict_rbf_dev(None, None, 3, 3, 0, None, None, None) == _lib.GP_EINVAL

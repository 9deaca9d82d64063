"""include/mvx.h against the ctypes table, for every function the header declares and in both directions: the names, the return
type, the parameter count, every parameter's type by the one rule of tests/abi.matches, the exported symbol; the parameter names
the tests pin; the version, in its one place. No GPU: nothing is called but mvx_version."""
import ctypes as C

import pytest

from molvoxel_amd.voxelizer.hip import _lib
from tests import abi
from tests import abi_calls

DECL = abi.declarations()


def test_the_header_and_the_table_name_the_same_functions():
    assert len(DECL) >= 52
    assert set(DECL) - set(_lib.SIGNATURES) == set(), "declared in include/mvx.h, missing from _lib.SIGNATURES"
    assert set(_lib.SIGNATURES) - set(DECL) == set(), "in _lib.SIGNATURES, not declared in include/mvx.h"


@pytest.mark.parametrize("name", list(DECL))
def test_the_ctypes_prototype_matches_the_header(name):
    res_text, params = DECL[name]
    assert name in _lib.SIGNATURES, f"{name} is declared in include/mvx.h but _lib.SIGNATURES does not have it"
    res, args = _lib.SIGNATURES[name]
    assert res is abi.RETURN[res_text], (name, res_text, res)
    assert len(args) == len(params), (name, len(args), len(params))
    for i, ((type_text, pname), ctype) in enumerate(zip(params, args)):
        assert abi.matches(type_text, ctype), f"{name}: parameter {i} is `{type_text} {pname}` in the header, {ctype.__name__} in the table"
    assert hasattr(_lib.load(), name), f"{name} declared in include/mvx.h but not exported"


@pytest.mark.parametrize("name", list(abi.PINNED_NAMES))
def test_the_header_keeps_the_pinned_parameter_names(name):
    assert [pname for _, pname in DECL[name][1]] == abi.PINNED_NAMES[name]


def test_the_version_is_pinned_in_one_place():
    assert _lib.load().mvx_version() == abi.header_version() == abi.VERSION


def test_the_struct_sizes_the_abi_promises():
    assert C.sizeof(_lib.MvxConfig) == 40 and C.sizeof(_lib.MvxXform) == 80


@pytest.mark.parametrize("name", list(abi_calls.ARGS))
def test_the_recorded_argument_lists_have_the_declared_length(name):
    assert len(abi_calls.ARGS[name]) == len(DECL[name][1])


def test_the_rule_itself():
    assert abi.matches("int64_t", C.c_int64) and not abi.matches("int64_t", C.c_int32) and not abi.matches("int64_t", C.c_void_p)
    assert abi.matches("const double *", C.c_void_p) and not abi.matches("const double *", C.c_int64)
    assert abi.matches("float *", C.POINTER(C.c_float)) and not abi.matches("float *", C.POINTER(C.c_int))
    assert abi.matches("mvx_handle **", C.POINTER(_lib.Handle)) and abi.matches("void **", C.POINTER(C.c_void_p))
    assert abi.matches("const char *", C.c_char_p) and not abi.matches("double", C.c_float)
    assert abi.MVX_ERR_INVALID == -1 and abi.MVX_ERR_ALLOC == -4

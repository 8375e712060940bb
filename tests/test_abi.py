"""CPU-side checks of the drop-in boundary: the shared library loads and exports every symbol
that include/dransac.h declares, and every entry checks its arguments before it launches anything
(no compute calls: there is no GPU here)."""
import ctypes
import os
import re

import pytest

from differentiable_ransac_amd import _lib as L


def _declared():
    src = open(L.HEADER_PATH).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(dr_[a-z0-9_]+)\s*\(", src)))


def test_library_exports_every_declared_symbol():
    assert os.path.exists(L.LIB_PATH), "run python -m differentiable_ransac_amd.build"
    lib = L.lib()
    names = _declared()
    assert "dr_msac_score_f32" in names and len(names) >= 10
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing


def test_version_and_error_string():
    lib = L.lib()
    assert lib.dr_version() == 1
    assert isinstance(lib.dr_last_error(), bytes)


def test_bad_arguments_return_einval_without_touching_the_gpu():
    lib = L.lib()
    rc = lib.dr_msac_score_f32(None, None, None, None, 1, 1, 1, None, None, None, None, None)
    assert rc == -1
    assert b"null" in lib.dr_last_error()


# ---- every entry: checks first, launch below; the error names the exported symbol ----------------------------------

def _zeros(name):
    """the entry's argument list with NULL in every pointer slot and 0 in every other: refused before any launch"""
    return [None if t is L.c_pointer else 0 for t in L.entries()[name]]


def test_the_parser_sees_every_declared_entry():
    names = list(L.entries())
    assert sorted(names + ["dr_version", "dr_last_error"]) == _declared()
    assert len(names) == len(set(names)) >= 100


@pytest.mark.parametrize("name", list(L.entries()))
def test_all_zero_arguments_are_refused_under_the_entrys_own_name(name):
    lib = L.lib()
    rc = getattr(lib, name)(*_zeros(name))
    assert rc == -1   # DR_EINVAL
    assert lib.dr_last_error().decode().startswith(name + ":"), lib.dr_last_error()


# ---- the binding: lib() types every entry from the header, call() refuses a list that does not fit --------------------

_EINVAL = "failed with status -1"      # the C function ran its checks: the argument list went through the binding
_BUF = (ctypes.c_char * 64)()


def test_every_entry_carries_the_argtypes_of_the_header():
    lib = L.lib()
    for name, argtypes in L.entries().items():
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and list(fn.argtypes) == argtypes, name
    pointers = sum(t is L.c_pointer for a in L.entries().values() for t in a)
    assert pointers > 500 and ctypes.c_void_p not in {t for a in L.entries().values() for t in a}


def _not_entered(name, *args, match):
    """L.call(name, *args) raises `match` and the C function does not run: the last error stays another entry's"""
    lib = L.lib()
    assert lib.dr_seed_next_n(None, None, 0, None) == -1 and lib.dr_last_error().startswith(b"dr_seed_next_n:")
    with pytest.raises(L.DransacError, match=match):
        L.call(name, *args)
    assert lib.dr_last_error().startswith(b"dr_seed_next_n:")


@pytest.mark.parametrize("name", ["dr_gumbel_topk_gather_f32", "dr_kabsch_gather_f64"])
def test_one_argument_too_few_or_too_many_is_refused(name):
    n = len(L.entries()[name])
    _not_entered(name, *_zeros(name)[:-1], match=f"{name} takes {n} arguments, {n - 1} given")
    _not_entered(name, *_zeros(name), None, match=f"{name} takes {n} arguments, {n + 1} given")
    with pytest.raises(L.DransacError, match=_EINVAL):
        L.call(name, *_zeros(name))


def test_a_value_of_the_wrong_kind_is_refused_with_its_position():
    _not_entered("dr_seed_next_n", _BUF, _BUF, 1.0, None, match="dr_seed_next_n: argument 3")        # a float in an int slot
    _not_entered("dr_seed_next_n", _BUF, 64, 1, None, match="dr_seed_next_n: argument 2")            # an int in a pointer slot
    _not_entered("dr_seed_next_n", 1, _BUF, _BUF, None, match="dr_seed_next_n: argument 1")          # a list shifted by one
    _not_entered("dr_rigid_residual_f64", _BUF, _BUF, "0.1", 1, 0, 3, _BUF, None, None, match="argument 3")
    _not_entered("dr_no_such_entry", None, match="dr_no_such_entry is not an entry")
    assert L.c_void_p.from_param(64) is not None       # (what the stock pointer type lets through)


@pytest.mark.parametrize("pointer", [None, L.ptr(None), _BUF, ctypes.cast(_BUF, ctypes.POINTER(ctypes.c_float)), L.c_pointer(0)])
@pytest.mark.parametrize("n", [3, True, L.c_int(3)])
def test_pointer_and_int_slots_take_plain_and_ready_made_values(pointer, n):
    with pytest.raises(L.DransacError, match=_EINVAL):
        L.call("dr_seed_next_n", pointer, None, n, None)


@pytest.mark.parametrize("thr", [1.0, 1, L.c_float(1.0)])
def test_a_float_slot_takes_floats_ints_and_c_float(thr):
    with pytest.raises(L.DransacError, match=_EINVAL):
        L.call("dr_rigid_residual_f32", _BUF, _BUF, thr, 1, 0, 3, _BUF, None, 0, None)      # M = 0
    with pytest.raises(L.DransacError, match=_EINVAL):
        L.call("dr_rigid_residual_f64", _BUF, _BUF, getattr(thr, "value", thr), 1, 0, 3, _BUF, None, None)


def test_a_refused_list_leaves_no_stale_devices_or_tensors():
    for bad in (["dr_seed_next_n", None, None, 1], ["dr_seed_next_n", None, None, 1.0, None]):
        L._reset()
        L._ctx.keep.append(object())        # what ptr() records for the list: a tensor to keep alive ...
        if len(bad) == 4:
            L._devices().add(5)             # ... and its device (the list of wrong length is refused before the device is looked at)
        with pytest.raises(L.DransacError, match="dr_seed_next_n"):
            L.call(*bad)
        assert L._ctx.devs == set() and L._ctx.keep == []
        with pytest.raises(L.DransacError, match=_EINVAL):      # the next call: no "tensors ... on different GPUs", no device switch
            L.call("dr_seed_next_n", None, None, 1, None)


def test_an_unknown_parameter_type_stops_the_parser():
    good = "int dr_a_f32(const float *x, int n, uint64_t seed, void *stream); /* int dr_b(size_t n); */\n// int dr_c(long n);\n"
    assert L.parse_header(good) == {"dr_a_f32": [L.c_pointer, ctypes.c_int, ctypes.c_uint64, L.c_pointer]}
    for bad in ("size_t n", "long n", "hipStream_t stream", "float x[9]", "int"):
        with pytest.raises(L.DransacError, match="dr_a_f32"):
            L.parse_header(good.replace("int n", bad))


def test_a_missing_header_is_an_error_that_names_the_path(monkeypatch, tmp_path):
    monkeypatch.setattr(L, "HEADER_PATH", str(tmp_path / "dransac.h"))
    with pytest.raises(L.DransacError, match=str(tmp_path / "dransac.h")):
        L.entries.__wrapped__()

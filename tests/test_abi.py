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
    lib.dr_msac_score_f32.restype = ctypes.c_int
    rc = lib.dr_msac_score_f32(None, None, None, None, 1, 1, 1, None, None, None, None, None)
    assert rc == -1
    assert b"null" in lib.dr_last_error()


# ---- every entry: checks first, launch below; the error names the exported symbol ----------------------------------

_SCALARS = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float,
            "double": ctypes.c_double}


def _entries():
    """(name, argtypes) of every int dr_*(...) declaration of the header."""
    src = open(L.HEADER_PATH).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    out = []
    for ret, name, params in re.findall(r"\b(int|const\s+char\s*\*)\s*(dr_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        if name in ("dr_version", "dr_last_error"):
            continue
        assert ret == "int", name
        argtypes = []
        for prm in params.split(","):
            ctype = " ".join(re.match(r"(.*?)\w+$", " ".join(prm.split())).group(1).split())   # the parameter less its name
            argtypes.append(ctypes.c_void_p if ctype.endswith("*") else _SCALARS[ctype])
        out.append((name, argtypes))
    return out


def test_the_parser_sees_every_declared_entry():
    names = [n for n, _ in _entries()]
    assert sorted(names + ["dr_version", "dr_last_error"]) == _declared()
    assert len(names) == len(set(names)) >= 100


@pytest.mark.parametrize("name,argtypes", _entries(), ids=[n for n, _ in _entries()])
def test_all_zero_arguments_are_refused_under_the_entrys_own_name(name, argtypes):
    lib = L.lib()
    fn = getattr(lib, name)
    fn.restype, fn.argtypes = ctypes.c_int, argtypes
    try:
        rc = fn(*[t(0) if t is not ctypes.c_void_p else None for t in argtypes])
    finally:
        fn.argtypes = None   # (the handle is shared with the wrappers, which pass ready-made ctypes values)
    assert rc == -1   # DR_EINVAL
    assert lib.dr_last_error().decode().startswith(name + ":"), lib.dr_last_error()

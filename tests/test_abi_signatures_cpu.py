"""CPU: the ctypes signatures of the shim against the prototypes of include/fa_mi355x.h.  A wrong argtypes entry is silent undefined
behaviour at the boundary, so every exported function's argtypes and restype must be what its declaration says, and the shim's
table of named fields must have one field per parameter."""
import ctypes
import os
import re

import pytest

import flashattention_lab_cuda as ext

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "fa_mi355x.h")

SCALARS = {"int64_t": ctypes.c_int64, "int": ctypes.c_int, "double": ctypes.c_double, "uint64_t": ctypes.c_uint64,
           "size_t": ctypes.c_size_t}


def _ctype(decl):
    """the ctypes type of a C parameter or return type: `const float* lse`, `int64_t bh`, `const char*`, ..."""
    words = decl.replace("*", " * ").split()
    words = [w for w in words if w != "const"]
    if "*" in words:
        assert words.count("*") == 1, decl
        return ctypes.c_char_p if words[0] == "char" else ctypes.c_void_p
    return SCALARS[words[0]]


def _prototypes():
    """{name: (restype, [argtypes], [parameter names])} of every function the header declares"""
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    src = re.sub(r"//[^\n]*", "", src)
    src = re.sub(r"^\s*#.*$", "", src, flags=re.M)
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(fa[0-9_a-z]*)\s*\(([^()]*)\)\s*;", src):
        params = [" ".join(p.split()) for p in params.split(",")]
        if params == ["void"]:
            params = []
        assert name not in out, name
        out[name] = (_ctype(ret), [_ctype(p) for p in params], [re.split(r"[\s\*]+", p)[-1] for p in params])
    return out


PROTOTYPES = _prototypes()


def test_the_header_parses_into_every_exported_symbol():
    assert set(PROTOTYPES) == set(ext.EXPORTED_C_SYMBOLS)
    assert PROTOTYPES["fa_last_error"] == (ctypes.c_char_p, [], [])
    assert PROTOTYPES["fa_set_option"][:2] == (ctypes.c_int, [ctypes.c_char_p, ctypes.c_int])
    assert PROTOTYPES["fa_ex_backward_workspace_bytes"][:2] == (ctypes.c_size_t, [ctypes.c_int64] * 4 + [ctypes.c_int])
    assert len(PROTOTYPES["fa_ex_forward_kvcache_varlen"][1]) == 63


@pytest.mark.parametrize("name", ext.EXPORTED_C_SYMBOLS)
def test_argtypes_and_restype_are_the_declaration(name):
    restype, argtypes, _names = PROTOTYPES[name]
    fn = getattr(ext._lib, name)
    assert fn.restype is restype
    assert list(fn.argtypes) == argtypes


@pytest.mark.parametrize("name", sorted(ext._SIGNATURES))
def test_the_table_names_one_field_per_parameter(name):
    _restype, argtypes, names = PROTOTYPES[name]
    fields = [field for field, _ctype in ext._SIGNATURES[name][1]]
    assert len(fields) == len(argtypes)
    assert len(set(fields)) == len(fields)   # (a family's getters find an argument by its field)
    assert fields == names                   # (and the fields carry the header's parameter names)


@pytest.mark.parametrize("name", sorted(ext._CALLS))
def test_call_hands_an_entry_point_its_own_arguments_of_the_widest_ones(name):
    _fn, own, count = ext._CALLS[name]
    widest = [w for w in ext._CALLS if len(ext._SIGNATURES[w][1]) == count and ext._CALLS[w][2] == count and
              set(PROTOTYPES[name][2]) <= set(PROTOTYPES[w][2])]
    assert len(widest) == 1
    assert list(own(tuple(PROTOTYPES[widest[0]][2]))) == PROTOTYPES[name][2]

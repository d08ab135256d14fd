"""CPU: every function include/aurppo.h declares is bound in ``_lib`` with that prototype's parameter count, parameter classes
and result type.  The header is the truth: ctypes converts whatever it is told to, so a binding that drifts from the header
passes a pointer where the library reads an int (or the reverse) without a word on the host."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"float": 4, "double": 8, "int": 4, "int32_t": 4, "uint32_t": 4, "uint8_t": 1, "int64_t": 8, "long long": 8}
OPAQUE = ("void", "aurppo_rng", "aurppo_p2p")          # no size on this side of the ABI: c_void_p only


def _prototypes():
    """{name: (result, [parameter type without its name, ...])} of every function the header declares."""
    src = open(os.path.join(ROOT, "include", "aurppo.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for res, name, params in re.findall(r"\b(int|size_t|const\s+char\s*\*)\s*(aurppo_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", src):
        types = []
        for p in (q.strip() for q in params.split(",")):
            if p == "void":
                continue
            p = re.sub(r"\s+", " ", p)
            types.append(p[:p.rindex("*") + 1] if "*" in p else p.rsplit(" ", 1)[0])      # drop the parameter's name
        assert name not in out, name
        out[name] = (re.sub(r"\s+", " ", res).replace(" *", "*"), types)
    return out


PROTOTYPES = _prototypes()


def _is_int(t, size, signed):
    return (isinstance(t, type) and issubclass(t, C._SimpleCData) and t._type_ not in "fdgPzZO?" and C.sizeof(t) == size
            and (t(-1).value == -1) == signed)


def _matches(ctype, decl):
    """Does the bound ctypes type fit the C parameter type ``decl`` (name already dropped)?"""
    if decl.endswith("*"):
        if ctype is C.c_void_p:
            return True
        pointee = decl[:-1].replace("const", "").strip()
        if pointee.endswith("*"):
            size = C.sizeof(C.c_void_p)
        elif pointee in OPAQUE:
            return False
        else:
            size = SIZES[pointee]
        return isinstance(ctype, type) and issubclass(ctype, C._Pointer) and C.sizeof(ctype._type_) == size
    if decl in ("int", "int32_t"):
        return _is_int(ctype, 4, True)
    if decl == "uint32_t":
        return _is_int(ctype, 4, False)
    if decl in ("int64_t", "long long"):
        return _is_int(ctype, 8, True)
    if decl == "double":
        return ctype is C.c_double
    raise AssertionError(f"a parameter type this test does not know: {decl!r}")


def test_the_header_parses_completely():
    from aur_ppo_amd import _lib
    assert len(PROTOTYPES) >= 63 and sorted(PROTOTYPES) == sorted(_lib.SYMBOLS)
    spellings = {t for _, types in PROTOTYPES.values() for t in types}
    assert len(spellings) >= 20 and all(t.endswith("*") or t in SIZES for t in spellings), sorted(spellings)
    sized = sorted(n for n, (res, _) in PROTOTYPES.items() if res == "size_t")
    assert "aurppo_mlp_wide_workspace_bytes" in sized and "aurppo_head_ppo_workspace_bytes" in sized and len(sized) >= 8
    assert [n for n, (res, _) in PROTOTYPES.items() if res == "const char*"] == ["aurppo_last_error"]


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    g.build()
    from aur_ppo_amd import _lib
    return _lib.load()


def test_size_t_results_are_bound_as_size_t(lib):
    """A workspace size read as a C int is truncated above 2 GB and sign-extended by ctypes."""
    names = sorted(n for n, (res, _) in PROTOTYPES.items() if res == "size_t")
    assert "aurppo_mlp_wide_workspace_bytes" in names and "aurppo_head_ppo_workspace_bytes" in names and len(names) >= 8
    for name in names:
        assert getattr(lib, name).restype is C.c_size_t, name


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
def test_binding_matches_the_header(lib, name):
    res, types = PROTOTYPES[name]
    fn = getattr(lib, name)
    bound = tuple(fn.argtypes or ())                  # never set: no parameters, which must be what the header says
    assert len(bound) == len(types), f"{name}: {len(bound)} argtypes bound, the header declares {len(types)}: {types}"
    for i, (ctype, decl) in enumerate(zip(bound, types)):
        assert _matches(ctype, decl), f"{name}: parameter {i} is {decl!r} in the header, bound as {ctype}"
    if res == "size_t":
        assert fn.restype is C.c_size_t, name          # read as a C int it is truncated above 2 GB and sign-extended
    elif res == "const char*":
        assert fn.restype is C.c_char_p, name
    else:
        assert _is_int(fn.restype, 4, True), name

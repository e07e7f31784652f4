"""The ctypes table of lol_amd/_abi.py against include/lolhip.h (host; reads the table and the header only, no built
library): ctypes truncates a 64-bit argument silently when `argtypes` is wrong and a 64-bit return when `restype` is
missing, so every bound entry's parameter kinds, parameter count and return type are compared with its prototype, the
bound set with the declared set, and the binding's constants with the header's enumerators."""
import ctypes as C
import os
import re

from lol_amd import _abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "lolhip.h")).read()

# the reference's own symbol names, for linking Lol's Haskell against the library; Python has the batched entries
DROP_IN = {"tensorCRTRq", "tensorCRTInvRq", "mulRq", "tensorLRq", "tensorLInvRq", "tensorGPowRq", "tensorGDecRq",
           "tensorGInvPowRq", "tensorGInvDecRq"}

SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "uint32_t": C.c_uint32, "int16_t": C.c_int16,
           "double": C.c_double}
RETURNS = {"int": C.c_int, "int64_t": C.c_int64, "void": None, "const char *": C.c_char_p}


def _code(text):
    """the header without comments and preprocessor lines"""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return "\n".join(ln for ln in text.split("\n") if not ln.lstrip().startswith("#"))


def _kind(param):
    """a parameter declaration -> "ptr" or its scalar type name"""
    if "*" in param or "[" in param:
        return "ptr"
    return " ".join([w for w in param.split() if w != "const"][:-1])      # the type, without the parameter's name


def prototypes():
    """{name: (return type, [parameter kind])} of every LOLHIP_API prototype"""
    out = {}
    for ret, name, params in re.findall(r"LOLHIP_API\s+([\w\s]+?[\w\*])\s*\b(\w+)\s*\(([^()]*)\)\s*;", _code(HEADER)):
        params = " ".join(params.split())
        out[name] = (" ".join(ret.split()), [] if params == "void" else [_kind(p.strip()) for p in params.split(",")])
    return out


def _ctypes_kind(t):
    if t in (C.c_void_p, C.c_char_p) or hasattr(t, "_type_") and not isinstance(t._type_, str):
        return "ptr"                                                       # POINTER(...) types carry the pointee in _type_
    return next(name for name, ct in SCALARS.items() if ct is t)


def test_every_prototype_is_parsed():
    assert len(prototypes()) == len(re.findall(r"\bLOLHIP_API\b", _code(HEADER))) > 100


def test_bound_set_is_the_declared_set_without_the_drop_in_symbols():
    declared = set(prototypes())
    assert DROP_IN <= declared
    assert set(_abi.ABI) == declared - DROP_IN


def test_parameter_kinds_and_counts():
    protos = prototypes()
    for name, (_, argtypes) in _abi.ABI.items():
        want = protos[name][1]
        assert set(want) <= set(SCALARS) | {"ptr"}, (name, want)
        assert [_ctypes_kind(t) for t in argtypes] == want, name


def test_return_types():
    protos = prototypes()
    for name, (restype, _) in _abi.ABI.items():
        assert restype is RETURNS[protos[name][0]], name


def test_bind_applies_the_table():
    class Fn:
        pass
    fake = type("Lib", (), {name: Fn() for name in _abi.ABI})()
    _abi.bind(fake)
    for name, (restype, argtypes) in _abi.ABI.items():
        assert getattr(fake, name).restype is restype and getattr(fake, name).argtypes == argtypes


def test_constants_equal_the_enumerators():
    enums = {k: int(v) for k, v in re.findall(r"\bLOLHIP_(\w+)\s*=\s*(-?\d+)", _code(HEADER))}
    ours = {k: v for k, v in vars(_abi).items() if k == "OK" or k.startswith(("ERR_", "OP_", "EXT_", "ELT_"))}
    groups = {g: {k for k in enums if k == g or k.startswith(g + "_")} for g in ("OK", "ERR", "OP", "EXT", "ELT")}
    assert all(groups.values())
    assert set(ours) == set().union(*groups.values())
    assert all(ours[k] == enums[k] for k in ours)
    import lol_amd.tensor as t
    assert all(getattr(t, k) == v for k, v in ours.items())

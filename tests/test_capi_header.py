"""CPU test: the prototype table and the ctypes structures of pinn_elastodynamics_amd/capi.py against include/pinn_hip.h.  Reads the header and
imports capi, nothing else: no built library is needed.  A wrong width in the table (c_int where the header says int64_t) would corrupt
arguments silently; here it fails by name."""
import ctypes as C
import os
import re

from pinn_elastodynamics_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64, "size_t": C.c_size_t, "double": C.c_double,
           "float": C.c_float}
ARG_SCALARS = ("int", "int64_t", "uint32_t", "uint64_t", "size_t", "double")
RETURNS = {"int": C.c_int, "size_t": C.c_size_t, "float": C.c_float, "void": None, "const char*": C.c_char_p}
STRUCTS = {"PointSet", "StreamSet", "Ball", "AdamState", "RangeState", "LbfgsOptions", "LbfgsRecord"}
DEFINES = {}


def class_name(c_name):
    """pinn_stream_set -> StreamSet"""
    assert c_name.startswith("pinn_")
    return "".join(p.title() for p in c_name[5:].split("_"))


def parse_header():
    """(prototypes {name: (return type, [parameter declarations])}, structs {typedef name: [field declarations]}) of the header, comments stripped"""
    src = open(os.path.join(ROOT, "include", "pinn_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    DEFINES.update({k: int(v) for k, v in re.findall(r"^\s*#\s*define\s+(\w+)\s+(\d+)\s*$", src, flags=re.M)})
    src = re.sub(r"^\s*#[^\n]*$", " ", src, flags=re.M)
    structs = {}
    for body, name in re.findall(r"typedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", src):
        structs[name] = [d.strip() for d in body.split(";") if d.strip()]
    src = re.sub(r"typedef\s+struct\s*\w*\s*\{[^{}]*\}\s*\w+\s*;", " ", src)
    src = re.sub(r"enum\s*\{[^{}]*\}\s*;", " ", src)
    src = re.sub(r'extern\s+"C"', " ", src).replace("{", " ").replace("}", " ")
    protos = {}
    for stmt in src.split(";"):
        m = re.match(r"^(.*?)\b(pinn_[a-z0-9_]+)\s*\((.*)\)$", " ".join(stmt.split()), flags=re.S)
        if m:
            ret, name, params = m.group(1).strip(), m.group(2), m.group(3).strip()
            assert name not in protos, f"{name} declared twice"
            protos[name] = (ret, [] if params in ("", "void") else [p.strip() for p in params.split(",")])
    return protos, structs


PROTOS, HEADER_STRUCTS = parse_header()


def is_pointer(t):
    return t in (C.c_void_p, C.c_char_p) or (isinstance(t, type) and issubclass(t, C._Pointer))


def base_type(decl):
    """'const float* x' -> 'float', 'const pinn_ball* balls' -> 'pinn_ball', 'int64_t n' -> 'int64_t', 'unsigned char h[128]' -> 'unsigned char'"""
    words = re.sub(r"\[[^\]]*\]", " ", decl).replace("*", " ").split()
    words = [w for w in words if w != "const"]
    return " ".join(words[:-1])


def test_table_and_header_declare_the_same_functions():
    assert len(PROTOS) >= 62, sorted(PROTOS)
    assert set(PROTOS) == set(capi.PROTOTYPES), (sorted(set(PROTOS) - set(capi.PROTOTYPES)), sorted(set(capi.PROTOTYPES) - set(PROTOS)))


def test_every_prototype_agrees_with_the_header():
    assert len(PROTOS) >= 62
    for name, (ret, params) in PROTOS.items():
        restype, argtypes = capi.PROTOTYPES[name]
        assert ret.replace(" *", "*") in RETURNS, (name, ret)
        assert restype is RETURNS[ret.replace(" *", "*")], (name, ret, restype)
        assert len(argtypes) == len(params), (name, len(params), len(argtypes))
        for k, (decl, t) in enumerate(zip(params, argtypes)):
            if "*" in decl or "[" in decl:
                assert is_pointer(t), (name, k, decl, t)
                if t not in (C.c_void_p, C.c_char_p) and issubclass(t._type_, C.Structure):      # a typed structure pointer: the header's structure
                    assert class_name(base_type(decl)) == t._type_.__name__, (name, k, decl, t._type_)
            else:
                assert base_type(decl) in ARG_SCALARS, (name, k, decl)
                assert t is SCALARS[base_type(decl)], (name, k, decl, t)


def header_fields(decls):
    """field declarations of a struct body -> [(name, 'ptr' | (ctypes scalar, dims))]; 'double lr, beta1;' declares two"""
    out = []
    for decl in decls:
        first, *more = [d.strip() for d in decl.split(",")]
        base = base_type(first)
        for d in [first] + [f"{base} {m}" for m in more]:
            name = re.sub(r"\[[^\]]*\]", "", d).replace("*", " ").split()[-1]
            if "*" in d:
                assert not more, f"pointer declarators share a line: {decl}"
                out.append((name, "ptr"))
            else:
                dims = tuple(int(DEFINES.get(v, v)) for v in re.findall(r"\[([^\]]*)\]", d))
                out.append((name, (SCALARS[base], dims)))
    return out


def ctypes_fields(struct):
    out = []
    for name, t in struct._fields_:
        dims = []
        while isinstance(t, type) and issubclass(t, C.Array):
            dims.append(t._length_)
            t = t._type_
        out.append((name, "ptr" if is_pointer(t) else (t, tuple(dims))))
    return out


def test_every_structure_agrees_with_the_header():
    assert {class_name(n) for n in HEADER_STRUCTS} == STRUCTS, sorted(HEADER_STRUCTS)
    for c_name, decls in HEADER_STRUCTS.items():
        struct = getattr(capi, class_name(c_name))
        assert issubclass(struct, C.Structure)
        assert ctypes_fields(struct) == header_fields(decls), (c_name, ctypes_fields(struct), header_fields(decls))


def test_the_parser_reads_what_it_is_given():
    """guards against a parser that passes by matching nothing: known declarations come out as written"""
    assert PROTOS["pinn_sample_box"] == ("int", ["uint64_t seed", "uint32_t stream_id", "uint64_t first", "int64_t n", "int dim", "const double lo[4]",
                                                 "const double hi[4]", "float* x", "float* y", "float* z", "float* t", "void* stream"])
    assert PROTOS["pinn_error_string"] == ("const char*", ["int code"]) and PROTOS["pinn_abi_version"] == ("int", [])
    assert header_fields(HEADER_STRUCTS["pinn_adam_state"]) == [("m", "ptr"), ("v", "ptr"), ("lr", (C.c_double, ())), ("beta1", (C.c_double, ())),
                                                                ("beta2", (C.c_double, ())), ("eps", (C.c_double, ())), ("step", (C.c_int64, ()))]
    assert header_fields(HEADER_STRUCTS["pinn_stream_set"])[5] == ("weights", (C.c_float, (5, 8)))

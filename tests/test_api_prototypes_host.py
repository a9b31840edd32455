"""The Python mirror of the C ABI (example_gui_opencl_raytracer_amd/api.py) against the headers it mirrors (include/opencl_wrap.h,
include/hip_wrap_ext.h): every line of the prototype table against its header prototype, the four records that exist as a ctypes Structure and
as a numpy dtype, and the one rule for a symbol a library lacks.  No GPU: the library is loaded, nothing in it is called.

The comparison is by class, not by spelling.  A parameter is a pointer (anything with `*` or `[`; on the Python side c_void_p, c_char_p, a
POINTER or an array type), an int (int, cl_int), a u32 (uint32_t, cl_uint), a u64 (uint64_t, cl_mem_flags, cl_device_type, size_t: one class,
all 8 bytes here), a float or a double; a return is one of these, `void` (None) or `const char*` (c_char_p).  A variadic prototype is
compared by its return only."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from render_common import api, header_text  # noqa: F401  (api: the fixture)

HEADERS = ("opencl_wrap.h", "hip_wrap_ext.h")
C_CLASSES = {"int": "int", "cl_int": "int", "uint32_t": "u32", "cl_uint": "u32", "uint64_t": "u64", "cl_mem_flags": "u64", "cl_device_type": "u64",
             "size_t": "u64", "float": "float", "double": "double"}
PY_CLASSES = {C.c_int: "int", C.c_int32: "int", C.c_uint32: "u32", C.c_uint64: "u64", C.c_size_t: "u64", C.c_float: "float", C.c_double: "double",
              C.c_void_p: "pointer", C.c_char_p: "pointer"}


def c_class(decl, is_return=False):
    """the class of one parameter declaration (with or without its name) or of a return type"""
    decl = " ".join(decl.split())
    if is_return and decl.replace(" ", "") == "constchar*":
        return "str"
    if "*" in decl or "[" in decl:
        return "pointer"
    words = [w for w in decl.split() if w not in ("const", "struct")]
    if is_return:
        return "void" if words == ["void"] else C_CLASSES.get(" ".join(words), "?" + decl)
    return C_CLASSES.get(" ".join(words[:-1]), "?" + decl)          # the last word is the parameter's name


def py_class(t, is_return=False):
    if is_return and (t is None or t is C.c_char_p):
        return "void" if t is None else "str"
    if isinstance(t, type) and issubclass(t, (C._Pointer, C.Array)):
        return "pointer"
    return PY_CLASSES.get(t, "?%r" % (t,))


def header_prototypes():
    """name -> (return class, [parameter classes] or None for a variadic prototype) of every cl_wrap_* / clw_ext_* / clw_host_* prototype"""
    found = {}
    for h in HEADERS:
        code = header_text(h, comments=False)
        for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b((?:cl_wrap|clw_ext|clw_host)_\w+)\s*\(([^;{()]*)\)\s*;", code):
            params = [p.strip() for p in params.split(",")]
            assert name not in found, name
            if params[-1] == "...":
                found[name] = (c_class(ret, True), None)
            else:
                found[name] = (c_class(ret, True), [] if params == ["void"] else [c_class(p) for p in params])
    return found


def mismatches(protos, table):
    """the names of `table` (name -> (restype, argtypes)) that do not agree with their header prototype, each with what differs"""
    bad = {}
    for name, (restype, argtypes) in table.items():
        ret, params = protos[name]
        why = []
        if py_class(restype, True) != ret:
            why.append("returns %s, bound as %s" % (ret, py_class(restype, True)))
        if params is None:
            if argtypes is not None:
                why.append("variadic, bound with argument types")
        elif argtypes is None or len(argtypes) != len(params):
            why.append("%d parameters, bound with %s" % (len(params), "none" if argtypes is None else len(argtypes)))
        else:
            why += ["parameter %d is %s, bound as %s" % (k, want, py_class(t)) for k, (want, t) in enumerate(zip(params, argtypes)) if py_class(t) != want]
        if why:
            bad[name] = why
    return bad


def test_every_binding_agrees_with_its_header_prototype(api):
    protos = header_prototypes()
    assert len(protos) >= 115
    assert set(protos) == set(api.SYMBOLS) == set(api.PROTOTYPES) and isinstance(api.SYMBOLS, list) and len(api.SYMBOLS) == len(protos)
    unknown = {n: p for n, p in protos.items() if any(c.startswith("?") for c in [p[0]] + (p[1] or []))}
    assert not unknown, unknown                                     # the classifier knows every type the headers use
    L = api.load_library()
    bound = {name: (getattr(L, name).restype, getattr(L, name).argtypes) for name in api.SYMBOLS}
    assert mismatches(protos, bound) == {}
    assert mismatches(protos, api.PROTOTYPES) == {}
    assert [n for n, p in protos.items() if p[1] is None] == ["cl_wrap_init", "cl_wrap_load_images"]


def test_the_comparison_can_fail(api):
    """three planted errors -- a uint64_t bound as c_uint32, a dropped parameter, a void* return bound as c_int -- and nothing else"""
    table = {name: (restype, None if argtypes is None else list(argtypes)) for name, (restype, argtypes) in api.PROTOTYPES.items()}
    assert table["clw_host_projection_rays"][1][2] is C.c_uint64
    table["clw_host_projection_rays"][1][2] = C.c_uint32
    table["clw_ext_pick"][1].pop()
    assert table["clw_ext_device_ptr"][0] is C.c_void_p
    table["clw_ext_device_ptr"] = (C.c_int, table["clw_ext_device_ptr"][1])
    bad = mismatches(header_prototypes(), table)
    assert sorted(bad) == ["clw_ext_device_ptr", "clw_ext_pick", "clw_host_projection_rays"], bad
    assert bad["clw_host_projection_rays"] == ["parameter 2 is u64, bound as u32"]
    assert bad["clw_ext_pick"] == ["4 parameters, bound with 3"]
    assert bad["clw_ext_device_ptr"] == ["returns pointer, bound as int"]


F32, U32, U64 = np.float32, np.uint32, np.uint64
RECORDS = {
    "RAY_QUERY": ("clw_ray", 32, [("origin", F32, 3), ("tmax", F32), ("dir", F32, 3), ("ignore", U32)]),
    "HIT": ("clw_hit", 32, [("t", F32), ("id", U32), ("normal", F32, 3), ("point", F32, 3)]),
    "LAYER": ("clw_layer", 8, [("t", F32), ("id", U32)]),
    "OBJECT_STAT": ("clw_object_stat", 48, [("id", U32), ("pixels", U32), ("x0", U32), ("y0", U32), ("x1", U32), ("y1", U32),
                                            ("depth_min", F32), ("depth_max", F32), ("sum_x", U64), ("sum_y", U64)]),
}


@pytest.mark.parametrize("name", sorted(RECORDS))
def test_a_record_has_one_layout(api, name):
    struct, size, fields = RECORDS[name]
    struct, got, want = getattr(api, struct), getattr(api, name), np.dtype(fields)
    assert isinstance(got, np.dtype) and got == want and got.names == want.names
    assert got.itemsize == want.itemsize == C.sizeof(struct) == size
    for field in want.names:
        assert got.fields[field][0] == want.fields[field][0], field
        assert got.fields[field][1] == want.fields[field][1] == getattr(struct, field).offset, field
    made = np.zeros(5, want)                                        # an array of the hand-written dtype passes into the API as it is
    assert np.shares_memory(np.ascontiguousarray(made, got), made)


STUB = "void cl_wrap_release(void* w) { (void)w; }\nconst char* clw_ext_version(void) { return \"stub\"; }\nint not_in_the_table(void) { return 7; }\n"


def test_one_rule_for_a_symbol_the_library_lacks(api, tmp_path):
    (tmp_path / "stub.c").write_text(STUB)
    so = str(tmp_path / "libstub.so")
    subprocess.run(["gcc", "-shared", "-fPIC", "-o", so, str(tmp_path / "stub.c")], check=True)
    have = ["cl_wrap_release", "clw_ext_version"]
    lacks = [n for n in api.SYMBOLS if n not in have]
    assert len(lacks) == len(api.SYMBOLS) - 2 >= 113
    L = C.CDLL(so)
    assert api.bind_prototypes(L, may_be_missing=True) is L
    for name in have:
        restype, argtypes = api.PROTOTYPES[name]
        assert getattr(L, name).restype is restype and list(getattr(L, name).argtypes) == list(argtypes), name
    assert L.clw_ext_version() == b"stub"
    assert not [n for n in lacks if hasattr(L, n)]
    assert L.not_in_the_table.argtypes is None and L.not_in_the_table() == 7        # the binding touches the table's names only
    with pytest.raises(AttributeError) as e:
        api.bind_prototypes(C.CDLL(so), may_be_missing=False)
    assert lacks[0] in str(e.value)

"""include/flyhip.h as the tests read it: its prototypes, and the ctypes type each declared C type binds to.

The header is regular -- one `ret name(type name, ...);` per entry point, comments in /* */ only -- so this is a
few regular expressions, not a C parser.  Test infrastructure: the product's table (fly_bproject_amd/_lib.py SYMBOLS)
stays a Python table that imports without the header on disk."""
import ctypes as C
import os
import re

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "flyhip.h")

SCALARS = {"int": C.c_int, "int32_t": C.c_int, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "float": C.c_float,
           "FlyHandle": C.c_void_p}
RETURNS = {"int": C.c_int, "int64_t": C.c_int64, "const char*": C.c_char_p}
STRUCTS = ("FlyConfig", "FlyBuffers", "FlyRenderConfig", "FlyRandomization")        # bound as ctypes structures
HANDLE_ARRAYS = ("FlyHandle*", "void**", "void* const*", "float* const*")            # pointers to host arrays of pointers


def header_text():
    """The header without its comments."""
    return re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)


def prototypes():
    """{name: (return type, [parameter type, ...])} of every function the header declares, types as written with single
    spaces and the `*` attached to the type (`const float*`, `void* const*`); an array parameter `T name[64]` is `T[]`."""
    out = {}
    for ret, name, args in re.findall(r"^((?:const\s+)?\w+\s*\*?)\s*\b(\w+)\s*\(([^)]*)\)\s*;", header_text(), flags=re.M):
        params = []
        for a in ([] if args.strip() == "void" else args.split(",")):
            m = re.fullmatch(r"\s*(.*?)\s*\b\w+\s*(\[\w*\])?\s*", a, flags=re.S)     # type | parameter name | [n]
            assert m and m.group(1), (name, a)
            params.append(" ".join(m.group(1).split()).replace(" *", "*") + ("[]" if m.group(2) else ""))
        assert name not in out, name
        out[name] = (" ".join(ret.split()).replace(" *", "*"), params)
    return out


def ctype_of(param, structs):
    """The ctypes type a parameter of C type `param` is bound as; `structs` = {C structure name: its ctypes binding}."""
    if param in SCALARS:
        return SCALARS[param]
    if param in HANDLE_ARRAYS:
        return C.POINTER(C.c_void_p)
    bare = param.replace("const ", "").rstrip("*")
    if param.endswith("*") and bare in STRUCTS:
        return C.POINTER(structs[bare])
    assert param.endswith(("*", "[]")), "a by-value type the binding has no rule for: %r" % param
    return C.c_void_p

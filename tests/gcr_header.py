"""include/gcr.h as the tests read it: shared by tests/test_abi_cpu.py and tests/test_spmm_launch_cpu.py."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_prototypes():
    """{name: (return type, [parameter types], [parameter names])} of every prototype of include/gcr.h, the types as ctypes:
    any `*` is a pointer (c_void_p; `const char*` as a return type c_char_p), the fixed-width integers, float and double
    are their ctypes."""
    import ctypes
    scalars = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32,
               "uint64_t": ctypes.c_uint64, "float": ctypes.c_float, "double": ctypes.c_double}

    def ctype(decl, is_return=False):
        if "*" in decl:
            return ctypes.c_char_p if is_return and decl.replace(" ", "") == "constchar*" else ctypes.c_void_p
        return scalars[decl.replace("const", "").strip()]

    text = open(os.path.join(ROOT, "include", "gcr.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"^\s*#.*$", "", text, flags=re.M)
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w\s\*]*?)\b(gcr_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text):
        assert name not in protos, f"{name} is declared twice"
        params = [] if params.strip() in ("", "void") else [p.strip() for p in params.split(",")]
        split = [re.fullmatch(r"(.*?)(\w+)", p, flags=re.S) for p in params]
        protos[name] = (ctype(ret, True), [ctype(m.group(1)) for m in split], [m.group(2) for m in split])
    return protos

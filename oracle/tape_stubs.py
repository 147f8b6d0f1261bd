"""Recording stand-ins for the C ABI, written to stdout as C: one weak definition per function declared in include/uz_api.h that
prints its own name and every argument (integers and pointers as integers, floats exactly) and returns 0.  Linked with
csrc/tape.hip compiled for the host, they show which entry point run_one() takes for a tape op and which slot lands in which
argument (tests/test_tape_dispatch_cpu.py); tape.hip's own functions are strong definitions and win at link time."""
import ctypes as C
import importlib.util
import os
import sys
import types

# the binding alone, without importing the package (torch): a bare parent module whose path lets _ffi find its one sibling, _knobs
_PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "unet-zoo_amd")
sys.modules["_uz"] = types.ModuleType("_uz")
sys.modules["_uz"].__path__ = [_PKG]
_spec = importlib.util.spec_from_file_location("_uz._ffi", os.path.join(_PKG, "_ffi.py"))
_ffi = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_ffi)

# ctypes type of _ffi.prototypes() -> (C type, printf conversion, cast of the printed value)
_ARG = {C.c_int: ("int", "%lld", "(long long)"), C.c_size_t: ("size_t", "%llu", "(unsigned long long)"),
        C.c_int64: ("int64_t", "%lld", "(long long)"), C.c_uint8: ("uint8_t", "%lld", "(long long)"),
        C.c_float: ("float", "%a", "(double)"), C.c_void_p: ("const void*", "%llu", "(unsigned long long)(uintptr_t)"),
        C.c_char_p: ("const char*", "%llu", "(unsigned long long)(uintptr_t)")}
_RET = {None: "void", C.c_int: "int", C.c_size_t: "size_t", C.c_int64: "int64_t", C.c_float: "float", C.c_char_p: "const char*",
        C.c_void_p: "void*"}


def main():
    print("#include <stdint.h>\n#include <stddef.h>\n#include <stdio.h>")
    for name, (restype, argtypes) in sorted(_ffi.prototypes().items()):
        args = [_ARG[t] for t in argtypes]
        decl = ", ".join(f"{a[0]} a{k}" for k, a in enumerate(args)) or "void"
        fmt = " ".join([name] + [a[1] for a in args])
        vals = "".join(f", {a[2]}a{k}" for k, a in enumerate(args))
        ret = "" if restype is None else " return 0;"
        print(f'__attribute__((weak)) {_RET[restype]} {name}({decl}) {{ printf("{fmt}\\n"{vals});{ret} }}')


if __name__ == "__main__":
    main()

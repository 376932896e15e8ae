"""What the tests of the C-ABI share: the headers under include/ as text, the entries and structs they declare, the built
HIP library and an oracle-backed CApi."""
import ctypes
import functools
import os
import re
import subprocess

from tests.procs import ROOT
from trafficsimulation_amd import _capi as capi

CTYPE = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
         "uint8_t": ctypes.c_uint8}


@functools.lru_cache(maxsize=None)
def header(name):
    """include/<name> without its comments."""
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)


def declared(name):
    """{entry: number of parameters} of every ts_* function the header declares."""
    src = header(name)
    found = {fn: 0 if args.strip() in ("", "void") else args.count(",") + 1
             for fn, args in re.findall(r"\b(ts_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", src)}
    # nothing that looks like an entry escapes the declaration pattern (a parameter list with parentheses of its own would)
    assert set(found) == set(re.findall(r"\b(ts_[a-z_0-9]+)\s*\(", src))
    return found


def struct_fields(header_name, struct):
    """[(field, ctypes type)] of `typedef struct <struct> { ... } <struct>;`: fixed-width integers, arrays of them, and
    pointers to them (as c_void_p)."""
    body = re.search(rf"typedef struct {struct} \{{(.*?)\}} {struct};", header(header_name), flags=re.S).group(1)
    fields = []
    for typ, names in re.findall(r"^\s*(?:const\s+)?(u?int(?:8|32|64)_t\s*\*?)\s*([^;]+);", body, flags=re.M):
        for n in names.split(","):
            m = re.fullmatch(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*", n)
            t = ctypes.c_void_p if typ.endswith("*") else CTYPE[typ.strip()]
            fields.append((m.group(1), t * int(m.group(2)) if m.group(2) else t))
    return fields


def c_layout(header_name, structs, tmp_path):
    """[[sizeof, offsetof of every field]] of [(struct, [field names])], as a C compiler sees the header."""
    prog = ['#include <stdio.h>', '#include <stddef.h>', f'#include "{header_name}"', 'int main(void) {']
    for cname, fields in structs:
        prog.append(f'  printf("%zu\\n", sizeof({cname}));')
        prog += [f'  printf("%zu\\n", offsetof({cname}, {f}));' for f in fields]
    prog += ['  return 0;', '}']
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(prog))
    subprocess.run([os.environ.get("CC", "cc"), "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = iter(int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    return [[next(out) for _ in range(1 + len(fields))] for _, fields in structs]


@functools.lru_cache(maxsize=None)
def _lib_path():
    import __graft_entry__ as ge
    ge.build_hip()
    from trafficsimulation_amd._lib import LIB_PATH
    return LIB_PATH


def hip_lib():
    """libtrafficsim_hip.so, built on the first call; every call opens a CDLL of its own, so that the argtypes one test
    sets are not another test's."""
    return ctypes.CDLL(_lib_path())


def oracle_api():
    from oracle import pyoracle
    return capi.CApi(ctypes.CDLL(pyoracle.build()), "tso_")

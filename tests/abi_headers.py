"""The headers of the C ABI (``include/``, ``build.ABI_HEADERS``) as the tests read them: the comment stripper, the declared names, the prototypes, the one
rule that turns a prototype's argument into the binding's ctypes type, and the number of entry points every header is frozen at.  tests/test_abi_cpu.py holds
all seventeen headers to it; the per-family tests take ``names`` and ``declarations`` from here for what is specific to their header."""
import ctypes
import os
import re

from coalign_amd import build, hip

LAB_HEADER = build.ABI_HEADERS[-1]

# entry points per header: ABI version 2 only grows by new headers, so an existing header keeps its count
FROZEN = {"coalign_amd.h": 68, "coalign_amd_narrow.h": 2, "coalign_amd_narrow_sparse.h": 1, "coalign_amd_align.h": 4, "coalign_amd_stage1.h": 3, "coalign_amd_disco.h": 2,
          "coalign_amd_v2v.h": 3, "coalign_amd_v2x.h": 3, "coalign_amd_v2x_window.h": 3, "coalign_amd_w2c.h": 3, "coalign_amd_v2v_robust.h": 7,
          "coalign_amd_where2comm.h": 2, "coalign_amd_where2comm_msg.h": 3, "coalign_amd_v2x_ffn.h": 2, "coalign_amd_lss.h": 3, "coalign_amd_lss_bev.h": 3,
          "coalign_amd_lab.h": 3}

# The headers whose prototypes say which pointer is what (``ctype`` below reproduces their tables).  In the other four (coalign_amd.h, _narrow_sparse.h, _align.h, _lab.h) a
# ``const int32_t *`` can be a device buffer and a ``const double *`` / ``const int64_t *`` a host array: their own tests map those arguments one by one.
TYPED_BY_RULE = ("coalign_amd_narrow.h", "coalign_amd_stage1.h", "coalign_amd_disco.h", "coalign_amd_v2v.h", "coalign_amd_v2x.h", "coalign_amd_v2x_window.h",
                 "coalign_amd_w2c.h", "coalign_amd_v2v_robust.h", "coalign_amd_where2comm.h", "coalign_amd_where2comm_msg.h", "coalign_amd_v2x_ffn.h", "coalign_amd_lss.h",
                 "coalign_amd_lss_bev.h")

RETURNS = {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "int64_t": ctypes.c_int64, "const char *": ctypes.c_char_p}
SCALARS = {"int": ctypes.c_int, "float": ctypes.c_float, "double": ctypes.c_double, "size_t": ctypes.c_size_t, "int64_t": ctypes.c_int64, "uint32_t": ctypes.c_uint32}


def path(header):
    return os.path.join(build.INCLUDE, header)


def table(header):
    """The ``hip`` table that binds ``header``."""
    return hip.LAB_SIGNATURES if header == LAB_HEADER else hip.HEADERS[header]


def text(header):
    """The header without its comments."""
    return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", open(path(header)).read(), flags=re.S))


def names(header):
    return set(re.findall(r"\b(coalign_[a-z0-9_]+)\s*\(", text(header)))


def declarations(header):
    """name -> (the return type as ctypes, the arguments as whitespace-normalised C text) of every prototype; a lone ``void`` means no arguments."""
    out = {}
    for ret, name, args in re.findall(r"\b(int|size_t|int64_t|const char \*)\s*(coalign_[a-z0-9_]+)\s*\(([^)]*)\)\s*;", text(header)):
        args = [" ".join(a.split()) for a in args.split(",")]
        out[name] = (RETURNS[ret], [] if args == ["void"] else args)
    return out


def ctype(arg):
    """A prototype's argument -> the binding's type: host arrays of pointers (``* const *``) and host int32 arrays (``const int32_t *name``) as typed pointers, every
    other pointer (device buffers, the stream) as ``hip.P``, scalars as themselves."""
    if re.search(r"\*\s*const\s*\*", arg):
        return ctypes.POINTER(hip.P)
    if re.match(r"const int32_t \*\w+$", arg):
        return ctypes.POINTER(ctypes.c_int32)
    if "*" in arg:
        return hip.P
    return SCALARS[arg.split()[-2]]

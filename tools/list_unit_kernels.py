#!/usr/bin/env python3
"""List the kernel instantiations that libneuronika_hip.so holds for given translation units, by the names a kernel trace
summary (tools/rocpd_kernel_stats.py) prints: `reduce_cols4_kernel<0>`, `binary_fwd_kernel<2, true>`.

    python tools/list_unit_kernels.py                      # the streaming units of tests/dispatch_paths.py
    python tools/list_unit_kernels.py nk_gemm.hip

The library's `.hip_fatbin` section is a run of clang offload bundles, one per translation unit; each holds one gfx950 code
object (an ELF) whose symbol table names every kernel twice: `<sym>` (the code) and `<sym>.kd` (its descriptor).  A kernel is
attributed to a unit by its function name: the `__global__` functions that unit's source defines.  Only the demangler is run
as a program (`c++filt` or `llvm-cxxfilt` when one is on the PATH; without one, the plain names these units use are decoded
here); everything else is parsed here."""
import os
import re
import shutil
import struct
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neuronika_amd", "csrc")
LIB = os.path.join(ROOT, "neuronika_amd", "lib", "libneuronika_hip.so")
STREAMING_UNITS = ("nk_elementwise.hip", "nk_reduce.hip", "nk_layout.hip", "nk_loss.hip", "nk_gemv.hip")
_MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib_path=LIB, arch="gfx950"):
    """the device ELF images of `arch` inside the library, in link order"""
    blob = open(lib_path, "rb").read()
    out, at = [], blob.find(_MAGIC)
    while at >= 0:
        (n,) = struct.unpack_from("<Q", blob, at + len(_MAGIC))
        p = at + len(_MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if arch in triple and size:
                out.append(blob[at + off:at + off + size])
        at = blob.find(_MAGIC, at + len(_MAGIC))
    return out


def kernel_symbols(elf):
    """mangled names of the kernels of one code object: the symbols that have a `.kd` descriptor twin"""
    assert elf[:4] == b"\x7fELF" and elf[4] == 2, "not an ELF64 image"
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    names = set()
    for i in range(shnum):
        _, stype, _, _, off, size, link, _, _, entsize = struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize)
        if stype not in (2, 11):   # SHT_SYMTAB, SHT_DYNSYM
            continue
        _, _, _, _, stroff, strsize, _, _, _, _ = struct.unpack_from("<IIQQQQIIQQ", elf, shoff + link * shentsize)
        for s in range(size // entsize):
            (st_name,) = struct.unpack_from("<I", elf, off + s * entsize)
            end = elf.index(b"\0", stroff + st_name)
            names.add(elf[stroff + st_name:end].decode())
    return sorted(n for n in names if n + ".kd" in names)


def _demangle_plain(m):
    """the subset of the Itanium mangling the streaming kernels use - an optionally nested function name with integer and
    bool template arguments - for machines without a demangler program; None for anything else"""
    g = re.match(r"_Z(N?)((?:\d+[A-Za-z_]\w*?)+?)(?:I((?:L[ib]n?\d+E)+)E)?(?(1)E|)(?=[^\d])", m)
    if not g:
        return None
    ids, rest = [], g.group(2)
    while rest:
        n = re.match(r"\d+", rest)
        if not n or len(rest) < n.end() + int(n.group()):
            return None
        ids.append(rest[n.end():n.end() + int(n.group())])
        rest = rest[n.end() + int(n.group()):]
    name = "::".join("(anonymous namespace)" if i == "_GLOBAL__N_1" else i for i in ids)
    if g.group(3):
        args = [("true" if v == "1" else "false") if t == "b" else ("-" if neg else "") + v
                for t, neg, v in re.findall(r"L([ib])(n?)(\d+)E", g.group(3))]
        name += "<" + ", ".join(args) + ">"
    return name + "("


def demangle(names):
    exe = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if exe is None:
        return [_demangle_plain(n) or n for n in names]
    r = subprocess.run([exe], input="\n".join(names) + "\n", capture_output=True, text=True, check=True)
    out = r.stdout.split("\n")[:len(names)]
    assert len(out) == len(names)
    return out


def trace_name(demangled):
    """what tools/rocpd_kernel_stats.py prints for a kernel: no `void`, no anonymous namespace, no argument list"""
    s = demangled.replace("(anonymous namespace)::", "")
    s = re.sub(r"\(.*$", "", s)
    return re.sub(r"^void\s+", "", s).strip()


def source_kernels(unit):
    """names of the `__global__` functions a unit's source defines"""
    txt = open(os.path.join(CSRC, unit)).read()
    txt = re.sub(r"//[^\n]*", "", txt)
    return set(re.findall(r"__global__\s+(?:__launch_bounds__\s*\([^)]*\)\s*)?void\s+(\w+)\s*\(", txt))


def unit_kernels(units=STREAMING_UNITS, lib_path=LIB):
    """{unit: sorted trace names of its kernel instantiations in the built library}"""
    mangled = sorted({k for elf in code_objects(lib_path) for k in kernel_symbols(elf)})
    built = {}
    for m, d in zip(mangled, demangle(mangled)):
        t = trace_name(d)
        built.setdefault(re.sub(r"<.*$", "", t), set()).add(t)
    out = {}
    for u in units:
        out[u] = sorted(t for fn in source_kernels(u) for t in built.get(fn, ()))
    return out


if __name__ == "__main__":
    for unit, ks in unit_kernels(tuple(sys.argv[1:]) or STREAMING_UNITS).items():
        for k in ks:
            print(unit, k)

#!/usr/bin/env python3
"""List the kernel instantiations that libneuronika_hip.so holds for given translation units, by the names a kernel trace
summary (tools/rocpd_kernel_stats.py) prints: `reduce_cols4_kernel<0>`, `binary_fwd_kernel<2, true>`.

    python tools/list_unit_kernels.py                      # the streaming units of tests/dispatch_paths.py
    python tools/list_unit_kernels.py nk_gemm.hip nk_conv.hip nk_attention.hip
    python tools/list_unit_kernels.py --all                # every translation unit of the library

The library's `.hip_fatbin` section is a run of clang offload bundles, one per translation unit; each holds one gfx950 code
object (an ELF) whose symbol table names every kernel twice: `<sym>` (the code) and `<sym>.kd` (its descriptor).  A kernel
belongs to the unit whose code object holds it; a code object is matched to its unit by function names: the `__global__`
functions the unit's source defines, in the `.hip` file itself or in the `nk_*.h` headers it includes (nk_conv.hip defines no
kernel of its own).  Only the demangler is run as a program (`c++filt` or `llvm-cxxfilt` when one is on the PATH; without one,
the plain names these units use are decoded here); everything else is parsed here."""
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
    """the subset of the Itanium mangling this library's kernels use - a function name, nested in namespaces or not, with integer
    and bool template arguments (any number of them), whatever the parameter list - for machines without a demangler program;
    an `extern "C"` kernel is its own name; None for anything else (type template arguments)"""
    if not m.startswith("_Z"):
        return m + "(" if re.fullmatch(r"[A-Za-z_]\w*", m) else None
    at, nested = 2, m.startswith("_ZN")
    at += nested
    ids = []
    while True:
        n = re.match(r"\d+", m[at:])
        if not n:
            break
        size, at = int(n.group()), at + n.end()
        if size == 0 or len(m) < at + size:
            return None
        ids.append(m[at:at + size])
        at += size
        if not nested:
            break
    if not ids or not all(re.fullmatch(r"[A-Za-z_]\w*", i) for i in ids):
        return None
    name = "::".join("(anonymous namespace)" if i == "_GLOBAL__N_1" else i for i in ids)
    if m[at:at + 1] == "I":
        g = re.match(r"I((?:L[ib]n?\d+E)+)E", m[at:])
        if not g:
            return None
        args = [("true" if v == "1" else "false") if t == "b" else ("-" if neg else "") + v
                for t, neg, v in re.findall(r"L([ib])(n?)(\d+)E", g.group(1))]
        name += "<" + ", ".join(args) + ">"
        at += g.end()
    if nested and m[at:at + 1] != "E":
        return None
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


def file_kernels(path):
    """names of the `__global__` functions one file defines itself: `__global__`, then in any order `void`, `static`, `inline` and a
    `__launch_bounds__(...)` whose argument list may nest parentheses, then the name and its `(`"""
    txt = open(path).read()
    txt = re.sub(r"//[^\n]*", "", txt)
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    names = set()
    for g in re.finditer(r"\b__global__\b", txt):
        at = g.end()
        while True:
            t = re.compile(r"\s*(\w+)").match(txt, at)
            if not t:
                break
            word, at = t.group(1), t.end()
            if word == "__launch_bounds__":
                o = re.compile(r"\s*\(").match(txt, at)
                if not o:
                    break
                depth, at = 1, o.end()
                while depth and at < len(txt):
                    depth += {"(": 1, ")": -1}.get(txt[at], 0)
                    at += 1
            elif word not in ("void", "static", "inline"):
                if re.compile(r"\s*\(").match(txt, at):
                    names.add(word)
                break
    return names


def unit_sources(unit):
    """the unit's own file and every `nk_*.h` it includes, directly or through another header"""
    seen, todo = [], [unit]
    while todo:
        f = todo.pop()
        if f in seen or not os.path.exists(os.path.join(CSRC, f)):
            continue
        seen.append(f)
        todo += re.findall(r'^\s*#\s*include\s+"(nk_\w+\.h)"', open(os.path.join(CSRC, f)).read(), re.M)
    return seen


def source_kernels(unit):
    """names of the `__global__` functions a unit defines: its own and those of the headers it includes"""
    return set().union(*(file_kernels(os.path.join(CSRC, f)) for f in unit_sources(unit)))


def all_units():
    return tuple(sorted(f for f in os.listdir(CSRC) if f.endswith(".hip")))


def object_kernels(lib_path=LIB):
    """[sorted trace names of the kernel instantiations of one code object], one entry per translation unit of the library"""
    out = []
    for elf in code_objects(lib_path):
        mangled = kernel_symbols(elf)
        out.append(sorted({trace_name(d) for d in demangle(mangled)}))
    return out


def unit_kernels(units=STREAMING_UNITS, lib_path=LIB):
    """{unit: sorted trace names of its kernel instantiations in the built library}: the kernels of the code object(s) that hold
    a function the unit's sources define"""
    objs = object_kernels(lib_path)
    out = {}
    for u in units:
        fns = source_kernels(u)
        out[u] = sorted({k for ks in objs if any(re.sub(r"<.*$", "", k) in fns for k in ks) for k in ks})
    return out


if __name__ == "__main__":
    args = sys.argv[1:]
    for unit, ks in unit_kernels(all_units() if args == ["--all"] else tuple(args) or STREAMING_UNITS).items():
        for k in ks:
            print(unit, k)

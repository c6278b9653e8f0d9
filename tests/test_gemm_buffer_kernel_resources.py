"""What the compiler made of the four buffer-only GEMM kernels - the aligned 128 x 128, 256-thread instantiations
`sgemm_kernel<TA, TB, true, 2, 2, 1, EPX>` of NN (plain and EPX), NT (EPX) and TN - read from the code-object metadata of the built
libneuronika_hip.so (no GPU needed).  They hold ONE block program, the buffer-addressed one, so that its k-loops own the kernel's
register budget: a private segment (scratch) of 0 bytes each, inside the 256 registers of two waves per SIMD.  The library is a
product of build(); its absence is a failure."""
import os
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import list_unit_kernels as luk    # noqa: E402

BUFFER_ONLY = ("sgemm_kernel<false, false, true, 2, 2, 1, false>", "sgemm_kernel<false, false, true, 2, 2, 1, true>",
               "sgemm_kernel<false, true, true, 2, 2, 1, true>", "sgemm_kernel<true, false, true, 2, 2, 1, false>")
NT_AMDGPU_METADATA = 32


def unpack(b, at=0):
    """(value, next offset) of the MessagePack item at b[at]: the subset code-object metadata uses (maps, arrays, strings, ints, bools)"""
    t = b[at]
    if t <= 0x7F:
        return t, at + 1
    if t >= 0xE0:
        return t - 0x100, at + 1
    if 0x80 <= t <= 0x8F or t in (0xDE, 0xDF):
        n, at = (t & 15, at + 1) if t <= 0x8F else (int.from_bytes(b[at + 1:at + (3 if t == 0xDE else 5)], "big"), at + (3 if t == 0xDE else 5))
        out = {}
        for _ in range(n):
            k, at = unpack(b, at)
            out[k], at = unpack(b, at)
        return out, at
    if 0x90 <= t <= 0x9F or t in (0xDC, 0xDD):
        n, at = (t & 15, at + 1) if t <= 0x9F else (int.from_bytes(b[at + 1:at + (3 if t == 0xDC else 5)], "big"), at + (3 if t == 0xDC else 5))
        out = []
        for _ in range(n):
            v, at = unpack(b, at)
            out.append(v)
        return out, at
    if 0xA0 <= t <= 0xBF:
        return b[at + 1:at + 1 + (t & 31)].decode(), at + 1 + (t & 31)
    if t in (0xD9, 0xDA, 0xDB, 0xC4, 0xC5, 0xC6):
        w = {0xD9: 1, 0xDA: 2, 0xDB: 4, 0xC4: 1, 0xC5: 2, 0xC6: 4}[t]
        n = int.from_bytes(b[at + 1:at + 1 + w], "big")
        raw = b[at + 1 + w:at + 1 + w + n]
        return (raw.decode() if t >= 0xD9 else raw), at + 1 + w + n
    if t in (0xC0, 0xC2, 0xC3):
        return {0xC0: None, 0xC2: False, 0xC3: True}[t], at + 1
    if t in (0xCC, 0xCD, 0xCE, 0xCF):
        w = 1 << (t - 0xCC)
        return int.from_bytes(b[at + 1:at + 1 + w], "big"), at + 1 + w
    if t in (0xD0, 0xD1, 0xD2, 0xD3):
        w = 1 << (t - 0xD0)
        return int.from_bytes(b[at + 1:at + 1 + w], "big", signed=True), at + 1 + w
    if t in (0xCA, 0xCB):
        w = 4 if t == 0xCA else 8
        return struct.unpack(">f" if w == 4 else ">d", b[at + 1:at + 1 + w])[0], at + 1 + w
    raise AssertionError(f"MessagePack type 0x{t:02x} is not one code-object metadata uses")


def kernel_metadata(elf):
    """the `amdhsa.kernels` list of one code object: its NT_AMDGPU_METADATA note"""
    shoff, = struct.unpack_from("<Q", elf, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    for i in range(shnum):
        _, stype, _, _, off, size, _, _, _, _ = struct.unpack_from("<IIQQQQIIQQ", elf, shoff + i * shentsize)
        if stype != 7:   # SHT_NOTE
            continue
        at = off
        while at + 12 <= off + size:
            namesz, descsz, ntype = struct.unpack_from("<III", elf, at)
            name = elf[at + 12:at + 12 + namesz].rstrip(b"\0")
            desc = at + 12 + (namesz + 3) // 4 * 4
            if name == b"AMDGPU" and ntype == NT_AMDGPU_METADATA:
                return unpack(elf[desc:desc + descsz])[0]["amdhsa.kernels"]
            at = desc + (descsz + 3) // 4 * 4
    return []


def test_buffer_only_gemm_kernels_have_no_private_segment():
    assert os.path.exists(luk.LIB), f"{luk.LIB} is missing: run build() (python -m neuronika_amd.build)"
    found = {}
    for elf in luk.code_objects():
        kernels = kernel_metadata(elf)
        for k, name in zip(kernels, luk.demangle([k[".name"] for k in kernels])):
            if luk.trace_name(name) in BUFFER_ONLY:
                found[luk.trace_name(name)] = k
    assert sorted(found) == sorted(BUFFER_ONLY), f"not in the library's metadata: {sorted(set(BUFFER_ONLY) - set(found))}"
    for name, k in sorted(found.items()):
        print(name, "vgpr_count", k[".vgpr_count"], "private_segment_fixed_size", k[".private_segment_fixed_size"])
    for name, k in found.items():
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"], "bytes of scratch")
        assert 0 < k[".vgpr_count"] <= 256, (name, k[".vgpr_count"], "two waves per SIMD leave 256 registers per lane")

"""What the compiler made of the paged decode kernels, read from the code-object metadata of the built libneuronika_hip.so as
tests/test_gemm_buffer_kernel_resources.py reads it (no GPU needed).  The page lookup must not cost a register class: the one-head
forms stay at four waves per SIMD (at most 128 VGPRs; the contiguous twins have 108 - 119), the eight-head forms at two (at most
256; the twins have 170 - 176), and no new kernel has a private segment (scratch).  The library is a product of build(); its
absence is a failure."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import list_unit_kernels as luk    # noqa: E402
from test_gemm_buffer_kernel_resources import kernel_metadata    # noqa: E402

ONE_HEAD = tuple("%s<%d, 1>" % (k, dh) for k in ("adp_partial_kernel", "adpw_partial_kernel") for dh in (32, 64, 128))
EIGHT_HEADS = tuple("%s<%d, 8>" % (k, dh) for k in ("adp_partial_kernel", "adpw_partial_kernel") for dh in (32, 64, 128))
OTHERS = ("adp_generic_kernel", "adpw_generic_kernel", "kv_pages_append_kernel<float4>", "kv_pages_append_kernel<float>",
          "kv_pages_copy_kernel<float4>", "kv_pages_copy_kernel<float>")


def _short(name):
    """`adp_partial_kernel<128, 1>` of the demangled symbol, HIP's vector type spelled as the source spells it"""
    name = name.replace("HIP_vector_type<float, 4u>", "float4").replace("(anonymous namespace)::", "")
    head = name[:name.index("(")] if "(" in name else name
    return head.replace("void ", "").replace("float4 >", "float4>").strip()


def test_register_classes_and_zero_scratch():
    assert os.path.exists(luk.LIB), f"{luk.LIB} is missing: run build() (python -m neuronika_amd.build)"
    found = {}
    for elf in luk.code_objects():
        kernels = kernel_metadata(elf)
        for k, name in zip(kernels, luk.demangle([k[".name"] for k in kernels])):
            if _short(name) in ONE_HEAD + EIGHT_HEADS + OTHERS:
                found[_short(name)] = k
    want = ONE_HEAD + EIGHT_HEADS + OTHERS
    assert sorted(found) == sorted(want), f"not in the library's metadata: {sorted(set(want) - set(found))}"
    for name, k in sorted(found.items()):
        print(name, "vgpr_count", k[".vgpr_count"], "sgpr_count", k[".sgpr_count"], "private_segment_fixed_size", k[".private_segment_fixed_size"])
    for name, k in found.items():
        assert k[".private_segment_fixed_size"] == 0, (name, k[".private_segment_fixed_size"], "bytes of scratch")
    for name in ONE_HEAD:
        assert 0 < found[name][".vgpr_count"] <= 128, (name, found[name][".vgpr_count"], "four waves per SIMD leave 128 registers per lane")
    for name in EIGHT_HEADS:
        assert 0 < found[name][".vgpr_count"] <= 256, (name, found[name][".vgpr_count"], "two waves per SIMD leave 256 registers per lane")
    for name in OTHERS:
        assert 0 < found[name][".vgpr_count"] <= 128, (name, found[name][".vgpr_count"])

"""The surface of the quantised Linear's MFMA path without a GPU: header, exported symbol, ctypes layer."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_library_and_ctypes_layer_have_the_rule_and_the_knob():
    from neuronika_amd import capi
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neuronika_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+nk_quant_linear_mma_rule\s*\(\s*int bits\s*\)\s*;", src) and re.search(r"\bNK_TUNE_QUANT_MMA = 10\b", src)
    assert "nk_quant_linear_mma_rule" in capi.EXPORTED and hasattr(capi.lib, "nk_quant_linear_mma_rule")
    assert capi.TUNE_QUANT_MMA == 10 and hasattr(capi.Device, "quant_mma")
    assert capi.quant_linear_mma_rule(3) == 0 and capi.quant_linear_mma_rule(8) >= 0 and capi.quant_linear_mma_rule(4) >= 0

"""The surface of AdamW and gradient clipping, layer by layer, without a GPU: the header declares the entry points, the ctypes
table and the built library have them, the host classes take the documented keywords, the kernels live in their own header
outside the inventoried units, and the Rust mirror names the ffi calls."""
import inspect
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("nk_adamw_step_multi", "nk_adamw_step", "nk_clip_grad_norm_multi")
HIP = os.path.join(ROOT, "integration", "neuronika-variable", "src", "hip")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_header_declares_the_entry_points():
    src = re.sub(r"/\*.*?\*/", "", _read("include", "neuronika_hip.h"), flags=re.S)
    flat = re.sub(r"\s+", " ", src)
    assert ("int nk_adamw_step_multi(nk_device* dev, int count, float* const* w, const float* const* grad, float* const* exp_avg, "
            "float* const* exp_avg_sq, float* const* max_exp_avg_sq, const size_t* n, const int* step, float lr, float beta1, "
            "float beta2, float eps, float weight_decay);") in flat
    assert "int nk_clip_grad_norm_multi(nk_device* dev, int count, float* const* grad, const size_t* n, float max_norm, float* out);" in flat
    assert re.search(r"int nk_adamw_step\(nk_device\* dev, float\* w, const float\* grad,[^;]*int step, float weight_decay\);", flat)
    doc = _read("include", "neuronika_hip.h")
    for phrase in ("1 - lr * weight_decay", "coef", "CAN be captured", "NaN", "Refuses capture"):
        assert phrase in doc, phrase


def test_ctypes_table_and_library_export_them():
    from neuronika_amd import capi
    for name in ENTRIES:
        assert name in capi.EXPORTED and hasattr(capi.lib, name), name
    assert len(capi._SIGS["nk_adamw_step_multi"]) == 14 and len(capi._SIGS["nk_adamw_step"]) == 13
    assert len(capi._SIGS["nk_clip_grad_norm_multi"]) == 6
    for wrapper, keys in (("adamw_step", ("lr", "beta1", "beta2", "eps", "step", "weight_decay")),
                          ("adamw_step_multi", ("steps", "lr", "beta1", "beta2", "eps", "weight_decay")),
                          ("clip_grad_norm_multi", ("grads", "max_norm", "out"))):
        params = inspect.signature(getattr(capi, wrapper)).parameters
        assert all(k in params for k in keys), (wrapper, list(params))


def test_host_classes_take_the_documented_keywords():
    import neuronika_amd
    optim = neuronika_amd.tape.optim
    opt = optim.AdamW(lr=0.01, beta1=0.8, beta2=0.9, eps=1e-3, weight_decay=0.05, amsgrad=True)
    assert isinstance(opt, optim.Optimizer) and abs(opt.get_lr() - 0.01) < 1e-9
    assert isinstance(optim.AdamW(0.01), optim.Optimizer)                # everything but the rate has a default
    doc = optim.AdamW.__init__.__doc__
    for key in ("lr", "beta1", "beta2", "eps", "weight_decay", "amsgrad"):
        assert re.search(rf"\b{key}:", doc), (key, doc)
    assert "l1" not in doc and "l2" not in doc                           # no Penalty: the decay is decoupled
    assert re.search(r"clip_grad_norm\(params: .*, max_norm: ", optim.clip_grad_norm.__doc__)
    assert re.search(r"clip_grad_norm\(self: .*, max_norm: ", optim.Optimizer.clip_grad_norm.__doc__)
    for cls in (optim.SGD, optim.Adam, optim.Adagrad, optim.RMSProp, optim.AdamW):
        assert hasattr(cls, "clip_grad_norm")                            # works with every optimizer
    hpp = _read("host", "neuronika.hpp")
    # the comment over the declaration says where clipping goes in a data-parallel step
    assert "GradientSync::join()" in hpp[:hpp.index("Var clip_grad_norm(const std::vector<VarDiff>& params")][-1200:]


def test_kernels_live_in_their_own_header_outside_the_inventoried_units():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import dispatch_paths
    import dispatch_paths_mfma
    import list_unit_kernels as luk
    header = os.path.join(luk.CSRC, "nk_optim_multi.h")
    mine = luk.file_kernels(header)
    assert {"adamw_multi_kernel", "grad_sumsq_multi_kernel", "grad_scale_multi_kernel"} <= mine
    includers = [u for u in luk.all_units() if "nk_optim_multi.h" in luk.unit_sources(u)]
    assert len(includers) == 1 and includers[0] in [u for u, _ in dispatch_paths_mfma.NOT_INVENTORIED]
    for u in dispatch_paths.UNITS + dispatch_paths_mfma.UNITS:
        assert not (mine & luk.source_kernels(u)), u
    src = re.sub(r"//[^\n]*", "", open(header).read())
    assert "atomic" not in src.lower()                                   # the norm is summed in a fixed order
    m = re.search(r"constexpr int OPT_MULTI_MAX = (\d+);", src)
    assert m and int(m.group(1)) >= 32


def test_rust_mirror_names_the_ffi_calls():
    ffi = open(os.path.join(HIP, "ffi.rs")).read()
    for name in ENTRIES:
        assert re.search(rf"pub fn {name}\(", ffi), name
    node = open(os.path.join(HIP, "node", "optim.rs")).read()
    body = node[node.index("fn adamw_step_multi"):]
    assert "ffi::nk_adamw_step_multi(" in body
    assert "ffi::nk_clip_grad_norm_multi(" in node[node.index("fn clip_grad_norm_multi"):]
    opt = open(os.path.join(HIP, "optimizer.rs")).read()
    assert "pub struct AdamW" in opt and "adamw_step_multi(" in opt[opt.index("impl AdamW"):]
    assert opt.count("pub fn clip_grad_norm(") == 2 and "clip_grad_norm_multi(" in opt
    assert "optimizer::AdamW" in open(os.path.join(HIP, "mod.rs")).read()

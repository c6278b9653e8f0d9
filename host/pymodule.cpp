// pybind11 glue exposing the C++ tape mirror (host/neuronika.hpp) to the Python test / bench
// harness as `neuronika_amd._tape`.  Harness plumbing only: the drop-in boundary is the C ABI.
#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/functional.h>
#include <pybind11/stl.h>

#include "neuronika.hpp"
#include "data.hpp"

namespace py = pybind11;
using namespace neuronika;

using Arr = py::array_t<float, py::array::c_style | py::array::forcecast>;

struct Status {
    std::shared_ptr<bool> flag;
};

static Shape shape_of(const Arr& a) {
    Shape s;
    for (py::ssize_t i = 0; i < a.ndim(); ++i) s.push_back((int)a.shape(i));
    return s;
}
static py::array_t<float> to_numpy(const HipArray& h) {
    std::vector<py::ssize_t> s(h.shape().begin(), h.shape().end());
    py::array_t<float> out(s);
    h.download(out.mutable_data());
    return out;
}

PYBIND11_MODULE(_tape, m) {
    m.doc() = "C++ mirror of neuronika's Var/VarDiff tape on the HIP backend";
    py::register_exception<Panic>(m, "Panic", PyExc_RuntimeError);

    py::class_<Graph, std::shared_ptr<Graph>>(m, "Graph").def("launch", &Graph::launch);
    py::class_<Device, std::shared_ptr<Device>>(m, "Device")
        .def(py::init(&Device::create), py::arg("idx") = 0)
        .def("sync", &Device::sync)
        .def("bytes_in_use", &Device::bytes_in_use)
        .def("graph_begin", &Device::graph_begin)
        .def("graph_end", &Device::graph_end)
        .def_property_readonly("index", &Device::index)
        .def("raw", [](const Device& d) { return (uintptr_t)d.raw(); });

    py::enum_<Reduction>(m, "Reduction").value("Sum", Reduction::Sum).value("Mean", Reduction::Mean);
    py::enum_<Activation>(m, "Activation")
        .value("Gelu", Activation::Gelu).value("GeluTanh", Activation::GeluTanh).value("Silu", Activation::Silu).value("Sigmoid", Activation::Sigmoid);

    py::class_<Status>(m, "Status")  // `Rc<Cell<bool>>` train/eval switch of the Dropout nodes
        .def(py::init([](bool v) { return Status{std::make_shared<bool>(v)}; }), py::arg("train") = true)
        .def("set", [](Status& s, bool v) { *s.flag = v; })
        .def("get", [](const Status& s) { return *s.flag; });

    py::class_<Var>(m, "Var")
        .def_property_readonly("shape", [](const Var& v) { return v.shape(); })
        .def("requires_grad", &Var::requires_grad)
        .def("forward", &Var::forward)
        .def("item", &Var::item)
        .def("data", [](const Var& v) { return to_numpy(*v.data); })
        .def("set_data", [](const Var& v, const Arr& a) {
            if ((size_t)a.size() != v.data->len()) panic("set_data: size mismatch");
            v.data->upload(a.data());
        })
        .def("history_len", [](const Var& v) { return v.history.len(); })
        .def("sum", &Var::sum).def("mean", &Var::mean).def("relu", &Var::relu)
        .def("__neg__", &Var::neg).def("pow", &Var::pow).def("sqrt", &Var::sqrt).def("leaky_relu", &Var::leaky_relu)
        .def("gelu", &Var::gelu, py::arg("tanh_approx") = false).def("silu", &Var::silu).def("glu", &Var::glu, py::arg("gate") = Activation::Sigmoid)
        .def("softplus", &Var::softplus).def("sigmoid", &Var::sigmoid).def("tanh", &Var::tanh).def("ln", &Var::ln)
        .def("exp", &Var::exp).def("unsqueeze", &Var::unsqueeze)
        .def("max_pool", &Var::max_pool, py::arg("kernel"), py::arg("stride") = std::vector<int>{}, py::arg("padding") = std::vector<int>{})
        .def("avg_pool", &Var::avg_pool, py::arg("kernel"), py::arg("stride") = std::vector<int>{}, py::arg("padding") = std::vector<int>{}, py::arg("count_include_pad") = true)
        .def("upsample", &Var::upsample, py::arg("out_size"), py::arg("mode") = "nearest", py::arg("align_corners") = false)
        .def("global_avg_pool", &Var::global_avg_pool).def("flatten", &Var::flatten)
        .def("softmax", &Var::softmax).def("log_softmax", &Var::log_softmax).def("t", &Var::t)
        .def("layer_norm", py::overload_cast<const Var&, const Var&, double>(&Var::layer_norm, py::const_), py::arg("gamma"), py::arg("beta"), py::arg("eps") = 1e-5)
        .def("layer_norm", py::overload_cast<const VarDiff&, const VarDiff&, double>(&Var::layer_norm, py::const_), py::arg("gamma"), py::arg("beta"), py::arg("eps") = 1e-5)
        .def("layer_norm", py::overload_cast<const Shape&, double>(&Var::layer_norm, py::const_), py::arg("normalized_shape"), py::arg("eps") = 1e-5)
        .def("rms_norm", py::overload_cast<const Var&, double>(&Var::rms_norm, py::const_), py::arg("gamma"), py::arg("eps") = 1e-6)
        .def("rms_norm", py::overload_cast<const VarDiff&, double>(&Var::rms_norm, py::const_), py::arg("gamma"), py::arg("eps") = 1e-6)
        .def("rms_norm", py::overload_cast<const Shape&, double>(&Var::rms_norm, py::const_), py::arg("normalized_shape"), py::arg("eps") = 1e-6)
        .def("group_norm", py::overload_cast<int, const Var&, const Var&, double>(&Var::group_norm, py::const_), py::arg("num_groups"), py::arg("gamma"), py::arg("beta"), py::arg("eps") = 1e-5)
        .def("group_norm", py::overload_cast<int, const VarDiff&, const VarDiff&, double>(&Var::group_norm, py::const_), py::arg("num_groups"), py::arg("gamma"), py::arg("beta"), py::arg("eps") = 1e-5)
        .def("group_norm", py::overload_cast<int, double>(&Var::group_norm, py::const_), py::arg("num_groups"), py::arg("eps") = 1e-5)
        // gamma / beta: VarDiff (differentiable result), Var, or None; running_mean / running_var: Var or None
        .def("batch_norm", [](const Var& x, const VarDiff& gamma, const VarDiff& beta, const Var* rm, const Var* rv, double momentum, double eps,
                              const Status& s) { return x.batch_norm(gamma, beta, rm, rv, momentum, eps, s.flag); },
             py::arg("gamma"), py::arg("beta"), py::arg("running_mean").none(true), py::arg("running_var").none(true), py::arg("momentum"), py::arg("eps"),
             py::arg("status"))
        .def("batch_norm", [](const Var& x, const Var* gamma, const Var* beta, const Var* rm, const Var* rv, double momentum, double eps,
                              const Status& s) { return x.batch_norm(gamma, beta, rm, rv, momentum, eps, s.flag); },
             py::arg("gamma").none(true), py::arg("beta").none(true), py::arg("running_mean").none(true), py::arg("running_var").none(true),
             py::arg("momentum"), py::arg("eps"), py::arg("status"))
        .def("dropout", [](const Var& v, double p, const Status& s) { return v.dropout(p, s.flag); }).def("chunks", &Var::chunks).def("cat", &Var::cat)
        .def("mse", &Var::mse).def("mae", &Var::mae).def("bce", &Var::bce).def("bce_with_logits", &Var::bce_with_logits)
        .def("kldiv", &Var::kldiv).def("nll", &Var::nll).def("stack", &Var::stack)
        .def("cross_entropy", &Var::cross_entropy, py::arg("target"), py::arg("reduction"), py::arg("ignore_index") = -1, py::arg("label_smoothing") = 0.0)
        .def("mv", py::overload_cast<const Var&>(&Var::mv, py::const_)).def("mv", py::overload_cast<const VarDiff&>(&Var::mv, py::const_))
        .def("vm", py::overload_cast<const Var&>(&Var::vm, py::const_)).def("vm", py::overload_cast<const VarDiff&>(&Var::vm, py::const_))
        .def("vv", py::overload_cast<const Var&>(&Var::vv, py::const_)).def("vv", py::overload_cast<const VarDiff&>(&Var::vv, py::const_)).def("pad", py::overload_cast<const std::vector<int>&, float>(&Var::pad, py::const_), py::arg("padding"), py::arg("value") = 0.f)
        .def("pad", py::overload_cast<const std::vector<int>&, PaddingMode>(&Var::pad, py::const_))
        .def("mm", py::overload_cast<const Var&>(&Var::mm, py::const_))
        .def("mm", py::overload_cast<const VarDiff&>(&Var::mm, py::const_))
        .def("mm_t", py::overload_cast<const Var&>(&Var::mm_t, py::const_))
        .def("mm_t", py::overload_cast<const VarDiff&>(&Var::mm_t, py::const_))
        .def("heads_attention", [](const Var& q, const Var& k, const Var& v, int B, int S, int H, int dh, float scale, double p, const Status& s,
                                   bool causal, int window) { return q.heads_attention(k, v, B, S, H, dh, scale, p, s.flag, causal, window); },
             py::arg("keys"), py::arg("values"), py::arg("B"), py::arg("S"), py::arg("H"), py::arg("dh"), py::arg("scale"), py::arg("p"),
             py::arg("status"), py::arg("causal") = false, py::arg("window") = 0)
        .def_static("attention_core_supported", &Var::attention_core_supported)
        .def("convolution", &Var::convolution)
        .def("__add__", [](const Var& a, const Var& b) { return a + b; })
        .def("__add__", [](const Var& a, const VarDiff& b) { return a + b; })
        .def("__add__", [](const Var& a, float b) { return a + b; })
        .def("__sub__", [](const Var& a, const Var& b) { return a - b; })
        .def("__sub__", [](const Var& a, const VarDiff& b) { return a - b; })
        .def("__sub__", [](const Var& a, float b) { return a - b; })
        .def("__mul__", [](const Var& a, const Var& b) { return a * b; })
        .def("__mul__", [](const Var& a, const VarDiff& b) { return a * b; })
        .def("__mul__", [](const Var& a, float b) { return a * b; })
        .def("__truediv__", [](const Var& a, const Var& b) { return a / b; })
        .def("__truediv__", [](const Var& a, const VarDiff& b) { return a / b; })
        .def("__truediv__", [](const Var& a, float b) { return a / b; });

    py::class_<VarDiff>(m, "VarDiff")
        .def_property_readonly("shape", [](const VarDiff& v) { return v.shape(); })
        .def("forward", &VarDiff::forward)
        .def("backward", [](const VarDiff& v, float seed) { v.backward(seed); }, py::arg("seed") = 1.f)
        .def("backward_from", [](const VarDiff& v, const Var& seed) { v.backward_from(seed); }, py::arg("seed"))
        .def("backward_sync", [](const VarDiff& v, float seed, dp::GradientSync& s) { v.backward(seed, &s); })
        .def("zero_grad", &VarDiff::zero_grad)
        .def("no_grad", &VarDiff::no_grad)
        .def("with_grad", &VarDiff::with_grad)
        .def("item", &VarDiff::item)
        .def("data", [](const VarDiff& v) { return to_numpy(*v.var.data); })
        .def("set_data", [](const VarDiff& v, const Arr& a) {
            if ((size_t)a.size() != v.var.data->len()) panic("set_data: size mismatch");
            v.var.data->upload(a.data());
        })
        .def("grad", [](const VarDiff& v) { return to_numpy(v.grad->borrow()); })
        .def("set_grad", [](const VarDiff& v, const Arr& a) {
            if ((size_t)a.size() != v.grad->borrow().len()) panic("set_grad: size mismatch");
            v.grad->borrow().upload(a.data());
        })
        .def("history_len", [](const VarDiff& v) { return v.history.len(); })
        .def("forward_history_len", [](const VarDiff& v) { return v.var.history.len(); })
        .def("sum", &VarDiff::sum).def("mean", &VarDiff::mean)
        // Python has no rvalues: a receiver nobody else references (`lin.forward(x).relu()`: the only reference is the call's own)
        // is the temporary Rust's `relu(self)` consumes; a named variable stays observable and gets the plain ReLU node
        .def("relu", [](py::handle self) {
            VarDiff& v = self.cast<VarDiff&>();
            return Py_REFCNT(self.ptr()) <= 1 ? std::move(v).relu() : v.relu();
        })
        .def("__neg__", &VarDiff::neg).def("pow", &VarDiff::pow).def("sqrt", &VarDiff::sqrt).def("leaky_relu", &VarDiff::leaky_relu)
        .def("gelu", &VarDiff::gelu, py::arg("tanh_approx") = false).def("silu", &VarDiff::silu).def("glu", &VarDiff::glu, py::arg("gate") = Activation::Sigmoid)
        .def("softplus", &VarDiff::softplus).def("sigmoid", &VarDiff::sigmoid).def("tanh", &VarDiff::tanh).def("ln", &VarDiff::ln)
        .def("exp", &VarDiff::exp).def("unsqueeze", &VarDiff::unsqueeze)
        .def("max_pool", &VarDiff::max_pool, py::arg("kernel"), py::arg("stride") = std::vector<int>{}, py::arg("padding") = std::vector<int>{})
        .def("avg_pool", &VarDiff::avg_pool, py::arg("kernel"), py::arg("stride") = std::vector<int>{}, py::arg("padding") = std::vector<int>{}, py::arg("count_include_pad") = true)
        .def("upsample", &VarDiff::upsample, py::arg("out_size"), py::arg("mode") = "nearest", py::arg("align_corners") = false)
        .def("global_avg_pool", &VarDiff::global_avg_pool).def("flatten", &VarDiff::flatten)
        .def("softmax", &VarDiff::softmax).def("log_softmax", &VarDiff::log_softmax).def("t", &VarDiff::t)
        .def("layer_norm", py::overload_cast<const VarDiff&, const VarDiff&, double>(&VarDiff::layer_norm, py::const_), py::arg("gamma"), py::arg("beta"), py::arg("eps") = 1e-5)
        .def("layer_norm", py::overload_cast<const Var&, const Var&, double>(&VarDiff::layer_norm, py::const_), py::arg("gamma"), py::arg("beta"), py::arg("eps") = 1e-5)
        .def("layer_norm", py::overload_cast<const Shape&, double>(&VarDiff::layer_norm, py::const_), py::arg("normalized_shape"), py::arg("eps") = 1e-5)
        .def("rms_norm", py::overload_cast<const VarDiff&, double>(&VarDiff::rms_norm, py::const_), py::arg("gamma"), py::arg("eps") = 1e-6)
        .def("rms_norm", py::overload_cast<const Var&, double>(&VarDiff::rms_norm, py::const_), py::arg("gamma"), py::arg("eps") = 1e-6)
        .def("rms_norm", py::overload_cast<const Shape&, double>(&VarDiff::rms_norm, py::const_), py::arg("normalized_shape"), py::arg("eps") = 1e-6)
        .def("group_norm", py::overload_cast<int, const VarDiff&, const VarDiff&, double>(&VarDiff::group_norm, py::const_), py::arg("num_groups"), py::arg("gamma"), py::arg("beta"), py::arg("eps") = 1e-5)
        .def("group_norm", py::overload_cast<int, const Var&, const Var&, double>(&VarDiff::group_norm, py::const_), py::arg("num_groups"), py::arg("gamma"), py::arg("beta"), py::arg("eps") = 1e-5)
        .def("group_norm", py::overload_cast<int, double>(&VarDiff::group_norm, py::const_), py::arg("num_groups"), py::arg("eps") = 1e-5)
        .def("embedding", &VarDiff::embedding, py::arg("indices"), py::arg("padding_idx") = -1)
        .def("batch_norm", [](const VarDiff& x, const VarDiff& gamma, const VarDiff& beta, const Var* rm, const Var* rv, double momentum, double eps,
                              const Status& s) { return x.batch_norm(gamma, beta, rm, rv, momentum, eps, s.flag); },
             py::arg("gamma"), py::arg("beta"), py::arg("running_mean").none(true), py::arg("running_var").none(true), py::arg("momentum"), py::arg("eps"),
             py::arg("status"))
        .def("batch_norm", [](const VarDiff& x, const Var* gamma, const Var* beta, const Var* rm, const Var* rv, double momentum, double eps,
                              const Status& s) { return x.batch_norm(gamma, beta, rm, rv, momentum, eps, s.flag); },
             py::arg("gamma").none(true), py::arg("beta").none(true), py::arg("running_mean").none(true), py::arg("running_var").none(true),
             py::arg("momentum"), py::arg("eps"), py::arg("status"))
        .def("dropout", [](const VarDiff& v, double p, const Status& s) { return v.dropout(p, s.flag); }).def("chunks", &VarDiff::chunks).def("cat", &VarDiff::cat)
        .def("mse", &VarDiff::mse).def("mae", &VarDiff::mae).def("bce", &VarDiff::bce).def("bce_with_logits", &VarDiff::bce_with_logits)
        .def("kldiv", &VarDiff::kldiv).def("nll", &VarDiff::nll).def("stack", &VarDiff::stack)
        .def("cross_entropy", &VarDiff::cross_entropy, py::arg("target"), py::arg("reduction"), py::arg("ignore_index") = -1, py::arg("label_smoothing") = 0.0)
        .def("mv", py::overload_cast<const Var&>(&VarDiff::mv, py::const_)).def("mv", py::overload_cast<const VarDiff&>(&VarDiff::mv, py::const_))
        .def("vm", py::overload_cast<const Var&>(&VarDiff::vm, py::const_)).def("vm", py::overload_cast<const VarDiff&>(&VarDiff::vm, py::const_))
        .def("vv", py::overload_cast<const Var&>(&VarDiff::vv, py::const_)).def("vv", py::overload_cast<const VarDiff&>(&VarDiff::vv, py::const_)).def("pad", py::overload_cast<const std::vector<int>&, float>(&VarDiff::pad, py::const_), py::arg("padding"), py::arg("value") = 0.f)
        .def("pad", py::overload_cast<const std::vector<int>&, PaddingMode>(&VarDiff::pad, py::const_))
        .def("mm", py::overload_cast<const Var&>(&VarDiff::mm, py::const_))
        .def("mm", py::overload_cast<const VarDiff&>(&VarDiff::mm, py::const_))
        .def("mm_t", py::overload_cast<const Var&>(&VarDiff::mm_t, py::const_))
        .def("mm_t", py::overload_cast<const VarDiff&>(&VarDiff::mm_t, py::const_))
        .def("heads_attention", [](const VarDiff& q, const VarDiff& k, const VarDiff& v, int B, int S, int H, int dh, float scale, double p,
                                   const Status& s, bool causal, int window) { return q.heads_attention(k, v, B, S, H, dh, scale, p, s.flag, causal, window); },
             py::arg("keys"), py::arg("values"), py::arg("B"), py::arg("S"), py::arg("H"), py::arg("dh"), py::arg("scale"), py::arg("p"),
             py::arg("status"), py::arg("causal") = false, py::arg("window") = 0)
        .def("convolution", py::overload_cast<const Var&, const std::vector<int>&, const std::vector<int>&, int>(&VarDiff::convolution, py::const_))
        .def("convolution", py::overload_cast<const VarDiff&, const std::vector<int>&, const std::vector<int>&, int>(&VarDiff::convolution, py::const_))
        .def("__add__", [](const VarDiff& a, const Var& b) { return a + b; })
        .def("__add__", [](const VarDiff& a, const VarDiff& b) { return a + b; })
        .def("__add__", [](const VarDiff& a, float b) { return a + b; })
        .def("__sub__", [](const VarDiff& a, const Var& b) { return a - b; })
        .def("__sub__", [](const VarDiff& a, const VarDiff& b) { return a - b; })
        .def("__sub__", [](const VarDiff& a, float b) { return a - b; })
        .def("__mul__", [](const VarDiff& a, const Var& b) { return a * b; })
        .def("__mul__", [](const VarDiff& a, const VarDiff& b) { return a * b; })
        .def("__mul__", [](const VarDiff& a, float b) { return a * b; })
        .def("__truediv__", [](const VarDiff& a, const Var& b) { return a / b; })
        .def("__truediv__", [](const VarDiff& a, const VarDiff& b) { return a / b; })
        .def("__truediv__", [](const VarDiff& a, float b) { return a / b; });

    m.def("from_ndarray", [](DevicePtr dev, const Arr& a) { return from_host(std::move(dev), shape_of(a), a.data()); });
    m.def("zeros", &zeros);
    m.def("ones", &ones);
    m.def("full", &full);
    m.def("rand", &neuronika::rand);
    m.def("manual_seed", &neuronika::manual_seed, py::arg("seed"));
    m.def("eye", &eye); m.def("linspace", &linspace); m.def("logspace", &logspace); m.def("geomspace", &geomspace);
    m.def("range", &neuronika::range);

    {   // neuronika-data mirror + device input pipeline
        namespace nd = neuronika::data;
        py::module_ dm = m.def_submodule("data");
        auto to_np = [](const nd::HostArray& a) {
            std::vector<py::ssize_t> shape(a.shape().begin(), a.shape().end());
            Arr out(shape);
            if (a.len()) std::memcpy(out.mutable_data(), a.ptr(), a.len() * sizeof(float));
            return out;
        };
        auto from_np = [](const Arr& a) { return nd::HostArray(shape_of(a), a.data()); };
        dm.def("batch_ranges", [](size_t len, size_t size, bool drop_last) {
            std::vector<std::pair<size_t, size_t>> out;
            for (const auto& r : nd::batch_ranges(len, size, drop_last)) out.emplace_back(r.start, r.rows);
            return out;
        });
        dm.def("kfold_ids", [](size_t len, size_t k) {
            std::vector<std::pair<std::vector<size_t>, std::vector<size_t>>> out;
            for (const auto& f : nd::kfold_ids(len, k)) out.emplace_back(f.train_ids, f.test_ids);
            return out;
        });
        dm.def("shuffle_permutation", &nd::shuffle_permutation);
        py::class_<nd::Dataset>(dm, "Dataset")
            .def(py::init([from_np](const Arr& a) { return new nd::Dataset(from_np(a)); }))
            .def("records", [to_np](const nd::Dataset& d) { return to_np(d.records()); })
            .def("pinned", [](const nd::Dataset& d) { return d.records().pinned(); })
            .def("__len__", &nd::Dataset::len).def("is_empty", &nd::Dataset::is_empty)
            .def("kfold", &nd::Dataset::kfold)
            .def("batch", [to_np](const nd::Dataset& d, size_t n, bool drop_last) {
                std::vector<Arr> out;
                for (const auto& b : d.batch(n, drop_last)) out.push_back(to_np(b));
                return out;
            }, py::arg("size"), py::arg("drop_last") = false)
            .def("split", &nd::Dataset::split)
            .def("shuffle_with_seed", [](nd::Dataset& d, uint64_t seed) { d.shuffle_with_seed(seed); });
        py::class_<nd::LabeledDataset>(dm, "LabeledDataset")
            .def(py::init([from_np](const Arr& r, const Arr& l) { return new nd::LabeledDataset(from_np(r), from_np(l)); }))
            .def("records", [to_np](const nd::LabeledDataset& d) { return to_np(d.records()); })
            .def("labels", [to_np](const nd::LabeledDataset& d) { return to_np(d.labels()); })
            .def("__len__", &nd::LabeledDataset::len).def("is_empty", &nd::LabeledDataset::is_empty)
            .def("kfold", &nd::LabeledDataset::kfold)
            .def("batch", [to_np](const nd::LabeledDataset& d, size_t n, bool drop_last) {
                std::vector<std::pair<Arr, Arr>> out;
                for (const auto& b : d.batch(n, drop_last)) out.emplace_back(to_np(b.first), to_np(b.second));
                return out;
            }, py::arg("size"), py::arg("drop_last") = false)
            .def("split", &nd::LabeledDataset::split)
            .def("shuffle_with_seed", [](nd::LabeledDataset& d, uint64_t seed) { d.shuffle_with_seed(seed); });
        py::class_<nd::DataLoader>(dm, "DataLoader")
            .def(py::init<>())
            .def("without_headers", [](nd::DataLoader& l) { l.without_headers(); return l; })
            .def("with_delimiter", [](nd::DataLoader& l, char d) { l.with_delimiter(d); return l; })
            .def("with_labels", &nd::DataLoader::with_labels)
            .def("from_csv", &nd::DataLoader::from_csv)
            .def("from_string", &nd::DataLoader::from_string);
        py::class_<nd::LabeledDataLoader>(dm, "LabeledDataLoader")
            .def("without_headers", [](nd::LabeledDataLoader& l) { l.without_headers(); return l; })
            .def("with_delimiter", [](nd::LabeledDataLoader& l, char d) { l.with_delimiter(d); return l; })
            .def("from_csv", &nd::LabeledDataLoader::from_csv)
            .def("from_string", &nd::LabeledDataLoader::from_string);
        py::class_<nd::DeviceLoader>(dm, "DeviceLoader")
            .def(py::init<DevicePtr, const nd::LabeledDataset&, size_t, bool>(), py::arg("dev"), py::arg("dataset"),
                 py::arg("batch_size"), py::arg("drop_last") = true)
            .def(py::init<DevicePtr, const nd::Dataset&, size_t, bool>(), py::arg("dev"), py::arg("dataset"),
                 py::arg("batch_size"), py::arg("drop_last") = true)
            .def("batches", &nd::DeviceLoader::batches)
            .def("next_into", [](nd::DeviceLoader& l, const Var& x) { return l.next_into(x, nullptr); })
            .def("next_into", [](nd::DeviceLoader& l, const Var& x, const Var& y) { return l.next_into(x, &y); })
            .def("next", [](nd::DeviceLoader& l) {
                auto b = l.next();
                return py::make_tuple(b.rows, b.rows ? py::cast(b.x) : py::none(), (b.rows && b.y.data) ? py::cast(b.y) : py::none());
            });
    }

    py::module_ sd = m.def_submodule("serde");
    sd.def("to_json", py::overload_cast<const Var&>(&serde::to_json));
    sd.def("to_json", py::overload_cast<const VarDiff&>(&serde::to_json));
    sd.def("to_json", py::overload_cast<const nn::Linear&>(&serde::to_json));
    sd.def("var_from_json", py::overload_cast<DevicePtr, const std::string&>(&serde::var_from_json));
    sd.def("vardiff_from_json", py::overload_cast<DevicePtr, const std::string&>(&serde::vardiff_from_json));
    sd.def("linear_from_json", py::overload_cast<DevicePtr, const std::string&>(&serde::linear_from_json));
    sd.def("to_json", py::overload_cast<const nn::LayerNorm&>(&serde::to_json));
    sd.def("layer_norm_from_json", py::overload_cast<DevicePtr, const std::string&, double>(&serde::layer_norm_from_json), py::arg("dev"), py::arg("text"),
           py::arg("eps") = 1e-5);
    sd.def("to_json", py::overload_cast<const nn::GroupNorm&>(&serde::to_json));
    sd.def("group_norm_from_json", py::overload_cast<DevicePtr, const std::string&, int, double>(&serde::group_norm_from_json), py::arg("dev"), py::arg("text"),
           py::arg("num_groups"), py::arg("eps") = 1e-5);
    sd.def("to_json", py::overload_cast<const nn::RMSNorm&>(&serde::to_json));
    sd.def("rms_norm_from_json", py::overload_cast<DevicePtr, const std::string&, double>(&serde::rms_norm_from_json), py::arg("dev"), py::arg("text"),
           py::arg("eps") = 1e-6);
    sd.def("to_json", py::overload_cast<const nn::Embedding&>(&serde::to_json));
    sd.def("embedding_from_json", py::overload_cast<DevicePtr, const std::string&, long>(&serde::embedding_from_json), py::arg("dev"), py::arg("text"),
           py::arg("padding_idx") = -1);

    sd.def("to_json", py::overload_cast<const nn::BatchNormNd&>(&serde::to_json));
    sd.def("batch_norm_load_json", py::overload_cast<nn::BatchNormNd&, const std::string&>(&serde::batch_norm_load_json), py::arg("layer"), py::arg("text"));

    py::module_ nn = m.def_submodule("nn");
    nn.def("set_relu_peephole", &nn::set_relu_peephole, py::arg("on"));
    py::class_<nn::Linear>(nn, "Linear")
        .def(py::init<DevicePtr, int, int, uint64_t>(), py::arg("dev"), py::arg("in_features"), py::arg("out_features"), py::arg("seed") = 0)
        .def(py::init<VarDiff, VarDiff>())
        .def_readonly("weight", &nn::Linear::weight)
        .def_readonly("bias", &nn::Linear::bias)
        .def_readwrite("fused", &nn::Linear::fused)
        .def("forward", py::overload_cast<const Var&>(&nn::Linear::forward, py::const_))
        .def("forward", py::overload_cast<const VarDiff&>(&nn::Linear::forward, py::const_))
        .def("forward_relu", py::overload_cast<const Var&>(&nn::Linear::forward_relu, py::const_))
        .def("forward_relu", py::overload_cast<const VarDiff&>(&nn::Linear::forward_relu, py::const_));
    py::class_<nn::QuantLinear>(nn, "QuantLinear")
        .def(py::init<const nn::Linear&, int, int>(), py::arg("linear"), py::arg("bits"), py::arg("group") = 0,
             "Weight-only quantised Linear for inference: packs the Linear's weight to int8 / int4 with per-group f32 scales (group 32, 64, "
             "128, or 0 for one per row) on the device and shares its bias. The Linear is left as it is. No parameters, no gradient, no serde.")
        .def_readonly("in_features", &nn::QuantLinear::in_features)
        .def_readonly("out_features", &nn::QuantLinear::out_features)
        .def_readonly("bits", &nn::QuantLinear::bits)
        .def_readonly("group", &nn::QuantLinear::group)
        .def("forward", py::overload_cast<const Var&>(&nn::QuantLinear::forward, py::const_), py::arg("input"),
             "(rows, in_features) -> (rows, out_features), one forward node on nk_quant_linear_fwd, no gradient.")
        // a differentiable input (what the layers return) enters through its data and forward tape
        .def("forward", py::overload_cast<const VarDiff&>(&nn::QuantLinear::forward, py::const_), py::arg("input"))
        .def("dequantize", &nn::QuantLinear::dequantize, "The (out_features, in_features) values float(q) * scale the layer multiplies by.");
    py::class_<nn::LayerNorm>(nn, "LayerNorm")
        .def(py::init<DevicePtr, Shape, double, bool>(), py::arg("dev"), py::arg("normalized_shape"), py::arg("eps") = 1e-5,
             py::arg("elementwise_affine") = true)
        .def(py::init<VarDiff, VarDiff, double>(), py::arg("weight"), py::arg("bias"), py::arg("eps") = 1e-5)
        // without affine parameters there is no weight and no bias: None
        .def_property_readonly("weight", [](const nn::LayerNorm& l) { return l.elementwise_affine ? py::cast(l.weight) : py::object(py::none()); })
        .def_property_readonly("bias", [](const nn::LayerNorm& l) { return l.elementwise_affine ? py::cast(l.bias) : py::object(py::none()); })
        .def_readonly("normalized_shape", &nn::LayerNorm::normalized_shape)
        .def_readwrite("eps", &nn::LayerNorm::eps)
        .def_readonly("elementwise_affine", &nn::LayerNorm::elementwise_affine)
        .def("forward", py::overload_cast<const Var&>(&nn::LayerNorm::forward, py::const_))
        .def("forward", py::overload_cast<const VarDiff&>(&nn::LayerNorm::forward, py::const_));
    py::class_<nn::RMSNorm>(nn, "RMSNorm")
        .def(py::init<DevicePtr, Shape, double, bool>(), py::arg("dev"), py::arg("normalized_shape"), py::arg("eps") = 1e-6,
             py::arg("elementwise_affine") = true)
        .def(py::init<VarDiff, double>(), py::arg("weight"), py::arg("eps") = 1e-6)
        // without affine parameters there is no weight: None
        .def_property_readonly("weight", [](const nn::RMSNorm& l) { return l.elementwise_affine ? py::cast(l.weight) : py::object(py::none()); })
        .def_readonly("normalized_shape", &nn::RMSNorm::normalized_shape)
        .def_readwrite("eps", &nn::RMSNorm::eps)
        .def_readonly("elementwise_affine", &nn::RMSNorm::elementwise_affine)
        .def("forward", py::overload_cast<const Var&>(&nn::RMSNorm::forward, py::const_))
        .def("forward", py::overload_cast<const VarDiff&>(&nn::RMSNorm::forward, py::const_));
    py::class_<nn::GroupNorm>(nn, "GroupNorm")
        .def(py::init<DevicePtr, int, int, double, bool>(), py::arg("dev"), py::arg("num_groups"), py::arg("num_channels"), py::arg("eps") = 1e-5,
             py::arg("affine") = true)
        .def(py::init<int, VarDiff, VarDiff, double>(), py::arg("num_groups"), py::arg("weight"), py::arg("bias"), py::arg("eps") = 1e-5)
        // without affine parameters there is no weight and no bias: None
        .def_property_readonly("weight", [](const nn::GroupNorm& l) { return l.affine ? py::cast(l.weight) : py::object(py::none()); })
        .def_property_readonly("bias", [](const nn::GroupNorm& l) { return l.affine ? py::cast(l.bias) : py::object(py::none()); })
        .def_readonly("num_groups", &nn::GroupNorm::num_groups)
        .def_readonly("num_channels", &nn::GroupNorm::num_channels)
        .def_readwrite("eps", &nn::GroupNorm::eps)
        .def_readonly("affine", &nn::GroupNorm::affine)
        .def("forward", py::overload_cast<const Var&>(&nn::GroupNorm::forward, py::const_))
        .def("forward", py::overload_cast<const VarDiff&>(&nn::GroupNorm::forward, py::const_));
    py::class_<nn::InstanceNormNd>(nn, "InstanceNormNd")
        .def_property_readonly("weight", [](const nn::InstanceNormNd& l) { return l.affine ? py::cast(l.weight) : py::object(py::none()); })
        .def_property_readonly("bias", [](const nn::InstanceNormNd& l) { return l.affine ? py::cast(l.bias) : py::object(py::none()); })
        .def_readonly("num_features", &nn::InstanceNormNd::num_features)
        .def_readwrite("eps", &nn::InstanceNormNd::eps)
        .def_readonly("affine", &nn::InstanceNormNd::affine)
        .def("forward", py::overload_cast<const Var&>(&nn::InstanceNormNd::forward, py::const_))
        .def("forward", py::overload_cast<const VarDiff&>(&nn::InstanceNormNd::forward, py::const_));
    py::class_<nn::InstanceNorm1d, nn::InstanceNormNd>(nn, "InstanceNorm1d")
        .def(py::init<DevicePtr, int, double, bool>(), py::arg("dev"), py::arg("num_features"), py::arg("eps") = 1e-5, py::arg("affine") = false);
    py::class_<nn::InstanceNorm2d, nn::InstanceNormNd>(nn, "InstanceNorm2d")
        .def(py::init<DevicePtr, int, double, bool>(), py::arg("dev"), py::arg("num_features"), py::arg("eps") = 1e-5, py::arg("affine") = false);
    py::class_<nn::InstanceNorm3d, nn::InstanceNormNd>(nn, "InstanceNorm3d")
        .def(py::init<DevicePtr, int, double, bool>(), py::arg("dev"), py::arg("num_features"), py::arg("eps") = 1e-5, py::arg("affine") = false);
    py::class_<nn::GELU>(nn, "GELU")
        .def(py::init<bool>(), py::arg("approximate_tanh") = false)
        .def_readonly("approximate_tanh", &nn::GELU::approximate_tanh)
        .def("forward", py::overload_cast<const Var&>(&nn::GELU::forward, py::const_))
        .def("forward", py::overload_cast<const VarDiff&>(&nn::GELU::forward, py::const_));
    py::class_<nn::SiLU>(nn, "SiLU")
        .def(py::init<>())
        .def("forward", py::overload_cast<const Var&>(&nn::SiLU::forward, py::const_))
        .def("forward", py::overload_cast<const VarDiff&>(&nn::SiLU::forward, py::const_));
    py::class_<nn::GLU>(nn, "GLU")
        .def(py::init<Activation>(), py::arg("gate") = Activation::Sigmoid)
        .def_readonly("gate", &nn::GLU::gate)
        .def("forward", py::overload_cast<const Var&>(&nn::GLU::forward, py::const_))
        .def("forward", py::overload_cast<const VarDiff&>(&nn::GLU::forward, py::const_));
    py::class_<nn::CrossEntropyLoss>(nn, "CrossEntropyLoss")
        .def(py::init<Reduction, long, double>(), py::arg("reduction") = Reduction::Mean, py::arg("ignore_index") = -1, py::arg("label_smoothing") = 0.0)
        .def_readonly("reduction", &nn::CrossEntropyLoss::reduction)
        .def_readonly("ignore_index", &nn::CrossEntropyLoss::ignore_index)
        .def_readonly("label_smoothing", &nn::CrossEntropyLoss::label_smoothing)
        .def("forward", py::overload_cast<const Var&, const Var&>(&nn::CrossEntropyLoss::forward, py::const_))
        .def("forward", py::overload_cast<const VarDiff&, const Var&>(&nn::CrossEntropyLoss::forward, py::const_));
    py::class_<nn::Embedding>(nn, "Embedding")
        .def(py::init<DevicePtr, size_t, size_t, long, uint64_t>(), py::arg("dev"), py::arg("num_embeddings"), py::arg("embedding_dim"),
             py::arg("padding_idx") = -1, py::arg("seed") = 0)
        .def(py::init<VarDiff, long>(), py::arg("weight"), py::arg("padding_idx") = -1)
        .def_readonly("weight", &nn::Embedding::weight)
        .def_readonly("num_embeddings", &nn::Embedding::num_embeddings)
        .def_readonly("embedding_dim", &nn::Embedding::embedding_dim)
        .def_readonly("padding_idx", &nn::Embedding::padding_idx)
        .def("forward", &nn::Embedding::forward);
    {
        py::module_ im = nn.def_submodule("init");
        im.def("calculate_gain", &nn::init::calculate_gain);
        im.def("calculate_fan_in_fan_out", &nn::init::calculate_fan_in_fan_out);
        im.def("constant", &nn::init::constant); im.def("zeros", &nn::init::zeros); im.def("ones", &nn::init::ones);
        im.def("eye", &nn::init::eye); im.def("dirac", &nn::init::dirac);
        im.def("uniform", &nn::init::uniform, py::arg("param"), py::arg("low"), py::arg("high"), py::arg("seed") = 0);
        im.def("normal", &nn::init::normal, py::arg("param"), py::arg("mean"), py::arg("std"), py::arg("seed") = 0);
        im.def("xavier_uniform", &nn::init::xavier_uniform, py::arg("param"), py::arg("gain"), py::arg("seed") = 0);
        im.def("xavier_normal", &nn::init::xavier_normal, py::arg("param"), py::arg("gain"), py::arg("seed") = 0);
    }
    using State = std::pair<VarDiff, VarDiff>;
    py::class_<nn::LSTMCell>(nn, "LSTMCell")
        .def(py::init<DevicePtr, int, int, uint64_t>(), py::arg("dev"), py::arg("input_size"), py::arg("hidden_size"), py::arg("seed") = 0)
        .def_readonly("weight_ih", &nn::LSTMCell::weight_ih).def_readonly("weight_hh", &nn::LSTMCell::weight_hh)
        .def_readonly("bias_ih", &nn::LSTMCell::bias_ih).def_readonly("bias_hh", &nn::LSTMCell::bias_hh)
        .def("forward", py::overload_cast<const State&, const Var&>(&nn::LSTMCell::forward, py::const_))
        .def("forward", py::overload_cast<const State&, const VarDiff&>(&nn::LSTMCell::forward, py::const_));
    py::class_<nn::GRUCell>(nn, "GRUCell")
        .def(py::init<DevicePtr, int, int, uint64_t>(), py::arg("dev"), py::arg("input_size"), py::arg("hidden_size"), py::arg("seed") = 0)
        .def_readonly("weight_ih", &nn::GRUCell::weight_ih).def_readonly("weight_hh", &nn::GRUCell::weight_hh)
        .def_readonly("bias_ih", &nn::GRUCell::bias_ih).def_readonly("bias_hh", &nn::GRUCell::bias_hh)
        .def("forward", py::overload_cast<const VarDiff&, const Var&>(&nn::GRUCell::forward, py::const_))
        .def("forward", py::overload_cast<const VarDiff&, const VarDiff&>(&nn::GRUCell::forward, py::const_));
    py::class_<PaddingMode>(m, "PaddingMode")
        .def_static("zero", &PaddingMode::zero).def_static("constant", &PaddingMode::constant)
        .def_static("reflective", &PaddingMode::reflective).def_static("replicative", &PaddingMode::replicative);
    py::class_<nn::ConvNd>(nn, "ConvNd")
        .def_readonly("weight", &nn::ConvNd::weight)
        .def_readonly("bias", &nn::ConvNd::bias)
        .def_readwrite("fused", &nn::ConvNd::fused)
        .def_readwrite("fold_padding", &nn::ConvNd::fold_padding)
        .def_readonly("groups", &nn::ConvNd::groups)
        .def_readonly("padding", &nn::ConvNd::padding).def_readonly("stride", &nn::ConvNd::stride).def_readonly("dilation", &nn::ConvNd::dilation)
        .def("forward", py::overload_cast<const Var&>(&nn::ConvNd::forward, py::const_))
        .def("forward", py::overload_cast<const VarDiff&>(&nn::ConvNd::forward, py::const_));
    // argument order of the reference's `new` (neuronika-nn/src/lib.rs:671-679, 762-770, 857-865) + seed; GroupedConv*: + groups
    py::class_<nn::Conv1d, nn::ConvNd>(nn, "Conv1d")
        .def(py::init<DevicePtr, int, int, int, int, PaddingMode, int, int, uint64_t>(), py::arg("dev"), py::arg("in_channels"),
             py::arg("out_channels"), py::arg("kernel_size"), py::arg("padding"), py::arg("padding_mode"), py::arg("stride"),
             py::arg("dilation"), py::arg("seed") = 0);
    py::class_<nn::Conv2d, nn::ConvNd>(nn, "Conv2d")
        .def(py::init<DevicePtr, int, int, std::vector<int>, std::vector<int>, PaddingMode, std::vector<int>, std::vector<int>, uint64_t>(),
             py::arg("dev"), py::arg("in_channels"), py::arg("out_channels"), py::arg("kernel_size"), py::arg("padding"),
             py::arg("padding_mode"), py::arg("stride"), py::arg("dilation"), py::arg("seed") = 0);
    py::class_<nn::Conv3d, nn::ConvNd>(nn, "Conv3d")
        .def(py::init<DevicePtr, int, int, std::vector<int>, std::vector<int>, PaddingMode, std::vector<int>, std::vector<int>, uint64_t>(),
             py::arg("dev"), py::arg("in_channels"), py::arg("out_channels"), py::arg("kernel_size"), py::arg("padding"),
             py::arg("padding_mode"), py::arg("stride"), py::arg("dilation"), py::arg("seed") = 0);
    py::class_<nn::GroupedConv1d, nn::ConvNd>(nn, "GroupedConv1d")
        .def(py::init<DevicePtr, int, int, int, int, PaddingMode, int, int, int, uint64_t>(), py::arg("dev"), py::arg("in_channels"),
             py::arg("out_channels"), py::arg("kernel_size"), py::arg("padding"), py::arg("padding_mode"), py::arg("stride"),
             py::arg("dilation"), py::arg("groups"), py::arg("seed") = 0);
    py::class_<nn::GroupedConv2d, nn::ConvNd>(nn, "GroupedConv2d")
        .def(py::init<DevicePtr, int, int, std::vector<int>, std::vector<int>, PaddingMode, std::vector<int>, std::vector<int>, int, uint64_t>(),
             py::arg("dev"), py::arg("in_channels"), py::arg("out_channels"), py::arg("kernel_size"), py::arg("padding"),
             py::arg("padding_mode"), py::arg("stride"), py::arg("dilation"), py::arg("groups"), py::arg("seed") = 0);
    py::class_<nn::GroupedConv3d, nn::ConvNd>(nn, "GroupedConv3d")
        .def(py::init<DevicePtr, int, int, std::vector<int>, std::vector<int>, PaddingMode, std::vector<int>, std::vector<int>, int, uint64_t>(),
             py::arg("dev"), py::arg("in_channels"), py::arg("out_channels"), py::arg("kernel_size"), py::arg("padding"),
             py::arg("padding_mode"), py::arg("stride"), py::arg("dilation"), py::arg("groups"), py::arg("seed") = 0);
    py::class_<nn::BatchNormNd>(nn, "BatchNormNd")
        // without affine parameters there is no weight and no bias, without tracked statistics no buffers: None
        .def_property_readonly("weight", [](const nn::BatchNormNd& l) { return l.affine ? py::cast(l.weight) : py::object(py::none()); })
        .def_property_readonly("bias", [](const nn::BatchNormNd& l) { return l.affine ? py::cast(l.bias) : py::object(py::none()); })
        .def_property_readonly("running_mean", [](const nn::BatchNormNd& l) { return l.track_running_stats ? py::cast(l.running_mean) : py::object(py::none()); })
        .def_property_readonly("running_var", [](const nn::BatchNormNd& l) { return l.track_running_stats ? py::cast(l.running_var) : py::object(py::none()); })
        .def_readonly("num_features", &nn::BatchNormNd::num_features)
        .def_readwrite("eps", &nn::BatchNormNd::eps)
        .def_readwrite("momentum", &nn::BatchNormNd::momentum)
        .def_readonly("affine", &nn::BatchNormNd::affine)
        .def_readonly("track_running_stats", &nn::BatchNormNd::track_running_stats)
        .def_property_readonly("training", [](const nn::BatchNormNd& l) { return *l.status; })
        .def("train", &nn::BatchNormNd::train)
        .def("eval", &nn::BatchNormNd::eval)
        .def("forward", py::overload_cast<const Var&>(&nn::BatchNormNd::forward, py::const_))
        .def("forward", py::overload_cast<const VarDiff&>(&nn::BatchNormNd::forward, py::const_));
    py::class_<nn::BatchNorm1d, nn::BatchNormNd>(nn, "BatchNorm1d")
        .def(py::init<DevicePtr, int, double, double, bool, bool>(), py::arg("dev"), py::arg("num_features"), py::arg("eps") = 1e-5,
             py::arg("momentum") = 0.1, py::arg("affine") = true, py::arg("track_running_stats") = true);
    py::class_<nn::BatchNorm2d, nn::BatchNormNd>(nn, "BatchNorm2d")
        .def(py::init<DevicePtr, int, double, double, bool, bool>(), py::arg("dev"), py::arg("num_features"), py::arg("eps") = 1e-5,
             py::arg("momentum") = 0.1, py::arg("affine") = true, py::arg("track_running_stats") = true);
    py::class_<nn::BatchNorm3d, nn::BatchNormNd>(nn, "BatchNorm3d")
        .def(py::init<DevicePtr, int, double, double, bool, bool>(), py::arg("dev"), py::arg("num_features"), py::arg("eps") = 1e-5,
             py::arg("momentum") = 0.1, py::arg("affine") = true, py::arg("track_running_stats") = true);
    py::class_<nn::PoolNd>(nn, "PoolNd")
        .def_readonly("kernel_size", &nn::PoolNd::kernel_size)
        .def_readonly("stride", &nn::PoolNd::stride)
        .def_readonly("padding", &nn::PoolNd::padding)
        .def_readonly("count_include_pad", &nn::PoolNd::count_include_pad)
        .def("forward", py::overload_cast<const Var&>(&nn::PoolNd::forward, py::const_))
        .def("forward", py::overload_cast<const VarDiff&>(&nn::PoolNd::forward, py::const_));
    py::class_<nn::MaxPool1d, nn::PoolNd>(nn, "MaxPool1d")
        .def(py::init<int, int, int>(), py::arg("kernel_size"), py::arg("stride") = 0, py::arg("padding") = 0);
    py::class_<nn::MaxPool2d, nn::PoolNd>(nn, "MaxPool2d")
        .def(py::init<std::vector<int>, std::vector<int>, std::vector<int>>(), py::arg("kernel_size"), py::arg("stride") = std::vector<int>{},
             py::arg("padding") = std::vector<int>{});
    py::class_<nn::MaxPool3d, nn::PoolNd>(nn, "MaxPool3d")
        .def(py::init<std::vector<int>, std::vector<int>, std::vector<int>>(), py::arg("kernel_size"), py::arg("stride") = std::vector<int>{},
             py::arg("padding") = std::vector<int>{});
    py::class_<nn::AvgPool1d, nn::PoolNd>(nn, "AvgPool1d")
        .def(py::init<int, int, int, bool>(), py::arg("kernel_size"), py::arg("stride") = 0, py::arg("padding") = 0, py::arg("count_include_pad") = true);
    py::class_<nn::AvgPool2d, nn::PoolNd>(nn, "AvgPool2d")
        .def(py::init<std::vector<int>, std::vector<int>, std::vector<int>, bool>(), py::arg("kernel_size"), py::arg("stride") = std::vector<int>{},
             py::arg("padding") = std::vector<int>{}, py::arg("count_include_pad") = true);
    py::class_<nn::AvgPool3d, nn::PoolNd>(nn, "AvgPool3d")
        .def(py::init<std::vector<int>, std::vector<int>, std::vector<int>, bool>(), py::arg("kernel_size"), py::arg("stride") = std::vector<int>{},
             py::arg("padding") = std::vector<int>{}, py::arg("count_include_pad") = true);
    py::class_<nn::Upsample>(nn, "Upsample")
        .def(py::init([](py::object size, py::object scale_factor, std::string mode, bool align_corners) {
                 // an int / a float stands for one entry, as in torch; None for "not given"
                 std::vector<int> sz;
                 std::vector<double> sc;
                 if (!size.is_none()) sz = py::isinstance<py::int_>(size) ? std::vector<int>{size.cast<int>()} : size.cast<std::vector<int>>();
                 if (!scale_factor.is_none())
                     sc = (py::isinstance<py::float_>(scale_factor) || py::isinstance<py::int_>(scale_factor)) ? std::vector<double>{scale_factor.cast<double>()}
                                                                                                              : scale_factor.cast<std::vector<double>>();
                 return nn::Upsample(std::move(sz), std::move(sc), std::move(mode), align_corners);
             }),
             py::arg("size") = py::none(), py::arg("scale_factor") = py::none(), py::arg("mode") = "nearest", py::arg("align_corners") = false)
        .def_readonly("size", &nn::Upsample::size)
        .def_readonly("scale_factor", &nn::Upsample::scale_factor)
        .def_readonly("mode", &nn::Upsample::mode)
        .def_readonly("align_corners", &nn::Upsample::align_corners)
        .def("output_size", [](const nn::Upsample& u, const std::vector<int>& shape) { return u.output_size(shape); }, py::arg("input_shape"))
        .def("forward", py::overload_cast<const Var&>(&nn::Upsample::forward, py::const_))
        .def("forward", py::overload_cast<const VarDiff&>(&nn::Upsample::forward, py::const_));
    py::class_<nn::Dropout>(nn, "Dropout")
        .def(py::init<double>())
        .def("train", &nn::Dropout::train)
        .def("eval", &nn::Dropout::eval)
        .def("forward", &nn::Dropout::forward);
    py::class_<nn::KvCache>(nn, "KvCache")
        .def(py::init<DevicePtr, int, int, int, int, bool>(), py::arg("dev"), py::arg("batch"), py::arg("heads"), py::arg("head_dim"),
             py::arg("capacity"), py::arg("rolling") = false,
             "Keys and values of one causal attention layer on the device, (batch, heads, capacity, head_dim) each, for "
             "MultiheadAttention.forward_step. rolling: a ring for a sliding-window layer, position p at slot p % capacity.")
        .def_readonly("rolling", &nn::KvCache::rolling)
        .def("workspace_floats", &nn::KvCache::workspace_floats, "floats of decode scratch the cache holds now")
        .def("high_water", [](const nn::KvCache& c) { return c.high_water(); }, "the largest length every sample reached since the last reset")
        .def_readonly("batch", &nn::KvCache::batch)
        .def_readonly("heads", &nn::KvCache::heads)
        .def_readonly("head_dim", &nn::KvCache::head_dim)
        .def_readonly("capacity", &nn::KvCache::capacity)
        .def("lens", [](const nn::KvCache& c) { return c.lens(); }, "positions held per sample")
        .def("reset", &nn::KvCache::reset, "every length back to 0")
        .def("truncate", &nn::KvCache::truncate, py::arg("lens"),
             "Give every sample a length no longer than its current one: ragged prompts after a right-padded prefill, roll-back.");
    py::class_<nn::PageTable>(nn, "PageTable")
        .def(py::init<int, int, int, int>(), py::arg("num_pages"), py::arg("page"), py::arg("max_seqs"), py::arg("max_pages"),
             "The page table of a paged key / value cache, on the host: per sequence a length and a row of page ids (-1: none), per "
             "page a reference count. Every operation that can fail raises before it changes anything.")
        .def_readonly("num_pages", &nn::PageTable::num_pages)
        .def_readonly("page", &nn::PageTable::page)
        .def_readonly("max_seqs", &nn::PageTable::max_seqs)
        .def_readonly("max_pages", &nn::PageTable::max_pages)
        .def("lens", [](const nn::PageTable& t) { return t.lens(); }, "positions held per sequence")
        .def("pages", &nn::PageTable::pages, py::arg("seq"), "the page ids the sequence owns, in position order")
        .def("row", &nn::PageTable::row, py::arg("seq"), "max_pages ints, -1 where the sequence owns nothing")
        .def("refcount", &nn::PageTable::refcount, py::arg("page"))
        .def("free_pages", &nn::PageTable::free_pages, "the free page ids, ascending")
        .def("behind", &nn::PageTable::behind, py::arg("seq"), "the first position the sequence still holds")
        .def("reserve", &nn::PageTable::reserve, py::arg("seqs"), py::arg("T"),
             "Grow every listed sequence by T positions, lowest free page first; returns the (old, new) page copies to make.")
        .def("truncate", &nn::PageTable::truncate, py::arg("seq"), py::arg("len"))
        .def("release", &nn::PageTable::release, py::arg("seq"))
        .def("fork", &nn::PageTable::fork, py::arg("src"), py::arg("dst"))
        .def("release_behind", &nn::PageTable::release_behind, py::arg("seq"), py::arg("pos"))
        .def("reset", &nn::PageTable::reset);
    py::class_<nn::PagedKvCache>(nn, "PagedKvCache")
        .def(py::init<DevicePtr, int, int, int, int, int, int>(), py::arg("dev"), py::arg("num_pages"), py::arg("page"), py::arg("kv_heads"),
             py::arg("head_dim"), py::arg("max_seqs"), py::arg("max_pages"),
             "Keys and values of one causal attention layer in pages: two pools (num_pages, kv_heads, page, head_dim) and a PageTable, "
             "for MultiheadAttention.forward_step(x, seqs, cache).")
        .def_readonly("num_pages", &nn::PagedKvCache::num_pages)
        .def_readonly("page", &nn::PagedKvCache::page)
        .def_readonly("heads", &nn::PagedKvCache::heads)
        .def_readonly("head_dim", &nn::PagedKvCache::head_dim)
        .def_readonly("max_seqs", &nn::PagedKvCache::max_seqs)
        .def_readonly("max_pages", &nn::PagedKvCache::max_pages)
        .def("workspace_floats", &nn::PagedKvCache::workspace_floats, "floats of decode scratch the cache holds now")
        .def("k_data", [](const nn::PagedKvCache& c) { return to_numpy(*c.k); }, "the key pool, downloaded")
        .def("v_data", [](const nn::PagedKvCache& c) { return to_numpy(*c.v); }, "the value pool, downloaded")
        .def("lens", [](const nn::PagedKvCache& c) { return c.lens(); }, "positions held per sequence")
        .def("pages", &nn::PagedKvCache::pages, py::arg("seq"))
        .def("row", &nn::PagedKvCache::row, py::arg("seq"))
        .def("refcount", &nn::PagedKvCache::refcount, py::arg("page"))
        .def("free_pages", &nn::PagedKvCache::free_pages)
        .def("behind", &nn::PagedKvCache::behind, py::arg("seq"))
        .def("reserve", &nn::PagedKvCache::reserve, py::arg("seqs"), py::arg("T"))
        .def("truncate", &nn::PagedKvCache::truncate, py::arg("seq"), py::arg("len"))
        .def("release", &nn::PagedKvCache::release, py::arg("seq"))
        .def("fork", &nn::PagedKvCache::fork, py::arg("src"), py::arg("dst"))
        .def("release_behind", &nn::PagedKvCache::release_behind, py::arg("seq"), py::arg("pos"))
        .def("reset", &nn::PagedKvCache::reset);
    py::class_<nn::Segments>(nn, "Segments")
        .def(py::init<DevicePtr, int, int, const std::vector<std::vector<int>>&>(), py::arg("dev"), py::arg("batch"), py::arg("S"), py::arg("doc_lens"),
             "Packed sequences: per sample the lengths of its documents (positive, sum <= S; a remainder is one more document). Holds the "
             "device arrays lo (start of the row's document) and pos (position inside it), uploaded once, for MultiheadAttention.forward.")
        .def_readonly("batch", &nn::Segments::batch)
        .def_readonly("S", &nn::Segments::S)
        .def_readonly("max_len", &nn::Segments::max_len)
        .def("lo", [](const nn::Segments& s) { return py::array_t<int>({s.batch, s.S}, s.lo_host.data()); }, "the host copy of lo, (batch, S) int32")
        .def("pos", [](const nn::Segments& s) { return py::array_t<int>({s.batch, s.S}, s.pos_host.data()); }, "the host copy of pos, (batch, S) int32");
    py::class_<nn::RotaryEmbedding, std::shared_ptr<nn::RotaryEmbedding>>(nn, "RotaryEmbedding")
        .def(py::init<DevicePtr, int, int, double, int, bool>(), py::arg("dev"), py::arg("head_dim"), py::arg("max_pos"), py::arg("base") = 10000.0,
             py::arg("rot") = 0, py::arg("interleaved") = false,
             "Rotary position embedding: owns the (max_pos, rot/2, 2) table of (cos, sin) of p * base^(-2j/rot), made in f64. rot = 0 means "
             "head_dim; interleaved pairs (2j, 2j+1) instead of (j, j + rot/2). No parameters.")
        .def_readonly("head_dim", &nn::RotaryEmbedding::head_dim)
        .def_readonly("max_pos", &nn::RotaryEmbedding::max_pos)
        .def_readonly("rot", &nn::RotaryEmbedding::rot)
        .def_readonly("base", &nn::RotaryEmbedding::base)
        .def_readonly("interleaved", &nn::RotaryEmbedding::interleaved)
        .def("table", [](const nn::RotaryEmbedding& r) { return to_numpy(*r.table); }, "the table as a (max_pos, rot/2, 2) array");
    // registered here, after the class they take: the signatures in the docstrings name it
    py::reinterpret_borrow<py::class_<Var>>(m.attr("Var"))
        .def("rope", &Var::rope, py::arg("rotary"), py::arg("batch"), py::arg("heads"),
             "Rotate the first `rot` columns of every head of a (batch*T, heads*head_dim) value by the angles of positions 0 .. T-1.");
    py::reinterpret_borrow<py::class_<VarDiff>>(m.attr("VarDiff"))
        .def("rope", &VarDiff::rope, py::arg("rotary"), py::arg("batch"), py::arg("heads"));
    // packed sequences: the trailing segments argument, as a second signature (the first one and its defaults stay as they are)
    py::reinterpret_borrow<py::class_<Var>>(m.attr("Var"))
        .def("heads_attention", [](const Var& q, const Var& k, const Var& v, int B, int S, int H, int dh, float scale, double p, const Status& s,
                                   bool causal, int window, const nn::Segments& seg) {
                 return q.heads_attention(k, v, B, S, H, dh, scale, p, s.flag, causal, window, &seg); },
             py::arg("keys"), py::arg("values"), py::arg("B"), py::arg("S"), py::arg("H"), py::arg("dh"), py::arg("scale"), py::arg("p"),
             py::arg("status"), py::arg("causal"), py::arg("window"), py::arg("segments"));
    py::reinterpret_borrow<py::class_<VarDiff>>(m.attr("VarDiff"))
        .def("heads_attention", [](const VarDiff& q, const VarDiff& k, const VarDiff& v, int B, int S, int H, int dh, float scale, double p,
                                   const Status& s, bool causal, int window, const nn::Segments& seg) {
                 return q.heads_attention(k, v, B, S, H, dh, scale, p, s.flag, causal, window, &seg); },
             py::arg("keys"), py::arg("values"), py::arg("B"), py::arg("S"), py::arg("H"), py::arg("dh"), py::arg("scale"), py::arg("p"),
             py::arg("status"), py::arg("causal"), py::arg("window"), py::arg("segments"));
    py::reinterpret_borrow<py::class_<Var>>(m.attr("Var"))
        .def("repeat_kv", &Var::repeat_kv, py::arg("groups"), py::arg("head_dim"),
             "Every head of a (rows, kv_heads*head_dim) value written `groups` times: (rows, kv_heads*groups*head_dim), a bit-exact copy.");
    py::reinterpret_borrow<py::class_<VarDiff>>(m.attr("VarDiff"))
        .def("repeat_kv", &VarDiff::repeat_kv, py::arg("groups"), py::arg("head_dim"));
    py::class_<nn::Sampler>(nn, "Sampler")
        .def(py::init<DevicePtr, float, int, float, uint64_t>(), py::arg("dev"), py::arg("temperature") = 1.0f, py::arg("top_k") = 0,
             py::arg("top_p") = 1.0f, py::arg("seed") = 0,
             "Token sampling on the device: greedy at temperature 0, else temperature, top-k (0: off) and top-p (1: off) and one Philox "
             "draw per row at (seed, offset). The members are read when forward builds its node; every execution of a node advances offset.")
        .def_readwrite("temperature", &nn::Sampler::temperature)
        .def_readwrite("top_k", &nn::Sampler::top_k)
        .def_readwrite("top_p", &nn::Sampler::top_p)
        .def_readwrite("seed", &nn::Sampler::seed)
        .def_property("offset", [](const nn::Sampler& s) { return *s.offset; }, [](nn::Sampler& s, uint64_t v) { *s.offset = v; },
                      "the Philox offset the next execution draws at; shared by every node this sampler built")
        .def("forward", py::overload_cast<const Var&, int>(&nn::Sampler::forward, py::const_), py::arg("logits"), py::arg("batch"),
             "(batch*T, V) logits -> the (batch,) ids of the last position of every sample, f32, no gradient: what Embedding.forward takes.")
        // a differentiable input (what the layers return) enters through its data and forward tape
        .def("forward", py::overload_cast<const VarDiff&, int>(&nn::Sampler::forward, py::const_), py::arg("logits"), py::arg("batch"));
    py::reinterpret_borrow<py::class_<Var>>(m.attr("Var"))
        .def("sample", &Var::sample, py::arg("sampler"), py::arg("batch"),
             "The ids of the last position of every sample of (batch*T, V) logits, drawn by `sampler` on the device.");
    py::class_<nn::MultiheadAttention>(nn, "MultiheadAttention")
        // kv_heads = 0: heads (plain multi-head attention); a divisor of heads: grouped-query attention, k and v (kv_heads*dh, d_model)
        .def(py::init([](DevicePtr dev, int d_model, int heads, double p, uint64_t seed, int kv_heads) {
                 return nn::MultiheadAttention(std::move(dev), d_model, heads, kv_heads == 0 ? heads : kv_heads, p, seed); }),
             py::arg("dev"), py::arg("d_model"), py::arg("heads"), py::arg("p") = 0.0, py::arg("seed") = 0, py::arg("kv_heads") = 0)
        .def(py::init<nn::Linear, nn::Linear, nn::Linear, nn::Linear, int, double, int>(), py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"),
             py::arg("heads"), py::arg("p") = 0.0, py::arg("kv_heads") = 0)  // four layers built elsewhere: not packed
        .def_readwrite("q", &nn::MultiheadAttention::q)   // public, assignable members in the C++ mirror as well
        .def_readwrite("k", &nn::MultiheadAttention::k)
        .def_readwrite("v", &nn::MultiheadAttention::v)
        .def_readwrite("o", &nn::MultiheadAttention::o)
        .def_readonly("drop", &nn::MultiheadAttention::drop)
        .def_readwrite("fused", &nn::MultiheadAttention::fused)
        .def_readwrite("strided_heads", &nn::MultiheadAttention::strided_heads)
        .def_readwrite("fused_core", &nn::MultiheadAttention::fused_core)
        .def_readwrite("packed_qkv", &nn::MultiheadAttention::packed_qkv)
        .def_readwrite("causal", &nn::MultiheadAttention::causal)
        .def_readwrite("window", &nn::MultiheadAttention::window)  // sliding window: 0 = off; needs causal
        .def_readwrite("rope", &nn::MultiheadAttention::rope)  // a shared RotaryEmbedding; None clears it
        .def_readonly("d_model", &nn::MultiheadAttention::d_model)
        .def_readonly("heads", &nn::MultiheadAttention::heads)
        .def_readonly("kv_heads", &nn::MultiheadAttention::kv_heads)
        .def("forward", py::overload_cast<const VarDiff&, int>(&nn::MultiheadAttention::forward, py::const_), py::arg("x"), py::arg("batch"))
        .def("forward", py::overload_cast<const VarDiff&, int, const nn::Segments&>(&nn::MultiheadAttention::forward, py::const_), py::arg("x"),
             py::arg("batch"), py::arg("segments"),
             "Packed sequences: every token attends to its own document only and rope restarts at every document start.")
        .def("forward_step", py::overload_cast<const Var&, int, nn::KvCache&>(&nn::MultiheadAttention::forward_step, py::const_), py::arg("x"),
             py::arg("batch"), py::arg("cache"),
             "Incremental decoding: x holds the new positions only, (batch*T, d_model); returns (batch*T, d_model) without a gradient. "
             "The cache's lengths advance when the node is built. Needs causal = True and inactive dropout (drop.eval()).")
        // a differentiable input (what the other layers return) enters through its data and forward tape; still no gradient out
        .def("forward_step", [](const nn::MultiheadAttention& m, const VarDiff& x, int batch, nn::KvCache& cache) {
                 return m.forward_step(x.var, batch, cache); }, py::arg("x"), py::arg("batch"), py::arg("cache"))
        .def("forward_step", py::overload_cast<const Var&, const std::vector<int>&, nn::PagedKvCache&>(&nn::MultiheadAttention::forward_step, py::const_),
             py::arg("x"), py::arg("seqs"), py::arg("cache"),
             "The same step over a paged cache: the batch is len(seqs), any subset of the cache's sequences in any order. Pages are "
             "reserved when the node is built; forward() runs the page copies, the append and the attention.")
        .def("forward_step", [](const nn::MultiheadAttention& m, const VarDiff& x, const std::vector<int>& seqs, nn::PagedKvCache& cache) {
                 return m.forward_step(x.var, seqs, cache); }, py::arg("x"), py::arg("seqs"), py::arg("cache"))
        .def("quantize", &nn::MultiheadAttention::quantize, py::arg("bits"), py::arg("group") = 0,
             "Build int8 / int4 images of the projections forward_step uses (the packed [Wq; Wk; Wv] storage while the module is still "
             "packed, three images otherwise) and of o; both forward_step overloads then project through nk_quant_linear_fwd. forward() "
             "is untouched. A snapshot: call it again after the weights change.")
        .def_property_readonly("quantized", &nn::MultiheadAttention::quantized);

    py::module_ optim = m.def_submodule("optim");
    {
        namespace ls = optim::lr_scheduler;
        py::module_ lm = optim.def_submodule("lr_scheduler");
        py::class_<ls::LRScheduler>(lm, "LRScheduler")
            .def("step", &ls::LRScheduler::step)
            .def("get_last_lr", &ls::LRScheduler::get_last_lr)
            .def("get_current_lr", &ls::LRScheduler::get_current_lr)
            .def("get_current_epoch", &ls::LRScheduler::get_current_epoch)
            .def("set_current_epoch", &ls::LRScheduler::set_current_epoch);
        py::class_<ls::StepLR, ls::LRScheduler>(lm, "StepLR")
            .def(py::init<optim::Optimizer&, size_t, float>(), py::keep_alive<1, 2>()).def("set_gamma", &ls::StepLR::set_gamma);
        py::class_<ls::MultiStepLR, ls::LRScheduler>(lm, "MultiStepLR")
            .def(py::init<optim::Optimizer&, std::vector<size_t>, float>(), py::keep_alive<1, 2>())
            .def("set_milestones", &ls::MultiStepLR::set_milestones);
        py::class_<ls::ExponentialLR, ls::LRScheduler>(lm, "ExponentialLR")
            .def(py::init<optim::Optimizer&, float>(), py::keep_alive<1, 2>()).def("set_gamma", &ls::ExponentialLR::set_gamma);
        py::class_<ls::LambdaLR, ls::LRScheduler>(lm, "LambdaLR")
            .def(py::init<optim::Optimizer&, std::function<float(size_t)>>(), py::keep_alive<1, 2>());
        py::class_<ls::MultiplicativeLR, ls::LRScheduler>(lm, "MultiplicativeLR")
            .def(py::init<optim::Optimizer&, std::function<float(size_t)>>(), py::keep_alive<1, 2>());
    }
    py::class_<optim::Optimizer>(optim, "Optimizer")
        .def("register", &optim::Optimizer::register_param)
        .def("step", &optim::Optimizer::step)
        .def("zero_grad", &optim::Optimizer::zero_grad)
        .def("get_lr", &optim::Optimizer::get_lr)
        .def("set_lr", &optim::Optimizer::set_lr)
        .def("clip_grad_norm", &optim::Optimizer::clip_grad_norm, py::arg("max_norm"),
             "Clip the registered parameters' gradients to the global L2 norm max_norm; returns the norm before clipping as a 0-d Var "
             "on the device (item() synchronises). The Var ALIASES a buffer the optimizer keeps, which is what lets the call be "
             "captured: it holds the norm of the LATEST call. Read it with item() before the next call if norms are collected.");
    optim.def("clip_grad_norm", &optim::clip_grad_norm, py::arg("params"), py::arg("max_norm"),
              "Clip the gradients of params to the global L2 norm max_norm; returns the norm before clipping as a 0-d Var on the "
              "device in a buffer of its own (item() synchronises). A parameter listed twice counts once; +inf measures only.");
    py::class_<optim::SGD, optim::Optimizer>(optim, "SGD")
        .def(py::init([](float lr, float l1, float l2, float momentum, float dampening, bool nesterov) {
                 return new optim::SGD(lr, optim::Penalty{l1, l2}, momentum, dampening, nesterov);
             }),
             py::arg("lr"), py::arg("l1") = 0.f, py::arg("l2") = 0.f, py::arg("momentum") = 0.f, py::arg("dampening") = 0.f,
             py::arg("nesterov") = false);
    py::class_<optim::Adam, optim::Optimizer>(optim, "Adam")
        .def(py::init([](float lr, float beta1, float beta2, float eps, float l1, float l2, bool amsgrad) {
                 return new optim::Adam(lr, beta1, beta2, eps, optim::Penalty{l1, l2}, amsgrad);
             }),
             py::arg("lr"), py::arg("beta1") = 0.9f, py::arg("beta2") = 0.999f, py::arg("eps") = 1e-8f, py::arg("l1") = 0.f,
             py::arg("l2") = 0.f, py::arg("amsgrad") = false);
    py::class_<optim::AdamW, optim::Optimizer>(optim, "AdamW")
        .def(py::init<float, float, float, float, float, bool>(), py::arg("lr"), py::arg("beta1") = 0.9f, py::arg("beta2") = 0.999f,
             py::arg("eps") = 1e-8f, py::arg("weight_decay") = 1e-2f, py::arg("amsgrad") = false);
    py::class_<optim::Adagrad, optim::Optimizer>(optim, "Adagrad")
        .def(py::init([](float lr, float lr_decay, float eps, float l1, float l2) {
                 return new optim::Adagrad(lr, lr_decay, eps, optim::Penalty{l1, l2});
             }),
             py::arg("lr"), py::arg("lr_decay") = 0.f, py::arg("eps") = 1e-10f, py::arg("l1") = 0.f, py::arg("l2") = 0.f);
    py::class_<optim::RMSProp, optim::Optimizer>(optim, "RMSProp")
        .def(py::init([](float lr, float alpha, float eps, float momentum, bool centered, float l1, float l2) {
                 return new optim::RMSProp(lr, alpha, eps, momentum, centered, optim::Penalty{l1, l2});
             }),
             py::arg("lr"), py::arg("alpha") = 0.99f, py::arg("eps") = 1e-8f, py::arg("momentum") = 0.f,
             py::arg("centered") = false, py::arg("l1") = 0.f, py::arg("l2") = 0.f);

    py::module_ dpm = m.def_submodule("dp");
    py::class_<dp::Communicator, std::shared_ptr<dp::Communicator>>(dpm, "Communicator")
        .def_static("unique_id", []() { return py::bytes(dp::Communicator::unique_id()); })
        .def(py::init([](DevicePtr dev, int nranks, int rank, py::bytes id) {
            return std::make_shared<dp::Communicator>(std::move(dev), nranks, rank, std::string(id));
        }))
        .def_static("replicas", &dp::Communicator::replicas, py::arg("device"), py::arg("nranks"), py::arg("channels") = 0, py::arg("gbps") = 0.0)
        .def("raw", [](const dp::Communicator& c) { return (uintptr_t)c.raw(); })  // nk_comm* for the raw C ABI (bench diagnostics)
        .def_property_readonly("rank", &dp::Communicator::rank)
        .def_property_readonly("size", &dp::Communicator::size);
    py::class_<dp::GradientSync>(dpm, "GradientSync")
        .def(py::init<std::shared_ptr<dp::Communicator>, const std::vector<VarDiff>&, size_t>(), py::arg("comm"), py::arg("params"),
             py::arg("small_elems") = (size_t)65536)
        .def("join", &dp::GradientSync::join)
        .def("bytes_per_step", &dp::GradientSync::bytes_per_step)
        .def("set_force_exchange", &dp::GradientSync::set_force_exchange)
        .def("set_busy_slots", &dp::GradientSync::set_busy_slots, py::arg("n"))
        .def("busy_slots", &dp::GradientSync::busy_slots)
        .def("set_parts", [](dp::GradientSync& s, const std::string& mode) {
            if (mode == "all") s.set_parts(dp::GradientSync::Parts::All);
            else if (mode == "last") s.set_parts(dp::GradientSync::Parts::LastOnly);
            else if (mode == "none") s.set_parts(dp::GradientSync::Parts::None);
            else throw std::invalid_argument("set_parts: all | last | none");
        })
        .def("exchanges_issued", &dp::GradientSync::exchanges_issued)
        .def("elements_exchanged", &dp::GradientSync::elements_exchanged);
    dpm.def("all_reduce_gradients", &dp::all_reduce_gradients);
}

// Implementation of the host-side tape mirror (see neuronika.hpp).  Every node's forward() /
// backward() body is ONE call into the C ABI (include/neuronika_hip.h), issued asynchronously
// on the device's compute stream in tape order.
#include "neuronika.hpp"

#include <climits>
#include <cstdlib>

#include <algorithm>
#include <charconv>
#include <cstring>
#include <cmath>
#include <random>

namespace neuronika {

void panic(const std::string& msg) { throw Panic(msg); }
void check(int status) {
    if (status != NK_OK) panic(nk_last_error());
}
size_t numel(const Shape& s) {
    size_t n = 1;
    for (int d : s) n *= (size_t)d;
    return n;
}

// =================================================================================================
// Device / HipArray / Gradient
// =================================================================================================
std::shared_ptr<Device> Device::create(int idx) {
    std::shared_ptr<Device> d(new Device());
    check(nk_device_create(idx, &d->h_));
    d->idx_ = idx;
    return d;
}
Device::~Device() {
    if (!h_) return;
    nk_device_sync(h_);
    for (auto& kv : pool_)
        for (float* p : kv.second) nk_free(h_, p);
    nk_device_destroy(h_);
}
void Device::sync() const { check(nk_device_sync(h_)); }
float* Device::alloc_zeroed(size_t n) {
    auto it = pool_.find(n);
    float* p = nullptr;
    if (it != pool_.end() && !it->second.empty()) {
        p = it->second.back();
        it->second.pop_back();
        check(nk_fill(h_, p, n, 0.f));
    } else {
        check(nk_alloc_zeroed(h_, n, &p));
    }
    in_use_ += n * sizeof(float);
    return p;
}
void Device::graph_begin() { check(nk_graph_begin(h_)); }
std::shared_ptr<Graph> Device::graph_end() {
    nk_graph* g = nullptr;
    check(nk_graph_end(h_, &g));
    return std::make_shared<Graph>(g, shared_from_this());
}
Graph::~Graph() { (void)nk_graph_destroy(g_); }  // dev_ (a member) is released after this body: the device outlives its graphs
void Graph::launch() const { check(nk_graph_launch(g_)); }

float* Device::alloc_uninit(size_t n) {
    auto it = pool_.find(n);
    float* p = nullptr;
    if (it != pool_.end() && !it->second.empty()) {
        p = it->second.back();
        it->second.pop_back();
    } else {
        check(nk_alloc_zeroed(h_, n, &p));
    }
    in_use_ += n * sizeof(float);
    return p;
}
void Device::release(float* p, size_t n) {
    if (!p) return;
    pool_[n].push_back(p);
    in_use_ -= n * sizeof(float);
}

HipArray::HipArray(DevicePtr dev, Shape shape)
    : dev_(std::move(dev)), shape_(std::move(shape)), len_(numel(shape_)), ptr_(dev_->alloc_zeroed(len_)) {}
HipArray::HipArray(DevicePtr dev, Shape shape, Uninit)
    : dev_(std::move(dev)), shape_(std::move(shape)), len_(numel(shape_)), ptr_(dev_->alloc_uninit(len_)) {}
HipArray::HipArray(std::shared_ptr<HipArray> parent, size_t offset, Shape shape)
    : dev_(parent->device()), shape_(std::move(shape)), len_(numel(shape_)), ptr_(parent->ptr() + offset), parent_(std::move(parent)) {
    if (offset + len_ > parent_->len()) panic("HipArray view: out of the parent's range");
}
HipArray::~HipArray() {
    if (!parent_) dev_->release(ptr_, len_);
}
std::shared_ptr<HipArray> HipArray::from_host(DevicePtr dev, const Shape& shape, const float* host) {
    auto a = std::make_shared<HipArray>(std::move(dev), shape);
    a->upload(host);
    return a;
}
void HipArray::upload(const float* host) { check(nk_upload(dev_->raw(), ptr_, host, len_)); }
void HipArray::download(float* host) const { check(nk_download(dev_->raw(), host, ptr_, len_)); }
std::vector<float> HipArray::to_vec() const {
    std::vector<float> v(len_);
    download(v.data());
    return v;
}
void HipArray::fill(float v) { check(nk_fill(dev_->raw(), ptr_, len_, v)); }

Gradient::Gradient(DevicePtr dev, Shape shape)
    : dev_(std::move(dev)), shape_(std::move(shape)), array_(std::make_shared<HipArray>(dev_, shape_, HipArray::Uninit{})) {}
Gradient::Gradient(Shared<HipArray> storage, size_t offset, Shape shape)
    : dev_(storage->device()), shape_(std::move(shape)), array_(std::make_shared<HipArray>(storage, offset, shape_)), storage_(std::move(storage)),
      offset_(offset) {}
HipArray& Gradient::borrow() const {
    if (!array_)
        panic("Trying to get a de-allocated gradient. Switch on the gradients first by using `.with_grad()`");
    if (pending_zero_) {
        array_->fill(0.f);
        pending_zero_ = false;
    }
    return *array_;
}
Shared<HipArray> Gradient::exchange_array(Shared<HipArray> external) {
    if (!array_) panic("Trying to get a de-allocated gradient. Switch on the gradients first by using `.with_grad()`");
    if (external->len() != array_->len()) panic("exchange_array: extent mismatch");
    std::swap(array_, external);
    pending_zero_ = false;
    return external;
}
HipArray& Gradient::borrow_first_write(bool& assign) const {
    if (!array_)
        panic("Trying to get a de-allocated gradient. Switch on the gradients first by using `.with_grad()`");
    assign = pending_zero_;
    pending_zero_ = false;
    return *array_;
}
void Gradient::zero() {
    if (!array_)
        panic("Trying to get a de-allocated gradient. Switch on the gradients first by using `.with_grad()`");
    pending_zero_ = true;
}
void Gradient::no_grad() { array_.reset(); }
void Gradient::with_grad() {
    if (!array_) {
        array_ = storage_ ? std::make_shared<HipArray>(storage_, offset_, shape_) : std::make_shared<HipArray>(dev_, shape_, HipArray::Uninit{});
        pending_zero_ = true;
    }
}

// =================================================================================================
// History
// =================================================================================================
template <class T>
void History<T>::merge(const History& other) {
    for (const Item& it : other.path_) {
        bool present = false;
        for (const Item& mine : path_)
            if (mine.ptr == it.ptr) { present = true; break; }
        if (!present) path_.push_back(it);
    }
    std::stable_sort(path_.begin(), path_.end(), [](const Item& a, const Item& b) { return a.order < b.order; });
}
template <class T>
void History<T>::insert(const void* ptr, T op) {
    path_.push_back(Item{ptr, path_.size(), std::move(op)});
    buffer_->clear();
}
template <class T>
std::vector<T> History<T>::to_vec() const {
    std::vector<T> v;
    v.reserve(path_.size());
    for (const Item& it : path_) v.push_back(it.op);
    return v;
}
template class History<ForwardEntry>;
template class History<BackwardEntry>;

// =================================================================================================
// helpers
// =================================================================================================
// Philox key of the next random node (Dropout, fused attention probabilities).  The reference draws from
// `rand::thread_rng()` (dropout/mod.rs:68-70), seeded by the OS; here every node gets its own key from one per-thread
// sequence that `manual_seed` restarts, so a run is reproducible and data-parallel ranks can decorrelate their masks
// (`manual_seed(base + rank)`).
static thread_local uint64_t g_node_seed = 0x9E3779B97F4A7C15ull;
void manual_seed(uint64_t seed) { g_node_seed = seed; }
static uint64_t next_node_seed() {
    const uint64_t s = g_node_seed;
    g_node_seed += 0x632BE59BD9B4E019ull;
    return s;
}

namespace {

nk_device* D(const Shared<HipArray>& a) { return a->device()->raw(); }
Shared<HipArray> zeros_like(const Shared<HipArray>& a, Shape s) { return std::make_shared<HipArray>(a->device(), std::move(s)); }

Shape cobroadcast(const Shape& l, const Shape& r) {  // utils.rs:97-125
    const Shape& big = l.size() >= r.size() ? l : r;
    const Shape& small = l.size() >= r.size() ? r : l;
    Shape out = big;
    const size_t off = big.size() - small.size();
    for (size_t i = 0; i < small.size(); ++i) {
        int& o = out[off + i];
        if (o != small[i]) {
            if (o == 1) o = small[i];
            else if (small[i] != 1) panic("The two tensors have incompatible shape.");
        }
    }
    return out;
}

// ---- forward nodes -------------------------------------------------------------------------------
struct BinaryFwd : Forward {  // node/{addition,subtraction,multiplication,division}/mod.rs
    int op;
    Shared<HipArray> l, r, out;
    BinaryFwd(int op, Shared<HipArray> l, Shared<HipArray> r, Shared<HipArray> out)
        : op(op), l(std::move(l)), r(std::move(r)), out(std::move(out)) {}
    void forward() const override {
        check(nk_binary_fwd(D(out), op, out->ptr(), out->shape().data(), (int)out->shape().size(), l->ptr(),
                            l->shape().data(), (int)l->shape().size(), r->ptr(), r->shape().data(),
                            (int)r->shape().size()));
    }
};
struct BinaryBwd : Backward {  // <Op>Backward{Left,Right}; either side may be absent
    int op;
    Shared<Gradient> lg, rg, g;
    Shared<HipArray> l, r;
    void backward() const override {
        const HipArray& G = g->borrow();
        bool assign = false;
        if (lg) {
            HipArray& d = lg->borrow_first_write(assign);
            check((assign ? nk_binary_bwd_left_assign : nk_binary_bwd_left)(D(l), op, d.ptr(), d.shape().data(), (int)d.shape().size(), G.ptr(),
                                     G.shape().data(), (int)G.shape().size(), r->ptr(), r->shape().data(),
                                     (int)r->shape().size()));
        }
        if (rg) {
            HipArray& d = rg->borrow_first_write(assign);
            check((assign ? nk_binary_bwd_right_assign : nk_binary_bwd_right)(D(l), op, d.ptr(), d.shape().data(), (int)d.shape().size(), G.ptr(),
                                      G.shape().data(), (int)G.shape().size(), l->ptr(), l->shape().data(),
                                      (int)l->shape().size(), r->ptr()));
        }
    }
    void targets(std::vector<const Gradient*>& out) const override {
        if (lg) out.push_back(lg.get());
        if (rg) out.push_back(rg.get());
    }
};

// First-write access to a gradient: `beta` = 0 when its zero fill is still pending (the node assigns), 1 otherwise.
static float* first_write(const Shared<Gradient>& gr, float& beta) {
    bool assign = false;
    HipArray& d = gr->borrow_first_write(assign);
    beta = assign ? 0.f : 1.f;
    return d.ptr();
}

enum class Unary { Relu, Softmax, LogSoftmax, Transpose, Sum, Mean };
struct UnaryFwd : Forward {
    Unary kind;
    int axis;
    Shared<HipArray> x, y;
    UnaryFwd(Unary k, int axis, Shared<HipArray> x, Shared<HipArray> y) : kind(k), axis(axis), x(std::move(x)), y(std::move(y)) {}
    void forward() const override {
        const int nd = (int)x->shape().size();
        switch (kind) {
            case Unary::Relu: check(nk_relu_fwd(D(x), x->ptr(), y->ptr(), x->len())); break;
            case Unary::Softmax: check(nk_softmax_fwd(D(x), x->ptr(), y->ptr(), x->shape().data(), nd, axis)); break;
            case Unary::LogSoftmax: check(nk_log_softmax_fwd(D(x), x->ptr(), y->ptr(), x->shape().data(), nd, axis)); break;
            case Unary::Transpose: check(nk_transpose_fwd(D(x), x->ptr(), y->ptr(), x->shape().data(), nd)); break;
            case Unary::Sum: check(nk_sum_fwd(D(x), x->ptr(), x->len(), y->ptr())); break;
            case Unary::Mean: check(nk_mean_fwd(D(x), x->ptr(), x->len(), y->ptr())); break;
        }
    }
};
struct UnaryBwd : Backward {
    Unary kind;
    int axis;
    Shared<Gradient> dx, g;
    Shared<HipArray> x, y;  // ReLU needs the input, (log)softmax the output
    void backward() const override {
        const HipArray& G = g->borrow();
        if (kind == Unary::Relu || kind == Unary::Sum || kind == Unary::Mean) {
            bool assign = false;
            HipArray& d = dx->borrow_first_write(assign);
            if (kind == Unary::Relu) check((assign ? nk_relu_bwd_assign : nk_relu_bwd)(D(x), d.ptr(), G.ptr(), x->ptr(), d.len()));
            else if (kind == Unary::Sum) check((assign ? nk_sum_bwd_assign : nk_sum_bwd)(d.device()->raw(), d.ptr(), d.len(), G.ptr()));
            else check((assign ? nk_mean_bwd_assign : nk_mean_bwd)(d.device()->raw(), d.ptr(), d.len(), G.ptr()));
            return;
        }
        if (kind == Unary::Transpose) {
            bool assign = false;
            HipArray& d = dx->borrow_first_write(assign);
            check((assign ? nk_transpose_bwd_assign : nk_transpose_bwd)(d.device()->raw(), d.ptr(), G.ptr(), d.shape().data(), (int)d.shape().size()));
            return;
        }
        if (kind == Unary::Softmax || kind == Unary::LogSoftmax) {
            bool assign = false;
            HipArray& d = dx->borrow_first_write(assign);
            auto fn = kind == Unary::Softmax ? (assign ? nk_softmax_bwd_assign : nk_softmax_bwd)
                                             : (assign ? nk_log_softmax_bwd_assign : nk_log_softmax_bwd);
            check(fn(D(y), d.ptr(), G.ptr(), y->ptr(), d.shape().data(), (int)d.shape().size(), axis));
            return;
        }
        panic("UnaryBwd: unknown node kind");
    }
    void targets(std::vector<const Gradient*>& out) const override { out.push_back(dx.get()); }
};

// MatMul family.  kind: 0 = mm, 1 = mm_t, 2 = batched mm over [B,*,*] tiles, 3 = batched mm_t
struct MatMulFwd : Forward {
    int kind;
    Shared<HipArray> a, b, c;
    MatMulFwd(int kind, Shared<HipArray> a, Shared<HipArray> b, Shared<HipArray> c)
        : kind(kind), a(std::move(a)), b(std::move(b)), c(std::move(c)) {}
    void forward() const override {
        const Shape& as = a->shape();
        const Shape& bs = b->shape();
        if (kind == 0) check(nk_mm_fwd(D(a), a->ptr(), b->ptr(), c->ptr(), as[0], as[1], bs[1]));
        else if (kind == 4) check(nk_mv_fwd(D(a), a->ptr(), b->ptr(), c->ptr(), as[0], as[1]));
        else if (kind == 5) check(nk_vm_fwd(D(a), a->ptr(), b->ptr(), c->ptr(), bs[0], bs[1]));
        else if (kind == 6) check(nk_vv_fwd(D(a), a->ptr(), b->ptr(), a->len(), c->ptr()));
        else if (kind == 1) check(nk_mm_t_fwd(D(a), a->ptr(), b->ptr(), c->ptr(), as[0], as[1], bs[0]));
        else if (kind == 2)  // C[b] (n,o) = A[b] (n,m) . B[b] (m,o)
            check(nk_sgemm_batched(D(a), 0, 0, as[1], bs[2], as[2], 1.f, a->ptr(), as[2], (long long)as[1] * as[2], 0,
                                   b->ptr(), bs[2], (long long)bs[1] * bs[2], 0, 0.f, c->ptr(), bs[2],
                                   (long long)as[1] * bs[2], 0, as[0], 1));
        else  // C[b] (n,o) = A[b] (n,m) . B[b] (o,m)^T
            check(nk_sgemm_batched(D(a), 0, 1, as[1], bs[1], as[2], 1.f, a->ptr(), as[2], (long long)as[1] * as[2], 0,
                                   b->ptr(), bs[2], (long long)bs[1] * bs[2], 0, 0.f, c->ptr(), bs[1],
                                   (long long)as[1] * bs[1], 0, as[0], 1));
    }
};
struct MatMulBwd : Backward {
    int kind;
    Shared<HipArray> a, b;
    Shared<Gradient> da, db, g;  // da / db may be null
    void backward() const override {
        const HipArray& G = g->borrow();
        const Shape& as = a->shape();
        const Shape& bs = b->shape();
        nk_device* dev = D(a);
        if (kind == 4) {  // matrix_vector_mul/mod.rs:63-69, :92-102
            if (da) check(nk_mv_bwd_left(dev, da->borrow().ptr(), G.ptr(), b->ptr(), as[0], as[1]));
            if (db) check(nk_mv_bwd_right(dev, db->borrow().ptr(), a->ptr(), G.ptr(), as[0], as[1]));
        } else if (kind == 5) {  // vector_matrix_mul/mod.rs:63-73, :95-101
            if (da) check(nk_vm_bwd_left(dev, da->borrow().ptr(), b->ptr(), G.ptr(), bs[0], bs[1]));
            if (db) check(nk_vm_bwd_right(dev, db->borrow().ptr(), a->ptr(), G.ptr(), bs[0], bs[1]));
        } else if (kind == 6) {  // vector_vector_mul/mod.rs:57-63
            if (da) check(nk_vv_bwd(dev, da->borrow().ptr(), b->ptr(), G.ptr(), a->len()));
            if (db) check(nk_vv_bwd(dev, db->borrow().ptr(), a->ptr(), G.ptr(), a->len()));
        } else if (kind == 0) {  // = nk_mm_bwd_left / nk_mm_bwd_right with beta 0 on a first write
            const int n = as[0], m = as[1], o = bs[1];
            float beta;
            if (da && db && da != db) {  // MatrixMatrixMulBackward::backward: both products as one call (one launch at small sizes)
                float beta_b;
                float* d = first_write(da, beta);
                float* e = first_write(db, beta_b);
                check(nk_mm_bwd(dev, d, e, G.ptr(), a->ptr(), b->ptr(), n, m, o, beta == 0.f, beta_b == 0.f));
                return;
            }
            if (da) { float* d = first_write(da, beta); check(nk_sgemm(dev, 0, 1, n, m, o, 1.f, G.ptr(), o, b->ptr(), o, beta, d, m)); }
            if (db) { float* d = first_write(db, beta); check(nk_sgemm(dev, 1, 0, m, o, n, 1.f, a->ptr(), m, G.ptr(), o, beta, d, o)); }
        } else if (kind == 1) {  // = nk_mm_t_bwd_left / nk_mm_t_bwd_right
            const int n = as[0], m = as[1], o = bs[0];
            float beta;
            if (da && db && da != db) {  // MatrixMatrixMulTBackward::backward as one call
                float beta_b;
                float* d = first_write(da, beta);
                float* e = first_write(db, beta_b);
                check(nk_mm_t_bwd(dev, d, e, G.ptr(), a->ptr(), b->ptr(), n, m, o, beta == 0.f, beta_b == 0.f));
                return;
            }
            if (da) { float* d = first_write(da, beta); check(nk_sgemm(dev, 0, 0, n, m, o, 1.f, G.ptr(), o, b->ptr(), m, beta, d, m)); }
            if (db) { float* d = first_write(db, beta); check(nk_sgemm(dev, 1, 0, o, m, n, 1.f, G.ptr(), o, a->ptr(), m, beta, d, m)); }
        } else if (kind == 2) {
            const int B = as[0], n = as[1], m = as[2], o = bs[2];
            float beta;
            if (da) {  // dA[b] += G[b] . B[b]^T
                float* d = first_write(da, beta);
                check(nk_sgemm_batched(dev, 0, 1, n, m, o, 1.f, G.ptr(), o, (long long)n * o, 0, b->ptr(), o,
                                       (long long)m * o, 0, beta, d, m, (long long)n * m, 0, B, 1));
            }
            if (db) {  // dB[b] += A[b]^T . G[b]
                float* d = first_write(db, beta);
                check(nk_sgemm_batched(dev, 1, 0, m, o, n, 1.f, a->ptr(), m, (long long)n * m, 0, G.ptr(), o,
                                       (long long)n * o, 0, beta, d, o, (long long)m * o, 0, B, 1));
            }
        } else {
            const int B = as[0], n = as[1], m = as[2], o = bs[1];
            float beta;
            if (da) {  // dA[b] += G[b] . B[b]
                float* d = first_write(da, beta);
                check(nk_sgemm_batched(dev, 0, 0, n, m, o, 1.f, G.ptr(), o, (long long)n * o, 0, b->ptr(), m,
                                       (long long)o * m, 0, beta, d, m, (long long)n * m, 0, B, 1));
            }
            if (db) {  // dB[b] += G[b]^T . A[b]
                float* d = first_write(db, beta);
                check(nk_sgemm_batched(dev, 1, 0, o, m, n, 1.f, G.ptr(), o, (long long)n * o, 0, a->ptr(), m,
                                       (long long)n * m, 0, beta, d, m, (long long)o * m, 0, B, 1));
            }
        }
    }
    void targets(std::vector<const Gradient*>& out) const override {
        if (da) out.push_back(da.get());
        if (db) out.push_back(db.get());
    }
};

struct ConvFwd : Forward {  // node/convolution/mod.rs:296-355 (+ the module's broadcast bias Addition when b is set)
    Shared<HipArray> x, w, b, y;
    std::vector<int> stride, dilation;
    std::vector<int> fold;  // module node with its Zero padding folded in: x is the UNPADDED input (nk_conv_bias_fwd_padded)
    int groups;
    void forward() const override {
        const int nd = (int)x->shape().size() - 2;
        if (!fold.empty())
            check(nk_conv_bias_fwd_padded(D(x), nd, x->ptr(), x->shape().data(), fold.data(), w->ptr(), w->shape().data(), b ? b->ptr() : nullptr,
                                          y->ptr(), stride.data(), dilation.data(), groups));
        else if (b)
            check(nk_conv_bias_fwd(D(x), nd, x->ptr(), x->shape().data(), w->ptr(), w->shape().data(), b->ptr(), y->ptr(),
                                   stride.data(), dilation.data(), groups));
        else
            check(nk_conv_fwd(D(x), nd, x->ptr(), x->shape().data(), w->ptr(), w->shape().data(), y->ptr(), stride.data(),
                              dilation.data(), groups));
    }
};
struct ConvBwd : Backward {  // ConvolutionBackward{Input,Kernel}  :357-510
    Shared<HipArray> x, w;
    Shared<Gradient> dx, dw, db, g;  // dx may be null (input is a non-differentiable Var); db only for the fused module node
    std::vector<int> stride, dilation;
    std::vector<int> padding;  // fused module node with Zero padding: x is the padded input, dx the UNPADDED input's gradient
    bool x_unpadded = false;   // ... and with the padding folded into forward and kernel gradient too: x is the UNPADDED input
    int groups;
    void backward() const override {
        const HipArray& G = g->borrow();
        const int nd = (int)x->shape().size() - 2;
        bool assign = false;
        if (dx) {
            HipArray& d = dx->borrow_first_write(assign);
            if (!padding.empty())  // ConvolutionBackwardInput + PadBackward in one kernel
                check((assign ? nk_conv_bwd_input_padded_assign : nk_conv_bwd_input_padded)(
                    D(x), nd, d.ptr(), d.shape().data(), padding.data(), G.ptr(), w->ptr(), w->shape().data(), stride.data(),
                    dilation.data(), groups));
            else
                check((assign ? nk_conv_bwd_input_assign : nk_conv_bwd_input)(D(x), nd, d.ptr(), x->shape().data(), G.ptr(), w->ptr(),
                                                                              w->shape().data(), stride.data(), dilation.data(), groups));
        }
        if (dw && x_unpadded) {  // the Pad node folded into the kernel-gradient pass (db optional)
            bool assign_b = false;
            HipArray& d = dw->borrow_first_write(assign);
            HipArray* b = db ? &db->borrow_first_write(assign_b) : nullptr;
            check(nk_conv_bwd_kernel_bias_padded(D(x), nd, d.ptr(), b ? b->ptr() : nullptr, w->shape().data(), G.ptr(), x->ptr(), x->shape().data(),
                                                 padding.data(), stride.data(), dilation.data(), groups, assign ? 1 : 0, assign_b ? 1 : 0));
        } else if (dw && db) {  // kernel and bias gradient of the fused module node in one pass over G
            bool assign_b = false;
            HipArray& d = dw->borrow_first_write(assign);
            HipArray& b = db->borrow_first_write(assign_b);
            check(nk_conv_bwd_kernel_bias(D(x), nd, d.ptr(), b.ptr(), w->shape().data(), G.ptr(), x->ptr(), x->shape().data(), stride.data(),
                                          dilation.data(), groups, assign ? 1 : 0, assign_b ? 1 : 0));
        } else if (dw) {
            HipArray& d = dw->borrow_first_write(assign);
            check((assign ? nk_conv_bwd_kernel_assign : nk_conv_bwd_kernel)(D(x), nd, d.ptr(), w->shape().data(), G.ptr(), x->ptr(),
                                                                            x->shape().data(), stride.data(), dilation.data(), groups));
        } else if (db) {  // AdditionBackwardRight of the bias: sum of G over every axis the (Cout,1,..) bias lacks
            HipArray& d = db->borrow_first_write(assign);
            check((assign ? nk_unbroadcast_assign : nk_unbroadcast_add)(D(x), d.ptr(), d.shape().data(), (int)d.shape().size(), G.ptr(),
                                                                        G.shape().data(), (int)G.shape().size()));
        }
    }
    void targets(std::vector<const Gradient*>& out) const override {
        if (dx) out.push_back(dx.get());
        if (dw) out.push_back(dw.get());
        if (db) out.push_back(db.get());
    }
};

struct PadFwd : Forward {
    Shared<HipArray> x, y;
    std::vector<int> padding;
    PaddingMode mode;
    void forward() const override {
        const int nd = (int)x->shape().size() - 2;
        switch (mode.kind) {
            case PaddingMode::Reflective:
                check(nk_pad_reflective_fwd(D(x), nd, x->ptr(), x->shape().data(), y->ptr(), padding.data()));
                break;
            case PaddingMode::Replicative:
                check(nk_pad_replicative_fwd(D(x), nd, x->ptr(), x->shape().data(), y->ptr(), padding.data()));
                break;
            default:
                check(nk_pad_const_fwd(D(x), nd, x->ptr(), x->shape().data(), y->ptr(), padding.data(), mode.value));
        }
    }
};
struct PadBwd : Backward {
    Shared<Gradient> dx, g;
    std::vector<int> padding;
    void backward() const override {
        bool assign = false;
        HipArray& d = dx->borrow_first_write(assign);
        check((assign ? nk_pad_bwd_assign : nk_pad_bwd)(d.device()->raw(), (int)d.shape().size() - 2, d.ptr(), d.shape().data(),
                                                        g->borrow().ptr(), padding.data()));
    }
    void targets(std::vector<const Gradient*>& out) const override { out.push_back(dx.get()); }
};

struct DropoutFwd : Forward {  // node/dropout/mod.rs:17-79
    Shared<HipArray> x, y, noise;
    double p;
    Shared<bool> status;
    uint64_t seed;
    Shared<uint64_t> calls;  // Philox offset advances on every forward (noise is resampled)
    void forward() const override {
        const uint64_t offset = (*calls) * ((x->len() + 7) / 8);  // 8 draws per Philox call (nk_common.h)
        check(nk_dropout_fwd(D(x), x->ptr(), y->ptr(), noise->ptr(), x->len(), p, *status ? 1 : 0, seed, offset));
        ++(*calls);  // only a forward that was issued consumes its Philox range (a refused capture throws above)
    }
};
struct DropoutBwd : Backward {
    Shared<Gradient> dx, g;
    Shared<HipArray> noise;
    double p;
    Shared<bool> status;
    void backward() const override {
        bool assign = false;
        HipArray& d = dx->borrow_first_write(assign);
        check((assign ? nk_dropout_bwd_assign : nk_dropout_bwd)(d.device()->raw(), d.ptr(), g->borrow().ptr(), noise->ptr(), d.len(), p,
                                                                *status ? 1 : 0));
    }
    void targets(std::vector<const Gradient*>& out) const override { out.push_back(dx.get()); }
};

// Fused attention probabilities: Multiplication(scalar) + Softmax(last axis) + Dropout
struct AttnProbsFwd : Forward {
    Shared<HipArray> x, probs, out;
    float scale;
    double p;
    Shared<bool> status;
    uint64_t seed;
    Shared<uint64_t> calls, last_offset;  // the backward node regenerates the mask of the LAST forward
    void forward() const override {
        const int L = x->shape().back();
        const long long rows = (long long)(x->len() / (size_t)L);
        const uint64_t offset = (*calls) * ((x->len() + 7) / 8);  // 8 draws per Philox call (nk_common.h)
        *last_offset = offset;
        check(nk_scale_softmax_dropout_fwd(D(x), x->ptr(), probs ? probs->ptr() : nullptr, out->ptr(), nullptr, rows, L, scale, p,
                                           *status ? 1 : 0, seed, offset));
        ++(*calls);  // only a forward that was issued consumes its Philox range (a refused capture throws above)
    }
};
struct AttnProbsBwd : Backward {
    Shared<Gradient> dx, g;
    Shared<HipArray> probs, scores;  // probs null: recomputed from the scores (the forward did not store them)
    float scale;
    double p;
    Shared<bool> status;
    uint64_t seed;
    Shared<uint64_t> last_offset;
    void backward() const override {
        bool assign = false;
        HipArray& d = dx->borrow_first_write(assign);
        const int L = d.shape().back();
        const long long rows = (long long)(d.len() / (size_t)L);
        if (!probs)
            check(nk_scale_softmax_dropout_bwd_from_scores(d.device()->raw(), d.ptr(), g->borrow().ptr(), scores->ptr(), nullptr, rows, L,
                                                           scale, p, *status ? 1 : 0, seed, *last_offset, assign ? 1 : 0));
        else
            check((assign ? nk_scale_softmax_dropout_bwd_assign : nk_scale_softmax_dropout_bwd)(d.device()->raw(), d.ptr(), g->borrow().ptr(), probs->ptr(), nullptr,
                                               rows, L, scale, p, *status ? 1 : 0, seed, *last_offset));
    }
    void targets(std::vector<const Gradient*>& out) const override { out.push_back(dx.get()); }
};

// Pointwise unary nodes: node/{negation,exp,logn,sqrt,sigmoid,tanh,softplus,leaky_relu,power}
struct PointwiseFwd : Forward {
    int op, iparam;
    Shared<HipArray> x, y;
    void forward() const override { check(nk_unary_fwd(D(x), op, x->ptr(), y->ptr(), x->len(), iparam)); }
};
struct PointwiseBwd : Backward {
    int op, iparam;
    Shared<Gradient> dx, g;
    Shared<HipArray> ref;  // the buffer the reference node keeps: operand data or node data
    void backward() const override {
        bool assign = false;
        HipArray& d = dx->borrow_first_write(assign);
        check((assign ? nk_unary_bwd_assign : nk_unary_bwd)(d.device()->raw(), op, d.ptr(), g->borrow().ptr(), ref ? ref->ptr() : nullptr,
                                                            d.len(), iparam));
    }
    void targets(std::vector<const Gradient*>& out) const override { out.push_back(dx.get()); }
};
// Unsqueeze: node/unsqueeze/mod.rs:35-40 (copy into the reshaped buffer), :70-78 (dx += g)
struct UnsqueezeFwd : Forward {
    Shared<HipArray> x, y;
    void forward() const override { check(nk_copy(D(x), y->ptr(), x->ptr(), x->len())); }
};
struct UnsqueezeBwd : Backward {
    Shared<Gradient> dx, g;
    void backward() const override {
        HipArray& d = dx->borrow();
        const int n = (int)d.len();
        check(nk_unbroadcast_add(d.device()->raw(), d.ptr(), &n, 1, g->borrow().ptr(), &n, 1));
    }
    void targets(std::vector<const Gradient*>& out) const override { out.push_back(dx.get()); }
};

struct ChunkFwd : Forward {
    Shared<HipArray> x, y;
    int chunk_no;
    void forward() const override {
        check(nk_chunk_fwd(D(x), x->ptr(), x->shape().data(), y->ptr(), y->shape().data(), (int)x->shape().size(), chunk_no));
    }
};
struct ChunkBwd : Backward {
    Shared<Gradient> dx, g;
    int chunk_no;
    void backward() const override {
        HipArray& d = dx->borrow();
        const HipArray& G = g->borrow();
        check(nk_chunk_bwd(d.device()->raw(), d.ptr(), d.shape().data(), G.ptr(), G.shape().data(), (int)d.shape().size(), chunk_no));
    }
    void targets(std::vector<const Gradient*>& out) const override { out.push_back(dx.get()); }
};

struct CatFwd : Forward {  // node/multi_concatenate/mod.rs
    std::vector<Shared<HipArray>> operands;
    Shared<HipArray> out;
    int axis;
    bool stack = false;  // node/multi_stack/mod.rs:37-47: every operand fills one index of a NEW axis
    void forward() const override {
        int off = 0;
        for (const auto& o : operands) {
            const int len = stack ? 1 : o->shape()[axis];
            check(nk_concat_fwd_part(D(out), o->ptr(), out->ptr(), out->shape().data(), (int)out->shape().size(), axis, off, len));
            off += len;
        }
    }
};
struct CatBwd : Backward {
    std::vector<Shared<Gradient>> operands;
    Shared<Gradient> g;
    int axis;
    bool stack = false;  // node/multi_stack/mod.rs:76-86
    void backward() const override {
        const HipArray& G = g->borrow();
        int off = 0;
        for (const auto& o : operands) {
            bool assign = false;
            HipArray& d = o->borrow_first_write(assign);
            const int len = stack ? 1 : d.shape()[axis];
            check((assign ? nk_concat_bwd_part_assign : nk_concat_bwd_part)(d.device()->raw(), d.ptr(), G.ptr(), G.shape().data(), (int)G.shape().size(), axis, off, len));
            off += len;
        }
    }
    void targets(std::vector<const Gradient*>& out) const override {
        for (const auto& o : operands) out.push_back(o.get());
    }
};

struct HeadsFwd : Forward {
    bool split;
    Shared<HipArray> x, y;
    int B, S, H, dh;
    void forward() const override {
        check(split ? nk_split_heads_fwd(D(x), x->ptr(), y->ptr(), B, S, H, dh) : nk_merge_heads_fwd(D(x), x->ptr(), y->ptr(), B, S, H, dh));
    }
};
struct HeadsBwd : Backward {
    bool split;
    Shared<Gradient> dx, g;
    int B, S, H, dh;
    void backward() const override {
        bool assign = false;
        HipArray& d = dx->borrow_first_write(assign);
        auto fn = split ? (assign ? nk_split_heads_bwd_assign : nk_split_heads_bwd)
                        : (assign ? nk_merge_heads_bwd_assign : nk_merge_heads_bwd);
        check(fn(d.device()->raw(), d.ptr(), g->borrow().ptr(), B, S, H, dh));
    }
    void targets(std::vector<const Gradient*>& out) const override { out.push_back(dx.get()); }
};

struct MseFwd : Forward {  // node/squared_error/mod.rs:42-59
    Shared<HipArray> x, t, out;
    Reduction red;
    void forward() const override { check(nk_mse_fwd(D(x), x->ptr(), t->ptr(), x->len(), (int)red, out->ptr())); }
};
struct MseBwd : Backward {
    Shared<HipArray> x, t;
    Shared<Gradient> dx, g;
    Reduction red;
    void backward() const override {
        bool assign = false;
        HipArray& d = dx->borrow_first_write(assign);
        check((assign ? nk_mse_bwd_assign : nk_mse_bwd)(D(x), d.ptr(), g->borrow().ptr(), x->ptr(), t->ptr(), x->len(), (int)red));
    }
    void targets(std::vector<const Gradient*>& out) const override { out.push_back(dx.get()); }
};

// Per-(batch, head) attention products on the (B*S, H*dh) projection layout: the B*H Chunk((S,dh)) tiles of the composed
// module (SURVEY 8a note) are addressed as strided GEMM operands instead of being copied out and back.
struct HeadsGeom {
    int B, S, H, dh;
    int d() const { return H * dh; }
    long long so() const { return (long long)S * H * dh; }  // sample stride in the flat layout
    long long po() const { return (long long)H * S * S; }   // sample stride of the (B*H, S, S) tensor
    long long pi() const { return (long long)S * S; }
};
struct HeadsScoresFwd : Forward {  // C_bh(S,S) = Q_bh(S,dh) . K_bh(S,dh)^T
    HeadsGeom hg;
    Shared<HipArray> q, k, c;
    void forward() const override {
        check(nk_sgemm_batched(D(q), 0, 1, hg.S, hg.S, hg.dh, 1.f, q->ptr(), hg.d(), hg.so(), hg.dh, k->ptr(), hg.d(), hg.so(), hg.dh, 0.f,
                               c->ptr(), hg.S, hg.po(), hg.pi(), hg.B, hg.H));
    }
};
struct HeadsScoresBwd : Backward {
    HeadsGeom hg;
    Shared<HipArray> q, k;
    Shared<Gradient> dq, dk, g;
    void backward() const override {
        const HipArray& G = g->borrow();
        nk_device* dev = D(q);
        float beta;
        {   // dQ_bh += G_bh . K_bh      (every element of dQ belongs to exactly one head block: a first write may assign)
            float* d = first_write(dq, beta);
            check(nk_sgemm_batched(dev, 0, 0, hg.S, hg.dh, hg.S, 1.f, G.ptr(), hg.S, hg.po(), hg.pi(), k->ptr(), hg.d(), hg.so(), hg.dh, beta,
                                   d, hg.d(), hg.so(), hg.dh, hg.B, hg.H));
        }
        {   // dK_bh += G_bh^T . Q_bh
            float* d = first_write(dk, beta);
            check(nk_sgemm_batched(dev, 1, 0, hg.S, hg.dh, hg.S, 1.f, G.ptr(), hg.S, hg.po(), hg.pi(), q->ptr(), hg.d(), hg.so(), hg.dh, beta,
                                   d, hg.d(), hg.so(), hg.dh, hg.B, hg.H));
        }
    }
    void targets(std::vector<const Gradient*>& out) const override { out.push_back(dq.get()); out.push_back(dk.get()); }
};
struct HeadsContextFwd : Forward {  // O_bh(S,dh) = P_bh(S,S) . V_bh(S,dh), written into the flat layout
    HeadsGeom hg;
    Shared<HipArray> p, v, o;
    void forward() const override {
        check(nk_sgemm_batched(D(p), 0, 0, hg.S, hg.dh, hg.S, 1.f, p->ptr(), hg.S, hg.po(), hg.pi(), v->ptr(), hg.d(), hg.so(), hg.dh, 0.f,
                               o->ptr(), hg.d(), hg.so(), hg.dh, hg.B, hg.H));
    }
};
struct HeadsContextBwd : Backward {
    HeadsGeom hg;
    Shared<HipArray> p, v;
    Shared<Gradient> dp, dv, g;
    void backward() const override {
        const HipArray& G = g->borrow();  // dO, flat layout
        nk_device* dev = D(p);
        float beta;
        {   // dP_bh += dO_bh . V_bh^T
            float* d = first_write(dp, beta);
            check(nk_sgemm_batched(dev, 0, 1, hg.S, hg.S, hg.dh, 1.f, G.ptr(), hg.d(), hg.so(), hg.dh, v->ptr(), hg.d(), hg.so(), hg.dh, beta,
                                   d, hg.S, hg.po(), hg.pi(), hg.B, hg.H));
        }
        {   // dV_bh += P_bh^T . dO_bh
            float* d = first_write(dv, beta);
            check(nk_sgemm_batched(dev, 1, 0, hg.S, hg.dh, hg.S, 1.f, p->ptr(), hg.S, hg.po(), hg.pi(), G.ptr(), hg.d(), hg.so(), hg.dh, beta,
                                   d, hg.d(), hg.so(), hg.dh, hg.B, hg.H));
        }
    }
    void targets(std::vector<const Gradient*>& out) const override { out.push_back(dp.get()); out.push_back(dv.get()); }
};

// S <= window: the band is the whole triangle, every path as without a window (the causal kernels as they are)
int band_of(int window, int S) { return window > 0 && S > window ? window : 0; }
// The banded scratch of the sliding-window core, sized by the library's three geometry functions and allocated WITHOUT a fill: the
// kernels define every element they read, and an O(S * ld) memset per graph would be pure loss.
struct BandScratch { Shape scores, mask; };
BandScratch band_scratch(int B, int S, int H, int window) {
    const size_t ext = nk_attention_band_scratch(S, window), words = nk_attention_band_mask_words(S, window);
    if (ext > 0x7fffffffu || words > 0x7fffffffu) panic("heads_attention: the banded scratch of one head exceeds 2^31 elements");
    return {Shape{B * H, (int)ext}, Shape{B * H, (int)words}};
}
Shared<HipArray> uninit_like(const Shared<HipArray>& a, Shape s) { return std::make_shared<HipArray>(a->device(), std::move(s), HipArray::Uninit{}); }

// What a causal form refuses, worded once for the two callers that refuse it under their own name.
struct FormRefusals {
    const char* who;
    bool causal;
    void window(int w) const {
        if (w < 0) panic(std::string(who) + ": window must not be negative, got " + std::to_string(w));
        if (w > 0 && !causal) panic(std::string(who) + ": a sliding window is a band of the CAUSAL triangle: set causal = true");
    }
    void segments(const nn::Segments* s, int B, int S, const Device* dev) const {
        if (s && !causal) panic(std::string(who) + ": segments are blocks of the CAUSAL triangle: set causal = true");
        if (s && (s->batch != B || s->S != S))
            panic(std::string(who) + ": the segments were built for (batch " + std::to_string(s->batch) + ", S " + std::to_string(s->S) + "), the call has (" +
                  std::to_string(B) + ", " + std::to_string(S) + ")");
        if (s && s->lo->device().get() != dev) panic(std::string(who) + ": the segments live on another device");
    }
};

// One call of the fused attention core, heads_scores -> attention_probs -> heads_context as one launch sequence (nk_attention_* on
// three operands, nk_attention_qkv_* on the packed buffer): the form, the dropout stream and the scratch.  The forward and the
// backward node of a graph hold copies of ONE description, so the arrays and `calls` are shared between them.
struct AttnCore {
    HeadsGeom hg;
    float scale = 0.f;
    double p = 0.0;
    Shared<bool> status;
    uint64_t seed = 0;
    Shared<uint64_t> calls;  // each forward draws a fresh mask (the Philox offset advances), as AttnProbsFwd
    bool causal = false;     // nk_attention_causal_*: query r attends to keys <= r (same draws, same offset advance)
    int span = 0;            // > 0: nk_attention_band_*, query r attends to keys r - span < k <= r; scores / mask are the banded scratch
    Shared<HipArray> lo;     // (B, S) int32 left edges: nk_attention_seg_* with `span`, which sizes the same scratch
    // mask: the dropout draws, 1 bit per score (u32 words in an f32 array).  All three are null in the dense form of a graph without
    // gradients: nothing is kept, no (B*H, S, S) tensor exists.  The band keeps its state in every graph.
    Shared<HipArray> scores, stats, mask;
    Shared<HipArray> ds, dropped;  // backward only: scratch of the extent of `scores`, written by the first kernel, read by the dK / dV products

    // Every decision about the form and its scratch.  `like` gives the device; keep: a backward node will read the state.
    static AttnCore build(const Shared<HipArray>& like, int B, int S, int H, int dh, float scale, double p, Shared<bool> status, bool causal,
                          int window, const nn::Segments* segments, bool keep) {
        AttnCore c;
        c.hg = {B, S, H, dh}; c.scale = scale; c.p = p; c.status = std::move(status); c.causal = causal;
        c.span = band_of(window, S);
        // one document per sample is the call without segments; otherwise the seg kernels on the band's scratch for span = min(max_len, window)
        if (segments && segments->max_len < S) {
            c.span = c.span ? std::min(c.span, segments->max_len) : segments->max_len;
            c.lo = segments->lo;
        }
        const int SP = (S + 31) / 32 * 32;  // the scratch tensors are padded to whole 32 x 32 tiles (include/neuronika_hip.h)
        if (c.span) {
            const BandScratch bs = band_scratch(B, S, H, c.span);
            c.scores = uninit_like(like, bs.scores);
            c.stats = uninit_like(like, Shape{B * H, SP, 2});
            c.mask = uninit_like(like, bs.mask);
        } else if (keep) {
            c.scores = zeros_like(like, Shape{B * H, SP, SP});
            c.stats = zeros_like(like, Shape{B * H, SP, 2});
            c.mask = zeros_like(like, Shape{B * H, SP, SP / 32});
        }
        c.seed = next_node_seed();
        c.calls = std::make_shared<uint64_t>(0);
        return c;
    }
    // the second step of a differentiable graph: the banded kernels define what they read, the dense ones want zeros
    void add_backward_scratch() {
        ds = (span ? uninit_like : zeros_like)(scores, scores->shape());
        dropped = (span ? uninit_like : zeros_like)(scores, scores->shape());
    }

    // q, k, v: the (B*S, H*dh) operands; k == null: q is the packed (B*S, 3 H*dh) buffer
    void forward(nk_device* dev, const float* q, const float* k, const float* v, float* o) const {
        const uint64_t sp = ((uint64_t)hg.S + 31) / 32 * 32;  // the draws are indexed in the padded (B*H, SP, SP) tensor (SP = S unless S is ragged)
        const uint64_t offset = (*calls) * (((uint64_t)hg.B * hg.H * sp * sp + 7) / 8);  // draws per forward, 8 per Philox call
        const int* edges = lo ? reinterpret_cast<const int*>(lo->ptr()) : nullptr;
        float *sc = scores ? scores->ptr() : nullptr, *st = stats ? stats->ptr() : nullptr;
        uint32_t* mk = mask ? reinterpret_cast<uint32_t*>(mask->ptr()) : nullptr;
        const int B = hg.B, S = hg.S, H = hg.H, dh = hg.dh, train = *status ? 1 : 0;
        if (lo)
            check(k ? nk_attention_seg_fwd(dev, q, k, v, edges, sc, st, mk, o, B, S, H, dh, span, scale, p, train, seed, offset)
                    : nk_attention_qkv_seg_fwd(dev, q, edges, sc, st, mk, o, B, S, H, dh, span, scale, p, train, seed, offset));
        else if (span > 0)
            check(k ? nk_attention_band_fwd(dev, q, k, v, sc, st, mk, o, B, S, H, dh, scale, p, train, seed, offset, span)
                    : nk_attention_qkv_band_fwd(dev, q, sc, st, mk, o, B, S, H, dh, scale, p, train, seed, offset, span));
        else if (k)
            check((causal ? nk_attention_causal_fwd : nk_attention_fwd)(dev, q, k, v, sc, st, mk, o, B, S, H, dh, scale, p, train, seed, offset));
        else
            check((causal ? nk_attention_qkv_causal_fwd : nk_attention_qkv_fwd)(dev, q, sc, st, mk, o, B, S, H, dh, scale, p, train, seed, offset));
        ++(*calls);  // only a forward that was issued consumes its Philox range (a refused capture throws above)
    }
    void forward(nk_device* dev, const float* qkv, float* o) const { forward(dev, qkv, nullptr, nullptr, o); }

    // dS and Pd are written by the fused kernel, dQ comes out of it; dK / dV are the two batched products on dS / Pd.
    // k == null: dq is the packed (B*S, 3 H*dh) gradient, q the packed buffer and aq the one assign flag.
    void backward(nk_device* dev, float* dq, float* dk, float* dv, const float* dO, const float* o, const float* q, const float* k, const float* v,
                  int aq, int ak, int av) const {
        const int* edges = lo ? reinterpret_cast<const int*>(lo->ptr()) : nullptr;
        float *s = ds->ptr(), *pd = dropped->ptr();
        const float *sc = scores->ptr(), *st = stats->ptr();
        const uint32_t* mk = reinterpret_cast<const uint32_t*>(mask->ptr());
        const int B = hg.B, S = hg.S, H = hg.H, dh = hg.dh, train = *status ? 1 : 0;
        if (lo)
            check(k ? nk_attention_seg_bwd(dev, dq, dk, dv, s, pd, dO, o, sc, st, mk, q, k, v, edges, B, S, H, dh, span, scale, p, train, aq, ak, av)
                    : nk_attention_qkv_seg_bwd(dev, dq, s, pd, dO, o, sc, st, mk, q, edges, B, S, H, dh, span, scale, p, train, aq));
        else if (span > 0)
            check(k ? nk_attention_band_bwd(dev, dq, dk, dv, s, pd, dO, o, sc, st, mk, q, k, v, B, S, H, dh, scale, p, train, aq, ak, av, span)
                    : nk_attention_qkv_band_bwd(dev, dq, s, pd, dO, o, sc, st, mk, q, B, S, H, dh, scale, p, train, aq, span));
        else if (k)
            check((causal ? nk_attention_causal_bwd : nk_attention_bwd)(dev, dq, dk, dv, s, pd, dO, o, sc, st, mk, q, k, v, B, S, H, dh, scale, p, train,
                                                                        aq, ak, av));
        else
            check((causal ? nk_attention_qkv_causal_bwd : nk_attention_qkv_bwd)(dev, dq, s, pd, dO, o, sc, st, mk, q, B, S, H, dh, scale, p, train, aq));
    }
    void backward(nk_device* dev, float* dqkv, const float* dO, const float* o, const float* qkv) const {
        backward(dev, dqkv, nullptr, nullptr, dO, o, qkv, nullptr, nullptr, 1, 0, 0);
    }
};

// the core on three projections in the flat layout
struct HeadsAttentionFwd : Forward {
    AttnCore core;
    Shared<HipArray> q, k, v, o;
    void forward() const override { core.forward(D(q), q->ptr(), k->ptr(), v->ptr(), o->ptr()); }
};
struct HeadsAttentionBwd : Backward {
    AttnCore core;
    Shared<HipArray> q, k, v, o;
    Shared<Gradient> dq, dk, dv, g;
    void backward() const override {
        const HipArray& G = g->borrow();  // dO, flat layout
        float bq, bk, bv;
        float* gq = first_write(dq, bq);
        float* gk = first_write(dk, bk);
        float* gv = first_write(dv, bv);
        core.backward(D(q), gq, gk, gv, G.ptr(), o->ptr(), q->ptr(), k->ptr(), v->ptr(), bq == 0.f ? 1 : 0, bk == 0.f ? 1 : 0, bv == 0.f ? 1 : 0);
    }
    void targets(std::vector<const Gradient*>& out) const override {
        out.push_back(dq.get()); out.push_back(dk.get()); out.push_back(dv.get());
    }
};

// The geometry of one rotary launch (nk_rope_*), shared by the rope node and the attention nodes that rotate Q and K in place.
struct RopeGeom {
    int B = 0, T = 0, NH = 0, dh = 0, rot = 0, max_pos = 0, interleaved = 0;
};
static RopeGeom rope_geom(const nn::RotaryEmbedding& r, int B, int T, int NH) {
    RopeGeom g;
    g.B = B; g.T = T; g.NH = NH; g.dh = r.head_dim; g.rot = r.rot; g.max_pos = r.max_pos; g.interleaved = r.interleaved ? 1 : 0;
    return g;
}
// in place over `NH` heads from column 0 of a buffer with row stride ld; start: device int32[B] or null
static void rope_inplace(nk_device* dev, float* x, int ld, const Shared<HipArray>& table, const int* start, const RopeGeom& g, bool inverse) {
    if (inverse) check(nk_rope_bwd_assign(dev, x, ld, x, ld, table->ptr(), start, g.B, g.T, g.NH, g.dh, g.rot, g.max_pos, g.interleaved));
    else check(nk_rope_fwd(dev, x, ld, x, ld, table->ptr(), start, g.B, g.T, g.NH, g.dh, g.rot, g.max_pos, g.interleaved));
}

// nn::MultiheadAttention with PACKED projections: x -> [Q | K | V] = x . [Wq; Wk; Wv]^T + [bq; bk; bv] (ONE GEMM, N = 3d) -> the
// fused attention core reading Q, K, V as column blocks of that output -> context.  One forward and one backward node for what
// the unpacked module runs as three Linear nodes + the attention node (same values bit for bit in the forward; the backward's
// input gradient is one K = 3d chain instead of three K = d chains added up).
struct QkvAttentionFwd : Forward {
    AttnCore core;
    Shared<HipArray> x, w, b, qkv, o;  // w (3d, d), b (3d): the packed storage; qkv (B*S, 3d)
    Shared<HipArray> rope;  // the rotary table or null; rg: 2 H heads over the Q|K blocks
    RopeGeom rg;
    Shared<HipArray> rope_start;  // packed sequences: one position per row (rg.B = B*S, rg.T = 1)
    void forward() const override {
        const int n = core.hg.B * core.hg.S, d = core.hg.d();
        check(nk_linear_fwd(D(x), x->ptr(), w->ptr(), b->ptr(), qkv->ptr(), n, d, 3 * d));
        if (rope) rope_inplace(D(x), qkv->ptr(), 3 * d, rope, rope_start ? reinterpret_cast<const int*>(rope_start->ptr()) : nullptr, rg, false);
        core.forward(D(x), qkv->ptr(), o->ptr());
    }
};
struct QkvAttentionBwd : Backward {
    AttnCore core;
    Shared<HipArray> x, w, qkv, o;
    Shared<HipArray> dqkv;               // scratch owned by the node: (B*S, 3d)
    Shared<HipArray> gw_all, gb_all;     // packed gradient storage: (3d, d), (3d)
    Shared<Gradient> dx, gw[3], gb[3], g;  // dx null for a non-differentiable input; gw / gb: views of gw_all / gb_all
    Shared<HipArray> rope;  // as in the forward node: [dQ | dK] of the rotated rows go back through R^T in place
    RopeGeom rg;
    Shared<HipArray> rope_start;
    // the three views are written by ONE kernel: it may assign only when all three still wait for their zero fill
    static float packed_beta(const Shared<Gradient> (&v)[3]) {
        bool all = true;
        for (const auto& q : v) all = all && q->zero_pending();
        bool assign = false;
        for (const auto& q : v) {
            if (all) (void)q->borrow_first_write(assign);  // hands the pending fill to the kernel below (beta = 0)
            else (void)q->borrow();                        // materialises a pending view, the kernel accumulates
        }
        return all ? 0.f : 1.f;
    }
    void backward() const override {
        const HipArray& G = g->borrow();  // dO (B*S, d)
        nk_device* dev = D(x);
        const int n = core.hg.B * core.hg.S, d = core.hg.d();
        core.backward(dev, dqkv->ptr(), G.ptr(), o->ptr(), qkv->ptr());
        if (rope) rope_inplace(dev, dqkv->ptr(), 3 * d, rope, rope_start ? reinterpret_cast<const int*>(rope_start->ptr()) : nullptr, rg, true);
        float beta;
        if (dx) {  // dX (+)= [dQ | dK | dV] . [Wq; Wk; Wv]: one NN product, K = 3d
            float* q = first_write(dx, beta);
            check(nk_sgemm(dev, 0, 0, n, d, 3 * d, 1.f, dqkv->ptr(), 3 * d, w->ptr(), d, beta, q, d));
        }
        {
            const int gs[2] = {n, 3 * d}, o3 = 3 * d;
            const bool assign = packed_beta(gb) == 0.f;
            check((assign ? nk_unbroadcast_assign : nk_unbroadcast_add)(dev, gb_all->ptr(), &o3, 1, dqkv->ptr(), gs, 2));
        }
        beta = packed_beta(gw);  // [dWq; dWk; dWv] (+)= [dQ | dK | dV]^T . x: one TN product, M = 3d
        check(nk_sgemm(dev, 1, 0, 3 * d, d, n, 1.f, dqkv->ptr(), 3 * d, x->ptr(), d, beta, gw_all->ptr(), d));
    }
    void targets(std::vector<const Gradient*>& out) const override {
        if (dx) out.push_back(dx.get());
        for (const auto& q : gw) out.push_back(q.get());
        for (const auto& q : gb) out.push_back(q.get());
    }
};

// nn::MultiheadAttention::forward_step: one slice of T new positions per sample against the layer's key / value cache, in
// inference.  Projections (one GEMM into qkv (n, d + 2 dkv) when packed - (n, 3d) without kv_heads -, three into q (n, d) and
// k / v (n, dkv) otherwise), rope, append of Hkv heads, attention, output projection.  `start` is the int32 image of the lengths the cache had when the node was built: a second forward() writes
// the same rows again.
struct DecodeStepFwd : Forward {
    int B, T, H, Hkv, dh, cap;  // Hkv == H: plain multi-head attention, the launches of the module without kv_heads
    int window = 0;             // > 0: every step the core does not take runs nk_attention_decode_window_fwd
    bool ring = false;          // a rolling cache: position p at slot p % cap
    Shared<HipArray> x, w[3], b[3], wo, bo;  // packed: w[0] / b[0] are the (d + 2 dkv, d) / (d + 2 dkv) storage, the others null
    nn::QuantImage qw[3], qwo;               // MultiheadAttention::quantize: the images of w[i] / wo the projections read instead; null without
    Shared<HipArray> qkv, q, k, v, ctx, out;
    Shared<HipArray> kc, vc, ws, start;
    Shared<HipArray> qf, kf, vf;  // grouped prefill on the core: K and V repeated to (n, d); qf: Q out of the packed buffer, contiguous
    float scale;
    bool core = false;  // every start 0, T >= 2, head size of the fused core
    Shared<HipArray> rope;  // the rotary table or null: the new Q and K rows are rotated at start[b] + t before the append
    RopeGeom rg, rgk;       // rg: NH = H + Hkv when packed (Q|K in one launch), H otherwise; rgk: the K launch of the unpacked form, NH = Hkv
    // page > 0: kc / vc are the pools of a PagedKvCache, cap is unused.  `start` then holds, in one upload, the B starts, the
    // (B, max_pages) table rows and the ncopy (src | dst) page ids of the copies reserve() asked for
    int page = 0, max_pages = 0, num_pages = 0, ncopy = 0;
    // y (n, out) = in (n, k) . W^T + bias: the f32 weight, or its quantised image when the node was built with one
    static void project(nk_device* dev, const Shared<HipArray>& in, const Shared<HipArray>& wt, const nn::QuantImage& img,
                        const Shared<HipArray>& bias, const Shared<HipArray>& y, int n, int k, int out) {
        if (img) check(nk_quant_linear_fwd(dev, in->ptr(), k, img.qweight->ptr(), img.scales->ptr(), bias->ptr(), y->ptr(), out, n, out, k, img.bits, img.group));
        else check(nk_linear_fwd(dev, in->ptr(), wt->ptr(), bias->ptr(), y->ptr(), n, k, out));
    }
    void forward() const override {
        nk_device* dev = D(x);
        const int n = B * T, d = H * dh, dkv = Hkv * dh;
        const float *Q, *K, *V;
        int ld, ldkv;
        if (qkv) {
            project(dev, x, w[0], qw[0], b[0], qkv, n, d, d + 2 * dkv);
            Q = qkv->ptr(); K = Q + d; V = Q + d + dkv; ld = ldkv = d + 2 * dkv;
        } else {
            Shared<HipArray> y[3] = {q, k, v};
            for (int i = 0; i < 3; ++i) project(dev, x, w[i], qw[i], b[i], y[i], n, d, i == 0 ? d : dkv);
            Q = q->ptr(); K = k->ptr(); V = v->ptr(); ld = d; ldkv = dkv;
        }
        const int* st = reinterpret_cast<const int*>(start->ptr());
        if (rope) {
            rope_inplace(dev, const_cast<float*>(Q), ld, rope, st, rg, false);
            if (!qkv) rope_inplace(dev, const_cast<float*>(K), ldkv, rope, st, rgk, false);
        }
        const int* tab = st + B;
        if (page > 0) {  // the copies first: a page reserve() made private must hold its prefix before the new rows land in it
            const int* cp = tab + (size_t)B * max_pages;
            if (ncopy > 0) check(nk_kv_pages_copy(dev, kc->ptr(), vc->ptr(), cp, cp + ncopy, ncopy, Hkv, dh, page, num_pages));
            check(nk_kv_pages_append(dev, kc->ptr(), vc->ptr(), K, V, ldkv, st, tab, max_pages, B, T, Hkv, dh, page, num_pages));
        } else if (ring) check(nk_kv_cache_append_ring(dev, kc->ptr(), vc->ptr(), K, V, ldkv, st, B, T, Hkv, dh, cap));
        else check(nk_kv_cache_append(dev, kc->ptr(), vc->ptr(), K, V, ldkv, st, B, T, Hkv, dh, cap));
        if (core && Hkv != H) {  // the core runs on H heads of K and V: the step's rows repeated into the node's temporaries
            const int G = H / Hkv;
            check(nk_repeat_kv_fwd(dev, K, ldkv, kf->ptr(), d, n, Hkv, G, dh));
            check(nk_repeat_kv_fwd(dev, V, ldkv, vf->ptr(), d, n, Hkv, G, dh));
            if (qf) {  // the core takes contiguous rows: the Q block of the packed buffer copied out (G = 1)
                check(nk_repeat_kv_fwd(dev, Q, ld, qf->ptr(), d, n, H, 1, dh));
                Q = qf->ptr();
            }
            check(nk_attention_causal_fwd(dev, Q, kf->ptr(), vf->ptr(), nullptr, nullptr, nullptr, ctx->ptr(), B, T, H, dh, scale, 0.0, 0, 0, 0));
        } else if (core && qkv)
            check(nk_attention_qkv_causal_fwd(dev, qkv->ptr(), nullptr, nullptr, nullptr, ctx->ptr(), B, T, H, dh, scale, 0.0, 0, 0, 0));
        else if (core)
            check(nk_attention_causal_fwd(dev, Q, K, V, nullptr, nullptr, nullptr, ctx->ptr(), B, T, H, dh, scale, 0.0, 0, 0, 0));
        else if (page > 0)
            check(nk_attention_decode_paged_fwd(dev, Q, ld, kc->ptr(), vc->ptr(), st, tab, max_pages, ctx->ptr(), ws->ptr(), B, T, H, Hkv, dh, page,
                                                num_pages, window, scale));
        else if (window > 0)
            check(nk_attention_decode_window_fwd(dev, Q, ld, kc->ptr(), vc->ptr(), st, ctx->ptr(), ws->ptr(), B, T, H, Hkv, dh, cap, window, ring ? 1 : 0,
                                                 scale));
        else if (Hkv != H)
            check(nk_attention_decode_gqa_fwd(dev, Q, ld, kc->ptr(), vc->ptr(), st, ctx->ptr(), ws->ptr(), B, T, H, Hkv, dh, cap, scale));
        else
            check(nk_attention_decode_fwd(dev, Q, ld, kc->ptr(), vc->ptr(), st, ctx->ptr(), ws->ptr(), B, T, H, dh, cap, scale));
        project(dev, ctx, wo, qwo, bo, out, n, d, d);
    }
};

// nn::QuantLinear::forward (ours; semantics at nk_quant_linear_fwd in neuronika_hip.h): (rows, in) -> (rows, out) on the packed integer
// weights.  No backward node: the layer is inference-only.
struct QuantLinearFwd : Forward {
    Shared<HipArray> x, bias, y;
    nn::QuantImage img;
    int rows = 0, in = 0, out = 0;
    void forward() const override {
        check(nk_quant_linear_fwd(D(x), x->ptr(), in, img.qweight->ptr(), img.scales->ptr(), bias ? bias->ptr() : nullptr, y->ptr(), out, rows, out, in,
                                  img.bits, img.group));
    }
};

// Scalar criteria: node/{absolute_error,bce,bce_with_logits,kldiv,nll}/mod.rs.  kind -1 = NLL.
struct LossFwd : Forward {
    int kind;
    Shared<HipArray> x, t, out;
    Reduction red;
    void forward() const override {
        const Shape& s = x->shape();
        if (kind < 0) check(nk_nll_fwd(D(x), x->ptr(), t->ptr(), s.data(), (int)s.size(), (int)red, out->ptr()));
        else check(nk_loss_fwd(D(x), kind, x->ptr(), t->ptr(), s.data(), (int)s.size(), (int)red, out->ptr()));
    }
};
struct LossBwd : Backward {
    int kind;
    Shared<HipArray> x, t;
    Shared<Gradient> dx, g;
    Reduction red;
    void backward() const override {
        HipArray& d = dx->borrow();
        const Shape& s = d.shape();
        if (kind < 0) check(nk_nll_bwd(D(x), d.ptr(), g->borrow().ptr(), t->ptr(), s.data(), (int)s.size(), (int)red));
        else check(nk_loss_bwd(D(x), kind, d.ptr(), g->borrow().ptr(), x->ptr(), t->ptr(), s.data(), (int)s.size(), (int)red));
    }
    void targets(std::vector<const Gradient*>& out) const override { out.push_back(dx.get()); }
};

// Smooth and gated activations (ours; the reference has no such node; semantics in neuronika_hip.h): one forward node, one backward
// entry that keeps the INPUT and recomputes from it.  `H` == 0: pointwise over the whole array; otherwise the gated form over
// (rows, 2 H).  The first writer of the input's gradient takes the assign form.
struct ActivationFwd : Forward {
    int act = 0, H = 0;
    Shared<HipArray> x, y;
    void forward() const override {
        if (H == 0) check(nk_activation_fwd(D(x), act, x->ptr(), y->ptr(), x->len()));
        else check(nk_glu_fwd(D(x), act, x->ptr(), y->ptr(), (long long)(y->len() / (size_t)H), H));
    }
};
struct ActivationBwd : Backward {
    int act = 0, H = 0;
    Shared<HipArray> x;
    Shared<Gradient> dx, g;
    void backward() const override {
        const HipArray& G = g->borrow();
        bool assign = false;
        HipArray& d = dx->borrow_first_write(assign);
        if (H == 0) check((assign ? nk_activation_bwd_assign : nk_activation_bwd)(D(x), act, d.ptr(), G.ptr(), x->ptr(), d.len()));
        else check((assign ? nk_glu_bwd_assign : nk_glu_bwd)(D(x), act, d.ptr(), G.ptr(), x->ptr(), (long long)(G.len() / (size_t)H), H));
    }
    void targets(std::vector<const Gradient*>& out) const override { out.push_back(dx.get()); }
};

// Rotary position embedding (ours; the reference has no such node; semantics in neuronika_hip.h) of a (B*T, NH*dh) value at positions
// 0 .. T-1.  The rotation is orthogonal: the backward is the same kernel with the sign of the sine flipped and holds the table and
// the geometry, nothing of the input.  The first writer of the input's gradient takes the assign form.
struct RopeFwd : Forward {
    RopeGeom rg;
    Shared<HipArray> x, y, table;
    Shared<HipArray> start;  // null: positions 0 .. T-1 of every sample; else one int32 per sample (rg.T = 1: per row)
    void forward() const override {
        const int ld = rg.NH * rg.dh;
        check(nk_rope_fwd(D(x), x->ptr(), ld, y->ptr(), ld, table->ptr(), start ? reinterpret_cast<const int*>(start->ptr()) : nullptr, rg.B, rg.T, rg.NH, rg.dh, rg.rot, rg.max_pos, rg.interleaved));
    }
};
struct RopeBwd : Backward {
    RopeGeom rg;
    Shared<HipArray> table, start;
    Shared<Gradient> dx, g;
    void backward() const override {
        const HipArray& G = g->borrow();
        bool assign = false;
        HipArray& d = dx->borrow_first_write(assign);
        const int ld = rg.NH * rg.dh;
        check((assign ? nk_rope_bwd_assign : nk_rope_bwd)(D(table), d.ptr(), ld, G.ptr(), ld, table->ptr(),
                                                          start ? reinterpret_cast<const int*>(start->ptr()) : nullptr, rg.B, rg.T, rg.NH, rg.dh, rg.rot,
                                                          rg.max_pos, rg.interleaved));
    }
    void targets(std::vector<const Gradient*>& out) const override { out.push_back(dx.get()); }
};

// repeat_kv (ours; the reference has no such node; semantics at nk_repeat_kv_fwd in neuronika_hip.h): a (rows, Hkv*dh) value with every
// head written G times in front of the attention core of a grouped-query layer.  The backward sums the gradients of the copies in
// ascending copy order and keeps nothing of the input.  The first writer of the input's gradient takes the assign form.
struct RepeatKvFwd : Forward {
    int rows = 0, Hkv = 0, G = 0, dh = 0;
    Shared<HipArray> x, y;
    void forward() const override { check(nk_repeat_kv_fwd(D(x), x->ptr(), Hkv * dh, y->ptr(), Hkv * G * dh, rows, Hkv, G, dh)); }
};
struct RepeatKvBwd : Backward {
    int rows = 0, Hkv = 0, G = 0, dh = 0;
    Shared<Gradient> dx, g;
    void backward() const override {
        const HipArray& Gr = g->borrow();
        bool assign = false;
        HipArray& d = dx->borrow_first_write(assign);
        check((assign ? nk_repeat_kv_bwd_assign : nk_repeat_kv_bwd)(Gr.device()->raw(), d.ptr(), Hkv * dh, Gr.ptr(), Hkv * G * dh, rows, Hkv, G, dh));
    }
    void targets(std::vector<const Gradient*>& out) const override { out.push_back(dx.get()); }
};

// Token sampling (ours; the reference has no such node; semantics at nk_sample_fwd in neuronika_hip.h): the ids of the last of T rows
// of every sample of (batch*T, V) logits, as f32.  No backward node: ids are data.  Every forward that was issued consumes one
// offset of the sampler's counter, the way the dropout node consumes its calls (a refused capture throws before the increment).
struct SampleFwd : Forward {
    Shared<HipArray> logits, ids;
    int batch = 0, T = 0, V = 0;
    float temperature = 1.f, top_p = 1.f;
    int top_k = 0;
    uint64_t seed = 0;
    Shared<uint64_t> offset;
    void forward() const override {
        check(nk_sample_fwd(D(logits), logits->ptr() + (size_t)(T - 1) * V, (long long)T * V, batch, V, ids->ptr(), temperature, top_k, top_p, seed,
                            *offset));
        ++(*offset);
    }
};

// Cross entropy of class logits against integer targets (ours; the reference has no such node; semantics in neuronika_hip.h):
// log-softmax and NLL in one forward node, which owns `lse` (one float per position); the backward recomputes the softmax from the
// logits.  The first writer of the logits' gradient takes the assign form (no memset, no read; inactive rows written as zeros).
struct CrossEntropyFwd : Forward {
    Shared<HipArray> x, t, lse, out;
    Reduction red;
    long long ignore_index = -1;
    double label_smoothing = 0.0;
    void forward() const override {
        const Shape& s = x->shape();
        check(nk_cross_entropy_fwd(D(x), x->ptr(), t->ptr(), s.data(), (int)s.size(), (int)red, ignore_index, label_smoothing, lse->ptr(),
                                   out->ptr()));
    }
};
struct CrossEntropyBwd : Backward {
    Shared<HipArray> x, t, lse;
    Shared<Gradient> dx, g;
    Reduction red;
    long long ignore_index = -1;
    double label_smoothing = 0.0;
    void backward() const override {
        const HipArray& G = g->borrow();
        bool assign = false;
        HipArray& d = dx->borrow_first_write(assign);
        const Shape& s = d.shape();
        check((assign ? nk_cross_entropy_bwd_assign : nk_cross_entropy_bwd)(D(x), d.ptr(), G.ptr(), x->ptr(), t->ptr(), lse->ptr(), s.data(),
                                                                            (int)s.size(), (int)red, ignore_index, label_smoothing));
    }
    void targets(std::vector<const Gradient*>& out) const override { out.push_back(dx.get()); }
};

// `Linear::forward` as one node: mm_t + broadcast Addition (neuronika-nn/src/lib.rs:443-446); `relu`: followed by the ReLU
// node (node/relu/mod.rs:29-38) in the same epilogue
struct LinearFwd : Forward {
    Shared<HipArray> x, w, b, y;
    bool relu = false;
    void forward() const override {
        check((relu ? nk_linear_relu_fwd : nk_linear_fwd)(D(x), x->ptr(), w->ptr(), b->ptr(), y->ptr(), x->shape()[0], x->shape()[1], w->shape()[0]));
    }
};
struct LinearBwd : Backward {
    Shared<HipArray> x, w;
    Shared<HipArray> y;              // set for the fused Linear+ReLU node: its output, the mask of its own gradient
    Shared<Gradient> dx, dw, db, g;  // dx null for a non-differentiable input
    mutable Shared<HipArray> masked_;  // (y > 0) * dL/dy of a pass whose writers stored plain values; owned by the node (see below)
    void backward() const override {
        // Linear+ReLU: g must hold dL/dz = (y > 0) * dL/dy.  When every writer of g on this tape applied the mask while
        // storing (`premasked`, decided by VarDiff::run_backward), it already does; otherwise mask it in place now
        // into a scratch copy (the traffic of an in-place pass): g itself keeps dL/dy, what `grad()` of this variable shows
        // in the reference's graph - also for a root, whose gradient is the seed
        // The scratch belongs to the NODE: allocated the first time a pass needs it and kept for the node's life, so that a pass
        // never allocates after the first one (a hipGraph captured from a warm step bakes in a pointer that stays this node's -
        // the pool cannot hand it to another tensor between replays).
        const bool mask_now = y && !g->premasked();
        if (mask_now) {
            const HipArray& Gy = g->borrow();
            if (!masked_ || masked_->shape() != Gy.shape()) masked_ = std::make_shared<HipArray>(x->device(), Gy.shape(), HipArray::Uninit{});
            check(nk_relu_bwd_assign(D(x), masked_->ptr(), Gy.ptr(), y->ptr(), Gy.len()));
        }
        const HipArray& G = mask_now ? *masked_ : g->borrow();
        nk_device* dev = D(x);
        const int n = x->shape()[0], m = x->shape()[1], o = w->shape()[0];
        // MatrixMatrixMulTBackward (left, right) and AdditionBackwardRight write three different buffers, so their
        // order is free: the bias gradient goes first (the data-parallel exchange then sends the small gradients of
        // the whole model as one group while the last weight-gradient GEMMs still run), the weight gradient last
        float beta;  // nk_mm_t_bwd_left / nk_mm_t_bwd_right, with beta 0 when the gradient's zero fill is still pending
        if (dx) {
            float* d = first_write(dx, beta);
            if (dx->premasked())  // x is the output of a Linear+ReLU node: store (x > 0) * (G . W), its pre-activation gradient
                check(nk_linear_bwd_input_relu(dev, d, G.ptr(), w->ptr(), x->ptr(), n, m, o, beta == 0.f ? 1 : 0));
            else
                check(nk_sgemm(dev, 0, 0, n, m, o, 1.f, G.ptr(), o, w->ptr(), m, beta, d, m));
        }
        {
            // (the bias gradient goes first and on its own: under the data-parallel hook the small gradients of the whole model
            //  leave as one group as soon as the last of them is final - in front of this layer's weight-gradient GEMMs.
            //  Summing it on the way in the weight-gradient GEMM - its A operand is G - was built and measured in round 3:
            //  the 16 adds per k-tile cost the TN GEMM 4 %, more than the 12 us reduction they replace)
            const int gs[2] = {n, o};
            bool assign = false;
            HipArray& d = db->borrow_first_write(assign);
            check((assign ? nk_unbroadcast_assign : nk_unbroadcast_add)(dev, d.ptr(), &o, 1, G.ptr(), gs, 2));
            if (BackwardHook* hook = parts_hook(db.get())) hook->grad_part_ready(db.get(), 0, (size_t)o);
        }
        {
            float* d = first_write(dw, beta);
            BackwardHook* hook = parts_hook(dw.get());  // null unless this node is the last writer of dW and the hook wants pieces
            // data-parallel exchange at row-block granularity (only for the weight gradient the hook asks for - by default
            // the one that becomes final last): each half of dW (still >= 512 tiles of 128x128, a full wave of resident
            // blocks) goes to the all-reduce as soon as it is issued, so only half a gradient's exchange is left exposed
            // behind the last GEMM of the backward pass
            const int h = o / 2;
            if (hook && o % 256 == 0 && (long long)(h / 128) * ((m + 127) / 128) >= 512) {
                for (int r0 = 0; r0 < o; r0 += h) {
                    check(nk_sgemm(dev, 1, 0, h, m, n, 1.f, G.ptr() + r0, o, x->ptr(), m, beta, d + (size_t)r0 * m, m));
                    hook->grad_part_ready(dw.get(), (size_t)r0 * m, (size_t)h * m);
                }
            } else {
                check(nk_sgemm(dev, 1, 0, o, m, n, 1.f, G.ptr(), o, x->ptr(), m, beta, d, m));
            }
        }
    }
    void targets(std::vector<const Gradient*>& out) const override {
        if (dx) out.push_back(dx.get());
        out.push_back(dw.get());
        out.push_back(db.get());
    }
    void premask_targets(std::vector<const Gradient*>& out) const override {
        // only when the mask source IS this node's input buffer (the gradient belongs to the node that produced x)
        if (dx && dx->premask_source() && dx->premask_source().get() == x.get()) out.push_back(dx.get());
    }
};

template <class Op>
BackwardEntry entry(Shared<Op> op, Shared<Gradient> grad) {
    return BackwardEntry{std::move(op), std::move(grad)};
}

// Layer normalisation over the trailing dimensions (ours; the reference has no such node): x read as (rows, dim).  The forward
// node owns `stats` = per-row {mean, rstd}, which the backward node reads; the no-gradient form keeps none.
struct LayerNormFwd : Forward {
    Shared<HipArray> x, gamma, beta, y, stats;  // gamma / beta null: no affine part; stats null: nothing kept for a backward pass
    long long rows;
    int dim;
    double eps;
    void forward() const override {
        check(nk_layer_norm_fwd(D(x), x->ptr(), gamma ? gamma->ptr() : nullptr, beta ? beta->ptr() : nullptr, y->ptr(),
                                stats ? stats->ptr() : nullptr, rows, dim, eps));
    }
};
// ONE backward entry for up to three gradients: dgamma and dbeta leave one pass over (g, x, stats) together, dx its own.  Each
// target is written only if that operand is differentiable, each through its own first-writer-assigns state.
struct LayerNormBwd : Backward {
    Shared<Gradient> dx, dgamma, dbeta, g;  // any of the three targets may be null
    Shared<HipArray> x, gamma, stats;
    long long rows;
    int dim;
    void backward() const override {
        const HipArray& G = g->borrow();
        nk_device* dev = D(x);
        bool ag = false, ab = false;
        float* pg = dgamma ? dgamma->borrow_first_write(ag).ptr() : nullptr;
        float* pb = dbeta ? dbeta->borrow_first_write(ab).ptr() : nullptr;
        auto params = [&](float* a, float* b, bool assign) {
            check((assign ? nk_layer_norm_bwd_params_assign : nk_layer_norm_bwd_params)(dev, a, b, G.ptr(), x->ptr(), stats->ptr(), rows, dim));
        };
        if (pg && pb && ag != ab) {  // one gradient already written in this pass (a shared parameter), the other not
            params(pg, nullptr, ag);
            params(nullptr, pb, ab);
        } else if (pg || pb) {
            params(pg, pb, pg ? ag : ab);
        }
        if (dx) {
            bool assign = false;
            HipArray& d = dx->borrow_first_write(assign);
            check((assign ? nk_layer_norm_bwd_assign : nk_layer_norm_bwd)(dev, d.ptr(), G.ptr(), x->ptr(), gamma ? gamma->ptr() : nullptr,
                                                                          stats->ptr(), rows, dim));
        }
    }
    void targets(std::vector<const Gradient*>& out) const override {
        if (dgamma) out.push_back(dgamma.get());
        if (dbeta) out.push_back(dbeta.get());
        if (dx) out.push_back(dx.get());
    }
};

// the normalised extent: `ns` must be the trailing dimensions of `xs`
int layer_norm_dim(const Shape& xs, const Shape& ns) {
    if (ns.empty() || ns.size() > xs.size() || !std::equal(ns.rbegin(), ns.rend(), xs.rbegin()))
        panic("layer_norm: normalized_shape must equal the trailing dimensions of the input");
    const size_t d = numel(ns);
    if (d == 0 || d > (size_t)1 << 30) panic("layer_norm: the normalised extent must be in 1 .. 2^30");
    return (int)d;
}
Shared<LayerNormFwd> layer_norm_fwd_node(const Var& x, const Var* gamma, const Var* beta, const Shape& ns, double eps, bool keep_stats) {
    if (gamma && gamma->shape() != ns) panic("layer_norm: gamma must have the normalised shape");
    if (beta && beta->shape() != ns) panic("layer_norm: beta must have the normalised shape");
    if (!(eps >= 0.0) || !std::isfinite(eps)) panic("layer_norm: eps must be finite and not negative");
    auto n = std::make_shared<LayerNormFwd>();
    n->dim = layer_norm_dim(x.shape(), ns);
    n->rows = (long long)(x.data->len() / (size_t)n->dim);
    if (keep_stats && n->rows > (1ll << 30)) panic("layer_norm: too many rows");
    n->x = x.data; n->gamma = gamma ? gamma->data : nullptr; n->beta = beta ? beta->data : nullptr;
    n->y = zeros_like(x.data, x.shape());
    if (keep_stats) n->stats = zeros_like(x.data, Shape{(int)n->rows, 2});
    n->eps = eps;
    return n;
}
Var layer_norm_var(const Var& x, const Var* gamma, const Var* beta, const Shape& ns, double eps) {
    History<ForwardEntry> h = x.history;
    if (gamma) h.merge(gamma->history);
    if (beta) h.merge(beta->history);
    auto n = layer_norm_fwd_node(x, gamma, beta, ns, eps, false);
    auto y = n->y;
    return Var::node(y, n, std::move(h));
}
// x, gamma, beta with their gradients and tapes where differentiable (null otherwise); at least one gradient is not null
VarDiff layer_norm_diff(const Var& x, const Shared<Gradient>& dx, const History<BackwardEntry>* hx, const Var* gamma,
                        const Shared<Gradient>& dgamma, const History<BackwardEntry>* hg, const Var* beta,
                        const Shared<Gradient>& dbeta, const History<BackwardEntry>* hb, const Shape& ns, double eps) {
    History<ForwardEntry> fh = x.history;
    if (gamma) fh.merge(gamma->history);
    if (beta) fh.merge(beta->history);
    auto n = layer_norm_fwd_node(x, gamma, beta, ns, eps, true);
    auto y = n->y;
    Var var = Var::node(y, n, std::move(fh));
    History<BackwardEntry> h;
    if (hx) h = *hx;
    if (hg) h.merge(*hg);
    if (hb) h.merge(*hb);
    auto grad = std::make_shared<Gradient>(var.device(), var.shape());
    auto bw = std::make_shared<LayerNormBwd>();
    bw->dx = dx; bw->dgamma = dgamma; bw->dbeta = dbeta; bw->g = grad;
    bw->x = x.data; bw->gamma = n->gamma; bw->stats = n->stats; bw->rows = n->rows; bw->dim = n->dim;
    return VarDiff::node(std::move(var), grad, entry(bw, grad), std::move(h));
}

// RMS normalisation over the trailing dimensions (ours; the reference has no such node): x read as (rows, dim).  The forward node
// owns `stats` = per-row rstd, which the backward node reads; the no-gradient form keeps none.
struct RmsNormFwd : Forward {
    Shared<HipArray> x, gamma, y, stats;  // gamma null: no weight; stats null: nothing kept for a backward pass
    long long rows;
    int dim;
    double eps;
    void forward() const override {
        check(nk_rms_norm_fwd(D(x), x->ptr(), gamma ? gamma->ptr() : nullptr, y->ptr(), stats ? stats->ptr() : nullptr, rows, dim, eps));
    }
};
// ONE backward entry for up to two gradients, each written only if that operand is differentiable, each through its own
// first-writer-assigns state.
struct RmsNormBwd : Backward {
    Shared<Gradient> dx, dgamma, g;  // either target may be null
    Shared<HipArray> x, gamma, stats;
    long long rows;
    int dim;
    void backward() const override {
        const HipArray& G = g->borrow();
        nk_device* dev = D(x);
        if (dgamma) {
            bool assign = false;
            HipArray& d = dgamma->borrow_first_write(assign);
            check((assign ? nk_rms_norm_bwd_gamma_assign : nk_rms_norm_bwd_gamma)(dev, d.ptr(), G.ptr(), x->ptr(), stats->ptr(), rows, dim));
        }
        if (dx) {
            bool assign = false;
            HipArray& d = dx->borrow_first_write(assign);
            check((assign ? nk_rms_norm_bwd_assign : nk_rms_norm_bwd)(dev, d.ptr(), G.ptr(), x->ptr(), gamma ? gamma->ptr() : nullptr,
                                                                      stats->ptr(), rows, dim));
        }
    }
    void targets(std::vector<const Gradient*>& out) const override {
        if (dgamma) out.push_back(dgamma.get());
        if (dx) out.push_back(dx.get());
    }
};

Shared<RmsNormFwd> rms_norm_fwd_node(const Var& x, const Var* gamma, const Shape& ns, double eps, bool keep_stats) {
    if (gamma && gamma->shape() != ns) panic("rms_norm: gamma must have the normalised shape");
    if (!(eps >= 0.0) || !std::isfinite(eps)) panic("rms_norm: eps must be finite and not negative");
    auto n = std::make_shared<RmsNormFwd>();
    if (ns.empty() || ns.size() > x.shape().size() || !std::equal(ns.rbegin(), ns.rend(), x.shape().rbegin()))
        panic("rms_norm: normalized_shape must equal the trailing dimensions of the input");
    n->dim = layer_norm_dim(x.shape(), ns);
    n->rows = (long long)(x.data->len() / (size_t)n->dim);
    if (keep_stats && n->rows > (1ll << 30)) panic("rms_norm: too many rows");
    n->x = x.data; n->gamma = gamma ? gamma->data : nullptr;
    n->y = zeros_like(x.data, x.shape());
    if (keep_stats) n->stats = zeros_like(x.data, Shape{(int)n->rows});
    n->eps = eps;
    return n;
}
Var rms_norm_var(const Var& x, const Var* gamma, const Shape& ns, double eps) {
    History<ForwardEntry> h = x.history;
    if (gamma) h.merge(gamma->history);
    auto n = rms_norm_fwd_node(x, gamma, ns, eps, false);
    auto y = n->y;
    return Var::node(y, n, std::move(h));
}
// x and gamma with their gradients and tapes where differentiable (null otherwise); at least one gradient is not null
VarDiff rms_norm_diff(const Var& x, const Shared<Gradient>& dx, const History<BackwardEntry>* hx, const Var* gamma,
                      const Shared<Gradient>& dgamma, const History<BackwardEntry>* hg, const Shape& ns, double eps) {
    History<ForwardEntry> fh = x.history;
    if (gamma) fh.merge(gamma->history);
    auto n = rms_norm_fwd_node(x, gamma, ns, eps, true);
    auto y = n->y;
    Var var = Var::node(y, n, std::move(fh));
    History<BackwardEntry> h;
    if (hx) h = *hx;
    if (hg) h.merge(*hg);
    auto grad = std::make_shared<Gradient>(var.device(), var.shape());
    auto bw = std::make_shared<RmsNormBwd>();
    bw->dx = dx; bw->dgamma = dgamma; bw->g = grad;
    bw->x = x.data; bw->gamma = n->gamma; bw->stats = n->stats; bw->rows = n->rows; bw->dim = n->dim;
    return VarDiff::node(std::move(var), grad, entry(bw, grad), std::move(h));
}

// Group normalisation (ours; the reference has no such node): x of shape (N, C, spatial...) read as (N, C, L), `groups` channel
// groups; groups == C is instance normalisation.  gamma / beta of shape (C), both or neither.  The forward node owns `stats` =
// {mean, rstd} per (sample, group), which the backward node reads; the no-gradient form keeps none.
struct GroupNormFwd : Forward {
    Shared<HipArray> x, gamma, beta, y, stats;  // gamma / beta null: no affine part; stats null: nothing kept for a backward pass
    long long N, L;
    int C, groups;
    double eps;
    void forward() const override {
        check(nk_group_norm_fwd(D(x), x->ptr(), gamma ? gamma->ptr() : nullptr, beta ? beta->ptr() : nullptr, y->ptr(),
                                stats ? stats->ptr() : nullptr, N, C, L, groups, eps));
    }
};
// ONE backward entry for up to three gradients, each written only if that operand is differentiable, each through its own
// first-writer-assigns state.
struct GroupNormBwd : Backward {
    Shared<Gradient> dx, dgamma, dbeta, g;  // any of the three targets may be null
    Shared<HipArray> x, gamma, stats;
    long long N, L;
    int C, groups;
    void backward() const override {
        const HipArray& G = g->borrow();
        nk_device* dev = D(x);
        auto params = [&](float* a, float* b, bool assign) {
            check((assign ? nk_group_norm_bwd_params_assign : nk_group_norm_bwd_params)(dev, a, b, G.ptr(), x->ptr(), stats->ptr(), N, C, L, groups));
        };
        bool ag = false, ab = false;
        float* pg = dgamma ? dgamma->borrow_first_write(ag).ptr() : nullptr;
        float* pb = dbeta ? dbeta->borrow_first_write(ab).ptr() : nullptr;
        if (pg && pb && ag != ab) {  // one gradient already written in this pass (a shared parameter), the other not
            params(pg, nullptr, ag);
            params(nullptr, pb, ab);
        } else if (pg || pb) {  // one pass over (g, x, stats) for both
            params(pg, pb, pg ? ag : ab);
        }
        if (dx) {
            bool assign = false;
            HipArray& d = dx->borrow_first_write(assign);
            check((assign ? nk_group_norm_bwd_assign : nk_group_norm_bwd)(dev, d.ptr(), G.ptr(), x->ptr(), gamma ? gamma->ptr() : nullptr,
                                                                          stats->ptr(), N, C, L, groups));
        }
    }
    void targets(std::vector<const Gradient*>& out) const override {
        if (dgamma) out.push_back(dgamma.get());
        if (dbeta) out.push_back(dbeta.get());
        if (dx) out.push_back(dx.get());
    }
};

Shared<GroupNormFwd> group_norm_fwd_node(const Var& x, int groups, const Var* gamma, const Var* beta, double eps, bool keep_stats) {
    const Shape& xs = x.shape();
    if (xs.size() < 2) panic("group_norm: expected an input of at least 2 dimensions (N, C, ...), got " + std::to_string(xs.size()));
    const int C = xs[1];
    if (groups <= 0 || C <= 0 || C % groups != 0)
        panic("group_norm: " + std::to_string(C) + " channels cannot be cut into " + std::to_string(groups) + " groups");
    if ((gamma == nullptr) != (beta == nullptr)) panic("group_norm: gamma and beta go together");
    if (gamma && gamma->shape() != Shape{C}) panic("group_norm: gamma must have shape (C)");
    if (beta && beta->shape() != Shape{C}) panic("group_norm: beta must have shape (C)");
    if (!(eps >= 0.0) || !std::isfinite(eps)) panic("group_norm: eps must be finite and not negative");
    auto n = std::make_shared<GroupNormFwd>();
    n->N = xs[0]; n->C = C; n->groups = groups;
    n->L = 1;
    for (size_t i = 2; i < xs.size(); ++i) n->L *= xs[i];
    if (n->L * (C / groups) > 0x7fffffffll || n->N * groups > 0x7fffffffll) panic("group_norm: a group row and the row count must each fit in 31 bits");
    n->x = x.data; n->gamma = gamma ? gamma->data : nullptr; n->beta = beta ? beta->data : nullptr;
    n->y = zeros_like(x.data, xs);
    if (keep_stats) n->stats = zeros_like(x.data, Shape{(int)(n->N * groups), 2});
    n->eps = eps;
    return n;
}
Var group_norm_var(const Var& x, int groups, const Var* gamma, const Var* beta, double eps) {
    History<ForwardEntry> h = x.history;
    if (gamma) h.merge(gamma->history);
    if (beta) h.merge(beta->history);
    auto n = group_norm_fwd_node(x, groups, gamma, beta, eps, false);
    auto y = n->y;
    return Var::node(y, n, std::move(h));
}
// x, gamma, beta with their gradients and tapes where differentiable (null otherwise); at least one gradient is not null
VarDiff group_norm_diff(const Var& x, const Shared<Gradient>& dx, const History<BackwardEntry>* hx, int groups, const Var* gamma,
                        const Shared<Gradient>& dgamma, const History<BackwardEntry>* hg, const Var* beta,
                        const Shared<Gradient>& dbeta, const History<BackwardEntry>* hb, double eps) {
    History<ForwardEntry> fh = x.history;
    if (gamma) fh.merge(gamma->history);
    if (beta) fh.merge(beta->history);
    auto n = group_norm_fwd_node(x, groups, gamma, beta, eps, true);
    auto y = n->y;
    Var var = Var::node(y, n, std::move(fh));
    History<BackwardEntry> h;
    if (hx) h = *hx;
    if (hg) h.merge(*hg);
    if (hb) h.merge(*hb);
    auto grad = std::make_shared<Gradient>(var.device(), var.shape());
    auto bw = std::make_shared<GroupNormBwd>();
    bw->dx = dx; bw->dgamma = dgamma; bw->dbeta = dbeta; bw->g = grad;
    bw->x = x.data; bw->gamma = n->gamma; bw->stats = n->stats; bw->N = n->N; bw->C = n->C; bw->L = n->L; bw->groups = groups;
    return VarDiff::node(std::move(var), grad, entry(bw, grad), std::move(h));
}

// Batch normalisation (ours; the reference has no such node): x read as (N, C, L), L the product of the extents behind the channel
// axis.  The forward node reads `status` each time it runs on the host (as Dropout's does): training normalises with the batch
// statistics and updates the running ones in place, inference normalises with the running ones.  Without running statistics the
// batch statistics serve in both modes.  `stats` = per-channel {mean, rstd} for the backward node; the no-gradient form keeps none.
struct BatchNormFwd : Forward {
    Shared<HipArray> x, gamma, beta, running_mean, running_var, y, stats;  // gamma / beta, the running pair, stats: null when absent
    int N, C, L;
    double eps, momentum;
    Shared<bool> status;
    Shared<bool> trained = std::make_shared<bool>(true);  // the mode of the last forward run, for the backward node
    void forward() const override {
        *trained = *status || !running_mean;
        auto p = [](const Shared<HipArray>& a) { return a ? a->ptr() : nullptr; };
        if (*trained)
            check(nk_batch_norm_fwd(D(x), x->ptr(), p(gamma), p(beta), y->ptr(), p(stats), p(running_mean), p(running_var), N, C, L, eps, momentum));
        else
            check(nk_batch_norm_infer_fwd(D(x), x->ptr(), p(gamma), p(beta), running_mean->ptr(), running_var->ptr(), y->ptr(), p(stats), N, C, L, eps));
    }
};
// ONE backward entry for up to three gradients: one reduction pass leaves {sum g, sum g * xhat} per channel in `sums`, which dx (in
// training) and both parameter gradients read.  Each target is written only if that operand is differentiable, each through its
// own first-writer-assigns state.
struct BatchNormBwd : Backward {
    Shared<Gradient> dx, dgamma, dbeta, g;  // any of the three targets may be null
    Shared<HipArray> x, gamma, stats, sums;
    Shared<bool> trained;
    int N, C, L;
    void backward() const override {
        const HipArray& G = g->borrow();
        nk_device* dev = D(x);
        const bool need_sums = dgamma || dbeta || (dx && *trained);
        if (need_sums) check(nk_batch_norm_bwd_sums(dev, sums->ptr(), G.ptr(), x->ptr(), stats->ptr(), N, C, L));
        bool ag = false, ab = false;
        float* pg = dgamma ? dgamma->borrow_first_write(ag).ptr() : nullptr;
        float* pb = dbeta ? dbeta->borrow_first_write(ab).ptr() : nullptr;
        auto params = [&](float* a, float* b, bool assign) {
            check((assign ? nk_batch_norm_bwd_params_assign : nk_batch_norm_bwd_params)(dev, a, b, sums->ptr(), C));
        };
        if (pg && pb && ag != ab) {  // one gradient already written in this pass (a shared parameter), the other not
            params(pg, nullptr, ag);
            params(nullptr, pb, ab);
        } else if (pg || pb) {
            params(pg, pb, pg ? ag : ab);
        }
        if (dx) {
            bool assign = false;
            HipArray& d = dx->borrow_first_write(assign);
            check((assign ? nk_batch_norm_bwd_assign : nk_batch_norm_bwd)(dev, d.ptr(), G.ptr(), x->ptr(), gamma ? gamma->ptr() : nullptr, stats->ptr(),
                                                                          *trained ? sums->ptr() : nullptr, N, C, L));
        }
    }
    void targets(std::vector<const Gradient*>& out) const override {
        if (dgamma) out.push_back(dgamma.get());
        if (dbeta) out.push_back(dbeta.get());
        if (dx) out.push_back(dx.get());
    }
};

Shared<BatchNormFwd> batch_norm_fwd_node(const Var& x, const Var* gamma, const Var* beta, const Var* running_mean, const Var* running_var,
                                         double momentum, double eps, Shared<bool> status, bool keep_stats) {
    const Shape& xs = x.shape();
    if (xs.size() < 2) panic("batch_norm: the input must have at least two dimensions (N, C, ...), got " + std::to_string(xs.size()));
    const int C = xs[1];
    if (C <= 0) panic("batch_norm: the channel extent must be positive");
    auto per_channel = [&](const Var* v, const char* name) {
        if (v && v->shape() != Shape{C}) panic(std::string("batch_norm: ") + name + " must have shape (C) = (" + std::to_string(C) + ")");
    };
    per_channel(gamma, "gamma"); per_channel(beta, "beta"); per_channel(running_mean, "running_mean"); per_channel(running_var, "running_var");
    if (!running_mean != !running_var) panic("batch_norm: running_mean and running_var come together or not at all");
    if (!(eps >= 0.0) || !std::isfinite(eps)) panic("batch_norm: eps must be finite and not negative");
    if (!(momentum >= 0.0 && momentum <= 1.0)) panic("batch_norm: momentum must be in [0, 1]");
    if (!status) panic("batch_norm: a status flag is required");
    size_t L = 1;
    for (size_t i = 2; i < xs.size(); ++i) L *= (size_t)xs[i];
    if ((size_t)xs[0] * L > (size_t)INT_MAX) panic("batch_norm: more than 2^31 - 1 values per channel");
    auto n = std::make_shared<BatchNormFwd>();
    n->N = xs[0]; n->C = C; n->L = (int)L;
    auto data = [](const Var* v) { return v ? v->data : nullptr; };
    n->x = x.data; n->gamma = data(gamma); n->beta = data(beta); n->running_mean = data(running_mean); n->running_var = data(running_var);
    n->y = zeros_like(x.data, xs);
    if (keep_stats) n->stats = zeros_like(x.data, Shape{C, 2});
    n->eps = eps; n->momentum = momentum; n->status = std::move(status);
    return n;
}
History<ForwardEntry> batch_norm_history(const Var& x, const Var* gamma, const Var* beta) {
    History<ForwardEntry> h = x.history;
    if (gamma) h.merge(gamma->history);
    if (beta) h.merge(beta->history);
    return h;
}
Var batch_norm_var(const Var& x, const Var* gamma, const Var* beta, const Var* rm, const Var* rv, double momentum, double eps, Shared<bool> status) {
    auto n = batch_norm_fwd_node(x, gamma, beta, rm, rv, momentum, eps, std::move(status), false);
    auto y = n->y;
    return Var::node(y, n, batch_norm_history(x, gamma, beta));
}
// x, gamma, beta with their gradients and tapes where differentiable (null otherwise); at least one gradient is not null
VarDiff batch_norm_diff(const Var& x, const Shared<Gradient>& dx, const History<BackwardEntry>* hx, const Var* gamma,
                        const Shared<Gradient>& dgamma, const History<BackwardEntry>* hg, const Var* beta, const Shared<Gradient>& dbeta,
                        const History<BackwardEntry>* hb, const Var* rm, const Var* rv, double momentum, double eps, Shared<bool> status) {
    auto n = batch_norm_fwd_node(x, gamma, beta, rm, rv, momentum, eps, std::move(status), true);
    auto y = n->y;
    Var var = Var::node(y, n, batch_norm_history(x, gamma, beta));
    History<BackwardEntry> h;
    if (hx) h = *hx;
    if (hg) h.merge(*hg);
    if (hb) h.merge(*hb);
    auto grad = std::make_shared<Gradient>(var.device(), var.shape());
    auto bw = std::make_shared<BatchNormBwd>();
    bw->dx = dx; bw->dgamma = dgamma; bw->dbeta = dbeta; bw->g = grad;
    bw->x = x.data; bw->gamma = n->gamma; bw->stats = n->stats; bw->sums = zeros_like(x.data, Shape{n->C, 2});
    bw->trained = n->trained; bw->N = n->N; bw->C = n->C; bw->L = n->L;
    return VarDiff::node(std::move(var), grad, entry(bw, grad), std::move(h));
}

// Pooling (ours; the reference has no such node; semantics in neuronika_hip.h).  The geometry is checked when the graph is built
// (nk_pool_out_shape holds the rules, the messages here name the offending axis); the max-pool node of a differentiable graph
// owns `idx`, the int32 offsets of the selected elements, in an f32 array of the output's shape (the same 4 bytes per element).
struct PoolFwd : Forward {
    Shared<HipArray> x, y, idx;  // idx: null for average pooling and for the no-gradient max pooling
    std::vector<int> kernel, stride, padding;
    bool average = false, count_include_pad = true;
    void forward() const override {
        const int nd = (int)kernel.size();
        if (average)
            check(nk_avg_pool_fwd(D(x), nd, x->ptr(), x->shape().data(), y->ptr(), kernel.data(), stride.data(), padding.data(), count_include_pad));
        else
            check(nk_max_pool_fwd(D(x), nd, x->ptr(), x->shape().data(), y->ptr(), idx ? reinterpret_cast<int*>(idx->ptr()) : nullptr, kernel.data(),
                                  stride.data(), padding.data()));
    }
};
struct PoolBwd : Backward {
    Shared<Gradient> dx, g;
    Shared<HipArray> idx;
    Shape x_shape;
    std::vector<int> kernel, stride, padding;
    bool average = false, count_include_pad = true;
    void backward() const override {
        const HipArray& G = g->borrow();
        bool assign = false;
        HipArray& d = dx->borrow_first_write(assign);
        nk_device* dev = d.device()->raw();
        const int nd = (int)kernel.size();
        if (average)
            check((assign ? nk_avg_pool_bwd_assign : nk_avg_pool_bwd)(dev, nd, d.ptr(), x_shape.data(), G.ptr(), kernel.data(), stride.data(),
                                                                      padding.data(), count_include_pad));
        else
            check((assign ? nk_max_pool_bwd_assign : nk_max_pool_bwd)(dev, nd, d.ptr(), x_shape.data(), G.ptr(), reinterpret_cast<const int*>(idx->ptr()),
                                                                      kernel.data(), stride.data(), padding.data()));
    }
    void targets(std::vector<const Gradient*>& out) const override { out.push_back(dx.get()); }
};

Shared<PoolFwd> pool_fwd_node(const char* what, const Var& x, const std::vector<int>& kernel, const std::vector<int>& stride_in,
                              const std::vector<int>& padding_in, bool average, bool count_include_pad, bool keep_idx) {
    const Shape& xs = x.shape();
    const std::string name = what;
    if (xs.size() < 3 || xs.size() > 5) panic(name + ": the input must be (N, C, spatial...) with 1 to 3 spatial axes, got " + std::to_string(xs.size()) + " dimensions");
    const size_t nd = xs.size() - 2;
    const std::vector<int> stride = stride_in.empty() ? kernel : stride_in;
    const std::vector<int> padding = padding_in.empty() ? std::vector<int>(nd, 0) : padding_in;
    if (kernel.size() != nd) panic(name + ": kernel has " + std::to_string(kernel.size()) + " entries for " + std::to_string(nd) + " spatial axes");
    if (stride.size() != nd) panic(name + ": stride has " + std::to_string(stride.size()) + " entries for " + std::to_string(nd) + " spatial axes");
    if (padding.size() != nd) panic(name + ": padding has " + std::to_string(padding.size()) + " entries for " + std::to_string(nd) + " spatial axes");
    for (size_t i = 0; i < nd; ++i) {
        const std::string axis = " of spatial axis " + std::to_string(i);
        if (kernel[i] < 1) panic(name + ": window " + std::to_string(kernel[i]) + axis + " (must be >= 1)");
        if (stride[i] < 1) panic(name + ": stride " + std::to_string(stride[i]) + axis + " (must be >= 1)");
        if (padding[i] < 0 || padding[i] > kernel[i] / 2)
            panic(name + ": padding " + std::to_string(padding[i]) + axis + " (must be in [0, window / 2] = [0, " + std::to_string(kernel[i] / 2) + "])");
        if (xs[2 + i] < 1 || xs[2 + i] + 2 * padding[i] < kernel[i])
            panic(name + ": window " + std::to_string(kernel[i]) + " exceeds the padded extent " + std::to_string(xs[2 + i]) + " + 2 * " +
                  std::to_string(padding[i]) + axis + ": no output");
    }
    Shape ys(xs.size());
    if (nk_pool_out_shape((int)nd, xs.data(), kernel.data(), stride.data(), padding.data(), ys.data()) != NK_OK) panic(name + ": " + nk_last_error());
    auto n = std::make_shared<PoolFwd>();
    n->x = x.data; n->y = zeros_like(x.data, ys);
    if (keep_idx) n->idx = zeros_like(x.data, ys);
    n->kernel = kernel; n->stride = stride; n->padding = padding;
    n->average = average; n->count_include_pad = count_include_pad;
    return n;
}
Var pool_var(const char* what, const Var& x, const std::vector<int>& kernel, const std::vector<int>& stride, const std::vector<int>& padding,
             bool average, bool count_include_pad) {
    auto n = pool_fwd_node(what, x, kernel, stride, padding, average, count_include_pad, false);
    auto y = n->y;
    return Var::node(y, n, x.history);
}
VarDiff pool_diff(const char* what, const VarDiff& x, const std::vector<int>& kernel, const std::vector<int>& stride, const std::vector<int>& padding,
                  bool average, bool count_include_pad) {
    auto n = pool_fwd_node(what, x.var, kernel, stride, padding, average, count_include_pad, !average);
    auto y = n->y;
    Var v = Var::node(y, n, x.var.history);
    auto g = std::make_shared<Gradient>(v.device(), v.shape());
    auto bw = std::make_shared<PoolBwd>();
    bw->dx = x.grad; bw->g = g; bw->idx = n->idx; bw->x_shape = x.shape();
    bw->kernel = n->kernel; bw->stride = n->stride; bw->padding = n->padding;
    bw->average = average; bw->count_include_pad = count_include_pad;
    return VarDiff::node(std::move(v), g, entry(bw, g), x.history);
}
// Upsampling (ours; the reference has no such node; semantics in neuronika_hip.h).  The mode's name is checked against the rank
// when the graph is built; the extents are checked by the library at the first forward, as every geometry it owns.
int upsample_mode(const std::string& mode, size_t nd) {
    if (mode == "nearest") return NK_UPSAMPLE_NEAREST;
    const char* linear[] = {"linear", "bilinear", "trilinear"};
    for (size_t i = 0; i < 3; ++i)
        if (mode == linear[i]) {
            if (nd != i + 1) panic("upsample: mode \"" + mode + "\" is for " + std::to_string(i + 1) + " spatial axes, the input has " + std::to_string(nd));
            return NK_UPSAMPLE_LINEAR;
        }
    panic("upsample: unknown mode \"" + mode + "\" (nearest, linear, bilinear, trilinear)");
    return -1;
}
struct UpsampleFwd : Forward {
    Shared<HipArray> x, y;
    std::vector<int> out_size;
    int mode = 0, align_corners = 0;
    void forward() const override {
        check(nk_upsample_fwd(D(x), (int)out_size.size(), mode, align_corners, x->ptr(), x->shape().data(), y->ptr(), out_size.data()));
    }
};
struct UpsampleBwd : Backward {
    Shared<Gradient> dx, g;
    Shape x_shape;
    std::vector<int> out_size;
    int mode = 0, align_corners = 0;
    void backward() const override {
        const HipArray& G = g->borrow();
        bool assign = false;
        HipArray& d = dx->borrow_first_write(assign);
        check((assign ? nk_upsample_bwd_assign : nk_upsample_bwd)(d.device()->raw(), (int)out_size.size(), mode, align_corners, d.ptr(), x_shape.data(),
                                                                  G.ptr(), out_size.data()));
    }
    void targets(std::vector<const Gradient*>& out) const override { out.push_back(dx.get()); }
};
Shared<UpsampleFwd> upsample_fwd_node(const Var& x, const std::vector<int>& out_size, const std::string& mode, bool align_corners) {
    const Shape& xs = x.shape();
    if (xs.size() < 3 || xs.size() > 5) panic("upsample: the input must be (N, C, spatial...) with 1 to 3 spatial axes, got " + std::to_string(xs.size()) + " dimensions");
    const size_t nd = xs.size() - 2;
    if (out_size.size() != nd) panic("upsample: out_size has " + std::to_string(out_size.size()) + " entries for " + std::to_string(nd) + " spatial axes");
    const int m = upsample_mode(mode, nd);
    if (m == NK_UPSAMPLE_NEAREST && align_corners) panic("upsample: align_corners has no meaning for the nearest mode");
    Shape ys(xs.begin(), xs.begin() + 2);
    size_t plane = 1;
    for (size_t i = 0; i < nd; ++i) {
        if (xs[2 + i] < 1) panic("upsample: spatial extent " + std::to_string(xs[2 + i]) + " of spatial axis " + std::to_string(i));
        if (out_size[i] < 1) panic("upsample: output extent " + std::to_string(out_size[i]) + " of spatial axis " + std::to_string(i) + " (must be >= 1)");
        plane *= (size_t)out_size[i];
        if (plane > (size_t)INT_MAX) panic("upsample: an output plane of more than 2^31 - 1 elements");
        ys.push_back(out_size[i]);
    }
    auto n = std::make_shared<UpsampleFwd>();
    n->x = x.data; n->y = zeros_like(x.data, ys);
    n->out_size = out_size; n->mode = m; n->align_corners = align_corners;
    return n;
}

std::vector<int> spatial_extents(const char* what, const Shape& s) {
    if (s.size() < 3 || s.size() > 5)
        panic(std::string(what) + ": the input must be (N, C, spatial...) with 1 to 3 spatial axes, got " + std::to_string(s.size()) + " dimensions");
    return std::vector<int>(s.begin() + 2, s.end());
}
Shape flat_shape(const Shape& s) {
    if (s.size() < 2) panic("flatten: the input must have at least two dimensions (N, ...), got " + std::to_string(s.size()));
    size_t n = 1;
    for (size_t i = 1; i < s.size(); ++i) n *= (size_t)s[i];
    if (n > (size_t)INT_MAX) panic("flatten: more than 2^31 - 1 values per sample");
    return Shape{s[0], (int)n};
}

// Embedding (ours; the reference has no such node; semantics in neuronika_hip.h): rows of the (V, D) table selected by the ids of
// `idx`, f32 as the NLL targets are, of any shape.  Differentiable in the table only; the ids are data.
struct EmbeddingFwd : Forward {
    Shared<HipArray> weight, idx, y;
    void forward() const override {
        const Shape& ws = weight->shape();
        check(nk_embedding_fwd(D(weight), weight->ptr(), idx->ptr(), y->ptr(), (long long)idx->len(), ws[0], ws[1]));
    }
};
// the table's gradient: the ordered sum per row.  The first writer of the pass takes the assign form, which covers the whole table
// (no memset, no read); a second embedding on the same table (tied weights) takes the `+=` form.
struct EmbeddingBwd : Backward {
    Shared<Gradient> dw, g;
    Shared<HipArray> idx;
    long long padding_idx = -1;
    void backward() const override {
        const HipArray& G = g->borrow();
        bool assign = false;
        HipArray& d = dw->borrow_first_write(assign);
        const Shape& ws = d.shape();
        check((assign ? nk_embedding_bwd_assign : nk_embedding_bwd)(d.device()->raw(), d.ptr(), G.ptr(), idx->ptr(), (long long)idx->len(), ws[0],
                                                                    ws[1], padding_idx));
    }
    void targets(std::vector<const Gradient*>& out) const override { out.push_back(dw.get()); }
};
Shared<EmbeddingFwd> embedding_fwd_node(const Var& weight, const Var& indices, long padding_idx) {
    const Shape& ws = weight.shape();
    if (ws.size() != 2 || ws[0] < 1 || ws[1] < 1) panic("embedding: the table must be (num_embeddings, embedding_dim), both at least 1");
    if (ws[0] > (1 << 24)) panic("embedding: at most 2^24 rows (ids are stored as f32), got " + std::to_string(ws[0]));
    if (padding_idx >= ws[0]) panic("embedding: padding_idx " + std::to_string(padding_idx) + " is not a row of a table of " + std::to_string(ws[0]));
    if (indices.data->len() > ((size_t)1 << 30)) panic("embedding: more than 2^30 ids");
    if (indices.device().get() != weight.device().get()) panic("embedding: table and ids live on different devices");
    Shape ys = indices.shape();
    ys.push_back(ws[1]);
    auto n = std::make_shared<EmbeddingFwd>();
    n->weight = weight.data; n->idx = indices.data; n->y = zeros_like(weight.data, ys);
    return n;
}

Shape mm_shape(const Shape& a, const Shape& b, int kind) {  // utils.rs:46-55 `DotDim`
    if (kind == 4) {
        if (a.size() != 2 || b.size() != 1) panic("mv: matrix and vector expected");
        if (a[1] != b[0]) panic("Shapes are incompatible for matrix-vector multiplication.");
        return Shape{a[0]};
    }
    if (kind == 5) {
        if (a.size() != 1 || b.size() != 2) panic("vm: vector and matrix expected");
        if (a[0] != b[0]) panic("Shapes are incompatible for vector-matrix multiplication.");
        return Shape{b[1]};
    }
    if (kind == 6) {
        if (a.size() != 1 || b.size() != 1) panic("vv: vectors expected");
        if (a[0] != b[0]) panic("Shapes are incompatible for vector-vector multiplication.");
        return Shape{};
    }
    if (kind <= 1) {
        if (a.size() != 2 || b.size() != 2) panic("mm: matrices expected");
        const int inner_b = kind == 0 ? b[0] : b[1];
        if (a[1] != inner_b) panic("Shapes are incompatible for matrix multiplication.");
        return Shape{a[0], kind == 0 ? b[1] : b[0]};
    }
    if (a.size() != 3 || b.size() != 3 || a[0] != b[0]) panic("bmm: [B,n,m] x [B,*,*] expected");
    const int inner_b = kind == 2 ? b[1] : b[2];
    if (a[2] != inner_b) panic("Shapes are incompatible for matrix multiplication.");
    return Shape{a[0], a[1], kind == 2 ? b[2] : b[1]};
}

Var matmul_var(int kind, const Var& a, const Var& b) {
    History<ForwardEntry> h = a.history;
    h.merge(b.history);
    auto out = zeros_like(a.data, mm_shape(a.shape(), b.shape(), kind));
    return Var::node(out, std::make_shared<MatMulFwd>(kind, a.data, b.data, out), std::move(h));
}
VarDiff matmul_diff(int kind, const Var& a, const Shared<Gradient>& da, const History<BackwardEntry>* ha, const Var& b,
                    const Shared<Gradient>& db, const History<BackwardEntry>* hb) {
    Var var = matmul_var(kind, a, b);
    History<BackwardEntry> h;
    if (ha) h = *ha;
    if (hb) h.merge(*hb);
    auto grad = std::make_shared<Gradient>(var.device(), var.shape());
    auto op = std::make_shared<MatMulBwd>();
    op->kind = kind; op->a = a.data; op->b = b.data; op->da = da; op->db = db; op->g = grad;
    return VarDiff::node(std::move(var), grad, entry(op, grad), std::move(h));
}

Var binary_var(int op, const Var& l, const Var& r) {
    History<ForwardEntry> h = l.history;
    h.merge(r.history);
    auto out = zeros_like(l.data, cobroadcast(l.shape(), r.shape()));
    return Var::node(out, std::make_shared<BinaryFwd>(op, l.data, r.data, out), std::move(h));
}
VarDiff binary_diff(int op, const Var& l, const Shared<Gradient>& lg, const History<BackwardEntry>* lh, const Var& r,
                    const Shared<Gradient>& rg, const History<BackwardEntry>* rh) {
    Var var = binary_var(op, l, r);
    History<BackwardEntry> h;
    if (lh) h = *lh;
    if (rh) h.merge(*rh);
    auto grad = std::make_shared<Gradient>(var.device(), var.shape());
    auto bw = std::make_shared<BinaryBwd>();
    bw->op = op; bw->lg = lg; bw->rg = rg; bw->g = grad; bw->l = l.data; bw->r = r.data;
    return VarDiff::node(std::move(var), grad, entry(bw, grad), std::move(h));
}

Var unary_var(Unary k, int axis, const Var& x, Shape out_shape) {
    auto y = zeros_like(x.data, std::move(out_shape));
    return Var::node(y, std::make_shared<UnaryFwd>(k, axis, x.data, y), x.history);
}
VarDiff unary_diff(Unary k, int axis, const VarDiff& x, Shape out_shape) {
    Var var = unary_var(k, axis, x.var, std::move(out_shape));
    auto grad = std::make_shared<Gradient>(var.device(), var.shape());
    auto bw = std::make_shared<UnaryBwd>();
    bw->kind = k; bw->axis = axis; bw->dx = x.grad; bw->g = grad; bw->x = x.var.data; bw->y = var.data;
    return VarDiff::node(std::move(var), grad, entry(bw, grad), x.history);
}

void check_axis(const Shape& s, int axis) {
    if (axis < 0 || axis >= (int)s.size()) panic("axis out of bounds");
}

Shape conv_out_shape(const Shape& in, const Shape& k, const std::vector<int>& stride, const std::vector<int>& dil, int groups) {
    // check_conv_args / check_groups_args / conv_out_shape  utils.rs:207-237, 427-497
    const int nd = (int)in.size() - 2;
    if ((int)stride.size() != nd) panic("Invalid stride for " + std::to_string(nd) + "d conv.");
    if ((int)dil.size() != nd) panic("Invalid dilation for " + std::to_string(nd) + "d conv.");
    if (k.size() != in.size()) panic("Invalid kernel shape for " + std::to_string(nd) + "d conv");
    if (in[1] % groups != 0) panic("In channels " + std::to_string(in[1]) + " is not divisible by groups " + std::to_string(groups));
    if (k[0] % groups != 0) panic("Out channels " + std::to_string(k[0]) + " is not divisible by groups " + std::to_string(groups));
    Shape out{in[0], k[0]};
    for (int d = 0; d < nd; ++d) {
        if (in[2 + d] < (k[2 + d] - 1) * dil[d] + 1) panic("The kernel size can't be greater than actual input size.");
        out.push_back((in[2 + d] - dil[d] * (k[2 + d] - 1) - 1) / stride[d] + 1);
    }
    return out;
}

}  // namespace

// =================================================================================================
// Var
// =================================================================================================
Var Var::leaf(Shared<HipArray> array) {
    Var v;
    v.data = std::move(array);
    return v;
}
Var Var::node(Shared<HipArray> data, Shared<Forward> op, History<ForwardEntry> h) {
    const void* ptr = op.get();
    h.insert(ptr, ForwardEntry{std::move(op), std::make_shared<bool>(false)});
    Var v;
    v.data = std::move(data);
    v.history = std::move(h);
    return v;
}
VarDiff Var::requires_grad() const { return VarDiff::leaf(*this, std::make_shared<Gradient>(device(), shape())); }
void Var::forward() const {
    auto& buffer = history.buffer_mut();
    if (buffer.empty()) buffer = history.to_vec();
    else
        for (auto& e : buffer) *e.computed = false;
    for (auto& e : buffer)
        if (!*e.computed) {
            e.op->forward();
            *e.computed = true;
        }
}
float Var::item() const {
    if (data->len() != 1) panic("item(): not a scalar");
    float v;
    data->download(&v);
    return v;
}
Var Var::sum() const { return unary_var(Unary::Sum, 0, *this, {}); }
Var Var::mean() const { return unary_var(Unary::Mean, 0, *this, {}); }
Var Var::relu() const { return unary_var(Unary::Relu, 0, *this, shape()); }
static Var pointwise_var(int op, int iparam, const Var& x) {
    auto n = std::make_shared<PointwiseFwd>();
    n->op = op; n->iparam = iparam; n->x = x.data; n->y = zeros_like(x.data, x.shape());
    auto y = n->y;
    return Var::node(y, n, x.history);
}
static VarDiff pointwise_diff(int op, int iparam, const VarDiff& x) {
    Var v = pointwise_var(op, iparam, x.var);
    auto g = std::make_shared<Gradient>(v.device(), v.shape());
    auto bw = std::make_shared<PointwiseBwd>();
    bw->op = op; bw->iparam = iparam; bw->dx = x.grad; bw->g = g;
    const bool keeps_output = op == NK_EXP || op == NK_SQRT || op == NK_SIGMOID || op == NK_TANH;
    if (op != NK_NEG) bw->ref = keeps_output ? v.data : x.var.data;
    return VarDiff::node(std::move(v), g, entry(bw, g), x.history);
}
// `gated`: the last axis is halved (it must be even)
static Shared<ActivationFwd> activation_fwd_node(const Var& x, Activation act, bool gated) {
    Shape out = x.shape();
    int H = 0;
    if (gated) {
        if (out.empty() || out.back() % 2 != 0) panic("glu: the last axis must have an even extent");
        H = out.back() / 2;
        out.back() = H;
        if (H == 0) panic("glu: the last axis is empty");
    }
    auto n = std::make_shared<ActivationFwd>();
    n->act = (int)act; n->H = H; n->x = x.data; n->y = zeros_like(x.data, out);
    return n;
}
static Var activation_var(const Var& x, Activation act, bool gated) {
    auto n = activation_fwd_node(x, act, gated);
    auto y = n->y;
    return Var::node(y, n, x.history);
}
static VarDiff activation_diff(const VarDiff& x, Activation act, bool gated) {
    auto n = activation_fwd_node(x.var, act, gated);
    auto y = n->y;
    Var v = Var::node(y, n, x.var.history);
    auto g = std::make_shared<Gradient>(v.device(), v.shape());
    auto bw = std::make_shared<ActivationBwd>();
    bw->act = n->act; bw->H = n->H; bw->x = x.var.data; bw->dx = x.grad; bw->g = g;
    return VarDiff::node(std::move(v), g, entry(bw, g), x.history);
}
Var Var::gelu(bool tanh_approx) const { return activation_var(*this, tanh_approx ? Activation::GeluTanh : Activation::Gelu, false); }
Var Var::silu() const { return activation_var(*this, Activation::Silu, false); }
Var Var::glu(Activation gate) const { return activation_var(*this, gate, true); }
static Shared<RopeFwd> rope_fwd_node(const Var& x, const nn::RotaryEmbedding& r, int batch, int heads) {
    const Shape& s = x.shape();
    if (s.size() != 2 || batch <= 0 || heads <= 0 || s[0] == 0 || s[0] % batch != 0 || s[1] != heads * r.head_dim)
        panic("rope: the input must be (batch*T, heads*head_dim) with head_dim = " + std::to_string(r.head_dim));
    if (s[0] / batch > r.max_pos)
        panic("rope: " + std::to_string(s[0] / batch) + " positions exceed the table's " + std::to_string(r.max_pos));
    if (r.table->device().get() != x.device().get()) panic("rope: the table lives on another device");
    auto n = std::make_shared<RopeFwd>();
    n->rg = rope_geom(r, batch, s[0] / batch, heads);
    n->x = x.data; n->table = r.table; n->y = zeros_like(x.data, s);
    return n;
}
Var Var::rope(const nn::RotaryEmbedding& rotary, int batch, int heads) const {
    auto n = rope_fwd_node(*this, rotary, batch, heads);
    auto y = n->y;
    return Var::node(y, n, history);
}
static Shared<RepeatKvFwd> repeat_kv_fwd_node(const Var& x, int groups, int head_dim) {
    const Shape& s = x.shape();
    if (groups <= 0 || head_dim <= 0) panic("repeat_kv: groups and head_dim must be positive");
    if (s.size() != 2 || s[0] <= 0 || s[1] <= 0 || s[1] % head_dim != 0)
        panic("repeat_kv: the input must be (rows, kv_heads*head_dim) with head_dim = " + std::to_string(head_dim));
    if ((long long)s[1] * groups > (long long)INT_MAX || (unsigned long long)s[0] * s[1] * groups > (unsigned long long)INT_MAX)
        panic("repeat_kv: the output must fit 31 bits");
    auto n = std::make_shared<RepeatKvFwd>();
    n->rows = s[0]; n->Hkv = s[1] / head_dim; n->G = groups; n->dh = head_dim;
    n->x = x.data; n->y = zeros_like(x.data, Shape{s[0], s[1] * groups});
    return n;
}
Var Var::repeat_kv(int groups, int head_dim) const {
    auto n = repeat_kv_fwd_node(*this, groups, head_dim);
    auto y = n->y;
    return Var::node(y, n, history);
}
Var Var::sample(const nn::Sampler& sp, int batch) const {
    const Shape& s = shape();
    if (s.size() != 2 || batch <= 0 || s[0] == 0 || s[0] % batch != 0 || s[1] <= 0)
        panic("sample: the logits must be (batch*T, V) with batch = " + std::to_string(batch) + " dividing the rows");
    if (s[1] > (1 << 20)) panic("sample: V = " + std::to_string(s[1]) + " exceeds 2^20");
    if (!(sp.temperature >= 0.f) || !std::isfinite(sp.temperature)) panic("sample: temperature must be finite and not negative");
    if (!(sp.top_p > 0.f)) panic("sample: top_p must be positive");
    if (sp.dev.get() != device().get()) panic("sample: the sampler lives on another device");
    auto n = std::make_shared<SampleFwd>();
    n->logits = data; n->ids = zeros_like(data, Shape{batch});
    n->batch = batch; n->T = s[0] / batch; n->V = s[1];
    n->temperature = sp.temperature; n->top_k = sp.top_k; n->top_p = sp.top_p; n->seed = sp.seed; n->offset = sp.offset;
    auto y = n->ids;
    return Var::node(y, n, history);
}
Var Var::neg() const { return pointwise_var(NK_NEG, 0, *this); }
Var Var::pow(int e) const { return pointwise_var(NK_POW, e, *this); }
Var Var::sqrt() const { return pointwise_var(NK_SQRT, 0, *this); }
Var Var::leaky_relu() const { return pointwise_var(NK_LEAKY_RELU, 0, *this); }
Var Var::softplus() const { return pointwise_var(NK_SOFTPLUS, 0, *this); }
Var Var::sigmoid() const { return pointwise_var(NK_SIGMOID, 0, *this); }
Var Var::tanh() const { return pointwise_var(NK_TANH, 0, *this); }
Var Var::ln() const { return pointwise_var(NK_LN, 0, *this); }
Var Var::exp() const { return pointwise_var(NK_EXP, 0, *this); }
Var Var::unsqueeze(int axis) const {
    if (axis < 0 || axis > (int)shape().size()) panic("unsqueeze: axis out of bounds");
    Shape s = shape();
    s.insert(s.begin() + axis, 1);
    auto n = std::make_shared<UnsqueezeFwd>();
    n->x = data; n->y = zeros_like(data, s);
    auto y = n->y;
    return Var::node(y, n, history);
}
Var Var::max_pool(const std::vector<int>& kernel, const std::vector<int>& stride, const std::vector<int>& padding) const {
    return pool_var("max_pool", *this, kernel, stride, padding, false, true);
}
Var Var::avg_pool(const std::vector<int>& kernel, const std::vector<int>& stride, const std::vector<int>& padding, bool count_include_pad) const {
    return pool_var("avg_pool", *this, kernel, stride, padding, true, count_include_pad);
}
Var Var::upsample(const std::vector<int>& out_size, const std::string& mode, bool align_corners) const {
    auto n = upsample_fwd_node(*this, out_size, mode, align_corners);
    auto y = n->y;
    return Var::node(y, n, history);
}
Var Var::global_avg_pool() const {
    const std::vector<int> k = spatial_extents("global_avg_pool", shape());
    return pool_var("global_avg_pool", *this, k, k, std::vector<int>(k.size(), 0), true, true);
}
Var Var::flatten() const {  // the Unsqueeze node with another shape: a copy into the reshaped buffer
    auto n = std::make_shared<UnsqueezeFwd>();
    n->x = data; n->y = zeros_like(data, flat_shape(shape()));
    auto y = n->y;
    return Var::node(y, n, history);
}
Var Var::softmax(int axis) const { check_axis(shape(), axis); return unary_var(Unary::Softmax, axis, *this, shape()); }
Var Var::log_softmax(int axis) const { check_axis(shape(), axis); return unary_var(Unary::LogSoftmax, axis, *this, shape()); }
Var Var::t() const { return unary_var(Unary::Transpose, 0, *this, Shape(shape().rbegin(), shape().rend())); }
Var Var::layer_norm(const Var& gamma, const Var& beta, double eps) const { return layer_norm_var(*this, &gamma, &beta, gamma.shape(), eps); }
Var Var::layer_norm(const Shape& normalized_shape, double eps) const { return layer_norm_var(*this, nullptr, nullptr, normalized_shape, eps); }
VarDiff Var::layer_norm(const VarDiff& gamma, const VarDiff& beta, double eps) const {
    return layer_norm_diff(*this, nullptr, nullptr, &gamma.var, gamma.grad, &gamma.history, &beta.var, beta.grad, &beta.history, gamma.shape(), eps);
}
Var Var::rms_norm(const Var& gamma, double eps) const { return rms_norm_var(*this, &gamma, gamma.shape(), eps); }
Var Var::rms_norm(const Shape& normalized_shape, double eps) const { return rms_norm_var(*this, nullptr, normalized_shape, eps); }
VarDiff Var::rms_norm(const VarDiff& gamma, double eps) const {
    return rms_norm_diff(*this, nullptr, nullptr, &gamma.var, gamma.grad, &gamma.history, gamma.shape(), eps);
}
Var Var::group_norm(int num_groups, const Var& gamma, const Var& beta, double eps) const { return group_norm_var(*this, num_groups, &gamma, &beta, eps); }
Var Var::group_norm(int num_groups, double eps) const { return group_norm_var(*this, num_groups, nullptr, nullptr, eps); }
VarDiff Var::group_norm(int num_groups, const VarDiff& gamma, const VarDiff& beta, double eps) const {
    return group_norm_diff(*this, nullptr, nullptr, num_groups, &gamma.var, gamma.grad, &gamma.history, &beta.var, beta.grad, &beta.history, eps);
}
Var Var::batch_norm(const Var* gamma, const Var* beta, const Var* running_mean, const Var* running_var, double momentum, double eps,
                    Shared<bool> status) const {
    return batch_norm_var(*this, gamma, beta, running_mean, running_var, momentum, eps, std::move(status));
}
VarDiff Var::batch_norm(const VarDiff& gamma, const VarDiff& beta, const Var* running_mean, const Var* running_var, double momentum, double eps,
                        Shared<bool> status) const {
    return batch_norm_diff(*this, nullptr, nullptr, &gamma.var, gamma.grad, &gamma.history, &beta.var, beta.grad, &beta.history, running_mean,
                           running_var, momentum, eps, std::move(status));
}
Var Var::dropout(double p, Shared<bool> status) const {
    if (!(p >= 0.0 && p <= 1.0)) panic("Wrong probability received: " + std::to_string(p) + ".");
    auto op = std::make_shared<DropoutFwd>();
    op->x = data; op->y = zeros_like(data, shape()); op->noise = zeros_like(data, shape());
    op->p = p; op->status = std::move(status);
    op->seed = next_node_seed();
    op->calls = std::make_shared<uint64_t>(0);
    auto y = op->y;
    return Var::node(y, op, history);
}
std::vector<Var> Var::chunks(const Shape& chunk_size) const {
    if (chunk_size.size() != shape().size()) panic("chunks: rank mismatch");
    size_t n = 1;
    for (size_t i = 0; i < chunk_size.size(); ++i) {
        if (chunk_size[i] <= 0) panic("chunks: chunk size must be positive");
        n *= (size_t)(shape()[i] / chunk_size[i]);
    }
    std::vector<Var> out;
    for (size_t i = 0; i < n; ++i) {
        auto op = std::make_shared<ChunkFwd>();
        op->x = data; op->y = zeros_like(data, chunk_size); op->chunk_no = (int)i;
        auto y = op->y;
        out.push_back(Var::node(y, op, history));
    }
    return out;
}
Var Var::cat(const std::vector<Var>& variables, int axis) const {
    check_axis(shape(), axis);
    History<ForwardEntry> h = history;
    auto op = std::make_shared<CatFwd>();
    op->operands.push_back(data);
    Shape s = shape();
    for (const Var& v : variables) {
        h.merge(v.history);
        op->operands.push_back(v.data);
        for (size_t i = 0; i < s.size(); ++i)
            if ((int)i != axis && v.shape()[i] != s[i]) panic("cat: incompatible shapes");
        s[axis] += v.shape()[axis];
    }
    op->axis = axis;
    op->out = zeros_like(data, s);
    auto y = op->out;
    return Var::node(y, op, std::move(h));
}
Var Var::stack(const std::vector<Var>& variables, int axis) const {
    if (axis < 0 || axis > (int)shape().size()) panic("stack: axis out of bounds");
    History<ForwardEntry> h = history;
    auto op = std::make_shared<CatFwd>();
    op->operands.push_back(data);
    for (const Var& v : variables) {
        if (v.shape() != shape()) panic("stack: all the variables must have the same shape");
        h.merge(v.history);
        op->operands.push_back(v.data);
    }
    Shape s = shape();
    s.insert(s.begin() + axis, (int)variables.size() + 1);
    op->axis = axis; op->stack = true;
    op->out = zeros_like(data, s);
    auto y = op->out;
    return Var::node(y, op, std::move(h));
}
static Var loss_var(int kind, const Var& x, const Var& target, Reduction reduction) {
    if (kind < 0) {  // nll: target has the input's shape without the class axis (var.rs:661)
        Shape want = x.shape();
        if (want.size() < 2) panic("nll: input of shape (minibatch, C, ...) expected");
        want.erase(want.begin() + 1);
        if (target.shape() != want) panic("nll: target must have shape (minibatch, d1, ..., dk)");
    } else if (target.shape() != x.shape()) {
        panic("loss: input and target shapes differ");
    }
    History<ForwardEntry> h = x.history;
    h.merge(target.history);
    auto op = std::make_shared<LossFwd>();
    op->kind = kind; op->x = x.data; op->t = target.data; op->out = zeros_like(x.data, {}); op->red = reduction;
    auto y = op->out;
    return Var::node(y, op, std::move(h));
}
static VarDiff loss_diff(int kind, const VarDiff& x, const Var& target, Reduction reduction) {
    Var out = loss_var(kind, x.var, target, reduction);
    auto g = std::make_shared<Gradient>(x.device(), Shape{});
    auto bw = std::make_shared<LossBwd>();
    bw->kind = kind; bw->x = x.var.data; bw->t = target.data; bw->dx = x.grad; bw->g = g; bw->red = reduction;
    return VarDiff::node(std::move(out), g, entry(bw, g), x.history);
}
static Shared<CrossEntropyFwd> cross_entropy_fwd_node(const Var& x, const Var& target, Reduction reduction, long ignore_index, double label_smoothing) {
    Shape want = x.shape();
    if (want.size() < 2) panic("cross_entropy: input of shape (minibatch, C, ...) expected");
    want.erase(want.begin() + 1);
    if (target.shape() != want) panic("cross_entropy: target must have shape (minibatch, d1, ..., dk)");
    if (!(label_smoothing >= 0.0 && label_smoothing < 1.0)) panic("cross_entropy: label_smoothing must be in [0, 1), got " + std::to_string(label_smoothing));
    if (target.device().get() != x.device().get()) panic("cross_entropy: logits and target live on different devices");
    auto op = std::make_shared<CrossEntropyFwd>();
    op->x = x.data; op->t = target.data; op->lse = zeros_like(x.data, want); op->out = zeros_like(x.data, {});
    op->red = reduction; op->ignore_index = ignore_index < 0 ? -1 : ignore_index; op->label_smoothing = label_smoothing;
    return op;
}
Var Var::cross_entropy(const Var& target, Reduction reduction, long ignore_index, double label_smoothing) const {
    auto op = cross_entropy_fwd_node(*this, target, reduction, ignore_index, label_smoothing);
    History<ForwardEntry> h = history;
    h.merge(target.history);
    auto y = op->out;
    return Var::node(y, op, std::move(h));
}
VarDiff VarDiff::cross_entropy(const Var& target, Reduction reduction, long ignore_index, double label_smoothing) const {
    auto op = cross_entropy_fwd_node(var, target, reduction, ignore_index, label_smoothing);
    History<ForwardEntry> h = var.history;
    h.merge(target.history);
    auto y = op->out;
    Var out = Var::node(y, op, std::move(h));
    auto g = std::make_shared<Gradient>(device(), Shape{});
    auto bw = std::make_shared<CrossEntropyBwd>();
    bw->x = var.data; bw->t = target.data; bw->lse = op->lse; bw->dx = grad; bw->g = g;
    bw->red = reduction; bw->ignore_index = op->ignore_index; bw->label_smoothing = label_smoothing;
    return VarDiff::node(std::move(out), g, entry(bw, g), history);
}
Var Var::mae(const Var& t, Reduction r) const { return loss_var(NK_LOSS_MAE, *this, t, r); }
Var Var::bce(const Var& t, Reduction r) const { return loss_var(NK_LOSS_BCE, *this, t, r); }
Var Var::bce_with_logits(const Var& t, Reduction r) const { return loss_var(NK_LOSS_BCE_WITH_LOGITS, *this, t, r); }
Var Var::kldiv(const Var& t, Reduction r) const { return loss_var(NK_LOSS_KLDIV, *this, t, r); }
Var Var::nll(const Var& t, Reduction r) const { return loss_var(-1, *this, t, r); }
VarDiff VarDiff::mae(const Var& t, Reduction r) const { return loss_diff(NK_LOSS_MAE, *this, t, r); }
VarDiff VarDiff::bce(const Var& t, Reduction r) const { return loss_diff(NK_LOSS_BCE, *this, t, r); }
VarDiff VarDiff::bce_with_logits(const Var& t, Reduction r) const { return loss_diff(NK_LOSS_BCE_WITH_LOGITS, *this, t, r); }
VarDiff VarDiff::kldiv(const Var& t, Reduction r) const { return loss_diff(NK_LOSS_KLDIV, *this, t, r); }
VarDiff VarDiff::nll(const Var& t, Reduction r) const { return loss_diff(-1, *this, t, r); }
Var Var::mv(const Var& rhs) const { return matmul_var(4, *this, rhs); }
VarDiff Var::mv(const VarDiff& rhs) const { return matmul_diff(4, *this, nullptr, nullptr, rhs.var, rhs.grad, &rhs.history); }
Var Var::vm(const Var& rhs) const { return matmul_var(5, *this, rhs); }
VarDiff Var::vm(const VarDiff& rhs) const { return matmul_diff(5, *this, nullptr, nullptr, rhs.var, rhs.grad, &rhs.history); }
Var Var::vv(const Var& rhs) const { return matmul_var(6, *this, rhs); }
VarDiff Var::vv(const VarDiff& rhs) const { return matmul_diff(6, *this, nullptr, nullptr, rhs.var, rhs.grad, &rhs.history); }
VarDiff VarDiff::mv(const Var& rhs) const { return matmul_diff(4, var, grad, &history, rhs, nullptr, nullptr); }
VarDiff VarDiff::mv(const VarDiff& rhs) const { return matmul_diff(4, var, grad, &history, rhs.var, rhs.grad, &rhs.history); }
VarDiff VarDiff::vm(const Var& rhs) const { return matmul_diff(5, var, grad, &history, rhs, nullptr, nullptr); }
VarDiff VarDiff::vm(const VarDiff& rhs) const { return matmul_diff(5, var, grad, &history, rhs.var, rhs.grad, &rhs.history); }
VarDiff VarDiff::vv(const Var& rhs) const { return matmul_diff(6, var, grad, &history, rhs, nullptr, nullptr); }
VarDiff VarDiff::vv(const VarDiff& rhs) const { return matmul_diff(6, var, grad, &history, rhs.var, rhs.grad, &rhs.history); }
Var Var::mse(const Var& target, Reduction reduction) const {
    if (target.shape() != shape()) panic("mse: input and target shapes differ");
    History<ForwardEntry> h = history;
    h.merge(target.history);
    auto op = std::make_shared<MseFwd>();
    op->x = data; op->t = target.data; op->out = zeros_like(data, {}); op->red = reduction;
    auto y = op->out;
    return Var::node(y, op, std::move(h));
}
Var Var::pad(const std::vector<int>& padding, float value) const { return pad(padding, PaddingMode::constant(value)); }
Var Var::pad(const std::vector<int>& padding, PaddingMode mode) const {
    if (padding.size() + 2 != shape().size()) panic("pad: one padding per spatial dimension expected");
    Shape s = shape();
    for (size_t i = 0; i < padding.size(); ++i) s[2 + i] += 2 * padding[i];
    auto op = std::make_shared<PadFwd>();
    op->x = data; op->y = zeros_like(data, s); op->padding = padding; op->mode = mode;
    auto y = op->y;
    return Var::node(y, op, history);
}
Var Var::mm(const Var& rhs) const { return matmul_var(0, *this, rhs); }
VarDiff Var::mm(const VarDiff& rhs) const { return matmul_diff(0, *this, nullptr, nullptr, rhs.var, rhs.grad, &rhs.history); }
Var Var::mm_t(const Var& rhs) const { return matmul_var(1, *this, rhs); }
VarDiff Var::mm_t(const VarDiff& rhs) const { return matmul_diff(1, *this, nullptr, nullptr, rhs.var, rhs.grad, &rhs.history); }
static void check_heads(const Shape& flat, const Shape& cube, int B, int S, int H, int dh, bool with_cube) {
    if (B <= 0 || S <= 0 || H <= 0 || dh <= 0) panic("heads: non-positive geometry");
    if (flat != Shape{B * S, H * dh}) panic("heads: the projection operand must have shape (B*S, H*dh)");
    if (with_cube && cube != Shape{B * H, S, S}) panic("heads: the probabilities must have shape (B*H, S, S)");
}
Var Var::heads_scores(const Var& keys, int B, int S, int H, int dh) const {
    check_heads(shape(), {}, B, S, H, dh, false);
    check_heads(keys.shape(), {}, B, S, H, dh, false);
    History<ForwardEntry> h = history;
    h.merge(keys.history);
    auto op = std::make_shared<HeadsScoresFwd>();
    op->hg = {B, S, H, dh}; op->q = data; op->k = keys.data; op->c = zeros_like(data, Shape{B * H, S, S});
    auto y = op->c;
    return Var::node(y, op, std::move(h));
}
Var Var::heads_context(const Var& values, int B, int S, int H, int dh) const {
    check_heads(values.shape(), shape(), B, S, H, dh, true);
    History<ForwardEntry> h = history;
    h.merge(values.history);
    auto op = std::make_shared<HeadsContextFwd>();
    op->hg = {B, S, H, dh}; op->p = data; op->v = values.data; op->o = zeros_like(data, Shape{B * S, H * dh});
    auto y = op->o;
    return Var::node(y, op, std::move(h));
}
VarDiff VarDiff::heads_scores(const VarDiff& keys, int B, int S, int H, int dh) const {
    Var out = var.heads_scores(keys.var, B, S, H, dh);
    History<BackwardEntry> h = history;
    h.merge(keys.history);
    auto g = std::make_shared<Gradient>(out.device(), out.shape());
    auto bw = std::make_shared<HeadsScoresBwd>();
    bw->hg = {B, S, H, dh}; bw->q = var.data; bw->k = keys.var.data; bw->dq = grad; bw->dk = keys.grad; bw->g = g;
    return VarDiff::node(std::move(out), g, entry(bw, g), std::move(h));
}
VarDiff VarDiff::heads_context(const VarDiff& values, int B, int S, int H, int dh) const {
    Var out = var.heads_context(values.var, B, S, H, dh);
    History<BackwardEntry> h = history;
    h.merge(values.history);
    auto g = std::make_shared<Gradient>(out.device(), out.shape());
    auto bw = std::make_shared<HeadsContextBwd>();
    bw->hg = {B, S, H, dh}; bw->p = var.data; bw->v = values.var.data; bw->dp = grad; bw->dv = values.grad; bw->g = g;
    return VarDiff::node(std::move(out), g, entry(bw, g), std::move(h));
}
bool Var::attention_core_supported(int S, int dh, double p) { return nk_attention_supported(S, dh, p, 1) != 0; }
static Shared<HeadsAttentionFwd> heads_attention_node(const Var& q, const Var& keys, const Var& values, int B, int S, int H, int dh, float scale,
                                                      double p, Shared<bool> status, bool keep, bool causal, int window,
                                                      const nn::Segments* segments) {
    const FormRefusals refuse{"heads_attention", causal};
    refuse.window(window);
    refuse.segments(segments, B, S, q.device().get());
    if (!(p >= 0.0 && p <= 1.0)) panic("Wrong probability received: " + std::to_string(p) + ".");
    check_heads(q.shape(), {}, B, S, H, dh, false);
    check_heads(keys.shape(), {}, B, S, H, dh, false);
    check_heads(values.shape(), {}, B, S, H, dh, false);
    if (!Var::attention_core_supported(S, dh, p)) panic("heads_attention: the fused kernels take dh in {32, 64, 128} and p < 1");
    auto op = std::make_shared<HeadsAttentionFwd>();
    op->q = q.data; op->k = keys.data; op->v = values.data;
    op->core = AttnCore::build(q.data, B, S, H, dh, scale, p, std::move(status), causal, window, segments, keep);
    op->o = zeros_like(q.data, Shape{B * S, H * dh});
    return op;
}
static Var heads_attention_var(const Var& q, const Var& keys, const Var& values, const Shared<HeadsAttentionFwd>& op) {
    History<ForwardEntry> h = q.history;
    h.merge(keys.history);
    h.merge(values.history);
    auto y = op->o;
    return Var::node(y, op, std::move(h));
}
Var Var::heads_attention(const Var& keys, const Var& values, int B, int S, int H, int dh, float scale, double p,
                         Shared<bool> status, bool causal, int window, const nn::Segments* segments) const {
    return heads_attention_var(*this, keys, values,
                               heads_attention_node(*this, keys, values, B, S, H, dh, scale, p, std::move(status), false, causal, window, segments));
}
VarDiff VarDiff::heads_attention(const VarDiff& keys, const VarDiff& values, int B, int S, int H, int dh, float scale, double p,
                                 Shared<bool> status, bool causal, int window, const nn::Segments* segments) const {
    auto fwd = heads_attention_node(var, keys.var, values.var, B, S, H, dh, scale, p, std::move(status), true, causal, window, segments);
    Var out = heads_attention_var(var, keys.var, values.var, fwd);
    History<BackwardEntry> h = history;
    h.merge(keys.history);
    h.merge(values.history);
    auto g = std::make_shared<Gradient>(out.device(), out.shape());
    auto bw = std::make_shared<HeadsAttentionBwd>();
    bw->core = fwd->core;
    bw->core.add_backward_scratch();
    bw->q = fwd->q; bw->k = fwd->k; bw->v = fwd->v; bw->o = fwd->o;
    bw->dq = grad; bw->dk = keys.grad; bw->dv = values.grad; bw->g = g;
    return VarDiff::node(std::move(out), g, entry(bw, g), std::move(h));
}
Var Var::bmm(const Var& rhs) const { return matmul_var(2, *this, rhs); }
Var Var::bmm_t(const Var& rhs) const { return matmul_var(3, *this, rhs); }
Var Var::attention_probs(float scale, double p, Shared<bool> status, bool store_probs) const {
    if (!(p >= 0.0 && p <= 1.0)) panic("Wrong probability received: " + std::to_string(p) + ".");
    if (shape().empty()) panic("attention_probs: at least one axis expected");
    auto op = std::make_shared<AttnProbsFwd>();
    op->x = data; op->out = zeros_like(data, shape());
    if (store_probs) op->probs = zeros_like(data, shape());
    op->scale = scale; op->p = p; op->status = std::move(status);
    op->seed = next_node_seed();
    op->calls = std::make_shared<uint64_t>(0);
    op->last_offset = std::make_shared<uint64_t>(0);
    auto y = op->out;
    return Var::node(y, op, history);
}
Var Var::convolution(const Var& input, const std::vector<int>& stride, const std::vector<int>& dilation, int groups) const {
    Shape kfull = shape();  // kernel (Cout, Cin/groups, k...) checked against the input
    Shape kcheck = kfull;
    kcheck[1] *= groups;
    (void)kcheck;
    Shape out = conv_out_shape(input.shape(), kfull, stride, dilation, groups);
    History<ForwardEntry> h = history;
    h.merge(input.history);
    auto op = std::make_shared<ConvFwd>();
    op->x = input.data; op->w = data; op->y = zeros_like(data, out); op->stride = stride; op->dilation = dilation; op->groups = groups;
    auto y = op->y;
    return Var::node(y, op, std::move(h));
}
static Var heads_var(bool split, const Var& x, int B, int S, int H, int dh) {
    auto op = std::make_shared<HeadsFwd>();
    op->split = split; op->x = x.data; op->B = B; op->S = S; op->H = H; op->dh = dh;
    const Shape want = split ? Shape{B * S, H * dh} : Shape{B * H, S, dh};
    if (x.shape() != want) panic("split/merge heads: unexpected input shape");
    op->y = zeros_like(x.data, split ? Shape{B * H, S, dh} : Shape{B * S, H * dh});
    auto y = op->y;
    return Var::node(y, op, x.history);
}
Var Var::split_heads(int B, int S, int H, int dh) const { return heads_var(true, *this, B, S, H, dh); }
Var Var::merge_heads(int B, int S, int H, int dh) const { return heads_var(false, *this, B, S, H, dh); }

// =================================================================================================
// VarDiff
// =================================================================================================
VarDiff VarDiff::leaf(Var var, Shared<Gradient> grad) {
    VarDiff v;
    v.var = std::move(var);
    v.grad = std::move(grad);
    return v;
}
VarDiff VarDiff::node(Var var, Shared<Gradient> grad, BackwardEntry op, History<BackwardEntry> h) {
    const void* ptr = op.op.get();
    h.insert(ptr, std::move(op));
    VarDiff v;
    v.var = std::move(var);
    v.grad = std::move(grad);
    v.history = std::move(h);
    return v;
}
void VarDiff::zero_grad() const { grad->zero(); }
void VarDiff::forward() const {
    var.forward();
    auto& buffer = history.buffer_mut();
    if (buffer.empty()) buffer = history.to_vec();
}
static thread_local BackwardHook* g_active_hook = nullptr;
// gradients whose LAST writer on the tape is the node whose backward() is running now
static thread_local const std::vector<const Gradient*>* g_final_here = nullptr;
BackwardHook* parts_hook(const Gradient* g) {
    if (!g_active_hook || !g_final_here) return nullptr;
    if (std::find(g_final_here->begin(), g_final_here->end(), g) == g_final_here->end()) return nullptr;
    return g_active_hook->wants_parts(g) ? g_active_hook : nullptr;
}
namespace {
struct ActiveHookScope {
    explicit ActiveHookScope(BackwardHook* h) { g_active_hook = h; }
    ~ActiveHookScope() { g_active_hook = nullptr; g_final_here = nullptr; }
};
}  // namespace

void VarDiff::backward(float seed, BackwardHook* hook) const {
    if (var.history.len() != var.history.buffer_len()) panic("Perhaps you forgot to call .forward()?");
    {
        bool assign = false;
        grad->borrow_first_write(assign).fill(seed);  // `grad_mut().fill(seed)` vardiff.rs:133
    }
    run_backward(hook);
}
void VarDiff::backward_from(const Var& seed, BackwardHook* hook) const {
    if (var.history.len() != var.history.buffer_len()) panic("Perhaps you forgot to call .forward()?");
    if (seed.shape() != shape()) panic("backward_from: the seed must have the shape of the root");
    // the root's backward nodes read the root gradient through `borrow()` when they run: let them see the seed's buffer
    const bool was_pending = grad->zero_pending();
    Shared<HipArray> own = grad->exchange_array(seed.data);
    struct Restore {
        const Shared<Gradient>& g; Shared<HipArray>& own; bool pending;
        ~Restore() { g->exchange_array(own); if (pending) g->zero(); }
    } restore{grad, own, was_pending};
    run_backward(hook);
}
// Pre-masked gradients (fused Linear+ReLU): a gradient that names a mask source is written pre-masked in THIS pass iff
// every tape node that writes it can do so.
static void decide_premasked(const std::vector<BackwardEntry>& buffer) {
    std::unordered_map<const Gradient*, std::pair<int, int>> count;  // gradient -> (writers, mask-capable writers)
    std::vector<const Gradient*> ts;
    for (const BackwardEntry& e : buffer) {
        if (const auto* own = dynamic_cast<const Gradient*>(e.grad.get()))
            if (own->premask_source()) count[own];  // a root has no writers: it is seeded with plain values
        ts.clear();
        e.op->targets(ts);
        for (const Gradient* g : ts)
            if (g->premask_source()) ++count[g].first;
        ts.clear();
        e.op->premask_targets(ts);
        for (const Gradient* g : ts) ++count[g].second;
    }
    for (const auto& kv : count) kv.first->set_premasked(kv.second.first > 0 && kv.second.first == kv.second.second);
}
void VarDiff::run_backward(BackwardHook* hook) const {
    auto& buffer = history.buffer_mut();
    decide_premasked(buffer);
    if (!hook) {
        for (auto it = buffer.rbegin(); it != buffer.rend(); ++it) it->op->backward();
        return;
    }
    ActiveHookScope scope(hook);
    // a gradient is final once the last node (in reverse order) that accumulates into it ran
    std::unordered_map<const Gradient*, size_t> last;
    std::vector<const Gradient*> ts, final_here;
    for (size_t i = 0; i < buffer.size(); ++i) {  // reverse execution order: index 0 runs last
        ts.clear();
        buffer[i].op->targets(ts);
        for (const Gradient* g : ts)
            if (!last.count(g)) last[g] = i;  // smallest index = last to run
    }
    for (size_t k = buffer.size(); k-- > 0;) {
        ts.clear();
        buffer[k].op->targets(ts);
        final_here.clear();
        for (const Gradient* g : ts)
            if (last[g] == k && std::find(final_here.begin(), final_here.end(), g) == final_here.end()) final_here.push_back(g);
        g_final_here = &final_here;  // what `parts_hook` answers for while this node runs
        buffer[k].op->backward();
        g_final_here = nullptr;
        for (const Gradient* g : final_here) hook->grad_ready(g);
    }
}
void VarDiff::no_grad() const {
    auto& buffer = history.buffer_mut();
    if (buffer.empty()) buffer = history.to_vec();
    for (auto& e : buffer) e.grad->no_grad();
}
void VarDiff::with_grad() const {
    auto& buffer = history.buffer_mut();
    if (buffer.empty()) buffer = history.to_vec();
    for (auto& e : buffer) e.grad->with_grad();
}

VarDiff VarDiff::sum() const { return unary_diff(Unary::Sum, 0, *this, {}); }
VarDiff VarDiff::mean() const { return unary_diff(Unary::Mean, 0, *this, {}); }
static thread_local bool g_relu_peephole = true;
namespace nn {
bool set_relu_peephole(bool on) { const bool was = g_relu_peephole; g_relu_peephole = on; return was; }
VarDiff linear_relu_from_origin(const LinearOrigin& o);
}  // namespace nn
VarDiff VarDiff::relu() const& { return unary_diff(Unary::Relu, 0, *this, shape()); }
VarDiff VarDiff::relu() && {
    // `lin.forward(x).relu()`: one Linear+ReLU node over the Linear's operands (see `linear_origin`); the temporary never runs
    if (linear_origin && g_relu_peephole) return nn::linear_relu_from_origin(*linear_origin);
    return unary_diff(Unary::Relu, 0, *this, shape());
}
VarDiff VarDiff::neg() const { return pointwise_diff(NK_NEG, 0, *this); }
VarDiff VarDiff::pow(int e) const { return pointwise_diff(NK_POW, e, *this); }
VarDiff VarDiff::sqrt() const { return pointwise_diff(NK_SQRT, 0, *this); }
VarDiff VarDiff::leaky_relu() const { return pointwise_diff(NK_LEAKY_RELU, 0, *this); }
VarDiff VarDiff::softplus() const { return pointwise_diff(NK_SOFTPLUS, 0, *this); }
VarDiff VarDiff::sigmoid() const { return pointwise_diff(NK_SIGMOID, 0, *this); }
VarDiff VarDiff::gelu(bool tanh_approx) const { return activation_diff(*this, tanh_approx ? Activation::GeluTanh : Activation::Gelu, false); }
VarDiff VarDiff::silu() const { return activation_diff(*this, Activation::Silu, false); }
VarDiff VarDiff::glu(Activation gate) const { return activation_diff(*this, gate, true); }
VarDiff VarDiff::rope(const nn::RotaryEmbedding& rotary, int batch, int heads) const {
    auto n = rope_fwd_node(var, rotary, batch, heads);
    auto y = n->y;
    Var v = Var::node(y, n, var.history);
    auto g = std::make_shared<Gradient>(v.device(), v.shape());
    auto bw = std::make_shared<RopeBwd>();
    bw->rg = n->rg; bw->table = n->table; bw->dx = grad; bw->g = g;
    return VarDiff::node(std::move(v), g, entry(bw, g), history);
}
// Packed sequences on the unpacked paths: the rope node with every ROW at its own position (nk_rope_* with B := rows, T := 1,
// start := positions, one int32 per row).  File-local: the positions are nn::Segments' pos, which forward() holds below max_pos.
static VarDiff rope_rows(const VarDiff& x, const nn::RotaryEmbedding& rotary, int heads, const Shared<HipArray>& positions) {
    if (!positions || x.shape().empty() || (int)positions->len() != x.shape()[0]) panic("rope: one position per row expected");
    auto n = rope_fwd_node(x.var, rotary, x.shape()[0], heads);
    n->start = positions;
    auto y = n->y;
    Var v = Var::node(y, n, x.var.history);
    auto g = std::make_shared<Gradient>(v.device(), v.shape());
    auto bw = std::make_shared<RopeBwd>();
    bw->rg = n->rg; bw->table = n->table; bw->start = n->start; bw->dx = x.grad; bw->g = g;
    return VarDiff::node(std::move(v), g, entry(bw, g), x.history);
}
VarDiff VarDiff::repeat_kv(int groups, int head_dim) const {
    auto n = repeat_kv_fwd_node(var, groups, head_dim);
    auto y = n->y;
    Var v = Var::node(y, n, var.history);
    auto g = std::make_shared<Gradient>(v.device(), v.shape());
    auto bw = std::make_shared<RepeatKvBwd>();
    bw->rows = n->rows; bw->Hkv = n->Hkv; bw->G = n->G; bw->dh = n->dh; bw->dx = grad; bw->g = g;
    return VarDiff::node(std::move(v), g, entry(bw, g), history);
}
VarDiff VarDiff::tanh() const { return pointwise_diff(NK_TANH, 0, *this); }
VarDiff VarDiff::ln() const { return pointwise_diff(NK_LN, 0, *this); }
VarDiff VarDiff::exp() const { return pointwise_diff(NK_EXP, 0, *this); }
VarDiff VarDiff::unsqueeze(int axis) const {
    Var v = var.unsqueeze(axis);
    auto g = std::make_shared<Gradient>(v.device(), v.shape());
    auto bw = std::make_shared<UnsqueezeBwd>();
    bw->dx = grad; bw->g = g;
    return VarDiff::node(std::move(v), g, entry(bw, g), history);
}
VarDiff VarDiff::max_pool(const std::vector<int>& kernel, const std::vector<int>& stride, const std::vector<int>& padding) const {
    return pool_diff("max_pool", *this, kernel, stride, padding, false, true);
}
VarDiff VarDiff::avg_pool(const std::vector<int>& kernel, const std::vector<int>& stride, const std::vector<int>& padding, bool count_include_pad) const {
    return pool_diff("avg_pool", *this, kernel, stride, padding, true, count_include_pad);
}
VarDiff VarDiff::upsample(const std::vector<int>& out_size, const std::string& mode, bool align_corners) const {
    auto n = upsample_fwd_node(var, out_size, mode, align_corners);
    auto y = n->y;
    Var v = Var::node(y, n, var.history);
    auto g = std::make_shared<Gradient>(v.device(), v.shape());
    auto bw = std::make_shared<UpsampleBwd>();
    bw->dx = grad; bw->g = g; bw->x_shape = shape(); bw->out_size = n->out_size; bw->mode = n->mode; bw->align_corners = n->align_corners;
    return VarDiff::node(std::move(v), g, entry(bw, g), history);
}
VarDiff VarDiff::global_avg_pool() const {
    const std::vector<int> k = spatial_extents("global_avg_pool", shape());
    return pool_diff("global_avg_pool", *this, k, k, std::vector<int>(k.size(), 0), true, true);
}
VarDiff VarDiff::flatten() const {
    Var v = var.flatten();
    auto g = std::make_shared<Gradient>(v.device(), v.shape());
    auto bw = std::make_shared<UnsqueezeBwd>();
    bw->dx = grad; bw->g = g;
    return VarDiff::node(std::move(v), g, entry(bw, g), history);
}
VarDiff VarDiff::softmax(int axis) const { check_axis(shape(), axis); return unary_diff(Unary::Softmax, axis, *this, shape()); }
VarDiff VarDiff::log_softmax(int axis) const { check_axis(shape(), axis); return unary_diff(Unary::LogSoftmax, axis, *this, shape()); }
VarDiff VarDiff::t() const { return unary_diff(Unary::Transpose, 0, *this, Shape(shape().rbegin(), shape().rend())); }
VarDiff VarDiff::layer_norm(const VarDiff& gamma, const VarDiff& beta, double eps) const {
    return layer_norm_diff(var, grad, &history, &gamma.var, gamma.grad, &gamma.history, &beta.var, beta.grad, &beta.history, gamma.shape(), eps);
}
VarDiff VarDiff::layer_norm(const Var& gamma, const Var& beta, double eps) const {
    return layer_norm_diff(var, grad, &history, &gamma, nullptr, nullptr, &beta, nullptr, nullptr, gamma.shape(), eps);
}
VarDiff VarDiff::layer_norm(const Shape& normalized_shape, double eps) const {
    return layer_norm_diff(var, grad, &history, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, normalized_shape, eps);
}
VarDiff VarDiff::rms_norm(const VarDiff& gamma, double eps) const {
    return rms_norm_diff(var, grad, &history, &gamma.var, gamma.grad, &gamma.history, gamma.shape(), eps);
}
VarDiff VarDiff::rms_norm(const Var& gamma, double eps) const {
    return rms_norm_diff(var, grad, &history, &gamma, nullptr, nullptr, gamma.shape(), eps);
}
VarDiff VarDiff::rms_norm(const Shape& normalized_shape, double eps) const {
    return rms_norm_diff(var, grad, &history, nullptr, nullptr, nullptr, normalized_shape, eps);
}
VarDiff VarDiff::group_norm(int num_groups, const VarDiff& gamma, const VarDiff& beta, double eps) const {
    return group_norm_diff(var, grad, &history, num_groups, &gamma.var, gamma.grad, &gamma.history, &beta.var, beta.grad, &beta.history, eps);
}
VarDiff VarDiff::group_norm(int num_groups, const Var& gamma, const Var& beta, double eps) const {
    return group_norm_diff(var, grad, &history, num_groups, &gamma, nullptr, nullptr, &beta, nullptr, nullptr, eps);
}
VarDiff VarDiff::group_norm(int num_groups, double eps) const {
    return group_norm_diff(var, grad, &history, num_groups, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, eps);
}
VarDiff VarDiff::embedding(const Var& indices, long padding_idx) const {
    auto n = embedding_fwd_node(var, indices, padding_idx);
    auto y = n->y;
    History<ForwardEntry> fh = var.history;
    fh.merge(indices.history);
    Var v = Var::node(y, n, std::move(fh));
    auto g = std::make_shared<Gradient>(v.device(), v.shape());
    auto bw = std::make_shared<EmbeddingBwd>();
    bw->dw = grad; bw->g = g; bw->idx = indices.data; bw->padding_idx = padding_idx < 0 ? -1 : padding_idx;
    return VarDiff::node(std::move(v), g, entry(bw, g), history);
}
VarDiff VarDiff::batch_norm(const VarDiff& gamma, const VarDiff& beta, const Var* running_mean, const Var* running_var, double momentum, double eps,
                            Shared<bool> status) const {
    return batch_norm_diff(var, grad, &history, &gamma.var, gamma.grad, &gamma.history, &beta.var, beta.grad, &beta.history, running_mean, running_var,
                           momentum, eps, std::move(status));
}
VarDiff VarDiff::batch_norm(const Var* gamma, const Var* beta, const Var* running_mean, const Var* running_var, double momentum, double eps,
                            Shared<bool> status) const {
    return batch_norm_diff(var, grad, &history, gamma, nullptr, nullptr, beta, nullptr, nullptr, running_mean, running_var, momentum, eps,
                           std::move(status));
}
VarDiff VarDiff::dropout(double p, Shared<bool> status) const {
    Var v = var.dropout(p, status);
    // the forward node owns the noise buffer; share it with the backward node (var.rs:375-393)
    auto fwd = std::dynamic_pointer_cast<DropoutFwd>(v.history.to_vec().back().op);
    auto g = std::make_shared<Gradient>(device(), shape());
    auto bw = std::make_shared<DropoutBwd>();
    bw->dx = grad; bw->g = g; bw->noise = fwd->noise; bw->p = p; bw->status = status;
    return VarDiff::node(std::move(v), g, entry(bw, g), history);
}
std::vector<VarDiff> VarDiff::chunks(const Shape& chunk_size) const {
    std::vector<Var> vs = var.chunks(chunk_size);
    std::vector<VarDiff> out;
    for (size_t i = 0; i < vs.size(); ++i) {
        auto g = std::make_shared<Gradient>(device(), chunk_size);
        auto bw = std::make_shared<ChunkBwd>();
        bw->dx = grad; bw->g = g; bw->chunk_no = (int)i;
        out.push_back(VarDiff::node(std::move(vs[i]), g, entry(bw, g), history));
    }
    return out;
}
VarDiff VarDiff::cat(const std::vector<VarDiff>& vars, int axis) const {
    std::vector<Var> vs;
    History<BackwardEntry> h = history;
    auto bw = std::make_shared<CatBwd>();
    bw->operands.push_back(grad);
    for (const VarDiff& v : vars) {
        vs.push_back(v.var);
        h.merge(v.history);
        bw->operands.push_back(v.grad);
    }
    Var out = var.cat(vs, axis);
    auto g = std::make_shared<Gradient>(device(), out.shape());
    bw->g = g; bw->axis = axis;
    return VarDiff::node(std::move(out), g, entry(bw, g), std::move(h));
}
VarDiff VarDiff::stack(const std::vector<VarDiff>& vars, int axis) const {
    std::vector<Var> vs;
    History<BackwardEntry> h = history;
    auto bw = std::make_shared<CatBwd>();
    bw->operands.push_back(grad);
    for (const VarDiff& v : vars) {
        vs.push_back(v.var);
        h.merge(v.history);
        bw->operands.push_back(v.grad);
    }
    Var out = var.stack(vs, axis);
    auto g = std::make_shared<Gradient>(device(), out.shape());
    bw->g = g; bw->axis = axis; bw->stack = true;
    return VarDiff::node(std::move(out), g, entry(bw, g), std::move(h));
}
VarDiff VarDiff::mse(const Var& target, Reduction reduction) const {
    Var out = var.mse(target, reduction);
    auto g = std::make_shared<Gradient>(device(), Shape{});
    auto bw = std::make_shared<MseBwd>();
    bw->x = var.data; bw->t = target.data; bw->dx = grad; bw->g = g; bw->red = reduction;
    return VarDiff::node(std::move(out), g, entry(bw, g), history);
}
VarDiff VarDiff::pad(const std::vector<int>& padding, float value) const { return pad(padding, PaddingMode::constant(value)); }
VarDiff VarDiff::pad(const std::vector<int>& padding, PaddingMode mode) const {
    Var out = var.pad(padding, mode);
    auto g = std::make_shared<Gradient>(device(), out.shape());
    auto bw = std::make_shared<PadBwd>();
    bw->dx = grad; bw->g = g; bw->padding = padding;
    return VarDiff::node(std::move(out), g, entry(bw, g), history);
}
VarDiff VarDiff::mm(const Var& rhs) const { return matmul_diff(0, var, grad, &history, rhs, nullptr, nullptr); }
VarDiff VarDiff::mm(const VarDiff& rhs) const { return matmul_diff(0, var, grad, &history, rhs.var, rhs.grad, &rhs.history); }
VarDiff VarDiff::mm_t(const Var& rhs) const { return matmul_diff(1, var, grad, &history, rhs, nullptr, nullptr); }
VarDiff VarDiff::mm_t(const VarDiff& rhs) const { return matmul_diff(1, var, grad, &history, rhs.var, rhs.grad, &rhs.history); }
VarDiff VarDiff::bmm(const VarDiff& rhs) const { return matmul_diff(2, var, grad, &history, rhs.var, rhs.grad, &rhs.history); }
VarDiff VarDiff::bmm_t(const VarDiff& rhs) const { return matmul_diff(3, var, grad, &history, rhs.var, rhs.grad, &rhs.history); }

VarDiff VarDiff::attention_probs(float scale, double p, Shared<bool> status, bool store_probs) const {
    Var v = var.attention_probs(scale, p, status, store_probs);
    auto fwd = std::dynamic_pointer_cast<AttnProbsFwd>(v.history.to_vec().back().op);
    auto g = std::make_shared<Gradient>(device(), shape());
    auto bw = std::make_shared<AttnProbsBwd>();
    bw->dx = grad; bw->g = g; bw->probs = fwd->probs; bw->scores = fwd->x; bw->scale = scale; bw->p = p; bw->status = status;
    bw->seed = fwd->seed; bw->last_offset = fwd->last_offset;
    return VarDiff::node(std::move(v), g, entry(bw, g), history);
}
static VarDiff conv_diff(const VarDiff& kernel, const Var& input, const Shared<Gradient>& dx,
                         const History<BackwardEntry>* hx, const std::vector<int>& stride,
                         const std::vector<int>& dilation, int groups, const VarDiff* bias = nullptr,
                         const std::vector<int>* crop = nullptr) {
    Var out = kernel.var.convolution(input, stride, dilation, groups);
    History<BackwardEntry> h = kernel.history;
    if (hx) h.merge(*hx);
    if (bias) {  // one node for `convolution(..) + bias`: the bias joins the forward node and both histories
        Shape want{out.shape()[1]};
        want.insert(want.end(), out.shape().size() - 2, 1);
        if (bias->shape() != want) panic("conv bias must have shape (out_channels, 1, ...)");
        auto fw = std::dynamic_pointer_cast<ConvFwd>(out.history.to_vec().back().op);
        fw->b = bias->var.data;
        out.history.merge(bias->var.history);
        h.merge(bias->history);
    }
    auto g = std::make_shared<Gradient>(out.device(), out.shape());
    auto bw = std::make_shared<ConvBwd>();
    bw->x = input.data; bw->w = kernel.var.data; bw->dx = dx; bw->dw = kernel.grad; bw->g = g;
    if (bias) bw->db = bias->grad;
    if (crop) bw->padding = *crop;  // `input` is the zero-padded copy of the Var whose gradient is dx
    bw->stride = stride; bw->dilation = dilation; bw->groups = groups;
    return VarDiff::node(std::move(out), g, entry(bw, g), std::move(h));
}
// The Conv module node WITHOUT its Pad node: forward and kernel gradient read the unpadded input through the library's folded
// entry points (nk_conv_bias_fwd_padded, nk_conv_bwd_kernel_bias_padded), the input gradient through nk_conv_bwd_input_padded as
// before.  Only built after nk_conv_padding_folds said yes for this geometry (ConvNd::forward).
static VarDiff conv_folded(const VarDiff& kernel, const Var& input, const Shared<Gradient>& dx, const History<BackwardEntry>* hx,
                           const std::vector<int>& padding, const std::vector<int>& stride, const std::vector<int>& dilation, int groups,
                           const VarDiff& bias) {
    Shape padded = input.shape();
    for (size_t i = 0; i < padding.size(); ++i) padded[2 + i] += 2 * padding[i];
    const Shape out = conv_out_shape(padded, kernel.shape(), stride, dilation, groups);
    Shape want{out[1]};
    want.insert(want.end(), out.size() - 2, 1);
    if (bias.shape() != want) panic("conv bias must have shape (out_channels, 1, ...)");
    History<ForwardEntry> fh = kernel.var.history;
    fh.merge(input.history);
    fh.merge(bias.var.history);
    auto fw = std::make_shared<ConvFwd>();
    fw->x = input.data; fw->w = kernel.var.data; fw->b = bias.var.data; fw->y = zeros_like(kernel.var.data, out);
    fw->stride = stride; fw->dilation = dilation; fw->groups = groups; fw->fold = padding;
    auto y = fw->y;
    Var outv = Var::node(y, fw, std::move(fh));
    History<BackwardEntry> h = kernel.history;
    if (hx) h.merge(*hx);
    h.merge(bias.history);
    auto g = std::make_shared<Gradient>(outv.device(), outv.shape());
    auto bw = std::make_shared<ConvBwd>();
    bw->x = input.data; bw->w = kernel.var.data; bw->dx = dx; bw->dw = kernel.grad; bw->db = bias.grad; bw->g = g;
    bw->padding = padding; bw->x_unpadded = true;
    bw->stride = stride; bw->dilation = dilation; bw->groups = groups;
    return VarDiff::node(std::move(outv), g, entry(bw, g), std::move(h));
}
static bool padding_folds(const Var& input, const VarDiff& weight, const std::vector<int>& padding, const std::vector<int>& stride,
                          const std::vector<int>& dilation, int groups) {
    int folds = 0;
    const int nd = (int)input.shape().size() - 2;
    check(nk_conv_padding_folds(input.device()->raw(), nd, input.shape().data(), padding.data(), weight.shape().data(), stride.data(),
                                dilation.data(), groups, &folds));
    return folds != 0;
}
VarDiff VarDiff::convolution(const Var& input, const std::vector<int>& stride, const std::vector<int>& dilation, int groups) const {
    return conv_diff(*this, input, nullptr, nullptr, stride, dilation, groups);
}
VarDiff VarDiff::convolution(const VarDiff& input, const std::vector<int>& stride, const std::vector<int>& dilation, int groups) const {
    return conv_diff(*this, input.var, input.grad, &input.history, stride, dilation, groups);
}
static VarDiff heads_diff(bool split, const VarDiff& x, int B, int S, int H, int dh) {
    Var out = split ? x.var.split_heads(B, S, H, dh) : x.var.merge_heads(B, S, H, dh);
    auto g = std::make_shared<Gradient>(out.device(), out.shape());
    auto bw = std::make_shared<HeadsBwd>();
    bw->split = split; bw->dx = x.grad; bw->g = g; bw->B = B; bw->S = S; bw->H = H; bw->dh = dh;
    return VarDiff::node(std::move(out), g, entry(bw, g), x.history);
}
VarDiff VarDiff::split_heads(int B, int S, int H, int dh) const { return heads_diff(true, *this, B, S, H, dh); }
VarDiff VarDiff::merge_heads(int B, int S, int H, int dh) const { return heads_diff(false, *this, B, S, H, dh); }

// ---- arithmetic operators -------------------------------------------------------------------------
static Var scalar_leaf(const DevicePtr& dev, float v) {  // the f32 is wrapped in an Ix0 leaf (var.rs:746-838)
    auto a = std::make_shared<HipArray>(dev, Shape{});
    a->fill(v);
    return Var::leaf(a);
}
#define NK_DEFINE_BINARY(OP, CODE)                                                                          \
    Var operator OP(const Var& l, const Var& r) { return binary_var(CODE, l, r); }                          \
    VarDiff operator OP(const Var& l, const VarDiff& r) { return binary_diff(CODE, l, nullptr, nullptr, r.var, r.grad, &r.history); } \
    VarDiff operator OP(const VarDiff& l, const Var& r) { return binary_diff(CODE, l.var, l.grad, &l.history, r, nullptr, nullptr); } \
    VarDiff operator OP(const VarDiff& l, const VarDiff& r) { return binary_diff(CODE, l.var, l.grad, &l.history, r.var, r.grad, &r.history); } \
    Var operator OP(const Var& l, float r) { return binary_var(CODE, l, scalar_leaf(l.device(), r)); }      \
    VarDiff operator OP(const VarDiff& l, float r) { return binary_diff(CODE, l.var, l.grad, &l.history, scalar_leaf(l.device(), r), nullptr, nullptr); }
NK_DEFINE_BINARY(+, NK_ADD)
NK_DEFINE_BINARY(-, NK_SUB)
NK_DEFINE_BINARY(*, NK_MUL)
NK_DEFINE_BINARY(/, NK_DIV)
#undef NK_DEFINE_BINARY

// ---- leaf constructors ----------------------------------------------------------------------------
Var from_host(DevicePtr dev, const Shape& shape, const float* host) { return Var::leaf(HipArray::from_host(std::move(dev), shape, host)); }
Var zeros(DevicePtr dev, const Shape& shape) { return Var::leaf(std::make_shared<HipArray>(std::move(dev), shape)); }
Var full(DevicePtr dev, const Shape& shape, float value) {
    auto a = std::make_shared<HipArray>(std::move(dev), shape);
    a->fill(value);
    return Var::leaf(a);
}
Var ones(DevicePtr dev, const Shape& shape) { return full(std::move(dev), shape, 1.f); }
static std::vector<float> uniform(size_t n, float lo, float hi, uint64_t seed) {
    std::mt19937_64 rng(seed);
    std::vector<float> v(n);
    for (float& x : v) x = lo + (hi - lo) * (float)((rng() >> 40) * (1.0 / 16777216.0));
    return v;
}
Var rand(DevicePtr dev, const Shape& shape, uint64_t seed) {
    const auto v = uniform(numel(shape), 0.f, 1.f, seed);
    return from_host(std::move(dev), shape, v.data());
}

// ndarray's `Linspace`: element i = start + step * i with step = (end - start) / (n - 1)
static std::vector<float> linspace_host(float start, float end, int n) {
    if (n < 0) panic("linspace: negative length");
    std::vector<float> v((size_t)n);
    const float step = n > 1 ? (end - start) / (float)(n - 1) : 0.f;
    for (int i = 0; i < n; ++i) v[(size_t)i] = start + step * (float)i;
    return v;
}
Var eye(DevicePtr dev, int n) {
    if (n < 0) panic("eye: negative size");
    std::vector<float> h((size_t)n * n, 0.f);
    for (int i = 0; i < n; ++i) h[(size_t)i * n + i] = 1.f;
    return from_host(std::move(dev), Shape{n, n}, h.data());
}
Var linspace(DevicePtr dev, float start, float end, int n) {
    const auto v = linspace_host(start, end, n);
    return from_host(std::move(dev), Shape{n}, v.data());
}
Var logspace(DevicePtr dev, float base, float start, float end, int n) {
    auto v = linspace_host(start, end, n);
    const float sign = base < 0.f ? -1.f : 1.f, b = std::fabs(base);
    for (float& e : v) e = sign * std::pow(b, e);
    return from_host(std::move(dev), Shape{n}, v.data());
}
Var geomspace(DevicePtr dev, float start, float end, int n) {
    if (start == 0.f || end == 0.f || (start < 0.f) != (end < 0.f))
        panic("geomspace: the reference returns None (an endpoint is zero or the endpoints differ in sign)");
    auto v = linspace_host(std::log(std::fabs(start)), std::log(std::fabs(end)), n);
    const float sign = start < 0.f ? -1.f : 1.f;
    for (float& e : v) e = sign * std::exp(e);
    return from_host(std::move(dev), Shape{n}, v.data());
}
Var range(DevicePtr dev, float start, float end, float step) {
    const float cnt = std::ceil((end - start) / step);
    const int n = (cnt > 0.f && std::isfinite(cnt)) ? (int)cnt : 0;  // `as usize` saturates negatives / NaN to 0
    std::vector<float> v((size_t)n);
    for (int i = 0; i < n; ++i) v[(size_t)i] = start + step * (float)i;
    return from_host(std::move(dev), Shape{n}, v.data());
}

// =================================================================================================
// nn
// =================================================================================================
namespace nn {

static VarDiff uniform_param(const DevicePtr& dev, const Shape& s, float k, uint64_t seed) {
    const auto v = uniform(numel(s), -k, k, seed);
    return from_host(dev, s, v.data()).requires_grad();
}
namespace init {
float calculate_gain(const std::string& nl) {
    if (nl == "linear" || nl == "sigmoid") return 1.f;
    if (nl == "tanh") return 5.f / 3.f;
    if (nl == "relu") return std::sqrt(2.f);
    if (nl == "leaky_relu") return std::sqrt(2.f / (1.f + 0.01f * 0.01f));
    panic("error: unsupported nonlinearity: " + nl);
}
std::pair<float, float> calculate_fan_in_fan_out(const VarDiff& param) {
    const Shape& s = param.shape();
    if (s.size() < 2) panic("index out of bounds: fan in / fan out need at least 2 dimensions");  // `shape[1]`
    size_t fan_in = (size_t)s[1], fan_out = (size_t)s[0];
    if (s.size() > 2) {
        size_t numel = 0;  // init.rs:55: `.skip(2).sum()` - the reference SUMS the trailing extents
        for (size_t i = 2; i < s.size(); ++i) numel += (size_t)s[i];
        fan_in *= numel; fan_out *= numel;
    }
    return {(float)fan_in, (float)fan_out};
}
void constant(const VarDiff& p, float v) { p.var.data->fill(v); }
void zeros(const VarDiff& p) { p.var.data->fill(0.f); }
void ones(const VarDiff& p) { p.var.data->fill(1.f); }
void eye(const VarDiff& p) {
    const Shape& s = p.shape();
    if (s.size() != 2) panic("eye: a 2-dimensional parameter is expected");
    std::vector<float> h(numel(s), 0.f);
    for (int i = 0; i < std::min(s[0], s[1]); ++i) h[(size_t)i * s[1] + i] = 1.f;
    p.var.data->upload(h.data());
}
void dirac(const VarDiff& p, int groups) {
    const Shape& s = p.shape();
    if (s.size() < 3 || s.size() > 5) panic("error: only 3, 4 and 5 dimensional parameters are supported.");
    if (groups < 1 || s[0] % groups != 0) panic("error: output channels must be divisible by groups.");
    std::vector<float> h = p.to_vec();  // only the selected elements are set (init.rs:152-169), the rest is kept
    const int opg = s[0] / groups, min_dim = std::min(opg, s[1]);
    std::vector<size_t> stride(s.size(), 1);
    for (int i = (int)s.size() - 2; i >= 0; --i) stride[i] = stride[i + 1] * (size_t)s[i + 1];
    for (int g = 0; g < groups; ++g)
        for (int d = 0; d < min_dim; ++d) {
            size_t off = (size_t)(g * opg + d) * stride[0] + (size_t)d * stride[1];
            for (size_t i = 2; i < s.size(); ++i) off += (size_t)(s[i] / 2) * stride[i];
            h[off] = 1.f;
        }
    p.var.data->upload(h.data());
}
void uniform(const VarDiff& p, float low, float high, uint64_t seed) {
    std::mt19937_64 rng(seed);
    std::uniform_real_distribution<float> d(low, high);
    std::vector<float> h(numel(p.shape()));
    for (float& v : h) v = d(rng);
    p.var.data->upload(h.data());
}
void normal(const VarDiff& p, float mean, float std, uint64_t seed) {
    if (!(std >= 0.f) || !std::isfinite(std)) panic("called `Result::unwrap()` on an `Err` value: BadVariance");  // Normal::new(..).unwrap()
    std::mt19937_64 rng(seed);
    std::normal_distribution<float> d(mean, std);
    std::vector<float> h(numel(p.shape()));
    for (float& v : h) v = std == 0.f ? mean : d(rng);
    p.var.data->upload(h.data());
}
void xavier_uniform(const VarDiff& p, float gain, uint64_t seed) {
    const auto f = calculate_fan_in_fan_out(p);
    const float sd = gain * std::sqrt(2.f / (f.first + f.second)), a = std::sqrt(3.f) * sd;
    uniform(p, -a, a, seed);
}
void xavier_normal(const VarDiff& p, float gain, uint64_t seed) {
    const auto f = calculate_fan_in_fan_out(p);
    normal(p, 0.f, gain * std::sqrt(2.f / (f.first + f.second)), seed);
}
}  // namespace init

Linear::Linear(DevicePtr dev, int in_features, int out_features, uint64_t seed)
    : weight(uniform_param(dev, {out_features, in_features}, 1.f / std::sqrt((float)in_features), seed)),
      bias(uniform_param(dev, {out_features}, 1.f / std::sqrt((float)in_features), seed + 1)) {}
LayerNorm::LayerNorm(DevicePtr dev, Shape normalized_shape, double eps, bool elementwise_affine)
    : normalized_shape(std::move(normalized_shape)), eps(eps), elementwise_affine(elementwise_affine) {
    if (this->normalized_shape.empty() || numel(this->normalized_shape) == 0) panic("LayerNorm: normalized_shape must not be empty");
    if (elementwise_affine) {
        weight = ones(dev, this->normalized_shape).requires_grad();
        bias = zeros(dev, this->normalized_shape).requires_grad();
    }
}
LayerNorm::LayerNorm(VarDiff w, VarDiff b, double eps) : weight(std::move(w)), bias(std::move(b)), normalized_shape(weight.shape()), eps(eps) {
    if (bias.shape() != normalized_shape) panic("LayerNorm: weight and bias must have the same shape");
}
VarDiff LayerNorm::forward(const Var& input) const {
    if (!elementwise_affine) panic("LayerNorm without affine parameters on a Var input has nothing to differentiate: use Var::layer_norm(normalized_shape, eps)");
    return input.layer_norm(weight, bias, eps);
}
VarDiff LayerNorm::forward(const VarDiff& input) const {
    return elementwise_affine ? input.layer_norm(weight, bias, eps) : input.layer_norm(normalized_shape, eps);
}
RMSNorm::RMSNorm(DevicePtr dev, Shape normalized_shape, double eps, bool elementwise_affine)
    : normalized_shape(std::move(normalized_shape)), eps(eps), elementwise_affine(elementwise_affine) {
    if (this->normalized_shape.empty() || numel(this->normalized_shape) == 0) panic("RMSNorm: normalized_shape must not be empty");
    if (elementwise_affine) weight = ones(dev, this->normalized_shape).requires_grad();
}
RMSNorm::RMSNorm(VarDiff w, double eps) : weight(std::move(w)), normalized_shape(weight.shape()), eps(eps) {}
VarDiff RMSNorm::forward(const Var& input) const {
    if (!elementwise_affine) panic("RMSNorm without a weight on a Var input has nothing to differentiate: use Var::rms_norm(normalized_shape, eps)");
    return input.rms_norm(weight, eps);
}
VarDiff RMSNorm::forward(const VarDiff& input) const {
    return elementwise_affine ? input.rms_norm(weight, eps) : input.rms_norm(normalized_shape, eps);
}
GroupNorm::GroupNorm(DevicePtr dev, int num_groups, int num_channels, double eps, bool affine)
    : num_groups(num_groups), num_channels(num_channels), eps(eps), affine(affine) {
    if (num_groups <= 0 || num_channels <= 0 || num_channels % num_groups != 0)
        panic("GroupNorm: num_channels must be a positive multiple of num_groups");
    if (affine) {
        weight = ones(dev, {num_channels}).requires_grad();
        bias = zeros(dev, {num_channels}).requires_grad();
    }
}
GroupNorm::GroupNorm(int num_groups, VarDiff w, VarDiff b, double eps)
    : weight(std::move(w)), bias(std::move(b)), num_groups(num_groups), num_channels(0), eps(eps) {
    if (weight.shape().size() != 1 || bias.shape() != weight.shape()) panic("GroupNorm: weight and bias must share one shape (C)");
    num_channels = weight.shape()[0];
    if (num_groups <= 0 || num_channels % num_groups != 0) panic("GroupNorm: num_channels must be a positive multiple of num_groups");
}
void GroupNorm::check_input(const Shape& s) const {
    if (s.size() < 2) panic("GroupNorm: expected an input of at least 2 dimensions, got " + std::to_string(s.size()));
    if (s[1] != num_channels) panic("GroupNorm: expected " + std::to_string(num_channels) + " channels, got " + std::to_string(s[1]));
}
VarDiff GroupNorm::forward(const Var& input) const {
    check_input(input.shape());
    if (!affine) panic("GroupNorm without affine parameters on a Var input has nothing to differentiate: use Var::group_norm(num_groups, eps)");
    return input.group_norm(num_groups, weight, bias, eps);
}
VarDiff GroupNorm::forward(const VarDiff& input) const {
    check_input(input.shape());
    return affine ? input.group_norm(num_groups, weight, bias, eps) : input.group_norm(num_groups, eps);
}
InstanceNormNd::InstanceNormNd(int nd, DevicePtr dev, int num_features, double eps, bool affine)
    : num_features(num_features), eps(eps), affine(affine), nd(nd) {
    if (num_features <= 0) panic("InstanceNorm: num_features must be positive");
    if (affine) {
        weight = ones(dev, {num_features}).requires_grad();
        bias = zeros(dev, {num_features}).requires_grad();
    }
}
void InstanceNormNd::check_input(const Shape& s) const {
    const std::string name = "InstanceNorm" + std::to_string(nd) + "d";
    if (s.size() != (size_t)nd + 2) panic(name + ": expected " + std::to_string(nd + 2) + "-dimensional input, got " + std::to_string(s.size()) + " dimensions");
    if (s[1] != num_features) panic(name + ": expected " + std::to_string(num_features) + " channels, got " + std::to_string(s[1]));
}
VarDiff InstanceNormNd::forward(const Var& input) const {
    check_input(input.shape());
    if (!affine) panic("InstanceNorm without affine parameters on a Var input has nothing to differentiate: use Var::group_norm(C, eps)");
    return input.group_norm(num_features, weight, bias, eps);
}
VarDiff InstanceNormNd::forward(const VarDiff& input) const {
    check_input(input.shape());
    return affine ? input.group_norm(num_features, weight, bias, eps) : input.group_norm(num_features, eps);
}
Var GELU::forward(const Var& input) const { return input.gelu(approximate_tanh); }
VarDiff GELU::forward(const VarDiff& input) const { return input.gelu(approximate_tanh); }
Var SiLU::forward(const Var& input) const { return input.silu(); }
VarDiff SiLU::forward(const VarDiff& input) const { return input.silu(); }
Var GLU::forward(const Var& input) const { return input.glu(gate); }
VarDiff GLU::forward(const VarDiff& input) const { return input.glu(gate); }
CrossEntropyLoss::CrossEntropyLoss(Reduction reduction, long ignore_index, double label_smoothing)
    : reduction(reduction), ignore_index(ignore_index < 0 ? -1 : ignore_index), label_smoothing(label_smoothing) {
    if (!(label_smoothing >= 0.0 && label_smoothing < 1.0)) panic("CrossEntropyLoss: label_smoothing must be in [0, 1), got " + std::to_string(label_smoothing));
}
Var CrossEntropyLoss::forward(const Var& logits, const Var& target) const { return logits.cross_entropy(target, reduction, ignore_index, label_smoothing); }
VarDiff CrossEntropyLoss::forward(const VarDiff& logits, const Var& target) const {
    return logits.cross_entropy(target, reduction, ignore_index, label_smoothing);
}
static void embedding_check(const Shape& ws, long padding_idx) {
    if (ws.size() != 2 || ws[0] < 1 || ws[1] < 1) panic("Embedding: the table must be (num_embeddings, embedding_dim), both at least 1");
    if (ws[0] > (1 << 24)) panic("Embedding: at most 2^24 rows (ids are stored as f32), got " + std::to_string(ws[0]));
    if (padding_idx >= ws[0]) panic("Embedding: padding_idx " + std::to_string(padding_idx) + " is not a row of a table of " + std::to_string(ws[0]));
}
Embedding::Embedding(DevicePtr dev, size_t num_embeddings, size_t embedding_dim, long padding_idx, uint64_t seed)
    : num_embeddings(num_embeddings), embedding_dim(embedding_dim), padding_idx(padding_idx < 0 ? -1 : padding_idx) {
    if (num_embeddings > ((size_t)1 << 24) || embedding_dim > ((size_t)1 << 24)) panic("Embedding: at most 2^24 rows (ids are stored as f32) of at most 2^24 values");
    const Shape ws{(int)num_embeddings, (int)embedding_dim};
    embedding_check(ws, padding_idx);
    std::mt19937_64 rng(seed);  // init::normal(weight, 0, 1, seed), with the padding row zeroed before the one upload
    std::normal_distribution<float> d(0.f, 1.f);
    std::vector<float> h(numel(ws));
    for (float& v : h) v = d(rng);
    if (padding_idx >= 0) std::fill(h.begin() + (size_t)padding_idx * embedding_dim, h.begin() + ((size_t)padding_idx + 1) * embedding_dim, 0.f);
    weight = from_host(dev, ws, h.data()).requires_grad();
}
Embedding::Embedding(VarDiff w, long padding_idx) : weight(std::move(w)), padding_idx(padding_idx < 0 ? -1 : padding_idx) {
    embedding_check(weight.shape(), padding_idx);
    num_embeddings = (size_t)weight.shape()[0];
    embedding_dim = (size_t)weight.shape()[1];
}
VarDiff Embedding::forward(const Var& indices) const { return weight.embedding(indices, padding_idx); }


BatchNormNd::BatchNormNd(int nd, DevicePtr dev, int num_features, double eps, double momentum, bool affine, bool track_running_stats)
    : num_features(num_features), eps(eps), momentum(momentum), affine(affine), track_running_stats(track_running_stats), nd(nd),
      status(std::make_shared<bool>(true)) {
    if (num_features <= 0) panic("BatchNorm: num_features must be positive");
    if (affine) {
        weight = ones(dev, {num_features}).requires_grad();
        bias = zeros(dev, {num_features}).requires_grad();
    }
    if (track_running_stats) {
        running_mean = zeros(dev, {num_features});
        running_var = ones(dev, {num_features});
    }
}
void BatchNormNd::check_input(const Shape& s) const {
    const std::string name = "BatchNorm" + std::to_string(nd) + "d";
    const bool rank_ok = nd == 1 ? (s.size() == 2 || s.size() == 3) : s.size() == (size_t)nd + 2;
    if (!rank_ok)
        panic(name + ": expected " + (nd == 1 ? std::string("a 2- or 3") : std::to_string(nd + 2)) + "-dimensional input, got " +
              std::to_string(s.size()) + " dimensions");
    if (s[1] != num_features) panic(name + ": expected " + std::to_string(num_features) + " channels, got " + std::to_string(s[1]));
}
VarDiff BatchNormNd::forward(const Var& input) const {
    check_input(input.shape());
    if (!affine) panic("BatchNorm without affine parameters on a Var input has nothing to differentiate: use Var::batch_norm");
    const Var* rm = track_running_stats ? &running_mean : nullptr;
    return input.batch_norm(weight, bias, rm, rm ? &running_var : nullptr, momentum, eps, status);
}
VarDiff BatchNormNd::forward(const VarDiff& input) const {
    check_input(input.shape());
    const Var* rm = track_running_stats ? &running_mean : nullptr;
    const Var* rv = track_running_stats ? &running_var : nullptr;
    return affine ? input.batch_norm(weight, bias, rm, rv, momentum, eps, status)
                  : input.batch_norm((const Var*)nullptr, (const Var*)nullptr, rm, rv, momentum, eps, status);
}

PoolNd::PoolNd(int nd, bool average, std::vector<int> kernel_size, std::vector<int> stride, std::vector<int> padding, bool count_include_pad)
    : kernel_size(std::move(kernel_size)), stride(std::move(stride)), padding(std::move(padding)), average(average),
      count_include_pad(count_include_pad), nd(nd) {
    const std::string name = std::string(average ? "AvgPool" : "MaxPool") + std::to_string(nd) + "d";
    if (this->stride.empty()) this->stride = this->kernel_size;
    if (this->padding.empty()) this->padding.assign(nd, 0);
    if ((int)this->kernel_size.size() != nd || (int)this->stride.size() != nd || (int)this->padding.size() != nd)
        panic(name + ": kernel_size, stride and padding take " + std::to_string(nd) + " entries each");
    for (int i = 0; i < nd; ++i) {
        if (this->kernel_size[i] < 1 || this->stride[i] < 1) panic(name + ": window and stride of axis " + std::to_string(i) + " must be >= 1");
        if (this->padding[i] < 0 || this->padding[i] > this->kernel_size[i] / 2)
            panic(name + ": padding of axis " + std::to_string(i) + " must be in [0, window / 2]");
    }
}
void PoolNd::check_input(const Shape& s) const {
    if (s.size() != (size_t)nd + 2)
        panic(std::string(average ? "AvgPool" : "MaxPool") + std::to_string(nd) + "d: expected " + std::to_string(nd + 2) + "-dimensional input, got " +
              std::to_string(s.size()) + " dimensions");
}
Var PoolNd::forward(const Var& input) const {
    check_input(input.shape());
    return average ? input.avg_pool(kernel_size, stride, padding, count_include_pad) : input.max_pool(kernel_size, stride, padding);
}
VarDiff PoolNd::forward(const VarDiff& input) const {
    check_input(input.shape());
    return average ? input.avg_pool(kernel_size, stride, padding, count_include_pad) : input.max_pool(kernel_size, stride, padding);
}

Upsample::Upsample(std::vector<int> size, std::vector<double> scale_factor, std::string mode, bool align_corners)
    : size(std::move(size)), scale_factor(std::move(scale_factor)), mode(std::move(mode)), align_corners(align_corners) {
    if (this->size.empty() == this->scale_factor.empty()) panic("Upsample: give either size or scale_factor, not both and not neither");
    if (this->mode != "nearest" && this->mode != "linear" && this->mode != "bilinear" && this->mode != "trilinear")
        panic("Upsample: unknown mode \"" + this->mode + "\" (nearest, linear, bilinear, trilinear)");
    if (this->mode == "nearest" && align_corners) panic("Upsample: align_corners has no meaning for the nearest mode");
    for (int s : this->size)
        if (s < 1) panic("Upsample: size entries must be >= 1");
    for (double s : this->scale_factor)
        if (!std::isfinite(s) || s <= 0.0) panic("Upsample: scale_factor entries must be finite and positive");
}
std::vector<int> Upsample::output_size(const Shape& s) const {
    if (s.size() < 3 || s.size() > 5) panic("Upsample: the input must be (N, C, spatial...) with 1 to 3 spatial axes, got " + std::to_string(s.size()) + " dimensions");
    const size_t nd = s.size() - 2;
    if (!size.empty()) {
        if (size.size() != nd) panic("Upsample: size has " + std::to_string(size.size()) + " entries for " + std::to_string(nd) + " spatial axes");
        return size;
    }
    if (scale_factor.size() != 1 && scale_factor.size() != nd)
        panic("Upsample: scale_factor has " + std::to_string(scale_factor.size()) + " entries for " + std::to_string(nd) + " spatial axes (one, or one per axis)");
    std::vector<double> sc(nd, scale_factor[0]);
    if (scale_factor.size() == nd) sc = scale_factor;
    std::vector<int> out(nd);
    if (nk_upsample_out_size((int)nd, s.data(), sc.data(), out.data()) != NK_OK) panic(std::string("Upsample: ") + nk_last_error());
    return out;
}
Var Upsample::forward(const Var& input) const { return input.upsample(output_size(input.shape()), mode, align_corners); }
VarDiff Upsample::forward(const VarDiff& input) const { return input.upsample(output_size(input.shape()), mode, align_corners); }

static VarDiff linear_node(const Linear& l, const Var& x, const Shared<Gradient>& dx, const History<BackwardEntry>* hx, bool relu = false) {
    const Shape& xs = x.shape();
    const Shape& ws = l.weight.shape();
    if (xs.size() != 2 || ws.size() != 2 || xs[1] != ws[1]) panic("Shapes are incompatible for matrix multiplication.");
    if (l.bias.shape() != Shape{ws[0]}) panic("Linear: bias must have shape (out_features)");
    History<ForwardEntry> h = x.history;
    h.merge(l.weight.var.history);
    h.merge(l.bias.var.history);
    auto fw = std::make_shared<LinearFwd>();
    fw->x = x.data; fw->w = l.weight.var.data; fw->b = l.bias.var.data; fw->y = zeros_like(x.data, Shape{xs[0], ws[0]});
    fw->relu = relu;
    auto y = fw->y;
    Var var = Var::node(y, fw, std::move(h));
    History<BackwardEntry> hb;
    if (hx) hb = *hx;
    hb.merge(l.weight.history);
    hb.merge(l.bias.history);
    auto g = std::make_shared<Gradient>(var.device(), var.shape());
    if (relu) g->set_premask_source(y);
    auto bw = std::make_shared<LinearBwd>();
    bw->x = x.data; bw->w = l.weight.var.data; bw->dx = dx; bw->dw = l.weight.grad; bw->db = l.bias.grad; bw->g = g;
    if (relu) bw->y = y;
    VarDiff out = VarDiff::node(std::move(var), g, entry(bw, g), std::move(hb));
    if (!relu) {
        auto origin = std::make_shared<LinearOrigin>();
        origin->weight = l.weight; origin->bias = l.bias; origin->input = x; origin->input_grad = dx;
        origin->differentiable_input = hx != nullptr;
        if (hx) origin->input_history = *hx;
        out.linear_origin = std::move(origin);
    }
    return out;
}
VarDiff linear_relu_from_origin(const LinearOrigin& o) {
    const Linear l(o.weight, o.bias);
    return linear_node(l, o.input, o.input_grad, o.differentiable_input ? &o.input_history : nullptr, true);
}
VarDiff Linear::forward(const Var& input) const {
    return fused ? linear_node(*this, input, nullptr, nullptr) : input.mm_t(weight) + bias;
}
VarDiff Linear::forward(const VarDiff& input) const {
    return fused ? linear_node(*this, input.var, input.grad, &input.history) : input.mm_t(weight) + bias;
}
VarDiff Linear::forward_relu(const Var& input) const {
    return fused ? linear_node(*this, input, nullptr, nullptr, true) : (input.mm_t(weight) + bias).relu();
}
VarDiff Linear::forward_relu(const VarDiff& input) const {
    return fused ? linear_node(*this, input.var, input.grad, &input.history, true) : (input.mm_t(weight) + bias).relu();
}

LSTMCell::LSTMCell(DevicePtr dev, int input_size, int hidden_size, uint64_t seed)
    : weight_ih(uniform_param(dev, {4 * hidden_size, input_size}, 1.f / std::sqrt((float)hidden_size), seed)),
      weight_hh(uniform_param(dev, {4 * hidden_size, hidden_size}, 1.f / std::sqrt((float)hidden_size), seed + 1)),
      bias_ih(uniform_param(dev, {4 * hidden_size}, 1.f / std::sqrt((float)hidden_size), seed + 2)),
      bias_hh(uniform_param(dev, {4 * hidden_size}, 1.f / std::sqrt((float)hidden_size), seed + 3)) {}
template <class I>
static std::pair<VarDiff, VarDiff> lstm_step(const LSTMCell& c, const std::pair<VarDiff, VarDiff>& state, const I& input) {
    const VarDiff& cell_state = state.first;
    const VarDiff& hidden = state.second;
    VarDiff gates = hidden.mm_t(c.weight_hh) + c.bias_hh + input.mm_t(c.weight_ih) + c.bias_ih;
    const Shape gs = gates.shape();
    auto ch = gates.chunks({gs[0], gs[1] / 4});
    VarDiff input_gate = ch[0].sigmoid(), forget_gate = ch[1].tanh(), cell_state_gate = ch[2].sigmoid(),
            output_gate = ch[3].sigmoid();
    VarDiff new_cell_state = forget_gate * cell_state + (input_gate * cell_state_gate);
    VarDiff new_hidden = output_gate * new_cell_state.tanh();
    return {new_cell_state, new_hidden};
}
std::pair<VarDiff, VarDiff> LSTMCell::forward(const std::pair<VarDiff, VarDiff>& st, const Var& in) const { return lstm_step(*this, st, in); }
std::pair<VarDiff, VarDiff> LSTMCell::forward(const std::pair<VarDiff, VarDiff>& st, const VarDiff& in) const { return lstm_step(*this, st, in); }

GRUCell::GRUCell(DevicePtr dev, int input_size, int hidden_size, uint64_t seed)
    : weight_ih(uniform_param(dev, {3 * hidden_size, input_size}, 1.f / std::sqrt((float)hidden_size), seed)),
      weight_hh(uniform_param(dev, {3 * hidden_size, hidden_size}, 1.f / std::sqrt((float)hidden_size), seed + 1)),
      bias_ih(uniform_param(dev, {3 * hidden_size}, 1.f / std::sqrt((float)hidden_size), seed + 2)),
      bias_hh(uniform_param(dev, {3 * hidden_size}, 1.f / std::sqrt((float)hidden_size), seed + 3)) {}
template <class I>
static VarDiff gru_step(const GRUCell& c, const VarDiff& hidden, const I& input) {
    VarDiff igates = input.mm_t(c.weight_ih) + c.bias_ih;
    VarDiff hgates = hidden.mm_t(c.weight_hh) + c.bias_hh;
    const Shape gs = hgates.shape();
    auto ci = igates.chunks({gs[0], gs[1] / 3}), chh = hgates.chunks({gs[0], gs[1] / 3});
    VarDiff reset_gate = (chh[0] + ci[0]).sigmoid();
    VarDiff input_gate = (chh[1] + ci[1]).sigmoid();
    VarDiff new_gate = (ci[2] + (chh[2] * reset_gate)).tanh();
    return (hidden - new_gate) * input_gate + new_gate;
}
VarDiff GRUCell::forward(const VarDiff& h, const Var& in) const { return gru_step(*this, h, in); }
VarDiff GRUCell::forward(const VarDiff& h, const VarDiff& in) const { return gru_step(*this, h, in); }

static Shape conv_weight_shape(int out_channels, int in_per_group, const std::vector<int>& kernel) {
    Shape w{out_channels, in_per_group};
    w.insert(w.end(), kernel.begin(), kernel.end());
    return w;
}
static Shape conv_bias_shape(int out_channels, int nd) {
    Shape b{out_channels};
    b.insert(b.end(), nd, 1);
    return b;
}
static float conv_init_bound(int in_per_group, const std::vector<int>& kernel) {
    int fan = in_per_group;
    for (int k : kernel) fan *= k;
    return std::sqrt(1.f / (float)fan);
}
ConvNd::ConvNd(int nd, DevicePtr dev, int in_channels, int out_channels, std::vector<int> kernel, std::vector<int> padding_,
               PaddingMode mode, std::vector<int> stride_, std::vector<int> dilation_, int groups_, uint64_t seed)
    : weight(uniform_param(dev, conv_weight_shape(out_channels, in_channels / groups_, kernel),
                           conv_init_bound(in_channels / groups_, kernel), seed)),
      bias(uniform_param(dev, conv_bias_shape(out_channels, nd), conv_init_bound(in_channels / groups_, kernel), seed + 1)),
      padding(std::move(padding_)), stride(std::move(stride_)), dilation(std::move(dilation_)), padding_mode(mode),
      groups(groups_) {
    if ((int)kernel.size() != nd || (int)padding.size() != nd || (int)stride.size() != nd || (int)dilation.size() != nd)
        panic("Conv" + std::to_string(nd) + "d: kernel/padding/stride/dilation need " + std::to_string(nd) + " entries");
}
VarDiff ConvNd::forward(const Var& input) const {
    const bool zero_pad = padding_mode.kind == PaddingMode::Zero || (padding_mode.kind == PaddingMode::Constant && padding_mode.value == 0.f);
    if (fused && fold_padding && zero_pad && padding_folds(input, weight, padding, stride, dilation, groups))
        return conv_folded(weight, input, nullptr, nullptr, padding, stride, dilation, groups, bias);
    const Var padded = input.pad(padding, padding_mode);
    if (!fused) return weight.convolution(padded, stride, dilation, groups) + bias;
    return conv_diff(weight, padded, nullptr, nullptr, stride, dilation, groups, &bias);
}
VarDiff ConvNd::forward(const VarDiff& input) const {
    bool any_pad = false;
    for (int p : padding) any_pad = any_pad || p != 0;
    if (fused && any_pad && (padding_mode.kind == PaddingMode::Zero || (padding_mode.kind == PaddingMode::Constant && padding_mode.value == 0.f))) {
        // pad -> convolution -> + bias with the Pad node's backward folded into the convolution's: the padded copy is a
        // forward-only node, the convolution's input gradient lands in input.grad directly (no padded gradient buffer) - or, where
        // the library's kernels read the unpadded input, no Pad node at all
        if (fold_padding && padding_folds(input.var, weight, padding, stride, dilation, groups))
            return conv_folded(weight, input.var, input.grad, &input.history, padding, stride, dilation, groups, bias);
        const Var padded = input.var.pad(padding, padding_mode);
        return conv_diff(weight, padded, input.grad, &input.history, stride, dilation, groups, &bias, &padding);
    }
    const VarDiff padded = input.pad(padding, padding_mode);
    if (!fused) return weight.convolution(padded, stride, dilation, groups) + bias;
    return conv_diff(weight, padded.var, padded.grad, &padded.history, stride, dilation, groups, &bias);
}

// a Linear whose weight / bias (and their gradients) are rows [row0, row0 + out) of the packed storage, initialised as
// `Linear(dev, d, out, seed)` would be
static Linear packed_linear(const Shared<HipArray>& w_all, const Shared<HipArray>& b_all, const Shared<HipArray>& gw_all,
                            const Shared<HipArray>& gb_all, int row0, int out, int d, uint64_t seed) {
    const float k = 1.f / std::sqrt((float)d);
    auto w = std::make_shared<HipArray>(w_all, (size_t)row0 * d, Shape{out, d});
    auto b = std::make_shared<HipArray>(b_all, (size_t)row0, Shape{out});
    w->upload(uniform((size_t)out * d, -k, k, seed).data());
    b->upload(uniform((size_t)out, -k, k, seed + 1).data());
    return Linear(VarDiff::leaf(Var::leaf(w), std::make_shared<Gradient>(gw_all, (size_t)row0 * d, Shape{out, d})),
                  VarDiff::leaf(Var::leaf(b), std::make_shared<Gradient>(gb_all, (size_t)row0, Shape{out})));
}
static Linear placeholder_linear(const DevicePtr& dev) { return Linear(zeros(dev, {1, 1}).requires_grad(), zeros(dev, {1}).requires_grad()); }
static void check_kv_heads(int d_model, int heads, int kv_heads) {
    if (heads <= 0 || d_model % heads != 0) panic("d_model must be divisible by heads");
    if (kv_heads <= 0 || kv_heads > heads || heads % kv_heads != 0)
        panic("MultiheadAttention: kv_heads must be positive and divide heads, got heads = " + std::to_string(heads) + ", kv_heads = " +
              std::to_string(kv_heads));
}
MultiheadAttention::MultiheadAttention(DevicePtr dev, int d_model_, int heads_, double p, uint64_t seed)
    : MultiheadAttention(std::move(dev), d_model_, heads_, heads_, p, seed) {}
MultiheadAttention::MultiheadAttention(DevicePtr dev, int d_model_, int heads_, int kv_heads_, double p, uint64_t seed)
    : q(placeholder_linear(dev)), k(placeholder_linear(dev)), v(placeholder_linear(dev)), o(dev, d_model_, d_model_, seed + 6),
      d_model(d_model_), heads(heads_), kv_heads(kv_heads_), drop(p) {
    check_kv_heads(d_model, heads, kv_heads);
    const int dkv = d_model / heads * kv_heads, rows = d_model + 2 * dkv;
    if (d_model % 4 != 0 || dkv % 4 != 0) {
        // the bias views of a packed allocation start d and d + dkv floats in: not 16-byte aligned unless both are multiples of 4,
        // and kernels that take whole float4s (nk_fill with a value, the pointwise kernels) refuse such a buffer.  Three ordinary layers.
        q = Linear(dev, d_model, d_model, seed); k = Linear(dev, d_model, dkv, seed + 2); v = Linear(dev, d_model, dkv, seed + 4);
        packed_qkv = false;
        return;
    }
    wqkv_ = std::make_shared<HipArray>(dev, Shape{rows, d_model});
    bqkv_ = std::make_shared<HipArray>(dev, Shape{rows});
    gwqkv_ = std::make_shared<HipArray>(dev, Shape{rows, d_model}, HipArray::Uninit{});
    gbqkv_ = std::make_shared<HipArray>(dev, Shape{rows}, HipArray::Uninit{});
    q = packed_linear(wqkv_, bqkv_, gwqkv_, gbqkv_, 0, d_model, d_model, seed);
    k = packed_linear(wqkv_, bqkv_, gwqkv_, gbqkv_, d_model, dkv, d_model, seed + 2);
    v = packed_linear(wqkv_, bqkv_, gwqkv_, gbqkv_, d_model + dkv, dkv, d_model, seed + 4);
}
MultiheadAttention::MultiheadAttention(Linear q_, Linear k_, Linear v_, Linear o_, int heads_, double p, int kv_heads_)
    : q(std::move(q_)), k(std::move(k_)), v(std::move(v_)), o(std::move(o_)), d_model(q.weight.shape()[1]), heads(heads_),
      kv_heads(kv_heads_ == 0 ? heads_ : kv_heads_), drop(p) {
    check_kv_heads(d_model, heads, kv_heads);
    if (kv_heads != heads) {
        const Shape want{d_model / heads * kv_heads, d_model};
        if (k.weight.shape() != want || v.weight.shape() != want)
            panic("MultiheadAttention: with " + std::to_string(kv_heads) + " kv heads of " + std::to_string(d_model / heads) +
                  " the k and v projections must be (" + std::to_string(want[0]) + ", " + std::to_string(d_model) + ")");
    }
    packed_qkv = false;
}
static VarDiff qkv_attention_node(const MultiheadAttention& m, const Shared<HipArray>& w, const Shared<HipArray>& b, const Shared<HipArray>& gw,
                                  const Shared<HipArray>& gb, const VarDiff& x, int B, int S, int H, int dh, float scale, const Segments* seg) {
    const int d = H * dh;
    History<ForwardEntry> hf = x.var.history;
    for (const Linear* l : {&m.q, &m.k, &m.v}) { hf.merge(l->weight.var.history); hf.merge(l->bias.var.history); }
    auto fw = std::make_shared<QkvAttentionFwd>();
    fw->x = x.var.data; fw->w = w; fw->b = b;
    fw->qkv = zeros_like(x.var.data, Shape{B * S, 3 * d});
    // (forward() checked window >= 0 and causal; seg: packed sequences with max_len < S)
    fw->core = AttnCore::build(x.var.data, B, S, H, dh, scale, m.drop.p, m.drop.status, m.causal, m.window, seg, true);
    fw->o = zeros_like(x.var.data, Shape{B * S, d});
    if (m.rope) {
        fw->rope = m.rope->table;
        fw->rg = seg ? rope_geom(*m.rope, B * S, 1, 2 * H) : rope_geom(*m.rope, B, S, 2 * H);  // packed sequences: every row at its own position
        if (seg) fw->rope_start = seg->pos;
    }
    Var out = Var::node(fw->o, fw, std::move(hf));
    History<BackwardEntry> hb = x.history;
    for (const Linear* l : {&m.q, &m.k, &m.v}) { hb.merge(l->weight.history); hb.merge(l->bias.history); }
    auto g = std::make_shared<Gradient>(out.device(), out.shape());
    auto bw = std::make_shared<QkvAttentionBwd>();
    bw->core = fw->core;
    bw->x = fw->x; bw->w = w; bw->qkv = fw->qkv; bw->o = fw->o;
    bw->dqkv = zeros_like(fw->qkv, fw->qkv->shape());
    bw->core.add_backward_scratch();
    bw->gw_all = gw; bw->gb_all = gb;
    bw->dx = x.grad;
    const Linear* ls[3] = {&m.q, &m.k, &m.v};
    for (int i = 0; i < 3; ++i) { bw->gw[i] = ls[i]->weight.grad; bw->gb[i] = ls[i]->bias.grad; }
    bw->g = g;
    bw->rope = fw->rope; bw->rg = fw->rg; bw->rope_start = fw->rope_start;
    return VarDiff::node(std::move(out), g, entry(bw, g), std::move(hb));
}
// q / k / v are public members: the packed path is only valid while they still ARE the views of the packed storage
// (after `mha.q = Linear(...)` or a swap with deserialised layers the three-node path runs on the new layers)
bool MultiheadAttention::still_packed() const {
    if (!wqkv_) return false;
    const Linear* ls[3] = {&q, &k, &v};
    const int dkv = d_model / heads * kv_heads;
    const int row0[3] = {0, d_model, d_model + dkv}, out[3] = {d_model, dkv, dkv};
    for (int i = 0; i < 3; ++i) {
        const size_t wo = (size_t)row0[i] * d_model;
        if (ls[i]->weight.var.data->ptr() != wqkv_->ptr() + wo || ls[i]->bias.var.data->ptr() != bqkv_->ptr() + (size_t)row0[i]) return false;
        if (ls[i]->weight.shape() != Shape{out[i], d_model} || ls[i]->bias.shape() != Shape{out[i]}) return false;
        if (!ls[i]->weight.grad->is_view_of(gwqkv_, wo) || !ls[i]->bias.grad->is_view_of(gbqkv_, (size_t)row0[i])) return false;
    }
    return true;
}
VarDiff MultiheadAttention::forward(const VarDiff& x, int batch) const { return forward_impl(x, batch, nullptr); }
VarDiff MultiheadAttention::forward(const VarDiff& x, int batch, const Segments& segments) const { return forward_impl(x, batch, &segments); }
VarDiff MultiheadAttention::forward_impl(const VarDiff& x, int batch, const Segments* seg) const {
    const int rows = x.shape()[0], S = rows / batch, dh = d_model / heads;
    if (rows % batch != 0 || x.shape()[1] != d_model) panic("MultiheadAttention: bad input shape");
    const FormRefusals refuse{"MultiheadAttention", causal};
    refuse.segments(seg, batch, S, x.var.device().get());
    if (seg) {
        if (rope && seg->max_len > rope->max_pos)
            panic("MultiheadAttention: a document of " + std::to_string(seg->max_len) + " positions exceeds rope's table of " + std::to_string(rope->max_pos));
        if (seg->max_len >= S) seg = nullptr;  // one document per sample: lo = 0 and pos = t - the call without segments, node for node
    }
    const float scale = 1.f / std::sqrt((float)dh);
    refuse.window(window);
    const bool banded = band_of(window, S) != 0;  // what the mask leaves below draw
    if (rope) {
        if (rope->head_dim != dh)
            panic("MultiheadAttention: rope was built for heads of " + std::to_string(rope->head_dim) + ", the module has heads of " + std::to_string(dh));
        if (!seg && S > rope->max_pos) panic("MultiheadAttention: " + std::to_string(S) + " positions exceed rope's table of " + std::to_string(rope->max_pos));
    }
    // the projections of the unpacked paths: queries and keys rotated when `rope` is set
    auto rotated = [&](const Linear& l, int nh) {
        return !rope ? l.forward(x) : seg ? rope_rows(l.forward(x), *rope, nh, seg->pos) : l.forward(x).rope(*rope, batch, nh);
    };
    // Grouped-query attention: kv head k written G times in front of the branches below, which then run on `heads` heads as they
    // are (kv_heads == heads: no node is added)
    const int G = heads / kv_heads;
    auto keys = [&]() { return G == 1 ? rotated(k, heads) : rotated(k, kv_heads).repeat_kv(G, dh); };
    auto values = [&]() { return G == 1 ? v.forward(x) : v.forward(x).repeat_kv(G, dh); };
    // Causal, where the fused core does not apply: the composition spelled out - one Addition node (broadcast over B*H) of a
    // constant (S, S) leaf, 0 on and below the diagonal and -inf above, in front of the Softmax, whose -inf lanes come out exactly 0.
    // Uploaded once per graph build; the fused `attention_probs` node has no mask operand and is not used.
    // With a window shorter than S the constant is banded - also -inf at k <= r - window; every row keeps its diagonal.  The fused
    // core takes the window where it takes the head size (nk_attention_band_*: the key tiles left of the band are skipped too and the
    // scratch is banded); this composition stays for the other head sizes and for fused_core = false.
    auto causal_mask = [&](int n) {
        std::vector<float> m((size_t)n * n, 0.f);
        for (int r = 0; r < n; ++r) {
            for (int c = r + 1; c < n; ++c) m[(size_t)r * n + c] = -INFINITY;
            if (banded)
                for (int c = 0; c <= r - window; ++c) m[(size_t)r * n + c] = -INFINITY;
        }
        return from_host(x.var.device(), Shape{n, n}, m.data());
    };
    // Packed sequences on these paths: the per-sample constant, M_b[r][k] = 0 for max(lo[b][r], r - window + 1) <= k <= r and -inf
    // elsewhere, written out for every (sample, head) - a (batch*heads, S, S) leaf, acceptable where the fused core does not apply.
    auto segment_mask = [&](int n) {
        std::vector<float> m((size_t)batch * heads * n * n, -INFINITY);
        for (int bh = 0; bh < batch * heads; ++bh)
            for (int r = 0; r < n; ++r) {
                const int first = std::max(seg->lo_host[(size_t)(bh / heads) * n + r], banded ? r - window + 1 : 0);
                for (int c = first; c <= r; ++c) m[((size_t)bh * n + r) * n + c] = 0.f;
            }
        return from_host(x.var.device(), Shape{batch * heads, n, n}, m.data());
    };
    auto mask_leaf = [&](int n) { return seg ? segment_mask(n) : causal_mask(n); };
    if (G == 1 && packed_qkv && wqkv_ && strided_heads && fused && fused_core && q.fused && k.fused && v.fused && Var::attention_core_supported(S, dh, drop.p) &&
        still_packed())
        return o.forward(qkv_attention_node(*this, wqkv_, bqkv_, gwqkv_, gbqkv_, x, batch, S, heads, dh, scale, seg));
    if (strided_heads && dh % 4 == 0) {  // attention GEMMs address the heads inside the projection layout: no copies
        const VarDiff Qf = rotated(q, heads), Kf = keys(), Vf = values();
        if (fused && fused_core && Var::attention_core_supported(S, dh, drop.p))
            return o.forward(Qf.heads_attention(Kf, Vf, batch, S, heads, dh, scale, drop.p, drop.status, causal, window, seg));
        const VarDiff scores = Qf.heads_scores(Kf, batch, S, heads, dh);
        const VarDiff P = causal ? drop.forward((scores * scale + mask_leaf(S)).softmax(2))
                          : (fused && S % 4 == 0 && S <= 2048) ? scores.attention_probs(scale, drop.p, drop.status)
                                                               : drop.forward((scores * scale).softmax(2));
        return o.forward(P.heads_context(Vf, batch, S, heads, dh));
    }
    const VarDiff Q = rotated(q, heads).split_heads(batch, S, heads, dh);
    const VarDiff K = keys().split_heads(batch, S, heads, dh);
    const VarDiff V = values().split_heads(batch, S, heads, dh);
    const VarDiff P = causal ? drop.forward((Q.bmm_t(K) * scale + mask_leaf(S)).softmax(2))
                      : (fused && S % 4 == 0 && S <= 2048) ? Q.bmm_t(K).attention_probs(scale, drop.p, drop.status)
                                                           : drop.forward((Q.bmm_t(K) * scale).softmax(2));
    const VarDiff O = P.bmm(V).merge_heads(batch, S, heads, dh);
    return o.forward(O);
}


Sampler::Sampler(DevicePtr dev_, float temperature_, int top_k_, float top_p_, uint64_t seed_)
    : dev(std::move(dev_)), temperature(temperature_), top_k(top_k_), top_p(top_p_), seed(seed_), offset(std::make_shared<uint64_t>(0)) {
    if (!(temperature >= 0.f) || !std::isfinite(temperature)) panic("Sampler: temperature must be finite and not negative");
    if (!(top_p > 0.f)) panic("Sampler: top_p must be positive");
}
Var Sampler::forward(const Var& logits, int batch) const { return logits.sample(*this, batch); }
Var Sampler::forward(const VarDiff& logits, int batch) const { return logits.var.sample(*this, batch); }

// The image of a (N, K) weight, packed on the device (nk_quant_linear_pack)
static QuantImage quant_image(const char* who, const Shared<HipArray>& w, int N, int K, int bits, int group) {
    const size_t words = nk_quant_linear_words(N, K, bits), ns = nk_quant_linear_scales(N, K, group);
    if (words == 0 || ns == 0)
        panic(std::string(who) + ": bits must be 8 or 4, group 32, 64, 128 or 0, and the input extent (" + std::to_string(K) +
              ") a multiple of 32 and of the group; got bits = " + std::to_string(bits) + ", group = " + std::to_string(group));
    QuantImage img;
    img.bits = bits; img.group = group;
    img.qweight = std::make_shared<HipArray>(w->device(), Shape{(int)words}, HipArray::Uninit{});
    img.scales = std::make_shared<HipArray>(w->device(), Shape{N, (int)(ns / (size_t)N)}, HipArray::Uninit{});
    check(nk_quant_linear_pack(D(w), w->ptr(), K, img.qweight->ptr(), img.scales->ptr(), N, K, bits, group));
    return img;
}
QuantLinear::QuantLinear(const Linear& lin, int bits_, int group_) : bits(bits_), group(group_) {
    const Shape& ws = lin.weight.shape();
    if (ws.size() != 2 || lin.bias.shape() != Shape{ws[0]}) panic("QuantLinear: the Linear must hold an (out, in) weight and an (out) bias");
    out_features = ws[0]; in_features = ws[1];
    const QuantImage img = quant_image("QuantLinear", lin.weight.var.data, out_features, in_features, bits, group);
    qweight = img.qweight; scales = img.scales;
    bias = lin.bias.var.data;
}
Var QuantLinear::forward(const Var& x) const {
    const Shape& s = x.shape();
    if (s.size() != 2 || s[1] != in_features) panic("QuantLinear: the input must be (rows, " + std::to_string(in_features) + ")");
    if (x.device().get() != qweight->device().get()) panic("QuantLinear: the input lives on another device");
    auto n = std::make_shared<QuantLinearFwd>();
    n->x = x.data; n->bias = bias;
    n->img.qweight = qweight; n->img.scales = scales; n->img.bits = bits; n->img.group = group;
    n->rows = s[0]; n->in = in_features; n->out = out_features;
    n->y = zeros_like(x.data, Shape{s[0], out_features});
    auto y = n->y;
    return Var::node(y, n, x.history);
}
Var QuantLinear::forward(const VarDiff& x) const { return forward(x.var); }
Var QuantLinear::dequantize() const {
    auto w = std::make_shared<HipArray>(qweight->device(), Shape{out_features, in_features});
    check(nk_quant_linear_unpack(D(w), qweight->ptr(), scales->ptr(), w->ptr(), in_features, out_features, in_features, bits, group));
    return Var::leaf(w);
}
void MultiheadAttention::quantize(int bits, int group) {
    const int dkv = d_model / heads * kv_heads;
    const bool packed = packed_qkv && still_packed();
    QuantImage img[3];
    if (packed) img[0] = quant_image("MultiheadAttention::quantize", wqkv_, d_model + 2 * dkv, d_model, bits, group);
    else {
        const Linear* ls[3] = {&q, &k, &v};
        for (int i = 0; i < 3; ++i) {
            const int out = i == 0 ? d_model : dkv;
            if (ls[i]->weight.shape() != Shape{out, d_model})
                panic("MultiheadAttention::quantize: the projections must be (d_model, d_model) - k and v (kv_heads*head_dim, d_model)");
            img[i] = quant_image("MultiheadAttention::quantize", ls[i]->weight.var.data, out, d_model, bits, group);
        }
    }
    if (o.weight.shape() != Shape{d_model, d_model}) panic("MultiheadAttention::quantize: the output projection must be (d_model, d_model)");
    const QuantImage io = quant_image("MultiheadAttention::quantize", o.weight.var.data, d_model, d_model, bits, group);
    for (int i = 0; i < 3; ++i) qimg_[i] = img[i];   // nothing changes when a panic fired above
    qo_ = io;
    qpacked_ = packed;
}

Segments::Segments(DevicePtr dev, int batch_, int S_, const std::vector<std::vector<int>>& doc_lens) : batch(batch_), S(S_), max_len(0) {
    if (!dev) panic("Segments: null device");
    check(nk_graph_refuse_capture(dev->raw(), "nn::Segments (its arrays are uploaded with a synchronising copy)"));  // before anything touches the stream
    if (batch <= 0 || S <= 0) panic("Segments: batch and S must be positive");
    if ((long long)batch * S > (long long)INT_MAX) panic("Segments: batch * S must fit 31 bits");
    if ((int)doc_lens.size() != batch)
        panic("Segments: " + std::to_string(doc_lens.size()) + " lists of document lengths for a batch of " + std::to_string(batch));
    lo_host.assign((size_t)batch * S, 0);
    pos_host.assign((size_t)batch * S, 0);
    for (int b = 0; b < batch; ++b) {
        long long t = 0;
        auto document = [&](int n) {
            for (int i = 0; i < n; ++i) { lo_host[(size_t)b * S + t + i] = (int)t; pos_host[(size_t)b * S + t + i] = i; }
            t += n;
            max_len = std::max(max_len, n);
        };
        for (int n : doc_lens[(size_t)b]) {
            if (n <= 0) panic("Segments: sample " + std::to_string(b) + " has a document of length " + std::to_string(n) + " (must be positive)");
            if (t + n > S)
                panic("Segments: the documents of sample " + std::to_string(b) + " hold more than S = " + std::to_string(S) + " positions");
            document(n);
        }
        if (t < S) document((int)(S - t));  // the padding tail: one more document
    }
    static_assert(sizeof(int) == sizeof(float), "the int32 arrays travel in f32 storage");
    lo = std::make_shared<HipArray>(dev, Shape{batch, S}, HipArray::Uninit{});
    pos = std::make_shared<HipArray>(dev, Shape{batch, S}, HipArray::Uninit{});
    lo->upload(reinterpret_cast<const float*>(lo_host.data()));
    pos->upload(reinterpret_cast<const float*>(pos_host.data()));
}

RotaryEmbedding::RotaryEmbedding(DevicePtr dev, int head_dim_, int max_pos_, double base_, int rot_, bool interleaved_)
    : head_dim(head_dim_), max_pos(max_pos_), rot(rot_ == 0 ? head_dim_ : rot_), base(base_), interleaved(interleaved_) {
    if (head_dim <= 0 || max_pos <= 0) panic("RotaryEmbedding: head_dim and max_pos must be positive");
    if (rot < 2 || rot > head_dim || rot % 2 != 0)
        panic("RotaryEmbedding: rot must be even and in [2, head_dim = " + std::to_string(head_dim) + "], got " + std::to_string(rot));
    if (!(base > 0.0) || !std::isfinite(base)) panic("RotaryEmbedding: base must be positive and finite");
    if ((unsigned long long)max_pos * rot > (unsigned long long)INT_MAX) panic("RotaryEmbedding: max_pos * rot must fit 31 bits");
    table = std::make_shared<HipArray>(dev, Shape{max_pos, rot / 2, 2}, HipArray::Uninit{});
    check(nk_rope_table(dev->raw(), table->ptr(), max_pos, rot, base));
}

KvCache::KvCache(DevicePtr dev, int batch_, int heads_, int head_dim_, int capacity_) : KvCache(std::move(dev), batch_, heads_, head_dim_, capacity_, false) {}
KvCache::KvCache(DevicePtr dev, int batch_, int heads_, int head_dim_, int capacity_, bool rolling_)
    : batch(batch_), heads(heads_), head_dim(head_dim_), capacity(capacity_), rolling(rolling_) {
    if (batch <= 0 || heads <= 0 || head_dim <= 0 || capacity <= 0) panic("KvCache: batch, heads, head_dim and capacity must be positive");
    if ((unsigned long long)batch * heads * capacity * head_dim > (unsigned long long)INT_MAX)
        panic("KvCache: batch * heads * capacity * head_dim must fit 31 bits");
    const Shape s{batch, heads, capacity, head_dim};
    k = std::make_shared<HipArray>(dev, s, HipArray::Uninit{});
    v = std::make_shared<HipArray>(dev, s, HipArray::Uninit{});
    lens_.assign((size_t)batch, 0);
    high_.assign((size_t)batch, 0);
    (void)workspace(1, heads);
}
void KvCache::remember_window(int window) { window_ = window; }
Shared<HipArray> KvCache::workspace(int T, int query_heads, int window) {
    window = std::min(window, capacity);  // the kernel's own clamp on a linear cache; a ring has window <= capacity
    if (T > ws_T_ || query_heads > ws_H_ || window > ws_W_) {
        T = std::max(T, ws_T_);
        query_heads = std::max(query_heads, ws_H_);
        window = std::max(window, ws_W_);
        size_t n = nk_attention_decode_workspace(batch, T, query_heads, head_dim, capacity);
        if (window > 0) n = std::max(n, nk_attention_decode_window_workspace(batch, T, query_heads, head_dim, window));
        if (n == 0 || n > (size_t)INT_MAX) panic("KvCache: the decode workspace for " + std::to_string(T) + " rows per sample does not fit 31 bits");
        ws_ = std::make_shared<HipArray>(k->device(), Shape{(int)n}, HipArray::Uninit{});
        ws_T_ = T; ws_H_ = query_heads; ws_W_ = window;
    }
    return ws_;
}
void KvCache::advance(int T) {
    for (size_t b = 0; b < lens_.size(); ++b) {
        lens_[b] += T;
        high_[b] = std::max(high_[b], lens_[b]);
    }
}
void KvCache::reset() {
    lens_.assign((size_t)batch, 0);
    high_.assign((size_t)batch, 0);
}
void KvCache::truncate(const std::vector<int>& lens) {
    if ((int)lens.size() != batch) panic("KvCache::truncate: " + std::to_string(lens.size()) + " lengths for a batch of " + std::to_string(batch));
    for (int b = 0; b < batch; ++b)
        if (lens[b] < 0 || lens[b] > lens_[b])
            panic("KvCache::truncate: sample " + std::to_string(b) + " holds " + std::to_string(lens_[b]) + " positions, asked for " +
                  std::to_string(lens[b]));
    if (rolling) {  // the slots hold positions [high - capacity, high): the next query's window must start inside them
        const int W = window_ > 0 ? window_ : capacity;
        for (int b = 0; b < batch; ++b)
            if (std::max(0, lens[b] - W) < high_[b] - capacity)
                panic("KvCache::truncate: sample " + std::to_string(b) + " of a rolling cache of " + std::to_string(capacity) + " slots reached " +
                      std::to_string(high_[b]) + " positions; a window of " + std::to_string(W) + " at length " + std::to_string(lens[b]) +
                      " would read positions that were overwritten");
    }
    lens_ = lens;
}

struct StepImages { const QuantImage* qkv; const QuantImage* o; bool packed; };  // MultiheadAttention::quantize's images; o null: none
static std::shared_ptr<DecodeStepFwd> decode_step_node(const MultiheadAttention& m, const Var& x, int batch, int T, bool fresh, bool packed,
                                                       const Shared<HipArray>& wqkv, const Shared<HipArray>& bqkv, History<ForwardEntry>& hf,
                                                       const StepImages& qi);

// What both forward_step overloads refuse before they look at their cache's contents, in the order they fire: the layer's mode,
// the input's shape, the cache's own geometry and device (`cache_fits(dh)`, worded by each overload), rope's head size, the
// window.  Returns T.
template <class CacheFits>
static int step_preamble(const MultiheadAttention& m, const Var& x, int batch, const CacheFits& cache_fits) {
    if (!m.causal) panic("MultiheadAttention::forward_step is the incremental form of the CAUSAL forward: set causal = true");
    if (*m.drop.status && m.drop.p > 0.0) panic("MultiheadAttention::forward_step runs in inference: dropout is active (p > 0 in train mode), call drop.eval() first");
    if (x.shape().size() != 2 || batch <= 0 || x.shape()[0] % batch != 0 || x.shape()[0] == 0 || x.shape()[1] != m.d_model)
        panic("MultiheadAttention::forward_step: bad input shape");
    const int T = x.shape()[0] / batch, dh = m.d_model / m.heads;
    cache_fits(dh);
    if (m.rope && m.rope->head_dim != dh)
        panic("MultiheadAttention::forward_step: rope was built for heads of " + std::to_string(m.rope->head_dim) + ", the module has heads of " +
              std::to_string(dh));
    if (m.window < 0) panic("MultiheadAttention::forward_step: window must not be negative, got " + std::to_string(m.window));
    return T;
}

Var MultiheadAttention::forward_step(const Var& x, int batch, KvCache& cache) const {
    const int T = step_preamble(*this, x, batch, [&](int dh) {
        if (cache.batch != batch || cache.heads != kv_heads || cache.head_dim != dh)
            panic("MultiheadAttention::forward_step: the cache was built for batch " + std::to_string(cache.batch) + ", " + std::to_string(cache.heads) +
                  " heads of " + std::to_string(cache.head_dim) + ", the step has batch " + std::to_string(batch) + ", " + std::to_string(kv_heads) +
                  " kv heads (of " + std::to_string(heads) + " query heads) of " + std::to_string(dh));
        if (cache.k->device().get() != x.device().get()) panic("MultiheadAttention::forward_step: the cache lives on another device");
    });
    if (rope && !cache.rolling && cache.capacity > rope->max_pos)
        panic("MultiheadAttention::forward_step: the cache's capacity of " + std::to_string(cache.capacity) + " exceeds rope's table of " +
              std::to_string(rope->max_pos));
    if (cache.rolling && window == 0)
        panic("MultiheadAttention::forward_step: a rolling cache keeps the last positions only: it needs a layer with window > 0");
    if (cache.rolling && T > cache.capacity)
        panic("MultiheadAttention::forward_step: " + std::to_string(T) + " rows per sample exceed the rolling cache's " +
              std::to_string(cache.capacity) + " slots: chunk the prompt");
    bool fresh = true;
    for (int b = 0; b < batch; ++b) {
        if (cache.rolling) {  // the positions keep growing: they must stay inside rope's table (and 31 bits)
            if (rope && (long long)cache.lens()[b] + T > rope->max_pos)
                panic("MultiheadAttention::forward_step: sample " + std::to_string(b) + " holds " + std::to_string(cache.lens()[b]) + " positions, " +
                      std::to_string(T) + " more exceed rope's table of " + std::to_string(rope->max_pos));
            if ((long long)cache.lens()[b] + T > (long long)INT_MAX - 1024)
                panic("MultiheadAttention::forward_step: sample " + std::to_string(b) + ": positions must stay below 2^31 - 1024");
        } else if (cache.lens()[b] + T > cache.capacity)
            panic("MultiheadAttention::forward_step: sample " + std::to_string(b) + " holds " + std::to_string(cache.lens()[b]) + " positions, " +
                  std::to_string(T) + " more exceed the cache's capacity of " + std::to_string(cache.capacity));
        fresh = fresh && cache.lens()[b] == 0;
    }
    History<ForwardEntry> hf = x.history;
    auto fw = decode_step_node(*this, x, batch, T, fresh, packed_qkv && still_packed(), wqkv_, bqkv_, hf, StepImages{qimg_, qo_ ? &qo_ : nullptr, qpacked_});
    fw->cap = cache.capacity;
    fw->ring = cache.rolling;
    fw->kc = cache.k; fw->vc = cache.v;
    if (!fw->core && cache.rolling && (long long)window + T - 1 > cache.capacity)
        panic("MultiheadAttention::forward_step: a rolling cache of " + std::to_string(cache.capacity) + " slots cannot hold a window of " +
              std::to_string(window) + " keys and " + std::to_string(T) + " new rows (window + T - 1 <= capacity): chunk the prompt into slices of at most " +
              std::to_string(std::max(0, cache.capacity - window + 1)) + " rows");
    if (!fw->core) fw->ws = cache.workspace(T, heads, window);  // one partial per QUERY head
    if (window > 0) cache.remember_window(window);              // for truncate(): the core path asks for no scratch
    static_assert(sizeof(int) == sizeof(float), "the start positions travel in an f32 array");
    fw->start = std::make_shared<HipArray>(x.device(), Shape{batch}, HipArray::Uninit{});
    fw->start->upload(reinterpret_cast<const float*>(cache.lens().data()));
    cache.advance(T);
    auto y = fw->out;
    return Var::node(y, fw, std::move(hf));
}

// The part of the step's node both forward_step overloads build the same way: the projections, the temporaries, rope and the
// decision for the causal core.  The caller adds the cache, the scratch and the start positions.
static std::shared_ptr<DecodeStepFwd> decode_step_node(const MultiheadAttention& m, const Var& x, int batch, int T, bool fresh, bool packed,
                                                const Shared<HipArray>& wqkv, const Shared<HipArray>& bqkv, History<ForwardEntry>& hf,
                                                const StepImages& qi) {
    const int d_model = m.d_model, heads = m.heads, kv_heads = m.kv_heads, window = m.window, dh = d_model / heads;
    const Linear &q = m.q, &k = m.k, &v = m.v, &o = m.o;
    const Shared<RotaryEmbedding>& rope = m.rope;
    auto fw = std::make_shared<DecodeStepFwd>();
    fw->B = batch; fw->T = T; fw->H = heads; fw->Hkv = kv_heads; fw->dh = dh;
    fw->window = window;
    fw->x = x.data;
    for (const Linear* l : {&q, &k, &v, &o}) { hf.merge(l->weight.var.history); hf.merge(l->bias.var.history); }
    const int n = batch * T, dkv = kv_heads * dh;
    if (packed) {
        fw->w[0] = wqkv; fw->b[0] = bqkv;
        fw->qkv = zeros_like(x.data, Shape{n, d_model + 2 * dkv});
    } else {
        const Linear* ls[3] = {&q, &k, &v};
        for (int i = 0; i < 3; ++i) {
            const int out = i == 0 ? d_model : dkv;
            if (ls[i]->weight.shape() != Shape{out, d_model} || ls[i]->bias.shape() != Shape{out})
                panic("MultiheadAttention::forward_step: the projections must be (d_model, d_model) - k and v (kv_heads*head_dim, d_model) - with a bias of their rows");
            fw->w[i] = ls[i]->weight.var.data; fw->b[i] = ls[i]->bias.var.data;
        }
        fw->q = zeros_like(x.data, Shape{n, d_model}); fw->k = zeros_like(x.data, Shape{n, dkv}); fw->v = zeros_like(x.data, Shape{n, dkv});
    }
    if (o.weight.shape() != Shape{d_model, d_model} || o.bias.shape() != Shape{d_model})
        panic("MultiheadAttention::forward_step: the output projection must be (d_model, d_model) with a (d_model) bias");
    fw->wo = o.weight.var.data; fw->bo = o.bias.var.data;
    if (qi.o) {  // quantize() was called: the node projects through the images, which must be of the form this step takes
        if (qi.packed != packed)
            panic("MultiheadAttention::forward_step: quantize() built the images of the " + std::string(qi.packed ? "packed" : "three separate") +
                  " projections, this step takes the " + (packed ? "packed" : "three separate") + " ones: call quantize() again");
        for (int i = 0; i < (packed ? 1 : 3); ++i) fw->qw[i] = qi.qkv[i];
        fw->qwo = *qi.o;
    }
    fw->ctx = zeros_like(x.data, Shape{n, d_model});
    fw->out = zeros_like(x.data, Shape{n, d_model});
    if (rope) {
        fw->rope = rope->table;
        fw->rg = rope_geom(*rope, batch, T, fw->qkv ? heads + kv_heads : heads);  // packed: the Q and K heads are contiguous columns
        fw->rgk = rope_geom(*rope, batch, T, kv_heads);
    }
    fw->scale = 1.f / std::sqrt((float)dh);
    // the core's own size guards (nk_attention.hip: mask words and projection elements below 2^31): past them the decode kernels
    // take the prefill instead of a refused call
    const long long tiles = (T + 31) / 32;
    const bool core_fits = (long long)batch * heads * tiles * tiles < (1ll << 31) / 32 && (long long)n * 3 * d_model < (1ll << 31);
    // with a window the core, which has none, takes the prefill only while the band is the whole triangle
    fw->core = fresh && T >= 2 && core_fits && nk_attention_supported(T, dh, 0.0, 0) != 0 && (window == 0 || T <= window);
    if (fw->core && kv_heads != heads) {  // nothing is allocated inside forward()
        fw->kf = zeros_like(x.data, Shape{n, d_model}); fw->vf = zeros_like(x.data, Shape{n, d_model});
        if (fw->qkv) fw->qf = zeros_like(x.data, Shape{n, d_model});
    }
    return fw;
}

Var MultiheadAttention::forward_step(const Var& x, const std::vector<int>& seqs, PagedKvCache& cache) const {
    const int batch = (int)seqs.size();
    const int T = step_preamble(*this, x, batch, [&](int dh) {
        if (cache.heads != kv_heads || cache.head_dim != dh)
            panic("MultiheadAttention::forward_step: the paged cache was built for " + std::to_string(cache.heads) + " heads of " +
                  std::to_string(cache.head_dim) + ", the step has " + std::to_string(kv_heads) + " kv heads (of " + std::to_string(heads) +
                  " query heads) of " + std::to_string(dh));
        if (cache.k->device().get() != x.device().get()) panic("MultiheadAttention::forward_step: the cache lives on another device");
    });
    bool fresh = true;
    for (int b = 0; b < batch; ++b) {
        const int s = seqs[b];
        if (s < 0 || s >= cache.max_seqs)
            panic("MultiheadAttention::forward_step: sequence id " + std::to_string(s) + " is outside [0, " + std::to_string(cache.max_seqs) + ")");
        const int len = cache.lens()[s], behind = cache.behind(s);
        if (rope && (long long)len + T > rope->max_pos)
            panic("MultiheadAttention::forward_step: sequence " + std::to_string(s) + " holds " + std::to_string(len) + " positions, " +
                  std::to_string(T) + " more exceed rope's table of " + std::to_string(rope->max_pos));
        if (behind > 0 && window == 0)
            panic("MultiheadAttention::forward_step: sequence " + std::to_string(s) + " released the pages below position " +
                  std::to_string(behind) + ": it needs a layer with window > 0");
        // row 0 of the step reads from position len + 1 - window on
        if (behind > 0 && std::max(0, len + 1 - window) < behind)
            panic("MultiheadAttention::forward_step: sequence " + std::to_string(s) + " released the pages below position " +
                  std::to_string(behind) + ", a window of " + std::to_string(window) + " at length " + std::to_string(len) +
                  " would read below it");
        fresh = fresh && len == 0;
    }
    const std::vector<int> starts_before = cache.lens();
    // the node and the scratch first (their panics: projection shapes, a scratch past 31 bits), then reserve(), which panics before
    // it changes anything (out of pages, max_pages exceeded, duplicate ids); after it nothing panics
    History<ForwardEntry> hf = x.history;
    auto fw = decode_step_node(*this, x, batch, T, fresh, packed_qkv && still_packed(), wqkv_, bqkv_, hf, StepImages{qimg_, qo_ ? &qo_ : nullptr, qpacked_});
    if (!fw->core) fw->ws = cache.workspace(batch, T, heads, window);  // one partial per QUERY head
    const std::vector<std::pair<int, int>> copies = cache.reserve(seqs, T);
    fw->cap = 0;
    fw->kc = cache.k; fw->vc = cache.v;
    fw->page = cache.page; fw->max_pages = cache.max_pages; fw->num_pages = cache.num_pages; fw->ncopy = (int)copies.size();
    static_assert(sizeof(int) == sizeof(float), "the start positions travel in an f32 array");
    std::vector<int> img((size_t)batch * (1 + cache.max_pages) + 2 * copies.size());
    for (int b = 0; b < batch; ++b) {
        img[b] = starts_before[seqs[b]];
        std::copy_n(cache.table.rows().begin() + (size_t)seqs[b] * cache.max_pages, cache.max_pages, img.begin() + batch + (size_t)b * cache.max_pages);
    }
    for (size_t i = 0; i < copies.size(); ++i) {
        img[(size_t)batch * (1 + cache.max_pages) + i] = copies[i].first;
        img[(size_t)batch * (1 + cache.max_pages) + copies.size() + i] = copies[i].second;
    }
    fw->start = std::make_shared<HipArray>(x.device(), Shape{(int)img.size()}, HipArray::Uninit{});
    fw->start->upload(reinterpret_cast<const float*>(img.data()));
    auto y = fw->out;
    return Var::node(y, fw, std::move(hf));
}

PageTable::PageTable(int num_pages_, int page_, int max_seqs_, int max_pages_)
    : num_pages(num_pages_), page(page_), max_seqs(max_seqs_), max_pages(max_pages_) {
    if (num_pages <= 0 || max_seqs <= 0 || max_pages <= 0) panic("PageTable: num_pages, max_seqs and max_pages must be positive");
    if (page < 16 || (page & (page - 1)) != 0) panic("PageTable: page must be a power of two and at least 16, got " + std::to_string(page));
    if ((long long)max_pages * page > (long long)INT_MAX - 1024) panic("PageTable: max_pages * page must stay below 2^31 - 1024");
    if ((long long)max_seqs * max_pages > (long long)INT_MAX) panic("PageTable: max_seqs * max_pages must fit 31 bits");
    reset();
}
void PageTable::reset() {
    lens_.assign((size_t)max_seqs, 0);
    behind_.assign((size_t)max_seqs, 0);
    rows_.assign((size_t)max_seqs * max_pages, -1);
    ref_.assign((size_t)num_pages, 0);
    free_.clear();
    for (int p = 0; p < num_pages; ++p) free_.insert(free_.end(), p);
}
void PageTable::check_seq(int seq, const char* what) const {
    if (seq < 0 || seq >= max_seqs)
        panic(std::string("PageTable::") + what + ": sequence id " + std::to_string(seq) + " is outside [0, " + std::to_string(max_seqs) + ")");
}
void PageTable::unref(int p) {
    if (--ref_[(size_t)p] == 0) free_.insert(p);
}
std::vector<int> PageTable::row(int seq) const {
    check_seq(seq, "row");
    return std::vector<int>(rows_.begin() + (size_t)seq * max_pages, rows_.begin() + (size_t)(seq + 1) * max_pages);
}
std::vector<int> PageTable::pages(int seq) const {
    std::vector<int> out;
    for (int p : row(seq))
        if (p >= 0) out.push_back(p);
    return out;
}
int PageTable::refcount(int p) const {
    if (p < 0 || p >= num_pages) panic("PageTable::refcount: page id " + std::to_string(p) + " is outside [0, " + std::to_string(num_pages) + ")");
    return ref_[(size_t)p];
}
std::vector<int> PageTable::free_pages() const { return std::vector<int>(free_.begin(), free_.end()); }
int PageTable::behind(int seq) const {
    check_seq(seq, "behind");
    return behind_[(size_t)seq];
}
std::vector<std::pair<int, int>> PageTable::reserve(const std::vector<int>& seqs, int T) {
    if (T <= 0) panic("PageTable::reserve: T must be positive, got " + std::to_string(T));
    // a dry run first: ids, duplicates, max_pages, and the pages needed - a shared partial last page costs one more, unless an
    // earlier sequence of this call already left it to this one
    std::vector<char> seen((size_t)max_seqs, 0);
    std::unordered_map<int, int> left;  // shared page -> owners other sequences of this call have taken away
    size_t need = 0;
    for (int s : seqs) {
        check_seq(s, "reserve");
        if (seen[(size_t)s]) panic("PageTable::reserve: sequence " + std::to_string(s) + " is listed twice");
        seen[(size_t)s] = 1;
        const long long len = lens_[(size_t)s], have = (len + page - 1) / page, want = (len + T + page - 1) / page;
        if (want > max_pages)
            panic("PageTable::reserve: sequence " + std::to_string(s) + " holds " + std::to_string(len) + " positions, " + std::to_string(T) +
                  " more exceed max_pages = " + std::to_string(max_pages) + " pages of " + std::to_string(page));
        need += (size_t)(want - have);
        if (len % page != 0) {
            const int last = rows_[(size_t)s * max_pages + (size_t)(have - 1)];
            if (ref_[(size_t)last] - left[last] > 1) {
                ++left[last];
                ++need;
            }
        }
    }
    if (need > free_.size())
        panic("PageTable::reserve: " + std::to_string(need) + " pages needed, " + std::to_string(free_.size()) + " of " + std::to_string(num_pages) +
              " are free");
    std::vector<std::pair<int, int>> copies;
    auto take = [this]() {
        const int p = *free_.begin();
        free_.erase(free_.begin());
        ref_[(size_t)p] = 1;
        return p;
    };
    for (int s : seqs) {
        int* r = rows_.data() + (size_t)s * max_pages;
        const int len = lens_[(size_t)s], have = (len + page - 1) / page, want = (int)(((long long)len + T + page - 1) / page);
        if (len % page != 0 && ref_[(size_t)r[have - 1]] > 1) {
            const int old = r[have - 1];
            --ref_[(size_t)old];  // still owned by another
            r[have - 1] = take();
            copies.emplace_back(old, r[have - 1]);
        }
        for (int i = have; i < want; ++i) r[i] = take();
        lens_[(size_t)s] = len + T;
    }
    return copies;
}
void PageTable::truncate(int seq, int len) {
    check_seq(seq, "truncate");
    if (len < 0 || len > lens_[(size_t)seq] || len < behind_[(size_t)seq])
        panic("PageTable::truncate: sequence " + std::to_string(seq) + " holds positions [" + std::to_string(behind_[(size_t)seq]) + ", " +
              std::to_string(lens_[(size_t)seq]) + "), asked for " + std::to_string(len));
    int* r = rows_.data() + (size_t)seq * max_pages;
    const int have = (lens_[(size_t)seq] + page - 1) / page;
    for (int i = (len + page - 1) / page; i < have; ++i)
        if (r[i] >= 0) {
            unref(r[i]);
            r[i] = -1;
        }
    lens_[(size_t)seq] = len;
}
void PageTable::release(int seq) {
    check_seq(seq, "release");
    int* r = rows_.data() + (size_t)seq * max_pages;
    for (int i = 0; i < max_pages; ++i)
        if (r[i] >= 0) {
            unref(r[i]);
            r[i] = -1;
        }
    lens_[(size_t)seq] = 0;
    behind_[(size_t)seq] = 0;
}
void PageTable::fork(int src, int dst) {
    check_seq(src, "fork");
    check_seq(dst, "fork");
    if (src == dst) panic("PageTable::fork: source and destination are both sequence " + std::to_string(src));
    if (lens_[(size_t)dst] != 0 || behind_[(size_t)dst] != 0)
        panic("PageTable::fork: sequence " + std::to_string(dst) + " is not empty: release it first");
    const int* from = rows_.data() + (size_t)src * max_pages;
    int* to = rows_.data() + (size_t)dst * max_pages;
    for (int i = 0; i < max_pages; ++i) {
        to[i] = from[i];
        if (from[i] >= 0) ++ref_[(size_t)from[i]];
    }
    lens_[(size_t)dst] = lens_[(size_t)src];
    behind_[(size_t)dst] = behind_[(size_t)src];
}
void PageTable::release_behind(int seq, int pos) {
    check_seq(seq, "release_behind");
    if (pos < 0 || pos > lens_[(size_t)seq])
        panic("PageTable::release_behind: sequence " + std::to_string(seq) + " holds " + std::to_string(lens_[(size_t)seq]) +
              " positions, asked to release below " + std::to_string(pos));
    int* r = rows_.data() + (size_t)seq * max_pages;
    for (int i = 0; i < pos / page; ++i)
        if (r[i] >= 0) {
            unref(r[i]);
            r[i] = -1;
        }
    behind_[(size_t)seq] = std::max(behind_[(size_t)seq], pos / page * page);
}

PagedKvCache::PagedKvCache(DevicePtr dev, int num_pages_, int page_, int kv_heads_, int head_dim_, int max_seqs_, int max_pages_)
    : num_pages(num_pages_), page(page_), heads(kv_heads_), head_dim(head_dim_), max_seqs(max_seqs_), max_pages(max_pages_),
      table(num_pages_, page_, max_seqs_, max_pages_) {
    if (heads <= 0 || head_dim <= 0) panic("PagedKvCache: kv_heads and head_dim must be positive");
    // KvCache's limit, on one pool
    if ((unsigned long long)num_pages * heads * page * head_dim > (unsigned long long)INT_MAX)
        panic("PagedKvCache: num_pages * kv_heads * page * head_dim must fit 31 bits");
    const Shape s{num_pages, heads, page, head_dim};
    k = std::make_shared<HipArray>(dev, s, HipArray::Uninit{});
    v = std::make_shared<HipArray>(dev, s, HipArray::Uninit{});
}
void PagedKvCache::fork(int src, int dst) { table.fork(src, dst); }
Shared<HipArray> PagedKvCache::workspace(int batch, int T, int query_heads, int window) {
    const size_t n = nk_attention_decode_paged_workspace(batch, T, query_heads, head_dim, max_pages, page, window);
    if (n == 0 || n > (size_t)INT_MAX)
        panic("PagedKvCache: the decode workspace for " + std::to_string(batch) + " sequences of " + std::to_string(T) + " rows does not fit 31 bits");
    if (n > ws_n_) {  // a node keeps the one it was built with alive
        ws_ = std::make_shared<HipArray>(k->device(), Shape{(int)n}, HipArray::Uninit{});
        ws_n_ = n;
    }
    return ws_;
}

}  // namespace nn

// =================================================================================================
// serde (neuronika-variable/src/serde.rs:10-58): ndarray's {"v":1,"dim":[..],"data":[..]} wire format
// =================================================================================================
namespace serde {

namespace {
struct Parser {
    const std::string& s;
    size_t i = 0;
    explicit Parser(const std::string& s) : s(s) {}
    [[noreturn]] void fail(const char* what) const { panic(std::string("json: ") + what + " at offset " + std::to_string(i)); }
    void ws() { while (i < s.size() && (s[i] == ' ' || s[i] == '\n' || s[i] == '\t' || s[i] == '\r')) ++i; }
    bool eat(char c) { ws(); if (i < s.size() && s[i] == c) { ++i; return true; } return false; }
    void expect(char c) { if (!eat(c)) fail("unexpected character"); }
    std::string string() {
        expect('"');
        std::string out;
        while (i < s.size() && s[i] != '"') {
            if (s[i] == '\\') {
                if (++i >= s.size()) fail("bad escape");
                switch (s[i]) {
                    case 'n': out += '\n'; break;
                    case 't': out += '\t'; break;
                    case 'r': out += '\r'; break;
                    case 'b': out += '\b'; break;
                    case 'f': out += '\f'; break;
                    case 'u': fail("\\u escapes are not needed for this schema");
                    default: out += s[i];
                }
                ++i;
            } else {
                out += s[i++];
            }
        }
        if (i >= s.size()) fail("unterminated string");
        ++i;
        return out;
    }
    Json value() {
        ws();
        if (i >= s.size()) fail("unexpected end");
        Json j;
        const char c = s[i];
        if (c == '{') {
            ++i; j.kind = Json::Object;
            if (eat('}')) return j;
            do {
                ws();
                std::string k = string();
                expect(':');
                j.members.emplace_back(std::move(k), value());
            } while (eat(','));
            expect('}');
        } else if (c == '[') {
            ++i; j.kind = Json::Array;
            if (eat(']')) return j;
            do { j.items.push_back(value()); } while (eat(','));
            expect(']');
        } else if (c == '"') {
            j.kind = Json::String; j.text = string();
        } else if (s.compare(i, 4, "true") == 0) { j.kind = Json::Bool; j.b = true; i += 4;
        } else if (s.compare(i, 5, "false") == 0) { j.kind = Json::Bool; i += 5;
        } else if (s.compare(i, 4, "null") == 0) { i += 4;
        } else {
            const size_t b = i;
            while (i < s.size() && (std::isdigit((unsigned char)s[i]) || s[i] == '-' || s[i] == '+' || s[i] == '.' || s[i] == 'e' || s[i] == 'E')) ++i;
            if (b == i) fail("unexpected token");
            j.kind = Json::Number; j.text = s.substr(b, i - b);
        }
        return j;
    }
};

void write_f32(std::string& out, float v) {
    if (!std::isfinite(v)) { out += "null"; return; }  // serde_json writes non-finite floats as null
    char buf[32];
    auto r = std::to_chars(buf, buf + sizeof buf, v);  // shortest representation that round-trips
    std::string t(buf, r.ptr);
    if (t.find_first_of(".en") == std::string::npos) t += ".0";  // serde_json keeps floats recognisable ("1.0")
    out += t;
}
float read_f32(const Json& j) {
    if (j.kind == Json::Null) return std::numeric_limits<float>::quiet_NaN();
    if (j.kind != Json::Number) panic("json: number expected in \"data\"");
    float v = 0.f;
    auto r = std::from_chars(j.text.data(), j.text.data() + j.text.size(), v);  // correctly rounded, like Rust's parser
    if (r.ec == std::errc::result_out_of_range) return j.text[0] == '-' ? -INFINITY : INFINITY;
    if (r.ec != std::errc() || r.ptr != j.text.data() + j.text.size()) panic("json: bad number '" + j.text + "'");
    return v;
}
std::string array_json(const Shape& shape, const std::vector<float>& data) {
    std::string out = "{\"v\":1,\"dim\":[";
    for (size_t i = 0; i < shape.size(); ++i) { if (i) out += ','; out += std::to_string(shape[i]); }
    out += "],\"data\":[";
    for (size_t i = 0; i < data.size(); ++i) { if (i) out += ','; write_f32(out, data[i]); }
    out += "]}";
    return out;
}
}  // namespace

const Json& Json::at(const std::string& key) const {
    for (const auto& m : members) if (m.first == key) return m.second;
    panic("json: missing field `" + key + "`");
}
bool Json::has(const std::string& key) const {
    for (const auto& m : members) if (m.first == key) return true;
    return false;
}
Json parse(const std::string& text) {
    Parser p(text);
    Json j = p.value();
    p.ws();
    if (p.i != text.size()) p.fail("trailing characters");
    return j;
}

std::string to_json(const Var& v) { return array_json(v.shape(), v.to_vec()); }
std::string to_json(const VarDiff& v) { return array_json(v.shape(), v.to_vec()); }

Var var_from_json(DevicePtr dev, const Json& j) {
    if (j.kind != Json::Object) panic("json: ndarray object expected");
    const Json& ver = j.at("v");
    if (ver.kind != Json::Number || ver.text != "1") panic("json: unknown array version");  // ndarray's ARRAY_FORMAT_VERSION
    const Json& dim = j.at("dim");
    Shape shape;
    if (dim.kind == Json::Array) {
        for (const Json& d : dim.items) {
            if (d.kind != Json::Number) panic("json: bad dim");
            shape.push_back(std::stoi(d.text));
        }
    } else if (dim.kind == Json::Number) {  // Ix1 may also be written as a bare integer by serde tuples of one
        shape.push_back(std::stoi(dim.text));
    } else {
        panic("json: bad dim");
    }
    const Json& data = j.at("data");
    if (data.kind != Json::Array) panic("json: bad data");
    if (data.items.size() != numel(shape)) panic("json: data length does not match dim");  // ndarray: "data and dimension must match in size"
    std::vector<float> host(data.items.size());
    for (size_t i = 0; i < host.size(); ++i) host[i] = read_f32(data.items[i]);
    return from_host(std::move(dev), shape, host.data());
}
Var var_from_json(DevicePtr dev, const std::string& text) { return var_from_json(std::move(dev), parse(text)); }
VarDiff vardiff_from_json(DevicePtr dev, const Json& j) { return var_from_json(std::move(dev), j).requires_grad(); }
VarDiff vardiff_from_json(DevicePtr dev, const std::string& text) { return vardiff_from_json(std::move(dev), parse(text)); }

std::string to_json(const nn::Linear& l) { return "{\"weight\":" + to_json(l.weight) + ",\"bias\":" + to_json(l.bias) + "}"; }
nn::Linear linear_from_json(DevicePtr dev, const Json& j) {
    return nn::Linear(vardiff_from_json(dev, j.at("weight")), vardiff_from_json(dev, j.at("bias")));
}
nn::Linear linear_from_json(DevicePtr dev, const std::string& text) { return linear_from_json(std::move(dev), parse(text)); }

std::string to_json(const nn::LayerNorm& l) {
    if (!l.elementwise_affine) panic("serde: a LayerNorm without affine parameters has nothing to serialise");
    return "{\"weight\":" + to_json(l.weight) + ",\"bias\":" + to_json(l.bias) + "}";
}
nn::LayerNorm layer_norm_from_json(DevicePtr dev, const Json& j, double eps) {
    return nn::LayerNorm(vardiff_from_json(dev, j.at("weight")), vardiff_from_json(dev, j.at("bias")), eps);
}
nn::LayerNorm layer_norm_from_json(DevicePtr dev, const std::string& text, double eps) { return layer_norm_from_json(std::move(dev), parse(text), eps); }
std::string to_json(const nn::GroupNorm& l) {
    if (!l.affine) panic("serde: a GroupNorm without affine parameters has nothing to serialise");
    return "{\"weight\":" + to_json(l.weight) + ",\"bias\":" + to_json(l.bias) + "}";
}
nn::GroupNorm group_norm_from_json(DevicePtr dev, const Json& j, int num_groups, double eps) {
    return nn::GroupNorm(num_groups, vardiff_from_json(dev, j.at("weight")), vardiff_from_json(dev, j.at("bias")), eps);
}
nn::GroupNorm group_norm_from_json(DevicePtr dev, const std::string& text, int num_groups, double eps) {
    return group_norm_from_json(std::move(dev), parse(text), num_groups, eps);
}
std::string to_json(const nn::RMSNorm& l) {
    if (!l.elementwise_affine) panic("serde: an RMSNorm without a weight has nothing to serialise");
    return "{\"weight\":" + to_json(l.weight) + "}";
}
nn::RMSNorm rms_norm_from_json(DevicePtr dev, const Json& j, double eps) { return nn::RMSNorm(vardiff_from_json(dev, j.at("weight")), eps); }
nn::RMSNorm rms_norm_from_json(DevicePtr dev, const std::string& text, double eps) { return rms_norm_from_json(std::move(dev), parse(text), eps); }

std::string to_json(const nn::Embedding& e) { return "{\"weight\":" + to_json(e.weight) + "}"; }
nn::Embedding embedding_from_json(DevicePtr dev, const Json& j, long padding_idx) {
    return nn::Embedding(vardiff_from_json(dev, j.at("weight")), padding_idx);
}
nn::Embedding embedding_from_json(DevicePtr dev, const std::string& text, long padding_idx) {
    return embedding_from_json(std::move(dev), parse(text), padding_idx);
}

std::string to_json(const nn::BatchNormNd& l) {
    if (!l.affine || !l.track_running_stats) panic("serde: a BatchNorm is serialised with its affine parameters and its running statistics");
    return "{\"weight\":" + to_json(l.weight) + ",\"bias\":" + to_json(l.bias) + ",\"running_mean\":" + to_json(l.running_mean) +
           ",\"running_var\":" + to_json(l.running_var) + "}";
}
void batch_norm_load_json(nn::BatchNormNd& l, const Json& j) {
    if (!l.affine || !l.track_running_stats) panic("serde: a BatchNorm is deserialised into a layer with affine parameters and running statistics");
    DevicePtr dev = l.running_mean.device();
    VarDiff w = vardiff_from_json(dev, j.at("weight")), b = vardiff_from_json(dev, j.at("bias"));
    Var rm = var_from_json(dev, j.at("running_mean")), rv = var_from_json(dev, j.at("running_var"));
    const Shape want{l.num_features};
    if (w.shape() != want || b.shape() != want || rm.shape() != want || rv.shape() != want) panic("serde: BatchNorm fields must have shape (num_features)");
    l.weight = std::move(w); l.bias = std::move(b); l.running_mean = std::move(rm); l.running_var = std::move(rv);
}
void batch_norm_load_json(nn::BatchNormNd& l, const std::string& text) { batch_norm_load_json(l, parse(text)); }

}  // namespace serde

// =================================================================================================
// optim
// =================================================================================================
namespace optim {

void Optimizer::register_param(const VarDiff& p) {
    params_.push_back(p);
    std::vector<Shared<HipArray>> st;
    for (int i = 0; i < nstate_; ++i) st.push_back(std::make_shared<HipArray>(p.device(), p.shape()));
    state_.push_back(std::move(st));
    steps_.push_back(0);
}
void Optimizer::step() {
    // a parameter's 1-based step number advances only once its update has been issued: a refused launch (Adam and a decayed
    // Adagrad refuse while the stream is captured) throws out of `optimize` and must leave the bias corrections on schedule
    for (size_t i = 0; i < params_.size(); ++i) {
        optimize(params_[i], state_[i], steps_[i] + 1);
        ++steps_[i];
    }
}
void Optimizer::zero_grad() const {
    for (const VarDiff& p : params_) p.zero_grad();
}

SGD::SGD(float lr, Penalty penalty, float momentum, float dampening, bool nesterov)
    : Optimizer(lr, penalty, momentum > 1.1920929e-7f ? 1 : 0), momentum_(momentum), dampening_(dampening), nesterov_(nesterov) {}
void SGD::step() {
    // one launch per device for all registered parameters (their updates are independent; optimizer.rs:81-86)
    std::vector<float*> w, g, v;
    std::vector<size_t> n, launched;
    std::vector<bool> done(params_.size(), false);
    for (size_t i = 0; i < params_.size(); ++i) {
        if (done[i]) continue;
        const DevicePtr dev = params_[i].device();
        w.clear(); g.clear(); v.clear(); n.clear(); launched.clear();
        for (size_t k = i; k < params_.size(); ++k) {
            if (done[k] || params_[k].device().get() != dev.get()) continue;
            // a parameter registered twice is updated twice, one after the other (the reference iterates its list,
            // optimizer.rs:81-86): the second registration waits for a later launch instead of racing in this one
            if (std::find(w.begin(), w.end(), params_[k].var.data->ptr()) != w.end()) continue;
            done[k] = true;
            launched.push_back(k);
            HipArray& gr = params_[k].grad->borrow();
            w.push_back(params_[k].var.data->ptr()); g.push_back(gr.ptr());
            v.push_back(state_[k].empty() ? nullptr : state_[k][0]->ptr()); n.push_back(gr.len());
        }
        check(nk_sgd_step_multi(dev->raw(), (int)w.size(), w.data(), g.data(), v.data(), n.data(), lr_, momentum_, dampening_,
                                nesterov_ ? 1 : 0, penalty_.l1, penalty_.l2));
        for (size_t k : launched) ++steps_[k];  // counted once issued, as in Optimizer::step (SGD itself ignores the number)
    }
}
void SGD::optimize(const VarDiff& p, std::vector<Shared<HipArray>>& st, int) {
    HipArray& g = p.grad->borrow();
    check(nk_sgd_step(p.device()->raw(), p.var.data->ptr(), g.ptr(), st.empty() ? nullptr : st[0]->ptr(), g.len(), lr_,
                      momentum_, dampening_, nesterov_ ? 1 : 0, penalty_.l1, penalty_.l2));
}

Adam::Adam(float lr, float beta1, float beta2, float eps, Penalty penalty, bool amsgrad)
    : Optimizer(lr, penalty, amsgrad ? 3 : 2), beta1_(beta1), beta2_(beta2), eps_(eps), amsgrad_(amsgrad) {}
void Adam::optimize(const VarDiff& p, std::vector<Shared<HipArray>>& st, int step) {
    HipArray& g = p.grad->borrow();
    check(nk_adam_step(p.device()->raw(), p.var.data->ptr(), g.ptr(), st[0]->ptr(), st[1]->ptr(),
                       amsgrad_ ? st[2]->ptr() : nullptr, g.len(), lr_, beta1_, beta2_, eps_, step, penalty_.l1, penalty_.l2));
}

AdamW::AdamW(float lr, float beta1, float beta2, float eps, float weight_decay, bool amsgrad)
    : Optimizer(lr, Penalty{}, amsgrad ? 3 : 2), beta1_(beta1), beta2_(beta2), eps_(eps), weight_decay_(weight_decay), amsgrad_(amsgrad) {}
void AdamW::step() {
    // one call per device for all registered parameters, as SGD::step; the 1-based step number travels per parameter (a
    // parameter registered late is at an earlier step than its neighbours in the same launch)
    std::vector<float*> w, m, v, vmax;
    std::vector<const float*> g;
    std::vector<size_t> n, launched;
    std::vector<int> step;
    std::vector<bool> done(params_.size(), false);
    for (size_t i = 0; i < params_.size(); ++i) {
        if (done[i]) continue;
        const DevicePtr dev = params_[i].device();
        w.clear(); g.clear(); m.clear(); v.clear(); vmax.clear(); n.clear(); step.clear(); launched.clear();
        for (size_t k = i; k < params_.size(); ++k) {
            if (done[k] || params_[k].device().get() != dev.get()) continue;
            // registered twice: the second update waits for a later call (nk_adamw_step_multi refuses one w twice)
            if (std::find(w.begin(), w.end(), params_[k].var.data->ptr()) != w.end()) continue;
            done[k] = true;
            launched.push_back(k);
            HipArray& gr = params_[k].grad->borrow();
            w.push_back(params_[k].var.data->ptr()); g.push_back(gr.ptr());
            m.push_back(state_[k][0]->ptr()); v.push_back(state_[k][1]->ptr());
            vmax.push_back(amsgrad_ ? state_[k][2]->ptr() : nullptr);
            n.push_back(gr.len()); step.push_back(steps_[k] + 1);
        }
        check(nk_adamw_step_multi(dev->raw(), (int)w.size(), w.data(), g.data(), m.data(), v.data(), vmax.data(), n.data(), step.data(),
                                  lr_, beta1_, beta2_, eps_, weight_decay_));
        for (size_t k : launched) ++steps_[k];  // only once issued: a refused capture leaves the bias corrections on schedule
    }
}
void AdamW::optimize(const VarDiff& p, std::vector<Shared<HipArray>>& st, int step) {
    HipArray& g = p.grad->borrow();
    check(nk_adamw_step(p.device()->raw(), p.var.data->ptr(), g.ptr(), st[0]->ptr(), st[1]->ptr(), amsgrad_ ? st[2]->ptr() : nullptr,
                        g.len(), lr_, beta1_, beta2_, eps_, step, weight_decay_));
}

// {total_norm, coef} of `params` into out[0..2) and the gradients scaled; returns the 0-d view of out[0]
static Var clip_into(const std::vector<VarDiff>& params, float max_norm, const Shared<HipArray>& out) {
    std::vector<float*> g;
    std::vector<size_t> n;
    for (const VarDiff& p : params) {
        if (p.device().get() != out->device().get())
            panic("clip_grad_norm: the parameters live on more than one device (a cross-device norm is not offered)");
        HipArray& gr = p.grad->borrow();
        if (std::find(g.begin(), g.end(), gr.ptr()) != g.end()) continue;  // listed twice: counted once
        g.push_back(gr.ptr()); n.push_back(gr.len());
    }
    check(nk_clip_grad_norm_multi(out->device()->raw(), (int)g.size(), g.data(), n.data(), max_norm, out->ptr()));
    return Var::leaf(std::make_shared<HipArray>(out, 0, Shape{}));
}
Var clip_grad_norm(const std::vector<VarDiff>& params, float max_norm) {
    if (params.empty()) panic("clip_grad_norm: no parameters");
    return clip_into(params, max_norm, std::make_shared<HipArray>(params[0].device(), Shape{2}, HipArray::Uninit{}));
}
Var Optimizer::clip_grad_norm(float max_norm) {
    if (params_.empty()) panic("clip_grad_norm: no parameters registered");
    if (!clip_out_) clip_out_ = std::make_shared<HipArray>(params_[0].device(), Shape{2}, HipArray::Uninit{});
    return clip_into(params_, max_norm, clip_out_);
}

Adagrad::Adagrad(float lr, float lr_decay, float eps, Penalty penalty)
    : Optimizer(lr, penalty, 1), lr_decay_(lr_decay), eps_(eps) {}
void Adagrad::optimize(const VarDiff& p, std::vector<Shared<HipArray>>& st, int step) {
    HipArray& g = p.grad->borrow();
    check(nk_adagrad_step(p.device()->raw(), p.var.data->ptr(), g.ptr(), st[0]->ptr(), g.len(), lr_, lr_decay_, eps_, step,
                          penalty_.l1, penalty_.l2));
}

RMSProp::RMSProp(float lr, float alpha, float eps, float momentum, bool centered, Penalty penalty)
    : Optimizer(lr, penalty, 3), alpha_(alpha), eps_(eps), momentum_(momentum), centered_(centered) {}
void RMSProp::optimize(const VarDiff& p, std::vector<Shared<HipArray>>& st, int) {
    HipArray& g = p.grad->borrow();
    const bool mom = momentum_ > 1.1920929e-7f;
    check(nk_rmsprop_step(p.device()->raw(), p.var.data->ptr(), g.ptr(), st[0]->ptr(), centered_ ? st[1]->ptr() : nullptr,
                          mom ? st[2]->ptr() : nullptr, g.len(), lr_, alpha_, eps_, momentum_, penalty_.l1, penalty_.l2));
}

namespace lr_scheduler {
void LRScheduler::step() {
    last_lr_ = current_lr_;  // prepare_step, lr_scheduler/mod.rs:51-59
    epoch_ += 1;
    float lr = current_lr_;
    if (update(lr)) {
        current_lr_ = lr;
        opt_.set_lr(current_lr_);
    }
}
bool StepLR::update(float& lr) {
    if (step_size_ == 0) panic("attempt to calculate the remainder with a divisor of zero");  // `rem_euclid(0)`
    if (epoch_ % step_size_ != 0) return false;
    lr = last_lr_ * gamma_;
    return true;
}
bool MultiStepLR::update(float& lr) {
    if (std::find(milestones_.begin(), milestones_.end(), epoch_) == milestones_.end()) return false;
    lr = last_lr_ * gamma_;
    return true;
}
}  // namespace lr_scheduler

}  // namespace optim

// =================================================================================================
// dp
// =================================================================================================
namespace dp {

std::string Communicator::unique_id() {
    std::string id(NK_COMM_ID_BYTES, '\0');
    check(nk_comm_unique_id(&id[0]));
    return id;
}
Communicator::Communicator(DevicePtr dev, int nranks, int rank, const std::string& id)
    : dev_(std::move(dev)), rank_(rank), size_(nranks) {
    if (id.size() != NK_COMM_ID_BYTES) panic("communicator id must be 128 bytes");
    check(nk_comm_init_rank(dev_->raw(), nranks, rank, id.data(), &h_));
}
Communicator::Communicator(DevicePtr dev, int nranks, int channels, double gbps) : dev_(std::move(dev)), rank_(0), size_(nranks) {
    check(nk_comm_init_replicas(dev_->raw(), nranks, channels, gbps, &h_));
}
std::shared_ptr<Communicator> Communicator::replicas(DevicePtr dev, int nranks, int channels, double gbps) {
    return std::shared_ptr<Communicator>(new Communicator(std::move(dev), nranks, channels, gbps));
}
Communicator::~Communicator() { nk_comm_destroy(h_); }

GradientSync::GradientSync(std::shared_ptr<Communicator> comm, const std::vector<VarDiff>& params, size_t small_elems)
    : comm_(std::move(comm)), small_elems_(small_elems) {
    for (const VarDiff& p : params) {
        if (!params_.emplace(p.grad.get(), p.grad).second) continue;  // registered twice: one exchange
        const size_t len = numel(p.shape());
        bytes_ += len * sizeof(float);
        n_small_ += len < small_elems_;
        for (int k = 0; k < 2; ++k) {  // up to two pieces per gradient in flight
            nk_event* ev = nullptr;
            check(nk_event_create(comm_->device()->raw(), &ev));
            events_.push_back(ev);
        }
    }
    nk_event* ev = nullptr;  // one more for the group of small gradients
    check(nk_event_create(comm_->device()->raw(), &ev));
    events_.push_back(ev);
}
GradientSync::~GradientSync() {
    if (busy_told_) nk_device_set_busy_slots(comm_->device()->raw(), 0);
    for (nk_event* e : events_) nk_event_destroy(e);
}
bool GradientSync::wants_parts(const Gradient* g) const {
    if (!active()) return false;
    auto it = params_.find(g);
    if (it == params_.end()) return false;
    // a small gradient is always welcome early (it is handed over whole: nothing is split for it) - the group of small
    // gradients leaves as soon as the last of them is final
    if (numel(it->second->shape()) < small_elems_) return parts_ != Parts::None;
    switch (parts_) {
        case Parts::All: return true;
        case Parts::None: return false;
        default: return g == split_next_;
    }
}
void GradientSync::flush_small() {
    if (small_pending_.empty()) return;
    std::vector<float*> bufs;
    std::vector<size_t> counts;
    for (const Gradient* g : small_pending_) {
        HipArray& a = params_.at(g)->borrow();
        bufs.push_back(a.ptr());
        counts.push_back(a.len());
        elems_ += a.len();
    }
    small_pending_.clear();
    nk_event* ev = events_[next_event_++ % events_.size()];
    check(nk_event_record(ev, 0));  // every pending small gradient was final before this point of the compute stream
    check(nk_allreduce_sum_group_async(comm_->raw(), bufs.data(), counts.data(), (int)bufs.size(), ev));
    ++issued_;
}
void GradientSync::grad_part_ready(const Gradient* g, size_t offset, size_t count) {
    auto it = params_.find(g);
    if (it == params_.end() || !active() || count == 0) return;
    HipArray& a = it->second->borrow();
    if (offset + count > a.len()) panic("grad_part_ready: piece exceeds the gradient");
    if (parts_done_[g] + count > a.len()) panic("grad_part_ready: pieces overlap");
    parts_done_[g] += count;
    if (a.len() < small_elems_) {  // a small gradient travels whole, with the group
        if (count != a.len()) panic("grad_part_ready: a small gradient must be handed over whole");
        small_pending_.push_back(g);
        if (small_pending_.size() == n_small_) flush_small();
        return;
    }
    last_large_ = g;
    nk_event* ev = events_[next_event_++ % events_.size()];
    check(nk_event_record(ev, 0));  // everything up to the launch that finished this piece
    check(nk_allreduce_sum_async(comm_->raw(), a.ptr() + offset, count, ev));
    elems_ += count;
    ++issued_;
    if (busy_slots_ > 0 && !busy_told_) {  // the exchange's workgroups share the chip with every launch from here to join()
        check(nk_device_set_busy_slots(comm_->device()->raw(), busy_slots_));
        busy_told_ = true;
    }
}
void GradientSync::grad_ready(const Gradient* g) {
    auto it = params_.find(g);
    if (it == params_.end()) return;
    if (!active()) return;  // nothing to exchange
    HipArray& a = it->second->borrow();
    auto pd = parts_done_.find(g);
    if (pd != parts_done_.end() && pd->second != 0) {
        const size_t done = pd->second;
        pd->second = 0;
        if (done == a.len()) return;  // already handed over piece by piece
        panic("GradientSync: a gradient was only partly exchanged piecewise");
    }
    grad_part_ready(g, 0, a.len());
    parts_done_[g] = 0;
}
void GradientSync::join() {
    flush_small();  // small gradients of parameters some of whose siblings never became final this pass
    split_next_ = last_large_;  // (every rank runs the same tape: the same gradient on every rank, so the collectives still pair up)
    last_large_ = nullptr;
    next_event_ = 0;
    for (auto& kv : parts_done_) kv.second = 0;
    if (busy_told_) {
        check(nk_device_set_busy_slots(comm_->device()->raw(), 0));
        busy_told_ = false;
    }
    if (active()) check(nk_comm_join(comm_->raw()));
}

void all_reduce_gradients(const Communicator& comm, const std::vector<VarDiff>& params) {
    if (comm.size() == 1) return;
    for (const VarDiff& p : params) {
        HipArray& a = p.grad->borrow();
        check(nk_allreduce_sum_async(comm.raw(), a.ptr(), a.len(), nullptr));
    }
    check(nk_comm_join(comm.raw()));
}

}  // namespace dp

}  // namespace neuronika

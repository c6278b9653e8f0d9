// Host-side mirror of neuronika's Var / VarDiff tape for the HIP backend (C++17).
//
// The reference's host code is Rust; no Rust toolchain exists in this environment, so the
// host side above the C ABI (include/neuronika_hip.h) is written in C++ with the reference's
// own names, argument meaning and error behaviour:
//
//   reference (neuronika-variable/src)              here
//   ------------------------------------------------------------------------------------------
//   autograd.rs:7-25    trait Forward / Backward     struct Forward / Backward
//   gradient.rs:8-79    NoGrad, Gradient             struct NoGrad, class Gradient
//   history.rs:9-125    HistoryId, History<T>        class History<T>
//   var.rs:34-128       Var<D>                       class Var   (rank is a run-time Shape)
//   vardiff.rs:35-168   VarDiff<D>                   class VarDiff
//   cuda/device.rs, cuda/cuarray.rs                  class Device, class HipArray
//   lib.rs:29-36        enum Reduction               enum class Reduction
//   neuronika-nn/src/lib.rs:406-448  Linear          nn::Linear   (+ Conv2d, Dropout, MHA)
//   neuronika-optim/src/optimizer.rs, sgd/mod.rs     optim::SGD
//   (net-new)                                         dp::Communicator / dp::GradientSync
//
// Semantics kept from the reference: graph construction allocates ZEROED output / gradient
// buffers and computes nothing; `.forward()` runs the forward tape in insertion order and
// overwrites every node output; `.backward(seed)` fills the root gradient with `seed` and runs
// the backward tape in reverse, every node accumulating (`+=`) into its operands' gradients;
// intermediate gradients are NOT re-zeroed between calls (vardiff.rs:125-141) — use
// `no_grad()` + `with_grad()` (gradient.rs:64-79) to drop and re-create them.
// Errors: the reference panics; here `neuronika::Panic` (a std::runtime_error) is thrown.
// Threading: like `Rc<RefCell<..>>` graphs, one host thread per graph/device.
#pragma once

#include <cstddef>
#include <cstdint>
#include <functional>
#include <memory>
#include <set>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "neuronika_hip.h"

namespace neuronika {

using Shape = std::vector<int>;

struct Panic : std::runtime_error {
    using std::runtime_error::runtime_error;
};
[[noreturn]] void panic(const std::string& msg);
void check(int status);  // non-zero C-ABI status -> Panic(nk_last_error())

size_t numel(const Shape& s);

// ---------------------------------------------------------------------------------------------
// Device + device array (reference template: cuda/device.rs:11-58, cuda/cuarray.rs:10-117)
// ---------------------------------------------------------------------------------------------
class Device : public std::enable_shared_from_this<Device> {
   public:
    static std::shared_ptr<Device> create(int idx);
    ~Device();
    nk_device* raw() const { return h_; }
    int index() const { return idx_; }
    void sync() const;
    // Stream-ordered caching allocator: blocks released by graph buffers are re-used for later
    // allocations of the same size (all work runs in order on the compute stream).
    float* alloc_zeroed(size_t n);
    float* alloc_uninit(size_t n);  // contents undefined (a gradient whose zero fill is still pending)
    void release(float* p, size_t n);
    size_t bytes_in_use() const { return in_use_; }
    // hipGraph capture of a launch-bound step (see nk_graph_begin in the C header for the rules)
    void graph_begin();
    std::shared_ptr<class Graph> graph_end();

   private:
    Device() = default;
    nk_device* h_ = nullptr;
    int idx_ = 0;
    std::unordered_map<size_t, std::vector<float*>> pool_;
    size_t in_use_ = 0;
};
using DevicePtr = std::shared_ptr<Device>;

class Graph {  // a captured, replayable sequence of launches on one device
   public:
    Graph(nk_graph* g, std::shared_ptr<Device> dev) : dev_(std::move(dev)), g_(g) {}
    ~Graph();
    Graph(const Graph&) = delete;
    Graph& operator=(const Graph&) = delete;
    void launch() const;

   private:
    std::shared_ptr<Device> dev_;  // a graph keeps its device alive (captured kernels hold the device's workspace addresses)
    nk_graph* g_;
};

class HipArray {
   public:
    HipArray(DevicePtr dev, Shape shape);  // `CuArray::zeroed`
    struct Uninit {};
    HipArray(DevicePtr dev, Shape shape, Uninit);  // undefined contents
    // `shape` elements of `parent` starting `offset` elements in: shares the parent's buffer and keeps it alive (the packed
    // projection weights of nn::MultiheadAttention: three parameters, one allocation)
    HipArray(std::shared_ptr<HipArray> parent, size_t offset, Shape shape);
    ~HipArray();
    HipArray(const HipArray&) = delete;
    HipArray& operator=(const HipArray&) = delete;

    static std::shared_ptr<HipArray> from_host(DevicePtr dev, const Shape& shape, const float* host);
    void upload(const float* host);              // `CuArray::from_ndarray`
    void download(float* host) const;            // `CuArray::as_ndarray`
    std::vector<float> to_vec() const;
    void fill(float v);
    size_t len() const { return len_; }
    const Shape& shape() const { return shape_; }
    float* ptr() const { return ptr_; }
    const DevicePtr& device() const { return dev_; }

   private:
    DevicePtr dev_;
    Shape shape_;
    size_t len_;
    float* ptr_;
    std::shared_ptr<HipArray> parent_;  // set for a view: the buffer belongs to the parent
};
template <class T>
using Shared = std::shared_ptr<T>;  // utils.rs:9  `Shared<T> = Rc<RefCell<T>>`

// ---------------------------------------------------------------------------------------------
// autograd.rs / gradient.rs
// ---------------------------------------------------------------------------------------------
struct Forward {
    virtual ~Forward() = default;
    virtual void forward() const = 0;
};
class Gradient;
struct Backward {
    virtual ~Backward() = default;
    virtual void backward() const = 0;
    // gradients this node accumulates into (used to tell when a leaf gradient is final)
    virtual void targets(std::vector<const Gradient*>& out) const = 0;
    // the subset of `targets` this node can write PRE-MASKED when the gradient asks for it (`Gradient::premask_source`):
    // a Linear node's input gradient, whose GEMM epilogue applies the ReLU mask of the node that produced the input
    virtual void premask_targets(std::vector<const Gradient*>&) const {}
};
// Called by VarDiff::backward right after the LAST tape node writing into a gradient has been
// issued: the hook of the data-parallel exchange (dp::GradientSync).
struct BackwardHook {
    virtual ~BackwardHook() = default;
    virtual void grad_ready(const Gradient* g) = 0;
    // Optional finer grain: a node that finishes a gradient before its own `backward()` returns (Linear: the bias
    // gradient first, then the weight gradient in row blocks) reports each finished contiguous piece, so the exchange
    // starts while the node is still issuing launches.  A node obtains the hook through `parts_hook(g)` only, which
    // answers null unless THIS node is the last writer of g on the tape (a shared / tied parameter keeps accumulating
    // in a later node; its exchange must wait for `grad_ready`).  `grad_ready` still follows once the node is done.
    virtual bool wants_parts(const Gradient*) const { return false; }
    virtual void grad_part_ready(const Gradient*, size_t /*offset*/, size_t /*count*/) {}
};
// The hook of the backward pass being issued on this thread if it wants pieces of `g` AND the node now running is
// the last tape node that writes g; null otherwise (also outside `backward(seed, hook)`).
BackwardHook* parts_hook(const Gradient* g);
struct NoGrad {
    virtual ~NoGrad() = default;
    virtual void no_grad() = 0;
    virtual void with_grad() = 0;
};

class Gradient : public NoGrad {
   public:
    // `ndarray_zeros` (gradient.rs:47-54).  The zero fill is LAZY: the buffer is allocated without a memset and
    // `zero_pending()` stays true until somebody looks at it.  `borrow()` (read / `+=` access) materialises the
    // zeros first; `borrow_first_write(assign)` hands a pending fill to a node that can ASSIGN instead of `+=`
    // (`0 + v`, same values, no memset and no read of the destination).
    Gradient(DevicePtr dev, Shape shape);
    // A gradient whose buffer is `shape` elements of `storage` starting at `offset` (packed parameters: the gradients of
    // several parameters in one allocation, so that ONE GEMM can write them all).  Same lazy zero fill, per view.
    Gradient(Shared<HipArray> storage, size_t offset, Shape shape);
    HipArray& borrow() const;              // panics when de-allocated
    HipArray& borrow_first_write(bool& assign) const;
    void zero();                           // `zero_grad` (vardiff.rs:100-102), lazily
    bool zero_pending() const { return pending_zero_; }
    Shared<HipArray> array() const { return array_; }
    // true for a view gradient over `storage` starting `offset` elements in (packed parameters)
    bool is_view_of(const Shared<HipArray>& storage, size_t offset) const { return storage_ && storage_.get() == storage.get() && offset_ == offset; }
    // Stand `external` in for this gradient's buffer (returns the previous one) without touching device memory: how
    // `VarDiff::backward_from` presents an upstream gradient tensor to the root's backward nodes (they read through
    // `borrow()` at run time).  The buffer counts as written.
    Shared<HipArray> exchange_array(Shared<HipArray> external);
    const Shape& shape() const { return shape_; }
    void no_grad() override;
    void with_grad() override;
    // Fused Linear+ReLU (`nn::Linear::forward_relu`): the gradient of its output y holds dL/dz of the PRE-activation.  The
    // node names y as the mask source; `VarDiff::backward` decides per pass (`set_premasked`) whether every node that
    // writes this gradient on the tape can apply `(y > 0) *` itself while storing (`Backward::premask_targets`); if not,
    // the writers store plain contributions and the owner masks the buffer in place before using it (idempotent).
    void set_premask_source(Shared<HipArray> y) { premask_src_ = std::move(y); }
    const Shared<HipArray>& premask_source() const { return premask_src_; }
    void set_premasked(bool on) const { premasked_ = on; }
    bool premasked() const { return premasked_; }

   private:
    DevicePtr dev_;
    Shape shape_;
    Shared<HipArray> array_;
    mutable bool pending_zero_ = true;
    Shared<HipArray> premask_src_;
    mutable bool premasked_ = false;
    Shared<HipArray> storage_;  // set for a view gradient
    size_t offset_ = 0;
};

// ---------------------------------------------------------------------------------------------
// history.rs — the tape.  Entries are identified by node address and ordered by the size of
// the history at insertion; merging keeps one entry per address.
// ---------------------------------------------------------------------------------------------
template <class T>
class History {
   public:
    void merge(const History& other);
    void insert(const void* ptr, T op);
    size_t len() const { return path_.size(); }
    size_t buffer_len() const { return buffer_->size(); }
    std::vector<T> to_vec() const;
    std::vector<T>& buffer_mut() const { return *buffer_; }

   private:
    struct Item {
        const void* ptr;
        size_t order;
        T op;
    };
    std::vector<Item> path_;  // sorted by order (stable)
    // the reference clones the RefCell<Vec> with the History; a fresh buffer per copy is
    // equivalent because insert() truncates it and forward() repopulates an empty one.
    std::shared_ptr<std::vector<T>> buffer_ = std::make_shared<std::vector<T>>();

   public:
    History() = default;
    History(const History& o) : path_(o.path_), buffer_(std::make_shared<std::vector<T>>(*o.buffer_)) {}
    History& operator=(const History& o) {
        path_ = o.path_;
        buffer_ = std::make_shared<std::vector<T>>(*o.buffer_);
        return *this;
    }
};

struct ForwardEntry {
    Shared<Forward> op;
    Shared<bool> computed;
};
struct BackwardEntry {
    Shared<Backward> op;
    Shared<NoGrad> grad;
};

enum class Reduction { Sum = 0, Mean = 1 };  // lib.rs:29-36
// The smooth activations of neuronika_hip.h (`enum nk_activation`, same values; ours: the reference has none of them): the gate of
// `glu`, and what `gelu` / `silu` run
enum class Activation { Gelu = 0, GeluTanh = 1, Silu = 2, Sigmoid = 3 };

class VarDiff;
namespace nn {
struct RotaryEmbedding;
struct Sampler;
struct Segments;
}

// ---------------------------------------------------------------------------------------------
// var.rs — non-differentiable variable
// ---------------------------------------------------------------------------------------------
// `PaddingMode` implementors (node/pad/{zero,constant,reflective,replicative}/mod.rs)
struct PaddingMode {
    enum Kind { Zero, Constant, Reflective, Replicative } kind = Zero;
    float value = 0.f;
    static PaddingMode zero() { return {Zero, 0.f}; }
    static PaddingMode constant(float v) { return {Constant, v}; }
    static PaddingMode reflective() { return {Reflective, 0.f}; }
    static PaddingMode replicative() { return {Replicative, 0.f}; }
};

class Var {
   public:
    Shared<HipArray> data;
    History<ForwardEntry> history;

    static Var leaf(Shared<HipArray> array);                                          // var.rs:46
    static Var node(Shared<HipArray> data, Shared<Forward> op, History<ForwardEntry> h);  // var.rs:53
    const Shape& shape() const { return data->shape(); }
    DevicePtr device() const { return data->device(); }

    VarDiff requires_grad() const;  // var.rs:103
    void forward() const;           // var.rs:110-128
    float item() const;             // var.rs:133
    std::vector<float> to_vec() const { return data->to_vec(); }

    Var sum() const;                                  // var.rs:201
    Var mean() const;                                 // var.rs:209
    Var relu() const;                                 // var.rs:243
    // pointwise nodes (var.rs:222-302) + negation (`-x`) and unsqueeze (var.rs:425)
    Var neg() const;
    Var pow(int exp) const;
    Var sqrt() const;
    Var leaky_relu() const;
    Var softplus() const;
    Var sigmoid() const;
    Var tanh() const;
    Var ln() const;
    Var exp() const;
    // Smooth and gated activations (ours: the reference has none; semantics in neuronika_hip.h), ONE node each:
    // gelu: x Phi(x) (torch's approximate="none"), or its tanh form; silu: x sigma(x);
    // glu: a * gate(b) over the two halves (a, b) of the last axis, which must be even - Sigmoid is torch's F.glu, Gelu is GeGLU,
    // Silu is SwiGLU
    Var gelu(bool tanh_approx = false) const;
    Var silu() const;
    Var glu(Activation gate = Activation::Sigmoid) const;
    // Rotary position embedding (ours; semantics in neuronika_hip.h) of a (batch*T, heads*head_dim) value at positions 0 .. T-1: the
    // first `rot` columns of every head rotated by the angles of the row's position, ONE node.  Panics on a shape mismatch or
    // T > max_pos.
    Var rope(const nn::RotaryEmbedding& rotary, int batch, int heads) const;
    // Grouped-query attention (ours; semantics at nk_repeat_kv_fwd in neuronika_hip.h): a (rows, kv_heads*head_dim) value with every
    // head written `groups` times, (rows, kv_heads*groups*head_dim) - what the attention core reads as the keys / values of
    // `kv_heads*groups` query heads.  One forward node, a bit-exact copy.
    Var repeat_kv(int groups, int head_dim) const;
    // The next token of every sample of (batch*T, V) logits (ours; semantics at nk_sample_fwd in neuronika_hip.h): a (batch,) value of
    // ids in f32, drawn from the LAST row of each sample, ONE node, no gradient.  Panics when batch does not divide the rows.
    Var sample(const nn::Sampler& sampler, int batch) const;
    Var unsqueeze(int axis) const;
    // Pooling over the spatial axes of an (N, C, spatial...) input (ours: the reference has none; semantics in neuronika_hip.h):
    // nd = rank - 2 = the length of `kernel`, `stride` (empty: stride = kernel) and `padding` (empty: zeros); floor mode, dilation 1.
    // global_avg_pool = avg_pool over the whole spatial extents, result (N, C, 1, ..); flatten: (N, d_1, .., d_r) -> (N, prod d_i).
    Var max_pool(const std::vector<int>& kernel, const std::vector<int>& stride, const std::vector<int>& padding) const;
    Var avg_pool(const std::vector<int>& kernel, const std::vector<int>& stride, const std::vector<int>& padding,
                 bool count_include_pad = true) const;
    Var global_avg_pool() const;
    // Resampling of the spatial axes of an (N, C, spatial...) input to `out_size` (one entry per axis; ours: the reference has none;
    // semantics in neuronika_hip.h): mode "nearest", or "linear" / "bilinear" / "trilinear" for 1 / 2 / 3 spatial axes.
    Var upsample(const std::vector<int>& out_size, const std::string& mode = "nearest", bool align_corners = false) const;
    Var flatten() const;
    Var softmax(int axis) const;                      // var.rs:318
    Var log_softmax(int axis) const;                  // var.rs:338
    Var t() const;                                    // var.rs:347
    // Layer normalisation over the trailing dimensions (ours: the reference has none; semantics in neuronika_hip.h).  The
    // normalised shape is gamma's (beta's must equal it), or `normalized_shape` without affine parameters.  The Var forms keep
    // no statistics; with differentiable parameters the result is differentiable in them alone.
    Var layer_norm(const Var& gamma, const Var& beta, double eps = 1e-5) const;
    Var layer_norm(const Shape& normalized_shape, double eps = 1e-5) const;
    VarDiff layer_norm(const VarDiff& gamma, const VarDiff& beta, double eps = 1e-5) const;
    // RMS normalisation over the trailing dimensions (ours: the reference has none; semantics in neuronika_hip.h): no centring,
    // no beta.  The normalised shape is gamma's, or `normalized_shape` without a weight.  The Var forms keep no statistics.
    Var rms_norm(const Var& gamma, double eps = 1e-6) const;
    Var rms_norm(const Shape& normalized_shape, double eps = 1e-6) const;
    VarDiff rms_norm(const VarDiff& gamma, double eps = 1e-6) const;
    // Group normalisation of an (N, C, spatial...) input over `num_groups` channel groups (ours: the reference has none; semantics
    // in neuronika_hip.h); num_groups == C is instance normalisation.  gamma / beta of shape (C), or neither.  The Var forms keep
    // no statistics.  The input needs at least 2 dimensions; C % num_groups != 0 throws before any launch.
    Var group_norm(int num_groups, const Var& gamma, const Var& beta, double eps = 1e-5) const;
    Var group_norm(int num_groups, double eps = 1e-5) const;
    VarDiff group_norm(int num_groups, const VarDiff& gamma, const VarDiff& beta, double eps = 1e-5) const;
    // Batch normalisation over (N, spatial...) for each channel of an (N, C, spatial...) input (ours: the reference has none;
    // semantics in neuronika_hip.h).  gamma / beta of shape (C), both or neither (null: no affine part); running_mean /
    // running_var of shape (C), both or neither, updated IN PLACE by a training forward.  `status` is read each time the forward
    // node runs: true trains (batch statistics), false infers (running statistics; the batch's when there are none).  The Var
    // forms keep no statistics; with differentiable parameters the result is differentiable in them alone.
    Var batch_norm(const Var* gamma, const Var* beta, const Var* running_mean, const Var* running_var, double momentum, double eps,
                   Shared<bool> status) const;
    VarDiff batch_norm(const VarDiff& gamma, const VarDiff& beta, const Var* running_mean, const Var* running_var, double momentum, double eps,
                       Shared<bool> status) const;
    Var dropout(double p, Shared<bool> status) const; // var.rs:375
    std::vector<Var> chunks(const Shape& chunk_size) const;             // var.rs:401
    Var cat(const std::vector<Var>& variables, int axis) const;         // var.rs:564
    Var stack(const std::vector<Var>& variables, int axis) const;       // var.rs:614 (MultiStack)
    Var mse(const Var& target, Reduction reduction) const;              // var.rs:454
    Var mae(const Var& target, Reduction reduction) const;              // var.rs:433
    Var bce(const Var& target, Reduction reduction) const;              // var.rs:484
    Var bce_with_logits(const Var& target, Reduction reduction) const;  // var.rs:513
    Var kldiv(const Var& target, Reduction reduction) const;            // var.rs:542
    Var nll(const Var& target, Reduction reduction) const;              // var.rs:671
    // Cross entropy of class logits (ours: the reference stops at nll; semantics in neuronika_hip.h): self is (minibatch, C, d1..dk),
    // `target` (minibatch, d1..dk) holds class ids as f32; log-softmax and NLL in ONE node, no (N, C) intermediate.  Ids >= C and
    // ids equal to `ignore_index` (< 0: none) are inactive; Mean divides by the number of active positions.
    Var cross_entropy(const Var& target, Reduction reduction, long ignore_index = -1, double label_smoothing = 0.0) const;
    Var mv(const Var& rhs) const;                                        // var.rs:1098 (matrix . vector)
    VarDiff mv(const VarDiff& rhs) const;
    Var vm(const Var& rhs) const;                                        // var.rs:1129 (vector . matrix)
    VarDiff vm(const VarDiff& rhs) const;
    Var vv(const Var& rhs) const;                                        // var.rs:1160 (dot product)
    VarDiff vv(const VarDiff& rhs) const;
    Var pad(const std::vector<int>& padding, float value = 0.f) const;  // var.rs:726 (Zero/Constant)
    Var pad(const std::vector<int>& padding, PaddingMode mode) const;   // any `PaddingMode` (pad/mod.rs:17-27)
    Var mm(const Var& rhs) const;                                        // var.rs:1034
    VarDiff mm(const VarDiff& rhs) const;
    Var mm_t(const Var& rhs) const;                                      // var.rs:1065
    VarDiff mm_t(const VarDiff& rhs) const;                              // var.rs:1081
    // `kernel.convolution(input, stride, dilation, groups)`  var.rs:1296-1371
    Var convolution(const Var& input, const std::vector<int>& stride, const std::vector<int>& dilation,
                    int groups) const;
    // composed-attention glue (Chunk((S,dh)) tiles / cat): SURVEY.md 8a note
    Var split_heads(int B, int S, int H, int dh) const;
    Var merge_heads(int B, int S, int H, int dh) const;
    // batched (b,h) matrix products over [B*H, S, *] tiles = B*H `mm` / `mm_t` nodes
    Var bmm(const Var& rhs) const;
    Var bmm_t(const Var& rhs) const;
    // the same per-(batch, head) products taken DIRECTLY on the (B*S, H*dh) projection layout (strided GEMM operands:
    // row stride H*dh, head offset h*dh) - no head split / merge copies:
    //   heads_scores : self = Q (B*S, H*dh), keys K (B*S, H*dh)      -> (B*H, S, S)   Q_bh . K_bh^T
    //   heads_context: self = P (B*H, S, S), values V (B*S, H*dh)    -> (B*S, H*dh)   P_bh . V_bh
    Var heads_scores(const Var& keys, int B, int S, int H, int dh) const;
    Var heads_context(const Var& values, int B, int S, int H, int dh) const;
    // dropout(softmax(self * scale, last axis), p): the Multiplication + Softmax + Dropout nodes of
    // the attention probabilities as ONE node (same values, one pass over the score tensor)
    // (store_probs = false: the backward pass recomputes the probabilities from the scores, bit-identically)
    Var attention_probs(float scale, double p, Shared<bool> status, bool store_probs = false) const;
    // the whole per-(sample, head) chain heads_scores -> attention_probs -> heads_context as ONE node on the fused
    // attention kernels (nk_attention_fwd): self = Q, all three operands (B*S, H*dh) -> (B*S, H*dh).  The score tile
    // stays on chip between the two products; see attention_core_supported() for the shapes it takes.
    // causal: query r attends to keys <= r (nk_attention_causal_fwd; the composition gains one Addition node in front of the Softmax)
    // window > 0 (needs causal): query r attends to keys r - window < k <= r.  S <= window is the causal node as it is; S > window
    // runs nk_attention_band_* on banded scratch sized by nk_attention_band_scratch / _mask_words and allocated without a fill -
    // in a graph without gradients too (the band kernels have no inference form).
    // segments (needs causal; batch and S must be B and S): query r attends to the keys of its own document only, max(lo[r], r -
    // window + 1) .. r.  One document per sample (max_len >= S) is the call without segments; otherwise nk_attention_seg_* on the
    // band's scratch at window := span = min(max_len, window), allocated without a fill, in every graph.
    Var heads_attention(const Var& keys, const Var& values, int B, int S, int H, int dh, float scale, double p,
                        Shared<bool> status, bool causal = false, int window = 0, const nn::Segments* segments = nullptr) const;
    static bool attention_core_supported(int S, int dh, double p);
};

// ---------------------------------------------------------------------------------------------
// vardiff.rs — differentiable variable
// ---------------------------------------------------------------------------------------------
namespace nn { struct LinearOrigin; }
class VarDiff {
    void run_backward(BackwardHook* hook) const;

   public:
    Var var;
    Shared<Gradient> grad;
    History<BackwardEntry> history;
    // Set on the output of a fused `nn::Linear::forward`: how to build the same product again.  `relu()` on such a
    // variable AS A TEMPORARY - the reference's spelling `lin.forward(x).relu()` (neuronika-nn/src/lib.rs:441-447; Rust's
    // `relu(self)` CONSUMES its operand, vardiff.rs:282-288) - answers the ONE Linear+ReLU node over the Linear's own operands
    // instead of a ReLU node over this output (graph-build peephole, `nn::set_relu_peephole`): the consumed pre-activation is
    // not observable in the reference either.  On a variable that is KEPT (`h = lin.forward(x); y = h.relu()` - Rust's
    // `h.clone().relu()`) `relu()` is the ReLU node over h: h is in y's history, its data and gradient are what the reference shows.
    Shared<const nn::LinearOrigin> linear_origin;

    static VarDiff leaf(Var var, Shared<Gradient> grad);                                        // vardiff.rs:48
    static VarDiff node(Var var, Shared<Gradient> grad, BackwardEntry op, History<BackwardEntry> h);  // :56
    const Shape& shape() const { return var.shape(); }
    DevicePtr device() const { return var.device(); }
    Shared<HipArray> data() const { return var.data; }

    void zero_grad() const;         // vardiff.rs:100
    void forward() const;           // vardiff.rs:106-116
    void backward(float seed, BackwardHook* hook = nullptr) const;  // vardiff.rs:125-141
    // The same pass seeded with an upstream gradient TENSOR (root gradient = `seed`, same shape) instead of a
    // scalar fill: what an enclosing graph would hand to this sub-graph's root.  Lets a benchmark time a module's
    // own backward nodes without `(y * G).sum()` scaffolding.  The seed's buffer stands in for the root gradient while
    // the tape runs (no copy); afterwards the root gradient is its own buffer again, holding what it held before.
    void backward_from(const Var& seed, BackwardHook* hook = nullptr) const;
    void no_grad() const;           // vardiff.rs:145
    void with_grad() const;         // vardiff.rs:157
    float item() const { return var.item(); }
    std::vector<float> to_vec() const { return var.to_vec(); }
    std::vector<float> grad_to_vec() const { return grad->borrow().to_vec(); }

    VarDiff sum() const;
    VarDiff mean() const;
    VarDiff relu() const&;  // the ReLU node over this (kept) variable
    VarDiff relu() &&;      // `relu(self)` on a temporary: may fold into the Linear that produced it (see `linear_origin`)
    VarDiff neg() const;
    VarDiff pow(int exp) const;
    VarDiff sqrt() const;
    VarDiff leaky_relu() const;
    VarDiff softplus() const;
    VarDiff sigmoid() const;
    VarDiff tanh() const;
    VarDiff ln() const;
    VarDiff exp() const;
    // ONE forward node and ONE backward entry each, which keeps the INPUT and recomputes from it; a gradient's first writer assigns,
    // a later one accumulates
    VarDiff gelu(bool tanh_approx = false) const;
    VarDiff silu() const;
    VarDiff glu(Activation gate = Activation::Sigmoid) const;
    // one forward and one backward node; the rotation is orthogonal, so the backward (the same kernel with the sign of the sine
    // flipped) holds the table and the geometry only
    VarDiff rope(const nn::RotaryEmbedding& rotary, int batch, int heads) const;
    // `Var::repeat_kv` with one backward entry: the gradients of the copies summed in ascending copy order (nk_repeat_kv_bwd); the
    // first writer of the input's gradient takes the assign form.
    VarDiff repeat_kv(int groups, int head_dim) const;
    VarDiff unsqueeze(int axis) const;
    // the differentiable max-pool node owns the int32 offsets of the selected elements (4 bytes per output)
    VarDiff max_pool(const std::vector<int>& kernel, const std::vector<int>& stride, const std::vector<int>& padding) const;
    VarDiff avg_pool(const std::vector<int>& kernel, const std::vector<int>& stride, const std::vector<int>& padding,
                     bool count_include_pad = true) const;
    VarDiff global_avg_pool() const;
    VarDiff upsample(const std::vector<int>& out_size, const std::string& mode = "nearest", bool align_corners = false) const;
    VarDiff flatten() const;
    VarDiff softmax(int axis) const;
    VarDiff log_softmax(int axis) const;
    VarDiff t() const;
    // one forward and ONE backward entry; gradients flow to self and, independently, to gamma and beta where differentiable
    VarDiff layer_norm(const VarDiff& gamma, const VarDiff& beta, double eps = 1e-5) const;
    VarDiff layer_norm(const Var& gamma, const Var& beta, double eps = 1e-5) const;
    VarDiff layer_norm(const Shape& normalized_shape, double eps = 1e-5) const;
    // one forward and ONE backward entry; gradients flow to self and, independently, to gamma where differentiable
    VarDiff rms_norm(const VarDiff& gamma, double eps = 1e-6) const;
    VarDiff rms_norm(const Var& gamma, double eps = 1e-6) const;
    VarDiff rms_norm(const Shape& normalized_shape, double eps = 1e-6) const;
    // one forward and ONE backward entry; gradients flow to self and, independently, to gamma and beta where differentiable
    VarDiff group_norm(int num_groups, const VarDiff& gamma, const VarDiff& beta, double eps = 1e-5) const;
    VarDiff group_norm(int num_groups, const Var& gamma, const Var& beta, double eps = 1e-5) const;
    VarDiff group_norm(int num_groups, double eps = 1e-5) const;
    // Embedding (ours: the reference has none; semantics in neuronika_hip.h): self is the (V, D) table, `indices` holds ids as f32
    // (read as the NLL targets are) in any shape; the result has shape indices.shape + (D,).  Differentiable in the table only:
    // its gradient is the ordered sum per row, no atomics; rows selected through `padding_idx` (< 0: none) receive no gradient.
    VarDiff embedding(const Var& indices, long padding_idx = -1) const;
    // one forward and ONE backward entry; gradients flow to self and, independently, to gamma and beta where differentiable
    VarDiff batch_norm(const VarDiff& gamma, const VarDiff& beta, const Var* running_mean, const Var* running_var, double momentum, double eps,
                       Shared<bool> status) const;
    VarDiff batch_norm(const Var* gamma, const Var* beta, const Var* running_mean, const Var* running_var, double momentum, double eps,
                       Shared<bool> status) const;
    VarDiff dropout(double p, Shared<bool> status) const;
    std::vector<VarDiff> chunks(const Shape& chunk_size) const;
    VarDiff cat(const std::vector<VarDiff>& vars, int axis) const;
    VarDiff stack(const std::vector<VarDiff>& vars, int axis) const;
    VarDiff mse(const Var& target, Reduction reduction) const;
    VarDiff mae(const Var& target, Reduction reduction) const;              // vardiff.rs:474
    VarDiff bce(const Var& target, Reduction reduction) const;              // vardiff.rs:525
    VarDiff bce_with_logits(const Var& target, Reduction reduction) const;  // vardiff.rs:554
    VarDiff kldiv(const Var& target, Reduction reduction) const;            // vardiff.rs:583
    VarDiff nll(const Var& target, Reduction reduction) const;              // vardiff.rs:725
    // ONE forward node (it owns the per-position lse) and ONE backward entry, which recomputes the softmax from the logits; the
    // first writer of the logits' gradient assigns (inactive rows written as zeros), a later one accumulates
    VarDiff cross_entropy(const Var& target, Reduction reduction, long ignore_index = -1, double label_smoothing = 0.0) const;
    VarDiff mv(const Var& rhs) const;
    VarDiff mv(const VarDiff& rhs) const;
    VarDiff vm(const Var& rhs) const;
    VarDiff vm(const VarDiff& rhs) const;
    VarDiff vv(const Var& rhs) const;
    VarDiff vv(const VarDiff& rhs) const;
    VarDiff pad(const std::vector<int>& padding, float value = 0.f) const;
    VarDiff pad(const std::vector<int>& padding, PaddingMode mode) const;
    VarDiff mm(const Var& rhs) const;
    VarDiff mm(const VarDiff& rhs) const;
    VarDiff mm_t(const Var& rhs) const;
    VarDiff mm_t(const VarDiff& rhs) const;
    VarDiff convolution(const Var& input, const std::vector<int>& stride, const std::vector<int>& dilation,
                        int groups) const;
    VarDiff convolution(const VarDiff& input, const std::vector<int>& stride, const std::vector<int>& dilation,
                        int groups) const;
    VarDiff split_heads(int B, int S, int H, int dh) const;
    VarDiff merge_heads(int B, int S, int H, int dh) const;
    VarDiff bmm(const VarDiff& rhs) const;
    VarDiff bmm_t(const VarDiff& rhs) const;
    VarDiff heads_scores(const VarDiff& keys, int B, int S, int H, int dh) const;
    VarDiff heads_context(const VarDiff& values, int B, int S, int H, int dh) const;
    VarDiff attention_probs(float scale, double p, Shared<bool> status, bool store_probs = false) const;
    VarDiff heads_attention(const VarDiff& keys, const VarDiff& values, int B, int S, int H, int dh, float scale, double p,
                            Shared<bool> status, bool causal = false, int window = 0, const nn::Segments* segments = nullptr) const;
};

// `Add/Sub/Mul/Div` with NumPy broadcasting, all four differentiability combinations
// (var.rs:859-1026, vardiff.rs:866-1069) and the f32 scalar forms (var.rs:746-838).
#define NK_DECLARE_BINARY(OP)                         \
    Var operator OP(const Var& l, const Var& r);      \
    VarDiff operator OP(const Var& l, const VarDiff& r);   \
    VarDiff operator OP(const VarDiff& l, const Var& r);   \
    VarDiff operator OP(const VarDiff& l, const VarDiff& r); \
    Var operator OP(const Var& l, float r);           \
    VarDiff operator OP(const VarDiff& l, float r);
NK_DECLARE_BINARY(+)
NK_DECLARE_BINARY(-)
NK_DECLARE_BINARY(*)
NK_DECLARE_BINARY(/)
#undef NK_DECLARE_BINARY

// leaf constructors (lib.rs:51-143)
Var from_host(DevicePtr dev, const Shape& shape, const float* host);  // `from_ndarray`
// lib.rs:160-240: `eye`, `linspace` (end inclusive), `logspace` (base^linspace, negative base -> negative values),
// `geomspace` (panics where the reference returns None: zero endpoint or endpoints of different sign), `range` (half open)
Var eye(DevicePtr dev, int n);
Var linspace(DevicePtr dev, float start, float end, int n);
Var logspace(DevicePtr dev, float base, float start, float end, int n);
Var geomspace(DevicePtr dev, float start, float end, int n);
Var range(DevicePtr dev, float start, float end, float step);
Var zeros(DevicePtr dev, const Shape& shape);
Var ones(DevicePtr dev, const Shape& shape);
Var full(DevicePtr dev, const Shape& shape, float value);
Var rand(DevicePtr dev, const Shape& shape, uint64_t seed);  // U[0,1) (host RNG, uploaded)

// ---------------------------------------------------------------------------------------------
// neuronika-nn
// ---------------------------------------------------------------------------------------------
// Restart the per-thread sequence of Philox keys handed to random nodes: the next Dropout / attention-probabilities
// node built on this thread uses key `seed`, the one after it seed + 0x632BE59BD9B4E019, ...
void manual_seed(uint64_t seed);

namespace nn {

// neuronika-nn/src/init.rs: parameter initialisers.  Values are produced on the host and uploaded (one-off work at
// model construction).  The random ones take an explicit seed (the reference draws from `thread_rng`).
namespace init {
float calculate_gain(const std::string& non_linearity);                 // init.rs:25-33
std::pair<float, float> calculate_fan_in_fan_out(const VarDiff& param);  // init.rs:45-64 (trailing extents are SUMMED there)
void constant(const VarDiff& param, float value);                        // :74
void zeros(const VarDiff& param);                                        // :83
void ones(const VarDiff& param);                                         // :92
void eye(const VarDiff& param);                                          // :104
void dirac(const VarDiff& param, int groups);                            // :131-170
void uniform(const VarDiff& param, float low, float high, uint64_t seed);            // :177
void normal(const VarDiff& param, float mean, float std, uint64_t seed);             // :195
void xavier_uniform(const VarDiff& param, float gain, uint64_t seed);                // :213
void xavier_normal(const VarDiff& param, float gain, uint64_t seed);                 // :236
}  // namespace init

// `Linear` neuronika-nn/src/lib.rs:406-448: weight (out,in), bias (out), U(-k,k), k = 1/sqrt(in)
struct Linear {
    VarDiff weight, bias;
    bool fused = true;  // bias added in the GEMM epilogue (one node); false: the reference's two nodes mm_t, +
    Linear(DevicePtr dev, int in_features, int out_features, uint64_t seed);
    Linear(VarDiff weight, VarDiff bias) : weight(std::move(weight)), bias(std::move(bias)) {}
    VarDiff forward(const Var& input) const;      // input.mm_t(W) + b
    VarDiff forward(const VarDiff& input) const;
    // `forward(input).relu()` as ONE node (ours; the reference composes the two): max(input.W^T + b, 0) from the GEMM
    // epilogue, the pre-activation never stored; in the backward pass the ReLU mask is applied by whichever GEMM produces
    // this node's output gradient (a following Linear's input-gradient GEMM), or in place when another kind of node does.
    // Same values and gradients as the two nodes, bit for bit; the one observable difference: in a pass where every writer
    // of the OUTPUT's gradient applied the mask while storing (a following Linear), the output's `grad()` holds
    // (y > 0) * dL/dy afterwards - the entries where y = 0 read 0.  (A root's gradient, and any gradient written by other
    // kinds of nodes, keeps dL/dy: the mask then goes into a scratch copy.)
    VarDiff forward_relu(const Var& input) const;
    VarDiff forward_relu(const VarDiff& input) const;
};
// What `VarDiff::relu()` needs to rebuild a fused Linear as Linear+ReLU (see `VarDiff::linear_origin`)
struct LinearOrigin {
    VarDiff weight, bias;
    Var input;
    bool differentiable_input = false;       // the input was a VarDiff: its gradient and tape follow
    Shared<Gradient> input_grad;
    History<BackwardEntry> input_history;
};
// The weight-only quantised image of one (out, in) weight (ours; format at nk_quant_linear_* in neuronika_hip.h): packed int8 / int4
// rows and their per-group f32 scales, both ordinary device arrays of opaque words.  Null arrays: no image.
struct QuantImage {
    Shared<HipArray> qweight, scales;
    int bits = 0, group = 0;
    explicit operator bool() const { return (bool)qweight; }
};
// Weight-only quantised Linear for inference (ours; the reference has no such layer): W8A32 / W4A32.  The constructor packs the
// weight of `lin` on the device and shares its bias array; the Linear is left as it is, and later updates of its weight do not reach
// the image.  forward(x): (rows, in_features) -> (rows, out_features) as ONE forward node on nk_quant_linear_fwd, without a
// gradient: a differentiable input enters through its data and forward tape.  dequantize(): the (out, in) values float(q) * s the
// node multiplies by.  It holds no parameters: the optimizers, dp::GradientSync and serde do not see it (serde of quantised layers is
// out of scope; keep the Linear, or the packer's output, to rebuild one).
// Panics: bits not 8 / 4, group not 32 / 64 / 128 / 0, in_features not a multiple of 32 and of the group, an input of another shape
// or device.
struct QuantLinear {
    Shared<HipArray> qweight, scales, bias;
    int in_features, out_features, bits, group;
    QuantLinear(const Linear& lin, int bits, int group = 0);
    Var forward(const Var& input) const;
    Var forward(const VarDiff& input) const;
    Var dequantize() const;
};
// Graph-build peephole `forward(x).relu()` -> the Linear+ReLU node (on by default, per thread; off: the ReLU node over the
// Linear's output, as the tests that pit the two graphs against each other bit for bit need it).  Returns the old setting.
bool set_relu_peephole(bool on);

// Layer normalisation over the trailing `normalized_shape` of the input (ours: the reference has no normalisation layer):
// y = (x - mean) / sqrt(var + eps) * weight + bias per row, biased variance.  weight = ones, bias = zeros, both of
// `normalized_shape`, ordinary leaves for the optimizers; without `elementwise_affine` there are no parameters (weight and bias
// stay empty) and y = xhat.
struct LayerNorm {
    VarDiff weight, bias;
    Shape normalized_shape;
    double eps = 1e-5;
    bool elementwise_affine = true;
    LayerNorm(DevicePtr dev, Shape normalized_shape, double eps = 1e-5, bool elementwise_affine = true);
    LayerNorm(VarDiff weight, VarDiff bias, double eps = 1e-5);  // parameters built elsewhere (e.g. deserialised)
    VarDiff forward(const Var& input) const;  // differentiable in the parameters: needs elementwise_affine
    VarDiff forward(const VarDiff& input) const;
};

// RMS normalisation over the trailing `normalized_shape` of the input (ours: the reference has no normalisation layer), the
// normalisation of LLaMA-style decoders: y = x / sqrt(mean(x^2) + eps) * weight per row, no centring and no bias.  weight = ones
// of `normalized_shape`, an ordinary leaf for the optimizers; without `elementwise_affine` there is no parameter (weight stays
// empty) and y = xhat.  The default eps is LLaMA's.
struct RMSNorm {
    VarDiff weight;
    Shape normalized_shape;
    double eps = 1e-6;
    bool elementwise_affine = true;
    RMSNorm(DevicePtr dev, Shape normalized_shape, double eps = 1e-6, bool elementwise_affine = true);
    RMSNorm(VarDiff weight, double eps = 1e-6);  // a parameter built elsewhere (e.g. deserialised)
    VarDiff forward(const Var& input) const;  // differentiable in the weight: needs elementwise_affine
    VarDiff forward(const VarDiff& input) const;
};

// Group normalisation (ours: the reference has no normalisation layer), torch's GroupNorm: the channels of an (N, C, spatial...)
// input are cut into `num_groups` groups and each (sample, group) is normalised over its channels and positions, then scaled and
// shifted per channel.  weight = ones, bias = zeros of shape (C): ordinary leaves for the optimizers; without `affine` there are no
// parameters.  It does not depend on the batch size, which is why it replaces BatchNorm at small per-device batches.
struct GroupNorm {
    VarDiff weight, bias;
    int num_groups, num_channels;
    double eps = 1e-5;
    bool affine = true;
    GroupNorm(DevicePtr dev, int num_groups, int num_channels, double eps = 1e-5, bool affine = true);
    GroupNorm(int num_groups, VarDiff weight, VarDiff bias, double eps = 1e-5);  // parameters built elsewhere (e.g. deserialised)
    VarDiff forward(const Var& input) const;  // differentiable in the parameters: needs affine
    VarDiff forward(const VarDiff& input) const;
   private:
    void check_input(const Shape& s) const;
};

// Instance normalisation, torch's InstanceNorm1d/2d/3d: group normalisation with one channel per group, each (sample, channel)
// plane normalised on its own.  No parameters by default (torch's default).  torch's track_running_stats is NOT built: the
// statistics are always the input's own, in training and in inference.
struct InstanceNormNd {
    VarDiff weight, bias;
    int num_features;
    double eps;
    bool affine;
    int nd;  // 1: (N, C, L); 2: (N, C, H, W); 3: (N, C, D, H, W)
    InstanceNormNd(int nd, DevicePtr dev, int num_features, double eps, bool affine);
    VarDiff forward(const Var& input) const;  // differentiable in the parameters: needs affine
    VarDiff forward(const VarDiff& input) const;
   private:
    void check_input(const Shape& s) const;
};
struct InstanceNorm1d : InstanceNormNd {
    InstanceNorm1d(DevicePtr dev, int num_features, double eps = 1e-5, bool affine = false) : InstanceNormNd(1, std::move(dev), num_features, eps, affine) {}
};
struct InstanceNorm2d : InstanceNormNd {
    InstanceNorm2d(DevicePtr dev, int num_features, double eps = 1e-5, bool affine = false) : InstanceNormNd(2, std::move(dev), num_features, eps, affine) {}
};
struct InstanceNorm3d : InstanceNormNd {
    InstanceNorm3d(DevicePtr dev, int num_features, double eps = 1e-5, bool affine = false) : InstanceNormNd(3, std::move(dev), num_features, eps, affine) {}
};

// Batch normalisation over (N, spatial...) per channel (ours: the reference has no normalisation layer), torch's BatchNorm1d/2d/3d:
// training normalises with the batch's mean and biased variance and moves the running statistics towards them by `momentum` (the
// running variance takes the unbiased estimate), inference normalises with the running statistics.  weight = ones, bias = zeros:
// ordinary leaves for the optimizers; running_mean = zeros, running_var = ones: plain buffers.  Without `affine` there are no
// parameters, without `track_running_stats` no buffers and the batch statistics serve in both modes.  Cumulative averaging and a
// batches-seen counter are not provided.
struct BatchNormNd {
    VarDiff weight, bias;
    Var running_mean, running_var;
    int num_features;
    double eps, momentum;
    bool affine, track_running_stats;
    int nd;  // 1: (N, C) or (N, C, L) inputs; 2: (N, C, H, W); 3: (N, C, D, H, W)
    Shared<bool> status;
    BatchNormNd(int nd, DevicePtr dev, int num_features, double eps, double momentum, bool affine, bool track_running_stats);
    void train() const { *status = true; }
    void eval() const { *status = false; }
    VarDiff forward(const Var& input) const;  // differentiable in the parameters: needs affine
    VarDiff forward(const VarDiff& input) const;
   private:
    void check_input(const Shape& s) const;
};
struct BatchNorm1d : BatchNormNd {
    BatchNorm1d(DevicePtr dev, int num_features, double eps = 1e-5, double momentum = 0.1, bool affine = true, bool track_running_stats = true)
        : BatchNormNd(1, std::move(dev), num_features, eps, momentum, affine, track_running_stats) {}
};
struct BatchNorm2d : BatchNormNd {
    BatchNorm2d(DevicePtr dev, int num_features, double eps = 1e-5, double momentum = 0.1, bool affine = true, bool track_running_stats = true)
        : BatchNormNd(2, std::move(dev), num_features, eps, momentum, affine, track_running_stats) {}
};
struct BatchNorm3d : BatchNormNd {
    BatchNorm3d(DevicePtr dev, int num_features, double eps = 1e-5, double momentum = 0.1, bool affine = true, bool track_running_stats = true)
        : BatchNormNd(3, std::move(dev), num_features, eps, momentum, affine, track_running_stats) {}
};

// Max / average pooling layers (ours: the reference has none), torch's MaxPool1d/2d/3d and AvgPool1d/2d/3d in floor mode with
// dilation 1: no parameters; an empty `stride` means stride = kernel_size, an empty `padding` zeros.
struct PoolNd {
    std::vector<int> kernel_size, stride, padding;
    bool average, count_include_pad;
    int nd;
    PoolNd(int nd, bool average, std::vector<int> kernel_size, std::vector<int> stride, std::vector<int> padding, bool count_include_pad);
    Var forward(const Var& input) const;
    VarDiff forward(const VarDiff& input) const;
   private:
    void check_input(const Shape& s) const;
};
// torch's nn.Upsample (ours: the reference has none): either `size` (one entry per spatial axis) or `scale_factor` (one value, or one
// per axis; out_i = floor(in_i * scale_i), then the index arithmetic sees in_i and out_i alone - torch's recompute_scale_factor=True),
// never both.  `mode` is checked against the input's rank at forward: "nearest" for any, "linear" / "bilinear" / "trilinear" for
// 1 / 2 / 3 spatial axes.  No parameters and no serde state.
struct Upsample {
    std::vector<int> size;
    std::vector<double> scale_factor;
    std::string mode;
    bool align_corners;
    Upsample(std::vector<int> size, std::vector<double> scale_factor, std::string mode = "nearest", bool align_corners = false);
    std::vector<int> output_size(const Shape& input) const;
    Var forward(const Var& input) const;
    VarDiff forward(const VarDiff& input) const;
};
struct MaxPool1d : PoolNd {
    MaxPool1d(int kernel_size, int stride = 0, int padding = 0)
        : PoolNd(1, false, {kernel_size}, stride ? std::vector<int>{stride} : std::vector<int>{}, {padding}, true) {}
};
struct MaxPool2d : PoolNd {
    MaxPool2d(std::vector<int> kernel_size, std::vector<int> stride = {}, std::vector<int> padding = {})
        : PoolNd(2, false, std::move(kernel_size), std::move(stride), std::move(padding), true) {}
};
struct MaxPool3d : PoolNd {
    MaxPool3d(std::vector<int> kernel_size, std::vector<int> stride = {}, std::vector<int> padding = {})
        : PoolNd(3, false, std::move(kernel_size), std::move(stride), std::move(padding), true) {}
};
struct AvgPool1d : PoolNd {
    AvgPool1d(int kernel_size, int stride = 0, int padding = 0, bool count_include_pad = true)
        : PoolNd(1, true, {kernel_size}, stride ? std::vector<int>{stride} : std::vector<int>{}, {padding}, count_include_pad) {}
};
struct AvgPool2d : PoolNd {
    AvgPool2d(std::vector<int> kernel_size, std::vector<int> stride = {}, std::vector<int> padding = {}, bool count_include_pad = true)
        : PoolNd(2, true, std::move(kernel_size), std::move(stride), std::move(padding), count_include_pad) {}
};
struct AvgPool3d : PoolNd {
    AvgPool3d(std::vector<int> kernel_size, std::vector<int> stride = {}, std::vector<int> padding = {}, bool count_include_pad = true)
        : PoolNd(3, true, std::move(kernel_size), std::move(stride), std::move(padding), count_include_pad) {}
};

// Embedding table (ours: the reference has no such layer): forward(indices) = the rows of `weight` (num_embeddings,
// embedding_dim) selected by the ids of `indices` (f32, any shape), shape indices.shape + (embedding_dim,).  weight ~ N(0, 1)
// (init::normal), the row `padding_idx` zeroed; that row receives no gradient, so it stays zero under the optimizers.  The
// weight is an ordinary leaf for the optimizers, dp::GradientSync and serde; two modules may share one (tied weights).
struct Embedding {
    VarDiff weight;
    size_t num_embeddings, embedding_dim;
    long padding_idx = -1;
    Embedding(DevicePtr dev, size_t num_embeddings, size_t embedding_dim, long padding_idx = -1, uint64_t seed = 0);
    Embedding(VarDiff weight, long padding_idx = -1);  // a table built elsewhere (deserialised, or shared with another module)
    VarDiff forward(const Var& indices) const;
};

// Token sampling on the device (ours: the reference has no generation loop; semantics at nk_sample_fwd in neuronika_hip.h): greedy at
// temperature 0, else temperature, top-k (0: off) and top-p (1: off) in that order and one Philox draw per row.  forward(logits,
// batch) takes (batch*T, V) logits and returns the (batch,) ids of the last position of every sample as f32 - the form
// Embedding::forward takes, so a generation loop never leaves the device.  The members are read when forward builds its node; every
// execution of a node's forward draws at (seed, *offset) and advances `offset`, the counter all nodes of one sampler share - the way
// the dropout node consumes its calls.  No parameters, no gradient.
struct Sampler {
    Sampler(DevicePtr dev, float temperature = 1.0f, int top_k = 0, float top_p = 1.0f, uint64_t seed = 0);
    DevicePtr dev;
    float temperature;
    int top_k;
    float top_p;
    uint64_t seed;
    Shared<uint64_t> offset;
    Var forward(const Var& logits, int batch) const;
    Var forward(const VarDiff& logits, int batch) const;  // enters through `.var`: the ids carry no gradient
};

// Activation modules (ours: the reference has none; `Var / VarDiff::gelu / silu / glu`).  No parameters.
struct GELU {
    bool approximate_tanh = false;
    explicit GELU(bool approximate_tanh = false) : approximate_tanh(approximate_tanh) {}
    Var forward(const Var& input) const;
    VarDiff forward(const VarDiff& input) const;
};
struct SiLU {
    Var forward(const Var& input) const;
    VarDiff forward(const VarDiff& input) const;
};
// forward(x) = x.glu(gate): the last axis (even) is halved
struct GLU {
    Activation gate = Activation::Sigmoid;
    explicit GLU(Activation gate = Activation::Sigmoid) : gate(gate) {}
    Var forward(const Var& input) const;
    VarDiff forward(const VarDiff& input) const;
};

// Cross entropy criterion (ours: the reference has no such layer): forward(logits, target) = logits.cross_entropy(target, reduction,
// ignore_index, label_smoothing).  No parameters.  `ignore_index` < 0: none (use it for padded tokens, with Embedding's padding_idx).
struct CrossEntropyLoss {
    Reduction reduction = Reduction::Mean;
    long ignore_index = -1;
    double label_smoothing = 0.0;
    explicit CrossEntropyLoss(Reduction reduction = Reduction::Mean, long ignore_index = -1, double label_smoothing = 0.0);
    Var forward(const Var& logits, const Var& target) const;
    VarDiff forward(const VarDiff& logits, const Var& target) const;
};

// `LSTMCell` neuronika-nn/src/lib.rs:453-541.  Weights (4H,in)/(4H,H), biases (4H), U(-k,k), k = 1/sqrt(H).
// `forward` keeps the reference's exact composition: state = (cell_state, hidden); gate chunks 0..3 get
// sigmoid, tanh, sigmoid, sigmoid (:528-533); returns (new_cell_state, new_hidden) (:534-537).
struct LSTMCell {
    VarDiff weight_ih, weight_hh, bias_ih, bias_hh;
    LSTMCell(DevicePtr dev, int input_size, int hidden_size, uint64_t seed);
    std::pair<VarDiff, VarDiff> forward(const std::pair<VarDiff, VarDiff>& state, const Var& input) const;
    std::pair<VarDiff, VarDiff> forward(const std::pair<VarDiff, VarDiff>& state, const VarDiff& input) const;
};

// `GRUCell` neuronika-nn/src/lib.rs:543-625.  Weights (3H,in)/(3H,H), biases (3H); forward :602-624.
struct GRUCell {
    VarDiff weight_ih, weight_hh, bias_ih, bias_hh;
    GRUCell(DevicePtr dev, int input_size, int hidden_size, uint64_t seed);
    VarDiff forward(const VarDiff& hidden, const Var& input) const;
    VarDiff forward(const VarDiff& hidden, const VarDiff& input) const;
};

// `Conv1d` / `Conv2d` / `Conv3d` struct/new neuronika-nn/src/lib.rs:630-722, 724-814, 816-916: weight
// (Cout, Cin/groups, k...), bias (Cout, 1...), U(-k,k) with k = sqrt(1/(Cin*prod(kernel))).  Their forward
// is `todo!()` in the reference snapshot (:716-721, :809-814, :908-914) and is defined here as
// pad(padding, padding_mode) -> convolution(stride, dilation, groups) -> + bias.
struct ConvNd {
    VarDiff weight, bias;
    std::vector<int> padding, stride, dilation;
    PaddingMode padding_mode;
    int groups = 1;
    bool fused = true;  // bias added in the convolution epilogue (one node); false: convolution node + Addition node
    // Zero padding folded into the forward and the kernel gradient where the library's kernels can read the unpadded input
    // (nk_conv_padding_folds: the Winograd geometries at sizes the rules give to those kernels): no Pad node, no padded copy
    // (C3: 110 MB and a 40 us kernel per step less); false: the padded copy as a forward-only node (what rounds 2 - 4 built)
    bool fold_padding = true;
    ConvNd(int nd, DevicePtr dev, int in_channels, int out_channels, std::vector<int> kernel, std::vector<int> padding,
           PaddingMode mode, std::vector<int> stride, std::vector<int> dilation, int groups, uint64_t seed);
    VarDiff forward(const Var& input) const;
    VarDiff forward(const VarDiff& input) const;
};
// Constructor argument order = the reference's `new` (neuronika-nn/src/lib.rs:671-679, 762-770, 857-865):
// (in_channels, out_channels, kernel_size, padding, padding_mode, stride, dilation); `seed` (ours, last) fixes the
// U(-k, k) initialisation.
struct Conv1d : ConvNd {
    Conv1d(DevicePtr dev, int in_channels, int out_channels, int kernel, int padding, PaddingMode mode, int stride,
           int dilation, uint64_t seed = 0)
        : ConvNd(1, std::move(dev), in_channels, out_channels, {kernel}, {padding}, mode, {stride}, {dilation}, 1, seed) {}
};
struct Conv2d : ConvNd {
    Conv2d(DevicePtr dev, int in_channels, int out_channels, std::vector<int> kernel, std::vector<int> padding,
           PaddingMode mode, std::vector<int> stride, std::vector<int> dilation, uint64_t seed = 0)
        : ConvNd(2, std::move(dev), in_channels, out_channels, std::move(kernel), std::move(padding), mode, std::move(stride),
                 std::move(dilation), 1, seed) {}
};
struct Conv3d : ConvNd {
    Conv3d(DevicePtr dev, int in_channels, int out_channels, std::vector<int> kernel, std::vector<int> padding,
           PaddingMode mode, std::vector<int> stride, std::vector<int> dilation, uint64_t seed = 0)
        : ConvNd(3, std::move(dev), in_channels, out_channels, std::move(kernel), std::move(padding), mode, std::move(stride),
                 std::move(dilation), 1, seed) {}
};
// `nn::GroupedConv1d / 2d / 3d`: named in the reference's module index (src/lib.rs:783-797,
// neuronika-nn/src/lib.rs:369-387) and in BASELINE.json's north_star; the structs themselves are absent from the
// reference snapshot (its grouped convolution lives at node level: `Convolution::convolution_with_groups`,
// node/convolution/mod.rs:125-144,256-294).  Same fields and argument order as ConvNd plus `groups` after `dilation`;
// weight (Cout, Cin / groups, k...), k = sqrt(1 / (Cin / groups * prod(kernel))).
struct GroupedConv1d : ConvNd {
    GroupedConv1d(DevicePtr dev, int in_channels, int out_channels, int kernel, int padding, PaddingMode mode, int stride,
                  int dilation, int groups, uint64_t seed = 0)
        : ConvNd(1, std::move(dev), in_channels, out_channels, {kernel}, {padding}, mode, {stride}, {dilation}, groups, seed) {}
};
struct GroupedConv2d : ConvNd {
    GroupedConv2d(DevicePtr dev, int in_channels, int out_channels, std::vector<int> kernel, std::vector<int> padding,
                  PaddingMode mode, std::vector<int> stride, std::vector<int> dilation, int groups, uint64_t seed = 0)
        : ConvNd(2, std::move(dev), in_channels, out_channels, std::move(kernel), std::move(padding), mode, std::move(stride),
                 std::move(dilation), groups, seed) {}
};
struct GroupedConv3d : ConvNd {
    GroupedConv3d(DevicePtr dev, int in_channels, int out_channels, std::vector<int> kernel, std::vector<int> padding,
                  PaddingMode mode, std::vector<int> stride, std::vector<int> dilation, int groups, uint64_t seed = 0)
        : ConvNd(3, std::move(dev), in_channels, out_channels, std::move(kernel), std::move(padding), mode, std::move(stride),
                 std::move(dilation), groups, seed) {}
};

// `ModelStatus`-style train/eval switch shared with the Dropout nodes (node/dropout/mod.rs:27).
struct Dropout {
    double p;
    Shared<bool> status;
    explicit Dropout(double p) : p(p), status(std::make_shared<bool>(true)) {}
    void train() const { *status = true; }
    void eval() const { *status = false; }
    VarDiff forward(const VarDiff& x) const { return x.dropout(p, status); }
};

// Rotary position embedding (ours: the reference has no position encoding; semantics at nk_rope_fwd in neuronika_hip.h).  Owns the
// (max_pos, rot/2, 2) table of (cos, sin) of p * base^(-2j/rot), made in f64 at construction; no parameters, nothing trainable.
// `rot` (even, 2 <= rot <= head_dim; 0 = head_dim) columns of every head are rotated, the others pass through; `interleaved`
// pairs (2j, 2j+1) (GPT-J / RoFormer) instead of (j, j + rot/2) (NeoX / LLaMA-HF).  Shared between the layers of a model:
// `MultiheadAttention::rope`, `Var / VarDiff::rope`.
struct RotaryEmbedding {
    RotaryEmbedding(DevicePtr dev, int head_dim, int max_pos, double base = 10000.0, int rot = 0, bool interleaved = false);
    int head_dim, max_pos, rot;
    double base;
    bool interleaved;
    Shared<HipArray> table;
};

// Packed sequences (ours; semantics at nk_attention_seg_fwd in neuronika_hip.h): several documents concatenated in one row of the
// batch.  doc_lens holds, per sample, the positive lengths of its documents in order, with sum <= S; a remainder forms one more
// document, the padding tail, whose targets the user masks with `CrossEntropyLoss::ignore_index`.  Holds two device arrays of
// batch*S int32 (in f32 storage, as the decode step's start positions travel) - lo[b][t], the start of t's document inside the
// sample, and pos[b][t] = t - lo[b][t], the position rope restarts at - their host copies, and max_len, the longest document.  Both
// are uploaded ONCE, at construction, by a synchronising upload: construction REFUSES stream capture (a panic before anything
// touches the stream - the capture stays valid - as nk_rope_table); the nodes built with it read nothing on the host and can be captured.  Shared between the layers of a model and the steps that use the same layout.
// Panics: batch or S not positive, doc_lens.size() != batch, a length <= 0, a sample's sum above S.
struct Segments {
    Segments(DevicePtr dev, int batch, int S, const std::vector<std::vector<int>>& doc_lens);
    int batch, S, max_len;
    Shared<HipArray> lo, pos;
    std::vector<int> lo_host, pos_host;
};

// The keys and values of one causal attention layer, kept on the device between the steps of incremental decoding (ours: the
// reference has no such thing; semantics at nk_kv_cache_append / nk_attention_decode_fwd in neuronika_hip.h).  Kc, Vc are
// (batch, heads, capacity, head_dim) - `heads` is the layer's kv_heads - head-major, allocated once and never initialised: nothing past a sample's length is read
// into a result.  The lengths live on the host; `MultiheadAttention::forward_step` advances them when it BUILDS its node.
//   reset()      every length back to 0 (the buffers are kept)
//   truncate(l)  every sample to a length no longer than its current one.  This is what makes ragged prompts work - prefill a
//                right-padded batch, then truncate each sample to its true prompt length: under the causal rule the padding never
//                influenced the real positions - and it gives roll-back.
//   rolling      (the second constructor's argument; false, and the first constructor: the object above, field for field) a ring for a sliding-window layer
//                (`MultiheadAttention::window`): position p lives at slot p % capacity, lens[b] grows past `capacity`, and
//                `high_water()[b]` is the largest length sample b has reached since the last reset() - the slots hold the positions
//                [high_water - capacity, high_water).  truncate(l) must leave the next window intact: it panics unless
//                max(0, l[b] - W) >= high_water[b] - capacity, with W the window of the layer that last stepped the cache (the cache
//                REMEMBERS it: forward_step records it (`remember_window`) when it builds its node; before any step W = capacity).  The ragged-prompt
//                recipe works whenever the prefill's T <= capacity: high_water = T then, and the right side is <= 0.
struct KvCache {
    KvCache(DevicePtr dev, int batch, int heads, int head_dim, int capacity);
    KvCache(DevicePtr dev, int batch, int heads, int head_dim, int capacity, bool rolling);
    int batch, heads, head_dim, capacity;
    bool rolling;
    const std::vector<int>& lens() const { return lens_; }
    const std::vector<int>& high_water() const { return high_; }
    void reset();  // rolling: clears the high-water marks too
    void truncate(const std::vector<int>& lens);
    // used by forward_step: the buffers, the scratch of nk_attention_decode_fwd (sized for T = 1 and `heads` query heads at
    // construction, regrown when a larger T or a grouped layer's larger query head count first arrives; a node keeps the one it was built with alive), and the lengths after a step of T rows
    Shared<HipArray> k, v;
    // window > 0: also at least nk_attention_decode_window_workspace(batch, T, query_heads, head_dim, window) floats - a window
    // that straddles one more chunk seam than the capacity has chunks needs a chunk more than the capacity-sized scratch.
    // workspace_floats(): the size of the scratch held now (a prefill the causal core takes asks for none and must not grow it).
    // remember_window(): forward_step records the layer's window with every step, for truncate()
    Shared<HipArray> workspace(int T, int query_heads, int window = 0);
    size_t workspace_floats() const { return ws_ ? ws_->len() : 0; }
    void remember_window(int window);
    void advance(int T);

   private:
    std::vector<int> lens_, high_;
    Shared<HipArray> ws_;
    int ws_T_ = 0, ws_H_ = 0, ws_W_ = 0;
    int window_ = 0;  // of the layer that last stepped the cache (0: none yet)
};

// The page table of a paged key / value cache (ours; layout at nk_attention_decode_paged_fwd in neuronika_hip.h): which of `num_pages`
// physical pages of `page` positions holds which positions of which of `max_seqs` sequences.  Pure host state, no device: sequence s
// has a length, a row of `max_pages` page ids (-1 where it owns nothing) and `behind`, the first position it still holds; every page
// has a reference count, and the pages nobody references are the free set.  Every operation that can fail panics BEFORE it changes
// any state: out of pages, max_pages exceeded, an id out of range, duplicate ids.
//   reserve(seqs, T)         grows every listed sequence by T positions, sequence by sequence in the order of `seqs`, taking the
//                            lowest-numbered free page each time.  A sequence whose last page is partial and shared (refcount > 1)
//                            first gets a page of its own there, and the pair (old, new) is returned as a copy to make before the
//                            append: a page with more than one owner is never written.
//   truncate(seq, len)       releases the pages wholly past `len`; panics for len > the length or len < behind(seq)
//   release(seq)             releases everything the sequence owns; length and behind back to 0
//   fork(src, dst)           dst must be empty: it shares every page of src by reference count and takes its length and behind
//   release_behind(seq, pos) releases the pages wholly below `pos` (<= the length) and sets their entries to -1: how a windowed
//                            layer bounds its memory.  behind(seq) becomes the first position of the first page kept
//   reset()                  back to the empty table
struct PageTable {
    PageTable(int num_pages, int page, int max_seqs, int max_pages);
    int num_pages, page, max_seqs, max_pages;
    const std::vector<int>& lens() const { return lens_; }
    std::vector<int> pages(int seq) const;  // the ids the sequence owns, in position order
    std::vector<int> row(int seq) const;    // max_pages ints
    const std::vector<int>& rows() const { return rows_; }  // (max_seqs, max_pages)
    int refcount(int page_id) const;
    std::vector<int> free_pages() const;  // ascending
    int behind(int seq) const;
    std::vector<std::pair<int, int>> reserve(const std::vector<int>& seqs, int T);
    void truncate(int seq, int len);
    void release(int seq);
    void fork(int src, int dst);
    void release_behind(int seq, int pos);
    void reset();

   private:
    void check_seq(int seq, const char* what) const;
    void unref(int page_id);
    std::vector<int> lens_, behind_, rows_, ref_;
    std::set<int> free_;
};

// A paged key / value cache: the two pools (num_pages, kv_heads, page, head_dim), allocated once and never initialised, a PageTable,
// and the decode scratch, regrown like KvCache::workspace.  The PageTable operations are forwarded.  As in KvCache, the elements of
// one pool must fit 31 bits (num_pages * kv_heads * page * head_dim <= INT_MAX).
struct PagedKvCache {
    PagedKvCache(DevicePtr dev, int num_pages, int page, int kv_heads, int head_dim, int max_seqs, int max_pages);
    int num_pages, page, heads, head_dim, max_seqs, max_pages;
    PageTable table;
    Shared<HipArray> k, v;
    const std::vector<int>& lens() const { return table.lens(); }
    std::vector<int> pages(int seq) const { return table.pages(seq); }
    std::vector<int> row(int seq) const { return table.row(seq); }
    int refcount(int page_id) const { return table.refcount(page_id); }
    std::vector<int> free_pages() const { return table.free_pages(); }
    int behind(int seq) const { return table.behind(seq); }
    std::vector<std::pair<int, int>> reserve(const std::vector<int>& seqs, int T) { return table.reserve(seqs, T); }
    void truncate(int seq, int len) { table.truncate(seq, len); }
    void release(int seq) { table.release(seq); }
    void fork(int src, int dst);  // the table's fork; the pages stay where they are
    void release_behind(int seq, int pos) { table.release_behind(seq, pos); }
    void reset() { table.reset(); }
    // at least nk_attention_decode_paged_workspace(batch, T, query_heads, head_dim, max_pages, page, window) floats
    Shared<HipArray> workspace(int batch, int T, int query_heads, int window);
    size_t workspace_floats() const { return ws_ ? ws_->len() : 0; }

   private:
    Shared<HipArray> ws_;
    size_t ws_n_ = 0;
};

// Multi-head attention composed from reference ops (the module does not exist in the reference;
// SURVEY.md 8a note): Q,K,V = x.mm_t(W)+b; per (b,h): P = dropout(softmax(Q.mm_t(K)*dh^-1/2, 1));
// O = P.mm(V); out = cat(O).mm_t(Wo)+bo.
struct MultiheadAttention {
    Linear q, k, v, o;
    int d_model, heads;
    // Grouped-query attention: `kv_heads` key / value heads (a divisor of `heads`; == heads: the module and the graphs of plain
    // multi-head attention, bit for bit), each shared by heads / kv_heads query heads.  k and v are (kv_heads*dh, d_model).  With
    // kv_heads < heads, forward() takes the unpacked branches below with K and V repeated in front of them (`VarDiff::repeat_kv`;
    // rope rotates kv_heads heads of K), forward_step() appends kv_heads heads to a cache built with kv_heads and attends through
    // nk_attention_decode_gqa_fwd, where the query heads of a group share one read of their keys and values.
    int kv_heads;
    Dropout drop;
    bool fused = true;  // scale + softmax + dropout as one node (false: three reference nodes)
    bool strided_heads = true;  // attention GEMMs read Q/K/V and write O in the projection layout (false: split/merge copies)
    bool fused_core = true;     // scores -> probabilities -> context as one node on the fused attention kernels (dh in {32, 64, 128}, any S)
    // The three projection weights (and biases, and their gradients) are views of ONE (3*d_model, d_model) allocation -
    // (d_model + 2*kv_heads*dh, d_model) with kv_heads < heads - rows [Wq; Wk; Wv]: with `packed_qkv` the projections run as one GEMM with N = 3*d_model, their input gradient as one GEMM
    // with K = 3*d_model, the weight gradients as one GEMM with M = 3*d_model, and the fused attention kernels read Q, K, V
    // as column blocks of the packed output (`nk_attention_qkv_*`).  q / k / v stay ordinary `Linear`s over those views
    // (optimizers, serde and the data-parallel exchange see three parameters as before).  false: three Linear nodes.
    bool packed_qkv = true;
    // Causal self-attention: query r of a sample attends to keys <= r of that sample - P = dropout(softmax(scores * scale + M)),
    // M[r][k] = 0 for k <= r and -inf above.  Read when forward() builds the graph, like the switches above, and honoured on every
    // path: the fused core runs its causal kernels (which skip the key tiles above the diagonal); the node-by-node paths add M, a
    // constant (S, S) leaf, on the broadcast Addition node.  Dropout draws keep their positions either way.
    bool causal = false;
    // Rotary position embedding of the queries and keys: null (the default) builds exactly the graph built without it.  Read when
    // forward() / forward_step() build their nodes, like `causal`, and honoured on every path, causal or not: the packed node rotates
    // Q|K in place in its (n, 3d) projection output (one launch, 2*heads heads, stride 3d) and applies the inverse to the first 2d
    // columns of its gradient in front of the three products that read it; the other paths rotate q.forward(x) and k.forward(x)
    // through `VarDiff::rope`.  forward_step rotates the new Q and K rows at lens[b] + t before the append: the cache holds ROTATED
    // keys.  Panics: rope->head_dim != d_model / heads, S > max_pos (forward), cache.capacity > max_pos (forward_step).
    Shared<RotaryEmbedding> rope;
    // Sliding-window attention (semantics at nk_attention_decode_window_fwd in neuronika_hip.h): query position i attends to the keys
    // max(0, i - window + 1) .. i.  0 (the default) = off: every path as without it, bit for bit, same launches.  Read when
    // forward() / forward_step() build their nodes, like `causal`; window > 0 with causal == false panics.
    //   forward()       S <= window: the band is the causal triangle - the paths above untouched, fused core included.  S > window:
    //                   where the fused core takes the head size (`Var::attention_core_supported`), the same ONE node - packed
    //                   (`nk_attention_qkv_band_*`) or strided, GQA behind `repeat_kv` - on the band kernels: they walk the key tiles
    //                   between the band's left edge and the diagonal only, O(S * window) work, and keep scores / dS / Pd in banded
    //                   scratch of O(S * window) floats that is allocated without a fill.  Other head sizes and fused_core = false:
    //                   the node-by-node paths (`heads_scores` / `bmm_t`) with the banded constant M[r][k] = 0 for r - window < k <= r,
    //                   -inf elsewhere, on the Addition node in place of the causal one.
    //   forward_step()  a fresh prefill with 2 <= T <= window keeps the causal core; every other step runs
    //                   nk_attention_decode_window_fwd over its T rows, on a linear cache or a rolling one (`KvCache::rolling`,
    //                   appended through nk_kv_cache_append_ring).  A step reads at most `window` keys per kv head whatever the length.
    //                   Panics: a rolling cache with window == 0; on a rolling cache T > capacity, or window + T - 1 > capacity for a
    //                   step the window kernel takes (the step's rows are appended before they are attended to and must not land on
    //                   a slot row 0 still reads: chunk the prompt into slices of at most capacity - window + 1 rows); a linear cache
    //                   overflowing, as without a window.  With rope on a rolling cache the positions keep growing: the guard is
    //                   lens[b] + T <= rope->max_pos instead of capacity <= max_pos.
    int window = 0;
    MultiheadAttention(DevicePtr dev, int d_model, int heads, double p, uint64_t seed);
    MultiheadAttention(DevicePtr dev, int d_model, int heads, int kv_heads, double p, uint64_t seed);
    // four Linear layers built elsewhere (e.g. deserialised): their weights are NOT packed, `packed_qkv` is off.  kv_heads 0 = heads;
    // k and v must be (kv_heads * d_model / heads, d_model)
    MultiheadAttention(Linear q, Linear k, Linear v, Linear o, int heads, double p, int kv_heads = 0);
    VarDiff forward(const VarDiff& x, int batch) const;  // x: (batch*seq, d_model)
    // Packed sequences: every token attends to its own document only - keys max(seg.lo, r - window + 1) .. r - and, with `rope`,
    // Q and K rows are rotated at seg.pos, the position INSIDE the document (nk_rope_* with B := batch*S, T := 1, start := pos).
    // One document per sample (seg.max_len >= S) is forward(x, batch): the same nodes, launches and bits.  Otherwise, where the
    // fused core takes the head size, ONE node on nk_attention_qkv_seg_* (packed) or nk_attention_seg_* (strided, GQA behind
    // `repeat_kv`) with span = min(max_len, window), on the band's scratch for that span allocated without a fill; other head
    // sizes and fused_core = false take the node-by-node paths with the per-sample constant M_b[r][k] = 0 for lo_eff <= k <= r, -inf
    // elsewhere (a (batch*heads, S, S) leaf).  forward_step() knows no segments.
    // Panics: causal == false; seg.batch / seg.S differ from the call's; seg.max_len > rope->max_pos.
    VarDiff forward(const VarDiff& x, int batch, const Segments& seg) const;
    // Incremental decoding: the causal forward, one slice of T = rows / batch positions at a time, in inference.  x holds the NEW
    // positions only, (batch*T, d_model); the result, (batch*T, d_model) without a gradient, equals rows lens[b] .. lens[b] + T - 1
    // of `forward` over each sample's whole prefix up to summation order.  ONE forward node: projections (the packed single GEMM
    // while the module is still packed), the append to `cache`, the attention, the output projection.  The node captures its
    // start positions when it is built (one upload of `batch` int32) and the cache's lengths advance right then, so running its
    // forward() again writes the same rows to the same places.  Attention part: every start 0, T >= 2 and a head size the fused
    // core takes -> the causal core in its inference form (no (T, T) tensor); otherwise the split-KV decode kernels over
    // (b, h, t), which also covers chunked prefill (T > 1 at start > 0).
    // With kv_heads < heads the cache is built with kv_heads as its head count; a fresh prefill repeats the step's K and V rows
    // into temporaries of the node for the causal core, every other step runs nk_attention_decode_gqa_fwd.
    // Panics: causal == false; dropout active (train mode and p > 0: call drop.eval() first); any lens[b] + T > capacity; a
    // batch / head size that differs from the cache's; cache.heads != kv_heads.
    Var forward_step(const Var& x, int batch, KvCache& cache) const;
    // The same node over a PAGED cache: the batch is seqs.size(), any subset of the cache's sequences in any order (continuous
    // batching); row b*T + t of x is position lens[seqs[b]] + t of sequence seqs[b].  Same preconditions (causal, dropout off) and
    // rope at lens + t.  When the node is built, `cache.reserve(seqs, T)` runs, then ONE upload of the starts, the seqs.size() *
    // max_pages table rows and the copy pairs reserve returned, if any.  forward() runs the page copies, then
    // nk_kv_pages_append, then the attention; running it again repeats the same writes.  A fresh prefill (T >= 2, every length 0, a
    // head size of the fused core, T <= window if windowed) keeps the causal core; every other step takes
    // nk_attention_decode_paged_fwd with the module's `window`.
    // Panics, all before any state changes: what reserve refuses (out of pages, max_pages, ids); a cache built for other kv heads /
    // head size; a sequence with behind > 0 stepped by a layer with window == 0, or whose window would reach below behind;
    // lens + T beyond rope's table.
    Var forward_step(const Var& x, const std::vector<int>& seqs, PagedKvCache& cache) const;
    // Weight-only quantised decoding (nn::QuantLinear's format): builds int8 / int4 images of the projections forward_step uses and
    // of `o` - ONE image of the packed [Wq; Wk; Wv] storage while the module is still packed and packed_qkv is on, three otherwise.
    // From then on both forward_step overloads project through nk_quant_linear_fwd; forward() for training is untouched and keeps
    // reading the f32 weights, which stay allocated.  The images are a snapshot: after an optimizer step, an assignment to q / k /
    // v / o or a change of packed_qkv, call quantize() again (forward_step panics when the form it needs has no image).  Never
    // called: null images, every launch and bit as before.  Panics: what QuantLinear refuses; d_model not a multiple of 32.
    void quantize(int bits, int group = 0);
    bool quantized() const { return (bool)qo_; }

   private:
    QuantImage qimg_[3], qo_;   // [0] alone: the packed storage's image; all three: q, k, v
    bool qpacked_ = false;
    VarDiff forward_impl(const VarDiff& x, int batch, const Segments* seg) const;
    bool still_packed() const;
    Shared<HipArray> wqkv_, bqkv_, gwqkv_, gbqkv_;  // packed storage (null when the layers were handed in)
};

}  // namespace nn

// ---------------------------------------------------------------------------------------------
// neuronika-variable/src/serde.rs:10-58 — (de)serialisation of leaves in ndarray's serde wire format
//   {"v":1,"dim":[d0,d1,...],"data":[row-major f32 values]}
// `Var`/`VarDiff` serialise their data (D2H copy); deserialising creates a leaf (`VarDiff`: a leaf with
// `requires_grad()`).  Modules serialise as objects of their parameters, like `#[derive(Serialize)]` on
// the reference structs (neuronika-nn/src/lib.rs:397-404: {"weight":..., "bias":...}).
// ---------------------------------------------------------------------------------------------
namespace serde {

struct Json {  // minimal JSON document model (object keys keep their order)
    enum Kind { Null, Bool, Number, String, Array, Object } kind = Null;
    bool b = false;
    std::string text;  // number literal or string value
    std::vector<Json> items;
    std::vector<std::pair<std::string, Json>> members;
    const Json& at(const std::string& key) const;
    bool has(const std::string& key) const;
};
Json parse(const std::string& text);

std::string to_json(const Var& v);
std::string to_json(const VarDiff& v);
Var var_from_json(DevicePtr dev, const Json& j);
Var var_from_json(DevicePtr dev, const std::string& text);
VarDiff vardiff_from_json(DevicePtr dev, const Json& j);
VarDiff vardiff_from_json(DevicePtr dev, const std::string& text);
std::string to_json(const nn::Linear& l);
nn::Linear linear_from_json(DevicePtr dev, const Json& j);
nn::Linear linear_from_json(DevicePtr dev, const std::string& text);
std::string to_json(const nn::LayerNorm& l);  // {"weight":..., "bias":...}; eps is not part of the wire format
nn::LayerNorm layer_norm_from_json(DevicePtr dev, const Json& j, double eps = 1e-5);
nn::LayerNorm layer_norm_from_json(DevicePtr dev, const std::string& text, double eps = 1e-5);
std::string to_json(const nn::GroupNorm& l);  // {"weight":..., "bias":...}; num_groups and eps are not part of the wire format
nn::GroupNorm group_norm_from_json(DevicePtr dev, const Json& j, int num_groups, double eps = 1e-5);
nn::GroupNorm group_norm_from_json(DevicePtr dev, const std::string& text, int num_groups, double eps = 1e-5);
std::string to_json(const nn::RMSNorm& l);  // {"weight":...}; eps is not part of the wire format
nn::RMSNorm rms_norm_from_json(DevicePtr dev, const Json& j, double eps = 1e-6);
nn::RMSNorm rms_norm_from_json(DevicePtr dev, const std::string& text, double eps = 1e-6);
std::string to_json(const nn::Embedding& e);  // {"weight":...}; padding_idx is not part of the wire format
nn::Embedding embedding_from_json(DevicePtr dev, const Json& j, long padding_idx = -1);
nn::Embedding embedding_from_json(DevicePtr dev, const std::string& text, long padding_idx = -1);

// {"weight":..., "bias":..., "running_mean":..., "running_var":...}; eps and momentum are not part of the wire format.  Loading
// replaces the four fields of an existing layer (any of BatchNorm1d/2d/3d) of the same num_features.
std::string to_json(const nn::BatchNormNd& l);
void batch_norm_load_json(nn::BatchNormNd& l, const Json& j);
void batch_norm_load_json(nn::BatchNormNd& l, const std::string& text);

}  // namespace serde

// ---------------------------------------------------------------------------------------------
// neuronika-optim: Optimizer / StochasticGD (optimizer.rs:33-95, sgd/mod.rs:186-236)
// ---------------------------------------------------------------------------------------------
namespace optim {

struct Penalty {  // penalty.rs:2-79
    float l1 = 0.f, l2 = 0.f;
};

// `Optimizer<T>` (optimizer.rs:33-95): register / step / zero_grad / get_lr / set_lr.  State
// buffers (momentum, moments) live on the device, zero-initialised like the reference's.
class Optimizer {
   public:
    virtual ~Optimizer() = default;
    void register_param(const VarDiff& p);  // `register`
    virtual void step();
    void zero_grad() const;
    float get_lr() const { return lr_; }
    void set_lr(float lr) { lr_ = lr; }
    const std::vector<VarDiff>& params() const { return params_; }
    // `optim::clip_grad_norm` over the registered parameters, whatever the optimizer.  The norm lands in a buffer the optimizer
    // keeps (allocated by the first call), so a later call allocates nothing and can be captured; the returned Var aliases that
    // buffer and holds the norm of the LATEST call.
    Var clip_grad_norm(float max_norm);

   protected:
    Optimizer(float lr, Penalty penalty, int nstate) : lr_(lr), penalty_(penalty), nstate_(nstate) {}
    virtual void optimize(const VarDiff& p, std::vector<Shared<HipArray>>& state, int step) = 0;
    float lr_;
    Penalty penalty_;

   protected:
    std::vector<VarDiff> params_;
    std::vector<std::vector<Shared<HipArray>>> state_;
    std::vector<int> steps_;

   private:
    int nstate_;
    Shared<HipArray> clip_out_;  // {total_norm, coef} of the latest clip_grad_norm
};

// Global-norm gradient clipping (ours; nk_clip_grad_norm_multi): every gradient of `params` is scaled by
// min(1, max_norm / (norm + 1e-6)), `norm` the L2 norm over ALL of them, summed in f64 on the device.  Returns a 0-d Var on the
// device that holds the norm before clipping; nothing synchronises with the host (`item()` is the caller's synchronisation).
// A parameter listed twice counts once; max_norm = +inf measures only.  The parameters must live on one device (a cross-device
// norm is not offered).  Under data parallelism call it after `dp::GradientSync::join()`: before that the buffers hold this
// rank's share, and every rank must clip the summed gradient by the same coefficient.
Var clip_grad_norm(const std::vector<VarDiff>& params, float max_norm);

class SGD : public Optimizer {  // sgd/mod.rs
   public:
    SGD(float lr, Penalty penalty = {}, float momentum = 0.f, float dampening = 0.f, bool nesterov = false);
    void step() override;  // every registered parameter of a device in ONE launch (nk_sgd_step_multi)

   private:
    void optimize(const VarDiff& p, std::vector<Shared<HipArray>>& state, int step) override;
    float momentum_, dampening_;
    bool nesterov_;
};

class Adam : public Optimizer {  // adam/mod.rs ; amsgrad/mod.rs when amsgrad = true
   public:
    Adam(float lr, float beta1 = 0.9f, float beta2 = 0.999f, float eps = 1e-8f, Penalty penalty = {}, bool amsgrad = false);

   private:
    void optimize(const VarDiff& p, std::vector<Shared<HipArray>>& state, int step) override;
    float beta1_, beta2_, eps_;
    bool amsgrad_;
};

// AdamW (ours: decoupled weight decay, w *= 1 - lr * weight_decay before the Adam update; no `Penalty` - the coupled L2 of
// `Adam` is rescaled by the Adam denominator and is a different rule).  weight_decay = 0 is `Adam` without a penalty.
class AdamW : public Optimizer {
   public:
    AdamW(float lr, float beta1 = 0.9f, float beta2 = 0.999f, float eps = 1e-8f, float weight_decay = 1e-2f, bool amsgrad = false);
    void step() override;  // every registered parameter of a device in one nk_adamw_step_multi call (32 parameters a launch)

   private:
    void optimize(const VarDiff& p, std::vector<Shared<HipArray>>& state, int step) override;
    float beta1_, beta2_, eps_, weight_decay_;
    bool amsgrad_;
};

class Adagrad : public Optimizer {  // adagrad/mod.rs
   public:
    Adagrad(float lr, float lr_decay = 0.f, float eps = 1e-10f, Penalty penalty = {});

   private:
    void optimize(const VarDiff& p, std::vector<Shared<HipArray>>& state, int step) override;
    float lr_decay_, eps_;
};

class RMSProp : public Optimizer {  // rmsprop/mod.rs
   public:
    RMSProp(float lr, float alpha = 0.99f, float eps = 1e-8f, float momentum = 0.f, bool centered = false, Penalty penalty = {});

   private:
    void optimize(const VarDiff& p, std::vector<Shared<HipArray>>& state, int step) override;
    float alpha_, eps_, momentum_;
    bool centered_;
};

// neuronika-optim/src/lr_scheduler/{mod,step_lr,multi_step_lr,exponential_lr,lambda_lr,multiplicative_lr}.rs:
// `step()` = prepare_step (last_lr <- current_lr, epoch += 1; mod.rs:51-59) then the policy, then `optimizer.set_lr`.
namespace lr_scheduler {

class LRScheduler {
   public:
    virtual ~LRScheduler() = default;
    void step();
    float get_last_lr() const { return last_lr_; }
    float get_current_lr() const { return current_lr_; }
    size_t get_current_epoch() const { return epoch_; }
    void set_current_epoch(size_t e) { epoch_ = e; }

   protected:
    explicit LRScheduler(Optimizer& opt) : opt_(opt), initial_lr_(opt.get_lr()), last_lr_(opt.get_lr()), current_lr_(opt.get_lr()) {}
    virtual bool update(float& lr) = 0;  // new lr for epoch_ (already incremented); false = unchanged
    Optimizer& opt_;
    float initial_lr_, last_lr_, current_lr_;
    size_t epoch_ = 0;
};
class StepLR : public LRScheduler {  // every `step_size` epochs: lr *= gamma  (step_lr/mod.rs:59-65)
   public:
    StepLR(Optimizer& opt, size_t step_size, float gamma) : LRScheduler(opt), step_size_(step_size), gamma_(gamma) {}
    void set_gamma(float g) { gamma_ = g; }

   private:
    bool update(float& lr) override;
    size_t step_size_;
    float gamma_;
};
class MultiStepLR : public LRScheduler {  // at each milestone: lr *= gamma  (multi_step_lr/mod.rs:56-67)
   public:
    MultiStepLR(Optimizer& opt, std::vector<size_t> milestones, float gamma) : LRScheduler(opt), milestones_(std::move(milestones)), gamma_(gamma) {}
    void set_milestones(std::vector<size_t> m) { milestones_ = std::move(m); }

   private:
    bool update(float& lr) override;
    std::vector<size_t> milestones_;
    float gamma_;
};
class ExponentialLR : public LRScheduler {  // every epoch: lr *= gamma  (exponential_lr/mod.rs:54-58)
   public:
    ExponentialLR(Optimizer& opt, float gamma) : LRScheduler(opt), gamma_(gamma) {}
    void set_gamma(float g) { gamma_ = g; }

   private:
    bool update(float& lr) override { lr = last_lr_ * gamma_; return true; }
    float gamma_;
};
class LambdaLR : public LRScheduler {  // lr = initial_lr * f(epoch)  (lambda_lr/mod.rs:56-61)
   public:
    LambdaLR(Optimizer& opt, std::function<float(size_t)> f) : LRScheduler(opt), f_(std::move(f)) {}

   private:
    bool update(float& lr) override { lr = initial_lr_ * f_(epoch_); return true; }
    std::function<float(size_t)> f_;
};
class MultiplicativeLR : public LRScheduler {  // lr = last_lr * f(epoch)  (multiplicative_lr/mod.rs:54-59)
   public:
    MultiplicativeLR(Optimizer& opt, std::function<float(size_t)> f) : LRScheduler(opt), f_(std::move(f)) {}

   private:
    bool update(float& lr) override { lr = last_lr_ * f_(epoch_); return true; }
    std::function<float(size_t)> f_;
};

}  // namespace lr_scheduler

}  // namespace optim

// ---------------------------------------------------------------------------------------------
// data-parallel gradient exchange (net-new): RCCL sum all-reduce of the registered parameters'
// gradient buffers on the side stream, bucketed in reverse registration order so a bucket can
// start as soon as backward has produced it.
// ---------------------------------------------------------------------------------------------
namespace dp {

class Communicator {
   public:
    static std::string unique_id();  // 128 raw bytes, create on rank 0
    Communicator(DevicePtr dev, int nranks, int rank, const std::string& id);
    // `nranks` virtual ranks holding this rank's values (nk_comm_init_replicas): sum all-reduce = multiply by nranks
    // (channels, gbps: the paced stand-in of benchmarks/overlap_projection.py; 0, 0: an unthrottled streaming pass)
    static std::shared_ptr<Communicator> replicas(DevicePtr dev, int nranks, int channels = 0, double gbps = 0.0);
    ~Communicator();
    int rank() const { return rank_; }
    int size() const { return size_; }
    nk_comm* raw() const { return h_; }
    DevicePtr device() const { return dev_; }

   private:
    Communicator(DevicePtr dev, int nranks, int channels, double gbps);
    DevicePtr dev_;
    nk_comm* h_ = nullptr;
    int rank_, size_;
};

// Overlapped exchange: pass to `loss.backward(1/world, &sync)`; each registered parameter's
// gradient is all-reduced (sum) on the side stream as soon as the last backward node writing it
// has been issued (reverse layer order), while the remaining backward GEMMs keep the compute
// stream busy.  Gradients below `small_elems` (biases: latency-bound) are collected and sent as
// ONE RCCL group as soon as the last of them is final.  `join()` makes the compute stream wait
// for the exchange (no host sync).  Every rank must run the same tape: the order of the
// collectives is the order in which backward finalises the gradients.
class GradientSync : public BackwardHook {
   public:
    GradientSync(std::shared_ptr<Communicator> comm, const std::vector<VarDiff>& params, size_t small_elems = 65536);
    ~GradientSync() override;
    void grad_ready(const Gradient* g) override;
    bool wants_parts(const Gradient* g) const override;
    void grad_part_ready(const Gradient* g, size_t offset, size_t count) override;
    void join();
    size_t bytes_per_step() const { return bytes_; }
    // run the exchange even with a single rank (RCCL then copies in place): lets one GPU exercise every code path
    void set_force_exchange(bool on) { force_ = on; }
    size_t exchanges_issued() const { return issued_; }  // collective launches so far (a group counts once)
    size_t elements_exchanged() const { return elems_; }
    // Which weight gradients are handed over in row blocks (two launches of the weight-gradient GEMM instead of one):
    //   All       every large gradient (rounds 1 - 2);
    //   LastOnly  only the large gradient that became final LAST in the previous backward pass - the one whose exchange is
    //             exposed behind the pass; the others have the rest of backward to hide behind and keep the single GEMM
    //             launch (a split weight-gradient GEMM pays its prologue / drain twice: profiles/r03_overlap_projection.md);
    //   None      never.
    // Default LastOnly; `set_parts` overrides (measurement aid).  The first pass of LastOnly splits nothing.
    enum class Parts { All, LastOnly, None };
    void set_parts(Parts p) { parts_ = p; }
    // How many of the GPU's resident-block slots the exchange occupies while it runs: RCCL's channel workgroups (one slot
    // each; cap them with NCCL_MAX_NCHANNELS and pass the same number).  From the first large gradient handed over until
    // `join()` the device handle is told (nk_device_set_busy_slots), and the backward GEMMs issued in between plan their last
    // round of tiles around the missing slots (sgemm_tail_kernel) instead of leaving a ragged one - 10 - 15 % per 4096^3 GEMM
    // otherwise (profiles/r04_gemm_under_load.md, profiles/r05_gemm_under_load.md).  0 (default): the GEMMs assume an idle chip.
    void set_busy_slots(int n) { busy_slots_ = n < 0 ? 0 : n; }
    int busy_slots() const { return busy_slots_; }

   private:
    void flush_small();
    std::shared_ptr<Communicator> comm_;
    std::unordered_map<const Gradient*, Shared<Gradient>> params_;
    std::unordered_map<const Gradient*, size_t> parts_done_;  // elements already handed over piecewise this pass
    std::vector<const Gradient*> small_pending_;               // small gradients that are final, not yet sent
    std::vector<nk_event*> events_;
    size_t next_event_ = 0;
    size_t bytes_ = 0;
    size_t issued_ = 0;
    size_t elems_ = 0;
    size_t small_elems_;
    size_t n_small_ = 0;
    bool force_ = false;
    int busy_slots_ = 0;
    bool busy_told_ = false;                      // the device handle currently carries busy_slots_
    Parts parts_ = Parts::LastOnly;
    const Gradient* last_large_ = nullptr;       // large gradient handed over last in the current pass
    const Gradient* split_next_ = nullptr;       // ... in the previous pass: the one LastOnly splits
    bool active() const { return comm_->size() > 1 || force_; }
};

// Non-overlapped form: all-reduce every gradient after backward has been issued.
void all_reduce_gradients(const Communicator& comm, const std::vector<VarDiff>& params);

}  // namespace dp

}  // namespace neuronika

"""`optim::AdamW`, `optim::clip_grad_norm` and `Optimizer::clip_grad_norm` through the tape, as whole trajectories against
tests/adamw_oracle.py: after EVERY step each parameter and its gradient buffer (after the clip) is compared with the f64 run of the
same gradients inside

    max|dev - w64| <= CPU_FACTOR * max|w32 - w64| + ELEMENTWISE_ATOL + ELEMENTWISE_RTOL * max|w64|      (tests/tolerance.py)

and the norm the clip returns with the f64 norm at ELEMENTWISE_RTOL.  tests/test_oracle_adamw.py shows that coupled, dropped or
unscaled decay, a dropped or per-parameter clip, a twice-counted parameter and a stale step number are each at least 10 of these
bounds away.  Bit-identity is asserted only between two device runs (replay against eager, one training run against another)."""
import numpy as np
import pytest

import adamw_oracle as A
import optim_trajectory as T
from tolerance import ELEMENTWISE_RTOL

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def nk():
    import neuronika_amd
    return neuronika_amd.tape


@pytest.fixture(scope="module")
def tdev(nk):
    return nk.Device(0)


def build(nk, config):
    """The host optimizer and scheduler of a config: every argument crosses the binding by keyword."""
    cls = {"adamw": nk.optim.AdamW, "sgd": nk.optim.SGD}[config["kind"]]
    opt = cls(config["lr"], **config["args"])
    sched = getattr(nk.optim.lr_scheduler, config["sched"][0])(opt, *config["sched"][1]) if config["sched"] else None
    return opt, sched


def leaves(nk, tdev, arrays):
    return [nk.from_ndarray(tdev, a).requires_grad() for a in arrays]


class Lockstep:
    """One device optimizer and the f32 and f64 `A.Reference` of the same config, driven by the same calls; a config with a
    `max_norm` clips through `Optimizer.clip_grad_norm` before every step."""

    def __init__(self, nk, config, label):
        self.opt, self.sched = build(nk, config)
        self.refs = [A.Reference(config, f32), A.Reference(config, np.float64)]
        self.max_norm = config["max_norm"]
        self.label, self.params, self.worst, self.norms = label, [], 0.0, []

    def add(self, p, register=True):
        w = p.data()
        self.params.append((p, [(np.array(w, dtype=r.dtype), np.zeros(w.shape, r.dtype)) for r in self.refs]))
        if register:
            self.register(len(self.params) - 1)
        return len(self.params) - 1

    def register(self, k):
        p, arrays = self.params[k]
        self.opt.register(p)
        for r, (w, g) in zip(self.refs, arrays):
            r.register(w, g)

    def set_grad(self, k, g):
        p, arrays = self.params[k]
        p.set_grad(g)
        for _, buf in arrays:
            buf[...] = g

    def step(self):
        norm = None
        if self.max_norm is not None:
            norm = self.opt.clip_grad_norm(self.max_norm)
            assert tuple(norm.shape) == ()
        self.opt.step()
        for r in self.refs:
            r.step()
        if norm is not None:
            got, want = norm.item(), float(self.refs[1].norms[-1])
            self.norms.append(got)
            assert abs(got - want) <= ELEMENTWISE_RTOL * want, (self.label, got, want)
        if self.sched is not None:
            self.sched.step()
            for r in self.refs:
                r.scheduler_step()
            assert f32(self.opt.get_lr()) == self.refs[0].lr

    def compare(self, t):
        for k, (p, ((w32, g32), (w64, g64))) in enumerate(self.params):
            try:
                self.worst = max(self.worst, T.check(self.label, p.data(), w32, w64))
                T.check(self.label + "/grad", p.grad(), g32, g64)
            except AssertionError as e:
                raise AssertionError(f"{self.label}: step {t}, parameter {k} of shape {w32.shape}: {e}") from e

    def run(self, steps, first=1):
        for t in range(first, first + steps):
            for k, (p, arrays) in enumerate(self.params):
                self.set_grad(k, T.gradient(t, k, arrays[0][0].shape))
            self.step()
            self.compare(t)


@pytest.mark.parametrize("name", list(A.CONFIGS))
def test_zoo_trajectory(nk, tdev, name):
    """Every config over the zoo registered together, 64 steps, scheduler stepped after each optimizer step.  With max_norm = 20 the
    first 24 steps are clipped and the other 40 leave through the early exit."""
    ls = Lockstep(nk, A.CONFIGS[name], f"adamw_trajectory/{name}")
    for p in leaves(nk, tdev, T.zoo()):
        ls.add(p)
    ls.run(A.STEPS)
    print(f"{name}: worst err / bound over {A.STEPS} steps = {ls.worst:.3f}")
    if ls.max_norm is not None:
        assert sum(n > ls.max_norm for n in ls.norms) == A.CLIPPED_STEPS and ls.refs[0].clipped == A.CLIPPED_STEPS
        assert len(ls.norms) == A.STEPS


@pytest.mark.parametrize("name", list(A.CONFIGS))
def test_parameter_registered_twice(nk, tdev, name):
    """Two sequential updates per step, each registration with its own state and its own step count; the second one goes into a later
    launch.  The clip counts the parameter once."""
    ls = Lockstep(nk, A.CONFIGS[name], f"adamw_trajectory_twice/{name}")
    for p in leaves(nk, tdev, T.zoo()[:5]):
        ls.add(p)
    ls.register(3); ls.register(0)
    ls.run(A.STEPS)
    print(f"{name}: worst err / bound = {ls.worst:.3f}")


@pytest.mark.parametrize("name", [n for n, c in A.CONFIGS.items() if c["kind"] == "adamw"])
def test_parameter_registered_late_starts_at_step_one(nk, tdev, name):
    """The step number is per registration: a parameter registered after 7 steps gets the bias corrections of step 1 while its
    neighbours in the same launch are at step 8."""
    ls = Lockstep(nk, A.CONFIGS[name], f"adamw_trajectory_late/{name}")
    params = leaves(nk, tdev, T.zoo()[:6])
    for p in params[:4]:
        ls.add(p)
    ls.run(7)
    for p in params[4:]:
        ls.add(p)
    ls.run(A.STEPS - 7, first=8)
    assert [s["step"] for s in ls.refs[0].slots] == [A.STEPS] * 4 + [A.STEPS - 7] * 2


def test_clip_grad_norm_function(nk, tdev):
    """`optim.clip_grad_norm(params, max_norm)`: a 0-d Var on the device, a parameter listed twice counts once, +inf measures only"""
    params = leaves(nk, tdev, T.zoo())
    grads = [T.gradient(1, k, tuple(p.shape)) for k, p in enumerate(params)]
    for p, g in zip(params, grads):
        p.set_grad(g)
    g32, g64 = [g.copy() for g in grads], [g.astype(np.float64) for g in grads]
    want, _ = A.clip_grad_norm(g64, float("inf"))
    norm = nk.optim.clip_grad_norm(params + [params[3], params[0]], float("inf"))
    assert tuple(norm.shape) == () and abs(norm.item() - float(want)) <= ELEMENTWISE_RTOL * float(want)
    for p, g in zip(params, grads):
        assert np.array_equal(p.grad(), g)
    norm = nk.optim.clip_grad_norm(params + [params[3], params[0]], A.MAX_NORM)
    A.clip_grad_norm(g32, A.MAX_NORM); A.clip_grad_norm(g64, A.MAX_NORM)
    assert abs(norm.item() - float(want)) <= ELEMENTWISE_RTOL * float(want)
    for p, a, b in zip(params, g32, g64):
        T.check("clip_grad_norm_function/grad", p.grad(), a, b)
    with pytest.raises(RuntimeError, match="max_norm"):
        nk.optim.clip_grad_norm(params, 0.0)
    with pytest.raises(RuntimeError, match="no parameters"):
        nk.optim.clip_grad_norm([], 1.0)


def test_every_optimizer_clips(nk, tdev):
    for make in (lambda: nk.optim.Adam(0.01), lambda: nk.optim.Adagrad(0.01), lambda: nk.optim.RMSProp(0.01)):
        opt = make()
        params = leaves(nk, tdev, T.zoo()[:5])
        g64 = []
        for k, p in enumerate(params):
            opt.register(p)
            p.set_grad(T.gradient(1, k, tuple(p.shape)))
            g64.append(T.gradient(1, k, tuple(p.shape)).astype(np.float64))
        want, _ = A.clip_grad_norm(g64, 5.0)
        g32 = [g.astype(f32) for g in (T.gradient(1, k, tuple(p.shape)) for k, p in enumerate(params))]
        A.clip_grad_norm(g32, 5.0)
        got = opt.clip_grad_norm(5.0).item()
        assert abs(got - float(want)) <= ELEMENTWISE_RTOL * float(want)
        for p, a, b in zip(params, g32, g64):
            T.check("every_optimizer_clips/grad", p.grad(), a, b)


def test_captured_clip_and_sgd_replay_the_eager_bits(nk, tdev):
    """clip + SGD capture (nothing in them depends on the step count): replays equal eager steps bit for bit.  The gradient is
    uploaded once and stays: the first eager clip scales it to the bound, so the replays run the coefficient-near-1 and early-exit
    side of the scale kernel; a replay that clips hard is tests/test_gpu_adamw.py's capture test, through the C ABI."""
    config = A.CONFIGS["sgd_clip"]

    def make():
        opt, _ = build(nk, config)
        params = leaves(nk, tdev, T.zoo())
        for k, p in enumerate(params):
            opt.register(p)
            p.set_grad(T.gradient(1, k, tuple(p.shape)))
        return opt, params

    opt_e, eager = make()
    for _ in range(2 + 6):
        norm_e = opt_e.clip_grad_norm(config["max_norm"])
        opt_e.step()
    opt_g, replayed = make()
    for _ in range(2):                                    # warm: the norm buffer and the workspace exist, every gradient is materialised
        opt_g.clip_grad_norm(config["max_norm"])
        opt_g.step()
    tdev.graph_begin()
    norm_g = opt_g.clip_grad_norm(config["max_norm"])
    opt_g.step()
    graph = tdev.graph_end()                              # recorded, not run
    for _ in range(6):
        graph.launch()
    assert np.array_equal(np.float32(norm_e.item()).view(np.uint32), np.float32(norm_g.item()).view(np.uint32))
    start = T.zoo()
    for k, (a, b) in enumerate(zip(eager, replayed)):
        assert np.array_equal(a.data(), b.data()) and np.array_equal(a.grad(), b.grad()), k
        assert np.isfinite(a.data()).all() and not np.array_equal(a.data(), start[k])
    total = np.sqrt(sum(float((p.grad().astype(np.float64) ** 2).sum()) for p in replayed))
    assert abs(total - config["max_norm"]) < 1e-4 * config["max_norm"]


def test_adamw_refuses_capture_and_stays_on_schedule(nk, tdev):
    ls = Lockstep(nk, A.CONFIGS["adamw_decay_clip"], "adamw_trajectory_refused_capture")
    for p in leaves(nk, tdev, T.zoo()):
        ls.add(p)
    ls.run(5)
    for k, (p, arrays) in enumerate(ls.params):
        p.set_grad(T.gradient(6, k, arrays[0][0].shape))
    other = nk.rand(tdev, [8, 8], 3).relu()
    other.forward()
    tdev.graph_begin()
    other.forward()                                       # (something to capture)
    with pytest.raises(RuntimeError, match="captured"):
        ls.opt.step()
    graph = tdev.graph_end()
    del graph
    ls.run(19, first=6)
    print(f"refused capture: worst err / bound = {ls.worst:.3f}")


# ---- a toy decoder block, trained --------------------------------------------------------------------------------------------------
def decoder(nk, tdev):
    """Embedding -> LayerNorm -> causal self-attention (+ residual) -> LayerNorm -> Linear / GELU / Linear (+ residual) -> Linear ->
    cross-entropy against the next token"""
    B, S, d, V = 2, 64, 128, 50
    rng = np.random.default_rng(12)
    tokens = rng.integers(0, V, (B, S + 1))
    ids, tgt = tokens[:, :-1].reshape(-1).astype(f32), tokens[:, 1:].reshape(-1).astype(f32)
    emb = nk.nn.Embedding(tdev, V, d, seed=31)
    ln1, ln2 = nk.nn.LayerNorm(tdev, [d]), nk.nn.LayerNorm(tdev, [d])
    mha = nk.nn.MultiheadAttention(tdev, d, 2, 0.0, 32)
    mha.causal = True
    up, down, head = nk.nn.Linear(tdev, d, 4 * d, 33), nk.nn.Linear(tdev, 4 * d, d, 34), nk.nn.Linear(tdev, d, V, 35)
    x = emb.forward(nk.from_ndarray(tdev, ids))
    x = x + mha.forward(ln1.forward(x), B)
    x = x + down.forward(up.forward(ln2.forward(x)).gelu())
    loss = nk.nn.CrossEntropyLoss().forward(head.forward(x), nk.from_ndarray(tdev, tgt))
    params = [emb.weight, ln1.weight, ln1.bias, ln2.weight, ln2.bias]
    params += [getattr(getattr(mha, n), f) for n in "qkvo" for f in ("weight", "bias")]
    params += [l_.weight for l_ in (up, down, head)] + [l_.bias for l_ in (up, down, head)]
    return loss, params


def test_toy_decoder_trains_with_adamw_and_clipping(nk, tdev):
    """20 steps of AdamW + clip on a decoder block: two runs end with the same bits, every loss is finite, and the loss falls."""
    def train():
        loss, params = decoder(nk, tdev)
        opt = nk.optim.AdamW(3e-3, weight_decay=0.1)
        for p in params:
            opt.register(p)
        losses, norms = [], []
        for _ in range(20):
            loss.forward(); loss.no_grad(); loss.with_grad(); loss.backward(1.0)
            losses.append(loss.item())
            norms.append(opt.clip_grad_norm(1.0).item())
            opt.step()
            opt.zero_grad()
        return losses, norms, [p.data().copy() for p in params]

    losses, norms, end = train()
    losses_b, norms_b, end_b = train()
    print(f"toy decoder: loss {losses[0]:.4f} -> {losses[-1]:.4f}; gradient norm {norms[0]:.3f} -> {norms[-1]:.3f}")
    assert np.isfinite(losses).all() and np.isfinite(norms).all() and all(n > 0 for n in norms)
    assert losses == losses_b and norms == norms_b
    for k, (a, b) in enumerate(zip(end, end_b)):
        assert np.array_equal(a, b), k
    assert losses[-1] < losses[0] and np.mean(losses[-5:]) < np.mean(losses[:5])

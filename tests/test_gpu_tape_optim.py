"""The host optimizer layer (`optim::SGD / Adam / Adagrad / RMSProp`, `lr_scheduler`) through the tape, as whole trajectories
against tests/optim_trajectory.py: after EVERY step each parameter, and its gradient buffer after the in-place penalty, is
compared with the f64 run of the same gradients inside

    max|dev - w64| <= CPU_FACTOR * max|w32 - w64| + ELEMENTWISE_ATOL + ELEMENTWISE_RTOL * max|w64|      (tests/tolerance.py)

tests/test_oracle_optim_trajectory.py shows that a step number one ahead, a stale rate, a dropped penalty, a default in place of
an argument, shared state or a missed second registration are each at least 10 of these bounds away.  Bit-identity is asserted
only between two device runs (blind against observed, replay against eager, packed against unpacked)."""
import numpy as np
import pytest

import optim_trajectory as T

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
    cls = {"sgd": nk.optim.SGD, "adam": nk.optim.Adam, "adagrad": nk.optim.Adagrad, "rmsprop": nk.optim.RMSProp}[config["kind"]]
    opt = cls(config["lr"], **config["args"])
    sched = getattr(nk.optim.lr_scheduler, config["sched"][0])(opt, *config["sched"][1]) if config["sched"] else None
    return opt, sched


def leaves(nk, tdev, arrays):
    return [nk.from_ndarray(tdev, a).requires_grad() for a in arrays]


class Lockstep:
    """One device optimizer and the f32 and f64 `T.Reference` of the same config, driven by the same calls."""

    def __init__(self, nk, config, label):
        self.opt, self.sched = build(nk, config)
        self.refs = [T.Reference(config, f32), T.Reference(config, np.float64)]
        self.label, self.params, self.worst = label, [], 0.0

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

    def step(self, scheduler=True):
        self.opt.step()
        for r in self.refs:
            r.step()
        if scheduler and self.sched is not None:
            self.sched.step()
            for r in self.refs:
                r.scheduler_step()
            assert f32(self.opt.get_lr()) == self.refs[0].lr

    def zero_grad(self):
        self.opt.zero_grad()
        for _, arrays in self.params:
            for _, g in arrays:
                g[...] = 0

    def compare(self, t, grads=True):
        for k, (p, ((w32, g32), (w64, g64))) in enumerate(self.params):
            try:
                self.worst = max(self.worst, T.check(self.label, p.data(), w32, w64))
                if grads:
                    T.check(self.label + "/grad", p.grad(), g32, g64)
            except AssertionError as e:
                raise AssertionError(f"{self.label}: step {t}, parameter {k} of shape {w32.shape}: {e}") from e

    def run(self, steps, first=1, grads=True):
        for t in range(first, first + steps):
            for k, (p, arrays) in enumerate(self.params):
                self.set_grad(k, T.gradient(t, k, arrays[0][0].shape))
            self.step()
            self.compare(t, grads)


# ---- a. injected gradients over the zoo --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(T.CONFIGS))
def test_zoo_trajectory(nk, tdev, name):
    """Every config over the zoo registered together (11 parameters: an SGD step is two launches), 64 steps, scheduler stepped
    after each optimizer step; zero_grad afterwards leaves zeros."""
    ls = Lockstep(nk, T.CONFIGS[name], f"optim_trajectory/{name}")
    params = leaves(nk, tdev, T.zoo())
    for p in params:
        ls.add(p)
    ls.run(T.STEPS)
    print(f"{name}: worst err / bound over {T.STEPS} steps = {ls.worst:.3f}")
    ls.opt.zero_grad()
    for p in params:
        assert not p.grad().any()


# ---- b. packed views and module parameters ---------------------------------------------------------------------------------------------
def module_parameters(nk, tdev):
    mha = nk.nn.MultiheadAttention(tdev, 128, 2, 0.0, 5)             # q / k / v weights, biases and their gradients: views of one allocation
    small = nk.nn.MultiheadAttention(tdev, 6, 3, 0.0, 6)             # d_model % 4 != 0: three ordinary layers
    ln = nk.nn.LayerNorm(tdev, [40])
    bn = nk.nn.BatchNorm2d(tdev, 5)
    emb = nk.nn.Embedding(tdev, 50, 12, padding_idx=3, seed=4)
    conv = nk.nn.Conv2d(tdev, 3, 4, [3, 3], [1, 1], nk.PaddingMode.zero(), [1, 1], [1, 1], 9)
    params = [getattr(getattr(m, n), f) for m in (mha, small) for n in "qkvo" for f in ("weight", "bias")]
    params += [ln.weight, ln.bias, bn.weight, bn.bias, emb.weight, conv.weight, conv.bias]
    return mha, params


@pytest.mark.parametrize("name", list(T.CONFIGS))
def test_module_parameter_trajectory(nk, tdev, name):
    """The same drive over the parameters of real modules.  Afterwards the packed storage holds exactly what the views say: the
    attention module gives the same bits through its packed projection and through the three Linear nodes over the views."""
    mha, params = module_parameters(nk, tdev)
    before = [p.data().copy() for p in params]
    ls = Lockstep(nk, T.CONFIGS[name], f"optim_trajectory_modules/{name}")
    for p in params:
        ls.add(p)
    ls.run(T.STEPS)
    print(f"{name}: worst err / bound over {T.STEPS} steps = {ls.worst:.3f}")
    for p, w0 in zip(params, before):
        assert not np.array_equal(p.data(), w0)
    B, S = 2, 128
    x = np.random.default_rng(1).standard_normal((B * S, 128)).astype(f32)
    outs = []
    for packed in (True, False):
        mha.packed_qkv = packed
        y = mha.forward(nk.from_ndarray(tdev, x).requires_grad(), B)
        assert y.history_len() == (2 if packed else 5)
        y.forward()
        outs.append(y.data())
    assert np.isfinite(outs[0]).all() and np.abs(outs[0]).max() > 0 and np.array_equal(outs[0], outs[1])


# ---- c. live loop --------------------------------------------------------------------------------------------------------------------
LIVE_CONFIGS = {
    "adam_steplr": dict(kind="adam", lr=0.01, args=dict(), sched=("StepLR", (8, 0.5))),
    "sgd_nesterov_l2": dict(kind="sgd", lr=0.02, args=dict(momentum=0.9, nesterov=True, l2=1e-3), sched=None),
}
LIVE_STEPS = 32


def mlp(nk, tdev):
    """C1's shape, spelled as the reference spells it: the ReLU peephole and the fused bias are in play."""
    lins = [nk.nn.Linear(tdev, 3, 5, 1), nk.nn.Linear(tdev, 5, 5, 2), nk.nn.Linear(tdev, 5, 1, 3)]
    X, Tg = nk.rand(tdev, [64, 3], 7), nk.rand(tdev, [64, 1], 8)
    loss = lins[2].forward(lins[1].forward(lins[0].forward(X).relu()).relu()).mse(Tg, nk.Reduction.Mean)
    return loss, [p for l in lins for p in (l.weight, l.bias)]


def attention_model(nk, tdev):
    B, S, d = 2, 64, 128
    mha = nk.nn.MultiheadAttention(tdev, d, 2, 0.0, 11)
    head = nk.nn.Linear(tdev, d, 4, 12)
    rng = np.random.default_rng(3)
    X = nk.from_ndarray(tdev, rng.standard_normal((B * S, d)).astype(f32)).requires_grad()
    Tg = nk.from_ndarray(tdev, rng.standard_normal((B * S, 4)).astype(f32))
    loss = head.forward(mha.forward(X, B)).mse(Tg, nk.Reduction.Mean)
    return loss, [getattr(getattr(mha, n), f) for n in "qkvo" for f in ("weight", "bias")] + [head.weight, head.bias]


@pytest.mark.parametrize("model", ["mlp", "attention"])
@pytest.mark.parametrize("name", list(LIVE_CONFIGS))
def test_live_loop(nk, tdev, model, name):
    """forward / backward / step / scheduler / zero_grad for 32 steps on two identical copies.  One is stepped blind.  On the other
    the gradients are read after zero_grad (which materialises the pending lazy zero) and before each step, and fed to the
    reference: it stays inside the bound, and the blind copy ends with the same bits."""
    config = LIVE_CONFIGS[name]
    make = mlp if model == "mlp" else attention_model
    label = f"optim_trajectory_live/{model}/{name}"

    def loop(observe):
        loss, params = make(nk, tdev)
        opt, sched = build(nk, config)
        for p in params:
            opt.register(p)
        init = [p.data().copy() for p in params]
        grads, datas, losses = [], [], []
        for _ in range(LIVE_STEPS):
            loss.forward(); loss.no_grad(); loss.with_grad(); loss.backward(1.0)
            if observe:
                grads.append([p.grad().copy() for p in params])
            opt.step()
            if sched is not None:
                sched.step()
            if observe:
                datas.append(([p.data().copy() for p in params], [p.grad().copy() for p in params]))
                losses.append(loss.item())
            opt.zero_grad()
            if observe:
                for p in params:
                    assert not p.grad().any()
        return init, grads, datas, losses, [p.data().copy() for p in params]

    init, grads, datas, losses, end_observed = loop(True)
    init_b, _, _, _, end_blind = loop(False)
    for a, b in zip(init, init_b):
        assert np.array_equal(a, b)
    W32, G32 = T.reference(config, f32, LIVE_STEPS, grads=grads, init=init)
    W64, G64 = T.reference(config, np.float64, LIVE_STEPS, grads=grads, init=init)
    worst = 0.0
    for t in range(LIVE_STEPS):
        for i in range(len(init)):
            worst = max(worst, T.check(label, datas[t][0][i], W32[t][i], W64[t][i]))
            T.check(label + "/grad", datas[t][1][i], G32[t][i], G64[t][i])
    print(f"{label}: worst err / bound = {worst:.3f}; loss {losses[0]:.4g} -> {losses[-1]:.4g}")
    assert np.isfinite(losses).all() and any(np.abs(g).max() > 0 for g in grads[-1])
    for i, (a, b) in enumerate(zip(end_observed, end_blind)):
        assert np.array_equal(a, b), (label, i)


# ---- d. edges of the host layer --------------------------------------------------------------------------------------------------------
def _without_penalty(config):
    return dict(config, args={k: v for k, v in config["args"].items() if k not in ("l1", "l2")})


EDGE_BASES = {"sgd": "sgd_momentum", "adam": "adam_defaults", "adagrad": "adagrad_decay_l1", "rmsprop": "rmsprop_momentum"}
EDGE_STEPS = 12


@pytest.mark.parametrize("kind", list(EDGE_BASES))
@pytest.mark.parametrize("l2", [0.0, 1e-2])
def test_parameter_the_loss_never_reaches(nk, tdev, kind, l2):
    """A registered parameter whose gradient is never written (its zero fill still pending when step() borrows it): with L2 it
    decays as the reference says, without a penalty it does not move."""
    config = _without_penalty(T.CONFIGS[EDGE_BASES[kind]])
    if l2:
        config = dict(config, args=dict(config["args"], l2=l2))
    ls = Lockstep(nk, config, f"optim_trajectory_unreached/{kind}/l2={l2}")
    reached, lonely = leaves(nk, tdev, [T.zoo()[3], T.zoo()[2]])
    ls.add(reached); ls.add(lonely)
    start = lonely.data().copy()
    for t in range(1, EDGE_STEPS + 1):
        ls.set_grad(0, T.gradient(t, 0, (129, 67)))
        ls.step()
        ls.compare(t)
        if not l2:
            assert np.array_equal(lonely.data(), start) and not lonely.grad().any()
        ls.zero_grad()                                    # pending again, for both
    assert not np.array_equal(reached.data(), T.zoo()[3])
    if l2:
        assert np.abs(lonely.data() - start).max() > 1e-4


@pytest.mark.parametrize("name", list(T.CONFIGS))
def test_parameter_registered_twice(nk, tdev, name):
    """Two sequential updates per step, each registration with its own state and its own step count (the second one sees the
    gradient with the penalty already added once)."""
    ls = Lockstep(nk, T.CONFIGS[name], f"optim_trajectory_twice/{name}")
    for p in leaves(nk, tdev, T.zoo()[:5]):
        ls.add(p)
    ls.register(3); ls.register(0)
    ls.run(16)


def test_two_optimizers_over_disjoint_parameters(nk, tdev):
    params = leaves(nk, tdev, T.zoo())
    a = Lockstep(nk, T.CONFIGS["adam_l1_l2"], "optim_trajectory_two/adam_l1_l2")
    b = Lockstep(nk, T.CONFIGS["rmsprop_centered_momentum_l1_l2"], "optim_trajectory_two/rmsprop_centered_momentum_l1_l2")
    for i, p in enumerate(params):
        (a if i % 2 == 0 else b).add(p)
    for t in range(1, 25):
        for ls in (a, b):
            for k, (p, arrays) in enumerate(ls.params):
                ls.set_grad(k, T.gradient(t, k, arrays[0][0].shape))
        a.step(); b.step()
        a.compare(t); b.compare(t)


@pytest.mark.parametrize("name", ["adam_l1_l2", "amsgrad_betas_eps_l2", "adagrad_decay_l1"])
def test_parameter_registered_late_starts_at_step_one(nk, tdev, name):
    """The step number is per registration: a parameter registered after 7 steps gets bias corrections / the decayed rate of step
    1 while the others are at step 8 (the rate itself, stepped by the scheduler, is the optimizer's)."""
    ls = Lockstep(nk, T.CONFIGS[name], f"optim_trajectory_late/{name}")
    params = leaves(nk, tdev, T.zoo()[:6])
    for p in params[:4]:
        ls.add(p)
    ls.run(7)
    for p in params[4:]:
        ls.add(p)
    ls.run(17, first=8)
    assert [s["step"] for s in ls.refs[0].slots] == [24] * 4 + [17] * 2


@pytest.mark.parametrize("name", ["sgd_momentum", "adam_l1_l2", "adagrad_plain_eps_l2", "rmsprop_centered_momentum_l1_l2"])
def test_gradient_buffer_reallocated_between_steps(nk, tdev, name):
    """no_grad() then with_grad() on a registered parameter (and on a root that reaches it) between steps: the optimizer holds the
    parameter, not a stale buffer, and its state is untouched."""
    ls = Lockstep(nk, T.CONFIGS[name], f"optim_trajectory_realloc/{name}")
    params = leaves(nk, tdev, T.zoo()[:6])
    for p in params:
        ls.add(p)
    root = (params[3] * 2.0).sum()
    for t in range(1, 17):
        if t % 3 == 0:
            for p in params:
                p.no_grad(); p.with_grad()
            root.no_grad(); root.with_grad()
        for k, (p, arrays) in enumerate(ls.params):
            ls.set_grad(k, T.gradient(t, k, arrays[0][0].shape))
        ls.step()
        ls.compare(t)


# ---- e. capture ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["adam_defaults", "amsgrad_betas_eps_l2", "adagrad_decay_l1"])
def test_refused_capture_leaves_the_optimizer_where_it_was(nk, tdev, name):
    """Adam and a decayed Adagrad refuse to be captured (their step number is a kernel argument).  The refusal throws out of the
    first parameter's update: no parameter's step counter may have advanced, or that parameter runs one step ahead of the others
    for the rest of training.  The whole trajectory equals the reference that never saw the attempt."""
    ls = Lockstep(nk, T.CONFIGS[name], f"optim_trajectory_refused_capture/{name}")
    for p in leaves(nk, tdev, T.zoo()):
        ls.add(p)
    ls.run(5)
    for k, (p, arrays) in enumerate(ls.params):
        p.set_grad(T.gradient(6, k, arrays[0][0].shape))     # uploaded before the capture: nothing but the step is attempted in it
    other = nk.rand(tdev, [8, 8], 3).relu()
    other.forward()
    tdev.graph_begin()
    other.forward()                                       # (something to capture)
    with pytest.raises(RuntimeError, match="captured"):
        ls.opt.step()
    graph = tdev.graph_end()
    del graph
    ls.run(19, first=6)
    print(f"{name}: worst err / bound = {ls.worst:.3f}")


@pytest.mark.parametrize("name", ["adagrad_plain_eps_l2", "rmsprop_plain", "rmsprop_centered_momentum_l1_l2", "sgd_nesterov_dampening_l2"])
def test_captured_step_replays_the_eager_bits(nk, tdev, name):
    """Adagrad without decay, RMSProp and SGD capture: replays equal eager steps bit for bit (the gradient is uploaded once and
    stays; with a penalty it grows in place, in both runs alike)."""
    def make():
        opt, _ = build(nk, T.CONFIGS[name])
        params = leaves(nk, tdev, T.zoo())
        for k, p in enumerate(params):
            opt.register(p)
            p.set_grad(T.gradient(1, k, tuple(p.shape)))
        return opt, params

    opt_e, eager = make()
    for _ in range(2 + 6):
        opt_e.step()
    opt_g, replayed = make()
    opt_g.step(); opt_g.step()                           # warm: the steady state, every gradient materialised
    tdev.graph_begin()
    opt_g.step()                                          # one linear chain of update launches
    graph = tdev.graph_end()                              # recorded, not run
    for _ in range(6):
        graph.launch()
    start = T.zoo()
    for k, (a, b) in enumerate(zip(eager, replayed)):
        assert np.array_equal(a.data(), b.data()) and np.array_equal(a.grad(), b.grad()), (name, k)
        assert np.isfinite(a.data()).all() and not np.array_equal(a.data(), start[k])


def test_replay_applies_the_captured_learning_rate(nk, tdev):
    """A captured SGD step has `lr` among its kernel arguments: `set_lr`, or a scheduler step, after the capture changes what the
    host reports and what a later EAGER step applies, not what a replay applies (include/neuronika_hip.h, graph capture)."""
    config = T.CONFIGS["sgd_momentum"]

    def make():
        opt, _ = build(nk, config)
        params = leaves(nk, tdev, T.zoo())
        for k, p in enumerate(params):
            opt.register(p)
            p.set_grad(T.gradient(1, k, tuple(p.shape)))
        return opt, params

    opt_e, eager = make()
    for _ in range(2 + 4):
        opt_e.step()                                      # all at the rate of the config
    opt_g, replayed = make()
    opt_g.step(); opt_g.step()
    tdev.graph_begin()
    opt_g.step()
    graph = tdev.graph_end()
    sched = nk.optim.lr_scheduler.ExponentialLR(opt_g, 0.1)
    graph.launch()
    sched.step()
    assert f32(opt_g.get_lr()) == f32(f32(config["lr"]) * f32(0.1))
    graph.launch()
    opt_g.set_lr(0.0)
    graph.launch(); graph.launch()
    for k, (a, b) in enumerate(zip(eager, replayed)):
        assert np.array_equal(a.data(), b.data()), k
    before = [p.data().copy() for p in replayed]
    opt_g.set_lr(config["lr"] * 0.1)
    opt_g.step()                                          # eager again: the host's rate applies
    opt_e.set_lr(config["lr"] * 0.1)
    opt_e.step()
    for k, (a, b, w0) in enumerate(zip(eager, replayed, before)):
        assert np.array_equal(a.data(), b.data()) and not np.array_equal(b.data(), w0), k

"""Reference driver for whole optimizer trajectories (NumPy only: no GPU, no torch).

The host layer `optim::SGD / Adam / Adagrad / RMSProp` + `lr_scheduler` (host/neuronika.{hpp,cpp}) decides, every step and for
every registered parameter, which state buffer, which 1-based step number, which learning rate and which penalty reach an update
kernel.  This module restates that layer on top of the oracle's single-step rules (`oracle/neuronika_oracle.py`:
sgd_step / adam_step / adagrad_step / rmsprop_step, dtype-generic) and the scheduler rules as tests/test_lr_scheduler.py states
them, so that a trajectory of many steps can be compared, after EVERY step, with the same trajectory in f64.

  CONFIGS        one entry per optimizer variant the host can build; every constructor argument is non-default in at least one
                 entry and default in at least one; every scheduler class drives at least one entry.
  PARAM_SHAPES   the parameter zoo registered together (`zoo()` gives its start values).
  gradient       deterministic f32 gradients whose scale drops to 1/8 after step 24.
  Reference      the host layer restated: register(w, g) / step() / scheduler_step().
  reference      a whole run: parameters, and gradients after the in-place penalty, after every step.
  bound / check  the comparison (the constants are tests/tolerance.py's).
  MUTANTS        deliberately wrong drivers; tests/test_oracle_optim_trajectory.py demands that each is at least 10 bounds away.

Every hyper-parameter is rounded to f32 before either precision uses it: the host classes hold `float`s, so the f64 run sees
the very values the device sees (1 - beta, 1 - alpha and 1 - dampening are then formed in the run's own precision)."""
import numpy as np

from oracle import neuronika_oracle as O
from tolerance import CPU_FACTOR, ELEMENTWISE_ATOL, ELEMENTWISE_RTOL

f32 = np.float32
STEPS = 64
DROP_AFTER, DROP = 24, 1.0 / 8.0        # gradient scale: 1 for steps 1 .. 24, 1/8 afterwards
MOMENTUM_EPS = 1.1920929e-7             # `momentum > f32::EPSILON` decides whether a buffer exists (sgd/mod.rs, rmsprop/mod.rs)

DEFAULTS = {
    "sgd": dict(l1=0.0, l2=0.0, momentum=0.0, dampening=0.0, nesterov=False),
    "adam": dict(beta1=0.9, beta2=0.999, eps=1e-8, l1=0.0, l2=0.0, amsgrad=False),
    "adagrad": dict(lr_decay=0.0, eps=1e-10, l1=0.0, l2=0.0),
    "rmsprop": dict(alpha=0.99, eps=1e-8, momentum=0.0, centered=False, l1=0.0, l2=0.0),
}


def _reciprocal_decay(epoch):            # LambdaLR: lr = initial * f(epoch)
    return 1.0 / (1.0 + 0.05 * epoch)


def _shrink(epoch):                      # MultiplicativeLR: lr = last * f(epoch)
    return 0.98 if epoch % 2 else 0.95


# kind: the host class; args: its keyword arguments as the Python binding names them (everything else stays at the default);
# sched: None or (scheduler class name, its arguments after the optimizer)
CONFIGS = {
    "sgd_plain_l1_l2": dict(kind="sgd", lr=0.05, args=dict(l1=1e-3, l2=1e-2), sched=("StepLR", (16, 0.5))),
    "sgd_momentum": dict(kind="sgd", lr=0.02, args=dict(momentum=0.9), sched=None),
    "sgd_nesterov_dampening_l2": dict(kind="sgd", lr=0.02, args=dict(momentum=0.8, dampening=0.3, nesterov=True, l2=1e-2),
                                      sched=("MultiStepLR", ([10, 30, 50], 0.5))),
    "adam_defaults": dict(kind="adam", lr=0.05, args=dict(), sched=None),
    "adam_l1_l2": dict(kind="adam", lr=0.05, args=dict(l1=1e-3, l2=1e-2), sched=("ExponentialLR", (0.97,))),
    "amsgrad_betas_eps_l2": dict(kind="adam", lr=0.05, args=dict(beta1=0.8, beta2=0.9, eps=1e-3, l2=1e-2, amsgrad=True),
                                 sched=("LambdaLR", (_reciprocal_decay,))),
    "adagrad_decay_l1": dict(kind="adagrad", lr=0.1, args=dict(lr_decay=0.05, l1=1e-3), sched=("MultiplicativeLR", (_shrink,))),
    "adagrad_plain_eps_l2": dict(kind="adagrad", lr=0.1, args=dict(eps=1e-2, l2=1e-2), sched=None),
    "rmsprop_plain": dict(kind="rmsprop", lr=0.01, args=dict(), sched=("StepLR", (16, 0.5))),
    "rmsprop_centered_alpha_eps": dict(kind="rmsprop", lr=0.01, args=dict(alpha=0.9, eps=1e-3, centered=True), sched=None),
    "rmsprop_momentum": dict(kind="rmsprop", lr=0.01, args=dict(momentum=0.5), sched=("MultiStepLR", ([8, 40], 0.25))),
    "rmsprop_centered_momentum_l1_l2": dict(kind="rmsprop", lr=0.01,
                                            args=dict(alpha=0.95, momentum=0.6, centered=True, l1=1e-3, l2=1e-2),
                                            sched=("ExponentialLR", (0.98,))),
}

# a 0-d scalar, one element, a length not divisible by 4, a matrix with an odd row length, one SGD_CHUNK (4096) plus one element,
# a conv kernel, two parameters of one shape (the shared-state mutant needs them), and enough entries (11 > SGD_MULTI_MAX = 8)
# that one SGD step is two launches
PARAM_SHAPES = [(), (1,), (7,), (129, 67), (4097,), (8, 3, 3, 3), (16,), (16,), (33, 3), (2, 5), (1, 6)]
TWINS = (6, 7)                           # the two entries of equal shape


def zoo(shapes=None, seed=20):
    """f32 start values in [-1, 1); every parameter of three or more elements starts with an exact +0.0 in its first and an exact
    -0.0 in its last element, the one-element parameter is -0.0 (Rust's `signum(+-0) = +-1` under L1)."""
    rng = np.random.default_rng(seed)
    out = []
    for shape in (PARAM_SHAPES if shapes is None else shapes):
        w = (rng.random(shape, dtype=f32) * f32(2) - f32(1)).astype(f32).reshape(shape)
        flat = w.reshape(-1)
        if flat.size >= 3:
            flat[0], flat[-1] = f32(0.0), f32(-0.0)
        elif shape == (1,):
            flat[0] = f32(-0.0)
        out.append(w)
    return out


def gradient(step, index, shape, seed=7):
    """The f32 gradient of parameter `index` at the 1-based `step`: N(0, 1) up to step 24, N(0, 1) / 8 afterwards, so that AMSGrad's
    running maximum holds a value the plain second moment has left."""
    rng = np.random.default_rng([seed, step, index])
    g = rng.standard_normal(shape, dtype=f32)
    return np.asarray(g * f32(1.0 if step <= DROP_AFTER else DROP), dtype=f32).reshape(shape)


class Scheduler:
    """`LRScheduler::step`: prepare_step (last <- current, epoch += 1), then the policy, in f32 (test_lr_scheduler.py)."""

    def __init__(self, name, args, lr):
        self.name, self.args = name, args
        self.initial = self.last = self.current = f32(lr)
        self.epoch = 0

    def step(self):
        self.last = self.current
        self.epoch += 1
        e, a = self.epoch, self.args
        if self.name == "StepLR":
            if e % a[0] == 0:
                self.current = f32(self.last * f32(a[1]))
        elif self.name == "MultiStepLR":
            if e in a[0]:
                self.current = f32(self.last * f32(a[1]))
        elif self.name == "ExponentialLR":
            self.current = f32(self.last * f32(a[0]))
        elif self.name == "LambdaLR":
            self.current = f32(self.initial * f32(a[0](e)))
        elif self.name == "MultiplicativeLR":
            self.current = f32(self.last * f32(a[0](e)))
        else:
            raise KeyError(self.name)
        return self.current


def hyper(config):
    """The constructor's arguments with the defaults filled in, every number as the f32 the host class stores."""
    h = dict(DEFAULTS[config["kind"]])
    h.update(config["args"])
    return {k: (v if isinstance(v, bool) else float(f32(v))) for k, v in h.items()}


def _signum0_penalty(w, l1, l2):
    dt = w.dtype.type
    return dt(l1) * np.sign(w) + (dt(2) * dt(l2) * w if l2 != 0.0 else dt(0))


class Reference:
    """`optim::Optimizer` restated: one state set and one 1-based step counter per REGISTRATION (a parameter registered twice is
    updated twice a step, each time with its own state), the gradient buffer belongs to the parameter and takes the penalty in
    place, the learning rate is a single f32 that a scheduler overwrites.  `flaws` switches on the wrong behaviours of MUTANTS."""

    def __init__(self, config, dtype, flaws=()):
        self.kind, self.h, self.dtype, self.flaws = config["kind"], hyper(config), np.dtype(dtype), set(flaws)
        self.lr = f32(config["lr"])
        self.sched = Scheduler(config["sched"][0], config["sched"][1], self.lr) if config["sched"] else None
        self.slots = []
        self.min_centered = np.inf       # smallest square_avg - grad_avg^2 met under a root (centered RMSProp)

    def _nstate(self):
        h = self.h
        return {"sgd": 1 if h.get("momentum", 0) > MOMENTUM_EPS else 0, "adam": 3 if h.get("amsgrad") else 2, "adagrad": 1, "rmsprop": 3}[self.kind]

    def register(self, w, g):
        """w, g: arrays of the run's dtype, updated in place; the caller fills g before each step()."""
        assert w.dtype == self.dtype and g.dtype == self.dtype and w.shape == g.shape
        if "registered_twice_updated_once" in self.flaws and any(s["w"] is w for s in self.slots):
            return
        state = [np.zeros_like(w) for _ in range(self._nstate())]
        if "shared_state" in self.flaws:
            for s in self.slots:
                if s["w"] is not w and s["w"].shape == w.shape:      # the zoo's TWINS
                    state = s["state"]
        self.slots.append(dict(w=w, g=g, state=state, step=0))

    def step(self):
        h, lr = self.h, float(self.lr)
        for s in self.slots:
            w, g, st = s["w"], s["g"], s["state"]
            s["step"] += 1
            n = s["step"] + (1 if "step_ahead" in self.flaws and s["step"] > 1 else 0)
            l1, l2 = h["l1"], h["l2"]
            if "signum_zero" in self.flaws:
                g += _signum0_penalty(w, l1, l2)
                l1 = l2 = 0.0
            if self.kind == "sgd":
                O.sgd_step(w, g, lr, st[0] if st else None, h["momentum"], h["dampening"], h["nesterov"], l1, l2)
            elif self.kind == "adam":
                O.adam_step(w, g, st[0], st[1], lr, h["beta1"], h["beta2"], h["eps"], n, st[2] if h["amsgrad"] else None, l1, l2)
            elif self.kind == "adagrad":
                O.adagrad_step(w, g, st[0], lr, h["lr_decay"], h["eps"], n, l1, l2)
            else:
                mom = h["momentum"] > MOMENTUM_EPS
                if h["centered"]:        # what the step below takes the root of, from the same inputs
                    dt = w.dtype.type
                    gp = g + O.penalty_grad(w, l1, l2)
                    sq = st[0] * dt(h["alpha"]) + gp * gp * dt(1.0 - h["alpha"])
                    av = st[1] * dt(h["alpha"]) + gp * dt(1.0 - h["alpha"])
                    live = sq > 0
                    if live.any():
                        self.min_centered = min(self.min_centered, float(((sq + (-av * av)) / np.where(live, sq, 1))[live].min()))
                O.rmsprop_step(w, g, st[0], lr, h["alpha"], h["eps"], st[1] if h["centered"] else None, st[2] if mom else None,
                               h["momentum"], l1, l2)

    def scheduler_step(self):
        if self.sched is not None:
            lr = self.sched.step()
            if "stale_lr" not in self.flaws:
                self.lr = lr


def reference(config, dtype, steps=STEPS, grads=None, init=None, twice=(), flaws=(), stats=None):
    """Run `steps` steps over the parameters `init` (default: the zoo), each registered once, those whose index is in `twice` a
    second time after all the others.  Gradients: `grads[step - 1][index]` (f32, e.g. what the device produced) or `gradient()`.
    Returns (W, G): W[step - 1][index] the parameter after that step, G[step - 1][index] its gradient buffer after that step
    (with the penalty added in place, once per registration), both in `dtype`.  `stats`, a dict, receives `min_centered`."""
    init = zoo() if init is None else init
    ws = [np.array(w, dtype=dtype) for w in init]
    gs = [np.zeros_like(w) for w in ws]
    ref = Reference(config, dtype, flaws)
    for i in list(range(len(ws))) + list(twice):
        ref.register(ws[i], gs[i])
    W, G = [], []
    for t in range(1, steps + 1):
        for i, g in enumerate(gs):
            g[...] = np.asarray(grads[t - 1][i] if grads is not None else gradient(t, i, g.shape), dtype=f32).reshape(g.shape)
        ref.step()
        W.append([w.copy() for w in ws])
        G.append([g.copy() for g in gs])
        ref.scheduler_step()
    if stats is not None:
        stats["min_centered"] = ref.min_centered
    return W, G


def bound(w32, w64):
    """max|dev - w64| <= CPU_FACTOR * max|w32 - w64| + ELEMENTWISE_ATOL + ELEMENTWISE_RTOL * max|w64|, per parameter and step."""
    w64 = np.asarray(w64, np.float64)
    return (CPU_FACTOR * float(np.abs(np.asarray(w32, np.float64) - w64).max())
            + ELEMENTWISE_ATOL + ELEMENTWISE_RTOL * float(np.abs(w64).max()))


def ratio(got, w32, w64):
    """max|got - w64| / bound(w32, w64); nan or inf in `got` gives inf."""
    err = float(np.abs(np.asarray(got, np.float64) - np.asarray(w64, np.float64)).max())
    return err / bound(w32, w64) if np.isfinite(err) else np.inf


def check(label, got, w32, w64):
    """Assert one device array against the f64 reference inside `bound`; reports through conftest.record_margin.  Returns
    err / bound."""
    from conftest import record_margin
    got64, w64 = np.asarray(got, np.float64), np.asarray(w64, np.float64)
    assert got64.shape == w64.shape, (label, got64.shape, w64.shape)
    err_dev = float(np.abs(got64 - w64).max())
    err_cpu = float(np.abs(np.asarray(w32, np.float64) - w64).max())
    elementwise = ELEMENTWISE_ATOL + ELEMENTWISE_RTOL * float(np.abs(w64).max())
    record_margin(label, err_dev, err_cpu, elementwise)
    b = CPU_FACTOR * err_cpu + elementwise
    assert np.isfinite(got64).all() and err_dev <= b, (label, err_dev, err_cpu, elementwise, np.unravel_index(
        int(np.nanargmax(np.abs(got64 - w64))), w64.shape) if w64.ndim else ())
    return err_dev / b


# ---- deliberately wrong drivers ---------------------------------------------------------------------------------------------------
def _differs(arg):
    return lambda c: hyper(c)[arg] != hyper(dict(c, args={}))[arg] if arg in DEFAULTS[c["kind"]] else False


def _with(**kw):
    return lambda c: dict(c, args=dict(c["args"], **kw))


def _default(arg):
    return lambda c: dict(c, args={k: v for k, v in c["args"].items() if k != arg})


def _keeps_state(c):
    return c["kind"] != "sgd" or hyper(c)["momentum"] > MOMENTUM_EPS


# name -> (applies(config), config -> config run in its place, Reference flaws, parameters registered twice in BOTH runs)
MUTANTS = {
    "step_ahead": (lambda c: c["kind"] == "adam" or (c["kind"] == "adagrad" and hyper(c)["lr_decay"] != 0), None, ("step_ahead",), ()),
    "stale_lr": (lambda c: c["sched"] is not None, None, ("stale_lr",), ()),
    "l2_dropped": (_differs("l2"), _default("l2"), (), ()),
    "l1_dropped": (_differs("l1"), _default("l1"), (), ()),
    "signum_zero": (_differs("l1"), None, ("signum_zero",), ()),
    "dampening_ignored": (_differs("dampening"), _default("dampening"), (), ()),
    "nesterov_ignored": (_differs("nesterov"), _default("nesterov"), (), ()),
    "amsgrad_max_ignored": (_differs("amsgrad"), _default("amsgrad"), (), ()),
    "centered_ignored": (_differs("centered"), _default("centered"), (), ()),
    "rmsprop_momentum_ignored": (lambda c: c["kind"] == "rmsprop" and _differs("momentum")(c), _default("momentum"), (), ()),
    "default_sgd_momentum": (lambda c: c["kind"] == "sgd" and _differs("momentum")(c), _default("momentum"), (), ()),
    "default_beta1": (_differs("beta1"), _default("beta1"), (), ()),
    "default_beta2": (_differs("beta2"), _default("beta2"), (), ()),
    "default_eps": (_differs("eps"), _default("eps"), (), ()),
    "default_alpha": (_differs("alpha"), _default("alpha"), (), ()),
    "default_lr_decay": (_differs("lr_decay"), _default("lr_decay"), (), ()),
    "shared_state": (_keeps_state, None, ("shared_state",), ()),
    "registered_twice_updated_once": (lambda c: True, None, ("registered_twice_updated_once",), (3, 0)),
}


def mutant_runs(name, config, steps=STEPS):
    """(W of the mutant in f32, W of the honest f32 run, W of the f64 run) for one applicable mutant."""
    applies, rewrite, flaws, twice = MUTANTS[name]
    assert applies(config), (name, config)
    wrong = rewrite(config) if rewrite else config
    return (reference(wrong, f32, steps, twice=twice, flaws=flaws)[0], reference(config, f32, steps, twice=twice)[0],
            reference(config, np.float64, steps, twice=twice)[0])

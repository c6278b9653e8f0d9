"""Reference driver for AdamW and global-norm gradient clipping (NumPy only: no GPU, no torch), in the manner of
tests/optim_trajectory.py, whose zoo, gradients, scheduler, bound, ratio and check it reuses.

  adamw_step      one parameter: w *= 1 - lr * weight_decay (skipped at weight_decay == 0), then the oracle's adam_step without a
                  penalty - dtype-generic, in place; the order and the expression of include/neuronika_hip.h.
  clip_grad_norm  the header's rule: every square and the whole sum in f64, total_norm rounded to f32, coef = max_norm /
                  (total_norm + 1e-6) in f32 and replaced by 1 when it exceeds 1; the gradients are scaled in their own dtype.
                  A gradient listed twice counts once.
  Reference       `optim::AdamW` / `optim::SGD` with `Optimizer::clip_grad_norm(max_norm)` called before every step when the config
                  has a `max_norm`: one state set and one 1-based step counter per REGISTRATION.
  CONFIGS         every constructor argument of AdamW default in one entry and non-default in another, AMSGrad, a warm-up through
                  LambdaLR, weight_decay = 0, clipping at max_norm = 20 (AdamW, and plain SGD).
  MUTANTS         deliberately wrong drivers; tests/test_oracle_adamw.py demands that each is at least 10 bounds away.

The zoo's global gradient norm is about 115 for steps 1 .. 24 and about 14.3 afterwards: max_norm = 20 clips exactly the first 24
of the 64 steps (CLIPPED_STEPS), so a trajectory runs both the scaling and the early-exit branch of the device's scale kernel."""
import numpy as np

import optim_trajectory as T
from oracle import neuronika_oracle as O

f32 = np.float32
STEPS = T.STEPS
MAX_NORM = 20.0
CLIPPED_STEPS = T.DROP_AFTER            # 24: the steps whose global norm (about 115) exceeds MAX_NORM; about 14.3 afterwards

DEFAULTS = {
    "adamw": dict(beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=1e-2, amsgrad=False),
    "sgd": T.DEFAULTS["sgd"],
}


def _warm_up(epoch):                     # LambdaLR: lr = initial * f(epoch); the first step runs at the initial rate
    return min(1.0, 0.25 + 0.075 * epoch)


# kind / lr / args / sched as in optim_trajectory.CONFIGS; max_norm: None, or the bound of the clip before every step
CONFIGS = {
    "adamw_defaults": dict(kind="adamw", lr=0.01, args=dict(), sched=None, max_norm=None),
    "adamw_decay_clip": dict(kind="adamw", lr=0.01, args=dict(weight_decay=0.1), sched=None, max_norm=MAX_NORM),
    "adamw_amsgrad_betas_eps_clip": dict(kind="adamw", lr=0.01, args=dict(beta1=0.8, beta2=0.9, eps=1e-3, weight_decay=0.05, amsgrad=True),
                                         sched=("StepLR", (16, 0.5)), max_norm=MAX_NORM),
    "adamw_warm_up": dict(kind="adamw", lr=0.02, args=dict(weight_decay=0.1), sched=("LambdaLR", (_warm_up,)), max_norm=None),
    "adamw_no_decay_amsgrad": dict(kind="adamw", lr=0.01, args=dict(weight_decay=0.0, amsgrad=True), sched=None, max_norm=None),
    "sgd_clip": dict(kind="sgd", lr=0.02, args=dict(), sched=None, max_norm=MAX_NORM),
}


def hyper(config):
    """The constructor's arguments with the defaults filled in, every number as the f32 the host class stores."""
    h = dict(DEFAULTS[config["kind"]])
    h.update(config["args"])
    return {k: (v if isinstance(v, bool) else float(f32(v))) for k, v in h.items()}


def adamw_step(w, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, weight_decay, max_exp_avg_sq=None):
    """In place, in the dtype of `w`; `step` is 1-based.  The gradient is read, not written."""
    dt = w.dtype.type
    if weight_decay != 0.0:
        w *= dt(1) - dt(lr) * dt(weight_decay)
    O.adam_step(w, grad.copy(), exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, max_exp_avg_sq)


def clip_grad_norm(grads, max_norm):
    """Scales the arrays of `grads` in place (one listed twice: once); returns (total_norm, coef), both f32."""
    unique = []
    for g in grads:
        if not any(g is u for u in unique):
            unique.append(g)
    total = 0.0
    for g in unique:
        g64 = np.asarray(g, np.float64).reshape(-1)
        total += float(np.dot(g64, g64))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        norm = f32(np.sqrt(np.float64(total)))
        coef = f32(max_norm) / f32(norm + f32(1e-6))
        coef = f32(1) if coef > 1 else f32(coef)       # a NaN norm gives a NaN coefficient, not 1
        if coef != 1 and np.isfinite(max_norm):        # +inf: measure only
            for g in unique:
                g *= g.dtype.type(coef)
    return norm, coef


class Reference:
    """`optim::AdamW` (or plain `optim::SGD`) restated, with `clip_grad_norm(max_norm)` before every step when the config asks for
    it.  `flaws` switches on the wrong behaviours of MUTANTS."""

    def __init__(self, config, dtype, flaws=()):
        self.kind, self.h, self.dtype, self.flaws = config["kind"], hyper(config), np.dtype(dtype), set(flaws)
        self.lr = f32(config["lr"])
        self.max_norm = config["max_norm"]
        self.sched = T.Scheduler(config["sched"][0], config["sched"][1], self.lr) if config["sched"] else None
        self.slots, self.norms, self.clipped = [], [], 0

    def register(self, w, g):
        assert w.dtype == self.dtype and g.dtype == self.dtype and w.shape == g.shape
        n = {"adamw": 3 if self.h.get("amsgrad") else 2, "sgd": 0}[self.kind]
        self.slots.append(dict(w=w, g=g, state=[np.zeros_like(w) for _ in range(n)], step=0))

    def clip(self):
        """`Optimizer::clip_grad_norm`: over the registered parameters, each once.  Returns the f32 norm."""
        grads = [s["g"] for s in self.slots]
        if "clip_per_parameter" in self.flaws:
            unique = [g for k, g in enumerate(grads) if not any(g is o for o in grads[:k])]
            norms = [clip_grad_norm([g], self.max_norm) for g in unique]
            norm, coef = max(n for n, _ in norms), min(c for _, c in norms)
        elif "twice_counted_twice" in self.flaws:
            total = sum(float(np.dot(g.astype(np.float64).reshape(-1), g.astype(np.float64).reshape(-1))) for g in grads)
            norm = f32(np.sqrt(total))
            coef = f32(self.max_norm) / f32(norm + f32(1e-6))
            coef = f32(1) if coef > 1 else coef
            done = []
            for g in grads:
                if not any(g is d for d in done):
                    done.append(g)
                    g *= g.dtype.type(coef)
        else:
            norm, coef = clip_grad_norm(grads, self.max_norm)
        self.norms.append(norm)
        self.clipped += int(coef < 1)
        return norm

    def step(self):
        if self.max_norm is not None and "clip_dropped" not in self.flaws:
            self.clip()
        h, lr = self.h, float(self.lr)
        for s in self.slots:
            w, g, st = s["w"], s["g"], s["state"]
            s["step"] += 1
            if self.kind == "sgd":
                O.sgd_step(w, g, lr)
                continue
            n = max(1, s["step"] - 1) if "stale_step" in self.flaws else s["step"]
            wd = h["weight_decay"]
            dt = w.dtype.type
            if "decay_coupled" in self.flaws:            # L2 folded into the gradient: the Adam denominator rescales it
                adamw_step(w, g + dt(wd) * w, st[0], st[1], lr, h["beta1"], h["beta2"], h["eps"], n, 0.0, st[2] if h["amsgrad"] else None)
            elif "decay_without_lr" in self.flaws:
                w *= dt(1) - dt(wd)
                adamw_step(w, g, st[0], st[1], lr, h["beta1"], h["beta2"], h["eps"], n, 0.0, st[2] if h["amsgrad"] else None)
            else:
                adamw_step(w, g, st[0], st[1], lr, h["beta1"], h["beta2"], h["eps"], n, wd, st[2] if h["amsgrad"] else None)

    def scheduler_step(self):
        if self.sched is not None:
            self.lr = self.sched.step()


def reference(config, dtype, steps=STEPS, grads=None, init=None, twice=(), flaws=(), stats=None):
    """As optim_trajectory.reference: (W, G) with W[step - 1][index] the parameter and G[step - 1][index] its gradient buffer (after
    the clip) after that step.  `stats`, a dict, receives `norms` (f32, one per clipped-or-measured step) and `clipped`."""
    init = T.zoo() if init is None else init
    ws = [np.array(w, dtype=dtype) for w in init]
    gs = [np.zeros_like(w) for w in ws]
    ref = Reference(config, dtype, flaws)
    for i in list(range(len(ws))) + list(twice):
        ref.register(ws[i], gs[i])
    W, G = [], []
    for t in range(1, steps + 1):
        for i, g in enumerate(gs):
            g[...] = np.asarray(grads[t - 1][i] if grads is not None else T.gradient(t, i, g.shape), dtype=f32).reshape(g.shape)
        ref.step()
        W.append([w.copy() for w in ws])
        G.append([g.copy() for g in gs])
        ref.scheduler_step()
    if stats is not None:
        stats["norms"], stats["clipped"] = list(ref.norms), ref.clipped
    return W, G


# ---- deliberately wrong drivers ---------------------------------------------------------------------------------------------------
def _decays(c):
    return c["kind"] == "adamw" and hyper(c)["weight_decay"] != 0


def _clips(c):
    return c["max_norm"] is not None


def _no_decay(c):
    return dict(c, args=dict(c["args"], weight_decay=0.0))


# name -> (applies(config), config -> config run in its place, Reference flaws, parameters registered twice in BOTH runs)
MUTANTS = {
    "decay_coupled": (_decays, None, ("decay_coupled",), ()),
    "decay_dropped": (_decays, _no_decay, (), ()),
    "decay_without_lr": (_decays, None, ("decay_without_lr",), ()),
    "clip_dropped": (_clips, None, ("clip_dropped",), ()),
    "clip_per_parameter": (_clips, None, ("clip_per_parameter",), ()),
    "twice_counted_twice": (_clips, None, ("twice_counted_twice",), (3, 0)),
    "stale_step": (lambda c: c["kind"] == "adamw", None, ("stale_step",), ()),
}


def mutant_runs(name, config, steps=STEPS):
    """(W of the mutant in f32, W of the honest f32 run, W of the f64 run) for one applicable mutant."""
    applies, rewrite, flaws, twice = MUTANTS[name]
    assert applies(config), (name, config)
    wrong = rewrite(config) if rewrite else config
    return (reference(wrong, f32, steps, twice=twice, flaws=flaws)[0], reference(config, f32, steps, twice=twice)[0],
            reference(config, np.float64, steps, twice=twice)[0])

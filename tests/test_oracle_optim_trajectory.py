"""tests/optim_trajectory.py on the CPU: the f32 trajectory of every optimizer config stays inside the bound of the f64 one, every
deliberately wrong driver (MUTANTS) leaves it by at least a factor 10, and the driver's scheduler rules give the numbers of
tests/test_lr_scheduler.py.  The second test is what the bound of tests/test_gpu_tape_optim.py rests on: the bound may move only
while every mutant is still detected."""
import numpy as np
import pytest

import optim_trajectory as T

f32 = np.float32
DETECTION_FACTOR = 10.0


@pytest.fixture(scope="module")
def runs():
    out = {}
    for name, config in T.CONFIGS.items():
        stats = {}
        W32, G32 = T.reference(config, f32, stats=stats)
        W64, G64 = T.reference(config, np.float64)
        out[name] = (W32, G32, W64, G64, stats)
    return out


def test_configs_cover_every_argument_and_scheduler():
    kinds = {c["kind"] for c in T.CONFIGS.values()}
    assert kinds == set(T.DEFAULTS)
    for kind, defaults in T.DEFAULTS.items():
        same = {c_name: T.hyper(c) for c_name, c in T.CONFIGS.items() if c["kind"] == kind}
        base = T.hyper(dict(kind=kind, args={}))
        for arg in defaults:
            values = {h[arg] for h in same.values()}
            assert base[arg] in values, (kind, arg, "the default is kept nowhere")
            assert len(values) > 1, (kind, arg, "never takes a non-default value")
    assert {c["sched"][0] if c["sched"] else None for c in T.CONFIGS.values()} == {
        None, "StepLR", "MultiStepLR", "ExponentialLR", "LambdaLR", "MultiplicativeLR"}
    rms = {(T.hyper(c)["centered"], T.hyper(c)["momentum"] > 0) for c in T.CONFIGS.values() if c["kind"] == "rmsprop"}
    assert len(rms) == 4
    # the zoo: more parameters than one SGD launch takes, both zeros planted, a chunk boundary crossed
    zoo = T.zoo()
    assert len(zoo) > 8 and [w.shape for w in zoo] == [tuple(s) for s in T.PARAM_SHAPES]
    assert zoo[T.TWINS[0]].shape == zoo[T.TWINS[1]].shape
    for w in zoo:
        assert w.dtype == f32 and np.abs(w).max() <= 1.0
        if w.size >= 3:
            flat = w.reshape(-1)
            assert flat[0] == 0 and not np.signbit(flat[0]) and flat[-1] == 0 and np.signbit(flat[-1])
    assert np.signbit(zoo[1][0]) and zoo[1][0] == 0 and zoo[0].shape == ()
    g_early, g_late = T.gradient(T.DROP_AFTER, 3, (129, 67)), T.gradient(T.DROP_AFTER + 1, 3, (129, 67))
    assert g_early.dtype == f32 and 0.9 < g_early.std() < 1.1 and 0.9 * T.DROP < g_late.std() < 1.1 * T.DROP
    assert np.array_equal(g_early, T.gradient(T.DROP_AFTER, 3, (129, 67))) and not np.array_equal(g_early, T.gradient(T.DROP_AFTER, 4, (129, 67)))


@pytest.mark.parametrize("name", list(T.CONFIGS))
def test_f32_trajectory_stays_inside_the_bound_of_the_f64_one(runs, name):
    W32, G32, W64, G64, stats = runs[name]
    assert len(W32) == T.STEPS
    worst = 0.0
    for t in range(T.STEPS):
        for i in range(len(W32[t])):
            assert np.isfinite(W32[t][i]).all() and np.isfinite(W64[t][i]).all() and np.isfinite(G32[t][i]).all(), (name, t + 1, i)
            assert W32[t][i].dtype == f32 and W64[t][i].dtype == np.float64
            worst = max(worst, float(np.abs(W32[t][i].astype(np.float64) - W64[t][i]).max()))
    print(f"{name}: max |w32 - w64| over {T.STEPS} steps = {worst:.3g}")
    # the f32 run is inside bound(w32, w64) by construction (the bound contains twice its error); what can be asserted is that
    # the run does not amplify rounding: 64 steps of a few ulp of values of order 1 are some 1e-5, and 1e-4 keeps the factor-2
    # term of the bound from swallowing the defects of MUTANTS (test_detection_condition measures exactly that)
    assert worst < 1e-4
    if T.hyper(T.CONFIGS[name]).get("centered"):
        # centered RMSProp takes the root of square_avg - grad_avg^2; in exact arithmetic it is >= alpha^step * square_avg
        print(f"{name}: min (square_avg - grad_avg^2) / square_avg in f32 = {stats['min_centered']:.3g}")
        assert stats["min_centered"] > 1e-4
    # the gradient buffer takes the penalty in place: it differs from the injected gradient exactly where a penalty is configured
    h = T.hyper(T.CONFIGS[name])
    moved = any(not np.array_equal(G32[0][i], T.gradient(1, i, G32[0][i].shape)) for i in range(len(G32[0])))
    assert moved == (h["l1"] != 0 or h["l2"] != 0)


CASES = [(m, c) for m in T.MUTANTS for c in T.CONFIGS if T.MUTANTS[m][0](T.CONFIGS[c])]


def test_every_mutant_applies_somewhere():
    assert {m for m, _ in CASES} == set(T.MUTANTS)
    for kind in T.DEFAULTS:                               # and every optimizer class meets the host-layer mutants
        names = [c for c, cfg in T.CONFIGS.items() if cfg["kind"] == kind]
        assert any(("registered_twice_updated_once", c) in CASES for c in names)
    assert any(m == "step_ahead" and T.CONFIGS[c]["kind"] == "adagrad" for m, c in CASES)
    assert sum(m == "step_ahead" and T.CONFIGS[c]["kind"] == "adam" for m, c in CASES) == 3


@pytest.mark.parametrize("mutant,name", CASES)
def test_detection_condition(mutant, name):
    """Every wrong driver exceeds the bound by at least DETECTION_FACTOR at some step, for some parameter."""
    Wm, W32, W64 = T.mutant_runs(mutant, T.CONFIGS[name])
    worst, where = 0.0, None
    for t in range(T.STEPS):
        for i in range(len(W64[t])):
            r = T.ratio(Wm[t][i], W32[t][i], W64[t][i])
            if r > worst:
                worst, where = r, (t + 1, i)
    print(f"{mutant} on {name}: {worst:.3g} bounds at (step, parameter) {where}")
    assert worst >= DETECTION_FACTOR, (mutant, name, worst, where)


def test_signum_zero_shows_at_the_first_step():
    """Why every step is compared and not only the last: the planted zeros move by lr * l1 at step 1."""
    Wm, W32, W64 = T.mutant_runs("signum_zero", T.CONFIGS["sgd_plain_l1_l2"], steps=1)
    assert max(T.ratio(Wm[0][i], W32[0][i], W64[0][i]) for i in range(len(W64[0]))) >= DETECTION_FACTOR


def test_scheduler_rules_give_the_reference_scenarios():
    """neuronika-optim/src/lr_scheduler/*/test.rs as tests/test_lr_scheduler.py::test_reference_scenarios states them: five
    epochs from lr = 1."""
    def run(name, args):
        s = T.Scheduler(name, args, 1.0)
        cur = []
        for epoch in range(5):
            cur.append(float(s.current))
            assert s.epoch == epoch
            s.step()
        return s, cur

    s, cur = run("StepLR", (1, 2.0))
    assert cur == [2.0 ** e for e in range(5)] and s.last == 16.0
    s, _ = run("ExponentialLR", (5.0,))
    assert s.last == 5.0 ** 4 and s.current == 5.0 ** 5
    s, _ = run("MultiStepLR", ([1, 2, 3, 4], 2.0))
    assert s.last == 16.0 and s.current == 16.0
    s, cur = run("LambdaLR", (lambda e: float(e),))
    assert cur[1:] == [1.0, 2.0, 3.0, 4.0] and s.last == 4.0
    s, _ = run("MultiplicativeLR", (lambda e: float(e),))
    assert s.last == 24.0 and s.current == 120.0
    # f32 at every stage, as test_step_and_multistep / test_exponential_lambda_multiplicative state it
    s, want = T.Scheduler("StepLR", (3, 0.1), 0.5), f32(0.5)
    for epoch in range(1, 11):
        s.step()
        last = want
        if epoch % 3 == 0:
            want = f32(want * f32(0.1))
        assert s.last == last and s.current == want and s.current.dtype == f32
    s = T.Scheduler("LambdaLR", (lambda e: 1.0 / (1 + e),), 2.0)
    for epoch in range(1, 5):
        assert s.step() == f32(f32(2.0) * f32(1.0 / (1 + epoch)))


def test_scheduler_rules_equal_the_host_classes():
    """The same scalars from the host classes (no device is touched): the rate every config's scheduler hands over per step."""
    import neuronika_amd
    opt_mod = neuronika_amd.tape.optim
    for name, config in T.CONFIGS.items():
        if config["sched"] is None:
            continue
        opt = opt_mod.SGD(config["lr"])
        sched = getattr(opt_mod.lr_scheduler, config["sched"][0])(opt, *config["sched"][1])
        mine = T.Scheduler(config["sched"][0], config["sched"][1], config["lr"])
        for _ in range(T.STEPS):
            sched.step()
            assert f32(opt.get_lr()) == mine.step(), (name, mine.epoch)

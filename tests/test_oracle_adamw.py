"""tests/adamw_oracle.py on the CPU: its f64 AdamW step is torch.optim.AdamW's, its clip is torch.nn.utils.clip_grad_norm_'s, the
f32 trajectory of every config stays inside the bound of the f64 one, max_norm = 20 clips exactly the 24 early steps, and every
deliberately wrong driver (MUTANTS) leaves the bound by at least a factor 10 - the margin tests/test_oracle_optim_trajectory.py
demands, and what the bound of tests/test_gpu_tape_adamw.py rests on."""
import os
import subprocess
import sys

import numpy as np
import pytest

import adamw_oracle as A
import optim_trajectory as T
f32 = np.float32
DETECTION_FACTOR = 10.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_configs_cover_every_argument():
    kinds = [c["kind"] for c in A.CONFIGS.values()]
    assert set(kinds) == {"adamw", "sgd"}
    same = {n: A.hyper(c) for n, c in A.CONFIGS.items() if c["kind"] == "adamw"}
    base = A.hyper(dict(kind="adamw", args={}))
    for arg in A.DEFAULTS["adamw"]:
        values = {h[arg] for h in same.values()}
        assert base[arg] in values, (arg, "the default is kept nowhere")
        assert len(values) > 1, (arg, "never takes a non-default value")
    assert any(h["weight_decay"] == 0 for h in same.values())
    assert any(c["sched"] and c["sched"][0] == "LambdaLR" for c in A.CONFIGS.values())
    assert any(c["max_norm"] == 20 and c["kind"] == "adamw" for c in A.CONFIGS.values())
    assert any(c["max_norm"] == 20 and c["kind"] == "sgd" for c in A.CONFIGS.values())
    assert any(c["max_norm"] is None for c in A.CONFIGS.values())
    warm = [A._warm_up(e) for e in range(12)]
    assert warm == sorted(warm) and warm[0] < 1 and warm[-1] == 1.0


# torch runs in a child process: a process that has loaded the HIP library must not import torch as well
_TORCH_CHECK = r"""
import sys
import numpy as np
import torch
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[2])
import adamw_oracle as A
import optim_trajectory as T
from tolerance import ELEMENTWISE_RTOL
f32 = np.float32
cases = 0
# a. 64 steps of the zoo in f64 against torch.optim.AdamW (CPU, f64, one tensor at a time): 1e-12 relative
lr, beta1, beta2, eps, wd = 0.01, 0.9, 0.999, 1e-8, 0.1
for amsgrad in (False, True):
    ws = [np.array(w, np.float64) for w in T.zoo()]
    state = [[np.zeros_like(w) for _ in range(3)] for w in ws]
    tp = [torch.tensor(w.copy(), dtype=torch.float64, requires_grad=True) for w in ws]
    opt = torch.optim.AdamW(tp, lr=lr, betas=(beta1, beta2), eps=eps, weight_decay=wd, amsgrad=amsgrad, foreach=False)
    for t in range(1, A.STEPS + 1):
        for i, w in enumerate(ws):
            g = T.gradient(t, i, w.shape).astype(np.float64)
            tp[i].grad = torch.tensor(g.copy(), dtype=torch.float64)
            g_before = g.copy()
            A.adamw_step(w, g, state[i][0], state[i][1], lr, beta1, beta2, eps, t, wd, state[i][2] if amsgrad else None)
            assert np.array_equal(g, g_before)                       # the gradient is read, not written
        opt.step()
        for i, w in enumerate(ws):
            got = tp[i].detach().numpy()
            assert np.abs(w - got).max() <= 1e-12 * max(1.0, np.abs(got).max()), (amsgrad, t, i)
    assert all(np.abs(w - w0).max() > 1e-3 for w, w0 in zip(ws[2:], T.zoo()[2:]))
    cases += 1
# b. the clip against torch.nn.utils.clip_grad_norm_.  torch computes in f64 throughout; the oracle rounds total_norm and the
# coefficient to f32 as the header states (2^-24 relative each), which ELEMENTWISE_RTOL = 1e-5 covers with room
for max_norm in (20.0, 200.0, float("inf")):
    for step in (1, 30):
        grads = [T.gradient(step, i, s).astype(np.float64) for i, s in enumerate(T.PARAM_SHAPES)]
        tp = [torch.zeros(g.shape, dtype=torch.float64, requires_grad=True) for g in grads]
        for p, g in zip(tp, grads):
            p.grad = torch.tensor(g.copy(), dtype=torch.float64)
        want = float(torch.nn.utils.clip_grad_norm_(tp, max_norm))
        mine = [g.copy() for g in grads]
        norm, coef = A.clip_grad_norm(mine + [mine[3]], max_norm)       # listed twice: counted once
        assert norm.dtype == f32 and coef.dtype == f32
        assert abs(float(norm) - want) <= ELEMENTWISE_RTOL * want
        assert (coef < 1) == (want > max_norm), (max_norm, step, coef, want)
        for p, g, g0 in zip(tp, mine, grads):
            assert np.abs(g - p.grad.numpy()).max() <= ELEMENTWISE_RTOL * np.abs(g0).max()
            if coef == 1:
                assert np.array_equal(g, g0)
        cases += 1
print("cases", cases)
"""


def test_against_torch():
    """the f64 adamw_step is torch.optim.AdamW's over 64 steps (amsgrad both ways, 1e-12 relative); clip_grad_norm is
    torch.nn.utils.clip_grad_norm_'s at three bounds and two gradient scales"""
    r = subprocess.run([sys.executable, "-c", _TORCH_CHECK, ROOT, os.path.join(ROOT, "tests")], capture_output=True, text=True)
    assert r.returncode == 0 and "cases 8" in r.stdout, r.stdout + r.stderr


def test_clip_edges():
    norm, coef = A.clip_grad_norm([], 1.0)
    assert norm == 0 and coef == 1
    g = np.array([3.0, np.nan, 4.0], f32)
    norm, coef = A.clip_grad_norm([g], 1.0)
    assert np.isnan(norm) and np.isnan(coef) and np.isnan(g).all()
    g = np.array([3.0, 4.0], f32)
    norm, coef = A.clip_grad_norm([g], 2.5)
    assert norm == 5 and coef == f32(2.5) / f32(f32(5) + f32(1e-6)) and np.array_equal(g, np.array([3.0, 4.0], f32) * coef)


@pytest.fixture(scope="module")
def runs():
    out = {}
    for name, config in A.CONFIGS.items():
        s32, s64 = {}, {}
        W32, G32 = A.reference(config, f32, stats=s32)
        W64, G64 = A.reference(config, np.float64, stats=s64)
        out[name] = (W32, G32, W64, G64, s32, s64)
    return out


@pytest.mark.parametrize("name", list(A.CONFIGS))
def test_f32_trajectory_stays_inside_the_bound_of_the_f64_one(runs, name):
    W32, G32, W64, G64, s32, s64 = runs[name]
    worst = 0.0
    for t in range(A.STEPS):
        for i in range(len(W32[t])):
            assert np.isfinite(W32[t][i]).all() and np.isfinite(W64[t][i]).all()
            assert W32[t][i].dtype == f32 and W64[t][i].dtype == np.float64
            worst = max(worst, float(np.abs(W32[t][i].astype(np.float64) - W64[t][i]).max()))
    print(f"{name}: max |w32 - w64| over {A.STEPS} steps = {worst:.3g}")
    assert worst < 1e-4                                   # as test_oracle_optim_trajectory.py: rounding is not amplified
    if A.CONFIGS[name]["max_norm"] is not None:
        # about 115 for 24 steps, about 14.3 afterwards, no step near the threshold: both precisions clip the same 24 steps, so the
        # trajectory runs the scaling and the early exit
        for s in (s32, s64):
            norms = np.array(s["norms"], np.float64)
            assert len(norms) == A.STEPS and s["clipped"] == A.CLIPPED_STEPS == 24
            assert (norms[:24] > 100).all() and (norms[:24] < 130).all() and (norms[24:] > 12).all() and (norms[24:] < 16).all()
        for t in (0, 23):
            total = np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in G32[t]))
            assert abs(total - A.MAX_NORM) < 1e-4 * A.MAX_NORM   # clipped gradients have the norm asked for
        assert all(np.array_equal(G32[40][i], T.gradient(41, i, G32[40][i].shape)) for i in range(len(G32[40])))


CASES = [(m, c) for m in A.MUTANTS for c in A.CONFIGS if A.MUTANTS[m][0](A.CONFIGS[c])]


def test_every_mutant_applies_somewhere():
    assert {m for m, _ in CASES} == set(A.MUTANTS)
    assert set(A.MUTANTS) >= {"decay_coupled", "decay_dropped", "decay_without_lr", "clip_dropped", "clip_per_parameter",
                              "twice_counted_twice", "stale_step"}
    assert any(A.CONFIGS[c]["kind"] == "sgd" for m, c in CASES if m == "clip_dropped")


@pytest.mark.parametrize("mutant,name", CASES)
def test_detection_condition(mutant, name):
    """Every wrong driver exceeds the bound by at least DETECTION_FACTOR at some step, for some parameter."""
    Wm, W32, W64 = A.mutant_runs(mutant, A.CONFIGS[name])
    worst, honest, where = 0.0, 0.0, None
    for t in range(A.STEPS):
        for i in range(len(W64[t])):
            r = T.ratio(Wm[t][i], W32[t][i], W64[t][i])
            honest = max(honest, T.ratio(W32[t][i], W32[t][i], W64[t][i]))
            if r > worst:
                worst, where = r, (t + 1, i)
    print(f"{mutant} on {name}: {worst:.3g} bounds at (step, parameter) {where}; the honest f32 run: {honest:.3g}")
    assert honest < 1.0
    assert worst >= DETECTION_FACTOR, (mutant, name, worst, where)

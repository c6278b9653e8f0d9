"""tests/dispatch_paths.py against what the library really contains (no GPU needed: the code object is read from the built
libneuronika_hip.so), against the ids tests/test_gpu_dispatch_paths.py really collects, and against the committed kernel
trace of that file.  A kernel instantiation someone adds to one of the five streaming units fails here until its row says
which test reaches it."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dispatch_paths as inv      # noqa: E402
import list_unit_kernels as luk   # noqa: E402


@pytest.fixture(scope="module")
def built():
    """{unit: [kernel, ...]} of the built library; the library is a product of build(), so its absence is a failure"""
    assert os.path.exists(luk.LIB), f"{luk.LIB} is missing: run build() (python -m neuronika_amd.build)"
    return luk.unit_kernels(inv.UNITS)


def test_units_are_the_listers_default():
    assert tuple(inv.UNITS) == tuple(luk.STREAMING_UNITS)


def test_every_unit_has_kernels(built):
    for unit in inv.UNITS:
        assert built[unit], f"no kernel of {unit} found in the library: the symbol listing is broken"
        for fn in luk.source_kernels(unit):
            assert any(re.sub(r"<.*$", "", k) == fn for k in built[unit]), f"{unit}: `{fn}` is defined but never instantiated"


def test_plain_demangler_agrees_with_the_program(built):
    """the lister decodes names itself where no demangler program exists: both ways must give the same table"""
    mangled = sorted({k for elf in luk.code_objects() for k in luk.kernel_symbols(elf)})
    plain = {luk.trace_name(d) for d in (luk._demangle_plain(m) for m in mangled) if d}
    for unit in inv.UNITS:
        assert set(built[unit]) <= plain, f"{unit}: not decoded: {sorted(set(built[unit]) - plain)}"


def test_kernel_names_belong_to_one_unit():
    """a kernel is attributed to a unit by its function name, so no other source may define the same name"""
    mine = {fn: u for u in inv.UNITS for fn in luk.source_kernels(u)}
    assert sum(len(luk.source_kernels(u)) for u in inv.UNITS) == len(mine), "two streaming units define the same kernel name"
    for f in sorted(os.listdir(luk.CSRC)):
        if f.endswith((".hip", ".h")) and f not in inv.UNITS:
            clash = set(mine) & luk.source_kernels(f)
            assert not clash, f"{f} also defines {sorted(clash)}"


def test_every_kernel_has_a_row_and_every_row_a_kernel(built):
    have = {k for ks in built.values() for k in ks}
    rows = [r.kernel for r in inv.ROWS]
    dup = sorted({k for k in rows if rows.count(k) > 1})
    assert not dup, f"kernels with more than one row: {dup}"
    missing = sorted(have - set(rows))
    assert not missing, "kernel instantiations without a row in tests/dispatch_paths.py (say which test reaches them): " + "; ".join(missing)
    stale = sorted(set(rows) - have)
    assert not stale, "rows of tests/dispatch_paths.py that name no kernel of the built library: " + "; ".join(stale)


def test_rows_are_well_formed():
    for r in inv.ROWS:
        given = [bool(r.tests), bool(r.covered_by), bool(r.unreachable)]
        assert sum(given) == 1, f"{r.kernel}: exactly one of tests / covered_by / unreachable"
        assert r.entry and r.condition, f"{r.kernel}: entry point and dispatch condition are required"


def _collected(path, extra=()):
    r = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider", path, *extra],
                       cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return {l.split("::", 1)[1] for l in r.stdout.splitlines() if "::" in l}


def test_named_tests_exist():
    ids = _collected(inv.TEST_FILE)
    assert ids, "nothing collected from " + inv.TEST_FILE
    for r in inv.ROWS:
        for t in r.tests:
            assert t in ids, f"{r.kernel}: `{t}` is not a test id of {inv.TEST_FILE}"
    for r in inv.ROWS:
        if r.covered_by:
            path, _, tid = r.covered_by.partition("::")
            assert os.path.exists(os.path.join(ROOT, path)), f"{r.kernel}: covered_by names no file: {r.covered_by}"
            assert tid in _collected(path), f"{r.kernel}: covered_by names no collected test: {r.covered_by}"


def test_traced_run_entered_every_attributed_kernel():
    """the committed summary of `rocprofv3 --kernel-trace` over the new file lists every kernel a row attributes to it"""
    path = os.path.join(ROOT, inv.TRACE_SUMMARY)
    assert os.path.exists(path), inv.TRACE_SUMMARY + " is missing"
    traced = set(re.findall(r"^\| `([^`]+)` \|", open(path).read(), re.M))
    absent = sorted(r.kernel for r in inv.ROWS if r.tests and r.kernel not in traced)
    assert not absent, f"attributed to {inv.TEST_FILE} but absent from its kernel trace: " + "; ".join(absent)
    entered = sorted(r.kernel for r in inv.ROWS if r.unreachable and r.kernel in traced)
    assert not entered, "declared unreachable, yet the trace holds them: " + "; ".join(entered)

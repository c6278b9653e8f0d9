"""The dispatch inventories - tests/dispatch_paths.py (the five streaming units) and tests/dispatch_paths_mfma.py (nk_gemm, nk_conv,
nk_attention) - against what the library really contains (no GPU needed: the code objects are read from the built
libneuronika_hip.so), against the ids their GPU test files really collect, and against the committed kernel traces of those
files.  Every check runs over every inventory (`over_inventories`: one test per check, under the id it has always had).  A kernel instantiation someone adds to an inventoried unit fails here until its
row says which test reaches it; a translation unit someone adds fails until it has rows or an entry in NOT_INVENTORIED."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dispatch_paths              # noqa: E402
import dispatch_paths_mfma         # noqa: E402
import list_unit_kernels as luk    # noqa: E402

INVENTORIES = (dispatch_paths, dispatch_paths_mfma)
_BUILT = {}


def _built(inv):
    """{unit: [kernel, ...]} of the built library; the library is a product of build(), so its absence is a failure"""
    assert os.path.exists(luk.LIB), f"{luk.LIB} is missing: run build() (python -m neuronika_amd.build)"
    if inv.__name__ not in _BUILT:
        _BUILT[inv.__name__] = luk.unit_kernels(inv.UNITS)
    return _BUILT[inv.__name__]


def over_inventories(check):
    """`check(inv)` as ONE test under its own name, run over every inventory module: the test ids stay what they were when there was
    one inventory, a second inventory cannot be left out of a check, and a failure in one inventory does not hide the next one's"""
    def test():
        failed = []
        for inv in INVENTORIES:
            try:
                check(inv)
            except AssertionError as e:
                failed.append(f"tests/{inv.__name__}.py: {e}")
        assert not failed, "\n".join(failed)
    test.__name__, test.__doc__, test.__module__ = check.__name__, check.__doc__, check.__module__
    return test


def test_units_are_the_listers_default():
    assert tuple(dispatch_paths.UNITS) == tuple(luk.STREAMING_UNITS)


def test_units_are_translation_units_and_no_unit_is_listed_twice():
    listed = [u for m in INVENTORIES for u in m.UNITS] + [u for u, _ in dispatch_paths_mfma.NOT_INVENTORIED]
    assert len(listed) == len(set(listed)), f"a unit appears in two lists: {sorted(u for u in listed if listed.count(u) > 1)}"
    assert set(listed) <= set(luk.all_units()), f"not a translation unit of the library: {sorted(set(listed) - set(luk.all_units()))}"
    for u, reason in dispatch_paths_mfma.NOT_INVENTORIED:
        assert reason.strip(), f"{u}: NOT_INVENTORIED needs a one-line reason"


def test_every_kernel_of_the_library_is_accounted_for():
    """library-wide: a kernel symbol belongs to an inventoried unit or to a unit named in NOT_INVENTORIED; a translation unit that
    arrives without rows and without an entry there fails here, and so does a code object no source file explains"""
    assert os.path.exists(luk.LIB), f"{luk.LIB} is missing: run build() (python -m neuronika_amd.build)"
    listed = [u for m in INVENTORIES for u in m.UNITS] + [u for u, _ in dispatch_paths_mfma.NOT_INVENTORIED]
    missing = sorted(set(luk.all_units()) - set(listed))
    assert not missing, "translation units with neither an inventory nor an entry in NOT_INVENTORIED: " + ", ".join(missing)
    everything = {k for ks in luk.object_kernels() for k in ks}
    by_unit = luk.unit_kernels(tuple(listed))
    claimed = [k for ks in by_unit.values() for k in ks]
    assert len(claimed) == len(set(claimed)), "a kernel is attributed to two units"
    orphans = sorted(everything - set(claimed))
    assert not orphans, "kernels of the library that no listed unit defines: " + "; ".join(orphans)
    rows = {r.kernel for m in INVENTORIES for r in m.ROWS}
    for m in INVENTORIES:
        for u in m.UNITS:
            assert set(by_unit[u]) <= rows, f"{u}: kernels without a row: {sorted(set(by_unit[u]) - rows)}"


@over_inventories
def test_every_unit_has_kernels(inv):
    built = _built(inv)
    for unit in inv.UNITS:
        assert built[unit], f"no kernel of {unit} found in the library: the symbol listing is broken"
        for fn in luk.source_kernels(unit):
            assert any(re.sub(r"<.*$", "", k) == fn for k in built[unit]), f"{unit}: `{fn}` is defined but never instantiated"


@over_inventories
def test_plain_demangler_agrees_with_the_program(inv):
    built = _built(inv)
    """the lister decodes names itself where no demangler program exists: both ways must give the same table"""
    mangled = sorted({k for elf in luk.code_objects() for k in luk.kernel_symbols(elf)})
    plain = {luk.trace_name(d) for d in (luk._demangle_plain(m) for m in mangled) if d}
    for unit in inv.UNITS:
        assert set(built[unit]) <= plain, f"{unit}: not decoded: {sorted(set(built[unit]) - plain)}"


@over_inventories
def test_kernel_names_belong_to_one_unit(inv):
    """a code object is matched to its unit by function names (the unit's own file and the headers it includes), so no other source
    may define the same name: not another inventoried unit, not any other translation unit with its headers, not a stray header"""
    mine = {fn: u for u in inv.UNITS for fn in luk.source_kernels(u)}
    assert sum(len(luk.source_kernels(u)) for u in inv.UNITS) == len(mine), "two units of one inventory define the same kernel name"
    own = {f for u in inv.UNITS for f in luk.unit_sources(u)}
    for f in sorted(os.listdir(luk.CSRC)):
        if f.endswith(".hip") and f not in inv.UNITS:
            clash = set(mine) & luk.source_kernels(f)
        elif f.endswith(".h") and f not in own:
            clash = set(mine) & luk.file_kernels(os.path.join(luk.CSRC, f))
        else:
            continue
        assert not clash, f"{f} also defines {sorted(clash)}"


@over_inventories
def test_every_kernel_has_a_row_and_every_row_a_kernel(inv):
    built = _built(inv)
    have = {k for ks in built.values() for k in ks}
    rows = [r.kernel for r in inv.ROWS]
    dup = sorted({k for k in rows if rows.count(k) > 1})
    assert not dup, f"kernels with more than one row: {dup}"
    missing = sorted(have - set(rows))
    assert not missing, f"kernel instantiations without a row in tests/{inv.__name__}.py (say which test reaches them): " + "; ".join(missing)
    stale = sorted(set(rows) - have)
    assert not stale, f"rows of tests/{inv.__name__}.py that name no kernel of the built library: " + "; ".join(stale)


@over_inventories
def test_rows_are_well_formed(inv):
    for r in inv.ROWS:
        given = [bool(r.tests), bool(r.covered_by), bool(r.unreachable)]
        assert sum(given) == 1, f"{r.kernel}: exactly one of tests / covered_by / unreachable"
        assert r.entry and r.condition, f"{r.kernel}: entry point and dispatch condition are required"


_COLLECTED = {}


def _collected(path, extra=()):
    if (path, tuple(extra)) not in _COLLECTED:
        _COLLECTED[path, tuple(extra)] = _collect(path, extra)
    return _COLLECTED[path, tuple(extra)]


def _collect(path, extra=()):
    r = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider", path, *extra],
                       cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return {l.split("::", 1)[1] for l in r.stdout.splitlines() if "::" in l}


@over_inventories
def test_named_tests_exist(inv):
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


@over_inventories
def test_traced_run_entered_every_attributed_kernel(inv):
    """the committed summary of `rocprofv3 --kernel-trace` over the new file lists every kernel a row attributes to it"""
    path = os.path.join(ROOT, inv.TRACE_SUMMARY)
    assert os.path.exists(path), inv.TRACE_SUMMARY + " is missing"
    traced = set(re.findall(r"^\| `([^`]+)` \|", open(path).read(), re.M))
    absent = sorted(r.kernel for r in inv.ROWS if r.tests and r.kernel not in traced)
    assert not absent, f"attributed to {inv.TEST_FILE} but absent from its kernel trace: " + "; ".join(absent)
    entered = sorted(r.kernel for r in inv.ROWS if r.unreachable and r.kernel in traced)
    assert not entered, "declared unreachable, yet the trace holds them: " + "; ".join(entered)

"""The ledger tests/streaming_sites.py against the source (no GPU, no library): the switch's own line, the call sites, the test ids."""
import os
import re
import subprocess
import sys
from collections import Counter

import streaming_sites as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "neuronika_amd", "csrc")
CALL = "nk_streams_past_cache("


def _argument(text, start):
    """the text between the parenthesis that opens at start - 1 and its partner"""
    depth, i = 1, start
    while depth:
        depth += {"(": 1, ")": -1}.get(text[i], 0)
        i += 1
    return text[start:i - 1].strip()


def source_sites():
    """[(file, expression)] of every call in csrc/, comments and the definition itself left out"""
    found = []
    for name in sorted(os.listdir(CSRC)):
        if not name.endswith((".hip", ".h")):
            continue
        for line in open(os.path.join(CSRC, name)).read().splitlines():
            code = re.sub(r"//.*", "", line)
            if "static inline bool " + CALL in code:
                continue
            at = code.find(CALL)
            while at >= 0:
                found.append((name, _argument(code, at + len(CALL))))
                at = code.find(CALL, at + 1)
    return found


def test_the_switch_is_384_mib_and_strict():
    text = open(os.path.join(CSRC, "nk_common.h")).read()
    assert text.count(SS.SOURCE_LINE) == 1
    assert "size_t(384) << 20" in SS.SOURCE_LINE and "bytes_touched > (" in SS.SOURCE_LINE
    assert SS.THRESHOLD == 384 << 20 == 402653184


def test_every_call_site_has_an_entry():
    src, led = Counter(source_sites()), Counter((s.file, s.expr) for s in SS.SITES)
    assert src == led, {"in the source only": sorted((src - led).elements()), "in the ledger only": sorted((led - src).elements())}
    assert sum(src.values()) == len(SS.SITES) == 19


def test_every_entry_crosses_by_its_own_arithmetic():
    for s in SS.SITES:
        assert s.bytes(**s.shape) > SS.THRESHOLD, (s.file, s.entry, s.bytes(**s.shape))
        assert s.switch in ("run-time bit",) or s.switch.startswith("template parameter"), s.switch
        assert s.passes and s.largest and isinstance(s.largest_bytes, int)
    # the two norms' fullsize calls and the activation's assign form sit on the threshold itself: `>` leaves the bit off
    assert SS.site("nk_layer_norm_bwd /").largest_bytes == SS.THRESHOLD
    assert (1 << 25) * 12 == SS.THRESHOLD


_COLLECTED = {}


def _collected(path):
    if path not in _COLLECTED:
        r = subprocess.run([sys.executable, "-m", "pytest", "--collect-only", "-q", "-p", "no:cacheprovider", path], cwd=ROOT, capture_output=True,
                           text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        _COLLECTED[path] = [l.strip() for l in r.stdout.splitlines() if "::" in l]
    return _COLLECTED[path]


def test_every_entry_names_a_collected_test():
    for s in SS.SITES:
        path = s.test.split("::")[0]
        ids = _collected(path)
        # a parametrised test is named with its case or by its function: then every case counts
        assert any(i == s.test or i.startswith(s.test + "[") for i in ids), (s.entry, s.test)

"""CPU: every header a kernel source includes is an input of its object's digest (mindtheedge_amd/_build.py), so editing a header recompiles."""
import os
import re
import shutil

import pytest

from mindtheedge_amd import _build

INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)


def _included(path, seen=None):
    """paths of the project headers `path` includes, transitively"""
    seen = set() if seen is None else seen
    with open(path) as f:
        for name in INCLUDE.findall(f.read()):
            h = os.path.normpath(os.path.join(os.path.dirname(path), name))
            if h not in seen:
                seen.add(h)
                _included(h, seen)
    return seen


@pytest.mark.parametrize("source", _build.SOURCES)
def test_every_included_header_is_a_digest_input(source):
    inputs = set(_build.headers())
    needed = _included(os.path.join(_build.CSRC, source))
    assert needed, source                                       # every source includes common.hpp at least
    assert all(os.path.exists(h) for h in needed), needed
    assert needed <= inputs, sorted(needed - inputs)


def test_one_changed_header_byte_changes_the_digest(tmp_path):
    copy = tmp_path / "csrc"
    copy.mkdir()
    for f in os.listdir(_build.CSRC):
        if f.endswith((".hpp", ".hip")):
            shutil.copy(os.path.join(_build.CSRC, f), copy / f)
    hdrs = _build.headers(str(copy))
    assert [os.path.basename(h) for h in hdrs] == [os.path.basename(h) for h in _build.headers()]
    flags = " ".join(_build.FLAGS)
    digest = lambda s: _build._digest([str(copy / s)] + hdrs, flags)
    before = {s: digest(s) for s in _build.SOURCES}
    assert before == {s: _build._digest([os.path.join(_build.CSRC, s)] + _build.headers(), flags) for s in _build.SOURCES}     # a faithful copy
    for h in hdrs:
        data = open(h, "rb").read()
        with open(h, "wb") as f:
            f.write(data[:-1] + bytes([data[-1] ^ 1]))
        users = [s for s in _build.SOURCES if os.path.join(_build.CSRC, os.path.basename(h)) in _included(os.path.join(_build.CSRC, s))]
        assert users, h                                         # no orphan header
        for s in users:
            assert digest(s) != before[s], (s, h)
        with open(h, "wb") as f:
            f.write(data)
    assert {s: digest(s) for s in _build.SOURCES} == before

"""Every file a translation unit includes is part of the build's dependency list (zflac_amd/build.py
DEPS), so of the source fingerprint: a header left out would let two different kernel sets report
the same build id, and every measurement under profiles/ leans on that id. Regex only, no compiler."""
from __future__ import annotations

import os
import re

from zflac_amd import build

INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)
INCLUDE_DIRS = (os.path.join(build.ROOT, "include"),)  # -I of every compile (build.build)


def resolve(name: str, includer: str) -> str:
    for d in (os.path.dirname(includer),) + INCLUDE_DIRS:
        p = os.path.normpath(os.path.join(d, name))
        if os.path.exists(p):
            return p
    raise AssertionError(f'{includer}: #include "{name}" not found')


def include_closure(sources):
    seen, todo = set(), [os.path.normpath(s) for s in sources]
    while todo:
        f = todo.pop()
        if f in seen:
            continue
        seen.add(f)
        with open(f, encoding="utf-8") as fh:
            todo += [resolve(n, f) for n in INCLUDE.findall(fh.read())]
    return seen


def test_every_included_file_is_a_dependency():
    deps = {os.path.normpath(d) for d in build.DEPS}
    missing = sorted(os.path.relpath(f, build.ROOT) for f in include_closure(build.SOURCES) - deps)
    assert not missing, f"included but not in build.DEPS (so not in the source fingerprint): {missing}"


def test_decode_headers_belong_to_the_decode_units_only():
    decode = {os.path.normpath(h) for h in build.DECODE_HEADERS}
    assert len(decode) > 1, "csrc/decode/*.h not found"
    for src in build.SOURCES:
        if src.endswith("abi.cpp"):  # embeds the fingerprint of every source
            continue
        closure = include_closure([src])
        obj_deps = {os.path.normpath(d) for d in build._obj_deps(src)}
        assert closure <= obj_deps, f"{os.path.basename(src)}: {sorted(closure - obj_deps)} not in its object's dependencies"
        assert bool(decode & obj_deps) == ("decode_k" in os.path.basename(src))


def test_basenames_are_unique():
    # source_fingerprint() names each file by its basename
    names = [os.path.basename(d) for d in build.DEPS]
    assert len(set(names)) == len(names), sorted(n for n in set(names) if names.count(n) > 1)

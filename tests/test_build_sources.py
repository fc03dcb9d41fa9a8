"""The build's source lists cover csrc: a new kernel file that is not compiled,
or a header whose edit does not rebuild the extension, is caught here and not
by a stale binary on a GPU box."""

from __future__ import annotations

import os
import re

from sparktorch_amd.ops import build


def _csrc(ext):
    return sorted(f for f in os.listdir(build.CSRC) if f.endswith(ext))


def test_build_lists_cover_csrc():
    # every kernel file is compiled
    assert _csrc(".hip") == sorted(build.HIP_SOURCES)
    # every source and every header gates the mtime-checked rebuild
    deps = set(build.build_dependencies())
    headers = _csrc(".h")
    for f in headers + build.HIP_SOURCES + build.CPP_SOURCES:
        assert os.path.join(build.CSRC, f) in deps, f


def _read(name):
    with open(os.path.join(build.CSRC, name)) as fh:
        return fh.read()


def test_c_linkage_interface_is_declared_once():
    """launchers.h is the one declaration of every C-linkage function: each
    .hip includes it (so the compiler holds the definition to it) and
    bindings.cpp declares nothing of its own."""
    header = re.sub(r"//[^\n]*", "", _read("launchers.h"))
    block = header[header.index('extern "C" {'):]
    declared = set(re.findall(r"\b(\w+)\s*\(", block))
    assert "launch_gemm_bf16" in declared
    for f in build.HIP_SOURCES:
        src = _read(f)
        assert '#include "launchers.h"' in src, f
        defined = re.findall(r'^extern "C"[^({;]*?\b(\w+)\s*\(', src, re.M)
        for name in defined:
            assert name in declared, "%s defines %s, launchers.h does not declare it" % (f, name)
        # a braced block would hide its definitions from the scan above
        assert 'extern "C" {' not in src, f
    for f in build.CPP_SOURCES:
        assert 'extern "C"' not in _read(f), f

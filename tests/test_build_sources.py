"""The build's source lists cover csrc: a new kernel file that is not compiled,
or a header whose edit does not rebuild the extension, is caught here and not
by a stale binary on a GPU box."""

from __future__ import annotations

import os

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

"""CPU-only tests of the graph cache (csrc/graph_cache.h, graph_cache.cpp): include/fdx.h, flashdeconv_amd/_lib.py and the library
agree on its entry, which validates without a device, and the HIP-free container passes its stand-alone program under
the address and undefined-behaviour sanitizers.  No kernel is launched here."""
import ctypes
import os
import re

import pytest

from conftest import ROOT

NEW = {"fdx_graph_cache_stats": 1}


def _declarations():
    text = open(os.path.join(ROOT, "include", "fdx.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\bint\s+(fdx_graph_cache_[a-z_]+)\s*\(([^)]*)\)\s*;", text)}


def test_header_binding_and_library_agree_on_the_graph_cache_entry():
    from flashdeconv_amd import _lib
    lib = _lib.load()
    decl = _declarations()
    assert set(decl) == set(NEW)
    for name, n_args in NEW.items():
        assert hasattr(lib, name), f"{name} is not exported by libfdx.so"
        restype, argtypes = _lib.SIGNATURES[name]
        assert restype is ctypes.c_int
        assert len(argtypes) == n_args == len(decl[name].split(",")), name


def test_graph_cache_stats_validates_without_a_device():
    from flashdeconv_amd import _lib
    lib = _lib.load()
    out = (ctypes.c_int64 * 4)(-1, -1, -1, -1)
    assert lib.fdx_graph_cache_stats(out) == 0
    assert all(v >= 0 for v in out) and out[2] <= 2 * 64            # at most two entries per device
    assert lib.fdx_graph_cache_stats(None) != 0 and b"null output" in lib.fdx_last_error()


def test_graph_cache_container_under_address_and_ub_sanitizers():
    """`make -C flashdeconv_amd/csrc asan-host` builds csrc/hosttest/graph_cache_asan.cpp (its own main, g++ -fsanitize=address,undefined,
    never loaded into Python) and runs it: key equality on every scalar, least-recently-used order, the per-device cap, reference
    counts across eviction and clear, four threads finding and inserting concurrently."""
    import shutil
    import subprocess
    if not shutil.which("g++") or not shutil.which("make"):
        pytest.skip("no g++ / make")
    r = subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "flashdeconv_amd", "csrc"), "asan-host"], capture_output=True, text=True,
                       timeout=300)
    if r.returncode != 0 and ("cannot find -lasan" in r.stderr or "libasan" in r.stderr):
        pytest.skip("no sanitizer runtime")
    assert r.returncode == 0, r.stdout + r.stderr
    assert "graph cache: ok under the sanitizers" in r.stdout

"""CPU checks of the radius pair matcher's boundary: both libraries export the two entry points the header declares, the
kernels behind them touch no scratch memory, and the drop-in C++ matcher has the two-set radiusMatch the reference's callers use."""
import ctypes
import os
import re
import subprocess

import pytest

import ethzasl_brisk_amd as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("brisk_hip_match_radius_pairs_device", "brisk_hip_match_radius_device")


def test_both_libraries_export_the_radius_pair_matcher():
    from ethzasl_brisk_amd import build
    hdr = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    declared = set(re.findall(r"\b(brisk_hip_[a-z_0-9]+)\s*\(", hdr))
    for lib in (build.build(), build.build_release()):
        L = ctypes.CDLL(lib)
        for s in NEW:
            assert s in declared, s
            assert s in B.ABI_SYMBOLS, s
            assert hasattr(L, s), (lib, s)


def test_python_context_has_the_radius_calls():
    assert callable(B.Context.match_radius_pairs) and callable(B.Context.match_radius_device)


def test_radius_pair_kernels_use_no_scratch():
    from ethzasl_brisk_amd import build
    build.build()
    res = build.kernel_resources()
    if not res:
        pytest.skip("the objects were not compiled here (no resource remarks beside them)")
    ks = {k: v for k, v in res.items() if "k_match_radius_pairs" in k}
    assert len(ks) >= 8                                             # pair and single-set kernels, four descriptor sizes each
    for k, v in ks.items():
        assert v["scratch"] == 0, (k, v)


def build_program():
    """tests/cpp/test_radius_match_two_sets.cc against the non-OpenCV flavour of the drop-in headers, the way
    tests/test_cpp_classes.py builds its programs"""
    from ethzasl_brisk_amd import build
    build.build()
    src = os.path.join(ROOT, "tests", "cpp", "test_radius_match_two_sets.cc")
    out = os.path.join(ROOT, "tests", "cpp", "test_radius_match_two_sets")
    hdrs = [os.path.join(d, f) for d, _, fs in os.walk(os.path.join(ROOT, "include")) for f in fs]
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in [src] + hdrs):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-pthread", "-I" + os.path.join(ROOT, "include"), "-o", out, src,
                               "-L" + os.path.join(ROOT, "ethzasl_brisk_amd"), "-lbrisk_hip",
                               "-Wl,-rpath," + os.path.join(ROOT, "ethzasl_brisk_amd"), "-Wl,-rpath,/opt/rocm/lib"])
    return out


def test_two_set_radius_match_compiles_without_opencv():
    b = build_program()
    r = subprocess.run([b], capture_output=True, text=True)
    if B.load_library().brisk_hip_device_count() > 0:
        assert r.returncode == 0 and "two-set radiusMatch OK" in r.stdout, r.stdout
    else:
        assert r.returncode == 2 and "brisk_hip_create failed" in r.stdout   # no CPU fallback behind the class

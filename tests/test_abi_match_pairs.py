"""CPU checks of the batch matcher's boundary: both libraries export the two entry points the header declares, and the
kernel behind them touches no scratch memory."""
import ctypes
import os
import re

import pytest

import ethzasl_brisk_amd as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("brisk_hip_batch_desc_set", "brisk_hip_match_knn_pairs_device")


def test_both_libraries_export_the_pair_matcher():
    from ethzasl_brisk_amd import build
    hdr = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    declared = set(re.findall(r"\b(brisk_hip_[a-z_0-9]+)\s*\(", hdr))
    for lib in (build.build(), build.build_release()):
        L = ctypes.CDLL(lib)
        for s in NEW:
            assert s in declared, s
            assert s in B.ABI_SYMBOLS, s
            assert hasattr(L, s), (lib, s)
    for name in ("brisk_hip_desc_set", "brisk_hip_pair_spec"):
        assert re.search(r"typedef struct %s \{" % name, hdr), name


def test_structures_match_the_header_layout():
    """DescSet / PairSpec as the C compiler lays the header's structs out (LP64: pointers and long 8 bytes)"""
    assert ctypes.sizeof(B.DescSet) == 40 and B.DescSet.frame_pitch.offset == 24 and B.DescSet.frames.offset == 36
    assert ctypes.sizeof(B.PairSpec) == 32 and B.PairSpec.d_pairs.offset == 24


def test_pair_kernels_use_no_scratch():
    from ethzasl_brisk_amd import build
    build.build()
    res = build.kernel_resources()
    if not res:
        pytest.skip("the objects were not compiled here (no resource remarks beside them)")
    ks = {k: v for k, v in res.items() if "k_match_knn_pairs" in k}
    assert ks
    for k, v in ks.items():
        assert v["scratch"] == 0, (k, v)

"""CPU proof that the list form of the tie kernel's static replay step computes what the unrolled form computes.

tests/emul/brisk_emul_tie_list.cpp runs the `__host__ __device__` functions of brisk_device_detect.h: brisk_state_static_list
walks the candidates of the tie's 9 x 9 window (entries 0 ... 40 with a score) where brisk_state_static walks the 24 neighbours
of the pixel.  k_tie_resolve takes the list form for windows of up to BRISK_TIE_LIST_CAP candidates, so `packed` and `dynmask`
must be equal bit for bit - the resolve step and the decision read them.  The functions are pure: the windows are random and
need not be states a frame can reach.  No GPU needed.
"""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle_lib import ROOT

EMUL_DIR = os.path.join(ROOT, "tests", "emul")
CSRC = os.path.join(ROOT, "ethzasl_brisk_amd", "csrc")
_lib = None


def lib():
    global _lib
    if _lib is None:
        so = os.path.join(EMUL_DIR, "libbrisk_emul_tie_list.so")
        src = os.path.join(EMUL_DIR, "brisk_emul_tie_list.cpp")
        deps = [src] + [os.path.join(CSRC, f) for f in ("brisk_common.h", "brisk_device_detect.h")]
        if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
            subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-w", "-o", so, src])
        L = C.CDLL(so)
        L.tl_list_mismatches.argtypes = [C.c_uint, C.c_int, C.c_void_p]
        _lib = L
    return _lib


def test_cap_leaves_room_on_both_sides():
    """the cap lies inside 1 ... 40: both forms run, and the cases `cap` and `cap + 1` below exist"""
    assert 1 <= lib().tl_cap() <= 39


def test_list_form_equals_unrolled_form():
    """160 000 random windows x 33 slots = 5.3 M (window, pixel slot) cases, each with both values of `own` and the three
    used combinations of float_patch / pass_touch2x2, plus the slot wrappers: equal packed, equal dynmask.  The windows carry
    arbitrary D, probe count, status, E5 and TOUCH bits, 1 (the tie alone) ... 41 candidates in entries 0 ... 40 with the cap
    and cap + 1 drawn on purpose, candidates at entries 39 and 40, ties in rows and columns 3 and 4 (and their mirror images),
    entries outside the image."""
    L = lib()
    cap = L.tl_cap()
    nwin = 160000
    out = np.zeros(8 + 42, np.int64)
    L.tl_list_mismatches(29, nwin, out.ctypes.data)
    hist = out[8:]
    print("cases %d, not final %d, with open events %d, entry 39 in %d windows, outside entries in %d, rows / columns 3-4 in %d"
          % (out[1], out[2], out[3], out[4], out[5], out[6]))
    print("candidates per window:", hist.tolist())
    assert out[0] == 0
    assert out[1] == nwin * 3 * 33 * 3 and nwin * 33 >= 5000000
    # the sample reaches what it claims to
    assert hist[0] == 0 and hist.sum() == nwin
    assert all(hist[k] > 1000 for k in range(1, cap + 2)), hist
    assert hist[41] > 1000
    assert out[2] > out[1] // 10 and out[3] > out[1] // 100
    assert out[4] > nwin // 10 and out[5] > nwin // 10 and out[6] > nwin // 10

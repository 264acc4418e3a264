"""CPU checks of the gated pair matchers' boundary: both libraries export the three entry points the header declares, Python has
the calls, the gated kernels touch no scratch memory while the ungated ones are still there, and the gate predicate - the very
function the kernels call, built here for the host - agrees with a numpy float32 restatement."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import ethzasl_brisk_amd as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("brisk_hip_batch_kp_set", "brisk_hip_match_knn_pairs_gated_device", "brisk_hip_match_radius_pairs_gated_device")


def test_both_libraries_export_the_gated_matchers():
    from ethzasl_brisk_amd import build
    hdr = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    declared = set(re.findall(r"\b(brisk_hip_[a-z_0-9]+)\s*\(", hdr))
    for lib in (build.build(), build.build_release()):
        L = ctypes.CDLL(lib)
        for s in NEW:
            assert s in declared, s
            assert s in B.ABI_SYMBOLS, s
            assert hasattr(L, s), (lib, s)
    for t in ("brisk_hip_kp_set", "brisk_hip_match_gate"):
        assert re.search(r"typedef struct %s\b" % t, hdr), t


def test_python_has_the_gate():
    assert callable(B.Context.batch_kp_set)
    for fn in (B.Context.match_knn_pairs, B.Context.match_radius_pairs):
        par = inspect.signature(fn).parameters
        for name in ("gate", "query_kps", "train_kps"):
            assert name in par and par[name].default is None, (fn.__name__, name)
    assert ctypes.sizeof(B.MatchGate) == 20 and ctypes.sizeof(B.KpSet) == 16
    g = B.MatchGate.all_pass()
    assert g.dx_min == -np.inf and g.dx_max == np.inf and g.dy_min == -np.inf and g.dy_max == np.inf and g.max_octave_diff == -1


def test_gated_kernels_use_no_scratch_and_the_ungated_ones_remain():
    from ethzasl_brisk_amd import build
    build.build()
    res = build.kernel_resources()
    if not res:
        pytest.skip("the objects were not compiled here (no resource remarks beside them)")
    gated = {k: v for k, v in res.items() if "k_match_knn_pairs_gated" in k or "k_match_radius_pairs_gated" in k}
    assert len(gated) == 12                     # k-NN with and without the cross check, radius; four descriptor sizes each
    for k, v in gated.items():
        assert v["scratch"] == 0, (k, v)
    ungated_knn = [k for k in res if "k_match_knn_pairs" in k and "gated" not in k]
    ungated_radius = [k for k in res if "k_match_radius_pairs" in k and "gated" not in k and "pairs_one" not in k]
    assert len(ungated_knn) == 8 and len(ungated_radius) == 4


# ---- the predicate ------------------------------------------------------------------------------------------------------------

def build_program():
    """tests/cpp/test_match_gate.cc: plain host C++ around csrc/brisk_match_gate.h (no HIP, no library)"""
    src = os.path.join(ROOT, "tests", "cpp", "test_match_gate.cc")
    hdr = os.path.join(ROOT, "ethzasl_brisk_amd", "csrc", "brisk_match_gate.h")
    out = os.path.join(ROOT, "tests", "cpp", "test_match_gate")
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in (src, hdr)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-I" + os.path.dirname(hdr), "-o", out, src])
    return out


def restated(rec):
    """the header's words in numpy float32: one subtraction each, float32 compares, the octave difference in exact integers"""
    f, i = rec.view(np.float32), rec.view(np.int32).astype(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = f[:, 8] - f[:, 5], f[:, 9] - f[:, 6]
        assert dx.dtype == np.float32
        pos = (f[:, 0] <= dx) & (dx <= f[:, 1]) & (f[:, 2] <= dy) & (dy <= f[:, 3])
    m = i[:, 4]
    return pos & ((m < 0) | (np.abs(i[:, 10] - i[:, 7]) <= m))


def gate_records():
    rng = np.random.default_rng(2024)
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    recs = []

    def add(gate, q, t):
        r = np.zeros(11, np.uint32)
        r[0:4] = np.array(gate[:4], np.float32).view(np.uint32)
        r[4] = np.array(gate[4], np.int32).view(np.uint32)
        r[5:7] = np.array(q[:2], np.float32).view(np.uint32)
        r[7] = np.array(q[2], np.int32).view(np.uint32)
        r[8:10] = np.array(t[:2], np.float32).view(np.uint32)
        r[10] = np.array(t[2], np.int32).view(np.uint32)
        recs.append(r)

    gates = [(-40, 40, -40, 40, 1), (-64, 0, -2, 2, -1), (-inf, inf, -inf, inf, -1), (-inf, 0, -2, inf, 0), (0, 0, 0, 0, 0),
             (-0.0, 0.0, -0.0, 0.0, 1), (nan, 40, -40, 40, 1), (-40, 40, -40, nan, -1), (-8, 8, -8, 8, 2), (5, -5, -1, 1, -1),
             (-40, 40, -40, 40, 2 ** 31 - 1), (-40, 40, -40, 40, -(2 ** 31))]
    special = [0.0, -0.0, 1.0, 40.0, -40.0, 64.0, 2.0, 0.5, 1e-3, 1919.75, inf, -inf, nan, 3.4e38, -3.4e38, 1e-40]
    octs = [0, 1, 2, 3, -1, 7, 2 ** 31 - 1, -(2 ** 31)]
    for g in gates:
        for _ in range(300):
            # coordinates on a quarter-pixel grid inside a window a little wider than the gates: differences hit the bounds exactly
            q = (rng.integers(0, 400) / 4, rng.integers(0, 400) / 4, int(rng.integers(0, 4)))
            t = (q[0] + rng.integers(-330, 331) / 4, q[1] + rng.integers(-170, 171) / 4, int(rng.integers(0, 4)))
            add(g, q, t)
        for _ in range(60):                                          # equal-to-bound differences, on purpose
            q = (float(rng.integers(0, 1000)), float(rng.integers(0, 1000)), int(rng.integers(0, 4)))
            dx = [g[0], g[1], 0.0][rng.integers(0, 3)]
            dy = [g[2], g[3], 0.0][rng.integers(0, 3)]
            dx, dy = (0.0 if not np.isfinite(dx) else dx), (0.0 if not np.isfinite(dy) else dy)
            add(g, q, (q[0] + dx, q[1] + dy, q[2] + int(rng.integers(-2, 3))))
        for _ in range(120):                                         # infinities, NaN, negative zero, huge values, extreme octaves
            q = (special[rng.integers(0, len(special))], special[rng.integers(0, len(special))], octs[rng.integers(0, len(octs))])
            t = (special[rng.integers(0, len(special))], special[rng.integers(0, len(special))], octs[rng.integers(0, len(octs))])
            add(g, q, t)
    return np.stack(recs)


def test_the_predicate_agrees_with_its_restatement(tmp_path):
    rec = gate_records()
    assert len(rec) >= 3000
    path = tmp_path / "gate_records.bin"
    rec.astype("<u4").tofile(path)
    r = subprocess.run([build_program(), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = np.array([c == "1" for c in r.stdout.strip()])
    want = restated(rec)
    assert len(got) == len(want)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (len(bad), rec[bad[:5]].view(np.float32), rec[bad[:5]].view(np.int32))
    # not vacuous: both answers occur, per gate kind
    f, i = rec.view(np.float32), rec.view(np.int32)
    assert want.any() and (~want).any()
    nan_rec = np.isnan(f[:, [0, 1, 2, 3, 5, 6, 8, 9]]).any(axis=1)
    assert nan_rec.sum() > 100 and not want[nan_rec].any()          # a NaN coordinate or bound: never allowed
    for m in (-1, 0, 1):
        sel = i[:, 4] == m
        assert want[sel].any() and (~want[sel]).any(), m
    with np.errstate(invalid="ignore", over="ignore"):
        edge = (f[:, 8] - f[:, 5] == f[:, 1]) | (f[:, 8] - f[:, 5] == f[:, 0])
    assert (want & edge).sum() > 20                                  # differences equal to a bound pass (closed intervals)

"""CPU checks of the pair matchers' exit (selected matches, packed): both libraries export the three entry points the header
declares, Python has the calls, the new kernels touch no scratch memory, and the selection rule - the very functions the kernels
call, built here for the host - agrees with a numpy float32 restatement."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import ethzasl_brisk_amd as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("brisk_hip_select_pair_matches_device", "brisk_hip_pair_matches_download", "brisk_hip_pair_matches_wait")
TOPUP = np.float32(2147483648.0)
MAXROW = 8


def test_both_libraries_export_the_exit():
    from ethzasl_brisk_amd import build
    hdr = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    declared = set(re.findall(r"\b(brisk_hip_[a-z_0-9]+)\s*\(", hdr))
    for lib in (build.build(), build.build_release()):
        L = ctypes.CDLL(lib)
        for s in NEW:
            assert s in declared, s
            assert s in B.ABI_SYMBOLS, s
            assert hasattr(L, s), (lib, s)
    for t in ("brisk_hip_match_select", "brisk_hip_pair_host_matches"):
        assert re.search(r"typedef struct %s\b" % t, hdr), t
    for name, value in (("BRISK_HIP_PAIR_ROWS_CUT", 1), ("BRISK_HIP_PAIR_BAD", 2), ("BRISK_HIP_PAIR_ENTRIES_CUT", 4), ("BRISK_HIP_ROWS_CUT", 0x100)):
        m = re.search(r"#define %s (0x[0-9a-fA-F]+|\d+)" % name, hdr)
        assert m and int(m.group(1), 0) == value, name


def test_python_has_the_exit():
    assert ctypes.sizeof(B.MatchSelect) == 12
    assert ctypes.sizeof(B.PairHostMatches) == 56
    assert (B.PAIR_ROWS_CUT, B.PAIR_BAD, B.PAIR_ENTRIES_CUT, B.ROWS_CUT) == (1, 2, 4, 0x100)
    par = inspect.signature(B.Context.select_pair_matches).parameters
    assert list(par)[1:] == ["out_triple", "per_row", "select", "matches_cap", "stream"]
    assert par["matches_cap"].default is None and par["stream"].default is None
    par = inspect.signature(B.Context.pair_matches_download).parameters
    assert list(par)[1:] == ["out_triple", "per_row", "select", "dst", "stream"] and par["stream"].default is None
    par = inspect.signature(B.Context.pair_matches_wait).parameters
    assert list(par)[1:] == ["ticket", "check"] and par["check"].default is True
    h = B.HostMatches(3, 10, pinned=False)
    assert h.pair_rows.shape == (3,) and h.counts.shape == (3,) and h.flags.shape == (3,) and h.offsets.shape == (4,)
    assert h.matches.dtype == B.DMATCH and h.matches.shape == (10,)
    assert h.struct.pairs_cap == 3 and h.struct.matches_cap == 10 and h.struct.matches == h.matches.ctypes.data
    h.offsets[:] = [0, 2, 2, 7]
    assert len(h.pair(0)) == 2 and len(h.pair(1)) == 0 and len(h.pair(2)) == 5
    assert h.pair(2).ctypes.data == h.matches.ctypes.data + 2 * 16
    # the matchers keep their signatures
    assert list(inspect.signature(B.Context.match_knn_pairs).parameters)[1:] == [
        "query", "train", "pairs", "k", "cross_check", "rows_cap", "stream", "dim_bytes", "out", "download", "gate", "query_kps", "train_kps"]
    assert list(inspect.signature(B.Context.match_radius_pairs).parameters)[1:] == [
        "query", "train", "pairs", "max_distance", "cap_per_query", "rows_cap", "stream", "dim_bytes", "out", "download", "gate", "query_kps",
        "train_kps"]


def test_exit_kernels_use_no_scratch():
    from ethzasl_brisk_amd import build
    build.build()
    res = build.kernel_resources()
    if not res:
        pytest.skip("the objects were not compiled here (no resource remarks beside them)")
    new = {k: v for k, v in res.items() if "k_pair_select" in k}
    assert len(new) == 4                         # count, offsets, scatter, egress
    for k, v in new.items():
        assert v["scratch"] == 0, (k, v)
        assert "k_match_knn_pairs" not in k and "k_match_radius_pairs" not in k


# ---- the rule -----------------------------------------------------------------------------------------------------------------

def build_program():
    """tests/cpp/test_match_select.cc: plain host C++ around csrc/brisk_match_select.h (no HIP, no library)"""
    src = os.path.join(ROOT, "tests", "cpp", "test_match_select.cc")
    hdr = os.path.join(ROOT, "ethzasl_brisk_amd", "csrc", "brisk_match_select.h")
    out = os.path.join(ROOT, "tests", "cpp", "test_match_select")
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in (src, hdr)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off", "-I" + os.path.dirname(hdr), "-o", out, src])
    return out


def restated_row(max_distance, ratio, keep, per_row, count, dist):
    """the header's words on one row, in numpy float32: how many leading entries are delivered"""
    max_distance, ratio = np.float32(max_distance), np.float32(ratio)
    d = np.asarray(dist, np.float32)[:max(min(int(count), int(per_row)), 0)]          # the stored entries
    with np.errstate(invalid="ignore", over="ignore"):
        ok = (d < max_distance) & (d != TOPUP)
        if ratio > 0:                                                                  # (False for NaN)
            if len(d) == 0 or not ok[0]:
                return 0
            if len(d) == 1 or d[1] == TOPUP:
                return 1
            bound = ratio * d[1]
            assert bound.dtype == np.float32
            return int(d[0] < bound)
    lead = ok[:min(len(d), int(keep))]
    return len(lead) if lead.all() else int(np.argmin(lead))


def select_records():
    rng = np.random.default_rng(77)
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    recs = []

    def add(max_distance, ratio, keep, per_row, count, dist):
        r = np.zeros(13, np.uint32)
        r[0:2] = np.array([max_distance, ratio], np.float32).view(np.uint32)
        r[2:5] = np.array([keep, per_row, count], np.int32).view(np.uint32)
        d = np.full(MAXROW, 777.0, np.float32)                      # behind the row: a value that passes everything (never read)
        d[:len(dist)] = np.array(dist, np.float32)
        r[5:] = d.view(np.uint32)
        recs.append(r)

    def sorted_row(n, hi=200):
        return np.sort(rng.integers(0, hi, n)).astype(np.float32)

    for _ in range(4000):                                           # random rows, every switch in every position
        per_row = int(rng.integers(1, MAXROW + 1))
        count = int(rng.choice([0, 1, 2, per_row - 1, per_row, per_row + 1, per_row + 30, int(rng.integers(0, 12))]))
        keep = int(rng.choice([1, 2, per_row, per_row + 3, 1000]))
        ratio = [0.0, -1.0, 0.8, 0.8, 0.5, 1.0, 1.25, nan, inf, -inf][rng.integers(0, 10)]
        md = [inf, inf, 50.0, 100.0, 0.0, -1.0, nan, -inf, 199.0, 1.0][rng.integers(0, 10)]
        d = sorted_row(MAXROW)
        stored = max(min(count, per_row), 0)
        if stored >= 1 and rng.integers(0, 6) == 0:                 # a topped-up row: the entries behind the real ones
            d[int(rng.integers(0, stored)):] = TOPUP
            if rng.integers(0, 2):
                d[1:] = TOPUP                                       # ... exactly one real entry (or none), then the top-up
        add(md, ratio, keep, per_row, count, d)
    for ratio in (0.8, 0.5, 0.75, 1.0):                             # ties d0 == ratio * d1 (exact in fp32), one ulp either side
        for d1 in (4.0, 20.0, 40.0, 100.0, 160.0):
            d0 = np.float32(ratio) * np.float32(d1)
            for dd0 in (d0, np.nextafter(d0, np.float32(0)), np.nextafter(d0, inf)):
                for md in (inf, 1000.0, float(dd0), nan):
                    add(md, ratio, 1, 2, 2, [dd0, d1])
                    add(md, ratio, 3, 4, 7, [dd0, d1, d1, d1 + 1])
    for ratio in (0.8, 1.0, 5.0, inf):                              # d1 == 0 (then d0 == 0): never strictly below
        add(inf, ratio, 1, 2, 2, [0.0, 0.0])
        add(inf, ratio, 1, 2, 2, [0.0, 1.0])
        add(inf, ratio, 1, 2, 1, [0.0, 0.0])                        # a single-entry row
        add(inf, ratio, 1, 2, 2, [5.0, TOPUP])                      # a top-up second entry
        add(inf, ratio, 1, 2, 2, [TOPUP, TOPUP])
        add(3.0, ratio, 1, 2, 2, [5.0, TOPUP])
    for keep in (1, 2, 5, 9, 2 ** 31 - 1):                          # keep_per_row against per_row, counts above per_row
        for per_row in (1, 4, 8):
            for count in (0, 1, per_row, per_row + 1, 2 ** 31 - 1, -1, -(2 ** 31)):
                add(inf, 0.0, keep, per_row, count, sorted_row(MAXROW))
                add(60.0, nan, keep, per_row, count, sorted_row(MAXROW, 120))
    return np.stack(recs)


def test_the_rule_agrees_with_its_restatement(tmp_path):
    rec = select_records()
    assert len(rec) >= 4000
    path = tmp_path / "select_records.bin"
    rec.astype("<u4").tofile(path)
    r = subprocess.run([build_program(), str(path)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    got = np.array([int(c) for c in r.stdout.strip()])
    f, i = rec.view(np.float32), rec.view(np.int32)
    want = np.array([restated_row(f[n, 0], f[n, 1], i[n, 2], i[n, 3], i[n, 4], f[n, 5:]) for n in range(len(rec))])
    assert len(got) == len(want)
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, (len(bad), rec[bad[:5]].view(np.float32), rec[bad[:5]].view(np.int32), got[bad[:5]], want[bad[:5]])
    # not vacuous: every kind of record both keeps and drops
    stored = np.clip(np.minimum(i[:, 4], i[:, 3]), 0, None)
    with np.errstate(invalid="ignore"):
        ratio_on = f[:, 1] > 0
    nan_md = np.isnan(f[:, 0])
    assert nan_md.sum() > 100 and not want[nan_md].any()             # NaN max_distance keeps nothing
    for sel in (ratio_on & (stored >= 2), ratio_on & (stored == 1), ~ratio_on & (stored >= 2)):
        assert (want[sel] > 0).any() and (want[sel] == 0).any()
    assert (want[ratio_on] <= 1).all()
    assert (want <= np.minimum(stored, np.maximum(i[:, 2], 0))).all()
    assert (want[~ratio_on] >= 3).any()                              # more than the ratio test could give
    over = i[:, 4] > i[:, 3]
    assert (want[over] > 0).any()                                    # counts above per_row: what was stored is used
    top2 = ratio_on & (stored >= 2) & (f[:, 6] == TOPUP) & (f[:, 5] != TOPUP)
    with np.errstate(invalid="ignore"):
        assert top2.sum() > 10 and (want[top2] == (f[top2, 5] < f[top2, 0])).all()   # "no second neighbour": the distance bound alone
    with np.errstate(invalid="ignore", over="ignore"):
        tie = ratio_on & (stored >= 2) & np.isfinite(f[:, 1]) & (f[:, 5] == f[:, 1] * f[:, 6])
    assert tie.sum() > 20 and not want[tie].any()                    # d0 == ratio * d1 is not below
    assert not want[(stored >= 1) & (f[:, 5] == TOPUP)].any()        # a top-up entry is never selected

"""CPU checks of the feature tracker (brisk_hip_link_tracks_device / brisk_hip_list_tracks_device): both libraries export the two
entry points the header declares, Python has the calls, the new kernels touch no scratch memory, and the link rule - the very
functions the kernels call, built here for the host - agrees with a numpy / Python restatement.  restated_link / restated_list are
the expectation of the GPU tests (test_gpu_tracks.py) too."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import ethzasl_brisk_amd as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("brisk_hip_link_tracks_device", "brisk_hip_list_tracks_device")
SENT32 = np.int32(0x5A5A5A5A)                    # what the matcher tests pre-fill outputs with (test_gpu_match_pairs.SENTINEL)
SENT64 = np.int64(0x5A5A5A5A5A5A5A5A)
INF_BITS = 0x7F800000


def test_both_libraries_export_the_tracker():
    from ethzasl_brisk_amd import build
    hdr = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    declared = set(re.findall(r"\b(brisk_hip_[a-z_0-9]+)\s*\(", hdr))
    for lib in (build.build(), build.build_release()):
        L = ctypes.CDLL(lib)
        for s in NEW:
            assert s in declared, s
            assert s in B.ABI_SYMBOLS, s
            assert hasattr(L, s), (lib, s)
    for t in ("brisk_hip_track_seed", "brisk_hip_track_obs"):
        assert re.search(r"typedef struct %s\b" % t, hdr), t
    m = re.search(r"#define BRISK_HIP_TRACKS_CUT (0x[0-9a-fA-F]+|\d+)", hdr)
    assert m and int(m.group(1), 0) == B.TRACKS_CUT == 1


def test_python_has_the_tracker():
    hdr = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    body = re.search(r"typedef struct brisk_hip_track_seed \{(.*?)\} brisk_hip_track_seed;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [f.strip() for f in body.split(";") if f.strip()]
    want = {"const long long* d_track": 8, "const int* d_age": 8, "long long first_new": 8, "const long long* d_first_new": 8}
    assert fields == list(want)                                         # the header's fields, in order: pointers and one long long
    assert ctypes.sizeof(B.TrackSeed) == sum(want.values()) == 32
    assert [n for n, _ in B.TrackSeed._fields_] == [f.split()[-1].lstrip("*") for f in fields]
    assert B.TRACK_OBS.itemsize == 8 and B.TRACK_OBS.names == ("node", "row")
    par = inspect.signature(B.Context.link_tracks).parameters
    assert list(par)[1:] == ["node_rows", "nodes", "rows_cap", "offsets", "matches", "seed", "stream"]
    assert par["seed"].default is None and par["stream"].default is None
    par = inspect.signature(B.Context.list_tracks).parameters
    assert list(par)[1:] == ["node_rows", "nodes", "rows_cap", "prev", "track", "age", "min_len", "tracks_cap", "obs_cap", "stream"]
    assert par["tracks_cap"].default is None and par["obs_cap"].default is None and par["stream"].default is None
    st = B.DescSet(None, 4096, 3, 0, 0, 10)                             # a chain out of a descriptor set: frames first + i * step
    assert B.Context._node_rows((st, 2, 2)) == (4096 + 4 * 2 * 3, 6)


def test_tracker_kernels_use_no_scratch():
    from ethzasl_brisk_amd import build
    build.build()
    res = build.kernel_resources()
    if not res:
        pytest.skip("the objects were not compiled here (no resource remarks beside them)")
    new = {k: v for k, v in res.items() if "k_track_" in k}
    assert len(new) == 12                                               # six of the link call, six of the list call
    for k, v in new.items():
        assert v["scratch"] == 0, (k, v)
        assert "k_pair_select" not in k and "k_match_knn_pairs" not in k and "k_match_radius_pairs" not in k


# ---- the rule, restated ---------------------------------------------------------------------------------------------------------

def lims(node_rows, rows_cap):
    return [min(max(int(n), 0), int(rows_cap)) for n in node_rows]


def restated_proposals(rec, lim_q, lim_t):
    """the header's words on the list of one pair (DMATCH records): (which records are proposals, their 64-bit keys)"""
    q, t = rec["queryIdx"].astype(np.int64), rec["trainIdx"].astype(np.int64)
    bits = rec["distance"].view(np.uint32).astype(np.uint64)
    first = np.ones(len(rec), bool)
    first[1:] = q[1:] != q[:-1]
    ok = first & (q >= 0) & (q < lim_q) & (t >= 0) & (t < lim_t) & (bits <= INF_BITS)
    return ok, (bits << np.uint64(32)) | (q & 0xFFFFFFFF).astype(np.uint64)


def restated_link(node_rows, rows_cap, offsets, matches, seed_track=None, seed_age=None, first_new=0):
    """(prev, track, age [nodes, rows_cap] - sentinel where the call writes nothing -, summary [8]) the rule gives"""
    nodes, lim = len(node_rows), lims(node_rows, rows_cap)
    prev = np.full((nodes, rows_cap), SENT32, np.int32)
    track = np.full((nodes, rows_cap), SENT64, np.int64)
    age = np.full((nodes, rows_cap), SENT32, np.int32)
    for i in range(nodes):
        prev[i, :lim[i]] = -1
    links = lost = ignored = 0
    for p in range(nodes - 1):
        rec = matches[int(offsets[p]):int(offsets[p + 1])]
        ok, keys = restated_proposals(rec, lim[p + 1], lim[p])
        ignored += int((~ok).sum())
        best = {}
        for j in np.flatnonzero(ok):
            t, k = int(rec["trainIdx"][j]), int(keys[j])
            best[t] = min(best.get(t, k), k)
        for j in np.flatnonzero(ok):
            t = int(rec["trainIdx"][j])
            if best[t] == int(keys[j]):
                prev[p + 1, int(rec["queryIdx"][j])] = t
                links += 1
            else:
                lost += 1
    nxt = int(first_new)
    for i in range(nodes):
        for r in range(lim[i]):
            t = int(prev[i, r])
            if t >= 0:
                track[i, r], age[i, r] = track[i - 1, t], age[i - 1, t] + 1
            elif i == 0 and seed_track is not None and int(seed_track[r]) >= 0:
                track[i, r], age[i, r] = seed_track[r], seed_age[r]
            else:
                track[i, r], age[i, r] = nxt, 0
                nxt += 1
    summary = np.array([nxt, nxt - int(first_new), links, lost, ignored, sum(lim), 0, 0], np.int64)
    return prev, track, age, summary


def restated_list(node_rows, rows_cap, prev, track, age, min_len, tracks_cap=None, obs_cap=None):
    """(list_track, list_len, list_offsets [stored + 1], list_obs [observations stored] as TRACK_OBS records, summary [4])"""
    nodes, lim = len(node_rows), lims(node_rows, rows_cap)
    nxt = {}
    for i in range(1, nodes):
        for r in range(lim[i]):
            if prev[i, r] >= 0:
                nxt[i - 1, int(prev[i, r])] = r
    pieces = []
    for i in range(nodes):
        for r in range(lim[i]):
            if prev[i, r] >= 0:
                continue
            obs, at = [(i, r)], (i, r)
            while at in nxt:
                at = (at[0] + 1, nxt[at])
                obs.append(at)
            if int(age[at]) + 1 >= min_len:
                pieces.append((int(track[i, r]), int(age[at]) + 1, obs))
    total_obs = sum(len(o) for _, _, o in pieces)
    tracks_cap = len(pieces) if tracks_cap is None else tracks_cap
    obs_cap = total_obs if obs_cap is None else obs_cap
    stored, used = 0, 0
    for _, _, o in pieces:
        if stored + 1 > tracks_cap or used + len(o) > obs_cap:
            break
        stored, used = stored + 1, used + len(o)
    keep = pieces[:stored]
    offsets = np.zeros(stored + 1, np.int64)
    offsets[1:] = np.cumsum([len(o) for _, _, o in keep])
    obs = np.array([x for _, _, o in keep for x in o], B.TRACK_OBS) if used else np.zeros(0, B.TRACK_OBS)
    summary = np.array([len(pieces), total_obs, stored, 1 if stored < len(pieces) else 0], np.int64)
    return (np.array([t for t, _, _ in keep], np.int64), np.array([n for _, n, _ in keep], np.int32), offsets, obs, summary)


# ---- the rule's own code against the restatement -----------------------------------------------------------------------------------

def build_program(sanitize=False):
    """tests/cpp/test_track_link.cc: plain host C++ around csrc/brisk_track_link.h (no HIP, no library)"""
    src = os.path.join(ROOT, "tests", "cpp", "test_track_link.cc")
    hdr = os.path.join(ROOT, "ethzasl_brisk_amd", "csrc", "brisk_track_link.h")
    out = os.path.join(ROOT, "tests", "cpp", "test_track_link" + ("_san" if sanitize else ""))
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in (src, hdr)):
        extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off"] + extra + ["-I" + os.path.dirname(hdr), "-o", out, src])
    return out


def f32(*values):
    return np.array(values, np.float32)


def link_cases():
    """[(lim_query, lim_train, DMATCH records of one pair)]"""
    rng = np.random.default_rng(1234)
    special = np.concatenate([f32(0.0, 1.0, 1.0, 37.0, np.inf, np.nan, -1.0, -0.0, 2147483648.0),
                              np.array([0x7F800001, 0xFFC00000, 0x80000001, 0xFFFFFFFF], np.uint32).view(np.float32)])
    cases = []

    def rec(rows):
        a = np.zeros(len(rows), B.DMATCH)
        for n, (q, t, d) in enumerate(rows):
            a[n] = (q, t, 7, d)
        return a

    lim = 10
    hand = []
    for q in (-1, 0, lim - 1, lim, lim + 1, -2 ** 31, 2 ** 31 - 1):          # indices at and beyond both ends
        for t in (-1, 0, lim - 1, lim, lim + 1, -2 ** 31, 2 ** 31 - 1):
            hand.append((q, t, 5.0))
    cases.append((lim, lim, rec(hand)))
    cases.append((lim, 4, rec(hand)))                                         # another limit per side
    cases.append((3, lim, rec(hand)))
    cases.append((lim, lim, rec([(n % lim, (3 * n) % lim, d) for n, d in enumerate(special)])))   # every distance kind
    cases.append((lim, lim, rec([(2, 5, 9.0), (2, 6, 9.5), (3, 5, 8.0), (3, 7, 8.5), (4, 5, 8.0), (5, 5, 0.0)])))  # a row whose first record loses
    cases.append((lim, lim, rec([(1, 1, 3.0), (1, 2, 3.0), (1, 3, 4.0), (2, 2, 3.0), (1, 4, 1.0)])))  # second records; row 1 again (malformed)
    cases.append((0, lim, rec([(0, 0, 1.0)])))
    cases.append((lim, 0, rec([(0, 0, 1.0)])))
    cases.append((-5, -5, rec([(0, 0, 1.0), (-5, -5, 1.0)])))                 # negative row counts: no rows
    cases.append((lim, lim, rec([])))
    for _ in range(300):                                                      # random lists: sorted by query row, up to 3 records a row
        lq, lt = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        rows = []
        for q in range(-1, lq + 2):
            for _k in range(int(rng.integers(0, 4))):
                d = special[rng.integers(0, len(special))] if rng.integers(0, 4) == 0 else np.float32(rng.integers(0, 6))
                rows.append((q, int(rng.integers(-1, lt + 2)), d))
        cases.append((lq, lt, rec(rows)))
    return cases


def run_program(prog, cases, path):
    words = []
    for lq, lt, r in cases:
        words.append(np.array([lq, lt, len(r)], np.int32).view(np.uint32))
        words.append(np.ascontiguousarray(r).view(np.uint32).reshape(-1))
    np.concatenate(words).astype("<u4").tofile(path)
    out = subprocess.run([prog, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    return out.stdout.split("\n")[:-1]


def test_the_rule_agrees_with_its_restatement(tmp_path):
    cases = link_cases()
    lines = run_program(build_program(), cases, tmp_path / "link_records.bin")
    assert len(lines) == sum(len(r) for _, _, r in cases)
    at = proposals = 0
    kinds = set()
    for lq, lt, r in cases:
        ok, keys = restated_proposals(r, max(lq, 0), max(lt, 0))
        for j in range(len(r)):
            want = "%016x %d" % (int(keys[j]), int(r["queryIdx"][j])) if ok[j] else "-"
            assert lines[at + j] == want, (lq, lt, r[max(j - 1, 0):j + 1], lines[at + j], want)
        at += len(r)
        proposals += int(ok.sum())
        bits = r["distance"].view(np.uint32)
        kinds |= {(int(b), bool(o)) for b, o in zip(bits, ok)}
    # not vacuous: records both propose and are ignored, and each distance kind behaves as the header says
    assert proposals > 1000 and at - proposals > 1000
    for d, proposes in ((0.0, True), (1.0, True), (np.inf, True), (2147483648.0, True), (np.nan, False), (-1.0, False), (-0.0, False)):
        b = int(f32(d).view(np.uint32)[0])
        assert (b, proposes) in kinds and ((b, True) in kinds) == proposes, d
    # the keys order proposals by (distance, query row): for such floats the bit order is the numeric order
    a, b = restated_proposals(np.array([(3, 0, 0, 2.0), (1, 0, 0, 2.0), (0, 0, 0, 2.5), (9, 0, 0, np.inf)], B.DMATCH), 10, 10)
    assert a.all() and int(b[1]) < int(b[0]) < int(b[2]) < int(b[3]) < 2 ** 64 - 1


def test_the_rule_under_sanitizers(tmp_path):
    """the same program with the address and undefined-behaviour sanitizers, run stand-alone (nothing sanitized is loaded into Python)"""
    cases = link_cases()
    plain = run_program(build_program(), cases, tmp_path / "a.bin")
    assert run_program(build_program(sanitize=True), cases, tmp_path / "b.bin") == plain


def test_the_restatement_on_a_chain_by_hand():
    """three nodes: a conflict, a loser whose second record names a free row, a seed, a cut node"""
    rows_cap = 4
    node_rows = [3, 6, 2]                                             # node 1 is cut at rows_cap
    m = np.array([(0, 0, 0, 2.0), (1, 0, 0, 1.0), (1, 2, 0, 1.5), (2, 1, 0, 3.0), (2, 2, 0, 3.5), (3, 2, 0, 9.0), (4, 2, 0, 0.0),   # pair 0
                  (0, 1, 1, 1.0), (1, 3, 1, np.nan), (1, 0, 1, 1.0)], B.DMATCH)                                                       # pair 1
    offsets = np.array([0, 7, 10], np.int64)
    seed_track, seed_age = np.array([100, -1, 7, 55], np.int64), np.array([4, 9, 0, 1], np.int32)
    prev, track, age, summary = restated_link(node_rows, rows_cap, offsets, m, seed_track, seed_age, first_new=2 ** 40)
    assert prev[0, :3].tolist() == [-1, -1, -1] and prev[0, 3] == SENT32
    assert prev[1].tolist() == [-1, 0, 1, 2]                         # row 0 loses train row 0 to row 1; row 4 does not exist
    assert prev[2, :2].tolist() == [1, -1] and prev[2, 2] == SENT32  # row 1's first record is NaN: the row proposes nothing
    n = 2 ** 40
    assert track[0, :3].tolist() == [100, n, 7] and age[0, :3].tolist() == [4, 0, 0]
    assert track[1].tolist() == [n + 1, 100, n, 7] and age[1].tolist() == [0, 5, 1, 1]
    assert track[2, :2].tolist() == [100, n + 2] and age[2, :2].tolist() == [6, 0]
    assert summary.tolist() == [n + 3, 3, 4, 1, 5, 9, 0, 0]
    lt, ll, lo, obs, s = restated_list(node_rows, rows_cap, prev, track, age, 2)
    assert lt.tolist() == [100, n, 7] and ll.tolist() == [7, 2, 2] and lo.tolist() == [0, 3, 5, 7]
    assert obs.tolist() == [(0, 0), (1, 1), (2, 0), (0, 1), (1, 2), (0, 2), (1, 3)] and s.tolist() == [3, 7, 3, 0]
    lt, ll, lo, obs, s = restated_list(node_rows, rows_cap, prev, track, age, 2, tracks_cap=3, obs_cap=4)
    assert lt.tolist() == [100] and lo.tolist() == [0, 3] and len(obs) == 3 and s.tolist() == [3, 7, 1, 1]
    lt, ll, lo, obs, s = restated_list(node_rows, rows_cap, prev, track, age, 4)     # nodes + 1: only the seeded piece is long enough
    assert lt.tolist() == [100] and ll.tolist() == [7] and s.tolist() == [1, 3, 1, 0]

"""CPU checks of the tracker's exit (brisk_hip_track_points_device, brisk_hip_tracks_download, brisk_hip_tracks_wait): both libraries
export the three entry points the header declares, Python has the types and the calls, the new kernels touch no scratch memory, the
point rule - the very function the kernel calls, built here for the host - agrees with a numpy restatement, the exit's arrays lie
where the layout helper puts them, and the rule's header is part of the kernel revision.  restated_points is the expectation of the
GPU tests (test_gpu_track_export.py) too."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np

import ethzasl_brisk_amd as B
from test_abi_transfer import layouts

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ethzasl_brisk_amd", "csrc")
NEW = ("brisk_hip_track_points_device", "brisk_hip_tracks_download", "brisk_hip_tracks_wait")
CTYPES = {"long long": ctypes.c_longlong, "int": ctypes.c_int}


def struct_fields(hdr, name):
    """[(type, field)] of a typedef struct of the header, comments removed, `int a, b` split"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        first, *more = [p.strip() for p in decl.split(",")]
        typ, field = first.rsplit(None, 1) if "*" not in first else (first[:first.rindex("*") + 1], first[first.rindex("*") + 1:].strip())
        out.append((typ.strip(), field))
        out += [(typ.strip(), m) for m in more]
    return out


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
    assert "brisk_track_export.hip" in build.SOURCES


def test_python_has_the_types_and_the_calls():
    hdr = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    # the point: node, row, then the keypoint record - 36 bytes, the fields where the header's struct has them
    assert struct_fields(hdr, "brisk_hip_track_point") == [("int", "node"), ("int", "row"), ("brisk_hip_keypoint", "kp")]
    kp = struct_fields(hdr, "brisk_hip_keypoint")
    assert [f for _, f in kp] == list(B.KEYPOINT.names)
    assert B.TRACK_POINT.itemsize == 36 and B.TRACK_POINT.names == ("node", "row") + B.KEYPOINT.names
    assert [B.TRACK_POINT.fields[n][1] for n in B.TRACK_POINT.names] == [0, 4] + [8 + B.KEYPOINT.fields[n][1] for n in B.KEYPOINT.names]
    assert [B.TRACK_POINT.fields[n][0] for n in B.KEYPOINT.names] == [B.KEYPOINT.fields[n][0] for n in B.KEYPOINT.names]
    assert B.TRACK_POINT.names[:2] == B.TRACK_OBS.names
    # the destination struct: two capacities and five pointers, 56 bytes
    fields = struct_fields(hdr, "brisk_hip_host_tracks")
    assert [f for _, f in fields] == [n for n, _ in B.HostTracks._fields_] == ["tracks_cap", "points_cap", "summary", "track", "len", "offsets",
                                                                                "points"]
    for (typ, field), (_, ct) in zip(fields, B.HostTracks._fields_):
        assert ct is (ctypes.c_void_p if typ.endswith("*") else CTYPES[typ]), (typ, field)
    assert ctypes.sizeof(B.HostTracks) == 56
    assert [typ for typ, _ in fields[2:]] == ["long long*", "long long*", "int*", "long long*", "brisk_hip_track_point*"]
    # the calls
    par = inspect.signature(B.Context.track_points).parameters
    assert list(par)[1:] == ["node_rows", "nodes", "rows_cap", "list_offsets", "list_obs", "list_summary", "kps", "kp_first", "kp_step", "stream"]
    assert par["kps"].default is None and par["kp_first"].default == 0 and par["kp_step"].default == 1 and par["stream"].default is None
    par = inspect.signature(B.Context.tracks_download).parameters
    assert list(par)[1:] == ["node_rows", "nodes", "rows_cap", "prev", "track", "age", "min_len", "dst", "kps", "kp_first", "kp_step", "stream"]
    par = inspect.signature(B.Context.tracks_wait).parameters
    assert list(par)[1:] == ["ticket", "check"] and par["check"].default is True
    h = B.HostTrackList(3, 10, pinned=False)
    assert h.summary.shape == (4,) and h.track.shape == (3,) and h.len.shape == (3,) and h.offsets.shape == (4,)
    assert h.summary.dtype == h.track.dtype == h.offsets.dtype == np.int64 and h.len.dtype == np.int32
    assert h.points.dtype == B.TRACK_POINT and h.points.shape == (10,)
    assert h.struct.tracks_cap == 3 and h.struct.points_cap == 10 and h.struct.points == h.points.ctypes.data
    h.summary[:] = [5, 20, 3, 1]
    h.offsets[:] = [0, 2, 2, 7]
    h.track[:], h.len[:] = [7, 8, 9], [2, 9, 5]
    assert h.stored == 3 and h.piece(1)[:2] == (8, 9) and len(h.piece(1)[2]) == 0 and len(h.piece(2)[2]) == 5
    assert h.piece(2)[2].ctypes.data == h.points.ctypes.data + 2 * 36
    # the tracker's calls keep their signatures
    assert list(inspect.signature(B.Context.link_tracks).parameters)[1:] == ["node_rows", "nodes", "rows_cap", "offsets", "matches", "seed", "stream"]
    assert list(inspect.signature(B.Context.list_tracks).parameters)[1:] == [
        "node_rows", "nodes", "rows_cap", "prev", "track", "age", "min_len", "tracks_cap", "obs_cap", "stream"]


def test_exit_kernels_use_no_scratch():
    from ethzasl_brisk_amd import build
    build.build()
    res = build.kernel_resources()
    if not res:                                                         # the library is here but not its objects: compile them
        build.build(force=True)
        res = build.kernel_resources()
    new = {k: v for k, v in res.items() if "k_tracklist_" in k}
    assert sorted(re.search(r"k_tracklist_[a-z]+", k).group(0) for k in new) == ["k_tracklist_egress", "k_tracklist_points"]
    for k, v in new.items():
        assert v["scratch"] == 0, (k, v)
        assert "k_track_" not in k and "k_pair_select" not in k          # the counts the other exits' tests make stay what they are
    assert len([k for k in res if "k_track_" in k]) == 12 and len([k for k in res if "k_pair_select" in k]) == 4


# ---- the rule, restated ---------------------------------------------------------------------------------------------------------

def restated_points(node_rows, rows_cap, obs, kp_words, frame_pitch, kp_first, kp_step):
    """the header's words: TRACK_POINT records of the observations `obs` (TRACK_OBS records).  node_rows: the chain's counts;
    kp_words(first, n): dwords [first, first + n) of the keypoint set - a function, or the set itself as a uint32 array"""
    if not callable(kp_words):
        whole = kp_words
        kp_words = lambda first, n: whole[first:first + n]                                       # noqa: E731
    nodes = len(node_rows)
    out = np.zeros((len(obs), 9), np.uint32)
    for i, (node, row) in enumerate(zip(obs["node"].tolist(), obs["row"].tolist())):
        out[i, 0], out[i, 1] = node & 0xFFFFFFFF, row & 0xFFFFFFFF
        if not 0 <= node < nodes or not 0 <= row < min(max(int(node_rows[node]), 0), rows_cap):
            continue                                                                             # 28 zero bytes, nothing read
        at = (kp_first + node * kp_step) * frame_pitch + row * 28                                # Python integers: no width
        assert at % 4 == 0 and at >= 0
        w = kp_words(at // 4, 7)
        assert len(w) == 7, (node, row, at)
        out[i, 2:] = w
    return out.reshape(-1).view(B.TRACK_POINT)


def build_program(sanitize=False):
    """tests/cpp/test_track_points.cc: plain host C++ around csrc/brisk_track_points.h (no HIP, no library)"""
    src = os.path.join(ROOT, "tests", "cpp", "test_track_points.cc")
    hdrs = [os.path.join(CSRC, "brisk_track_points.h"), os.path.join(CSRC, "brisk_track_link.h")]
    out = os.path.join(ROOT, "tests", "cpp", "test_track_points" + ("_san" if sanitize else ""))
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in [src] + hdrs):
        extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall"] + extra + ["-I" + CSRC, "-o", out, src])
    return out


def point_cases():
    """[(node_rows at `stride`, stride, rows_cap, kp_first, kp_step, frame_pitch, obs, kp dwords)]: the keypoint set holds exactly the
    frames the chain names with exactly lim rows in the last one - a read for an observation that names no keypoint leaves it"""
    rng = np.random.default_rng(36)
    cases = []
    for n in range(300):
        nodes, rows_cap = int(rng.integers(1, 9)), int(rng.integers(1, 12))
        counts = [int(v) for v in rng.integers(-2, rows_cap + 4, nodes)]              # negative counts, counts beyond rows_cap
        kp_first, kp_step = [(1, 2), (3, -1), (0, 1), (5, 0)][n % 4]
        if kp_first + (nodes - 1) * kp_step < 0:
            nodes = 4                                                                 # (3, -1): frames 3, 2, 1, 0
            counts = (counts * 4)[:4]
        lim = [min(max(c, 0), rows_cap) for c in counts]
        frame_pitch = rows_cap * 28 + 4 * int(rng.integers(0, 5))                     # often no multiple of 28
        stride = int(rng.integers(1, 4))
        nr = np.full(nodes * stride, 77777, np.int32)
        nr[::stride] = counts
        frames = [kp_first + i * kp_step for i in range(nodes)]
        end = max(f * frame_pitch + l * 28 for f, l in zip(frames, lim))               # the last byte any existing row has
        kp = rng.integers(0, 2 ** 32, end // 4, dtype=np.uint64).astype(np.uint32)
        kp[rng.integers(0, 4, len(kp)) == 0] = 0x7FC00001 + n                         # NaN payloads
        obs = np.zeros(60, B.TRACK_OBS)
        obs["node"] = rng.integers(-1, nodes + 1, 60)
        obs["row"] = rng.integers(-1, rows_cap + 2, 60)
        obs["node"][:4], obs["row"][:4] = [-1, nodes, 0, nodes - 1], [0, 0, -1, lim[-1]]
        obs["node"][4:6], obs["row"][4:6] = [-2 ** 31, 2 ** 31 - 1], [2 ** 31 - 1, -2 ** 31]
        cases.append((nr, stride, rows_cap, kp_first, kp_step, frame_pitch, obs, kp, counts))
    return cases


def run_program(prog, cases, path):
    words = []
    for nr, stride, rows_cap, kp_first, kp_step, frame_pitch, obs, kp, _ in cases:
        words.append(np.array([len(nr) // stride, rows_cap, stride, kp_first, kp_step, frame_pitch, len(obs), len(kp)], np.int32).view(np.uint32))
        words += [nr.view(np.uint32), np.ascontiguousarray(obs).view(np.uint32).reshape(-1), kp]
    np.concatenate(words).astype("<u4").tofile(path)
    out = subprocess.run([prog, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    return out.stdout.split("\n")[:-1]


def test_the_rule_agrees_with_its_restatement(tmp_path):
    cases = point_cases()
    lines = run_program(build_program(), cases, tmp_path / "points.bin")
    assert len(lines) == sum(len(c[6]) for c in cases)
    at = real = zero = 0
    for nr, stride, rows_cap, kp_first, kp_step, frame_pitch, obs, kp, counts in cases:
        want = restated_points(counts, rows_cap, obs, kp, frame_pitch, kp_first, kp_step).view(np.uint32).reshape(-1, 9)
        for i in range(len(obs)):
            assert lines[at + i] == " ".join("%08x" % v for v in want[i]), (at, i, obs[i], lines[at + i])
        at += len(obs)
        nz = want[:, 2:].any(axis=1)
        real, zero = real + int(nz.sum()), zero + int((~nz).sum())
    # not vacuous: keypoints were found and refused, pitches that are no multiple of 28 and both (kp_first, kp_step) pairs were used
    assert real > 1000 and zero > 1000
    assert any(c[5] % 28 for c in cases) and {(1, 2), (3, -1)} <= {(c[3], c[4]) for c in cases}
    # a NaN payload and every bit of class_id survive: the record is copied, not interpreted
    kp = np.array([0x7FC00001, 0xFFC12345, 0x7F800001, 0xFFFFFFFF, 0x80000000, 0xDEADBEEF, 0xFFFFFFFF], np.uint32)
    p = restated_points([1], 4, np.array([(0, 0)], B.TRACK_OBS), kp, 28, 0, 1)
    assert p.view(np.uint32).tolist() == [0, 0] + kp.tolist() and p["class_id"][0] == -1 and np.isnan(p["x"][0])


def test_the_rule_under_sanitizers(tmp_path):
    """the same program with the address and undefined-behaviour sanitizers, run stand-alone (nothing sanitized is loaded into
    Python): the keypoint set is an allocation of exactly the rows that exist, so a read for a refused observation would show"""
    cases = point_cases()
    plain = run_program(build_program(), cases, tmp_path / "a.bin")
    assert run_program(build_program(sanitize=True), cases, tmp_path / "b.bin") == plain


# ---- where the exit's arrays lie ------------------------------------------------------------------------------------------------

def track_arrays(tracks, points):
    """byte sizes of summary, track, len, offsets, points of a list (brisk_hip_host_tracks)"""
    return [32, 8 * tracks, 4 * tracks, 8 * (tracks + 1), 36 * points]


def test_the_exit_s_layout():
    # each array at the next multiple of 256 behind the previous one, the total = the rounded end + 256; worked out by hand
    want = {(1, 0): ([0, 256, 512, 768, 1024], 1280),
            (3, 10): ([0, 256, 512, 768, 1024], 1792),
            (2 ** 31 + 5, 2 ** 31 + 7): ([0, 256, 17179869696, 25769804544, 42949673984], 120259085824)}
    for (shape, w), g in zip(want.items(), layouts([track_arrays(*k) for k in want])):
        assert g == w, (shape, g, w)
    # the library lays the arrays out in this order with this helper
    capi = open(os.path.join(CSRC, "brisk_capi.hip")).read()
    body = re.search(r"static SlabLayout tracks_layout\(.*?\n\}", capi, re.S).group(0)
    adds = re.findall(r"LY\.add\((.*?)\);\s*// (\w+)", body)
    assert [name for _, name in adds] == ["summary", "track", "len", "offsets", "points"]
    assert "sizeof(brisk_hip_track_point) * (size_t)points" in adds[4][0] and "(size_t)tracks + 1" in adds[3][0]


def test_the_rule_s_header_is_in_the_kernel_revision(tmp_path, monkeypatch):
    from ethzasl_brisk_amd import build
    rev = build.kernel_revision()
    copy = tmp_path / "csrc"
    shutil.copytree(CSRC, copy)
    monkeypatch.setattr(build, "CSRC", str(copy))
    assert build.kernel_revision() == rev
    for name in ("brisk_transfer.h", "brisk_capi.hip", "brisk_slab_layout.h"):      # host code only
        text = (copy / name).read_text()
        assert "__global__" not in text and "__device__" not in text, name
        (copy / name).write_text(text + "// changed\n")
        assert build.kernel_revision() == rev, name
    moved = []
    for name in ("brisk_track_points.h", "brisk_track_export.hip"):                 # device code
        (copy / name).write_text((copy / name).read_text() + "// changed\n")
        moved.append(build.kernel_revision())
    assert moved[0] != rev and moved[1] not in (rev, moved[0])

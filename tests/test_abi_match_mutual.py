"""CPU checks of the mutual guided pair matchers' boundary: both libraries export the two entry points the header declares, Python has
the two calls, the eight kernels touch no scratch memory, and the rule - the very functions the kernels call
(csrc/brisk_match_guide.h, csrc/brisk_match_epiline.h), built here for the host - agrees with a NumPy restatement: the backward
predicate equals the forward one on every record of the guided sections' generators, and whole small pairs matched with loops over
the header functions keep the rows the restatement keeps.  The pairs are the inputs of tests/test_gpu_match_mutual.py; that each of
its cases holds every class of row is shown here, on the restatement alone."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import ethzasl_brisk_amd as B
from test_abi_match_gated import restated as gate_restated
from test_abi_match_guided import IDENTITY, PAIR_BAD, PAIR_NO_MODEL, guide_records, restated as guide_restated, restated_centres
from test_abi_match_epiline import (RECTIFIED, cross, epiline_records, gate_view, is_guided, restated as epiline_restated, restated_band,
                                    restated_lines, scaled)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ethzasl_brisk_amd", "csrc")
NEW = ("brisk_hip_match_mutual_pairs_guided_device", "brisk_hip_match_mutual_pairs_epipolar_guided_device")
GUIDED = ("brisk_hip_match_knn_pairs_guided_device", "brisk_hip_match_knn_pairs_epipolar_guided_device")
COUNTED = ("k_guided_", "k_match_", "k_epiline_", "k_epipolar_", "k_verify_", "k_pair_select", "k_track_", "k_tracklist_", "k_refit_models",
           "k_tie_resolve")
INF, NAN = float("inf"), float("nan")
CENTRE, LINE = 0, 1


def arguments(hdr, name):
    """the declaration's argument list, one string per argument, white space squeezed"""
    m = re.search(r"\bint " + name + r"\(([^;]*)\);", hdr)
    assert m, name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_both_libraries_export_the_mutual_matchers():
    from ethzasl_brisk_amd import build
    hdr = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    declared = set(re.findall(r"\b(brisk_hip_[a-z_0-9]+)\s*\(", hdr))
    for lib in (build.build(), build.build_release()):
        L = ctypes.CDLL(lib)
        for s in NEW:
            assert s in declared, s
            assert s in B.ABI_SYMBOLS, s
            assert hasattr(L, s), (lib, s)
    for new, old in zip(NEW, GUIDED):                               # the guided k-NN calls' lists minus `int k`
        want = arguments(hdr, old)
        assert "int k" in want
        want.remove("int k")
        assert arguments(hdr, new) == want, new
    assert "NO CROSS CHECK in the guided form" not in hdr           # the sentence the new section replaces


def test_python_has_the_mutual_calls():
    lead = ["self", "query", "train", "pairs", "models", "guide", "rows_cap", "query_kps", "train_kps", "stream", "dim_bytes", "out", "download"]
    for fn in (B.Context.match_mutual_pairs_guided, B.Context.match_mutual_pairs_epipolar_guided):
        par = inspect.signature(fn).parameters
        assert list(par) == lead, fn.__name__
        for name in lead[6:-1]:
            assert par[name].default is None, (fn.__name__, name)
        assert par["download"].default is False
    # the existing calls keep their signatures
    assert list(inspect.signature(B.Context.match_knn_pairs_guided).parameters) == \
        ["self", "query", "train", "pairs", "k", "models", "guide", "rows_cap", "query_kps", "train_kps", "stream", "dim_bytes", "out", "download"]


def test_mutual_kernels_use_no_scratch():
    from ethzasl_brisk_amd import build
    build.build()
    res = build.kernel_resources()
    if not res:
        pytest.skip("the objects were not compiled here (no resource remarks beside them)")
    centre = {k: v for k, v in res.items() if "k_mutual_centre_knn" in k}
    line = {k: v for k, v in res.items() if "k_mutual_line_knn" in k}
    assert len(centre) == 4 and len(line) == 4                      # four descriptor sizes each
    for k, v in {**centre, **line}.items():
        assert v["scratch"] == 0, (k, v)
        for other in COUNTED:
            assert other not in k                                    # the sibling tests count kernels by these substrings


# ---- the backward predicate is the forward one ------------------------------------------------------------------------------------

def build_program(sanitize=False):
    """tests/cpp/test_match_mutual.cc: plain host C++ around the two rule headers (no HIP, no library)"""
    src = os.path.join(ROOT, "tests", "cpp", "test_match_mutual.cc")
    hdrs = [os.path.join(CSRC, f) for f in ("brisk_match_epiline.h", "brisk_match_guide.h", "brisk_match_gate.h", "brisk_pair_epipolar.h",
                                            "brisk_pair_verify.h")]
    out = os.path.join(ROOT, "tests", "cpp", "test_match_mutual" + ("_san" if sanitize else ""))
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in [src] + hdrs):
        extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off"] + extra + ["-I" + CSRC, "-o", out, src])
    return out


def run_program(prog, mode, path):
    out = subprocess.run([prog, mode, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    return out.stdout.split("\n")[:-1]


def check_predicates(prog, tmp_path):
    for mode, rec in (("centre", guide_records()[0]), ("line", epiline_records()[0])):
        M = guide_restated(rec)[3] if mode == "centre" else epiline_restated(rec)[5]
        path = tmp_path / (mode + ".bin")
        rec.tofile(path)
        got = np.array([[c == "1" for c in ln.split()] for ln in run_program(prog, mode, path)])
        assert got.shape == (len(rec), 2) and len(rec) >= 3000
        assert np.array_equal(got[:, 0], M), mode                   # (what the sibling tests show; the comparison below rests on it)
        bad = np.flatnonzero(got[:, 1] != got[:, 0])
        assert len(bad) == 0, (mode, len(bad), rec[bad[:3]])
        assert M.sum() > 500 and (~M).sum() > 500


def test_the_backward_predicate_is_the_forward_one(tmp_path):
    """brisk_guide_train_row / brisk_epiguide_train_row against brisk_guide_allows / brisk_epiguide_allows on every record of the two
    guided sections' generators"""
    check_predicates(build_program(), tmp_path)


# ---- whole pairs ------------------------------------------------------------------------------------------------------------------

class Pair:
    """one frame pair: keypoints (B.KEYPOINT) and descriptors ([n, dim] uint8) of both sides, and the pair's model record"""

    def __init__(self, kq, kt, dq, dt, model, hypothesis, flags):
        self.kq, self.kt, self.dq, self.dt, self.model, self.hypothesis, self.flags = kq, kt, dq, dt, model, hypothesis, flags


class Case:
    """the inputs of one call: pair p is frame p of the query set against frame p of the train set"""

    def __init__(self, form, dim, window, band, fallback, rows_cap, pairs):
        self.form, self.dim, self.window, self.band, self.fallback, self.rows_cap, self.pairs = form, dim, window, band, fallback, rows_cap, pairs

    def records(self):
        """the pairs' model records: B.PAIR_MODEL or B.PAIR_EPIPOLAR_MODEL"""
        rec = np.zeros(len(self.pairs), B.PAIR_EPIPOLAR_MODEL if self.form == LINE else B.PAIR_MODEL)
        for r, p in zip(rec, self.pairs):
            r["f" if self.form == LINE else "h"], r["hypothesis"], r["flags"] = p.model, p.hypothesis, p.flags
            r["records"], r["usable"], r["inliers"], r["valid"] = -1, -2, -3, -4      # (not read)
        return rec


def restated_mask(form, window, band, fallback, model, hypothesis, flags, kq, kt):
    """M[q][t] of a pair and, per query row, whether it takes part at all (has a centre / a line, or the fallback's plain gate):
    restated_centres, restated_lines, restated_band and the gate's restatement"""
    nq, nt = len(kq), len(kt)
    qx, qy = kq["x"].astype(np.float32), kq["y"].astype(np.float32)
    guided = bool(is_guided(hypothesis, flags))
    if form == CENTRE:
        cx, cy, has = restated_centres(np.asarray(model, np.float64), hypothesis, flags, fallback, qx, qy)
    else:
        cx, cy = qx, qy
        l0, l1, l2, w, has = restated_lines(np.asarray(model, np.float64), hypothesis, flags, np.float32(band), qx, qy)
        if not guided:
            has = np.full(nq, fallback != 0)
    if nq == 0 or nt == 0:
        return np.zeros((nq, nt), bool), np.asarray(has, bool).reshape(nq)
    qi, ti = np.repeat(np.arange(nq), nt), np.tile(np.arange(nt), nq)
    g = gate_view(window[:4], window[4], np.stack([cx[qi], cy[qi]], axis=1), kq["octave"][qi], np.stack([kt["x"][ti], kt["y"][ti]], axis=1),
                  kt["octave"][ti])
    M = gate_restated(g).reshape(nq, nt) & np.asarray(has, bool)[:, None]
    if form == LINE and guided:
        M &= restated_band(l0[:, None], l1[:, None], l2[:, None], w[:, None], kt["x"][None, :], kt["y"][None, :])
    return M, np.asarray(has, bool)


def distances(dq, dt, step=1 << 16):
    """all Hamming distances [len(dq), len(dt)]; `step` rows of dq at a time: the unpacked bits of millions of rows are never held"""
    b = np.unpackbits(dt, axis=1).astype(np.float32)
    out = np.zeros((len(dq), len(dt)), np.int64)
    for r0 in range(0, len(dq), step):
        a = np.unpackbits(dq[r0:r0 + step], axis=1).astype(np.float32)
        out[r0:r0 + step] = a @ (1 - b).T + (1 - a) @ b.T
    return out


def restated_mutual(case, pair):
    """the rule of the header's section in NumPy.  Returns per row q < min(n_a, rows_cap): f(q) (-1: none), its distance, kept; and the
    classes of rows the pair holds"""
    M, has = restated_mask(case.form, case.window, case.band, case.fallback, pair.model, pair.hypothesis, pair.flags, pair.kq, pair.kt)
    return mutual_under_mask(M, has, pair.dq, pair.dt, case.rows_cap)


def mutual_under_mask(M, has, dq, dt, rows_cap):
    """forward, backward, kept under a given mask M [n_a, n_b]; has [n_a]: the rows that take part at all (only the classes read it)"""
    M, has = np.asarray(M, bool), np.asarray(has, bool)
    na, nb = len(dq), len(dt)
    rows = min(na, rows_cap)
    ft, fd, kept = np.full(rows, -1), np.zeros(rows, np.int64), np.zeros(rows, bool)
    classes = dict.fromkeys(("kept", "dropped", "dropped_beyond_cap", "forward_tie", "backward_tie", "absent_would_win"), 0)
    if na == 0 or nb == 0:
        return ft, fd, kept, classes
    D = distances(dq, dt)
    BIG = np.int64(1) << 40
    fkey = np.where(M, (D << 22) | np.arange(nb)[None, :], BIG)
    bkey = np.where(M, (D << 22) | np.arange(na)[:, None], BIG)
    anykey = (D << 22) | np.arange(na)[:, None]                     # the backward keys with the mask left out
    for q in range(rows):
        t = int(np.argmin(fkey[q]))
        if fkey[q, t] == BIG:
            continue
        ft[q], fd[q] = t, D[q, t]
        g = int(np.argmin(bkey[:, t]))
        kept[q] = g == q
        classes["kept"] += int(kept[q])
        classes["dropped"] += int(not kept[q])
        classes["dropped_beyond_cap"] += int(not kept[q] and g >= rows_cap)
        classes["forward_tie"] += int((M[q] & (D[q] == D[q, t])).sum() >= 2)
        classes["backward_tie"] += int((M[:, t] & (D[:, t] == D[g, t])).sum() >= 2)
        classes["absent_would_win"] += int((~has & (anykey[:, t] < bkey[g, t])).any())
    return ft, fd, kept, classes


def low_entropy(rng, n, dim):
    return (rng.integers(0, 4, (n, dim), dtype=np.uint8) * 85).astype(np.uint8)


def grid_keypoints(rng, n, nan_every):
    k = np.frombuffer(rng.integers(0, 256, max(n, 1) * B.KEYPOINT.itemsize, dtype=np.uint8).tobytes(), B.KEYPOINT)[:n].copy()
    k["x"], k["y"], k["octave"] = 8.0 * rng.integers(0, 8, n), 8.0 * rng.integers(0, 6, n), rng.integers(0, 4, n)
    if nan_every:
        k["x"][3::nan_every] = np.nan
        k["y"][11::2 * nan_every] = np.nan
    return k


# where the planted query keypoints lie: far from the grid of the random rows and from each other, so that each group's rows see only
# each other through any of the windows used here
SPOTS = [(1000.0 + 100.0 * g, 1000.0 + 100.0 * g) for g in range(6)]
# z = x - 24 maps the far spots onto one another; near its pole the images lie hundreds of pixels apart
Z_POLE = (10.0, 0.0, 0.0, 0.0, 10.0, 0.0, 1.0, 0.0, -24.0)
Z_POLE_SPOTS = [(25.0, 0.0), (26.0, 0.0), (23.0, 0.0), (22.0, 0.0), (25.0, 20.0), (23.0, 20.0)]


def make_pair(rng, form, dim, na, nb, rows_cap, model, hypothesis, flags, fallback, absent="nan"):
    """random rows on a coarse grid - low-entropy descriptors, some NaN coordinates - and, where the pair is large enough (n_a >
    rows_cap + 1, n_b >= 7, n_a >= 12), six planted groups of rows that see only each other:
      kept             a[4] and b[0] carry one descriptor
      dropped          a[2] is two bits from b[1], a[3] equals it: b[1] answers a[3]
      beyond the cap   a[5] is two bits from b[2], the LAST row of frame a (>= rows_cap) equals it
      forward tie      b[3] and b[4] carry a[6]'s descriptor at one position: the smaller index
      backward tie     a[7] and a[8] carry b[5]'s descriptor: the smaller index is kept, the larger dropped
      absent row       a[9] equals b[6] but has no centre / no line (absent: a NaN coordinate, or the position `absent`); a[10], two
                       bits away, is kept"""
    kq, kt = grid_keypoints(rng, na, 17), grid_keypoints(rng, nb, 23)
    dq, dt = low_entropy(rng, na, dim), low_entropy(rng, nb, dim)
    if na > rows_cap + 1 and na >= 12 and nb >= 7:
        spots = Z_POLE_SPOTS if tuple(model) == Z_POLE else SPOTS
        guided = bool(is_guided(hypothesis, flags))

        def image(x, y):
            if form == LINE or not guided:
                return x, y
            cx, cy, _ = restated_centres(np.asarray(model, np.float64), hypothesis, flags, 1, np.float32(x), np.float32(y))
            return (float(np.round(cx * 4) / 4), float(np.round(cy * 4) / 4)) if np.isfinite(cx) and np.isfinite(cy) else (x, y)

        def put(k, i, xy):
            k["x"][i], k["y"][i], k["octave"][i] = xy[0], xy[1], 1

        fresh = rng.integers(0, 256, (6, dim), dtype=np.uint8)
        near = fresh.copy()
        near[:, 0] ^= 3
        groups = [([(4, fresh[0])], [(0, fresh[0])]),
                  ([(2, near[1]), (3, fresh[1])], [(1, fresh[1])]),
                  ([(5, near[2]), (na - 1, fresh[2])], [(2, fresh[2])]),
                  ([(6, fresh[3])], [(3, fresh[3]), (4, fresh[3])]),
                  ([(7, fresh[4]), (8, fresh[4])], [(5, fresh[4])]),
                  ([(10, near[5])], [(6, fresh[5])])]
        for spot, (qs, ts) in zip(spots, groups):
            for i, d in qs:
                put(kq, i, spot)
                dq[i] = d
            for i, d in ts:
                put(kt, i, image(*spot))
                dt[i] = d
        put(kq, 9, (NAN, spots[5][1]) if absent == "nan" else absent)
        dq[9] = fresh[5]
    return Pair(kq, kt, dq, dt, tuple(model), hypothesis, flags)


SIZES = [0, 1, 5, 63, 64, 65, 130, 777]
ROWS_CAP = 128
# every size on either side, the large ones against each other: several workgroups per pair, n_a > rows_cap, fewer rows than waves, and
# 777 = 8 slices of 98 rows - a second, partial staging block
EQUAL_COUNTS = [(777, 777), (130, 777), (777, 130), (130, 130), (777, 65), (65, 777), (64, 64), (63, 5), (5, 63), (1, 1), (0, 777), (777, 0),
                (1, 64), (64, 1), (130, 0), (0, 0), (5, 5), (65, 63), (777, 64), (130, 63)]
EQUAL_WINDOW = (-16.0, 16.0, -8.0, 8.0, 1)
GARBAGE = (NAN, 1e300, -INF, 0.0, 0.0, 5.0, 0.0, 0.0, 0.0)
DIMS = [(16, 20, 0, 0), (32, 48, 0, 4), (48, 64, 0, 0), (48, 51, 1, 3), (64, 64, 0, 0)]   # dim, row pitch, base offset, frame slack


def equal_case(form, dim, seed):
    """consequence 1: identity models (centre) or any F under band = +inf (line) in the even pairs, unguided pairs under the fallback in
    the odd ones - the gated matcher's mask in both"""
    rng = np.random.default_rng(seed)
    pairs = []
    for p, (na, nb) in enumerate(EQUAL_COUNTS):
        if p % 2 == 0:
            model, hyp, flags = (IDENTITY if form == CENTRE else scaled(RECTIFIED, [1.0, 0.5, -2.0][p % 3])), p, 0
        else:
            model, hyp, flags = GARBAGE, [-1, 3, 0][p % 3], [0, PAIR_BAD, PAIR_NO_MODEL][p % 3]
        pairs.append(make_pair(rng, form, dim, na, nb, ROWS_CAP, model, hyp, flags, 1))
    return Case(form, dim, EQUAL_WINDOW, INF, 1, ROWS_CAP, pairs)


GENERAL_COUNTS = [(140, 70), (130, 33), (200, 64), (65, 0), (5, 9), (131, 130), (0, 5), (150, 40), (133, 20), (140, 64)]
GENERAL_WINDOW = (-8.0, 8.0, -8.0, 8.0)
EPIPOLE = (2000.0, 304.0)


def general_models(form, rng):
    """(model, hypothesis, flags, where the absent row lies) per pair of GENERAL_COUNTS"""
    if form == CENTRE:
        a = rng.uniform(-0.02, 0.02, 4)
        near_identity = (1 + a[0], a[1], 3.0, a[2], 1 + a[3], -2.0, 1e-5, -2e-5, 1.0)
        return [((1.0, 0.0, 8.0, 0.0, 1.0, -8.0, 0.0, 0.0, 1.0), 0, 0, "nan"), (near_identity, 7, 0x100, "nan"), (Z_POLE, 4095, 0x1, (24.0, 0.0)),
                (IDENTITY, 1, 0, "nan"), ((1.0, 0.0, 0.0, 0.0, 1.0, NAN, 0.0, 0.0, 1.0), 1, 0, "nan"), (GARBAGE, -1, 0, "nan"),
                (IDENTITY, 2, 0, "nan"), (tuple(-e for e in near_identity), 3, 0, "nan"), (GARBAGE, 3, PAIR_NO_MODEL, "nan"),
                ((0.0,) * 9, 2, 0, "nan")]
    return [(scaled(RECTIFIED, 1.0), 0, 0, "nan"), (cross(*EPIPOLE), 7, 0x100, EPIPOLE), (scaled(RECTIFIED, -2.0), 4095, 0x1, "nan"),
            (cross(*EPIPOLE), 1, 0, "nan"), ((0.0, 0.0, 0.0, 0.0, 0.0, NAN, 0.0, 1.0, 0.0), 1, 0, "nan"), (GARBAGE, -1, 0, "nan"),
            (RECTIFIED, 2, 0, "nan"), (scaled(cross(*EPIPOLE), 0.5), 3, 0, EPIPOLE), (GARBAGE, 3, PAIR_NO_MODEL, "nan"), ((0.0,) * 9, 2, 0, "nan")]


def general_case(form, dim, max_octave_diff, fallback, seed):
    """a model per pair: translations, near-identity homographies and the model with a pole (centre), rectified and translating rigs
    (line), models that guide nothing, unguided pairs; n_b = 0 and n_a = 0 among the pairs"""
    rng = np.random.default_rng(seed)
    models = general_models(form, rng)
    pairs = [make_pair(rng, form, dim, na, nb, ROWS_CAP, m, hyp, flags, fallback, absent)
             for (na, nb), (m, hyp, flags, absent) in zip(GENERAL_COUNTS, models)]
    return Case(form, dim, GENERAL_WINDOW + (max_octave_diff,), 3.0, fallback, ROWS_CAP, pairs)


# the GPU tests' parametrised cases, by the names they use
EQUAL_CASES = {(form, dim, pitch): (form, dim, 100 * dim + pitch + form) for form in (CENTRE, LINE) for dim, pitch, _, _ in DIMS}
GENERAL_CASES = {(form, mod): (form, [16, 32, 48, 64][2 * form + mod], mod, mod, 7 + 2 * form + mod) for form in (CENTRE, LINE) for mod in (0, 1)}
MEMORY_CASES = {form: (form, 48, 1, 0, 31 + form) for form in (CENTRE, LINE)}


def all_cases():
    for key, args in EQUAL_CASES.items():
        yield ("equal",) + key, equal_case(*args)
    for key, args in GENERAL_CASES.items():
        yield ("general",) + key, general_case(*args)
    for key, args in MEMORY_CASES.items():
        yield ("memory", key), general_case(*args)


def test_every_gpu_case_holds_every_class_of_row():
    """on the restatement alone: a kept row, a row the backward scan drops, a row dropped by a competitor at or beyond rows_cap, a
    forward and a backward tie decided by index, and a query row without a centre (or line) that would otherwise have won"""
    for name, case in all_cases():
        total = {}
        for pair in case.pairs:
            for k, v in restated_mutual(case, pair)[3].items():
                total[k] = total.get(k, 0) + v
        for k, v in total.items():
            assert v >= 1, (name, total)
        guided = [bool(is_guided(p.hypothesis, p.flags)) for p in case.pairs]
        assert any(guided) and not all(guided), name


def test_the_planted_groups_do_what_they_say():
    case = general_case(CENTRE, 48, 1, 0, 5)
    ft, fd, kept, _ = restated_mutual(case, case.pairs[0])          # the translation, 140 x 70
    na = len(case.pairs[0].kq)
    assert na - 1 >= ROWS_CAP
    assert (ft[4], fd[4], kept[4]) == (0, 0, True)
    assert (ft[2], fd[2], kept[2]) == (1, 2, False) and (ft[3], fd[3], kept[3]) == (1, 0, True)
    assert (ft[5], fd[5], kept[5]) == (2, 2, False)
    assert (ft[6], fd[6], kept[6]) == (3, 0, True)
    assert (ft[7], kept[7], ft[8], kept[8]) == (5, True, 5, False)
    assert ft[9] == -1 and (ft[10], fd[10], kept[10]) == (6, 2, True)
    zp = restated_mutual(case, case.pairs[2])                       # the model with a pole: the absent row lies on it
    assert zp[0][9] == -1 and (zp[0][10], zp[2][10]) == (6, True) and (zp[0][5], zp[2][5]) == (2, False)


def write_pairs(case, path):
    hdr = np.dtype([("i", "<i4", (9,)), ("f", "<f4", (5,)), ("model", "<f8", (9,))])
    kp3 = np.dtype([("x", "<f4"), ("y", "<f4"), ("octave", "<i4")])
    with open(path, "wb") as f:
        for p in case.pairs:
            h = np.zeros((), hdr)
            h["i"] = (case.form, len(p.kq), len(p.kt), case.rows_cap, case.dim // 4, p.hypothesis, p.flags, case.fallback, case.window[4])
            h["f"], h["model"] = case.window[:4] + (case.band,), p.model
            f.write(h.tobytes())
            for k in (p.kq, p.kt):
                k3 = np.zeros(len(k), kp3)
                k3["x"], k3["y"], k3["octave"] = k["x"], k["y"], k["octave"]
                f.write(k3.tobytes())
            f.write(np.ascontiguousarray(p.dq).tobytes())
            f.write(np.ascontiguousarray(p.dt).tobytes())


def check_pairs(prog, tmp_path):
    cases = [general_case(*GENERAL_CASES[key]) for key in GENERAL_CASES] + [equal_case(CENTRE, 16, 1), equal_case(LINE, 32, 2)]
    for n, case in enumerate(cases):
        path = tmp_path / ("pairs%d.bin" % n)
        write_pairs(case, path)
        lines = iter(run_program(prog, "pairs", path))
        kept_total = 0
        for p, pair in enumerate(case.pairs):
            ft, fd, kept, _ = restated_mutual(case, pair)
            assert next(lines).split() == ["pair", str(p), str(len(ft))]
            got = np.array([[int(v) for v in next(lines).split()] for _ in range(len(ft))], np.int64).reshape(len(ft), 4)
            assert np.array_equal(got[:, 0], np.arange(len(ft)))
            assert np.array_equal(got[:, 1], ft) and np.array_equal(got[:, 2], fd) and np.array_equal(got[:, 3] == 1, kept), (n, p)
            kept_total += int(kept.sum())
        assert next(lines, None) is None and kept_total > 50


def test_whole_pairs_agree_with_the_restatement(tmp_path):
    check_pairs(build_program(), tmp_path)


def test_the_rule_under_sanitizers(tmp_path):
    """the same program with the address and undefined-behaviour sanitizers, run stand-alone (nothing sanitized is loaded into
    Python)"""
    prog = build_program(sanitize=True)
    check_predicates(prog, tmp_path)
    check_pairs(prog, tmp_path)

"""CPU checks of the epipolar-guided pair matchers' boundary: both libraries export the two entry points the header declares, Python
has the structure and the calls, the eight kernels touch no scratch memory, and the rule - the very functions the kernels call
(csrc/brisk_match_epiline.h), built here for the host - agrees with a NumPy restatement: the line and the band's bound bit for bit,
has-line and the mask M."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import ethzasl_brisk_amd as B
from test_abi_epipolar import restated_inliers8
from test_abi_match_gated import gate_records, restated as gate_restated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ethzasl_brisk_amd", "csrc")
NEW = ("brisk_hip_match_knn_pairs_epipolar_guided_device", "brisk_hip_match_radius_pairs_epipolar_guided_device")
PAIR_BAD, PAIR_NO_MODEL = 0x2, 0x8
INF, NAN = float("inf"), float("nan")


def test_both_libraries_export_the_epipolar_guided_matchers():
    from ethzasl_brisk_amd import build
    hdr = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    declared = set(re.findall(r"\b(brisk_hip_[a-z_0-9]+)\s*\(", hdr))
    for lib in (build.build(), build.build_release()):
        L = ctypes.CDLL(lib)
        for s in NEW:
            assert s in declared, s
            assert s in B.ABI_SYMBOLS, s
            assert hasattr(L, s), (lib, s)
    assert re.search(r"typedef struct brisk_hip_match_epipolar_guide\b", hdr)
    # the model argument is the epipolar record: a homography record does not compile in
    for s in NEW:
        assert re.search(s + r"\([^;]*const brisk_hip_pair_epipolar_model\* d_models,\s*const brisk_hip_match_epipolar_guide\* guide", hdr), s
    # the verifier's header text no longer lists the second pass under what is not done
    not_done = re.search(r"Not done here: essential matrices \(no intrinsics enter\).*?\*/", hdr, re.S).group(0)
    not_done = " ".join(not_done.replace("\n *", " ").split())
    assert "guided matching along epipolar lines" not in not_done.split(". ")[0] and "matched again inside a band" in not_done


def test_python_has_the_epipolar_guide():
    assert ctypes.sizeof(B.MatchEpipolarGuide) == 28
    g = B.MatchEpipolarGuide.around(3)
    w = g.window
    assert (w.dx_min, w.dx_max, w.dy_min, w.dy_max, w.max_octave_diff, g.band, g.fallback) == (-INF, INF, -INF, INF, -1, 3.0, 0)
    g = B.MatchEpipolarGuide.around(2.5, window=(-64, 0, -INF, INF), max_octave_diff=1, fallback=1)
    w = g.window
    assert (w.dx_min, w.dx_max, w.dy_min, w.dy_max, w.max_octave_diff, g.band, g.fallback) == (-64.0, 0.0, -INF, INF, 1, 2.5, 1)
    g = B.MatchEpipolarGuide.around(1, window=B.MatchGate(-1, 2, -3, 4, 7))
    assert (g.window.dx_min, g.window.dy_max, g.window.max_octave_diff) == (-1.0, 4.0, -1)
    for fn, lead in ((B.Context.match_knn_pairs_epipolar_guided, ["self", "query", "train", "pairs", "k", "models", "guide"]),
                     (B.Context.match_radius_pairs_epipolar_guided,
                      ["self", "query", "train", "pairs", "max_distance", "cap_per_query", "models", "guide"])):
        par = inspect.signature(fn).parameters
        assert list(par)[:len(lead)] == lead
        assert list(par)[len(lead):] == ["rows_cap", "query_kps", "train_kps", "stream", "dim_bytes", "out", "download"]
        for name in ("rows_cap", "query_kps", "train_kps", "stream", "dim_bytes", "out"):
            assert par[name].default is None, (fn.__name__, name)
        assert "cross_check" not in par
    # the existing calls keep their signatures
    assert list(inspect.signature(B.Context.match_knn_pairs_guided).parameters) == \
        ["self", "query", "train", "pairs", "k", "models", "guide", "rows_cap", "query_kps", "train_kps", "stream", "dim_bytes", "out", "download"]
    assert list(inspect.signature(B.MatchGuide.around).parameters) == ["radius", "max_octave_diff", "fallback"]


def test_epiline_kernels_use_no_scratch():
    from ethzasl_brisk_amd import build
    build.build()
    res = build.kernel_resources()
    if not res:
        pytest.skip("the objects were not compiled here (no resource remarks beside them)")
    knn = {k: v for k, v in res.items() if "k_epiline_knn_pairs" in k}
    radius = {k: v for k, v in res.items() if "k_epiline_radius_pairs" in k}
    assert len(knn) == 4 and len(radius) == 4                       # four descriptor sizes each
    sib_knn = {v["lds"] for k, v in res.items() if "k_guided_knn_pairs" in k}
    sib_radius = {v["lds"] for k, v in res.items() if "k_guided_radius_pairs" in k}
    for k, v in {**knn, **radius}.items():
        assert v["scratch"] == 0, (k, v)
        assert {v["lds"]} == (sib_knn if k in knn else sib_radius), (k, v)     # no LDS beyond the guided siblings'
        for other in ("k_guided_", "k_match_", "k_epipolar_", "k_verify_", "k_pair_select", "k_track_"):
            assert other not in k                                    # the sibling tests count kernels by these substrings


def test_the_rule_s_header_is_in_the_kernel_revision(tmp_path, monkeypatch):
    import shutil
    from ethzasl_brisk_amd import build
    rev = build.kernel_revision()
    copy = tmp_path / "csrc"
    shutil.copytree(CSRC, copy)
    with open(copy / "brisk_match_epiline.h", "a") as f:
        f.write("// changed\n")
    monkeypatch.setattr(build, "CSRC", str(copy))
    assert build.kernel_revision() != rev


# ---- the rule -------------------------------------------------------------------------------------------------------------------

REC = np.dtype([("f", "<f8", (9,)), ("hypothesis", "<i4"), ("flags", "<i4"), ("window", "<f4", (4,)), ("max_octave_diff", "<i4"),
                ("band", "<f4"), ("fallback", "<i4"), ("q", "<f4", (2,)), ("qo", "<i4"), ("t", "<f4", (2,)), ("to", "<i4"), ("pad", "<i4")])
assert REC.itemsize == 136


def build_program(sanitize=False):
    """tests/cpp/test_match_epiline.cc: plain host C++ around csrc/brisk_match_epiline.h (no HIP, no library)"""
    src = os.path.join(ROOT, "tests", "cpp", "test_match_epiline.cc")
    hdrs = [os.path.join(CSRC, f) for f in ("brisk_match_epiline.h", "brisk_match_guide.h", "brisk_match_gate.h", "brisk_pair_epipolar.h",
                                            "brisk_pair_verify.h")]
    out = os.path.join(ROOT, "tests", "cpp", "test_match_epiline" + ("_san" if sanitize else ""))
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in [src] + hdrs):
        extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off"] + extra + ["-I" + CSRC, "-o", out, src])
    return out


def run_program(prog, rec, path):
    rec.tofile(path)
    out = subprocess.run([prog, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    return out.stdout.split("\n")[:-1]


def is_guided(hypothesis, flags):
    return (np.asarray(hypothesis) >= 0) & ((np.asarray(flags) & (PAIR_BAD | PAIR_NO_MODEL)) == 0)


def restated_lines(f, hypothesis, flags, band, x, y):
    """the header's words in NumPy: float64 elementwise (a*b + c*d) + e.  f [..., 9]; band, x, y float32.  Returns l0, l1, l2, w
    (zeros in an unguided pair, whose line is not made) and has-line."""
    f = np.asarray(f, np.float64)
    band, x, y = np.asarray(band, np.float32), np.asarray(x, np.float32), np.asarray(y, np.float32)
    guided = is_guided(hypothesis, flags)
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    with np.errstate(all="ignore"):
        l0 = (f[..., 0] * xd + f[..., 1] * yd) + f[..., 2]
        l1 = (f[..., 3] * xd + f[..., 4] * yd) + f[..., 5]
        l2 = (f[..., 6] * xd + f[..., 7] * yd) + f[..., 8]
        n = l0 * l0 + l1 * l1
        b2 = band.astype(np.float64) * band.astype(np.float64)
        w = b2 * n
        has = guided & (band > np.float32(0)) & (n > 0) & ((n - n) == 0) & ((l2 - l2) == 0)
    zero = np.float64(0)
    return tuple(np.where(guided, v, zero) for v in (l0, l1, l2, w)) + (has,)


def restated_band(l0, l1, l2, w, tx, ty):
    with np.errstate(all="ignore"):
        r = (np.asarray(tx, np.float32).astype(np.float64) * l0 + np.asarray(ty, np.float32).astype(np.float64) * l1) + l2
        return r * r <= w


def gate_view(window, max_octave_diff, q, qo, t, to):
    """test_abi_match_gated's record layout of these fields, for its restated()"""
    n = len(qo)
    g = np.zeros((n, 11), np.uint32)
    g[:, 0:4] = np.asarray(window, np.float32).view(np.uint32)
    g[:, 4] = np.asarray(max_octave_diff, np.int32).view(np.uint32)
    g[:, 5:7] = np.asarray(q, np.float32).view(np.uint32)
    g[:, 7] = np.asarray(qo, np.int32).view(np.uint32)
    g[:, 8:10] = np.asarray(t, np.float32).view(np.uint32)
    g[:, 10] = np.asarray(to, np.int32).view(np.uint32)
    return g


def restated(rec):
    l0, l1, l2, w, has = restated_lines(rec["f"], rec["hypothesis"], rec["flags"], rec["band"], rec["q"][:, 0], rec["q"][:, 1])
    band_ok = restated_band(l0, l1, l2, w, rec["t"][:, 0], rec["t"][:, 1])
    gate = gate_restated(gate_view(rec["window"], rec["max_octave_diff"], rec["q"], rec["qo"], rec["t"], rec["to"]))
    guided = is_guided(rec["hypothesis"], rec["flags"])
    M = np.where(guided, has & band_ok & gate, (rec["fallback"] != 0) & gate)
    return l0, l1, l2, w, has, M


ALL_PASS = (-INF, INF, -INF, INF, -1)
WIDE = (-300.0, 300.0, -300.0, 300.0, 1)
DISPARITY = (-16.0, 16.0, -INF, INF, 1)
RECTIFIED = (0.0, 0.0, 0.0, 0.0, 0.0, -1.0, 0.0, 1.0, 0.0)


def scaled(f, s):
    return tuple(e * s + 0.0 for e in f)                             # (+ 0.0: no negative zeros from the scaling)


def vertical(c):
    """the line of (x, y) is x' = x + c: r = x' - x - c exactly on the grid"""
    return (0.0, 0.0, 1.0, 0.0, 0.0, 0.0, -1.0, 0.0, -c)


def cross(ex, ey):
    """[e]_x of e = (ex, ey, 1): rank 2, F e = 0 exactly"""
    return (0.0, -1.0, ey, 1.0, 0.0, -ex, -ey, ex, 0.0)


def epiline_records():
    """(records, kind of each, the gate's own records used).  Coordinates lie on a quarter-pixel grid; T is placed around the restated
    line so that both answers of M occur."""
    rng = np.random.default_rng(2026)
    recs, kinds = [], []

    def add(kind, f, q, t, hypothesis=0, flags=0, window=WIDE, band=3.0, fallback=0):
        r = np.zeros((), REC)
        r["f"], r["hypothesis"], r["flags"], r["window"], r["max_octave_diff"] = f, hypothesis, flags, window[:4], window[4]
        r["band"], r["fallback"], r["q"], r["qo"], r["t"], r["to"] = band, fallback, q[:2], q[2], t[:2], t[2]
        recs.append(r)
        kinds.append(kind)

    def grid_q():
        return (rng.integers(0, 400) / 4, rng.integers(0, 400) / 4, int(rng.integers(0, 4)))

    def near_q(q, spread=80):
        return (q[0] + rng.integers(-spread, spread + 1) / 4, q[1] + rng.integers(-spread, spread + 1) / 4, q[2] + int(rng.integers(-2, 3)))

    def near_line(f, q, band=3.0):
        """a train keypoint up to 2 band from the line of q under f and up to 30 pixels along it from q's foot, on the quarter-pixel grid"""
        l0, l1, l2, _, _ = restated_lines(f, 0, 0, np.float32(1), np.float32(q[0]), np.float32(q[1]))
        n = float(l0 * l0 + l1 * l1)
        if not np.isfinite(n) or n <= 0 or not np.isfinite(l2):
            return near_q(q)
        s = n ** 0.5
        nx, ny = float(l0) / s, float(l1) / s
        d0 = (q[0] * float(l0) + q[1] * float(l1) + float(l2)) / s   # q's own distance to its line in the train image
        off, along = rng.uniform(-2 * band, 2 * band), rng.uniform(-30, 30)
        x, y = q[0] - (d0 - off) * nx - along * ny, q[1] - (d0 - off) * ny + along * nx
        if abs(x) > 1e5 or abs(y) > 1e5:
            return near_q(q)
        return (round(x * 4) / 4, round(y * 4) / 4, q[2] + int(rng.integers(-2, 3)))

    def random_f():
        f = rng.uniform(-1, 1, 9)
        f[[0, 1, 3, 4]] *= 1e-2                                      # (lines that pass near the image, as an F of two cameras has)
        f[8] *= 50
        return tuple(f / np.abs(f).max())

    for i in range(600):                                             # random models scaled to largest element 1, and their negations
        f, q = random_f(), grid_q()
        t = near_line(f, q)
        win = [WIDE, ALL_PASS][i % 2]
        add("random", f, q, t, window=win)
        add("negated", tuple(-e for e in f), q, t, window=win)
    for i in range(450):                                             # rectified stereo at three scales: |y' - y| <= band, exactly
        q = grid_q()
        s = [1.0, 0.5, -2.0][i % 3]
        band = [8.0, 2.5, 0.25][(i // 3) % 3]
        t = (q[0] + rng.integers(-100, 101) / 4, q[1] + rng.integers(-int(band * 8), int(band * 8) + 1) / 4, q[2] + int(rng.integers(-2, 3)))
        add("rectified", scaled(RECTIFIED, s), q, t, window=DISPARITY, band=band, hypothesis=[0, 4095][i % 2], flags=[0, 0x100][i % 2])
    for i in range(300):                                             # train points exactly on the bound, and a quarter pixel beyond
        q = grid_q()
        c = rng.integers(-200, 201) / 4
        band = [3.0, 0.5, 6.25][i % 3]
        e = [band, -band, band + 0.25, -band - 0.25][(i // 3) % 4]
        add("bound" if abs(e) == band else "beyond", vertical(c), q, (q[0] + c + e, q[1] + rng.integers(-40, 41) / 4, q[2]), band=band)
    for i in range(240):                                             # a query exactly at the epipole of [e]_x, and queries around it
        e = grid_q()
        q = e if i % 2 == 0 else (e[0] + rng.integers(1, 80) / 4, e[1] + rng.integers(-80, 81) / 4, e[2])
        add("epipole" if i % 2 == 0 else "epipole_off", cross(e[0], e[1]), q, near_line(cross(e[0], e[1]), q) if i % 2 else near_q(q),
            window=ALL_PASS)
    for i in range(160):                                             # NaN / infinite / zero / huge models
        q = grid_q()
        f = list(random_f())
        f[rng.integers(0, 9)] = NAN
        add("nan_model", f, q, near_q(q), window=ALL_PASS)
        f = list(random_f())
        f[rng.integers(0, 9)] = [INF, -INF][i % 2]
        add("inf_model", f, q, near_q(q), window=ALL_PASS)
        add("huge_model", scaled(random_f(), 1e200), q, near_q(q), window=ALL_PASS)
        if i % 4 == 0:
            add("zero_model", (0.0,) * 9, q, near_q(q), window=ALL_PASS)
    for i in range(160):                                             # NaN keypoints, on either side
        q, f = grid_q(), random_f()
        t = list(near_line(f, q))
        if i % 2:
            bad = list(q)
            bad[(i // 2) % 2] = NAN
            add("nan_query", f, bad, t, window=ALL_PASS)
        else:
            t[(i // 2) % 2] = NAN
            add("nan_train", f, q, t, window=ALL_PASS)
    for i in range(300):                                             # the band itself: zero, negative, NaN, +inf, subnormal
        q = grid_q()
        c = rng.integers(-80, 81) / 4
        kind, band = [("band_zero", 0.0), ("band_zero", -0.0), ("band_negative", -3.0), ("band_nan", NAN), ("band_inf", INF),
                      ("band_subnormal", 1e-40)][i % 6]
        dx = [0.0, 0.0, 0.25, -7.5][(i // 6) % 4]                    # on the line twice as often as off it
        add(kind, vertical(c), q, (q[0] + c + dx, q[1] + rng.integers(-400, 401) / 4, q[2] + int(rng.integers(-2, 3))), band=band)
    garbage = (NAN, 1e300, -INF, 0.0, 0.0, 5.0, 0.0, 0.0, 0.0)
    for i in range(480):                                             # pairs without a usable model, both fallbacks; the model is not read
        q = grid_q()
        hyp, fl = [(-1, 0), (3, PAIR_BAD), (0, PAIR_NO_MODEL), (-1, PAIR_BAD | PAIR_NO_MODEL), (5, PAIR_NO_MODEL | 0x100), (-(2 ** 31), 0)][i % 6]
        fb = [0, 1, -7][(i // 6) % 3]
        f = garbage if i % 2 else scaled(RECTIFIED, 1.0)
        add("unguided_fallback" if fb else "unguided", f, q, near_q(q), hypothesis=hyp, flags=fl, fallback=fb, window=(-10.0, 10.0, -10.0, 10.0, 1),
            band=[3.0, NAN, 0.0][i % 3])
    for i in range(160):                                             # flag bits that do NOT unguide a pair
        f, q = random_f(), grid_q()
        add("other_flags", f, q, near_line(f, q), hypothesis=int(rng.integers(0, 4096)), flags=[0x1, 0x4, 0x100, 0x115][i % 4], fallback=i % 2)
    # the gate's own special records: as the fallback of an unguided pair, and under a band that passes everything
    g = gate_records()
    gf, gi = g.view(np.float32), g.view(np.int32)
    for j in range(0, len(g), 2):
        win = (gf[j, 0], gf[j, 1], gf[j, 2], gf[j, 3], int(gi[j, 4]))
        q, t = (gf[j, 5], gf[j, 6], int(gi[j, 7])), (gf[j, 8], gf[j, 9], int(gi[j, 10]))
        add("gate_fallback", garbage, q, t, hypothesis=-1, window=win, fallback=1, band=NAN)
        add("gate_all_pass_band", scaled(RECTIFIED, 1.0), q, t, window=win, band=INF)
    return np.array(recs, REC), np.array(kinds), g[::2]


def canonical(bits, values):
    """a NaN's payload is not the rule's business: every NaN compares as one pattern"""
    return np.where(np.isnan(values), np.uint64(0x7FF8000000000000), bits)


def parse(lines):
    cols = [ln.split() for ln in lines]
    vals = [np.array([int(c[i], 16) for c in cols], np.uint64) for i in range(4)]
    return [canonical(v, v.view(np.float64)) for v in vals] + [np.array([c[4] == "1" for c in cols]), np.array([c[5] == "1" for c in cols])]


def test_the_restatement_is_not_vacuous():
    """what the comparison below rests on, shown on the restatement alone"""
    rec, kinds, gate = epiline_records()
    assert len(rec) >= 3000
    l0, l1, l2, w, has, M = restated(rec)
    for kind in ("random", "negated", "rectified", "epipole_off", "band_inf", "band_subnormal", "unguided_fallback", "other_flags",
                 "gate_fallback", "gate_all_pass_band"):             # both answers of M where both can occur
        sel = kinds == kind
        assert sel.sum() >= 40 and M[sel].any() and (~M[sel]).any(), kind
    for kind in ("random", "negated", "rectified", "bound", "beyond", "epipole_off", "nan_train", "band_inf", "band_subnormal", "other_flags"):
        assert has[kinds == kind].all(), kind                        # finite models and queries, a positive band: always a line
    for kind in ("epipole", "nan_model", "inf_model", "zero_model", "huge_model", "nan_query", "band_zero", "band_negative", "band_nan",
                 "unguided"):                                        # kinds that must have no line
        sel = kinds == kind
        assert sel.sum() >= 40 and not has[sel].any() and not M[sel].any(), kind
    assert not M[kinds == "nan_train"].any()                         # a NaN r fails
    assert not has[kinds == "unguided_fallback"].any() and not has[kinds == "gate_fallback"].any()   # (no line is made: the plain gate)
    # the epipole: l = 0 exactly; the huge model: n overflows
    sel = kinds == "epipole"
    assert (l0[sel] == 0).all() and (l1[sel] == 0).all() and (l2[sel] == 0).all()
    sel = kinds == "huge_model"
    with np.errstate(all="ignore"):
        assert np.isinf(l0[sel] * l0[sel] + l1[sel] * l1[sel]).all() and np.isfinite(l0[sel]).all()
    # the negated model has the same mask, and the same w bit for bit
    p, n = kinds == "random", kinds == "negated"
    assert np.array_equal(M[p], M[n]) and np.array_equal(w[p].view(np.uint64), w[n].view(np.uint64)) and np.array_equal(l0[p], -l0[n])
    # exactly on the bound passes (the interval is closed), a quarter pixel beyond does not
    sel = kinds == "bound"
    assert sel.sum() > 100 and M[sel].all()
    sel = kinds == "beyond"
    assert sel.sum() > 100 and not M[sel].any()
    # a band of +inf passes whatever the gate passes; a subnormal band passes the points exactly on the line, and only those
    sel = kinds == "band_inf"
    assert np.isinf(w[sel]).all()
    gate_all = gate_restated(gate_view(rec["window"], rec["max_octave_diff"], rec["q"], rec["qo"], rec["t"], rec["to"]))
    assert np.array_equal(M[sel], gate_all[sel])
    sel = kinds == "band_subnormal"
    with np.errstate(all="ignore"):                                  # (other kinds' f8 are not offsets; only `sel` is read)
        on_line = rec["t"][:, 0] == rec["q"][:, 0] + (-rec["f"][:, 8]).astype(np.float32)
    assert (w[sel] > 0).all() and (w[sel] < 1e-70).all() and np.array_equal(M[sel], (on_line & gate_all)[sel])
    # RECTIFIED STEREO REDUCES TO THE GATE: the mask is the gate's with dy in [-band, band]
    sel = kinds == "rectified"
    r = rec[sel]
    win = r["window"].copy()
    assert np.isinf(win[:, 2]).all() and np.isinf(win[:, 3]).all()
    win[:, 2], win[:, 3] = -r["band"], r["band"]
    want = gate_restated(gate_view(win, r["max_octave_diff"], r["q"], r["qo"], r["t"], r["to"]))
    assert np.array_equal(M[sel], want) and want.sum() > 50 and (~want).sum() > 50
    for s in (1.0, 0.5, -2.0):
        assert (r["f"][:, 7] == s).sum() > 100
    # ... and the fallback and the all-pass band give the gate's own answer wherever the keypoints are finite
    want = gate_restated(gate)
    for kind in ("gate_fallback", "gate_all_pass_band"):
        sel = kinds == kind
        fin = np.isfinite(rec["q"][sel]).all(axis=1) & np.isfinite(rec["t"][sel]).all(axis=1)
        assert fin.sum() > 1000 and np.array_equal(M[sel][fin], want[fin]), kind
    assert np.array_equal(M[kinds == "gate_fallback"], want)         # (the fallback: everywhere)
    # THE BAND LIES INSIDE THE SAMPSON TEST: whatever the band allows is an inlier of that F at max_error = band
    band_ok = has & restated_band(l0, l1, l2, w, rec["t"][:, 0], rec["t"][:, 1])
    fin = np.isfinite(rec["q"]).all(axis=1) & np.isfinite(rec["t"]).all(axis=1) & is_guided(rec["hypothesis"], rec["flags"])
    thr2 = rec["band"].astype(np.float64) * rec["band"].astype(np.float64)
    col = lambda v: v.astype(np.float64)[:, None]                    # noqa: E731 (one F per record: [n, 1] points)
    with np.errstate(all="ignore"):
        inl = restated_inliers8(rec["f"], thr2[:, None], col(rec["q"][:, 0]), col(rec["q"][:, 1]), col(rec["t"][:, 0]), col(rec["t"][:, 1]))[:, 0]
    assert (band_ok & fin).sum() > 1000 and not (band_ok & fin & ~inl).any()
    assert (fin & inl & ~band_ok).sum() > 20                         # (the band is the narrower test, not the same one)


def check(lines, rec):
    l0, l1, l2, w, has, M = restated(rec)
    got = parse(lines)
    assert len(got[0]) == len(rec)
    exp = [canonical(v.view(np.uint64), v) for v in (l0, l1, l2, w)] + [has, M]
    for name, g, e in zip(("l0", "l1", "l2", "w", "has", "M"), got, exp):
        bad = np.flatnonzero(g != e)
        assert len(bad) == 0, (name, len(bad), rec[bad[:3]], g[bad[:3]], e[bad[:3]])


def test_the_rule_agrees_with_its_restatement(tmp_path):
    rec, _, _ = epiline_records()
    check(run_program(build_program(), rec, tmp_path / "epiline.bin"), rec)


def test_the_rule_under_sanitizers(tmp_path):
    """the same program with the address and undefined-behaviour sanitizers, run stand-alone (nothing sanitized is loaded into
    Python)"""
    rec, _, _ = epiline_records()
    lines = run_program(build_program(sanitize=True), rec, tmp_path / "epiline_san.bin")
    check(lines, rec)

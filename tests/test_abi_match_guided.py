"""CPU checks of the guided pair matchers' boundary: both libraries export the two entry points the header declares, Python has the
structure and the calls, the eight guided kernels touch no scratch memory, and the rule - the very functions the kernels call
(csrc/brisk_match_guide.h), built here for the host - agrees with a NumPy restatement: the centres bit for bit, has-centre and the
mask M."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import ethzasl_brisk_amd as B
from test_abi_match_gated import gate_records, restated as gate_restated

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ethzasl_brisk_amd", "csrc")
NEW = ("brisk_hip_match_knn_pairs_guided_device", "brisk_hip_match_radius_pairs_guided_device")
PAIR_BAD, PAIR_NO_MODEL = 0x2, 0x8


def test_both_libraries_export_the_guided_matchers():
    from ethzasl_brisk_amd import build
    hdr = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    declared = set(re.findall(r"\b(brisk_hip_[a-z_0-9]+)\s*\(", hdr))
    for lib in (build.build(), build.build_release()):
        L = ctypes.CDLL(lib)
        for s in NEW:
            assert s in declared, s
            assert s in B.ABI_SYMBOLS, s
            assert hasattr(L, s), (lib, s)
    assert re.search(r"typedef struct brisk_hip_match_guide\b", hdr)
    assert set(re.findall(r"#define (BRISK_HIP_PAIR_BAD|BRISK_HIP_PAIR_NO_MODEL) (0x[0-9a-fA-F]+)", hdr)) == \
        {("BRISK_HIP_PAIR_BAD", "0x2"), ("BRISK_HIP_PAIR_NO_MODEL", "0x8")}


def test_python_has_the_guide():
    assert ctypes.sizeof(B.MatchGuide) == 24
    g = B.MatchGuide.around(6, max_octave_diff=1)
    w = g.window
    assert (w.dx_min, w.dx_max, w.dy_min, w.dy_max, w.max_octave_diff, g.fallback) == (-6.0, 6.0, -6.0, 6.0, 1, 0)
    g = B.MatchGuide.around(2.5, fallback=1)
    assert (g.window.dx_min, g.window.dy_max, g.window.max_octave_diff, g.fallback) == (-2.5, 2.5, -1, 1)
    for fn, lead in ((B.Context.match_knn_pairs_guided, ["self", "query", "train", "pairs", "k", "models", "guide"]),
                     (B.Context.match_radius_pairs_guided, ["self", "query", "train", "pairs", "max_distance", "cap_per_query", "models", "guide"])):
        par = inspect.signature(fn).parameters
        assert list(par)[:len(lead)] == lead
        for name in ("rows_cap", "query_kps", "train_kps", "stream"):
            assert name in par and par[name].default is None, (fn.__name__, name)
        assert "cross_check" not in par                              # the guided form has no cross check
    # the existing calls keep their signatures
    assert list(inspect.signature(B.Context.match_knn_pairs).parameters) == \
        ["self", "query", "train", "pairs", "k", "cross_check", "rows_cap", "stream", "dim_bytes", "out", "download", "gate", "query_kps",
         "train_kps"]


def test_guided_kernels_use_no_scratch():
    from ethzasl_brisk_amd import build
    build.build()
    res = build.kernel_resources()
    if not res:
        pytest.skip("the objects were not compiled here (no resource remarks beside them)")
    knn = {k: v for k, v in res.items() if "k_guided_knn_pairs" in k}
    radius = {k: v for k, v in res.items() if "k_guided_radius_pairs" in k}
    assert len(knn) == 4 and len(radius) == 4                       # four descriptor sizes each
    for k, v in {**knn, **radius}.items():
        assert v["scratch"] == 0, (k, v)
        for other in ("k_match_knn_pairs", "k_match_radius_pairs", "k_pair_select", "k_track_"):
            assert other not in k                                    # the sibling tests count kernels by these substrings


def test_the_rule_s_header_is_in_the_kernel_revision(tmp_path, monkeypatch):
    import shutil
    from ethzasl_brisk_amd import build
    rev = build.kernel_revision()
    copy = tmp_path / "csrc"
    shutil.copytree(CSRC, copy)
    with open(copy / "brisk_match_guide.h", "a") as f:
        f.write("// changed\n")
    monkeypatch.setattr(build, "CSRC", str(copy))
    assert build.kernel_revision() != rev


# ---- the rule -------------------------------------------------------------------------------------------------------------------

REC = np.dtype([("h", "<f8", (9,)), ("hypothesis", "<i4"), ("flags", "<i4"), ("window", "<f4", (4,)), ("max_octave_diff", "<i4"),
                ("fallback", "<i4"), ("q", "<f4", (2,)), ("qo", "<i4"), ("t", "<f4", (2,)), ("to", "<i4")])
assert REC.itemsize == 128


def build_program(sanitize=False):
    """tests/cpp/test_match_guide.cc: plain host C++ around csrc/brisk_match_guide.h (no HIP, no library)"""
    src = os.path.join(ROOT, "tests", "cpp", "test_match_guide.cc")
    hdrs = [os.path.join(CSRC, f) for f in ("brisk_match_guide.h", "brisk_match_gate.h", "brisk_pair_verify.h")]
    out = os.path.join(ROOT, "tests", "cpp", "test_match_guide" + ("_san" if sanitize else ""))
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in [src] + hdrs):
        extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off"] + extra + ["-I" + CSRC, "-o", out, src])
    return out


def run_program(prog, rec, path):
    rec.tofile(path)
    out = subprocess.run([prog, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    return out.stdout.split("\n")[:-1]


def restated_centres(h, hypothesis, flags, fallback, x, y):
    """the header's words in NumPy: float64 elementwise (a*b + c*d) + e, one `/` each, .astype(float32); an unguided pair's centre
    is the keypoint's own bits.  h [..., 9]; x, y float32.  Returns (cx, cy) float32 and has-centre."""
    h = np.asarray(h, np.float64)
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    guided = (np.asarray(hypothesis) >= 0) & ((np.asarray(flags) & (PAIR_BAD | PAIR_NO_MODEL)) == 0)
    xd, yd = x.astype(np.float64), y.astype(np.float64)
    with np.errstate(all="ignore"):
        z = (h[..., 6] * xd + h[..., 7] * yd) + h[..., 8]
        u = (h[..., 0] * xd + h[..., 1] * yd) + h[..., 2]
        v = (h[..., 3] * xd + h[..., 4] * yd) + h[..., 5]
        cx = np.where(guided, (u / z).astype(np.float32), x)
        cy = np.where(guided, (v / z).astype(np.float32), y)
    assert cx.dtype == np.float32 and cy.dtype == np.float32
    has = (guided | (np.asarray(fallback) != 0)) & np.isfinite(cx) & np.isfinite(cy)
    return cx, cy, has


def restated(rec):
    cx, cy, has = restated_centres(rec["h"], rec["hypothesis"], rec["flags"], rec["fallback"], rec["q"][:, 0], rec["q"][:, 1])
    w = rec["window"]
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = rec["t"][:, 0] - cx, rec["t"][:, 1] - cy
        assert dx.dtype == np.float32
        pos = (w[:, 0] <= dx) & (dx <= w[:, 1]) & (w[:, 2] <= dy) & (dy <= w[:, 3])
    m = rec["max_octave_diff"].astype(np.int64)
    octv = (m < 0) | (np.abs(rec["to"].astype(np.int64) - rec["qo"].astype(np.int64)) <= m)
    return cx, cy, has, has & pos & octv


IDENTITY = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
WINDOW = (-6.0, 6.0, -6.0, 6.0, 1)


def guide_records():
    """(records, kind of each).  Coordinates lie on a quarter-pixel grid; T is placed around the restated centre so that both answers of
    M occur."""
    rng = np.random.default_rng(2025)
    recs, kinds = [], []

    def add(kind, h, q, t, hypothesis=0, flags=0, window=WINDOW, fallback=0):
        r = np.zeros((), REC)
        r["h"], r["hypothesis"], r["flags"], r["window"], r["max_octave_diff"], r["fallback"] = h, hypothesis, flags, window[:4], window[4], fallback
        r["q"], r["qo"], r["t"], r["to"] = q[:2], q[2], t[:2], t[2]
        recs.append(r)
        kinds.append(kind)

    def grid_q():
        return (rng.integers(0, 400) / 4, rng.integers(0, 400) / 4, int(rng.integers(0, 4)))

    def near(h, q, spread=40, **kw):
        """a train keypoint up to spread / 4 pixels from the centre the model gives q, on the quarter-pixel grid"""
        cx, cy, has = restated_centres(h, kw.get("hypothesis", 0), kw.get("flags", 0), 1, np.float32(q[0]), np.float32(q[1]))
        cx, cy = (float(np.round(c * 4) / 4) if np.isfinite(c) and abs(c) < 1e6 else float(q[i]) for i, c in enumerate((cx, cy)))
        return (cx + rng.integers(-spread, spread + 1) / 4, cy + rng.integers(-spread, spread + 1) / 4, q[2] + int(rng.integers(-2, 3)))

    def projective():
        a = rng.uniform(-0.1, 0.1, 4)
        return (1 + a[0], a[1], rng.uniform(-20, 20), a[2], 1 + a[3], rng.uniform(-20, 20), rng.uniform(-1e-3, 1e-3), rng.uniform(-1e-3, 1e-3), 1.0)

    for _ in range(700):                                             # random projective models, z of either sign (the negated model)
        h, q = projective(), grid_q()
        add("projective", h, q, near(h, q))
        add("negated", tuple(-e for e in h), q, near(h, q))
    for _ in range(250):
        q = grid_q()
        add("identity", IDENTITY, q, near(IDENTITY, q), window=[WINDOW, (-40.0, 40.0, -40.0, 40.0, -1), (0.0, 0.0, 0.0, 0.0, 0)][rng.integers(0, 3)])
    for _ in range(300):                                             # pure translations: the centre lands exactly on a bound, or a quarter beyond
        q = grid_q()
        tx, ty = rng.integers(-200, 201) / 4, rng.integers(-200, 201) / 4
        h = (1.0, 0.0, tx, 0.0, 1.0, ty, 0.0, 0.0, 1.0)
        ex, ey = [(-6.0, 0.0), (6.0, 0.0), (0.0, -6.0), (0.0, 6.0), (6.0, 6.0), (-6.25, 0.0), (0.0, 6.25)][rng.integers(0, 7)]
        add("translation", h, q, (q[0] + tx + ex, q[1] + ty + ey, q[2] + int(rng.integers(-1, 2))))
    for i in range(300):                                             # z = x - c: zero exactly at x == c, of either sign around it
        q = grid_q()
        c = q[0] + [0.0, 0.0, 1.0, -1.0, 0.25, -17.5][i % 6]
        h = (2.0, 0.0, 0.0, 0.0, 3.0, 1.0, 1.0, 0.0, -c)
        add("z_zero" if c == q[0] else "z_sign", h, q, near(h, q))
    for i in range(200):                                             # NaN / infinite / all-zero models
        q = grid_q()
        h = list(projective())
        h[rng.integers(0, 9)] = np.nan
        add("nan_model", h, q, near(IDENTITY, q))
        h = list(projective())
        h[rng.integers(0, 9)] = [np.inf, -np.inf][i % 2]
        add("inf_model", h, q, near(h, q))
        if i % 4 == 0:
            add("zero_model", (0.0,) * 9, q, near(IDENTITY, q))
    for i in range(120):                                             # the conversion to fp32 overflows (not for a keypoint at the origin)
        q = grid_q() if i % 6 else (0.0, 0.0, 1)
        h = (1e300, 0.0, 0.0, 0.0, -1e300, 0.0, 0.0, 0.0, 1.0) if i % 2 else (3.5e38, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
        add("overflow", h, q, near(IDENTITY, q))
    for i in range(60):                                              # centres below the smallest normal fp32
        q = grid_q()
        h = (1e-40, 0.0, 0.0, 0.0, 1e-42, 0.0, 0.0, 0.0, 1.0)
        add("subnormal", h, q, (rng.integers(-30, 31) / 4, rng.integers(-30, 31) / 4, q[2]))
    for i in range(150):                                             # NaN keypoints under every kind of pair
        q = list(grid_q())
        q[i % 2] = np.nan
        h = [IDENTITY, projective()][i % 2]
        add("nan_keypoint", h, q, near(IDENTITY, grid_q()), hypothesis=[0, -1][i % 3 == 0], fallback=i % 2)
    garbage = (np.nan, 1e300, -np.inf, 0.0, 0.0, 5.0, 0.0, 0.0, 0.0)
    for i in range(480):                                             # pairs without a usable model, both fallbacks; the model is not read
        q = grid_q()
        hyp, fl = [(-1, 0), (3, PAIR_BAD), (0, PAIR_NO_MODEL), (-1, PAIR_BAD | PAIR_NO_MODEL), (5, PAIR_NO_MODEL | 0x100), (-(2 ** 31), 0)][i % 6]
        fb = [0, 1, -7][(i // 6) % 3]
        h = garbage if i % 2 else projective()
        add("unguided_fallback" if fb else "unguided", h, q, near(IDENTITY, q), hypothesis=hyp, flags=fl, fallback=fb)
    for i in range(120):                                             # flag bits that do NOT unguide a pair
        h, q = projective(), grid_q()
        add("other_flags", h, q, near(h, q), hypothesis=int(rng.integers(0, 4096)), flags=[0x1, 0x4, 0x100, 0x105][i % 4], fallback=i % 2)
    # the gate's own special records: under the identity model, and as the fallback of an unguided pair
    g = gate_records()
    gf, gi = g.view(np.float32), g.view(np.int32)
    for j in range(0, len(g), 2):
        win = (gf[j, 0], gf[j, 1], gf[j, 2], gf[j, 3], int(gi[j, 4]))
        q, t = (gf[j, 5], gf[j, 6], int(gi[j, 7])), (gf[j, 8], gf[j, 9], int(gi[j, 10]))
        add("gate_identity", IDENTITY, q, t, window=win)
        add("gate_fallback", garbage, q, t, hypothesis=-1, window=win, fallback=1)
    return np.array(recs, REC), np.array(kinds), g[::2]


def canonical(bits, values):
    """a NaN's payload is not the rule's business: every NaN compares as one pattern"""
    return np.where(np.isnan(values), np.uint32(0x7FC00000), bits)


def parse(lines):
    a = np.array([[int(x, 16), int(y, 16), int(h), int(m)] for x, y, h, m in (ln.split() for ln in lines)], np.int64)
    bx, by = a[:, 0].astype(np.uint32), a[:, 1].astype(np.uint32)
    return canonical(bx, bx.view(np.float32)), canonical(by, by.view(np.float32)), a[:, 2] == 1, a[:, 3] == 1


def test_the_restatement_is_not_vacuous():
    """what the comparison below rests on, shown on the restatement alone"""
    rec, kinds, gate = guide_records()
    assert len(rec) >= 3000
    cx, cy, has, M = restated(rec)
    both = ("projective", "negated", "identity", "translation", "z_sign", "unguided_fallback", "other_flags", "gate_identity", "gate_fallback")
    for kind in both:                                                # both answers of has-centre ... and of M, per model kind
        sel = kinds == kind
        assert M[sel].any() and (~M[sel]).any(), kind
        if kind in ("gate_identity", "gate_fallback"):               # (the others have finite keypoints and models: always a centre)
            assert has[sel].any() and (~has[sel]).any(), kind
        else:
            assert has[sel].all(), kind
    for kind in ("z_zero", "nan_model", "zero_model", "unguided", "nan_keypoint"):   # kinds that can have no centre
        sel = kinds == kind
        assert sel.sum() >= 40 and not has[sel].any() and not M[sel].any(), kind
    sel = kinds == "overflow"
    assert has[sel].any() and (~has[sel]).sum() > 80                 # only the keypoint at the origin keeps a centre
    assert (np.isinf(cx[sel]) | np.isinf(cy[sel])).sum() > 80
    sel = kinds == "inf_model"
    assert (~has[sel]).sum() > 100                                   # (an infinite h6 ... h8 can still give a finite quotient)
    sel = kinds == "subnormal"
    tiny = np.float32(2.0 ** -126)
    assert ((np.abs(cx[sel]) < tiny) & (cx[sel] != 0)).sum() > 40 and has[sel].all() and M[sel].any()
    # z of either sign, and the negated model has the same centre bit for bit
    with np.errstate(all="ignore"):
        zs = rec["h"][:, 6] * rec["q"][:, 0].astype(np.float64) + rec["h"][:, 7] * rec["q"][:, 1].astype(np.float64) + rec["h"][:, 8]
    sel = kinds == "z_sign"
    assert (zs[sel] > 0).sum() > 20 and (zs[sel] < 0).sum() > 20 and M[sel & (zs < 0)].any() and M[sel & (zs > 0)].any()
    assert (zs[kinds == "z_zero"] == 0).all()
    p, n = kinds == "projective", kinds == "negated"
    assert np.array_equal(cx[p].view(np.uint32), cx[n].view(np.uint32)) and np.array_equal(cy[p].view(np.uint32), cy[n].view(np.uint32))
    assert (zs[n] < 0).all() and (zs[p] > 0).all()
    # centres exactly on a bound pass (closed intervals), a quarter pixel beyond does not
    sel = kinds == "translation"
    with np.errstate(all="ignore"):
        dx, dy = rec["t"][:, 0] - cx, rec["t"][:, 1] - cy
    edge = sel & ((np.abs(dx) == 6) | (np.abs(dy) == 6)) & (np.abs(dx) <= 6) & (np.abs(dy) <= 6)
    assert edge.sum() > 100 and (M[edge] | (np.abs(rec["to"] - rec["qo"]) > 1)[edge]).all()
    assert not M[sel & ((np.abs(dx) == 6.25) | (np.abs(dy) == 6.25))].any()
    # the identity model and the fallback give the gate's own answer wherever the keypoint is finite
    want = gate_restated(gate)
    for kind in ("gate_identity", "gate_fallback"):
        sel = kinds == kind
        fin = np.isfinite(rec["q"][sel]).all(axis=1)
        assert fin.sum() > 1000 and np.array_equal(M[sel][fin], want[fin]), kind


def check(lines, rec):
    cx, cy, has, M = restated(rec)
    gx, gy, ghas, gM = parse(lines)
    assert len(gx) == len(rec)
    for name, got, exp in (("cx", gx, canonical(cx.view(np.uint32), cx)), ("cy", gy, canonical(cy.view(np.uint32), cy)), ("has", ghas, has),
                           ("M", gM, M)):
        bad = np.flatnonzero(got != exp)
        assert len(bad) == 0, (name, len(bad), rec[bad[:3]], got[bad[:3]], exp[bad[:3]])


def test_the_rule_agrees_with_its_restatement(tmp_path):
    rec, _, _ = guide_records()
    check(run_program(build_program(), rec, tmp_path / "guide.bin"), rec)


def test_the_rule_under_sanitizers(tmp_path):
    """the same program with the address and undefined-behaviour sanitizers, run stand-alone (nothing sanitized is loaded into
    Python)"""
    rec, _, _ = guide_records()
    lines = run_program(build_program(sanitize=True), rec, tmp_path / "guide_san.bin")
    check(lines, rec)

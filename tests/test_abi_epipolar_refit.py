"""CPU checks of the refit of epipolar pair models (brisk_hip_refit_pair_models_epipolar_device): both libraries export the entry
point the header declares, Python has the call, k_refit_epipolar touches no scratch memory, and the rule - the very functions the
kernel calls (csrc/brisk_pair_epipolar_refit.h), built here for the host - agrees BIT FOR BIT with a NumPy float64 restatement
written with the header's parenthesisation and its order of summation.  restated_epipolar_refit is the expectation of the GPU tests
(test_gpu_epipolar_refit.py) too.  The checks at the end do not involve the code under test at all: the restatement against
numpy.linalg.lstsq and numpy.linalg.svd, and two conditions on the inputs."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import ethzasl_brisk_amd as B
from test_abi_verify import PAIR_BAD, PAIR_NO_MODEL, ROWS_CUT, header_fields, hexes, records
from test_abi_refit import PAIR_REFIT, finite, lane_sums, restated_report
from test_abi_epipolar import SQ8, planted_depth, project, restated_inliers8, restated_pair8, rotation

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("brisk_hip_refit_pair_models_epipolar_device",)
SUMS = 44
SEAMS = (8, 9, 255, 256, 257, 1023, 1024, 1025, 2049)          # the seams of the sums (256 lanes) and of the staged chunk (1 024)


def test_both_libraries_export_the_epipolar_refit():
    from ethzasl_brisk_amd import build
    hdr = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    declared = set(re.findall(r"\b(brisk_hip_[a-z_0-9]+)\s*\(", hdr))
    for lib in (build.build(), build.build_release()):
        L = ctypes.CDLL(lib)
        for s in NEW:
            assert s in declared, s
            assert s in B.ABI_SYMBOLS, s
            assert hasattr(L, s), (lib, s)
    assert re.search(r"typedef struct brisk_hip_pair_epipolar_refit\b", hdr)
    assert len(re.findall(r"#define BRISK_HIP_PAIR_REFIT\b", hdr)) == 1 and B.PAIR_REFIT == PAIR_REFIT      # no new flag bit
    # the rule's header says what the flag tells a caller
    rule = " ".join(open(os.path.join(ROOT, "ethzasl_brisk_amd", "csrc", "brisk_pair_epipolar_refit.h")).read().replace("//", " ").split())
    assert "does not carry BRISK_HIP_PAIR_REFIT" in rule and "the flag is how a caller knows" in rule


def test_python_has_the_epipolar_refit():
    hdr = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    f = header_fields(hdr, "brisk_hip_pair_epipolar_refit")
    assert f == [("float", "max_error"), ("int", "rounds"), ("int", "min_inliers"), ("int", "keep_unverified"), ("int", "rank2")]
    assert [n for n, _ in B.PairEpipolarRefit._fields_] == [n for _, n in f]
    assert [t for _, t in B.PairEpipolarRefit._fields_] == [ctypes.c_float] + [ctypes.c_int] * 4
    assert ctypes.sizeof(B.PairEpipolarRefit) == 20
    par = inspect.signature(B.Context.refit_pair_models_epipolar).parameters
    assert list(par)[1:] == ["query", "train", "pairs", "rows_cap", "offsets", "matches", "models", "refit", "out_cap", "query_kps",
                             "train_kps", "stream"]
    assert list(par) == list(inspect.signature(B.Context.refit_pair_models).parameters)
    assert all(par[n].default is None for n in ("out_cap", "query_kps", "train_kps", "stream"))
    # the C arguments: the homography refit's, name for name and type for type, except the models' and the structure's types
    decl = re.search(r"int brisk_hip_refit_pair_models_epipolar_device\((.*?)\);", hdr, re.S).group(1)
    base = re.search(r"int brisk_hip_refit_pair_models_device\((.*?)\);", hdr, re.S).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args == [" ".join(a.split()).replace("brisk_hip_pair_model*", "brisk_hip_pair_epipolar_model*")
                    .replace("brisk_hip_pair_refit*", "brisk_hip_pair_epipolar_refit*") for a in base.split(",")]
    assert "const brisk_hip_pair_epipolar_model* d_models" in args and "brisk_hip_pair_epipolar_model* d_out_models" in args


def test_epipolar_refit_kernel_uses_no_scratch():
    from ethzasl_brisk_amd import build
    build.build()
    res = build.kernel_resources()
    if not res:
        pytest.skip("the objects were not compiled here (no resource remarks beside them)")
    new = {k: v for k, v in res.items() if "k_refit_epipolar" in k}
    assert len(new) == 1
    v = list(new.values())[0]
    assert v["scratch"] == 0, v
    assert v["lds"] >= 1024 * 16                                     # the staged chunk: 1 024 records of four floats
    for name in ("k_refit_models", "k_verify_ransac", "k_epipolar_ransac"):
        old = [v for k, v in res.items() if name in k]
        assert len(old) == 1 and old[0]["scratch"] == 0, (name, old)


# ---- the rule, restated ---------------------------------------------------------------------------------------------------------

def term_pairs():
    return [(i, j) for i in range(9) for j in range(i, 9)]          # term number 9 i - i (i - 1) / 2 + (j - i)


def restated_null(A):
    """the diagonally pivoted elimination of A [D, D] (destroyed) -> (ok, z [D] by position, perm [D])"""
    D = len(A)
    perm = list(range(D))
    for s in range(D - 1):
        best, at = np.float64(0.0), s
        for i in range(s, D):
            if A[i, i] > best:
                best, at = A[i, i], i
        if not (best > 0 and finite(best)):
            return False, np.zeros(D), perm
        A[[s, at], :] = A[[at, s], :]
        A[:, [s, at]] = A[:, [at, s]]
        perm[s], perm[at] = perm[at], perm[s]
        piv = A[s, s]
        for i in range(s + 1, D):
            f = A[i, s] / piv
            A[i, s + 1:] = A[i, s + 1:] - f * A[s, s + 1:]             # (element by element: j = s + 1 .. D - 1)
    z = np.zeros(D, np.float64)
    z[D - 1] = 1.0
    for i in range(D - 2, -1, -1):
        t = np.float64(0.0)
        for j in range(i + 1, D):
            t = t + A[i, j] * z[j]
        z[i] = (-t) / A[i, i]
    return True, z, perm


def restated_rank2(fn):
    """fn [9] -> (ok, fn' [9], e [3])"""
    N = np.zeros((3, 3), np.float64)
    for i in range(3):
        for j in range(3):
            N[i, j] = (fn[i] * fn[j] + fn[3 + i] * fn[3 + j]) + fn[6 + i] * fn[6 + j]
    ok, z, perm = restated_null(N)
    if not ok:
        return False, fn, np.zeros(3)
    e = np.zeros(3, np.float64)
    e[perm] = z
    q = (e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]
    if not (q > 0 and finite(q)):
        return False, fn, e
    out = fn.copy()
    for i in range(3):
        w = (fn[3 * i] * e[0] + fn[3 * i + 1] * e[1]) + fn[3 * i + 2] * e[2]
        for j in range(3):
            out[3 * i + j] = fn[3 * i + j] - (w * e[j]) / q
    return True, out, e


def restated_fit8(pts, inl, rank2, detail=None):
    """(3): the fit to the inlier set inl [m] bool of pts [m, 4] -> (ok, the fitted model [9], the free index or -1).  detail: a
    dict that receives the rows, the normal matrix, the linear and the final normalised solution"""
    idx = np.flatnonzero(inl)
    n = len(idx)
    p = pts[idx]
    fail = (False, np.zeros(9), -1)
    with np.errstate(all="ignore"):
        c = lane_sums(p, idx) / np.float64(n)                        # cx, cy, cu, cv
        d = p - c
        sp = lane_sums(np.where(d < 0, -d, d), idx)
        a, at = sp[0] + sp[1], sp[2] + sp[3]
        k, kt = np.float64(2 * n) / a, np.float64(2 * n) / at
        if not (a > 0 and at > 0):
            return fail
        X, Y, U, V = d[:, 0] * k, d[:, 1] * k, d[:, 2] * kt, d[:, 3] * kt
        rows = np.stack([U * X, U * Y, U, V * X, V * Y, V, X, Y, np.ones_like(X)], axis=1)
        t = np.stack([rows[:, i] * rows[:, j] for i, j in term_pairs()[:SUMS]], axis=1)
        s = lane_sums(t, idx)
        M = np.zeros((9, 9), np.float64)
        for kk, (i, j) in enumerate(term_pairs()):
            M[i, j] = M[j, i] = s[kk] if kk < SUMS else np.float64(n)
        ok, z, perm = restated_null(M.copy())
        if not ok:
            return fail
        fn = np.zeros(9, np.float64)
        fn[perm] = z
        free = perm[8]
        lin = fn.copy()
        if rank2:
            ok, fn, _ = restated_rank2(fn)
            if not ok:
                return fail
        if detail is not None:
            detail.update(rows=rows, M=M, linear=lin, fn=fn.copy(), free=free)
        g = np.zeros(9, np.float64)
        for i in range(3):
            g[3 * i] = fn[3 * i] * k
            g[3 * i + 1] = fn[3 * i + 1] * k
            g[3 * i + 2] = fn[3 * i + 2] - (g[3 * i] * c[0] + g[3 * i + 1] * c[1])
        o = np.zeros(9, np.float64)
        for j in range(3):
            o[j] = kt * g[j]
            o[3 + j] = kt * g[3 + j]
            o[6 + j] = g[6 + j] - (o[j] * c[2] + o[3 + j] * c[3])
        if not finite(o).all():
            return fail
        return True, restated_report(o), free


def restated_score8(F, thr2, pts, usable):
    """(2) -> (inlier [m] bool, count)"""
    S = np.zeros(len(pts), bool)
    u = np.flatnonzero(usable)
    S[u] = restated_inliers8(np.asarray(F, np.float64)[None, :], thr2, pts[u, 0], pts[u, 1], pts[u, 2], pts[u, 3])[0]
    return S, int(S.sum())


def restated_epipolar_refit_pair(rounds, min_inliers, keep_unverified, rank2, max_error, lim_a, lim_b, kq, kt, rec, f_in, hypothesis, flags):
    """one pair that is not BAD, as test_abi_refit.restated_refit_pair.  Returns a dict: has_model, n0, trace [(round, fit ok, n', free
    index, F')], count, replaced, accepted, usable [m], keep [m], inliers [m], model [9], flags, pts."""
    m = len(rec)
    q, t = rec["queryIdx"].astype(np.int64), rec["trainIdx"].astype(np.int64)
    usable = (q >= 0) & (q < lim_a) & (t >= 0) & (t < lim_b)
    pts = np.zeros((m, 4), np.float64)
    for j in np.flatnonzero(usable):
        c = np.array([kq[q[j], 0], kq[q[j], 1], kt[t[j], 0], kt[t[j], 1]], np.float32)
        usable[j] = np.isfinite(c).all()
        pts[j] = c.astype(np.float64)
    f_in = np.asarray(f_in, np.float64)
    max_error = np.float32(max_error)
    thr2 = np.float64(max_error) * np.float64(max_error)
    has_model = bool(hypothesis >= 0 and (flags & (PAIR_BAD | PAIR_NO_MODEL)) == 0 and finite(f_in).all() and max_error > 0)
    F, S, n, replaced, trace = f_in.copy(), np.zeros(m, bool), 0, 0, []
    with np.errstate(all="ignore"):
        if has_model:
            S, n = restated_score8(F, thr2, pts, usable)
        n0 = n
        if has_model:
            for r in range(1, int(rounds) + 1):
                if n < 8:
                    break
                ok, F1, free = restated_fit8(pts, S, rank2)
                S1, n1 = restated_score8(F1, thr2, pts, usable) if ok else (None, 0)
                trace.append((r, ok, n1, free if ok else -1, F1 if ok else np.zeros(9)))
                if not ok or n1 < n:
                    break
                F, S, n, replaced = F1, S1, n1, replaced + 1
    accepted = has_model and n >= min_inliers
    keep = S.copy() if accepted else (usable.copy() if keep_unverified else np.zeros(m, bool))
    model = (F if replaced else f_in.copy()) if has_model else np.zeros(9, np.float64)
    return {"has_model": has_model, "n0": n0, "trace": trace, "count": n, "replaced": replaced, "accepted": bool(accepted), "usable": usable,
            "keep": keep, "inliers": S, "model": model, "flags": (PAIR_REFIT if replaced else 0) | (0 if accepted else PAIR_NO_MODEL),
            "pts": pts}


def restated_epipolar_refit(frames, counts_q, counts_t, rows_cap, kq, kt, offsets, matches, in_models, refit, in_cap, out_cap, frames_q=None,
                            frames_t=None):
    """the whole call, as test_abi_refit.restated_refit.  in_models: PAIR_EPIPOLAR_MODEL [npairs]; refit: (max_error, rounds,
    min_inliers, keep_unverified, rank2).  Returns (models PAIR_EPIPOLAR_MODEL [npairs], counts, flags, offsets [npairs + 1], the
    stored records)."""
    max_error, rounds, min_inl, keep_unv, rank2 = refit
    n = len(frames)
    frames_q = len(counts_q) if frames_q is None else frames_q
    frames_t = len(counts_t) if frames_t is None else frames_t
    models = np.zeros(n, B.PAIR_EPIPOLAR_MODEL)
    kept = []
    for p, (a, b) in enumerate(frames):
        b0, b1 = int(offsets[p]), int(offsets[p + 1])
        range_ok = 0 <= b0 <= b1 <= in_cap and b1 - b0 <= 0x7FFFFFFF
        if not (range_ok and 0 <= a < frames_q and 0 <= b < frames_t):
            models[p] = (np.zeros(9), b1 - b0 if range_ok else 0, 0, 0, -1, 0, PAIR_BAD | PAIR_NO_MODEL)
            kept.append(matches[:0])
            continue
        lim_a, lim_b = min(max(int(counts_q[a]), 0), rows_cap), min(max(int(counts_t[b]), 0), rows_cap)
        rec = matches[b0:b1]
        M = in_models[p]
        r = restated_epipolar_refit_pair(rounds, min_inl, keep_unv, rank2, max_error, lim_a, lim_b, kq[a], kt[b], rec, M["f"],
                                         int(M["hypothesis"]), int(M["flags"]))
        models[p] = (r["model"], len(rec), int(r["usable"].sum()), r["count"], int(M["hypothesis"]) if r["has_model"] else -1,
                     r["replaced"], r["flags"])
        if r["has_model"] and not r["replaced"]:
            models["f"][p] = M["f"]                                    # (the input's bytes)
        kept.append(rec[r["keep"]])
    counts = np.array([len(k) for k in kept], np.int32)
    offs = np.zeros(n + 1, np.int64)
    cut = n
    for p in range(n):
        if counts[p] > 0 and offs[p] + counts[p] > out_cap:
            cut = p
            break
        offs[p + 1] = offs[p] + counts[p]
    offs[cut:] = offs[cut]
    models["flags"][cut:] |= ROWS_CUT
    stored = np.concatenate(kept[:cut]) if cut else matches[:0]
    return models, counts, models["flags"].astype(np.int32), offs, stored


# ---- scenes -------------------------------------------------------------------------------------------------------------------------

def winner_of(seed, p, hyps, max_error, kq, kt, rec, lim_a=None, lim_b=None, min_inl=8):
    """the input record of a pair: what the epipolar verifier (its restatement) reports -> (f [9], hypothesis, flags, its count)"""
    lim_a = len(kq) if lim_a is None else lim_a
    lim_b = len(kt) if lim_b is None else lim_b
    v = restated_pair8(seed, p, hyps, min_inl, 0, max_error, lim_a, lim_b, kq, kt, rec)
    return v["model"], v["winner"], 0 if v["accepted"] else PAIR_NO_MODEL, v["wcount"]


def case(kq, kt, rec, model, rounds=1, min_inl=8, keep_unv=0, rank2=1, max_error=1.0, lim_a=None, lim_b=None, f_in=None, hypothesis=None,
         flags=None):
    f, h, fl, _ = model
    lim_a = len(kq) if lim_a is None else lim_a
    lim_b = len(kt) if lim_b is None else lim_b
    return dict(rounds=rounds, min_inl=min_inl, keep_unv=keep_unv, rank2=rank2, max_error=np.float32(max_error),
                f_in=np.asarray(f if f_in is None else f_in, np.float64), hypothesis=h if hypothesis is None else hypothesis,
                flags=fl if flags is None else flags, lim_a=lim_a, lim_b=lim_b, kq=np.asarray(kq, np.float32).reshape(-1, 2)[:lim_a],
                kt=np.asarray(kt, np.float32).reshape(-1, 2)[:lim_b], rec=rec)


def hand_views():
    """test_abi_epipolar's twelve points of a volume seen by two cameras, and the rectified second view"""
    P = np.stack([(SQ8[:, 0] - 100) / 50.0, (SQ8[:, 1] - 100) / 60.0, 5.0 + (np.arange(12) * 7 % 5)], axis=1)
    sq = np.stack(project(P, np.eye(3), np.zeros(3)), axis=1).astype(np.float32)
    st = np.stack(project(P, rotation(0.03, -0.05, 0.02), np.array([0.4, 0.1, -0.2])), axis=1).astype(np.float32)
    stereo = np.stack(project(P, np.eye(3), np.array([-0.35, 0.0, 0.0])), axis=1).astype(np.float32)
    stereo[:, 1] = sq[:, 1]
    return sq, st, stereo


def onto_lines(F, q, near):
    """the points of `near` [n, 2] moved onto the epipolar lines F (q, 1) of q [n, 2], along the lines' normals"""
    F = np.asarray(F, np.float64).reshape(3, 3)
    l = np.concatenate([q.astype(np.float64), np.ones((len(q), 1))], axis=1) @ F.T
    r = (l[:, :2] * near).sum(axis=1) + l[:, 2]
    return (near - (r / (l[:, :2] ** 2).sum(axis=1))[:, None] * l[:, :2]).astype(np.float32)


def degenerate_scenes(F):
    """twelve inliers of the model F each: a side without extent, a side on an axis-parallel line, a side on a slanted line.
    -> [(name, kq, kt)]"""
    sq, st, _ = hand_views()
    Ft = np.asarray(F, np.float64).reshape(3, 3).T.reshape(9)
    one_q, one_t = np.tile(sq[:1], (12, 1)), np.tile(st[:1], (12, 1))
    flat_y = sq.copy()
    flat_y[:, 1] = 77.0
    slant = sq.copy()
    slant[:, 1] = slant[:, 0] * np.float32(0.5) + np.float32(7.0)
    # the train points on the vertical line x' = 31.5: where each query point's epipolar line crosses it
    l = np.concatenate([sq.astype(np.float64), np.ones((12, 1))], axis=1) @ np.asarray(F, np.float64).reshape(3, 3).T
    flat_x = np.stack([np.full(12, 31.5), -(l[:, 0] * 31.5 + l[:, 2]) / l[:, 1]], axis=1).astype(np.float32)
    return [("no extent", one_q, onto_lines(F, one_q, st.astype(np.float64))),
            ("no extent", onto_lines(Ft, one_t, sq.astype(np.float64)), one_t),
            ("axis", flat_y, onto_lines(F, flat_y, st.astype(np.float64))),
            ("axis", sq, flat_x),
            ("slant", slant, onto_lines(F, slant, st.astype(np.float64)))]


def seam_scene(m, noise=0.25):
    """m records of a noisy depth scene, three quarters of them true (all of them at m <= 9), and its input record"""
    true = m if m <= 9 else m - m // 4
    kq, kt, rec, _ = planted_depth(np.random.default_rng(900 + m), ("general", "stereo", "plane")[m % 3], true, m - true, noise=noise)
    return kq, kt, rec, winner_of(m, 0, 64, 1.5, kq, kt, rec)


def refit_cases():
    rng = np.random.default_rng(2468)
    cases, names = [], []

    def add(name, c):
        names.append(name)
        cases.append(c)

    sq, st, stereo = hand_views()
    ident = records([(j, j) for j in range(12)])
    # the twelve-point hand scene at every m from 0 to 12, both keep settings
    for m in range(0, 13):
        for keep_unv in (0, 1):
            add("hand", case(sq, st, ident[:m], winner_of(1, m, 16, 1.0, sq, st, ident[:m]), rounds=2, keep_unv=keep_unv, rank2=m & 1))
    hand = winner_of(7, 0, 64, 1.0, sq, st, ident)
    add("beyond", case(sq, st, ident, hand, rounds=2, min_inl=13, keep_unv=1))          # min_inliers beyond the records: not accepted
    # rectified stereo of the same points: the last element of F is 0
    for p in range(4):
        for rank2 in (0, 1):
            add("stereo", case(sq, stereo, ident, winner_of(9, p, 64, 1.0, sq, stereo, ident), rounds=2, rank2=rank2))
    # a side without extent, on an axis-parallel line, on a slanted line: twelve inliers of the hand scene's model
    for name, kq, kt in degenerate_scenes(hand[0]):
        for keep_unv in (0, 1):
            add(name, case(kq, kt, ident, hand, rounds=3, keep_unv=keep_unv, max_error=2.0))
    # duplicate points and duplicate records
    dup = records([(0, 0), (0, 0), (1, 1), (1, 1), (2, 2), (3, 3), (2, 2), (4, 4), (5, 5), (6, 6), (7, 7), (7, 7), (8, 8), (9, 9), (10, 10)])
    add("duplicates", case(sq, st, dup, winner_of(5, 0, 128, 1.0, sq, st, dup), rounds=2, keep_unv=1))
    # NaN / inf / -0.0 coordinates, on either side
    for side in (0, 1):
        for v in (np.nan, np.inf, -np.inf, -0.0):
            a, b = sq.copy(), st.copy()
            (a if side == 0 else b)[2, side] = v
            (a if side == 0 else b)[6, 1 - side] = v
            for keep_unv in (0, 1):
                add("coordinates", case(a, b, ident, hand, rounds=2, keep_unv=keep_unv))
    # indices at and beyond both limits, +-2^31 included; the keypoint arrays hold lim rows only
    lim = 10
    edge = [(q, t) for q in (-1, 0, lim - 1, lim, lim + 1, -2 ** 31, 2 ** 31 - 1) for t in (-1, 0, lim - 1, lim, -2 ** 31, 2 ** 31 - 1)]
    erec = records(edge + [(j, j) for j in range(lim)])
    for keep_unv in (0, 1):
        add("limits", case(sq, st, erec, hand, rounds=2, keep_unv=keep_unv, lim_a=lim, lim_b=lim))
        add("limits", case(sq, st, erec, hand, rounds=2, keep_unv=keep_unv, lim_a=lim, lim_b=5))
        add("limits", case(sq, st, ident, hand, rounds=2, keep_unv=keep_unv, lim_a=0, lim_b=lim))
    # max_error 0 / negative / NaN / inf
    for keep_unv in (0, 1):
        for e in (0.0, -1.0, np.nan, -np.inf):
            add("threshold off", case(sq, st, ident, hand, keep_unv=keep_unv, max_error=e))
        add("threshold inf", case(sq, st, ident, hand, keep_unv=keep_unv, max_error=np.inf))
    # input records that are no model: zeros, NaN / infinite elements, hypothesis -1, BAD / NO_MODEL flags
    kq, kt, rec, _ = planted_depth(rng, "general", 40, 12)
    planted = winner_of(3, 0, 64, 1.5, kq, kt, rec)
    for keep_unv in (0, 1):
        for i, v in ((0, np.nan), (8, np.inf), (4, -np.inf)):
            f = planted[0].copy()
            f[i] = v
            add("not finite", case(kq, kt, rec, planted, keep_unv=keep_unv, max_error=1.5, f_in=f))
        add("no hypothesis", case(kq, kt, rec, planted, keep_unv=keep_unv, max_error=1.5, hypothesis=-1))
        add("no hypothesis", case(kq, kt, rec, planted, keep_unv=keep_unv, max_error=1.5, hypothesis=-2 ** 31))
        for fl in (PAIR_BAD, PAIR_NO_MODEL, PAIR_BAD | PAIR_NO_MODEL):
            add("flagged", case(kq, kt, rec, planted, keep_unv=keep_unv, max_error=1.5, flags=fl))
        add("other flags", case(kq, kt, rec, planted, keep_unv=keep_unv, max_error=1.5, flags=ROWS_CUT | PAIR_REFIT | 1 | 4))     # these carry a model
        add("all zero", case(kq, kt, rec, planted, keep_unv=keep_unv, max_error=1.5, f_in=np.zeros(9)))
    # rounds 1, 2 and 8, rank2 0 and 1, both keep settings; a min_inliers the pair does not reach
    for rounds in (1, 2, 8):
        for rank2 in (0, 1):
            for keep_unv in (0, 1):
                add("planted", case(kq, kt, rec, planted, rounds=rounds, rank2=rank2, keep_unv=keep_unv, max_error=1.5))
    add("beyond", case(kq, kt, rec, planted, rounds=2, min_inl=50, max_error=1.5))
    # record counts at the seams of the sums and of the chunk
    for m in SEAMS:
        kq, kt, rec, model = seam_scene(m)
        add("seam", case(kq, kt, rec, model, rounds=2, rank2=m & 1, max_error=1.5))
    # no records at all
    add("empty", case(sq, st, ident[:0], hand, keep_unv=1))
    # two hundred random pairs: the three scenes with noise and random records, unusable records mixed in
    for n in range(200):
        m = int(rng.integers(8, 70))
        true = int(rng.integers(m // 2, m + 1))
        kq, kt, rec, _ = planted_depth(rng, ("general", "stereo", "plane")[n % 3], true, m - true, noise=float(rng.choice([0.0, 0.25, 1.0])))
        lim_a, lim_b = m, m
        if rng.integers(0, 4) == 0:
            lim_a, lim_b = int(rng.integers(m // 2, m + 1)), int(rng.integers(m // 2, m + 1))      # some rows do not exist
        if rng.integers(0, 3) == 0:
            bad = rng.integers(0, m, 3)
            rec["queryIdx"][bad[0]] = -1
            rec["trainIdx"][bad[1]] = m
            kq[bad[2], 0] = np.nan
        max_error = float(rng.choice([0.5, 1.5, 3.0]))
        model = winner_of(int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 3000)), int(rng.choice([7, 16, 64])), max_error, kq[:lim_a], kt[:lim_b],
                          rec, lim_a, lim_b)
        add("random", case(kq, kt, rec, model, rounds=int(rng.choice([1, 2, 8])), min_inl=int(rng.integers(8, 24)), keep_unv=int(rng.integers(0, 2)),
                           rank2=int(rng.integers(0, 2)), max_error=max_error, lim_a=lim_a, lim_b=lim_b))
    return names, cases


# ---- the rule's own code against the restatement -----------------------------------------------------------------------------------

def build_program(sanitize=False):
    """tests/cpp/test_pair_epipolar_refit.cc: plain host C++ around csrc/brisk_pair_epipolar_refit.h (no HIP, no library), without
    contraction; built the way test_abi_epipolar.build_program builds its own"""
    src = os.path.join(ROOT, "tests", "cpp", "test_pair_epipolar_refit.cc")
    inc = os.path.join(ROOT, "ethzasl_brisk_amd", "csrc")
    hdrs = [os.path.join(inc, h) for h in ("brisk_pair_epipolar_refit.h", "brisk_pair_epipolar.h", "brisk_pair_refit.h", "brisk_pair_verify.h",
                                           "brisk_match_guide.h", "brisk_match_gate.h")]
    out = os.path.join(ROOT, "tests", "cpp", "test_pair_epipolar_refit" + ("_san" if sanitize else ""))
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in [src] + hdrs):
        extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off"] + extra + ["-I" + inc, "-o", out, src])
    return out


def run_program(prog, cases, path):
    words = []
    for c in cases:
        words.append(np.array([c["max_error"]], np.float32).view(np.uint32))
        words.append(np.array([c["rounds"], c["min_inl"], c["keep_unv"], c["rank2"], c["hypothesis"], c["flags"]], np.int32).view(np.uint32))
        words.append(np.ascontiguousarray(c["f_in"], np.float64).view(np.uint32))
        words.append(np.array([c["lim_a"], c["lim_b"], len(c["rec"])], np.uint32))
        assert len(c["kq"]) == c["lim_a"] and len(c["kt"]) == c["lim_b"]
        words.append(np.ascontiguousarray(c["kq"]).view(np.uint32).reshape(-1))
        words.append(np.ascontiguousarray(c["kt"]).view(np.uint32).reshape(-1))
        words.append(np.ascontiguousarray(c["rec"]).view(np.uint32).reshape(-1))
    np.concatenate(words).astype("<u4").tofile(path)
    out = subprocess.run([prog, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    return out.stdout.split("\n")[:-1]


def restated_case(c):
    return restated_epipolar_refit_pair(c["rounds"], c["min_inl"], c["keep_unv"], c["rank2"], c["max_error"], c["lim_a"], c["lim_b"], c["kq"],
                                        c["kt"], c["rec"], c["f_in"], c["hypothesis"], c["flags"])


def expected_lines(r):
    out = ["s %d %d" % (int(r["has_model"]), r["n0"])]
    out += ["f %d %d %d %d %s" % (rnd, int(ok), n1, free, hexes(F1)) for rnd, ok, n1, free, F1 in r["trace"]]
    out.append("w %d %d %d %d %d" % (r["count"], r["replaced"], int(r["accepted"]), int(r["usable"].sum()), r["flags"]))
    out.append("k " + "".join("1" if k else "0" for k in r["keep"]))
    out.append("m " + hexes(r["model"]))
    return out


_RESTATED = {}


def restated_all():
    """(names, cases, the restatement's result per case), computed once"""
    if not _RESTATED:
        names, cases = refit_cases()
        _RESTATED["all"] = (names, cases, [restated_case(c) for c in cases])
    return _RESTATED["all"]


def test_the_rule_agrees_with_its_restatement(tmp_path):
    names, cases, results = restated_all()
    lines = run_program(build_program(), cases, tmp_path / "epipolar_refit_cases.bin")
    at = 0
    seen = {}
    for n, (name, c, r) in enumerate(zip(names, cases, results)):
        want = expected_lines(r)
        got = lines[at:at + len(want)]
        assert got == want, (n, name, [(g, w) for g, w in zip(got, want) if g != w][:2], len(got), len(want))
        at += len(want)
        seen.setdefault(name, []).append((r, c))
    assert at == len(lines)
    # NOT VACUOUS, with counts
    every = [r for r in results]
    replaced = sum(r["replaced"] > 0 for r in every)
    failed = sum(any(not t[1] for t in r["trace"]) for r in every)
    lost = sum(r["has_model"] and not r["accepted"] for r in every)
    grown = sum(r["count"] > r["n0"] for r in every)
    rejected = sum(bool(r["trace"]) and r["trace"][-1][1] and r["trace"][-1][2] < r["count"] for r in every)
    free = np.bincount([t[3] for r in every for t in r["trace"] if t[1]], minlength=9)
    print("models replaced in %d pairs, fits failed in %d, pairs that lost acceptance %d, kept lists grown %d, fitted models rejected %d"
          % (replaced, failed, lost, grown, rejected))
    print("the free index, over every fit:", free.tolist())
    assert replaced > 150 and failed >= 8 and lost >= 10 and grown >= 40
    assert (free > 0).sum() >= 3
    # the scenes are what their names say
    for r, c in seen["hand"]:
        m = len(c["rec"])
        assert r["has_model"] == (m >= 8) and (r["n0"] == m or m < 8)
        if m < 8:
            assert r["flags"] == PAIR_NO_MODEL and (r["model"] == 0).all() and r["keep"].sum() == (m if c["keep_unv"] else 0)
    assert sum(r["replaced"] > 0 for r, _ in seen["hand"]) >= 6
    stereo_free = [t[3] for r, _ in seen["stereo"] for t in r["trace"]]
    assert len(stereo_free) >= 8 and 8 not in stereo_free and -1 not in stereo_free        # rectified: the last element is never the free one
    for r, _ in seen["stereo"]:
        assert r["replaced"] > 0 and r["flags"] == PAIR_REFIT and abs(r["model"][8]) < 1e-9 and r["count"] == 12
    for name in ("no extent", "axis"):
        for r, c in seen[name]:
            assert r["has_model"] and r["n0"] == 12 and len(r["trace"]) == 1 and not r["trace"][0][1] and r["replaced"] == 0, name
            assert r["accepted"] and r["flags"] == 0 and r["model"].tobytes() == c["f_in"].tobytes() and r["keep"].all()
    assert all(r["has_model"] and r["n0"] == 12 and len(r["trace"]) >= 1 for r, _ in seen["slant"])
    for r, c in seen["beyond"]:
        assert r["has_model"] and not r["accepted"] and r["flags"] & PAIR_NO_MODEL and np.array_equal(r["keep"], r["usable"] & bool(c["keep_unv"]))
    for name in ("not finite", "no hypothesis", "flagged", "threshold off"):
        for r, c in seen[name]:
            assert not r["has_model"] and r["flags"] == PAIR_NO_MODEL and (r["model"] == 0).all() and r["count"] == 0
            assert np.array_equal(r["keep"], r["usable"] if c["keep_unv"] else np.zeros(len(r["keep"]), bool))
    assert all(r["has_model"] and r["replaced"] for r, _ in seen["other flags"] + seen["threshold inf"])
    assert all(r["has_model"] and r["count"] == 0 and not r["accepted"] for r, _ in seen["all zero"])
    assert all(0 < r["usable"].sum() < len(r["usable"]) for r, c in seen["limits"] if c["lim_a"] > 0)
    assert sum(r["usable"].sum() == 10 for r, _ in seen["coordinates"]) == 12 and sum(r["usable"].all() for r, _ in seen["coordinates"]) == 4
    assert all(r["replaced"] and r["count"] >= r["n0"] for r, _ in seen["planted"])
    assert sorted(len(c["rec"]) for _, c in seen["seam"]) == sorted(SEAMS)
    assert all(r["has_model"] and r["n0"] >= 8 and r["trace"] for r, _ in seen["seam"])
    assert sum(r["replaced"] > 0 for r, _ in seen["seam"]) >= 7 and any(r["count"] > r["n0"] for r, _ in seen["seam"])
    assert seen["empty"][0][0]["has_model"] and seen["empty"][0][0]["count"] == 0
    assert sum(0 < r["usable"].sum() < len(r["usable"]) for r, _ in seen["random"]) > 40


def test_the_rule_under_sanitizers(tmp_path):
    """the same program with the address and undefined-behaviour sanitizers, run stand-alone (nothing sanitized is loaded into Python)"""
    names, cases, _ = restated_all()
    plain = run_program(build_program(), cases, tmp_path / "a.bin")
    assert run_program(build_program(sanitize=True), cases, tmp_path / "b.bin") == plain


# ---- checks that do not involve the code under test -----------------------------------------------------------------------------------

KINDS = ("general", "stereo", "plane")
PLANTED_CLOSER = {k: (1, 2, 3, 4, 5, 6) for k in KINDS}        # the seeds the conditions below were met with
PLANTED_GROWS = {k: (1, 2, 3, 4) for k in KINDS}


def planted_pair(kind, seed, noise, max_error, hyps=256):
    """48 true + 12 random records of test_abi_epipolar.planted_depth with default_rng(700 + seed), verified with seed `seed`;
    and the same scene without noise (the generator draws the same numbers whatever the noise's scale)"""
    kq, kt, rec, is_true = planted_depth(np.random.default_rng(700 + seed), kind, 48, 12, noise=noise)
    kq0, kt0, rec0, _ = planted_depth(np.random.default_rng(700 + seed), kind, 48, 12, noise=0.0)
    assert np.array_equal(kq, kq0) and np.array_equal(rec, rec0)
    return dict(kq=kq, kt=kt, rec=rec, is_true=is_true, kt0=kt0, model=winner_of(seed, 0, hyps, max_error, kq, kt, rec), max_error=max_error)


_PLANTED = {}


def planted_refit(kind, seed, noise, max_error, rank2, rounds=4):
    key = (kind, seed, noise, max_error, rank2, rounds)
    if key not in _PLANTED:
        sc = planted_pair(kind, seed, noise, max_error)
        f, h, fl, wcount = sc["model"]
        r = restated_epipolar_refit_pair(rounds, 8, 0, rank2, max_error, 60, 60, sc["kq"], sc["kt"], sc["rec"], f, h, fl)
        _PLANTED[key] = (sc, r, wcount)
    return _PLANTED[key]


def line_distance(F, q, t):
    """the mean distance of the points t [n, 2] from the epipolar lines F (q, 1)"""
    F = np.asarray(F, np.float64).reshape(3, 3)
    l = np.concatenate([q.astype(np.float64), np.ones((len(q), 1))], axis=1) @ F.T
    return float(np.mean(np.abs((l[:, :2] * t.astype(np.float64)).sum(axis=1) + l[:, 2]) / np.hypot(l[:, 0], l[:, 1])))


def test_a_refit_lies_closer_to_the_true_geometry():
    """A CONDITION ON THE INPUTS, met by the restatement alone: 48 true + 12 random records, noise 0.25 px, max_error 1.5, 256
    hypotheses, 4 rounds, rank 2 - the noise-free true train points lie closer (mean distance) to the epipolar lines of their
    noise-free query points under the refitted model than under the eight-point winner, in every case"""
    for kind in KINDS:
        for seed in PLANTED_CLOSER[kind]:
            sc, r, _ = planted_refit(kind, seed, 0.25, 1.5, 1)
            true = sc["rec"][sc["is_true"]]
            q, t = sc["kq"][true["queryIdx"]], sc["kt0"][true["trainIdx"]]
            before, after = line_distance(sc["model"][0], q, t), line_distance(r["model"], q, t)
            print("%s %d: %.3f px -> %.3f px, inliers %d -> %d" % (kind, seed, before, after, r["n0"], r["count"]))
            assert r["replaced"] >= 1 and r["flags"] == PAIR_REFIT and after < before, (kind, seed, before, after)


def test_a_refit_finds_more_inliers():
    """A CONDITION ON THE INPUTS: noise 0.5 px, max_error 0.75 - the final inlier count exceeds the winner's, in every case"""
    for kind in KINDS:
        for seed in PLANTED_GROWS[kind]:
            _, r, wcount = planted_refit(kind, seed, 0.5, 0.75, 1)
            print("%s %d: inliers %d -> %d" % (kind, seed, wcount, r["count"]))
            assert r["n0"] == wcount and r["count"] > wcount, (kind, seed, wcount, r["count"])


def first_fit(kind, seed, noise, max_error, rank2):
    sc, r, _ = planted_refit(kind, seed, noise, max_error, rank2)
    thr2 = np.float64(np.float32(max_error)) ** 2
    S, n = restated_score8(sc["model"][0], thr2, r["pts"], r["usable"])
    d = {}
    ok, _, free = restated_fit8(r["pts"], S, rank2, detail=d)
    assert ok and n >= 8 and free == d["free"]
    return d


def planted_grid():
    return [(k, s, 0.25, 1.5) for k in KINDS for s in PLANTED_CLOSER[k]] + [(k, s, 0.5, 0.75) for k in KINDS for s in PLANTED_GROWS[k]]


def test_the_normalised_solution_agrees_with_lstsq():
    """INDEPENDENT OF THE CODE UNDER TEST: the normal matrix eliminated with diagonal pivoting against numpy.linalg.lstsq (an SVD) on
    the same rows with the same free element held at 1.  Tolerance, per case: 100 x cond(M) x 2^-52 on the largest element
    difference, relative to the solution's largest element"""
    for kind, seed, noise, max_error in planted_grid():
        d = first_fit(kind, seed, noise, max_error, 0)
        A, free = d["rows"], d["free"]
        rest = [j for j in range(9) if j != free]
        ref = np.zeros(9)
        ref[free] = 1.0
        ref[rest] = np.linalg.lstsq(A[:, rest], -A[:, free], rcond=None)[0]
        cond = float(np.linalg.cond(d["M"]))
        tol = 100 * cond * 2.0 ** -52
        diff = float(np.abs(d["linear"] - ref).max() / np.abs(ref).max())
        print("%s %d noise %.2f: free %d, cond(M) %.3g, difference %.3g, tolerance %.3g" % (kind, seed, noise, free, cond, diff, tol))
        assert diff <= tol, (kind, seed, diff, tol)


def test_the_rank2_step_against_the_svd():
    """INDEPENDENT OF THE CODE UNDER TEST: numpy.linalg.svd of the normalised result - with rank2 sigma3 / sigma2 <= 1e-12 and the
    Frobenius distance from the SVD truncation of the linear fit is at most 1e-2 of the distance the linear fit had (sigma3); without
    rank2 sigma3 / sigma2 is above 1e-6 on the general scenes, so the step does something"""
    for kind, seed, noise, max_error in planted_grid():
        d = first_fit(kind, seed, noise, max_error, 1)
        lin, fn = d["linear"].reshape(3, 3), d["fn"].reshape(3, 3)
        u, s, vt = np.linalg.svd(lin)
        trunc = (u[:, :2] * s[:2]) @ vt[:2]
        s2 = np.linalg.svd(fn, compute_uv=False)
        had, has = float(np.linalg.norm(lin - trunc)), float(np.linalg.norm(fn - trunc))
        print("%s %d noise %.2f: sigma3/sigma2 %.3g -> %.3g, distance from the truncation %.3g -> %.3g (ratio %.3g)"
              % (kind, seed, noise, s[2] / s[1], s2[2] / s2[1], had, has, has / had))
        assert s2[2] / s2[1] <= 1e-12, (kind, seed, s2)
        assert has <= 1e-2 * had, (kind, seed, has, had)
        if kind == "general":
            assert s[2] / s[1] > 1e-6, (kind, seed, s)

"""CPU checks of the epipolar verification of pair matches (brisk_hip_verify_pair_matches_epipolar_device): both libraries export
the entry point the header declares, Python has the call, k_epipolar_ransac touches no scratch memory, and the rule - the very
functions the kernel calls (csrc/brisk_pair_epipolar.h), built here for the host - agrees BIT FOR BIT with a NumPy float64
restatement written with the header's parenthesisation.  restated_epipolar is the expectation of the GPU tests
(test_gpu_epipolar.py) too."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import ethzasl_brisk_amd as B
from test_abi_verify import M32, PAIR_BAD, PAIR_NO_MODEL, ROWS_CUT, case, header_fields, hexes, mix, records, run_program

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("brisk_hip_verify_pair_matches_epipolar_device",)


def test_both_libraries_export_the_epipolar_verifier():
    from ethzasl_brisk_amd import build
    hdr = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    declared = set(re.findall(r"\b(brisk_hip_[a-z_0-9]+)\s*\(", hdr))
    for lib in (build.build(), build.build_release()):
        L = ctypes.CDLL(lib)
        for s in NEW:
            assert s in declared, s
            assert s in B.ABI_SYMBOLS, s
            assert hasattr(L, s), (lib, s)
    assert re.search(r"typedef struct brisk_hip_pair_epipolar_model\b", hdr)
    # the header says what the model is and is not
    text = " ".join(hdr.split())
    for phrase in ("RANK 2 IS NOT ENFORCED", "coplanar", "essential matrices", "the refit of F", "guided matching along epipolar lines"):
        assert phrase in text, phrase
    not_done = re.search(r"\* Not done here: ([^*]*?)adaptive stopping", hdr).group(1)      # the homography verifier's list
    assert "fundamental" not in not_done


def test_python_has_the_epipolar_verifier():
    hdr = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    f = header_fields(hdr, "brisk_hip_pair_verify")                  # the parameter structure is the verifier's, unchanged
    assert f == [("float", "max_error"), ("int", "hypotheses"), ("int", "min_inliers"), ("int", "keep_unverified"), ("unsigned", "seed")]
    f = header_fields(hdr, "brisk_hip_pair_epipolar_model")
    assert f == [("double", "f[9]")] + [("int", n) for n in ("records", "usable", "inliers", "hypothesis", "valid", "flags")]
    D = B.PAIR_EPIPOLAR_MODEL
    assert D.names == ("f", "records", "usable", "inliers", "hypothesis", "valid", "flags")
    assert D.itemsize == 96 and D["f"].shape == (9,) and D["f"].base == np.dtype("<f8")
    assert all(D[n] == np.dtype("<i4") for n in D.names[1:])
    assert [D.fields[n][1] for n in D.names] == [B.PAIR_MODEL.fields[n][1] for n in B.PAIR_MODEL.names]    # the same layout
    par = inspect.signature(B.Context.verify_pair_matches_epipolar).parameters
    assert list(par) == list(inspect.signature(B.Context.verify_pair_matches).parameters)
    assert all(par[n].default is None for n in ("out_cap", "query_kps", "train_kps", "stream"))
    # the C arguments: the verifier's, name for name and type for type, except the model's type
    decl = re.search(r"int brisk_hip_verify_pair_matches_epipolar_device\((.*?)\);", hdr, re.S).group(1)
    base = re.search(r"int brisk_hip_verify_pair_matches_device\((.*?)\);", hdr, re.S).group(1)
    args = [" ".join(a.split()) for a in decl.split(",")]
    assert args == [" ".join(a.split()).replace("brisk_hip_pair_model*", "brisk_hip_pair_epipolar_model*") for a in base.split(",")]
    assert "brisk_hip_pair_epipolar_model* d_models" in args


def test_epipolar_kernel_uses_no_scratch():
    from ethzasl_brisk_amd import build
    build.build()
    res = build.kernel_resources()
    if not res:
        pytest.skip("the objects were not compiled here (no resource remarks beside them)")
    new = {k: v for k, v in res.items() if "k_epipolar_" in k}
    assert sorted(re.search(r"k_epipolar_[a-z]+", k).group(0) for k in new) == ["k_epipolar_ransac"]
    for k, v in new.items():
        assert v["scratch"] == 0, (k, v)
        assert v["lds"] >= 1024 * 16                                  # the staged chunk: 1 024 records of four floats
        assert v["occupancy"] >= 1                                    # waves per SIMD: the solve has one wave's registers, no fewer
    # the packing kernels are the verifier's: no kernel of this call carries its prefix
    assert sorted(re.search(r"k_verify_[a-z]+", k).group(0) for k in res if "k_verify_" in k) == ["k_verify_offsets", "k_verify_ransac",
                                                                                                "k_verify_scatter"]


# ---- the rule, restated ---------------------------------------------------------------------------------------------------------

def absv(v):
    return np.where(v < 0, -v, v)


def finite(v):
    return (v - v) == 0


def restated_sample8(seed, p, h, m):
    """(b): [len(h), 8] record indices, in draw order; m >= 8"""
    h = np.asarray(h, np.uint64)
    pair_seed = mix((mix(np.uint64(seed) ^ np.uint64(0x9E3779B9)) + np.uint64(p & 0xFFFFFFFF)) & M32)
    out = np.zeros((len(h), 8), np.int64)
    for k in range(8):
        r = (mix((pair_seed + np.uint64(8) * h + np.uint64(k)) & M32) * np.uint64(m - k)) >> np.uint64(32)
        r = r.astype(np.int64)
        chosen = np.sort(out[:, :k], axis=1)
        for c in range(k):                                              # the indices chosen before, in ascending order
            r = r + (chosen[:, c] <= r)
        out[:, k] = r
    return out


def scalar_sample8(seed, p, h, m):
    """(b) once more with Python integers, one hypothesis: what the pinned samples were worked out with"""
    def mix1(x):
        x &= 0xFFFFFFFF
        x ^= x >> 16
        x = (x * 0x7feb352d) & 0xFFFFFFFF
        x ^= x >> 15
        x = (x * 0x846ca68b) & 0xFFFFFFFF
        return x ^ (x >> 16)
    pair_seed = mix1(mix1(seed ^ 0x9E3779B9) + (p & 0xFFFFFFFF))
    out = []
    for k in range(8):
        r = (mix1(pair_seed + 8 * h + k) * (m - k)) >> 32
        for c in sorted(out):
            if c <= r:
                r += 1
        out.append(r)
    return out


def side_norm(x, y):
    """x, y [n, 8] -> (ok [n], cx, cy, k)"""
    cx, cy = x[:, 0], y[:, 0]
    for i in range(1, 8):
        cx = cx + x[:, i]
        cy = cy + y[:, i]
    cx, cy = cx / 8.0, cy / 8.0
    ax, ay = absv(x[:, 0] - cx), absv(y[:, 0] - cy)
    for i in range(1, 8):
        ax = ax + absv(x[:, i] - cx)
        ay = ay + absv(y[:, i] - cy)
    a = ax + ay
    return a > 0, cx, cy, 16.0 / a


def first_largest(a):
    """a [n, k] magnitudes -> (index of the first largest, that magnitude): the scan from 0.0 that only a strictly larger value
    replaces (a NaN never replaces; nothing > 0: the magnitude returned is not > 0)"""
    key = np.where(np.isnan(a), -1.0, a)
    arg = key.argmax(axis=1)
    return arg, key[np.arange(len(a)), arg]


def null_vector(A):
    """A [n, 8, 9] (destroyed) -> (ok [n], fn [n, 9], free column [n]); rows that failed hold garbage"""
    n = len(A)
    rows = np.arange(n)
    ok = np.ones(n, bool)
    perm = np.tile(np.arange(9), (n, 1))
    for s in range(8):
        arg, best = first_largest(absv(A[:, s:, s:]).reshape(n, -1))
        ok &= (best > 0) & finite(best)
        pr, pc = s + arg // (9 - s), s + arg % (9 - s)
        t = A[rows, s, :].copy()
        A[rows, s, :] = A[rows, pr, :]
        A[rows, pr, :] = t
        t = A[rows, :, s].copy()
        A[rows, :, s] = A[rows, :, pc]
        A[rows, :, pc] = t
        t = perm[rows, s].copy()
        perm[rows, s] = perm[rows, pc]
        perm[rows, pc] = t
        for i in range(s + 1, 8):
            f = A[:, i, s] / A[:, s, s]
            A[:, i, s + 1:] = A[:, i, s + 1:] - f[:, None] * A[:, s, s + 1:]                   # (element by element: j = s + 1..8)
    z = np.zeros((n, 9), np.float64)
    z[:, 8] = 1.0
    for i in range(7, -1, -1):
        t = np.zeros(n, np.float64)
        for j in range(i + 1, 9):
            t = t + A[:, i, j] * z[:, j]
        z[:, i] = (-t) / A[:, i, i]
    fn = np.zeros((n, 9), np.float64)
    fn[rows[:, None], perm] = z
    return ok, fn, perm[:, 8]


def report_rows(F):
    """brisk_verify_report, row by row of F [n, 9]"""
    arg, best = first_largest(absv(F))
    scale = F[np.arange(len(F)), arg]
    return np.where((best > 0)[:, None], F / scale[:, None], F)


def restated_model8(x, y, u, v):
    """(c): the eight point pairs of n samples [n, 8] -> (ok [n], F [n, 9], free column [n])"""
    ok_q, cx, cy, k = side_norm(x, y)
    ok_t, cu, cv, kt = side_norm(u, v)
    X, Y = (x - cx[:, None]) * k[:, None], (y - cy[:, None]) * k[:, None]
    U, V = (u - cu[:, None]) * kt[:, None], (v - cv[:, None]) * kt[:, None]
    A = np.stack([U * X, U * Y, U, V * X, V * Y, V, X, Y, np.ones_like(X)], axis=2)
    ok, fn, free = null_vector(A)
    g = np.zeros_like(fn)
    for i in range(3):
        g[:, 3 * i] = fn[:, 3 * i] * k
        g[:, 3 * i + 1] = fn[:, 3 * i + 1] * k
        g[:, 3 * i + 2] = fn[:, 3 * i + 2] - (g[:, 3 * i] * cx + g[:, 3 * i + 1] * cy)
    d = np.zeros_like(fn)
    for j in range(3):
        d[:, j] = kt * g[:, j]
        d[:, 3 + j] = kt * g[:, 3 + j]
        d[:, 6 + j] = g[:, 6 + j] - (d[:, j] * cu + d[:, 3 + j] * cv)
    ok = ok_q & ok_t & ok & finite(d).all(axis=1)
    return ok, report_rows(d), free


def restated_inliers8(F, thr2, x, y, xt, yt):
    """(d): F [n, 9], the points [m] -> [n, m] bool (for usable records, with the threshold on)"""
    f = [F[:, i][:, None] for i in range(9)]
    l0 = (f[0] * x + f[1] * y) + f[2]
    l1 = (f[3] * x + f[4] * y) + f[5]
    l2 = (f[6] * x + f[7] * y) + f[8]
    r = (xt * l0 + yt * l1) + l2
    m0 = (f[0] * xt + f[3] * yt) + f[6]
    m1 = (f[1] * xt + f[4] * yt) + f[7]
    g = ((l0 * l0 + l1 * l1) + m0 * m0) + m1 * m1
    return (g > 0) & (r * r <= thr2 * g)


def restated_pair8(seed, p, hypotheses, min_inliers, keep_unverified, max_error, lim_a, lim_b, kq, kt, rec):
    """one pair, as test_abi_verify.restated_pair.  Returns a dict: per hypothesis valid / idx / free / count / F (zeros unless
    valid), and the pair's winner, count, accepted, nvalid, usable [m], keep [m], model [9]."""
    m = len(rec)
    q, t = rec["queryIdx"].astype(np.int64), rec["trainIdx"].astype(np.int64)
    usable = (q >= 0) & (q < lim_a) & (t >= 0) & (t < lim_b)
    pts = np.zeros((m, 4), np.float64)
    for j in np.flatnonzero(usable):
        c = np.array([kq[q[j], 0], kq[q[j], 1], kt[t[j], 0], kt[t[j], 1]], np.float32)
        usable[j] = np.isfinite(c).all()
        pts[j] = c.astype(np.float64)
    nh = int(hypotheses)
    valid, idx, count = np.zeros(nh, bool), np.full((nh, 8), -1, np.int64), np.zeros(nh, np.int64)
    F, free = np.zeros((nh, 9), np.float64), np.full(nh, -1, np.int64)
    max_error = np.float32(max_error)
    thr_on = bool(max_error > 0)
    thr2 = np.float64(max_error) * np.float64(max_error)
    u = np.flatnonzero(usable)
    with np.errstate(all="ignore"):
        if m >= 8:
            idx = restated_sample8(seed, p, np.arange(nh), m)
            assert (idx >= 0).all() and (idx < m).all() and all(len(set(r)) == 8 for r in idx[:64].tolist())
            full = usable[idx].all(axis=1)
            s = pts[idx]                                                # [nh, 8 points, 4 coordinates]
            ok, Fs, fr = restated_model8(s[:, :, 0], s[:, :, 1], s[:, :, 2], s[:, :, 3])
            valid = full & ok
            F[valid], free[valid] = Fs[valid], fr[valid]
            if thr_on:
                for a in range(0, nh, 256):
                    sl = slice(a, a + 256)
                    count[sl] = restated_inliers8(F[sl], thr2, pts[u, 0], pts[u, 1], pts[u, 2], pts[u, 3]).sum(axis=1)
                count[~valid] = 0
        winner, wcount = -1, 0
        for h in np.flatnonzero(valid):                                # the most inliers, the smallest h
            if winner < 0 or count[h] > wcount:
                winner, wcount = int(h), int(count[h])
        accepted = winner >= 0 and wcount >= min_inliers
        keep = np.zeros(m, bool)
        if accepted:
            keep[u] = restated_inliers8(F[winner:winner + 1], thr2, pts[u, 0], pts[u, 1], pts[u, 2], pts[u, 3])[0]
            assert int(keep.sum()) == wcount
        elif keep_unverified:
            keep = usable.copy()
        model = F[winner].copy() if winner >= 0 else np.zeros(9, np.float64)
    return {"valid": valid, "idx": idx, "free": free, "count": count, "F": F, "winner": winner, "wcount": wcount, "accepted": bool(accepted),
            "nvalid": int(valid.sum()), "usable": usable, "keep": keep, "model": model}


def restated_epipolar(frames, counts_q, counts_t, rows_cap, kq, kt, offsets, matches, verify, in_cap, out_cap, frames_q=None, frames_t=None):
    """the whole call, as test_abi_verify.restated_verify.  Returns (models PAIR_EPIPOLAR_MODEL [npairs], counts, flags, offsets
    [npairs + 1], the stored records)."""
    max_error, hyps, min_inl, keep_unv, seed = verify
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
        r = restated_pair8(seed, p, hyps, min_inl, keep_unv, max_error, lim_a, lim_b, kq[a], kt[b], rec)
        models[p] = (r["model"], len(rec), int(r["usable"].sum()), r["wcount"], r["winner"], r["nvalid"], 0 if r["accepted"] else PAIR_NO_MODEL)
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


# ---- scenes with depth ----------------------------------------------------------------------------------------------------------

K_CAM = np.array([[500.0, 0, 320], [0, 500.0, 240], [0, 0, 1]])


def rotation(rx, ry, rz):
    cx, sx, cy, sy, cz, sz = np.cos(rx), np.sin(rx), np.cos(ry), np.sin(ry), np.cos(rz), np.sin(rz)
    return (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
            @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))


def scene_points(rng, kind, n):
    """n points in front of the first camera: a volume, or (kind "plane") a tilted plane"""
    x, y = rng.uniform(-2.2, 2.2, n), rng.uniform(-1.6, 1.6, n)
    z = 6.0 + 0.5 * x + 0.3 * y if kind == "plane" else rng.uniform(4.0, 9.0, n)
    return np.stack([x, y, z], axis=1)


def scene_motion(rng, kind):
    """(R, t) of the second camera: "stereo" is rectified (no rotation, a baseline along x), the others a general motion"""
    if kind == "stereo":
        return np.eye(3), np.array([-0.35, 0.0, 0.0])
    return rotation(*rng.uniform(-0.08, 0.08, 3)), np.array([rng.uniform(0.3, 0.6), rng.uniform(-0.2, 0.2), rng.uniform(-0.3, 0.3)])


def project(P, R, t):
    c = (P @ R.T + t) @ K_CAM.T
    return c[:, 0] / c[:, 2], c[:, 1] / c[:, 2]


def planted_depth(rng, kind, true, random, noise=0.25, shuffle=True):
    """true + random records of one pair of views of a scene with depth (kind: "general", "stereo", "plane"): the first `true`
    (before shuffling) are projections of one 3-D point into both views, with Gaussian noise of `noise` px on the train side; the
    others name a train point drawn anywhere in the frame.  Everything rounded to float as keypoints are.
    Returns (kq, kt, rec, is_true [n])."""
    n = true + random
    P = scene_points(rng, kind, n)
    R, t = scene_motion(rng, kind)
    x, y = project(P, np.eye(3), np.zeros(3))
    xt, yt = project(P, R, t)
    xt, yt = xt + rng.normal(0, noise, n), yt + rng.normal(0, noise, n)
    xt[true:], yt[true:] = rng.uniform(0, 640, random), rng.uniform(0, 480, random)
    order = rng.permutation(n) if shuffle else np.arange(n)
    tperm = rng.permutation(n)                                         # train rows in another order than query rows
    kq = np.stack([x, y], axis=1).astype(np.float32)
    kt = np.zeros((n, 2), np.float32)
    kt[tperm] = np.stack([xt, yt], axis=1).astype(np.float32)
    rec = records([(int(j), int(tperm[j])) for j in order])
    return kq, kt, rec, order < true


# ---- the rule's own code against the restatement -----------------------------------------------------------------------------------

def build_program(sanitize=False):
    """tests/cpp/test_pair_epipolar.cc: plain host C++ around csrc/brisk_pair_epipolar.h (no HIP, no library)"""
    src = os.path.join(ROOT, "tests", "cpp", "test_pair_epipolar.cc")
    inc = os.path.join(ROOT, "ethzasl_brisk_amd", "csrc")
    hdrs = [os.path.join(inc, h) for h in ("brisk_pair_epipolar.h", "brisk_pair_verify.h")]
    out = os.path.join(ROOT, "tests", "cpp", "test_pair_epipolar" + ("_san" if sanitize else ""))
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in [src] + hdrs):
        extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off"] + extra + ["-I" + inc, "-o", out, src])
    return out


SQ8 = np.array([[10, 10], [200, 15], [210, 180], [5, 190], [100, 100], [50, 150], [150, 60], [120, 170], [33, 77], [180, 120],
                [90, 20], [60, 60]], np.float32)


def epipolar_cases():
    rng = np.random.default_rng(8642)
    cases = []
    # hand cases: twelve points of a volume seen by two cameras; every m from 0 to 12; both keep settings
    P = np.stack([(SQ8[:, 0] - 100) / 50.0, (SQ8[:, 1] - 100) / 60.0, 5.0 + (np.arange(12) * 7 % 5)], axis=1)
    sq = np.stack(project(P, np.eye(3), np.zeros(3)), axis=1).astype(np.float32)
    st = np.stack(project(P, rotation(0.03, -0.05, 0.02), np.array([0.4, 0.1, -0.2])), axis=1).astype(np.float32)
    ident = records([(j, j) for j in range(12)])
    for m in range(0, 13):
        for keep_unv in (0, 1):
            cases.append(case(1, m, 16, 8, keep_unv, 1.0, 12, 12, sq, st, ident[:m]))
    cases.append(case(7, 0, 64, 8, 0, 1.0, 12, 12, sq, st, ident))
    cases.append(case(7, 1, 64, 12, 0, 1.0, 12, 12, sq, st, ident))
    cases.append(case(7, 2, 64, 13, 1, 1.0, 12, 12, sq, st, ident))            # min_inliers beyond the records: not accepted
    # rectified stereo of the same points: y' = y, the last element of F is 0 - the free column is not the last
    stereo = np.stack(project(P, np.eye(3), np.array([-0.35, 0.0, 0.0])), axis=1).astype(np.float32)
    stereo[:, 1] = sq[:, 1]
    for p in range(4):
        cases.append(case(9, p, 64, 8, 0, 1.0, 12, 12, sq, stereo, ident))
    # no extent: all points of a side equal; a side on one axis-parallel line (three zero columns); on a slanted line
    one = np.tile(sq[:1], (12, 1))
    flat_y, flat_x, slant = sq.copy(), sq.copy(), sq.copy()
    flat_y[:, 1] = 77.0
    flat_x[:, 0] = 31.5
    slant[:, 1] = slant[:, 0] * np.float32(0.5) + np.float32(7.0)
    for keep_unv in (0, 1):
        cases.append(case(3, 0, 64, 8, keep_unv, 2.0, 12, 12, one, st, ident))
        cases.append(case(3, 1, 64, 8, keep_unv, 2.0, 12, 12, sq, one, ident))
        cases.append(case(3, 2, 64, 8, keep_unv, 2.0, 12, 12, flat_y, st, ident))
        cases.append(case(3, 3, 64, 8, keep_unv, 2.0, 12, 12, sq, flat_x, ident))
        cases.append(case(3, 4, 64, 8, keep_unv, 2.0, 12, 12, slant, st, ident))
    # duplicate points (two records with the same keypoints) and duplicate records
    dup = records([(0, 0), (0, 0), (1, 1), (1, 1), (2, 2), (3, 3), (2, 2), (4, 4), (5, 5), (6, 6), (7, 7), (7, 7)])
    cases.append(case(5, 0, 128, 8, 1, 1.0, 12, 12, sq, st, dup))
    # NaN / inf / -0.0 coordinates, on either side
    for side in (0, 1):
        for v in (np.nan, np.inf, -np.inf, -0.0):
            a, b = sq.copy(), st.copy()
            (a if side == 0 else b)[2, side] = v
            (a if side == 0 else b)[6, 1 - side] = v
            for keep_unv in (0, 1):
                cases.append(case(11, side, 64, 8, keep_unv, 1.0, 12, 12, a, b, ident))
    # indices at and beyond both limits, +-2^31 included; the keypoint arrays hold lim rows only
    lim = 10
    edge = [(q, t) for q in (-1, 0, lim - 1, lim, lim + 1, -2 ** 31, 2 ** 31 - 1) for t in (-1, 0, lim - 1, lim, -2 ** 31, 2 ** 31 - 1)]
    for keep_unv in (0, 1):
        cases.append(case(13, 0, 256, 8, keep_unv, 1.0, lim, lim, sq[:lim], st[:lim], records(edge + [(j, j) for j in range(lim)])))
        cases.append(case(13, 1, 256, 8, keep_unv, 1.0, lim, 5, sq[:lim], st[:5], records(edge + [(j, j) for j in range(lim)])))
        cases.append(case(13, 2, 16, 8, keep_unv, 1.0, 0, lim, sq[:0], st[:lim], ident))
    # max_error 0 / negative / NaN / inf
    for e in (0.0, -1.0, np.nan, np.inf, 1e-3):
        for keep_unv in (0, 1):
            cases.append(case(17, 0, 32, 8, keep_unv, e, 12, 12, sq, st, ident))
    # hypothesis counts 1 and 4096; huge seeds and pair numbers
    kq, kt, rec, _ = planted_depth(rng, "general", 24, 16)
    cases.append(case(0xFFFFFFFF, 2 ** 31 - 1, 1, 8, 1, 1.0, 40, 40, kq, kt, rec))
    cases.append(case(0, 0, 4096, 8, 0, 1.0, 40, 40, kq, kt, rec))
    # large coordinates, up to where fp32 ends
    for s in (8191.0, 1e6, 1e30, 3e38):
        cases.append(case(19, 0, 32, 8, 1, 1.0, 12, 12, sq * np.float32(s / 640.0), st * np.float32(s / 640.0), ident))
    # two hundred random pairs: the three scenes with noise and random records, unusable records mixed in
    for n in range(200):
        m = int(rng.integers(8, 70))
        true = int(rng.integers(0, m + 1))
        kq, kt, rec, _ = planted_depth(rng, ("general", "stereo", "plane")[n % 3], true, m - true, noise=float(rng.choice([0.0, 0.25, 1.0])))
        lim_a, lim_b = m, m
        if rng.integers(0, 3) == 0:
            lim_a, lim_b = int(rng.integers(0, m + 1)), int(rng.integers(0, m + 1))       # some rows do not exist
        if rng.integers(0, 3) == 0:
            bad = rng.integers(0, m, 3)
            rec["queryIdx"][bad[0]] = -1
            rec["trainIdx"][bad[1]] = m
            kq[bad[2], 0] = np.nan
        cases.append(case(int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 3000)), int(rng.choice([1, 7, 16, 64, 100])),
                          int(rng.integers(8, 16)), int(rng.integers(0, 2)), float(rng.choice([0.5, 1.5, 3.0])), lim_a, lim_b,
                          kq[:lim_a], kt[:lim_b], rec))
    return cases


def expected_lines(c):
    r = restated_pair8(c["seed"], c["p"], c["hyps"], c["min_inl"], c["keep_unv"], c["max_error"], c["lim_a"], c["lim_b"], c["kq"], c["kt"],
                       c["rec"])
    out = ["h %d %d %s %d %d %s" % (h, int(r["valid"][h]), " ".join(str(int(i)) for i in r["idx"][h]), int(r["free"][h]), int(r["count"][h]),
                                    hexes(r["F"][h])) for h in range(c["hyps"])]
    out.append("w %d %d %d %d %d" % (r["winner"], r["wcount"], int(r["accepted"]), r["nvalid"], int(r["usable"].sum())))
    out.append("k " + "".join("1" if k else "0" for k in r["keep"]))
    out.append("m " + hexes(r["model"]))
    return out, r


STEREO_CASES = slice(29, 33)         # where epipolar_cases puts the rectified pairs


def test_the_rule_agrees_with_its_restatement(tmp_path):
    cases = epipolar_cases()
    lines = run_program(build_program(), cases, tmp_path / "epipolar_cases.bin")
    assert len(lines) == sum(c["hyps"] + 3 for c in cases)
    at = 0
    accepted = rejected = invalid = partial = 0
    free = np.zeros(9, np.int64)
    stereo_free = np.zeros(9, np.int64)
    for n, c in enumerate(cases):
        want, r = expected_lines(c)
        got = lines[at:at + len(want)]
        for g, w in zip(got, want):
            assert g == w, (n, {k: v for k, v in c.items() if k not in ("kq", "kt", "rec")}, g, w)
        at += len(want)
        accepted += r["accepted"]
        rejected += not r["accepted"]
        invalid += int((~r["valid"]).sum())
        partial += bool(r["accepted"] and 0 < r["keep"].sum() < r["usable"].sum())
        free += np.bincount(r["free"][r["valid"]], minlength=9)
        if n in range(*STEREO_CASES.indices(len(cases))):
            assert c["p"] == n - STEREO_CASES.start and c["seed"] == 9
            stereo_free += np.bincount(r["free"][r["valid"]], minlength=9)
            assert r["accepted"] and r["wcount"] == 12                # exact rectified pairs: every record agrees
            assert abs(r["model"][8]) < 1e-9 and np.abs(r["model"][[5, 7]]).max() == 1.0       # F = [0 0 0; 0 0 -1; 0 1 0]
    print("the column left free, over every valid hypothesis:", free.tolist())
    print("in the rectified-stereo pairs:", stereo_free.tolist())
    # not vacuous: models are accepted and refused, hypotheses are invalid, accepted models drop usable records, and the pivoting
    # leaves other columns than the last free - always so in rectified stereo, where the last element of F is 0
    assert accepted > 60 and rejected > 50 and invalid > 1000 and partial > 40
    assert free[8] > 0 and (free[:8] > 0).sum() >= 3
    assert stereo_free.sum() > 100 and stereo_free[8] == 0


def test_the_rule_under_sanitizers(tmp_path):
    """the same program with the address and undefined-behaviour sanitizers, run stand-alone (nothing sanitized is loaded into Python)"""
    cases = epipolar_cases()
    plain = run_program(build_program(), cases, tmp_path / "a.bin")
    assert run_program(build_program(sanitize=True), cases, tmp_path / "b.bin") == plain


PINNED = [((0, 0, 0, 8), [4, 0, 7, 3, 1, 2, 5, 6]), ((0, 0, 1, 8), [3, 0, 5, 4, 2, 1, 7, 6]), ((1, 2, 3, 9), [4, 5, 8, 3, 0, 7, 6, 1]),
          ((4294967295, 2147483647, 4095, 40), [10, 20, 22, 39, 35, 24, 26, 2]), ((12345, 7, 100, 30), [4, 3, 14, 13, 11, 15, 19, 0]),
          ((9, 1025, 257, 2049), [1410, 846, 1367, 2016, 953, 352, 1794, 575]),
          ((42, 3, 63, 1000000), [815188, 579501, 505929, 942326, 378954, 957132, 451462, 127796])]


def test_a_pinned_sample():
    """literal (seed, p, h, m) -> eight indices, worked out with scalar_sample8: a silent change of the sampler shows"""
    assert len(PINNED) >= 6
    for (seed, p, h, m), want in PINNED:
        got = restated_sample8(seed, p, [h], m)[0].tolist()
        assert got == want == scalar_sample8(seed, p, h, m), ((seed, p, h, m), got, want)
        assert len(set(got)) == 8 and all(0 <= i < m for i in got)
    # distinct by construction, whatever m: at m = 8 every sample is a permutation of the eight records
    idx = restated_sample8(5, 9, np.arange(2000), 8)
    assert (np.sort(idx, axis=1) == np.arange(8)).all() and len({tuple(r) for r in idx.tolist()}) > 1900
    idx = restated_sample8(5, 9, np.arange(2000), 11)
    assert all(len(set(r)) == 8 for r in idx.tolist()) and idx.min() == 0 and idx.max() == 10
    for h in range(50):
        assert idx[h].tolist() == scalar_sample8(5, 9, h, 11)


PLANTED = {"general": (1, 2, 3), "stereo": (1, 2, 3), "plane": (1, 2, 3)}       # the seeds the condition below was met with


@pytest.mark.parametrize("kind", ["general", "stereo", "plane"])
def test_planted_models_are_found(kind):
    """NOT VACUOUS, a condition on the inputs: 48 true + 12 random records, noise 0.25 px, max_error 1.5, 256 hypotheses - the
    restatement alone accepts a model that keeps at least 90 % of the true records and at most 4 random ones"""
    for seed in PLANTED[kind]:
        rng = np.random.default_rng(700 + seed)
        kq, kt, rec, is_true = planted_depth(rng, kind, 48, 12)
        r = restated_pair8(seed, 0, 256, 8, 0, 1.5, 60, 60, kq, kt, rec)
        true_kept, random_kept = int((r["keep"] & is_true).sum()), int((r["keep"] & ~is_true).sum())
        print(kind, seed, "true kept", true_kept, "of 48, random kept", random_kept, "of 12, free column", int(r["free"][r["winner"]]))
        assert r["accepted"] and true_kept >= 0.9 * 48 and random_kept <= 4, (kind, seed, true_kept, random_kept)
        assert np.abs(r["model"]).max() == 1.0

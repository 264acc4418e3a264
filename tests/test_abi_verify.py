"""CPU checks of the geometric verification of pair matches (brisk_hip_verify_pair_matches_device): both libraries export the entry
point the header declares, Python has the call, the three kernels touch no scratch memory, and the rule - the very functions the
kernels call (csrc/brisk_pair_verify.h), built here for the host - agrees BIT FOR BIT with a NumPy float64 restatement written with
the header's parenthesisation.  restated_verify is the expectation of the GPU tests (test_gpu_verify.py) too."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import ethzasl_brisk_amd as B
from test_oracle_golden import H_1TO2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("brisk_hip_verify_pair_matches_device",)
M32 = np.uint64(0xFFFFFFFF)
PAIR_BAD, PAIR_NO_MODEL, ROWS_CUT = 2, 8, 0x100


def test_both_libraries_export_the_verifier():
    from ethzasl_brisk_amd import build
    hdr = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    declared = set(re.findall(r"\b(brisk_hip_[a-z_0-9]+)\s*\(", hdr))
    for lib in (build.build(), build.build_release()):
        L = ctypes.CDLL(lib)
        for s in NEW:
            assert s in declared, s
            assert s in B.ABI_SYMBOLS, s
            assert hasattr(L, s), (lib, s)
    for t in ("brisk_hip_pair_verify", "brisk_hip_pair_model"):
        assert re.search(r"typedef struct %s\b" % t, hdr), t
    m = re.search(r"#define BRISK_HIP_PAIR_NO_MODEL (0x[0-9a-fA-F]+|\d+)", hdr)
    assert m and int(m.group(1), 0) == B.PAIR_NO_MODEL == PAIR_NO_MODEL
    assert B.PAIR_BAD == PAIR_BAD and B.ROWS_CUT == ROWS_CUT


def header_fields(hdr, name):
    """[(type, declarator)] of a struct of the header, a declaration of several names taken apart"""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in (f.strip() for f in body.split(";") if f.strip()):
        parts = [x.strip() for x in decl.split(",")]
        kind, first = parts[0].rsplit(" ", 1)
        out += [(kind.strip(), n) for n in [first] + parts[1:]]
    return out


def test_python_has_the_verifier():
    hdr = open(os.path.join(ROOT, "include", "brisk_hip.h")).read()
    f = header_fields(hdr, "brisk_hip_pair_verify")
    assert f == [("float", "max_error"), ("int", "hypotheses"), ("int", "min_inliers"), ("int", "keep_unverified"), ("unsigned", "seed")]
    assert [n for n, _ in B.PairVerify._fields_] == [n for _, n in f]
    assert [t for _, t in B.PairVerify._fields_] == [ctypes.c_float, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_uint]
    assert ctypes.sizeof(B.PairVerify) == 20
    f = header_fields(hdr, "brisk_hip_pair_model")
    assert f == [("double", "h[9]")] + [("int", n) for n in ("records", "usable", "inliers", "hypothesis", "valid", "flags")]
    assert B.PAIR_MODEL.names == ("h", "records", "usable", "inliers", "hypothesis", "valid", "flags")
    assert B.PAIR_MODEL.itemsize == 96 and B.PAIR_MODEL["h"].shape == (9,) and B.PAIR_MODEL["h"].base == np.dtype("<f8")
    assert all(B.PAIR_MODEL[n] == np.dtype("<i4") for n in B.PAIR_MODEL.names[1:])
    par = inspect.signature(B.Context.verify_pair_matches).parameters
    assert list(par)[1:] == ["query", "train", "pairs", "rows_cap", "offsets", "matches", "verify", "out_cap", "query_kps", "train_kps",
                             "stream"]
    assert all(par[n].default is None for n in ("out_cap", "query_kps", "train_kps", "stream"))
    # the C arguments, in the header's order
    decl = re.search(r"int brisk_hip_verify_pair_matches_device\((.*?)\);", hdr, re.S).group(1)
    names = [a.strip().rsplit(" ", 1)[1].lstrip("*") for a in decl.split(",")]
    assert names == ["ctx", "query", "train", "query_kps", "train_kps", "pairs", "rows_cap", "d_offsets", "d_matches", "in_cap", "verify",
                     "out_cap", "d_models", "d_out_counts", "d_out_flags", "d_out_offsets", "d_out_matches", "stream"]


def test_verify_kernels_use_no_scratch():
    from ethzasl_brisk_amd import build
    build.build()
    res = build.kernel_resources()
    if not res:
        pytest.skip("the objects were not compiled here (no resource remarks beside them)")
    new = {k: v for k, v in res.items() if "k_verify_" in k}
    assert sorted(re.search(r"k_verify_[a-z]+", k).group(0) for k in new) == ["k_verify_offsets", "k_verify_ransac", "k_verify_scatter"]
    for k, v in new.items():
        assert v["scratch"] == 0, (k, v)
    ransac = [v for k, v in new.items() if "k_verify_ransac" in k][0]
    assert ransac["lds"] >= 1024 * 16                                  # the staged chunk: 1 024 records of four floats
    assert ransac["occupancy"] >= 5                                    # waves per SIMD: what the kernel had before its pieces were shared


# ---- the rule, restated ---------------------------------------------------------------------------------------------------------

def mix(x):
    x = np.asarray(x, np.uint64) & M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7feb352d)) & M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846ca68b)) & M32
    return x ^ (x >> np.uint64(16))


def restated_sample(seed, p, h, m):
    """(b): [len(h), 4] record indices, in draw order; m >= 4"""
    h = np.asarray(h, np.uint64)
    pair_seed = mix((mix(np.uint64(seed) ^ np.uint64(0x9E3779B9)) + np.uint64(p & 0xFFFFFFFF)) & M32)
    out = np.zeros((len(h), 4), np.int64)
    for k in range(4):
        r = (mix((pair_seed + np.uint64(4) * h + np.uint64(k)) & M32) * np.uint64(m - k)) >> np.uint64(32)
        r = r.astype(np.int64)
        chosen = np.sort(out[:, :k], axis=1)
        for c in range(k):                                              # the indices chosen before, in ascending order
            r = r + (chosen[:, c] <= r)
        out[:, k] = r
    return out


def det3(ax, ay, bx, by, cx, cy):
    m0 = bx * cy - cx * by
    m1 = cx * ay - ax * cy
    m2 = ax * by - bx * ay
    return (m0 + m1) + m2


def nonzero(d):
    return (d < 0) | (d > 0)


def basis(x, y):
    """x, y [n, 4] -> (ok [n], M[i][j] [n] as a 3 x 3 nest): [d0 p0 | d1 p1 | d2 p2]"""
    d = det3(x[:, 0], y[:, 0], x[:, 1], y[:, 1], x[:, 2], y[:, 2])
    d0 = det3(x[:, 3], y[:, 3], x[:, 1], y[:, 1], x[:, 2], y[:, 2])
    d1 = det3(x[:, 0], y[:, 0], x[:, 3], y[:, 3], x[:, 2], y[:, 2])
    d2 = det3(x[:, 0], y[:, 0], x[:, 1], y[:, 1], x[:, 3], y[:, 3])
    M = [[d0 * x[:, 0], d1 * x[:, 1], d2 * x[:, 2]], [d0 * y[:, 0], d1 * y[:, 1], d2 * y[:, 2]], [d0, d1, d2]]
    return nonzero(d) & nonzero(d0) & nonzero(d1) & nonzero(d2), M


def restated_model(x, y, xt, yt):
    """(c): the four point pairs of n samples [n, 4] -> (ok [n], H [n, 9])"""
    ok_a, A = basis(x, y)
    ok_b, Bm = basis(xt, yt)
    c = [[A[1][1] * A[2][2] - A[1][2] * A[2][1], A[0][2] * A[2][1] - A[0][1] * A[2][2], A[0][1] * A[1][2] - A[0][2] * A[1][1]],
         [A[1][2] * A[2][0] - A[1][0] * A[2][2], A[0][0] * A[2][2] - A[0][2] * A[2][0], A[0][2] * A[1][0] - A[0][0] * A[1][2]],
         [A[1][0] * A[2][1] - A[1][1] * A[2][0], A[0][1] * A[2][0] - A[0][0] * A[2][1], A[0][0] * A[1][1] - A[0][1] * A[1][0]]]
    H = np.stack([(Bm[i][0] * c[0][j] + Bm[i][1] * c[1][j]) + Bm[i][2] * c[2][j] for i in range(3) for j in range(3)], axis=1)
    return ok_a & ok_b, H


def restated_inliers(H, z_ref, thr2, x, y, xt, yt):
    """(d): H [n, 9], z_ref [n], the points [m] -> [n, m] bool (for usable records, with the threshold on)"""
    h = [H[:, i][:, None] for i in range(9)]
    z = (h[6] * x + h[7] * y) + h[8]
    ex = ((h[0] * x + h[1] * y) + h[2]) - z * xt
    ey = ((h[3] * x + h[4] * y) + h[5]) - z * yt
    return (z * z_ref[:, None] > 0) & ((ex * ex + ey * ey) <= thr2 * (z * z))


def restated_report(H):
    a = np.where(H < 0, -H, H)
    best, scale = 0.0, 0.0
    for i in range(9):
        if a[i] > best:
            best, scale = a[i], H[i]
    return H / scale if best > 0 else H.copy()


def restated_pair(seed, p, hypotheses, min_inliers, keep_unverified, max_error, lim_a, lim_b, kq, kt, rec):
    """one pair.  kq / kt: [rows, 2] float32 (x, y) of the two frames - only rows below lim are touched -, rec: DMATCH records.
    Returns a dict: per hypothesis valid / idx / count / H (zeros unless the four sampled records are usable), and the pair's
    winner, count, accepted, nvalid, usable [m], keep [m], model [9]."""
    m = len(rec)
    q, t = rec["queryIdx"].astype(np.int64), rec["trainIdx"].astype(np.int64)
    usable = (q >= 0) & (q < lim_a) & (t >= 0) & (t < lim_b)
    pts = np.zeros((m, 4), np.float64)
    for j in np.flatnonzero(usable):
        c = np.array([kq[q[j], 0], kq[q[j], 1], kt[t[j], 0], kt[t[j], 1]], np.float32)
        usable[j] = np.isfinite(c).all()
        pts[j] = c.astype(np.float64)
    nh = int(hypotheses)
    valid, idx, count, H = np.zeros(nh, bool), np.full((nh, 4), -1, np.int64), np.zeros(nh, np.int64), np.zeros((nh, 9), np.float64)
    z_ref = np.zeros(nh, np.float64)
    max_error = np.float32(max_error)
    thr_on = bool(max_error > 0)
    thr2 = np.float64(max_error) * np.float64(max_error)
    with np.errstate(all="ignore"):
        if m >= 4:
            idx = restated_sample(seed, p, np.arange(nh), m)
            assert (idx >= 0).all() and (idx < m).all() and all(len(set(r)) == 4 for r in idx[:64].tolist())
            full = usable[idx].all(axis=1)
            s = pts[idx]                                                # [nh, 4 points, 4 coordinates]
            ok, Hs = restated_model(s[:, :, 0], s[:, :, 1], s[:, :, 2], s[:, :, 3])
            valid = full & ok
            H[full] = Hs[full]
            z_ref = (H[:, 6] * s[:, 0, 0] + H[:, 7] * s[:, 0, 1]) + H[:, 8]
            if thr_on:
                u = np.flatnonzero(usable)
                for a in range(0, nh, 256):
                    sl = slice(a, a + 256)
                    inl = restated_inliers(H[sl], z_ref[sl], thr2, pts[u, 0], pts[u, 1], pts[u, 2], pts[u, 3])
                    count[sl] = inl.sum(axis=1)
                count[~valid] = 0
        winner, wcount = -1, 0
        for h in np.flatnonzero(valid):                                # the most inliers, the smallest h
            if winner < 0 or count[h] > wcount:
                winner, wcount = int(h), int(count[h])
        accepted = winner >= 0 and wcount >= min_inliers
        keep = np.zeros(m, bool)
        if accepted:
            u = np.flatnonzero(usable)
            keep[u] = restated_inliers(H[winner:winner + 1], z_ref[winner:winner + 1], thr2, pts[u, 0], pts[u, 1], pts[u, 2], pts[u, 3])[0]
            assert int(keep.sum()) == wcount
        elif keep_unverified:
            keep = usable.copy()
        model = restated_report(H[winner]) if winner >= 0 else np.zeros(9, np.float64)
    return {"valid": valid, "idx": idx, "count": count, "H": H, "winner": winner, "wcount": wcount, "accepted": bool(accepted),
            "nvalid": int(valid.sum()), "usable": usable, "keep": keep, "model": model}


def restated_verify(frames, counts_q, counts_t, rows_cap, kq, kt, offsets, matches, verify, in_cap, out_cap, frames_q=None, frames_t=None):
    """the whole call.  frames: [(a, b)] per pair; counts_q / counts_t: the sets' row counts per frame; kq / kt: per frame a [rows, 2]
    float32 array; verify: (max_error, hypotheses, min_inliers, keep_unverified, seed).  Returns (models PAIR_MODEL [npairs], counts,
    flags, offsets [npairs + 1], the stored records)."""
    max_error, hyps, min_inl, keep_unv, seed = verify
    n = len(frames)
    frames_q = len(counts_q) if frames_q is None else frames_q
    frames_t = len(counts_t) if frames_t is None else frames_t
    models = np.zeros(n, B.PAIR_MODEL)
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
        r = restated_pair(seed, p, hyps, min_inl, keep_unv, max_error, lim_a, lim_b, kq[a], kt[b], rec)
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


# ---- the rule's own code against the restatement -----------------------------------------------------------------------------------

def build_program(sanitize=False):
    """tests/cpp/test_pair_verify.cc: plain host C++ around csrc/brisk_pair_verify.h (no HIP, no library)"""
    src = os.path.join(ROOT, "tests", "cpp", "test_pair_verify.cc")
    hdr = os.path.join(ROOT, "ethzasl_brisk_amd", "csrc", "brisk_pair_verify.h")
    out = os.path.join(ROOT, "tests", "cpp", "test_pair_verify" + ("_san" if sanitize else ""))
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in (src, hdr)):
        extra = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-ffp-contract=off"] + extra + ["-I" + os.path.dirname(hdr), "-o", out, src])
    return out


def records(rows):
    a = np.zeros(len(rows), B.DMATCH)
    for n, (q, t) in enumerate(rows):
        a[n] = (q, t, 3, float(n % 7))
    return a


def apply_h(H, x, y):
    """the reference's transfer (test-match.cc:105-106), rounded to float as keypoints are"""
    w = H[2, 0] * x + H[2, 1] * y + H[2, 2]
    return (((H[0, 0] * x + H[0, 1] * y + H[0, 2]) / w).astype(np.float32), ((H[1, 0] * x + H[1, 1] * y + H[1, 2]) / w).astype(np.float32))


def planted(rng, n, inliers, noise=0.0, shuffle=True):
    """n records, the first `inliers` (before shuffling) exact float-rounded inliers of the reference's H_1to2, the others with a
    random train point at least 20 px from where H sends them.  Returns (kq, kt, rec, is_inlier [n])."""
    x = rng.uniform(20, 620, n).astype(np.float32)
    y = rng.uniform(20, 460, n).astype(np.float32)
    xt, yt = apply_h(H_1TO2, x.astype(np.float64), y.astype(np.float64))
    if noise:
        xt = (xt + rng.normal(0, noise, n)).astype(np.float32)
        yt = (yt + rng.normal(0, noise, n)).astype(np.float32)
    for j in range(inliers, n):
        while True:
            ox, oy = np.float32(rng.uniform(0, 640)), np.float32(rng.uniform(0, 640))
            if np.hypot(ox - xt[j], oy - yt[j]) > 20:
                break
        xt[j], yt[j] = ox, oy
    order = rng.permutation(n) if shuffle else np.arange(n)
    tperm = rng.permutation(n)                                         # train rows in another order than query rows
    kq = np.stack([x, y], axis=1)
    kt = np.zeros((n, 2), np.float32)
    kt[tperm] = np.stack([xt, yt], axis=1)
    rec = records([(int(j), int(tperm[j])) for j in order])
    return kq, kt, rec, order < inliers


def case(seed, p, hyps, min_inl, keep_unv, max_error, lim_a, lim_b, kq, kt, rec):
    return dict(seed=seed, p=p, hyps=hyps, min_inl=min_inl, keep_unv=keep_unv, max_error=np.float32(max_error), lim_a=lim_a, lim_b=lim_b,
                kq=np.asarray(kq, np.float32).reshape(-1, 2), kt=np.asarray(kt, np.float32).reshape(-1, 2), rec=rec)


def verify_cases():
    rng = np.random.default_rng(4321)
    cases = []
    sq = np.array([[10, 10], [200, 15], [210, 180], [5, 190], [100, 100], [50, 150], [150, 60], [120, 170]], np.float32)
    st = np.stack(apply_h(H_1TO2, sq[:, 0].astype(np.float64), sq[:, 1].astype(np.float64)), axis=1)
    ident = records([(j, j) for j in range(8)])
    # hand cases: exact inliers of one model; every m from 0 to 5; both keep settings
    for m in range(0, 6):
        for keep_unv in (0, 1):
            cases.append(case(1, m, 16, 4, keep_unv, 1.0, 8, 8, sq, st, ident[:m]))
    cases.append(case(7, 0, 64, 4, 0, 1.0, 8, 8, sq, st, ident))
    cases.append(case(7, 1, 64, 8, 0, 1.0, 8, 8, sq, st, ident))
    cases.append(case(7, 2, 64, 9, 1, 1.0, 8, 8, sq, st, ident))              # min_inliers beyond the records: not accepted
    # collinear points: every sample has three on a line on the query side; then on the train side only
    line = np.stack([np.arange(8, dtype=np.float32) * 10, np.arange(8, dtype=np.float32) * 20 + 5], axis=1)
    cases.append(case(3, 0, 64, 4, 1, 2.0, 8, 8, line, st, ident))
    cases.append(case(3, 1, 64, 4, 0, 2.0, 8, 8, sq, line, ident))
    # duplicate points (two records with the same keypoints) and duplicate records
    dup = records([(0, 0), (0, 0), (1, 1), (1, 1), (2, 2), (3, 3), (2, 2), (4, 4)])
    cases.append(case(5, 0, 128, 4, 1, 1.0, 8, 8, sq, st, dup))
    same = sq.copy()
    same[1] = same[0]
    cases.append(case(5, 1, 128, 4, 1, 1.0, 8, 8, same, st, ident))
    # NaN / inf / -0.0 coordinates, on either side
    for side in (0, 1):
        for v in (np.nan, np.inf, -np.inf, -0.0):
            a, b = sq.copy(), st.copy()
            (a if side == 0 else b)[2, side] = v
            (a if side == 0 else b)[6, 1 - side] = v
            for keep_unv in (0, 1):
                cases.append(case(11, side, 64, 4, keep_unv, 1.0, 8, 8, a, b, ident))
    # indices at and beyond both limits, +-2^31 included; the keypoint arrays hold lim rows only
    lim = 6
    edge = [(q, t) for q in (-1, 0, lim - 1, lim, lim + 1, -2 ** 31, 2 ** 31 - 1) for t in (-1, 0, lim - 1, lim, -2 ** 31, 2 ** 31 - 1)]
    for keep_unv in (0, 1):
        cases.append(case(13, 0, 256, 4, keep_unv, 1.0, lim, lim, sq[:lim], st[:lim], records(edge + [(j, j) for j in range(lim)])))
        cases.append(case(13, 1, 256, 4, keep_unv, 1.0, lim, 3, sq[:lim], st[:3], records(edge + [(j, j) for j in range(lim)])))
        cases.append(case(13, 2, 16, 4, keep_unv, 1.0, 0, lim, sq[:0], st[:lim], ident))
    # max_error 0 / negative / NaN / inf
    for e in (0.0, -1.0, np.nan, np.inf, 1e-3):
        for keep_unv in (0, 1):
            cases.append(case(17, 0, 32, 4, keep_unv, e, 8, 8, sq, st, ident))
    # hypothesis counts 1 and 4096; huge seeds and pair numbers
    kq, kt, rec, _ = planted(rng, 40, 24)
    cases.append(case(0xFFFFFFFF, 2 ** 31 - 1, 1, 4, 1, 1.0, 40, 40, kq, kt, rec))
    cases.append(case(0, 0, 4096, 4, 0, 1.0, 40, 40, kq, kt, rec))
    # large coordinates: beyond the 8191 the magnitudes are stated for, up to where fp64 overflows
    for s in (8191.0, 1e6, 1e30, 3e38):
        cases.append(case(19, 0, 32, 4, 1, 1.0, 8, 8, sq * np.float32(s / 210.0), st * np.float32(s / 400.0), ident))
    # a few hundred random pairs: planted models with noise and outliers, unusable records mixed in
    for n in range(300):
        m = int(rng.integers(4, 80))
        kq, kt, rec, _ = planted(rng, m, int(rng.integers(0, m + 1)), noise=float(rng.choice([0.0, 0.3, 1.0])))
        lim_a, lim_b = m, m
        if rng.integers(0, 3) == 0:
            lim_a, lim_b = int(rng.integers(0, m + 1)), int(rng.integers(0, m + 1))       # some rows do not exist
        if rng.integers(0, 3) == 0:
            bad = rng.integers(0, m, 3)
            rec["queryIdx"][bad[0]] = -1
            rec["trainIdx"][bad[1]] = m
            kq[bad[2], 0] = np.nan
        cases.append(case(int(rng.integers(0, 2 ** 32)), int(rng.integers(0, 3000)), int(rng.choice([1, 7, 16, 64, 100])),
                          int(rng.integers(4, 12)), int(rng.integers(0, 2)), float(rng.choice([0.5, 1.0, 3.0])), lim_a, lim_b,
                          kq[:lim_a], kt[:lim_b], rec))
    return cases


def run_program(prog, cases, path):
    words = []
    for c in cases:
        words.append(np.array([c["seed"], c["p"] & 0xFFFFFFFF, c["hyps"], c["min_inl"], c["keep_unv"]], np.uint32))
        words.append(np.array([c["max_error"]], np.float32).view(np.uint32))
        words.append(np.array([c["lim_a"], c["lim_b"], len(c["rec"])], np.uint32))
        assert len(c["kq"]) == c["lim_a"] and len(c["kt"]) == c["lim_b"]
        words.append(np.ascontiguousarray(c["kq"]).view(np.uint32).reshape(-1))
        words.append(np.ascontiguousarray(c["kt"]).view(np.uint32).reshape(-1))
        words.append(np.ascontiguousarray(c["rec"]).view(np.uint32).reshape(-1))
    np.concatenate(words).astype("<u4").tofile(path)
    out = subprocess.run([prog, str(path)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    return out.stdout.split("\n")[:-1]


def hexes(v):
    return " ".join("%016x" % int(b) for b in np.asarray(v, np.float64).view(np.uint64))


def expected_lines(c):
    r = restated_pair(c["seed"], c["p"], c["hyps"], c["min_inl"], c["keep_unv"], c["max_error"], c["lim_a"], c["lim_b"], c["kq"], c["kt"],
                      c["rec"])
    out = ["h %d %d %d %d %d %d %d %s" % ((h, int(r["valid"][h])) + tuple(int(i) for i in r["idx"][h]) + (int(r["count"][h]), hexes(r["H"][h])))
           for h in range(c["hyps"])]
    out.append("w %d %d %d %d %d" % (r["winner"], r["wcount"], int(r["accepted"]), r["nvalid"], int(r["usable"].sum())))
    out.append("k " + "".join("1" if k else "0" for k in r["keep"]))
    out.append("m " + hexes(r["model"]))
    return out, r


def test_the_rule_agrees_with_its_restatement(tmp_path):
    cases = verify_cases()
    lines = run_program(build_program(), cases, tmp_path / "verify_cases.bin")
    assert len(lines) == sum(c["hyps"] + 3 for c in cases)
    at = 0
    accepted = rejected = invalid = partial = 0
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
    # not vacuous: models are accepted and refused, hypotheses are invalid, accepted models drop usable records
    assert accepted > 100 and rejected > 50 and invalid > 1000 and partial > 50


def test_the_rule_under_sanitizers(tmp_path):
    """the same program with the address and undefined-behaviour sanitizers, run stand-alone (nothing sanitized is loaded into Python)"""
    cases = verify_cases()
    plain = run_program(build_program(), cases, tmp_path / "a.bin")
    assert run_program(build_program(sanitize=True), cases, tmp_path / "b.bin") == plain


PINNED = [((0, 0, 0, 4), [2, 0, 3, 1]), ((0, 0, 1, 4), [0, 1, 2, 3]), ((1, 2, 3, 5), [0, 2, 1, 4]),
          ((4294967295, 2147483647, 4095, 40), [18, 7, 26, 27]), ((12345, 7, 100, 30), [26, 16, 4, 7]),
          ((9, 1025, 257, 2049), [1863, 627, 446, 1277]), ((42, 3, 63, 1000000), [361481, 824902, 349243, 91935])]


def test_a_pinned_sample():
    """literal (seed, p, h, m) -> indices: a silent change of the sampler shows"""
    for (seed, p, h, m), want in PINNED:
        got = restated_sample(seed, p, [h], m)[0].tolist()
        assert got == want, ((seed, p, h, m), got, want)
        assert len(set(got)) == 4 and all(0 <= i < m for i in got)
    # distinct by construction, whatever m: every 4-subset position is reachable at m = 4
    idx = restated_sample(5, 9, np.arange(2000), 4)
    assert (np.sort(idx, axis=1) == np.arange(4)).all() and len({tuple(r) for r in idx.tolist()}) == 24
    idx = restated_sample(5, 9, np.arange(2000), 7)
    assert all(len(set(r)) == 4 for r in idx.tolist()) and idx.min() == 0 and idx.max() == 6


def test_planted_models_are_found():
    """NOT VACUOUS, a condition: on noise-free inliers of the reference's H_1to2 (rounded to float), at least half of 40 records,
    256 hypotheses, max_error 1.0, the restatement alone accepts the model and keeps every planted inlier and no outlier"""
    for seed, inl in ((1, 20), (2, 24), (3, 30), (4, 20), (5, 36)):
        rng = np.random.default_rng(100 + seed)
        kq, kt, rec, is_inl = planted(rng, 40, inl)
        r = restated_pair(seed, 0, 256, 8, 0, 1.0, 40, 40, kq, kt, rec)
        assert r["accepted"] and r["wcount"] == inl, (seed, inl, r["wcount"])
        assert np.array_equal(r["keep"], is_inl), (seed, inl)
        # the reported model transfers every planted inlier to within max_error of its train point - the reference's own check
        # (test-match.cc:105-107), with the division the rule avoids
        M = r["model"].reshape(3, 3)
        q, t = rec["queryIdx"][is_inl], rec["trainIdx"][is_inl]
        x, y = kq[q, 0].astype(np.float64), kq[q, 1].astype(np.float64)
        w = M[2, 0] * x + M[2, 1] * y + M[2, 2]
        ex, ey = (M[0, 0] * x + M[0, 1] * y + M[0, 2]) / w - kt[t, 0], (M[1, 0] * x + M[1, 1] * y + M[1, 2]) / w - kt[t, 1]
        assert np.hypot(ex, ey).max() <= 1.0 + 1e-9
        assert np.abs(M).max() == 1.0

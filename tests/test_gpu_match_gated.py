"""GPU tests of brisk_hip_match_knn_pairs_gated_device / brisk_hip_match_radius_pairs_gated_device: the pair matchers behind a
position gate on the rows' keypoints.  The gate defines a mask per pair; everything is compared with the CPU oracle matching with
that mask (oracle/brisk_oracle_match.c) - k-NN rows without the reference's top-up entries (distance 2147483648.f), which the
gated call never writes - integer fields equal, distances equal as bit patterns, counts equal: no tolerance."""
import ctypes as C

import numpy as np
import pytest

from gpu_prefill import settled
import oracle_lib as O
from test_gpu_match_pairs import CAP, COUNTS_A, COUNTS_B, SENTINEL, SynthSet, batch_frames, pair_list, same_rows
from test_oracle_golden import H_1TO2, homography_outliers

pytestmark = pytest.mark.gpu

INF = float("inf")
WINDOW = (-40.0, 40.0, -40.0, 40.0, 1)      # a tracking window
BAND = (-64.0, 0.0, -2.0, 2.0, -1)          # a stereo band
ALL_PASS = (-INF, INF, -INF, INF, -1)
TOP_UP = np.float32(2147483648.0)
LIST = 32                                   # MRP_LIST: radius rows with more hits take the kernel's dense path


@pytest.fixture(scope="module")
def B():
    import ethzasl_brisk_amd as B
    from ethzasl_brisk_amd import build
    build.build()
    B.load_library()
    return B


# ---- the oracle under the mask a gate defines ------------------------------------------------------------------------------

def gate_mask(g, kq, kt):
    """M[q][t] in numpy float32: one subtraction each, float32 compares (NaN: false), octave difference in integers"""
    qx, qy, qo = kq["x"].astype(np.float32), kq["y"].astype(np.float32), kq["octave"].astype(np.int64)
    tx, ty, to = kt["x"].astype(np.float32), kt["y"].astype(np.float32), kt["octave"].astype(np.int64)
    with np.errstate(invalid="ignore"):
        dx, dy = tx[None, :] - qx[:, None], ty[None, :] - qy[:, None]
        m = (dx >= np.float32(g[0])) & (dx <= np.float32(g[1])) & (dy >= np.float32(g[2])) & (dy <= np.float32(g[3]))
    if g[4] >= 0:
        m &= np.abs(to[None, :] - qo[:, None]) <= g[4]
    return np.ascontiguousarray(m.astype(np.uint8))


def oracle_knn(dq, dt, M, b, k):
    if len(dq) == 0:
        return []
    if len(dt) == 0:
        return [np.zeros(0, O.DMATCH) for _ in range(len(dq))]
    want = [r[r["distance"] != TOP_UP] for r in O.match_knn(dq, [dt], k, masks=[M])]
    for r in want:
        r["imgIdx"] = b
    return want


def oracle_cross(dq, dt, M, b):
    fwd = oracle_knn(dq, dt, M, b, 1)
    back = oracle_knn(dt, dq, np.ascontiguousarray(M.T), 0, 1)
    return [r if len(r) == 1 and len(back[int(r[0]["trainIdx"])]) == 1 and back[int(r[0]["trainIdx"])][0]["trainIdx"] == q else r[:0]
            for q, r in enumerate(fwd)]


def oracle_radius(dq, dt, M, b, max_distance):
    if len(dq) == 0:
        return []
    if len(dt) == 0:
        return [np.zeros(0, O.DMATCH) for _ in range(len(dq))]
    want = O.match_radius(dq, [dt], max_distance, masks=[M])
    for r in want:
        r["imgIdx"] = b
    return want


def same_cut(got_rows, got_counts, want, cap):
    assert len(got_rows) == len(want) == len(got_counts)
    assert [int(c) for c in got_counts] == [len(w) for w in want]
    same_rows(got_rows, [w[:cap] for w in want])


def knn_rows(B, host, k):
    m, cnt, rows = host
    npairs, cap = cnt.shape
    m = m.view(B.DMATCH).reshape(npairs, cap, k)
    return [[m[p, q, :cnt[p, q]] for q in range(min(max(int(rows[p]), 0), cap))] for p in range(npairs)], rows


def radius_rows(B, host, cpq):
    m, cnt, rows = host
    npairs, cap = cnt.shape
    m = m.view(B.DMATCH).reshape(npairs, cap, cpq)
    nrows = [min(max(int(rows[p]), 0), cap) for p in range(npairs)]
    return ([[m[p, q, :min(cnt[p, q], cpq)] for q in range(nrows[p])] for p in range(npairs)], [cnt[p, :nrows[p]] for p in range(npairs)],
            rows)


def wave_skip_share(M):
    """share of the (64-query wave, train row) steps in which no lane is allowed"""
    steps = skipped = 0
    for w0 in range(0, M.shape[0], 64):
        live = M[w0:w0 + 64].any(axis=0)
        steps, skipped = steps + live.size, skipped + int((~live).sum())
    return skipped / max(steps, 1)


# ---- 1: the batch's own results, nothing on the host in between --------------------------------------------------------------

BATCH_CAP = 8


def homography_gate(kq):
    """a gate that contains the displacement H_1TO2 gives every query keypoint, with 8 pixels to spare (the inlier bound is 5)"""
    p = H_1TO2 @ np.stack([kq["x"].astype(np.float64), kq["y"].astype(np.float64), np.ones(len(kq))])
    dx, dy = p[0] / p[2] - kq["x"], p[1] / p[2] - kq["y"]
    return (float(np.floor(dx.min() - 8)), float(np.ceil(dx.max() + 8)), float(np.floor(dy.min() - 8)), float(np.ceil(dy.max() + 8)), -1)


@pytest.fixture(scope="module")
def batch(B, golden_ast):
    import torch
    frames = batch_frames(golden_ast)
    n, h, w = frames.shape
    d = torch.from_numpy(frames).cuda()
    ctx = B.Context(0)
    ext = B.BriskDescriptorExtractor(context=ctx)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    spec = B.PairSpec(n - 1, 1, 1, 0, 1, None)   # frame to previous frame
    # the homography gate needs img1's keypoints, which only exist after a batch: taken from the oracle's own detection instead
    hk, _ = O.Extractor().compute(golden_ast[0]["image"], O.detect(golden_ast[0]["image"], 70, 2))
    gates = {"window": WINDOW, "band": BAND, "homography": homography_gate(hk)}
    # detect + describe and all gated calls back to back on one stream: counts, rows, keypoints and pitches never visit the host
    ctx.detect_describe_batch(ext, d.data_ptr(), n, w, h, w * h, w, 70, 2, s.cuda_stream)
    st, dim = ctx.batch_desc_set()
    kps = ctx.batch_kp_set()
    res = {}
    for name, g in gates.items():
        gate = B.MatchGate(*g)
        for kk in (1, 2):
            res[name, kk] = ctx.match_knn_pairs(st, st, spec, kk, stream=s.cuda_stream, gate=gate, query_kps=kps, train_kps=kps)
        res[name, "cross"] = ctx.match_knn_pairs(st, st, spec, 1, cross_check=True, stream=s.cuda_stream, gate=gate)   # (kps: the batch's)
        for r in (50.0, 90.0):
            res[name, r] = ctx.match_radius_pairs(st, st, spec, r, BATCH_CAP, stream=s.cuda_stream, gate=gate, query_kps=kps, train_kps=kps)
    torch.cuda.synchronize()
    assert ctx.batch_status(n) == 0
    host = {key: tuple(t.cpu().numpy() for t in v) for key, v in res.items()}
    kd = [ctx.batch_download(f, True, strings=dim) for f in range(n)]
    out = {"n": n, "dim": dim, "kps": [k for k, _ in kd], "desc": [dd for _, dd in kd], "host": host, "B": B, "gates": gates}
    yield out
    ext.close()
    ctx.close()


@pytest.mark.parametrize("name", ["window", "band"])
def test_batch_results_without_the_host(batch, name):
    B, desc, kps, n, g = batch["B"], batch["desc"], batch["kps"], batch["n"], batch["gates"][name]
    assert batch["dim"] == 48 and n >= 8
    counts = np.array([len(d) for d in desc])
    assert counts[3] == 0 and (np.delete(counts, 3) > 0).all()     # the blank frame is inside the batch
    masks = [gate_mask(g, kps[p + 1], kps[p]) for p in range(n - 1)]
    allowed = np.concatenate([M.sum(axis=1) for M in masks])
    density = sum(int(M.sum()) for M in masks) / max(sum(M.size for M in masks), 1)
    skip = np.mean([wave_skip_share(M) for M in masks if M.size])
    print("%s: mask density %.4f, rows with nothing / one / more than two allowed: %d / %d / %d of %d, skippable steps %.3f" %
          (name, density, (allowed == 0).sum(), (allowed == 1).sum(), (allowed > 2).sum(), allowed.size, skip))
    # not vacuous - on what the ORACLE's masks give
    assert (allowed == 0).sum() >= 1 and (allowed == 1).sum() >= 1 and (allowed > 2).sum() >= 1
    for k in (1, 2):
        got, rows = knn_rows(B, batch["host"][name, k], k)
        assert np.array_equal(rows, counts[1:])                    # d_pair_rows = the described counts of the query frames
        for p in range(n - 1):
            same_rows(got[p], oracle_knn(desc[p + 1], desc[p], masks[p], p, k))
    got, rows = knn_rows(B, batch["host"][name, "cross"], 1)
    assert np.array_equal(rows, counts[1:])
    kept = rejected = 0
    for p in range(n - 1):
        want = oracle_cross(desc[p + 1], desc[p], masks[p], p)
        fwd = oracle_knn(desc[p + 1], desc[p], masks[p], p, 1)
        kept += sum(len(w) for w in want)
        rejected += sum(len(f) - len(w) for f, w in zip(fwd, want))
        same_rows(got[p], want)
    print("%s: the cross check keeps %d and rejects %d" % (name, kept, rejected))
    assert kept >= 1 and rejected >= 1
    for r in (50.0, 90.0):
        got, cnt, rows = radius_rows(B, batch["host"][name, r], BATCH_CAP)
        assert np.array_equal(rows, counts[1:])
        hits = 0
        for p in range(n - 1):
            want = oracle_radius(desc[p + 1], desc[p], masks[p], p, r)
            same_cut(got[p], cnt[p], want, BATCH_CAP)
            hits += sum(len(w) for w in want)
        print("%s: %d radius hits at %g" % (name, hits, r))
        if name == "window":                                       # (the band leaves too few to mean anything)
            assert hits >= 1


def test_pair_0_under_a_gate_that_contains_the_homography(batch):
    B, desc, kps, g = batch["B"], batch["desc"], batch["kps"], batch["gates"]["homography"]
    got, _ = knn_rows(B, batch["host"]["homography", 1], 1)
    M = gate_mask(g, kps[1], kps[0])
    same_rows(got[0], oracle_knn(desc[1], desc[0], M, 0, 1))
    print("homography gate", g, "density %.3f" % M.mean())
    assert 0 < M.mean() < 1
    # pair 0 = (img1, img2): the reference's matching test (brisk/src/test/test-match.cc:49-126).  Every ungated best match below 50
    # bits is an inlier (tests/test_gpu_match_pairs.py), so it lies inside this gate and stays the best: the same > 100 matches
    best = np.concatenate([r for r in got[0] if len(r) and r[0]["distance"] < 50])
    assert len(best) > 100
    assert homography_outliers(kps[1], kps[0], best) == 0


# ---- 2: caller sets in torch device memory ------------------------------------------------------------------------------------

class SynthKp:
    """keypoint records for the rows of a SynthSet, on a coarse grid (differences hit the gate's bounds exactly); the bytes of the
    buffer outside the counted records are random, some counted records have NaN coordinates"""

    def __init__(self, B, rng, counts, cap, slack=0, nan_every=0, spread=(8, 6)):
        import torch
        rec = B.KEYPOINT.itemsize
        assert rec == 28
        pitch = cap * rec + slack
        buf = rng.integers(0, 256, len(counts) * pitch + 64, dtype=np.uint8)
        self.kps = []
        for f, c in enumerate(counts):
            k = np.frombuffer(rng.integers(0, 256, max(c, 1) * rec, dtype=np.uint8).tobytes(), B.KEYPOINT)[:c].copy()
            k["x"] = 8.0 * rng.integers(0, spread[0], c)
            k["y"] = 8.0 * rng.integers(0, spread[1], c)
            k["octave"] = rng.integers(0, 4, c)
            if nan_every:
                k["x"][f % nan_every::nan_every] = np.nan
                k["y"][(f + 2) % (2 * nan_every)::2 * nan_every] = np.nan
            buf[f * pitch:f * pitch + c * rec] = k.view(np.uint8)
            self.kps.append(k)
        self.t_buf = torch.from_numpy(buf).cuda()
        self.set = B.KpSet(self.t_buf.data_ptr(), pitch)


GRID_GATE = (-16.0, 16.0, -8.0, 8.0, 1)


def spec_of(B, pairs):
    import torch
    if isinstance(pairs, tuple):
        return B.PairSpec(pairs[0], *pairs[1:], None), pair_list(pairs[1:], pairs[0]), None
    keep = torch.from_numpy(np.array(pairs, np.int32).reshape(-1, 2)).cuda()
    return B.PairSpec(len(pairs), 0, 0, 0, 0, keep.data_ptr()), list(pairs), keep


def run_knn(B, ctx, qs, qk, ts, tk, pairs, g, k, cross=False, rows_cap=CAP, classes=None):
    import torch
    spec, plist, keep = spec_of(B, pairs)
    torch.cuda.synchronize()
    got = ctx.match_knn_pairs(qs.set, ts.set, spec, k, cross_check=cross, rows_cap=rows_cap, dim_bytes=qs.dim, download=True,
                              gate=B.MatchGate(*g), query_kps=qk.set, train_kps=tk.set)
    assert len(got) == len(plist)
    for (a, b), rows in zip(plist, got):
        if not (0 <= a < len(qs.desc) and 0 <= b < len(ts.desc)):
            assert rows == []                                       # a bad entry of the list: d_pair_rows -1, no rows
            continue
        M = gate_mask(g, qk.kps[a], tk.kps[b])
        want = oracle_cross(qs.desc[a], ts.desc[b], M, b) if cross else oracle_knn(qs.desc[a], ts.desc[b], M, b, k)
        same_rows(rows, want[:rows_cap])
        if classes is not None:
            classes += [len(w) for w in want[:rows_cap]]


def run_radius(B, ctx, qs, qk, ts, tk, pairs, g, max_distance, cap, rows_cap=CAP, classes=None):
    import torch
    spec, plist, keep = spec_of(B, pairs)
    torch.cuda.synchronize()
    got, counts = ctx.match_radius_pairs(qs.set, ts.set, spec, max_distance, cap, rows_cap=rows_cap, dim_bytes=qs.dim, download=True,
                                         gate=B.MatchGate(*g), query_kps=qk.set, train_kps=tk.set)
    assert len(got) == len(plist) == len(counts)
    for (a, b), rows, c in zip(plist, got, counts):
        if not (0 <= a < len(qs.desc) and 0 <= b < len(ts.desc)):
            assert rows == [] and len(c) == 0
            continue
        want = oracle_radius(qs.desc[a], ts.desc[b], gate_mask(g, qk.kps[a], tk.kps[b]), b, max_distance)[:rows_cap]
        same_cut(rows, c, want, cap)
        if classes is not None:
            classes += [len(w) for w in want]


def forms(A, Ak, Bs, Bk, nA, shuffled):
    return [(A, Ak, A, Ak, (nA - 1, 1, 1, 0, 1)),      # frame to previous frame
            (A, Ak, A, Ak, (nA // 2, 0, 2, 1, 2)),     # interleaved stereo
            (A, Ak, Bs, Bk, (nA, 0, 1, 0, 1)),         # two sets side by side
            (A, Ak, Bs, Bk, (nA, 0, 1, 3, 0)),         # all against a keyframe with ONE row
            (Bs, Bk, A, Ak, (nA, 0, 1, 5, 0)),         # ... and against the full frame (130 rows)
            (A, Ak, Bs, Bk, shuffled)]                 # a shuffled device list with a repeat and a bad entry


@pytest.mark.parametrize("dim,pitch,base_off,slack", [(16, 20, 0, 0), (32, 48, 0, 4), (48, 64, 0, 0), (48, 51, 1, 3), (64, 64, 0, 0)])
def test_caller_sets_and_pair_forms(B, dim, pitch, base_off, slack):
    rng = np.random.default_rng(dim * 1000 + pitch + 1)
    ctx = B.default_context(0)
    A = SynthSet(B, rng, dim, pitch, COUNTS_A, CAP, base_off, 3, slack)          # (48, 51, 1, 3): unaligned rows
    Bs = SynthSet(B, rng, dim, pitch + 4 * (dim == 48), COUNTS_B, CAP, 0, 1, 0)
    Ak = SynthKp(B, rng, COUNTS_A, CAP, slack=40, nan_every=17)                  # a frame pitch larger than cap * 28
    Bk = SynthKp(B, rng, COUNTS_B, CAP, nan_every=23)
    nA = len(COUNTS_A)
    shuffled = [(int(a), int(b)) for a, b in zip(rng.integers(0, nA, 9), rng.integers(0, nA, 9))]
    shuffled.insert(4, shuffled[1])                                 # a repeated pair
    shuffled.insert(2, (nA, 0))                                     # a bad entry
    all_forms = forms(A, Ak, Bs, Bk, nA, shuffled)
    n1, n2, nx, nr = [], [], [], []
    for qs, qk, ts, tk, pr in all_forms:
        run_knn(B, ctx, qs, qk, ts, tk, pr, GRID_GATE, 1, classes=n1)
        run_knn(B, ctx, qs, qk, ts, tk, pr, GRID_GATE, 2, classes=n2)
        run_knn(B, ctx, qs, qk, ts, tk, pr, GRID_GATE, 1, cross=True, classes=nx)
        run_radius(B, ctx, qs, qk, ts, tk, pr, GRID_GATE, 4 * dim + 0.5, 8, classes=nr)
        run_radius(B, ctx, qs, qk, ts, tk, pr, (0.0, INF, -INF, 0.0, 0), 1e9, 5)
    print("dim %d: k = 2 rows of length 0 / 1 / 2: %s; cross-check rows kept %d of %d; radius rows without / with hits %d / %d" %
          (dim, np.bincount(n2, minlength=3), sum(nx), sum(n1), nr.count(0), len(nr) - nr.count(0)))
    assert n2.count(0) and n2.count(1) and n2.count(2)              # nothing allowed, the short row, full rows
    assert 0 < sum(nx) < sum(n1)
    assert nr.count(0) and len(nr) > nr.count(0)
    # rows_cap cutting a frame: 65 and 130 rows are cut, the cross check still searches all of frame a
    for qs, qk, ts, tk, pr in all_forms[2:5]:
        run_knn(B, ctx, qs, qk, ts, tk, pr, GRID_GATE, 2, rows_cap=64)
        run_knn(B, ctx, qs, qk, ts, tk, pr, GRID_GATE, 1, cross=True, rows_cap=64)
        run_radius(B, ctx, qs, qk, ts, tk, pr, GRID_GATE, 4 * dim + 0.5, 8, rows_cap=64)


def sentinel_outputs(npairs, rows_cap, k):
    import torch
    return settled(torch.full((npairs, rows_cap, k, 4), SENTINEL, dtype=torch.int32, device="cuda"),
                   torch.full((npairs, rows_cap), SENTINEL, dtype=torch.int32, device="cuda"),
                   torch.full((npairs,), SENTINEL, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("mode", ["k1", "k2", "cross", "radius"])
def test_nothing_behind_counts_or_beyond_rows_is_written(B, mode):
    import torch
    rng = np.random.default_rng(11)
    ctx = B.default_context(0)
    A, Bs = SynthSet(B, rng, 48, 64, COUNTS_A, CAP), SynthSet(B, rng, 48, 64, COUNTS_B, CAP)
    Ak, Bk = SynthKp(B, rng, COUNTS_A, CAP, nan_every=17), SynthKp(B, rng, COUNTS_B, CAP, slack=12)
    nA, rows_cap = len(COUNTS_A), 64
    per = {"k1": 1, "k2": 2, "cross": 1, "radius": 6}[mode]
    out = sentinel_outputs(nA, rows_cap, per)
    spec, gate = B.PairSpec(nA, 0, 1, 0, 1, None), B.MatchGate(*GRID_GATE)
    torch.cuda.synchronize()
    if mode == "radius":
        ctx.match_radius_pairs(A.set, Bs.set, spec, 4 * 48 + 0.5, per, rows_cap=rows_cap, dim_bytes=48, out=out, gate=gate, query_kps=Ak.set,
                               train_kps=Bk.set)
    else:
        ctx.match_knn_pairs(A.set, Bs.set, spec, per, cross_check=mode == "cross", rows_cap=rows_cap, dim_bytes=48, out=out, gate=gate,
                            query_kps=Ak.set, train_kps=Bk.set)
    torch.cuda.synchronize()
    m, cnt, rows = (t.cpu().numpy() for t in out)
    assert np.array_equal(rows, np.array(COUNTS_A))                 # the TRUE counts, also where rows were cut
    m = m.view(B.DMATCH).reshape(nA, rows_cap, per)
    sent = np.full(4, SENTINEL, np.int32).view(B.DMATCH)[0]
    for p in range(nA):
        M = gate_mask(GRID_GATE, Ak.kps[p], Bk.kps[p])
        if mode == "radius":
            want = oracle_radius(A.desc[p], Bs.desc[p], M, p, 4 * 48 + 0.5)
        else:
            want = oracle_cross(A.desc[p], Bs.desc[p], M, p) if mode == "cross" else oracle_knn(A.desc[p], Bs.desc[p], M, p, per)
        nrows = min(COUNTS_A[p], rows_cap)
        same_cut([m[p, q, :min(cnt[p, q], per)] for q in range(nrows)], cnt[p, :nrows], want[:rows_cap], per)
        for q in range(nrows):                                      # entries behind min(count, entries per row): untouched
            assert all(e == sent for e in m[p, q, min(cnt[p, q], per):])
        assert (cnt[p, nrows:] == SENTINEL).all()                   # rows beyond min(n_a, rows_cap): untouched
        assert (m[p, nrows:].view(np.int32) == SENTINEL).all()


# ---- 3: the radius kernel's dense path under a gate --------------------------------------------------------------------------

def test_dense_path_under_a_gate(B):
    rng = np.random.default_rng(31)
    ctx = B.default_context(0)
    A, Bs = SynthSet(B, rng, 16, 16, COUNTS_A, CAP), SynthSet(B, rng, 16, 24, COUNTS_B, CAP, 2, 2, 1)
    Ak, Bk = SynthKp(B, rng, COUNTS_A, CAP, nan_every=29), SynthKp(B, rng, COUNTS_B, CAP)
    nA = len(COUNTS_A)
    pr = (nA, 0, 1, 1, 0)                                           # all frames of A against the 130 rows of B's frame 1
    for g, cap in (((-24.0, 24.0, -INF, INF, -1), 160), ((-24.0, 24.0, -INF, INF, -1), 5), ((-8.0, 8.0, -8.0, 8.0, 1), 40)):
        nh, ungated = [], []
        run_radius(B, ctx, A, Ak, Bs, Bk, pr, g, 1e9, cap, classes=nh)          # every allowed row hits
        for a in range(nA):
            ungated += [len(w) for w in O.match_radius(A.desc[a], [Bs.desc[1]], 1e9)]
        nh, ungated = np.array(nh), np.array(ungated)
        print("gate %s: rows over the list %d, rows with 1 ... 31 allowed hits and more than 32 ungated ones %d" %
              (g, (nh > LIST).sum(), ((nh > 0) & (nh < LIST) & (ungated > LIST)).sum()))
        if g[4] < 0:
            assert (nh > LIST).sum() >= 1                           # the dense path under a gate
        else:
            assert ((nh > 0) & (nh < LIST) & (ungated > LIST)).sum() >= 1   # the gate keeps a row OFF the dense path
    run_radius(B, ctx, A, Ak, Bs, Bk, pr, (-24.0, 24.0, -INF, INF, -1), 4 * 16 + 0.5, 160)   # dense rows with a real threshold


# ---- 4: an all-pass gate = the ungated call -------------------------------------------------------------------------------------

def test_all_pass_gate_gives_the_ungated_rows(B):
    import torch
    rng = np.random.default_rng(41)
    ctx = B.default_context(0)
    A, Bs = SynthSet(B, rng, 48, 64, COUNTS_A, CAP), SynthSet(B, rng, 48, 52, COUNTS_B, CAP)
    Ak, Bk = SynthKp(B, rng, COUNTS_A, CAP), SynthKp(B, rng, COUNTS_B, CAP)       # (no NaN: NaN records pass no gate at all)
    nA = len(COUNTS_A)
    spec, gate = B.PairSpec(nA, 0, 1, 0, 1, None), B.MatchGate.all_pass()
    torch.cuda.synchronize()
    short = 0
    for k, cross in ((1, False), (2, False), (1, True)):
        plain = ctx.match_knn_pairs(A.set, Bs.set, spec, k, cross_check=cross, rows_cap=CAP, dim_bytes=48, download=True)
        gated = ctx.match_knn_pairs(A.set, Bs.set, spec, k, cross_check=cross, rows_cap=CAP, dim_bytes=48, download=True, gate=gate,
                                    query_kps=Ak.set, train_kps=Bk.set)
        for p in range(nA):
            stripped = [r[r["distance"] != TOP_UP] for r in plain[p]]     # n_b < k: the ungated call's top-up entry is not there
            short += sum(len(s) < len(r) for s, r in zip(stripped, plain[p]))
            same_rows(gated[p], stripped)
    assert short >= 1                                               # COUNTS_B has a frame with one row: k = 2 tops up, the gate does not
    for r, cap in ((4 * 48 + 0.5, 8), (1e9, 140)):
        plain, pc = ctx.match_radius_pairs(A.set, Bs.set, spec, r, cap, rows_cap=CAP, dim_bytes=48, download=True)
        gated, gc = ctx.match_radius_pairs(A.set, Bs.set, spec, r, cap, rows_cap=CAP, dim_bytes=48, download=True, gate=gate,
                                           query_kps=Ak.set, train_kps=Bk.set)
        for p in range(nA):
            assert np.array_equal(pc[p], gc[p])
            same_rows(gated[p], plain[p])


# ---- 5: rows a whole wavefront skips ------------------------------------------------------------------------------------------------

def test_a_gate_that_allows_nothing_and_one_that_allows_one_pair(B):
    import torch
    rng = np.random.default_rng(51)
    ctx = B.default_context(0)
    A, Bs = SynthSet(B, rng, 48, 64, COUNTS_A, CAP), SynthSet(B, rng, 48, 64, COUNTS_B, CAP)
    Ak, Bk = SynthKp(B, rng, COUNTS_A, CAP), SynthKp(B, rng, COUNTS_B, CAP)
    nA = len(COUNTS_A)
    spec = B.PairSpec(nA, 0, 1, 0, 1, None)
    nothing = B.MatchGate(1e6, 2e6, -INF, INF, -1)
    for mode in ("k2", "cross", "radius"):
        per = {"k2": 2, "cross": 1, "radius": 4}[mode]
        out = sentinel_outputs(nA, CAP, per)
        torch.cuda.synchronize()
        if mode == "radius":
            ctx.match_radius_pairs(A.set, Bs.set, spec, 1e9, per, rows_cap=CAP, dim_bytes=48, out=out, gate=nothing, query_kps=Ak.set,
                                   train_kps=Bk.set)
        else:
            ctx.match_knn_pairs(A.set, Bs.set, spec, per, cross_check=mode == "cross", rows_cap=CAP, dim_bytes=48, out=out, gate=nothing,
                                query_kps=Ak.set, train_kps=Bk.set)
        torch.cuda.synchronize()
        m, cnt, rows = (t.cpu().numpy() for t in out)
        assert list(rows) == COUNTS_A                               # still the true counts
        assert (m == SENTINEL).all()
        for p in range(nA):
            assert (cnt[p, :COUNTS_A[p]] == 0).all() and (cnt[p, COUNTS_A[p]:] == SENTINEL).all()
    # exactly one (q, t) of the pair (frame 5 of A, frame 1 of B: 130 x 130 rows) is allowed: only there dx is 1000
    q0, t0 = 77, 101
    Ak.kps[5]["x"][q0], Bk.kps[1]["x"][t0] = 2000.0, 3000.0
    rec = B.KEYPOINT.itemsize
    for K, f, r in ((Ak, 5, q0), (Bk, 1, t0)):
        K.t_buf[f * K.set.frame_pitch + r * rec:f * K.set.frame_pitch + (r + 1) * rec] = torch.from_numpy(K.kps[f][r:r + 1].view(np.uint8).copy()).cuda()
    settled()                                                        # the two records are in place before a call reads them
    one = (1000.0, 1000.0, -INF, INF, -1)
    M = gate_mask(one, Ak.kps[5], Bk.kps[1])
    assert M.sum() == 1 and M[q0, t0] == 1
    pr = [(5, 1)]
    for k, cross in ((1, False), (2, False), (1, True)):
        n = []
        run_knn(B, ctx, A, Ak, Bs, Bk, pr, one, k, cross=cross, classes=n)
        assert sum(n) == 1 and n[q0] == 1
    n = []
    run_radius(B, ctx, A, Ak, Bs, Bk, pr, one, 1e9, 4, classes=n)
    assert sum(n) == 1 and n[q0] == 1


# ---- 6: arguments -------------------------------------------------------------------------------------------------------------------

def test_arguments(B):
    import torch
    rng = np.random.default_rng(3)
    ctx = B.default_context(0)
    A = SynthSet(B, rng, 48, 64, COUNTS_A, CAP, count_stride=1)
    Ak = SynthKp(B, rng, COUNTS_A, CAP)
    nA, cpq = len(COUNTS_A), 2
    out = sentinel_outputs(nA, CAP, cpq)
    torch.cuda.synchronize()
    m, cnt, rows = (t.data_ptr() for t in out)
    L, h = ctx._L, ctx._h
    gate = B.MatchGate(*WINDOW)
    ARG, UNSUPPORTED = 1, 7

    def ref(x):
        return None if x is None else C.byref(x)

    def knn(q=A.set, t=A.set, qk=Ak.set, tk=Ak.set, g=gate, spec=(nA - 1, 1, 1, 0, 1, None), dim=48, k=2, cross=0, cap=CAP, m=m, cnt=cnt,
            rows=rows):
        return L.brisk_hip_match_knn_pairs_gated_device(h, ref(q), ref(t), ref(qk), ref(tk), ref(g), C.byref(B.PairSpec(*spec)), dim, k, cross,
                                                        cap, m, cnt, rows, None)

    def radius(q=A.set, t=A.set, qk=Ak.set, tk=Ak.set, g=gate, spec=(nA - 1, 1, 1, 0, 1, None), dim=48, r=200.0, cpq=cpq, cap=CAP, m=m,
               cnt=cnt, rows=rows):
        return L.brisk_hip_match_radius_pairs_gated_device(h, ref(q), ref(t), ref(qk), ref(tk), ref(g), C.byref(B.PairSpec(*spec)), dim, r,
                                                           cpq, cap, m, cnt, rows, None)

    for call in (knn, radius):
        # the gate's own arguments
        assert call(qk=None) == ARG and call(tk=None) == ARG and call(g=None) == ARG
        assert call(qk=B.KpSet(None, CAP * 28)) == ARG and call(tk=B.KpSet(None, CAP * 28)) == ARG
        assert call(qk=B.KpSet(Ak.set.d_kps + 2, CAP * 28)) == ARG and call(tk=B.KpSet(Ak.set.d_kps, CAP * 28 + 2)) == ARG
        assert call(tk=B.KpSet(Ak.set.d_kps, -28)) == ARG
        # ... and those of the ungated calls
        assert call(dim=40) == UNSUPPORTED and call(dim=96) == UNSUPPORTED
        assert call(spec=(nA, 1, 1, 0, 1, None)) == ARG            # the last pair's query frame is outside the set
        assert call(spec=(nA, 0, 1, -1, 1, None)) == ARG
        assert call(spec=(-1, 0, 1, 0, 1, None)) == ARG
        assert call(cap=0) == ARG
        narrow = B.DescSet(A.set.d_desc, A.set.d_counts, 1, A.set.frame_pitch, 40, nA)
        assert call(q=narrow) == ARG and call(t=narrow) == ARG      # row_pitch < dim_bytes
        assert call(m=None) == ARG and call(cnt=None) == ARG and call(rows=None) == ARG
        assert call(q=None) == ARG and call(t=None) == ARG
        assert call(spec=(0, 0, 1, 0, 1, None)) == 0                # no pairs: fine, nothing to do ...
        assert call(spec=(0, 0, 1, 0, 1, None), qk=None, tk=None, g=None, m=None, cnt=None, rows=None) == 0   # ... and nothing is looked at
    assert knn(k=3) == ARG and knn(k=0) == ARG and knn(k=2, cross=1) == ARG
    assert radius(cpq=0) == ARG and radius(cpq=-1) == ARG
    with pytest.raises(B.BriskHipError) as ei:
        ctx.match_knn_pairs(A.set, A.set, B.PairSpec(2, 0, 1, 0, 1, None), 3, rows_cap=CAP, dim_bytes=48, out=out, gate=gate, query_kps=Ak.set,
                            train_kps=Ak.set)
    assert ei.value.code == ARG
    torch.cuda.synchronize()
    for t in out:                                                   # none of these calls launched anything
        assert (t.cpu().numpy() == SENTINEL).all()
    # a NaN bound is no error: nothing is allowed
    assert knn(g=B.MatchGate(float("nan"), 40.0, -40.0, 40.0, 1), spec=(nA, 0, 1, 0, 1, None)) == 0
    torch.cuda.synchronize()
    hm, hc, hr = (t.cpu().numpy() for t in out)
    assert list(hr) == COUNTS_A and (hm == SENTINEL).all()
    for p in range(nA):
        assert (hc[p, :COUNTS_A[p]] == 0).all() and (hc[p, COUNTS_A[p]:] == SENTINEL).all()

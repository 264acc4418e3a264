"""GPU tests of brisk_hip_match_knn_pairs_device: all frame pairs of a batch matched by one asynchronous call, the row counts
read on the device.  Everything is compared per pair with the CPU oracle's knnMatch (oracle/brisk_oracle_match.c): integer
fields equal, distances equal as bit patterns - there is no tolerance in this feature."""
import ctypes as C

import numpy as np
import pytest

from gpu_prefill import settled
import oracle_lib as O
from test_oracle_golden import homography_outliers

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def B():
    import ethzasl_brisk_amd as B
    from ethzasl_brisk_amd import build
    build.build()
    B.load_library()
    return B


def same_rows(got, want):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert len(g) == len(w), "query %d: %d vs %d matches" % (i, len(g), len(w))
        for f in ("queryIdx", "trainIdx", "imgIdx"):
            assert np.array_equal(g[f], w[f]), (i, f, g, w)
        assert np.array_equal(g["distance"].view(np.uint32), w["distance"].view(np.uint32)), (i, g, w)


def oracle_pair(dq, dt, b, k, rows_cap=None):
    """what pair (a, b) must hold: the oracle's knnMatch of frame a's rows against frame b's as the one train image, with
    imgIdx = the train frame's index in its set"""
    want = O.match_knn(dq, [dt], k)
    for r in want:
        r["imgIdx"] = b
    return want if rows_cap is None else want[:rows_cap]


def oracle_cross(dq, dt, b):
    """k = 1 with the cross check: row q keeps its forward match t exactly when the best match of row t of frame b among the
    rows of frame a is q"""
    fwd = oracle_pair(dq, dt, b, 1)
    back = O.match_knn(dt, [dq], 1)
    out = []
    for q, r in enumerate(fwd):
        keep = len(r) == 1 and back[int(r[0]["trainIdx"])][0]["trainIdx"] == q
        out.append(r if keep else r[:0])
    return out


def pair_list(spec_or_list, n=None):
    if isinstance(spec_or_list, tuple):
        qf, qs, tf, ts = spec_or_list
        return [(qf + p * qs, tf + p * ts) for p in range(n)]
    return list(spec_or_list)


# ---- 1 / 4: the batch's own results, nothing on the host in between ---------------------------------------------------

def batch_frames(golden_ast):
    """img2, img1 (so that the frame-to-previous-frame pair 0 is (img1, img2), the reference's matching test) and seeded
    variants: shifted, darkened, one blank frame (a frame without keypoints inside the batch)"""
    rng = np.random.default_rng(7)
    i1, i2 = golden_ast[0]["image"], golden_ast[1]["image"]
    assert i1.shape == i2.shape

    def shifted(im):
        dy, dx = (int(v) for v in rng.integers(3, 40, 2))
        return np.roll(np.roll(im, dy, axis=0), dx, axis=1)

    def darkened(im):
        return (im.astype(np.float32) * float(rng.uniform(0.55, 0.8))).astype(np.uint8)

    return np.stack([i2, i1, shifted(i1), np.zeros_like(i1), darkened(i2), shifted(i2), darkened(i1), i1, shifted(darkened(i2))])


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
    # detect + describe and the three matching calls back to back on one stream: counts, rows and pitches never visit the host
    ctx.detect_describe_batch(ext, d.data_ptr(), n, w, h, w * h, w, 70, 2, s.cuda_stream)
    st, dim = ctx.batch_desc_set()
    res = {kk: ctx.match_knn_pairs(st, st, spec, kk, stream=s.cuda_stream) for kk in (1, 2)}
    res["cross"] = ctx.match_knn_pairs(st, st, spec, 1, cross_check=True, stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert ctx.batch_status(n) == 0
    host = {key: tuple(t.cpu().numpy() for t in v) for key, v in res.items()}
    kd = [ctx.batch_download(f, True, strings=dim) for f in range(n)]
    out = {"n": n, "dim": dim, "kps": [k for k, _ in kd], "desc": [dd for _, dd in kd], "host": host, "B": B,
           "rows_cap": res[1][0].shape[1]}
    yield out
    ext.close()
    ctx.close()


def rows_of(B, host, k):
    m, cnt, rows = host
    npairs, cap = cnt.shape
    m = m.view(B.DMATCH).reshape(npairs, cap, k)
    return [[m[p, q, :cnt[p, q]] for q in range(min(max(int(rows[p]), 0), cap))] for p in range(npairs)], rows


def test_batch_results_without_the_host(batch):
    B, desc, n = batch["B"], batch["desc"], batch["n"]
    assert batch["dim"] == 48 and n >= 8
    counts = np.array([len(d) for d in desc])
    assert counts[3] == 0 and (np.delete(counts, 3) > 0).all()     # the blank frame is inside the batch
    for k in (1, 2):
        got, rows = rows_of(B, batch["host"][k], k)
        assert np.array_equal(rows, counts[1:])                    # d_pair_rows = the described counts of the query frames
        for p in range(n - 1):
            same_rows(got[p], oracle_pair(desc[p + 1], desc[p], p, k))
    # pair 0 = (img1, img2): the reference's matching test (brisk/src/test/test-match.cc:49-126)
    got, _ = rows_of(B, batch["host"][1], 1)
    best = np.concatenate([r for r in got[0] if len(r) and r[0]["distance"] < 50])
    assert len(best) > 100
    assert homography_outliers(batch["kps"][1], batch["kps"][0], best) == 0


def test_cross_check_on_the_batch(batch):
    B, desc, n = batch["B"], batch["desc"], batch["n"]
    got, rows = rows_of(B, batch["host"]["cross"], 1)
    fwd, _ = rows_of(B, batch["host"][1], 1)
    assert np.array_equal(rows, np.array([len(d) for d in desc])[1:])
    kept = 0
    for p in range(n - 1):
        want = oracle_cross(desc[p + 1], desc[p], p)
        same_rows(got[p], want)
        for g, f in zip(got[p], fwd[p]):                           # survivors carry the forward row unchanged
            assert len(g) == 0 or g.tobytes() == f.tobytes()
        kept += sum(len(g) for g in got[p])
    assert 0 < kept < sum(len(f) for p in fwd for f in p)          # the check both keeps and drops rows here
    best = np.concatenate([r for r in got[0] if len(r) and r[0]["distance"] < 50])
    assert len(best) > 100
    assert homography_outliers(batch["kps"][1], batch["kps"][0], best) == 0


# ---- 2 / 3 / 4 / 5: caller sets in torch device memory --------------------------------------------------------------------

class SynthSet:
    """frames of low-entropy descriptors (plenty of equal distances) in one device buffer: every byte outside the counted
    rows is random too, so a kernel that reads a row it should not read computes something else.  prepared: frame -> its rows
    ([counts[f], dim] uint8) where a test builds them itself instead of taking random ones"""

    def __init__(self, B, rng, dim, row_pitch, counts, cap, base_off=0, count_stride=3, frame_slack=0, prepared=None):
        import torch
        self.counts, self.dim = list(counts), dim
        frames = len(counts)
        frame_pitch = cap * row_pitch + frame_slack
        buf = (rng.integers(0, 4, base_off + frames * frame_pitch + 64, dtype=np.uint8) * 85).astype(np.uint8)
        self.desc = []
        for f, c in enumerate(counts):
            if prepared is not None and f in prepared:
                rows = np.ascontiguousarray(prepared[f], np.uint8)
                assert rows.shape == (c, dim)
            else:
                rows = (rng.integers(0, 4, (c, dim), dtype=np.uint8) * 85).astype(np.uint8)
                if f > 0 and c > 4 and len(self.desc[0]) > 4:
                    rows[:3] = self.desc[0][:3]                     # the same descriptors in several frames: distance 0
            o = base_off + f * frame_pitch
            np.lib.stride_tricks.as_strided(buf[o:], (c, dim), (row_pitch, 1))[...] = rows
            self.desc.append(rows)
        cnt = rng.integers(100, 1000, frames * count_stride + 1).astype(np.int32)
        cnt[0:frames * count_stride:count_stride] = counts
        self.t_buf, self.t_cnt = torch.from_numpy(buf).cuda(), torch.from_numpy(cnt).cuda()
        self.set = B.DescSet(self.t_buf.data_ptr() + base_off, self.t_cnt.data_ptr(), count_stride, frame_pitch, row_pitch, frames)


CAP = 130
COUNTS_A = [65, 0, 1, 63, 64, CAP, 1, 7]
COUNTS_B = [64, CAP, 0, 1, 65, 63, 2, 0]


def run_pairs(B, ctx, qs, ts, pairs, k, cross=False, rows_cap=CAP):
    import torch
    if isinstance(pairs, tuple):
        n, spec, keep = pairs[0], B.PairSpec(pairs[0], *pairs[1:], None), None
        plist = pair_list(pairs[1:], n)
    else:
        keep = torch.from_numpy(np.array(pairs, np.int32).reshape(-1, 2)).cuda()
        spec, plist = B.PairSpec(len(pairs), 0, 0, 0, 0, keep.data_ptr()), list(pairs)
    torch.cuda.synchronize()
    got = ctx.match_knn_pairs(qs.set, ts.set, spec, k, cross_check=cross, rows_cap=rows_cap, dim_bytes=qs.dim, download=True)
    assert len(got) == len(plist)
    for (a, b), g in zip(plist, got):
        want = oracle_cross(qs.desc[a], ts.desc[b], b) if cross else oracle_pair(qs.desc[a], ts.desc[b], b, k)
        same_rows(g, want[:rows_cap])


@pytest.mark.parametrize("dim,pitch,base_off,slack", [(16, 16, 0, 0), (16, 20, 0, 0), (32, 32, 0, 0), (32, 48, 0, 4), (48, 48, 0, 0),
                                                      (48, 64, 0, 0), (48, 51, 1, 3), (64, 64, 0, 0), (64, 80, 0, 0)])
def test_caller_sets_and_pair_forms(B, dim, pitch, base_off, slack):
    rng = np.random.default_rng(dim * 1000 + pitch)
    ctx = B.default_context(0)
    A = SynthSet(B, rng, dim, pitch, COUNTS_A, CAP, base_off, 3, slack)
    Bs = SynthSet(B, rng, dim, pitch + 4 * (dim == 48), COUNTS_B, CAP, 0, 1, 0)
    nA = len(COUNTS_A)
    shuffled = [(int(a), int(b)) for a, b in zip(rng.integers(0, nA, 9), rng.integers(0, nA, 9))]
    shuffled.insert(4, shuffled[1])                                 # a repeated pair
    for k in (1, 2):
        run_pairs(B, ctx, A, A, (nA - 1, 1, 1, 0, 1), k)            # frame to previous frame
        run_pairs(B, ctx, A, A, (nA // 2, 0, 2, 1, 2), k)           # interleaved stereo
        run_pairs(B, ctx, A, Bs, (nA, 0, 1, 0, 1), k)               # two sets side by side
        run_pairs(B, ctx, A, Bs, (nA, 0, 1, 3, 0), k)               # all against a keyframe with ONE row (k = 2: the top-up)
        run_pairs(B, ctx, Bs, A, (nA, 0, 1, 5, 0), k)               # ... and against the full frame
        run_pairs(B, ctx, A, Bs, shuffled, k)


def test_cross_check_with_heavy_ties(B):
    rng = np.random.default_rng(99)
    ctx = B.default_context(0)
    A = SynthSet(B, rng, 16, 16, COUNTS_A, CAP)                     # 16 bytes of 4 values each: ties everywhere
    Bs = SynthSet(B, rng, 16, 24, COUNTS_B, CAP, 2, 2, 1)
    nA = len(COUNTS_A)
    run_pairs(B, ctx, A, A, (nA - 1, 1, 1, 0, 1), 1, cross=True)
    run_pairs(B, ctx, A, Bs, (nA, 0, 1, 0, 1), 1, cross=True)
    run_pairs(B, ctx, Bs, A, [(1, 5), (5, 1), (4, 0), (1, 5), (6, 6)], 1, cross=True)
    run_pairs(B, ctx, Bs, A, (nA, 0, 1, 5, 0), 1, cross=True, rows_cap=64)   # the backward search covers rows beyond the cap
    D = SynthSet(B, rng, 48, 64, COUNTS_A, CAP)
    run_pairs(B, ctx, D, D, (nA - 1, 1, 1, 0, 1), 1, cross=True)


def sentinel_outputs(npairs, rows_cap, k):
    import torch
    return settled(torch.full((npairs, rows_cap, k, 4), SENTINEL, dtype=torch.int32, device="cuda"),
                   torch.full((npairs, rows_cap), SENTINEL, dtype=torch.int32, device="cuda"),
                   torch.full((npairs,), SENTINEL, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("k,cross", [(1, False), (2, False), (1, True)])
def test_cut_rows_leave_the_rest_untouched(B, k, cross):
    import torch
    rng = np.random.default_rng(5 + k)
    ctx = B.default_context(0)
    A = SynthSet(B, rng, 48, 64, COUNTS_A, CAP)
    Bs = SynthSet(B, rng, 48, 64, COUNTS_B, CAP)
    nA, cap = len(COUNTS_A), 64                                     # 65 and 130 rows are cut, 64 and 63 are not
    out = sentinel_outputs(nA, cap, k)
    torch.cuda.synchronize()
    ctx.match_knn_pairs(A.set, Bs.set, B.PairSpec(nA, 0, 1, 0, 1, None), k, cross_check=cross, rows_cap=cap, dim_bytes=48, out=out)
    torch.cuda.synchronize()
    m, cnt, rows = (t.cpu().numpy() for t in out)
    assert np.array_equal(rows, np.array(COUNTS_A))                 # the TRUE counts, also where rows were cut
    m = m.view(B.DMATCH).reshape(nA, cap, k)
    sent = np.full(4, SENTINEL, np.int32).view(B.DMATCH)[0]
    for p in range(nA):
        want = oracle_cross(A.desc[p], Bs.desc[p], p) if cross else oracle_pair(A.desc[p], Bs.desc[p], p, k)
        nrows = min(COUNTS_A[p], cap)
        same_rows([m[p, q, :cnt[p, q]] for q in range(nrows)], want[:cap])
        for q in range(nrows):                                      # entries behind a row's count: untouched
            assert all(e == sent for e in m[p, q, cnt[p, q]:])
        assert (cnt[p, nrows:] == SENTINEL).all()                   # rows beyond min(n_a, rows_cap): untouched
        assert (m[p, nrows:].view(np.int32) == SENTINEL).all()


def test_arguments(B):
    import torch
    rng = np.random.default_rng(3)
    ctx = B.default_context(0)
    A = SynthSet(B, rng, 48, 64, COUNTS_A, CAP, count_stride=1)
    nA = len(COUNTS_A)
    out = sentinel_outputs(nA, CAP, 2)
    torch.cuda.synchronize()
    m, cnt, rows = (t.data_ptr() for t in out)
    L, h = ctx._L, ctx._h

    def call(q=A.set, t=A.set, spec=(nA - 1, 1, 1, 0, 1, None), dim=48, k=2, cross=0, cap=CAP, m=m, cnt=cnt, rows=rows):
        return L.brisk_hip_match_knn_pairs_device(h, C.byref(q), C.byref(t), C.byref(B.PairSpec(*spec)), dim, k, cross, cap, m, cnt, rows, None)

    ARG, UNSUPPORTED = 1, 7
    assert call(k=3) == ARG
    assert call(k=0) == ARG
    assert call(k=2, cross=1) == ARG
    assert call(dim=40) == UNSUPPORTED
    assert call(dim=96) == UNSUPPORTED
    assert call(spec=(nA, 1, 1, 0, 1, None)) == ARG                # the last pair's query frame is outside the set
    assert call(spec=(nA, 0, 1, -1, 1, None)) == ARG               # the first pair's train frame is
    assert call(spec=(3, 0, 1, 0, nA, None)) == ARG
    assert call(spec=(-1, 0, 1, 0, 1, None)) == ARG
    narrow = B.DescSet(A.set.d_desc, A.set.d_counts, 1, A.set.frame_pitch, 40, nA)
    assert call(q=narrow) == ARG and call(t=narrow) == ARG          # row_pitch < dim_bytes
    assert call(m=None) == ARG and call(cnt=None) == ARG and call(rows=None) == ARG
    assert call(cap=0) == ARG
    assert L.brisk_hip_match_knn_pairs_device(h, None, C.byref(A.set), C.byref(B.PairSpec(1, 0, 1, 0, 1, None)), 48, 1, 0, CAP, m, cnt,
                                              rows, None) == ARG
    with pytest.raises(B.BriskHipError) as ei:
        ctx.match_knn_pairs(A.set, A.set, B.PairSpec(2, 0, 1, 0, 1, None), 3, rows_cap=CAP, dim_bytes=48, out=out)
    assert ei.value.code == ARG
    assert call(spec=(0, 0, 1, 0, 1, None)) == 0                    # no pairs: fine, nothing to do
    assert call(spec=(0, 50, 1, 50, 1, None), m=None, cnt=None, rows=None) == 0
    torch.cuda.synchronize()
    for t in out:                                                   # none of these calls launched anything
        assert (t.cpu().numpy() == SENTINEL).all()
    # a list on the device is checked there: a bad entry gives -1 rows for that pair only
    plist = [(0, 4), (nA, 0), (3, 5), (2, -1), (5, 0)]
    d_pairs = torch.from_numpy(np.array(plist, np.int32)).cuda()
    torch.cuda.synchronize()
    assert call(spec=(len(plist), 0, 0, 0, 0, d_pairs.data_ptr())) == 0
    torch.cuda.synchronize()
    hm, hc, hr = (t.cpu().numpy() for t in out)
    assert list(hr[:len(plist)]) == [COUNTS_A[0], -1, COUNTS_A[3], -1, COUNTS_A[5]] and (hr[len(plist):] == SENTINEL).all()
    hm = hm.view(B.DMATCH).reshape(nA, CAP, 2)
    for p, (a, b) in enumerate(plist):
        if hr[p] < 0:
            assert (hc[p] == SENTINEL).all() and (hm[p].view(np.int32) == SENTINEL).all()
        else:
            same_rows([hm[p, q, :hc[p, q]] for q in range(COUNTS_A[a])], oracle_pair(A.desc[a], A.desc[b], b, 2))
    assert (hc[len(plist):] == SENTINEL).all()

"""GPU tests of brisk_hip_match_radius_pairs_device / brisk_hip_match_radius_device: the radius matches of all frame pairs of a
batch by one asynchronous call, the row counts read on the device.  Everything is compared per pair with the CPU oracle's
radiusMatch (oracle/brisk_oracle_match.c) - rows cut to cap_per_query, the count compared with the oracle's full length:
integer fields equal, distances equal as bit patterns, counts equal - there is no tolerance in this feature."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from gpu_prefill import settled
import oracle_lib as O
from test_gpu_match_pairs import CAP, COUNTS_A, COUNTS_B, SENTINEL, SynthSet, batch_frames, pair_list, same_rows
from test_oracle_golden import homography_outliers

pytestmark = pytest.mark.gpu

LIST = 32   # keys per query the kernel holds in LDS (MRP_LIST); rows with more hits take its dense path


@pytest.fixture(scope="module")
def B():
    import ethzasl_brisk_amd as B
    from ethzasl_brisk_amd import build
    build.build()
    B.load_library()
    return B


def oracle_pair(dq, dt, b, max_distance):
    """what pair (a, b) must hold, uncut: the oracle's radiusMatch of frame a's rows against frame b's as the one train image,
    with imgIdx = the train frame's index in its set"""
    want = O.match_radius(dq, [dt], max_distance)
    for r in want:
        r["imgIdx"] = b
    return want


def same_cut(got_rows, got_counts, want, cap):
    """stored rows = the oracle's cut to cap, counts = the oracle's full lengths"""
    assert len(got_rows) == len(want) == len(got_counts)
    assert [int(c) for c in got_counts] == [len(w) for w in want]
    same_rows(got_rows, [w[:cap] for w in want])


# ---- 1: the batch's own results, nothing on the host in between -------------------------------------------------------------

BATCH_CAP = 8


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
    # detect + describe and the matching calls back to back on one stream: counts, rows and pitches never visit the host
    ctx.detect_describe_batch(ext, d.data_ptr(), n, w, h, w * h, w, 70, 2, s.cuda_stream)
    st, dim = ctx.batch_desc_set()
    res = {r: ctx.match_radius_pairs(st, st, spec, r, BATCH_CAP, stream=s.cuda_stream) for r in (50.0, 90.0)}
    torch.cuda.synchronize()
    assert ctx.batch_status(n) == 0
    host = {key: tuple(t.cpu().numpy() for t in v) for key, v in res.items()}
    kd = [ctx.batch_download(f, True, strings=dim) for f in range(n)]
    out = {"n": n, "dim": dim, "kps": [k for k, _ in kd], "desc": [dd for _, dd in kd], "host": host, "B": B}
    yield out
    ext.close()
    ctx.close()


def rows_of(B, host, cap):
    m, cnt, rows = host
    npairs, rows_cap = cnt.shape
    m = m.view(B.DMATCH).reshape(npairs, rows_cap, cap)
    nrows = [min(max(int(rows[p]), 0), rows_cap) for p in range(npairs)]
    return ([[m[p, q, :min(cnt[p, q], cap)] for q in range(nrows[p])] for p in range(npairs)],
            [cnt[p, :nrows[p]] for p in range(npairs)], rows)


@pytest.mark.parametrize("max_distance", [50.0, 90.0])
def test_batch_results_without_the_host(batch, max_distance):
    B, desc, n = batch["B"], batch["desc"], batch["n"]
    assert batch["dim"] == 48 and n >= 8
    counts = np.array([len(d) for d in desc])
    assert counts[3] == 0 and (np.delete(counts, 3) > 0).all()     # the blank frame is inside the batch
    got, cnt, rows = rows_of(B, batch["host"][max_distance], BATCH_CAP)
    assert np.array_equal(rows, counts[1:])                        # d_pair_rows = the described counts of the query frames
    hits = 0
    for p in range(n - 1):
        want = oracle_pair(desc[p + 1], desc[p], p, max_distance)
        same_cut(got[p], cnt[p], want, BATCH_CAP)
        hits += sum(len(w) for w in want)
    print("radius %g: %d hits in %d rows" % (max_distance, hits, int(counts[1:].sum())))
    assert hits > 0
    if max_distance == 50.0:
        # pair 0 = (img1, img2): the reference's matching test (brisk/src/test/test-match.cc:49-126) on the radius hits
        inside = np.concatenate(got[0])
        print("pair 0 at 50: %d hits into the homography check" % len(inside))
        assert len(inside) >= 100
        assert homography_outliers(batch["kps"][1], batch["kps"][0], inside) == 0


# ---- 2: caller sets in torch device memory, every pair form --------------------------------------------------------------

def run_pairs(B, ctx, qs, ts, pairs, max_distance, cap, rows_cap=CAP, classes=None):
    import torch
    if isinstance(pairs, tuple):
        n, spec, keep = pairs[0], B.PairSpec(pairs[0], *pairs[1:], None), None
        plist = pair_list(pairs[1:], n)
    else:
        keep = torch.from_numpy(np.array(pairs, np.int32).reshape(-1, 2)).cuda()
        spec, plist = B.PairSpec(len(pairs), 0, 0, 0, 0, keep.data_ptr()), list(pairs)
    torch.cuda.synchronize()
    got, counts = ctx.match_radius_pairs(qs.set, ts.set, spec, max_distance, cap, rows_cap=rows_cap, dim_bytes=qs.dim, download=True)
    assert len(got) == len(plist) == len(counts)
    for (a, b), g, c in zip(plist, got, counts):
        want = oracle_pair(qs.desc[a], ts.desc[b], b, max_distance)
        same_cut(g, c, want[:rows_cap], cap)
        if classes is not None:
            classes += [len(w) for w in want[:rows_cap]]


PITCHES = [(16, 16, 0, 0), (16, 20, 0, 0), (32, 32, 0, 0), (32, 48, 0, 4), (48, 48, 0, 0), (48, 64, 0, 0), (48, 51, 1, 3), (64, 64, 0, 0),
           (64, 80, 0, 0)]


def forms(A, Bs, nA, shuffled):
    return [(A, A, (nA - 1, 1, 1, 0, 1)),            # frame to previous frame
            (A, A, (nA // 2, 0, 2, 1, 2)),           # interleaved stereo
            (A, Bs, (nA, 0, 1, 0, 1)),               # two sets side by side
            (A, Bs, (nA, 0, 1, 3, 0)),               # all against a keyframe with ONE row
            (Bs, A, (nA, 0, 1, 5, 0)),               # ... and against the full frame (130 rows)
            (A, Bs, shuffled)]                       # a shuffled device list with a repeat


@pytest.mark.parametrize("dim,pitch,base_off,slack", PITCHES)
def test_caller_sets_and_pair_forms(B, dim, pitch, base_off, slack):
    rng = np.random.default_rng(dim * 1000 + pitch)
    ctx = B.default_context(0)
    A = SynthSet(B, rng, dim, pitch, COUNTS_A, CAP, base_off, 3, slack)
    Bs = SynthSet(B, rng, dim, pitch + 4 * (dim == 48), COUNTS_B, CAP, 0, 1, 0)
    nA = len(COUNTS_A)
    shuffled = [(int(a), int(b)) for a, b in zip(rng.integers(0, nA, 9), rng.integers(0, nA, 9))]
    shuffled.insert(4, shuffled[1])                                 # a repeated pair
    all_forms = forms(A, Bs, nA, shuffled)
    # only the planted identical rows (distance 0) hit
    n0 = []
    for qs, ts, pr in all_forms:
        run_pairs(B, ctx, qs, ts, pr, 0.5, 8, classes=n0)
    assert 0 < sum(n0) and max(n0) <= 3 and n0.count(0) > 0
    # the centre of the distances: rows without a hit, rows inside the cap, rows over the cap, rows over the kernel's list
    mid = 4 * dim + 0.5
    for i, (qs, ts, pr) in enumerate(all_forms):
        nh = []
        run_pairs(B, ctx, qs, ts, pr, mid, 8, classes=nh)
        if i == 2:                                                  # side by side: every class is there
            nh = np.array(nh)
            print("dim %d at %g: %d rows without a hit, %d with 1-8, %d with more (max %d), %d beyond the list" %
                  (dim, mid, (nh == 0).sum(), ((nh > 0) & (nh <= 8)).sum(), (nh > 8).sum(), nh.max(), (nh > LIST).sum()))
            assert (nh == 0).any() and ((nh >= 1) & (nh <= 8)).any() and ((nh > 8) & (nh <= LIST)).any() and (nh > LIST).any()
    # everything hits: up to 130 per row, the cap below and above that
    for cap in (5, 160):
        for i, (qs, ts, pr) in enumerate(all_forms):
            nh = []
            run_pairs(B, ctx, qs, ts, pr, 1e9, cap, classes=nh)
            if i == 4:
                assert max(nh) == CAP and min(nh) == CAP            # every row of every frame hits all 130 rows of the keyframe
    # strictness: a threshold that IS a distance of the set is excluded
    probe = oracle_pair(A.desc[0], Bs.desc[0], 0, 4 * dim + 1)
    occurring = sorted({int(m["distance"]) for r in probe for m in r})
    edge = float(occurring[-1])
    want = oracle_pair(A.desc[0], Bs.desc[0], 0, edge)
    assert all(m["distance"] < edge for r in want for m in r)       # the oracle excludes it ...
    assert sum(len(r) for r in want) < sum(len(r) for r in probe)
    for qs, ts, pr in all_forms:
        run_pairs(B, ctx, qs, ts, pr, edge, 8)                      # ... and so must the kernel


# ---- 3: cut rows and untouched memory --------------------------------------------------------------------------------------

def sentinel_outputs(npairs, rows_cap, cap):
    import torch
    return settled(torch.full((npairs, rows_cap, cap, 4), SENTINEL, dtype=torch.int32, device="cuda"),
                   torch.full((npairs, rows_cap), SENTINEL, dtype=torch.int32, device="cuda"),
                   torch.full((npairs,), SENTINEL, dtype=torch.int32, device="cuda"))


@pytest.mark.parametrize("max_distance,cap", [(0.5, 4), (4 * 48 + 0.5, 8), (1e9, 40), (1e9, 140)])
def test_cut_rows_leave_the_rest_untouched(B, max_distance, cap):
    import torch
    rng = np.random.default_rng(5 + cap)
    ctx = B.default_context(0)
    A = SynthSet(B, rng, 48, 64, COUNTS_A, CAP)
    Bs = SynthSet(B, rng, 48, 64, COUNTS_B, CAP)
    nA, rows_cap = len(COUNTS_A), 64                                # 65 and 130 rows are cut, 64 and 63 are not
    out = sentinel_outputs(nA, rows_cap, cap)
    torch.cuda.synchronize()
    ctx.match_radius_pairs(A.set, Bs.set, B.PairSpec(nA, 0, 1, 0, 1, None), max_distance, cap, rows_cap=rows_cap, dim_bytes=48, out=out)
    torch.cuda.synchronize()
    m, cnt, rows = (t.cpu().numpy() for t in out)
    assert np.array_equal(rows, np.array(COUNTS_A))                 # the TRUE counts, also where rows were cut
    m = m.view(B.DMATCH).reshape(nA, rows_cap, cap)
    sent = np.full(4, SENTINEL, np.int32).view(B.DMATCH)[0]
    for p in range(nA):
        want = oracle_pair(A.desc[p], Bs.desc[p], p, max_distance)[:rows_cap]
        nrows = min(COUNTS_A[p], rows_cap)
        same_cut([m[p, q, :min(cnt[p, q], cap)] for q in range(nrows)], cnt[p, :nrows], want, cap)
        for q in range(nrows):                                      # entries behind min(count, cap): untouched
            assert all(e == sent for e in m[p, q, min(cnt[p, q], cap):])
        assert (cnt[p, nrows:] == SENTINEL).all()                   # rows beyond min(n_a, rows_cap): untouched
        assert (m[p, nrows:].view(np.int32) == SENTINEL).all()


# ---- 4: arguments ----------------------------------------------------------------------------------------------------------

def test_arguments(B):
    import torch
    rng = np.random.default_rng(3)
    ctx = B.default_context(0)
    A = SynthSet(B, rng, 48, 64, COUNTS_A, CAP, count_stride=1)
    nA, cpq = len(COUNTS_A), 8
    out = sentinel_outputs(nA, CAP, cpq)
    torch.cuda.synchronize()
    m, cnt, rows = (t.data_ptr() for t in out)
    L, h = ctx._L, ctx._h
    fn = L.brisk_hip_match_radius_pairs_device

    def call(q=A.set, t=A.set, spec=(nA - 1, 1, 1, 0, 1, None), dim=48, r=200.0, cpq=cpq, cap=CAP, m=m, cnt=cnt, rows=rows):
        return fn(h, C.byref(q), C.byref(t), C.byref(B.PairSpec(*spec)), dim, r, cpq, cap, m, cnt, rows, None)

    ARG, UNSUPPORTED = 1, 7
    assert call(dim=40) == UNSUPPORTED
    assert call(dim=80) == UNSUPPORTED
    assert call(dim=96) == UNSUPPORTED
    assert call(spec=(nA, 1, 1, 0, 1, None)) == ARG                # the last pair's query frame is outside the set
    assert call(spec=(nA, 0, 1, -1, 1, None)) == ARG               # the first pair's train frame is
    assert call(spec=(3, 0, 1, 0, nA, None)) == ARG
    assert call(spec=(-1, 0, 1, 0, 1, None)) == ARG                # npairs < 0
    assert call(cap=0) == ARG and call(cap=-5) == ARG              # rows_cap < 1
    assert call(cpq=0) == ARG and call(cpq=-1) == ARG              # cap_per_query < 1
    narrow = B.DescSet(A.set.d_desc, A.set.d_counts, 1, A.set.frame_pitch, 40, nA)
    assert call(q=narrow) == ARG and call(t=narrow) == ARG          # row_pitch < dim_bytes
    assert call(m=None) == ARG and call(cnt=None) == ARG and call(rows=None) == ARG
    one = C.byref(B.PairSpec(1, 0, 1, 0, 1, None))
    assert fn(h, None, C.byref(A.set), one, 48, 200.0, cpq, CAP, m, cnt, rows, None) == ARG
    assert fn(h, C.byref(A.set), None, one, 48, 200.0, cpq, CAP, m, cnt, rows, None) == ARG
    with pytest.raises(B.BriskHipError) as ei:
        ctx.match_radius_pairs(A.set, A.set, B.PairSpec(2, 0, 1, 0, 1, None), 200.0, 0, rows_cap=CAP, dim_bytes=48, out=out)
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
    hm = hm.view(B.DMATCH).reshape(nA, CAP, cpq)
    for p, (a, b) in enumerate(plist):
        if hr[p] < 0:
            assert (hc[p] == SENTINEL).all() and (hm[p].view(np.int32) == SENTINEL).all()
        else:
            na = COUNTS_A[a]
            same_cut([hm[p, q, :min(hc[p, q], cpq)] for q in range(na)], hc[p, :na], oracle_pair(A.desc[a], A.desc[b], b, 200.0), cpq)
    assert (hc[len(plist):] == SENTINEL).all()
    # nothing can be closer than 0, a negative threshold or NaN: counts 0, entries untouched, not an error
    for r in (0.0, -3.0, float("nan")):
        out2 = sentinel_outputs(nA, CAP, cpq)
        torch.cuda.synchronize()
        m2, c2, r2 = (t.data_ptr() for t in out2)
        assert call(spec=(nA, 0, 1, 0, 1, None), r=r, m=m2, cnt=c2, rows=r2) == 0
        torch.cuda.synchronize()
        hm, hc, hr = (t.cpu().numpy() for t in out2)
        assert list(hr) == COUNTS_A and (hm == SENTINEL).all()
        for p in range(nA):
            assert (hc[p, :COUNTS_A[p]] == 0).all() and (hc[p, COUNTS_A[p]:] == SENTINEL).all()


# ---- 5: the single-set device form ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,pitch", [(16, 16), (48, 52), (64, 64), (80, 96)])     # 80 bytes: the distance-matrix path
def test_single_set_device_form(B, dim, pitch):
    import torch
    rng = np.random.default_rng(dim)
    ctx = B.default_context(0)
    cpq = 8

    def rows(n):
        buf = (rng.integers(0, 4, (max(n, 1), pitch), dtype=np.uint8) * 85).astype(np.uint8)
        return buf, buf[:n, :dim].copy()

    for nq, nt in ((150, 97), (64, 130), (1, 1), (70, 0)):         # nq not a multiple of 64, nt == 0
        qb, q = rows(nq)
        tb, t = rows(nt)
        if nt > 3:
            tb[2, :dim] = qb[1, :dim]
            t[2] = q[1]                                             # a planted identical row
        dq, dt = torch.from_numpy(qb).cuda(), torch.from_numpy(tb).cuda()
        for r in (0.5, 4 * dim + 0.5, float(4 * dim), 1e9):
            m, c = settled(torch.full((nq, cpq, 4), SENTINEL, dtype=torch.int32, device="cuda"),
                           torch.full((nq,), SENTINEL, dtype=torch.int32, device="cuda"))
            ctx.match_radius_device(dq.data_ptr(), nq, pitch, dt.data_ptr() if nt else None, nt, pitch, dim, r, cpq, m.data_ptr(),
                                    c.data_ptr())
            torch.cuda.synchronize()
            hm, hc = m.cpu().numpy().view(B.DMATCH).reshape(nq, cpq), c.cpu().numpy()
            want = O.match_radius(q, [t], r)
            same_cut([hm[i, :min(hc[i], cpq)] for i in range(nq)], hc, want, cpq)
            sent = np.full(4, SENTINEL, np.int32).view(B.DMATCH)[0]
            for i in range(nq):
                assert all(e == sent for e in hm[i, min(hc[i], cpq):])
    L, h = ctx._L, ctx._h
    assert L.brisk_hip_match_radius_device(h, dq.data_ptr(), 4, pitch, dt.data_ptr(), 0, pitch, dim, 10.0, 0, m.data_ptr(), c.data_ptr(), None) == 1
    assert L.brisk_hip_match_radius_device(h, dq.data_ptr(), 4, dim - 1, dt.data_ptr(), 0, pitch, dim, 10.0, 4, m.data_ptr(), c.data_ptr(), None) == 1
    assert L.brisk_hip_match_radius_device(h, dq.data_ptr(), 4, 240, dt.data_ptr(), 0, 240, 240, 10.0, 4, m.data_ptr(), c.data_ptr(), None) == 7


# ---- 6: agreement with the host call ----------------------------------------------------------------------------------------

def test_agreement_with_the_host_call(B):
    rng = np.random.default_rng(17)
    ctx = B.default_context(0)
    A = SynthSet(B, rng, 48, 64, COUNTS_A, CAP)
    Bs = SynthSet(B, rng, 48, 64, COUNTS_B, CAP)
    import torch
    torch.cuda.synchronize()
    for r, cap in ((4 * 48 + 0.5, 64), (1e9, CAP)):                 # (the first cuts some rows, the second none)
        got, counts = ctx.match_radius_pairs(A.set, Bs.set, B.PairSpec(1, 5, 1, 1, 1, None), r, cap, rows_cap=CAP, dim_bytes=48,
                                             download=True)
        matcher = B.BruteForceMatcher(ctx)
        matcher.add(Bs.desc[1])
        host = matcher.radiusMatch(A.desc[5], r)                    # brisk_hip_match_radius on host copies of the rows
        for row in host:
            row["imgIdx"] = 1
        same_cut(got[0], counts[0], host, cap)


def test_two_set_radius_match_of_the_cpp_class():
    from test_abi_match_radius_pairs import build_program
    r = subprocess.run([build_program()], capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "two-set radiusMatch OK" in r.stdout

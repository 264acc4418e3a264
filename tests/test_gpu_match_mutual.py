"""GPU tests of brisk_hip_match_mutual_pairs_guided_device / brisk_hip_match_mutual_pairs_epipolar_guided_device: the two guided k-NN
calls for k = 1 with the cross check.  Integers in, integers out: every comparison is of bytes.  The inputs are the cases of
tests/test_abi_match_mutual.py, where the rule is restated in NumPy, checked against the header functions on the host, and every case
is shown to hold every class of row."""
import ctypes as C

import numpy as np
import pytest

from test_abi_match_guided import PAIR_BAD, PAIR_NO_MODEL
from test_abi_match_mutual import (CENTRE, DIMS, EQUAL_CASES, GENERAL_CASES, LINE, MEMORY_CASES, ROWS_CAP, Pair, equal_case, general_case,
                                   mutual_under_mask, restated_mutual)
from test_gpu_match_epiline import epi_mask
from test_gpu_match_gated import knn_rows, sentinel_outputs
from test_gpu_match_guided import Kp, guide_mask, upload_models
from test_gpu_match_pairs import SENTINEL, SynthSet, batch_frames
from test_gpu_stream_order import begin, env, race, run_batch, sptr  # noqa: F401 (env: the fixture of the held stream)

pytestmark = pytest.mark.gpu

LAYOUT = {16: (20, 0, 0), 32: (48, 0, 4), 48: (51, 1, 3), 64: (64, 0, 0)}     # dim -> row pitch, base offset, frame slack
ARG, UNSUPPORTED = 1, 7


@pytest.fixture(scope="module")
def B():
    import ethzasl_brisk_amd as B
    from ethzasl_brisk_amd import build
    build.build()
    B.load_library()
    return B


class Frames:
    """a case on the device: pair p's query rows are frame p of A, its train rows frame p of Bs"""

    def __init__(self, B, case, pitch, base_off, slack):
        rng = np.random.default_rng(1)
        na, nb = [len(p.kq) for p in case.pairs], [len(p.kt) for p in case.pairs]
        cap = max(na + nb + [1])
        self.A = SynthSet(B, rng, case.dim, pitch, na, cap, base_off, 3, slack, prepared={f: p.dq for f, p in enumerate(case.pairs)})
        self.Bs = SynthSet(B, rng, case.dim, pitch + 4 * (case.dim == 48), nb, cap, 0, 1, 0, prepared={f: p.dt for f, p in enumerate(case.pairs)})
        self.Ak, self.Bk = Kp(B, [p.kq for p in case.pairs], cap), Kp(B, [p.kt for p in case.pairs], cap)
        self.models = upload_models(case.records())


def guide_of(B, case):
    gate = B.MatchGate(*case.window)
    return B.MatchEpipolarGuide(gate, case.band, case.fallback) if case.form == LINE else B.MatchGuide(gate, case.fallback)


def mutual(ctx, case):
    return ctx.match_mutual_pairs_epipolar_guided if case.form == LINE else ctx.match_mutual_pairs_guided


def pair_spec(B, pairs):
    """(PairSpec, the tensor that keeps a device list alive)"""
    import torch
    if isinstance(pairs, tuple):
        return B.PairSpec(pairs[0], *pairs[1:], None), None
    keep = torch.from_numpy(np.array(pairs, np.int32).reshape(-1, 2)).cuda()
    return B.PairSpec(len(pairs), 0, 0, 0, 0, keep.data_ptr()), keep


def compare(B, out, want, rows_cap):
    """the three poison-filled outputs against the restatement.  want[p]: None for a bad pair, else (n_a, b, f, distance, kept).  A kept
    row holds its record and count 1, a dropped row count 0; nothing else is written.  Returns the records kept."""
    m, cnt, rows = (t.cpu().numpy() for t in out)
    exp_m = np.full(m.shape, SENTINEL, np.int32).view(B.DMATCH).reshape(len(want), rows_cap)
    exp_c, exp_r = np.full(cnt.shape, SENTINEL, np.int32), np.full(rows.shape, SENTINEL, np.int32)
    for p, w in enumerate(want):
        if w is None:
            exp_r[p] = -1
            continue
        na, b, ft, fd, kept = w
        exp_r[p] = na
        exp_c[p, :len(kept)] = kept
        for q in np.flatnonzero(kept):
            exp_m[p, q] = (q, ft[q], b, np.float32(fd[q]))
    assert rows.tobytes() == exp_r.tobytes(), (rows, exp_r)
    bad = np.argwhere(cnt != exp_c)
    assert len(bad) == 0, (len(bad), bad[:5], cnt[tuple(bad[0])], exp_c[tuple(bad[0])])
    got_m = m.view(B.DMATCH).reshape(len(want), rows_cap)
    bad = np.argwhere(got_m != exp_m)
    assert len(bad) == 0, (len(bad), bad[:5], got_m[tuple(bad[0])], exp_m[tuple(bad[0])])
    assert m.tobytes() == exp_m.tobytes()
    return int((exp_c == 1).sum())


# ---- 1: identity models, the fallback, band = +inf: the gated matcher's cross check ---------------------------------------------------

@pytest.mark.parametrize("form", [CENTRE, LINE])
@pytest.mark.parametrize("dim,pitch,base_off,slack", DIMS)
def test_equal_to_the_gated_cross_check(B, dim, pitch, base_off, slack, form):
    """d_out, d_out_count and d_pair_rows byte for byte, the sentinel-filled parts included (neither call writes a dropped row)"""
    import torch
    ctx = B.default_context(0)
    case = equal_case(*EQUAL_CASES[(form, dim, pitch)])
    fr = Frames(B, case, pitch, base_off, slack)
    n = len(case.pairs)
    spec = B.PairSpec(n, 0, 1, 0, 1, None)
    want, got = sentinel_outputs(n, ROWS_CAP, 1), sentinel_outputs(n, ROWS_CAP, 1)
    torch.cuda.synchronize()
    ctx.match_knn_pairs(fr.A.set, fr.Bs.set, spec, 1, cross_check=True, rows_cap=ROWS_CAP, dim_bytes=dim, out=want, gate=B.MatchGate(*case.window),
                        query_kps=fr.Ak.set, train_kps=fr.Bk.set)
    mutual(ctx, case)(fr.A.set, fr.Bs.set, spec, fr.models, guide_of(B, case), rows_cap=ROWS_CAP, query_kps=fr.Ak.set, train_kps=fr.Bk.set,
                      dim_bytes=dim, out=got)
    torch.cuda.synchronize()
    for name, g, w in zip(("matches", "counts", "pair_rows"), got, want):
        g, w = g.cpu().numpy(), w.cpu().numpy()
        assert g.tobytes() == w.tobytes(), (name, np.argwhere(g != w)[:5])
    cnt = want[1].cpu().numpy()
    assert (cnt == 1).sum() > 300 and (cnt == 0).sum() > 300       # (the comparison is not one of sentinels alone)
    assert want[2].cpu().numpy().tolist() == [len(p.kq) for p in case.pairs]


# ---- 2: a model per pair, all pair forms, against the restatement ------------------------------------------------------------------

def expected(case, pair, b):
    ft, fd, kept, _ = restated_mutual(case, pair)
    return len(pair.kq), b, ft, fd, kept


@pytest.mark.parametrize("max_octave_diff", [0, 1])
@pytest.mark.parametrize("form", [CENTRE, LINE])
def test_a_model_per_pair(B, form, max_octave_diff):
    """side by side, the keyframe form (train_step = 0: the models are indexed by PAIR) and a device list with bad entries; unguided
    pairs with fallback 0 (max_octave_diff 0) and 1, n_b = 0 and n_a = 0 among the pairs; all outputs poison-filled"""
    import torch
    ctx = B.default_context(0)
    case = general_case(*GENERAL_CASES[(form, max_octave_diff)])
    fr = Frames(B, case, *LAYOUT[case.dim])
    n, P = len(case.pairs), case.pairs
    # side by side
    out = sentinel_outputs(n, ROWS_CAP, 1)
    torch.cuda.synchronize()
    mutual(ctx, case)(fr.A.set, fr.Bs.set, B.PairSpec(n, 0, 1, 0, 1, None), fr.models, guide_of(B, case), rows_cap=ROWS_CAP, query_kps=fr.Ak.set,
                      train_kps=fr.Bk.set, dim_bytes=case.dim, out=out)
    torch.cuda.synchronize()
    assert compare(B, out, [expected(case, p, b) for b, p in enumerate(P)], ROWS_CAP) > 100
    # every query frame against train frame 0, pair p under model p
    out = sentinel_outputs(n, ROWS_CAP, 1)
    mutual(ctx, case)(fr.A.set, fr.Bs.set, B.PairSpec(n, 0, 1, 0, 0, None), fr.models, guide_of(B, case), rows_cap=ROWS_CAP, query_kps=fr.Ak.set,
                      train_kps=fr.Bk.set, dim_bytes=case.dim, out=out)
    torch.cuda.synchronize()
    key = [Pair(p.kq, P[0].kt, p.dq, P[0].dt, p.model, p.hypothesis, p.flags) for p in P]
    by_frame = [Pair(p.kq, P[0].kt, p.dq, P[0].dt, P[0].model, P[0].hypothesis, P[0].flags) for p in P]
    assert sum(not np.array_equal(restated_mutual(case, a)[2], restated_mutual(case, b)[2]) for a, b in zip(key, by_frame)) >= 2
    assert compare(B, out, [expected(case, p, 0) for p in key], ROWS_CAP) > 20
    # a device list: repeated and crossed pairs, two entries outside the sets; list entry i under model i
    plist = [(0, 0), (2, 1), (n, 0), (1, 2), (5, 5), (0, -1), (7, 0), (0, 0)]
    spec, keep = pair_spec(B, plist)
    out = sentinel_outputs(len(plist), ROWS_CAP, 1)
    mutual(ctx, case)(fr.A.set, fr.Bs.set, spec, fr.models, guide_of(B, case), rows_cap=ROWS_CAP, query_kps=fr.Ak.set, train_kps=fr.Bk.set,
                      dim_bytes=case.dim, out=out)
    torch.cuda.synchronize()
    want = []
    for i, (a, b) in enumerate(plist):
        ok = 0 <= a < n and 0 <= b < n
        want.append(expected(case, Pair(P[a].kq, P[b].kt, P[a].dq, P[b].dt, P[i].model, P[i].hypothesis, P[i].flags), b) if ok else None)
    assert compare(B, out, want, ROWS_CAP) > 20
    # rows_cap cutting more: the backward scan still covers all of frame a
    small = 64
    out = sentinel_outputs(n, small, 1)
    mutual(ctx, case)(fr.A.set, fr.Bs.set, B.PairSpec(n, 0, 1, 0, 1, None), fr.models, guide_of(B, case), rows_cap=small, query_kps=fr.Ak.set,
                      train_kps=fr.Bk.set, dim_bytes=case.dim, out=out)
    torch.cuda.synchronize()
    cut = type(case)(case.form, case.dim, case.window, case.band, case.fallback, small, P)
    assert compare(B, out, [expected(cut, p, b) for b, p in enumerate(P)], small) > 50


# ---- 3: what is kept is the guided call's record -------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", [CENTRE, LINE])
def test_kept_records_are_the_guided_call_s(B, form):
    import torch
    ctx = B.default_context(0)
    case = general_case(*MEMORY_CASES[form])
    fr = Frames(B, case, *LAYOUT[case.dim])
    n = len(case.pairs)
    spec = B.PairSpec(n, 0, 1, 0, 1, None)
    one, both = sentinel_outputs(n, ROWS_CAP, 1), sentinel_outputs(n, ROWS_CAP, 1)
    guided = ctx.match_knn_pairs_epipolar_guided if form == LINE else ctx.match_knn_pairs_guided
    torch.cuda.synchronize()
    guided(fr.A.set, fr.Bs.set, spec, 1, fr.models, guide_of(B, case), rows_cap=ROWS_CAP, query_kps=fr.Ak.set, train_kps=fr.Bk.set,
           dim_bytes=case.dim, out=one)
    mutual(ctx, case)(fr.A.set, fr.Bs.set, spec, fr.models, guide_of(B, case), rows_cap=ROWS_CAP, query_kps=fr.Ak.set, train_kps=fr.Bk.set,
                      dim_bytes=case.dim, out=both)
    torch.cuda.synchronize()
    (m1, c1, r1), (m2, c2, r2) = ([t.cpu().numpy() for t in o] for o in (one, both))
    assert r1.tobytes() == r2.tobytes()
    m1, m2 = m1.reshape(n, ROWS_CAP, 4), m2.reshape(n, ROWS_CAP, 4)
    kept = c2 == 1
    assert kept.sum() > 100 and ((c1 == 1) & (c2 == 0)).sum() > 20 and not ((c2 == 1) & (c1 != 1)).any()
    assert m2[kept].tobytes() == m1[kept].tobytes()
    assert (m2[~kept] == SENTINEL).all() and ((c2 == c1) | (c2 == 0)).all()
    for p in range(n):                                               # mutual: no train row twice within a pair
        t = m2[p][kept[p]][:, 1]
        assert len(np.unique(t)) == len(t), p


# ---- 4: nothing behind a count, beyond rows or of a bad pair is written ----------------------------------------------------------------

@pytest.mark.parametrize("form", [CENTRE, LINE])
def test_nothing_else_is_written(B, form):
    """all three outputs poison-filled; a list with a bad entry; pair_rows holds the TRUE counts, also where rows_cap cuts the frame
    or the pair is unguided (fallback 0)"""
    import torch
    ctx = B.default_context(0)
    case = general_case(*MEMORY_CASES[form])
    assert case.fallback == 0
    fr = Frames(B, case, *LAYOUT[case.dim])
    n, P = len(case.pairs), case.pairs
    plist = [(p, p) for p in range(n)]
    plist.insert(3, (-1, 2))
    rec = case.records()
    models = upload_models(np.concatenate([rec[:3], rec[:1], rec[3:]]))
    spec, keep = pair_spec(B, plist)
    out = sentinel_outputs(len(plist), 96, 1)
    torch.cuda.synchronize()
    mutual(ctx, case)(fr.A.set, fr.Bs.set, spec, models, guide_of(B, case), rows_cap=96, query_kps=fr.Ak.set, train_kps=fr.Bk.set,
                      dim_bytes=case.dim, out=out)
    torch.cuda.synchronize()
    cut = type(case)(case.form, case.dim, case.window, case.band, case.fallback, 96, P)
    want = [None if a < 0 else expected(cut, P[a], b) for a, b in plist]
    assert compare(B, out, want, 96) > 50
    rows = out[2].cpu().numpy()
    unguided = [i for i, (a, _) in enumerate(plist) if a >= 0 and (P[a].hypothesis < 0 or P[a].flags & (PAIR_BAD | PAIR_NO_MODEL))]
    assert unguided and all(rows[i] == len(P[plist[i][0]].kq) for i in unguided)
    assert (rows > 96).sum() >= 3


# ---- 5: the real path, no host in between ------------------------------------------------------------------------------------------

SELECT, VERIFY, EPI_VERIFY = (90.0, 0.8, 1), (3.0, 256, 12, 0, 2024), (1.5, 128, 12, 0, 2026)
GUIDE_WINDOW, RESELECT = (-6.0, 6.0, -6.0, 6.0, 1), (90.0, 0.0, 1)
EPI_WINDOW, EPI_BAND = (-200.0, 200.0, -200.0, 200.0, 1), 1.5


@pytest.mark.parametrize("branch", ["homography", "epipolar"])
def test_the_real_path_without_the_host(B, golden_ast, branch):
    """detect + describe, k-NN (k = 2), select (ratio 0.8), verify, the mutual guided pass reading the verifier's models in place, select
    (keep 1), link - one stream, one synchronisation at the end.  The mutual pass against the restatement under the models the
    verifier wrote; every selected record is linked: mutual matches leave the linker's claim rule nothing to settle."""
    import torch
    frames = batch_frames(golden_ast)
    n, h, w = frames.shape
    d = torch.from_numpy(frames).cuda()
    ctx = B.Context(0)
    ext = B.BriskDescriptorExtractor(context=ctx)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    spec = B.PairSpec(n - 1, 1, 1, 0, 1, None)
    ctx.detect_describe_batch(ext, d.data_ptr(), n, w, h, w * h, w, 70, 2, s.cuda_stream)
    st, dim = ctx.batch_desc_set()
    first = ctx.match_knn_pairs(st, st, spec, 2, stream=s.cuda_stream)
    rows_cap = int(first[1].shape[1])
    sel = ctx.select_pair_matches(first, 2, B.MatchSelect(*SELECT), stream=s.cuda_stream)
    if branch == "homography":
        ver = ctx.verify_pair_matches(st, st, spec, rows_cap, sel[3], sel[0], B.PairVerify(*VERIFY), stream=s.cuda_stream)
        guide = B.MatchGuide(B.MatchGate(*GUIDE_WINDOW), 0)
        mut = ctx.match_mutual_pairs_guided(st, st, spec, ver[4], guide, rows_cap=rows_cap, stream=s.cuda_stream)
    else:
        ver = ctx.verify_pair_matches_epipolar(st, st, spec, rows_cap, sel[3], sel[0], B.PairVerify(*EPI_VERIFY), stream=s.cuda_stream)
        guide = B.MatchEpipolarGuide(B.MatchGate(*EPI_WINDOW), EPI_BAND, 0)
        mut = ctx.match_mutual_pairs_epipolar_guided(st, st, spec, ver[4], guide, rows_cap=rows_cap, stream=s.cuda_stream)
    resel = ctx.select_pair_matches(mut, 1, B.MatchSelect(*RESELECT), stream=s.cuda_stream)
    linked = ctx.link_tracks((st, 0, 1), n, rows_cap, resel[3], resel[0], stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert ctx.batch_status(n) == 0
    kd = [ctx.batch_download(f, True, strings=dim) for f in range(n)]
    kps, desc = [k for k, _ in kd], [dd for _, dd in kd]
    models = ver[4].cpu().numpy().reshape(-1).view(B.PAIR_EPIPOLAR_MODEL if branch == "epipolar" else B.PAIR_MODEL)
    got_rows, pair_rows = knn_rows(B, tuple(t.cpu().numpy() for t in mut), 1)
    assert np.array_equal(pair_rows, np.array([len(k) for k in kps[1:]]))
    kept_total = dropped_total = 0
    for p in range(n - 1):
        kq, kt = kps[p + 1], kps[p]
        if branch == "homography":
            M, has = guide_mask(GUIDE_WINDOW, 0, models[p], kq, kt)
        else:
            M, has = epi_mask(EPI_WINDOW, EPI_BAND, 0, models[p], kq, kt)
        ft, fd, kept, _ = mutual_under_mask(M, has, desc[p + 1], desc[p], rows_cap)
        assert len(got_rows[p]) == len(kept)
        for q, r in enumerate(got_rows[p]):
            assert len(r) == int(kept[q]), (p, q)
            if kept[q]:
                assert (r[0]["queryIdx"], r[0]["trainIdx"], r[0]["imgIdx"], r[0]["distance"]) == (q, ft[q], p, np.float32(fd[q])), (p, q)
        kept_total, dropped_total = kept_total + int(kept.sum()), dropped_total + int(((ft >= 0) & ~kept).sum())
    summary = linked[3].cpu().numpy()
    selected = int(resel[3].cpu().numpy()[-1])
    print("%s: %d rows kept, %d dropped by the backward scan; %d selected, %d linked, %d claim losers" %
          (branch, kept_total, dropped_total, selected, int(summary[2]), int(summary[3])))
    assert kept_total > 100 and dropped_total > 0 and 0 < selected <= kept_total
    assert int(summary[2]) == selected and int(summary[3]) == 0 and int(summary[4]) == 0
    prev = linked[0].cpu().numpy()
    assert sum(int((prev[i, :min(len(k), rows_cap)] >= 0).sum()) for i, k in enumerate(kps)) == selected   # (only a node's rows are written)
    ext.close()
    ctx.close()


# ---- 6: arguments -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", [CENTRE, LINE])
def test_arguments(B, form):
    """the guided calls' list, all before anything is launched"""
    import torch
    ctx = B.default_context(0)
    case = general_case(*MEMORY_CASES[form])
    fr = Frames(B, case, 64, 0, 0)
    n = len(case.pairs)
    cap = max(len(p.kq) for p in case.pairs)
    out = sentinel_outputs(n, ROWS_CAP, 1)
    torch.cuda.synchronize()
    m, cnt, rows = (t.data_ptr() for t in out)
    L, h = ctx._L, ctx._h
    fn = L.brisk_hip_match_mutual_pairs_epipolar_guided_device if form == LINE else L.brisk_hip_match_mutual_pairs_guided_device
    A, Ak = fr.A.set, fr.Ak.set

    def ref(x):
        return None if x is None else C.byref(x)

    def call(q=A, t=fr.Bs.set, qk=Ak, tk=fr.Bk.set, md=fr.models.data_ptr(), g=guide_of(B, case), spec=(n, 0, 1, 0, 1, None), dim=48, cap=ROWS_CAP,
             m=m, cnt=cnt, rows=rows):
        return fn(h, ref(q), ref(t), ref(qk), ref(tk), C.byref(B.PairSpec(*spec)), md, ref(g), dim, cap, m, cnt, rows, None)

    assert call(md=None) == ARG and call(md=fr.models.data_ptr() + 4) == ARG and call(g=None) == ARG
    assert call(qk=None) == ARG and call(tk=None) == ARG
    assert call(qk=B.KpSet(None, cap * 28)) == ARG and call(tk=B.KpSet(None, cap * 28)) == ARG
    assert call(qk=B.KpSet(Ak.d_kps + 2, cap * 28)) == ARG and call(tk=B.KpSet(Ak.d_kps, cap * 28 + 2)) == ARG
    assert call(tk=B.KpSet(Ak.d_kps, -28)) == ARG
    assert call(dim=40) == UNSUPPORTED and call(dim=96) == UNSUPPORTED
    assert call(spec=(n + 1, 0, 1, 0, 1, None)) == ARG             # the last pair's frames are outside the sets
    assert call(spec=(n, 0, 1, -1, 1, None)) == ARG
    assert call(spec=(-1, 0, 1, 0, 1, None)) == ARG
    assert call(cap=0) == ARG
    narrow = B.DescSet(A.d_desc, A.d_counts, 3, A.frame_pitch, 40, n)
    assert call(q=narrow) == ARG and call(t=narrow) == ARG          # row_pitch < dim_bytes
    assert call(m=None) == ARG and call(cnt=None) == ARG and call(rows=None) == ARG
    assert call(q=None) == ARG and call(t=None) == ARG
    assert call(spec=(0, 0, 1, 0, 1, None)) == 0                    # no pairs: fine, nothing to do ...
    assert call(spec=(0, 0, 1, 0, 1, None), qk=None, tk=None, md=None, g=None, m=None, cnt=None, rows=None) == 0   # ... nothing is looked at
    assert fn(None, ref(A), ref(A), ref(Ak), ref(Ak), C.byref(B.PairSpec(n, 0, 1, 0, 1, None)), fr.models.data_ptr(), ref(guide_of(B, case)), 48,
              ROWS_CAP, m, cnt, rows, None) == ARG
    torch.cuda.synchronize()
    for t in out:                                                    # none of these calls launched anything
        assert (t.cpu().numpy() == SENTINEL).all()
    for dim in (16, 32, 64):                                         # the other descriptor sizes are accepted (rows of 64 bytes hold them)
        assert call(dim=dim) == 0
    torch.cuda.synchronize()


# ---- 7: stream order ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def mutual_env(env):
    """the held-stream environment of tests/test_gpu_stream_order.py, and the mutual call's serial outputs for its two batches"""
    e, torch = env, env.torch
    e.mutual_guide = e.B.MatchGuide(e.B.MatchGate(-6.0, 6.0, -6.0, 6.0, 1), 1)
    e.mutual_out = tuple(torch.empty(s, dtype=torch.int32, device="cuda") for s in ((e.n - 1, e.cap, 1, 4), (e.n - 1, e.cap), (e.n - 1,)))
    e.mutual_serial = {}
    for b in (1, 2):
        assert run_batch(e, b, sptr(e.main)) == 0
        fill_mutual(e)
        assert call_mutual(e, b, sptr(e.main)) == 0
        torch.cuda.synchronize()
        e.mutual_serial[b] = [t.cpu().numpy().copy() for t in e.mutual_out]
    for a1, a2 in zip(*e.mutual_serial.values()):                   # a case on equal bytes would prove nothing
        assert a1.tobytes() != a2.tobytes()
    return e


def fill_mutual(e):
    for t in e.mutual_out:
        t.view(e.torch.uint8).fill_(0x5A)
    e.torch.cuda.synchronize()


def call_mutual(e, b, s):
    """the mutual call on the context's own sets, under the models the serial verification of batch b wrote (caller memory)"""
    m, cnt, rows = e.mutual_out
    return e.L.brisk_hip_match_mutual_pairs_guided_device(e.h, C.byref(e.st), C.byref(e.st), C.byref(e.kp), C.byref(e.kp), C.byref(e.spec),
                                                          C.c_void_p(e.serial_dev[b]["verify"][4].data_ptr()), C.byref(e.mutual_guide), e.dim,
                                                          e.cap, m.data_ptr(), cnt.data_ptr(), rows.data_ptr(), s)


def compare_mutual(e, b):
    for i, (name, t) in enumerate(zip(("matches", "counts", "pair_rows"), e.mutual_out)):
        g = t.cpu().numpy()
        assert g.tobytes() == e.mutual_serial[b][i].tobytes(), "%s is not the serial run's of batch %d; equal to batch %d's: %s" % (
            name, b, 3 - b, g.tobytes() == e.mutual_serial[3 - b][i].tobytes())


def test_write_after_read(mutual_env):
    """batch 1 complete; the mutual call on the held S, batch 2 - which overwrites the descriptors, keypoints and counts it is given - on
    S2.  Its outputs are batch 1's: batch 2 waited for it."""
    e = mutual_env
    begin(e)
    fill_mutual(e)
    race(e, lambda s: call_mutual(e, 1, s), lambda s: run_batch(e, 2, s))
    compare_mutual(e, 1)


def test_read_after_write(mutual_env):
    """batch 1 complete; batch 2 on the held S, the mutual call - given batch 2's models - on S2.  Its outputs are batch 2's: it waited
    for the batch."""
    e = mutual_env
    begin(e)
    fill_mutual(e)
    race(e, lambda s: run_batch(e, 2, s), lambda s: call_mutual(e, 2, s))
    compare_mutual(e, 2)

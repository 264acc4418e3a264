"""GPU tests of the pair matchers' exit: brisk_hip_select_pair_matches_device (selected matches, packed on the device) and
brisk_hip_pair_matches_download / _wait (the same in host memory, asynchronous, with a ticket).  The expectation is always the
numpy restatement of the selection rule (test_abi_match_export.restated_row) applied to the downloaded padded arrays - which the
sibling tests pin to the oracle.  Records are compared as bit patterns, counts, flags and offsets must be equal: no tolerance."""
import ctypes as C

import numpy as np
import pytest

from gpu_prefill import settled
from test_abi_match_export import restated_row
from test_gpu_match_gated import GRID_GATE, SynthKp
from test_gpu_match_pairs import CAP, COUNTS_A, COUNTS_B, SENTINEL, SynthSet, batch_frames, run_pairs
from test_oracle_golden import homography_outliers

pytestmark = pytest.mark.gpu

INF = float("inf")
ROWS_CUT = 0x100
RADIUS_CAP = 4
RADIUS = {16: 48.0, 48: 165.0}     # about 8 % of random train rows are nearer: rows with fewer and with more than RADIUS_CAP hits
NEAR = {16: 40.0, 48: 150.0}       # about the best distance a row finds among ~100 random train rows


@pytest.fixture(scope="module")
def B():
    import ethzasl_brisk_amd as B
    from ethzasl_brisk_amd import build
    build.build()
    B.load_library()
    return B


# ---- the expectation --------------------------------------------------------------------------------------------------------

def host_triple(B, triple, per_row):
    """the padded arrays of a matcher call on the host: (records [npairs, rows_cap, per_row], counts, pair_rows)"""
    m, cnt, rows = (t.cpu().numpy() for t in triple)
    return m.view(B.DMATCH).reshape(cnt.shape[0], cnt.shape[1], per_row), cnt, rows


def expect(host, per_row, sel, matches_cap=None):
    """(matches, counts, flags, offsets, rows that give an entry, rows that lose a stored entry) the rule gives for the padded
    arrays `host`"""
    m, cnt, rows = host
    npairs, rows_cap = cnt.shape
    md, ratio, keep = sel
    lists, counts, flags = [], np.zeros(npairs, np.int32), np.zeros(npairs, np.int32)
    kept = dropped = 0
    for p in range(npairs):
        r = int(rows[p])
        flags[p] = (1 if r > rows_cap else 0) | (2 if r == -1 else 0)
        sel_p = []
        for q in range(min(max(r, 0), rows_cap)):
            c = int(cnt[p, q])
            if c > per_row:
                flags[p] |= 4
            n = restated_row(md, ratio, keep, per_row, c, m[p, q, :max(min(c, per_row), 0)]["distance"])
            sel_p.append(m[p, q, :n])
            kept, dropped = kept + (n > 0), dropped + (n < min(c, per_row))
        lists.append(np.concatenate(sel_p) if sel_p else m[0, 0, :0])
        counts[p] = len(lists[-1])
    offsets = np.zeros(npairs + 1, np.int64)
    cut = npairs
    if matches_cap is not None:
        run = 0
        for p in range(npairs):
            if counts[p] > 0 and run + counts[p] > matches_cap:
                cut = p
                break
            run += counts[p]
    flags[cut:] |= ROWS_CUT
    for p in range(npairs):
        offsets[p + 1] = offsets[p] + (counts[p] if p < cut else 0)
    stored = np.concatenate(lists[:cut]) if cut else m[0, 0, :0]
    return stored, counts, flags, offsets, kept, dropped


def same_selection(got, want):
    """got: (matches records, counts, flags, offsets) on the host"""
    gm, gc, gf, go = got
    wm, wc, wf, wo = want[:4]
    assert np.array_equal(gc, wc), (gc, wc)
    assert np.array_equal(gf, wf), (gf, wf)
    assert np.array_equal(go, wo), (go, wo)
    n = int(wo[-1])
    assert n == len(wm)
    assert gm[:n].tobytes() == wm.tobytes()                         # bit patterns, all four fields


def device_select(B, ctx, triple, per_row, sel, matches_cap=None):
    import torch
    res = ctx.select_pair_matches(triple, per_row, B.MatchSelect(*sel), matches_cap=matches_cap)
    torch.cuda.synchronize()
    m, c, f, o = (t.cpu().numpy() for t in res)
    return m.view(B.DMATCH).reshape(-1), c, f, o


def selections(dim, per_row, radius=False):
    """name -> (max_distance, ratio, keep_per_row)"""
    s = {"everything": (INF, 0.0, per_row), "distance": (NEAR[dim] if not radius else RADIUS[dim] - 8, 0.0, per_row)}
    if per_row >= 2 and not radius:
        s["ratio"] = (INF, 0.8, 1)
        s["ratio+distance"] = (NEAR[dim] - 10, 0.8, 1)
    if radius:
        s["keep1"] = (INF, -1.0, 1)
        s["ratio"] = (INF, 0.8, 1)
    return s


# ---- 1: caller sets -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=[16, 48])
def synth(B, request):
    """the padded results of k = 1, k = 2 and radius matching for frame-to-previous-frame inside set A and A beside B"""
    import torch
    dim = request.param
    rng = np.random.default_rng(500 + dim)
    ctx = B.default_context(0)
    A = SynthSet(B, rng, dim, dim + 16 * (dim == 48), COUNTS_A, CAP)
    Bs = SynthSet(B, rng, dim, dim, COUNTS_B, CAP, 0, 1, 0)
    nA = len(COUNTS_A)
    forms = {"previous": (A, A, B.PairSpec(nA - 1, 1, 1, 0, 1, None)), "beside": (A, Bs, B.PairSpec(nA, 0, 1, 0, 1, None))}
    torch.cuda.synchronize()
    run_pairs(B, ctx, A, A, (nA - 1, 1, 1, 0, 1), 2)               # (the padded arrays are the oracle's rows: pinned once more here)
    out = {}
    for name, (qs, ts, spec) in forms.items():
        for k in (1, 2):
            out[name, "knn", k] = ctx.match_knn_pairs(qs.set, ts.set, spec, k, rows_cap=CAP, dim_bytes=dim)
        out[name, "radius", RADIUS_CAP] = ctx.match_radius_pairs(qs.set, ts.set, spec, RADIUS[dim], RADIUS_CAP, rows_cap=CAP, dim_bytes=dim)
    torch.cuda.synchronize()
    return {"dim": dim, "ctx": ctx, "A": A, "Bs": Bs, "dev": out, "host": {key: host_triple(B, v, key[2]) for key, v in out.items()}}


def test_caller_sets(B, synth):
    dim, ctx = synth["dim"], synth["ctx"]
    both = {}
    for key, triple in synth["dev"].items():
        form, kind, per_row = key
        for name, sel in selections(dim, per_row, kind == "radius").items():
            want = expect(synth["host"][key], per_row, sel)
            same_selection(device_select(B, ctx, triple, per_row, sel), want)
            print(key, name, "selected %d, rows kept %d dropped %d, flags %s" % (want[3][-1], want[4], want[5], sorted(set(want[2].tolist()))))
            both.setdefault((kind, name), []).append(want[4] > 0 and want[5] > 0)
        if kind == "radius":
            assert (expect(synth["host"][key], per_row, (INF, 0.0, per_row))[2] & 4).any()   # some row found more than cap_per_query
    for (kind, name), cases in both.items():                        # every selection both keeps and drops somewhere
        if name != "everything":
            assert any(cases), (kind, name)
    # the top-up entries of k = 2 against a one-row frame are there, and are not delivered
    m, cnt, rows = synth["host"]["previous", "knn", 2]
    top = sum(int((m[p, q, :cnt[p, q]]["distance"] == np.float32(2147483648.0)).sum()) for p in range(len(rows)) for q in range(max(int(rows[p]), 0)))
    assert top > 0
    everything = expect(synth["host"]["previous", "knn", 2], 2, (INF, 0.0, 2))
    assert not (everything[0]["distance"] == np.float32(2147483648.0)).any()
    assert everything[3][-1] == sum(int(cnt[p, :max(int(rows[p]), 0)].sum()) for p in range(len(rows))) - top


# ---- 2: cut rows, bad pairs ---------------------------------------------------------------------------------------------------

def test_rows_cap_below_a_pair_and_a_bad_pair(B, synth):
    import torch
    ctx, A, Bs, dim = synth["ctx"], synth["A"], synth["Bs"], synth["dim"]
    nA, cap = len(COUNTS_A), 64                                     # 65 and 130 rows are cut, 64 and 63 are not
    plist = [(0, 0), (nA, 0), (5, 1), (3, -1), (4, 4), (2, 6)]
    d_pairs = torch.from_numpy(np.array(plist, np.int32)).cuda()
    torch.cuda.synchronize()
    triple = ctx.match_knn_pairs(A.set, Bs.set, B.PairSpec(len(plist), 0, 0, 0, 0, d_pairs.data_ptr()), 2, rows_cap=cap, dim_bytes=dim)
    torch.cuda.synchronize()
    host = host_triple(B, triple, 2)
    assert list(host[2]) == [COUNTS_A[0], -1, COUNTS_A[5], -1, COUNTS_A[4], COUNTS_A[2]]
    for sel in ((INF, 0.0, 2), (INF, 0.8, 1)):
        want = expect(host, 2, sel)
        assert list(want[2]) == [1, 2, 1, 2, 0, 0]
        assert want[1][1] == 0 and want[1][3] == 0 and want[1].sum() > 0
        same_selection(device_select(B, ctx, triple, 2, sel), want)


# ---- 3: matches_cap -----------------------------------------------------------------------------------------------------------

def raw_select(ctx, triple, per_row, sel, matches_cap, outs, npairs=None, rows_cap=None, stream=None):
    m, cnt, rows = triple
    ptr = lambda t: None if t is None else t.data_ptr()
    return ctx._L.brisk_hip_select_pair_matches_device(ctx._h, ptr(m), ptr(cnt), ptr(rows), cnt.shape[0] if npairs is None else npairs,
                                                       cnt.shape[1] if rows_cap is None else rows_cap, per_row,
                                                       None if sel is None else C.byref(sel), matches_cap, ptr(outs[1]), ptr(outs[2]),
                                                       ptr(outs[3]), ptr(outs[0]), stream)


def sentinel_select_outputs(npairs, matches):
    import torch
    return settled(torch.full((matches, 4), SENTINEL, dtype=torch.int32, device="cuda"), torch.full((npairs,), SENTINEL, dtype=torch.int32, device="cuda"),
                   torch.full((npairs,), SENTINEL, dtype=torch.int32, device="cuda"),
                   torch.full((npairs + 1,), SENTINEL, dtype=torch.int64, device="cuda"))


@pytest.mark.parametrize("short", ["one", "all", "middle"])
def test_matches_cap(B, synth, short):
    import torch
    ctx = synth["ctx"]
    key = ("previous", "knn", 2)                                    # its last pairs: (6, 5) one row, (7, 6) against one row
    triple, host, sel = synth["dev"][key], synth["host"][key], (INF, 0.0, 2)
    full = expect(host, 2, sel)
    total, npairs = int(full[3][-1]), len(full[1])
    cap = {"one": total - 1, "all": 0, "middle": int(full[3][npairs // 2 + 1]) - 1}[short]
    want = expect(host, 2, sel, matches_cap=cap)
    first_cut = int(np.flatnonzero(want[2] & ROWS_CUT)[0])
    assert (want[2][first_cut:] & ROWS_CUT).all() and not (want[2][:first_cut] & ROWS_CUT).any()
    assert np.array_equal(want[1], full[1])                         # the counts are still reported
    assert (want[3][first_cut:] == want[3][-1]).all() and want[3][-1] <= cap
    if short == "one":
        assert first_cut == int(np.flatnonzero(full[1])[-1])
    if short == "all":
        assert want[3][-1] == 0 and first_cut == int(np.flatnonzero(full[1])[0])
    outs = sentinel_select_outputs(npairs, total + 8)
    torch.cuda.synchronize()
    assert raw_select(ctx, triple, 2, B.MatchSelect(*sel), cap, outs) == 0
    torch.cuda.synchronize()
    m, c, f, o = (t.cpu().numpy() for t in outs)
    same_selection((m.view(B.DMATCH).reshape(-1), c, f, o), want)   # the pairs before the cut are intact
    assert (m[int(o[-1]):] == SENTINEL).all()                       # nothing behind the stored matches is written


# ---- 4: gated rows ----------------------------------------------------------------------------------------------------------------

def test_gated_rows(B, synth):
    import torch
    ctx, A, Bs, dim = synth["ctx"], synth["A"], synth["Bs"], synth["dim"]
    rng = np.random.default_rng(9)
    Ak, Bk = SynthKp(B, rng, COUNTS_A, CAP), SynthKp(B, rng, COUNTS_B, CAP)
    spec = B.PairSpec(len(COUNTS_A), 0, 1, 0, 1, None)
    torch.cuda.synchronize()
    res = {name: ctx.match_knn_pairs(A.set, Bs.set, spec, 2, rows_cap=CAP, dim_bytes=dim, gate=B.MatchGate(*g), query_kps=Ak.set, train_kps=Bk.set)
           for name, g in (("all", (-INF, INF, -INF, INF, -1)), ("window", GRID_GATE))}
    torch.cuda.synchronize()
    host = {name: host_triple(B, t, 2) for name, t in res.items()}
    nrows = lambda h: [min(max(int(r), 0), CAP) for r in h[2]]
    single = sum(int((host["window"][1][p, :n] == 1).sum()) for p, n in enumerate(nrows(host["window"])))
    assert single > 0                                               # rows with one entry under the ratio test
    for name in res:
        for sel in ((INF, 0.8, 1), (NEAR[dim], 0.8, 1), (INF, 0.0, 2)):
            want = expect(host[name], 2, sel)
            assert want[4] > 0
            same_selection(device_select(B, ctx, res[name], 2, sel), want)
    # an all-pass gate differs from the ungated call by the top-up entries alone: the selections are the same
    for sel in ((INF, 0.8, 1), (INF, 0.0, 2)):
        ungated = expect(synth["host"]["beside", "knn", 2], 2, sel)
        gated = expect(host["all"], 2, sel)
        for a, b in zip(ungated[:4], gated[:4]):
            assert a.tobytes() == b.tobytes()
    m, cnt, rows = synth["host"]["beside", "knn", 2]                # (B's frame 3 has one row: ungated rows topped up, gated rows of one entry)
    assert (m[3, :COUNTS_A[3], 1]["distance"] == np.float32(2147483648.0)).all() and (host["all"][1][3, :COUNTS_A[3]] == 1).all()


# ---- 5 / 6: the host form -----------------------------------------------------------------------------------------------------------

def host_got(dst, npairs):
    return dst.matches, dst.counts[:npairs], dst.flags[:npairs], dst.offsets[:npairs + 1]


@pytest.mark.parametrize("pinned", [True, False])
def test_host_form_on_a_batch(B, golden_ast, pinned):
    """detect + describe, k = 2 matching and the download on one stream without a synchronisation, the next batch (other frames,
    the same match arrays) issued at once; the rows' own download and two match downloads outstanding together"""
    import torch
    frames = batch_frames(golden_ast)
    n, h, w = frames.shape
    d1, d2 = torch.from_numpy(frames).cuda(), torch.from_numpy(np.ascontiguousarray(frames[::-1])).cuda()
    ctx = B.Context(0)
    ext = B.BriskDescriptorExtractor(context=ctx)
    s = torch.cuda.Stream()
    spec = B.PairSpec(n - 1, 1, 1, 0, 1, None)                      # frame to previous frame
    sel = (50.0, 0.8, 1)
    dst = [B.HostMatches(n - 1, (n - 1) * 16384, pinned=pinned) for _ in range(2)]
    rows_dst = B.HostResults(n, n * 16384, 48, pinned=pinned)
    torch.cuda.synchronize()
    ctx.detect_describe_batch(ext, d1.data_ptr(), n, w, h, w * h, w, 70, 2, s.cuda_stream)
    st, dim = ctx.batch_desc_set()
    out = ctx.match_knn_pairs(st, st, spec, 2, stream=s.cuda_stream)
    t1 = ctx.pair_matches_download(out, 2, B.MatchSelect(*sel), dst[0], stream=s.cuda_stream)
    dev1 = ctx.select_pair_matches(out, 2, B.MatchSelect(*sel), matches_cap=(n - 1) * 16384, stream=s.cuda_stream)
    with torch.cuda.stream(s):
        saved1 = tuple(t.clone() for t in out)
    # the next batch at once: its results and its matches overwrite the first batch's
    ctx.detect_describe_batch(ext, d2.data_ptr(), n, w, h, w * h, w, 70, 2, s.cuda_stream)
    st2, _ = ctx.batch_desc_set()
    ctx.match_knn_pairs(st2, st2, spec, 2, stream=s.cuda_stream, out=out)
    tr = ctx.batch_download_all(rows_dst, stream=s.cuda_stream)
    t2 = ctx.pair_matches_download(out, 2, B.MatchSelect(*sel), dst[1], stream=s.cuda_stream)
    # one transfer of rows and two of matches are outstanding: every wait succeeds, in any order
    assert ctx.pair_matches_wait(t2) == 0
    assert ctx.batch_download_wait(tr) == 0
    assert ctx.pair_matches_wait(t1) == 0
    torch.cuda.synchronize()
    assert ctx.batch_status(n) == 0
    kd = [ctx.batch_download(f, True, strings=dim) for f in range(n)]          # the second batch: frame f = frames[n - 1 - f]
    for f in range(n):
        assert rows_dst.frame(f, dim)[0].tobytes() == kd[f][0].tobytes() and np.array_equal(rows_dst.frame(f, dim)[1], kd[f][1])
    want1 = expect(host_triple(B, saved1, 2), 2, sel)
    m, c, f, o = (t.cpu().numpy() for t in dev1)
    same_selection((m.view(B.DMATCH).reshape(-1), c, f, o), want1)  # the device form ...
    same_selection(host_got(dst[0], n - 1), want1)                  # ... and the host form equal the rule
    assert np.array_equal(dst[0].pair_rows[:n - 1], saved1[2].cpu().numpy())
    want2 = expect(host_triple(B, out, 2), 2, sel)
    same_selection(host_got(dst[1], n - 1), want2)
    assert want1[4] > 0 and want1[5] > 0 and want2[0].tobytes() != want1[0].tobytes()
    # pair 0 of the first batch = (img1, img2): the reference's matching test (brisk/src/test/test-match.cc:49-126)
    best = dst[0].pair(0)
    assert len(best) > 100 and (best["distance"] < 50).all()
    assert homography_outliers(kd[n - 2][0], kd[n - 1][0], best) == 0          # (frames 1 and 0 of the first batch)
    ext.close()
    ctx.close()


def test_three_downloads_in_flight(B, synth):
    import torch
    ctx = synth["ctx"]
    keys = [("beside", "knn", 1), ("previous", "knn", 2), ("beside", "radius", RADIUS_CAP)]
    sels = [(NEAR[synth["dim"]], 0.0, 1), (INF, 0.8, 1), (INF, 0.0, 2)]
    dsts = [B.HostMatches(8, 4096, pinned=False), B.HostMatches(8, 4096, pinned=True), B.HostMatches(8, 4096, pinned=True)]
    torch.cuda.synchronize()
    tickets = [ctx.pair_matches_download(synth["dev"][k], k[2], B.MatchSelect(*sel), dst) for k, sel, dst in zip(keys, sels, dsts)]
    assert len(set(tickets)) == 3 and 0 not in tickets
    flagged = int((expect(synth["host"][keys[2]], keys[2][2], sels[2])[2] != 0).sum())
    assert flagged > 0                                              # (radius rows cut by cap_per_query: information, not an error)
    assert ctx.pair_matches_wait(tickets[2]) == flagged             # completes the second as well; the third call completed the first
    for k, sel, dst in zip(keys, sels, dsts):
        npairs = synth["host"][k][1].shape[0]
        want = expect(synth["host"][k], k[2], sel)
        same_selection(host_got(dst, npairs), want)
        assert np.array_equal(dst.pair_rows[:npairs], synth["host"][k][2])
        assert [len(dst.pair(p)) for p in range(npairs)] == list(want[1])
    assert ctx.pair_matches_wait(tickets[1]) == 0
    rc, _ = ctx.pair_matches_wait(tickets[0], check=False)
    assert rc == 1                                                  # its slot went to the third transfer: unknown ticket
    rc, _ = ctx.pair_matches_wait(12345, check=False)
    assert rc == 1
    # a destination too small for the matches: the clean pairs in place, BRISK_HIP_ERR_CAPACITY
    k, sel = keys[1], (INF, 0.0, 2)
    full = expect(synth["host"][k], 2, sel)
    small = B.HostMatches(8, int(full[3][-1]) - 1, pinned=True)
    rc, flagged = ctx.pair_matches_wait(ctx.pair_matches_download(synth["dev"][k], 2, B.MatchSelect(*sel), small), check=False)
    want = expect(synth["host"][k], 2, sel, matches_cap=int(full[3][-1]) - 1)
    assert rc == 4 and flagged == int((want[2] != 0).sum())
    assert "matches_cap" in ctx._L.brisk_hip_last_error(ctx._h).decode()
    same_selection(host_got(small, len(want[1])), want)


# ---- 7: arguments ---------------------------------------------------------------------------------------------------------------

def test_arguments(B, synth):
    import torch
    ctx = synth["ctx"]
    key = ("beside", "knn", 2)
    triple = synth["dev"][key]
    npairs = triple[1].shape[0]
    outs = sentinel_select_outputs(npairs, 64)
    one = synth["dev"]["beside", "knn", 1]
    torch.cuda.synchronize()
    ARG = 1
    ok = B.MatchSelect(INF, 0.0, 2)
    for i in range(4):                                              # a NULL output (d_matches: with a capacity above 0)
        assert raw_select(ctx, triple, 2, ok, 64, tuple(None if j == i else t for j, t in enumerate(outs))) == ARG
    for i in range(3):                                              # a NULL match array
        assert raw_select(ctx, tuple(None if j == i else t for j, t in enumerate(triple)), 2, ok, 64, outs, npairs=npairs, rows_cap=CAP) == ARG
    assert raw_select(ctx, triple, 0, ok, 64, outs) == ARG          # per_row < 1
    assert raw_select(ctx, triple, 2, B.MatchSelect(INF, 0.0, 0), 64, outs) == ARG     # keep_per_row < 1
    assert raw_select(ctx, triple, 2, B.MatchSelect(INF, 0.0, -3), 64, outs) == ARG
    assert raw_select(ctx, one, 1, B.MatchSelect(INF, 0.8, 1), 64, outs) == ARG        # the ratio test on rows of one entry
    assert raw_select(ctx, triple, 2, ok, -1, outs) == ARG          # negative caps
    assert raw_select(ctx, triple, 2, ok, 64, outs, npairs=-1) == ARG
    assert raw_select(ctx, triple, 2, ok, 64, outs, rows_cap=0) == ARG
    assert raw_select(ctx, triple, 2, None, 64, outs) == ARG
    with pytest.raises(B.BriskHipError) as ei:
        ctx.select_pair_matches(one, 1, B.MatchSelect(INF, 0.8, 1))
    assert ei.value.code == ARG
    dst = B.HostMatches(npairs, 64, pinned=True)
    with pytest.raises(B.BriskHipError) as ei:
        ctx.pair_matches_download(triple, 2, B.MatchSelect(INF, 0.0, 0), dst)
    assert ei.value.code == ARG
    with pytest.raises(B.BriskHipError) as ei:
        ctx.pair_matches_download(triple, 2, ok, B.HostMatches(npairs - 1, 64, pinned=True))    # pairs_cap below npairs
    assert ei.value.code == ARG
    torch.cuda.synchronize()
    for t in outs:                                                  # none of these calls launched anything
        assert (t.cpu().numpy() == SENTINEL).all()
    # no pairs: fine, the one offset is written
    assert raw_select(ctx, triple, 2, ok, 64, outs, npairs=0) == 0
    assert raw_select(ctx, (None, None, None), 2, ok, 0, (None, None, None, None), npairs=0, rows_cap=CAP) == 0
    torch.cuda.synchronize()
    assert int(outs[3][0]) == 0 and (outs[3][1:].cpu().numpy() == SENTINEL).all()
    for t in outs[:3]:
        assert (t.cpu().numpy() == SENTINEL).all()
    # keep_per_row above per_row is fine: the stored entries bound it
    assert raw_select(ctx, triple, 2, B.MatchSelect(INF, 0.0, 1000), 64 * 1024, sentinel_select_outputs(npairs, 64 * 1024)) == 0
    torch.cuda.synchronize()


# ---- 8: both exits in flight on one context ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def three_frames(golden_ast):
    import torch
    frames = np.ascontiguousarray(batch_frames(golden_ast)[:3])     # img2, img1, img1 shifted: keypoints in every frame
    return torch.from_numpy(frames).cuda(), frames.shape


class BothExits:
    """a fresh context with a described batch of three frames and its k = 2 matches over the pairs (0, 1), (1, 2), (0, 2), all on the
    context's own stream, and what the synchronous routes deliver for them: per-frame batch_download, select_pair_matches + copy"""
    SEL = (INF, 0.0, 2)

    def __init__(self, B, three_frames):
        import torch
        d, (n, h, w) = three_frames
        self.B, self.n = B, n
        self.ctx = B.Context(0)
        self.ext = B.BriskDescriptorExtractor(context=self.ctx)
        self.d_pairs = torch.from_numpy(np.array([(0, 1), (1, 2), (0, 2)], np.int32)).cuda()
        torch.cuda.synchronize()
        self.ctx.detect_describe_batch(self.ext, d.data_ptr(), n, w, h, w * h, w, 70, 2)
        st, self.dim = self.ctx.batch_desc_set()
        self.out = self.ctx.match_knn_pairs(st, st, B.PairSpec(3, 0, 0, 0, 0, self.d_pairs.data_ptr()), 2)
        self.rows = [self.ctx.batch_download(f, True, strings=self.dim) for f in range(n)]
        self.nrows = sum(len(k) for k, _ in self.rows)
        self.matches = self.select()
        self.nmatches = int(self.matches[3][-1])
        self.pair_rows = self.out[2].cpu().numpy()                  # (behind select()'s synchronise)
        assert all(len(k) > 100 for k, _ in self.rows) and (self.matches[1] > 100).all() and self.dim % 4 == 0

    def select(self, matches_cap=None):
        m, c, f, o = device_select(self.B, self.ctx, self.out, 2, self.SEL, matches_cap)    # (synchronises before the copy)
        return m[:int(o[-1])], c, f, o                              # the stored records, not the array's capacity

    def downloads(self, rows_cap, matches_cap, pinned):
        """queues one transfer of each exit; -> (HostResults, its ticket, HostMatches, its ticket)"""
        r, m = self.B.HostResults(self.n, rows_cap, self.dim, pinned=pinned), self.B.HostMatches(3, matches_cap, pinned=pinned)
        tr = self.ctx.batch_download_all(r)
        return r, tr, m, self.ctx.pair_matches_download(self.out, 2, self.B.MatchSelect(*self.SEL), m)

    def last_error(self):
        return self.ctx._L.brisk_hip_last_error(self.ctx._h).decode()

    def close(self):
        self.ext.close()
        self.ctx.close()


@pytest.mark.parametrize("pinned", [True, False])
def test_both_exits_in_flight(B, three_frames, pinned):
    """three transfers of rows and three of matches queued alternately without a wait, completed in reverse order of issue: each exit
    keeps its own two transfers in flight and counts its own tickets; pageable destinations go through both exits' bounce buffers"""
    X = BothExits(B, three_frames)
    ctx = X.ctx
    got = [X.downloads(X.nrows, X.nmatches, pinned) for _ in range(3)]
    assert [g[1] for g in got] == [1, 2, 3] and [g[3] for g in got] == [1, 2, 3]
    for i in (2, 1, 0):
        rc_m, flagged_m = ctx.pair_matches_wait(got[i][3], check=False)
        msg_m = X.last_error()
        rc_r, flagged_r = ctx.batch_download_wait(got[i][1], check=False)
        msg_r = X.last_error()
        if i == 0:                                                  # completed when the third transfer took the slot, then replaced
            assert (rc_m, rc_r) == (1, 1)
            assert msg_m.startswith("brisk_hip_pair_matches_wait: unknown ticket") and msg_r.startswith("brisk_hip_batch_download_wait: unknown ticket")
        else:
            assert (rc_m, flagged_m, rc_r, flagged_r) == (0, 0, 0, 0)
    for r, _, m, _ in got[1:]:
        assert np.array_equal(r.counts, [len(k) for k, _ in X.rows]) and not r.flags.any()
        assert np.array_equal(r.offsets, np.cumsum([0] + [len(k) for k, _ in X.rows]))
        for f in range(X.n):
            assert r.frame(f, X.dim)[0].tobytes() == X.rows[f][0].tobytes() and r.frame(f, X.dim)[1].tobytes() == X.rows[f][1].tobytes()
        same_selection(host_got(m, 3), X.matches)
        assert m.matches[:X.nmatches].tobytes() == X.matches[0][:X.nmatches].tobytes()
        assert np.array_equal(m.pair_rows, X.pair_rows)
    X.close()


@pytest.mark.parametrize("pinned", [True, False])
def test_both_exits_short_of_capacity(B, three_frames, pinned):
    """rows_cap and matches_cap one below what the batch needs, in both exits at once: each wait answers BRISK_HIP_ERR_CAPACITY with
    its own message and its own count of flagged entries"""
    X = BothExits(B, three_frames)
    ctx = X.ctx
    r, tr, m, tm = X.downloads(X.nrows - 1, X.nmatches - 1, pinned)
    assert (tr, tm) == (1, 1)
    want = X.select(matches_cap=X.nmatches - 1)                     # the last pair does not fit
    assert list(want[2] & ROWS_CUT) == [0, 0, ROWS_CUT]
    rc, flagged = ctx.pair_matches_wait(tm, check=False)
    assert (rc, flagged) == (4, int((want[2] != 0).sum())) and flagged >= 1
    assert "1 pair(s) did not fit the destination's matches_cap" in X.last_error()
    rc, flagged = ctx.batch_download_wait(tr, check=False)
    assert (rc, flagged) == (4, 1)                                  # the last frame does not fit
    assert "1 frame(s) did not fit the destination's rows_cap" in X.last_error()
    same_selection(host_got(m, 3), want)
    counts = [len(k) for k, _ in X.rows]
    assert np.array_equal(r.counts, counts) and list(r.flags) == [0, 0, ROWS_CUT]
    assert list(r.offsets) == [0, counts[0], counts[0] + counts[1], counts[0] + counts[1]]
    for f in range(2):                                              # the frames before the cut are in place
        assert r.frame(f, X.dim)[0].tobytes() == X.rows[f][0].tobytes() and r.frame(f, X.dim)[1].tobytes() == X.rows[f][1].tobytes()
    X.close()

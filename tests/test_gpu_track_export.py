"""GPU tests of the tracker's exit: brisk_hip_track_points_device (a list's observations -> points with their keypoints) and
brisk_hip_tracks_download / brisk_hip_tracks_wait (list + points + the transfer of the exact bytes to host memory).  The expectation
is always test_abi_tracks.restated_list on the restated link plus the numpy join test_abi_track_export.restated_points; every
array is compared as bytes, and destinations are pre-filled with the sentinel so that a write behind the stored prefixes shows."""
import ctypes as C

import numpy as np
import pytest

from gpu_prefill import settled
from test_abi_track_export import restated_points
from test_abi_tracks import SENT32, SENT64, restated_link, restated_list
from test_gpu_match_pairs import SENTINEL, batch_frames
from test_gpu_tracks import CAP, ROWS, Chain, make_chain, raw_link, raw_list

pytestmark = pytest.mark.gpu

SLACK = 16
PITCH = CAP * 28 + 4                       # no multiple of 28
STEPS = ((0, 1), (1, 2))                   # (kp_first, kp_step)


@pytest.fixture(scope="module")
def B():
    import ethzasl_brisk_amd as B
    from ethzasl_brisk_amd import build
    build.build()
    B.load_library()
    assert int(SENT32) == SENTINEL
    return B


@pytest.fixture(scope="module")
def ctx(B):
    c = B.Context(0)
    yield c
    c.close()


# ---- keypoints, destinations, calls -------------------------------------------------------------------------------------------

def kp_pattern(nwords):
    """a distinct bit pattern per dword (so per frame, row and word): quiet and signalling NaNs, negative values, small integers"""
    idx = np.arange(nwords, dtype=np.uint32)
    assert nwords < 2 ** 22
    top = np.array([0x7FC00000, 0x80000000, 0, 0xFF800000, 0x7F800000], np.uint32)[idx % 5]   # low bits non-zero: NaNs, not infinities
    return (idx + 1) | top


class Kps:
    """`frames` frames of keypoint records at PITCH on the device, every dword another bit pattern"""

    def __init__(self, B, frames, pitch=PITCH):
        import torch
        self.pitch, self.words = pitch, kp_pattern(frames * pitch // 4)
        self.d = torch.from_numpy(self.words.view(np.int32)).cuda()
        self.set = B.KpSet(self.d.data_ptr(), pitch)


class Dst:
    """destination arrays of brisk_hip_tracks_download with SLACK elements behind the capacities, sentinel everywhere.  kind:
    "pinned" (every array 16-byte aligned), "pinned+4" (points 4 bytes further: no 16-byte stores), "pageable" (numpy: the bounce
    buffer); null: NULL in place of the arrays a capacity of 0 leaves unused"""

    def __init__(self, B, tracks_cap, points_cap, kind="pinned", null=False):
        self.keep = []
        pinned = kind != "pageable"

        def arr(n, dtype, shift=0):
            raw = B._host_array((n + SLACK) * np.dtype(dtype).itemsize + 32, np.uint8, pinned, self.keep)
            raw[:] = 0x5A
            at = (-raw.ctypes.data) % 16 + shift
            return raw[at:at + (n + SLACK) * np.dtype(dtype).itemsize].view(dtype)
        self.summary, self.track, self.len = arr(4, np.int64), arr(tracks_cap, np.int64), arr(tracks_cap, np.int32)
        self.offsets = arr(tracks_cap + 1, np.int64)
        self.points = arr(points_cap, B.TRACK_POINT, 4 if kind == "pinned+4" else 0)
        assert self.points.ctypes.data % 16 == (4 if kind == "pinned+4" else 0) and self.track.ctypes.data % 16 == 0
        p = lambda a, unused: None if (null and unused) else a.ctypes.data                       # noqa: E731
        self.struct = B.HostTracks(tracks_cap, points_cap, self.summary.ctypes.data, p(self.track, tracks_cap == 0), p(self.len, tracks_cap == 0),
                                   self.offsets.ctypes.data, p(self.points, points_cap == 0))

    def untouched(self):
        return all((a.view(np.uint8) == 0x5A).all() for a in (self.summary, self.track, self.len, self.offsets, self.points))


def raw_download(ctx, ch, link_out, min_len, kps, kp_first, kp_step, dst, stream=None):
    t = C.c_uint(0xDEAD)
    rc = ctx._L.brisk_hip_tracks_download(ctx._h, ch.d_rows.data_ptr(), ch.stride, ch.nodes, ch.rows_cap, link_out[0].data_ptr(),
                                          link_out[1].data_ptr(), link_out[2].data_ptr(), int(min_len), C.byref(kps), kp_first, kp_step,
                                          C.byref(dst.struct), stream, C.byref(t))
    return rc, t.value


def raw_points(ctx, ch, lo, obs_cap, kps, kp_first, kp_step, points=None):
    """the device form on what raw_list returned; the points pre-filled"""
    import torch
    if points is None:
        points = settled(torch.full((obs_cap + SLACK, 9), SENTINEL, dtype=torch.int32, device="cuda"))
    rc = ctx._L.brisk_hip_track_points_device(ctx._h, ch.d_rows.data_ptr(), ch.stride, ch.nodes, ch.rows_cap, lo[2].data_ptr(), lo[3].data_ptr(),
                                              lo[4].data_ptr(), int(obs_cap), C.byref(kps), kp_first, kp_step, points.data_ptr(), None)
    return rc, points


def words(points):
    """TRACK_POINT records as rows of nine dwords"""
    return np.ascontiguousarray(points).view(np.uint32).reshape(-1, 9)


def same_points(B, got, want):
    """got: pre-filled TRACK_POINT records; the prefix is the join's, everything behind it still sentinel"""
    got = np.ascontiguousarray(got).view(np.uint32).reshape(-1, 9)
    w = want.view(np.uint32).reshape(-1, 9)
    if got[:len(w)].tobytes() != w.tobytes():
        bad = np.argwhere(got[:len(w)] != w)
        raise AssertionError(("points", len(bad), bad[:5].tolist(), got[tuple(bad[0])], w[tuple(bad[0])]))
    assert (got[len(w):] == np.uint32(SENTINEL)).all()


def same_download(B, dst, wl, wp):
    """the destination holds list `wl` (restated_list) and points `wp`, and nothing else"""
    wt, wlen, wo, wobs, ws = wl
    n, m = int(ws[2]), int(wo[-1])
    assert dst.summary[:4].tolist() == ws.tolist(), (dst.summary[:4], ws)
    assert (dst.summary[4:] == SENT64).all()
    assert dst.track[:n].tobytes() == wt.tobytes() and (dst.track[n:] == SENT64).all()
    assert dst.len[:n].tobytes() == wlen.tobytes() and (dst.len[n:] == SENT32).all()
    assert dst.offsets[:n + 1].tobytes() == wo.tobytes() and (dst.offsets[n + 1:] == SENT64).all()
    assert len(wp) == m and words(wp)[:, :2].tobytes() == wobs.tobytes()
    same_points(B, dst.points, wp)


def linked(B, ctx, nodes, seed, cap=CAP, node_rows=None, through=False, stride=1):
    """a hand-made chain, linked on the device; the restatement of the link"""
    node_rows = node_rows or (ROWS * 40)[:nodes]
    offsets, m = make_chain(B, seed, node_rows, through=through)
    ch = Chain(B, node_rows, cap, offsets, m, stride=stride)
    rc, out = raw_link(B, ctx, ch)
    assert rc == 0
    return ch, out, restated_link(node_rows, cap, offsets, m)


@pytest.fixture(scope="module")
def chain65(B, ctx):
    ch, out, want = linked(B, ctx, 65, 165, stride=3)
    return {"ch": ch, "out": out, "want": want, "kps": Kps(B, 1 + 64 * 2 + 1)}


# ---- 1: hand-made chains, both forms ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nodes", [1, 2, 3, 65])
def test_hand_made_chains(B, ctx, nodes, chain65):
    import torch
    if nodes == 65:
        ch, out, want, kps = (chain65[k] for k in ("ch", "out", "want", "kps"))
    else:
        ch, out, want = linked(B, ctx, nodes, 100 + nodes)
        kps = Kps(B, 1 + (nodes - 1) * 2 + 1)
    points_seen = 0
    for min_len in (1, 3):
        wl = restated_list(ch.node_rows, CAP, *want[:3], min_len)
        pieces, obs = int(wl[4][0]), int(wl[4][1])
        for kp_first, kp_step in STEPS:
            wp = restated_points(ch.node_rows, CAP, wl[3], kps.words, PITCH, kp_first, kp_step)
            # the device form on the list call's arrays
            rc, lo = raw_list(B, ctx, ch, out, min_len, pieces, obs)
            assert rc == 0
            rc, pts = raw_points(ctx, ch, lo, obs, kps.set, kp_first, kp_step)
            assert rc == 0, ctx._L.brisk_hip_last_error(ctx._h)
            torch.cuda.synchronize()
            dev = pts.cpu().numpy()
            same_points(B, dev.view(B.TRACK_POINT).reshape(-1), wp)
            # the download form: the same points
            dst = Dst(B, pieces, obs)
            rc, t = raw_download(ctx, ch, out, min_len, kps.set, kp_first, kp_step, dst)
            assert rc == 0 and t != 0, ctx._L.brisk_hip_last_error(ctx._h)
            assert ctx.tracks_wait(t) == 0
            same_download(B, dst, wl, wp)
            assert dst.points[:obs].tobytes() == dev[:obs].tobytes()
            points_seen += obs
            if obs:
                assert wp.view(np.uint32).reshape(-1, 9)[:, 2:].all()                       # every stored observation names a real row
    assert points_seen > (0 if nodes == 1 else 100) or nodes == 1
    if nodes == 65:                          # not vacuous: pieces over several nodes, a node beyond rows_cap, strided counts
        assert wl[1].max() >= 3 and pieces > 20 and max(ch.node_rows) > CAP and ch.stride == 3


# ---- 2: one track through 257 nodes -------------------------------------------------------------------------------------------

def test_one_track_through_257_nodes(B, ctx):
    nodes, cap = 257, 8
    ch, out, want = linked(B, ctx, nodes, 9, cap=cap, node_rows=[5] * nodes, through=True)
    pitch = cap * 28 + 4
    kps = Kps(B, nodes, pitch)
    wl = restated_list(ch.node_rows, cap, *want[:3], nodes)
    assert wl[4].tolist() == [1, nodes, 1, 0] and wl[1].tolist() == [nodes]
    wp = restated_points(ch.node_rows, cap, wl[3], kps.words, pitch, 0, 1)
    assert wp["node"].tolist() == list(range(nodes)) and wp["row"].tolist() == [i % 5 for i in range(nodes)]   # each point from another frame
    dst = Dst(B, 1, nodes)
    rc, t = raw_download(ctx, ch, out, nodes, kps.set, 0, 1, dst)
    assert rc == 0 and ctx.tracks_wait(t) == 0
    same_download(B, dst, wl, wp)


# ---- 3: the cut ---------------------------------------------------------------------------------------------------------------

def test_the_cut(B, ctx, chain65):
    ch, out, want, kps = (chain65[k] for k in ("ch", "out", "want", "kps"))
    full = restated_list(ch.node_rows, CAP, *want[:3], 2)
    pieces, obs = int(full[4][0]), int(full[4][1])
    assert pieces > 20
    for tcap, pcap, null in ((pieces, obs, False), (pieces - 1, obs, False), (pieces, obs - 1, False), (0, obs, True), (pieces, 0, True),
                             (0, 0, True), (0, 0, False)):
        wl = restated_list(ch.node_rows, CAP, *want[:3], 2, tcap, pcap)
        wp = restated_points(ch.node_rows, CAP, wl[3], kps.words, PITCH, 1, 2)
        dst = Dst(B, tcap, pcap, null=null)
        rc, t = raw_download(ctx, ch, out, 2, kps.set, 1, 2, dst)
        assert rc == 0, (tcap, pcap, ctx._L.brisk_hip_last_error(ctx._h))
        rc, cut = ctx.tracks_wait(t, check=False)
        is_cut = tcap < pieces or pcap < obs
        assert (rc, cut) == ((4, 1) if is_cut else (0, 0)), (tcap, pcap)
        if is_cut:
            assert b"TRACKS_CUT" in ctx._L.brisk_hip_last_error(ctx._h)
        assert wl[4].tolist() == [pieces, obs, int(wl[4][2]), int(is_cut)] and int(wl[4][3]) == B.TRACKS_CUT * is_cut
        same_download(B, dst, wl, wp)                                    # the stored pieces are in place, the true counts reported
        assert ctx.tracks_wait(t, check=False) == (rc, cut)              # waiting twice: the same answer


# ---- 4: destinations ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["pinned", "pinned+4", "pageable"])
def test_destinations(B, ctx, chain65, kind):
    ch, out, want, kps = (chain65[k] for k in ("ch", "out", "want", "kps"))
    full = restated_list(ch.node_rows, CAP, *want[:3], 1)
    pieces, obs = int(full[4][0]), int(full[4][1])
    odd = max(t for t in range(pieces + 1) if int(full[2][t]) * 9 % 4 != 0)       # points whose dword count is no multiple of 4 ...
    even = max(t for t in range(pieces + 1) if int(full[2][t]) * 9 % 4 == 0 and full[2][t] > 0)   # ... and one that is
    for tcap in (pieces, odd, even):
        wl = restated_list(ch.node_rows, CAP, *want[:3], 1, tcap, obs)
        wp = restated_points(ch.node_rows, CAP, wl[3], kps.words, PITCH, 0, 1)
        dst = Dst(B, tcap, obs, kind)
        rc, t = raw_download(ctx, ch, out, 1, kps.set, 0, 1, dst)
        assert rc == 0
        assert ctx.tracks_wait(t, check=False) == ((4, 1) if tcap < pieces else (0, 0))
        same_download(B, dst, wl, wp)
        assert len(wp) > 100
    assert (int(full[2][odd]) * 9) % 4 != 0


# ---- 5: the ring --------------------------------------------------------------------------------------------------------------

def test_three_downloads_in_flight(B, ctx, chain65):
    import torch
    ch, out, want, kps = (chain65[k] for k in ("ch", "out", "want", "kps"))
    torch.cuda.synchronize()
    jobs = []
    for min_len, kind, (kp_first, kp_step) in ((1, "pageable", STEPS[0]), (2, "pinned", STEPS[1]), (3, "pinned+4", STEPS[0])):
        wl = restated_list(ch.node_rows, CAP, *want[:3], min_len)
        dst = Dst(B, int(wl[4][0]), int(wl[4][1]), kind)
        jobs.append((wl, restated_points(ch.node_rows, CAP, wl[3], kps.words, PITCH, kp_first, kp_step), dst, (min_len, kp_first, kp_step)))
    tickets = []
    for wl, wp, dst, (min_len, kp_first, kp_step) in jobs:                  # issued before any wait: the third completes the first
        rc, t = raw_download(ctx, ch, out, min_len, kps.set, kp_first, kp_step, dst)
        assert rc == 0
        tickets.append(t)
    assert len(set(tickets)) == 3 and 0 not in tickets
    assert ctx.tracks_wait(tickets[2]) == 0                                  # waits in reverse order
    assert ctx.tracks_wait(tickets[1]) == 0
    for wl, wp, dst, _ in jobs:
        same_download(B, dst, wl, wp)
    assert jobs[0][0][4][0] > jobs[1][0][4][0] > jobs[2][0][4][0] > 0        # three different lists
    rc, _ = ctx.tracks_wait(tickets[0], check=False)
    assert rc == 1                                                           # its slot went to the third transfer: as in the other exits
    rc, cut = ctx.tracks_wait(tickets[2] + 1000, check=False)
    assert (rc, cut) == (1, 0)                                               # a ticket never issued
    assert ctx._L.brisk_hip_tracks_wait(ctx._h, 0, None) == 1


# ---- 6: wide addresses --------------------------------------------------------------------------------------------------------

def test_keypoints_beyond_four_gib(B, ctx):
    import torch
    nodes, cap, pitch = 5, 8, 2 ** 30 + 4
    node_rows = [5, 3, 8, 9, 2]
    ch, out, want = linked(B, ctx, nodes, 77, cap=cap, node_rows=node_rows)
    big = torch.empty(nodes * pitch, dtype=torch.uint8, device="cuda")      # 5 GiB, uninitialised: only the rows used are filled
    rows = {}
    for i, n in enumerate(node_rows):
        lim = min(n, cap)
        rows[i] = ((np.arange(lim * 7, dtype=np.uint32) + 1) * np.uint32(2654435761)) ^ np.uint32(0x01010101 * (i + 1))
        big[i * pitch:i * pitch + lim * 28] = torch.from_numpy(rows[i].view(np.uint8).copy()).cuda()
    settled(big)                                                            # the rows are in place before a call reads them

    def kp_words(first, n):
        i, at = divmod(first * 4, pitch)
        assert at % 4 == 0 and at // 4 + n <= len(rows[i])
        return rows[i][at // 4:at // 4 + n]
    kset = B.KpSet(big.data_ptr(), pitch)
    wl = restated_list(node_rows, cap, *want[:3], 1)
    pieces, obs = int(wl[4][0]), int(wl[4][1])
    wp = restated_points(node_rows, cap, wl[3], kp_words, pitch, 0, 1)
    assert (wl[3]["node"] == 4).any() and 4 * pitch > 2 ** 32 and obs == sum(min(n, cap) for n in node_rows)
    rc, lo = raw_list(B, ctx, ch, out, 1, pieces, obs)
    assert rc == 0
    rc, pts = raw_points(ctx, ch, lo, obs, kset, 0, 1)
    assert rc == 0
    torch.cuda.synchronize()
    same_points(B, pts.cpu().numpy().view(B.TRACK_POINT).reshape(-1), wp)
    dst = Dst(B, pieces, obs)
    rc, t = raw_download(ctx, ch, out, 1, kset, 0, 1, dst)
    assert rc == 0 and ctx.tracks_wait(t) == 0
    same_download(B, dst, wl, wp)
    del big


# ---- 7: the device form on a caller's list --------------------------------------------------------------------------------------

def test_observations_that_name_no_keypoint(B, ctx):
    import torch
    node_rows = [65, 0, 1, 131]
    nodes = len(node_rows)
    ch = Chain(B, node_rows, CAP, np.zeros(nodes, np.int64), np.zeros(0, B.DMATCH))
    kps = Kps(B, 2 + 3 * 2)
    obs = np.array([(0, 0), (-1, 0), (nodes, 0), (0, 65), (0, -1), (0, 64), (1, 0), (2, 0), (2, 1), (3, CAP - 1), (3, CAP), (3, 130),
                    (-2 ** 31, 5), (2 ** 31 - 1, 5), (2, -2 ** 31), (2, 2 ** 31 - 1), (3, 0)], B.TRACK_OBS)
    n = len(obs)
    for kp_first, kp_step in STEPS:
        want = restated_points(node_rows, CAP, obs, kps.words, PITCH, kp_first, kp_step)
        real = want.view(np.uint32).reshape(-1, 9)[:, 2:].any(axis=1)
        assert real.tolist() == [True, False, False, False, False, True, False, True, False, True, False, False, False, False, False, False, True]
        lo = (None, None, torch.tensor([0, 3, n], dtype=torch.int64, device="cuda"),
              torch.from_numpy(np.concatenate([obs, np.zeros(9, B.TRACK_OBS)]).view(np.int32).reshape(-1, 2).copy()).cuda(),
              torch.tensor([2, n, 2, 0], dtype=torch.int64, device="cuda"))
        rc, pts = raw_points(ctx, ch, lo, n + 9, kps.set, kp_first, kp_step)
        assert rc == 0
        torch.cuda.synchronize()
        same_points(B, pts.cpu().numpy().view(B.TRACK_POINT).reshape(-1), want)     # and nothing behind the count, capacity or not


# ---- 5 / 8: the real path, the three rings side by side -----------------------------------------------------------------------

@pytest.fixture(scope="module")
def real(B, golden_ast):
    """detect + describe, k = 2 matching, selection (ratio 0.8), link and the tracks' download on one stream; the matches' and the
    rows' downloads in flight beside it; the list call for comparison"""
    import torch
    frames = batch_frames(golden_ast)
    n, h, w = frames.shape
    d = torch.from_numpy(frames).cuda()
    ctx = B.Context(0)
    ext = B.BriskDescriptorExtractor(context=ctx)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    ctx.detect_describe_batch(ext, d.data_ptr(), n, w, h, w * h, w, 70, 2, s.cuda_stream)
    st, dim = ctx.batch_desc_set()
    triple = ctx.match_knn_pairs(st, st, B.PairSpec(n - 1, 1, 1, 0, 1, None), 2, stream=s.cuda_stream)
    rows_cap = int(triple[1].shape[1])
    sel = B.MatchSelect(float("inf"), 0.8, 1)
    matches, counts, flags, offsets = ctx.select_pair_matches(triple, 2, sel, stream=s.cuda_stream)
    hm = B.HostMatches(n - 1, (n - 1) * rows_cap)
    tm = ctx.pair_matches_download(triple, 2, sel, hm, stream=s.cuda_stream)
    hr = B.HostResults(n, n * rows_cap, 48)
    tr = ctx.batch_download_all(hr, stream=s.cuda_stream)
    lk = ctx.link_tracks((st, 0, 1), n, rows_cap, offsets, matches, stream=s.cuda_stream)
    ht = B.HostTrackList(n * rows_cap, n * rows_cap)
    for a in (ht.summary, ht.track, ht.len, ht.offsets, ht.points):
        a.view(np.uint8)[:] = 0x5A
    tt = ctx.tracks_download((st, 0, 1), n, rows_cap, *lk[:3], 3, ht, stream=s.cuda_stream)     # kps: the batch's own
    listed = ctx.list_tracks((st, 0, 1), n, rows_cap, *lk[:3], 3, stream=s.cuda_stream)
    pts = ctx.track_points((st, 0, 1), n, rows_cap, listed[2], listed[3], listed[4], stream=s.cuda_stream)
    # one transfer of each exit is outstanding: every wait succeeds, in any order
    assert ctx.tracks_wait(tt) == 0
    assert ctx.batch_download_wait(tr) == 0
    assert ctx.pair_matches_wait(tm) == 0
    torch.cuda.synchronize()
    assert ctx.batch_status(n) == 0
    r = {"n": n, "ht": ht, "hm": hm, "hr": hr, "dim": dim, "listed": tuple(t.cpu().numpy() for t in listed), "pts": pts.cpu().numpy(),
         "kd": [ctx.batch_download(f, True, strings=dim) for f in range(n)], "sel": (matches.cpu().numpy(), offsets.cpu().numpy())}
    ext.close()
    ctx.close()
    return r


def test_the_real_path(B, real):
    ht, (lt, ll, lo, lobs, ls) = real["ht"], real["listed"]
    pieces, obs = int(ls[2]), int(lo[int(ls[2])])
    assert ls[3] == 0 and pieces > 10 and obs >= 3 * pieces
    # the list arrays equal list_tracks' arrays, nothing behind them is written
    assert ht.summary.tolist() == ls.tolist() and ht.stored == pieces
    assert ht.track[:pieces].tobytes() == lt[:pieces].tobytes() and (ht.track[pieces:] == SENT64).all()
    assert ht.len[:pieces].tobytes() == ll[:pieces].tobytes() and (ht.len[pieces:] == SENT32).all()
    assert ht.offsets[:pieces + 1].tobytes() == lo[:pieces + 1].tobytes() and (ht.offsets[pieces + 1:] == SENT64).all()
    assert words(ht.points[:obs])[:, :2].tobytes() == lobs[:obs].tobytes()
    assert (ht.points[obs:].view(np.uint8) == 0x5A).all()
    # every point's keypoint, byte for byte, is batch_download's record of its frame and row
    for p, w in zip(ht.points[:obs], words(ht.points[:obs])):
        k = real["kd"][int(p["node"])][0][int(p["row"])]
        assert w[2:].tobytes() == k.tobytes(), p
    assert ht.points[:obs].tobytes() == real["pts"][:obs].tobytes()              # the device form: the same points
    t, n, pts = ht.piece(0)
    assert n >= 3 and len(pts) == int(lo[1]) and t == lt[0]


def test_the_three_rings_side_by_side(B, real):
    """the matches' and the rows' transfers that were in flight beside the tracks' arrived whole"""
    n, hm, hr, dim = real["n"], real["hm"], real["hr"], real["dim"]
    m, o = real["sel"]
    assert hm.offsets[:n].tobytes() == o.tobytes() and o[-1] > 100
    assert hm.matches[:int(o[-1])].tobytes() == m[:int(o[-1])].tobytes()
    for f in range(n):
        assert hr.frame(f, dim)[0].tobytes() == real["kd"][f][0].tobytes() and np.array_equal(hr.frame(f, dim)[1], real["kd"][f][1])


# ---- 9: arguments -------------------------------------------------------------------------------------------------------------

def test_arguments(B, ctx):
    import torch
    ch, out, want = linked(B, ctx, 3, 103, node_rows=[65, 7, 63])
    kps = Kps(B, 6)
    L, h = ctx._L, ctx._h
    dst = Dst(B, 50, 200)
    ticket = C.c_uint(0xDEAD)

    def kset(ptr=kps.d.data_ptr(), pitch=PITCH):
        return C.byref(B.KpSet(ptr, pitch))

    def host(**kw):
        f = dict(tracks_cap=50, points_cap=200, summary=dst.summary.ctypes.data, track=dst.track.ctypes.data, len=dst.len.ctypes.data,
                 offsets=dst.offsets.ctypes.data, points=dst.points.ctypes.data)
        f.update(kw)
        return C.byref(B.HostTracks(*(f[k] for k, _ in B.HostTracks._fields_)))
    good = [ch.d_rows.data_ptr(), 1, 3, CAP, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), 2, kset(), 1, 2, host(), None,
            C.byref(ticket)]
    S = dst.struct
    bad = [(2, 0), (3, 0), (1, 0), (0, None), (0, good[0] + 2),                                  # the chain's errors
           (4, None), (5, None), (6, None), (5, good[5] + 4), (4, good[4] + 2), (6, good[6] + 1), (7, 0), (7, -3),   # the list call's
           (11, host(tracks_cap=-1)), (11, host(points_cap=-1)),
           (8, None), (11, None), (8, kset(ptr=None)), (8, kset(ptr=kps.d.data_ptr() + 2)), (8, kset(pitch=-PITCH)), (8, kset(pitch=PITCH + 2)),
           (9, -1), (10, -1),                                                                    # frames 1, 0, -1
           (11, host(summary=None)), (11, host(track=None)), (11, host(len=None)), (11, host(offsets=None)), (11, host(points=None)),
           (11, host(tracks_cap=0, track=None, len=None, offsets=None)),
           (11, host(summary=S.summary + 4)), (11, host(track=S.track + 4)), (11, host(offsets=S.offsets + 4)), (11, host(len=S.len + 2)),
           (11, host(points=S.points + 2))]
    for at, v in bad:
        a = list(good)
        a[at] = v
        ticket.value = 0xDEAD
        assert L.brisk_hip_tracks_download(h, *a) == 1, (at, v)
        assert ticket.value == 0, (at, v)
    a = list(good)
    a[13] = None
    assert L.brisk_hip_tracks_download(h, *a) == 1                       # no ticket
    assert L.brisk_hip_tracks_download(None, *good) == 1
    torch.cuda.synchronize()
    assert dst.untouched()                                               # nothing was launched, nothing written
    # the device form
    rc, lo = raw_list(B, ctx, ch, out, 2, 50, 200)
    assert rc == 0
    pts = settled(torch.full((200 + SLACK, 9), SENTINEL, dtype=torch.int32, device="cuda"))
    gdev = [ch.d_rows.data_ptr(), 1, 3, CAP, lo[2].data_ptr(), lo[3].data_ptr(), lo[4].data_ptr(), 200, kset(), 1, 2, pts.data_ptr(), None]
    bad = [(2, 0), (3, 0), (1, 0), (0, None), (0, gdev[0] + 2), (4, None), (5, None), (6, None), (7, -1), (11, None),
           (4, gdev[4] + 4), (5, gdev[5] + 4), (6, gdev[6] + 4), (11, gdev[11] + 2),
           (8, None), (8, kset(ptr=None)), (8, kset(ptr=kps.d.data_ptr() + 2)), (8, kset(pitch=-PITCH)), (8, kset(pitch=PITCH + 2)), (9, -1), (10, -1)]
    for at, v in bad:
        a = list(gdev)
        a[at] = v
        assert L.brisk_hip_track_points_device(h, *a) == 1, (at, v)
    assert L.brisk_hip_track_points_device(None, *gdev) == 1
    torch.cuda.synchronize()
    assert (pts.cpu().numpy() == SENTINEL).all()
    # what is valid: a negative step whose frames stay at or above 0, NULL arrays behind a capacity of zero - and the good calls themselves
    wl = restated_list(ch.node_rows, CAP, *want[:3], 2)
    assert 0 < wl[4][0] <= 50 and 0 < wl[4][1] <= 200
    a = list(gdev)
    a[9], a[10] = 2, -1
    assert L.brisk_hip_track_points_device(h, *a) == 0
    torch.cuda.synchronize()
    same_points(B, pts.cpu().numpy().view(B.TRACK_POINT).reshape(-1), restated_points(ch.node_rows, CAP, wl[3], kps.words, PITCH, 2, -1))
    a = list(gdev)
    a[5], a[7], a[11] = None, 0, None
    lo0 = raw_list(B, ctx, ch, out, 2, 50, 0)[1]
    a[4], a[6] = lo0[2].data_ptr(), lo0[4].data_ptr()
    assert L.brisk_hip_track_points_device(h, *a) == 0
    assert L.brisk_hip_tracks_download(h, *good) == 0 and ticket.value != 0
    assert ctx.tracks_wait(ticket.value) == 0
    same_download(B, dst, wl, restated_points(ch.node_rows, CAP, wl[3], kps.words, PITCH, 1, 2))

"""GPU tests of the feature tracker and its exit where counts get wide (the chains: tests/track_wide_cases.py, their conditions
asserted without a GPU in tests/test_track_wide_cases.py):
  1  65 535, 65 536 and 65 537 nodes: the second trip of the twelve node loops of brisk_track.hip, cut before node 65 535, before
     pair 65 535 and before node 65 536; walks that start in one launch's nodes and store into the next launch's
  2  the 65 537-node chain linked in two calls that meet at node 65 534, 65 535 or 65 536
  3  about 70 000 rows per node: more records in a pair than k_track_propose / k_track_resolve have lanes (the second trip of their
     record loops, the record before a workgroup's and a trip's first), rows, train rows and seeds >= 65 536 (blockIdx.x >= 256), and
     more points than one trip of k_tracklist_points (point 29 127 lies across the trips)
  4  list capacities that end exactly on a workgroup's running total of pieces or observations
  5  gpu_prefill.settled, which orders the tests' sentinel fills in front of the calls they guard
The method is test_gpu_tracks.py's and test_gpu_track_export.py's: the expectation is restated_link / restated_list / restated_points
on the host copies of the inputs, every output is pre-filled with the sentinel with slack behind its capacity, every array is
compared as bytes.

Deliberate changes, each applied alone to a scratch copy of the kernels and run once on an MI355X (this file and the three
existing tracker files test_gpu_tracks.py, test_gpu_track_export.py, test_gpu_stream_order.py):
  change                                               fails here                                               existing files
  1 k_track_number: node = blockIdx.y                  node_chunks[65536, 65537], the python calls,             pass
                                                       split[65535, 65536] (first calls of 65 536 / 65 537 nodes)
  2 k_track_list_next: node = 1 + blockIdx.y           node_chunks[65537], the python calls                     pass
  3 k_track_propose: one trip                          the row-wide link (the `wide` fixture: 9 839 cells of    pass
                                                       prev differ), so all four tests that use it error
  4 tk_proposal: before = 0 at (j - o0) % 256 == 0     the row-wide link (151 cells of prev differ), as above   test_gpu_tracks.py::test_more_workgroup_
                                                                                                                sums_than_the_offsets_kernel_has_threads
                                                                                                                fails too (71 cells): not "all pass"
  5 k_tracklist_points: one trip                       node_chunks[all three], the python calls,                pass
                                                       rows_wide_lists[2] (192 000 and 99 190 points)
Changes 1 and 2 fail nothing but the node cases, 3 and 4 nothing here but the row-wide link, 5 nothing but points and download.
"""
import time

import numpy as np
import pytest

import track_wide_cases as W
from gpu_prefill import settled
from test_abi_track_export import restated_points
from test_abi_tracks import SENT32, SENT64, restated_link
from test_gpu_match_pairs import SENTINEL
from test_gpu_track_export import Dst, Kps, raw_download, raw_points, same_download, same_points, words
from test_gpu_tracks import CAP, ROWS, Chain, host, make_chain, raw_link, raw_list, same_link, same_list, sentinel_link_outputs

pytestmark = pytest.mark.gpu


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


class Clock:
    """wall time of the device work between marks (the device idle at each), printed with the test's output"""

    def __init__(self, what):
        import torch
        self.torch, self.what, self.parts = torch, what, []
        torch.cuda.synchronize()
        self.t = time.perf_counter()

    def mark(self, name):
        self.torch.cuda.synchronize()
        now = time.perf_counter()
        self.parts.append("%s %.1f ms" % (name, (now - self.t) * 1e3))
        self.t = now

    def restart(self):
        self.torch.cuda.synchronize()
        self.t = time.perf_counter()

    def show(self):
        print("\n%s: %s" % (self.what, ", ".join(self.parts)))


def device_seed(case, first_new=W.FIRST_NEW):
    import torch
    return settled(torch.from_numpy(case.st).cuda(), torch.from_numpy(case.sa).cuda()) + (first_new, None)


def link_and_compare(B, ctx, ch, want, seed, clock, name):
    out = sentinel_link_outputs(ch.nodes, ch.rows_cap)
    clock.restart()
    rc, out = raw_link(B, ctx, ch, seed, out=settled(*out))
    assert rc == 0, ctx._L.brisk_hip_last_error(ctx._h)
    clock.mark(name)
    same_link(host(out), want)
    return out


def list_and_compare(B, ctx, ch, link_out, want, min_len, tracks_cap, obs_cap, clock=None, name=None):
    if clock:
        clock.restart()
    rc, lo = raw_list(B, ctx, ch, link_out, min_len, tracks_cap, obs_cap)
    assert rc == 0, (tracks_cap, obs_cap, ctx._L.brisk_hip_last_error(ctx._h))
    if clock:
        clock.mark(name)
    same_list(B, host(lo), want)
    return lo


def points_and_download(B, ctx, ch, link_out, lo, wl, min_len, kps, pitch, clock):
    """the device form on the list `lo` and the download form: both hold restated_points of the restated list `wl`"""
    import torch
    pieces, obs = int(wl[4][0]), int(wl[4][1])
    wp = restated_points(ch.node_rows, ch.rows_cap, wl[3], kps.words, pitch, 0, 1)
    clock.restart()
    rc, pts = raw_points(ctx, ch, lo, obs, kps.set, 0, 1)
    assert rc == 0, ctx._L.brisk_hip_last_error(ctx._h)
    clock.mark("points (%d)" % obs)
    dev = pts.cpu().numpy()
    same_points(B, dev.view(B.TRACK_POINT).reshape(-1), wp)
    dst = Dst(B, pieces, obs)
    torch.cuda.synchronize()
    clock.restart()
    rc, t = raw_download(ctx, ch, link_out, min_len, kps.set, 0, 1, dst)
    assert rc == 0 and t != 0, ctx._L.brisk_hip_last_error(ctx._h)
    assert ctx.tracks_wait(t) == 0
    clock.mark("download")
    same_download(B, dst, wl, wp)
    assert dst.points[:obs].tobytes() == dev[:obs].tobytes()
    return wp, dev


# ---- 1: more nodes than one launch ------------------------------------------------------------------------------------------------

NODE_PITCH = W.NODE_CAP * 28 + 4


@pytest.fixture(scope="module")
def node_kps(B):
    return Kps(B, W.NODES, NODE_PITCH)


def node_chain(B, case, nodes):
    return Chain(B, case.node_rows[:nodes], case.rows_cap, case.offsets[:nodes].copy(), case.matches)


@pytest.mark.parametrize("nodes", W.NODE_LENGTHS)
def test_node_chunks(B, ctx, node_kps, nodes):
    case = W.node_case(B)
    ch = node_chain(B, case, nodes)
    clock = Clock("%d nodes" % nodes)
    out = link_and_compare(B, ctx, ch, case.link(nodes), None, clock, "link")
    link_and_compare(B, ctx, ch, case.link(nodes, seeded=True), device_seed(case), clock, "link seeded")
    for min_len in W.NODE_MIN_LENS:
        wl = case.list(min_len, nodes)
        lo = list_and_compare(B, ctx, ch, out, wl, min_len, int(wl[4][0]), int(wl[4][1]), clock, "list min_len %d" % min_len)
    assert wl[1].max() == nodes and int(wl[4][0]) > 10000                   # the through-track among the listed pieces
    points_and_download(B, ctx, ch, out, lo, wl, W.NODE_MIN_LENS[-1], node_kps, NODE_PITCH, clock)
    clock.show()


def test_node_chunks_through_the_python_calls(B, ctx, node_kps):
    """Context.link_tracks, list_tracks and tracks_download on the 65 537 nodes: the same arrays where they write"""
    import torch
    case = W.node_case(B)
    nodes, cap = W.NODES, W.NODE_CAP
    ch = node_chain(B, case, nodes)
    want, wl = case.link(), case.list(3)
    got = ctx.link_tracks((ch.d_rows, ch.stride), nodes, cap, ch.d_offsets, ch.d_matches)
    listed = ctx.list_tracks((ch.d_rows, ch.stride), nodes, cap, *got[:3], 3)
    pieces, obs = int(wl[4][0]), int(wl[4][1])
    ht = B.HostTrackList(pieces + 16, obs + 16)
    for a in (ht.summary, ht.track, ht.len, ht.offsets, ht.points):
        a.view(np.uint8)[:] = 0x5A
    ticket = ctx.tracks_download((ch.d_rows, ch.stride), nodes, cap, *got[:3], 3, ht, kps=node_kps.set)
    assert ctx.tracks_wait(ticket) == 0
    torch.cuda.synchronize()
    got, listed = tuple(t.cpu().numpy() for t in got), tuple(t.cpu().numpy() for t in listed)
    wrote = want[0] != SENT32
    for name, g, w in zip(("prev", "track", "age"), got, want):
        assert np.array_equal(g[wrote], w[wrote]), name
    assert got[3].tolist() == want[3].tolist()
    assert listed[4].tolist() == wl[4].tolist()
    assert listed[0][:pieces].tobytes() == wl[0].tobytes() and listed[1][:pieces].tobytes() == wl[1].tobytes()
    assert listed[2][:pieces + 1].tobytes() == wl[2].tobytes() and listed[3][:obs].tobytes() == wl[3].tobytes()
    wp = restated_points(ch.node_rows, cap, wl[3], node_kps.words, NODE_PITCH, 0, 1)
    assert ht.summary.tolist() == wl[4].tolist() and ht.stored == pieces
    assert ht.track[:pieces].tobytes() == wl[0].tobytes() and (ht.track[pieces:] == SENT64).all()
    assert ht.len[:pieces].tobytes() == wl[1].tobytes() and (ht.len[pieces:] == SENT32).all()
    assert ht.offsets[:pieces + 1].tobytes() == wl[2].tobytes() and (ht.offsets[pieces + 1:] == SENT64).all()
    assert ht.points[:obs].tobytes() == wp.tobytes() and (ht.points[obs:].view(np.uint8) == 0x5A).all()


# ---- 2: one chain in two calls across the seam ------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", W.SPLITS)
def test_a_chain_split_in_two_calls_across_the_seam(B, ctx, m):
    """test_gpu_tracks.test_a_chain_split_in_two_calls on the 65 537 nodes: nodes [0, m], then [m, nodes) seeded with node m's rows of
    the first call and its next_new through the device word, no synchronisation in between"""
    case = W.node_case(B)
    want = case.link(seeded=True)
    st, sa, first_new, _ = device_seed(case)
    first = node_chain(B, case, m + 1)
    second = Chain(B, case.node_rows[m:], case.rows_cap, case.offsets[m:].copy(), case.matches)
    o1, o2 = sentinel_link_outputs(first.nodes, first.rows_cap), sentinel_link_outputs(second.nodes, second.rows_cap)
    settled(*(o1 + o2))
    rc, o1 = raw_link(B, ctx, first, (st, sa, first_new, None), out=o1)
    assert rc == 0
    rc, o2 = raw_link(B, ctx, second, (o1[1][m], o1[2][m], -1, o1[3]), out=o2)
    assert rc == 0
    h1, h2 = host(o1), host(o2)
    assert h1[1].tobytes() == want[1][:m + 1].tobytes() and h1[2].tobytes() == want[2][:m + 1].tobytes()
    assert h1[0].tobytes() == want[0][:m + 1].tobytes()
    assert h2[1].tobytes() == want[1][m:].tobytes() and h2[2].tobytes() == want[2][m:].tobytes()
    assert h2[0][1:].tobytes() == want[0][m + 1:].tobytes()
    assert h2[3][0] == want[3][0] and h1[3][1] + h2[3][1] == want[3][1] and h1[3][2] + h2[3][2] == want[3][2]
    assert h1[3][0] > W.FIRST_NEW + 100000


# ---- 3: rows wide -------------------------------------------------------------------------------------------------------------------

WIDE_PITCH = W.WIDE_CAP * 28 + 4


@pytest.fixture(scope="module")
def wide(B, ctx):
    """the row-wide chain on the device, linked without and with the seeds: both results are the restatement's"""
    case = W.wide_case(B)
    ch = Chain(B, case.node_rows, case.rows_cap, case.offsets, case.matches)
    clock = Clock("rows wide (%d and %d records)" % (case.offsets[1], case.offsets[2] - case.offsets[1]))
    plain = link_and_compare(B, ctx, ch, case.link(), None, clock, "link")
    seeded = link_and_compare(B, ctx, ch, case.link(seeded=True), device_seed(case), clock, "link seeded")
    clock.show()
    return {"case": case, "ch": ch, "plain": plain, "seeded": seeded, "kps": Kps(B, 3, WIDE_PITCH)}


def test_rows_wide_link(B, wide):
    """(the comparison is the fixture's) what the compared arrays hold"""
    case = wide["case"]
    got = host(wide["plain"])
    (qw, tw), (qa, ta), (qb, tb) = (case.hand[k] for k in ("win", "tie_a", "tie_b"))
    assert got[0][2, qw] == tw >= 65536 and got[0][2, qa] == ta >= 65536 and got[0][2, qb] == -1 and qb > qa >= 65536
    assert got[3][3] > 40000 and got[3][4] > 40000
    seeded = host(wide["seeded"])
    assert (seeded[1][0, 65536:] == case.st[65536:]).sum() > 1000 and seeded[3][0] > W.FIRST_NEW


@pytest.mark.parametrize("min_len", W.WIDE_MIN_LENS)
def test_rows_wide_lists(B, ctx, wide, min_len):
    case, ch = wide["case"], wide["ch"]
    clock = Clock("rows wide, min_len %d" % min_len)
    for seeded in (True, False):
        wl = case.list(min_len, seeded=seeded)
        lo = list_and_compare(B, ctx, ch, wide["seeded" if seeded else "plain"], wl, min_len, int(wl[4][0]), int(wl[4][1]), clock,
                              "list%s" % (" seeded" if seeded else ""))
    if min_len == W.WIDE_MIN_LENS[-1]:                                   # points of the unseeded list: more than one trip
        obs = int(wl[4][1])
        assert obs > W.POINTS_PER_TRIP + 1
        wp, dev = points_and_download(B, ctx, ch, wide["plain"], lo, wl, min_len, wide["kps"], WIDE_PITCH, clock)
        at = W.POINTS_PER_TRIP                                           # word 0 in the first trip, words 1 .. 8 in the second
        assert dev[at].view(np.uint32).tolist() == words(wp)[at].tolist() and words(wp)[at][2:].all()
        assert dev[at - 1].view(np.uint32).tolist() == words(wp)[at - 1].tolist()
    clock.show()


# ---- 4: the cut at workgroup seams ------------------------------------------------------------------------------------------------

def test_the_cut_at_workgroup_seams(B, ctx, wide):
    """tracks_cap, then obs_cap, on the running total before a workgroup, one piece into it, one piece before its end and at its
    end, for three workgroups; once both bind.  The stored prefix is the restatement's, the sentinel behind it, the summary carries
    the true totals with the cut flag."""
    case, ch = wide["case"], wide["ch"]
    full = case.list(2)
    pieces, obs = int(full[4][0]), int(full[4][1])
    cut = 0
    for tracks_cap, obs_cap, what in case.cuts:
        w = case.list(2, tracks_cap=tracks_cap, obs_cap=obs_cap)
        list_and_compare(B, ctx, ch, wide["plain"], w, 2, tracks_cap, obs_cap)
        assert w[4][:2].tolist() == [pieces, obs] and int(w[4][3]) == (int(w[4][2]) < pieces), what
        cut += int(w[4][3])
    assert 18 <= cut < len(case.cuts) == 25


# ---- 5: the helper that orders the pre-fills --------------------------------------------------------------------------------------

def test_settled_orders_a_prefill(B, ctx):
    """the null stream held by a bounded spin kernel, a sentinel fill queued behind it: settled() returns when the hold is over and
    the fill has landed, and the link call issued then - on the context's own stream, which does not wait for the null stream - gives
    the restatement's bytes.  (Without settled() the call overtakes the fill and the sentinel comes back over its results.)"""
    import types

    import torch
    from test_gpu_stream_order import HOLD_MIN_MS, timed_sleep
    node_rows = ROWS[:8]
    offsets, m = make_chain(B, 3, node_rows)
    ch = Chain(B, node_rows, CAP, offsets, m)
    want = restated_link(node_rows, CAP, offsets, m)
    out = (torch.empty((8, CAP), dtype=torch.int32, device="cuda"), torch.empty((8, CAP), dtype=torch.int64, device="cuda"),
           torch.empty((8, CAP), dtype=torch.int32, device="cuda"), torch.empty((8,), dtype=torch.int64, device="cuda"))
    e = types.SimpleNamespace(torch=torch, S=torch.cuda.default_stream())
    timed_sleep(e, 1000)
    small = max(timed_sleep(e, 1000000), 1e-3)
    cycles = int(1000000 * 2.0 * HOLD_MIN_MS / small)                 # about 200 ms
    torch.cuda.synchronize()
    behind = torch.cuda.Event()
    torch.cuda._sleep(cycles)
    for t, v in zip(out, (SENT32, SENT64, SENT32, SENT64)):
        t.fill_(int(v))
    behind.record()
    pending = not behind.query()
    assert settled(*out) is not None
    assert behind.query(), "settled() returned while the null stream was still held"
    assert pending, "the hold ended before the fills were queued: the run proved nothing"
    rc, out = raw_link(B, ctx, ch, out=out)
    assert rc == 0
    same_link(host(out), want)

"""GPU tests of the feature tracker: brisk_hip_link_tracks_device (a chain's packed match lists -> prev / track / age per row) and
brisk_hip_list_tracks_device (the tracks worth keeping, packed).  The expectation is always the Python restatement of the rule
(test_abi_tracks.restated_link / restated_list) on the downloaded inputs; every array is compared as bytes, and outputs are
pre-filled with the matcher tests' sentinel so that a write outside the rows shows."""
import ctypes as C

import numpy as np
import pytest

from gpu_prefill import settled
from test_abi_tracks import SENT32, SENT64, restated_link, restated_list
from test_gpu_match_pairs import SENTINEL, batch_frames

pytestmark = pytest.mark.gpu

CAP = 130
ROWS = [65, 0, 1, 63, 64, 130, 131, 7]   # empty nodes inside the chain, a node beyond rows_cap
ODD = np.concatenate([np.array([np.inf, np.nan, -1.0, -0.0, 2147483648.0], np.float32),
                      np.array([0x7F800001, 0xFFFFFFFF], np.uint32).view(np.float32)])


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


# ---- chains made by hand ------------------------------------------------------------------------------------------------------

def make_chain(B, seed, node_rows, empty_pair=None, through=False):
    """(offsets [nodes], records) of packed lists as the selection writes them: sorted by query row, one or two records a row.
    Rows are named up to the nodes' TRUE counts (a node beyond rows_cap: records that name cut rows) and a little beyond; many rows
    ask for the train rows 0 .. 2 (conflicts, with equal distances too); a loser's second record often names a free row; odd
    distances and indices of -1 are mixed in.  through: row (p + 1) % 5 of every node takes row p % 5 of the node before at
    distance 0 - one track through the whole chain."""
    rng = np.random.default_rng(seed)
    lists = []
    for p in range(len(node_rows) - 1):
        nq, nt = int(node_rows[p + 1]), int(node_rows[p])
        rows = []
        if p != empty_pair:
            if rng.integers(0, 4) == 0:
                rows.append((-1, 0, 1.0))
            for q in range(nq + (2 if rng.integers(0, 3) == 0 else 0)):       # rows lim and lim + 1 now and then
                if through and q == (p + 1) % 5:
                    rows.append((q, p % 5, 0.0))
                    continue
                if rng.integers(0, 5) == 0:
                    continue
                d = float(rng.integers(1, 5))
                t = int(rng.integers(0, 3)) if rng.integers(0, 3) == 0 else int(rng.integers(-1, nt + 2))
                if rng.integers(0, 12) == 0:
                    d = ODD[rng.integers(0, len(ODD))]
                rows.append((q, t, d))
                if rng.integers(0, 2) == 0:                                   # a second record: never proposed, whatever it names
                    rows.append((q, int(rng.integers(0, max(nt, 1))), float(d) + 1.0 if np.isfinite(d) else 1.0))
        a = np.zeros(len(rows), B.DMATCH)
        for n, (q, t, d) in enumerate(rows):
            a[n] = (q, t, p, d)
        lists.append(a)
    offsets = np.zeros(max(len(node_rows), 1), np.int64)
    if lists:
        offsets[1:] = np.cumsum([len(a) for a in lists])
    return offsets, (np.concatenate(lists) if lists else np.zeros(0, B.DMATCH))


class Chain:
    """a chain's inputs on the device: the row counts at `stride` ints (garbage between them), offsets, records"""

    def __init__(self, B, node_rows, rows_cap, offsets, matches, stride=1):
        import torch
        self.node_rows, self.rows_cap, self.nodes, self.stride = [int(n) for n in node_rows], int(rows_cap), len(node_rows), stride
        self.offsets, self.matches = offsets, matches
        nr = np.full(self.nodes * stride, 77777, np.int32)
        nr[::stride] = self.node_rows
        self.d_rows = torch.from_numpy(nr).cuda()
        self.d_offsets = torch.from_numpy(offsets).cuda()
        self.d_matches = torch.from_numpy(np.ascontiguousarray(matches).view(np.int32).reshape(-1, 4).copy()).cuda()
        if len(matches) == 0:
            self.d_matches = settled(torch.zeros((1, 4), dtype=torch.int32, device="cuda"))

    def sub(self, B, a, b):
        """nodes [a, b) as a chain of their own (the same records: the offsets are absolute)"""
        return Chain(B, self.node_rows[a:b], self.rows_cap, self.offsets[a:b].copy(), self.matches)


def sentinel_link_outputs(nodes, rows_cap):
    import torch
    return settled(torch.full((nodes, rows_cap), SENTINEL, dtype=torch.int32, device="cuda"),
                   torch.full((nodes, rows_cap), int(SENT64), dtype=torch.int64, device="cuda"),
                   torch.full((nodes, rows_cap), SENTINEL, dtype=torch.int32, device="cuda"),
                   torch.full((8,), int(SENT64), dtype=torch.int64, device="cuda"))


def raw_link(B, ctx, ch, seed=None, out=None):
    """the C entry point on pre-filled outputs; seed: (d_track tensor, d_age tensor, first_new, d_first_new tensor or None)"""
    out = out or sentinel_link_outputs(ch.nodes, ch.rows_cap)
    s = None
    if seed is not None:
        st, sa, first, dfirst = seed
        s = B.TrackSeed(st.data_ptr() if st is not None else None, sa.data_ptr() if sa is not None else None, int(first),
                        dfirst.data_ptr() if dfirst is not None else None)
    rc = ctx._L.brisk_hip_link_tracks_device(ctx._h, ch.d_rows.data_ptr(), ch.stride, ch.nodes, ch.rows_cap, ch.d_offsets.data_ptr(),
                                             ch.d_matches.data_ptr(), C.byref(s) if s is not None else None, out[0].data_ptr(),
                                             out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), None)
    return rc, out


def host(tensors):
    import torch
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in tensors)


def same_link(got, want):
    for name, g, w in zip(("prev", "track", "age", "summary"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, name
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w)
            raise AssertionError((name, len(bad), bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


def seed_arrays(rng, rows_cap):
    """seeds with -1 entries and with ages > 0"""
    st = rng.integers(0, 1000, rows_cap).astype(np.int64) + 2 ** 33
    st[rng.integers(0, 3, rows_cap) == 0] = -1
    return st, rng.integers(0, 100, rows_cap).astype(np.int32)


def sentinel_list_outputs(tracks_cap, obs_cap, slack=16):
    import torch
    return settled(torch.full((tracks_cap + slack,), int(SENT64), dtype=torch.int64, device="cuda"),
                   torch.full((tracks_cap + slack,), SENTINEL, dtype=torch.int32, device="cuda"),
                   torch.full((tracks_cap + 1 + slack,), int(SENT64), dtype=torch.int64, device="cuda"),
                   torch.full((obs_cap + slack, 2), SENTINEL, dtype=torch.int32, device="cuda"),
                   torch.full((4,), int(SENT64), dtype=torch.int64, device="cuda"))


def raw_list(B, ctx, ch, link_out, min_len, tracks_cap, obs_cap, out=None):
    out = out or sentinel_list_outputs(tracks_cap, obs_cap)
    rc = ctx._L.brisk_hip_list_tracks_device(ctx._h, ch.d_rows.data_ptr(), ch.stride, ch.nodes, ch.rows_cap, link_out[0].data_ptr(),
                                             link_out[1].data_ptr(), link_out[2].data_ptr(), int(min_len), int(tracks_cap), int(obs_cap),
                                             out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), out[4].data_ptr(),
                                             None)
    return rc, out


def same_list(B, got, want):
    """got: the pre-filled arrays on the host; the stored prefix is the restatement's, everything behind it still sentinel"""
    gt, gl, go, gobs, gs = got
    wt, wl, wo, wobs, ws = want
    assert gs.tolist() == ws.tolist(), (gs, ws)
    n, m = int(ws[2]), int(wo[-1])
    assert gt[:n].tobytes() == wt.tobytes() and (gt[n:] == SENT64).all()
    assert gl[:n].tobytes() == wl.tobytes() and (gl[n:] == SENT32).all()
    assert go[:n + 1].tobytes() == wo.tobytes() and (go[n + 1:] == SENT64).all()
    assert gobs[:m].tobytes() == wobs.tobytes() and (gobs[m:] == SENT32).all()


# ---- 1: hand-made lists -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nodes", [1, 2, 3, 65, 257])
def test_hand_made_lists(B, ctx, nodes):
    rng = np.random.default_rng(nodes)
    node_rows = (ROWS * 40)[:nodes]
    offsets, m = make_chain(B, 100 + nodes, node_rows, empty_pair=nodes // 2 if nodes > 3 else None)
    ch = Chain(B, node_rows, CAP, offsets, m, stride=3 if nodes == 65 else 1)
    st, sa = seed_arrays(rng, CAP)
    for seeded in (False, True):
        import torch
        seed = (torch.from_numpy(st).cuda(), torch.from_numpy(sa).cuda(), 5, None) if seeded else None
        rc, out = raw_link(B, ctx, ch, seed)
        assert rc == 0, ctx._L.brisk_hip_last_error(ctx._h)
        want = restated_link(node_rows, CAP, offsets, m, st if seeded else None, sa if seeded else None, 5 if seeded else 0)
        same_link(host(out), want)
    if nodes >= 65:      # not vacuous: conflicts were lost, records ignored, the cut node's rows named, tracks span nodes
        assert want[3][3] > 50 and want[3][4] > 200 and want[3][2] > 500 and want[2][want[2] != SENT32].max() >= 3
        assert (m["queryIdx"] >= CAP).any() and (m["trainIdx"] >= CAP).any() and offsets[nodes // 2] == offsets[nodes // 2 + 1]
    # the Python call gives the same arrays where it writes
    if nodes > 1:
        got = host(ctx.link_tracks((ch.d_rows, ch.stride), nodes, CAP, ch.d_offsets, ch.d_matches))
        plain = restated_link(node_rows, CAP, offsets, m)
        wrote = plain[0] != SENT32
        for g, w in zip(got[:3], plain[:3]):
            assert np.array_equal(g[wrote], w[wrote])
        assert got[3].tolist() == plain[3].tolist()


# ---- 2: the longest walk and the workgroup sums -------------------------------------------------------------------------------

def test_one_track_through_2049_nodes(B, ctx):
    nodes, cap = 2049, 8
    node_rows = [5] * nodes
    offsets, m = make_chain(B, 9, node_rows, through=True)
    ch = Chain(B, node_rows, cap, offsets, m)
    rc, out = raw_link(B, ctx, ch)
    assert rc == 0
    want = restated_link(node_rows, cap, offsets, m)
    same_link(host(out), want)
    assert want[2][nodes - 1, (nodes - 1) % 5] == nodes - 1 and want[1][nodes - 1, (nodes - 1) % 5] == 0   # track 0, seen 2 049 times
    assert want[3][1] > nodes                                                                            # ... beside short ones
    rc, lo = raw_list(B, ctx, ch, out, 3, nodes * 5, nodes * 5)
    assert rc == 0
    wl = restated_list(node_rows, cap, *want[:3], 3)
    same_list(B, host(lo), wl)
    assert wl[1].max() == nodes and wl[4][0] > 100


def test_more_workgroup_sums_than_the_offsets_kernel_has_threads(B, ctx):
    """1 100 nodes x rows_cap 300: two 256-row workgroups per node, 2 200 sums for the 1 024 threads of the offsets kernels; nodes
    of exactly 63 ... 257 rows"""
    nodes, cap = 1100, 300
    rng = np.random.default_rng(31)
    node_rows = [int(v) for v in rng.choice([63, 64, 65, 255, 256, 257, 0, 300, 301], nodes)]
    node_rows[:6] = [63, 64, 65, 255, 256, 257]
    offsets, m = make_chain(B, 32, node_rows, empty_pair=500)
    ch = Chain(B, node_rows, cap, offsets, m)
    rc, out = raw_link(B, ctx, ch)
    assert rc == 0
    want = restated_link(node_rows, cap, offsets, m)
    same_link(host(out), want)
    wl = restated_list(node_rows, cap, *want[:3], 2)
    rc, lo = raw_list(B, ctx, ch, out, 2, int(wl[4][0]), int(wl[4][1]))
    assert rc == 0
    same_list(B, host(lo), wl)
    cut = restated_list(node_rows, cap, *want[:3], 2, int(wl[4][0]) // 2, int(wl[4][1]))    # a cut deep inside the sums
    rc, lo = raw_list(B, ctx, ch, out, 2, int(wl[4][0]) // 2, int(wl[4][1]))
    assert rc == 0
    same_list(B, host(lo), cut)
    assert cut[4][3] == 1 and cut[4][2] == int(wl[4][0]) // 2


# ---- 3: numbers beyond 32 bits, seeds, the split property ---------------------------------------------------------------------

@pytest.fixture(scope="module")
def chain65(B):
    node_rows = (ROWS * 9)[:65]
    offsets, m = make_chain(B, 65, node_rows, empty_pair=40)
    rng = np.random.default_rng(650)
    st, sa = seed_arrays(rng, CAP)
    return {"ch": Chain(B, node_rows, CAP, offsets, m), "st": st, "sa": sa,
            "want": restated_link(node_rows, CAP, offsets, m, st, sa, 2 ** 40)}


@pytest.mark.parametrize("through_device", [False, True])
def test_first_new_beyond_32_bits(B, ctx, chain65, through_device):
    import torch
    ch = chain65["ch"]
    st, sa = torch.from_numpy(chain65["st"]).cuda(), torch.from_numpy(chain65["sa"]).cuda()
    word = torch.tensor([2 ** 40, 123], dtype=torch.int64, device="cuda")
    rc, out = raw_link(B, ctx, ch, (st, sa, 999 if through_device else 2 ** 40, word if through_device else None))
    assert rc == 0
    got = host(out)
    same_link(got, chain65["want"])
    assert got[3][0] > 2 ** 40 + 1000 and (got[1][got[0] == -1] >= 2 ** 33).all()
    # determinism: the same call again, the same bytes
    rc, again = raw_link(B, ctx, ch, (st, sa, 999 if through_device else 2 ** 40, word if through_device else None))
    assert rc == 0 and all(a.tobytes() == b.tobytes() for a, b in zip(host(again), got))


def test_first_new_from_the_call_s_own_summary(B, ctx, chain65):
    """one summary buffer for call after call: d_first_new is read before the summary is written"""
    import torch
    ch = chain65["ch"]
    st, sa = torch.from_numpy(chain65["st"]).cuda(), torch.from_numpy(chain65["sa"]).cuda()
    out = sentinel_link_outputs(ch.nodes, ch.rows_cap)
    out[3][0] = 2 ** 40
    settled()                                                           # (a fill on the null stream, like the sentinel's)
    rc, out = raw_link(B, ctx, ch, (st, sa, 0, out[3]), out=out)
    assert rc == 0
    same_link(host(out), chain65["want"])


@pytest.mark.parametrize("m", [0, 1, 31, 63])
def test_a_chain_split_in_two_calls(B, ctx, chain65, m):
    import torch
    ch, want = chain65["ch"], chain65["want"]
    st, sa = torch.from_numpy(chain65["st"]).cuda(), torch.from_numpy(chain65["sa"]).cuda()
    first, second = ch.sub(B, 0, m + 1), ch.sub(B, m, ch.nodes)
    rc, o1 = raw_link(B, ctx, first, (st, sa, 2 ** 40, None))
    assert rc == 0
    # node m's rows of the first call seed the second, its next_new comes through the device word: no synchronisation in between
    rc, o2 = raw_link(B, ctx, second, (o1[1][m], o1[2][m], -1, o1[3]))
    assert rc == 0
    h1, h2 = host(o1), host(o2)
    assert h1[1].tobytes() == want[1][:m + 1].tobytes() and h1[2].tobytes() == want[2][:m + 1].tobytes()
    assert h2[1].tobytes() == want[1][m:].tobytes() and h2[2].tobytes() == want[2][m:].tobytes()
    assert h2[3][0] == want[3][0] and h1[3][1] + h2[3][1] == want[3][1] and h1[3][2] + h2[3][2] == want[3][2]
    assert h2[0][1:].tobytes() == want[0][m + 1:].tobytes()


# ---- 4: lists -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def linked65(B, ctx, chain65):
    import torch
    ch = chain65["ch"]
    st, sa = torch.from_numpy(chain65["st"]).cuda(), torch.from_numpy(chain65["sa"]).cuda()
    rc, out = raw_link(B, ctx, ch, (st, sa, 2 ** 40, None))
    assert rc == 0
    same_link(host(out), chain65["want"])
    return out


@pytest.mark.parametrize("min_len", [1, 2, 3, 66])
def test_lists(B, ctx, chain65, linked65, min_len):
    ch, want = chain65["ch"], chain65["want"]
    full = restated_list(ch.node_rows, CAP, *want[:3], min_len)
    pieces, obs = int(full[4][0]), int(full[4][1])
    assert pieces > 5 and obs >= pieces
    if min_len == 66:                                                   # nodes + 1: seeded pieces only
        assert set(full[0].tolist()) <= set(chain65["st"].tolist()) and (full[1] >= 66).all()
    for tracks_cap, obs_cap in ((pieces, obs), (pieces - 1, obs), (pieces, obs - 1), (0, obs), (pieces, 0), (0, 0), (pieces + 9, obs + 9),
                                (pieces // 2, obs), (pieces, obs // 2)):
        w = restated_list(ch.node_rows, CAP, *want[:3], min_len, tracks_cap, obs_cap)
        rc, lo = raw_list(B, ctx, ch, linked65, min_len, tracks_cap, obs_cap)
        assert rc == 0, (tracks_cap, obs_cap)
        same_list(B, host(lo), w)
        assert int(w[4][3]) == (tracks_cap < pieces or obs_cap < obs) and w[4][:2].tolist() == [pieces, obs]
    # the Python call: everything fits
    got = host(ctx.list_tracks((ch.d_rows, 1), ch.nodes, CAP, *linked65[:3], min_len))
    assert got[4].tolist() == full[4].tolist()
    assert got[0][:pieces].tobytes() == full[0].tobytes() and got[2][:pieces + 1].tobytes() == full[2].tobytes()
    assert got[3][:obs].tobytes() == full[3].tobytes()
    # determinism
    rc, a = raw_list(B, ctx, ch, linked65, min_len, pieces, obs)
    rc2, b = raw_list(B, ctx, ch, linked65, min_len, pieces, obs)
    assert rc == 0 and rc2 == 0 and all(x.tobytes() == y.tobytes() for x, y in zip(host(a), host(b)))


# ---- 5: the real path ---------------------------------------------------------------------------------------------------------

def run_real(B, ctx, frames, k, cross, sel, first_new=0, min_len=3):
    """detect + describe, match, select, link, list on one stream; returns the host copies and the restatement of both calls"""
    import torch
    n, h, w = frames.shape
    d = torch.from_numpy(frames).cuda()
    ext = B.BriskDescriptorExtractor(context=ctx)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    ctx.detect_describe_batch(ext, d.data_ptr(), n, w, h, w * h, w, 70, 2, s.cuda_stream)
    st, dim = ctx.batch_desc_set()
    triple = ctx.match_knn_pairs(st, st, B.PairSpec(n - 1, 1, 1, 0, 1, None), k, cross_check=cross, stream=s.cuda_stream)
    rows_cap = int(triple[1].shape[1])
    matches, counts, flags, offsets = ctx.select_pair_matches(triple, k, sel, stream=s.cuda_stream)
    seed = B.TrackSeed(None, None, first_new, None)
    linked = ctx.link_tracks((st, 0, 1), n, rows_cap, offsets, matches, seed=seed, stream=s.cuda_stream)
    listed = ctx.list_tracks((st, 0, 1), n, rows_cap, *linked[:3], min_len, stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert ctx.batch_status(n) == 0
    node_rows = np.array([len(ctx.batch_download(f, True, strings=dim)[0]) for f in range(n)])
    ho = offsets.cpu().numpy()
    hm = matches.cpu().numpy().view(B.DMATCH).reshape(-1)[:int(ho[-1])]            # the records stored
    want = restated_link(node_rows, rows_cap, ho, hm, first_new=first_new)
    got = tuple(t.cpu().numpy() for t in linked)
    wrote = want[0] != SENT32
    for name, g, w_ in zip(("prev", "track", "age"), got, want):
        assert np.array_equal(g[wrote], w_[wrote]), name
    assert got[3].tolist() == want[3].tolist()
    wl = restated_list(node_rows, rows_cap, *want[:3], min_len)
    gl = tuple(t.cpu().numpy() for t in listed)
    pieces, obs = int(wl[4][0]), int(wl[4][1])
    assert gl[4].tolist() == wl[4].tolist()
    assert gl[0][:pieces].tobytes() == wl[0].tobytes() and gl[1][:pieces].tobytes() == wl[1].tobytes()
    assert gl[2][:pieces + 1].tobytes() == wl[2].tobytes() and gl[3][:obs].tobytes() == wl[3].tobytes()
    desc0 = ctx.batch_download(0, True, strings=dim)[1]
    ext.close()
    return {"node_rows": node_rows, "rows_cap": rows_cap, "offsets": ho, "matches": hm, "link": want, "list": wl, "desc0": desc0}


def test_the_real_path(B, ctx, golden_ast):
    frames = batch_frames(golden_ast)
    r = run_real(B, ctx, frames, 2, False, B.MatchSelect(float("inf"), 0.8, 1))
    s = r["link"][3]
    assert s[2] > 100 and s[3] > 0 and r["list"][4][0] > 10      # links, conflicts that were lost, tracks of three frames
    # k = 1 with the cross check: every record is a link
    r = run_real(B, ctx, frames, 1, True, B.MatchSelect.everything(1))
    prev, m, o = r["link"][0], r["matches"], r["offsets"]
    assert len(m) > 100 and r["link"][3][3] == 0 and r["link"][3][4] == 0 and r["link"][3][2] == len(m)
    for p in range(len(frames) - 1):
        rec = m[int(o[p]):int(o[p + 1])]
        assert np.array_equal(prev[p + 1, rec["queryIdx"]], rec["trainIdx"])


def test_one_frame_eight_times(B, ctx, golden_ast):
    """the known answer: a row whose descriptor is the only one of its kind in the frame finds itself at distance 0 with a second
    neighbour further away, passes the ratio test and is claimed by nobody else - n tracks of length 8, track[i][r] = first_new + r,
    age = i.  A row that shares its descriptor with another has two neighbours at distance 0, fails the ratio test and starts a
    new track in every frame; the answer is as exact with such rows as without."""
    frames = np.stack([golden_ast[0]["image"]] * 8)
    first = 2 ** 35 + 3
    r = run_real(B, ctx, frames, 2, False, B.MatchSelect(float("inf"), 0.8, 1), first_new=first, min_len=8)
    n = int(r["node_rows"][0])
    assert n > 100 and (r["node_rows"] == n).all() and n <= r["rows_cap"]
    _, inverse, counts = np.unique(r["desc0"], axis=0, return_inverse=True, return_counts=True)
    uniq = counts[inverse.reshape(-1)] == 1
    nu, nd = int(uniq.sum()), int((~uniq).sum())
    assert nu > 100 and nu + nd == n
    prev, track, age, s = r["link"]
    assert np.array_equal(track[0, :n], first + np.arange(n)) and (age[0, :n] == 0).all()
    for i in range(1, 8):
        assert np.array_equal(track[i, :n][uniq], first + np.flatnonzero(uniq)) and (age[i, :n][uniq] == i).all()
        assert np.array_equal(prev[i, :n][uniq], np.flatnonzero(uniq)) and (prev[i, :n][~uniq] == -1).all()
        assert np.array_equal(track[i, :n][~uniq], first + n + (i - 1) * nd + np.arange(nd)) and (age[i, :n][~uniq] == 0).all()
    assert s.tolist() == [first + n + 7 * nd, n + 7 * nd, 7 * nu, 0, 0, 8 * n, 0, 0]
    lt, ll, lo, obs, ls = r["list"]
    assert ls.tolist() == [nu, 8 * nu, nu, 0] and (ll == 8).all() and np.array_equal(lt, first + np.flatnonzero(uniq))
    assert np.array_equal(obs["node"].reshape(nu, 8), np.tile(np.arange(8), (nu, 1)))
    assert np.array_equal(obs["row"].reshape(nu, 8), np.tile(np.flatnonzero(uniq)[:, None], (1, 8)))


# ---- 6: arguments -------------------------------------------------------------------------------------------------------------

def test_arguments(B, ctx):
    import torch
    node_rows = ROWS[:3]
    offsets, m = make_chain(B, 3, node_rows)
    ch = Chain(B, node_rows, CAP, offsets, m)
    out = sentinel_link_outputs(3, CAP)
    L, h = ctx._L, ctx._h
    good = [ch.d_rows.data_ptr(), 1, 3, CAP, ch.d_offsets.data_ptr(), ch.d_matches.data_ptr(), None, out[0].data_ptr(), out[1].data_ptr(),
            out[2].data_ptr(), out[3].data_ptr(), None]
    st, sa = settled(torch.zeros(CAP + 1, dtype=torch.int64, device="cuda"), torch.zeros(CAP + 1, dtype=torch.int32, device="cuda"))

    def seed(t, a, w=None):
        return C.byref(B.TrackSeed(t, a, 0, w))

    bad = [(2, 0), (2, -1), (3, 0), (1, 0), (1, -2), (0, None), (4, None), (5, None), (7, None), (8, None), (9, None), (10, None),
           (5, good[5] + 8), (4, good[4] + 4), (8, good[8] + 4), (10, good[10] + 4), (7, good[7] + 2), (9, good[9] + 1), (0, good[0] + 2),
           (6, seed(st.data_ptr(), None)), (6, seed(None, sa.data_ptr())), (6, seed(st.data_ptr() + 4, sa.data_ptr())),
           (6, seed(st.data_ptr(), sa.data_ptr() + 2)), (6, seed(st.data_ptr(), sa.data_ptr(), st.data_ptr() + 4))]
    for at, v in bad:
        a = list(good)
        a[at] = v
        assert L.brisk_hip_link_tracks_device(h, *a) == 1, (at, v)
    assert L.brisk_hip_link_tracks_device(None, *good) == 1
    torch.cuda.synchronize()
    assert all((t.cpu().numpy().view(np.int32) == SENTINEL).all() for t in out)        # nothing was launched
    # nodes == 1 is valid without lists: every row is a head
    one = list(good)
    one[2], one[4], one[5] = 1, None, None
    assert L.brisk_hip_link_tracks_device(h, *one) == 0
    assert L.brisk_hip_link_tracks_device(h, *good) == 0
    same_link(host(out), restated_link(node_rows, CAP, offsets, m))

    lo = sentinel_list_outputs(50, 200)
    glist = [ch.d_rows.data_ptr(), 1, 3, CAP, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(), 2, 50, 200, lo[0].data_ptr(),
             lo[1].data_ptr(), lo[2].data_ptr(), lo[3].data_ptr(), lo[4].data_ptr(), None]
    bad = [(2, 0), (3, 0), (1, 0), (0, None), (4, None), (5, None), (6, None), (7, 0), (7, -3), (8, -1), (9, -1), (10, None), (11, None),
           (12, None), (13, None), (14, None), (5, glist[5] + 4), (10, glist[10] + 4), (12, glist[12] + 4), (13, glist[13] + 4),
           (14, glist[14] + 4), (11, glist[11] + 2), (4, glist[4] + 2), (6, glist[6] + 1)]
    for at, v in bad:
        a = list(glist)
        a[at] = v
        assert L.brisk_hip_list_tracks_device(h, *a) == 1, (at, v)
    torch.cuda.synchronize()
    assert all((t.cpu().numpy().view(np.int32) == SENTINEL).all() for t in lo)
    # NULL arrays behind a capacity of zero are allowed
    a = list(glist)
    a[8], a[9], a[10], a[11], a[13] = 0, 0, None, None, None
    assert L.brisk_hip_list_tracks_device(h, *a) == 0
    got = host(lo)
    want = restated_list(node_rows, CAP, *restated_link(node_rows, CAP, offsets, m)[:3], 2, 0, 0)
    same_list(B, got, want)
    assert got[2][0] == 0 and got[4][2] == 0

"""GPU tests of the pair matchers and their exit where pair and row indices get wide: more pairs than one launch holds (65 535),
train and query indices beyond 2^16 and at the keys' limit 2^22, the largest distances (bit 31 of a key), more workgroup sums than the
offsets pass has threads, rows ending at the selection passes' workgroup boundaries, and exactly 32 / 33 radius hits (the list /
dense boundary).  The expectation of a matcher call is always the CPU oracle (oracle/brisk_oracle_match.c; gated calls: with the mask
of test_gpu_match_gated.gate_mask), of the exit the numpy restatement of the selection rule (test_gpu_match_export.expect) - never
another entry point of the engine.  Whole padded arrays are compared, the memory that must stay untouched included: no tolerance.

The 65 605 pairs of the first part are drawn from 36 distinct (a, b): the oracle and `expect` run once per distinct pair and the
arrays of the call are assembled from those blocks with numpy indexing (expect_drawn) - `expect`'s own loop over 262 420 rows would
take longer than everything else here together.  Every "the input reaches the case" assertion is made on the oracle's output."""
import types

import numpy as np
import pytest

from gpu_prefill import settled
import oracle_lib as O
import test_gpu_match_gated as G
import test_gpu_match_radius_pairs as R
from test_gpu_match_export import INF, ROWS_CUT, expect, host_got, raw_select, same_selection, sentinel_select_outputs
from test_gpu_match_gated import GRID_GATE, SynthKp, gate_mask
from test_gpu_match_pairs import SENTINEL, SynthSet, oracle_cross, oracle_pair, same_rows, sentinel_outputs

pytestmark = pytest.mark.gpu

LIST = 32                   # MRP_LIST
IDX_BITS = 22               # MF_IDX_BITS
LAUNCH = 65535              # pairs per launch
TOP_UP = np.float32(2147483648.0)
PAIR_ROWS_CUT, PAIR_BAD, PAIR_ENTRIES_CUT = 1, 2, 4


@pytest.fixture(scope="module")
def B():
    import ethzasl_brisk_amd as B
    from ethzasl_brisk_amd import build
    build.build()
    B.load_library()
    return B


# ---- what the tests share ---------------------------------------------------------------------------------------------------------

def flipped(row, bits):
    """a copy of the descriptor with the given bit positions inverted: Hamming distance len(bits)"""
    out = np.array(row, np.uint8)
    for b in bits:
        out[b >> 3] ^= np.uint8(1 << (b & 7))
    return out


def block(want, rows_cap, per):
    """the padded arrays of one pair whose stored rows the oracle gives as `want` (uncut in length: a radius row may be longer than
    per): entries behind min(found, per) and rows behind len(want) keep the sentinel"""
    assert len(want) <= rows_cap
    m, c = np.full((rows_cap, per, 4), SENTINEL, np.int32), np.full(rows_cap, SENTINEL, np.int32)
    for q, w in enumerate(want):
        c[q] = len(w)
        s = min(len(w), per)
        m[q, :s] = np.ascontiguousarray(w[:s]).view(np.int32).reshape(s, 4)
    return m, c


def same_padded(host, p, want, pair_rows):
    """pair p of the downloaded arrays holds exactly the oracle's rows and the true row count, everything else the sentinel"""
    m, cnt, rows = host
    rows_cap, per = cnt.shape[1], m.shape[2]
    assert int(rows[p]) == pair_rows
    em, ec = block(want, rows_cap, per)
    if not (np.array_equal(cnt[p], ec) and np.array_equal(m[p], em)):
        n = len(want)                                               # the readable message first
        assert [int(c) for c in cnt[p, :n]] == [len(w) for w in want]
        same_rows([m[p, q, :min(len(w), per)].reshape(-1).view(O.DMATCH) for q, w in enumerate(want)], [w[:per] for w in want])
        assert np.array_equal(cnt[p], ec) and np.array_equal(m[p], em), "memory behind the counted entries or rows was written"


def run(B, ctx, Q, T, plist, per, rows_cap, radius=None, cross=False, gate=None, qk=None, tk=None):
    """one call on a device pair list into sentinel-filled arrays: (the arrays on the host, the device triple)"""
    import torch
    d_pairs = torch.from_numpy(np.ascontiguousarray(np.array(plist, np.int32).reshape(-1, 2))).cuda()
    out = sentinel_outputs(len(d_pairs), rows_cap, per)
    spec = B.PairSpec(len(d_pairs), 0, 0, 0, 0, d_pairs.data_ptr())
    kw = dict(rows_cap=rows_cap, dim_bytes=Q.dim, out=out)
    if gate is not None:
        kw.update(gate=B.MatchGate(*gate), query_kps=qk.set, train_kps=tk.set)
    torch.cuda.synchronize()
    if radius is None:
        ctx.match_knn_pairs(Q.set, T.set, spec, per, cross_check=cross, **kw)
    else:
        ctx.match_radius_pairs(Q.set, T.set, spec, radius, per, **kw)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out), out


def one_frame(B, rng, rows, cap=None):
    rows = np.ascontiguousarray(rows, np.uint8)
    return SynthSet(B, rng, rows.shape[1], rows.shape[1], [len(rows)], cap or max(len(rows), 1), count_stride=1, prepared={0: rows})


def device_select(B, ctx, triple, per_row, sel, matches_cap=None):
    import torch
    res = ctx.select_pair_matches(triple, per_row, B.MatchSelect(*sel), matches_cap=matches_cap)
    torch.cuda.synchronize()
    m, c, f, o = (t.cpu().numpy() for t in res)
    return m.view(B.DMATCH).reshape(-1), c, f, o


def capped_select(B, ctx, triple, per_row, sel, cap, want):
    """the device form under matches_cap into sentinel-filled outputs: the rule's lists, and nothing behind the stored matches"""
    import torch
    npairs = triple[1].shape[0]
    outs = sentinel_select_outputs(npairs, int(cap) + 8)
    torch.cuda.synchronize()
    assert raw_select(ctx, triple, per_row, B.MatchSelect(*sel), int(cap), outs) == 0
    torch.cuda.synchronize()
    m, c, f, o = (t.cpu().numpy() for t in outs)
    same_selection((m.view(B.DMATCH).reshape(-1), c, f, o), want)
    assert (m[int(o[-1]):] == SENTINEL).all()


# ---- 1: more than 65 535 pairs in one call ---------------------------------------------------------------------------------------

NPAIRS = LAUNCH + 70
POOL_A = [0, 1, 2, 3, 5, 4]         # rows of the query frames: one has more than MANY_CAP
POOL_B = [3, 0, 5, 1, 4, 2]         # ... of the train frames: an empty one, one with a single row (k = 2: the top-up)
MANY_CAP = 4
MANY_RADIUS, MANY_CPQ = 64.5, 2
BAD = {9: (-1, 2), 30001: (6, 0), LAUNCH - 3: (3, -1), LAUNCH + 6: (2, 6), NPAIRS - 2: (7, 7)}
SEAM = {LAUNCH - 1: (4, 2), LAUNCH: (3, 4), LAUNCH + 1: (5, 0)}     # the last pair of the first launch, the first two of the second


def drawn_pairs():
    rng = np.random.default_rng(65535)
    pairs = rng.integers(0, len(POOL_A), (NPAIRS, 2)).astype(np.int32)
    for p, ab in {**BAD, **SEAM}.items():
        pairs[p] = ab
    return pairs


class Drawn:
    """the pool, the pair list and what assembles a call's expected arrays from one oracle call per distinct pair"""

    def __init__(self, B):
        import torch
        rng = np.random.default_rng(1906)
        self.B = B
        self.A = SynthSet(B, rng, 16, 16, POOL_A, 5)
        self.Bs = SynthSet(B, rng, 16, 20, POOL_B, 5, 4, 2, 8)
        self.Ak, self.Bk = SynthKp(B, rng, POOL_A, 5), SynthKp(B, rng, POOL_B, 5, slack=4)
        self.pairs = drawn_pairs()
        nA, nB = len(POOL_A), len(POOL_B)
        pa, pb = self.pairs[:, 0], self.pairs[:, 1]
        self.good = (pa >= 0) & (pa < nA) & (pb >= 0) & (pb < nB)
        self.slot = np.where(self.good, pa * nB + pb, nA * nB)       # the distinct pair of every entry; the last slot: a bad entry
        self.distinct = sorted({(int(a), int(b)) for a, b in self.pairs[self.good]})
        self.d_pairs = torch.from_numpy(self.pairs).cuda()
        self.masks = {(a, b): gate_mask(GRID_GATE, self.Ak.kps[a], self.Bk.kps[b]) for a, b in self.distinct}
        self.results = {}

    def want(self, mode, a, b):
        """the oracle's rows of pair (a, b), cut to the stored rows"""
        dq, dt = self.A.desc[a], self.Bs.desc[b]
        if mode == "k2":
            w = oracle_pair(dq, dt, b, 2)
        elif mode == "cross":
            w = oracle_cross(dq, dt, b)
        elif mode == "radius":
            w = R.oracle_pair(dq, dt, b, MANY_RADIUS)
        elif mode == "gated_k2":
            w = G.oracle_knn(dq, dt, self.masks[a, b], b, 2)
        else:
            w = G.oracle_radius(dq, dt, self.masks[a, b], b, MANY_RADIUS)
        return w[:MANY_CAP]

    def table(self, mode):
        """(matches, counts, pair_rows) per slot: the blocks the expected arrays are assembled from, and the oracle's rows"""
        per = MANY_CPQ if "radius" in mode else (1 if mode == "cross" else 2)
        n = len(POOL_A) * len(POOL_B) + 1
        tm, tc = np.full((n, MANY_CAP, per, 4), SENTINEL, np.int32), np.full((n, MANY_CAP), SENTINEL, np.int32)
        tr = np.full(n, -1, np.int32)
        rows = {}
        for a, b in self.distinct:
            rows[a, b] = self.want(mode, a, b)
            s = a * len(POOL_B) + b
            tm[s], tc[s] = block(rows[a, b], MANY_CAP, per)
            tr[s] = POOL_A[a]
        return (tm, tc, tr), rows, per

    def call(self, mode):
        """the call of `mode` on all pairs, once: (host arrays, device triple)"""
        import torch
        if mode not in self.results:
            B, per = self.B, MANY_CPQ if "radius" in mode else (1 if mode == "cross" else 2)
            out = sentinel_outputs(NPAIRS, MANY_CAP, per)
            spec = B.PairSpec(NPAIRS, 0, 0, 0, 0, self.d_pairs.data_ptr())
            kw = dict(rows_cap=MANY_CAP, dim_bytes=16, out=out)
            if mode.startswith("gated"):
                kw.update(gate=B.MatchGate(*GRID_GATE), query_kps=self.Ak.set, train_kps=self.Bk.set)
            torch.cuda.synchronize()
            if "radius" in mode:
                self.ctx.match_radius_pairs(self.A.set, self.Bs.set, spec, MANY_RADIUS, per, **kw)
            else:
                self.ctx.match_knn_pairs(self.A.set, self.Bs.set, spec, per, cross_check=mode == "cross", **kw)
            torch.cuda.synchronize()
            self.results[mode] = (tuple(t.cpu().numpy() for t in out), out)
        return self.results[mode]


def drawn_checks(pairs, good, distinct, tables):
    """what the committed seed must give, on the list and on the oracle's rows alone (tables: mode -> Drawn.table(mode)[1])"""
    assert len(pairs) == NPAIRS > LAUNCH and len(distinct) == len(POOL_A) * len(POOL_B)
    assert not good[list(BAD)].any() and good.sum() == NPAIRS - len(BAD)
    assert min(BAD) < LAUNCH - 1 and max(BAD) > LAUNCH + 1           # bad entries in both launches
    seam = [tuple(pairs[p]) for p in sorted(SEAM)]
    assert sorted(SEAM) == [LAUNCH - 1, LAUNCH, LAUNCH + 1] and len(set(seam)) == 3 and good[sorted(SEAM)].all()
    assert max(POOL_A) > MANY_CAP and 0 in POOL_A and 0 in POOL_B and 1 in POOL_B
    k2 = [tuple(len(r) for r in tables["k2"][ab]) for ab in seam]
    assert len({tables["k2"][ab][0].tobytes() for ab in seam}) == 3, k2      # the three pairs at the seam have different first rows
    hits = np.array([len(r) for rows in tables["radius"].values() for r in rows])
    assert (hits == 0).any() and (hits == 1).any() and (hits == 2).any() and (hits > MANY_CPQ).any()
    kept = [len(r) for rows in tables["cross"].values() for r in rows]
    assert 0 < sum(kept) < len(kept)                                # the cross check keeps and drops
    g2 = [len(r) for rows in tables["gated_k2"].values() for r in rows]
    assert g2.count(0) and g2.count(1) and g2.count(2)
    gr = np.array([len(r) for rows in tables["gated_radius"].values() for r in rows])
    assert (gr == 0).any() and (gr > 0).any() and gr.sum() < hits.sum()


@pytest.fixture(scope="module")
def drawn(B):
    d = Drawn(B)
    d.ctx = B.default_context(0)
    allowed = np.concatenate([M.reshape(-1) for M in d.masks.values()])
    assert allowed.any() and not allowed.all()                      # the one gate allows some and forbids some rows
    d.tables = {mode: d.table(mode) for mode in ("k2", "cross", "radius", "gated_k2", "gated_radius")}
    drawn_checks(d.pairs, d.good, d.distinct, {mode: t[1] for mode, t in d.tables.items()})
    return d


@pytest.mark.parametrize("mode", ["k2", "cross", "radius", "gated_k2", "gated_radius"])
def test_more_pairs_than_one_launch(drawn, mode):
    (tm, tc, tr), _, per = drawn.tables[mode]
    m, cnt, rows = drawn.call(mode)[0]
    assert m.shape == (NPAIRS, MANY_CAP, per, 4)
    want_m, want_c, want_r = tm[drawn.slot], tc[drawn.slot], tr[drawn.slot]
    for name, got, want in (("pair_rows", rows, want_r), ("counts", cnt, want_c), ("matches", m, want_m)):
        if not np.array_equal(got, want):
            bad = np.flatnonzero((got != want).reshape(NPAIRS, -1).any(axis=1))
            p = int(bad[0])
            assert False, "%s: %d pairs differ, the first is %d = %s: got %s, want %s" % (name, len(bad), p, drawn.pairs[p], got[p].tolist(), want[p].tolist())


def expect_drawn(drawn, sel, matches_cap=None):
    """test_gpu_match_export.expect for the k = 2 call: the rule (restated_row, through `expect`) on the blocks of the distinct
    pairs, the call's lists assembled from them"""
    (tm, tc, tr), _, per = drawn.tables["k2"]
    stored, counts, flags, offsets = expect((tm.reshape(-1).view(O.DMATCH).reshape(len(tr), MANY_CAP, per), tc, tr), per, sel)[:4]
    c = counts[drawn.slot].astype(np.int64)
    fl = flags[drawn.slot].copy()
    incl = np.cumsum(c)
    cut = NPAIRS
    if matches_cap is not None:
        over = np.flatnonzero((c > 0) & (incl > matches_cap))       # (prefixes grow: the first pair with matches that does not fit)
        cut = int(over[0]) if len(over) else NPAIRS
    fl[cut:] |= ROWS_CUT
    off = np.zeros(NPAIRS + 1, np.int64)
    off[1:] = np.cumsum(np.where(np.arange(NPAIRS) < cut, c, 0))
    ck = c[:cut]
    src = np.repeat(offsets[drawn.slot[:cut]] - (off[1:cut + 1] - ck), ck) + np.arange(int(ck.sum()))
    return stored[src], counts[drawn.slot], fl, off


def test_export_of_more_pairs_than_one_launch(B, drawn):
    host, triple = drawn.call("k2")
    ctx = drawn.ctx
    everything, ratio = (INF, 0.0, 2), (INF, 0.8, 1)
    full = expect_drawn(drawn, everything)
    # the assembled expectation is `expect` itself: on the 100 pairs around the seam of the two launches
    lo, hi = LAUNCH - 50, LAUNCH + 50
    (tm, tc, tr), _, _ = drawn.tables["k2"]
    s = drawn.slot[lo:hi]
    part = expect((tm[s].reshape(-1).view(O.DMATCH).reshape(hi - lo, MANY_CAP, 2), tc[s], tr[s]), 2, everything)
    assert np.array_equal(part[1], full[1][lo:hi]) and np.array_equal(part[2], full[2][lo:hi])
    assert part[0].tobytes() == full[0][int(full[3][lo]):int(full[3][hi])].tobytes()
    assert (full[2][list(BAD)] == PAIR_BAD).all() and (full[1][list(BAD)] == 0).all()
    assert (full[2] & PAIR_ROWS_CUT).any() and full[1][1024:].sum() > 0 and full[1][LAUNCH:].sum() > 0
    assert not (full[0]["distance"] == TOP_UP).any()
    rows = host[2]
    assert (tm[drawn.slot[drawn.good]][..., 3].view(np.float32) == TOP_UP).any()   # the top-up entries are in the arrays, and are not delivered
    for sel in (everything, ratio):
        want = expect_drawn(drawn, sel)
        assert 0 < want[3][-1] and (sel is everything or want[3][-1] < full[3][-1])
        same_selection(device_select(B, ctx, triple, 2, sel), want)
    # a cut at a pair of the second launch
    c = int(np.flatnonzero(full[1][LAUNCH + 10:])[0]) + LAUNCH + 10
    cap = int(full[3][c + 1]) - 1
    want = expect_drawn(drawn, everything, matches_cap=cap)
    assert (want[2][c:] & ROWS_CUT).all() and not (want[2][:c] & ROWS_CUT).any() and want[3][-1] == full[3][c]
    capped_select(B, ctx, triple, 2, everything, cap, want)
    # the host form, into pinned memory
    total = int(full[3][-1])
    dst = B.HostMatches(NPAIRS, total, pinned=True)
    ticket = ctx.pair_matches_download(triple, 2, B.MatchSelect(*everything), dst)
    assert ctx.pair_matches_wait(ticket) == int((full[2] != 0).sum())
    same_selection(host_got(dst, NPAIRS), full)
    assert np.array_equal(dst.pair_rows[:NPAIRS], rows)


# ---- 2: wide train and query indices, the keys' limit, the largest distances -----------------------------------------------------

WIDE_NB, WIDE_NA = 70000, 65
WIDE_LIST_RADIUS, WIDE_DENSE_RADIUS = 42.0, 50.5


def wide_rows():
    """65 query rows against 70 000 train rows (16 bytes, random): exact copies above index 65 536, equal best distances at a low and
    a high index, second-best entries at high indices, the best of one row in the very last train row"""
    rng = np.random.default_rng(2201)
    t = rng.integers(0, 256, (WIDE_NB, 16), dtype=np.uint8)
    q = rng.integers(0, 256, (WIDE_NA, 16), dtype=np.uint8)
    plan = {"copy": {}, "tie": {}, "second": {}}
    for i in range(5):
        plan["copy"][i] = 65536 + 700 * i + 3
        t[plan["copy"][i]] = q[i]
    for i in range(5, 10):
        plan["tie"][i] = (100 + i, 66000 + i)
        t[100 + i], t[66000 + i] = flipped(q[i], [1, 2, 3]), flipped(q[i], [9, 70, 127])
    for i in range(10, 15):
        plan["second"][i] = (200 + i, 69000 + i)
        t[200 + i], t[69000 + i] = flipped(q[i], [5]), flipped(q[i], [7, 8])
    t[WIDE_NB - 1] = flipped(q[15], [0])
    return q, t, plan


def wide_wants(q, t, plan):
    """the oracle's rows of every mode of the wide pair, with the assertions that they reach indices of 2^16 and more"""
    w = {1: oracle_pair(q, t, 0, 1), 2: oracle_pair(q, t, 0, 2), "list": R.oracle_pair(q, t, 0, WIDE_LIST_RADIUS),
         "dense": R.oracle_pair(q, t, 0, WIDE_DENSE_RADIUS)}
    for i, at in plan["copy"].items():
        assert w[1][i][0]["trainIdx"] == at >= 65536 and w[1][i][0]["distance"] == 0
    for i, (low, high) in plan["tie"].items():                      # the same distance twice: the low index wins, the high one is second
        assert list(w[2][i]["trainIdx"]) == [low, high] and list(w[2][i]["distance"]) == [3, 3] and high >= 65536
    for i, (low, high) in plan["second"].items():
        assert list(w[2][i]["trainIdx"]) == [low, high] and high >= 65536
    assert w[1][15][0]["trainIdx"] == WIDE_NB - 1
    assert sum(int(r[0]["trainIdx"]) >= 65536 for r in w[1]) >= 6 and sum(int(r[1]["trainIdx"]) >= 65536 for r in w[2]) >= 10
    n_list = np.array([len(r) for r in w["list"]])
    assert n_list.max() <= LIST and (n_list > 2).any() and sum(int((r["trainIdx"] >= 65536).sum()) for r in w["list"]) >= 10
    n_dense = np.array([len(r) for r in w["dense"]])
    assert n_dense.min() > LIST and n_dense.min() > WIDE_CAPS[0] and n_dense.max() < WIDE_CAPS[1]
    for cap in WIDE_CAPS:                                            # high indices among the stored entries, under both caps
        assert sum(int((r[:cap]["trainIdx"] >= 65536).sum()) for r in w["dense"]) >= 10
    return w


WIDE_CAPS = (16, 1024)      # cap_per_query below and above the hits of every row at WIDE_DENSE_RADIUS


@pytest.fixture(scope="module")
def wide(B):
    q, t, plan = wide_rows()
    rng = np.random.default_rng(1)
    return {"Q": one_frame(B, rng, q), "T": one_frame(B, rng, t), "want": wide_wants(q, t, plan), "ctx": B.default_context(0)}


@pytest.mark.parametrize("mode", ["k1", "k2", "list", "dense_cut", "dense_all"])
def test_train_indices_beyond_16_bits(B, wide, mode):
    ctx, Q, T, w = wide["ctx"], wide["Q"], wide["T"], wide["want"]
    if mode in ("k1", "k2"):
        k = int(mode[1])
        host, _ = run(B, ctx, Q, T, [(0, 0)], k, WIDE_NA + 5)
        same_padded(host, 0, w[k], WIDE_NA)
    elif mode == "list":
        host, _ = run(B, ctx, Q, T, [(0, 0)], 8, WIDE_NA + 5, radius=WIDE_LIST_RADIUS)
        same_padded(host, 0, w["list"], WIDE_NA)
    else:
        host, _ = run(B, ctx, Q, T, [(0, 0)], WIDE_CAPS[mode == "dense_all"], WIDE_NA, radius=WIDE_DENSE_RADIUS)
        same_padded(host, 0, w["dense"], WIDE_NA)


CROSS_NA, CROSS_CAP = 70000, 64


def cross_rows():
    """frame a: 70 000 rows of which the first 64 are matched; frame b: 64 rows.  Row q < 32 of a has its partner in row q of b at
    distance 2.  q < 12: a row beyond index 65 536 of a is nearer to that partner - the match is dropped; 12 <= q < 16: such a row at
    the SAME distance - the lower index q wins, the match is kept"""
    rng = np.random.default_rng(2202)
    a = rng.integers(0, 256, (CROSS_NA, 16), dtype=np.uint8)
    b = rng.integers(0, 256, (CROSS_CAP, 16), dtype=np.uint8)
    for q in range(32):
        b[q] = flipped(a[q], [3, 40 + q])
    for q in range(12):                                              # (q < 6: at 2^16 + q, whose low 16 bits are q itself)
        a[65536 + (q if q < 6 else 300 * q + 7)] = flipped(b[q], [100]) if q % 2 else b[q]
    for q in range(12, 16):
        a[66000 + q] = flipped(b[q], [60, 61])
    return a, b


def cross_want(a, b):
    want = oracle_cross(a, b, 0)[:CROSS_CAP]
    fwd = oracle_pair(a[:CROSS_CAP], b, 0, 1)
    back = O.match_knn(b, [a], 1)
    partner = [int(back[int(f[0]["trainIdx"])][0]["trainIdx"]) for f in fwd]
    assert all(len(want[q]) == 0 and partner[q] >= 65536 for q in range(12))       # dropped for a backward partner beyond 2^16
    assert all(partner[q] == 65536 + q for q in range(6))
    assert all(len(want[q]) == 1 and want[q][0]["trainIdx"] == q for q in range(12, 32))
    assert 0 < sum(len(w) for w in want) < CROSS_CAP
    return want


def test_cross_check_over_a_long_query_frame(B):
    a, b = cross_rows()
    want = cross_want(a, b)
    rng = np.random.default_rng(2)
    ctx = B.default_context(0)
    host, _ = run(B, ctx, one_frame(B, rng, a), one_frame(B, rng, b), [(0, 0)], 1, CROSS_CAP, cross=True)
    same_padded(host, 0, want, CROSS_NA)                            # (pair_rows: the true count)


LIMIT = (1 << IDX_BITS) - 1         # the most train rows a pair may have


def limit_rows():
    """two query rows against 2^22 - 1 train rows from ONE generator call; the best and second-best rows of both queries are the
    last two (indices 2^22 - 2 and 2^22 - 3), and 38 more rows in front of them lie nearer than any random row"""
    rng = np.random.default_rng(2203)
    t = rng.integers(0, 256, (LIMIT, 16), dtype=np.uint8)
    q0 = rng.integers(0, 256, 16, dtype=np.uint8)
    q = np.stack([q0, flipped(q0, [127])])
    t[LIMIT - 1] = q0
    t[LIMIT - 2] = flipped(q0, [0, 1])
    for j in range(38):
        t[LIMIT - 3 - j] = flipped(q0, [8 + i for i in range(4 + j % 5)])
    return q, t


@pytest.fixture(scope="module")
def limit(B):
    import torch
    q, t = limit_rows()
    want = {1: oracle_pair(q, t, 0, 1), 2: oracle_pair(q, t, 0, 2), "list": R.oracle_pair(q, t, 0, 3.5), "dense": R.oracle_pair(q, t, 0, 10.0)}
    for r in want[2]:
        assert list(r["trainIdx"]) == [LIMIT - 1, LIMIT - 2] == [(1 << IDX_BITS) - 2, (1 << IDX_BITS) - 3]
    assert [list(r["trainIdx"]) for r in want["list"]] == [[LIMIT - 1, LIMIT - 2]] * 2
    assert [len(r) for r in want["dense"]] == [40, 40] and all(r["trainIdx"].min() == LIMIT - 40 for r in want["dense"])
    rng = np.random.default_rng(3)
    d_t, d_n = torch.from_numpy(t).cuda(), torch.tensor([LIMIT], dtype=torch.int32).cuda()
    T = types.SimpleNamespace(dim=16, keep=(d_t, d_n), set=B.DescSet(d_t.data_ptr(), d_n.data_ptr(), 1, LIMIT * 16, 16, 1))
    return {"Q": one_frame(B, rng, q), "T": T, "want": want, "ctx": B.default_context(0)}


@pytest.mark.parametrize("mode", ["k1", "k2", "list", "dense"])
def test_the_most_train_rows_the_keys_hold(B, limit, mode):
    ctx, Q, T, w = limit["ctx"], limit["Q"], limit["T"], limit["want"]
    if mode in ("k1", "k2"):
        host, _ = run(B, ctx, Q, T, [(0, 0)], int(mode[1]), 3)
        same_padded(host, 0, w[int(mode[1])], 2)
    elif mode == "list":
        for cpq in (1, 3):
            host, _ = run(B, ctx, Q, T, [(0, 0)], cpq, 3, radius=3.5)
            same_padded(host, 0, w["list"], 2)
    else:
        for cpq in (8, 48):
            host, _ = run(B, ctx, Q, T, [(0, 0)], cpq, 3, radius=10.0)
            same_padded(host, 0, w["dense"], 2)


def test_a_count_the_keys_do_not_hold(B):
    """a count of exactly 2^22 while the frame's buffer holds 64 rows: as a train frame (and as a query frame under the cross check)
    the pair is refused before a row is read; as a query frame of a plain call its first rows_cap rows are matched"""
    import torch
    rng = np.random.default_rng(2204)
    ctx = B.default_context(0)
    S = SynthSet(B, rng, 16, 16, [64, 64, 64], 64, count_stride=2)
    torch.cuda.synchronize()
    S.t_cnt[2] = 1 << IDX_BITS                                      # frame 1 claims 2^22 rows
    torch.cuda.synchronize()
    plist = [(0, 2), (0, 1), (1, 0), (2, 0)]
    for per, radius, cross in ((1, None, False), (2, None, False), (1, None, True), (3, 40.5, False)):
        host, triple = run(B, ctx, S, S, plist, per, 64, radius=radius, cross=cross)
        m, cnt, rows = host
        back = cross                                                 # the cross check's keys index frame a too
        assert list(rows) == [64, -1, -1 if back else 1 << IDX_BITS, 64]
        for p, (a, b) in enumerate(plist):
            if rows[p] == -1:
                assert (cnt[p] == SENTINEL).all() and (m[p] == SENTINEL).all()
                continue
            dq, dt = S.desc[a], S.desc[b]
            want = R.oracle_pair(dq, dt, b, radius) if radius else (oracle_cross(dq, dt, b) if cross else oracle_pair(dq, dt, b, per))
            same_padded(host, p, want, int(rows[p]))
        if cross:
            continue
        sel = (INF, 0.0, per)
        want = expect((m.reshape(-1).view(O.DMATCH).reshape(len(plist), 64, per), cnt, rows), per, sel)
        assert want[2][1] == PAIR_BAD and want[1][1] == 0 and want[2][2] & PAIR_ROWS_CUT and want[1][2] > 0
        same_selection(device_select(B, ctx, triple, per, sel), want)


def far_sets(B, dim):
    """a query frame {q, ~q} and three train frames: the complement of q alone; 40 complements and one row 5 bits nearer; 5
    complements and one row 5 bits nearer"""
    rng = np.random.default_rng(2205 + dim)
    q = rng.integers(0, 256, dim, dtype=np.uint8)
    far, near = ~q, flipped(~q, [1, 9, 17, 8 * dim - 1, 8 * dim - 2])
    t1, t2 = np.tile(far, (41, 1)), np.tile(far, (6, 1))
    t1[17], t2[4] = near, near
    Q = SynthSet(B, rng, dim, dim, [2], 2, count_stride=1, prepared={0: np.stack([q, far])})
    T = SynthSet(B, rng, dim, dim + 4, [1, 41, 6], 41, prepared={0: far[None], 1: t1, 2: t2})
    return Q, T


@pytest.mark.parametrize("dim", [16, 48, 64])
def test_the_largest_distance(B, dim):
    ctx = B.default_context(0)
    Q, T = far_sets(B, dim)
    top = 8 * dim
    plist = [(0, 0), (0, 1), (0, 2)]
    for k in (1, 2):
        want = [oracle_pair(Q.desc[0], T.desc[b], b, k) for b in range(3)]
        assert want[0][0][0]["distance"] == top and want[0][1][0]["distance"] == 0
        assert [int(r["trainIdx"]) for r in want[1][0]] == [17, 0][:k] and [int(r["distance"]) for r in want[1][0]] == [top - 5, top][:k]
        if k == 2:
            assert want[0][0][1]["distance"] == TOP_UP               # one train row: the top-up entry behind the largest distance
        host, _ = run(B, ctx, Q, T, plist, k, 2)
        for p in range(3):
            same_padded(host, p, want[p], 2)
    for radius, cpq in ((float(top), 8), (top + 0.5, 8), (top + 0.5, 48), (1e9, 48), (INF, 48), (INF, 3)):
        want = [R.oracle_pair(Q.desc[0], T.desc[b], b, radius) for b in range(3)]
        hits = [len(w[0]) for w in want]                             # of the row q: every complement is at the largest distance
        assert hits == ([0, 1, 1] if radius == top else [1, 41, 6])  # strict at 8 * dim; above it the dense path (41) and the list (6)
        assert radius == top or (want[2][0]["distance"][-1] == top and want[2][0]["distance"][0] == top - 5)
        host, _ = run(B, ctx, Q, T, plist, cpq, 2, radius=radius)
        for p in range(3):
            same_padded(host, p, want[p], 2)


# ---- 3: the exit beyond 1 024 workgroup sums, and at workgroup boundaries -----------------------------------------------------------

MANY_SUMS_PAIRS, MANY_SUMS_CAP = 350, 700                            # 3 workgroups of 256 rows per pair: 1 050 sums, 2 per thread
EDGE_ROWS = [255, 256, 257, 511, 512, 513, 700, 701]


def padded_arrays(per_row, seed):
    """padded arrays as a matcher leaves them, built in numpy: sorted distances in the stored entries of the stored rows, random
    bits everywhere else (never read); counts 0, negative, up to per_row + 3; some top-up entries; pair_rows -1, 0, above rows_cap"""
    rng = np.random.default_rng(seed)
    npairs, cap = MANY_SUMS_PAIRS, MANY_SUMS_CAP
    rows = rng.integers(1, 40, npairs).astype(np.int32)
    rows[rng.choice(npairs, 30, replace=False)] = rng.integers(200, 700, 30)
    at = np.linspace(3, npairs - 4, len(EDGE_ROWS)).astype(int)
    rows[at] = EDGE_ROWS
    rows[at + 1] = 0                                                 # an empty pair behind each of them
    rows[[40, 41, 42, 170]] = [0, -1, 0, -1]
    rows[[99, 345]] = [5000, 1 << 22]
    rows[npairs - 1] = 300
    m = rng.integers(-2 ** 31, 2 ** 31, (npairs, cap, per_row, 4)).astype(np.int32).reshape(-1).view(O.DMATCH).reshape(npairs, cap, per_row)
    cnt = rng.integers(-2 ** 31, 2 ** 31, (npairs, cap)).astype(np.int32)
    for p in range(npairs):
        n = min(max(int(rows[p]), 0), cap)
        c = rng.choice([0, 0, 1, per_row, per_row, per_row, per_row + 3, -1, -7], n).astype(np.int32)
        cnt[p, :n] = c
        d = np.sort(rng.integers(0, 200, (n, per_row)), axis=1).astype(np.float32)
        d[rng.integers(0, 25, n) == 0, 1:] = TOP_UP                  # rows of one real entry, the rest topped up
        m[p, :n]["distance"] = d
        m[p, :n]["queryIdx"] = np.arange(n)[:, None]
        m[p, :n]["imgIdx"] = p
        m[p, :n]["trainIdx"] = rng.integers(0, 1 << 22, (n, per_row))
    return m, cnt, rows


@pytest.fixture(scope="module")
def sums(B):
    """per_row -> the arrays on the host and on the device"""
    import torch
    bpp = -(-MANY_SUMS_CAP // 256)
    out = {"ctx": B.default_context(0), "first_beyond": -(-1024 // bpp)}         # the first pair all of whose sums lie behind the 1 024th
    memo = {}

    def uncut(per_row, sel):                                         # (computed once per selection)
        if (per_row, sel) not in memo:
            memo[per_row, sel] = expect(out[per_row][0], per_row, sel)
        return memo[per_row, sel]
    out["expect"] = uncut
    for per_row in (2, 4):
        host = padded_arrays(per_row, 3300 + per_row)
        m, cnt, rows = host
        triple = (torch.from_numpy(m.view(np.int32).reshape(m.shape + (4,))).cuda(), torch.from_numpy(cnt).cuda(), torch.from_numpy(rows).cuda())
        assert MANY_SUMS_PAIRS * bpp > 1024 and set(EDGE_ROWS) <= set(rows.tolist()) and {-1, 0}.issubset(rows.tolist()) and rows.max() > MANY_SUMS_CAP
        out[per_row] = (host, triple)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("per_row", [2, 4])
def test_more_sums_than_the_offsets_pass_has_threads(B, sums, per_row):
    ctx, (host, triple) = sums["ctx"], sums[per_row]
    sels = {2: [(INF, 0.0, 2), (INF, 0.8, 1), (100.0, 0.0, 2)], 4: [(INF, 0.0, 3)]}[per_row]
    for sel in sels:
        want = sums["expect"](per_row, sel)
        counts, flags = want[1], want[2]
        assert want[4] > 0 and counts[sums["first_beyond"]:].sum() > 0  # pairs whose sums lie behind the 1 024th give matches
        assert (flags & PAIR_BAD).any() and (flags & PAIR_ROWS_CUT).any() and (flags & PAIR_ENTRIES_CUT).any()
        assert sel[0] == INF and sel[1] == 0.0 or want[5] > 0           # the ratio test and the bound drop entries
        same_selection(device_select(B, ctx, triple, per_row, sel), want)


@pytest.mark.parametrize("case", ["exact", "one short", "empty successor"])
def test_matches_cap_cuts_of_many_sums(B, sums, case):
    ctx, (host, triple) = sums["ctx"], sums[2]
    sel = (INF, 0.0, 2)
    full = sums["expect"](2, sel)
    total, npairs = int(full[3][-1]), MANY_SUMS_PAIRS
    if case == "exact":
        cap, cut = total, npairs
    elif case == "one short":
        cap, cut = total - 1, int(np.flatnonzero(full[1])[-1])
    else:                                                            # the pair with 513 rows does not fit; its successor is empty
        cut = int(np.flatnonzero(host[2] == 513)[0])
        cap = int(full[3][cut + 1]) - 1
        assert full[1][cut] > 0 and full[1][cut + 1] == 0 and host[2][cut + 1] == 0
    want = expect(host, 2, sel, matches_cap=cap)
    assert (want[2][cut:] & ROWS_CUT).all() and not (want[2][:cut] & ROWS_CUT).any() and want[3][-1] == full[3][cut]
    capped_select(B, ctx, triple, 2, sel, cap, want)


def test_many_sums_through_the_bounce_buffer(B, sums):
    per_row = 4
    ctx, (host, triple) = sums["ctx"], sums[per_row]
    sel = (INF, 0.0, per_row)
    want = sums["expect"](per_row, sel)
    dst = B.HostMatches(MANY_SUMS_PAIRS, int(want[3][-1]), pinned=False)           # pageable: through the engine's bounce buffer
    dst.matches.view(np.int32)[:] = SENTINEL
    ticket = ctx.pair_matches_download(triple, per_row, B.MatchSelect(*sel), dst)
    assert ctx.pair_matches_wait(ticket) == int((want[2] != 0).sum())
    same_selection(host_got(dst, MANY_SUMS_PAIRS), want)
    assert np.array_equal(dst.pair_rows[:MANY_SUMS_PAIRS], host[2])


# ---- 4: exactly 32 and 33 radius hits ---------------------------------------------------------------------------------------------

EDGE_RADIUS = 10.0
EDGE_HITS = [31, 32, 33, 64, 0]


def edge_rows():
    """48-byte rows.  Queries 0, 1, 2 = a centre C with 4, 2, 0 bits inverted (bits no train row touches), query 3 = another centre
    D, query 4 random.  36 train rows are C with f other bits inverted - distance f + 4 / f + 2 / f to queries 0 / 1 / 2: 31 with
    f <= 5, one with f = 7, one with f = 9, three with f >= 10 - and 64 are D with 0 ... 9 bits inverted, in shuffled order.  At
    radius 10 (strict) the queries have 31, 32, 33, 64 and 0 hits.  Returns the queries, the train rows and the train row that
    only query 2 hits"""
    rng = np.random.default_rng(2206)
    C, D = rng.integers(0, 256, 48, dtype=np.uint8), rng.integers(0, 256, 48, dtype=np.uint8)
    q = np.stack([flipped(C, [380, 381, 382, 383]), flipped(C, [380, 381]), C, D, rng.integers(0, 256, 48, dtype=np.uint8)])
    fs = [i % 6 for i in range(31)] + [7, 9, 10, 11, 30]
    rows = [flipped(C, rng.choice(370, f, replace=False)) for f in fs]
    rows += [flipped(D, rng.choice(384, i % 10, replace=False)) for i in range(64)]
    order = rng.permutation(100)
    t = np.stack(rows)[order]
    only2 = int(np.flatnonzero(order == 32)[0])                      # the row with f = 9
    return q, t, only2


def edge_kps(B, rng, q_n, t_n, moved):
    """all keypoints at the origin but train row `moved`, 100 pixels away"""
    import torch
    Qk, Tk = SynthKp(B, rng, [q_n], q_n), SynthKp(B, rng, [t_n], t_n)
    for K, n in ((Qk, q_n), (Tk, t_n)):
        K.kps[0]["x"], K.kps[0]["y"], K.kps[0]["octave"] = 0.0, 0.0, 0
    Tk.kps[0]["x"][moved] = 100.0
    for K in (Qk, Tk):                                               # (the calls synchronise before they start)
        K.t_buf[:K.kps[0].nbytes] = torch.from_numpy(K.kps[0].view(np.uint8).copy()).cuda()
    settled()
    return Qk, Tk


def test_exactly_32_and_33_radius_hits(B):
    q, t, only2 = edge_rows()
    want = R.oracle_pair(q, t, 0, EDGE_RADIUS)
    assert [len(w) for w in want] == EDGE_HITS and LIST in EDGE_HITS and LIST + 1 in EDGE_HITS
    assert only2 in want[2]["trainIdx"] and all(only2 not in want[i]["trainIdx"] for i in (0, 1, 3, 4))
    rng = np.random.default_rng(4)
    ctx = B.default_context(0)
    Q, T = one_frame(B, rng, q), one_frame(B, rng, t)
    Qk, Tk = edge_kps(B, rng, len(q), len(t), only2)
    window = (-4.0, 4.0, -INF, INF, -1)
    M = gate_mask(window, Qk.kps[0], Tk.kps[0])
    assert M.sum() == M.size - len(q) and not M[:, only2].any()      # the gate forbids that one train row, nothing else
    behind = G.oracle_radius(q, t, M, 0, EDGE_RADIUS)
    assert [len(w) for w in behind] == [31, 32, 32, 64, 0]           # query 2 is back on the list path
    all_pass = G.oracle_radius(q, t, gate_mask(G.ALL_PASS, Qk.kps[0], Tk.kps[0]), 0, EDGE_RADIUS)
    assert [w.tobytes() for w in all_pass] == [w.tobytes() for w in want]
    for cpq in (40, 8):
        host, _ = run(B, ctx, Q, T, [(0, 0)], cpq, len(q) + 2, radius=EDGE_RADIUS)
        same_padded(host, 0, want, len(q))
        host, _ = run(B, ctx, Q, T, [(0, 0)], cpq, len(q) + 2, radius=EDGE_RADIUS, gate=G.ALL_PASS, qk=Qk, tk=Tk)
        same_padded(host, 0, all_pass, len(q))
        host, _ = run(B, ctx, Q, T, [(0, 0)], cpq, len(q) + 2, radius=EDGE_RADIUS, gate=window, qk=Qk, tk=Tk)
        same_padded(host, 0, behind, len(q))

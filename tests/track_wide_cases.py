"""The chains of tests/test_gpu_tracks_wide.py: the tracker where its counts get wide - more nodes than one launch holds (grid.y =
65 535), more records in a pair than its launch has lanes, rows, train rows and seeds beyond 65 536, more points than one trip of
the points kernel, and list capacities that end exactly on a workgroup's running total.  NumPy only: no torch, no GPU.  Every
builder returns its chain together with `conditions`, {what the input must reach: whether it does}, worked out with the
restatements (test_abi_tracks.restated_link / restated_list); tests/test_track_wide_cases.py asserts them without a GPU, so that a
changed seed or constant cannot make a GPU test vacuous unnoticed.  The builders are cached: one chain per process."""
import functools

import numpy as np

from test_abi_tracks import lims, restated_link, restated_list, restated_proposals
from test_gpu_tracks import make_chain, seed_arrays

ROWS_PER_GROUP = 256                      # rows (or records) of one workgroup of the row passes (TK_ROWS)
NODES_PER_LAUNCH = 65535                  # what grid.y holds
FIRST_NEW = 2 ** 40

# ---- 1 / 2: more nodes than one launch ------------------------------------------------------------------------------------------
NODE_SEED, NODE_CAP = 13, 8
NODE_LENGTHS = (65535, 65536, 65537)
NODES = NODE_LENGTHS[-1]
NODE_MIN_LENS = (1, 3)
SPLITS = (65534, 65535, 65536)

# ---- 3 / 4: rows wide -----------------------------------------------------------------------------------------------------------
WIDE_SEED, WIDE_CAP = 9, 70000
WIDE_ROWS = [70001, 69999, 70003]
WIDE_GROUPS = (WIDE_CAP + ROWS_PER_GROUP - 1) // ROWS_PER_GROUP            # 274 workgroups per node
WIDE_LANES = WIDE_GROUPS * ROWS_PER_GROUP                                  # 70 144 lanes per pair: one trip of the record loops
NAMED = (ROWS_PER_GROUP, 65536, WIDE_LANES)                                # record indices behind a pair's first: a workgroup seam,
#                                                                            workgroup 256, the second trip's first record
GAP_GROUP = 2                             # rows 512 .. 767 of node 0 head no piece of two rows: workgroup 3 follows a workgroup without
LANE0_ROW = (GAP_GROUP + 1) * ROWS_PER_GROUP                               # a listed head in lane 0 of workgroup 3
WIDE_GROUP = 260                          # a workgroup of node 0 with blockIdx.x >= 256
LANE255_ROW = WIDE_GROUP * ROWS_PER_GROUP + 255                            # a listed head in its last lane (row 66 815)
WIDE_MIN_LENS = (1, 2)
POINTS_PER_TRIP = 1024 * 256 // 9         # 29 127: point 29 127 has word 0 in the first trip of the points kernel, the rest in the second


class Case:
    """a chain on the host (node_rows, rows_cap, offsets, matches, the seeds st / sa), its restatements - computed once, on first
    use - and the conditions"""

    def __init__(self, node_rows, rows_cap, offsets, matches, st, sa):
        self.node_rows, self.rows_cap, self.offsets, self.matches, self.st, self.sa = list(node_rows), rows_cap, offsets, matches, st, sa
        self.conditions = {}
        self._link, self._list = {}, {}

    def link(self, nodes=None, seeded=False):
        """restated_link of the first `nodes` nodes as a chain of their own; seeded: with st / sa and first_new = 2^40"""
        nodes = nodes or len(self.node_rows)
        if (nodes, seeded) not in self._link:
            seed = (self.st, self.sa, FIRST_NEW) if seeded else (None, None, 0)
            self._link[nodes, seeded] = restated_link(self.node_rows[:nodes], self.rows_cap, self.offsets[:nodes], self.matches, *seed)
        return self._link[nodes, seeded]

    def list(self, min_len, nodes=None, seeded=False, tracks_cap=None, obs_cap=None):
        nodes = nodes or len(self.node_rows)
        key = (nodes, seeded, min_len, tracks_cap, obs_cap)
        if key not in self._list:
            self._list[key] = restated_list(self.node_rows[:nodes], self.rows_cap, *self.link(nodes, seeded)[:3], min_len, tracks_cap, obs_cap)
        return self._list[key]


def pair_counts(case, p):
    """(links, lost, ignored) of pair p alone"""
    lim = lims(case.node_rows, case.rows_cap)
    rec = case.matches[int(case.offsets[p]):int(case.offsets[p + 1])]
    ok, keys = restated_proposals(rec, lim[p + 1], lim[p])
    best = {}
    for j in np.flatnonzero(ok):
        t, k = int(rec["trainIdx"][j]), int(keys[j])
        best[t] = min(best.get(t, k), k)
    links = sum(1 for j in np.flatnonzero(ok) if best[int(rec["trainIdx"][j])] == int(keys[j]))
    return links, int(ok.sum()) - links, int((~ok).sum())


def heads_of(listed):
    """(node, row, observations) of every stored piece of a restated list"""
    o = listed[2]
    first = listed[3][o[:-1]] if len(o) > 1 else listed[3][:0]
    return first["node"].astype(np.int64), first["row"].astype(np.int64), np.diff(o)


@functools.lru_cache(maxsize=None)
def node_case(B):
    """65 537 nodes of 5 .. 10 rows at rows_cap 8, one track through all of them; the shorter lengths are its prefixes"""
    rng = np.random.default_rng(NODE_SEED)
    node_rows = [int(v) for v in rng.integers(5, 11, NODES)]
    offsets, m = make_chain(B, NODE_SEED, node_rows, through=True)
    st, sa = seed_arrays(rng, NODE_CAP)
    st[0] = -1                                                        # the through-track starts in this chain, seeded or not
    case = Case(node_rows, NODE_CAP, offsets, m, st, sa)
    prev, track, age, summary = case.link()
    last = NODES - 1
    c = case.conditions
    c["no empty node, some beyond rows_cap"] = min(node_rows) >= 5 and max(node_rows) > NODE_CAP
    c["the through-track has age 65 536 at the last node"] = age[last, last % 5] == last and track[last, last % 5] == track[0, 0] == 0
    full = case.list(1)
    hn, hr, n = heads_of(full)
    c["one listed piece of 65 537 rows"] = (n == NODES).sum() == 1 and full[1].max() == NODES and (hn[n == NODES] == 0).all()
    for p in (NODES - 3, NODES - 2):                                  # pairs 65 534 and 65 535: the last of the first launch, the second's
        links, lost, ignored = pair_counts(case, p)
        c["pair %d has links, a lost proposal and an ignored record" % p] = links > 0 and lost > 0 and ignored > 0
    for node in (NODES - 2, NODES - 1):
        c["heads start at node %d" % node] = (prev[node, :lims(node_rows, NODE_CAP)[node]] == -1).any()
    tail = hn + n - 1                                                 # the node of a piece's last row
    across = (n < NODES) & (hn <= NODES - 3) & (tail >= NODES - 1)
    c["another listed piece starts at or before node 65 534 and ends at or behind 65 536"] = across.any()
    l3 = case.list(3)
    hn3, _, n3 = heads_of(l3)
    c["... at min_len 3 too"] = ((n3 < NODES) & (hn3 <= NODES - 3) & (hn3 + n3 - 1 >= NODES - 1)).any()
    c["summary[5] is the sum of the limits"] = summary[5] == sum(lims(node_rows, NODE_CAP)) and summary[3] > 1000 and summary[4] > 1000
    c["the seeds continue tracks"] = (st[:5] >= 0).any()
    return case


# ---- the row-wide chain ---------------------------------------------------------------------------------------------------------

def firsts(q):
    """which records are the first of their query row"""
    f = np.ones(len(q), bool)
    f[1:] = q[1:] != q[:-1]
    return f


def two_record_rows(rec, lim_q, lim_t):
    """indices i with: record i the first of its row and a proposal, record i + 1 its second and last"""
    q = rec["queryIdx"]
    f = firsts(q)
    i = np.flatnonzero(f[:-1] & ~f[1:] & restated_proposals(rec, lim_q, lim_t)[0][:-1])
    return i[(i + 2 >= len(q)) | f[np.minimum(i + 2, len(q) - 1)]]


def first_record_of(rec, row, lim):
    """the index of the first record of the first query row >= `row` that exists (< lim)"""
    q = rec["queryIdx"]
    i = np.flatnonzero(firsts(q) & (q >= row) & (q < lim))
    return int(i[0])


def put_row_at(rec, k, second, lim_q, lim_t):
    """deletes the records between index k (k - 1 with `second`) and the next row of two records: that row's second (first) record
    then has index k"""
    at = k - 1 if second else k
    rows = two_record_rows(rec, lim_q, lim_t)
    i = int(rows[rows >= at][0])
    return np.concatenate([rec[:at], rec[i:]])


@functools.lru_cache(maxsize=None)
def wide_case(B):
    """3 nodes of about 70 000 rows: make_chain's lists, plus by hand
    - pair 1: a row of two records whose SECOND record has index 256, 65 536, 70 144 and the last of the pair's range;
    - pair 0: such a row whose FIRST record has those indices - the last record of pair 0 and the first of pair 1 name one query row,
      and the latter proposes: it is the first of its range;
    - pair 1: proposals with query and train rows >= 65 536, one that wins alone and two that tie on the distance;
    - pair 0: no proposal for the rows of workgroup 2 of node 0, winners for row 768 (lane 0 of workgroup 3) and row 66 815 (lane
      255 of workgroup 260)."""
    offsets, m = make_chain(B, WIDE_SEED, WIDE_ROWS)
    lim = lims(WIDE_ROWS, WIDE_CAP)
    p0, p1 = m[int(offsets[0]):int(offsets[1])].copy(), m[int(offsets[1]):int(offsets[2])].copy()
    hand = {}
    # pair 0, contents: the gap and the two planted heads
    gap = (p0["trainIdx"] >= GAP_GROUP * ROWS_PER_GROUP) & (p0["trainIdx"] < LANE0_ROW)
    p0["trainIdx"][gap] = -1
    for name, row, train in (("lane0", 1000, LANE0_ROW), ("lane255", 66000, LANE255_ROW)):
        i = first_record_of(p0, row, lim[1])
        p0["trainIdx"][i], p0["distance"][i] = train, 0.25
        hand[name] = (int(p0["queryIdx"][i]), train)
    # pair 1, contents: wide proposals
    for name, row, train, d in (("win", 66000, 66001, 0.25), ("tie_a", 67000, 68000, 0.5), ("tie_b", 67100, 68000, 0.5)):
        i = first_record_of(p1, row, lim[2])
        p1["trainIdx"][i], p1["distance"][i] = train, d
        hand[name] = (int(p1["queryIdx"][i]), train)
    # the last record of pair 0: the first of a row of two that pair 1 does not name; that row's second comes first in pair 1
    rows = two_record_rows(p0, lim[1], lim[0])
    ok = rows[~np.isin(p0["queryIdx"][rows], p1["queryIdx"])]
    i = int(ok[-1])
    shared = int(p0["queryIdx"][i])
    p0 = p0[:i + 1]
    head = np.zeros(1, B.DMATCH)
    head[0] = (shared, 69000, 1, 0.75)
    p1 = np.concatenate([head, p1])
    hand["shared"] = shared
    # the rows of two records at the named indices
    for k in NAMED:
        p0 = put_row_at(p0, k, False, lim[1], lim[0])
        p1 = put_row_at(p1, k, True, lim[2], lim[1])
    p1 = p1[:int(two_record_rows(p1, lim[2], lim[1])[-1]) + 2]
    m = np.concatenate([p0, p1])
    offsets = np.array([0, len(p0), len(p0) + len(p1)], np.int64)
    rng = np.random.default_rng(WIDE_SEED)
    st, sa = seed_arrays(rng, WIDE_CAP)
    case = Case(WIDE_ROWS, WIDE_CAP, offsets, m, st, sa)
    case.hand = hand
    wide_conditions(case, p0, p1, lim)
    case.cuts = wide_cuts(case)
    return case


def wide_conditions(case, p0, p1, lim):
    c, hand = case.conditions, case.hand
    c["both pairs hold more records than their launch has lanes"] = len(p0) > WIDE_LANES + 1000 and len(p1) > WIDE_LANES + 1000
    q0, q1 = p0["queryIdx"], p1["queryIdx"]
    ok0, _ = restated_proposals(p0, lim[1], lim[0])
    ok1, _ = restated_proposals(p1, lim[2], lim[1])
    for ok, q, p in ((ok0, q0, 0), (ok1, q1, 1)):
        c["no query row of pair %d proposes twice" % p] = len(np.unique(q[ok])) == int(ok.sum())
    for k in NAMED + (len(p1) - 1,):
        c["pair 1: record %d is the second of a row of two whose first proposes" % k] = bool(
            q1[k] == q1[k - 1] and q1[k - 2] != q1[k - 1] and (k + 1 == len(q1) or q1[k + 1] != q1[k]) and ok1[k - 1] and q1[k] != 0)
    for k in NAMED:
        c["pair 0: record %d is the first of a row of two and proposes" % k] = bool(
            q0[k] == q0[k + 1] and q0[k - 1] != q0[k] and q0[k + 2] != q0[k] and ok0[k] and q0[k] != 0)
    c["the last record of pair 0 and the first of pair 1 name one row, and both propose"] = bool(
        q0[-1] == q1[0] == hand["shared"] and q0[-2] != q0[-1] and ok0[-1] and ok1[0])
    prev, track, age, summary = case.link()
    sp, strack, sage, ssum = case.link(seeded=True)
    (qw, tw), (qa, ta), (qb, tb) = hand["win"], hand["tie_a"], hand["tie_b"]
    c["a proposal with query and train row >= 65 536 wins"] = min(qw, tw) >= 65536 and prev[2, qw] == tw
    c["two such proposals tie on the distance: the smaller query row wins"] = bool(
        min(qa, qb, ta) >= 65536 and ta == tb and qa < qb and prev[2, qa] == ta and prev[2, qb] == -1)
    c["many lost proposals, many ignored records"] = summary[3] > 40000 and summary[4] > 40000
    rows = np.arange(65536, lim[0])
    claimed = np.zeros(WIDE_CAP, bool)
    claimed[prev[1, :lim[1]][prev[1, :lim[1]] >= 0]] = True
    cont = rows[(case.st[rows] >= 0) & claimed[rows]]
    c["seeds at rows >= 65 536 continue tracks into node 1"] = len(cont) > 100 and bool(
        (strack[1][sp[1] == cont[0]] == case.st[cont[0]]).all() and (sage[1][sp[1] == cont[0]] == case.sa[cont[0]] + 1).all())
    c["lists of more points than one trip of the points kernel"] = all(
        int(case.list(n, seeded=s)[4][1]) > POINTS_PER_TRIP + 1 for n in WIDE_MIN_LENS for s in (False, True))
    (q, t) = hand["lane0"]
    c["row 768 of node 0 is won"] = prev[1, q] == t == LANE0_ROW
    (q, t) = hand["lane255"]
    c["row 66 815 of node 0 is won by a row >= 65 536"] = prev[1, q] == t == LANE255_ROW and q >= 65536


def wide_cuts(case):
    """the capacities of case 4 on the unseeded link at min_len 2: [(tracks_cap, obs_cap, what)], every one with the restated list
    under it in case.list(2, tracks_cap=..., obs_cap=...)"""
    full = case.list(2)
    hn, hr, n = heads_of(full)
    pieces, obs = int(full[4][0]), int(full[4][1])
    grp = hn * WIDE_GROUPS + hr // ROWS_PER_GROUP
    ngroups = len(case.node_rows) * WIDE_GROUPS
    per_p = np.bincount(grp, minlength=ngroups)
    per_o = np.bincount(grp, weights=n, minlength=ngroups).astype(np.int64)
    cum_p, cum_o = np.concatenate([[0], np.cumsum(per_p)]), np.concatenate([[0], np.cumsum(per_o)])
    after_gap = [g for g in range(1, ngroups) if per_p[g] > 0 and per_p[g - 1] == 0]
    groups = {"after a workgroup without pieces": after_gap[0] if after_gap else -1, "blockIdx.x >= 256": WIDE_GROUP,
              "the last with pieces": int(np.flatnonzero(per_p)[-1])}
    cuts = []
    for what, g in groups.items():
        for cap in (cum_p[g], cum_p[g] + 1, cum_p[g + 1] - 1, cum_p[g + 1]):
            cuts.append((int(cap), obs, "tracks_cap, workgroup %s" % what))
        for cap in (cum_o[g], cum_o[g] + 1, cum_o[g + 1] - 1, cum_o[g + 1]):
            cuts.append((pieces, int(cap), "obs_cap, workgroup %s" % what))
    ga = groups["after a workgroup without pieces"]
    cuts.append((int(cum_p[WIDE_GROUP + 1] - 1), int(cum_o[ga + 1] - 1), "both bind, in two workgroups"))
    c = case.conditions
    c["workgroup 3 of node 0 has pieces, workgroup 2 none"] = ga == GAP_GROUP + 1
    c["the three workgroups differ and hold several pieces each"] = len(set(groups.values())) == 3 and all(per_p[g] > 3 for g in groups.values())
    c["the last workgroup with pieces is the last of node 1"] = groups["the last with pieces"] == 2 * WIDE_GROUPS - 1
    lanes, bound = [], []
    for tcap, ocap, what in cuts:
        w = case.list(2, tracks_cap=tcap, obs_cap=ocap)
        stored = int(w[4][2])
        if stored < pieces:
            lanes.append(int(hr[stored]) % ROWS_PER_GROUP)
            bound.append((stored + 1 > tcap, int(w[2][-1]) + int(n[stored]) > ocap))
    case.left_out_lanes = lanes
    c["the first piece left out sits in lane 0 once"] = 0 in lanes
    c["... in lane 255 once"] = 255 in lanes
    c["... in a lane between once"] = any(0 < v < 255 for v in lanes)
    c["most capacities cut, some by pieces, some by observations"] = len(lanes) >= 18 and (True, False) in bound and (False, True) in bound
    both = case.list(2, tracks_cap=cuts[-1][0], obs_cap=cuts[-1][1])
    c["both bind: the observations cut first"] = int(both[4][2]) < cuts[-1][0] and int(both[4][3]) == 1
    return cuts

"""The inputs of tests/test_gpu_tracks_wide.py reach the cases they are built for - asserted on the restatements alone, without a
GPU: the committed seeds and constants are verified here.  The builders (tests/track_wide_cases.py) need no torch."""
import numpy as np

import ethzasl_brisk_amd as B
import track_wide_cases as W
from test_abi_tracks import lims


def test_the_builders_need_no_torch():
    src = open(W.__file__).read()
    top = [ln for ln in src.splitlines() if ln.startswith(("import ", "from "))]
    assert top and not any("torch" in ln for ln in top)


def test_the_constants_are_the_kernels():
    """the launch seams as csrc/brisk_track.hip and csrc/brisk_track_export.hip have them"""
    import os
    csrc = os.path.join(os.path.dirname(os.path.abspath(B.__file__)), "csrc")
    track, export = open(os.path.join(csrc, "brisk_track.hip")).read(), open(os.path.join(csrc, "brisk_track_export.hip")).read()
    assert "#define TK_ROWS %d " % W.ROWS_PER_GROUP in track and track.count("+= %d)" % W.NODES_PER_LAUNCH) == 10
    assert "#define TX_THREADS 256" in export and "#define TX_MAX_BLOCKS 1024 " in export and B.TRACK_POINT.itemsize == 36
    assert W.POINTS_PER_TRIP == 29127 and W.WIDE_GROUPS == 274 and W.WIDE_LANES == 70144
    assert W.NODE_LENGTHS == (W.NODES_PER_LAUNCH, W.NODES_PER_LAUNCH + 1, W.NODES_PER_LAUNCH + 2)
    assert W.SPLITS == (W.NODES_PER_LAUNCH - 1, W.NODES_PER_LAUNCH, W.NODES_PER_LAUNCH + 1)


def test_more_nodes_than_one_launch():
    """65 537 nodes: the through-track, pieces, lost proposals, ignored records and new heads on both sides of every cut of the
    node loops (before node 65 535, before pair 65 535, before node 65 536)"""
    case = W.node_case(B)
    assert len(case.node_rows) == 65537 and case.rows_cap == 8 and set(case.node_rows) == {5, 6, 7, 8, 9, 10}
    assert all(case.offsets[p] < case.offsets[p + 1] for p in range(len(case.node_rows) - 1))          # no empty pair
    bad = [name for name, holds in case.conditions.items() if not holds]
    assert not bad and len(case.conditions) >= 11, bad
    # the shorter lengths are prefixes, restated on their own: the same rows, other summaries
    long_ = case.link()
    for n in W.NODE_LENGTHS[:2]:
        short = case.link(n)
        assert short[1].tobytes() == long_[1][:n].tobytes() and short[3][1] < long_[3][1] and short[3][5] == sum(lims(case.node_rows[:n], 8))


def test_rows_wide():
    """three nodes of about 70 000 rows: the hand-made records sit where the record loops have their seams, and the capacities of
    the cut runs end on the running totals of three workgroups"""
    case = W.wide_case(B)
    assert case.node_rows == [70001, 69999, 70003] and case.rows_cap == 70000
    bad = [name for name, holds in case.conditions.items() if not holds]
    assert not bad and len(case.conditions) >= 26, bad
    assert len(case.cuts) == 25 and len(set(case.cuts)) == 25
    # every run's expectation carries the true totals; a run is cut iff a capacity is below them
    full = case.list(2)
    pieces, obs = int(full[4][0]), int(full[4][1])
    for tcap, ocap, what in case.cuts:
        w = case.list(2, tracks_cap=tcap, obs_cap=ocap)
        assert w[4][:2].tolist() == [pieces, obs] and int(w[4][2]) <= tcap and int(w[2][-1]) <= ocap, what
        assert int(w[4][3]) == (int(w[4][2]) < pieces), what
    assert sorted(set(case.left_out_lanes))[0] == 0 and sorted(set(case.left_out_lanes))[-1] == 255
    # the figures the chain was chosen by (make_chain's own lists, before the hand-made records: 167 587 records, 50 050 lost)
    s = case.link()[3]
    print("records %d, lost %d, ignored %d; min_len 2: %d pieces, %d observations" % (len(case.matches), s[3], s[4], pieces, obs))
    assert abs(len(case.matches) - 167587) < 100 and abs(int(s[3]) - 50050) < 200 and np.isin(case.offsets[1:3] - case.offsets[0:2] > 70144, True).all()

"""CPU checks of what test_gpu_batch_scale.py rests on (batch_scale_lib.py, the committed seeds): the frames of a batch all
differ, frames 8 apart differ in what the oracle describes, the special frames are where the GPU tests need them, and the
NumPy statement of the export rule agrees with a frame-by-frame loop."""
import numpy as np
import pytest

import batch_scale_lib as S

NS = (257, 1024, 1025, 2048, 2049)   # frames per launch of the GPU tests (128 x 96)
W, H = 128, 96


@pytest.fixture(scope="module")
def counts():
    """{n: (detected, described) counts per frame}; the oracle runs once per frame index and kind"""
    out = {}
    for n in sorted(NS, reverse=True):
        o = S.oracle(n, W, H)
        out[n] = (np.array([len(x[0]) for x in o]), np.array([len(x[1]) for x in o]))
    return out


@pytest.mark.parametrize("n,w,h", [(n, W, H) for n in NS] + [(1025, 120, 90)])
def test_all_frames_of_a_batch_differ(n, w, h):
    fr = S.frames(n, w, h)
    assert fr.shape == (n, h, w) and fr.dtype == np.uint8
    assert len({f.tobytes() for f in fr}) == n


@pytest.mark.parametrize("n", NS)
def test_described_counts_differ_between_frames_8_apart(counts, n):
    """a residue-class mix-up (frame f ^ 8 or f + 8 in place of f) changes the described count of at least 90 % of the
    ordinary frames: a condition on the inputs, from the oracle's counts alone"""
    nd = counts[n][1]
    ordinary = S.kinds(n) == S.ORDINARY
    for name, other in (("f ^ 8", lambda f: f ^ 8), ("f + 8", lambda f: f + 8)):
        pairs = [(f, other(f)) for f in range(n) if other(f) < n and ordinary[f] and ordinary[other(f)]]
        differ = sum(int(nd[a] != nd[b]) for a, b in pairs)
        print(n, name, differ, len(pairs))
        assert len(pairs) > 0.9 * (n - 16) and differ >= 0.9 * len(pairs), (n, name, differ, len(pairs))


@pytest.mark.parametrize("n", NS)
def test_special_frames_are_what_and_where_they_should_be(counts, n):
    nk, nd = counts[n]
    kinds = S.kinds(n)
    assert np.all((nk[kinds == S.FLAT] == 0) & (nd[kinds == S.FLAT] == 0))
    assert np.all((nk[kinds == S.UNDESCRIBED] > 0) & (nd[kinds == S.UNDESCRIBED] == 0))
    assert np.all((nk[kinds == S.DENSE] >= S.dense_min(W, H)) & (nd[kinds == S.DENSE] > 0)) and S.dense_min(W, H) > S.CAP_REDUCED
    assert np.all(nd[kinds == S.ORDINARY] > 0)          # no frame is empty by accident
    for kind in (S.FLAT, S.UNDESCRIBED, S.DENSE):
        at = np.flatnonzero(kinds == kind)
        assert np.any(at < 1024) and np.any(at >= n - 3), (n, kind)
        if n >= 2048:
            assert np.any((at >= 1024) & (at < 2048)), (n, kind)
    for f in (0, 7, 8, 255, 256, 1023, 1024, 2047, 2048):
        if f < n - 3:
            assert kinds[f] == S.ORDINARY, f
    for f in (1024, 2048):
        if f < n:
            assert nd[f] > 0, f
    assert nd[n - 1] > 0


@pytest.mark.parametrize("n", NS)
def test_over_capacity_frames_are_a_few_percent_of_the_batch(counts, n):
    nk = counts[n][0]
    over = int((nk > S.CAP_REDUCED).sum())
    print(n, over)
    assert 0.01 * n <= over <= 0.10 * n, (n, over)
    assert S.CAP_REDUCED >= 16                           # (the engine's smallest keypoint capacity)
    # frames of every kind on both sides of the capacity: ordinary ones above it, and below it
    ordinary = S.kinds(n) == S.ORDINARY
    assert (nk[ordinary] > S.CAP_REDUCED).any() and (nk[ordinary] < S.CAP_REDUCED).sum() > 0.8 * n


def _export_loop(counts, overflow, rows_cap):
    """the export rule frame by frame"""
    n = len(counts)
    flags, offsets = [0] * n, [0] * (n + 1)
    p, cutting = 0, False
    for f in range(n):
        want = 0 if overflow[f] else int(counts[f])
        if not cutting and want > 0 and p + want > rows_cap:
            cutting = True
        offsets[f] = p
        flags[f] = int(overflow[f])
        if want > 0:
            if cutting:
                flags[f] |= S.ROWS_CUT
            else:
                p += want
    offsets[n] = p
    return list(map(int, counts)), flags, offsets


def test_expected_export_against_a_frame_by_frame_loop():
    rng = np.random.default_rng(77)
    seen_cut = seen_fit = seen_zero_behind = 0
    for case in range(200):
        n = int(rng.integers(1, 90))
        c = rng.integers(0, 60, n)
        c[rng.random(n) < 0.25] = 0
        ov = np.where(rng.random(n) < 0.15, rng.choice([1, 2, 4, 6, 8, 16], n), 0)
        want = np.where(ov != 0, 0, c)
        prefix = np.concatenate([[0], np.cumsum(want)])
        caps = {0, int(prefix[-1]), int(prefix[-1]) + 5, 1 << 40}
        for q in rng.integers(0, n + 1, 3):
            caps.update({int(prefix[q]), max(int(prefix[q]) - 1, 0)})
        for cap in sorted(caps):
            got = S.expected_export(c, ov, cap)
            ref = _export_loop(c, ov, cap)
            assert [list(map(int, a)) for a in got] == [list(a) for a in ref], (case, cap)
            cut = (got[1] & S.ROWS_CUT) != 0
            assert got[2][n] <= cap                       # never more rows stored than the destination holds
            if cut.any():
                first = int(np.argmax(cut))
                seen_cut += 1
                seen_zero_behind += int(np.any(want[first:] == 0))
                assert np.all(got[2][first:] == got[2][n]) and np.all(cut[first:] == (want[first:] > 0))
            else:
                seen_fit += 1
                assert got[2][n] == prefix[-1]
    assert seen_cut > 200 and seen_fit > 200 and seen_zero_behind > 100


@pytest.mark.parametrize("nd", [3, 4, 7, 8])
def test_slot_filling_puts_different_frames_8_slots_apart(nd):
    for n in (65, 128, 255, 512):
        s = [S.slot_frame(f, nd) for f in range(n)]
        assert set(s) == set(range(nd)) and set(s[:8]) == set(range(min(nd, 8)))
        assert all(s[f] != s[f + 8] for f in range(n - 8)) and all(s[f] != s[f ^ 8] for f in range(n) if (f ^ 8) < n)

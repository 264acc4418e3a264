"""GPU tests of brisk_hip_verify_pair_matches_device: a batch's packed pair matches checked against a homography estimated per pair.
The expectation is always the NumPy restatement of the rule (test_abi_verify.restated_verify) on the host copies of the inputs;
every array - models, counts, flags, offsets, the kept records - is compared as bytes, and outputs are pre-filled with the matcher
tests' sentinel so that a write outside them shows.  The shapes sit at the seams of the kernels: the LDS chunk of 1 024 records, the
scatter chunk of 256, the wave of 64 and the pass of 256 hypotheses, the 1 024 threads of the offsets workgroup."""
import ctypes as C

import numpy as np
import pytest

from gpu_prefill import settled
from test_abi_tracks import SENT32, restated_link, restated_list
from test_abi_verify import PAIR_BAD, PAIR_NO_MODEL, ROWS_CUT, restated_pair, restated_verify
from test_gpu_match_pairs import SENTINEL, batch_frames

pytestmark = pytest.mark.gpu

CAP = 256          # rows_cap
PAD = 8            # records behind out_cap that must keep the sentinel


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


# ---- scenes made by hand ------------------------------------------------------------------------------------------------------

def homography(rng):
    """a mild projective map of a 640 x 480 frame"""
    a = float(rng.uniform(-0.1, 0.1))
    return np.array([[np.cos(a) * rng.uniform(0.9, 1.1), -np.sin(a), rng.uniform(-30, 30)],
                     [np.sin(a), np.cos(a) * rng.uniform(0.9, 1.1), rng.uniform(-30, 30)],
                     [rng.uniform(-1e-4, 1e-4), rng.uniform(-1e-4, 1e-4), 1.0]])


class Scene:
    """`frames` frames that see the same base points, each through a homography of its own: row r of frame a and row r of frame b are
    an exact (float-rounded) pair of H_b H_a^-1, rows r and r' != r an outlier.  rows[f]: the frame's TRUE count (a count beyond
    rows_cap: rows that do not exist for the call); the keypoint arrays hold max(rows) records per frame, x and y among NaN-filled
    other fields.  stride: the counts lie at `stride` ints with garbage between them."""

    def __init__(self, B, seed, rows, stride=3, nan_rows=(), model=homography, alloc=None):
        import torch
        rng = np.random.default_rng(seed)
        self.B, self.rng, self.rows, self.nframes, self.stride = B, rng, [int(r) for r in rows], len(rows), stride
        self.alloc = alloc or max(max(self.rows), 1)
        base = np.stack([rng.uniform(20, 620, self.alloc), rng.uniform(20, 460, self.alloc)], axis=1)
        self.kps = np.zeros((self.nframes, self.alloc), B.KEYPOINT)
        for name in ("size", "angle", "response"):
            self.kps[name] = np.nan
        self.kps["octave"], self.kps["class_id"] = 0x7FFFFFFF, -1
        for f in range(self.nframes):
            H = model(rng)
            w = H[2, 0] * base[:, 0] + H[2, 1] * base[:, 1] + H[2, 2]
            self.kps["x"][f] = ((H[0, 0] * base[:, 0] + H[0, 1] * base[:, 1] + H[0, 2]) / w).astype(np.float32)
            self.kps["y"][f] = ((H[1, 0] * base[:, 0] + H[1, 1] * base[:, 1] + H[1, 2]) / w).astype(np.float32)
        for f, r, field, v in nan_rows:
            self.kps[field][f, r] = v
        cnt = np.full(self.nframes * stride, 77777, np.int32)
        cnt[::stride] = self.rows
        self.d_counts = torch.from_numpy(cnt).cuda()
        self.desc_set = B.DescSet(None, self.d_counts.data_ptr(), stride, 0, 0, self.nframes)
        self.upload()

    def upload(self):
        """the keypoints (as they are now) to the device"""
        import torch
        self.d_kps = torch.from_numpy(self.kps.view(np.int32).reshape(self.nframes, self.alloc, 7).copy()).cuda()
        self.kp_set = self.B.KpSet(self.d_kps.data_ptr(), self.alloc * 28)
        self.xy = [np.stack([self.kps["x"][f], self.kps["y"][f]], axis=1) for f in range(self.nframes)]

    def lim(self, f):
        return min(max(self.rows[f], 0), CAP)

    def records(self, a, b, m, inliers=0.7, odd=0.0):
        """m records of pair (a, b), sorted by query row as the selection leaves them; odd: the share of records that name no row
        (index -1, index = lim, a row beyond rows_cap, +-2^31)"""
        rng, B = self.rng, self.B
        la, lb = max(self.lim(a), 1), max(self.lim(b), 1)
        common = max(min(la, lb), 1)
        q = np.sort(rng.integers(0, common, m))
        t = np.where(rng.random(m) < inliers, q, rng.integers(0, lb, m))
        rec = np.zeros(m, B.DMATCH)
        rec["queryIdx"], rec["trainIdx"], rec["imgIdx"], rec["distance"] = q, t, b, rng.integers(0, 90, m).astype(np.float32)
        for j in np.flatnonzero(rng.random(m) < odd):
            field = "queryIdx" if rng.integers(0, 2) else "trainIdx"
            lim = self.lim(a) if field == "queryIdx" else self.lim(b)
            rec[field][j] = int(rng.choice([-1, lim, lim + 1, CAP, self.alloc - 1, -2 ** 31, 2 ** 31 - 1]))
        return rec


class Lists:
    """the packed lists of a call on the device: offsets [npairs + 1], records [in_cap] (sentinel-filled behind the total)"""

    def __init__(self, B, per_pair, slack=5):
        import torch
        self.per_pair = per_pair
        self.offsets = np.zeros(len(per_pair) + 1, np.int64)
        self.offsets[1:] = np.cumsum([len(r) for r in per_pair])
        total = int(self.offsets[-1])
        self.in_cap = total + slack
        self.matches = np.concatenate(list(per_pair) + [np.zeros(0, B.DMATCH)])
        full = np.full((self.in_cap, 4), SENTINEL, np.int32)
        full[:total] = self.matches.view(np.int32).reshape(-1, 4)
        self.d_offsets = torch.from_numpy(self.offsets).cuda()
        self.d_matches = torch.from_numpy(full).cuda()


def sentinel_outputs(npairs, out_cap):
    import torch
    return settled(torch.full((max(out_cap, 0) + PAD, 4), SENTINEL, dtype=torch.int32, device="cuda"),
                   torch.full((npairs,), SENTINEL, dtype=torch.int32, device="cuda"), torch.full((npairs,), SENTINEL, dtype=torch.int32, device="cuda"),
                   torch.full((npairs + 2,), int(np.int64(0x5A5A5A5A5A5A5A5A)), dtype=torch.int64, device="cuda"),
                   torch.full((npairs + 1, 24), SENTINEL, dtype=torch.int32, device="cuda"))


def raw_verify(B, ctx, qs, ts, spec, lists, verify, out_cap, out=None, stream=None, in_cap=None):
    """the C entry point on pre-filled outputs (matches, counts, flags, offsets, models)"""
    out = out or sentinel_outputs(spec.npairs, out_cap)
    v = B.PairVerify(*verify)
    rc = ctx._L.brisk_hip_verify_pair_matches_device(ctx._h, C.byref(qs.desc_set), C.byref(ts.desc_set), C.byref(qs.kp_set), C.byref(ts.kp_set),
                                                     C.byref(spec), CAP, lists.d_offsets.data_ptr(), lists.d_matches.data_ptr(),
                                                     lists.in_cap if in_cap is None else in_cap, C.byref(v), out_cap, out[4].data_ptr(),
                                                     out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), out[0].data_ptr(),
                                                     C.c_void_p(stream) if stream else None)
    return rc, out


def same(B, got, want, npairs, out_cap):
    """got: the five device tensors; want: what restated_verify returned.  Everything as bytes, the sentinel behind every array."""
    import torch
    torch.cuda.synchronize()
    gm, gc, gf, go, gmod = (t.cpu().numpy() for t in got)
    models, counts, flags, offs, stored = want
    assert gc.tobytes() == counts.tobytes(), (gc.tolist(), counts.tolist())
    assert gf.tobytes() == flags.tobytes(), (gf.tolist(), flags.tolist())
    assert go[:npairs + 1].tobytes() == offs.tobytes(), (go.tolist(), offs.tolist())
    assert go[npairs + 1] == np.int64(0x5A5A5A5A5A5A5A5A)
    wm = np.full((max(out_cap, 0) + PAD, 4), SENTINEL, np.int32)
    wm[:len(stored)] = np.ascontiguousarray(stored).view(np.int32).reshape(-1, 4)
    assert len(stored) == offs[-1] <= max(out_cap, 0)
    if gm.tobytes() != wm.tobytes():
        bad = np.flatnonzero((gm != wm).any(axis=1))
        raise AssertionError(("matches", len(bad), bad[:5].tolist(), gm[bad[0]].tolist(), wm[bad[0]].tolist()))
    gmod_rec = gmod[:npairs].reshape(-1).view(B.PAIR_MODEL)
    for p in range(npairs):
        assert gmod_rec[p].tobytes() == models[p].tobytes(), (p, gmod_rec[p], models[p])
    assert (gmod[npairs] == SENTINEL).all()


def expect(qs, ts, frames, lists, verify, out_cap, in_cap=None):
    return restated_verify(frames, qs.rows, ts.rows, CAP, qs.xy, ts.xy, lists.offsets, lists.matches, verify,
                           lists.in_cap if in_cap is None else in_cap, out_cap)


def chain_frames(n):
    return [(p + 1, p) for p in range(n)]


SEAMS = [0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 2049]


@pytest.fixture(scope="module")
def seam_scene(B):
    sc = Scene(B, 11, [300] * (len(SEAMS) + 1))                      # 300 rows a frame, 256 exist
    return sc, Lists(B, [sc.records(p + 1, p, m) for p, m in enumerate(SEAMS)])


def test_record_counts_at_the_chunk_seams(B, ctx, seam_scene):
    sc, lists = seam_scene
    n = len(SEAMS)
    spec = B.PairSpec(n, 1, 1, 0, 1, None)
    verify = (2.0, 64, 8, 0, 5)
    out_cap = int(lists.offsets[-1])
    rc, out = raw_verify(B, ctx, sc, sc, spec, lists, verify, out_cap)
    assert rc == 0
    want = expect(sc, sc, chain_frames(n), lists, verify, out_cap)
    same(B, out, want, n, out_cap)
    models = want[0]
    assert models["records"].tolist() == SEAMS
    big = models["records"] >= 255
    assert (models["flags"][big] == 0).all() and (models["inliers"][big] > 0.5 * models["records"][big]).all()   # models are found ...
    assert (want[1][big] < models["usable"][big]).all() and (models["flags"][:3] == PAIR_NO_MODEL).all()         # ... and records dropped


@pytest.mark.parametrize("hyps", [1, 63, 64, 65, 256, 257, 4096])
def test_hypothesis_counts_at_the_wave_and_pass_seams(B, ctx, hyps):
    ms = [0, 3, 4, 5, 40, 257, 1025]                                # 1 025 records: a pair that restages its chunks in every pass
    sc = Scene(B, 20 + hyps, [200] * (len(ms) + 1))
    lists = Lists(B, [sc.records(p + 1, p, m, inliers=0.5, odd=0.05) for p, m in enumerate(ms)])
    spec = B.PairSpec(len(ms), 1, 1, 0, 1, None)
    verify = (1.5, hyps, 6, 1, 77)
    out_cap = int(lists.offsets[-1])
    rc, out = raw_verify(B, ctx, sc, sc, spec, lists, verify, out_cap)
    assert rc == 0
    want = expect(sc, sc, chain_frames(len(ms)), lists, verify, out_cap)
    same(B, out, want, len(ms), out_cap)
    assert (want[0]["valid"][2:] <= hyps).all() and want[0]["valid"][4:].min() > 0


def test_winner_ties_go_to_the_smallest_hypothesis(B, ctx):
    """integer points under an integer translation: every record is an exact inlier of every valid hypothesis"""
    def shift(rng):
        return np.array([[1.0, 0, float(rng.integers(-20, 20))], [0, 1.0, float(rng.integers(-20, 20))], [0, 0, 1.0]])
    sc = Scene(B, 31, [64, 64, 64], model=shift)
    for f in range(3):                                               # integer base points: the translation is exact in fp32
        sc.kps["x"][f], sc.kps["y"][f] = np.round(sc.kps["x"][f]), np.round(sc.kps["y"][f])
    sc.upload()
    lists = Lists(B, [sc.records(p + 1, p, 50, inliers=1.0) for p in range(2)])
    spec = B.PairSpec(2, 1, 1, 0, 1, None)
    verify = (0.5, 300, 4, 0, 9)
    rc, out = raw_verify(B, ctx, sc, sc, spec, lists, verify, 100)
    assert rc == 0
    want = expect(sc, sc, chain_frames(2), lists, verify, 100)
    same(B, out, want, 2, 100)
    for p in range(2):
        r = restated_pair(9, p, 300, 4, 0, 0.5, 64, 64, sc.xy[p + 1], sc.xy[p], lists.per_pair[p])
        full = np.flatnonzero(r["valid"] & (r["count"] == 50))
        assert len(full) > 100 and want[0]["hypothesis"][p] == full[0] == np.flatnonzero(r["valid"])[0]    # many tie, the first wins
        assert want[0]["inliers"][p] == 50 and want[1][p] == 50


@pytest.mark.parametrize("keep", [0, 1])
def test_no_valid_hypothesis(B, ctx, keep):
    """all keypoints of the query frame on one line: no sample gives a model"""
    sc = Scene(B, 41, [80, 80, 80])
    sc.kps["x"][1], sc.kps["y"][1] = np.round(sc.kps["x"][1] / 2) * 2, np.round(sc.kps["x"][1] / 2) + 7      # exactly on y = x / 2 + 7
    sc.upload()
    lists = Lists(B, [sc.records(1, 0, 60, odd=0.1), sc.records(2, 1, 60)])
    spec = B.PairSpec(2, 1, 1, 0, 1, None)
    verify = (2.0, 128, 4, keep, 3)
    rc, out = raw_verify(B, ctx, sc, sc, spec, lists, verify, 120)
    assert rc == 0
    want = expect(sc, sc, chain_frames(2), lists, verify, 120)
    same(B, out, want, 2, 120)
    mod = want[0]
    assert mod["hypothesis"].tolist() == [-1, -1] and mod["valid"].tolist() == [0, 0] and (mod["h"] == 0).all()
    assert mod["flags"].tolist() == [PAIR_NO_MODEL] * 2
    assert want[1].tolist() == ([int(mod["usable"][0]), 60] if keep else [0, 0]) and 40 < mod["usable"][0] < 60


@pytest.mark.parametrize("keep", [0, 1])
def test_unusable_records(B, ctx, keep):
    """indices of -1, = lim, beyond rows_cap, NaN / inf keypoint coordinates; pairs with and without a model in one call"""
    nan_rows = [(1, 3, "x", np.nan), (1, 9, "y", np.inf), (0, 5, "y", np.nan), (2, 0, "x", -np.inf), (2, 17, "x", np.nan)]
    sc = Scene(B, 51, [300, 120, 256, 40, 257], nan_rows=nan_rows)  # frame 0 and 4 beyond rows_cap, frame 3 short
    per = [sc.records(1, 0, 200, odd=0.15), sc.records(2, 1, 300, odd=0.15), sc.records(3, 2, 90, inliers=0.0, odd=0.15),
           sc.records(4, 3, 70, odd=0.3)]
    for rec in per[:2]:                                             # records that name the rows with NaN coordinates
        rec["queryIdx"][:4], rec["trainIdx"][:4] = [3, 3, 9, 9], [3, 5, 9, 5]
    lists = Lists(B, per)
    spec = B.PairSpec(4, 1, 1, 0, 1, None)
    verify = (1.0, 256, 10, keep, 123)
    out_cap = int(lists.offsets[-1])
    rc, out = raw_verify(B, ctx, sc, sc, spec, lists, verify, out_cap)
    assert rc == 0
    want = expect(sc, sc, chain_frames(4), lists, verify, out_cap)
    same(B, out, want, 4, out_cap)
    mod = want[0]
    assert (mod["usable"] < mod["records"]).all() and (mod["usable"] > 0).all()
    assert mod["flags"][0] == 0 and mod["flags"][1] == 0 and mod["flags"][2] == PAIR_NO_MODEL     # pure outliers: no model
    assert want[1][2] == (mod["usable"][2] if keep else 0)


def test_pair_forms(B, ctx):
    import torch
    sc = Scene(B, 61, [90, 100, 110, 120, 130, 140])
    verify = (1.0, 64, 6, 0, 8)
    # a list on the device with entries outside the sets between good pairs
    frames = [(1, 0), (6, 0), (3, 5), (2, -1), (4, 4), (-2147483648, 2), (0, 6), (5, 1)]
    per = [sc.records(max(min(a, 5), 0), max(min(b, 5), 0), 50) for a, b in frames]
    lists = Lists(B, per)
    d_pairs = torch.from_numpy(np.array(frames, np.int32)).cuda()
    spec = B.PairSpec(len(frames), 9, 9, 9, 9, d_pairs.data_ptr())
    out_cap = int(lists.offsets[-1])
    rc, out = raw_verify(B, ctx, sc, sc, spec, lists, verify, out_cap)
    assert rc == 0
    want = expect(sc, sc, frames, lists, verify, out_cap)
    same(B, out, want, len(frames), out_cap)
    assert [int(f) for f in want[2]] == [0, PAIR_BAD | PAIR_NO_MODEL, 0, PAIR_BAD | PAIR_NO_MODEL, 0, PAIR_BAD | PAIR_NO_MODEL,
                                        PAIR_BAD | PAIR_NO_MODEL, 0]
    itself = int((per[4]["queryIdx"] == per[4]["trainIdx"]).sum())  # a frame against itself: the identity, exact for every such record
    assert want[0]["flags"][4] == 0 and want[1][4] >= itself > 25
    # everything against one frame
    frames = [(p + 1, 0) for p in range(5)]
    lists = Lists(B, [sc.records(a, b, 45) for a, b in frames])
    rc, out = raw_verify(B, ctx, sc, sc, B.PairSpec(5, 1, 1, 0, 0, None), lists, verify, 225)
    assert rc == 0
    same(B, out, expect(sc, sc, frames, lists, verify, 225), 5, 225)
    # interleaved stereo: left frames 0, 2, 4 against right frames 1, 3, 5 - and two sets side by side
    frames = [(0, 1), (2, 3), (4, 5)]
    lists = Lists(B, [sc.records(a, b, 45) for a, b in frames])
    rc, out = raw_verify(B, ctx, sc, sc, B.PairSpec(3, 0, 2, 1, 2, None), lists, verify, 135)
    assert rc == 0
    same(B, out, expect(sc, sc, frames, lists, verify, 135), 3, 135)
    # two sets side by side: the other set sees the same points through the same homographies (the seed) with fewer rows a frame,
    # so some records name train rows that do not exist there
    other = Scene(B, 61, [70, 80, 85], stride=1, alloc=sc.alloc)
    frames = [(3, 0), (4, 1), (5, 2)]
    lists = Lists(B, [sc.records(a, b, 45) for a, b in frames])
    rc, out = raw_verify(B, ctx, sc, other, B.PairSpec(3, 3, 1, 0, 1, None), lists, verify, 135)
    assert rc == 0
    want = expect(sc, other, frames, lists, verify, 135)
    same(B, out, want, 3, 135)
    assert (want[0]["usable"] < 45).all() and (want[0]["flags"] == 0).all()


def test_capacity(B, ctx):
    """out_cap equal to the total, one short (the cut falls in the last pair that keeps anything, an empty pair in front of it and
    one behind), and 0"""
    sc = Scene(B, 71, [100] * 7)
    per = [sc.records(1, 0, 60), sc.records(2, 1, 0), sc.records(3, 2, 70), sc.records(4, 3, 30, inliers=0.0), sc.records(5, 4, 80),
           sc.records(6, 5, 0)]
    lists = Lists(B, per)
    spec = B.PairSpec(6, 1, 1, 0, 1, None)
    verify = (1.0, 128, 10, 0, 4)
    free = expect(sc, sc, chain_frames(6), lists, verify, 10 ** 6)
    total = int(free[3][-1])
    assert free[1][3] == 0 and free[1][4] > 20 and free[1][5] == 0 and total == free[1].sum()
    for out_cap in (total, total - 1, 0):
        rc, out = raw_verify(B, ctx, sc, sc, spec, lists, verify, out_cap)
        assert rc == 0
        want = expect(sc, sc, chain_frames(6), lists, verify, out_cap)
        same(B, out, want, 6, out_cap)
        cut = [bool(f & ROWS_CUT) for f in want[2]]
        assert cut == {total: [False] * 6, total - 1: [False] * 4 + [True] * 2, 0: [True] * 6}[out_cap]
        assert want[1].tolist() == free[1].tolist()                  # the true counts are still reported
    # d_out_matches may be NULL with out_cap 0
    out = sentinel_outputs(6, 0)
    v = B.PairVerify(*verify)
    rc = ctx._L.brisk_hip_verify_pair_matches_device(ctx._h, C.byref(sc.desc_set), C.byref(sc.desc_set), C.byref(sc.kp_set), C.byref(sc.kp_set),
                                                     C.byref(spec), CAP, lists.d_offsets.data_ptr(), lists.d_matches.data_ptr(), lists.in_cap,
                                                     C.byref(v), 0, out[4].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                                     out[3].data_ptr(), None, None)
    assert rc == 0
    same(B, out, expect(sc, sc, chain_frames(6), lists, verify, 0), 6, 0)


def test_more_pairs_than_the_offsets_workgroup_has_threads(B, ctx):
    """1 500 pairs of 0 ... 9 records: the chunked sums of k_verify_offsets (two pairs a thread, the last threads idle), with a cut"""
    import torch
    rng = np.random.default_rng(81)
    sc = Scene(B, 81, [60] * 12)
    n = 1500
    frames = [(int(a), int(b)) for a, b in rng.integers(0, 12, (n, 2))]
    lists = Lists(B, [sc.records(a, b, int(rng.integers(0, 10)), inliers=0.9) for a, b in frames])
    d_pairs = torch.from_numpy(np.array(frames, np.int32)).cuda()
    spec = B.PairSpec(n, 0, 0, 0, 0, d_pairs.data_ptr())
    verify = (1.0, 16, 4, 1, 2)
    free = expect(sc, sc, frames, lists, verify, 10 ** 7)
    total = int(free[3][-1])
    assert total > 3000
    for out_cap in (total, total * 2 // 3):
        rc, out = raw_verify(B, ctx, sc, sc, spec, lists, verify, out_cap)
        assert rc == 0
        want = free if out_cap == total else expect(sc, sc, frames, lists, verify, out_cap)
        same(B, out, want, n, out_cap)
    assert 1024 - 400 < int(np.flatnonzero(want[2] & ROWS_CUT)[0]) < 1024 + 400


def test_a_second_call_on_the_stream_reuses_the_scratch(B, ctx, seam_scene):
    """two calls back to back on one stream, the second smaller than the first (it runs in the scratch the first one grew), no
    synchronisation in between; then the first one again"""
    import torch
    sc, big = seam_scene
    small_sc = Scene(B, 91, [50, 60, 70])
    small = Lists(B, [small_sc.records(1, 0, 33), small_sc.records(2, 1, 44)])
    s = torch.cuda.Stream()
    n = len(SEAMS)
    v1, v2 = (2.0, 64, 8, 0, 5), (1.0, 32, 5, 1, 6)
    cap1, cap2 = int(big.offsets[-1]), 77
    rc1, out1 = raw_verify(B, ctx, sc, sc, B.PairSpec(n, 1, 1, 0, 1, None), big, v1, cap1, stream=s.cuda_stream)
    rc2, out2 = raw_verify(B, ctx, small_sc, small_sc, B.PairSpec(2, 1, 1, 0, 1, None), small, v2, cap2, stream=s.cuda_stream)
    rc3, out3 = raw_verify(B, ctx, sc, sc, B.PairSpec(n, 1, 1, 0, 1, None), big, v1, cap1, stream=s.cuda_stream)
    assert rc1 == 0 and rc2 == 0 and rc3 == 0
    want1 = expect(sc, sc, chain_frames(n), big, v1, cap1)
    same(B, out1, want1, n, cap1)
    same(B, out2, expect(small_sc, small_sc, chain_frames(2), small, v2, cap2), 2, cap2)
    same(B, out3, want1, n, cap1)


def test_the_pipeline(B, ctx, golden_ast):
    """a small batch through match -> select -> verify -> link -> list on one stream; the linker's output is the restated link of
    the restated verified lists"""
    import torch
    frames = batch_frames(golden_ast)[:5]
    n, h, w = frames.shape
    d = torch.from_numpy(frames).cuda()
    ext = B.BriskDescriptorExtractor(context=ctx)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    ctx.detect_describe_batch(ext, d.data_ptr(), n, w, h, w * h, w, 70, 2, s.cuda_stream)
    st, dim = ctx.batch_desc_set()
    spec = B.PairSpec(n - 1, 1, 1, 0, 1, None)
    triple = ctx.match_knn_pairs(st, st, spec, 2, stream=s.cuda_stream)
    rows_cap = int(triple[1].shape[1])
    sel = ctx.select_pair_matches(triple, 2, B.MatchSelect(90.0, 0.9, 1), stream=s.cuda_stream)
    verify = (3.0, 256, 12, 0, 2024)
    ver = ctx.verify_pair_matches(st, st, spec, rows_cap, sel[3], sel[0], B.PairVerify(*verify), stream=s.cuda_stream)
    linked = ctx.link_tracks((st, 0, 1), n, rows_cap, ver[3], ver[0], stream=s.cuda_stream)
    listed = ctx.list_tracks((st, 0, 1), n, rows_cap, *linked[:3], 2, stream=s.cuda_stream)
    torch.cuda.synchronize()
    assert ctx.batch_status(n) == 0
    kps = [ctx.batch_download(f, True, strings=dim)[0] for f in range(n)]
    node_rows = [len(k) for k in kps]
    xy = [np.stack([k["x"], k["y"]], axis=1).astype(np.float32).reshape(-1, 2) for k in kps]
    so = sel[3].cpu().numpy()
    sm = sel[0].cpu().numpy().view(B.DMATCH).reshape(-1)
    in_cap = len(sm)
    want = restated_verify(chain_frames(n - 1), node_rows, node_rows, rows_cap, xy, xy, so, sm[:int(so[-1])], verify, in_cap, in_cap)
    models, counts, flags, offs, stored = want
    assert ver[1].cpu().numpy().tobytes() == counts.tobytes() and ver[2].cpu().numpy().tobytes() == flags.tobytes()
    assert ver[3].cpu().numpy().tobytes() == offs.tobytes()
    assert ver[0].cpu().numpy()[:len(stored)].tobytes() == stored.tobytes()
    assert ver[4].cpu().numpy().tobytes() == models.tobytes()
    # pair 0 is (img1, img2), the reference's matching test: a model is found and it drops matches the descriptor test let through
    assert models["flags"][0] == 0 and 50 < counts[0] < models["usable"][0]
    assert models["flags"][2] == PAIR_NO_MODEL and models["records"][2] == 0      # the blank frame
    wl = restated_link(node_rows, rows_cap, offs, stored)
    gl = tuple(t.cpu().numpy() for t in linked)
    wrote = wl[0] != SENT32
    for name, g, w_ in zip(("prev", "track", "age"), gl, wl):
        assert np.array_equal(g[wrote], w_[wrote]), name
    assert gl[3].tolist() == wl[3].tolist() and wl[3][2] > 100
    wlist = restated_list(node_rows, rows_cap, *wl[:3], 2)
    glist = tuple(t.cpu().numpy() for t in listed)
    assert glist[4].tolist() == wlist[4].tolist()
    pieces, obs = int(wlist[4][0]), int(wlist[4][1])
    assert glist[0][:pieces].tobytes() == wlist[0].tobytes() and glist[3][:obs].tobytes() == wlist[3].tobytes()
    ext.close()


def test_arguments(B, ctx):
    """BRISK_HIP_ERR_ARG before anything is launched: the sentinel stays in every output"""
    import torch
    sc = Scene(B, 101, [50, 60, 70])
    lists = Lists(B, [sc.records(1, 0, 30), sc.records(2, 1, 30)])
    out = sentinel_outputs(2, 60)
    L, h = ctx._L, ctx._h

    def call(**kw):
        a = dict(ctx=h, query=sc.desc_set, train=sc.desc_set, query_kps=sc.kp_set, train_kps=sc.kp_set, pairs=B.PairSpec(2, 1, 1, 0, 1, None),
                 rows_cap=CAP, offsets=lists.d_offsets.data_ptr(), matches=lists.d_matches.data_ptr(), in_cap=lists.in_cap,
                 verify=B.PairVerify(1.0, 64, 6, 0, 1), out_cap=60, models=out[4].data_ptr(), counts=out[1].data_ptr(), flags=out[2].data_ptr(),
                 out_offsets=out[3].data_ptr(), out_matches=out[0].data_ptr())
        a.update(kw)
        ref = lambda v: None if v is None else C.byref(v)
        return L.brisk_hip_verify_pair_matches_device(a["ctx"], ref(a["query"]), ref(a["train"]), ref(a["query_kps"]), ref(a["train_kps"]),
                                                      ref(a["pairs"]), a["rows_cap"], a["offsets"], a["matches"], a["in_cap"], ref(a["verify"]),
                                                      a["out_cap"], a["models"], a["counts"], a["flags"], a["out_offsets"], a["out_matches"], None)

    def desc(**kw):
        f = dict(d_desc=None, d_counts=sc.d_counts.data_ptr(), count_stride=sc.stride, frame_pitch=0, row_pitch=0, frames=3)
        f.update(kw)
        return B.DescSet(f["d_desc"], f["d_counts"], f["count_stride"], f["frame_pitch"], f["row_pitch"], f["frames"])

    kp = sc.d_kps.data_ptr()
    bad = [dict(ctx=None), dict(query=None), dict(train=None), dict(query_kps=None), dict(train_kps=None), dict(pairs=None), dict(verify=None),
           dict(rows_cap=0), dict(in_cap=-1), dict(out_cap=-1), dict(pairs=B.PairSpec(-1, 1, 1, 0, 1, None)),
           dict(offsets=None), dict(matches=None), dict(models=None), dict(counts=None), dict(flags=None), dict(out_offsets=None),
           dict(out_matches=None),
           dict(offsets=lists.d_offsets.data_ptr() + 4), dict(matches=lists.d_matches.data_ptr() + 8), dict(models=out[4].data_ptr() + 4),
           dict(counts=out[1].data_ptr() + 2), dict(flags=out[2].data_ptr() + 1), dict(out_offsets=out[3].data_ptr() + 4),
           dict(out_matches=out[0].data_ptr() + 8),
           dict(verify=B.PairVerify(1.0, 0, 6, 0, 1)), dict(verify=B.PairVerify(1.0, 4097, 6, 0, 1)), dict(verify=B.PairVerify(1.0, -5, 6, 0, 1)),
           dict(verify=B.PairVerify(1.0, 64, 3, 0, 1)), dict(verify=B.PairVerify(1.0, 64, -1, 0, 1)),
           # an arithmetic-form frame outside its set, at either end, on either side
           dict(pairs=B.PairSpec(2, 2, 1, 0, 1, None)), dict(pairs=B.PairSpec(2, 1, 1, -1, 1, None)), dict(pairs=B.PairSpec(2, 1, 1, 2, 1, None)),
           dict(pairs=B.PairSpec(2, 0, -1, 0, 1, None)), dict(pairs=B.PairSpec(2, 1, 1, 0, 1, lists.d_offsets.data_ptr() + 2)),
           dict(query=desc(d_counts=None)), dict(train=desc(frames=0)), dict(query=desc(count_stride=0)),
           dict(train=desc(d_counts=sc.d_counts.data_ptr() + 2)),
           # the keypoint-set errors of the gated matchers
           dict(query_kps=B.KpSet(None, 28)), dict(train_kps=B.KpSet(kp + 2, 28)), dict(query_kps=B.KpSet(kp, -28)),
           dict(train_kps=B.KpSet(kp, 30))]
    for kw in bad:
        assert call(**kw) == 1, kw
    torch.cuda.synchronize()
    assert all((t.cpu().numpy().view(np.int32) == SENTINEL).all() for t in out)        # nothing was launched
    # npairs == 0: OK, d_out_offsets[0] = 0 and nothing else; NULL arrays are then allowed
    assert call(pairs=B.PairSpec(0, 1, 1, 0, 1, None), out_offsets=None, models=None, counts=None, flags=None, offsets=None) == 0
    assert call(pairs=B.PairSpec(0, 7, 7, 7, 7, None)) == 0
    torch.cuda.synchronize()
    o = out[3].cpu().numpy()
    assert o[0] == 0 and (o[1:] == np.int64(0x5A5A5A5A5A5A5A5A)).all()
    assert all((t.cpu().numpy().view(np.int32) == SENTINEL).all() for t in (out[0], out[1], out[2], out[4]))
    # offsets that are no range inside [0, in_cap]: the pair is flagged bad on the device, nothing of it is read
    verify = (1.0, 64, 6, 0, 1)
    rc, got = raw_verify(B, ctx, sc, sc, B.PairSpec(2, 1, 1, 0, 1, None), lists, verify, 60, in_cap=45)
    assert rc == 0
    want = expect(sc, sc, chain_frames(2), lists, verify, 60, in_cap=45)
    same(B, got, want, 2, 60)
    assert want[2].tolist() == [0, PAIR_BAD | PAIR_NO_MODEL] and want[1][0] > 6 and want[1][1] == 0
    assert call() == 0
    same(B, out, expect(sc, sc, chain_frames(2), lists, verify, 60), 2, 60)

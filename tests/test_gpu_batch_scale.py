"""GPU tests (run with -m gpu) of the batch path at 257 ... 2 049 frames per launch with frames that ALL differ
(batch_scale_lib.py; its conditions are pinned by test_batch_scale_fixture.py): the regimes in which the code changes form -
k_export_offsets with 2 and 3 frames per thread (above 1 024 frames), k_describe's queues at their full 256 entries (2 048
frames) and with nine groups (2 049), slot byte offsets beyond 2^31 and 2^32 - and the cross-frame bookkeeping modulo 8, which
batches filled from 8, 4 or 3 distinct frames cannot see.  Everything is bit-exact against the CPU oracle; the exit to host
memory against batch_scale_lib.expected_export, a restatement of the contract in include/brisk_hip.h."""
import numpy as np
import pytest

import batch_scale_lib as S
from test_gpu_parity import same_kps, explain  # noqa: F401

pytestmark = pytest.mark.gpu

W, H = 128, 96
CAND = 4096      # max_candidates of every context here (these frames have a few hundred candidates)
ERR_CAPACITY = 4


@pytest.fixture(scope="module")
def B():
    import ethzasl_brisk_amd as B
    from ethzasl_brisk_amd import build
    build.build()
    B.load_library()
    return B


def _launch(B, ctx, ext, d, n, w, h):
    import torch
    ctx.detect_describe_batch(ext, d.data_ptr(), n, w, h, w * h, w, S.THR, S.OCT, torch.cuda.current_stream().cuda_stream)
    assert ctx.profile_frames_per_launch() == n          # one launch over all frames


def _filled(B, n, rows, stride, pinned):
    """a destination with slack in both capacities, every byte 0xEE"""
    res = B.HostResults(n + 3, rows + 17, stride, pinned=pinned)
    for a in (res.counts, res.flags, res.offsets, res.kps) + ((res.desc,) if stride else ()):
        a.view(np.uint8)[...] = 0xEE
    return res


def _rows_of(want, which):
    """all rows the oracle has, frame after frame: (keypoints, descriptors or None)"""
    k = np.concatenate([x[which] for x in want])
    return k, (np.concatenate([x[2] for x in want]) if which else None)


def _compare_rows(res, want, which, stored, tag):
    """counts, flags, offsets of `res` are checked by the caller; the rows of the frames in `stored` (a bool per frame)
    against the oracle, and the rows behind offsets[n] untouched"""
    n = len(want)
    off = res.offsets[:n + 1].astype(np.int64)
    idx = np.flatnonzero(stored)
    wk = np.concatenate([want[f][which] for f in idx]) if len(idx) else np.zeros(0, S.O.KP)
    total = int(off[n])
    assert total == len(wk), (tag, total, len(wk))
    got_k = res.kps[:total]
    if not same_kps(got_k, wk):                          # which frame, which field
        for f in idx:
            k = res.kps[off[f]:off[f + 1]]
            assert same_kps(k, want[f][which]), (tag, int(f), explain(k, want[f][which]))
        raise AssertionError((tag, "rows differ although every frame agrees"))
    assert np.all(res.kps[total:].view(np.uint8) == 0xEE), (tag, "keypoint rows behind offsets[n] were written")
    if which and res.desc is not None:
        wd = np.concatenate([want[f][2] for f in idx]) if len(idx) else np.zeros((0, 48), np.uint8)
        if not np.array_equal(res.desc[:total, :48], wd):
            for f in idx:
                assert np.array_equal(res.desc[off[f]:off[f + 1], :48], want[f][2]), (tag, int(f), "descriptors")
        assert np.all(res.desc[total:] == 0xEE), (tag, "descriptor rows behind offsets[n] were written")


def _compare_all(B, ctx, want, pinned, tag, per_frame=()):
    """both exits of the last batch (detected keypoints; described keypoints + descriptors) against the oracle: counts, flags,
    all offsets, every row; then the per-frame download of the frames in per_frame"""
    import torch
    n = len(want)
    stream = torch.cuda.current_stream().cuda_stream
    for which in (0, 1):
        cnt = np.array([len(x[which]) for x in want])
        res = _filled(B, n, int(cnt.sum()), 48 if which else 0, pinned)
        assert ctx.batch_download_wait(ctx.batch_download_all(res, described=bool(which), stream=stream)) == 0, (tag, which)
        c, fl, off = S.expected_export(cnt, np.zeros(n, int), res.rows)
        assert np.array_equal(res.counts[:n], c), (tag, which, np.flatnonzero(res.counts[:n] != c)[:8])
        assert np.array_equal(res.flags[:n], fl), (tag, which, np.flatnonzero(res.flags[:n] != fl)[:8])
        assert np.array_equal(res.offsets[:n + 1], off), (tag, which, np.flatnonzero(res.offsets[:n + 1] != off)[:8])
        _compare_rows(res, want, which, np.ones(n, bool), (tag, which))
    for f in per_frame:
        if 0 <= f < n:
            ko, ko2, do = want[f]
            kd, _ = ctx.batch_download(f, described=False)
            kg, dg = ctx.batch_download(f, described=True)
            assert same_kps(kd, ko), (tag, "per-frame download", f, explain(kd, ko))
            assert same_kps(kg, ko2), (tag, "per-frame download", f, explain(kg, ko2))
            assert np.array_equal(dg, do), (tag, "per-frame download", f)


@pytest.mark.parametrize("n", [257, 1024, 1025, 2048, 2049])
def test_every_frame_distinct(B, n):
    """n distinct 128 x 96 frames, device-resident, one launch: 257 - queues of 32 / 33 entries; 1 024 - the last batch with
    one frame per thread of k_export_offsets; 1 025 - two frames per thread, the last thread stretches empty; 2 048 - queues of
    256 entries (cum[] / cnt_q[] full, four rounds of 64); 2 049 - nine groups, three frames per thread.  Twice (fresh and
    dirty workspace): status, both exits in full against the oracle, rows behind the stored ones untouched, and the per-frame
    download of frames around the boundaries (a failure there and not here, or here and not there, tells the exit from the
    batch).  With the default keypoint capacity the descriptor slot of frame 2 048 starts at byte 2^31."""
    import torch
    want = S.oracle(n, W, H)
    d = torch.from_numpy(S.frames(n, W, H)).cuda()
    ctx = B.Context(0, max_candidates=CAND)
    ext = B.BriskDescriptorExtractor(context=ctx)
    for rep in range(2):
        _launch(B, ctx, ext, d, n, W, H)
        torch.cuda.synchronize()
        assert ctx.batch_status(n) == 0
        _compare_all(B, ctx, want, True, (n, rep), per_frame=(0, 7, 8, 255, 256, 1023, 1024, n - 2, n - 1))
    ctx.close()


def test_pageable_destination_and_copied_layer0(B):
    """1 025 frames of 120 x 90: the row pitch is no multiple of 64, so the engine copies layer 0 instead of reading the
    caller's frames in place; pageable destinations (the context's bounce buffer, the host copy inside the wait)."""
    import torch
    n, w, h = 1025, 120, 90
    want = S.oracle(n, w, h)
    d = torch.from_numpy(S.frames(n, w, h)).cuda()
    ctx = B.Context(0, max_candidates=CAND)
    ext = B.BriskDescriptorExtractor(context=ctx)
    _launch(B, ctx, ext, d, n, w, h)
    torch.cuda.synchronize()
    assert ctx.batch_status(n) == 0
    _compare_all(B, ctx, want, False, "120x90", per_frame=(0, 8, 1023, 1024))
    ctx.close()


def test_capacity_flags_and_row_cuts_at_2049(B):
    """2 049 frames (three per thread of k_export_offsets).  A keypoint capacity of CAP_REDUCED: exactly the frames in which
    the oracle detects more carry bit 2 and store no rows - neither detected nor described ones -, every other frame is
    complete, and the wait answers BRISK_HIP_ERR_CAPACITY with their number.  Then the default capacity and destinations that
    miss a frame by one row: the cut frame is the first of a thread's three, the middle one, or the very last frame of the
    batch; flat frames lie before and behind the first two cuts (behind the last frame there is nothing): counts, flags,
    offsets and the stored rows against expected_export, the wait's count against the ROWS_CUT flags."""
    import torch
    n = 2049
    want = S.oracle(n, W, H)
    nk = np.array([len(x[0]) for x in want])
    nd = np.array([len(x[1]) for x in want])
    kinds = S.kinds(n)
    d = torch.from_numpy(S.frames(n, W, H)).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    over = nk > S.CAP_REDUCED
    assert 20 < over.sum() < 205
    ctx = B.Context(0, max_candidates=CAND, max_keypoints=S.CAP_REDUCED)
    ext = B.BriskDescriptorExtractor(context=ctx)
    _launch(B, ctx, ext, d, n, W, H)
    for which, cnt in ((1, nd), (0, nk)):
        res = _filled(B, n, int(cnt.sum()), 48 if which else 0, True)
        rc, flagged = ctx.batch_download_wait(ctx.batch_download_all(res, described=bool(which), stream=stream), check=False)
        assert rc == ERR_CAPACITY and flagged == over.sum(), (which, rc, flagged, int(over.sum()))
        c, fl, off = S.expected_export(cnt, np.where(over, 4, 0), res.rows)
        got_fl = res.flags[:n]
        assert np.array_equal(got_fl != 0, over) and np.all(got_fl[over] & 4), (which, np.flatnonzero((got_fl != 0) != over)[:8])
        assert np.array_equal(res.counts[:n][~over], c[~over]), which
        assert np.array_equal(res.offsets[:n + 1], off), (which, np.flatnonzero(res.offsets[:n + 1] != off)[:8])
        _compare_rows(res, want, which, ~over, ("capacity", which))
    ctx.close()

    ctx = B.Context(0, max_candidates=CAND)
    ext = B.BriskDescriptorExtractor(context=ctx)
    _launch(B, ctx, ext, d, n, W, H)
    assert (n + 1023) // 1024 == 3
    flat = np.flatnonzero(kinds == S.FLAT)
    first = next(f for f in range(600, n) if f % 3 == 0 and kinds[f] == S.ORDINARY and nd[f] > 1)
    middle = next(f for f in range(1500, n) if f % 3 == 1 and kinds[f] == S.ORDINARY and nd[f] > 1)
    for cut_at in (first, middle):
        assert flat.min() < cut_at < flat.max()
    assert nd[n - 1] > 1
    prefix = np.concatenate([[0], np.cumsum(nd)])
    for cut_at in (first, middle, n - 1):
        rows_cap = int(prefix[cut_at] + nd[cut_at] - 1)
        res = _filled(B, n, int(nd.sum()), 48, True)
        res.struct.rows_cap = rows_cap                   # (the arrays are larger: what lies behind rows_cap must stay as it is)
        rc, flagged = ctx.batch_download_wait(ctx.batch_download_all(res, stream=stream), check=False)
        c, fl, off = S.expected_export(nd, np.zeros(n, int), rows_cap)
        is_cut = fl == S.ROWS_CUT
        assert is_cut[cut_at] and not is_cut[:cut_at].any() and is_cut.sum() == (nd[cut_at:] > 0).sum() and off[n] == prefix[cut_at]
        assert rc == ERR_CAPACITY and flagged == is_cut.sum(), (cut_at, rc, flagged, int(is_cut.sum()))
        assert np.array_equal(res.counts[:n], c), (cut_at, np.flatnonzero(res.counts[:n] != c)[:8])
        assert np.array_equal(res.flags[:n], fl), (cut_at, np.flatnonzero(res.flags[:n] != fl)[:8])
        assert np.array_equal(res.offsets[:n + 1], off), (cut_at, np.flatnonzero(res.offsets[:n + 1] != off)[:8])
        _compare_rows(res, want, 1, np.arange(n) < cut_at, ("cut", cut_at))
    ctx.close()


def test_descriptor_slots_beyond_4_gib(B):
    """2 049 frames on Context(0, max_candidates=4096, max_keypoints=32768): with 64-byte descriptor rows the descriptor slot
    of frame 1 024 starts at byte 2^31 and that of frame 2 048 at 2^32; the keypoint slots (28-byte records) pass 2^31 at frame
    2 341 only, the 16-byte records at frame 4 096 - not in this batch.  The workspace is 2 049 x 6.4 MB = 13.1 GB: per frame
    32 768 x 172 bytes of keypoint, record and descriptor slots (5.6 MB; 11.5 GB of the total), 4 096 x 108 bytes + 64 KB for
    candidates and ties, 0.3 MB pyramid, score map, integral image and band sums.  An allocation that fails fails the test.
    Both exits in full against the oracle, once, and the per-frame download on both sides of the two boundaries."""
    import torch
    n = 2049
    want = S.oracle(n, W, H)
    d = torch.from_numpy(S.frames(n, W, H)).cuda()
    ctx = B.Context(0, max_candidates=CAND, max_keypoints=32768)
    ext = B.BriskDescriptorExtractor(context=ctx)
    _launch(B, ctx, ext, d, n, W, H)
    torch.cuda.synchronize()
    assert ctx.batch_status(n) == 0
    st, dim = ctx.batch_desc_set()
    assert dim == 48 and st.frame_pitch * 1024 == 1 << 31 and st.frame_pitch * 2048 == 1 << 32
    _compare_all(B, ctx, want, True, "4 GiB", per_frame=(1023, 1024, 2047, 2048))
    ctx.close()


def test_host_to_host_1025_frames(B):
    """brisk_hip_detect_describe_batch_host_results with 1 025 frames from pinned host memory (slices of 64 frames behind their
    copies): two batches in flight, the second with the frames in reverse order; every frame of both against the oracle."""
    import torch
    n = 1025
    want = S.oracle(n, W, H)
    fr = S.frames(n, W, H)
    orders = [np.arange(n), np.arange(n)[::-1]]
    srcs = [torch.from_numpy(np.ascontiguousarray(fr[o])).pin_memory() for o in orders]
    ctx = B.Context(0, max_candidates=CAND)
    ext = B.BriskDescriptorExtractor(context=ctx)
    total = sum(len(x[1]) for x in want)
    dsts = [_filled(B, n, total, 48, True) for _ in orders]
    tickets = [ctx.detect_describe_batch_host_results(ext, srcs[b].data_ptr(), n, W, H, W * H, W, S.THR, S.OCT, dsts[b]) for b in range(2)]
    for b in (1, 0):                                     # (waiting for the later one completes the earlier one as well)
        assert ctx.batch_download_wait(tickets[b]) == 0, b
    for b, o in enumerate(orders):
        w_b = [want[i] for i in o]
        c, fl, off = S.expected_export([len(x[1]) for x in w_b], np.zeros(n, int), dsts[b].rows)
        assert np.array_equal(dsts[b].counts[:n], c) and np.array_equal(dsts[b].flags[:n], fl), b
        assert np.array_equal(dsts[b].offsets[:n + 1], off), (b, np.flatnonzero(dsts[b].offsets[:n + 1] != off)[:8])
        _compare_rows(dsts[b], w_b, 1, np.ones(n, bool), ("host", b))
    ctx.close()

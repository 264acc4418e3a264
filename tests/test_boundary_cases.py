"""The case builders of boundary_cases.py without a GPU: each builder asserts, on the ORACLE's counts, the condition that makes
its case reach the engine branch it is there for (test_gpu_boundary.py then compares the engine with the same expected values).
The counts are printed (pytest -s)."""
import numpy as np
import pytest

import boundary_cases as BC
import oracle_lib as O


@pytest.mark.parametrize("w,h", BC.A_SIZES)
def test_batch_frames_have_work_in_every_queue(w, h):
    distinct, want = BC.batch_frames(w, h)
    print("(a) %d x %d: detected / described per frame" % (w, h), [(len(x[0]), len(x[1])) for x in want])
    assert len({img.tobytes() for img in distinct}) == 4
    assert sum(len(x[0]) for x in want) > 200 and sum(len(x[1]) for x in want) > 100


def test_dense_frames_are_beyond_the_single_frame_and_small_kernel_limits():
    _, (ko, ko2, _) = BC.dense_single()
    print("(b) 640 x 480: %d detected, %d described = %d bytes" % (len(ko), len(ko2), len(ko2) * BC.ROW_BYTES))
    assert len(ko2) * BC.ROW_BYTES > BC.SINGLE_BYTES and len(ko) > BC.FN_SMALL and len(ko2) > BC.DP_SMALL_N
    _, want = BC.dense_batch()
    print("(b) 320 x 240:", [(len(x[0]), len(x[1])) for x in want], "keypoints per megapixel",
          [int(len(x[0]) / 0.0768) for x in want])
    assert all(len(x[0]) > BC.FN_SMALL and len(x[1]) > BC.DP_SMALL_N for x in want)
    assert all(len(x[0]) / 0.0768 > 2 * BC.DENSITY_RULE for x in want)
    assert len(BC.flat_batch()) == 4


@pytest.mark.parametrize("name", BC.VARIANTS)
def test_describe_variants(name):
    kw, X, k, (ko, do), frames, want = BC.variant(name)
    print("(d) %s: %d-byte descriptors, %d of %d provided kept, batch frames" % (name, X.strings, len(ko), len(k)),
          [(len(x[0]), len(x[1])) for x in want])
    assert X.strings == (128 if name.startswith("v1") else 48) and do.shape == (len(ko), X.strings)


def test_ordered_and_compute_scale_cases():
    _, want = BC.ordered_frame()
    _, ko = BC.no_scale_nms_frame()
    img, lists = BC.compute_scale_lists()
    print("(e) ordered: %d / %d keypoints; no scale NMS: %d; ComputeScale:" % (len(want[0]), len(want[1]), len(ko)),
          [(len(k), len(o)) for k, o in lists])
    assert len(want[0]) > 500
    assert 4 * len(lists[0][0]) <= 2 * BC.CS_CAND_CAP < 4 * len(lists[1][0])


def test_pool_and_postfilter_cases():
    print("(f) pool frames:", [(x[0].shape, len(x[3][0]), len(x[3][1])) for x in BC.pool_frames()])
    img, (r, mu, ku), (nbu, nbv, mb, kb), n = BC.postfilter_case()
    print("(g) %d detected, uniformity keeps %d, bucketing keeps %d" % (n, len(ku), len(kb)))
    assert len(ku) < n and len(kb) < n


def test_16bit_sweep_covers_every_width_residue_and_the_refused_shapes():
    """widths 13 ... 48: every residue of the 8- and 16-element blocks (and of the 12-element block of the two-thirds sampler)
    at least twice; some shapes the reference's loops write nothing for"""
    ws = sorted({w for _, w in BC.SHAPES16})
    assert ws == list(range(13, 49)) and sorted({h for h, _ in BC.SHAPES16}) == list(range(3, 15))
    for m in (8, 12, 16):
        assert all(sum(1 for w in ws if w % m == r) >= 2 for r in range(m))
    none_half = sum(O.halfsample16(BC.image16(h, w)) is None for h, w in BC.SHAPES16)
    none_23 = sum(O.twothirdsample16(BC.image16(h, w)) is None for h, w in BC.SHAPES16)
    print("(g) %d shapes: halfsample16 writes nothing for %d, twothirdsample16 for %d" % (len(BC.SHAPES16), none_half, none_23))
    assert 0 < none_half < len(BC.SHAPES16) and none_23 < len(BC.SHAPES16)   # (the two-thirds sampler takes every width from 13 on)
    assert np.isfinite(O.integral16(BC.image16(14, 48))).all()

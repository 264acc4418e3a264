"""Frames and expected values for the batch tests at 257 ... 2 049 frames per launch (test_batch_scale_fixture.py,
test_gpu_batch_scale.py).  No GPU in here: the frames come from synth.gen, the expected values from the CPU oracle and - for
the exit to host memory - from a NumPy restatement of the contract in include/brisk_hip.h.

Every frame of a batch differs from every other one, so that a kernel which takes a count, a record list or an integral
image from another frame of the batch (the engine's cross-frame bookkeeping is modulo 8: frame f +- 8 k is the likely
victim) changes a result.  Three kinds of special frames are spliced in at fixed places of the index range, and as the last
three frames of every batch: flat ones (nothing detected), ones with detections but no described keypoint (texture only
where the extractor's border filter removes every keypoint), and dense ones (more detections than CAP_REDUCED, the reduced
keypoint capacity of the capacity test)."""
import numpy as np

import oracle_lib as O
import synth

THR, OCT = 40, 2          # detector threshold and octaves of every batch in these tests
NRECT = 6                 # rectangles of an ordinary frame (synth.gen)
NRECT_DENSE = 40          # of a dense one
SEED0 = 5000              # frame f of a batch is synth.gen(w, h, SEED0 + f, NRECT)
# Reduced keypoint capacity of the capacity test (128 x 96 frames): ordinary frames have 63 ... 127 detections, about 3 % of
# them more than this; every dense frame has at least DENSE_MIN_128x96 (test_batch_scale_fixture.py pins both).
CAP_REDUCED = 110
DENSE_MIN_128x96 = 130
ROWS_CUT = 0x100          # BRISK_HIP_ROWS_CUT

ORDINARY, FLAT, UNDESCRIBED, DENSE = 0, 1, 2, 3
# Fixed places of the special frames: each kind in [0, 1024) and in [1024, 2048), next to one another around 1 024 ... 1 031
# (a thread of the offsets kernel then owns frames of several kinds), none on 0, 7, 8, 255, 256, 1 023, 1 024, 2 047 or 2 048.
FIXED = {
    FLAT: (5, 261, 770, 1030, 1290, 1801),
    UNDESCRIBED: (13, 520, 1027, 1540, 2040),
    DENSE: (21, 515, 1031, 1550, 2041),
}
TAIL = (FLAT, UNDESCRIBED, DENSE)   # kinds of frames n - 3, n - 2, n - 1: the last frame of a batch always has described rows

_cache = {}   # (w, h, seed0, f, kind) -> (image, detected keypoints, described keypoints, descriptors)
_extractor = None


def kinds(n):
    """kind of each of the n frames of a batch"""
    assert n >= 32
    k = np.zeros(n, np.int8)
    for kind, places in FIXED.items():
        for f in places:
            if f < n - len(TAIL):
                k[f] = kind
    k[n - len(TAIL):] = TAIL
    return k


def _oracle(img):
    global _extractor
    if _extractor is None:
        _extractor = O.Extractor()
    ko = O.detect(img, THR, OCT)
    ko2, do = _extractor.compute(img, ko)
    return ko, ko2, do


def dense_min(w, h):
    return DENSE_MIN_128x96 * w * h // (128 * 96)


def _make(w, h, seed0, f, kind):
    """-> (image, detected, described, descriptors) of frame f as a frame of that kind"""
    if kind == ORDINARY:
        img = synth.gen(w, h, seed0 + f, NRECT)
        return (img,) + _oracle(img)
    if kind == FLAT:
        img = np.full((h, w), 20 + f % 211, np.uint8)
        return (img,) + _oracle(img)
    if kind == UNDESCRIBED:
        # a frame of its own seed, the interior flattened; the band of texture that is left is the widest (of an even
        # width) in which the oracle detects keypoints and describes none
        base = synth.gen(w, h, seed0 + f, NRECT)
        for band in range(20, 4, -2):
            img = base.copy()
            inner = img[band:h - band, band:w - band]
            inner[:] = int(inner.mean())
            r = _oracle(img)
            if len(r[0]) > 0 and len(r[1]) == 0:
                return (img,) + r
        raise AssertionError("no band of frame %d keeps detections and loses every described keypoint" % f)
    assert kind == DENSE
    for s in range(64):
        img = synth.gen(w, h, seed0 + 100000 + 64 * f + s, NRECT_DENSE)
        r = _oracle(img)
        if len(r[0]) >= dense_min(w, h):
            return (img,) + r
    raise AssertionError("no dense frame found for index %d" % f)


def _entries(n, w, h, seed0):
    out = []
    for f, kind in enumerate(kinds(n)):
        key = (w, h, seed0, f, int(kind))
        if key not in _cache:
            _cache[key] = _make(w, h, seed0, f, int(kind))
        out.append(_cache[key])
    return out


def frames(n, w, h, seed0=SEED0):
    """(n, h, w) uint8: n frames that all differ, the special ones at kinds(n)'s places"""
    return np.stack([e[0] for e in _entries(n, w, h, seed0)])


def oracle(n, w, h, seed0=SEED0):
    """per frame of frames(n, w, h, seed0): (detected keypoints, described keypoints, descriptors); cached for the process -
    the entries are shared: leave them unchanged"""
    return [e[1:] for e in _entries(n, w, h, seed0)]


def expected_export(counts, overflow, rows_cap):
    """What brisk_hip_batch_download_all stores for frames with `counts` rows and capacity flags `overflow` in a destination of
    rows_cap rows, from the contract in include/brisk_hip.h: -> (counts, flags, offsets[n + 1]).
    A frame flagged for capacity wants no rows; offsets are the exclusive prefix sums of the wanted rows; the first frame whose
    rows do not fit is cut together with every later frame that wants rows: a cut frame is flagged ROWS_CUT, keeps its true
    count, and its offset - like offsets[n] - is the prefix at the cut; frames behind the cut that want no rows are not flagged."""
    counts = np.asarray(counts, np.int64)
    overflow = np.asarray(overflow, np.int64)
    n = len(counts)
    want = np.where(overflow != 0, 0, counts)
    prefix = np.concatenate([[0], np.cumsum(want)])
    misfit = (want > 0) & (prefix[1:] > rows_cap)
    cut = np.zeros(n, bool)
    stop = prefix[n]
    if misfit.any():
        first = int(np.argmax(misfit))
        stop = prefix[first]
        cut = (np.arange(n) >= first) & (want > 0)
    offsets = np.minimum(prefix, stop)
    flags = overflow | np.where(cut, ROWS_CUT, 0)
    return counts.astype(np.int32), flags.astype(np.int32), offsets.astype(np.int64)


def slot_frame(f, nd):
    """The distinct frame (of nd >= 2) that slot f of a batch filled from nd frames holds: (f + f // 8) % nd moves on by one
    more every 8 slots, so slots f and f +- 8 (f ^ 8 is one of them) are 9 frames apart and hold different frames - unless nd
    divides 9 (three distinct frames): there the step per 8 slots is 2 (10 frames apart)."""
    step = 1 if 9 % nd else 2
    return (f + step * (f // 8)) % nd

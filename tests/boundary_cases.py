"""Inputs and expected values of test_gpu_boundary.py (and of its second run on the release library, test_gpu_release.py).
No GPU in here: the inputs come from synth.gen / NumPy generators, the expected values from the CPU oracle.

Every case exists to make the engine take one branch of its dispatch - a tie-kernel form, the staged exit of a single-frame
result, the large-count kernels, an integral format, a k_describe variant, ComputeScale's two forms.  Which branch a call takes
depends on frame, layer and keypoint COUNTS, so each builder asserts, on the oracle's counts, the condition that makes its
case reach the branch (test_boundary_cases.py runs the builders without a GPU); the limits below restate the engine's constants.

The builders cache their results for the process; the entries are shared: leave them unchanged."""
import os

import numpy as np

import oracle_lib as O
import synth

HERE = os.path.dirname(os.path.abspath(__file__))

# the engine's limits the conditions are about
SINGLE_BYTES = 1 << 20      # BRISK_SINGLE_BYTES (brisk_capi.hip): pinned buffer of a single-frame result; beyond it, staged copies
ROW_BYTES = 28 + 64         # a described row in that buffer: keypoint record + descriptor row
FN_SMALL = 3072             # brisk_kernels.hip: more keypoints than this in a frame -> k_finalize_large
DP_SMALL_N = 2048           # brisk_describe.hip: more described keypoints -> k_dp_count / k_dp_scan / k_dp_scatter
DENSITY_RULE = 3000.0       # integral_format (brisk_capi.hip): candidates per megapixel of the previous batch, above -> 32 bits
HOST_SLICE = 64             # default slice of the host-fed batch entry

# (a) batches by frame count
A_THR, A_OCT = 40, 2
A_SIZES = ((256, 192), (201, 131))    # layer 0 read in place (width a multiple of 64) / copied, odd column classes
A_COUNTS = (1, 9, 33, 65, 129, 200, 257)
A_COUNTS_ODD = (9, 65)
A_NRECT = 24

_cache = {}


def _memo(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]


def oracle_frame(img, thr, octaves, extractor=None):
    """(detected keypoints, described keypoints, descriptors)"""
    ko = O.detect(img, thr, octaves)
    return (ko,) + tuple((extractor or O.Extractor()).compute(img, ko))


def batch_frames(w, h):
    """(a): four distinct frames of w x h and their oracle results at A_THR / A_OCT"""
    def make():
        X = O.Extractor()
        distinct = [synth.gen(w, h, 8800 + s, A_NRECT) for s in range(4)]
        want = [oracle_frame(img, A_THR, A_OCT, X) for img in distinct]
        nk, nd = sum(len(x[0]) for x in want), sum(len(x[1]) for x in want)
        # enough work in every layer's tie / describe queues to tell a wrong form from a right one
        assert nk > 200 and nd > 100, "frames of %d x %d are too sparse (%d detected, %d described): raise the size" % (w, h, nk, nd)
        return distinct, want
    return _memo(("a", w, h), make)


def noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)


# (b) dense frames
B_THR = 30


def dense_single():
    """(b): 640 x 480 uniform noise, 4 octaves -> (image, oracle result); the three branch conditions asserted"""
    def make():
        img = noise(640, 480, 4100)
        want = oracle_frame(img, B_THR, 4)
        nk, nd = len(want[0]), len(want[1])
        assert nd * ROW_BYTES > SINGLE_BYTES, (nd, "the described result fits the pinned single-frame buffer")
        assert nk > 4096 and nk > FN_SMALL, (nk, "k_finalize orders this frame on chip")
        assert nd > DP_SMALL_N, (nd, "k_desc_prepare's one-workgroup form takes this frame")
        assert nk <= 65536, nk   # (the capacity the test's context is given)
        return img, want
    return _memo("b1", make)


def dense_batch():
    """(b), (c): four 320 x 240 noise frames, 2 octaves -> (frames, oracle results); every frame beyond both kernel limits,
    and denser than twice the density rule"""
    def make():
        X = O.Extractor()
        frames = [noise(320, 240, 4200 + s) for s in range(4)]
        want = [oracle_frame(img, B_THR, 2, X) for img in frames]
        for ko, ko2, _ in want:
            assert len(ko) > FN_SMALL and len(ko2) > DP_SMALL_N, (len(ko), len(ko2))
            # candidates are at least as many as keypoints: the batch is on the 32-bit side of the rule with a factor of two to spare
            assert len(ko) / (320 * 240 / 1e6) > 2 * DENSITY_RULE, len(ko)
        return frames, want
    return _memo("b2", make)


def flat_batch():
    """(c): four constant 320 x 240 frames: no keypoints (so no candidates: the sparse side of the density rule)"""
    def make():
        frames = [np.full((240, 320), 40 + 50 * s, np.uint8) for s in range(4)]
        for img in frames:
            assert len(O.detect(img, B_THR, 2)) == 0
        return frames
    return _memo("c", make)


# (d) the other k_describe variants
def golden_image():
    from setfile import read_set
    return _memo("golden", lambda: read_set(os.path.join(HERE, "golden", "brisk_verification_harris.set"))[0])


def provided_from_golden(sizes=None):
    """the golden set's keypoints as provided ones (orientation to be estimated); sizes: (lo, hi) spreads them over the scales"""
    g = golden_image()["keypoints"]
    k = np.zeros(len(g), O.KP)
    for f in ("x", "y", "size", "response", "octave", "class_id"):
        k[f] = g[f]
    k["angle"] = -1
    if sizes:
        k["size"] = np.linspace(sizes[0], sizes[1], len(k)).astype(np.float32)
    return k


D_THR, D_OCT = 70, 3
VARIANTS = ("v1_scale_0.7", "ptn_scale_0.45")


def variant(name):
    """(d): -> (constructor arguments of the engine's extractor, oracle extractor, provided keypoints, their oracle result,
    two distinct frames for the batch, their oracle results)"""
    def make():
        img = golden_image()["image"]
        if name == "v1_scale_0.7":
            kw = dict(version=1, patternScale=0.7)
            X = O.Extractor(version=1, pattern_scale=0.7)
            k = provided_from_golden()
            assert X.strings == 128     # 1 024 short pairs, more than the 512 the register variant holds: the LDS-table variant
        else:
            import ptn
            text = ptn.custom_pattern(1, sigma_factor=0.6, drop_points=6)
            kw = dict(pattern_text=text, patternScale=0.45)
            X = O.Extractor(pattern_text=text, pattern_scale=0.45)
            k = provided_from_golden((7.0, 40.0))   # small scales: sigma_half < 0.5, SmoothedIntensity's bilinear branch
            assert X.strings == 48
        ko, do = X.compute(img, k)
        assert len(ko) > 300, len(ko)
        frames = [img, np.ascontiguousarray(img[::-1])]
        want = [oracle_frame(f, D_THR, D_OCT, X) for f in frames]
        assert all(len(x[1]) > 100 for x in want), [len(x[1]) for x in want]
        return kw, X, k, (ko, do), frames, want
    return _memo(("d", name), make)


# (e) ordered path and ComputeScale
def ordered_frame():
    """a 160 x 120 frame at threshold 5 (below 20: the ordered path) with more than 500 keypoints"""
    def make():
        img = synth.gen(160, 120, 61, 12)
        ko = O.detect(img, 5, 2)
        assert len(ko) > 500, len(ko)
        return img, (ko,) + tuple(O.Extractor().compute(img, ko))
    return _memo("e1", make)


def no_scale_nms_frame():
    """four layers, suppressScaleNonmaxima = false, texture confined to the top rows (where the reference's result is defined)"""
    def make():
        from test_emul_parity import banded
        img = banded(0, cell=3)
        ko = O.detect(img, 60, 2, suppress_scale_nonmaxima=False)
        assert ko is not None and len(ko) > 300 and len(set(ko["size"])) >= 2
        return img, ko
    return _memo("e2", make)


CS_CAND_CAP = 4096           # candidate capacity of the ComputeScale context
CS_THR, CS_OCT = 60, 2       # four layers: the parallel form holds lists of up to 2 * CS_CAND_CAP / 4 = 2 048 points


def compute_scale_lists():
    """-> (image, [(provided list, oracle result)] x 2): a list within 2 * cand_cap / nlayers (parallel form) and one beyond
    (the one-lane walk)"""
    def make():
        img = synth.gen(320, 240, 9, 30)
        rng = np.random.default_rng(77)
        nlayers = 2 * CS_OCT
        limit = 2 * CS_CAND_CAP // nlayers
        out = []
        for n in (limit - 48, limit + 452):
            k = np.zeros(n, O.KP)
            k["x"] = rng.uniform(0, 320, n).astype(np.float32)
            k["y"] = rng.uniform(0, 240 - 75, n).astype(np.float32)   # (the bottom band has no defined result in the reference)
            k["size"], k["angle"] = 10, -1
            k["class_id"] = rng.integers(-1, 50, n)
            ko = O.compute_scale(img, k, CS_THR, CS_OCT, True)
            assert ko is not None and len(ko) > 100, n
            out.append((k, ko))
        assert nlayers * len(out[0][0]) <= 2 * CS_CAND_CAP < nlayers * len(out[1][0])
        return img, out
    return _memo("e3", make)


# (f) the pool
def pool_frames():
    """two frame sizes / thresholds / octave counts: [(image, threshold, octaves, oracle result)]"""
    def make():
        X = O.Extractor()
        out = []
        for i in range(3):
            img = synth.gen(333, 201, 7700 + i, 40)
            out.append((img, 60, 2, oracle_frame(img, 60, 2, X)))
        distinct, want = batch_frames(256, 192)
        for img, w in zip(distinct[:3], want[:3]):
            out.append((img, A_THR, A_OCT, w))
        assert all(len(x[3][1]) > 20 for x in out)
        return out
    return _memo("f", make)


# (g) post-filters and the 16-bit functions
G_THR, G_OCT = 60, 4


def postfilter_case():
    """-> (image, uniformity: (radius, budget, kept), bucketing: (nbu, nbv, budget, kept)); both filters remove keypoints"""
    def make():
        img = golden_image()["image"]
        h, w = img.shape
        ko = O.detect(img, G_THR, G_OCT)
        ku = O.enforce_uniformity(ko, h, w, 20.0, 400)
        kb = O.key_point_bucketing(ko, h, w, 240, 8, 6)
        assert kb is not None and 0 < len(ku) < len(ko) and 0 < len(kb) < len(ko), (len(ko), len(ku), len(kb))
        return img, (20.0, 400, ku), (8, 6, 240, kb), len(ko)
    return _memo("g1", make)


SHAPES16 = [(h, w) for h in range(3, 15) for w in range(13, 49)]


def image16(h, w):
    """random uint16 content with saturated stripes"""
    img = np.random.default_rng(h * 64 + w).integers(0, 65536, (h, w), dtype=np.uint16)
    img[::5, ::3] = 65535
    return img

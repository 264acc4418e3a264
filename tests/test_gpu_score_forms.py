"""GPU tests (run with -m gpu) of the packed forms of the detector gate and the 9-of-16 score in their kernels: k_detect's
pre-gate (pass flags collected with byte permutes from the unmasked differences), its phase B and k_score_blocks (arcs by
prefix / suffix minima, the centre subtracted from the reduced values).  One batch of three small frames through the batch
path, bit-exact against the CPU oracle, at three thresholds: 80 (the benchmark's; gate multiplier K = 204, shift s = 8),
20 (K = 51, s = 8) and 255 (K = 163, s = 6).  tests/test_emul_score_forms.py proves the forms themselves on the host."""
import functools

import numpy as np
import pytest

import oracle_lib as O
import synth
from test_gpu_parity import same_kps, explain

pytestmark = pytest.mark.gpu

W, H, OCT = 200, 152, 2   # 3 full 64-wide tiles + 8 columns, 2 full 64-high tiles + 24 rows on layer 0


@pytest.fixture(scope="module")
def B():
    import ethzasl_brisk_amd as B
    from ethzasl_brisk_amd import build
    build.build()
    B.load_library()
    return B


@functools.lru_cache(maxsize=None)
def frames():
    rng = np.random.default_rng(41)
    recipe = synth.gen(W, H, 9, 14)
    # 0 / 255 blocks with single-pixel impulses: saturated differences (+-255 against the centre) and ties between equal scores
    blocks = (np.kron(rng.integers(0, 2, (H // 8, W // 8)), np.ones((8, 8))) * 255).astype(np.uint8)
    ys, xs = rng.integers(0, H, 160), rng.integers(0, W, 160)
    blocks[ys, xs] = rng.choice(np.array([0, 255], np.uint8), 160)
    # texture only in the band around the 3-pixel border and in the last, partial 64 x 64 tile (columns 192 ..., rows 128 ...)
    edge = np.full((H, W), 128, np.uint8)
    tex = rng.choice(np.array([8, 128, 128, 128, 248], np.uint8), (H, W))
    band = np.zeros((H, W), bool)
    band[:8, :] = band[-8:, :] = True
    band[:, :8] = band[:, -8:] = True
    band[128:, 192:] = True
    band[120:, 186:] = True
    edge[band] = tex[band]
    f = np.ascontiguousarray(np.stack([recipe, blocks, edge]))
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def oracle(thr):
    X = O.Extractor()
    out = []
    for img in frames():
        ko = O.detect(np.ascontiguousarray(img), thr, OCT)
        assert ko is not None
        ko2, do = X.compute(np.ascontiguousarray(img), ko)
        out.append((ko, ko2, do))
    return out


@pytest.mark.parametrize("thr", [80, 20, 255])
def test_batch_of_three_frames_vs_oracle(B, thr):
    """a recipe frame, a frame of 0 / 255 blocks with impulses, a frame with texture only along the border band and in the last
    partial tile: detected keypoints, described keypoints and descriptors of every frame equal the oracle's"""
    import torch
    want = oracle(thr)
    d = torch.from_numpy(np.array(frames())).cuda()
    ctx = B.Context(0)
    ext = B.BriskDescriptorExtractor(context=ctx)
    n = len(want)
    ctx.detect_describe_batch(ext, d.data_ptr(), n, W, H, W * H, W, thr, OCT, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert ctx.batch_status(n) == 0
    print("threshold %d: keypoints per frame %s" % (thr, [len(x[0]) for x in want]))
    for f in range(n):
        ko, ko2, do = want[f]
        kd, _ = ctx.batch_download(f, described=False)
        kg, dg = ctx.batch_download(f, described=True)
        assert same_kps(kd, ko), (thr, f, explain(kd, ko))
        assert same_kps(kg, ko2), (thr, f, explain(kg, ko2))
        assert np.array_equal(dg, do), (thr, f)
    if thr == 80:
        assert all(len(x[0]) > 0 for x in want)   # every frame exercises phase B and the score blocks

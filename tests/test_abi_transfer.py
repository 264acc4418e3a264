"""CPU checks of what the two exits to host memory share (brisk_hip_batch_download_all, brisk_hip_pair_matches_download): the
layout helper - the very header the library includes, built here for the host - places the arrays of a transfer where the two
exits have always had them, and the host-only headers stay out of the kernel revision."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "ethzasl_brisk_amd", "csrc")
KEYPOINT_BYTES, DMATCH_BYTES = 28, 16


def build_program():
    """tests/cpp/test_slab_layout.cc: plain host C++ around csrc/brisk_slab_layout.h (no HIP, no library)"""
    src = os.path.join(ROOT, "tests", "cpp", "test_slab_layout.cc")
    hdr = os.path.join(CSRC, "brisk_slab_layout.h")
    out = os.path.join(ROOT, "tests", "cpp", "test_slab_layout")
    if not os.path.exists(out) or any(os.path.getmtime(p) > os.path.getmtime(out) for p in (src, hdr)):
        subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-I" + os.path.dirname(hdr), "-o", out, src])
    return out


def batch_arrays(frames, rows, desc_stride):
    """byte sizes of counts, flags, offsets, kps, desc of a batch's results (brisk_hip_batch_host_results)"""
    return [4 * frames, 4 * frames, 8 * (frames + 1), KEYPOINT_BYTES * rows, rows * desc_stride]


def match_arrays(pairs, matches):
    """byte sizes of pair_rows, counts, flags, offsets, matches of a call's selected matches (brisk_hip_pair_host_matches)"""
    return [4 * pairs, 4 * pairs, 4 * pairs, 8 * (pairs + 1), DMATCH_BYTES * matches]


def layouts(size_lists):
    """[(offsets, bytes)] the helper gives for each list of array sizes"""
    r = subprocess.run([build_program()] + [",".join(str(int(b)) for b in sizes) for sizes in size_lists], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    rows = [[int(v) for v in ln.split()] for ln in r.stdout.splitlines()]
    assert len(rows) == len(size_lists)
    return [(row[:-1], row[-1]) for row in rows]


def test_the_exits_layouts_are_where_they_were():
    # offsets and totals of the two layout structs this helper replaced, worked out from their formulas (each array at the
    # next multiple of 256 behind the previous one, the total = the rounded end + 256)
    batch = {(65, 1000, 48): ([0, 512, 1024, 1792, 29952], 78336),
             (1, 0, 4): ([0, 256, 512, 768, 768], 1024),
             (4, 2 ** 31, 64): ([0, 256, 512, 768, 60129542912], 197568496640)}
    match = {(3, 10): ([0, 256, 512, 768, 1024], 1536),
             (1, 0): ([0, 256, 512, 768, 1024], 1280)}
    got = layouts([batch_arrays(*k) for k in batch] + [match_arrays(*k) for k in match])
    for (shape, want), g in zip(list(batch.items()) + list(match.items()), got):
        assert g == want, (shape, g, want)


def test_arrays_are_aligned_and_apart():
    rng = np.random.default_rng(256)
    sizes = []
    for i in range(300):
        if i % 2:
            sizes.append(batch_arrays(int(rng.integers(1, 600)), int(rng.choice([0, 1, 9, 255, 256, int(rng.integers(0, 2 ** 20)), 2 ** 31 + int(rng.integers(0, 999))])),
                                      4 * int(rng.integers(1, 57))))
        else:
            sizes.append(match_arrays(int(rng.integers(1, 3000)), int(rng.choice([0, 1, 15, 16, 17, int(rng.integers(0, 2 ** 22)), 2 ** 31 + int(rng.integers(0, 999))]))))
    sizes.append([int(b) for b in rng.integers(0, 1025, 8)])            # as many arrays as a layout holds, of any size
    wide = 0
    for arrays, (offsets, total) in zip(sizes, layouts(sizes)):
        assert len(offsets) == len(arrays) and offsets[0] == 0
        assert all(o % 256 == 0 for o in offsets)
        for i in range(1, len(arrays)):
            assert offsets[i] >= offsets[i - 1] + arrays[i - 1]          # no overlap ...
            assert offsets[i] - (offsets[i - 1] + arrays[i - 1]) < 256   # ... and no gap beyond the rounding
        assert total % 256 == 0 and offsets[-1] + arrays[-1] + 256 <= total < offsets[-1] + arrays[-1] + 512
        wide += total > 2 ** 32
    assert wide > 20                                                     # totals no 32-bit value holds were among them


def test_host_headers_stay_out_of_the_kernel_revision(tmp_path, monkeypatch):
    """bench.py reads profiles/traffic.json only for the kernel revision it measured: a change to host-only code must not move it"""
    import shutil
    from ethzasl_brisk_amd import build
    rev = build.kernel_revision()
    assert len(rev) == 12
    copy = tmp_path / "csrc"
    shutil.copytree(CSRC, copy)
    monkeypatch.setattr(build, "CSRC", str(copy))
    assert build.kernel_revision() == rev
    for name in ("brisk_hostmem.h", "brisk_slab_layout.h", "brisk_transfer.h", "brisk_capi.hip", "brisk_pool.inc"):
        text = (copy / name).read_text()
        assert "__global__" not in text and "__device__" not in text, name
        (copy / name).write_text(text + "// changed\n")
        assert build.kernel_revision() == rev, name
    (copy / "brisk_kernels.h").write_text((copy / "brisk_kernels.h").read_text() + "// changed\n")
    assert build.kernel_revision() != rev                               # (device code does move it)

"""The release library (libbrisk_hip_release.so - what INTEGRATION.md links; no BRISK_HIP_TUNING) on every dispatch branch of
the public ABI.  Each test is ONE fresh child process of tests/release_run.py with BRISK_HIP_LIB set to the release library
(one GPU process at a time): the case groups (a) ... (g) of test_gpu_boundary.py, the chain matcher -> selection -> verify ->
guided matcher -> linker -> exports once, slices of the fuzz suites of tools/soak_cases/, and the C++ drop-in classes linked
with -lbrisk_hip_release.  The child refuses any other library before its first HIP call.

Each child's time limit is its measured duration on the tuning library times five, rounded up to ten seconds (DURATIONS_S:
wall seconds of the child's work on an MI355X, python's start included).  A child that ends by an abort, a
segmentation fault or its time limit is recorded: every later test of the module then fails at once without starting a child.

What each child is there for, with the oracle-side count that shows the branch is reached (boundary_cases.py asserts them), its
seconds on the tuning library and its limit:
  a  tie-kernel forms by frame count (1 / 9 / 33 / 65 / 129 / 200 / 257 frames x 4 layers), k_describe's ticketed queues;
     four distinct frames: 1 496 detected / 917 described at 256 x 192, 885 / 365 at 201 x 131                       4.5 s  30 s
  b  staged single-frame exit, k_finalize_large, k_dp_*: 18 900 detected / 15 718 described = 1 446 056 bytes > 2^20;
     batch frames 4 338 ... 4 388 / 3 055 ... 3 137 (> 3 072 / > 2 048)                                                4.9 s  30 s
  c  integral format 24 / 32 / 32 / 24 / 32 by the density rule: D frames 56 484 ... 57 135 keypoints per megapixel
     (> 2 x 3 000), F frames 0; then 24 and 32 bits set by the caller                                                  4.5 s  30 s
  d  LDS-table variant (briskV1 x 0.7: 128-byte descriptors = 1 024 short pairs; 454 provided kept) and bilinear variant
     (.ptn x 0.45: 450 of 454 kept); nine-frame batches 663 ... 718 described per frame                                4.2 s  30 s
  e  ordered path (threshold 5: 1 462 keypoints > 500), no scale NMS on four layers (916), ComputeScale parallel form
     (2 000 points x 4 layers <= 2 x 4 096) and one-lane walk (2 500 points x 4 > 8 192)                               5.4 s  30 s
  f  host-fed batch of 65 frames > the slice of 64, pageable and pinned; pool of six threads, two frame sizes          5.0 s  30 s
  g  uniformity (1 613 -> 400) and bucketing (1 613 -> 240); 16-bit functions on 432 shapes (36 the reference refuses)  4.0 s  20 s
  chain     matcher -> selection -> verify -> guided matcher -> linker -> exports, 7 cases                             5.2 s  30 s
  callspace 300 cases 4.4 s 30 s; options 100 cases 4.2 s 30 s; matcher 120 cases 4.3 s 30 s; hostpaths 80 cases 4.2 s 30 s;
  large 150 cases 3.7 s 20 s; describe (fixed size) 3.9 s 20 s; ordered (fixed size) 3.0 s 20 s
  C++ test_binary_equal 0.5 s 10 s; test_host_results 0.4 s 10 s

The limit of this net: the edits change no result, so a release build with BRISK_SINGLE_BYTES = 4 MiB passes everything (b's single
frame then stays in the pinned buffer: the staged exit is no longer run), and so does one whose integral_format always answers 32
(c's first and fourth batch and its 24-bit descriptor-only calls then run the 32-bit kernels).  Bit-exact output shows that the
branch a build takes is right, not which branch it takes."""
import math
import os
import re
import subprocess
import sys

import pytest

import release_run

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
gpu = pytest.mark.gpu

# measured wall seconds of each child on the tuning library (python start and imports included)
DURATIONS_S = {
    "a": 4.5, "b": 4.9, "c": 4.5, "d": 4.2, "e": 5.4, "f": 5.0, "g": 4.0, "chain": 5.2,
    "callspace": 4.4, "options": 4.2, "matcher": 4.3, "hostpaths": 4.2, "large": 3.7, "describe": 3.9, "ordered": 3.0,
    "cpp_test_binary_equal": 0.5, "cpp_test_host_results": 0.4,
}


def limit(key):
    return int(math.ceil(DURATIONS_S[key] * 5 / 10.0) * 10)


_fatal = []   # the first child that aborted, faulted or ran into its limit


def run(cmd, key, env=None):
    """one child process under its time limit -> (return code, output); fatal ends recorded"""
    if _fatal:
        pytest.fail("not started: an earlier child of this module ended abnormally (%s)" % _fatal[0])
    what = " ".join(os.path.basename(c) for c in cmd[:4])
    try:
        r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit(key))
    except subprocess.TimeoutExpired as e:
        _fatal.append("%s: no end within %d s" % (what, limit(key)))
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        print(out[-4000:])
        pytest.fail(_fatal[0])
    print(r.stdout[-6000:])
    if r.returncode in (134, 139, -6, -11):
        _fatal.append("%s: status %d" % (what, r.returncode))
    return r.returncode, r.stdout


def child(args, key, lib=None):
    """one child of release_run.py with BRISK_HIP_LIB = the release library (or `lib`)"""
    from ethzasl_brisk_amd import build
    lib = lib or build.build_release()
    return run([sys.executable, os.path.join(ROOT, "tests", "release_run.py")] + list(args), key, dict(os.environ, BRISK_HIP_LIB=lib))


def served_from_release(out):
    from ethzasl_brisk_amd import build
    lines = [ln for ln in out.splitlines() if ln.startswith(release_run.SERVED)]
    return len(lines) == 1 and os.path.realpath(lines[0][len(release_run.SERVED):].strip()) == os.path.realpath(build.LIB_RELEASE)


def run_pytest_ids(ids, expected, key):
    """pytest mode: status 0, the served-from line, and exactly `expected` tests passed - none skipped, failed or deselected"""
    rc, out = child(["pytest"] + ids, key)
    assert rc == 0, (rc, out[-1500:])
    assert served_from_release(out), out[:500]
    summary = [ln for ln in out.splitlines() if re.search(r"\b\d+ passed\b", ln)]
    assert summary, out[-1500:]
    counts = {k: int(v) for v, k in re.findall(r"(\d+) (passed|failed|skipped|deselected|error|errors|xfailed|xpassed)", summary[-1])}
    assert counts == {"passed": expected}, (counts, expected)


def test_a_library_that_is_not_the_release_build_is_refused():
    """BRISK_HIP_LIB = the tuning library: the child ends with its own status and a message before it runs anything"""
    from ethzasl_brisk_amd import build
    rc, out = child(["pytest", os.path.join(ROOT, "tests", "test_gpu_boundary.py")], "g", lib=build.build())
    assert rc == release_run.REFUSED and "REFUSED" in out, (rc, out[-1500:])
    assert release_run.SERVED not in out and "passed" not in out and "failed" not in out
    rc, out = child(["soak", "matcher", "20", "3"], "g", lib=build.LIB)
    assert rc == release_run.REFUSED and release_run.SERVED not in out and "matcher:" not in out


def test_the_release_library_exports_the_abi_and_no_debug_entry_point():
    import ethzasl_brisk_amd as B
    from ethzasl_brisk_amd import build
    rel, tun = release_run.exported_symbols(build.build_release()), release_run.exported_symbols(build.build())
    assert not [s for s in B.ABI_SYMBOLS if s not in rel]
    assert not [s for s in rel if s.startswith("brisk_hip_debug_")]
    assert not [s for s in B.DEBUG_SYMBOLS if s not in tun]   # (the reader sees them where they exist)


def boundary_group(g):
    import test_gpu_boundary as T
    tests = T.GROUPS[g]
    return [os.path.join(ROOT, "tests", "test_gpu_boundary.py") + "::" + name for name in sorted(tests)], sum(tests.values())


@gpu
@pytest.mark.parametrize("group", list("abcdefg"))
def test_boundary_group_on_the_release_library(group):
    """(a) tie-kernel / k_describe queue forms by frame count, (b) staged single-frame exit + large-count kernels, (c) integral
    format by the density rule, (d) LDS-table and bilinear k_describe variants, (e) ordered path + both ComputeScale forms,
    (f) host-fed slices + pool, (g) post-filters + 16-bit functions"""
    if group == "a":
        from test_gpu_boundary import require_256_cus
        require_256_cus()
    ids, expected = boundary_group(group)
    run_pytest_ids(ids, expected, group)


# (node id, its number of cases)
CHAIN = [("test_gpu_match.py::test_pipeline_in_hbm_detect_describe_match", 1), ("test_gpu_verify.py::test_the_pipeline", 1),
         ("test_gpu_match_guided.py::test_the_real_path_without_the_host", 1), ("test_gpu_tracks.py::test_the_real_path", 1),
         ("test_gpu_track_export.py::test_the_real_path", 1), ("test_gpu_match_export.py::test_host_form_on_a_batch", 2)]


@gpu
def test_the_chain_once_on_the_release_library():
    """matcher, selection, verify, guided matcher, linker and the exports name no debug flag: one pass through each on what the
    release engine produces shows that they link and run there"""
    run_pytest_ids([os.path.join(ROOT, "tests", t) for t, _ in CHAIN], sum(n for _, n in CHAIN), "chain")


# fuzz slices: (suite, arguments, the summary line's start, its clean mark); seeds other than test_gpu_round3.py's 11 and 13.
# Case counts: about five seconds per child (test_gpu_round3.py's runs on the tuning library took 4.1 s for 250 callspace cases,
# 7.7 s for 200 option cases, 5.5 s for 200 matcher cases, about 2 s of each being python's start); describe and ordered have fixed sizes.
FUZZ = [("callspace", ["300", "17"], "callspace: 300 cases", " 0 bad"), ("options", ["100", "19"], "options: 100 cases", " 0 bad"),
        ("matcher", ["120", "29"], "matcher: 120 cases", " 0 bad"), ("hostpaths", ["80", "29"], "hostpaths: 80 cases", " 0 bad"),
        ("large", ["150", "31"], "large: 150 16-bit images", " 0 bad"), ("describe", [], "describe: ", "describe: 0 mismatching"),
        ("ordered", [], "ordered: ", " 0 mismatches")]


@gpu
@pytest.mark.parametrize("suite,args,start,clean", FUZZ, ids=[f[0] for f in FUZZ])
def test_fuzz_slice_on_the_release_library(suite, args, start, clean):
    rc, out = child(["soak", suite] + args, suite)
    tail = [ln for ln in out.splitlines() if ln.startswith((suite + ":", "ERROR", "MISMATCH"))]
    assert rc == 0 and served_from_release(out), (rc, out[-1500:])
    assert tail and tail[-1].startswith(start) and clean in tail[-1], tail[-5:]
    assert not [ln for ln in tail if ln.startswith(("ERROR", "MISMATCH"))]


def release_binary(name):
    from test_cpp_classes import build_binary
    b = build_binary(name, lib="brisk_hip_release")
    blob = open(b, "rb").read()
    assert b"libbrisk_hip_release.so" in blob and b"libbrisk_hip.so" not in blob   # (what the loader will look for)
    return b


def test_the_link_line_of_the_integration_guide_builds():
    for name in ("test_binary_equal", "test_host_results"):
        assert release_binary(name).endswith(name + "_release")


@gpu
def test_drop_in_classes_linked_with_the_release_library():
    """tests/cpp/test_binary_equal and test_host_results built with -lbrisk_hip_release: the reference's golden test through the
    C++ classes, and the batch path host memory -> host memory through the C ABI"""
    for name, args, check in (("test_binary_equal", [os.path.join(ROOT, "tests", "golden")], lambda o: "Verification success" in o and o.count("OK") == 5),
                              ("test_host_results", [], lambda o: "host results OK" in o)):
        rc, out = run([release_binary(name)] + args, "cpp_" + name)
        assert rc == 0 and check(out), (name, rc)

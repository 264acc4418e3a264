"""Runs existing test code on the RELEASE library (libbrisk_hip_release.so: no BRISK_HIP_TUNING - no environment knobs, no debug
bits, no brisk_hip_debug_* exports; the library INTEGRATION.md links).  Started as a fresh child process with
BRISK_HIP_LIB=<build.build_release()> (tests/test_gpu_release.py does), never as an exec from a process that has used the GPU.

  python3 tests/release_run.py pytest <node ids ...>     pytest.main on the ids with -m gpu, in this process
  python3 tests/release_run.py soak <suite> [args ...]   tools/soak_cases/<suite>.py in this process with those arguments

Before anything else it checks that the library the package will load is the release library and exports none of
B.DEBUG_SYMBOLS - from the file's dynamic symbol table, without loading it: no HIP call happens before the check, and the check
initialises nothing (the fuzz suites fork their oracle workers before HIP is loaded).  A library that fails the check ends the
process with status REFUSED and a message; nothing is run.  Otherwise it prints one line that names the library it serves from."""
import os
import struct
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

REFUSED = 97                                  # exit status of a refused library
SERVED = "release_run: serving from "         # the line the parent asserts on


def exported_symbols(path):
    """names the ELF64 shared object `path` defines in its dynamic symbol table (read from the file: nothing is loaded)"""
    with open(path, "rb") as f:
        data = f.read()
    if data[:6] != b"\x7fELF\x02\x01":
        raise ValueError("%s is no little-endian ELF64 file" % path)
    shoff, = struct.unpack_from("<Q", data, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", data, 0x3A)
    sections = [struct.unpack_from("<IIQQQQIIQQ", data, shoff + i * shentsize) for i in range(shnum)]
    names = set()
    for s in sections:
        if s[1] != 11:                        # SHT_DYNSYM
            continue
        stroff = sections[s[6]][4]            # sh_link: its string table
        for off in range(s[4], s[4] + s[5], s[9] or 24):
            st_name, _, _, st_shndx = struct.unpack_from("<IBBH", data, off)
            if st_shndx != 0 and st_name:     # defined here
                end = data.index(b"\0", stroff + st_name)
                names.add(data[stroff + st_name:end].decode())
    return names


def check_library():
    """-> path of the release library the package will load, or exits with REFUSED"""
    import ethzasl_brisk_amd as B
    from ethzasl_brisk_amd import build
    path = os.path.realpath(B.LIB_PATH)
    if not os.environ.get("BRISK_HIP_LIB") or path != os.path.realpath(build.LIB_RELEASE):
        print("release_run: REFUSED - BRISK_HIP_LIB names %s, not the release library %s" % (B.LIB_PATH, build.LIB_RELEASE), flush=True)
        sys.exit(REFUSED)
    if not os.path.exists(path):
        print("release_run: REFUSED - %s has not been built" % path, flush=True)
        sys.exit(REFUSED)
    syms = exported_symbols(path)
    debug = sorted(s for s in syms if s in B.DEBUG_SYMBOLS or s.startswith("brisk_hip_debug_"))
    if debug or "brisk_hip_create" not in syms:
        print("release_run: REFUSED - %s %s" % (path, ("exports " + ", ".join(debug)) if debug else "exports no brisk_hip_create"), flush=True)
        sys.exit(REFUSED)
    return path


def main(argv):
    if len(argv) < 2 or argv[0] not in ("pytest", "soak"):
        print(__doc__)
        return 2
    path = check_library()
    print(SERVED + path, flush=True)
    if argv[0] == "pytest":
        import pytest
        return int(pytest.main(["-m", "gpu", "-q", "-rA", "-p", "no:cacheprovider", "--rootdir", ROOT] + argv[1:]))
    suite = os.path.join(ROOT, "tools", "soak_cases", argv[1] + ".py")
    if not os.path.isfile(suite):
        print("release_run: no suite %s" % suite)
        return 2
    import runpy
    sys.argv = [suite] + argv[2:]
    try:
        runpy.run_path(suite, run_name="__main__")
    except SystemExit as e:
        return e.code if isinstance(e.code, int) else (0 if e.code is None else 1)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))

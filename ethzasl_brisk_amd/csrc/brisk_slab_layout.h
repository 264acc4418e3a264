// brisk_slab_layout.h - host code only, plain C++ (no HIP): where the arrays of a transfer lie inside one allocation - a device
// slab, a pinned bounce buffer, a pool group's result block.  tests/cpp/test_slab_layout.cc includes it as it is.
// (No device compiler output depends on this file: build.kernel_revision() leaves it out, like brisk_capi.hip.)
#pragma once
#include <assert.h>
#include <stddef.h>
#include <stdint.h>

// Arrays appended one after another, each at the next multiple of 256 bytes; the total is the rounded end plus 256 bytes (it decides
// when a slab or a bounce buffer grows).  All arithmetic is size_t: row and match capacities above 2^31 are ordinary.
struct SlabLayout {
  size_t off[8] = {};  // off[i]: byte offset of the i-th array appended
  int n = 0;
  size_t end = 0;      // end of the last array

  static size_t up(size_t v) { return (v + 255) & ~(size_t)255; }
  size_t add(size_t bytes) {
    assert(n < 8);
    off[n] = up(end);
    end = off[n] + bytes;
    return off[n++];
  }
  size_t bytes() const { return up(end) + 256; }  // what the allocation must hold

  template <class T>
  T* at(uint8_t* base, int i) const { return reinterpret_cast<T*>(base + off[i]); }
};

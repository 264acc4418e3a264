// Host build of the layout helper of the exits to host memory (ethzasl_brisk_amd/csrc/brisk_slab_layout.h - what places the arrays
// of a transfer inside a slab, a bounce buffer and a pool group's block) for tests/test_abi_transfer.py.  Every argument is one
// layout: the byte sizes of its arrays, in order, joined by commas.  Prints one line per layout: the offset of every array, then
// the byte total.
#include <cstdio>
#include <cstdlib>

#include "brisk_slab_layout.h"

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    SlabLayout LY;
    for (char* p = argv[a]; *p;) {
      char* end = nullptr;
      const unsigned long long bytes = std::strtoull(p, &end, 10);
      if (end == p || (*end && *end != ',')) return 2;
      std::printf("%zu ", LY.add((size_t)bytes));
      p = *end ? end + 1 : end;
    }
    std::printf("%zu\n", LY.bytes());
  }
  return 0;
}

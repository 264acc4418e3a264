// Host build of the guided pair matchers' rule (ethzasl_brisk_amd/csrc/brisk_match_guide.h - the functions the kernels of
// brisk_match.hip call) for tests/test_abi_match_guided.py.  Reads records of 128 bytes, little endian, from the file argv[1]:
//   h[9] (double)  hypothesis flags (int)  dx_min dx_max dy_min dy_max (float) max_octave_diff (int)  fallback (int)
//   Q.x Q.y (float) Q.octave (int)  T.x T.y (float) T.octave (int)
// and prints one line per record: the bit patterns of the centre's cx and cy (hex), has-centre (0 / 1), M (0 / 1).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "brisk_match_guide.h"

struct Record {
  double h[9];
  int hypothesis, flags;
  float dx_min, dx_max, dy_min, dy_max;
  int max_octave_diff, fallback;
  float qx, qy;
  int qoct;
  float tx, ty;
  int toct;
};
static_assert(sizeof(Record) == 128, "record layout");

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<Record> recs;  // (an allocation of exactly the records read)
  Record r;
  while (std::fread(&r, sizeof(r), 1, f) == 1) recs.push_back(r);
  std::fclose(f);
  for (const Record& c : recs) {
    const BriskMatchGuide g{BriskMatchGate{c.dx_min, c.dx_max, c.dy_min, c.dy_max, c.max_octave_diff}, c.fallback};
    const BriskHomography H{c.h[0], c.h[1], c.h[2], c.h[3], c.h[4], c.h[5], c.h[6], c.h[7], c.h[8]};
    const bool guided = brisk_guide_guided(c.hypothesis, c.flags);
    const BriskGuideCentre ce = brisk_guide_centre(guided, c.fallback, H, c.qx, c.qy);
    uint32_t bx, by;
    std::memcpy(&bx, &ce.x, 4);
    std::memcpy(&by, &ce.y, 4);
    std::printf("%08x %08x %d %d\n", bx, by, ce.has ? 1 : 0, brisk_guide_allows(g, guided, H, c.qx, c.qy, c.qoct, c.tx, c.ty, c.toct) ? 1 : 0);
  }
  return 0;
}

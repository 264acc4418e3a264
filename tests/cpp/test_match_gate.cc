// Host build of the gated pair matchers' predicate (ethzasl_brisk_amd/csrc/brisk_match_gate.h - the function the kernels of
// brisk_match.hip call) for tests/test_abi_match_gated.py.  Reads records of 11 little-endian 32-bit words from the file argv[1]:
//   dx_min dx_max dy_min dy_max (float)  max_octave_diff (int)  Q.x Q.y (float) Q.octave (int)  T.x T.y (float) T.octave (int)
// and prints one character per record: '1' the pair may match, '0' it may not.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "brisk_match_gate.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint32_t> w;
  uint32_t rec[11];
  while (std::fread(rec, sizeof(rec), 1, f) == 1) w.insert(w.end(), rec, rec + 11);
  std::fclose(f);
  for (size_t i = 0; i + 11 <= w.size(); i += 11) {
    float fl[11];
    int in[11];
    std::memcpy(fl, &w[i], sizeof(fl));
    std::memcpy(in, &w[i], sizeof(in));
    const BriskMatchGate g{fl[0], fl[1], fl[2], fl[3], in[4]};
    std::putchar(brisk_gate_allows(g, fl[5], fl[6], in[7], fl[8], fl[9], in[10]) ? '1' : '0');
  }
  std::putchar('\n');
  return 0;
}

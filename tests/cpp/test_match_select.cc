// Host build of the selection rule of the pair matchers' exit (ethzasl_brisk_amd/csrc/brisk_match_select.h - the functions the
// kernels of brisk_match_export.hip call) for tests/test_abi_match_export.py.  Reads records of 13 little-endian 32-bit words from
// the file argv[1]:
//   max_distance ratio (float)  keep_per_row per_row count (int)  distance[0 .. 8) (float; the first min(count, per_row) are the row)
// and prints one character per record: the number of leading entries the rule selects ('0' ... '8').
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "brisk_match_select.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint32_t> w;
  uint32_t rec[13];
  while (std::fread(rec, sizeof(rec), 1, f) == 1) w.insert(w.end(), rec, rec + 13);
  std::fclose(f);
  for (size_t i = 0; i + 13 <= w.size(); i += 13) {
    float fl[13];
    int in[13];
    std::memcpy(fl, &w[i], sizeof(fl));
    std::memcpy(in, &w[i], sizeof(in));
    const BriskMatchSelect s{fl[0], fl[1], in[2]};
    if (in[3] < 1 || in[3] > 8) return 3;
    const int stored = brisk_select_stored(in[4], in[3]);
    const float* d = fl + 5;
    const int n = brisk_select_row(s, stored, [&](int e) { return e < stored ? d[e] : -1.0f; });
    if (n < 0 || n > 8) return 4;
    std::putchar('0' + n);
  }
  std::putchar('\n');
  return 0;
}

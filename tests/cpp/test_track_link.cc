// Host build of the link rule of the feature tracker (ethzasl_brisk_amd/csrc/brisk_track_link.h - the functions the kernels of
// brisk_track.hip call) for tests/test_abi_tracks.py.  Reads little-endian 32-bit words from the file argv[1], case after case:
//   lim_query lim_train n   then n records of 4 words: queryIdx trainIdx imgIdx distance-bits   (the list of ONE pair)
// and prints one line per record: '-' for a record the rule ignores, else the proposal's 64-bit key as 16 hex digits and the row
// the key names as a forward pointer.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "brisk_track_link.h"

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint32_t> w;
  uint32_t word;
  while (std::fread(&word, sizeof(word), 1, f) == 1) w.push_back(word);
  std::fclose(f);
  size_t at = 0;
  while (at < w.size()) {
    if (at + 3 > w.size()) return 3;
    int head[3];
    std::memcpy(head, &w[at], sizeof(head));
    at += 3;
    const int lim_q = brisk_track_lim(head[0], 0x7FFFFFFF), lim_t = brisk_track_lim(head[1], 0x7FFFFFFF), n = head[2];
    if (n < 0 || at + 4 * (size_t)n > w.size()) return 3;
    std::vector<int> rec(4 * (size_t)n + 1);
    std::memcpy(rec.data(), w.data() + at, 4 * (size_t)n * sizeof(int));
    for (int j = 0; j < n; ++j) {
      const int q = rec[4 * (size_t)j], t = rec[4 * (size_t)j + 1];
      const unsigned bits = (unsigned)rec[4 * (size_t)j + 3];
      const bool first = brisk_track_first_of_row(j, 0, q, j > 0 ? rec[4 * (size_t)(j - 1)] : 0);
      if (!brisk_track_proposes(first, q, t, bits, lim_q, lim_t)) {
        std::puts("-");
        continue;
      }
      const unsigned long long key = brisk_track_key(bits, q);
      if (!brisk_track_wins(key, key) || key == BRISK_TRACK_NO_CLAIM) return 4;
      std::printf("%016llx %d\n", key, brisk_track_next_row(key));
    }
    at += 4 * (size_t)n;
  }
  if (brisk_track_next_row(BRISK_TRACK_NO_CLAIM) != -1) return 4;
  return 0;
}

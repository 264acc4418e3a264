// Host build of the mutual guided pair matchers' rule (ethzasl_brisk_amd/csrc/brisk_match_guide.h and brisk_match_epiline.h - the
// functions the kernels of brisk_match.hip call) for tests/test_abi_match_mutual.py.  Three modes, argv[1]:
//   centre FILE   the 128-byte records of tests/cpp/test_match_guide.cc: per record "F B" - the forward predicate brisk_guide_allows and
//                 the backward one, brisk_guide_train_row on what brisk_guide_centre makes of the query keypoint (0 / 1 each)
//   line FILE     the 136-byte records of tests/cpp/test_match_epiline.cc: the same with brisk_epiguide_allows and
//                 brisk_epiguide_train_row on what brisk_epiguide_lane makes of the query keypoint
//   pairs FILE    whole pairs, matched here with plain loops over the header functions.  Per pair, little endian:
//                   form (0 centre, 1 line) n_a n_b rows_cap words32 hypothesis flags fallback max_octave_diff (int)
//                   dx_min dx_max dy_min dy_max band (float)  model[9] (double)
//                   n_a query keypoints, n_b train keypoints (x y float, octave int)
//                   n_a query descriptors, n_b train descriptors (words32 u32 each)
//                 and prints "pair N ROWS" and per row q < ROWS "q t d kept": the forward match (t = -1: none) and whether the
//                 backward scan over ALL n_a rows gives q back.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "brisk_match_epiline.h"
#include "brisk_match_guide.h"

struct GuideRecord {
  double h[9];
  int hypothesis, flags;
  float dx_min, dx_max, dy_min, dy_max;
  int max_octave_diff, fallback;
  float qx, qy;
  int qoct;
  float tx, ty;
  int toct;
};
static_assert(sizeof(GuideRecord) == 128, "record layout");
struct LineRecord {
  double f[9];
  int hypothesis, flags;
  float dx_min, dx_max, dy_min, dy_max;
  int max_octave_diff;
  float band;
  int fallback;
  float qx, qy;
  int qoct;
  float tx, ty;
  int toct;
  int pad;
};
static_assert(sizeof(LineRecord) == 136, "record layout");

struct PairHeader {
  int form, n_a, n_b, rows_cap, words32, hypothesis, flags, fallback, max_octave_diff;
  float dx_min, dx_max, dy_min, dy_max, band;
  double model[9];
};
static_assert(sizeof(PairHeader) == 128, "pair header layout");
struct Kp {
  float x, y;
  int octave;
};

template <class R>
static std::vector<R> read_all(const char* path) {
  std::vector<R> recs;
  FILE* f = std::fopen(path, "rb");
  if (!f) return recs;
  R r;
  while (std::fread(&r, sizeof(r), 1, f) == 1) recs.push_back(r);
  std::fclose(f);
  return recs;
}

static int run_centre(const char* path) {
  for (const GuideRecord& c : read_all<GuideRecord>(path)) {
    const BriskMatchGuide g{BriskMatchGate{c.dx_min, c.dx_max, c.dy_min, c.dy_max, c.max_octave_diff}, c.fallback};
    const BriskHomography H{c.h[0], c.h[1], c.h[2], c.h[3], c.h[4], c.h[5], c.h[6], c.h[7], c.h[8]};
    const bool guided = brisk_guide_guided(c.hypothesis, c.flags);
    const BriskGuideCentre ce = brisk_guide_centre(guided, c.fallback, H, c.qx, c.qy);
    const BriskGateLane tl = brisk_gate_lane(g.window, c.tx, c.ty, c.toct);
    std::printf("%d %d\n", brisk_guide_allows(g, guided, H, c.qx, c.qy, c.qoct, c.tx, c.ty, c.toct) ? 1 : 0,
                brisk_guide_train_row(g.window, tl, ce.has, ce.x, ce.y, c.qoct) ? 1 : 0);
  }
  return 0;
}

static int run_line(const char* path) {
  for (const LineRecord& c : read_all<LineRecord>(path)) {
    const BriskMatchEpiGuide g{BriskMatchGate{c.dx_min, c.dx_max, c.dy_min, c.dy_max, c.max_octave_diff}, c.band, c.fallback};
    const BriskFundamental F{c.f[0], c.f[1], c.f[2], c.f[3], c.f[4], c.f[5], c.f[6], c.f[7], c.f[8]};
    const bool guided = brisk_guide_guided(c.hypothesis, c.flags);
    BriskEpiLane L;
    const bool has = brisk_epiguide_lane(g, guided, F, c.qx, c.qy, c.qoct, L);
    const BriskGateLane tl = brisk_gate_lane(g.window, c.tx, c.ty, c.toct);
    std::printf("%d %d\n", brisk_epiguide_allows(g, guided, F, c.qx, c.qy, c.qoct, c.tx, c.ty, c.toct) ? 1 : 0,
                brisk_epiguide_train_row(g.window, guided, tl, has, L.line, c.qx, c.qy, c.qoct) ? 1 : 0);
  }
  return 0;
}

static unsigned hamming(const uint32_t* a, const uint32_t* b, int words32) {
  unsigned d = 0;
  for (int w = 0; w < words32; ++w) d += (unsigned)__builtin_popcount(a[w] ^ b[w]);
  return d;
}

static int run_pairs(const char* path) {
  FILE* f = std::fopen(path, "rb");
  if (!f) return 2;
  PairHeader h;
  for (int pair = 0; std::fread(&h, sizeof(h), 1, f) == 1; ++pair) {
    if (h.n_a < 0 || h.n_b < 0 || h.words32 < 1 || h.rows_cap < 1) return 3;
    std::vector<Kp> kq(h.n_a), kt(h.n_b);
    std::vector<uint32_t> dq((size_t)h.n_a * h.words32), dt((size_t)h.n_b * h.words32);
    if (std::fread(kq.data(), sizeof(Kp), kq.size(), f) != kq.size() || std::fread(kt.data(), sizeof(Kp), kt.size(), f) != kt.size() ||
        std::fread(dq.data(), 4, dq.size(), f) != dq.size() || std::fread(dt.data(), 4, dt.size(), f) != dt.size())
      return 3;
    const BriskMatchGate window{h.dx_min, h.dx_max, h.dy_min, h.dy_max, h.max_octave_diff};
    const BriskMatchGuide gc{window, h.fallback};
    const BriskMatchEpiGuide gl{window, h.band, h.fallback};
    const BriskHomography H{h.model[0], h.model[1], h.model[2], h.model[3], h.model[4], h.model[5], h.model[6], h.model[7], h.model[8]};
    const BriskFundamental F{h.model[0], h.model[1], h.model[2], h.model[3], h.model[4], h.model[5], h.model[6], h.model[7], h.model[8]};
    const bool guided = brisk_guide_guided(h.hypothesis, h.flags);
    const int rows = h.n_a < h.rows_cap ? h.n_a : h.rows_cap;
    std::printf("pair %d %d\n", pair, rows);
    for (int q = 0; q < rows; ++q) {
      // forward: the allowed train row of smallest (distance, t)
      int ft = -1;
      unsigned fd = 0;
      for (int t = 0; t < h.n_b; ++t) {
        const bool ok = h.form ? brisk_epiguide_allows(gl, guided, F, kq[q].x, kq[q].y, kq[q].octave, kt[t].x, kt[t].y, kt[t].octave)
                               : brisk_guide_allows(gc, guided, H, kq[q].x, kq[q].y, kq[q].octave, kt[t].x, kt[t].y, kt[t].octave);
        if (!ok) continue;
        const unsigned d = hamming(&dq[(size_t)q * h.words32], &dt[(size_t)t * h.words32], h.words32);
        if (ft < 0 || d < fd) ft = t, fd = d;
      }
      // backward: among ALL rows of frame a, the one of smallest (distance, q') that the mask - asked from the train side - allows
      int bq = -1;
      if (ft >= 0) {
        const BriskGateLane tl = brisk_gate_lane(window, kt[ft].x, kt[ft].y, kt[ft].octave);
        unsigned bd = 0;
        for (int r = 0; r < h.n_a; ++r) {
          bool ok;
          if (h.form) {
            BriskEpiLane L;
            const bool has = brisk_epiguide_lane(gl, guided, F, kq[r].x, kq[r].y, kq[r].octave, L);
            ok = brisk_epiguide_train_row(window, guided, tl, has, L.line, kq[r].x, kq[r].y, kq[r].octave);
          } else {
            const BriskGuideCentre ce = brisk_guide_centre(guided, h.fallback, H, kq[r].x, kq[r].y);
            ok = brisk_guide_train_row(window, tl, ce.has, ce.x, ce.y, kq[r].octave);
          }
          if (!ok) continue;
          const unsigned d = hamming(&dq[(size_t)r * h.words32], &dt[(size_t)ft * h.words32], h.words32);
          if (bq < 0 || d < bd) bq = r, bd = d;
        }
      }
      std::printf("%d %d %u %d\n", q, ft, ft >= 0 ? fd : 0u, ft >= 0 && bq == q ? 1 : 0);
    }
  }
  std::fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  if (!std::strcmp(argv[1], "centre")) return run_centre(argv[2]);
  if (!std::strcmp(argv[1], "line")) return run_line(argv[2]);
  if (!std::strcmp(argv[1], "pairs")) return run_pairs(argv[2]);
  return 2;
}

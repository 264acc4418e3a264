// Host build of the epipolar verification rule (ethzasl_brisk_amd/csrc/brisk_pair_epipolar.h - the functions k_epipolar_ransac
// calls) for tests/test_abi_epipolar.py.  Reads the input format of tests/cpp/test_pair_verify.cc - little-endian 32-bit words from
// the file argv[1], pair after pair:
//   seed p hypotheses min_inliers keep_unverified max_error-bits lim_a lim_b m
//   lim_a x {x-bits y-bits}   the query frame's keypoints      lim_b x {x-bits y-bits}   the train frame's
//   m records of 4 words: queryIdx trainIdx imgIdx distance-bits
// (the keypoint arrays hold exactly lim rows: a read for an unusable record is a read outside them) and prints, per hypothesis,
//   h <h> <valid> <i0> .. <i7> <free column> <inliers> <F0 .. F8 as 16 hex digits each>
// (indices -1 when m < 8; the free column is -1 and F zeros unless the hypothesis is valid), then per pair
//   w <winner or -1> <its inliers> <accepted> <valid hypotheses> <usable records>
//   k <one keep byte per record, as 0 / 1>
//   m <the reported model: nine times 16 hex digits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "brisk_pair_epipolar.h"

static unsigned long long bits_of(double v) {
  unsigned long long b;
  std::memcpy(&b, &v, sizeof(b));
  return b;
}
static float float_of(uint32_t w) {
  float f;
  std::memcpy(&f, &w, sizeof(f));
  return f;
}

struct Pair {
  int lim_a, lim_b, m;
  std::vector<float> qk, tk;  // x, y per row
  std::vector<int> rec;       // 4 ints per record
  // record j -> its point pair; false = unusable (the keypoints are not touched then)
  bool resolve(int j, BriskVerifyPoints& pt) const {
    const int q = rec[4 * (size_t)j], t = rec[4 * (size_t)j + 1];
    if (!brisk_verify_index_ok(q, t, lim_a, lim_b)) return false;
    const float x = qk.at(2 * (size_t)q), y = qk.at(2 * (size_t)q + 1), xt = tk.at(2 * (size_t)t), yt = tk.at(2 * (size_t)t + 1);
    pt = BriskVerifyPoints{(double)x, (double)y, (double)xt, (double)yt};
    return brisk_verify_coords_ok(x, y, xt, yt);
  }
};

static void print_model(const char* head, const BriskFundamental& F) {
  const double v[9] = {F.f0, F.f1, F.f2, F.f3, F.f4, F.f5, F.f6, F.f7, F.f8};
  std::fputs(head, stdout);
  for (int i = 0; i < 9; ++i) std::printf(" %016llx", bits_of(v[i]));
  std::putchar('\n');
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<uint32_t> w;
  uint32_t word;
  while (std::fread(&word, sizeof(word), 1, f) == 1) w.push_back(word);
  std::fclose(f);
  const BriskFundamental zero{0, 0, 0, 0, 0, 0, 0, 0, 0};
  size_t at = 0;
  while (at < w.size()) {
    if (at + 9 > w.size()) return 3;
    int head[9];
    std::memcpy(head, &w[at], sizeof(head));
    at += 9;
    const unsigned seed = (unsigned)head[0];
    const int p = head[1], hyps = head[2], min_inliers = head[3], keep_unverified = head[4];
    const float max_error = float_of((uint32_t)head[5]);
    Pair P;
    P.lim_a = head[6];
    P.lim_b = head[7];
    P.m = head[8];
    if (P.lim_a < 0 || P.lim_b < 0 || P.m < 0 || hyps < 1 || hyps > BRISK_VERIFY_MAX_HYPOTHESES) return 3;
    const size_t need = 2 * (size_t)P.lim_a + 2 * (size_t)P.lim_b + 4 * (size_t)P.m;
    if (at + need > w.size()) return 3;
    for (int i = 0; i < 2 * P.lim_a; ++i) P.qk.push_back(float_of(w[at++]));
    for (int i = 0; i < 2 * P.lim_b; ++i) P.tk.push_back(float_of(w[at++]));
    P.rec.resize(4 * (size_t)P.m);
    if (P.m) std::memcpy(P.rec.data(), &w[at], 4 * (size_t)P.m * sizeof(int));
    at += 4 * (size_t)P.m;

    const uint32_t pair_seed = brisk_verify_pair_seed(seed, p);
    const bool thr_on = brisk_verify_threshold_on(max_error);
    const double thr2 = brisk_verify_thr2(max_error);
    std::vector<BriskVerifyPoints> pts((size_t)P.m);
    std::vector<char> usable((size_t)P.m);
    int nusable = 0;
    for (int j = 0; j < P.m; ++j) {
      usable[j] = P.resolve(j, pts[j]);
      nusable += usable[j];
    }
    unsigned long long best = 0;
    int nvalid = 0;
    BriskFundamental W = zero;
    for (int h = 0; h < hyps; ++h) {
      int i[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
      BriskFundamental F = zero;
      bool valid = false;
      int free_col = -1;
      if (P.m >= BRISK_EPIPOLAR_MIN_SAMPLE) {
        brisk_epipolar_sample(pair_seed, h, P.m, i);
        bool all = true;
        for (int k = 0; k < 8; ++k) {
          if (i[k] < 0 || i[k] >= P.m) return 4;
          all = all && usable[i[k]];
        }
        if (all) {
          const BriskVerifyPoints s[8] = {pts[i[0]], pts[i[1]], pts[i[2]], pts[i[3]], pts[i[4]], pts[i[5]], pts[i[6]], pts[i[7]]};
          valid = brisk_epipolar_model(s, F, free_col);
        }
      }
      if (!valid) {
        F = zero;
        free_col = -1;
      }
      int count = 0;
      if (valid && thr_on)
        for (int j = 0; j < P.m; ++j) count += usable[j] && brisk_epipolar_inlier(F, thr2, pts[j].x, pts[j].y, pts[j].xt, pts[j].yt);
      const unsigned long long key = brisk_verify_key(valid, count, h);
      if (key > best) {
        best = key;
        W = F;
      }
      nvalid += valid;
      std::printf("h %d %d %d %d %d %d %d %d %d %d %d %d", h, (int)valid, i[0], i[1], i[2], i[3], i[4], i[5], i[6], i[7], free_col, count);
      print_model("", F);
    }
    const bool accepted = brisk_verify_accepted(best, min_inliers);
    const int hwin = brisk_verify_key_hypothesis(best);
    std::printf("w %d %d %d %d %d\n", hwin, brisk_verify_key_count(best), (int)accepted, nvalid, nusable);
    std::string keep = "k ";
    for (int j = 0; j < P.m; ++j) {
      const bool inl = accepted && usable[j] && brisk_epipolar_inlier(W, thr2, pts[j].x, pts[j].y, pts[j].xt, pts[j].yt);
      keep += brisk_verify_keeps(accepted, usable[j], inl, keep_unverified) ? '1' : '0';
    }
    std::puts(keep.c_str());
    print_model("m", hwin >= 0 ? W : zero);
  }
  return 0;
}

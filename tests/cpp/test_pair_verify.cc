// Host build of the verification rule (ethzasl_brisk_amd/csrc/brisk_pair_verify.h - the functions the kernels of
// brisk_pair_verify.hip call) for tests/test_abi_verify.py.  Reads little-endian 32-bit words from the file argv[1], pair after pair:
//   seed p hypotheses min_inliers keep_unverified max_error-bits lim_a lim_b m
//   lim_a x {x-bits y-bits}   the query frame's keypoints      lim_b x {x-bits y-bits}   the train frame's
//   m records of 4 words: queryIdx trainIdx imgIdx distance-bits
// (the keypoint arrays hold exactly lim rows: a read for an unusable record is a read outside them) and prints, per hypothesis,
//   h <h> <valid> <i0> <i1> <i2> <i3> <inliers> <H0 .. H8 as 16 hex digits each>
// (indices -1 when m < 4; H zeros unless all four sampled records are usable), then per pair
//   w <winner or -1> <its inliers> <accepted> <valid hypotheses> <usable records>
//   k <one keep byte per record, as 0 / 1>
//   m <the reported model: nine times 16 hex digits>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "brisk_pair_verify.h"

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

static void print_model(const char* head, const double* v) {
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
    BriskHomography W{0, 0, 0, 0, 0, 0, 0, 0, 0};
    double w_ref = 0;
    for (int h = 0; h < hyps; ++h) {
      int i[4] = {-1, -1, -1, -1};
      BriskHomography H{0, 0, 0, 0, 0, 0, 0, 0, 0};
      bool valid = false;
      double z_ref = 0;
      if (P.m >= BRISK_VERIFY_MIN_SAMPLE) {
        brisk_verify_sample(pair_seed, h, P.m, i[0], i[1], i[2], i[3]);
        for (int k = 0; k < 4; ++k)
          if (i[k] < 0 || i[k] >= P.m) return 4;
        if (usable[i[0]] && usable[i[1]] && usable[i[2]] && usable[i[3]]) {
          valid = brisk_verify_model(pts[i[0]], pts[i[1]], pts[i[2]], pts[i[3]], H);
          z_ref = brisk_verify_z(H, pts[i[0]].x, pts[i[0]].y);
        }
      }
      int count = 0;
      if (valid && thr_on)
        for (int j = 0; j < P.m; ++j)
          count += usable[j] && brisk_verify_inlier(H, z_ref, thr2, pts[j].x, pts[j].y, pts[j].xt, pts[j].yt);
      const unsigned long long key = brisk_verify_key(valid, count, h);
      if (key > best) {
        best = key;
        W = H;
        w_ref = z_ref;
      }
      nvalid += valid;
      std::printf("h %d %d %d %d %d %d %d", h, (int)valid, i[0], i[1], i[2], i[3], count);
      const double v[9] = {H.h0, H.h1, H.h2, H.h3, H.h4, H.h5, H.h6, H.h7, H.h8};
      print_model("", v);
    }
    const bool accepted = brisk_verify_accepted(best, min_inliers);
    const int hwin = brisk_verify_key_hypothesis(best);
    std::printf("w %d %d %d %d %d\n", hwin, brisk_verify_key_count(best), (int)accepted, nvalid, nusable);
    std::string keep = "k ";
    for (int j = 0; j < P.m; ++j) {
      const bool inl = accepted && usable[j] && brisk_verify_inlier(W, w_ref, thr2, pts[j].x, pts[j].y, pts[j].xt, pts[j].yt);
      keep += brisk_verify_keeps(accepted, usable[j], inl, keep_unverified) ? '1' : '0';
    }
    std::puts(keep.c_str());
    double model[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (hwin >= 0) brisk_verify_report(W, model);
    print_model("m", model);
  }
  return 0;
}

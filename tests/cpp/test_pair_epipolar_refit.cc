// Host build of the epipolar refit rule (ethzasl_brisk_amd/csrc/brisk_pair_epipolar_refit.h - the functions k_refit_epipolar of
// brisk_pair_verify.hip calls) for tests/test_abi_epipolar_refit.py.  Reads little-endian 32-bit words from the file argv[1], pair
// after pair:
//   max_error-bits rounds min_inliers keep_unverified rank2 hypothesis flags   18 words: the input model's nine doubles   lim_a lim_b m
//   lim_a x {x-bits y-bits}   the query frame's keypoints      lim_b x {x-bits y-bits}   the train frame's
//   m records of 4 words: queryIdx trainIdx imgIdx distance-bits
// (the keypoint arrays hold exactly lim rows: a read for an unusable record is a read outside them) and prints per pair
//   s <has a model> <n_0>
//   f <round> <fit ok> <n'> <free index> <the fitted model: nine times 16 hex digits>   for every round that is begun, in the rule's
//                                                       literal form (no stop at a fixed point); zeros when the fit fails
//   w <final count> <rounds that replaced> <accepted> <usable records> <flags>
//   k <one keep byte per record, as 0 / 1>
//   m <the output model: nine times 16 hex digits>
// The sums run in the header's order: 256 partials by list index modulo 256, the xor butterfly inside blocks of 64, then the blocks;
// the 44 sums of the normal matrix in the kernel's three sweeps.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "brisk_pair_epipolar_refit.h"

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

static void print_model(const char* head, const double* v) {
  std::fputs(head, stdout);
  for (int i = 0; i < 9; ++i) std::printf(" %016llx", bits_of(v[i]));
  std::putchar('\n');
}

struct Pair {
  int m = 0;
  std::vector<BriskVerifyPoints> pts;
  std::vector<char> usable;
  BriskEpirefitWork work;

  int score(const BriskFundamental& F, double thr2, std::vector<char>& inl) const {
    inl.assign((size_t)m, 0);
    int n = 0;
    for (int j = 0; j < m; ++j) {
      inl[j] = usable[j] && brisk_epipolar_inlier(F, thr2, pts[j].x, pts[j].y, pts[j].xt, pts[j].yt);
      n += inl[j];
    }
    return n;
  }

  // K sums over the inliers in the header's order; term(j, t) fills the K terms of record j
  template <int K, class Term>
  void sums(const std::vector<char>& inl, Term term, double* out) const {
    static double part[BRISK_REFIT_LANES][K], next[BRISK_REFIT_LANES][K];
    for (int l = 0; l < BRISK_REFIT_LANES; ++l)
      for (int i = 0; i < K; ++i) part[l][i] = 0.0;
    for (int j = 0; j < m; ++j) {
      if (!inl[j]) continue;
      double t[K];
      term(j, t);
      for (int i = 0; i < K; ++i) part[j % BRISK_REFIT_LANES][i] = part[j % BRISK_REFIT_LANES][i] + t[i];
    }
    for (int off = 32; off > 0; off >>= 1) {
      for (int l = 0; l < BRISK_REFIT_LANES; ++l)
        for (int i = 0; i < K; ++i) next[l][i] = part[l][i] + part[l ^ off][i];
      std::memcpy(part, next, sizeof(part));
    }
    for (int i = 0; i < K; ++i) out[i] = ((part[0][i] + part[64][i]) + part[128][i]) + part[192][i];
  }

  template <int K0, int CNT>
  void sweep(const std::vector<char>& inl, const BriskRefitNorm& N) {
    sums<CNT>(inl, [&](int j, double (&t)[CNT]) {
      double a[9];
      brisk_epirefit_row(N, pts[j].x, pts[j].y, pts[j].xt, pts[j].yt, a);
      brisk_epirefit_terms<K0, CNT>(a, t);
    }, work.s + K0);
  }

  bool fit(const std::vector<char>& inl, int n, int rank2, BriskFundamental& F, int& free_index) {
    BriskRefitNorm N;
    double s4[4];
    free_index = -1;
    sums<4>(inl, [&](int j, double* t) { t[0] = pts[j].x; t[1] = pts[j].y; t[2] = pts[j].xt; t[3] = pts[j].yt; }, s4);
    brisk_refit_centroids(s4, n, N);
    sums<4>(inl, [&](int j, double* t) { brisk_refit_spread_terms(N, pts[j].x, pts[j].y, pts[j].xt, pts[j].yt, t); }, s4);
    if (!brisk_refit_scales(s4, n, N)) return false;
    sweep<0, BRISK_EPIREFIT_SWEEP>(inl, N);
    sweep<BRISK_EPIREFIT_SWEEP, BRISK_EPIREFIT_SWEEP>(inl, N);
    sweep<2 * BRISK_EPIREFIT_SWEEP, BRISK_EPIREFIT_SUMS - 2 * BRISK_EPIREFIT_SWEEP>(inl, N);
    return brisk_epirefit_fit(n, N, rank2, work, F, free_index);
  }
};

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
    if (at + 28 > w.size()) return 3;
    int head[7];
    std::memcpy(head, &w[at], sizeof(head));
    const float max_error = float_of((uint32_t)head[0]);
    const int rounds = head[1], min_inliers = head[2], keep_unverified = head[3], rank2 = head[4], hypothesis = head[5], flags = head[6];
    double f_in[9];
    std::memcpy(f_in, &w[at + 7], sizeof(f_in));
    int dims[3];
    std::memcpy(dims, &w[at + 25], sizeof(dims));
    at += 28;
    const int lim_a = dims[0], lim_b = dims[1];
    Pair P;
    P.m = dims[2];
    if (lim_a < 0 || lim_b < 0 || P.m < 0 || rounds < 1 || rounds > BRISK_REFIT_MAX_ROUNDS) return 3;
    const size_t need = 2 * (size_t)lim_a + 2 * (size_t)lim_b + 4 * (size_t)P.m;
    if (at + need > w.size()) return 3;
    std::vector<float> qk, tk;
    for (int i = 0; i < 2 * lim_a; ++i) qk.push_back(float_of(w[at++]));
    for (int i = 0; i < 2 * lim_b; ++i) tk.push_back(float_of(w[at++]));
    std::vector<int> rec(4 * (size_t)P.m);
    if (P.m) std::memcpy(rec.data(), &w[at], 4 * (size_t)P.m * sizeof(int));
    at += 4 * (size_t)P.m;

    P.pts.resize((size_t)P.m);
    P.usable.assign((size_t)P.m, 0);
    int nusable = 0;
    for (int j = 0; j < P.m; ++j) {
      const int q = rec[4 * (size_t)j], t = rec[4 * (size_t)j + 1];
      if (!brisk_verify_index_ok(q, t, lim_a, lim_b)) continue;
      const float x = qk.at(2 * (size_t)q), y = qk.at(2 * (size_t)q + 1), xt = tk.at(2 * (size_t)t), yt = tk.at(2 * (size_t)t + 1);
      P.pts[j] = BriskVerifyPoints{(double)x, (double)y, (double)xt, (double)yt};
      P.usable[j] = brisk_verify_coords_ok(x, y, xt, yt);
      nusable += P.usable[j];
    }

    const bool has_model = brisk_refit_has_model(f_in, hypothesis, flags, max_error);
    const double thr2 = brisk_verify_thr2(max_error);
    BriskFundamental F{f_in[0], f_in[1], f_in[2], f_in[3], f_in[4], f_in[5], f_in[6], f_in[7], f_in[8]};
    std::vector<char> S((size_t)P.m, 0), S1;
    int n = 0, replaced = 0;
    if (has_model) n = P.score(F, thr2, S);
    std::printf("s %d %d\n", (int)has_model, n);
    const double zero[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (has_model)
      for (int r = 1; r <= rounds; ++r) {
        if (n < BRISK_EPIPOLAR_MIN_SAMPLE) break;
        BriskFundamental F1{0, 0, 0, 0, 0, 0, 0, 0, 0};
        int free_index = -1;
        const bool ok = P.fit(S, n, rank2, F1, free_index);
        const double v[9] = {F1.f0, F1.f1, F1.f2, F1.f3, F1.f4, F1.f5, F1.f6, F1.f7, F1.f8};
        const int n1 = ok ? P.score(F1, thr2, S1) : 0;
        std::printf("f %d %d %d %d", r, (int)ok, n1, ok ? free_index : -1);
        print_model("", ok ? v : zero);
        if (!ok || !brisk_refit_replaces(n1, n)) break;
        F = F1;
        S = S1;
        n = n1;
        ++replaced;
      }
    const bool accepted = brisk_refit_accepted(has_model, n, min_inliers);
    const int out_flags = (replaced > 0 ? BRISK_REFIT_PAIR_REFIT : 0) | (accepted ? 0 : 0x8);
    std::printf("w %d %d %d %d %d\n", n, replaced, (int)accepted, nusable, out_flags);
    std::string keep = "k ";
    for (int j = 0; j < P.m; ++j) keep += brisk_verify_keeps(accepted, P.usable[j], S[j], keep_unverified) ? '1' : '0';
    std::puts(keep.c_str());
    const double v[9] = {F.f0, F.f1, F.f2, F.f3, F.f4, F.f5, F.f6, F.f7, F.f8};
    print_model("m", has_model ? (replaced > 0 ? v : f_in) : zero);
  }
  return 0;
}

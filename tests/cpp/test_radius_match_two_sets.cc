// The two-set radiusMatch(query, train, matches, maxDistance) of the drop-in brisk::BruteForceMatcher - the form the
// reference's callers use (its live demo and camera test).  Compiling this file is the check that the overload exists
// in the flavour of the class in use; with a GPU it also compares the call with the add() + radiusMatch() form and
// with a host loop over brisk::Hamming.
#include <brisk/brute-force-matcher.h>

#include <cstdio>
#include <exception>
#include <vector>

int main() {
  const int nq = 70, nt = 45, dim = 48;
  std::vector<unsigned char> q(nq * dim), t(nt * dim);
  unsigned s = 12345u;
  auto next = [&s]() { s = s * 1664525u + 1013904223u; return (unsigned char)(((s >> 24) & 3u) * 85u); };  // bytes from {0, 85, 170, 255}
  for (auto& b : q) b = next();
  for (auto& b : t) b = next();
  for (int i = 0; i < dim; ++i) t[5 * dim + i] = q[9 * dim + i];  // one identical row: distance 0
  agast::Mat query(nq, dim, CV_8UC1, q.data()), train(nt, dim, CV_8UC1, t.data());
  const float maxDistance = 4.f * dim;  // the centre of these sets' distances; an integer, so strictness matters
#ifdef BRISK_HAVE_OPENCV
  typedef cv::DMatch Match;
#else
  typedef brisk::DMatch Match;
#endif
  try {
    brisk::BruteForceMatcher matcher;
    std::vector<std::vector<Match> > two, added;
    matcher.radiusMatch(query, train, two, maxDistance);
    brisk::BruteForceMatcher other;
    other.add(std::vector<agast::Mat>(1, train));
    other.radiusMatch(query, added, maxDistance);
    if (two.size() != (size_t)nq || added.size() != (size_t)nq) { std::printf("FAIL rows\n"); return 1; }
    brisk::Hamming hamming;
    size_t total = 0;
    for (int i = 0; i < nq; ++i) {
      std::vector<int> want;
      for (int j = 0; j < nt; ++j)
        if ((float)hamming(&q[i * dim], &t[j * dim], dim) < maxDistance) want.push_back(j);
      if (two[i].size() != want.size() || added[i].size() != want.size()) { std::printf("FAIL count of row %d\n", i); return 1; }
      for (size_t m = 0; m < two[i].size(); ++m) {
        const Match &a = two[i][m], &b = added[i][m];
        if (a.queryIdx != i || a.imgIdx != 0 || a.trainIdx != b.trainIdx || a.distance != b.distance ||
            a.distance != (float)hamming(&q[i * dim], &t[a.trainIdx * dim], dim) || !(a.distance < maxDistance) ||
            (m > 0 && (two[i][m - 1].distance > a.distance ||
                       (two[i][m - 1].distance == a.distance && two[i][m - 1].trainIdx >= a.trainIdx)))) {
          std::printf("FAIL row %d entry %zu\n", i, m);
          return 1;
        }
      }
      total += want.size();
    }
    if (two[9].empty() || two[9][0].trainIdx != 5 || two[9][0].distance != 0.f) { std::printf("FAIL planted row\n"); return 1; }
    std::printf("two-set radiusMatch OK (%zu matches)\n", total);
    return 0;
  } catch (const std::exception& e) {
    std::printf("%s\n", e.what());
    return 2;
  }
}

// brisk_emul_score_forms.cpp - TEST-ONLY host harness for the packed forms of the detector gate and the 9-of-16 score
// (ethzasl_brisk_amd/csrc/brisk_device_detect.h: brisk_oast9_16_arcs_pk / _M_from_px, brisk_pregate_pair_d,
// brisk_pregate_flags_*).  The forms the library shipped before - window doubling with the centre subtracted per ring pixel,
// the gate's masked result, the shifted-in pass flags - are kept here as reference functions.
// Built into its own library by tests/test_emul_score_forms.py; never linked into or loaded by the product library.
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../../ethzasl_brisk_amd/csrc/brisk_common.h"
#include "../../ethzasl_brisk_amd/csrc/brisk_device_detect.h"

namespace {

struct Rng {
  uint32_t s;
  uint32_t operator()() { s = s * 1664525u + 1013904223u; return s >> 8; }
};

// ---- reference: M by window doubling (2, 4, 8, then the ninth element) on the ring DIFFERENCES
uint32_t ref_ring_pair(uint32_t px_i, uint32_t px_i8, uint32_t centre_both) { return brisk_pk_sub(px_i | (px_i8 << 16), centre_both); }
int ref_M_from_pk(const uint32_t* P) {
  uint32_t lo2[8], hi2[8], lo4[8], hi4[8], lo8[8], hi8[8];
  for (int i = 0; i < 8; ++i) {
    lo2[i] = (i < 7) ? brisk_pk_min(P[i], P[i + 1]) : brisk_pk_min_sw(P[7], P[0]);
    hi2[i] = (i < 7) ? brisk_pk_max(P[i], P[i + 1]) : brisk_pk_max_sw(P[7], P[0]);
  }
  for (int i = 0; i < 8; ++i) {
    lo4[i] = (i < 6) ? brisk_pk_min(lo2[i], lo2[i + 2]) : brisk_pk_min_sw(lo2[i], lo2[i - 6]);
    hi4[i] = (i < 6) ? brisk_pk_max(hi2[i], hi2[i + 2]) : brisk_pk_max_sw(hi2[i], hi2[i - 6]);
  }
  for (int i = 0; i < 8; ++i) {
    lo8[i] = (i < 4) ? brisk_pk_min(lo4[i], lo4[i + 4]) : brisk_pk_min_sw(lo4[i], lo4[i - 4]);
    hi8[i] = (i < 4) ? brisk_pk_max(hi4[i], hi4[i + 4]) : brisk_pk_max_sw(hi4[i], hi4[i - 4]);
  }
  uint32_t bb = 0, bd = 0;
  for (int i = 0; i < 8; ++i) {
    const uint32_t lo9 = brisk_pk_min_sw(lo8[i], P[i]), hi9 = brisk_pk_max_sw(hi8[i], P[i]);
    bb = (i == 0) ? lo9 : brisk_pk_max(bb, lo9);
    bd = (i == 0) ? hi9 : brisk_pk_min(bd, hi9);
  }
  const int best_bright = brisk_max((int)(int16_t)(bb & 0xFFFFu), (int)(int16_t)(bb >> 16));
  const int best_dark = brisk_min((int)(int16_t)(bd & 0xFFFFu), (int)(int16_t)(bd >> 16));
  return brisk_max(best_bright, -best_dark);
}

// one ring (16 pixel values, centre c): 0 if the new forms (pixels + centre, and differences) equal the doubling form and
// the scalar brisk_oast9_16_M_from_d
int ring_mismatch(const int* ring, int c) {
  uint32_t Pd[8], Q[8];
  int d[16];
  const uint32_t cc = (uint32_t)c * 0x10001u;
  for (int i = 0; i < 16; ++i) d[i] = ring[i] - c;
  for (int i = 0; i < 8; ++i) {
    Pd[i] = ref_ring_pair((uint32_t)ring[i], (uint32_t)ring[i + 8], cc);
    Q[i] = brisk_pk_ring_pair((uint32_t)ring[i], (uint32_t)ring[i + 8]);
  }
  const int ref = ref_M_from_pk(Pd);
  return (brisk_oast9_16_M_from_px(Q, c) != ref) || (brisk_oast9_16_M_from_pk(Pd) != ref) || (brisk_oast9_16_M_from_d(d) != ref);
}

// ---- reference: the gate as shipped (its own copy of the constants, the result masked to the two flag bits)
struct RefPregate { uint32_t K, shift, lower; };
RefPregate ref_pregate_make(int thr, int lower_threshold = BRISK_LOWER_THRESHOLD) {
  int s = 8;
  while (s > 0 && 230 * ((thr << s) / 100) > 65535) --s;
  const uint32_t K = (uint32_t)((thr << s) / 100);
  RefPregate g;
  g.K = K | (K << 16);
  g.shift = (uint32_t)s | ((uint32_t)s << 16);
  g.lower = (uint32_t)lower_threshold * 0x10001u;
  return g;
}
uint32_t ref_pregate_pair(uint32_t c, uint32_t n, uint32_t s, uint32_t w, uint32_t e, const RefPregate& g) {
  const uint32_t mxNS = brisk_pk_max(n, s), mnNS = brisk_pk_min(n, s);
  const uint32_t mxWE = brisk_pk_max(w, e), mnWE = brisk_pk_min(w, e);
  const uint32_t vb = brisk_pk_min(mxNS, mxWE);
  const uint32_t vd = brisk_pk_max(mnNS, mnWE);
  const uint32_t t5 = brisk_pk_sub(brisk_pk_max(mxNS, mxWE), brisk_pk_min(mnNS, mnWE));
  const uint32_t upper = (uint32_t)BRISK_UPPER_THRESHOLD * 0x10001u;
  const uint32_t tc = brisk_pk_min(brisk_pk_max(t5, g.lower), upper);
  const uint32_t b2p = brisk_pk_shr(brisk_pk_mul(tc, g.K), g.shift);
  const uint32_t ev = brisk_pk_max(brisk_pk_sub(vb, c), brisk_pk_sub(c, vd));
  return brisk_pk_sub(b2p, ev) & 0x80008000u;
}

// the gate's difference b2' - ev of one pixel in wide integers
long gate_difference_wide(int c, int n, int s, int w, int e, int K, int sh) {
  const int mxNS = brisk_max(n, s), mnNS = brisk_min(n, s), mxWE = brisk_max(w, e), mnWE = brisk_min(w, e);
  const int vb = brisk_min(mxNS, mxWE), vd = brisk_max(mnNS, mnWE);
  const int t5 = brisk_max(mxNS, mxWE) - brisk_min(mnNS, mnWE);
  const int tc = brisk_min(brisk_max(t5, BRISK_LOWER_THRESHOLD), BRISK_UPPER_THRESHOLD);
  const int ev = brisk_max(vb - c, c - vd);
  return (((long)tc * K) >> sh) - (long)ev;
}

// one pixel's five values: random, extreme (0 / 255 and their neighbours), or around a centre
void draw_compass(Rng& rnd, int* v /* c n s w e */) {
  static const int ext[6] = {0, 1, 2, 253, 254, 255};
  const unsigned mode = rnd() % 4;
  const int base = (int)(rnd() % 256), spread = 1 + (int)(rnd() % 64);
  for (int k = 0; k < 5; ++k) {
    int x = mode == 0 ? (int)(rnd() % 256) : mode == 1 ? ext[rnd() % 6] : mode == 2 ? base + (int)(rnd() % (2 * spread + 1)) - spread
            : ((rnd() & 1) ? ext[rnd() % 6] : (int)(rnd() % 256));
    v[k] = brisk_min(brisk_max(x, 0), 255);
  }
}

}  // namespace

extern "C" {

// ---- M: new forms against the doubling form ----
// random rings (uniform, plateaus with outliers, two-level runs); returns mismatches
int sf_M_random_mismatches(unsigned seed, int n) {
  Rng rnd = {seed};
  int bad = 0;
  for (int it = 0; it < n; ++it) {
    int ring[16];
    const unsigned mode = rnd() % 4;
    const int c = (int)(rnd() % 256);
    const int run = (int)(rnd() % 17), start = (int)(rnd() % 16);
    for (int j = 0; j < 16; ++j)
      ring[j] = mode == 0 ? (int)(rnd() % 256) : mode == 1 ? ((rnd() % 4) ? 200 : (int)(rnd() % 256)) : mode == 2 ? ((rnd() % 4) ? 10 : (int)(rnd() % 256))
                : ((((j - start) & 15) < run) ? 255 : 0);
    bad += ring_mismatch(ring, c);
  }
  return bad;
}
// every ring of {0, 1, 254, 255}^16 whose index is congruent to `phase` modulo `step` (step 1: all 4^16), for the given centre
long sf_M_extreme_mismatches(int c, unsigned step, unsigned phase) {
  static const int lv[4] = {0, 1, 254, 255};
  long bad = 0;
  for (uint64_t code = phase; code < (1ull << 32); code += step) {
    int ring[16];
    for (int j = 0; j < 16; ++j) ring[j] = lv[(code >> (2 * j)) & 3];
    bad += ring_mismatch(ring, c);
  }
  return bad;
}
// every ring of {lo, hi}^16 for the given centre
int sf_M_two_level_mismatches(int c, int lo, int hi) {
  int bad = 0;
  for (unsigned code = 0; code < 65536u; ++code) {
    int ring[16];
    for (int j = 0; j < 16; ++j) ring[j] = ((code >> j) & 1) ? hi : lo;
    bad += ring_mismatch(ring, c);
  }
  return bad;
}
// rings with exactly one 9-arc at the threshold: the arc starting at `start` is c + pol * (b + delta) (b + delta at its
// weakest pixel, more elsewhere), every other pixel breaks the neighbouring arcs; both polarities, every start, delta in
// {-1, 0, 1}.  Checks the forms against each other and M == b + delta.  Returns mismatches.
int sf_M_threshold_mismatches(unsigned seed, int n) {
  Rng rnd = {seed};
  int bad = 0;
  for (int it = 0; it < n; ++it) {
    const int pol = (rnd() & 1) ? 1 : -1;
    const int b = 1 + (int)(rnd() % 120), delta = (int)(rnd() % 3) - 1;
    const int c = pol > 0 ? (int)(rnd() % (255 - b - 1)) : b + 1 + (int)(rnd() % (255 - b - 1));
    const int start = (int)(rnd() % 16), weakest = (int)(rnd() % 9);
    int ring[16];
    for (int j = 0; j < 16; ++j) {
      const int k = (j - start) & 15;
      if (k < 9) {
        const int room = pol > 0 ? 255 - (c + b + delta) : (c - b - delta);
        const int extra = (k == weakest || room <= 0) ? 0 : (int)(rnd() % (unsigned)(room + 1));
        ring[j] = c + pol * (b + delta + extra);
      } else {
        ring[j] = c - pol * (int)(rnd() % (unsigned)(pol > 0 ? c + 1 : 256 - c));  // on the other side of the centre (or equal)
      }
    }
    int d[16];
    for (int j = 0; j < 16; ++j) d[j] = ring[j] - c;
    bad += ring_mismatch(ring, c);
    if (brisk_oast9_16_M_from_d(d) != b + delta) ++bad;
  }
  return bad;
}

// ---- pre-gate ----
// n random / extreme pixel pairs at one threshold.  out[0]: pixels whose difference leaves the signed 16-bit range (wide
// arithmetic), out[1]: pixels whose packed sign bit disagrees with the wide difference's sign, out[2]: pixels the new gate
// passes, out[3]: pixels the old gate passes, out[4]: pixels the old gate passes and the new one does not, out[5]: pixels
// whose new and old flags differ, out[6]: pixels that the exact compass condition of a detection
// (ev > (clamp(t5) * thr) / 100) admits and the new gate drops, out[7]: smallest ev seen
void sf_pregate_random(int thr, unsigned seed, int n, long* out) {
  Rng rnd = {seed ^ (unsigned)thr * 2654435761u};
  const BriskPregate g = brisk_pregate_make(thr);
  const RefPregate r = ref_pregate_make(thr);
  const int K = (int)(g.K & 0xFFFFu), s = (int)(g.shift & 0xFFFFu);
  for (int k = 0; k < 8; ++k) out[k] = 0;
  out[7] = 255;
  for (int it = 0; it < n; ++it) {
    int a[5], b[5];
    draw_compass(rnd, a);
    draw_compass(rnd, b);
    uint32_t p[5];
    for (int k = 0; k < 5; ++k) p[k] = (uint32_t)a[k] | ((uint32_t)b[k] << 16);
    const uint32_t dn = brisk_pregate_pair_d(p[0], p[1], p[2], p[3], p[4], g);
    const uint32_t fn = brisk_pregate_pair(p[0], p[1], p[2], p[3], p[4], g);
    const uint32_t fo = ref_pregate_pair(p[0], p[1], p[2], p[3], p[4], r);
    for (int lane = 0; lane < 2; ++lane) {
      const int* v = lane ? b : a;
      const long D = gate_difference_wide(v[0], v[1], v[2], v[3], v[4], K, s);
      if (D < -32768 || D > 32767) ++out[0];
      const bool pass_new = ((dn >> (16 * lane)) & 0x8000u) != 0, pass_old = ((fo >> (16 * lane)) & 0xFFFFu) != 0;
      if (pass_new != (D < 0) || pass_new != (((fn >> (16 * lane)) & 0xFFFFu) == 0x8000u)) ++out[1];
      out[2] += pass_new;
      out[3] += pass_old;
      if (pass_old && !pass_new) ++out[4];
      if (pass_old != pass_new) ++out[5];
      const int mxNS = brisk_max(v[1], v[2]), mnNS = brisk_min(v[1], v[2]), mxWE = brisk_max(v[3], v[4]), mnWE = brisk_min(v[3], v[4]);
      const int t5 = brisk_max(mxNS, mxWE) - brisk_min(mnNS, mnWE);
      const int ev = brisk_max(brisk_min(mxNS, mxWE) - v[0], v[0] - brisk_max(mnNS, mnWE));
      if (ev > (brisk_min(brisk_max(t5, BRISK_LOWER_THRESHOLD), BRISK_UPPER_THRESHOLD) * thr) / 100 && !pass_new) ++out[6];
      if (ev < out[7]) out[7] = ev;
    }
  }
}
// an image walked as k_detect pairs the pixels.  out[0]: detections (brisk_detect_px) the new gate drops, out[1]: pixels the
// new gate passes, out[2]: pixels the old gate passes, out[3]: pixels whose flags differ, out[4]: pixels walked,
// out[5]: differences outside the signed 16-bit range
void sf_pregate_image(const uint8_t* img, int w, int h, int stride, int thr, long* out) {
  const BriskPregate g = brisk_pregate_make(thr);
  const RefPregate r = ref_pregate_make(thr);
  const int K = (int)(g.K & 0xFFFFu), s = (int)(g.shift & 0xFFFFu);
  for (int k = 0; k < 6; ++k) out[k] = 0;
  auto px = [&](int x, int y) -> uint32_t { return img[(long)y * stride + x]; };
  for (int y = 3; y <= h - 4; ++y)
    for (int x = 3; x <= w - 4; x += 2) {
      const int x1 = (x + 1 <= w - 4) ? x + 1 : x;
      auto pair = [&](int dx, int dy) { return px(x + dx, y + dy) | (px(x1 + dx, y + dy) << 16); };
      const uint32_t dn = brisk_pregate_pair_d(pair(0, 0), pair(0, -3), pair(0, 3), pair(-3, 0), pair(3, 0), g);
      const uint32_t fo = ref_pregate_pair(pair(0, 0), pair(0, -3), pair(0, 3), pair(-3, 0), pair(3, 0), r);
      const int lanes[2] = {x, x1};
      for (int k = 0; k < 2; ++k) {
        if (k == 1 && x1 == x) break;
        const int X = lanes[k];
        const bool pass_new = ((dn >> (16 * k)) & 0x8000u) != 0, pass_old = ((fo >> (16 * k)) & 0xFFFFu) != 0;
        const long D = gate_difference_wide((int)px(X, y), (int)px(X, y - 3), (int)px(X, y + 3), (int)px(X - 3, y), (int)px(X + 3, y), K, s);
        if (D < -32768 || D > 32767) ++out[5];
        out[1] += pass_new;
        out[2] += pass_old;
        out[3] += (pass_new != pass_old);
        ++out[4];
        if (!pass_new && brisk_detect_px(img + (long)y * stride + X, stride, thr)) ++out[0];
      }
    }
}

// ---- pass flags ----
// n random pass patterns of a thread's 4 columns x rows pixels, the bits of the gate's results that carry no meaning random:
// the new collection (brisk_pregate_flags_row / _mask / _decode) and the old one (flags shifted in from the top, its decode)
// must both give back the input set.  Returns mismatches.
int sf_flags_mismatches(unsigned seed, int n, int rows) {
  Rng rnd = {seed};
  int bad = 0;
  for (int it = 0; it < n; ++it) {
    const unsigned density = rnd() % 4;
    bool pass[8][4];
    uint32_t m = 0, mo = 0;
    for (int rr = 0; rr < rows; ++rr) {
      uint32_t d[2];
      for (int q = 0; q < 2; ++q) {
        const uint32_t junk = (rnd() | (rnd() << 24)) & 0x7FFF7FFFu;
        uint32_t f = 0;
        for (int lane = 0; lane < 2; ++lane) {
          const bool p = density == 0 ? false : density == 1 ? (rnd() % 50 == 0) : density == 2 ? (rnd() & 1) : true;
          pass[rr][2 * q + lane] = p;
          if (p) f |= 0x8000u << (16 * lane);
        }
        d[q] = f | junk;
      }
      m = brisk_pregate_flags_row(m, d[0], d[1], rr);
      mo = (mo >> 1) | (d[0] & 0x80008000u);  // (the shipped collection: pair k = 2 rr + q ends at bits 16 - 2 rows + k and 32 - 2 rows + k)
      mo = (mo >> 1) | (d[1] & 0x80008000u);
    }
    m = brisk_pregate_flags_mask(m, rows);
    bool got[8][4], goto_[8][4];
    memset(got, 0, sizeof(got));
    memset(goto_, 0, sizeof(goto_));
    int count = 0;
    for (uint32_t t = m; t; t &= t - 1) {
      int col, row;
      brisk_pregate_flags_decode(__builtin_ctz(t), &col, &row);
      if (col < 0 || col > 3 || row < 0 || row >= rows || got[row][col]) { ++bad; continue; }
      got[row][col] = true;
      ++count;
    }
    for (uint32_t t = mo; t; t &= t - 1) {
      const int bit = __builtin_ctz(t);
      const int k = (bit & 15) - (16 - 2 * rows), half = bit >> 4;
      goto_[k >> 1][((k & 1) << 1) + half] = true;
    }
    for (int rr = 0; rr < rows; ++rr)
      for (int j = 0; j < 4; ++j)
        if (got[rr][j] != pass[rr][j] || goto_[rr][j] != pass[rr][j]) ++bad;
    if (count != __builtin_popcount(m)) ++bad;
  }
  return bad;
}

}  // extern "C"

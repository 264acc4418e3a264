// brisk_emul_tie_list.cpp - TEST-ONLY host harness for the list form of the tie kernel's static replay step
// (ethzasl_brisk_amd/csrc/brisk_device_detect.h: brisk_state_static_list / brisk_tie_slot_static_list) against the unrolled
// form it replaces on short lists (brisk_state_static / brisk_tie_slot_static), on random 9 x 9 windows.
// Built into its own library by tests/test_emul_tie_list.py; never linked into or loaded by the product library.
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

// a random entry that is a candidate: arbitrary D != 0 (small values, values around the "D > 2" test, anything), probe
// count (all 16 codes), status and E5
unsigned draw_candidate(Rng& rnd) {
  const unsigned dsel = rnd() % 4;
  const unsigned D = dsel == 0 ? 1 + rnd() % 2 : dsel == 1 ? 3 + rnd() % 3 : 1 + rnd() % 255;
  return D | ((rnd() % 16) << 8) | ((rnd() % 4) << 12) | ((rnd() % 2) ? BRISK_SM_E5 : 0u);
}

}  // namespace

extern "C" {

int tl_cap() { return BRISK_TIE_LIST_CAP; }

// What the list form would meet on an image's full-resolution layer: hist[k], k = 1 ... 41, = detections (every tie is one)
// whose window has k detections among entries 0 ... 40, itself included.  Returns the number of detections.
int tl_window_histogram(const uint8_t* img, int w, int h, int stride, int thr, long* hist) {
  uint8_t* det = (uint8_t*)calloc((size_t)w * h, 1);
  int n = 0;
  for (int k = 0; k < 42; ++k) hist[k] = 0;
  for (int y = 3; y <= h - 4; ++y)
    for (int x = 3; x <= w - 4; ++x) det[(long)y * w + x] = brisk_detect_px(img + (long)y * stride + x, stride, thr) ? 1 : 0;
  for (int y = 3; y <= h - 4; ++y)
    for (int x = 3; x <= w - 4; ++x) {
      if (!det[(long)y * w + x]) continue;
      int c = 0;
      for (int e = 0; e <= BRISK_TIE_WIN_SELF; ++e) {
        const int qx = x + e % BRISK_TIE_WIN - 4, qy = y + e / BRISK_TIE_WIN - 4;
        if (qx >= 0 && qy >= 0 && qx < w && qy < h) c += det[(long)qy * w + qx];
      }
      ++hist[c];
      ++n;
    }
  free(det);
  return n;
}

// `nwin` random windows; each is compared on all 33 slots x both values of `own` x the three touch geometries, and through
// the slot wrappers.  out[0]: (window, slot, own, geometry) cases whose packed or dynmask differ, out[1]: cases compared,
// out[2]: cases whose result is not final, out[3]: cases with a non-empty dynmask, out[4]: windows with a candidate at
// entry 39, out[5]: windows with entries outside the image, out[6]: windows of a tie in row or column 3 or 4,
// out[8 + k], k = 0 ... 41: windows with k candidates in entries 0 ... 40.
void tl_list_mismatches(unsigned seed, int nwin, long* out) {
  Rng rnd = {seed};
  const int cap = BRISK_TIE_LIST_CAP;
  for (int k = 0; k < 8 + 42; ++k) out[k] = 0;
  for (int it = 0; it < nwin; ++it) {
    BriskLayerView L;
    memset(&L, 0, sizeof(L));
    L.w = 12 + (int)(rnd() % 30);
    L.h = 12 + (int)(rnd() % 30);
    L.stride = L.w;
    // the tie: anywhere a candidate can lie, or in rows / columns 3 and 4 and their mirror images (brisk_border3 and
    // window entries outside the image take part)
    auto coord = [&](int n) {
      const unsigned m = rnd() % 8;
      return m == 0 ? 3 : m == 1 ? 4 : m == 2 ? n - 4 : m == 3 ? n - 5 : 3 + (int)(rnd() % (unsigned)(n - 6));
    };
    const int cx = coord(L.w), cy = coord(L.h);
    if (cx <= 4 || cy <= 4) ++out[6];
    // candidates among entries 0 ... 40, the tie (entry 40) included: 1, 2, ..., around the cap, all 41, or any number
    const unsigned csel = rnd() % 8;
    int want = csel == 0 ? 1 : csel == 1 ? cap : csel == 2 ? cap + 1 : csel == 3 ? 41 : csel == 4 ? 1 + (int)(rnd() % 41)
               : 1 + (int)(rnd() % (unsigned)(cap + 2));
    if (want > 41) want = 41;
    int order[40];
    for (int e = 0; e < 40; ++e) order[e] = e;
    for (int e = 0; e < 40; ++e) {
      const int j = e + (int)(rnd() % (unsigned)(40 - e));
      const int t = order[e]; order[e] = order[j]; order[j] = t;
    }
    if (want > 1 && rnd() % 3 == 0)  // a candidate specifically at entry 39, the tie's left neighbour
      for (int e = 0; e < 40; ++e)
        if (order[e] == 39) { order[e] = order[0]; order[0] = 39; break; }
    bool is_cand[81];
    memset(is_cand, 0, sizeof(is_cand));
    is_cand[40] = true;
    for (int k = 0; k < want - 1; ++k) is_cand[order[k]] = true;
    const unsigned later_density = rnd() % 9;
    const bool zero_outside = rnd() % 4 != 0;  // (the kernel's windows are 0 outside the image; the function is pure: also without)
    uint16_t win[81];
    bool any_outside = false;
    for (int e = 0; e < 81; ++e) {
      const int qx = cx + e % 9 - 4, qy = cy + e / 9 - 4;
      const bool inside = qx >= 0 && qy >= 0 && qx < L.w && qy < L.h;
      any_outside = any_outside || !inside;
      if (e > 40) is_cand[e] = rnd() % 8 < later_density;
      unsigned v = is_cand[e] ? draw_candidate(rnd) : ((rnd() % 16) << 8) | ((rnd() % 4) << 12) | ((rnd() % 2) ? BRISK_SM_E5 : 0u);
      if (rnd() % 4 == 0) v |= BRISK_SM_TOUCH;
      if (!inside && zero_outside) v = 0;
      win[e] = (uint16_t)v;
    }
    unsigned long long list = 0;
    for (int e = 0; e <= 40; ++e)
      if (BRISK_SM_D((unsigned)win[e]) != 0) list |= 1ull << e;
    ++out[8 + __builtin_popcountll(list)];
    if (list & (1ull << 39)) ++out[4];
    if (any_outside) ++out[5];
    uint8_t kp5[25];
    for (int q = 0; q < 25; ++q) kp5[q] = (uint8_t)((rnd() % 3 == 0) ? rnd() % 6 : rnd() % 256);
    for (int geo = 0; geo < 3; ++geo) {
      const bool float_patch = geo > 0, touch2x2 = geo == 2;
      for (int slot = 0; slot < 33; ++slot) {
        int sx, sy;
        bool slot_own;
        brisk_tie_slot_offset(slot, &sx, &sy, &slot_own);
        for (int own = 0; own < 2; ++own) {
          unsigned dyn_ref = 0xDEADBEEFu, dyn = 0xDEADBEEFu;
          const unsigned ref = brisk_state_static(L, float_patch, touch2x2, cx + sx, cy + sy, cx, cy, own != 0, win, cx - 4, cy - 4, 9, kp5, &dyn_ref);
          const unsigned got = brisk_state_static_list(L, float_patch, touch2x2, cx + sx, cy + sy, cx, cy, own != 0, win, kp5, list, 0u, &dyn);
          ++out[1];
          if (ref != got || dyn_ref != dyn) ++out[0];
          if (!(ref & BRISK_SS_FINAL)) ++out[2];
          if (dyn_ref) ++out[3];
        }
        // the kernel's calls: the slot decides `own`, the centre's slot is final
        unsigned dyn_ref = 0xDEADBEEFu, dyn = 0xDEADBEEFu;
        const unsigned ref = brisk_tie_slot_static(L, float_patch, touch2x2, cx, cy, slot, win, cx - 4, cy - 4, 9, kp5, &dyn_ref);
        const unsigned got = brisk_tie_slot_static_list(L, float_patch, touch2x2, cx, cy, slot, win, kp5, list, 0u, &dyn);
        ++out[1];
        if (ref != got || dyn_ref != dyn) ++out[0];
      }
      {  // a lane without a slot: final, no open events
        unsigned dyn = 0xDEADBEEFu;
        if (brisk_tie_slot_static_list(L, float_patch, touch2x2, cx, cy, -1, win, kp5, list, 0u, &dyn) != BRISK_SS_FINAL || dyn != 0) ++out[0];
      }
    }
  }
}

}  // extern "C"

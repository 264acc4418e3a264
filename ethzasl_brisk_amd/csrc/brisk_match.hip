// brisk_match.hip - Hamming brute-force matcher kernels (the step after the detect + describe path).
//
// Replaces brisk::BruteForceMatcher::commonKnnMatchImpl / commonRadiusMatchImpl
// (brisk/src/brute-force-matcher.cc:80-213) with brisk::Hamming (brisk/include/brisk/internal/hamming.h:98-112)
// as the distance: popcount of a ^ b over size / 16 128-bit words.  Integer work, HBM/L2-bound, no MFMA:
//   k_match_dist    u16 distance matrix of a block of queries against all train descriptors (all train images
//                   concatenated in image order); 0xFFFF = the reference's INT_MAX (masked pair)
//   k_match_knn     one wave per query: k rounds of "first minimum" selection, as the reference does
//   k_match_radius  one wave per query: distance histogram in LDS, then stable placement by (distance, image,
//                   train index)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "brisk_kernels.h"

#define MT_THREADS 256
#define MT_QTILE 32
#define MT_MAXWORDS_LONG 28  // descriptors up to 224 bytes (generateKernel at small pattern scales); BRISK's own are 48 and 64 (8 x u64)

// grid: (ceil(nt / 256), ceil(nqb / MT_QTILE)); thread = one train descriptor, loop over the query tile in LDS
template <int MT_MAXWORDS>
__global__ void __launch_bounds__(MT_THREADS) k_match_dist(const uint8_t* __restrict__ query, int q_pitch, int q0, int nqb,
                                                           const uint8_t* __restrict__ train, int t_pitch, int nt,
                                                           int words /* u64 per descriptor */,
                                                           const uint8_t* __restrict__ mask, long mask_pitch,
                                                           uint16_t* __restrict__ dist, long dist_pitch) {
  __shared__ unsigned long long qs[MT_QTILE][MT_MAXWORDS];
  const int t = blockIdx.x * MT_THREADS + threadIdx.x;
  const int qt0 = blockIdx.y * MT_QTILE;
  for (int i = threadIdx.x; i < MT_QTILE * words; i += MT_THREADS) {
    const int q = i / words, w = i % words;
    unsigned long long v = 0;
    if (qt0 + q < nqb) {
      const uint8_t* p = query + (long)(q0 + qt0 + q) * q_pitch + w * 8;
      for (int b = 0; b < 8; ++b) v |= (unsigned long long)p[b] << (8 * b);  // (no alignment assumption on the rows)
    }
    qs[q][w] = v;
  }
  __syncthreads();
  if (t >= nt) return;
  unsigned long long tv[MT_MAXWORDS];
#pragma unroll
  for (int w = 0; w < MT_MAXWORDS; ++w) {
    tv[w] = 0;
    if (w < words) {
      const uint8_t* p = train + (long)t * t_pitch + w * 8;
      unsigned long long v = 0;
      for (int b = 0; b < 8; ++b) v |= (unsigned long long)p[b] << (8 * b);
      tv[w] = v;
    }
  }
  const int nq = min(MT_QTILE, nqb - qt0);
  for (int q = 0; q < nq; ++q) {
    int d = 0;
#pragma unroll
    for (int w = 0; w < MT_MAXWORDS; ++w)
      if (w < words) d += __popcll(tv[w] ^ qs[q][w]);
    if (mask && mask[(long)(q0 + qt0 + q) * mask_pitch + t] == 0) d = 0xFFFF;
    dist[(long)(qt0 + q) * dist_pitch + t] = (uint16_t)d;
  }
}

// masked-out queries (OpenCV DescriptorMatcher::isMaskedOut: `outCount == masks.size()`): EVERY image has a non-empty
// mask whose row for this query is all zero - the query can match nothing anywhere.
// grid: nqb blocks of 64 threads; img_start[nimg + 1] are the offsets of the images in the concatenated train set,
// has_mask[i] != 0 if image i has a mask.
__global__ void __launch_bounds__(64) k_match_masked_out(const uint8_t* __restrict__ mask, long mask_pitch, int q0,
                                                         const int* __restrict__ img_start, const int* __restrict__ has_mask,
                                                         int nimg, int* __restrict__ masked) {
  const int q = blockIdx.x, lane = threadIdx.x;
  int out = nimg > 0 ? 1 : 0;
  for (int i = 0; i < nimg && out; ++i) {
    if (!has_mask[i]) { out = 0; break; }  // no mask, or no train descriptors (an empty cv::Mat): not counted
    bool any = false;
    for (int t = img_start[i] + lane; t < img_start[i + 1]; t += 64) any |= mask[(long)(q0 + q) * mask_pitch + t] != 0;
    if (__any(any)) out = 0;
  }
  if (lane == 0) masked[q] = out;
}

// (img_start == nullptr: a single train image [0, nt))
__device__ __forceinline__ int mt_image_of(const int* img_start, int nimg, int t) {
  if (!img_start) return 0;
  int i = 0;
  while (i + 1 < nimg && t >= img_start[i + 1]) ++i;
  return i;
}

// one wave per query; out row = (q0 + q) * k
__global__ void __launch_bounds__(64) k_match_knn(const uint16_t* __restrict__ dist, long dist_pitch, int q0, int nt,
                                                  const int* __restrict__ img_start, int nimg, const int* __restrict__ masked,
                                                  int k, BriskDMatch* __restrict__ out, int* __restrict__ out_count) {
  const int q = blockIdx.x, lane = threadIdx.x;
  const uint16_t* row = dist + (long)q * dist_pitch;
  BriskDMatch* orow = out + (long)(q0 + q) * k;
  if (masked && masked[q]) {
    if (lane == 0) out_count[q0 + q] = 0;
    return;
  }
  int last_nonempty = -1;
  if (!img_start) last_nonempty = nt > 0 ? 0 : -1;
  else
    for (int i = 0; i < nimg; ++i)
      if (img_start[i + 1] > img_start[i]) last_nonempty = i;
  int count = 0;
  unsigned long long last = 0;
  bool have_last = false;
  for (int kk = 0; kk < k; ++kk) {
    // first minimum over (distance, concatenated index) = the reference's minMaxLoc per image + strict '<' across
    // images.  The reference overwrites a selected entry with INT_MAX; selections come in strictly increasing
    // (distance, index) order, so "the smallest key above the previous selection" is the same thing without a write.
    unsigned long long best = ~0ull;
    for (int t = lane; t < nt; t += 64) {
      const unsigned long long key = ((unsigned long long)row[t] << 32) | (unsigned)t;
      if ((!have_last || key > last) && key < best) best = key;
    }
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long o = __shfl_xor(best, off, 64);
      best = o < best ? o : best;
    }
    const unsigned d = (unsigned)(best >> 32);
    if (nt == 0 || d >= 0xFFFFu) break;  // nothing real left
    const int t = (int)(best & 0xFFFFFFFFu);
    if (lane == 0) {
      const int img = mt_image_of(img_start, nimg, t);
      BriskDMatch m;
      m.queryIdx = q0 + q; m.trainIdx = t - (img_start ? img_start[img] : 0); m.imgIdx = img; m.distance = (float)d;
      orow[count] = m;
    }
    last = best;
    have_last = true;
    ++count;
  }
  // reference quirk (brute-force-matcher.cc:139-153): with every entry at INT_MAX the comparison
  // `minVal < bestMatch.distance` still succeeds (2147483647.0 < FLT_MAX, and again against float(INT_MAX) =
  // 2147483648), so the remaining k - count slots are filled with {train 0 of the LAST non-empty image, 2147483648.f}
  if (last_nonempty >= 0 && lane == 0) {
    for (int c = count; c < k; ++c) {
      BriskDMatch m;
      m.queryIdx = q0 + q; m.trainIdx = 0; m.imgIdx = last_nonempty; m.distance = 2147483648.0f;
      orow[c] = m;
    }
  }
  if (last_nonempty >= 0) count = k;
  if (lane == 0) out_count[q0 + q] = count;
}

// one wave per query.  out row = (q0 + q) * cap, at most cap matches are stored, out_count = matches found.
#define MR_BINS 1793  // distances 0 ... 8 x 224 bytes (BRISK's own descriptors: 0 ... 512; the prefix below only walks the first 513 bins then)
__global__ void __launch_bounds__(64) k_match_radius(const uint16_t* __restrict__ dist, long dist_pitch, int q0, int nt,
                                                     const int* __restrict__ img_start, int nimg,
                                                     const int* __restrict__ masked, float max_distance, int cap,
                                                     BriskDMatch* __restrict__ out, int* __restrict__ out_count, int nbins) {
  __shared__ int bins[MR_BINS + 1];
  const int q = blockIdx.x, lane = threadIdx.x;
  const uint16_t* row = dist + (long)q * dist_pitch;
  BriskDMatch* orow = out + (long)(q0 + q) * cap;
  if (masked && masked[q]) {
    if (lane == 0) out_count[q0 + q] = 0;
    return;
  }
  for (int b = lane; b <= nbins; b += 64) bins[b] = 0;
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  for (int t = lane; t < nt; t += 64) {
    const unsigned d = row[t];
    if (d != 0xFFFFu && (float)d < max_distance) atomicAdd(&bins[d], 1);
  }
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  if (lane == 0) {  // exclusive prefix over the nbins (513 for a 64-byte descriptor) distance values
    int acc = 0;
    for (int b = 0; b < nbins; ++b) { const int c = bins[b]; bins[b] = acc; acc += c; }
    bins[nbins] = acc;
  }
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  const int total = bins[nbins];
  // stable placement: chunks of 64 train entries in order; inside a chunk equal distances keep lane order
  for (int t0 = 0; t0 < nt; t0 += 64) {
    const int t = t0 + lane;
    unsigned d = 0xFFFFu;
    if (t < nt) d = row[t];
    const bool hit = d != 0xFFFFu && (float)d < max_distance;
    unsigned long long todo = __ballot(hit);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const unsigned dsel = __shfl(d, leader, 64);
      const unsigned long long same = __ballot(hit && d == dsel);
      const int base = bins[dsel];
      if (hit && d == dsel) {
        const int pos = base + __popcll(same & ((1ull << lane) - 1ull));
        if (pos < cap) {
          const int img = mt_image_of(img_start, nimg, t);
          BriskDMatch m;
          m.queryIdx = q0 + q; m.trainIdx = t - (img_start ? img_start[img] : 0); m.imgIdx = img; m.distance = (float)d;
          orow[pos] = m;
        }
      }
      __builtin_amdgcn_wave_barrier();
      if (lane == leader) bins[dsel] = base + __popcll(same);
      __builtin_amdgcn_s_waitcnt(0);
      __builtin_amdgcn_wave_barrier();
      todo &= ~same;
    }
  }
  if (lane == 0) out_count[q0 + q] = total;
}

// ------------------------------------------------------------------------------------------------
// Fused k-NN for k <= 2, one train set, no masks (the frame-to-frame / frame-to-map case): no distance matrix.
// Workgroup = 64 queries (one per lane, descriptor in registers) x MF_WAVES waves; wave w scans the w-th slice of
// the train set, whose descriptors are wave-uniform (scalar loads, XOR against SGPRs); per pair 2 x W32 VALU
// (v_xor + v_bcnt with accumulate) and a 3-instruction top-2 update on packed keys (distance << 22 | train
// index).  The MF_WAVES partial top-2 lists of a query are merged through LDS.
// ------------------------------------------------------------------------------------------------
#define MF_WAVES 16
#define MF_IDX_BITS 22
template <int W32>
__global__ void __launch_bounds__(MF_WAVES * 64) k_match_knn_fused(const uint8_t* __restrict__ query, int q_pitch, int nq,
                                                                    const uint8_t* __restrict__ train, int t_pitch, int nt,
                                                                    int k, BriskDMatch* __restrict__ out,
                                                                    int* __restrict__ out_count) {
  __shared__ unsigned part[MF_WAVES][2][64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int q = blockIdx.x * 64 + lane;
  unsigned qv[W32];
  {
    const uint8_t* p = query + (long)min(q, nq - 1) * q_pitch;
#pragma unroll
    for (int w = 0; w < W32; ++w)  // (byte loads: no alignment assumption on caller rows)
      qv[w] = (unsigned)p[4 * w] | ((unsigned)p[4 * w + 1] << 8) | ((unsigned)p[4 * w + 2] << 16) | ((unsigned)p[4 * w + 3] << 24);
  }
  const int per = (nt + MF_WAVES - 1) / MF_WAVES;
  const int t0 = __builtin_amdgcn_readfirstlane(wave * per), t1 = min(nt, t0 + per);
  unsigned b1 = 0xFFFFFFFFu, b2 = 0xFFFFFFFFu;
  const bool aligned = (((uintptr_t)train | (unsigned)t_pitch) & 3) == 0;
  if (aligned) {
    for (int t = t0; t < t1; ++t) {
      const unsigned* tp = reinterpret_cast<const unsigned*>(train + (long)t * t_pitch);  // wave-uniform address
      unsigned d = 0;
#pragma unroll
      for (int w = 0; w < W32; ++w) d += __popc(qv[w] ^ tp[w]);
      const unsigned key = (d << MF_IDX_BITS) | (unsigned)t;
      b2 = min(b2, max(b1, key));
      b1 = min(b1, key);
    }
  } else {
    for (int t = t0; t < t1; ++t) {
      const uint8_t* tp = train + (long)t * t_pitch;
      unsigned d = 0;
#pragma unroll
      for (int w = 0; w < W32; ++w) {
        const unsigned tv = (unsigned)tp[4 * w] | ((unsigned)tp[4 * w + 1] << 8) | ((unsigned)tp[4 * w + 2] << 16) | ((unsigned)tp[4 * w + 3] << 24);
        d += __popc(qv[w] ^ tv);
      }
      const unsigned key = (d << MF_IDX_BITS) | (unsigned)t;
      b2 = min(b2, max(b1, key));
      b1 = min(b1, key);
    }
  }
  part[wave][0][lane] = b1;
  part[wave][1][lane] = b2;
  __syncthreads();
  if (wave == 0 && q < nq) {
    unsigned m1 = 0xFFFFFFFFu, m2 = 0xFFFFFFFFu;
#pragma unroll
    for (int w = 0; w < MF_WAVES; ++w)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const unsigned key = part[w][i][lane];
        m2 = min(m2, max(m1, key));
        m1 = min(m1, key);
      }
    BriskDMatch* orow = out + (long)q * k;
    BriskDMatch m;
    m.queryIdx = q; m.imgIdx = 0;
    m.trainIdx = (int)(m1 & ((1u << MF_IDX_BITS) - 1)); m.distance = (float)(m1 >> MF_IDX_BITS);
    orow[0] = m;
    if (k > 1) {
      m.trainIdx = (int)(m2 & ((1u << MF_IDX_BITS) - 1)); m.distance = (float)(m2 >> MF_IDX_BITS);
      orow[1] = m;
    }
    out_count[q] = k;
  }
}

// returns false when the case is not covered (the caller uses the distance-matrix path)
bool brisk_launch_match_knn_fused(const uint8_t* query, int q_pitch, int nq, const uint8_t* train, int t_pitch, int nt,
                                  int words32, int k, BriskDMatch* out, int* out_count, hipStream_t s) {
  if (k < 1 || k > 2 || nt < k || nt >= (1 << MF_IDX_BITS) || nq <= 0) return false;
  const dim3 grid((nq + 63) / 64), block(MF_WAVES * 64);
  switch (words32) {
    case 4: hipLaunchKernelGGL(k_match_knn_fused<4>, grid, block, 0, s, query, q_pitch, nq, train, t_pitch, nt, k, out, out_count); break;
    case 8: hipLaunchKernelGGL(k_match_knn_fused<8>, grid, block, 0, s, query, q_pitch, nq, train, t_pitch, nt, k, out, out_count); break;
    case 12: hipLaunchKernelGGL(k_match_knn_fused<12>, grid, block, 0, s, query, q_pitch, nq, train, t_pitch, nt, k, out, out_count); break;
    case 16: hipLaunchKernelGGL(k_match_knn_fused<16>, grid, block, 0, s, query, q_pitch, nq, train, t_pitch, nt, k, out, out_count); break;
    default: return false;
  }
  return true;
}

// ------------------------------------------------------------------------------------------------
// The frame pairs of a batch in one launch (brisk_hip_match_knn_pairs_device): k_match_knn_fused's scheme - 64 queries per
// workgroup, one per lane with the descriptor in registers, MP_WAVES (8) waves each scanning a slice of the train rows through
// wave-uniform loads, packed keys, merge through LDS - with everything a pair needs resolved on the device: grid
// (ceil(rows_cap / 64), pairs); the workgroup finds its pair (arithmetic form or the caller's list), reads the two row
// counts from the sets' count arrays and leaves at once when its 64 rows lie beyond min(n_a, rows_cap).
// CROSS (k == 1): the forward match t of row q is kept only if the best match of row t of frame b among ALL rows of frame
// a is q.  Fused: once the forward keys are merged, lane q takes row t of frame b into its registers and the waves scan
// frame a the same way (top-1) - the same work as a role-swapped launch, without a scratch buffer of backward keys and
// without any hand-off between workgroups.
// ------------------------------------------------------------------------------------------------
#ifndef MP_WAVES
// waves of a workgroup = slices of the train rows.  8, not k_match_knn_fused's 16: a CU holds ONE workgroup of 16 waves (71 VGPRs
// with the 32-key merge unrolled: 7 waves per SIMD) but four of 8 (39 VGPRs), and with several resident the prologue (pair and
// count look-ups, the query row) and the LDS merge of one are covered by the scans of the others (measured both)
#define MP_WAVES 8
#endif
template <int W32>
__device__ __forceinline__ void mp_load_row(const uint8_t* p, bool aligned, unsigned (&v)[W32]) {
  if (aligned) {
    const unsigned* p32 = reinterpret_cast<const unsigned*>(p);
#pragma unroll
    for (int w = 0; w < W32; ++w) v[w] = p32[w];
  } else {
#pragma unroll
    for (int w = 0; w < W32; ++w)
      v[w] = (unsigned)p[4 * w] | ((unsigned)p[4 * w + 1] << 8) | ((unsigned)p[4 * w + 2] << 16) | ((unsigned)p[4 * w + 3] << 24);
  }
}
// rows [t0, t1) of one frame (wave-uniform addresses) against the lane's descriptor: the two smallest keys
template <int W32>
__device__ __forceinline__ void mp_scan(const unsigned (&qv)[W32], const uint8_t* rows, int pitch, bool aligned, int t0, int t1,
                                        unsigned& b1, unsigned& b2) {
  if (aligned) {  // (batch results: 4-byte aligned rows at pitch 64)
    for (int t = t0; t < t1; ++t) {
      const unsigned* tp = reinterpret_cast<const unsigned*>(rows + (long)t * pitch);
      unsigned d = 0;
#pragma unroll
      for (int w = 0; w < W32; ++w) d += __popc(qv[w] ^ tp[w]);
      const unsigned key = (d << MF_IDX_BITS) | (unsigned)t;
      b2 = min(b2, max(b1, key));
      b1 = min(b1, key);
    }
  } else {  // (a caller's set whose base, frame pitch or row pitch is not)
    for (int t = t0; t < t1; ++t) {
      const uint8_t* tp = rows + (long)t * pitch;
      unsigned d = 0;
#pragma unroll
      for (int w = 0; w < W32; ++w) {
        const unsigned tv = (unsigned)tp[4 * w] | ((unsigned)tp[4 * w + 1] << 8) | ((unsigned)tp[4 * w + 2] << 16) | ((unsigned)tp[4 * w + 3] << 24);
        d += __popc(qv[w] ^ tv);
      }
      const unsigned key = (d << MF_IDX_BITS) | (unsigned)t;
      b2 = min(b2, max(b1, key));
      b1 = min(b1, key);
    }
  }
}

template <int W32, bool CROSS>
__global__ void __launch_bounds__(MP_WAVES * 64) k_match_knn_pairs(const BriskDescSet Q, const BriskDescSet T, const BriskPairSpec P,
                                                                    int pair0, int k, int rows_cap, BriskDMatch* __restrict__ out,
                                                                    int* __restrict__ out_count, int* __restrict__ pair_rows) {
  __shared__ unsigned part[MP_WAVES][2][64];
  __shared__ unsigned fwd[64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int p = pair0 + blockIdx.y;
  int a, b;
  if (P.pairs) {
    a = P.pairs[2 * (long)p];
    b = P.pairs[2 * (long)p + 1];
  } else {
    a = P.query_first + p * P.query_step;
    b = P.train_first + p * P.train_step;
  }
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  if (a < 0 || a >= Q.frames || b < 0 || b >= T.frames) {  // (a bad entry of the caller's list; the arithmetic form is checked on the host)
    if (first) pair_rows[p] = -1;
    return;
  }
  const int n_a = max(0, Q.counts[(long)a * Q.count_stride]), n_b = max(0, T.counts[(long)b * T.count_stride]);
  if (n_b >= (1 << MF_IDX_BITS) || (CROSS && n_a >= (1 << MF_IDX_BITS))) {  // (the keys hold 22 index bits)
    if (first) pair_rows[p] = -1;
    return;
  }
  if (first) pair_rows[p] = n_a;
  const int rows = min(n_a, rows_cap);
  if ((int)blockIdx.x * 64 >= rows) return;
  const int q = blockIdx.x * 64 + lane;
  BriskDMatch* orow = out + ((long)p * rows_cap + q) * k;
  int* ocnt = out_count + (long)p * rows_cap + q;
  if (n_b == 0) {  // nothing to match against: empty rows (the reference tops up only when some train image has rows)
    if (wave == 0 && q < rows) *ocnt = 0;
    return;
  }
  const uint8_t* qrows = Q.desc + (long)a * Q.frame_pitch;
  const uint8_t* trows = T.desc + (long)b * T.frame_pitch;
  const bool q_aligned = (((uintptr_t)Q.desc | (unsigned long)Q.frame_pitch | (unsigned)Q.row_pitch) & 3) == 0;
  const bool t_aligned = (((uintptr_t)T.desc | (unsigned long)T.frame_pitch | (unsigned)T.row_pitch) & 3) == 0;
  unsigned qv[W32];
  mp_load_row<W32>(qrows + (long)min(q, rows - 1) * Q.row_pitch, q_aligned, qv);
  unsigned b1 = 0xFFFFFFFFu, b2 = 0xFFFFFFFFu;
  {
    const int per = (n_b + MP_WAVES - 1) / MP_WAVES;
    const int t0 = __builtin_amdgcn_readfirstlane(wave * per), t1 = min(n_b, t0 + per);
    mp_scan<W32>(qv, trows, T.row_pitch, t_aligned, t0, t1, b1, b2);
  }
  part[wave][0][lane] = b1;
  part[wave][1][lane] = b2;
  __syncthreads();
  unsigned m1 = 0xFFFFFFFFu, m2 = 0xFFFFFFFFu;
  if (wave == 0) {
#pragma unroll
    for (int w = 0; w < MP_WAVES; ++w)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const unsigned key = part[w][i][lane];
        m2 = min(m2, max(m1, key));
        m1 = min(m1, key);
      }
  }
  bool keep = true;
  if (CROSS) {
    if (wave == 0) fwd[lane] = m1;
    __syncthreads();  // (also: wave 0 has read part[] before anybody writes it again)
    const int t = (int)(fwd[lane] & ((1u << MF_IDX_BITS) - 1));  // (n_b >= 1: every lane has a real forward match)
    unsigned tv[W32];
    mp_load_row<W32>(trows + (long)t * T.row_pitch, t_aligned, tv);
    unsigned c1 = 0xFFFFFFFFu, c2 = 0xFFFFFFFFu;
    const int per = (n_a + MP_WAVES - 1) / MP_WAVES;
    const int r0 = __builtin_amdgcn_readfirstlane(wave * per), r1 = min(n_a, r0 + per);
    mp_scan<W32>(tv, qrows, Q.row_pitch, q_aligned, r0, r1, c1, c2);  // ALL rows of frame a, also those beyond rows_cap
    part[wave][0][lane] = c1;
    __syncthreads();
    if (wave == 0) {
      unsigned best = 0xFFFFFFFFu;
#pragma unroll
      for (int w = 0; w < MP_WAVES; ++w) best = min(best, part[w][0][lane]);
      keep = (int)(best & ((1u << MF_IDX_BITS) - 1)) == q;
    }
  }
  if (wave == 0 && q < rows) {
    if (!keep) {
      *ocnt = 0;
      return;
    }
    BriskDMatch m;
    m.queryIdx = q; m.imgIdx = b;
    m.trainIdx = (int)(m1 & ((1u << MF_IDX_BITS) - 1)); m.distance = (float)(m1 >> MF_IDX_BITS);
    orow[0] = m;
    if (k > 1) {
      if (m2 != 0xFFFFFFFFu) {
        m.trainIdx = (int)(m2 & ((1u << MF_IDX_BITS) - 1)); m.distance = (float)(m2 >> MF_IDX_BITS);
      } else {  // n_b < k: the reference's top-up entry (k_match_knn above; brute-force-matcher.cc:139-153)
        m.trainIdx = 0; m.distance = 2147483648.0f;
      }
      orow[1] = m;
    }
    *ocnt = k;
  }
}

template <int W32>
static void mp_launch(const BriskDescSet& Q, const BriskDescSet& T, const BriskPairSpec& P, int k, bool cross, int rows_cap,
                      BriskDMatch* out, int* out_count, int* pair_rows, hipStream_t s) {
  const dim3 block(MP_WAVES * 64);
  for (int p0 = 0; p0 < P.npairs; p0 += 65535) {  // (grid.y holds 65535)
    const dim3 grid((rows_cap + 63) / 64, min(65535, P.npairs - p0));
    if (cross)
      hipLaunchKernelGGL((k_match_knn_pairs<W32, true>), grid, block, 0, s, Q, T, P, p0, k, rows_cap, out, out_count, pair_rows);
    else
      hipLaunchKernelGGL((k_match_knn_pairs<W32, false>), grid, block, 0, s, Q, T, P, p0, k, rows_cap, out, out_count, pair_rows);
  }
}
// false: descriptor size not covered (16, 32, 48, 64 bytes are)
bool brisk_launch_match_knn_pairs(const BriskDescSet& Q, const BriskDescSet& T, const BriskPairSpec& P, int words32, int k, bool cross,
                                  int rows_cap, BriskDMatch* out, int* out_count, int* pair_rows, hipStream_t s) {
  switch (words32) {
    case 4: mp_launch<4>(Q, T, P, k, cross, rows_cap, out, out_count, pair_rows, s); break;
    case 8: mp_launch<8>(Q, T, P, k, cross, rows_cap, out, out_count, pair_rows, s); break;
    case 12: mp_launch<12>(Q, T, P, k, cross, rows_cap, out, out_count, pair_rows, s); break;
    case 16: mp_launch<16>(Q, T, P, k, cross, rows_cap, out, out_count, pair_rows, s); break;
    default: return false;
  }
  return true;
}

// ------------------------------------------------------------------------------------------------
// Radius matching in k_match_knn_pairs' shape (brisk_hip_match_radius_pairs_device / brisk_hip_match_radius_device): 64 queries
// per workgroup, one per lane with the descriptor in registers, MP_WAVES waves each scanning a slice of the train rows through
// wave-uniform loads.  No distance matrix: a hit ((float)d < max_distance, brute-force-matcher.cc:203-207) bumps its query's
// counter in LDS and, while the query's short LDS list has room, drops its packed key (d << 22 | t) there.  Keys are unique per
// train row, so the order of collection does not matter:
//   sparse rows (count <= MRP_LIST): MP_WAVES threads per query rank the keys of the list against each other and store those
//       of rank < cap at their rank - (distance, trainIdx) order;
//   dense rows (the list overflowed): one wave per such query runs k_match_radius' algorithm with the distances recomputed on
//       the fly (lane = train row, the query wave-uniform): histogram over the distances below the threshold, exclusive prefix,
//       stable placement in train order.  Second phase of the same workgroup: nothing between the phases leaves the CU.
// The counter holds the number FOUND in both cases.
// ------------------------------------------------------------------------------------------------
#ifndef MRP_LIST
#define MRP_LIST 32  // keys per query held in LDS (8 KiB per workgroup); a row with more hits takes the dense path
#endif
#define MRP_BINS 513                    // distances 0 ... 512 (descriptors of at most 64 bytes)
#define MRP_PER ((MRP_BINS + 63) / 64)  // bins per lane in the prefix

template <int W32, bool ALIGNED>
__device__ __forceinline__ unsigned mrp_dist(const unsigned (&qv)[W32], const uint8_t* tp) {
  unsigned d = 0;
  if (ALIGNED) {
    const unsigned* tp32 = reinterpret_cast<const unsigned*>(tp);
#pragma unroll
    for (int w = 0; w < W32; ++w) d += __popc(qv[w] ^ tp32[w]);
  } else {
#pragma unroll
    for (int w = 0; w < W32; ++w) {
      const unsigned tv = (unsigned)tp[4 * w] | ((unsigned)tp[4 * w + 1] << 8) | ((unsigned)tp[4 * w + 2] << 16) | ((unsigned)tp[4 * w + 3] << 24);
      d += __popc(qv[w] ^ tv);
    }
  }
  return d;
}
// rows [t0, t1) of one frame (wave-uniform addresses) against the lane's descriptor: hits (d < thr) into the lane's counter and list
template <int W32, bool ALIGNED>
__device__ __forceinline__ void mrp_scan(const unsigned (&qv)[W32], const uint8_t* rows, int pitch, int t0, int t1, unsigned thr,
                                         int* cnt, unsigned (*list)[64], int lane) {
  for (int t = t0; t < t1; ++t) {
    const unsigned d = mrp_dist<W32, ALIGNED>(qv, rows + (long)t * pitch);
    if (d < thr) {
      const int slot = atomicAdd(&cnt[lane], 1);
      if (slot < MRP_LIST) list[slot][lane] = (d << MF_IDX_BITS) | (unsigned)t;
    }
  }
}
// the gated kernels' view of a pair: the gate and the keypoint records of the two frames, row for row with the descriptors
struct MpGate {
  BriskMatchGate g;
  const char* qk;
  const char* tk;
};
__device__ __forceinline__ const BriskKeyPoint* mp_kp(const char* kps, int r) {
  return reinterpret_cast<const BriskKeyPoint*>(kps + (long)r * (long)sizeof(BriskKeyPoint));
}
// the dense path's distance of train row t (one per lane) to the wave's query; GATE: a row the gate forbids is no hit (thr)
template <int W32, bool ALIGNED, bool GATE>
__device__ __forceinline__ unsigned mrp_dense_dist(const unsigned (&uq)[W32], const uint8_t* trows, int t_pitch, int t, unsigned thr,
                                                   const MpGate& G, const BriskGateLane& QL) {
  if (GATE) {
    const BriskKeyPoint* kp = mp_kp(G.tk, t);
    if (!brisk_gate_query_lane(G.g, QL, kp->x, kp->y, kp->octave)) return thr;
  }
  return mrp_dist<W32, ALIGNED>(uq, trows + (long)t * t_pitch);
}
// one wave, one query with more than MRP_LIST hits.  bins: thr + 1 ints of this wave's own
template <int W32, bool ALIGNED, bool GATE>
__device__ __forceinline__ void mrp_dense(int* bins, const unsigned (&uq)[W32], const uint8_t* trows, int t_pitch, int n_b, unsigned thr,
                                          int cap, int lane, int q, int img, BriskDMatch* __restrict__ orow, const MpGate& G,
                                          const BriskGateLane& QL) {
  for (int b = lane; b <= (int)thr; b += 64) bins[b] = 0;
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  for (int t = lane; t < n_b; t += 64) {
    const unsigned d = mrp_dense_dist<W32, ALIGNED, GATE>(uq, trows, t_pitch, t, thr, G, QL);
    if (d < thr) atomicAdd(&bins[d], 1);
  }
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  {  // exclusive prefix over the thr (<= 513) bins: MRP_PER consecutive bins per lane, a scan of the lane sums in between
    int loc[MRP_PER], sum = 0;
#pragma unroll
    for (int i = 0; i < MRP_PER; ++i) {
      const int b = lane * MRP_PER + i;
      loc[i] = b < (int)thr ? bins[b] : 0;
      sum += loc[i];
    }
    int incl = sum;
    for (int off = 1; off < 64; off <<= 1) {
      const int o = __shfl_up(incl, off, 64);
      if (lane >= off) incl += o;
    }
    int acc = incl - sum;
#pragma unroll
    for (int i = 0; i < MRP_PER; ++i) {
      const int b = lane * MRP_PER + i;
      if (b < (int)thr) bins[b] = acc;
      acc += loc[i];
    }
  }
  __builtin_amdgcn_s_waitcnt(0);
  __builtin_amdgcn_wave_barrier();
  // stable placement (k_match_radius): chunks of 64 train rows in order; inside a chunk equal distances keep lane order.  A bin's
  // base only grows: a hit whose bin has reached cap is never stored and takes no part
  for (int t0 = 0; t0 < n_b; t0 += 64) {
    const int t = t0 + lane;
    unsigned d = thr;
    if (t < n_b) d = mrp_dense_dist<W32, ALIGNED, GATE>(uq, trows, t_pitch, t, thr, G, QL);
    const bool hit = d < thr && bins[d] < cap;
    unsigned long long todo = __ballot(hit);
    while (todo) {
      const int leader = __ffsll((long long)todo) - 1;
      const unsigned dsel = __shfl(d, leader, 64);
      const unsigned long long same = __ballot(hit && d == dsel);
      const int base = bins[dsel];
      if (hit && d == dsel) {
        const int pos = base + __popcll(same & ((1ull << lane) - 1ull));
        if (pos < cap) {
          BriskDMatch m;
          m.queryIdx = q; m.trainIdx = t; m.imgIdx = img; m.distance = (float)d;
          orow[pos] = m;
        }
      }
      __builtin_amdgcn_wave_barrier();
      if (lane == leader) bins[dsel] = base + __popcll(same);
      __builtin_amdgcn_s_waitcnt(0);
      __builtin_amdgcn_wave_barrier();
      todo &= ~same;
    }
  }
}

// The gated scans (k_match_knn_pairs_gated / k_match_radius_pairs_gated).  The keypoint of the wave-uniform row comes through the same
// scalar loads as the row itself, MPG_CHUNK records ahead of the rows they belong to (one wait for the chunk, not one per row); the
// predicate is a handful of VALU compares whose result lives in a lane mask.  A row that NO lane of the wave may match is left
// without its descriptor loads and popcounts: a uniform branch on the mask.  `on`: the lane takes part at all.
// ok[i]: this lane may match row tc + i; live[i]: the lanes of the wave that may.  The ballots are taken for the whole chunk BEFORE
// the first branch (a ballot is not moved below a branch), so the chunk's keypoint loads and compares stay together in front of
// its rows instead of one load and wait in front of each.  (No scheduling barrier between the loads and the compares: with one
// the compiler no longer takes the loop's loads - the descriptor rows included - for scalar loads.)
#define MPG_CHUNK 4
template <bool SWAP>
__device__ __forceinline__ void mpg_allowed(const BriskMatchGate& g, const BriskGateLane& L, bool on, const char* kps, int tc, int t1,
                                            bool (&ok)[MPG_CHUNK], unsigned long long (&live)[MPG_CHUNK]) {
#pragma unroll
  for (int i = 0; i < MPG_CHUNK; ++i) {
    const BriskKeyPoint* kp = mp_kp(kps, min(tc + i, t1 - 1));
    const bool pass = SWAP ? brisk_gate_train_lane(g, L, kp->x, kp->y, kp->octave) : brisk_gate_query_lane(g, L, kp->x, kp->y, kp->octave);
    ok[i] = on && tc + i < t1 && pass;
    live[i] = __ballot(ok[i]);
  }
}
template <int W32, bool ALIGNED>
__device__ __forceinline__ void mrpg_scan(const unsigned (&qv)[W32], const uint8_t* rows, int pitch, int t0, int t1, unsigned thr,
                                          const BriskMatchGate& g, const BriskGateLane& L, bool on, const char* kps, int* cnt,
                                          unsigned (*list)[64], int lane) {
  for (int tc = t0; tc < t1; tc += MPG_CHUNK) {
    bool ok[MPG_CHUNK];
    unsigned long long live[MPG_CHUNK];
    mpg_allowed<false>(g, L, on, kps, tc, t1, ok, live);
#pragma unroll
    for (int i = 0; i < MPG_CHUNK; ++i) {
      if (live[i] == 0) continue;  // wave-uniform
      const int t = tc + i;
      const unsigned d = mrp_dist<W32, ALIGNED>(qv, rows + (long)t * pitch);
      if (ok[i] && d < thr) {
        const int slot = atomicAdd(&cnt[lane], 1);
        if (slot < MRP_LIST) list[slot][lane] = (d << MF_IDX_BITS) | (unsigned)t;
      }
    }
  }
}

// the workgroup's 64 query rows [blockIdx.x * 64, ...) of `rows` against the n_b train rows; out / out_count: row 0 of this query set
template <int W32, bool GATE = false>
__device__ __forceinline__ void mrp_body(const uint8_t* qrows, int q_pitch, bool q_aligned, int rows, const uint8_t* trows, int t_pitch,
                                         bool t_aligned, int n_b, float max_distance, int cap, int img, BriskDMatch* __restrict__ out,
                                         int* __restrict__ out_count, const MpGate& G = MpGate()) {
  __shared__ int cnt[64];
  __shared__ unsigned list[MRP_LIST][64];
  __shared__ int bins[MP_WAVES][MRP_BINS + 3];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int q = blockIdx.x * 64 + lane;
  // d is an integer: (float)d < max_distance <=> d < ceil(max_distance); nothing hits for max_distance <= 0 or NaN, and no
  // distance exceeds 32 * W32
  const unsigned thr = max_distance > 0.f ? (unsigned)fminf(ceilf(max_distance), (float)(32 * W32 + 1)) : 0u;
  if (n_b == 0 || thr == 0) {  // (radius matching has no top-up entry)
    if (wave == 0 && q < rows) out_count[q] = 0;
    return;
  }
  if (wave == 0) cnt[lane] = 0;
  __syncthreads();
  {
    unsigned qv[W32];
    mp_load_row<W32>(qrows + (long)min(q, rows - 1) * q_pitch, q_aligned, qv);
    const unsigned thr_lane = q < rows ? thr : 0u;  // (the lanes behind the last row collect nothing)
    const int per = (n_b + MP_WAVES - 1) / MP_WAVES;
    const int t0 = wave * per, t1 = min(n_b, t0 + per);
    if (GATE) {
      const BriskKeyPoint* kp = mp_kp(G.qk, min(q, rows - 1));
      const BriskGateLane L = brisk_gate_lane(G.g, kp->x, kp->y, kp->octave);
      if (t_aligned) mrpg_scan<W32, true>(qv, trows, t_pitch, t0, t1, thr, G.g, L, q < rows, G.tk, cnt, list, lane);
      else mrpg_scan<W32, false>(qv, trows, t_pitch, t0, t1, thr, G.g, L, q < rows, G.tk, cnt, list, lane);
    } else {
      if (t_aligned) mrp_scan<W32, true>(qv, trows, t_pitch, t0, t1, thr_lane, cnt, list, lane);
      else mrp_scan<W32, false>(qv, trows, t_pitch, t0, t1, thr_lane, cnt, list, lane);
    }
  }
  __syncthreads();
  {  // counts of all rows; sparse rows: MP_WAVES threads per query, each ranks every MP_WAVES-th key of the list
    const int ql = threadIdx.x / MP_WAVES, sub = threadIdx.x % MP_WAVES;
    const int qq = blockIdx.x * 64 + ql;
    if (qq < rows) {
      const int c = cnt[ql];
      if (sub == 0) out_count[qq] = c;
      if (c <= MRP_LIST) {
        BriskDMatch* orow = out + (long)qq * cap;
        for (int j = sub; j < c; j += MP_WAVES) {
          const unsigned key = list[j][ql];
          int rank = 0;
          for (int i = 0; i < c; ++i) rank += list[i][ql] < key ? 1 : 0;
          if (rank < cap) {
            BriskDMatch m;
            m.queryIdx = qq; m.trainIdx = (int)(key & ((1u << MF_IDX_BITS) - 1)); m.imgIdx = img; m.distance = (float)(key >> MF_IDX_BITS);
            orow[rank] = m;
          }
        }
      }
    }
  }
  for (int ql = wave; ql < 64; ql += MP_WAVES) {  // dense rows: one wave each
    const int qq = blockIdx.x * 64 + ql;
    if (qq >= rows) break;
    if (cnt[ql] <= MRP_LIST) continue;
    unsigned uq[W32];
    mp_load_row<W32>(qrows + (long)qq * q_pitch, q_aligned, uq);
    BriskGateLane QL = {};
    if (GATE) {
      const BriskKeyPoint* kp = mp_kp(G.qk, qq);  // (wave-uniform)
      QL = brisk_gate_lane(G.g, kp->x, kp->y, kp->octave);
    }
    if (t_aligned) mrp_dense<W32, true, GATE>(bins[wave], uq, trows, t_pitch, n_b, thr, cap, lane, qq, img, out + (long)qq * cap, G, QL);
    else mrp_dense<W32, false, GATE>(bins[wave], uq, trows, t_pitch, n_b, thr, cap, lane, qq, img, out + (long)qq * cap, G, QL);
  }
}

// grid (ceil(rows_cap / 64), pairs): pair and counts resolved as k_match_knn_pairs does
template <int W32>
__global__ void __launch_bounds__(MP_WAVES * 64) k_match_radius_pairs(const BriskDescSet Q, const BriskDescSet T, const BriskPairSpec P,
                                                                       int pair0, float max_distance, int cap, int rows_cap,
                                                                       BriskDMatch* __restrict__ out, int* __restrict__ out_count,
                                                                       int* __restrict__ pair_rows) {
  const int p = pair0 + blockIdx.y;
  int a, b;
  if (P.pairs) {
    a = P.pairs[2 * (long)p];
    b = P.pairs[2 * (long)p + 1];
  } else {
    a = P.query_first + p * P.query_step;
    b = P.train_first + p * P.train_step;
  }
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  if (a < 0 || a >= Q.frames || b < 0 || b >= T.frames) {  // (a bad entry of the caller's list; the arithmetic form is checked on the host)
    if (first) pair_rows[p] = -1;
    return;
  }
  const int n_a = max(0, Q.counts[(long)a * Q.count_stride]), n_b = max(0, T.counts[(long)b * T.count_stride]);
  if (n_b >= (1 << MF_IDX_BITS)) {  // (the keys hold 22 index bits)
    if (first) pair_rows[p] = -1;
    return;
  }
  if (first) pair_rows[p] = n_a;
  const int rows = min(n_a, rows_cap);
  if ((int)blockIdx.x * 64 >= rows) return;
  const bool q_aligned = (((uintptr_t)Q.desc | (unsigned long)Q.frame_pitch | (unsigned)Q.row_pitch) & 3) == 0;
  const bool t_aligned = (((uintptr_t)T.desc | (unsigned long)T.frame_pitch | (unsigned)T.row_pitch) & 3) == 0;
  mrp_body<W32>(Q.desc + (long)a * Q.frame_pitch, Q.row_pitch, q_aligned, rows, T.desc + (long)b * T.frame_pitch, T.row_pitch, t_aligned,
                n_b, max_distance, cap, b, out + (long)p * rows_cap * cap, out_count + (long)p * rows_cap);
}

// one query set against one train set, counts from the host (brisk_hip_match_radius_device); grid ceil(nq / 64)
template <int W32>
__global__ void __launch_bounds__(MP_WAVES * 64) k_match_radius_pairs_one(const uint8_t* __restrict__ query, int q_pitch, int nq,
                                                                           const uint8_t* __restrict__ train, int t_pitch, int nt,
                                                                           float max_distance, int cap, BriskDMatch* __restrict__ out,
                                                                           int* __restrict__ out_count) {
  const bool q_aligned = (((uintptr_t)query | (unsigned)q_pitch) & 3) == 0, t_aligned = (((uintptr_t)train | (unsigned)t_pitch) & 3) == 0;
  mrp_body<W32>(query, q_pitch, q_aligned, nq, train, t_pitch, t_aligned, nt, max_distance, cap, 0, out, out_count);
}

template <int W32>
static void mrp_launch(const BriskDescSet& Q, const BriskDescSet& T, const BriskPairSpec& P, float max_distance, int cap, int rows_cap,
                       BriskDMatch* out, int* out_count, int* pair_rows, hipStream_t s) {
  const dim3 block(MP_WAVES * 64);
  for (int p0 = 0; p0 < P.npairs; p0 += 65535) {  // (grid.y holds 65535)
    const dim3 grid((rows_cap + 63) / 64, min(65535, P.npairs - p0));
    hipLaunchKernelGGL(k_match_radius_pairs<W32>, grid, block, 0, s, Q, T, P, p0, max_distance, cap, rows_cap, out, out_count, pair_rows);
  }
}
// false: descriptor size not covered (16, 32, 48, 64 bytes are)
bool brisk_launch_match_radius_pairs(const BriskDescSet& Q, const BriskDescSet& T, const BriskPairSpec& P, int words32, float max_distance,
                                     int cap, int rows_cap, BriskDMatch* out, int* out_count, int* pair_rows, hipStream_t s) {
  switch (words32) {
    case 4: mrp_launch<4>(Q, T, P, max_distance, cap, rows_cap, out, out_count, pair_rows, s); break;
    case 8: mrp_launch<8>(Q, T, P, max_distance, cap, rows_cap, out, out_count, pair_rows, s); break;
    case 12: mrp_launch<12>(Q, T, P, max_distance, cap, rows_cap, out, out_count, pair_rows, s); break;
    case 16: mrp_launch<16>(Q, T, P, max_distance, cap, rows_cap, out, out_count, pair_rows, s); break;
    default: return false;
  }
  return true;
}
// false: not covered (descriptor size, nt >= 2^22): the caller uses the distance-matrix path
bool brisk_launch_match_radius_fused(const uint8_t* query, int q_pitch, int nq, const uint8_t* train, int t_pitch, int nt, int words32,
                                     float max_distance, int cap, BriskDMatch* out, int* out_count, hipStream_t s) {
  if (nq <= 0 || nt < 0 || nt >= (1 << MF_IDX_BITS) || cap < 1) return false;
  const dim3 grid((nq + 63) / 64), block(MP_WAVES * 64);
  switch (words32) {
    case 4: hipLaunchKernelGGL(k_match_radius_pairs_one<4>, grid, block, 0, s, query, q_pitch, nq, train, t_pitch, nt, max_distance, cap, out, out_count); break;
    case 8: hipLaunchKernelGGL(k_match_radius_pairs_one<8>, grid, block, 0, s, query, q_pitch, nq, train, t_pitch, nt, max_distance, cap, out, out_count); break;
    case 12: hipLaunchKernelGGL(k_match_radius_pairs_one<12>, grid, block, 0, s, query, q_pitch, nq, train, t_pitch, nt, max_distance, cap, out, out_count); break;
    case 16: hipLaunchKernelGGL(k_match_radius_pairs_one<16>, grid, block, 0, s, query, q_pitch, nq, train, t_pitch, nt, max_distance, cap, out, out_count); break;
    default: return false;
  }
  return true;
}

// ------------------------------------------------------------------------------------------------
// The two pair matchers behind a position gate (brisk_hip_match_knn_pairs_gated_device / brisk_hip_match_radius_pairs_gated_device):
// the mask of a pair is the predicate of brisk_match_gate.h on the two rows' keypoints, evaluated inside the scan (mpg_allowed
// above).  Same grid, same 8-wave workgroups, same LDS, no scratch, no workspace.  k-NN: a lane the gate forbids keeps its key
// 0xFFFFFFFF, so a row holds min(k, allowed rows) REAL matches and is never topped up.  CROSS: the roles swap - the lane holds
// keypoint T of its forward match (a lane without one takes no part), the row passing by is q'.
// ------------------------------------------------------------------------------------------------
// pair, counts and d_pair_rows as k_match_knn_pairs / k_match_radius_pairs resolve them; false: nothing to do for this workgroup
__device__ __forceinline__ bool mpg_resolve(const BriskDescSet& Q, const BriskDescSet& T, const BriskPairSpec& P, int p, bool back_keys,
                                            int rows_cap, int* __restrict__ pair_rows, int& a, int& b, int& n_a, int& n_b, int& rows) {
  if (P.pairs) {
    a = P.pairs[2 * (long)p];
    b = P.pairs[2 * (long)p + 1];
  } else {
    a = P.query_first + p * P.query_step;
    b = P.train_first + p * P.train_step;
  }
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  if (a < 0 || a >= Q.frames || b < 0 || b >= T.frames) {  // (a bad entry of the caller's list; the arithmetic form is checked on the host)
    if (first) pair_rows[p] = -1;
    return false;
  }
  n_a = max(0, Q.counts[(long)a * Q.count_stride]);
  n_b = max(0, T.counts[(long)b * T.count_stride]);
  if (n_b >= (1 << MF_IDX_BITS) || (back_keys && n_a >= (1 << MF_IDX_BITS))) {  // (the keys hold 22 index bits)
    if (first) pair_rows[p] = -1;
    return false;
  }
  if (first) pair_rows[p] = n_a;
  rows = min(n_a, rows_cap);
  return (int)blockIdx.x * 64 < rows;
}

// rows [t0, t1) of one frame against the lane's descriptor, behind the gate: the two smallest keys among the allowed rows
template <int W32, bool ALIGNED, bool SWAP>
__device__ __forceinline__ void mpg_scan(const unsigned (&qv)[W32], const uint8_t* rows, int pitch, int t0, int t1, const BriskMatchGate& g,
                                         const BriskGateLane& L, bool on, const char* kps, unsigned& b1, unsigned& b2) {
  for (int tc = t0; tc < t1; tc += MPG_CHUNK) {
    bool ok[MPG_CHUNK];
    unsigned long long live[MPG_CHUNK];
    mpg_allowed<SWAP>(g, L, on, kps, tc, t1, ok, live);
#pragma unroll
    for (int i = 0; i < MPG_CHUNK; ++i) {
      if (live[i] == 0) continue;  // wave-uniform
      const int t = tc + i;
      const unsigned d = mrp_dist<W32, ALIGNED>(qv, rows + (long)t * pitch);
      const unsigned key = ok[i] ? (d << MF_IDX_BITS) | (unsigned)t : 0xFFFFFFFFu;
      b2 = min(b2, max(b1, key));
      b1 = min(b1, key);
    }
  }
}

template <int W32, bool CROSS>
__global__ void __launch_bounds__(MP_WAVES * 64) k_match_knn_pairs_gated(const BriskDescSet Q, const BriskDescSet T, const BriskKpSet QK,
                                                                          const BriskKpSet TK, const BriskMatchGate gate,
                                                                          const BriskPairSpec P, int pair0, int k, int rows_cap,
                                                                          BriskDMatch* __restrict__ out, int* __restrict__ out_count,
                                                                          int* __restrict__ pair_rows) {
  __shared__ unsigned part[MP_WAVES][2][64];
  __shared__ unsigned fwd[64];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int p = pair0 + blockIdx.y;
  int a, b, n_a, n_b, rows;
  if (!mpg_resolve(Q, T, P, p, CROSS, rows_cap, pair_rows, a, b, n_a, n_b, rows)) return;
  const int q = blockIdx.x * 64 + lane;
  BriskDMatch* orow = out + ((long)p * rows_cap + q) * k;
  int* ocnt = out_count + (long)p * rows_cap + q;
  if (n_b == 0) {
    if (wave == 0 && q < rows) *ocnt = 0;
    return;
  }
  const uint8_t* qrows = Q.desc + (long)a * Q.frame_pitch;
  const uint8_t* trows = T.desc + (long)b * T.frame_pitch;
  const char* qk = QK.kps + (long)a * QK.frame_pitch;
  const char* tk = TK.kps + (long)b * TK.frame_pitch;
  const bool q_aligned = (((uintptr_t)Q.desc | (unsigned long)Q.frame_pitch | (unsigned)Q.row_pitch) & 3) == 0;
  const bool t_aligned = (((uintptr_t)T.desc | (unsigned long)T.frame_pitch | (unsigned)T.row_pitch) & 3) == 0;
  unsigned b1 = 0xFFFFFFFFu, b2 = 0xFFFFFFFFu;
  {
    unsigned qv[W32];
    mp_load_row<W32>(qrows + (long)min(q, rows - 1) * Q.row_pitch, q_aligned, qv);
    const BriskKeyPoint* kp = mp_kp(qk, min(q, rows - 1));
    const BriskGateLane L = brisk_gate_lane(gate, kp->x, kp->y, kp->octave);
    const int per = (n_b + MP_WAVES - 1) / MP_WAVES;
    const int t0 = __builtin_amdgcn_readfirstlane(wave * per), t1 = min(n_b, t0 + per);
    if (t_aligned) mpg_scan<W32, true, false>(qv, trows, T.row_pitch, t0, t1, gate, L, q < rows, tk, b1, b2);
    else mpg_scan<W32, false, false>(qv, trows, T.row_pitch, t0, t1, gate, L, q < rows, tk, b1, b2);
  }
  part[wave][0][lane] = b1;
  part[wave][1][lane] = b2;
  __syncthreads();
  unsigned m1 = 0xFFFFFFFFu, m2 = 0xFFFFFFFFu;
  if (wave == 0) {
#pragma unroll
    for (int w = 0; w < MP_WAVES; ++w)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const unsigned key = part[w][i][lane];
        m2 = min(m2, max(m1, key));
        m1 = min(m1, key);
      }
  }
  bool keep = true;
  if (CROSS) {
    if (wave == 0) fwd[lane] = m1;
    __syncthreads();  // (also: wave 0 has read part[] before anybody writes it again)
    const unsigned f = fwd[lane];
    const bool has = f != 0xFFFFFFFFu;  // (the gate may have left the row without a forward match)
    const int t = has ? (int)(f & ((1u << MF_IDX_BITS) - 1)) : 0;
    unsigned tv[W32];
    mp_load_row<W32>(trows + (long)t * T.row_pitch, t_aligned, tv);
    const BriskKeyPoint* kp = mp_kp(tk, t);
    const BriskGateLane L = brisk_gate_lane(gate, kp->x, kp->y, kp->octave);
    unsigned c1 = 0xFFFFFFFFu, c2 = 0xFFFFFFFFu;
    const int per = (n_a + MP_WAVES - 1) / MP_WAVES;
    const int r0 = __builtin_amdgcn_readfirstlane(wave * per), r1 = min(n_a, r0 + per);
    // ALL rows q' of frame a, also those beyond rows_cap: M[q'][t]
    if (q_aligned) mpg_scan<W32, true, true>(tv, qrows, Q.row_pitch, r0, r1, gate, L, has, qk, c1, c2);
    else mpg_scan<W32, false, true>(tv, qrows, Q.row_pitch, r0, r1, gate, L, has, qk, c1, c2);
    part[wave][0][lane] = c1;
    __syncthreads();
    if (wave == 0) {
      unsigned best = 0xFFFFFFFFu;
#pragma unroll
      for (int w = 0; w < MP_WAVES; ++w) best = min(best, part[w][0][lane]);
      keep = has && (int)(best & ((1u << MF_IDX_BITS) - 1)) == q;
    }
  }
  if (wave == 0 && q < rows) {
    int n = 0;
    if (keep && m1 != 0xFFFFFFFFu) {
      BriskDMatch m;
      m.queryIdx = q; m.imgIdx = b;
      m.trainIdx = (int)(m1 & ((1u << MF_IDX_BITS) - 1)); m.distance = (float)(m1 >> MF_IDX_BITS);
      orow[0] = m;
      n = 1;
      if (k > 1 && m2 != 0xFFFFFFFFu) {  // (no top-up: a second entry only where a second row is allowed)
        m.trainIdx = (int)(m2 & ((1u << MF_IDX_BITS) - 1)); m.distance = (float)(m2 >> MF_IDX_BITS);
        orow[1] = m;
        n = 2;
      }
    }
    *ocnt = n;
  }
}

template <int W32>
__global__ void __launch_bounds__(MP_WAVES * 64) k_match_radius_pairs_gated(const BriskDescSet Q, const BriskDescSet T, const BriskKpSet QK,
                                                                             const BriskKpSet TK, const BriskMatchGate gate,
                                                                             const BriskPairSpec P, int pair0, float max_distance, int cap,
                                                                             int rows_cap, BriskDMatch* __restrict__ out,
                                                                             int* __restrict__ out_count, int* __restrict__ pair_rows) {
  const int p = pair0 + blockIdx.y;
  int a, b, n_a, n_b, rows;
  if (!mpg_resolve(Q, T, P, p, false, rows_cap, pair_rows, a, b, n_a, n_b, rows)) return;
  const bool q_aligned = (((uintptr_t)Q.desc | (unsigned long)Q.frame_pitch | (unsigned)Q.row_pitch) & 3) == 0;
  const bool t_aligned = (((uintptr_t)T.desc | (unsigned long)T.frame_pitch | (unsigned)T.row_pitch) & 3) == 0;
  const MpGate G{gate, QK.kps + (long)a * QK.frame_pitch, TK.kps + (long)b * TK.frame_pitch};
  mrp_body<W32, true>(Q.desc + (long)a * Q.frame_pitch, Q.row_pitch, q_aligned, rows, T.desc + (long)b * T.frame_pitch, T.row_pitch,
                      t_aligned, n_b, max_distance, cap, b, out + (long)p * rows_cap * cap, out_count + (long)p * rows_cap, G);
}

template <int W32>
static void mpg_launch(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK, const BriskMatchGate& gate,
                       const BriskPairSpec& P, int k, bool cross, int rows_cap, BriskDMatch* out, int* out_count, int* pair_rows,
                       hipStream_t s) {
  const dim3 block(MP_WAVES * 64);
  for (int p0 = 0; p0 < P.npairs; p0 += 65535) {  // (grid.y holds 65535)
    const dim3 grid((rows_cap + 63) / 64, min(65535, P.npairs - p0));
    if (cross)
      hipLaunchKernelGGL((k_match_knn_pairs_gated<W32, true>), grid, block, 0, s, Q, T, QK, TK, gate, P, p0, k, rows_cap, out, out_count,
                         pair_rows);
    else
      hipLaunchKernelGGL((k_match_knn_pairs_gated<W32, false>), grid, block, 0, s, Q, T, QK, TK, gate, P, p0, k, rows_cap, out, out_count,
                         pair_rows);
  }
}
// false: descriptor size not covered (16, 32, 48, 64 bytes are)
bool brisk_launch_match_knn_pairs_gated(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK,
                                        const BriskMatchGate& gate, const BriskPairSpec& P, int words32, int k, bool cross, int rows_cap,
                                        BriskDMatch* out, int* out_count, int* pair_rows, hipStream_t s) {
  switch (words32) {
    case 4: mpg_launch<4>(Q, T, QK, TK, gate, P, k, cross, rows_cap, out, out_count, pair_rows, s); break;
    case 8: mpg_launch<8>(Q, T, QK, TK, gate, P, k, cross, rows_cap, out, out_count, pair_rows, s); break;
    case 12: mpg_launch<12>(Q, T, QK, TK, gate, P, k, cross, rows_cap, out, out_count, pair_rows, s); break;
    case 16: mpg_launch<16>(Q, T, QK, TK, gate, P, k, cross, rows_cap, out, out_count, pair_rows, s); break;
    default: return false;
  }
  return true;
}

template <int W32>
static void mrpg_launch(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK, const BriskMatchGate& gate,
                        const BriskPairSpec& P, float max_distance, int cap, int rows_cap, BriskDMatch* out, int* out_count, int* pair_rows,
                        hipStream_t s) {
  const dim3 block(MP_WAVES * 64);
  for (int p0 = 0; p0 < P.npairs; p0 += 65535) {  // (grid.y holds 65535)
    const dim3 grid((rows_cap + 63) / 64, min(65535, P.npairs - p0));
    hipLaunchKernelGGL(k_match_radius_pairs_gated<W32>, grid, block, 0, s, Q, T, QK, TK, gate, P, p0, max_distance, cap, rows_cap, out,
                       out_count, pair_rows);
  }
}
// false: descriptor size not covered (16, 32, 48, 64 bytes are)
bool brisk_launch_match_radius_pairs_gated(const BriskDescSet& Q, const BriskDescSet& T, const BriskKpSet& QK, const BriskKpSet& TK,
                                           const BriskMatchGate& gate, const BriskPairSpec& P, int words32, float max_distance, int cap,
                                           int rows_cap, BriskDMatch* out, int* out_count, int* pair_rows, hipStream_t s) {
  switch (words32) {
    case 4: mrpg_launch<4>(Q, T, QK, TK, gate, P, max_distance, cap, rows_cap, out, out_count, pair_rows, s); break;
    case 8: mrpg_launch<8>(Q, T, QK, TK, gate, P, max_distance, cap, rows_cap, out, out_count, pair_rows, s); break;
    case 12: mrpg_launch<12>(Q, T, QK, TK, gate, P, max_distance, cap, rows_cap, out, out_count, pair_rows, s); break;
    case 16: mrpg_launch<16>(Q, T, QK, TK, gate, P, max_distance, cap, rows_cap, out, out_count, pair_rows, s); break;
    default: return false;
  }
  return true;
}

void brisk_launch_match_dist(const uint8_t* query, int q_pitch, int q0, int nqb, const uint8_t* train, int t_pitch, int nt,
                             int words, const uint8_t* mask, long mask_pitch, uint16_t* dist, long dist_pitch,
                             hipStream_t s) {
  if (nt <= 0 || nqb <= 0) return;
  const dim3 grid((nt + MT_THREADS - 1) / MT_THREADS, (nqb + MT_QTILE - 1) / MT_QTILE);
  if (words <= 8)
    hipLaunchKernelGGL(k_match_dist<8>, grid, dim3(MT_THREADS), 0, s, query, q_pitch, q0, nqb, train, t_pitch, nt, words, mask,
                       mask_pitch, dist, dist_pitch);
  else
    hipLaunchKernelGGL(k_match_dist<MT_MAXWORDS_LONG>, grid, dim3(MT_THREADS), 0, s, query, q_pitch, q0, nqb, train, t_pitch, nt,
                       words, mask, mask_pitch, dist, dist_pitch);
}
void brisk_launch_match_masked_out(const uint8_t* mask, long mask_pitch, int q0, int nqb, const int* img_start,
                                   const int* has_mask, int nimg, int* masked, hipStream_t s) {
  if (nqb <= 0) return;
  hipLaunchKernelGGL(k_match_masked_out, dim3(nqb), dim3(64), 0, s, mask, mask_pitch, q0, img_start, has_mask, nimg, masked);
}
void brisk_launch_match_knn(const uint16_t* dist, long dist_pitch, int q0, int nqb, int nt, const int* img_start, int nimg,
                            const int* masked, int k, BriskDMatch* out, int* out_count, hipStream_t s) {
  if (nqb <= 0) return;
  hipLaunchKernelGGL(k_match_knn, dim3(nqb), dim3(64), 0, s, dist, dist_pitch, q0, nt, img_start, nimg, masked, k, out,
                     out_count);
}
void brisk_launch_match_radius(const uint16_t* dist, long dist_pitch, int q0, int nqb, int nt, const int* img_start,
                               int nimg, const int* masked, float max_distance, int cap, BriskDMatch* out, int* out_count,
                               int dim_bytes, hipStream_t s) {
  if (nqb <= 0) return;
  hipLaunchKernelGGL(k_match_radius, dim3(nqb), dim3(64), 0, s, dist, dist_pitch, q0, nt, img_start, nimg, masked,
                     max_distance, cap, out, out_count, min(dim_bytes * 8 + 1, MR_BINS));
}

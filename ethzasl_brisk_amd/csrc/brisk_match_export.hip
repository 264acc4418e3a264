// brisk_match_export.hip - the pair matchers' exit (brisk_hip_select_pair_matches_device, brisk_hip_pair_matches_download).
//
// The four pair matchers leave padded arrays in HBM: d_out [npairs][rows_cap][per_row] cv::DMatch records, d_out_count
// [npairs][rows_cap], d_pair_rows [npairs].  What a caller takes from them - the reference's callers match under a distance bound
// (brisk/src/test-cameras.cc:131: radiusMatch at 50) - is selected per row by ONE rule (brisk_match_select.h) and packed in
// (pair, query row, rank) order by stable compaction:
//   k_pair_select_count    one lane per row, blockIdx.y = pair: the row's selected count, reduced to one sum per workgroup
//   k_pair_select_offsets  one workgroup: the exclusive prefix sums of the workgroup sums, the pairs' counts / flags / offsets
//                          and the cut at matches_cap (the pattern of k_export_offsets, brisk_export.hip)
//   k_pair_select_scatter  the count pass again, a scan inside the workgroup, the selected records to their places (16-byte
//                          loads and stores)
//   k_pair_select_egress   packed slab -> host memory, the exact bytes only (on the context's egress stream)
#include <hip/hip_runtime.h>

#include "brisk_common.h"
#include "brisk_kernels.h"
#include "brisk_export_copy.h"

#define MX_ROWS 256      // rows = lanes of a workgroup of the count / scatter passes
#define MX_WAVES (MX_ROWS / 64)
#define MX_THREADS 1024  // the offsets workgroup

// the selected count of row `row` = p * rows_cap + q (q below the pair's stored rows) and whether the matcher found more than the row holds
__device__ __forceinline__ int mx_row_count(const BriskDMatch* __restrict__ out, const int* __restrict__ out_count, long long row, int per_row,
                                            const BriskMatchSelect& sel, bool* over) {
  const int c = out_count[row];
  *over = c > per_row;
  const int stored = brisk_select_stored(c, per_row);
  if (stored < 1) return 0;  // (the entries of a row whose count is 0 were never written)
  const float* d = &out[row * per_row].distance;
  return brisk_select_row(sel, stored, [&](int i) { return d[4 * (long long)i]; });
}

__global__ void __launch_bounds__(MX_ROWS) k_pair_select_count(const BriskDMatch* __restrict__ out, const int* __restrict__ out_count,
                                                               const int* __restrict__ pair_rows, int p0, int rows_cap, int per_row,
                                                               BriskMatchSelect sel, long long* __restrict__ blk_sum,
                                                               int* __restrict__ blk_over) {
  __shared__ long long part[MX_WAVES];
  __shared__ int pov[MX_WAVES];
  const int p = p0 + blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long blk = (long long)p * gridDim.x + blockIdx.x;
  const int nrows = min(pair_rows[p], rows_cap);
  if ((int)blockIdx.x * MX_ROWS >= nrows) {  // (rows behind the pair's own are never read)
    if (tid == 0) { blk_sum[blk] = 0; blk_over[blk] = 0; }
    return;
  }
  const int q = blockIdx.x * MX_ROWS + tid;
  bool over = false;
  long long n = q < nrows ? mx_row_count(out, out_count, (long long)p * rows_cap + q, per_row, sel, &over) : 0;
  for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off, 64);
  const bool any_over = __ballot(over) != 0ull;
  if (lane == 0) { part[wave] = n; pov[wave] = any_over; }
  __syncthreads();
  if (tid == 0) {
    long long s = 0;
    int o = 0;
    for (int w = 0; w < MX_WAVES; ++w) { s += part[w]; o |= pov[w]; }
    blk_sum[blk] = s;
    blk_over[blk] = o;
  }
}

// blk[i] (sums of the bpp workgroups of every pair, pair after pair) -> exclusive prefix sums in place; per pair: count, flags,
// offset.  The first pair with matches that does not fit matches_cap and every pair behind it are cut: their counts are reported,
// their offsets stay at the total stored.  rows_copy (may be NULL): d_pair_rows for the host form's slab.
__global__ void __launch_bounds__(MX_THREADS) k_pair_select_offsets(long long* blk, const int* __restrict__ blk_over,
                                                                    const int* __restrict__ pair_rows, int npairs, int bpp, int rows_cap,
                                                                    long long matches_cap, int* __restrict__ counts, int* __restrict__ flags,
                                                                    long long* __restrict__ offsets, int* __restrict__ rows_copy) {
  __shared__ long long part[MX_THREADS / 64];
  __shared__ int red[MX_THREADS / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long long nblk = (long long)npairs * bpp;
  const long long per = (nblk + MX_THREADS - 1) / MX_THREADS;
  const long long i0 = min(tid * per, nblk), i1 = min(i0 + per, nblk);
  long long sum = 0;
  for (long long i = i0; i < i1; ++i) sum += blk[i];
  // exclusive scan of the threads' sums: inside the wave, then over the 16 wave totals
  long long incl = sum;
  for (int off = 1; off < 64; off <<= 1) {
    const long long v = __shfl_up(incl, off, 64);
    if (lane >= off) incl += v;
  }
  if (lane == 63) part[wave] = incl;
  __syncthreads();
  long long base = incl - sum, total = 0;
  for (int w = 0; w < MX_THREADS / 64; ++w) {
    const long long v = part[w];
    base += w < wave ? v : 0;
    total += v;
  }
  for (long long i = i0; i < i1; ++i) {
    const long long v = blk[i];
    blk[i] = base;
    base += v;
  }
  __syncthreads();  // (the offsets of all workgroups are in place: the pairs read them below)
  auto first_of = [&](int p) { return p < npairs ? blk[(long long)p * bpp] : total; };
  // the first pair that does not fit (prefixes grow: every pair with matches behind it does not fit either)
  int cutp = npairs;
  for (int p = tid; p < npairs; p += MX_THREADS) {
    const long long o = first_of(p), c = first_of(p + 1) - o;
    if (c > 0 && o + c > matches_cap) cutp = min(cutp, p);
  }
  for (int off = 32; off > 0; off >>= 1) cutp = min(cutp, __shfl_xor(cutp, off, 64));
  if (lane == 0) red[wave] = cutp;
  __syncthreads();
  for (int w = 0; w < MX_THREADS / 64; ++w) cutp = min(cutp, red[w]);
  const long long stop = first_of(cutp);
  for (int p = tid; p < npairs; p += MX_THREADS) {
    const long long o = first_of(p), c = first_of(p + 1) - o;
    const int rows = pair_rows[p];
    int fl = (rows > rows_cap ? BRISK_PAIR_ROWS_CUT : 0) | (rows == -1 ? BRISK_PAIR_BAD : 0);
    const int used = (min(rows, rows_cap) + MX_ROWS - 1) / MX_ROWS;  // (workgroups behind the pair's rows wrote 0)
    int over = 0;
    for (int b = 0; b < used; ++b) over |= blk_over[(long long)p * bpp + b];
    if (over) fl |= BRISK_PAIR_ENTRIES_CUT;
    if (p >= cutp) fl |= BRISK_PAIR_MATCHES_CUT;
    counts[p] = (int)min(c, (long long)0x7FFFFFFF);
    flags[p] = fl;
    offsets[p] = p >= cutp ? stop : o;
    if (rows_copy) rows_copy[p] = rows;
  }
  if (tid == 0) offsets[npairs] = stop;
}

__global__ void __launch_bounds__(MX_ROWS) k_pair_select_scatter(const BriskDMatch* __restrict__ out, const int* __restrict__ out_count,
                                                                 const int* __restrict__ pair_rows, int p0, int rows_cap, int per_row,
                                                                 BriskMatchSelect sel, const long long* __restrict__ blk_off,
                                                                 const int* __restrict__ flags, long long matches_cap,
                                                                 BriskDMatch* __restrict__ matches) {
  __shared__ long long part[MX_WAVES];
  const int p = p0 + blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int nrows = min(pair_rows[p], rows_cap);
  if ((int)blockIdx.x * MX_ROWS >= nrows || (flags[p] & BRISK_PAIR_MATCHES_CUT)) return;
  const int q = blockIdx.x * MX_ROWS + tid;
  const long long row = (long long)p * rows_cap + q;
  bool over;
  const int n = q < nrows ? mx_row_count(out, out_count, row, per_row, sel, &over) : 0;
  // exclusive scan of the rows' counts: inside the wave, then over the wave totals
  long long incl = n;
  for (int off = 1; off < 64; off <<= 1) {
    const long long v = __shfl_up(incl, off, 64);
    if (lane >= off) incl += v;
  }
  if (lane == 63) part[wave] = incl;
  __syncthreads();
  long long pos = blk_off[(long long)p * gridDim.x + blockIdx.x] + incl - n;
  for (int w = 0; w < wave; ++w) pos += part[w];
  const uint4* src = reinterpret_cast<const uint4*>(out + row * per_row);
  uint4* dst = reinterpret_cast<uint4*>(matches);
  for (int i = 0; i < n; ++i)
    if (pos + i < matches_cap) dst[pos + i] = src[i];  // (always true while the arrays did not change between the passes)
}

__global__ void __launch_bounds__(256) k_pair_select_egress(const int* __restrict__ s_rows, const int* __restrict__ s_counts,
                                                            const int* __restrict__ s_flags, const long long* __restrict__ s_offsets,
                                                            const uint32_t* __restrict__ s_matches, int npairs, int* h_rows, int* h_counts,
                                                            int* h_flags, long long* h_offsets, uint32_t* h_matches) {
  const long gt = (long)blockIdx.x * blockDim.x + threadIdx.x, gn = (long)gridDim.x * blockDim.x;
  if (blockIdx.x == 0) {
    for (int i = threadIdx.x; i < npairs; i += blockDim.x) { h_rows[i] = s_rows[i]; h_counts[i] = s_counts[i]; h_flags[i] = s_flags[i]; }
    for (int i = threadIdx.x; i <= npairs; i += blockDim.x) h_offsets[i] = s_offsets[i];
  }
  ex_copy_words(h_matches, s_matches, s_offsets[npairs] * (long long)(sizeof(BriskDMatch) / 4), gt, gn);
}

int brisk_match_export_blocks_per_pair(int rows_cap) { return (rows_cap + MX_ROWS - 1) / MX_ROWS; }

void brisk_launch_pair_select(const BriskDMatch* out, const int* out_count, const int* pair_rows, int npairs, int rows_cap, int per_row,
                              const BriskMatchSelect& sel, long long* blk, int* blk_over, long long matches_cap, int* counts, int* flags,
                              long long* offsets, BriskDMatch* matches, int* rows_copy, hipStream_t s) {
  const int bpp = brisk_match_export_blocks_per_pair(rows_cap);
  // grid (workgroups per pair, pairs), 65535 pairs at a time (what grid.y holds)
  for (int p0 = 0; p0 < npairs; p0 += 65535)
    hipLaunchKernelGGL(k_pair_select_count, dim3(bpp, min(65535, npairs - p0)), dim3(MX_ROWS), 0, s, out, out_count, pair_rows, p0, rows_cap,
                       per_row, sel, blk, blk_over);
  hipLaunchKernelGGL(k_pair_select_offsets, dim3(1), dim3(MX_THREADS), 0, s, blk, blk_over, pair_rows, npairs, bpp, rows_cap, matches_cap,
                     counts, flags, offsets, rows_copy);
  for (int p0 = 0; p0 < npairs; p0 += 65535)
    hipLaunchKernelGGL(k_pair_select_scatter, dim3(bpp, min(65535, npairs - p0)), dim3(MX_ROWS), 0, s, out, out_count, pair_rows, p0, rows_cap,
                       per_row, sel, blk, flags, matches_cap, matches);
}

void brisk_launch_pair_select_egress(const int* s_rows, const int* s_counts, const int* s_flags, const long long* s_offsets,
                                     const BriskDMatch* s_matches, int npairs, int* h_rows, int* h_counts, int* h_flags, long long* h_offsets,
                                     void* h_matches, hipStream_t s) {
  // the link bounds this kernel, not the chip (brisk_launch_export_egress): few workgroups, the CUs stay with the next batch
  hipLaunchKernelGGL(k_pair_select_egress, dim3(48), dim3(256), 0, s, s_rows, s_counts, s_flags, s_offsets,
                     reinterpret_cast<const uint32_t*>(s_matches), npairs, h_rows, h_counts, h_flags, h_offsets,
                     static_cast<uint32_t*>(h_matches));
}

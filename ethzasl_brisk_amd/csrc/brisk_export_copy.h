// The dword copy of the egress kernels (brisk_export.hip: keypoints and descriptors; brisk_match_export.hip: matches;
// brisk_track_export.hip: tracks): packed device slab -> host memory the device can write, over the link.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// dwords [0, n) of src (16-byte aligned) -> dst (host memory, 4-byte aligned): 16-byte stores where dst allows them
__device__ __forceinline__ void ex_copy_words(uint32_t* __restrict__ dst, const uint32_t* __restrict__ src, long long n, long gt, long gn) {
  if ((reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
    const long long nv = n >> 2;
    const uint4* s4 = reinterpret_cast<const uint4*>(src);
    uint4* d4 = reinterpret_cast<uint4*>(dst);
    for (long long i = gt; i < nv; i += gn) d4[i] = s4[i];
    for (long long i = (nv << 2) + gt; i < n; i += gn) dst[i] = src[i];
  } else {
    for (long long i = gt; i < n; i += gn) dst[i] = src[i];
  }
}

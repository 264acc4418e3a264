// brisk_hostmem.h - host code only: the owner of one device or pinned host allocation of a context / pool group.
// (No device compiler output depends on this file: build.kernel_revision() leaves it out, like brisk_capi.hip.)
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

enum class MemKind { Device, Pinned };  // hipMalloc / hipFree, hipHostMalloc / hipHostFree

// Grown when a call asks for more than it holds, never shrunk, released with its owner.  grow() allocates exactly what was
// asked (+ slack); it does not synchronise: the caller first waits for whatever may still use the old allocation and drops
// what it remembers about the old contents.
template <MemKind K>
struct GrowBuf {
  void* p = nullptr;
  size_t cap = 0;  // bytes the allocation was grown to (without the slack)

  GrowBuf() = default;
  GrowBuf(const GrowBuf&) = delete;
  GrowBuf& operator=(const GrowBuf&) = delete;
  ~GrowBuf() { reset(); }

  template <class T>
  T* as() const { return static_cast<T*>(p); }

  void reset() {
    if (p) (void)(K == MemKind::Device ? hipFree(p) : hipHostFree(p));
    p = nullptr;
    cap = 0;
  }
  // hipSuccess at once when `bytes` fit; after a failure the buffer is empty
  hipError_t grow(size_t bytes, size_t slack = 0) { return grow_flags(bytes, slack, hipHostMallocDefault); }
  // pinned buffers only: with hipHostMalloc's flags
  hipError_t grow(size_t bytes, size_t slack, unsigned host_flags) {
    static_assert(K == MemKind::Pinned, "hipHostMalloc flags on a device buffer");
    return grow_flags(bytes, slack, host_flags);
  }

 private:
  hipError_t grow_flags(size_t bytes, size_t slack, unsigned host_flags) {
    if (bytes <= cap) return hipSuccess;
    reset();
    const hipError_t e = K == MemKind::Device ? hipMalloc(&p, bytes + slack) : hipHostMalloc(&p, bytes + slack, host_flags);
    if (e != hipSuccess) {
      p = nullptr;
      return e;
    }
    cap = bytes;
    return hipSuccess;
  }
};
using DeviceBuf = GrowBuf<MemKind::Device>;
using PinnedBuf = GrowBuf<MemKind::Pinned>;

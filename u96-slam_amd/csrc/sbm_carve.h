// sbm_carve.h -- how several pieces share one buffer (internal). Plain C++ over <stddef.h>: nothing here needs HIP, and under
// HIP the same statements are device code as well.
#pragma once
#include <stddef.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define SBM_HD __host__ __device__
#else
#define SBM_HD
#endif

namespace sbm {

// Bytes up to the next 16-byte boundary: where pieces that share a buffer begin unless their layout names another alignment.
SBM_HD inline size_t pad16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

// Consecutive pieces of one buffer, each beginning on a boundary of `align` bytes (a power of two; the base is at least that
// aligned). Over a null base it only counts. A layout is one function of a Carve, run twice: the statements that place the
// pieces are the ones that size the buffer. No constructors: Carve{base} is the 16-byte layout, Carve{base, 0, a} any other.
struct Carve {
  char* base;
  size_t off = 0, align = 16;
  template <class T> SBM_HD T* take(size_t n) {
    T* piece = base ? (T*)(base + off) : nullptr;
    off += (n * sizeof(T) + align - 1) & ~(align - 1);
    return piece;
  }
};
// The bytes a layout needs: its counting pass.
template <class Layout> SBM_HD inline size_t carve_bytes(Layout layout, size_t align = 16) {
  Carve count{nullptr, 0, align};
  layout(count);
  return count.off;
}

}  // namespace sbm

// omc_carve.h -- one walk that both sizes and places the arrays of a packed buffer.  A Carve holds a base pointer and a running byte
// offset; take<T>(count) rounds the offset up to the array's alignment, hands out base + offset and advances.  With a null base the walk
// only measures: the same callable run twice gives the size to allocate and then the pointers, so a size formula and a pointer walk cannot
// disagree.  The base is taken to be aligned for every array of the walk (device allocations are aligned to 256 bytes).
// Plain C++17: no HIP header, no device call (tests/host/carve_check.cpp runs every walk of omc_walks.h on the host).
#pragma once
#include <stddef.h>
#include <stdint.h>

class Carve {
 public:
  explicit Carve(void* base_ = nullptr) : base((uintptr_t)base_) {}
  // `count` elements of T at the next offset that is a multiple of `align` bytes; in a measuring walk the pointer is only an offset and must
  // not be dereferenced
  template <class T> T* take(size_t count, size_t align = alignof(T)) {
    off = (off + align - 1) / align * align;
    T* p = (T*)(base + off);      // integer arithmetic: a measuring walk offsets a null base
    off += count * sizeof(T);
    return p;
  }
  size_t bytes() const { return off; }

 private:
  uintptr_t base;
  size_t off = 0;
};

// Workspace carving (host): every sub-array of a caller-provided workspace starts on a 256-byte boundary.  A *_workspace()
// size function runs the same carve over a null base and returns total(), so the size and the layout cannot drift apart.
#pragma once
#include <cstddef>

static inline size_t nm_align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct NmCarver {
  char* base;       // may be null: then only total() means anything
  size_t off = 0;
  explicit NmCarver(void* b) : base((char*)b) {}
  // `count` elements of T at the running offset; advances by their size rounded up to 256 bytes
  template <typename T>
  T* take(size_t count) {
    T* p = (T*)(base + off);
    off += nm_align256(count * sizeof(T));
    return p;
  }
  size_t total() const { return off; }
};

// One description per device scratch buffer, for its size and its carving.
//
// A layout is a plain struct of typed pointers with one member function
//   void fill(carver& c, <dimensions>)
// that takes its regions from the carver in order.  The function runs twice:
// over a null base it only counts (layout_bytes: the size the buffer needs),
// over the buffer's base it yields the pointers.  Host code only (capi.hip's
// carve() is the one place that sizes, allocates and carves a DevBuf; the
// stand-alone tests/scratch_layout_check.hip carves heap blocks of exactly
// layout_bytes).
#pragma once
#include <cstddef>
#include <cstdint>

namespace dgpu {

struct carver {
  uint8_t* base;  // nullptr: the sizing pass (every take() returns nullptr)
  size_t off = 0;
  // `count` elements of T, the region's start rounded up to `align` bytes
  // (relative to the base: a hipMalloc base is aligned far beyond any of ours)
  template <class T>
  T* take(size_t count, size_t align = alignof(T)) {
    off = (off + align - 1) / align * align;
    const size_t at = off;
    off += count * sizeof(T);
    return base ? reinterpret_cast<T*>(base + at) : nullptr;
  }
  size_t bytes() const { return off; }
};

// The bytes a buffer of layout L needs for these dimensions.
template <class L, class... D>
size_t layout_bytes(D... dims) {
  L l{};
  carver c{nullptr};
  l.fill(c, dims...);
  return c.bytes();
}

// L carved from `base` (layout_bytes<L>(dims...) bytes).
template <class L, class... D>
L layout_at(void* base, D... dims) {
  L l{};
  carver c{static_cast<uint8_t*>(base)};
  l.fill(c, dims...);
  return l;
}

}  // namespace dgpu

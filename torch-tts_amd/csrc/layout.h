// Host-side layout helpers shared by every C-ABI family: the alignment grid, the 1-D launch grid, and the Carver that walks a
// workspace or a weight blob.
#pragma once
#include "common.h"

namespace ttsdec {

constexpr size_t kAlign = 64;  // floats (256 bytes): every buffer of a workspace and every tensor of a blob starts on this grid
inline size_t up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline dim3 grid1(size_t n) { return dim3((unsigned)((n + 255) / 256)); }  // n elements, one per lane of 256-thread workgroups

// A workspace is walked once per call by a carve routine: with the caller's pointer it hands out the buffers, with none it only
// counts - so the size a *_workspace_bytes function reports is the layout the call uses.  A blob layout is the same walk kept as
// offsets (take_off).  Buffers are kAlign floats apart.
struct Carver {
  float* base;  // nullptr: count only
  size_t off = 0, slack = 0;  // floats handed out; floats reported on top of them (vits2.hip carve_stack)
  size_t take_off(size_t n) {
    const size_t o = off;
    off += up(n, kAlign);
    return o;
  }
  float* take(size_t n) {
    const size_t o = take_off(n);
    return base ? base + o : nullptr;
  }
  f16* take_h(size_t n) { return reinterpret_cast<f16*>(take(n)); }  // n floats = the hi + lo planes of n elements
  size_t bytes() const { return (off + slack) * sizeof(float); }
};

}  // namespace ttsdec

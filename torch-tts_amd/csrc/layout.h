// Host-side layout helpers shared by every C-ABI family: the alignment grid, the 1-D launch grid, the Carver that walks a
// workspace or a weight blob, and what every blob walk starts from.
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

// The LSTM kernels of the ttsdec_, ttsenc_ and ttsenc_style_ families address each GEMM operand through ONE buffer descriptor
// based at the lowest of its K segments (gemm_tile.h DmaDesc::PerPlane).  Every segment of their A operand lies in the call's
// workspace (the style encoder's last state buffer: in enc_out, which has the size of a workspace buffer), every segment of
// their B operand in the packed blob, so neither allocation may reach the descriptor's range: beyond it a lane would count as
// out of range and zeros, not data, would land in LDS.  -> bytes, or 0 = refused.  The workspace walks of the three families
// end in this call, so *_workspace_bytes and the calls that carve the workspace give one answer; *_create asks it of the blob.
inline size_t within_dma_reach(size_t bytes) { return bytes < kBufRange ? bytes : 0; }

// A weight blob is walked once, at *_create, into one record per weight; layout, pack, the tensor count and the forward calls read
// the records.  BlobWalk is what every family's walk starts from: the carver hands out the offsets in blob order, src the source
// indices in the order include/ttsdec.h documents - the two orders are the same - so src, at the end, is *_num_weight_tensors.
struct Vec {  // a tensor kept as given, plain fp32 (a bias, LayerNorm gamma / beta, a table): offset and elements in floats
  size_t off, n;
  int src;
};
struct BlobWalk {
  Carver cv{nullptr};
  int src = 0;
  Vec vec(size_t n) { return {cv.take_off(n), n, src++}; }
};

}  // namespace ttsdec

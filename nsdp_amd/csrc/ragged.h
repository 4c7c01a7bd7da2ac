// Packed ("ragged") query sets: the rows of B shapes concatenated, packed[cap, C], with offsets[B + 1] int32 ON THE DEVICE
// (shape s owns rows offsets[s] .. offsets[s + 1], offsets[B] = total <= cap; rows at or beyond total are padding that no
// kernel reads as a result or writes).  The host knows only `cap` and `B`: they fix the launch grid, so one captured graph
// serves every mix of sizes.
//
// Who owns a tile.  The rows of a shape are cut into tiles of kTile rows starting at the shape's first row (16 for a decoder
// wave, 256 for a kNN workgroup): a tile never straddles two shapes, a shape's last tile is partial.  Tiles are numbered
// shape after shape, so sum_s ceil(n_s / kTile) <= ceil(cap / kTile) + B of them exist and the grid is sized for that bound;
// a tile index beyond the sum is surplus and returns.  The owner of tile t is found by walking `offsets` (B is small: a few
// scalar loads against the thousands of MFMAs a decoder wave issues).
//
// Whatever `offsets` holds, the walk yields rows inside [0, cap) and a shape inside [0, B): every entry is clamped to
// [previous entry, cap] as it is read, so a corrupt offsets tensor gives wrong numbers, never an access outside the buffers.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nsdp {

// `tile` must be uniform over the wave.  true: rows [row0, end) of shape b are this tile's (0 <= b < B,
// 0 <= row0 < end <= cap, end - row0 may exceed kTile: `end` is the SHAPE's end, the clamp target of a partial tile).
// b, row0 and end come back through readfirstlane: provably wave-uniform, so the per-shape table bases stay scalar.
template <int kTile>
__device__ __forceinline__ bool ragged_tile(const int32_t *__restrict__ offsets, int B, int cap, int tile, int &b,
                                            int &row0, int &end) {
  int lo = min(max(offsets[0], 0), cap);
  for (int s = 0; s < B; ++s) {
    const int hi = min(max(offsets[s + 1], lo), cap);
    const int nt = (hi - lo + kTile - 1) / kTile;
    if (tile < nt) {
      b = __builtin_amdgcn_readfirstlane(s);
      row0 = __builtin_amdgcn_readfirstlane(lo + tile * kTile);
      end = __builtin_amdgcn_readfirstlane(hi);
      return true;
    }
    tile -= nt;
    lo = hi;
  }
  return false;
}

// Rows [lo, hi) of shape b (0 <= b < B) of a packed set, clamped like ragged_tile clamps them: 0 <= lo <= hi <= cap whatever
// `offsets` holds.  `b` must be uniform over the wave; a few scalar loads.
__device__ __forceinline__ void ragged_range(const int32_t *__restrict__ offsets, int b, int cap, int &lo, int &hi) {
  int l = min(max(offsets[0], 0), cap);
  for (int s = 0; s < b; ++s) l = min(max(offsets[s + 1], l), cap);
  lo = __builtin_amdgcn_readfirstlane(l);
  hi = __builtin_amdgcn_readfirstlane(min(max(offsets[b + 1], l), cap));
}

// upper bound of the tiles of a packed set of `cap` rows in B shapes (see above)
inline long long ragged_max_tiles(long long cap, long long B, int tile) { return (cap + tile - 1) / tile + B; }

}  // namespace nsdp

// The LDS tile through which a 256-thread block (4 wave64) writes X^T next to X.
//
// A kernel that holds a 64-row tile of its bf16 output in registers stores it row-major as usual,
// `put`s the same 16-B vectors here, and after one __syncthreads() `store_t` writes the tile's
// transpose: no separate transpose pass re-reads X from HBM.
//
// Layout: 64 rows x NV vectors of 16 B (8 bf16), NV = 8, 16 or 32 (a 64-, 128- or 256-column tile).
// XOR swizzle: vector v of row r sits in slot v ^ ((r >> 3) & 7) of its row.  It touches the low 3 bits only,
// so a row stays a permutation of its own 16 * NV bytes and `put` is one ds_write_b128 per vector.
//
// Transposed read-out: output row c (a tile column), 16-B vector p = tile rows 8p .. 8p+7 of that
// column, gathered by 8 ds_read_u16.  In one such instruction the 64 lanes of a wave take ONE column
// vector vc (8 columns, cl = lane & 7) x the 8 row groups p = lane >> 3.  Why this has no bank
// conflicts: a row is 16 * NV bytes, a multiple of the 128 B that the 32 banks span, so the row
// index drops out of the bank number; every row r of group p has (r >> 3) & 7 == p, so the 8 row
// groups read slots vc ^ p, 8 different 16-B slots = 8 disjoint sets of 4 banks; inside a slot the 8
// columns cl are 4 dwords, two lanes to a dword (a shared dword is a broadcast, not a conflict).  64
// lanes, 32 distinct banks.  Without the XOR the 8 row groups would all hit slot vc: 8-way conflicts.
// The 4 waves take vc = 4i + wave for i < NV / 4, and every output row receives 8 x 16 B = 128
// contiguous bytes per tile.
#pragma once

#include "bf16.h"

namespace gtk {

template <int NV>
struct TileT {
  static_assert(NV == 8 || NV == 16 || NV == 32, "tile width: 64, 128 or 256 columns");
  u16x8 slot[64][NV];

  __device__ __forceinline__ void put(int row, int vec, u16x8 x) { slot[row][vec ^ ((row >> 3) & 7)] = x; }

  // rows 8p .. 8p+7 of column 8 * vc + cl
  __device__ __forceinline__ u16x8 get_t(int p, int vc, int cl) const {
    const u16* lds = reinterpret_cast<const u16*>(&slot[0][0]);
    u16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = lds[((8 * p + j) * NV + (vc ^ p)) * 8 + cl];
    return o;
  }

  // the whole tile transposed into out [.., ld]: tile element (r, c) -> out[(c0 + c) * ld + r0 + r].
  // All 256 threads call it, after the __syncthreads() that follows the last put.
  __device__ __forceinline__ void store_t(u16* __restrict__ out, size_t ld, size_t c0, size_t r0) const {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int p = lane >> 3, cl = lane & 7;
#pragma unroll 4
    for (int i = 0; i < NV / 4; ++i) {
      const int vc = 4 * i + wave;
      *reinterpret_cast<u16x8*>(out + (c0 + 8 * vc + cl) * ld + r0 + 8 * p) = get_t(p, vc, cl);
    }
  }
};

}  // namespace gtk

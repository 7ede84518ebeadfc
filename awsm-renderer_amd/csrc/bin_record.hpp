// bin_record.hpp — what k_bin<count> leaves per triangle for k_bin<fill>: which tiles of the triangle's window it goes to, in 8 bytes, so that the fill
// pass neither loads the 80-byte set-up record again nor repeats a tile test.  Plain C++ (no HIP types): the kernels and a host program (tests/native)
// include the same pack and unpack.
//
//   word 0: bit 0 ok (the triangle reaches at least one owned tile row), bit 1 big (more than kBinRecTiles tiles: walked from the full record, the
//           fields below are not meaningful), bits 2..5 window width - 1, bits 6..9 window height - 1, bits 10..19 first tile column, bits 20..29 first
//           LOCAL tile row of the shard
//   word 1: bits 0..15 one bit per tile of the window in the count pass's own loop order (row by row: bit (l - ty0) * width + (tx - tx0)), set where
//           bin_tile_hit said yes
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AWSM_BINREC_FN __host__ __device__ inline
#else
#define AWSM_BINREC_FN inline
#endif

namespace awsm {

constexpr uint32_t kBinRecTiles = 16;          // a small triangle's window holds at most this many tiles (k_bin: big = ntiles > kBinRecTiles)
constexpr uint32_t kBinRecExtentBits = 4;      // width - 1 and height - 1: a 1 x 16 or 16 x 1 window is a small one
constexpr uint32_t kBinRecTileBits = 10;       // first tile column / local tile row
// the frames the record can describe; a larger one keeps the fill pass on the set-up records (bin_rec_fits)
constexpr uint32_t kBinRecMaxTileCols = 1u << kBinRecTileBits, kBinRecMaxTileRows = 1u << kBinRecTileBits;
static_assert(kBinRecTiles <= 16, "the mask is 16 bits");
static_assert((1u << kBinRecExtentBits) >= kBinRecTiles, "a window of kBinRecTiles tiles in one row or column must fit the extent fields");
static_assert(2 + 2 * kBinRecExtentBits + 2 * kBinRecTileBits <= 32, "word 0");
// the set-up record keeps pixel coordinates in 15 bits (raster_setup.hpp: tri_rec_store), 32-pixel tiles: no frame it can describe has more columns or rows
static_assert(((1u << 15) >> 5) <= kBinRecMaxTileCols && ((1u << 15) >> 5) <= kBinRecMaxTileRows, "tile coordinates of the largest frame");
static_assert((3840 + 31) / 32 <= kBinRecMaxTileCols && (2160 + 31) / 32 <= kBinRecMaxTileRows, "the 4K frame");

struct BinRecWords { uint32_t w0, w1; };
struct BinRec {
    bool ok, big;
    uint32_t tx0, ty0;      // first tile column, first local tile row
    uint32_t wm1, hm1;      // window width - 1, height - 1
    uint32_t mask;          // bit per tile, row by row
};

AWSM_BINREC_FN bool bin_rec_fits(uint32_t tiles_x, uint32_t tiles_y) { return tiles_x <= kBinRecMaxTileCols && tiles_y <= kBinRecMaxTileRows; }

AWSM_BINREC_FN BinRecWords bin_rec_pack(const BinRec& r) {
    BinRecWords w;
    w.w0 = (r.ok ? 1u : 0u) | (r.big ? 2u : 0u) | ((r.wm1 & ((1u << kBinRecExtentBits) - 1u)) << 2) | ((r.hm1 & ((1u << kBinRecExtentBits) - 1u)) << (2 + kBinRecExtentBits)) |
           ((r.tx0 & ((1u << kBinRecTileBits) - 1u)) << (2 + 2 * kBinRecExtentBits)) | ((r.ty0 & ((1u << kBinRecTileBits) - 1u)) << (2 + 2 * kBinRecExtentBits + kBinRecTileBits));
    w.w1 = r.mask & 0xFFFFu;
    return w;
}

AWSM_BINREC_FN BinRec bin_rec_unpack(BinRecWords w) {
    BinRec r;
    r.ok = (w.w0 & 1u) != 0u; r.big = (w.w0 & 2u) != 0u;
    r.wm1 = (w.w0 >> 2) & ((1u << kBinRecExtentBits) - 1u);
    r.hm1 = (w.w0 >> (2 + kBinRecExtentBits)) & ((1u << kBinRecExtentBits) - 1u);
    r.tx0 = (w.w0 >> (2 + 2 * kBinRecExtentBits)) & ((1u << kBinRecTileBits) - 1u);
    r.ty0 = (w.w0 >> (2 + 2 * kBinRecExtentBits + kBinRecTileBits)) & ((1u << kBinRecTileBits) - 1u);
    r.mask = w.w1 & 0xFFFFu;
    return r;
}

}  // namespace awsm

// The two tile images of German credit's matrix-core likelihoods: where the host (arp_build.hip: build_german) stores
// every element, and the LDS addresses at which the kernels (model_german.h: likelihood_mfma, likelihood_bf3) read them
// back.  Both sides call the functions below, and the static_asserts at the end hold the two to each other, and to the
// matrix-core operand layouts, in every build.  (Four lane offsets are still written out in the kernels, next to the
// name of their function here -- german_bwd_row, bf3_a_a, bf3_b_h, bf3_b_a: the compiler tidies a function up before it
// inlines it, and through these calls the kernels came out with other instructions than with the expression in place.)
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <hip/hip_runtime.h>

#define ARP_IMG_FN __host__ __device__ __forceinline__ constexpr

namespace arp {

constexpr int kGermanCols = 64;   // padded row length of the device design matrix
// Tile image of the matrix-core likelihood (built by arp_build.hip: build_german): the design matrix in tiles of 128
// observations, each stored as the exact byte image of its LDS copy so that LDS-DMA (global_load_lds_dwordx4: 64 lanes
// x 16 contiguous bytes per instruction, no registers, no VALU) moves it.  A tile is 32 pieces of 1 KiB = 4 rows of 64
// floats; the 16-byte chunk c of row r is stored at chunk position c ^ (r & 11), followed by one piece with the 128
// outcomes.  With that XOR both operand reads of the matrix-core products are bank-conflict free as ds_read_b128
// (forward: 16 rows x one chunk of a 64-byte feature block; backward: 4 rows x 16 consecutive chunks per lane group),
// checked lane by lane against the gfx950 bank rules (4 groups of 16 lanes, bank = dword address mod 64).
constexpr int kGermanTileRows = 128;
constexpr int kGermanImgTile = 33 * 256;   // floats per tile of the image
constexpr int kGermanBlkB = 16 * kGermanCols * 4;   // bytes of a 16-row block: the block immediate of both operand reads
constexpr int kGermanYBlkB = 16 * 4;                // ... and of the outcome read

// word of element (row r, feature f) of a tile, and of the outcome of row r
ARP_IMG_FN int german_x_word(int r, int f) {
  return r * kGermanCols + ((((f >> 2) ^ (r & 11)) & 15) << 2) + (f & 3);
}
ARP_IMG_FN int german_y_word(int r) { return kGermanTileRows * kGermanCols + r; }
// Byte offsets lane (g, j) of the matrix-core layout forms, relative to the X buffer (outcomes: to the outcome buffer);
// block BLK adds BLK * kGermanBlkB (kGermanYBlkB).
//   forward read i : row j, columns 16 g + 4 i .. + 3 (chunk 4 g + i)
//   backward read s: row 4 g + s, columns 4 j .. + 3 (chunk j);  (4 g + s) & 11 = s | (g & 2) << 2
//   outcomes       : rows 4 g .. 4 g + 3
ARP_IMG_FN uint32_t german_fwd_base(uint32_t g, uint32_t j) { return j * 256u + (((g << 2) ^ (j & 8u)) << 4); }
ARP_IMG_FN uint32_t german_fwd_chunk(uint32_t j, uint32_t i) { return (i ^ (j & 3u)) << 4; }
ARP_IMG_FN uint32_t german_bwd_base(uint32_t g) { return g * 1024u; }
ARP_IMG_FN uint32_t german_bwd_row(uint32_t g, uint32_t j, uint32_t s) {
  return s * 256u + ((j ^ s ^ ((g & 2u) << 2)) << 4);
}
ARP_IMG_FN uint32_t german_y_off(uint32_t g) { return g * 16u; }

// Tile image of the bf16 x 3 likelihood (round 5; built by arp_build.hip: build_german).  Every f32 value is the exact
// sum of three bf16 pieces x = h + m + l (8 + 8 + 8 significant bits, by truncation), and a product of two such values is
// the sum of nine bf16 products, of which the six leading ones carry it to 2^-23: matrix-core work at 16 x the f32 rate.
// The data make it cheaper still: a column of zeros and ones (54 one-hot columns and the intercept of German credit) IS
// its h piece, so only the few SPLIT columns (the standardised numerics: at most 8) have m and l pieces at all, and all
// their cross terms fit ONE extra K = 32 step per product:
//   forward   eta = Xh (bh + bm + bl)  +  [Xm | Xm | Xl | 0] [bh ; bm ; bh ; 0]          (split columns only)
//   backward  v   = Xh' (wh + wm + wl) +  [Xm ; Xl]' wh + [Xm ; Xl]' wm                   (16 extra output rows)
// i.e. 7 v_mfma_f32_16x16x32_bf16 per 16 observations forward and 14 per 32 backward (224 cycles per 32 observations
// against 2 048 on v_mfma_f32_16x16x4_f32), operands read from LDS with 11 ds_read_b128 per 32 observations and wave.
// A tile holds 64 observations in 23 pieces of 1 KiB (the exact byte image of its LDS copy, moved by LDS-DMA):
//   XhF [64 rows][64 features] bf16, 16-byte chunk c of row r at chunk c ^ ((r >> 1) & 7)           8 KiB  forward A operand
//   XaF [64 rows][xm(8) | xm(8) | xl(8) | 0(8)] bf16, chunk g of row r at g ^ ((r >> 2) & 3)        4 KiB
//   XhB [2 k-steps][64 features][4 lane groups g][8] bf16: element j of group g is observation
//       32 s + (j < 4 ? 4 g + j : 16 + 4 g + j - 4) -- the order in which two forward blocks leave their residuals in a
//       lane's registers --, chunk g of feature f at g ^ ((f >> 2) & 3)                             8 KiB  backward A operand
//   XaB [2 k-steps][16 rows: xm of split column o, xl of split column o - 8][4][8] bf16, same order  2 KiB
//   y   [64] f32                                                                                   256 B
// (both operand reads are conflict free: 16 lanes x 16 bytes cover the 64 banks once).
constexpr int kBf3Rows = 64;
constexpr int kBf3Pieces = 23;
constexpr int kBf3ImgTile = kBf3Pieces * 256;   // floats per tile of the image
constexpr int kBf3XhF = 0, kBf3XaF = 8192, kBf3XhB = 12288, kBf3XaB = 20480, kBf3Y = 22528;   // byte offsets in a tile
constexpr int kBf3MaxSplit = 8;
// immediates of the operand reads: forward block (16 rows) in XhF / XaF / y, backward feature block (16 output rows) in
// XhB, backward k-step (32 observations) in XhB / XaB
constexpr int kBf3BlkH = 16 * 128, kBf3BlkA = 16 * 64, kBf3BlkY = 16 * 4;
constexpr int kBf3FbH = 16 * 64, kBf3StepH = 64 * 64, kBf3StepA = 16 * 64;

// x = h + m + l exactly, each piece a bf16 (as the f32 bit pattern with a zero low half): truncation twice, the third
// piece is what is left (at most 8 significant bits).  The same on host (the images) and device (beta, the residuals).
__host__ __device__ inline void bf3_split(float x, uint32_t& h, uint32_t& m, uint32_t& l) {
  union { float f; uint32_t u; } a, b_, c_;
  a.f = x; h = a.u & 0xffff0000u;
  b_.u = h; b_.f = x - b_.f; m = b_.u & 0xffff0000u;
  c_.u = m; c_.f = b_.f - c_.f; l = c_.u;
}

// where observation r of a tile sits in a backward fragment: k-step s, lane group g, element e
struct Bf3Frag { int s, g, e; };
ARP_IMG_FN Bf3Frag bf3_frag(int r) {
  const int rr = r & 31;
  return {r >> 5, rr < 16 ? rr >> 2 : (rr - 16) >> 2, rr < 16 ? rr & 3 : 4 + ((rr - 16) & 3)};
}
// byte position in a tile of the h piece of (row r, feature f), forward and backward copy
ARP_IMG_FN size_t bf3_xhf_byte(size_t r, size_t f) {
  return kBf3XhF + r * 128 + (((f >> 3) ^ ((r >> 1) & 7)) << 4) + (f & 7) * 2;
}
ARP_IMG_FN size_t bf3_xhb_byte(Bf3Frag p, size_t f) {
  return kBf3XhB + (size_t)p.s * 4096 + f * 64 + (((size_t)p.g ^ ((f >> 2) & 3)) << 4) + p.e * 2;
}
// ... of split column q's pieces: forward, chunk 0 and 1 (m) or 2 (l) of row r; backward, output row o = q (m) or 8 + q (l)
ARP_IMG_FN size_t bf3_xaf_byte(size_t r, size_t chunk, size_t q) {
  return kBf3XaF + r * 64 + ((chunk ^ ((r >> 2) & 3)) << 4) + q * 2;
}
ARP_IMG_FN size_t bf3_xab_byte(Bf3Frag p, size_t o) {
  return kBf3XaB + (size_t)p.s * 1024 + o * 64 + (((size_t)p.g ^ ((o >> 2) & 3)) << 4) + p.e * 2;
}
// Byte offsets lane (g, j) forms, relative to the buffer: row / feature / output row j, chunk g (XOR-permuted per row)
ARP_IMG_FN uint32_t bf3_a_h(uint32_t g, uint32_t j, uint32_t kh) {   // features 32 kh + 8 g ..; + block * kBf3BlkH
  return kBf3XhF + j * 128u + (((4u * kh + g) ^ ((j >> 1) & 7u)) << 4);
}
ARP_IMG_FN uint32_t bf3_a_a(uint32_t g, uint32_t j) {   // + block * kBf3BlkA
  return kBf3XaF + j * 64u + ((g ^ ((j >> 2) & 3u)) << 4);
}
ARP_IMG_FN uint32_t bf3_b_h(uint32_t g, uint32_t j) {   // + fb * kBf3FbH + s * kBf3StepH
  return kBf3XhB + j * 64u + ((g ^ ((j >> 2) & 3u)) << 4);
}
ARP_IMG_FN uint32_t bf3_b_a(uint32_t g, uint32_t j) {   // + s * kBf3StepA
  return kBf3XaB + j * 64u + ((g ^ ((j >> 2) & 3u)) << 4);
}
ARP_IMG_FN uint32_t bf3_y_o(uint32_t g) { return kBf3Y + g * 16u; }   // + block * kBf3BlkY

// ---- the contract, proved at compile time against the functions above ----
namespace german_image_check {

// the f32 tile is a permutation: no hole, no overwrite
constexpr bool f32_permutation() {
  bool seen[kGermanTileRows * kGermanCols] = {};
  for (int r = 0; r < kGermanTileRows; ++r)
    for (int f = 0; f < kGermanCols; ++f) {
      const int w = german_x_word(r, f);
      if (w < 0 || w >= kGermanTileRows * kGermanCols || seen[w]) return false;
      seen[w] = true;
    }
  return true;   // 8 192 distinct words in [0, 8 192)
}
// v_mfma_f32_16x16x4_f32, forward: lane (g, j) supplies row j of the block and, in read i, columns 16 g + 4 i .. + 3;
// backward: rows 4 g + s, columns 4 j .. + 3; the outcomes of rows 4 g .. 4 g + 3 sit beside the forward result
constexpr bool f32_operands() {
  for (uint32_t blk = 0; blk < kGermanTileRows / 16; ++blk)
    for (uint32_t g = 0; g < 4; ++g)
      for (uint32_t j = 0; j < 16; ++j)
        for (uint32_t i = 0; i < 4; ++i)
          for (uint32_t w = 0; w < 4; ++w) {
            const uint32_t fw = german_fwd_base(g, j) + german_fwd_chunk(j, i) + blk * kGermanBlkB + 4 * w;
            const uint32_t bw = german_bwd_base(g) + german_bwd_row(g, j, i) + blk * kGermanBlkB + 4 * w;
            if (fw != 4u * german_x_word(16 * blk + j, 16 * g + 4 * i + w)) return false;
            if (bw != 4u * german_x_word(16 * blk + 4 * g + i, 4 * j + w)) return false;
            if (german_y_off(g) + blk * kGermanYBlkB + 4 * w != 4u * (german_y_word(16 * blk + 4 * g + w) - german_y_word(0)))
              return false;
          }
  return true;
}
// v_mfma_f32_16x16x32_bf16: lane (g, j) holds row j, k = 8 g .. 8 g + 7 of an operand.  Forward, block b: row = observation
// 16 b + j, k = feature 32 kh + 8 g + e (XhF) or piece chunk g, split column e (XaF; chunk 3 stays zero).
constexpr bool bf3_forward() {
  bool seen[kBf3XaF - kBf3XhF] = {};   // XhF, in bytes / 2
  for (uint32_t b = 0; b < kBf3Rows / 16; ++b)
    for (uint32_t g = 0; g < 4; ++g)
      for (uint32_t j = 0; j < 16; ++j)
        for (uint32_t e = 0; e < 8; ++e) {
          for (uint32_t kh = 0; kh < 2; ++kh) {
            const size_t at = bf3_xhf_byte(16 * b + j, 32 * kh + 8 * g + e);
            if (bf3_a_h(g, j, kh) + b * kBf3BlkH + 2 * e != at) return false;
            if (at < (size_t)kBf3XhF || at >= (size_t)kBf3XaF || seen[at - kBf3XhF]) return false;
            seen[at - kBf3XhF] = true;
          }
          const size_t at = bf3_a_a(g, j) + b * kBf3BlkA + 2 * e;
          if (g < 3 && at != bf3_xaf_byte(16 * b + j, g, e)) return false;
          if (at < (size_t)kBf3XaF || at >= (size_t)kBf3XhB) return false;
          if (bf3_y_o(g) + b * kBf3BlkY + 4 * (e & 3) != kBf3Y + 4 * (16 * b + 4 * g + (e & 3))) return false;
        }
  return true;
}
// Backward, k-step s: row = feature 16 fb + j (XhB) or output row j of the split pieces (XaB), k = 8 g + e = the
// observation whose residual likelihood_bf3 has in element e of its B fragment: block 2 s + (e >> 2) of the forward
// product left the residuals of observations 16 b + 4 g + r in w[b][r], and w[2 s], w[2 s + 1] make k-step s.
constexpr bool bf3_backward() {
  bool seen[kBf3XaB - kBf3XhB] = {};
  for (int s = 0; s < kBf3Rows / 32; ++s)
    for (int g = 0; g < 4; ++g)
      for (int e = 0; e < 8; ++e) {
        const int r = 16 * (2 * s + (e >> 2)) + 4 * g + (e & 3);
        const Bf3Frag p = bf3_frag(r);
        if (p.s != s || p.g != g || p.e != e) return false;
        for (uint32_t j = 0; j < 16; ++j) {
          for (uint32_t fb = 0; fb < 4; ++fb) {
            const size_t at = bf3_xhb_byte(p, 16 * fb + j);
            if (bf3_b_h(g, j) + fb * kBf3FbH + s * kBf3StepH + 2 * e != at) return false;
            if (at < (size_t)kBf3XhB || at >= (size_t)kBf3XaB || seen[at - kBf3XhB]) return false;
            seen[at - kBf3XhB] = true;
          }
          const size_t at = bf3_xab_byte(p, j);
          if (bf3_b_a(g, j) + s * kBf3StepA + 2 * e != at) return false;
          if (at < (size_t)kBf3XaB || at >= (size_t)kBf3Y) return false;
        }
      }
  return true;
}

static_assert(f32_permutation(), "f32 tile image: german_x_word is not a permutation of the tile");
static_assert(f32_operands(), "f32 tile image: a lane's operand address misses the element the matrix-core layout assigns it");
static_assert(bf3_forward(), "bf16 x 3 tile image: a forward operand address misses its element (XhF / XaF / y)");
static_assert(bf3_backward(), "bf16 x 3 tile image: a backward operand address or the fragment order misses its element (XhB / XaB)");
static_assert(german_y_word(0) * 4 + kGermanTileRows * 4 <= kGermanImgTile * 4, "f32 tile image: outcomes past the tile");
static_assert(kBf3XhF == 0 && kBf3XaF == kBf3XhF + kBf3Rows * 128 && kBf3XhB == kBf3XaF + kBf3Rows * 64 &&
                  kBf3XaB == kBf3XhB + 2 * kGermanCols * 64 && kBf3Y == kBf3XaB + 2 * 16 * 64 &&
                  (kBf3Y + kBf3Rows * 4 + 1023) / 1024 == kBf3Pieces,
              "bf16 x 3 tile image: the regions must follow one another and end in the last of the kBf3Pieces KiB");

}  // namespace german_image_check

}  // namespace arp

// Array-sample gather for curvine_amd: fixed-shape uint8 image arrays
// ([N, H, W, C], the body of a .npy file) living in the arena -> the
// normalised float tensor a training step consumes.  array_samples_kernel
// reads every source byte inside the crop once and writes its element
// cropped, flipped, widened, scaled, biased, cast and in the destination
// layout, so no raw-byte tensor, no f32 temporary and no per-sample crop
// launches exist.
//
// A sample is H*W*C consecutive bytes, HWC order, 1 <= C <= 4, at ANY byte
// alignment.  Batch row b carries (dy, dx, flip); the output is one dense
// tensor of F32 / F16 / BF16, NCHW [batch, C, h, w] or NHWC
// [batch, h, w, C], its base aligned to the itemsize only.  Output row r,
// column q, channel c takes source pixel (dy + r, dx + (flip ? w-1-q : q)).
//
// One piece = `n` source bytes at arena byte `src_off`: bytes e0 .. e0+n-1
// of sample `row`.  A sample cut by cache blocks arrives as several pieces;
// a cut may fall anywhere, between the channels of one pixel too.  Every
// source byte inside the crop is converted exactly once; an output element
// whose source byte is in no piece is not written.
//
// Access pattern (memory-bound): a tile is ARRAY_TILE source bytes of one
// piece.  The workgroup stages them in LDS at their offset from the 16-byte
// grid: aligned 16-byte global loads for the body, single bytes for what
// lies before and behind it, so nothing outside the tile is read.  Then one
// lane forms one 16-byte destination unit on the destination's own 16-byte
// grid, 16/itemsize consecutive columns of a plane row (NCHW) or consecutive
// elements of a pixel row (NHWC), from byte reads of LDS; consecutive lanes
// take consecutive units, so a wave's stores are contiguous.  Rows begin at
// itemsize alignment: a unit that the row or the tile covers only in part
// (head, tail, a cut) stores its elements singly.  A tile whose source lines
// all lie outside the crop rows loads nothing.

#include <hip/hip_runtime.h>
#include <stdint.h>

// source bytes per workgroup tile
#define ARRAY_TILE 4096

#define ARRAY_NCHW 0u
#define ARRAY_NHWC 1u

struct ArrayPiece {
  uint64_t src_off;     // bytes into the arena, any alignment
  uint64_t row;         // sample (row of the batch)
  uint64_t e0;          // index of the piece's first byte in its sample
  uint64_t n;           // bytes, e0 + n <= H*W*C
};

// one per batch row
struct ArrayRow { uint32_t dy, dx, flip; };

// H*W*C < 2^31 (the host checks), so byte indices of a sample are 32-bit
struct ArrayShape {
  uint32_t H, W, C;     // source sample
  uint32_t h, w;        // crop
  uint32_t layout;      // ARRAY_NCHW / ARRAY_NHWC
  float scale[4], bias[4];
};

__host__ __device__ inline bool array_dst_supported(uint32_t d) {
  return d == DT_F32 || d == DT_F16 || d == DT_BF16;
}

// ---------------------------------------------------------------------------
// Scalar routines (the ONE definition; host + device)
// ---------------------------------------------------------------------------

// float(v) * scale rounded to f32, + bias rounded to f32, never fused: what
// numpy's x.astype(f32) * scale + bias computes; then the cast of
// tensor_cast.hip
__host__ __device__ inline uint32_t array_value(uint32_t v, float scale,
                                                float bias, uint32_t ddt) {
#pragma clang fp contract(off)
  float t = (float)v * scale;
  float r = t + bias;
  uint32_t u;
  __builtin_memcpy(&u, &r, 4);
  return cvt_from_f32(u, ddt);
}

// v[c] without indexing: the table is a kernel argument, and a lane-varying
// index would move it to scratch
__host__ __device__ inline float array_pick(const float* v, uint32_t c) {
  float lo = c & 1u ? v[1] : v[0], hi = c & 1u ? v[3] : v[2];
  return c & 2u ? hi : lo;
}

// element index of (row, r, q, c) in the dense output
__host__ __device__ inline uint64_t array_dst_index(const ArrayShape& p,
                                                    uint64_t row, uint32_t r,
                                                    uint32_t q, uint32_t c) {
  if (p.layout == ARRAY_NHWC)
    return ((row * p.h + r) * p.w + q) * p.C + c;
  return ((row * p.C + c) * p.h + r) * p.w + q;
}

__host__ __device__ inline void array_store(uint8_t* d, uint32_t bits,
                                            uint32_t ds) {
  if (ds == 4) *reinterpret_cast<uint32_t*>(d) = bits;
  else *reinterpret_cast<uint16_t*>(d) = (uint16_t)bits;
}

// byte e of sample `row` carrying v: written when it lies inside the crop
__host__ __device__ inline void array_one(uint32_t v, uint8_t* out,
                                          uint64_t row, const ArrayRow& a,
                                          uint32_t e, const ArrayShape& p,
                                          uint32_t ddt, uint32_t ds) {
  uint32_t wc = p.W * p.C;
  uint32_t y = e / wc, rem = e - y * wc;
  uint32_t xs = rem / p.C, c = rem - xs * p.C;
  if (y < a.dy || y - a.dy >= p.h || xs < a.dx || xs - a.dx >= p.w) return;
  uint32_t q = xs - a.dx;
  if (a.flip) q = p.w - 1 - q;
  array_store(out + array_dst_index(p, row, y - a.dy, q, c) * ds,
              array_value(v, array_pick(p.scale, c), array_pick(p.bias, c),
                          ddt),
              ds);
}

// ---------------------------------------------------------------------------
// Kernel
// ---------------------------------------------------------------------------

// bytes [t0, t1) of piece g, all WG threads cooperating.  lds holds
// ARRAY_TILE + 16 bytes.  Every branch around a barrier is tile-uniform.
template <uint32_t DDT, uint32_t C, uint32_t LAYOUT>
__device__ __forceinline__ void array_tile(
    const uint8_t* base, uint8_t* out, const ArrayPiece& g, const ArrayRow& a,
    uint32_t t0, uint32_t t1, const ArrayShape& p, uint8_t* lds) {
  constexpr uint32_t DS = DDT == DT_F32 ? 4 : 2;
  constexpr uint32_t K = 16 / DS;               // elements per unit
  const uint32_t wc = p.W * C;
  const uint32_t E0 = (uint32_t)g.e0 + t0, E1 = (uint32_t)g.e0 + t1;
  // source lines of the tile that are crop rows
  uint32_t y0 = E0 / wc, y1 = (E1 - 1) / wc;
  if (y0 < a.dy) y0 = a.dy;
  if (y1 > a.dy + p.h - 1) y1 = a.dy + p.h - 1;
  if (y0 > y1) return;                          // no loads, no barrier

  // stage: LDS byte i is the byte at address s_al + i
  const uint8_t* s = base + g.src_off + t0;
  const uint8_t* s_end = s + (t1 - t0);
  const uint8_t* s_al = (const uint8_t*)((uintptr_t)s & ~(uintptr_t)15);
  const uint8_t* b0 = (const uint8_t*)(((uintptr_t)s + 15) & ~(uintptr_t)15);
  const uint8_t* b1 = (const uint8_t*)((uintptr_t)s_end & ~(uintptr_t)15);
  if (b0 > s_end) b0 = s_end;                   // a piece inside one 16 B cell
  if (b1 < b0) b1 = b0;
  const uint32_t nq = (uint32_t)(b1 - b0) / 16; // <= ARRAY_TILE / 16 = WG
  for (uint32_t i = threadIdx.x; i < nq; i += WG)
    *reinterpret_cast<uint4*>(lds + (b0 - s_al) + i * 16) =
        *reinterpret_cast<const uint4*>(b0 + i * 16);
  const uint32_t n_lo = (uint32_t)(b0 - s);     // <= 15 each
  const uint32_t n_edge = n_lo + (uint32_t)(s_end - b1);
  for (uint32_t i = threadIdx.x; i < n_edge; i += WG) {
    const uint8_t* q = i < n_lo ? s + i : b1 + (i - n_lo);
    lds[q - s_al] = *q;
  }
  __syncthreads();
  const uint32_t shift = (uint32_t)(s - s_al);  // LDS index of byte E0

  // units: lines x (channels) x 16-byte cells of the destination row
  const uint32_t run = LAYOUT == ARRAY_NHWC ? p.w * C : p.w;  // elements
  const uint32_t ups = (run * DS + 15) / 16 + 1;  // cells a row can touch
  const uint32_t segs = (y1 - y0 + 1) * (LAYOUT == ARRAY_NHWC ? 1u : C);
  const uint32_t total = segs * ups;
  for (uint32_t u = threadIdx.x; u < total; u += WG) {
    uint32_t seg = u / ups, cell = u - seg * ups;
    uint32_t line = LAYOUT == ARRAY_NHWC ? seg : seg / C;
    uint32_t cs = LAYOUT == ARRAY_NHWC ? 0u : seg - line * C;
    uint32_t y = y0 + line;
    uint8_t* rowp = out + array_dst_index(p, g.row, y - a.dy, 0, cs) * DS;
    uint8_t* up = (uint8_t*)((uintptr_t)rowp & ~(uintptr_t)15) + cell * 16;
    // element m of the row sits at up + k*DS for m = m0 + k (m0 may be < 0)
    int32_t m0 = (int32_t)((intptr_t)(up - rowp) / (intptr_t)DS);
    uint32_t o[4] = {0u, 0u, 0u, 0u};
    uint32_t valid = 0;
#pragma unroll
    for (uint32_t k = 0; k < K; ++k) {
      int32_t m = m0 + (int32_t)k;
      if (m < 0 || (uint32_t)m >= run) continue;
      uint32_t q, c;
      if (LAYOUT == ARRAY_NHWC) { q = (uint32_t)m / C; c = (uint32_t)m - q * C; }
      else { q = (uint32_t)m; c = cs; }
      uint32_t xs = a.dx + (a.flip ? p.w - 1 - q : q);
      uint32_t e = y * wc + xs * C + c;
      if (e < E0 || e >= E1) continue;          // another tile's byte
      uint32_t bits = array_value(lds[shift + (e - E0)],
                                  array_pick(p.scale, c),
                                  array_pick(p.bias, c), DDT);
      if (DS == 4) o[k] = bits;
      else o[k >> 1] |= bits << ((k & 1u) * 16u);
      valid |= 1u << k;
    }
    if (valid == (1u << K) - 1u) {
      *reinterpret_cast<uint4*>(up) = make_uint4(o[0], o[1], o[2], o[3]);
    } else if (valid) {
#pragma unroll
      for (uint32_t k = 0; k < K; ++k)
        if (valid & (1u << k)) {
          uint32_t bits = DS == 4 ? o[k] : (o[k >> 1] >> ((k & 1u) * 16u));
          array_store(up + k * DS, bits, DS);
        }
    }
  }
  __syncthreads();                              // LDS is reused by the next tile
}

template <uint32_t DDT, uint32_t C, uint32_t LAYOUT>
__device__ __forceinline__ void array_tiles(
    const uint8_t* base, const ArrayPiece* pieces, const uint32_t* tile_piece,
    const uint64_t* tile_off, uint32_t n_tiles, const ArrayRow* rows,
    uint8_t* out, const ArrayShape& p, uint8_t* lds) {
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    ArrayPiece g = pieces[tile_piece[tile]];
    ArrayRow a = rows[g.row];
    uint64_t t0 = tile_off[tile];
    uint64_t t1 = min(t0 + (uint64_t)ARRAY_TILE, g.n);
    array_tile<DDT, C, LAYOUT>(base, out, g, a, (uint32_t)t0, (uint32_t)t1, p,
                               lds);
  }
}

// Tile table as in token_windows_kernel: tile -> piece, tile -> first byte
// of the piece; grid-stride over tiles.  No workgroup waits on another.
extern "C" __global__ __launch_bounds__(WG) void array_samples_kernel(
    const uint8_t* __restrict__ base, const ArrayPiece* __restrict__ pieces,
    const uint32_t* __restrict__ tile_piece,
    const uint64_t* __restrict__ tile_off, uint32_t n_tiles,
    const ArrayRow* __restrict__ rows, uint8_t* __restrict__ out,
    ArrayShape p, uint32_t dst_dt) {
  __shared__ uint4 lds4[ARRAY_TILE / 16 + 1];
  uint8_t* lds = reinterpret_cast<uint8_t*>(lds4);
#define ARRAY_CASE(D, CH, L)                                                  \
  case ((D) * 8u + (CH)) * 2u + (L):                                          \
    array_tiles<D, CH, L>(base, pieces, tile_piece, tile_off, n_tiles, rows,  \
                          out, p, lds);                                       \
    break;
#define ARRAY_CASES(D)                                                        \
  ARRAY_CASE(D, 1, ARRAY_NCHW) ARRAY_CASE(D, 1, ARRAY_NHWC)                   \
  ARRAY_CASE(D, 2, ARRAY_NCHW) ARRAY_CASE(D, 2, ARRAY_NHWC)                   \
  ARRAY_CASE(D, 3, ARRAY_NCHW) ARRAY_CASE(D, 3, ARRAY_NHWC)                   \
  ARRAY_CASE(D, 4, ARRAY_NCHW) ARRAY_CASE(D, 4, ARRAY_NHWC)
  switch ((dst_dt * 8u + p.C) * 2u + p.layout) {
    ARRAY_CASES(DT_F32) ARRAY_CASES(DT_F16) ARRAY_CASES(DT_BF16)
    default: break;   // host rejects everything else before launch
  }
#undef ARRAY_CASES
#undef ARRAY_CASE
}

// host arena + host destination: the same pieces, the same scalar routines,
// plain loops
static void array_samples_host(const uint8_t* base, const ArrayPiece& g,
                               const ArrayRow* rows, uint8_t* out,
                               const ArrayShape& p, uint32_t ddt) {
  uint32_t ds = cast_itemsize(ddt);
  for (uint64_t i = 0; i < g.n; ++i)
    array_one(base[g.src_off + i], out, g.row, rows[g.row],
              (uint32_t)(g.e0 + i), p, ddt, ds);
}

// one whole sample (H*W*C bytes at `src`) -> its dense C*h*w output at `out`
static void array_sample_host(const uint8_t* src, const ArrayRow& a,
                              uint8_t* out, const ArrayShape& p, uint32_t ddt) {
  ArrayPiece g{0, 0, 0, (uint64_t)p.H * p.W * p.C};
  array_samples_host(src, g, &a, out, p, ddt);
}

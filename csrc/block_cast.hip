// Two-dimensional block scales for curvine_amd: an F8_E4M3 tensor (..., M, K)
// whose bm x bn tiles (128 x 128 in the checkpoints that ship this layout)
// share one F32 scale, w = q * scale_inv, the scales a dense F32 tensor of
// shape (..., ceil(M/bm), ceil(K/bn)).  Leading dimensions are batches of
// matrices: a tile never spans two of them.  Three kernels on the tile
// tables of tensor_cast.hip:
//
//   block_absmax_kernel  rows-of-runs F32/F16/BF16 sources at absolute
//                        addresses -> amax bits in the tile slots
//                        (scale_slots_kernel zeroes and finishes them)
//   block_store_kernel   the same sources -> F8_E4M3 in the arena
//   block_load_kernel    F8_E4M3 in the arena -> F32/F16/BF16
//
// Numerics: those of tensor_cast.hip, nothing new.  scale = max(amax,
// 2^-40) / 448 (cast_scale_of_amax), q = saturate(x / scale) and y = q *
// scale with one IEEE f32 divide or multiply (cvt_scaled), shared by the
// kernels and the host loops.
//
// A segment is `rows` runs of `run` elements `src_pitch` bytes apart.  The
// element in row r, column c of the segment is element t = scale_e0 + r *
// scale_pitch + c of its tensor and looks its scale up by its own tensor
// coordinates (block_scale_index), so a piece may start and end anywhere:
// mid-row, mid-tile, in a collapsed layout whose runs are longer than a
// row, or in a shard whose parts cut the tiles.
//
// Access pattern, as in mx_cast.hip: one unit of 8 elements per lane per
// pass, aligned on the destination, so a wave's store is contiguous (uint2
// quantised, 16 or 32 B dequantised).  A unit inside one row and one tile
// column fetches one scale; a unit that crosses a row end or a tile-column
// edge, heads, tails and sources whose alignment allows no vector load go
// element-wise.  Nothing outside a run's bytes is read but the aligned
// dword holding its first byte (cast_load_words).

// tile slots a workgroup reduces in LDS at a time (block_absmax_kernel)
#define BLOCK_LDS_SLOTS 1024u

struct BlockSeg {
  uint64_t src;         // absmax, store: absolute address of row 0;
                        // load: bytes into the arena, any alignment
  uint64_t dst;         // store: bytes into the arena; load: absolute
                        // address of dense element 0; absmax: unused
  uint64_t rows, run;   // rows runs of run elements
  uint64_t src_pitch;   // bytes between run starts
  uint64_t scale_ptr;   // absolute address of the tensor's f32 tile scales
                        // (absmax: of its amax slots)
  uint64_t scale_e0;    // tensor index of row 0, column 0
  uint64_t scale_pitch; // tensor elements between run starts
  uint64_t M, K;        // the tensor's last two dimensions
  uint64_t bm, bn;      // tile height and width
  uint64_t tm, tn;      // ceil(M / bm), ceil(K / bn): filled in by the host
  uint32_t dt;          // F32/F16/BF16: the source (absmax, store) or the
                        // destination (load)
  uint32_t pad;
};

// most tensors index in 32 bits, where a divide costs a fraction of the
// 64-bit one
__host__ __device__ inline uint64_t block_div(uint64_t a, uint64_t b) {
  return ((a | b) >> 32) ? a / b : (uint64_t)((uint32_t)a / (uint32_t)b);
}

// Scale of tensor element t: row = t / K, col = t % K,
// ((row / M) * ceil(M/bm) + (row % M) / bm) * ceil(K/bn) + col / bn.
// left: the elements from t to the end of its tile column or of its row,
// all under the same scale.
__host__ __device__ inline uint64_t block_scale_index(const BlockSeg& g,
                                                      uint64_t t,
                                                      uint64_t& left) {
  uint64_t row = block_div(t, g.K), col = t - row * g.K;
  uint64_t mat = row < g.M ? 0 : block_div(row, g.M), rm = row - mat * g.M;
  uint64_t tc = block_div(col, g.bn);
  uint64_t end = (tc + 1) * g.bn;
  left = (end < g.K ? end : g.K) - col;
  return (mat * g.tm + block_div(rm, g.bm)) * g.tn + tc;
}

__host__ __device__ inline void block_locate(const BlockSeg& g, uint64_t e,
                                             uint64_t& r, uint64_t& c) {
  if (g.rows == 1) { r = 0; c = e; }
  else { r = block_div(e, g.run); c = e - r * g.run; }
}

// scale index of the element in row r, column c of the segment
__host__ __device__ inline uint64_t block_scale_at(const BlockSeg& g,
                                                   uint64_t r, uint64_t c) {
  uint64_t left;
  return block_scale_index(g, g.scale_e0 + r * g.scale_pitch + c, left);
}

// source bits of an absmax / store segment's element
__host__ __device__ inline uint32_t block_src_bits(const BlockSeg& g,
                                                   const uint8_t* src,
                                                   uint64_t r, uint64_t c) {
  if (g.dt == DT_F32)
    return *reinterpret_cast<const uint32_t*>(src + r * g.src_pitch + c * 4);
  return *reinterpret_cast<const uint16_t*>(src + r * g.src_pitch + c * 2);
}

// one element, quantised: the kernels' edges and the host loop
__host__ __device__ inline uint32_t block_quant_at(const BlockSeg& g,
                                                   const uint8_t* src,
                                                   uint64_t e) {
  uint64_t r, c;
  block_locate(g, e, r, c);
  return cvt_scaled(
      block_src_bits(g, src, r, c), g.dt, DT_F8_E4M3,
      reinterpret_cast<const float*>(g.scale_ptr)[block_scale_at(g, r, c)]);
}

// one element, dequantised to the bits of the destination dtype
__host__ __device__ inline uint32_t block_dequant_at(const BlockSeg& g,
                                                     const uint8_t* src,
                                                     uint64_t e) {
  uint64_t r, c;
  block_locate(g, e, r, c);
  return cvt_scaled(
      src[r * g.src_pitch + c], DT_F8_E4M3, g.dt,
      reinterpret_cast<const float*>(g.scale_ptr)[block_scale_at(g, r, c)]);
}

__host__ __device__ inline void block_put(uint8_t* d, uint64_t e,
                                          uint32_t bits, uint32_t ddt) {
  if (ddt == DT_F32) reinterpret_cast<uint32_t*>(d)[e] = bits;
  else reinterpret_cast<uint16_t*>(d)[e] = (uint16_t)bits;
}

// ---------------------------------------------------------------------------
// Kernels
// ---------------------------------------------------------------------------

template <uint32_t SDT>
__device__ __forceinline__ void block_store_tile(const BlockSeg& g,
                                                 uint8_t* dst, uint64_t t0,
                                                 uint64_t t1) {
  constexpr int SS = SDT == DT_F32 ? 4 : 2;
  const uint8_t* src = reinterpret_cast<const uint8_t*>(g.src);
  const float* scales = reinterpret_cast<const float*>(g.scale_ptr);
  uint64_t n = g.rows * g.run;
  uint64_t hd = (0 - (uintptr_t)dst) & 7;          // to an 8-byte store
  if (hd > n) hd = n;
  uint64_t nb = (n - hd) / 8, tail0 = hd + nb * 8, u0, u1;
  mx_tile_units(hd, nb, t0, t1, u0, u1);
  for (uint64_t u = u0 + threadIdx.x; u < u1; u += WG) {
    uint64_t e = hd + u * 8, r, c, left;
    block_locate(g, e, r, c);
    uint64_t si = block_scale_index(g, g.scale_e0 + r * g.scale_pitch + c,
                                    left);
    uint32_t q[8], x[8];
    if (c + 8 <= g.run && left >= 8 &&
        mx_load_unit<SDT>(src + r * g.src_pitch + c * SS, x)) {
      float s = scales[si];
#pragma unroll
      for (int k = 0; k < 8; ++k) q[k] = cvt_scaled(x[k], SDT, DT_F8_E4M3, s);
    } else {
      for (int k = 0; k < 8; ++k) q[k] = block_quant_at(g, src, e + k);
    }
    uint32_t o0 = 0, o1 = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      o0 |= q[k] << (8 * k);
      o1 |= q[k + 4] << (8 * k);
    }
    *reinterpret_cast<uint2*>(dst + e) = make_uint2(o0, o1);
  }
  // head + tail: byte stores of distinct bytes, each by the tile that
  // holds the element
  uint64_t edge = hd + (n - tail0);
  for (uint64_t i = threadIdx.x; i < edge; i += WG) {
    uint64_t e = i < hd ? i : tail0 + (i - hd);
    if (e < t0 || e >= t1) continue;
    dst[e] = (uint8_t)block_quant_at(g, src, e);
  }
}

extern "C" __global__ __launch_bounds__(WG) void block_store_kernel(
    uint8_t* __restrict__ base, const BlockSeg* __restrict__ segs,
    const uint32_t* __restrict__ tile_seg, const uint64_t* __restrict__ tile_off,
    uint32_t n_tiles) {
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    BlockSeg g = segs[tile_seg[tile]];
    uint64_t t0 = tile_off[tile];
    uint64_t t1 = min(t0 + (uint64_t)CAST_TILE, g.rows * g.run);
    uint8_t* dst = base + g.dst;
    switch (g.dt) {
      case DT_F32: block_store_tile<DT_F32>(g, dst, t0, t1); break;
      case DT_F16: block_store_tile<DT_F16>(g, dst, t0, t1); break;
      case DT_BF16: block_store_tile<DT_BF16>(g, dst, t0, t1); break;
      default: break;   // host rejects every other source before launch
    }
  }
}

template <uint32_t DDT>
__device__ __forceinline__ void block_load_tile(const BlockSeg& g,
                                                const uint8_t* src,
                                                uint64_t t0, uint64_t t1) {
  constexpr int DS = DDT == DT_F32 ? 4 : 2;
  uint8_t* dst = reinterpret_cast<uint8_t*>(g.dst);
  const float* scales = reinterpret_cast<const float*>(g.scale_ptr);
  uint64_t n = g.rows * g.run;
  uint64_t hd = ((0 - (uintptr_t)dst) & 15) / DS;    // to a 16-byte store
  if (hd > n) hd = n;
  uint64_t nb = (n - hd) / 8, tail0 = hd + nb * 8, u0, u1;
  mx_tile_units(hd, nb, t0, t1, u0, u1);
  for (uint64_t u = u0 + threadIdx.x; u < u1; u += WG) {
    uint64_t e = hd + u * 8, r, c, left;
    block_locate(g, e, r, c);
    uint64_t si = block_scale_index(g, g.scale_e0 + r * g.scale_pitch + c,
                                    left);
    uint32_t f[8];
    bool fast = c + 8 <= g.run && left >= 8;
    int mode = 0;
    const uint8_t* p = src + r * g.src_pitch + c;
    if (fast) {
      mode = ((uintptr_t)p & 7) == 0 ? 0 : (((uintptr_t)p & 3) == 0 ? 1 : 2);
      // the shifted load reads up to 3 bytes past its unit: only where
      // the run still holds them
      if (mode == 2 && g.run - c - 8 < 3) fast = false;
    }
    if (fast) {
      uint32_t w[2];
      cast_load_words<2>(p, mode, w);
      float s = scales[si];
#pragma unroll
      for (int k = 0; k < 8; ++k)
        f[k] = cvt_scaled((w[k >> 2] >> ((k & 3) * 8)) & 0xFFu, DT_F8_E4M3,
                          DDT, s);
    } else {
      for (int k = 0; k < 8; ++k) f[k] = block_dequant_at(g, src, e + k);
    }
    if constexpr (DS == 4) {
      uint4* o = reinterpret_cast<uint4*>(dst + e * 4);
      o[0] = make_uint4(f[0], f[1], f[2], f[3]);
      o[1] = make_uint4(f[4], f[5], f[6], f[7]);
    } else {
      *reinterpret_cast<uint4*>(dst + e * 2) =
          make_uint4(f[0] | (f[1] << 16), f[2] | (f[3] << 16),
                     f[4] | (f[5] << 16), f[6] | (f[7] << 16));
    }
  }
  uint64_t edge = hd + (n - tail0);
  for (uint64_t i = threadIdx.x; i < edge; i += WG) {
    uint64_t e = i < hd ? i : tail0 + (i - hd);
    if (e < t0 || e >= t1) continue;
    block_put(dst, e, block_dequant_at(g, src, e), DDT);
  }
}

extern "C" __global__ __launch_bounds__(WG) void block_load_kernel(
    const uint8_t* __restrict__ base, const BlockSeg* __restrict__ segs,
    const uint32_t* __restrict__ tile_seg, const uint64_t* __restrict__ tile_off,
    uint32_t n_tiles) {
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    BlockSeg g = segs[tile_seg[tile]];
    uint64_t t0 = tile_off[tile];
    uint64_t t1 = min(t0 + (uint64_t)CAST_TILE, g.rows * g.run);
    const uint8_t* src = base + g.src;
    switch (g.dt) {
      case DT_F32: block_load_tile<DT_F32>(g, src, t0, t1); break;
      case DT_F16: block_load_tile<DT_F16>(g, src, t0, t1); break;
      case DT_BF16: block_load_tile<DT_BF16>(g, src, t0, t1); break;
      default: break;   // host rejects every other destination before launch
    }
  }
}

// amax of the tile slots: the slots hold zero before and the f32 bits of
// each tile's largest finite |x| after (non-negative f32 patterns order as
// unsigned integers and max is order-independent: deterministic).  A
// workgroup tile of CAST_TILE elements meets the slots [g_lo, g_hi]; it
// reduces them BLOCK_LDS_SLOTS at a time: lanes -> runs of lanes in the
// same slot (cross-lane) -> the slot's LDS word -> one global atomicMax per
// slot and workgroup.  The real geometry needs one window; tiny tiles take
// several, and a unit outside the current window is skipped before its
// load.
template <uint32_t SDT>
__device__ __forceinline__ void block_absmax_tile(const BlockSeg& g,
                                                  uint64_t t0, uint64_t t1,
                                                  uint32_t* lds) {
  constexpr int SS = SDT == DT_F32 ? 4 : 2;
  const uint8_t* src = reinterpret_cast<const uint8_t*>(g.src);
  uint32_t* out = reinterpret_cast<uint32_t*>(g.scale_ptr);
  const uint32_t lane = threadIdx.x & 63u;
  uint64_t r, c, left;
  block_locate(g, t0, r, c);
  uint64_t ta = g.scale_e0 + r * g.scale_pitch + c;
  block_locate(g, t1 - 1, r, c);
  uint64_t tb = g.scale_e0 + r * g.scale_pitch + c;
  // tensor indices grow with the dense index (scale_pitch >= run) and the
  // slot grows with the row: first slot of ta's row .. last slot of tb's
  uint64_t g_lo = block_scale_index(g, block_div(ta, g.K) * g.K, left);
  uint64_t g_hi = block_scale_index(g, block_div(tb, g.K) * g.K + g.K - 1,
                                    left);
  uint64_t nu = (t1 - t0 + 7) / 8;
  for (uint64_t w = g_lo; w <= g_hi; w += BLOCK_LDS_SLOTS) {
    for (uint32_t k = threadIdx.x; k < BLOCK_LDS_SLOTS; k += WG) lds[k] = 0u;
    __syncthreads();
    for (uint64_t ub = 0; ub < nu; ub += WG) {       // wave-uniform trips
      uint64_t u = ub + threadIdx.x;
      uint32_t m = 0u, slot = 0xFFFFFFFFu;           // slot - w, none yet
      if (u < nu) {
        uint64_t e = t0 + u * 8;
        block_locate(g, e, r, c);
        uint64_t si = block_scale_index(
            g, g.scale_e0 + r * g.scale_pitch + c, left);
        if (e + 8 <= t1 && c + 8 <= g.run && left >= 8) {
          if (si - w < BLOCK_LDS_SLOTS) {            // in the window
            uint32_t x[8];
            if (!mx_load_unit<SDT>(src + r * g.src_pitch + c * SS, x))
              for (int k = 0; k < 8; ++k)
                x[k] = block_src_bits(g, src, r, c + k);
#pragma unroll
            for (int k = 0; k < 8; ++k) m = max(m, absmax_key(x[k], SDT));
            slot = (uint32_t)(si - w);
          }
        } else {
          // crosses a row end or a tile-column edge, or the segment's
          // last elements: each element to its own slot
          for (uint64_t k = e; k < e + 8 && k < t1; ++k) {
            block_locate(g, k, r, c);
            uint64_t sk = block_scale_at(g, r, c);
            if (sk - w >= BLOCK_LDS_SLOTS) continue;
            uint32_t key = absmax_key(block_src_bits(g, src, r, c), SDT);
            if (key) atomicMax(&lds[sk - w], key);
          }
        }
      }
      // runs of lanes in the same slot: the last lane of a run ends up
      // with the run's max (merging lanes of the same slot from another
      // run is harmless)
#pragma unroll
      for (uint32_t o = 1; o < 64; o <<= 1) {
        uint32_t om = (uint32_t)__shfl_up((int)m, o);
        uint32_t os = (uint32_t)__shfl_up((int)slot, o);
        if (lane >= o && os == slot) m = max(m, om);
      }
      uint32_t nx = (uint32_t)__shfl_down((int)slot, 1);
      if (slot != 0xFFFFFFFFu && m && (lane == 63u || nx != slot))
        atomicMax(&lds[slot], m);
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < BLOCK_LDS_SLOTS && w + k <= g_hi;
         k += WG) {
      uint32_t v = lds[k];
      if (v) atomicMax(out + w + k, cvt_to_f32(v, SDT));   // slots start at 0
    }
    __syncthreads();                       // before the next window's zeroing
  }
}

extern "C" __global__ __launch_bounds__(WG) void block_absmax_kernel(
    const BlockSeg* __restrict__ segs, const uint32_t* __restrict__ tile_seg,
    const uint64_t* __restrict__ tile_off, uint32_t n_tiles) {
  __shared__ uint32_t lds[BLOCK_LDS_SLOTS];
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    BlockSeg g = segs[tile_seg[tile]];
    uint64_t t0 = tile_off[tile];
    uint64_t t1 = min(t0 + (uint64_t)CAST_TILE, g.rows * g.run);
    switch (g.dt) {
      case DT_F32: block_absmax_tile<DT_F32>(g, t0, t1, lds); break;
      case DT_F16: block_absmax_tile<DT_F16>(g, t0, t1, lds); break;
      case DT_BF16: block_absmax_tile<DT_BF16>(g, t0, t1, lds); break;
      default: break;   // host rejects every other source before launch
    }
  }
}

// ---------------------------------------------------------------------------
// Host twins: cpu tensors, host arenas and the byte path
// ---------------------------------------------------------------------------

static void block_absmax_segment_host(const BlockSeg& g) {
  const uint8_t* src = reinterpret_cast<const uint8_t*>(g.src);
  uint32_t* out = reinterpret_cast<uint32_t*>(g.scale_ptr);
  for (uint64_t r = 0; r < g.rows; ++r)
    for (uint64_t c = 0; c < g.run; ++c) {
      uint32_t a = cvt_to_f32(absmax_key(block_src_bits(g, src, r, c), g.dt),
                              g.dt);
      uint32_t* slot = out + block_scale_at(g, r, c);
      if (a > *slot) *slot = a;
    }
}

// src: row 0 of the source; dst: the first destination byte
static void block_store_segment_host(const uint8_t* src, uint8_t* dst,
                                     const BlockSeg& g) {
  uint64_t n = g.rows * g.run;
  for (uint64_t e = 0; e < n; ++e) dst[e] = (uint8_t)block_quant_at(g, src, e);
}

// src: row 0 of the quantised source; dst: dense element 0
static void block_load_segment_host(const uint8_t* src, uint8_t* dst,
                                    const BlockSeg& g) {
  uint64_t n = g.rows * g.run;
  for (uint64_t e = 0; e < n; ++e)
    block_put(dst, e, block_dequant_at(g, src, e), g.dt);
}

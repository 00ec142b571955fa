// OCP Microscaling (MX) tensors for curvine_amd: blocks of 32 consecutive
// elements of the last dimension share one E8M0 power-of-two scale byte,
// the elements are OCP E4M3 (MXFP8) or E2M1 packed two per byte (MXFP4).
// Three kernels on the tile tables of tensor_cast.hip:
//
//   mx_scales_kernel   rows-of-runs F32/F16/BF16 sources at absolute
//                      addresses -> the E8M0 bytes of whole tensors
//   mx_store_kernel    the same sources -> quantised elements in the arena
//   mx_load_kernel     quantised elements in the arena -> F32/F16/BF16
//
// Numerics: integer bit manipulation only, shared by the kernels and the
// host loops.  A scale is 2^(s-127); quantising is x * 2^(127-s) rounded
// ONCE (ties to the even code, saturating) and dequantising value(q) *
// 2^(s-127) rounded once, both done on the exponent field, so no result
// depends on the denormal mode and f32-subnormal sources come out right.
//
// A segment is `rows` runs of `run` elements `src_pitch` bytes apart.  The
// element in row r, column c uses the scale byte at
// (scale_e0 + r * scale_pitch + c) / 32 of its tensor: a store's dense side
// is the tensor (scale_pitch == run, scale_e0 the piece's first dense
// element), a load's rows lie scale_pitch tensor elements apart (a shard).
//
// Access pattern: one unit of 8 elements per lane per pass, aligned on the
// destination, so a wave's store is contiguous (uint2 / dword quantised,
// 16 B dequantised) and a block of 32 is four adjacent lanes.  Heads,
// tails, units that cross a row and sources whose alignment allows no
// vector load go element-wise.  Nothing outside a run's bytes is read but
// the aligned dword holding its first byte (cast_load_words).

#define MX_BLOCK 32u

enum MxFmt : uint32_t { MX_E4M3 = 0, MX_E2M1 = 1, MX_FMT_COUNT = 2 };

// dtype codes of the stored elements as Python names them (native.DTYPES)
#define DT_F8_E8M0 16u
#define DT_F4 17u

__host__ __device__ inline uint32_t mx_bits(uint32_t fmt) {
  return fmt == MX_E2M1 ? 4u : 8u;
}

// E8M0 byte of a block from the f32 bits of its amax (largest finite |x|):
// max(E - emax, 0) with E the biased exponent field, emax that of the
// element format's largest value; never 255
__host__ __device__ inline uint32_t mx_scale_of_amax(uint32_t amax_bits,
                                                     uint32_t fmt) {
  uint32_t e = (amax_bits >> 23) & 0xFFu, emax = fmt == MX_E2M1 ? 2u : 8u;
  return e > emax ? e - emax : 0u;
}

// |x| * 2^k (a: non-zero finite f32 magnitude bits) rounded once, ties to
// even, onto a format of MB mantissa bits and exponent bias BIAS, saturated
// at code MAXC.  Subnormal codes are multiples of the smallest quantum and
// a carry runs into the exponent field on its own.
template <int MB, int BIAS, uint32_t MAXC, int EMAX>
__host__ __device__ inline uint32_t mx_round_code(uint32_t a, int k) {
  uint32_t e = a >> 23, m = a & 0x7FFFFFu;
  int ex;                                   // exponent of the leading bit
  if (e == 0u) {                            // f32 subnormal: normalise
    uint32_t p = 31u - (uint32_t)__builtin_clz(m);
    m = m << (23u - p);
    ex = (int)p - 149;
  } else {
    m |= 0x800000u;
    ex = (int)e - 127;
  }
  ex += k;
  if (ex > EMAX) return MAXC;
  constexpr int EMIN = 1 - BIAS;
  int sh = 23 - MB;
  uint32_t base = 0;
  if (ex < EMIN) sh += EMIN - ex;
  else base = (uint32_t)(ex - EMIN) << MB;
  if (sh > 25) return 0u;                   // below a quarter quantum
  uint32_t r = m >> sh, rem = m & ((1u << sh) - 1u), half = 1u << (sh - 1);
  if (rem > half || (rem == half && (r & 1u))) r++;
  uint32_t code = base + r;
  return code > MAXC ? MAXC : code;
}

// f32 bits -> element code under scale byte s
__host__ __device__ inline uint32_t mx_quant(uint32_t f, uint32_t s,
                                             uint32_t fmt) {
  uint32_t a = f & 0x7FFFFFFFu;
  int k = 127 - (int)s;
  if (fmt == MX_E2M1) {
    uint32_t sign = (f >> 28) & 8u;
    if (a >= 0x7F800000u) return sign | 7u;           // inf and NaN
    if (a == 0u) return sign;
    return sign | mx_round_code<1, 1, 7u, 2>(a, k);
  }
  uint32_t sign = (f >> 24) & 0x80u;
  if (a > 0x7F800000u) return sign | 0x7Fu;
  if (a == 0x7F800000u) return sign | 0x7Eu;
  if (a == 0u) return sign;
  return sign | mx_round_code<3, 7, 0x7Eu, 8>(a, k);
}

// element code under scale byte s -> exact f32 bits (every product fits
// f32, subnormals included; past the largest finite it is inf)
__host__ __device__ inline uint32_t mx_dequant(uint32_t code, uint32_t s,
                                               uint32_t fmt) {
  uint32_t sign, mant;
  int x;                                    // value = mant * 2^x
  if (fmt == MX_E2M1) {
    sign = (code & 8u) << 28;
    uint32_t e = (code >> 1) & 3u, m = code & 1u;
    mant = e ? 2u + m : m;
    x = e ? (int)e - 2 : -1;
  } else {
    sign = (code & 0x80u) << 24;
    if ((code & 0x7Fu) == 0x7Fu) return sign | 0x7FC00000u;
    uint32_t e = (code >> 3) & 15u, m = code & 7u;
    mant = e ? 8u + m : m;
    x = e ? (int)e - 10 : -9;
  }
  if (s == 255u) return sign | 0x7FC00000u;
  if (mant == 0u) return sign;
  x += (int)s - 127;
  int p = 31 - __builtin_clz(mant);         // 0..3
  int lead = x + p;
  if (lead > 127) return sign | 0x7F800000u;
  if (lead >= -126)
    return sign | ((uint32_t)(lead + 127) << 23) |
           ((mant << (23 - p)) & 0x7FFFFFu);
  return sign | (mant << (x + 149));        // x >= -136: exact subnormal
}

struct MxSeg {
  uint64_t src;         // scales, store: absolute address of row 0;
                        // load: bytes into the arena, any alignment
  uint64_t dst;         // store: bytes into the arena; load: absolute
                        // address of dense element 0; scales: unused
  uint64_t rows, run;   // rows runs of run elements
  uint64_t src_pitch;   // bytes between run starts
  uint64_t scale_ptr;   // absolute address of the tensor's E8M0 bytes
  uint64_t scale_e0;    // tensor index of row 0, column 0
  uint64_t scale_pitch; // tensor elements between run starts
  uint32_t dt;          // F32/F16/BF16: the source (scales, store) or the
                        // destination (load)
  uint32_t fmt;         // MxFmt
};

__host__ __device__ inline void mx_locate(const MxSeg& g, uint64_t e,
                                          uint64_t& r, uint64_t& c) {
  if (g.rows == 1) { r = 0; c = e; }
  else { r = e / g.run; c = e - r * g.run; }
}

__host__ __device__ inline uint32_t mx_scale_at(const MxSeg& g, uint64_t r,
                                                uint64_t c) {
  return reinterpret_cast<const uint8_t*>(g.scale_ptr)[
      (g.scale_e0 + r * g.scale_pitch + c) / MX_BLOCK];
}

// source bits of dense element e of a scales / store segment
__host__ __device__ inline uint32_t mx_src_bits(const MxSeg& g,
                                                const uint8_t* src,
                                                uint64_t r, uint64_t c) {
  if (g.dt == DT_F32)
    return *reinterpret_cast<const uint32_t*>(src + r * g.src_pitch + c * 4);
  return *reinterpret_cast<const uint16_t*>(src + r * g.src_pitch + c * 2);
}

// one element, quantised: the kernels' edges and the host loop
__host__ __device__ inline uint32_t mx_quant_at(const MxSeg& g,
                                                const uint8_t* src,
                                                uint64_t e) {
  uint64_t r, c;
  mx_locate(g, e, r, c);
  return mx_quant(cvt_to_f32(mx_src_bits(g, src, r, c), g.dt),
                  mx_scale_at(g, r, c), g.fmt);
}

// one element, dequantised to f32 bits
__host__ __device__ inline uint32_t mx_dequant_at(const MxSeg& g,
                                                  const uint8_t* src,
                                                  uint64_t e) {
  uint64_t r, c;
  mx_locate(g, e, r, c);
  const uint8_t* row = src + r * g.src_pitch;
  uint32_t code = g.fmt == MX_E2M1 ? (row[c >> 1] >> ((c & 1u) * 4u)) & 0xFu
                                   : row[c];
  return mx_dequant(code, mx_scale_at(g, r, c), g.fmt);
}

__host__ __device__ inline void mx_put(uint8_t* d, uint64_t e, uint32_t f,
                                       uint32_t ddt) {
  uint32_t out = cvt_from_f32(f, ddt);
  if (ddt == DT_F32) reinterpret_cast<uint32_t*>(d)[e] = out;
  else reinterpret_cast<uint16_t*>(d)[e] = (uint16_t)out;
}

// ---------------------------------------------------------------------------
// Kernels
// ---------------------------------------------------------------------------

// the 8 source elements of a unit that lies inside one run, starting at p:
// vector loads where p allows them.  false: p is only 2-byte aligned.
template <uint32_t SDT>
__device__ __forceinline__ bool mx_load_unit(const uint8_t* p,
                                             uint32_t (&x)[8]) {
  if constexpr (SDT == DT_F32) {
    int mode = ((uintptr_t)p & 15) == 0 ? 0 : 1;
    uint32_t a[4], b[4];
    cast_load_words<4>(p, mode, a);
    cast_load_words<4>(p + 16, mode, b);
#pragma unroll
    for (int k = 0; k < 4; ++k) { x[k] = a[k]; x[k + 4] = b[k]; }
    return true;
  } else {
    if ((uintptr_t)p & 3) return false;
    uint32_t w[4];
    cast_load_words<4>(p, ((uintptr_t)p & 15) == 0 ? 0 : 1, w);
#pragma unroll
    for (int k = 0; k < 8; ++k) x[k] = cast_extract<SDT, 2>(w, k);
    return true;
  }
}

// the two scale bytes a unit of 8 elements starting at tensor index t can
// meet: element k uses lo while (t % 32) + k < 32
__device__ __forceinline__ void mx_unit_scales(const MxSeg& g, uint64_t t,
                                               uint32_t& lo, uint32_t& hi) {
  const uint8_t* sc = reinterpret_cast<const uint8_t*>(g.scale_ptr);
  lo = sc[t / MX_BLOCK];
  hi = ((uint32_t)t & 31u) > 24u ? sc[(t + 7) / MX_BLOCK] : lo;
}

// body units [u0, u1) of a tile: those whose first element lies in
// [t0, t1), hd elements before unit 0, nb units in the segment
__device__ __forceinline__ void mx_tile_units(uint64_t hd, uint64_t nb,
                                              uint64_t t0, uint64_t t1,
                                              uint64_t& u0, uint64_t& u1) {
  u0 = t0 <= hd ? 0 : (t0 - hd + 7) / 8;
  u1 = t1 <= hd ? 0 : min(nb, (t1 - hd + 7) / 8);
}

template <uint32_t SDT, uint32_t FMT>
__device__ __forceinline__ void mx_store_tile(const MxSeg& g, uint8_t* dst,
                                              uint64_t t0, uint64_t t1) {
  constexpr int SS = SDT == DT_F32 ? 4 : 2;
  constexpr uint64_t EPB = FMT == MX_E2M1 ? 2 : 1;   // elements per byte
  const uint8_t* src = reinterpret_cast<const uint8_t*>(g.src);
  uint64_t n = g.rows * g.run;
  // unit stores are 8 (E4M3) or 4 (E2M1) aligned bytes
  uint64_t hd = FMT == MX_E2M1 ? ((0 - (uintptr_t)dst) & 3) * 2
                               : ((0 - (uintptr_t)dst) & 7);
  if (hd > n) hd = n;
  uint64_t nb = (n - hd) / 8, tail0 = hd + nb * 8, u0, u1;
  mx_tile_units(hd, nb, t0, t1, u0, u1);
  for (uint64_t u = u0 + threadIdx.x; u < u1; u += WG) {
    uint64_t e = hd + u * 8, r, c;
    mx_locate(g, e, r, c);
    uint32_t q[8];
    uint32_t x[8];
    if (c + 8 <= g.run &&
        mx_load_unit<SDT>(src + r * g.src_pitch + c * SS, x)) {
      uint64_t t = g.scale_e0 + r * g.scale_pitch + c;
      uint32_t lo, hi, split = 32u - ((uint32_t)t & 31u);
      mx_unit_scales(g, t, lo, hi);
#pragma unroll
      for (int k = 0; k < 8; ++k)
        q[k] = mx_quant(cvt_to_f32(x[k], SDT), (uint32_t)k < split ? lo : hi,
                        FMT);
    } else {
      for (int k = 0; k < 8; ++k) q[k] = mx_quant_at(g, src, e + k);
    }
    if constexpr (FMT == MX_E2M1) {
      uint32_t o = 0;
#pragma unroll
      for (int k = 0; k < 8; ++k) o |= q[k] << (4 * k);
      *reinterpret_cast<uint32_t*>(dst + e / 2) = o;
    } else {
      uint32_t o0 = 0, o1 = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        o0 |= q[k] << (8 * k);
        o1 |= q[k + 4] << (8 * k);
      }
      *reinterpret_cast<uint2*>(dst + e) = make_uint2(o0, o1);
    }
  }
  // head + tail: byte stores of distinct bytes, each by the tile that
  // holds the byte's first element
  uint64_t hb = hd / EPB, edge = hb + (n - tail0) / EPB;
  for (uint64_t i = threadIdx.x; i < edge; i += WG) {
    uint64_t e = (i < hb ? i : tail0 / EPB + (i - hb)) * EPB;
    if (e < t0 || e >= t1) continue;
    uint32_t b = mx_quant_at(g, src, e);
    if constexpr (FMT == MX_E2M1) b |= mx_quant_at(g, src, e + 1) << 4;
    dst[e / EPB] = (uint8_t)b;
  }
}

extern "C" __global__ __launch_bounds__(WG) void mx_store_kernel(
    uint8_t* __restrict__ base, const MxSeg* __restrict__ segs,
    const uint32_t* __restrict__ tile_seg, const uint64_t* __restrict__ tile_off,
    uint32_t n_tiles) {
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    MxSeg g = segs[tile_seg[tile]];
    uint64_t t0 = tile_off[tile];
    uint64_t t1 = min(t0 + (uint64_t)CAST_TILE, g.rows * g.run);
    uint8_t* dst = base + g.dst;
#define MX_CASE(S, F) \
  case (S) * 2u + (F): mx_store_tile<S, F>(g, dst, t0, t1); break;
    switch (g.dt * 2u + g.fmt) {
      MX_CASE(DT_F32, MX_E4M3) MX_CASE(DT_F32, MX_E2M1)
      MX_CASE(DT_F16, MX_E4M3) MX_CASE(DT_F16, MX_E2M1)
      MX_CASE(DT_BF16, MX_E4M3) MX_CASE(DT_BF16, MX_E2M1)
      default: break;   // host rejects every other pair before launch
    }
#undef MX_CASE
  }
}

template <uint32_t FMT, uint32_t DDT>
__device__ __forceinline__ void mx_load_tile(const MxSeg& g,
                                             const uint8_t* src, uint64_t t0,
                                             uint64_t t1) {
  constexpr int DS = DDT == DT_F32 ? 4 : 2;
  constexpr int NB = FMT == MX_E2M1 ? 4 : 8;         // source bytes per unit
  uint8_t* dst = reinterpret_cast<uint8_t*>(g.dst);
  uint64_t n = g.rows * g.run;
  uint64_t hd = ((0 - (uintptr_t)dst) & 15) / DS;    // to a 16-byte store
  if (hd > n) hd = n;
  uint64_t nb = (n - hd) / 8, tail0 = hd + nb * 8, u0, u1;
  mx_tile_units(hd, nb, t0, t1, u0, u1);
  for (uint64_t u = u0 + threadIdx.x; u < u1; u += WG) {
    uint64_t e = hd + u * 8, r, c;
    mx_locate(g, e, r, c);
    uint32_t f[8];
    bool fast = c + 8 <= g.run && (FMT == MX_E4M3 || (c & 1u) == 0);
    int mode = 0;
    const uint8_t* p = src + r * g.src_pitch + (FMT == MX_E2M1 ? c / 2 : c);
    if (fast) {
      mode = ((uintptr_t)p & (NB - 1)) == 0 ? 0
             : (((uintptr_t)p & 3) == 0 ? 1 : 2);
      // the shifted load reads up to 3 bytes past its unit: only where
      // the run still holds them
      if (mode == 2 && (g.run - c - 8) * mx_bits(FMT) / 8 < 3) fast = false;
    }
    if (fast) {
      uint32_t w[NB / 4];
      cast_load_words<NB / 4>(p, mode, w);
      uint64_t t = g.scale_e0 + r * g.scale_pitch + c;
      uint32_t lo, hi, split = 32u - ((uint32_t)t & 31u);
      mx_unit_scales(g, t, lo, hi);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        uint32_t code = FMT == MX_E2M1 ? (w[0] >> (4 * k)) & 0xFu
                                       : (w[k >> 2] >> ((k & 3) * 8)) & 0xFFu;
        f[k] = mx_dequant(code, (uint32_t)k < split ? lo : hi, FMT);
      }
    } else {
      for (int k = 0; k < 8; ++k) f[k] = mx_dequant_at(g, src, e + k);
    }
    if constexpr (DS == 4) {
      uint4* o = reinterpret_cast<uint4*>(dst + e * 4);
      o[0] = make_uint4(f[0], f[1], f[2], f[3]);
      o[1] = make_uint4(f[4], f[5], f[6], f[7]);
    } else {
      uint32_t o[4];
#pragma unroll
      for (int k = 0; k < 4; ++k)
        o[k] = cvt_from_f32(f[2 * k], DDT) |
               (cvt_from_f32(f[2 * k + 1], DDT) << 16);
      *reinterpret_cast<uint4*>(dst + e * 2) = make_uint4(o[0], o[1], o[2], o[3]);
    }
  }
  uint64_t edge = hd + (n - tail0);
  for (uint64_t i = threadIdx.x; i < edge; i += WG) {
    uint64_t e = i < hd ? i : tail0 + (i - hd);
    if (e < t0 || e >= t1) continue;
    mx_put(dst, e, mx_dequant_at(g, src, e), DDT);
  }
}

extern "C" __global__ __launch_bounds__(WG) void mx_load_kernel(
    const uint8_t* __restrict__ base, const MxSeg* __restrict__ segs,
    const uint32_t* __restrict__ tile_seg, const uint64_t* __restrict__ tile_off,
    uint32_t n_tiles) {
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    MxSeg g = segs[tile_seg[tile]];
    uint64_t t0 = tile_off[tile];
    uint64_t t1 = min(t0 + (uint64_t)CAST_TILE, g.rows * g.run);
    const uint8_t* src = base + g.src;
#define MX_CASE(F, D) \
  case (F) * 4u + (D): mx_load_tile<F, D>(g, src, t0, t1); break;
    switch (g.fmt * 4u + g.dt) {
      MX_CASE(MX_E4M3, DT_F32) MX_CASE(MX_E4M3, DT_F16) MX_CASE(MX_E4M3, DT_BF16)
      MX_CASE(MX_E2M1, DT_F32) MX_CASE(MX_E2M1, DT_F16) MX_CASE(MX_E2M1, DT_BF16)
      default: break;   // host rejects every other pair before launch
    }
#undef MX_CASE
  }
}

// Block scales of whole tensors: run is a multiple of 32 and tiles start
// on a multiple of 32, so the four lanes of a block (8 elements each) are
// adjacent, active together, and reduce with two cross-lane steps.
template <uint32_t SDT>
__device__ __forceinline__ void mx_scales_tile(const MxSeg& g, uint64_t t0,
                                               uint64_t t1) {
  constexpr int SS = SDT == DT_F32 ? 4 : 2;
  const uint8_t* src = reinterpret_cast<const uint8_t*>(g.src);
  uint8_t* out = reinterpret_cast<uint8_t*>(g.scale_ptr);
  for (uint64_t u = t0 / 8 + threadIdx.x; u < t1 / 8; u += WG) {
    uint64_t r, c;
    mx_locate(g, u * 8, r, c);
    uint32_t x[8], m = 0;
    if (!mx_load_unit<SDT>(src + r * g.src_pitch + c * SS, x))
      for (int k = 0; k < 8; ++k) x[k] = mx_src_bits(g, src, r, c + k);
#pragma unroll
    for (int k = 0; k < 8; ++k) m = max(m, absmax_key(x[k], SDT));
    m = max(m, (uint32_t)__shfl_xor((int)m, 1));
    m = max(m, (uint32_t)__shfl_xor((int)m, 2));
    if ((threadIdx.x & 3u) == 0)
      out[(g.scale_e0 + r * g.scale_pitch + c) / MX_BLOCK] =
          (uint8_t)mx_scale_of_amax(cvt_to_f32(m, SDT), g.fmt);
  }
}

extern "C" __global__ __launch_bounds__(WG) void mx_scales_kernel(
    const MxSeg* __restrict__ segs, const uint32_t* __restrict__ tile_seg,
    const uint64_t* __restrict__ tile_off, uint32_t n_tiles) {
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    MxSeg g = segs[tile_seg[tile]];
    uint64_t t0 = tile_off[tile];
    uint64_t t1 = min(t0 + (uint64_t)CAST_TILE, g.rows * g.run);
    switch (g.dt) {
      case DT_F32: mx_scales_tile<DT_F32>(g, t0, t1); break;
      case DT_F16: mx_scales_tile<DT_F16>(g, t0, t1); break;
      case DT_BF16: mx_scales_tile<DT_BF16>(g, t0, t1); break;
      default: break;   // host rejects every other source before launch
    }
  }
}

// ---------------------------------------------------------------------------
// Host twins: cpu tensors, host arenas and the byte path
// ---------------------------------------------------------------------------

static void mx_scales_segment_host(const MxSeg& g) {
  const uint8_t* src = reinterpret_cast<const uint8_t*>(g.src);
  uint8_t* out = reinterpret_cast<uint8_t*>(g.scale_ptr);
  for (uint64_t r = 0; r < g.rows; ++r)
    for (uint64_t c = 0; c < g.run; c += MX_BLOCK) {
      uint32_t m = 0;
      for (uint64_t k = 0; k < MX_BLOCK; ++k) {
        uint32_t key = absmax_key(mx_src_bits(g, src, r, c + k), g.dt);
        if (key > m) m = key;
      }
      out[(g.scale_e0 + r * g.scale_pitch + c) / MX_BLOCK] =
          (uint8_t)mx_scale_of_amax(cvt_to_f32(m, g.dt), g.fmt);
    }
}

// src: row 0 of the source; dst: the first destination byte
static void mx_store_segment_host(const uint8_t* src, uint8_t* dst,
                                  const MxSeg& g) {
  uint64_t n = g.rows * g.run;
  if (g.fmt == MX_E2M1) {
    for (uint64_t e = 0; e < n; e += 2)
      dst[e / 2] = (uint8_t)(mx_quant_at(g, src, e) |
                             (mx_quant_at(g, src, e + 1) << 4));
  } else {
    for (uint64_t e = 0; e < n; ++e) dst[e] = (uint8_t)mx_quant_at(g, src, e);
  }
}

// src: row 0 of the quantised source; dst: dense element 0
static void mx_load_segment_host(const uint8_t* src, uint8_t* dst,
                                 const MxSeg& g) {
  uint64_t n = g.rows * g.run;
  for (uint64_t e = 0; e < n; ++e)
    mx_put(dst, e, mx_dequant_at(g, src, e), g.dt);
}

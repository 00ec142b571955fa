// Typed tensor load and store for curvine_amd: optionally strided source ->
// dtype-converted dense destination.  Load (convert_segments_kernel): arena
// bytes -> torch tensor, safetensors weights living in the HBM cache land
// in torch parameters in one pass.  Store (store_segments_kernel): torch
// tensor or row-strided view -> arena bytes, a checkpoint's data section is
// written where it will be cached, with no host hop.
//
// One segment = `rows` runs of `run` contiguous source elements, the runs
// `src_pitch` bytes apart, written densely at the destination.  A load's
// source may sit at ANY byte alignment (the safetensors data section starts
// wherever the JSON header ends); a store's source is aligned to its own
// itemsize only (views with a storage offset, run starts inside a strided
// tensor).  The destination is aligned to its own itemsize but run
// boundaries inside it are not.
//
// Numerics: integer bit manipulation only, shared by the kernel and the
// host loop (`__host__ __device__`), bitwise equal to torch's CPU `.to()`:
// round-to-nearest-even downcasts, subnormals kept in both directions,
// overflow to inf, every narrow source widened exactly to f32 first so
// bf16<->f16 rounds once.  The scaled fp8 pairs (quantising store F32/F16/
// BF16 -> F8_E4M3, dequantising load back) add one IEEE f32 divide or
// multiply by the element's group scale; absmax_segments_kernel computes
// those scales from the same segments.
//
// Access pattern (memory-bound, no LDS): a unit is the element group whose
// wider side is 16 B, one unit per lane per pass, so both the load and the
// store instruction of a wave are contiguous.  Source tiers: vector load
// when the run start allows it, aligned dwords, aligned dwords + byte
// shift for odd offsets, byte loads for heads/tails/short runs.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <cstring>

#ifndef WG
#define WG 256
#endif

// dtype codes (mirrored by curvine_amd.native.DTYPES)
enum CastDt : uint32_t {
  DT_F32 = 0, DT_F16 = 1, DT_BF16 = 2, DT_F8_E4M3 = 3, DT_F8_E5M2 = 4,
  DT_F64 = 5, DT_I64 = 6, DT_I32 = 7, DT_I16 = 8, DT_I8 = 9, DT_U8 = 10,
  DT_BOOL = 11, DT_U16 = 12, DT_U32 = 13, DT_U64 = 14, DT_COUNT = 15
};

__host__ __device__ inline uint32_t cast_itemsize(uint32_t dt) {
  switch (dt) {
    case DT_F64: case DT_I64: case DT_U64: return 8;
    case DT_F32: case DT_I32: case DT_U32: return 4;
    case DT_F16: case DT_BF16: case DT_I16: case DT_U16: return 2;
    default: return 1;
  }
}

// a converting pair: narrow/wide float source, F32/F16/BF16 destination
__host__ __device__ inline bool cast_pair_converts(uint32_t s, uint32_t d) {
  return s != d && s <= DT_F8_E5M2 && d <= DT_BF16;
}

// ---------------------------------------------------------------------------
// Scalar conversions on raw bit patterns (the ONE definition; host + device)
// ---------------------------------------------------------------------------

__host__ __device__ inline uint32_t cvt_f16_to_f32(uint32_t h) {
  uint32_t sign = (h & 0x8000u) << 16;
  uint32_t e = (h >> 10) & 31u, m = h & 0x3FFu;
  if (e == 31u) return sign | 0x7F800000u | (m << 13);
  if (e == 0u) {
    if (m == 0u) return sign;
    // subnormal m * 2^-24: top set bit p -> 2^(p-24) * 1.x
    uint32_t p = 31u - (uint32_t)__builtin_clz(m);
    return sign | ((p + 103u) << 23) | ((m << (23u - p)) & 0x7FFFFFu);
  }
  return sign | ((e + 112u) << 23) | (m << 13);
}

__host__ __device__ inline uint32_t cvt_f8e4m3_to_f32(uint32_t b) {
  uint32_t sign = (b & 0x80u) << 24;
  uint32_t e = (b >> 3) & 15u, m = b & 7u;
  if (e == 15u && m == 7u) return sign | 0x7FC00000u;   // the only NaN, no inf
  if (e == 0u) {
    if (m == 0u) return sign;
    uint32_t p = 31u - (uint32_t)__builtin_clz(m);      // m * 2^-9
    return sign | ((p + 118u) << 23) | ((m << (23u - p)) & 0x7FFFFFu);
  }
  return sign | ((e + 120u) << 23) | (m << 20);
}

// widen any supported float source to exact f32 bits
__host__ __device__ inline uint32_t cvt_to_f32(uint32_t bits, uint32_t sdt) {
  switch (sdt) {
    case DT_F16: return cvt_f16_to_f32(bits);
    case DT_BF16: return bits << 16;
    case DT_F8_E4M3: return cvt_f8e4m3_to_f32(bits);
    case DT_F8_E5M2: return cvt_f16_to_f32(bits << 8);  // e5m2 = top byte of f16
    default: return bits;
  }
}

__host__ __device__ inline uint32_t cvt_f32_to_bf16(uint32_t u) {
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return ((u >> 16) & 0x8000u) | 0x7FC0u;
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;   // RNE; inf/subnormal safe
}

__host__ __device__ inline uint32_t cvt_f32_to_f16(uint32_t u) {
  uint32_t sign = (u >> 16) & 0x8000u;
  uint32_t a = u & 0x7FFFFFFFu;
  if (a >= 0x7F800000u) return sign | (a > 0x7F800000u ? 0x7E00u : 0x7C00u);
  if (a >= 0x47800000u) return sign | 0x7C00u;          // >= 65536
  if (a < 0x38800000u) {                                // < 2^-14: subnormal out
    if (a <= 0x33000000u) return sign;                  // <= 2^-25 (tie -> even 0)
    uint32_t e = a >> 23;                               // 102..112
    uint32_t m = (a & 0x7FFFFFu) | 0x800000u;
    uint32_t sh = 126u - e;                             // 14..24
    uint32_t r = m >> sh, rem = m & ((1u << sh) - 1u), half = 1u << (sh - 1u);
    if (rem > half || (rem == half && (r & 1u))) r++;   // may carry to 0x0400
    return sign | r;
  }
  uint32_t r = a - 0x38000000u;                         // rebias 127 -> 15
  r += 0xFFFu + ((r >> 13) & 1u);                       // RNE; 65520 -> inf
  return sign | (r >> 13);
}

__host__ __device__ inline uint32_t cvt_from_f32(uint32_t f, uint32_t ddt) {
  switch (ddt) {
    case DT_F16: return cvt_f32_to_f16(f);
    case DT_BF16: return cvt_f32_to_bf16(f);
    default: return f;
  }
}

// f32 -> OCP e4m3, saturating: RNE, subnormals kept (smallest 2^-9, exactly
// 2^-10 ties to 0), |x| >= 448 and inf give +-448, NaN gives 0x7F | sign.
// Bitwise torch CPU's x.clamp(-448, 448).to(torch.float8_e4m3fn).
__host__ __device__ inline uint32_t cvt_f32_to_f8e4m3_sat(uint32_t u) {
  uint32_t sign = (u >> 24) & 0x80u;
  uint32_t a = u & 0x7FFFFFFFu;
  if (a > 0x7F800000u) return sign | 0x7Fu;
  if (a >= 0x43E00000u) return sign | 0x7Eu;            // >= 448
  if (a < 0x3C800000u) {                                // < 2^-6: subnormal out
    if (a <= 0x3A800000u) return sign;                  // <= 2^-10 (tie -> even 0)
    uint32_t e = a >> 23;                               // 117..120
    uint32_t m = (a & 0x7FFFFFu) | 0x800000u;
    uint32_t sh = 141u - e;                             // 21..24
    uint32_t r = m >> sh, rem = m & ((1u << sh) - 1u), half = 1u << (sh - 1u);
    if (rem > half || (rem == half && (r & 1u))) r++;   // may carry to 0x08
    return sign | r;
  }
  uint32_t r = a - 0x3C000000u;                         // rebias 127 -> 7
  r += 0x7FFFFu + ((r >> 20) & 1u);                     // RNE; tops out at 0x7E
  return sign | (r >> 20);
}

// a quantising pair: F32/F16/BF16 -> F8_E4M3, always with a scale
__host__ __device__ inline bool cast_pair_quantizes(uint32_t s, uint32_t d) {
  return s <= DT_BF16 && d == DT_F8_E4M3;
}
// a pair that takes a scale on load: F8_E4M3 -> F32/F16/BF16
__host__ __device__ inline bool cast_pair_dequantizes(uint32_t s, uint32_t d) {
  return s == DT_F8_E4M3 && d <= DT_BF16;
}

__host__ __device__ inline float cast_f32_of(uint32_t u) {
  return __builtin_bit_cast(float, u);
}
__host__ __device__ inline uint32_t cast_bits_of(float f) {
  return __builtin_bit_cast(uint32_t, f);
}

// scale of a group from the bits of its amax (largest finite |x|):
// max(amax, 2^-40) / 448, so an all-zero, all-NaN or all-inf group gets
// 2^-40/448 and no scale is ever denormal
__host__ __device__ inline uint32_t cast_scale_of_amax(uint32_t amax_bits) {
  float a = cast_f32_of(amax_bits < 0x2B800000u ? 0x2B800000u : amax_bits);
  return cast_bits_of(a / 448.0f);
}

// the scaled element: one correctly rounded f32 divide (quantise) or
// multiply (dequantise) around the integer conversions.  No reciprocal:
// it would change bits.
__host__ __device__ inline uint32_t cvt_scaled(uint32_t bits, uint32_t sdt,
                                               uint32_t ddt, float scale) {
  uint32_t f = cvt_to_f32(bits, sdt);
  if (ddt == DT_F8_E4M3)
    return cvt_f32_to_f8e4m3_sat(cast_bits_of(cast_f32_of(f) / scale));
  return cvt_from_f32(cast_bits_of(cast_f32_of(f) * scale), ddt);
}

// |x| of a source element as an order-preserving key in its own format
// (widening is monotonic on non-negative finite values, so the max is taken
// on keys and widened once); 0 for NaN and inf, which the amax skips
__host__ __device__ inline uint32_t absmax_key(uint32_t bits, uint32_t sdt) {
  if (sdt == DT_F32) {
    uint32_t a = bits & 0x7FFFFFFFu;
    return a > 0x7F7FFFFFu ? 0u : a;
  }
  uint32_t a = bits & 0x7FFFu;
  return a > (sdt == DT_F16 ? 0x7BFFu : 0x7F7Fu) ? 0u : a;
}

// one element, byte loads, store at the destination itemsize
__host__ __device__ inline void cast_one(const uint8_t* s, uint8_t* d,
                                         uint32_t sdt, uint32_t ddt) {
  uint32_t ss = cast_itemsize(sdt);
  uint32_t bits = 0;
  for (uint32_t i = 0; i < ss; ++i) bits |= (uint32_t)s[i] << (8u * i);
  uint32_t out = cvt_from_f32(cvt_to_f32(bits, sdt), ddt);
  if (ddt == DT_F32) *reinterpret_cast<uint32_t*>(d) = out;
  else *reinterpret_cast<uint16_t*>(d) = (uint16_t)out;
}

// the same for a scaled pair (1-byte store when quantising)
__host__ __device__ inline void cast_one_scaled(const uint8_t* s, uint8_t* d,
                                                uint32_t sdt, uint32_t ddt,
                                                float scale) {
  uint32_t ss = cast_itemsize(sdt);
  uint32_t bits = 0;
  for (uint32_t i = 0; i < ss; ++i) bits |= (uint32_t)s[i] << (8u * i);
  uint32_t out = cvt_scaled(bits, sdt, ddt, scale);
  if (ddt == DT_F32) *reinterpret_cast<uint32_t*>(d) = out;
  else if (ddt == DT_F8_E4M3) *d = (uint8_t)out;
  else *reinterpret_cast<uint16_t*>(d) = (uint16_t)out;
}

// ---------------------------------------------------------------------------
// Kernel
// ---------------------------------------------------------------------------

struct CastSeg {
  uint64_t src_off;     // load: bytes into the arena, any alignment;
                        // store: absolute source address of row 0
  uint64_t dst_ptr;     // load: absolute address of dense element 0;
                        // store: bytes into the arena
  uint64_t rows, run;   // rows runs of run elements
  uint64_t src_pitch;   // bytes between run starts in the source
  uint32_t src_dt, dst_dt;
  uint64_t scale_ptr;   // absolute address of the f32 group scales, 0 = unscaled
  uint64_t scale_every; // dense elements per group, 0 = one group
  uint64_t scale_e0;    // dense index of element 0 within its tensor: dense
                        // element e uses scale (scale_e0 + e) / scale_every
};

__host__ __device__ inline uint64_t cast_group_of(uint64_t every, uint64_t e0,
                                                  uint64_t e) {
  return every ? (e0 + e) / every : 0;
}

// dense destination elements per workgroup tile; same-dtype copies are
// flattened to bytes by the host and tile at 64 KiB like copy_extents_kernel
#define CAST_TILE 16384
__host__ __device__ inline uint64_t cast_tile_elems(uint32_t sdt, uint32_t ddt) {
  return sdt == ddt ? 4u * CAST_TILE : CAST_TILE;
}
// runs shorter than this are handled element-wise with div/mod
#define CAST_SHORT_RUN 64

// load W dwords of source for one unit. mode 0: natural vector alignment,
// 1: 4-byte aligned, 2: unaligned (aligned dwords + byte funnel shift; reads
// the aligned dword that holds p's byte, so up to 3 bytes before p, and up
// to 3 bytes past the unit).  Guarantee of cast_run, which holds for an
// absolute source (a torch tensor) as for an arena offset: before a run at
// most the aligned dword that holds the run's first byte is touched, which
// lies in the same allocation and page as that byte; past the run's last
// byte nothing is touched.
template <int W>
__device__ __forceinline__ void cast_load_words(const uint8_t* p, int mode,
                                                uint32_t (&w)[W]) {
  if (mode == 0) {
    if constexpr (W == 4) {
      uint4 v = *reinterpret_cast<const uint4*>(p);
      w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else if constexpr (W == 2) {
      uint2 v = *reinterpret_cast<const uint2*>(p);
      w[0] = v.x; w[1] = v.y;
    } else {
      w[0] = *reinterpret_cast<const uint32_t*>(p);
    }
  } else if (mode == 1) {
    const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
    for (int i = 0; i < W; ++i) w[i] = q[i];
  } else {
    uint32_t sh = ((uint32_t)(uintptr_t)p & 3u) * 8u;   // 8, 16 or 24
    const uint32_t* q = reinterpret_cast<const uint32_t*>(
        (uintptr_t)p & ~(uintptr_t)3);
    uint32_t t[W + 1];
#pragma unroll
    for (int i = 0; i <= W; ++i) t[i] = q[i];
#pragma unroll
    for (int i = 0; i < W; ++i) w[i] = (t[i] >> sh) | (t[i + 1] << (32u - sh));
  }
}

template <int OW>
__device__ __forceinline__ void cast_store_words(uint8_t* p,
                                                 const uint32_t (&o)[OW]) {
  if constexpr (OW == 4) {
    *reinterpret_cast<uint4*>(p) = make_uint4(o[0], o[1], o[2], o[3]);
  } else if constexpr (OW == 2) {
    *reinterpret_cast<uint2*>(p) = make_uint2(o[0], o[1]);
  } else {
    *reinterpret_cast<uint32_t*>(p) = o[0];
  }
}

template <uint32_t SDT, int SS>
__device__ __forceinline__ uint32_t cast_extract(const uint32_t* w, int k) {
  if constexpr (SS == 4) return w[k];
  else if constexpr (SS == 2) return (w[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu;
  else return (w[k >> 2] >> ((k & 3) * 8)) & 0xFFu;
}

// one contiguous run of n elements, all WG threads cooperating.
// SDT == DDT == DT_U8 is the raw byte copy.  SC: a scaled pair, the whole
// run in one scale group.  A quantising run has a 1-byte destination: K is
// 4 (F32 source, one dword store per lane) or 8 (16-bit source, uint2
// store), the head runs up to the first 4- or 8-byte aligned destination
// byte, and head and tail are byte stores of distinct bytes.
template <uint32_t SDT, uint32_t DDT, bool SC>
__device__ __forceinline__ void cast_run(const uint8_t* s, uint8_t* d,
                                         uint64_t n, float scale) {
  constexpr bool COPY = (SDT == DDT);
  constexpr int SS = COPY ? 1 : (SDT == DT_F32 ? 4 : (SDT <= DT_BF16 ? 2 : 1));
  constexpr int DS = COPY ? 1 : (DDT == DT_F32 ? 4 : (DDT == DT_F8_E4M3 ? 1 : 2));
  constexpr int K = 16 / (SS > DS ? SS : DS);   // elements per unit
  constexpr int W = K * SS / 4;                 // source dwords per unit
  constexpr int OW = K * DS / 4;                // destination dwords per unit

  // head: up to the first destination address aligned to the unit store
  uint64_t hd = ((0 - (uintptr_t)d) & (uintptr_t)(K * DS - 1)) / DS;
  if (hd > n) hd = n;
  uint64_t nb = (n - hd) / K;
  const uint8_t* sb = s + hd * SS;
  int mode = ((uintptr_t)sb & (W * 4 - 1)) == 0 ? 0
             : (((uintptr_t)sb & 3) == 0 ? 1 : 2);
  // the shifted loads over-read up to 3 bytes past their unit: keep the
  // last unit out of the body, so those bytes belong to the unit after it
  // and nothing past the run's last byte is read
  if (mode == 2 && nb > 0) nb--;
  uint64_t tail0 = hd + nb * K;

  for (uint64_t u = threadIdx.x; u < nb; u += WG) {
    uint32_t w[W], o[OW];
    cast_load_words<W>(sb + u * (K * SS), mode, w);
    if constexpr (COPY) {
#pragma unroll
      for (int i = 0; i < OW; ++i) o[i] = w[i];
    } else {
#pragma unroll
      for (int k = 0; k < K; ++k) {
        uint32_t x = cast_extract<SDT, SS>(w, k), r;
        if constexpr (SC) r = cvt_scaled(x, SDT, DDT, scale);
        else r = cvt_from_f32(cvt_to_f32(x, SDT), DDT);
        if constexpr (DS == 4) o[k] = r;
        else if constexpr (DS == 2) {
          if ((k & 1) == 0) o[k >> 1] = r;
          else o[k >> 1] |= r << 16;
        } else {
          if ((k & 3) == 0) o[k >> 2] = r;
          else o[k >> 2] |= r << ((k & 3) * 8);
        }
      }
    }
    cast_store_words<OW>(d + (hd + u * K) * DS, o);
  }
  // head + tail: at most 3*K elements, byte loads, element stores
  uint64_t edge = hd + (n - tail0);
  for (uint64_t i = threadIdx.x; i < edge; i += WG) {
    uint64_t e = i < hd ? i : tail0 + (i - hd);
    if constexpr (COPY) d[e] = s[e];
    else if constexpr (SC) cast_one_scaled(s + e * SS, d + e * DS, SDT, DDT, scale);
    else cast_one(s + e * SS, d + e * DS, SDT, DDT);
  }
}

template <uint32_t SDT, uint32_t DDT, bool SC>
__device__ __forceinline__ void cast_tile(const uint8_t* src, uint8_t* dst,
                                          const CastSeg& g, uint64_t t0,
                                          uint64_t t1) {
  constexpr bool COPY = (SDT == DDT);
  constexpr uint32_t SS = COPY ? 1 : (SDT == DT_F32 ? 4 : (SDT <= DT_BF16 ? 2 : 1));
  constexpr uint32_t DS = COPY ? 1 : (DDT == DT_F32 ? 4 : (DDT == DT_F8_E4M3 ? 1 : 2));
  const float* scales = reinterpret_cast<const float*>(g.scale_ptr);
  // groups shorter than a short run (row scales of a narrow tensor) go
  // element-wise too: one scale fetch per element
  bool by_run = g.run >= CAST_SHORT_RUN;
  if constexpr (SC)
    by_run = by_run && (g.scale_every == 0 || g.scale_every >= CAST_SHORT_RUN);
  if (by_run) {
    uint64_t e = t0;
    while (e < t1) {                       // workgroup-uniform loop
      uint64_t r = e / g.run, c = e - r * g.run;
      uint64_t len = min(g.run - c, t1 - e);
      float scale = 1.0f;
      if constexpr (SC) {
        // a run is cut where its scale group ends (a collapsed layout has
        // runs longer than a row): one scale fetch per piece
        uint64_t grp = cast_group_of(g.scale_every, g.scale_e0, e);
        if (g.scale_every)
          len = min(len, (grp + 1) * g.scale_every - (g.scale_e0 + e));
        scale = scales[grp];
      }
      cast_run<SDT, DDT, SC>(src + r * g.src_pitch + c * SS, dst + e * DS, len,
                             scale);
      e += len;
    }
  } else {
    // many short runs: element-wise, one div per element
    for (uint64_t e = t0 + threadIdx.x; e < t1; e += WG) {
      uint64_t r = e / g.run, c = e - r * g.run;
      const uint8_t* sp = src + r * g.src_pitch + c * SS;
      if constexpr (COPY) dst[e] = *sp;
      else if constexpr (SC)
        cast_one_scaled(sp, dst + e * DS, SDT, DDT,
                        scales[cast_group_of(g.scale_every, g.scale_e0, e)]);
      else cast_one(sp, dst + e * DS, SDT, DDT);
    }
  }
}

// Tile table as in copy_extents_kernel: tile -> segment, tile -> first dense
// element; grid-stride over tiles so one huge embedding and 300
// norm vectors in the same call spread evenly over the CUs.  `src` and
// `dst` are the segment's row 0 and dense element 0.
__device__ __forceinline__ void cast_segment_tiles(
    const uint8_t* src, uint8_t* dst, const CastSeg& g, uint64_t t0) {
  uint64_t t1 = min(t0 + cast_tile_elems(g.src_dt, g.dst_dt), g.rows * g.run);
#define CAST_CASE(S, D) \
  case (S) * 16u + (D): cast_tile<S, D, false>(src, dst, g, t0, t1); break;
#define CAST_CASE_SCALED(S, D) \
  case 256u + (S) * 16u + (D): cast_tile<S, D, true>(src, dst, g, t0, t1); break;
  switch ((g.scale_ptr ? 256u : 0u) + g.src_dt * 16u + g.dst_dt) {
    CAST_CASE_SCALED(DT_F32, DT_F8_E4M3) CAST_CASE_SCALED(DT_F16, DT_F8_E4M3)
    CAST_CASE_SCALED(DT_BF16, DT_F8_E4M3)
    CAST_CASE_SCALED(DT_F8_E4M3, DT_F32) CAST_CASE_SCALED(DT_F8_E4M3, DT_F16)
    CAST_CASE_SCALED(DT_F8_E4M3, DT_BF16)
    CAST_CASE(DT_U8, DT_U8)
    CAST_CASE(DT_F32, DT_F16) CAST_CASE(DT_F32, DT_BF16)
    CAST_CASE(DT_F16, DT_F32) CAST_CASE(DT_F16, DT_BF16)
    CAST_CASE(DT_BF16, DT_F32) CAST_CASE(DT_BF16, DT_F16)
    CAST_CASE(DT_F8_E4M3, DT_F32) CAST_CASE(DT_F8_E4M3, DT_F16)
    CAST_CASE(DT_F8_E4M3, DT_BF16)
    CAST_CASE(DT_F8_E5M2, DT_F32) CAST_CASE(DT_F8_E5M2, DT_F16)
    CAST_CASE(DT_F8_E5M2, DT_BF16)
    default: break;   // host rejects every other pair before launch
  }
#undef CAST_CASE
#undef CAST_CASE_SCALED
}

extern "C" __global__ __launch_bounds__(WG) void convert_segments_kernel(
    const uint8_t* __restrict__ base, const CastSeg* __restrict__ segs,
    const uint32_t* __restrict__ tile_seg, const uint64_t* __restrict__ tile_off,
    uint32_t n_tiles) {
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    CastSeg g = segs[tile_seg[tile]];
    cast_segment_tiles(base + g.src_off, reinterpret_cast<uint8_t*>(g.dst_ptr),
                       g, tile_off[tile]);
  }
}

// The scatter direction: absolute sources (src_off holds the address),
// dense destinations at dst_ptr bytes into the arena at `base`.
extern "C" __global__ __launch_bounds__(WG) void store_segments_kernel(
    uint8_t* __restrict__ base, const CastSeg* __restrict__ segs,
    const uint32_t* __restrict__ tile_seg, const uint64_t* __restrict__ tile_off,
    uint32_t n_tiles) {
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    CastSeg g = segs[tile_seg[tile]];
    cast_segment_tiles(reinterpret_cast<const uint8_t*>(g.src_off),
                       base + g.dst_ptr, g, tile_off[tile]);
  }
}

// host arena: the same segments, the same scalar routines, plain loops
static void cast_segment_host(const uint8_t* src, uint8_t* dst,
                              const CastSeg& g) {
  uint32_t ss = cast_itemsize(g.src_dt), ds = cast_itemsize(g.dst_dt);
  for (uint64_t r = 0; r < g.rows; ++r) {
    const uint8_t* s = src + r * g.src_pitch;
    uint8_t* d = dst + r * g.run * ds;
    if (g.src_dt == g.dst_dt) {
      std::memcpy(d, s, g.run * ss);
      continue;
    }
    if (g.scale_ptr) {
      const float* scales = reinterpret_cast<const float*>(g.scale_ptr);
      for (uint64_t c = 0; c < g.run; ++c)
        cast_one_scaled(
            s + c * ss, d + c * ds, g.src_dt, g.dst_dt,
            scales[cast_group_of(g.scale_every, g.scale_e0, r * g.run + c)]);
      continue;
    }
    for (uint64_t c = 0; c < g.run; ++c)
      cast_one(s + c * ss, d + c * ds, g.src_dt, g.dst_dt);
  }
}

static void convert_segment_host(const uint8_t* base, const CastSeg& g) {
  cast_segment_host(base + g.src_off, reinterpret_cast<uint8_t*>(g.dst_ptr), g);
}

// host arena, CPU source: src_off is the absolute source address
static void store_segment_host(uint8_t* base, const CastSeg& g) {
  cast_segment_host(reinterpret_cast<const uint8_t*>(g.src_off),
                    base + g.dst_ptr, g);
}

// ---------------------------------------------------------------------------
// absmax: the group scales a quantising store divides by
// ---------------------------------------------------------------------------
//
// The same rows-of-runs segments at an absolute address, reduced instead of
// stored.  Dense element e of a segment belongs to group
// (scale_e0 + e) / scale_every of its tensor, whose f32 slot is
// out_ptr[group].  The slots are zeroed first, hold the bits of the group's
// amax after absmax_segments_kernel (non-negative f32 patterns order as
// unsigned integers and max is order-independent: deterministic), and are
// turned into scales in place by scale_slots_kernel on the same stream.

struct AbsmaxSeg {
  uint64_t src_ptr;     // absolute address of row 0, aligned to the itemsize
  uint64_t rows, run;   // rows runs of run elements
  uint64_t src_pitch;   // bytes between run starts
  uint64_t out_ptr;     // absolute address of the tensor's f32 group slots
  uint64_t scale_every; // dense elements per group, 0 = one group
  uint64_t scale_e0;    // dense index of element 0 within its tensor
  uint32_t src_dt, pad;
};

struct ScaleSlots {
  uint64_t ptr, n;      // n f32 slots at ptr
};

// per-thread max of the keys of one contiguous run, all WG threads
// cooperating: 16-byte loads from the first 16-byte aligned source byte,
// element loads for the head and the tail.  Reads the run's bytes only.
template <uint32_t SDT>
__device__ __forceinline__ uint32_t absmax_run(const uint8_t* s, uint64_t n,
                                               uint32_t m) {
  constexpr int SS = SDT == DT_F32 ? 4 : 2;
  constexpr int K = 16 / SS;
  uint64_t hd = ((0 - (uintptr_t)s) & (uintptr_t)15) / SS;
  if (hd > n) hd = n;
  uint64_t nb = (n - hd) / K;
  const uint8_t* sb = s + hd * SS;
  for (uint64_t u = threadIdx.x; u < nb; u += WG) {
    uint32_t w[4];
    cast_load_words<4>(sb + u * 16, 0, w);
#pragma unroll
    for (int k = 0; k < K; ++k)
      m = max(m, absmax_key(cast_extract<SDT, SS>(w, k), SDT));
  }
  uint64_t tail0 = hd + nb * K;
  uint64_t edge = hd + (n - tail0);
  for (uint64_t i = threadIdx.x; i < edge; i += WG) {
    uint64_t e = i < hd ? i : tail0 + (i - hd);
    uint32_t x;
    if constexpr (SS == 4) x = *reinterpret_cast<const uint32_t*>(s + e * 4);
    else x = *reinterpret_cast<const uint16_t*>(s + e * 2);
    m = max(m, absmax_key(x, SDT));
  }
  return m;
}

// lanes -> wave (cross-lane) -> workgroup (LDS) -> one atomicMax on the slot
__device__ __forceinline__ void absmax_commit(uint32_t m, uint32_t sdt,
                                              uint32_t* slot, uint32_t* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
  __syncthreads();                         // the previous commit has read lds
  if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = m;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < WG / 64; ++w) m = max(m, lds[w]);
    if (m) atomicMax(slot, cvt_to_f32(m, sdt));   // slots start at zero
  }
}

template <uint32_t SDT>
__device__ __forceinline__ void absmax_tile(const AbsmaxSeg& g, uint64_t t0,
                                            uint64_t t1, uint32_t* lds) {
  constexpr uint32_t SS = SDT == DT_F32 ? 4 : 2;
  const uint8_t* src = reinterpret_cast<const uint8_t*>(g.src_ptr);
  uint32_t* out = reinterpret_cast<uint32_t*>(g.out_ptr);
  if (g.run >= CAST_SHORT_RUN &&
      (g.scale_every == 0 || g.scale_every >= CAST_SHORT_RUN)) {
    uint64_t e = t0, cur = cast_group_of(g.scale_every, g.scale_e0, e);
    uint32_t m = 0;
    while (e < t1) {                       // workgroup-uniform loop
      uint64_t r = e / g.run, c = e - r * g.run;
      uint64_t len = min(g.run - c, t1 - e);
      uint64_t grp = cast_group_of(g.scale_every, g.scale_e0, e);
      if (g.scale_every)
        len = min(len, (grp + 1) * g.scale_every - (g.scale_e0 + e));
      if (grp != cur) {
        absmax_commit(m, SDT, out + cur, lds);
        m = 0;
        cur = grp;
      }
      m = absmax_run<SDT>(src + r * g.src_pitch + c * SS, len, m);
      e += len;
    }
    absmax_commit(m, SDT, out + cur, lds);
  } else {
    // short runs or short groups: element-wise, one atomic per lane per
    // group it meets (groups only grow along a lane's elements)
    uint64_t cur = 0;
    uint32_t m = 0;
    for (uint64_t e = t0 + threadIdx.x; e < t1; e += WG) {
      uint64_t r = e / g.run, c = e - r * g.run;
      const uint8_t* sp = src + r * g.src_pitch + c * SS;
      uint32_t x;
      if constexpr (SS == 4) x = *reinterpret_cast<const uint32_t*>(sp);
      else x = *reinterpret_cast<const uint16_t*>(sp);
      uint64_t grp = cast_group_of(g.scale_every, g.scale_e0, e);
      if (grp != cur) {
        if (m) atomicMax(out + cur, cvt_to_f32(m, SDT));
        m = 0;
        cur = grp;
      }
      m = max(m, absmax_key(x, SDT));
    }
    if (m) atomicMax(out + cur, cvt_to_f32(m, SDT));
  }
}

extern "C" __global__ __launch_bounds__(WG) void absmax_segments_kernel(
    const AbsmaxSeg* __restrict__ segs, const uint32_t* __restrict__ tile_seg,
    const uint64_t* __restrict__ tile_off, uint32_t n_tiles) {
  __shared__ uint32_t lds[WG / 64];
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    AbsmaxSeg g = segs[tile_seg[tile]];
    uint64_t t0 = tile_off[tile];
    uint64_t t1 = min(t0 + (uint64_t)CAST_TILE, g.rows * g.run);
    switch (g.src_dt) {
      case DT_F32: absmax_tile<DT_F32>(g, t0, t1, lds); break;
      case DT_F16: absmax_tile<DT_F16>(g, t0, t1, lds); break;
      case DT_BF16: absmax_tile<DT_BF16>(g, t0, t1, lds); break;
      default: break;   // host rejects every other source before launch
    }
  }
}

// finish == 0: zero the slots; finish != 0: amax bits -> scale bits in place
extern "C" __global__ __launch_bounds__(WG) void scale_slots_kernel(
    const ScaleSlots* __restrict__ ranges, uint32_t n_ranges, int finish) {
  for (uint32_t i = blockIdx.x; i < n_ranges; i += gridDim.x) {
    uint32_t* p = reinterpret_cast<uint32_t*>(ranges[i].ptr);
    for (uint64_t k = threadIdx.x; k < ranges[i].n; k += WG)
      p[k] = finish ? cast_scale_of_amax(p[k]) : 0u;
  }
}

// host twins: cpu tensors and host arenas
static void absmax_segment_host(const AbsmaxSeg& g) {
  uint32_t ss = cast_itemsize(g.src_dt);
  uint32_t* out = reinterpret_cast<uint32_t*>(g.out_ptr);
  for (uint64_t r = 0; r < g.rows; ++r) {
    const uint8_t* s = reinterpret_cast<const uint8_t*>(g.src_ptr) +
                       r * g.src_pitch;
    for (uint64_t c = 0; c < g.run; ++c) {
      uint32_t bits = 0;
      for (uint32_t i = 0; i < ss; ++i)
        bits |= (uint32_t)s[c * ss + i] << (8u * i);
      uint32_t a = cvt_to_f32(absmax_key(bits, g.src_dt), g.src_dt);
      uint32_t* slot =
          out + cast_group_of(g.scale_every, g.scale_e0, r * g.run + c);
      if (a > *slot) *slot = a;
    }
  }
}

static void scale_slots_host(const ScaleSlots& r, bool finish) {
  uint32_t* p = reinterpret_cast<uint32_t*>(r.ptr);
  for (uint64_t k = 0; k < r.n; ++k)
    p[k] = finish ? cast_scale_of_amax(p[k]) : 0u;
}

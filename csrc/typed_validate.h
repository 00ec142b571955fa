// Argument checks of the typed load, store and scale entry points
// (typed_io.cpp): everything between the integers a caller passes and the
// kernels and host loops that dereference them.  Pure C++ over the host
// helpers of tensor_cast.hip, mx_cast.hip and block_cast.hip, which are
// included before this file: no pybind11 and no HIP runtime call, so a
// stand-alone program can drive it (scripts/typed_validate_sweep.cpp).
// Every refusal is a std::invalid_argument reading "<who>: <what>".

#pragma once

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

[[noreturn]] static void typed_reject(const char* who, const char* what) {
  throw std::invalid_argument(std::string(who) + ": " + what);
}

// end = base + (rows - 1) * pitch + run, rows >= 1: the byte past a strided
// range, or the element past a segment in its tensor.  True when it wraps.
static bool span_overflows(uint64_t base, uint64_t rows, uint64_t pitch,
                           uint64_t run, uint64_t* end) {
  uint64_t span;
  return __builtin_mul_overflow(rows - 1, pitch, &span) ||
         __builtin_add_overflow(span, run, &span) ||
         __builtin_add_overflow(base, span, end);
}

// ---- plain and group-scaled segments (tensor_cast.hip) ----
//
// Load: (src_off, dst_ptr, rows, run, src_pitch, src_dtype, dst_dtype), the
// source an arena offset, the destination an absolute address.  Store: the
// scatter direction, (src_ptr, dst_off, ...).  A 10-tuple appends
// (scale_ptr, scale_every, scale_e0): F8_E4M3 <-> F32/F16/BF16 under the f32
// scale of each dense element's group.

enum CastKind { CAST_LOAD, CAST_STORE };

// segment fields as they arrive from Python: 7 without, 10 with a scale
struct SegArgs {
  uint64_t a, b, rows, run, pitch, sdt, ddt;
  uint64_t scale_ptr = 0, scale_every = 0, scale_e0 = 0;
};

// The scale fields against the dtype pair (codes already range-checked):
// a quantising pair needs a scale, F8_E4M3 -> F32/F16/BF16 takes one or is
// the plain upcast, no other pair takes one.  Returns false when the pair
// is not a scaled one, for the caller's own pair check.
static bool scale_validate(const char* who, const SegArgs& s, uint64_t total,
                           bool quant_ok, bool dequant_ok) {
  bool quant = cast_pair_quantizes((uint32_t)s.sdt, (uint32_t)s.ddt);
  bool dequant = cast_pair_dequantizes((uint32_t)s.sdt, (uint32_t)s.ddt);
  if (!s.scale_ptr) {
    if (quant && quant_ok)
      typed_reject(who, "unsupported dtype pair without a scale_ptr");
    return false;
  }
  if (!((quant && quant_ok) || (dequant && dequant_ok)))
    typed_reject(who, "scale_ptr on a dtype pair that takes none");
  if (s.scale_ptr % 4) typed_reject(who, "scale_ptr misaligned");
  uint64_t last, bytes, end;
  if (__builtin_add_overflow(s.scale_e0, total, &last) ||
      __builtin_mul_overflow(s.scale_every ? last / s.scale_every + 1 : 1,
                             (uint64_t)4, &bytes) ||
      __builtin_add_overflow(s.scale_ptr, bytes, &end))
    typed_reject(who, "scale range overflows");
  return true;
}

// [first, last) bytes of the scales a validated scaled segment reads
static std::pair<uint64_t, uint64_t> scale_span(const CastSeg& g) {
  uint64_t total = g.rows * g.run;
  uint64_t g0 = cast_group_of(g.scale_every, g.scale_e0, 0);
  uint64_t g1 = cast_group_of(g.scale_every, g.scale_e0, total - 1);
  return {g.scale_ptr + g0 * 4, g.scale_ptr + (g1 + 1) * 4};
}

// [first, last) bytes of the strided side of a validated segment with
// elements: the source of a store, of absmax, of the MX and block stores
static std::pair<uint64_t, uint64_t> source_span(uint64_t src, uint64_t rows,
                                                 uint64_t pitch,
                                                 uint64_t run_bytes) {
  return {src, src + (rows - 1) * pitch + run_bytes};   // validated: no wrap
}

// The two directions differ in which side is the arena's, in what is
// aligned, and in that the store checks its dense destination even without
// elements (the load's strided range means nothing then).  quant_ok: the
// quantising pairs are accepted under a scale (the store; the host
// converter, which loads from a one-row arena, in both directions).
static CastSeg cast_validate(CastKind kind, uint64_t cap, const SegArgs& in,
                             bool quant_ok) {
  const bool load = kind == CAST_LOAD;
  const char* who = load ? "convert" : "store";
  if (in.sdt >= DT_COUNT || in.ddt >= DT_COUNT)
    typed_reject(who, "unknown dtype code");
  uint64_t total;
  if (__builtin_mul_overflow(in.rows, in.run, &total))
    typed_reject(who, "segment size overflows");
  bool scaled = scale_validate(who, in, total, quant_ok, load);
  if (in.sdt != in.ddt && !scaled &&
      !cast_pair_converts((uint32_t)in.sdt, (uint32_t)in.ddt))
    typed_reject(who, "unsupported dtype pair");
  uint64_t ss = cast_itemsize((uint32_t)in.sdt);
  uint64_t ds = cast_itemsize((uint32_t)in.ddt);
  uint64_t run_b, dst_b, end;
  if (__builtin_mul_overflow(in.run, ss, &run_b) ||
      __builtin_mul_overflow(total, ds, &dst_b) ||
      __builtin_add_overflow(in.b, dst_b, &end))
    typed_reject(who, "segment size overflows");
  if (!load && end > cap) typed_reject(who, "arena range out of bounds");
  if (total) {
    if (span_overflows(in.a, in.rows, in.pitch, run_b, &end))
      typed_reject(who, load ? "segment range overflows"
                             : "source range overflows");
    if (load) {
      if (end > cap) typed_reject(who, "arena range out of bounds");
      if (in.b == 0 || in.b % ds)
        typed_reject(who, "dst_ptr null or misaligned");
    } else {
      if (in.a == 0 || in.a % ss)
        typed_reject(who, "src_ptr null or misaligned");
      if (in.b % ds) typed_reject(who, "dst_off misaligned");
    }
  }
  CastSeg g;
  g.src_off = in.a; g.dst_ptr = in.b; g.rows = in.rows; g.run = in.run;
  g.src_pitch = in.pitch; g.src_dt = (uint32_t)in.sdt;
  g.dst_dt = (uint32_t)in.ddt; g.scale_ptr = in.scale_ptr;
  g.scale_every = in.scale_every; g.scale_e0 = in.scale_e0;
  if (in.sdt == in.ddt) {      // raw copy at any itemsize: flatten to bytes
    g.run = run_b;
    g.src_dt = g.dst_dt = DT_U8;
  }
  return g;
}

// ---- group scales for the quantising store (tensor_cast.hip) ----
//
// (src_ptr, rows, run, src_pitch, src_dtype, out_ptr, scale_every, scale_e0,
// n_groups): out_ptr[0:n_groups] are the f32 scales of the segment's tensor.

struct AbsmaxArgs {
  uint64_t src, rows, run, pitch, sdt, out, every, e0, n_groups;
};

// g is filled in when the segment has elements (the return value); its
// slots are the caller's to zero and finish either way
static bool absmax_validate(const AbsmaxArgs& in, AbsmaxSeg& g) {
  const char* who = "absmax";
  if (in.sdt > DT_BF16)
    typed_reject(who, "source dtype is not F32/F16/BF16");
  uint64_t ss = cast_itemsize((uint32_t)in.sdt);
  uint64_t run_b, total, end, last, out_b;
  if (__builtin_mul_overflow(in.run, ss, &run_b) ||
      __builtin_mul_overflow(in.rows, in.run, &total) ||
      __builtin_add_overflow(in.e0, total, &last) ||
      __builtin_mul_overflow(in.n_groups, (uint64_t)4, &out_b) ||
      __builtin_add_overflow(in.out, out_b, &end))
    typed_reject(who, "segment size overflows");
  if (in.n_groups == 0 || in.out == 0 || in.out % 4)
    typed_reject(who, "out_ptr null, misaligned or empty");
  if (!total) return false;
  if (span_overflows(in.src, in.rows, in.pitch, run_b, &end))
    typed_reject(who, "source range overflows");
  if (in.src == 0 || in.src % ss)
    typed_reject(who, "src_ptr null or misaligned");
  if ((in.every ? (last - 1) / in.every : 0) >= in.n_groups)
    typed_reject(who, "groups pass n_groups");
  g.src_ptr = in.src; g.rows = in.rows; g.run = in.run;
  g.src_pitch = in.pitch; g.out_ptr = in.out; g.scale_every = in.every;
  g.scale_e0 = in.e0; g.src_dt = (uint32_t)in.sdt; g.pad = 0;
  return true;
}

// each slot is zeroed and finished once, however the segments share them
static std::vector<ScaleSlots> merge_scale_slots(std::vector<ScaleSlots> slots) {
  std::sort(slots.begin(), slots.end(),
            [](const ScaleSlots& x, const ScaleSlots& y) { return x.ptr < y.ptr; });
  std::vector<ScaleSlots> merged;
  for (auto& r : slots) {
    if (!merged.empty() && r.ptr <= merged.back().ptr + merged.back().n * 4) {
      uint64_t end = std::max(merged.back().ptr + merged.back().n * 4,
                              r.ptr + r.n * 4);
      merged.back().n = (end - merged.back().ptr) / 4;
    } else {
      merged.push_back(r);
    }
  }
  return merged;
}

// ---- MX tensors: E8M0 block scales, E4M3 / E2M1 elements (mx_cast.hip) ----
//
// A segment names its high-precision side (F32/F16/BF16) and its stored
// side (F8_E4M3, or F4 = code 17) and carries (scale_ptr, scale_e0,
// scale_pitch, 32): the element in row r, column c uses the E8M0 byte at
// scale_ptr[(scale_e0 + r * scale_pitch + c) / 32].

enum MxKind { MX_SCALES, MX_STORE, MX_LOAD };

struct MxArgs {
  uint64_t a, b, rows, run, pitch, hp_dt, stored_dt, scale_ptr, scale_e0,
      scale_pitch, block;
};

// kind MX_SCALES / MX_STORE: a = absolute source; MX_STORE: b = arena
// offset; MX_LOAD: a = arena offset, b = absolute destination
static MxSeg mx_validate(const char* who, MxKind kind, uint64_t cap,
                         const MxArgs& in) {
  if (in.block != MX_BLOCK) typed_reject(who, "block size is not 32");
  if (in.hp_dt > DT_BF16)
    typed_reject(who, "not F32/F16/BF16 on the wide side");
  if (in.stored_dt != DT_F8_E4M3 && in.stored_dt != DT_F4)
    typed_reject(who, "stored dtype is not F8_E4M3 or F4");
  uint32_t fmt = in.stored_dt == DT_F4 ? MX_E2M1 : MX_E4M3;
  uint64_t hs = cast_itemsize((uint32_t)in.hp_dt), bits = mx_bits(fmt);
  uint64_t total, run_b, q_b, hp_b, end, last;
  if (__builtin_mul_overflow(in.rows, in.run, &total) ||
      __builtin_mul_overflow(total, hs, &hp_b) ||
      __builtin_mul_overflow(in.run, kind == MX_LOAD ? bits : hs * 8, &run_b))
    typed_reject(who, "segment size overflows");
  run_b /= 8;
  q_b = total / 8 * bits + total % 8 * bits / 8;
  uint64_t odd = in.run | in.scale_e0 | (in.rows > 1 ? in.scale_pitch : 0);
  if (fmt == MX_E2M1 && (odd & 1)) typed_reject(who, "F4 piece splits a byte");
  if (kind == MX_SCALES && (odd % MX_BLOCK))
    typed_reject(who, "not whole blocks of 32");
  MxSeg g;
  g.src = in.a; g.dst = in.b; g.rows = in.rows; g.run = in.run;
  g.src_pitch = in.pitch; g.scale_ptr = in.scale_ptr;
  g.scale_e0 = in.scale_e0; g.scale_pitch = in.scale_pitch;
  g.dt = (uint32_t)in.hp_dt; g.fmt = fmt;
  if (!total) return g;
  if (!in.scale_ptr) typed_reject(who, "scale_ptr is null");
  if (span_overflows(in.scale_e0, in.rows, in.scale_pitch, in.run, &last) ||
      __builtin_add_overflow(in.scale_ptr, last / MX_BLOCK + 1, &end))
    typed_reject(who, "scale range overflows");
  if (span_overflows(in.a, in.rows, in.pitch, run_b, &end))
    typed_reject(who, "source range overflows");
  if (in.rows > 1 && in.pitch < run_b) typed_reject(who, "rows overlap");
  if (kind == MX_LOAD) {
    if (end > cap) typed_reject(who, "arena range out of bounds");
    if (in.b == 0 || in.b % hs || __builtin_add_overflow(in.b, hp_b, &end))
      typed_reject(who, "dst_ptr null, misaligned or overflowing");
  } else {
    if (in.a == 0 || in.a % hs)
      typed_reject(who, "src_ptr null or misaligned");
    if (kind == MX_STORE &&
        (__builtin_add_overflow(in.b, q_b, &end) || end > cap))
      typed_reject(who, "arena range out of bounds");
  }
  return g;
}

// (src_ptr, rows, run, src_pitch, src_dtype, stored_dtype, out_ptr): the
// E8M0 bytes of a whole tensor of rows * run elements (run a multiple of
// 32) land at out_ptr[0 : rows * run / 32]
struct MxScaleArgs {
  uint64_t src, rows, run, pitch, hp_dt, stored_dt, out;
};

static MxSeg mx_scales_validate(const MxScaleArgs& in) {
  return mx_validate("mx scales", MX_SCALES, 0,
                     {in.src, 0, in.rows, in.run, in.pitch, in.hp_dt,
                      in.stored_dt, in.out, 0, in.run, MX_BLOCK});
}

// [first, last) of the E8M0 bytes a validated segment touches
static std::pair<uint64_t, uint64_t> mx_scale_span(const MxSeg& g) {
  uint64_t last = g.scale_e0 + (g.rows - 1) * g.scale_pitch + g.run - 1;
  return {g.scale_ptr + g.scale_e0 / MX_BLOCK,
          g.scale_ptr + last / MX_BLOCK + 1};
}

// ---- 2-D block scales: one F32 scale per bm x bn tile (block_cast.hip) ----
//
// A segment names its high-precision side (F32/F16/BF16) and F8_E4M3 and
// carries (scale_ptr, scale_e0, scale_pitch, M, K, bm, bn): the element in
// row r, column c is element t = scale_e0 + r * scale_pitch + c of a tensor
// (..., M, K) and uses the f32 scale of its tile, block_scale_index(t).

enum BlockKind { BLOCK_ABSMAX, BLOCK_STORE, BLOCK_LOAD };

struct BlockArgs {
  uint64_t a, b, rows, run, pitch, hp_dt, stored_dt, scale_ptr, scale_e0,
      scale_pitch, M, K, bm, bn;
};

// [first, last] of the scale indices a segment with elements can meet:
// the first tile of its first element's row .. the last of its last one's
static std::pair<uint64_t, uint64_t> block_scale_range(const BlockSeg& g) {
  uint64_t left;
  uint64_t tb = g.scale_e0 + (g.rows - 1) * g.scale_pitch + g.run - 1;
  return {block_scale_index(g, g.scale_e0 / g.K * g.K, left),
          block_scale_index(g, tb / g.K * g.K + g.K - 1, left)};
}

// kind BLOCK_ABSMAX / BLOCK_STORE: a = absolute source; BLOCK_STORE: b =
// arena offset; BLOCK_LOAD: a = arena offset, b = absolute destination.
// n_scales: how many scales scale_ptr holds, 0 = not known here.
static BlockSeg block_validate(const char* who, BlockKind kind, uint64_t cap,
                               const BlockArgs& in, uint64_t n_scales = 0) {
  if (in.hp_dt > DT_BF16)
    typed_reject(who, "not F32/F16/BF16 on the wide side");
  if (in.stored_dt != DT_F8_E4M3)
    typed_reject(who, "stored dtype is not F8_E4M3");
  if (!in.M || !in.K || !in.bm || !in.bn)
    typed_reject(who, "M, K, bm and bn must be positive");
  uint64_t hs = cast_itemsize((uint32_t)in.hp_dt);
  uint64_t ss = kind == BLOCK_LOAD ? 1 : hs;         // source itemsize
  uint64_t total, run_b, hp_b, end, last;
  if (__builtin_mul_overflow(in.rows, in.run, &total) ||
      __builtin_mul_overflow(total, hs, &hp_b) ||
      __builtin_mul_overflow(in.run, ss, &run_b))
    typed_reject(who, "segment size overflows");
  BlockSeg g;
  g.src = in.a; g.dst = in.b; g.rows = in.rows; g.run = in.run;
  g.src_pitch = in.pitch; g.scale_ptr = in.scale_ptr;
  g.scale_e0 = in.scale_e0; g.scale_pitch = in.scale_pitch;
  g.M = in.M; g.K = in.K; g.bm = in.bm; g.bn = in.bn;
  g.tm = (in.M - 1) / in.bm + 1; g.tn = (in.K - 1) / in.bn + 1;
  g.dt = (uint32_t)in.hp_dt; g.pad = 0;
  if (!total) return g;
  if (!in.scale_ptr || in.scale_ptr % 4)
    typed_reject(who, "scale_ptr null or misaligned");
  if (in.rows > 1 && in.scale_pitch < in.run)
    typed_reject(who, "rows overlap in the tensor");
  uint64_t per_mat, n_mat, hi_b;
  if (span_overflows(in.scale_e0, in.rows, in.scale_pitch, in.run, &last) ||
      __builtin_add_overflow(last, in.K, &end) ||
      __builtin_mul_overflow(g.tm, g.tn, &per_mat) ||
      __builtin_mul_overflow((last - 1) / in.K / in.M + 1, per_mat, &n_mat) ||
      __builtin_mul_overflow(n_mat, (uint64_t)4, &hi_b) ||
      __builtin_add_overflow(in.scale_ptr, hi_b, &end))
    typed_reject(who, "scale range overflows");
  if (n_scales && block_scale_range(g).second >= n_scales)
    typed_reject(who, "tiles pass the scales given");
  if (span_overflows(in.a, in.rows, in.pitch, run_b, &end))
    typed_reject(who, "source range overflows");
  if (in.rows > 1 && (in.pitch < run_b || in.pitch % ss))
    typed_reject(who, "rows overlap or pitch misaligned");
  if (kind == BLOCK_LOAD) {
    if (end > cap) typed_reject(who, "arena range out of bounds");
    if (in.b == 0 || in.b % hs || __builtin_add_overflow(in.b, hp_b, &end))
      typed_reject(who, "dst_ptr null, misaligned or overflowing");
  } else {
    if (in.a == 0 || in.a % ss)
      typed_reject(who, "src_ptr null or misaligned");
    if (kind == BLOCK_STORE &&
        (__builtin_add_overflow(in.b, total, &end) || end > cap))
      typed_reject(who, "arena range out of bounds");
  }
  return g;
}

// (src_ptr, rows, run, src_pitch, src_dtype, out_ptr, scale_e0, scale_pitch,
// M, K, bm, bn, n_slots): out_ptr[0:n_slots] are the f32 tile scales of the
// segment's tensor
struct BlockAbsmaxArgs {
  uint64_t src, rows, run, pitch, hp_dt, out, scale_e0, scale_pitch, M, K, bm,
      bn, n_slots;
};

static BlockSeg block_absmax_validate(const BlockAbsmaxArgs& in) {
  uint64_t out_b, end;
  if (in.n_slots == 0 || in.out == 0 || in.out % 4 ||
      __builtin_mul_overflow(in.n_slots, (uint64_t)4, &out_b) ||
      __builtin_add_overflow(in.out, out_b, &end))
    typed_reject("block absmax",
                 "out_ptr null, misaligned, empty or overflowing");
  return block_validate("block absmax", BLOCK_ABSMAX, 0,
                        {in.src, 0, in.rows, in.run, in.pitch, in.hp_dt,
                         DT_F8_E4M3, in.out, in.scale_e0, in.scale_pitch, in.M,
                         in.K, in.bm, in.bn},
                        in.n_slots);
}

// Typed tensor load, store and scales: the entry points over the kernels of
// tensor_cast.hip, mx_cast.hip and block_cast.hip.  Included by module.cpp
// behind the arena, scratch and tile-table plumbing it uses.
//
// Every entry point validates its tuples (typed_validate.h) while it holds
// the GIL, so every argument error is raised on the host before anything
// runs, and then goes through one of two drivers: arena_typed_run for the
// six that move elements between an arena and absolute addresses,
// stream_typed_run for the three that compute scales on the caller's thread
// stream.  The three *_convert_host are the byte paths' host twins.

#include <tuple>

#include "typed_validate.h"

// Python tuple -> the validator's argument struct, field by field; a tuple
// shorter than the struct leaves the rest at its defaults
template <class Args, class Tuple> static Args args_of(const Tuple& t) {
  return std::apply([](auto... v) { return Args{v...}; }, t);
}

// validate every tuple, keep the segments that have elements
template <class Tuple, class Validate>
static auto typed_segments(const std::vector<Tuple>& in, Validate validate) {
  std::vector<decltype(validate(in[0]))> segs;
  segs.reserve(in.size());
  for (auto& t : in) {
    auto g = validate(t);
    if (g.rows * g.run) segs.push_back(g);
  }
  return segs;
}

// ---- device ranges ----

// allocations already checked in this call
typedef std::vector<std::pair<uint64_t, uint64_t>> KnownRanges;

// a kernel on `device` dereferences [first, last): it has to be memory of
// that GPU (or pinned host memory), and where the runtime knows the
// allocation's extent the range has to lie inside it.  `known` holds the
// allocations already checked in this call: the tensors of a checkpoint
// mostly share a few allocator blocks, and the runtime queries cost more
// than the rest of a small call.  Errors read "<who>: <ptr> is not ..." and
// "<who>: <noun> lives ...".  Caller has set the device.
static void check_device_range(int device, uint64_t first, uint64_t last,
                               const char* who_is, const char* ptr,
                               const char* noun, KnownRanges& known) {
  for (auto& k : known)
    if (first >= k.first && last <= k.second) return;
  const std::string who = who_is;   // a miss: the messages may need it
  hipPointerAttribute_t at;
  const void* p = (const void*)(uintptr_t)first;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();
    throw std::invalid_argument(who + ": " + ptr +
                                " is not device-visible memory");
  }
  if (at.type == hipMemoryTypeDevice && at.device != device)
    throw std::invalid_argument(who + ": " + noun + " lives on another device");
  if (at.type != hipMemoryTypeDevice && at.type != hipMemoryTypeHost &&
      at.type != hipMemoryTypeManaged)
    throw std::invalid_argument(who + ": " + ptr +
                                " is not device-visible memory");
  hipDeviceptr_t lo;
  size_t sz;
  if (hipMemGetAddressRange(&lo, &sz, (hipDeviceptr_t)p) != hipSuccess) {
    (void)hipGetLastError();   // extent unknown to the runtime: type check only
    return;
  }
  if (last > (uint64_t)(uintptr_t)lo + sz)
    throw std::invalid_argument(who + ": " + noun +
                                " runs past its allocation");
  known.emplace_back((uint64_t)(uintptr_t)lo, (uint64_t)(uintptr_t)lo + sz);
}

static void check_span(int device, std::pair<uint64_t, uint64_t> span,
                       const char* who, const char* ptr, const char* noun,
                       KnownRanges& known) {
  check_device_range(device, span.first, span.second, who, ptr, noun, known);
}

// the absolute side of a validated segment and then its scales, as the
// kernels of a device arena (or of absmax / mx_scales) dereference them
static void cast_check_ranges(int device, const char* who, CastKind kind,
                              const CastSeg& g, KnownRanges& known) {
  if (kind == CAST_STORE)
    check_span(device,
               source_span(g.src_off, g.rows, g.src_pitch,
                           g.run * cast_itemsize(g.src_dt)),
               who, "src_ptr", "source", known);
  if (g.scale_ptr)
    check_span(device, scale_span(g), who, "scale_ptr", "scales", known);
}

// MxSeg and BlockSeg name their fields alike
template <class Seg>
static void scaled_check_side(int device, const char* who, bool load,
                              const Seg& g, KnownRanges& known) {
  uint64_t hs = cast_itemsize(g.dt);
  if (load)
    check_device_range(device, g.dst, g.dst + g.rows * g.run * hs, who,
                       "dst_ptr", "destination", known);
  else
    check_span(device, source_span(g.src, g.rows, g.src_pitch, g.run * hs),
               who, "src_ptr", "source", known);
}

static void mx_check_ranges(int device, const char* who, MxKind kind,
                            const MxSeg& g, KnownRanges& known) {
  scaled_check_side(device, who, kind == MX_LOAD, g, known);
  check_span(device, mx_scale_span(g), who, "scale_ptr", "scales", known);
}

static void block_check_ranges(int device, const char* who, BlockKind kind,
                               const BlockSeg& g, KnownRanges& known) {
  scaled_check_side(device, who, kind == BLOCK_LOAD, g, known);
  auto range = block_scale_range(g);
  check_device_range(device, g.scale_ptr + range.first * 4,
                     g.scale_ptr + (range.second + 1) * 4, who, "scale_ptr",
                     "scales", known);
}

// ---- the two drivers ----

// dense elements per workgroup tile
static uint64_t typed_tile_elems(const CastSeg& g) {
  return cast_tile_elems(g.src_dt, g.dst_dt);
}
template <class Seg> static uint64_t typed_tile_elems(const Seg&) {
  return CAST_TILE;
}

template <class Seg> static Tiles typed_tiles(const std::vector<Seg>& segs,
                                              const char* who) {
  return build_tiles(
      segs.size(), [&](size_t i) { return segs[i].rows * segs[i].run; },
      [&](size_t i) { return typed_tile_elems(segs[i]); }, who);
}

// Validated segments with elements between arena `a` and absolute
// addresses.  A host arena runs host(base, segment) for each.  A device
// arena cuts the segments into tiles, takes the arena's lock, has
// check(device, segment, known) look at what the kernel will dereference
// outside the arena, uploads the tables into the arena's scratch and runs
// one launch of `kernel` on its kernel stream, synchronised on return: a
// store's sources are the caller's to free or overwrite by then.  Base is
// const uint8_t for the loads, uint8_t for the stores.
template <class Seg, class Base, class Check, class Host>
static void arena_typed_run(Arena* a, const std::vector<Seg>& segs,
                            const char* who, Check check, Host host,
                            void (*kernel)(Base*, const Seg*, const uint32_t*,
                                           const uint64_t*, uint32_t)) {
  if (segs.empty()) return;
  py::gil_scoped_release rel;
  Base* base = (Base*)a->base;
  if (!a->is_dev()) {
    for (auto& g : segs) host(base, g);
    return;
  }
  Tiles tiles = typed_tiles(segs, who);
  std::lock_guard<std::mutex> lock(a->mu);
  HIP_CHECK(hipSetDevice(a->device));
  KnownRanges known;
  for (auto& g : segs) check(a->device, g, known);
  Scratch sc(a, tiles.room<Seg>(segs.size()));
  DevTiles<Seg> d = upload_tiles(a, sc, segs, tiles);
  launch(kernel, d.grid(), WG, a->kstream, base, d.items, d.tile_item,
         d.tile_off, d.n_tiles);
  HIP_CHECK(hipStreamSynchronize(a->kstream));
}

// Validated segments with elements whose kernel writes scales; not tied to
// an arena: a checkpoint's scales are needed before its first block is
// placed.  device -1 runs host(segment) for each; device >= 0 runs one
// launch of `kernel` on the caller's thread stream, the tables in memory of
// this call, synchronised on return.  With `slots` (merged f32 slots the
// kernel reduces amax bits into) the slots are zeroed before and turned
// into scales after, on either side, and checked as "out_ptr".
template <class Seg, class Check, class Host>
static void stream_typed_run(int device, const std::vector<Seg>& segs,
                             const std::vector<ScaleSlots>* slots,
                             const char* who, Check check, Host host,
                             void (*kernel)(const Seg*, const uint32_t*,
                                            const uint64_t*, uint32_t)) {
  static const std::vector<ScaleSlots> none;
  const std::vector<ScaleSlots>& merged = slots ? *slots : none;
  if (slots ? merged.empty() : segs.empty()) return;
  py::gil_scoped_release rel;
  if (device < 0) {
    for (auto& r : merged) scale_slots_host(r, false);
    for (auto& g : segs) host(g);
    for (auto& r : merged) scale_slots_host(r, true);
    return;
  }
  Tiles tiles = typed_tiles(segs, who);
  HIP_CHECK(hipSetDevice(device));
  KnownRanges known;
  for (auto& g : segs) check(device, g, known);
  for (auto& r : merged)
    check_device_range(device, r.ptr, r.ptr + r.n * 4, who, "out_ptr",
                       "scales", known);
  hipStream_t s = thread_stream(device);
  CallScratch sc(tiles.room<Seg>(segs.size()) +
                 (slots ? Scratch::room<ScaleSlots>(merged.size()) : 0));
  const ScaleSlots* d_slots = nullptr;
  unsigned slot_grid = (unsigned)std::min<size_t>(merged.size(), TILE_GRID_CAP);
  if (slots) {
    ScaleSlots* up = sc.take<ScaleSlots>(merged.size());
    HIP_CHECK(hipMemcpyAsync(up, merged.data(),
                             merged.size() * sizeof(ScaleSlots),
                             hipMemcpyHostToDevice, s));
    d_slots = up;
    launch(scale_slots_kernel, slot_grid, WG, s, d_slots,
           (uint32_t)merged.size(), 0);
  }
  if (!tiles.empty()) {
    DevTiles<Seg> d = upload_tiles(s, sc, segs, tiles);
    launch(kernel, d.grid(), WG, s, d.items, d.tile_item, d.tile_off,
           d.n_tiles);
  }
  if (slots)
    launch(scale_slots_kernel, slot_grid, WG, s, d_slots,
           (uint32_t)merged.size(), 1);
  // the scales are read and the tables freed once this returns
  HIP_CHECK(hipStreamSynchronize(s));
}

// ---- plain and group-scaled segments (tensor_cast.hip) ----

typedef std::tuple<uint64_t, uint64_t, uint64_t, uint64_t, uint64_t, uint64_t,
                   uint64_t> CastSegTuple;
typedef std::tuple<uint64_t, uint64_t, uint64_t, uint64_t, uint64_t, uint64_t,
                   uint64_t, uint64_t, uint64_t, uint64_t> ScaledSegTuple;
typedef std::variant<CastSegTuple, ScaledSegTuple> AnySegTuple;

static std::vector<CastSeg> cast_segments(CastKind kind, uint64_t cap,
                                          const std::vector<AnySegTuple>& in) {
  return typed_segments(in, [&](const AnySegTuple& v) {
    SegArgs args = std::visit(
        [](auto& t) { return args_of<SegArgs>(t); }, v);
    return cast_validate(kind, cap, args, kind == CAST_STORE);
  });
}

static void arena_convert_ptr(int h, std::vector<AnySegTuple> segs_in) {
  Arena* a = get_arena(h);
  arena_typed_run(
      a, cast_segments(CAST_LOAD, a->cap, segs_in), "convert",
      [](int dev, const CastSeg& g, KnownRanges& known) {
        cast_check_ranges(dev, "convert", CAST_LOAD, g, known);
      },
      convert_segment_host, convert_segments_kernel);
}

static void arena_store_ptr(int h, std::vector<AnySegTuple> segs_in) {
  Arena* a = get_arena(h);
  arena_typed_run(
      a, cast_segments(CAST_STORE, a->cap, segs_in), "store",
      [](int dev, const CastSeg& g, KnownRanges& known) {
        cast_check_ranges(dev, "store", CAST_STORE, g, known);
      },
      store_segment_host, store_segments_kernel);
}

// Segments: (src_ptr, rows, run, src_pitch, src_dtype, out_ptr, scale_every,
// scale_e0, n_groups).  out_ptr[0:n_groups] is zeroed, receives each
// group's amax, and becomes max(amax, 2^-40) / 448.  Segments may share
// slots (a tensor given in pieces).
typedef std::tuple<uint64_t, uint64_t, uint64_t, uint64_t, uint64_t, uint64_t,
                   uint64_t, uint64_t, uint64_t> AbsmaxSegTuple;

static void absmax_scales(int device, std::vector<AbsmaxSegTuple> segs_in) {
  if (device < -1) throw std::invalid_argument("absmax: bad device");
  std::vector<AbsmaxSeg> segs;
  std::vector<ScaleSlots> slots;
  segs.reserve(segs_in.size());
  for (auto& t : segs_in) {
    AbsmaxArgs in = args_of<AbsmaxArgs>(t);
    AbsmaxSeg g;
    if (absmax_validate(in, g)) segs.push_back(g);
    slots.push_back({in.out, in.n_groups});
  }
  slots = merge_scale_slots(std::move(slots));
  stream_typed_run(
      device, segs, &slots, "absmax",
      [](int dev, const AbsmaxSeg& g, KnownRanges& known) {
        check_span(dev,
                   source_span(g.src_ptr, g.rows, g.src_pitch,
                               g.run * cast_itemsize(g.src_dt)),
                   "absmax", "src_ptr", "source", known);
      },
      absmax_segment_host, absmax_segments_kernel);
}

// host conversion of `n` packed elements (the slow path of the typed
// reader: file-tier extents and elements straddling a block boundary go
// through the same scalar routines as the kernel).  With `scales` (a host
// buffer of the tensor's f32 group scales) also the scaled pairs in both
// directions: the byte path of the typed writer quantises here.

// what a host converter returns: 8-byte words, aligned for every
// destination itemsize, of at most 1 TiB
struct HostOut {
  std::vector<uint64_t> words;
  uint64_t n_bytes;
  HostOut(const char* who, uint64_t n_bytes_) : n_bytes(n_bytes_) {
    if (n_bytes > (1ull << 40)) typed_reject(who, "segment size overflows");
    words.resize(n_bytes / 8 + 1);
  }
  uint8_t* data() { return (uint8_t*)words.data(); }
  py::bytes bytes() const {
    return py::bytes((const char*)words.data(), n_bytes);
  }
};

static uint64_t buffer_bytes(const py::buffer_info& bi) {
  return (uint64_t)bi.size * bi.itemsize;
}

static py::bytes convert_host(py::buffer src, uint64_t sdt, uint64_t ddt,
                              uint64_t n, py::object scales,
                              uint64_t scale_every, uint64_t scale_e0) {
  py::buffer_info bi = src.request();
  SegArgs in{0, 0, 1, n, 0, sdt, ddt};
  py::buffer_info sbi;
  if (!scales.is_none()) {
    sbi = py::cast<py::buffer>(scales).request();
    uint64_t have = buffer_bytes(sbi) / 4, last;
    if (!sbi.ptr || (uintptr_t)sbi.ptr % 4 || !have)
      throw std::invalid_argument("convert: scales empty or misaligned");
    if (n && (__builtin_add_overflow(scale_e0, n - 1, &last) ||
              (scale_every ? last / scale_every : 0) >= have))
      throw std::invalid_argument("convert: scales shorter than the groups");
    in.scale_ptr = (uint64_t)(uintptr_t)sbi.ptr;
    in.scale_every = scale_every;
    in.scale_e0 = scale_e0;
  }
  uint64_t ds = ddt < DT_COUNT ? cast_itemsize((uint32_t)ddt) : 1;
  uint64_t out_b;
  if (__builtin_mul_overflow(n, ds, &out_b)) out_b = ~0ull;
  HostOut out("convert", out_b);
  // a load from a one-row arena that is the source buffer
  in.b = (uint64_t)(uintptr_t)out.data();
  CastSeg g = cast_validate(CAST_LOAD, buffer_bytes(bi), in, true);
  if (g.rows * g.run) convert_segment_host((const uint8_t*)bi.ptr, g);
  return out.bytes();
}

// The MX and block converters quantise when src_dtype is F32/F16/BF16 and
// dequantise otherwise.  `in` carries the scale fields of one row of n
// elements; validate(load, cap, in) is the family's validator.  Quantising
// is a store from the source buffer into an arena without bounds, the
// source's length checked here; dequantising is a load from a one-row arena
// that is the source buffer, to a destination of this call's own.
template <class Args, class Validate>
static auto host_validate(const char* who, const py::buffer_info& bi,
                          uint64_t sdt, uint64_t ddt, uint64_t n, Args in,
                          Validate validate) {
  bool quant = sdt <= DT_BF16;
  in.rows = 1; in.run = n; in.scale_pitch = n;
  in.hp_dt = quant ? sdt : ddt;
  in.stored_dt = quant ? ddt : sdt;
  if (!quant) {
    in.b = 8;
    return validate(true, buffer_bytes(bi), in);
  }
  in.a = (uint64_t)(uintptr_t)bi.ptr;
  auto g = validate(false, ~0ull, in);
  if (n > buffer_bytes(bi) / cast_itemsize(g.dt))
    typed_reject(who, "source shorter than n");
  return g;
}

// out_b bytes of store(src, out, g) or load(src, out, g)
template <class Seg, class Store, class Load>
static py::bytes host_convert(const char* who, const py::buffer_info& bi,
                              bool quant, const Seg& g, uint64_t out_b,
                              Store store, Load load) {
  HostOut out(who, out_b);
  if (g.run) {
    if (quant) store((const uint8_t*)bi.ptr, out.data(), g);
    else load((const uint8_t*)bi.ptr, out.data(), g);
  }
  return out.bytes();
}

// ---- MX tensors (mx_cast.hip) ----

typedef std::tuple<uint64_t, uint64_t, uint64_t, uint64_t, uint64_t, uint64_t,
                   uint64_t, uint64_t, uint64_t, uint64_t, uint64_t> MxSegTuple;

// Segments: (src_ptr, dst_off, rows, run, src_pitch, src_dtype, dst_dtype,
// scale_ptr, scale_e0, scale_pitch, 32), F32/F16/BF16 -> F8_E4M3 or F4.
static void arena_mx_store_ptr(int h, std::vector<MxSegTuple> segs_in) {
  Arena* a = get_arena(h);
  arena_typed_run(
      a, typed_segments(segs_in, [&](const MxSegTuple& t) {
        return mx_validate("mx store", MX_STORE, a->cap, args_of<MxArgs>(t));
      }),
      "mx store",
      [](int dev, const MxSeg& g, KnownRanges& known) {
        mx_check_ranges(dev, "mx store", MX_STORE, g, known);
      },
      [](uint8_t* base, const MxSeg& g) {
        mx_store_segment_host((const uint8_t*)g.src, base + g.dst, g);
      },
      mx_store_kernel);
}

// Segments: (src_off, dst_ptr, rows, run, src_pitch, src_dtype, dst_dtype,
// scale_ptr, scale_e0, scale_pitch, 32), F8_E4M3 or F4 -> F32/F16/BF16.
static void arena_mx_convert_ptr(int h, std::vector<MxSegTuple> segs_in) {
  Arena* a = get_arena(h);
  arena_typed_run(
      a, typed_segments(segs_in, [&](const MxSegTuple& t) {
        MxArgs in = args_of<MxArgs>(t);
        std::swap(in.hp_dt, in.stored_dt);   // the tuple is (src, dst) ordered
        return mx_validate("mx convert", MX_LOAD, a->cap, in);
      }),
      "mx convert",
      [](int dev, const MxSeg& g, KnownRanges& known) {
        mx_check_ranges(dev, "mx convert", MX_LOAD, g, known);
      },
      [](const uint8_t* base, const MxSeg& g) {
        mx_load_segment_host(base + g.src, (uint8_t*)g.dst, g);
      },
      mx_load_kernel);
}

// Segments: (src_ptr, rows, run, src_pitch, src_dtype, stored_dtype,
// out_ptr), see MxScaleArgs.
typedef std::tuple<uint64_t, uint64_t, uint64_t, uint64_t, uint64_t, uint64_t,
                   uint64_t> MxScaleTuple;

static void mx_scales(int device, std::vector<MxScaleTuple> segs_in) {
  if (device < -1) throw std::invalid_argument("mx scales: bad device");
  stream_typed_run(
      device, typed_segments(segs_in, [](const MxScaleTuple& t) {
        return mx_scales_validate(args_of<MxScaleArgs>(t));
      }),
      nullptr, "mx scales",
      [](int dev, const MxSeg& g, KnownRanges& known) {
        mx_check_ranges(dev, "mx scales", MX_SCALES, g, known);
      },
      mx_scales_segment_host, mx_scales_kernel);
}

// host conversion of `n` packed elements under the E8M0 bytes in `scales`,
// element i using scales[(scale_e0 + i) / 32]: quantising when dst_dtype is
// F8_E4M3 / F4, dequantising when src_dtype is (the byte paths)
static py::bytes mx_convert_host(py::buffer src, uint64_t sdt, uint64_t ddt,
                                 uint64_t n, py::buffer scales,
                                 uint64_t scale_e0) {
  py::buffer_info bi = src.request(), sbi = scales.request();
  MxArgs in{};
  in.scale_ptr = (uint64_t)(uintptr_t)sbi.ptr;
  in.scale_e0 = scale_e0;
  in.block = MX_BLOCK;
  MxSeg g = host_validate(
      "mx convert", bi, sdt, ddt, n, in,
      [](bool load, uint64_t cap, const MxArgs& x) {
        return mx_validate("mx convert", load ? MX_LOAD : MX_STORE, cap, x);
      });
  bool quant = sdt <= DT_BF16;
  uint64_t last;
  if (n && (__builtin_add_overflow(scale_e0, n - 1, &last) || !sbi.ptr ||
            last / MX_BLOCK >= buffer_bytes(sbi)))
    throw std::invalid_argument("mx convert: scales shorter than the blocks");
  return host_convert(
      "mx convert", bi, quant, g,
      quant ? n * mx_bits(g.fmt) / 8 : n * cast_itemsize(g.dt),
      mx_store_segment_host, mx_load_segment_host);
}

// ---- 2-D block scales (block_cast.hip) ----

typedef std::tuple<uint64_t, uint64_t, uint64_t, uint64_t, uint64_t, uint64_t,
                   uint64_t, uint64_t, uint64_t, uint64_t, uint64_t, uint64_t,
                   uint64_t, uint64_t> BlockSegTuple;

// Segments: (src_ptr, dst_off, rows, run, src_pitch, src_dtype, dst_dtype,
// scale_ptr, scale_e0, scale_pitch, M, K, bm, bn), F32/F16/BF16 -> F8_E4M3.
static void arena_block_store_ptr(int h, std::vector<BlockSegTuple> segs_in) {
  Arena* a = get_arena(h);
  arena_typed_run(
      a, typed_segments(segs_in, [&](const BlockSegTuple& t) {
        return block_validate("block store", BLOCK_STORE, a->cap,
                              args_of<BlockArgs>(t));
      }),
      "block store",
      [](int dev, const BlockSeg& g, KnownRanges& known) {
        block_check_ranges(dev, "block store", BLOCK_STORE, g, known);
      },
      [](uint8_t* base, const BlockSeg& g) {
        block_store_segment_host((const uint8_t*)g.src, base + g.dst, g);
      },
      block_store_kernel);
}

// Segments: (src_off, dst_ptr, rows, run, src_pitch, src_dtype, dst_dtype,
// scale_ptr, scale_e0, scale_pitch, M, K, bm, bn), F8_E4M3 -> F32/F16/BF16.
static void arena_block_convert_ptr(int h, std::vector<BlockSegTuple> segs_in) {
  Arena* a = get_arena(h);
  arena_typed_run(
      a, typed_segments(segs_in, [&](const BlockSegTuple& t) {
        BlockArgs in = args_of<BlockArgs>(t);
        std::swap(in.hp_dt, in.stored_dt);   // the tuple is (src, dst) ordered
        return block_validate("block convert", BLOCK_LOAD, a->cap, in);
      }),
      "block convert",
      [](int dev, const BlockSeg& g, KnownRanges& known) {
        block_check_ranges(dev, "block convert", BLOCK_LOAD, g, known);
      },
      [](const uint8_t* base, const BlockSeg& g) {
        block_load_segment_host(base + g.src, (uint8_t*)g.dst, g);
      },
      block_load_kernel);
}

// Segments: (src_ptr, rows, run, src_pitch, src_dtype, out_ptr, scale_e0,
// scale_pitch, M, K, bm, bn, n_slots), see BlockAbsmaxArgs.  out_ptr
// [0:n_slots] is zeroed, receives each tile's amax and becomes
// max(amax, 2^-40) / 448, as in absmax_scales.  Segments may share slots.
typedef std::tuple<uint64_t, uint64_t, uint64_t, uint64_t, uint64_t, uint64_t,
                   uint64_t, uint64_t, uint64_t, uint64_t, uint64_t, uint64_t,
                   uint64_t> BlockAbsmaxTuple;

static void block_absmax_scales(int device,
                                std::vector<BlockAbsmaxTuple> segs_in) {
  if (device < -1) throw std::invalid_argument("block absmax: bad device");
  std::vector<ScaleSlots> slots;
  std::vector<BlockSeg> segs =
      typed_segments(segs_in, [&](const BlockAbsmaxTuple& t) {
        BlockAbsmaxArgs in = args_of<BlockAbsmaxArgs>(t);
        BlockSeg g = block_absmax_validate(in);
        slots.push_back({in.out, in.n_slots});
        return g;
      });
  slots = merge_scale_slots(std::move(slots));
  stream_typed_run(
      device, segs, &slots, "block absmax",
      [](int dev, const BlockSeg& g, KnownRanges& known) {
        block_check_ranges(dev, "block absmax", BLOCK_ABSMAX, g, known);
      },
      block_absmax_segment_host, block_absmax_kernel);
}

// host conversion of `n` packed elements, element i being element
// scale_e0 + i of a tensor (..., M, K) under bm x bn tile scales:
// quantising when dst_dtype is F8_E4M3, dequantising when src_dtype is (the
// byte paths).  `scales` holds the tensor's f32 scales from index scale_g0
// on; it must cover every tile the elements meet.
static py::bytes block_convert_host(py::buffer src, uint64_t sdt, uint64_t ddt,
                                    uint64_t n, py::buffer scales,
                                    uint64_t scale_e0, uint64_t M, uint64_t K,
                                    uint64_t bm, uint64_t bn,
                                    uint64_t scale_g0) {
  py::buffer_info bi = src.request(), sbi = scales.request();
  BlockArgs in{};
  in.scale_ptr = (uint64_t)(uintptr_t)sbi.ptr;
  in.scale_e0 = scale_e0;
  in.M = M; in.K = K; in.bm = bm; in.bn = bn;
  BlockSeg g = host_validate(
      "block convert", bi, sdt, ddt, n, in,
      [](bool load, uint64_t cap, const BlockArgs& x) {
        return block_validate("block convert",
                              load ? BLOCK_LOAD : BLOCK_STORE, cap, x);
      });
  bool quant = sdt <= DT_BF16;
  if (n) {
    auto range = block_scale_range(g);
    if (range.first < scale_g0 ||
        range.second - scale_g0 >= buffer_bytes(sbi) / 4)
      throw std::invalid_argument("block convert: scales do not cover the tiles");
    g.scale_ptr -= 4 * scale_g0;           // index 0 of the tensor's scales
  }
  return host_convert("block convert", bi, quant, g,
                      quant ? n : n * cast_itemsize(g.dt),
                      block_store_segment_host, block_load_segment_host);
}

// Host-side sanitizer sweep for the argument checks of csrc/typed_validate.h:
// cast_validate (both directions, with and without quant_ok), absmax_validate,
// mx_validate / mx_scales_validate and block_validate /
// block_absmax_validate are driven with valid segments whose fields are
// replaced, one to three at a time, by edge values (zeros, the UINT64_MAX
// neighbourhood, powers of two, pitches below the run, odd F4 runs, edge
// tiles, scale_e0 near the wrap) and by seeded random ones.  For every
// segment a validator ACCEPTS, the first and last byte of its source and of
// its destination and the scales it can touch are recomputed in unsigned
// __int128 and must lie inside the arena where one is involved, must not
// wrap 64 bits, and must agree with source_span, scale_span, mx_scale_span
// and block_scale_range.  The validators dereference nothing, so the
// addresses are numbers only.
//
// Host code only, never run on a GPU machine:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 \
//     -Xarch_host -fsanitize=address,undefined \
//     scripts/typed_validate_sweep.cpp -o /tmp/typed_validate_sweep \
//     && /tmp/typed_validate_sweep

#include "../csrc/tensor_cast.hip"
#include "../csrc/mx_cast.hip"
#include "../csrc/block_cast.hip"
#include "../csrc/typed_validate.h"

#include <cstdio>

typedef unsigned __int128 u128;
static const u128 TOP = (u128)1 << 64;            // one past UINT64_MAX
static const uint64_t U = ~0ull;

static uint64_t checks = 0, failures = 0, accepted = 0, refused = 0;

static void check(bool ok, const char* what, const char* who) {
  ++checks;
  if (ok) return;
  if (failures++ < 20) std::fprintf(stderr, "FAIL %s: %s\n", who, what);
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 7;
  rng_state ^= rng_state << 17;
  return rng_state;
}
static uint64_t below(uint64_t n) { return rnd() % n; }

static uint64_t edge_value() {
  static const uint64_t fixed[] = {
      0, 1, 2, 3, 4, 5, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128,
      255, 256, 4095, 4096, 4097, 1ull << 31, 1ull << 32, (1ull << 32) + 1,
      1ull << 33, 1ull << 40, 1ull << 61, (1ull << 61) + 1, 1ull << 62,
      1ull << 63, (1ull << 63) + 1, U, U - 1, U - 2, U - 3, U - 4, U - 7,
      U - 8, U - 31, U - 32, U - 63, U - 64, U - 4095, U / 2, U / 3, U / 4};
  uint64_t k = below(64);
  if (k < sizeof(fixed) / sizeof(fixed[0])) return fixed[k];
  if (k < 56) return below(8192);
  if (k < 60) return U - below(8192);
  return rnd();
}

// replace up to three of the n fields at f
static void mutate(uint64_t* f, int n) {
  int k = (int)below(4);
  for (int i = 0; i < k; ++i) f[below(n)] = edge_value();
}

template <class Fn> static bool accepts(Fn fn) {
  try {
    fn();
    ++accepted;
    return true;
  } catch (const std::invalid_argument&) {
    ++refused;
    return false;
  }
}

static u128 strided_end(uint64_t base, uint64_t rows, uint64_t pitch,
                        u128 run_bytes) {
  return (u128)base + (u128)(rows - 1) * pitch + run_bytes;
}

// ---- cast ----

static void cast_case(CastKind kind, bool quant_ok, uint64_t cap,
                      SegArgs in) {
  const char* who = kind == CAST_LOAD ? "cast load" : "cast store";
  CastSeg g;
  if (!accepts([&] { g = cast_validate(kind, cap, in, quant_ok); })) return;
  u128 total = (u128)in.rows * in.run;
  uint64_t ss = cast_itemsize((uint32_t)in.sdt);
  uint64_t ds = cast_itemsize((uint32_t)in.ddt);
  check(in.sdt < DT_COUNT && in.ddt < DT_COUNT, "dtype codes", who);
  check(total < TOP, "element count fits", who);
  u128 dense_end = (u128)in.b + total * ds;
  check(dense_end <= (kind == CAST_STORE ? (u128)cap : TOP - 1),
        "dense side in range", who);
  check(g.rows * g.run * cast_itemsize(g.src_dt) == (uint64_t)(total * ss) &&
            g.rows * g.run * cast_itemsize(g.dst_dt) == (uint64_t)(total * ds),
        "segment keeps its bytes", who);
  check((in.sdt == in.ddt) == (g.src_dt == DT_U8 && g.dst_dt == DT_U8 &&
                               g.run == in.run * ss) ||
            (in.sdt == DT_U8 && in.ddt == DT_U8),
        "same-dtype flatten", who);
  bool quant = cast_pair_quantizes((uint32_t)in.sdt, (uint32_t)in.ddt);
  bool dequant = cast_pair_dequantizes((uint32_t)in.sdt, (uint32_t)in.ddt);
  if (in.scale_ptr)
    check((quant && quant_ok) || (dequant && kind == CAST_LOAD),
          "scale only on a scaled pair", who);
  else
    check(!(quant && quant_ok) &&
              (in.sdt == in.ddt ||
               cast_pair_converts((uint32_t)in.sdt, (uint32_t)in.ddt)),
          "unscaled pair converts", who);
  if (total == 0) return;
  u128 strided = strided_end(in.a, in.rows, in.pitch, (u128)in.run * ss);
  check(strided <= (kind == CAST_LOAD ? (u128)cap : TOP - 1),
        "strided side in range", who);
  auto sp = source_span(g.src_off, g.rows, g.src_pitch,
                        g.run * cast_itemsize(g.src_dt));
  check(sp.first == in.a && (u128)sp.second == strided, "source_span", who);
  if (kind == CAST_LOAD) check(in.b && in.b % ds == 0, "dst aligned", who);
  else check(in.a && in.a % ss == 0 && in.b % ds == 0, "store aligned", who);
  if (in.scale_ptr) {
    u128 g0 = in.scale_every ? (u128)in.scale_e0 / in.scale_every : 0;
    u128 g1 = in.scale_every
                  ? ((u128)in.scale_e0 + total - 1) / in.scale_every : 0;
    u128 first = (u128)in.scale_ptr + g0 * 4;
    u128 last = (u128)in.scale_ptr + (g1 + 1) * 4;
    check(last < TOP && in.scale_ptr % 4 == 0, "scales in range", who);
    auto span = scale_span(g);
    check((u128)span.first == first && (u128)span.second == last,
          "scale_span", who);
  }
}

static void cast_sweep(uint64_t n) {
  static const uint64_t dts[] = {DT_F32, DT_F16, DT_BF16, DT_F8_E4M3,
                                 DT_F8_E5M2, DT_F64, DT_I64, DT_U8, DT_COUNT};
  for (uint64_t i = 0; i < n; ++i) {
    CastKind kind = (i & 1) ? CAST_STORE : CAST_LOAD;
    bool quant_ok = kind == CAST_STORE || (i & 2);
    uint64_t cap = (i & 4) ? 4096 : edge_value();
    uint64_t sdt = dts[below(9)], ddt = (i & 8) ? sdt : dts[below(9)];
    uint64_t ss = cast_itemsize((uint32_t)sdt), ds = cast_itemsize((uint32_t)ddt);
    uint64_t rows = 1 + below(4), run = below(40);
    uint64_t pitch = run * ss + ((i & 16) ? below(64) : 0);
    uint64_t arena_off = below(64) * 8, addr = 0x7f0000001000ull + below(64) * 8;
    uint64_t f[10] = {kind == CAST_LOAD ? arena_off : addr,
                      kind == CAST_LOAD ? addr : arena_off, rows, run, pitch,
                      sdt, ddt, 0, 0, 0};
    if ((i & 32) && ((sdt <= DT_BF16 && ddt == DT_F8_E4M3) ||
                     (sdt == DT_F8_E4M3 && ddt <= DT_BF16))) {
      f[7] = 0x7e0000002000ull + below(16) * 4;
      f[8] = below(3) ? below(70) : 0;
      f[9] = below(3) ? below(500) : U - below(200);
    }
    (void)ds;
    mutate(f, 10);
    SegArgs in{f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], f[9]};
    cast_case(kind, quant_ok, cap, in);
  }
}

// ---- absmax ----

static void absmax_sweep(uint64_t n) {
  const char* who = "absmax";
  for (uint64_t i = 0; i < n; ++i) {
    uint64_t sdt = below(3), ss = cast_itemsize((uint32_t)sdt);
    uint64_t rows = 1 + below(4), run = below(40), every = below(3) ? 1 + below(64) : 0;
    uint64_t e0 = below(300);
    uint64_t groups = every ? (e0 + rows * run) / every + 1 : 1;
    uint64_t f[9] = {0x7f0000001000ull + below(64) * 8, rows, run,
                     run * ss + ((i & 1) ? below(64) : 0), sdt,
                     0x7e0000002000ull + below(16) * 4, every, e0, groups};
    mutate(f, 9);
    AbsmaxArgs in{f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8]};
    AbsmaxSeg g;
    bool has = false;
    if (!accepts([&] { has = absmax_validate(in, g); })) continue;
    u128 total = (u128)in.rows * in.run;
    check(in.sdt <= DT_BF16, "source dtype", who);
    check(has == (total != 0) && total < TOP, "element count", who);
    check(in.out && in.out % 4 == 0 && in.n_groups &&
              (u128)in.out + (u128)in.n_groups * 4 < TOP,
          "slots in range", who);
    if (!has) continue;
    ss = cast_itemsize((uint32_t)in.sdt);
    u128 end = strided_end(in.src, in.rows, in.pitch, (u128)in.run * ss);
    check(end < TOP && in.src && in.src % ss == 0, "source in range", who);
    auto sp = source_span(g.src_ptr, g.rows, g.src_pitch,
                          g.run * cast_itemsize(g.src_dt));
    check(sp.first == in.src && (u128)sp.second == end, "source_span", who);
    u128 top = in.every ? ((u128)in.e0 + total - 1) / in.every : 0;
    check(top < in.n_groups, "groups inside the slots", who);
    check(cast_group_of(g.scale_every, g.scale_e0, g.rows * g.run - 1) ==
              (uint64_t)top, "cast_group_of", who);
  }
}

static void merge_sweep(uint64_t n) {
  for (uint64_t i = 0; i < n; ++i) {
    std::vector<ScaleSlots> in;
    for (uint64_t k = below(8); k > 0; --k)
      in.push_back({0x1000 + below(64) * 4, 1 + below(16)});
    std::vector<ScaleSlots> out = merge_scale_slots(in);
    std::vector<int> want(0x1000 / 4 + 64 + 16 + 1, 0), got(want.size(), 0);
    for (auto& r : in)
      for (uint64_t k = 0; k < r.n; ++k) want[r.ptr / 4 + k] = 1;
    for (auto& r : out)
      for (uint64_t k = 0; k < r.n; ++k) got[r.ptr / 4 + k] += 1;
    check(want == got, "every slot exactly once", "merge_scale_slots");
  }
}

// ---- MX ----

static void mx_check(const char* who, MxKind kind, uint64_t cap,
                     const MxArgs& in, const MxSeg& g) {
  u128 total = (u128)in.rows * in.run;
  check(in.block == MX_BLOCK && in.hp_dt <= DT_BF16 &&
            (in.stored_dt == DT_F8_E4M3 || in.stored_dt == DT_F4),
        "formats", who);
  uint64_t bits = in.stored_dt == DT_F4 ? 4 : 8;
  uint64_t hs = cast_itemsize((uint32_t)in.hp_dt);
  check(total < TOP && total * hs < TOP, "element count", who);
  uint64_t odd = in.run | in.scale_e0 | (in.rows > 1 ? in.scale_pitch : 0);
  if (bits == 4) check(!(odd & 1), "F4 pieces on whole bytes", who);
  if (kind == MX_SCALES) check(odd % 32 == 0, "whole blocks", who);
  if (total == 0) return;
  u128 run_b = (u128)in.run * (kind == MX_LOAD ? bits : hs * 8) / 8;
  u128 end = strided_end(in.a, in.rows, in.pitch, run_b);
  check(end <= (kind == MX_LOAD ? (u128)cap : TOP - 1), "source in range", who);
  check(in.rows == 1 || in.pitch >= run_b, "rows apart", who);
  if (kind == MX_LOAD) {
    check(in.b && in.b % hs == 0 && (u128)in.b + total * hs < TOP,
          "destination in range", who);
  } else {
    check(in.a && in.a % hs == 0, "source aligned", who);
    auto sp = source_span(g.src, g.rows, g.src_pitch, g.run * hs);
    check(sp.first == in.a && (u128)sp.second == end, "source_span", who);
    if (kind == MX_STORE)
      check((u128)in.b + total * bits / 8 <= cap, "destination in range", who);
  }
  u128 t1 = (u128)in.scale_e0 + (u128)(in.rows - 1) * in.scale_pitch +
            in.run - 1;
  u128 first = (u128)in.scale_ptr + in.scale_e0 / 32;
  u128 last = (u128)in.scale_ptr + t1 / 32 + 1;
  check(in.scale_ptr && t1 < TOP && last < TOP, "scales in range", who);
  auto span = mx_scale_span(g);
  check((u128)span.first == first && (u128)span.second == last,
        "mx_scale_span", who);
}

static void mx_sweep(uint64_t n) {
  static const uint64_t stored[] = {DT_F8_E4M3, DT_F4, DT_F8_E5M2};
  for (uint64_t i = 0; i < n; ++i) {
    MxKind kind = (MxKind)(i % 3);
    uint64_t cap = (i & 4) ? 4096 : edge_value();
    uint64_t hp = below(3), st = stored[below(8) ? below(2) : 2];
    uint64_t hs = cast_itemsize((uint32_t)hp), bits = st == DT_F4 ? 4 : 8;
    uint64_t unit = kind == MX_SCALES ? 32 : (below(4) ? 2 : 1);
    uint64_t rows = 1 + below(4), run = below(20) * unit;
    uint64_t run_b = kind == MX_LOAD ? run * bits / 8 : run * hs;
    uint64_t pitch = run_b + ((i & 8) ? below(64) * hs : 0);
    uint64_t e0 = (i & 16) ? below(40) * unit : (U - 4096 + below(4096)) / unit * unit;
    uint64_t spitch = run + below(6) * unit;
    uint64_t arena_off = below(64) * 8, addr = 0x7f0000001000ull + below(64) * 8;
    uint64_t sptr = 0x7e0000002000ull + below(64);
    if (kind == MX_SCALES) {
      uint64_t f[7] = {addr, rows, run, pitch, hp, st, sptr};
      mutate(f, 7);
      MxScaleArgs s{f[0], f[1], f[2], f[3], f[4], f[5], f[6]};
      MxSeg g;
      if (!accepts([&] { g = mx_scales_validate(s); })) continue;
      MxArgs in{s.src, 0, s.rows, s.run, s.pitch, s.hp_dt, s.stored_dt, s.out,
                0, s.run, MX_BLOCK};
      mx_check("mx scales", kind, 0, in, g);
      continue;
    }
    uint64_t f[11] = {kind == MX_LOAD ? arena_off : addr,
                      kind == MX_LOAD ? addr : arena_off, rows, run, pitch, hp,
                      st, sptr, e0, spitch, MX_BLOCK};
    mutate(f, 11);
    MxArgs in{f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], f[9], f[10]};
    MxSeg g;
    const char* who = kind == MX_LOAD ? "mx convert" : "mx store";
    if (!accepts([&] { g = mx_validate(who, kind, cap, in); })) continue;
    mx_check(who, kind, cap, in, g);
  }
}

// ---- block ----

static u128 tile_of(const BlockArgs& in, u128 t, uint64_t tm, uint64_t tn,
                    bool row_end) {
  u128 row = t / in.K, col = row_end ? in.K - 1 : 0;
  return ((row / in.M) * tm + (row % in.M) / in.bm) * tn + col / in.bn;
}

static void block_check(const char* who, BlockKind kind, uint64_t cap,
                        const BlockArgs& in, const BlockSeg& g,
                        uint64_t n_scales) {
  u128 total = (u128)in.rows * in.run;
  check(in.hp_dt <= DT_BF16 && in.stored_dt == DT_F8_E4M3 && in.M && in.K &&
            in.bm && in.bn, "formats and geometry", who);
  uint64_t hs = cast_itemsize((uint32_t)in.hp_dt);
  uint64_t ss = kind == BLOCK_LOAD ? 1 : hs;
  check(total < TOP && total * hs < TOP, "element count", who);
  uint64_t tm = (in.M - 1) / in.bm + 1, tn = (in.K - 1) / in.bn + 1;
  check(g.tm == tm && g.tn == tn, "tile counts", who);
  if (total == 0) return;
  u128 run_b = (u128)in.run * ss;
  u128 end = strided_end(in.a, in.rows, in.pitch, run_b);
  check(end <= (kind == BLOCK_LOAD ? (u128)cap : TOP - 1), "source in range",
        who);
  check(in.rows == 1 || (in.pitch >= run_b && in.pitch % ss == 0 &&
                         in.scale_pitch >= in.run), "rows apart", who);
  if (kind == BLOCK_LOAD) {
    check(in.b && in.b % hs == 0 && (u128)in.b + total * hs < TOP,
          "destination in range", who);
  } else {
    check(in.a && in.a % ss == 0, "source aligned", who);
    auto sp = source_span(g.src, g.rows, g.src_pitch, g.run * hs);
    check(sp.first == in.a && (u128)sp.second == end, "source_span", who);
    if (kind == BLOCK_STORE)
      check((u128)in.b + total <= cap, "destination in range", who);
  }
  u128 t1 = (u128)in.scale_e0 + (u128)(in.rows - 1) * in.scale_pitch +
            in.run - 1;
  u128 lo = tile_of(in, in.scale_e0, tm, tn, false);
  u128 hi = tile_of(in, t1, tm, tn, true);
  check(in.scale_ptr && in.scale_ptr % 4 == 0 && t1 < TOP &&
            (u128)in.scale_ptr + (hi + 1) * 4 < TOP, "scales in range", who);
  auto range = block_scale_range(g);
  check((u128)range.first == lo && (u128)range.second == hi,
        "block_scale_range", who);
  if (n_scales) check(hi < n_scales, "tiles inside the slots", who);
  // every element's own tile lies inside the range
  for (int k = 0; k < 4; ++k) {
    uint64_t r = below(in.rows), c = below(in.run);
    uint64_t idx = block_scale_at(g, r, c);
    check(idx >= range.first && idx <= range.second, "element tile in range",
          who);
  }
}

static void block_sweep(uint64_t n) {
  for (uint64_t i = 0; i < n; ++i) {
    BlockKind kind = (BlockKind)(i % 3);
    uint64_t cap = (i & 4) ? 4096 : edge_value();
    uint64_t hp = below(3), hs = cast_itemsize((uint32_t)hp);
    uint64_t ss = kind == BLOCK_LOAD ? 1 : hs;
    uint64_t M = 1 + below(20), K = 1 + below(40);
    uint64_t bm = 1 + below(M + 3), bn = 1 + below(K + 3);
    uint64_t rows = 1 + below(4), run = below(50);
    uint64_t pitch = run * ss + ((i & 8) ? below(64) * ss : 0);
    uint64_t e0 = (i & 16) ? below(2000) : U - 8192 + below(8192);
    uint64_t spitch = run + below(2 * K);
    uint64_t arena_off = below(64) * 8, addr = 0x7f0000001000ull + below(64) * 8;
    uint64_t sptr = 0x7e0000002000ull + below(64) * 4;
    if (kind == BLOCK_ABSMAX) {
      uint64_t tm = (M - 1) / bm + 1, tn = (K - 1) / bn + 1;
      uint64_t slots = ((e0 + rows * spitch + run) / K / M + 1) * tm * tn;
      if (below(4) == 0) slots = 1 + below(slots + 1);
      uint64_t f[13] = {addr, rows, run, pitch, hp, sptr, e0, spitch,
                        M, K, bm, bn, slots};
      mutate(f, 13);
      BlockAbsmaxArgs s{f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8],
                        f[9], f[10], f[11], f[12]};
      BlockSeg g;
      if (!accepts([&] { g = block_absmax_validate(s); })) continue;
      check(s.out && s.out % 4 == 0 && s.n_slots &&
                (u128)s.out + (u128)s.n_slots * 4 < TOP, "slots in range",
            "block absmax");
      BlockArgs in{s.src, 0, s.rows, s.run, s.pitch, s.hp_dt, DT_F8_E4M3, s.out,
                   s.scale_e0, s.scale_pitch, s.M, s.K, s.bm, s.bn};
      block_check("block absmax", kind, 0, in, g, s.n_slots);
      continue;
    }
    uint64_t f[14] = {kind == BLOCK_LOAD ? arena_off : addr,
                      kind == BLOCK_LOAD ? addr : arena_off, rows, run, pitch,
                      hp, DT_F8_E4M3, sptr, e0, spitch, M, K, bm, bn};
    mutate(f, 14);
    BlockArgs in{f[0], f[1], f[2], f[3], f[4], f[5], f[6], f[7], f[8], f[9],
                 f[10], f[11], f[12], f[13]};
    BlockSeg g;
    const char* who = kind == BLOCK_LOAD ? "block convert" : "block store";
    if (!accepts([&] { g = block_validate(who, kind, cap, in); })) continue;
    block_check(who, kind, cap, in, g, 0);
  }
}

int main() {
  const uint64_t n = 400000;
  struct { const char* name; void (*sweep)(uint64_t); } sweeps[] = {
      {"cast", cast_sweep}, {"absmax", absmax_sweep}, {"merge", merge_sweep},
      {"mx", mx_sweep}, {"block", block_sweep}};
  for (auto& s : sweeps) {
    uint64_t a0 = accepted, r0 = refused, c0 = checks;
    s.sweep(n);
    std::printf("%-6s %llu accepted, %llu refused, %llu checks\n", s.name,
                (unsigned long long)(accepted - a0),
                (unsigned long long)(refused - r0),
                (unsigned long long)(checks - c0));
  }
  std::printf("%llu checks, %llu failures\n", (unsigned long long)checks,
              (unsigned long long)failures);
  return failures ? 1 : 0;
}

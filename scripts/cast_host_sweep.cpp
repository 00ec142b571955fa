// Host-side sanitizer sweep for the typed load/store loops of
// csrc/tensor_cast.hip: store_segment_host and convert_segment_host over
// every source element offset 0..15 x counts x destination element offset
// 0..3, plus strided shapes.  Sources and destinations are heap blocks of
// exactly the touched size, so AddressSanitizer sees any byte read or
// written outside a run; results are compared with cast_one.
//
// Host code only, never run on a GPU machine:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 \
//     -Xarch_host -fsanitize=address,undefined \
//     scripts/cast_host_sweep.cpp -o /tmp/cast_host_sweep && /tmp/cast_host_sweep

#include "../csrc/tensor_cast.hip"

#include <cstdio>
#include <cstdlib>
#include <vector>

static int failures = 0;

static void check(bool ok, const char* what, uint32_t s, uint32_t d,
                  uint64_t a, uint64_t b, uint64_t c) {
  if (ok) return;
  if (failures++ < 20)
    std::fprintf(stderr, "FAIL %s pair %u->%u (%llu, %llu, %llu)\n", what, s, d,
                 (unsigned long long)a, (unsigned long long)b,
                 (unsigned long long)c);
}

// the bytes of element e of a strided source, converted one at a time
static void expect_elem(const uint8_t* src, uint64_t e, uint64_t run,
                        uint64_t pitch, uint32_t s, uint32_t d, uint8_t* out) {
  uint32_t ss = cast_itemsize(s), ds = cast_itemsize(d);
  const uint8_t* p = src + (e / run) * pitch + (e % run) * ss;
  if (s == d) std::memcpy(out, p, ss);
  else {
    alignas(4) uint8_t tmp[4];
    cast_one(p, tmp, s, d);
    std::memcpy(out, tmp, ds);
  }
}

static void one_case(uint32_t s, uint32_t d, uint64_t mis, uint64_t rows,
                     uint64_t run, uint64_t pitch_el, uint64_t doff) {
  uint32_t ss = cast_itemsize(s), ds = cast_itemsize(d);
  uint64_t pitch = pitch_el * ss;
  uint64_t src_b = (rows - 1) * pitch + run * ss;
  uint64_t dst_b = rows * run * ds;
  // exact-size heap blocks: element `mis` of the first, element `doff` of
  // the second are where the segment begins
  std::vector<uint8_t> sbuf(mis * ss + src_b), arena(doff * ds + dst_b),
      dense(dst_b + 8);
  for (size_t i = 0; i < sbuf.size(); ++i)
    sbuf[i] = (uint8_t)((i * 131u + 7u) ^ (i >> 8));
  CastSeg g;
  g.rows = rows; g.run = run; g.src_pitch = pitch; g.src_dt = s; g.dst_dt = d;

  // store: absolute source -> arena offset
  g.src_off = (uint64_t)(uintptr_t)(sbuf.data() + mis * ss);
  g.dst_ptr = doff * ds;
  store_segment_host(arena.data(), g);
  // convert: arena offset -> absolute dense destination
  uint8_t* dd = dense.data() + ((0 - (uintptr_t)dense.data()) & 7);
  g.src_off = mis * ss;
  g.dst_ptr = (uint64_t)(uintptr_t)dd;
  convert_segment_host(sbuf.data(), g);

  uint8_t exp[8];
  for (uint64_t e = 0; e < rows * run; ++e) {
    expect_elem(sbuf.data() + mis * ss, e, run, pitch, s, d, exp);
    check(!std::memcmp(exp, arena.data() + (doff + e) * ds, ds), "store", s, d,
          mis, rows * run, e);
    check(!std::memcmp(exp, dd + e * ds, ds), "convert", s, d, mis,
          rows * run, e);
  }
}

int main() {
  const uint32_t pairs[][2] = {
      {DT_F32, DT_BF16}, {DT_BF16, DT_F16}, {DT_BF16, DT_F32},
      {DT_F32, DT_F16},  {DT_F16, DT_F32},  {DT_F8_E4M3, DT_BF16},
      {DT_F8_E5M2, DT_F32}, {DT_I8, DT_I8}, {DT_I64, DT_I64},
      {DT_BF16, DT_BF16}};
  const uint64_t counts[] = {1, 2, 3, 7, 8, 9, 63, 64, 65, 4097};
  const uint64_t shapes[][3] = {{5, 4, 12}, {4097, 3, 7}, {9, 5000, 5003},
                                {3, 64, 64}, {700, 63, 65}};
  uint64_t n_cases = 0;
  for (auto& p : pairs) {
    for (uint64_t mis = 0; mis < 16; ++mis)
      for (uint64_t n : counts)
        for (uint64_t doff = 0; doff < 4; ++doff, ++n_cases)
          one_case(p[0], p[1], mis, 1, n, n, doff);
    for (auto& sh : shapes)
      for (uint64_t mis = 0; mis < 2; ++mis, ++n_cases)
        one_case(p[0], p[1], mis, sh[0], sh[1], sh[2], 1);
  }
  std::printf("%llu cases, %d failures\n", (unsigned long long)n_cases,
              failures);
  return failures ? 1 : 0;
}

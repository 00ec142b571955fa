// Host-side sanitizer sweep for the host twin of csrc/array_gather.hip:
// array_samples_host and array_sample_host over the shapes of the test
// cases: 16x16xC with every byte value, 5x7x3 at every source residue
// 0..15 with every 3x5 crop and both flips, 9x11xC cut at every byte into
// two pieces and into three with a one-byte middle piece, and 61x67x3 cut
// around ARRAY_TILE, for the three destination dtypes and both layouts.
// The source is a heap block that ends with the sample's last byte, the
// destination a heap block of exactly batch * C*h*w elements, so
// AddressSanitizer sees any byte read or written outside them; results are
// compared with loops written here, and the elements no piece covers must
// keep their sentinel.
//
// Host code only, never run on a GPU machine:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 \
//     -Xarch_host -fsanitize=address,undefined \
//     scripts/array_host_sweep.cpp -o /tmp/array_host_sweep && \
//     /tmp/array_host_sweep

#include "../csrc/tensor_cast.hip"
#include "../csrc/array_gather.hip"

#include <cstdio>
#include <vector>

static int failures = 0;
static uint64_t checks = 0;

static void check(bool ok, const char* what, uint64_t a, uint64_t b,
                  uint64_t c) {
  ++checks;
  if (ok) return;
  if (failures++ < 20)
    std::fprintf(stderr, "FAIL %s (%llu, %llu, %llu)\n", what,
                 (unsigned long long)a, (unsigned long long)b,
                 (unsigned long long)c);
}

static const uint64_t kBatch = 3;
static const uint8_t kSentinel = 0xAB;

// the reference: two separately rounded f32 steps, then the cast written
// out with the compiler's own narrow types
static uint32_t ref_bits(uint8_t v, float scale, float bias, uint32_t ddt) {
  volatile float t = (float)v * scale;          // volatile: rounded here
  volatile float r = t + bias;
  float f = r;
  if (ddt == DT_F16) {
    _Float16 hf = (_Float16)f;
    uint16_t u;
    std::memcpy(&u, &hf, 2);
    return u;
  }
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if (ddt == DT_BF16) return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;  // finite
  return u;
}

static uint32_t read_dst(const std::vector<uint8_t>& d, uint64_t e,
                         uint32_t ds) {
  if (ds == 4) {
    uint32_t v;
    std::memcpy(&v, d.data() + e * 4, 4);
    return v;
  }
  uint16_t v;
  std::memcpy(&v, d.data() + e * 2, 2);
  return v;
}

static ArrayShape make_shape(uint32_t H, uint32_t W, uint32_t C, uint32_t h,
                             uint32_t w, uint32_t layout, uint32_t seed) {
  ArrayShape p{H, W, C, h, w, layout, {0, 0, 0, 0}, {0, 0, 0, 0}};
  const float scales[4] = {1.0f / (255.0f * 0.229f), 1.0f / 255.0f, 1000.0f,
                           1e-7f};
  const float biases[4] = {-0.485f / 0.229f, 0.0f, -3.0f, 0.5f};
  for (uint32_t c = 0; c < C; ++c) {
    p.scale[c] = scales[(seed + c) % 4];
    p.bias[c] = biases[(seed + 2 * c) % 4];
  }
  return p;
}

// one sample at residue r, cut at c1 <= c2 (equal cuts or a cut at 0 or n
// give fewer pieces), pieces [first, last] of the three passed on, last one
// first, landing in row `row`
static void sweep_one(const ArrayShape& p, uint32_t ddt, ArrayRow a,
                      uint32_t r, uint64_t c1, uint64_t c2, uint64_t row,
                      int first, int last, uint32_t seed) {
  uint32_t ds = cast_itemsize(ddt);
  uint64_t n = (uint64_t)p.H * p.W * p.C;
  uint64_t out_el = (uint64_t)p.C * p.h * p.w;
  std::vector<uint8_t> src(r + n);
  for (uint64_t i = 0; i < n; ++i)
    src[r + i] = (uint8_t)((seed * 2654435761u + (uint32_t)i * 40503u) >> 13);
  std::vector<uint8_t> out(kBatch * out_el * ds, kSentinel);
  std::vector<ArrayRow> rows(kBatch, ArrayRow{0, 0, 0});
  rows[row] = a;
  uint64_t cuts[4] = {0, c1, c2, n};
  std::vector<char> covered(n, 0);
  for (int k = last; k >= first; --k) {
    if (cuts[k] == cuts[k + 1]) continue;
    ArrayPiece g{r + cuts[k], row, cuts[k], cuts[k + 1] - cuts[k]};
    array_samples_host(src.data(), g, rows.data(), out.data(), p, ddt);
    for (uint64_t e = cuts[k]; e < cuts[k + 1]; ++e) covered[e] = 1;
  }
  uint32_t sent = ds == 4 ? 0xABABABABu : 0xABABu;
  for (uint64_t rr = 0; rr < kBatch; ++rr)
    for (uint32_t c = 0; c < p.C; ++c)
      for (uint32_t y = 0; y < p.h; ++y)
        for (uint32_t q = 0; q < p.w; ++q) {
          uint32_t xs = a.dx + (a.flip ? p.w - 1 - q : q);
          uint64_t e = ((uint64_t)(a.dy + y) * p.W + xs) * p.C + c;
          uint64_t at = p.layout == ARRAY_NHWC
                            ? ((rr * p.h + y) * p.w + q) * p.C + c
                            : ((rr * p.C + c) * p.h + y) * p.w + q;
          uint32_t ex = sent;
          if (rr == row && covered[e])
            ex = ref_bits(src[r + e], p.scale[c], p.bias[c], ddt);
          check(read_dst(out, at, ds) == ex, "element", ddt * 2 + p.layout, e,
                at);
        }
  if (first == 0 && last == 2) {
    // the whole sample through the slow path's routine: the same bytes
    std::vector<uint8_t> one(out_el * ds, kSentinel);
    array_sample_host(src.data() + r, a, one.data(), p, ddt);
    check(std::memcmp(one.data(), out.data() + row * out_el * ds,
                      out_el * ds) == 0, "sample", ddt, p.layout, r);
  }
}

int main() {
  const uint32_t dts[3] = {DT_F32, DT_F16, DT_BF16};
  uint32_t seed = 1;
  for (uint32_t ddt : dts)
    for (uint32_t layout : {ARRAY_NCHW, ARRAY_NHWC}) {
      check(array_dst_supported(ddt), "dtype", ddt, 0, 0);
      // exhaustive values: every byte value in every channel
      for (uint32_t C = 1; C <= 4; ++C)
        for (uint32_t s = 0; s < 4; ++s) {
          ArrayShape p = make_shape(16, 16, C, 16, 16, layout, s);
          for (uint32_t c = 0; c < C; ++c) {
            p.scale[c] = p.scale[0];
            p.bias[c] = p.bias[0];
          }
          sweep_one(p, ddt, ArrayRow{0, 0, 0}, s, 0, 0, s % kBatch, 0, 2,
                    seed++);
        }
      for (uint32_t v = 0; v < 256; ++v) {
        ArrayShape p = make_shape(1, 1, 1, 1, 1, layout, v);
        uint8_t b = (uint8_t)v;
        uint32_t word = 0;
        array_sample_host(&b, ArrayRow{0, 0, 0}, (uint8_t*)&word, p, ddt);
        check(word == ref_bits(b, p.scale[0], p.bias[0], ddt), "value", ddt,
              v, word);
      }
      // residues: 5x7x3, crop 3x5 at every place, both flips
      for (uint32_t r = 0; r < 16; ++r)
        for (uint32_t dy = 0; dy <= 2; ++dy)
          for (uint32_t dx = 0; dx <= 2; ++dx)
            for (uint32_t flip = 0; flip <= 1; ++flip) {
              ArrayShape p = make_shape(5, 7, 3, 3, 5, layout, seed);
              sweep_one(p, ddt, ArrayRow{dy, dx, flip}, r, 0, 0,
                        (r + dy) % kBatch, 0, 2, seed++);
            }
      // splits: 9x11xC, crop 7x8 at (1, 2)
      for (uint32_t C = 3; C <= 4; ++C)
        for (uint32_t flip = 0; flip <= 1; ++flip) {
          ArrayShape p = make_shape(9, 11, C, 7, 8, layout, seed);
          ArrayRow a{1, 2, flip};
          uint64_t n = 9 * 11 * C;
          for (uint64_t k = 1; k < n; ++k) {
            sweep_one(p, ddt, a, (uint32_t)(k % 16), k, k, k % kBatch, 0, 2,
                      seed++);
            sweep_one(p, ddt, a, (uint32_t)(k % 16), k, k + 1 < n ? k + 1 : n,
                      k % kBatch, 0, 2, seed++);
          }
          // one piece of two only: the rest keeps the sentinel
          sweep_one(p, ddt, a, 3, n / 2, n / 2, 1, 0, 0, seed++);
          sweep_one(p, ddt, a, 5, n / 2, n / 2, 2, 2, 2, seed++);
        }
      // long: 61x67x3, crops 53x64 and 53x63, cut around the tile
      for (uint32_t w : {64u, 63u})
        for (uint64_t cut : {(uint64_t)0, (uint64_t)ARRAY_TILE - 1,
                             (uint64_t)ARRAY_TILE, (uint64_t)ARRAY_TILE + 1}) {
          ArrayShape p = make_shape(61, 67, 3, 53, w, layout, seed);
          sweep_one(p, ddt, ArrayRow{8, 67 - w, 1}, 1, cut, cut, 0, 0, 2, seed++);
          sweep_one(p, ddt, ArrayRow{0, 0, 0}, 2, cut, 2 * cut, 1, 0, 2, seed++);
          sweep_one(p, ddt, ArrayRow{4, 1, 1}, 15, cut, cut, 2, 0, 2, seed++);
        }
    }
  check(!array_dst_supported(DT_U8), "dtype", DT_U8, 1, 0);
  check(!array_dst_supported(DT_I64), "dtype", DT_I64, 1, 0);
  check(!array_dst_supported(DT_F64), "dtype", DT_F64, 1, 0);
  std::printf("%llu checks, %d failures\n", (unsigned long long)checks,
              failures);
  return failures ? 1 : 0;
}

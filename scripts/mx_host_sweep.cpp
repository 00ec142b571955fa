// Host-side sanitizer sweep for the MX loops of csrc/mx_cast.hip:
// mx_scales_segment_host, mx_store_segment_host and mx_load_segment_host
// over all 65 536 F16 and BF16 patterns (one per block beside an anchor
// that sets the scale, three anchors), F32 subnormals, and every element
// code under every scale byte for the three destination dtypes.  Sources,
// scales and destinations are heap blocks of exactly the touched size, so
// AddressSanitizer sees any byte read or written outside them; results are
// compared with a double-precision reference (ldexp + nearbyint).
//
// Host code only, never run on a GPU machine:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 \
//     -Xarch_host -fsanitize=address,undefined \
//     scripts/mx_host_sweep.cpp -o /tmp/mx_host_sweep && /tmp/mx_host_sweep

#include "../csrc/tensor_cast.hip"
#include "../csrc/mx_cast.hip"

#include <cmath>
#include <cstdio>
#include <vector>

static int failures = 0;

static void check(bool ok, const char* what, uint64_t a, uint64_t b,
                  uint64_t c) {
  if (ok) return;
  if (failures++ < 20)
    std::fprintf(stderr, "FAIL %s (%llu, %llu, %llu)\n", what,
                 (unsigned long long)a, (unsigned long long)b,
                 (unsigned long long)c);
}

static double code_value(uint32_t mag, uint32_t fmt) {
  if (fmt == MX_E2M1) {
    static const double t[8] = {0, 0.5, 1, 1.5, 2, 3, 4, 6};
    return t[mag];
  }
  uint32_t e = mag >> 3, m = mag & 7u;
  return e ? std::ldexp(8.0 + m, (int)e - 10) : std::ldexp((double)m, -9);
}

static uint32_t ref_quant(float x, uint32_t s, uint32_t fmt) {
  uint32_t sign = std::signbit(x) ? (fmt == MX_E2M1 ? 8u : 0x80u) : 0u;
  uint32_t top = fmt == MX_E2M1 ? 7u : 0x7Eu;
  if (std::isnan(x)) return sign | (fmt == MX_E2M1 ? 7u : 0x7Fu);
  if (std::isinf(x)) return sign | top;
  double v = std::ldexp(std::fabs((double)x), 127 - (int)s);
  int ex;
  std::frexp(v, &ex);
  int mb = fmt == MX_E2M1 ? 1 : 3, emin = fmt == MX_E2M1 ? 0 : -6;
  int qe = (v == 0 || ex - 1 < emin ? emin : ex - 1) - mb;
  double r = std::ldexp(std::nearbyint(std::ldexp(v, -qe)), qe);
  if (r >= code_value(top, fmt)) return sign | top;
  for (uint32_t c = 0; c <= top; ++c)
    if (code_value(c, fmt) == r) return sign | c;
  return 0xFFFFu;                       // off the grid: never
}

static void store_sweep(uint32_t sdt, uint32_t fmt, const std::vector<float>& xs) {
  uint64_t n = xs.size();               // a multiple of 32
  uint32_t ss = cast_itemsize(sdt);
  std::vector<uint8_t> src(n * ss), scales(n / 32), out(n * mx_bits(fmt) / 8);
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t f = cast_bits_of(xs[i]);
    uint32_t b = sdt == DT_F32 ? f : sdt == DT_BF16 ? f >> 16
                                                    : cvt_f32_to_f16(f);
    std::memcpy(src.data() + i * ss, &b, ss);
  }
  MxSeg g;
  g.src = (uint64_t)(uintptr_t)src.data(); g.dst = 0; g.rows = 1; g.run = n;
  g.src_pitch = 0; g.scale_ptr = (uint64_t)(uintptr_t)scales.data();
  g.scale_e0 = 0; g.scale_pitch = n; g.dt = sdt; g.fmt = fmt;
  mx_scales_segment_host(g);
  mx_store_segment_host(src.data(), out.data(), g);
  for (uint64_t b = 0; b < n / 32; ++b) {
    float amax = 0;
    for (int k = 0; k < 32; ++k) {
      float a = std::fabs(xs[b * 32 + k]);
      if (std::isfinite(a) && a > amax) amax = a;
    }
    uint32_t e = (cast_bits_of(amax) >> 23) & 0xFFu, em = fmt == MX_E2M1 ? 2 : 8;
    check(scales[b] == (e > em ? e - em : 0), "scale", sdt, fmt, b);
    for (int k = 0; k < 32; ++k) {
      uint64_t i = b * 32 + k;
      uint32_t got = fmt == MX_E2M1 ? (out[i / 2] >> ((i & 1) * 4)) & 0xFu
                                    : out[i];
      check(got == ref_quant(xs[i], scales[b], fmt), "quant", sdt, fmt, i);
    }
  }
}

static void load_sweep(uint32_t fmt, uint32_t ddt) {
  uint32_t n_codes = fmt == MX_E2M1 ? 16 : 256, per = n_codes < 32 ? 32 : n_codes;
  uint64_t n = 256ull * per;
  std::vector<uint8_t> src(n * mx_bits(fmt) / 8), scales(n / 32),
      out(n * cast_itemsize(ddt));
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t c = (uint32_t)(i % n_codes);
    if (fmt == MX_E2M1) src[i / 2] |= (uint8_t)(c << ((i & 1) * 4));
    else src[i] = (uint8_t)c;
  }
  for (uint64_t b = 0; b < n / 32; ++b) scales[b] = (uint8_t)(b * 32 / per);
  MxSeg g;
  g.src = 0; g.dst = (uint64_t)(uintptr_t)out.data(); g.rows = 1; g.run = n;
  g.src_pitch = 0; g.scale_ptr = (uint64_t)(uintptr_t)scales.data();
  g.scale_e0 = 0; g.scale_pitch = n; g.dt = ddt; g.fmt = fmt;
  mx_load_segment_host(src.data(), out.data(), g);
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t c = (uint32_t)(i % n_codes), s = scales[i / 32];
    uint32_t sb = fmt == MX_E2M1 ? 8u : 0x80u;
    bool nan = s == 255 || (fmt == MX_E4M3 && (c & 0x7Fu) == 0x7Fu);
    double v = nan ? 0 : std::ldexp(code_value(c & (sb - 1), fmt), (int)s - 127);
    float f = (float)((c & sb) ? -v : v);          // exact or overflow to inf
    uint32_t exp = cvt_from_f32(cast_bits_of(f), ddt), got = 0;
    std::memcpy(&got, out.data() + i * cast_itemsize(ddt), cast_itemsize(ddt));
    if (nan) {
      uint32_t f32 = cvt_to_f32(got, ddt);
      check((f32 & 0x7FFFFFFFu) > 0x7F800000u, "nan", fmt, ddt, i);
    } else {
      check(got == exp, "dequant", fmt, ddt, i);
    }
  }
}

int main() {
  for (uint32_t fmt = 0; fmt < MX_FMT_COUNT; ++fmt) {
    for (uint32_t sdt : {DT_F16, DT_BF16}) {
      const float anchors[3] = {1.0f, sdt == DT_F16 ? 16384.0f : 0x1p60f,
                                sdt == DT_F16 ? 0x1p-14f : 0x1p-60f};
      for (float a : anchors) {
        std::vector<float> xs(65536 * 32, 0.0f);
        for (uint32_t p = 0; p < 65536; ++p) {
          xs[p * 32] = cast_f32_of(cvt_to_f32(p, sdt));
          xs[p * 32 + 1] = a;
          xs[p * 32 + 2] = -a / 4;
        }
        store_sweep(sdt, fmt, xs);
      }
    }
    // F32: subnormal sources, ties around every grid point of a block
    // whose scale byte is 127, and blocks of subnormals only
    std::vector<float> xs;
    float anchor = fmt == MX_E2M1 ? 4.0f : 256.0f;
    for (int i = 0; i < 31 * 600; ++i) {
      if (i % 31 == 0 && i) xs.push_back(anchor);
      float base = (float)(i % 1200) * anchor / 1024.0f;
      xs.push_back(std::nextafterf(base, (i & 1) ? 1e9f : -1e9f) *
                   ((i & 2) ? -1.0f : 1.0f));
    }
    xs.push_back(anchor);
    for (uint32_t i = 0; i < 32 * 64; ++i)
      xs.push_back(cast_f32_of((i * 4099u + 1u) & 0x807FFFFFu));
    xs.resize(xs.size() / 32 * 32);
    store_sweep(DT_F32, fmt, xs);
    for (uint32_t ddt : {DT_F32, DT_F16, DT_BF16}) load_sweep(fmt, ddt);
  }
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}

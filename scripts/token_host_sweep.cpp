// Host-side sanitizer sweep for the host twin of csrc/token_gather.hip:
// token_windows_host over every dtype pair, every source residue 0..15,
// every split of a window into two pieces and a set of three-piece splits,
// for small T, with and without a vocabulary.  The source is a heap block
// that ends with the window's last byte, x and y are heap blocks of exactly
// batch * T elements, so AddressSanitizer sees any byte read or written
// outside them; results are compared with a loop written here, and the
// elements no piece covers must keep their sentinel.
//
// Host code only, never run on a GPU machine:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 \
//     -Xarch_host -fsanitize=address,undefined \
//     scripts/token_host_sweep.cpp -o /tmp/token_host_sweep && \
//     /tmp/token_host_sweep

#include "../csrc/tensor_cast.hip"
#include "../csrc/token_gather.hip"

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

static const uint32_t kSpecial[] = {0u, 0x7FFFu, 0x8000u, 0xFFFFu, 0x7FFFFFFFu,
                                    0x80000000u, 0xFFFFFFFFu, 999u, 1000u};
static const uint64_t kBatch = 3, kSentinel = 0xABABABABABABABABull;

// the reference: what token j of a window is worth, written out here
static int64_t ref_value(uint32_t bits, uint32_t sdt) {
  if (sdt == DT_U16) return (int64_t)(bits & 0xFFFFu);
  if (sdt == DT_U32) return (int64_t)bits;
  return (int64_t)(int32_t)bits;
}

static bool ref_bad(int64_t v, uint64_t vocab) {
  return vocab && (v < 0 || (uint64_t)v >= vocab);
}

static int64_t read_dst(const std::vector<uint8_t>& d, uint64_t e, uint32_t ds) {
  if (ds == 8) {
    int64_t v;
    std::memcpy(&v, d.data() + e * 8, 8);
    return v;
  }
  int32_t v;
  std::memcpy(&v, d.data() + e * 4, 4);
  return v;
}

// one window of T + 1 tokens at residue r, cut at c1 <= c2 (equal cuts or a
// cut at 0 or T + 1 give fewer pieces), landing in row `row`
static void sweep_one(uint32_t sdt, uint32_t ddt, uint64_t T, uint32_t r,
                      uint64_t c1, uint64_t c2, uint64_t row, uint64_t vocab,
                      uint32_t seed) {
  uint32_t ss = cast_itemsize(sdt), ds = cast_itemsize(ddt);
  uint64_t n = T + 1;
  std::vector<uint8_t> src(r + n * ss);
  std::vector<uint32_t> bits(n);
  for (uint64_t i = 0; i < n; ++i) {
    uint32_t b = kSpecial[(seed + i * 7u) % 9u];
    if ((seed + i) % 4u == 3u) b = (seed * 2654435761u + (uint32_t)i * 40503u);
    if (ss == 2) b &= 0xFFFFu;
    bits[i] = b;
    std::memcpy(src.data() + r + i * ss, &b, ss);
  }
  std::vector<uint8_t> x(kBatch * T * ds, 0xAB), y(kBatch * T * ds, 0xAB);
  uint64_t cuts[4] = {0, c1, c2, n}, got = 0;
  for (int p = 2; p >= 0; --p) {               // last piece first
    if (cuts[p] == cuts[p + 1]) continue;
    TokenPiece g{r + cuts[p] * ss, row, cuts[p], cuts[p + 1] - cuts[p]};
    got += token_windows_host(src.data(), g, x.data(), y.data(), T, sdt, ddt,
                              vocab);
  }
  uint64_t exp_bad = 0;
  int64_t sent = ds == 8 ? (int64_t)kSentinel : (int64_t)(int32_t)kSentinel;
  for (uint64_t i = 0; i < n; ++i)
    exp_bad += ref_bad(ref_value(bits[i], sdt), vocab);
  check(got == exp_bad, "count", sdt, T, got);
  for (uint64_t rr = 0; rr < kBatch; ++rr)
    for (uint64_t j = 0; j < T; ++j) {
      int64_t ex = sent, ey = sent;
      if (rr == row) {
        ex = ref_value(bits[j], sdt);
        ey = ref_value(bits[j + 1], sdt);
        if (ds == 4) { ex = (int32_t)ex; ey = (int32_t)ey; }
      }
      check(read_dst(x, rr * T + j, ds) == ex, "x", sdt * 16 + ddt, T, j);
      check(read_dst(y, rr * T + j, ds) == ey, "y", sdt * 16 + ddt, T, j);
    }
}

int main() {
  const uint32_t pairs[5][2] = {{DT_U16, DT_I32}, {DT_U16, DT_I64},
                                {DT_U32, DT_I64}, {DT_I32, DT_I32},
                                {DT_I32, DT_I64}};
  uint32_t seed = 1;
  for (auto& p : pairs) {
    check(token_pair_supported(p[0], p[1]), "pair", p[0], p[1], 0);
    for (uint64_t T = 1; T <= 12; ++T)
      for (uint32_t r = 0; r < 16; ++r)
        for (uint64_t vocab : {(uint64_t)0, (uint64_t)1000}) {
          // every two-piece split, the unsplit window among them
          for (uint64_t c = 0; c <= T; ++c)
            sweep_one(p[0], p[1], T, r, c, c, (r + c) % kBatch, vocab, seed++);
          // three pieces: token 0 alone, token T alone, and a middle cut
          for (uint64_t c = 1; c <= T; ++c)
            sweep_one(p[0], p[1], T, r, 1 < c ? 1 : c, c < T ? c : T,
                      (r + c) % kBatch, vocab, seed++);
          sweep_one(p[0], p[1], T, r, 1, T, r % kBatch, vocab, seed++);
        }
  }
  check(!token_pair_supported(DT_U32, DT_I32), "pair", DT_U32, DT_I32, 1);
  check(!token_pair_supported(DT_U16, DT_U16), "pair", DT_U16, DT_U16, 1);
  check(!token_pair_supported(DT_U8, DT_I64), "pair", DT_U8, DT_I64, 1);
  std::printf("%llu checks, %d failures\n", (unsigned long long)checks,
              failures);
  return failures ? 1 : 0;
}

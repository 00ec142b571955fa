// Host-side sanitizer sweep for the host twin of csrc/token_docs.hip:
// token_docs_host over both dtypes, rows 1..3, every T in 1..20 and every
// eos pattern of a row that 2^min(T, 10) bit masks describe (shifted per
// row), plus rows longer than a chunk with eos around the chunk edge, for
// every subset of the three outputs.  x, position_ids and doc_ids are heap
// blocks of exactly rows * T elements and cu_seqlens one of exactly
// rows * T + 1 int32, so AddressSanitizer sees any byte read or written
// outside them; results are compared with a loop written here, and the
// cu_seqlens entries past n_seqs + 1 must keep their sentinel.
//
// Host code only, never run on a GPU machine:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 \
//     -Xarch_host -fsanitize=address,undefined \
//     scripts/token_docs_host_sweep.cpp -o /tmp/token_docs_host_sweep && \
//     /tmp/token_docs_host_sweep

#include "../csrc/tensor_cast.hip"
#include "../csrc/token_gather.hip"
#include "../csrc/token_docs.hip"

#include <cstdio>
#include <cstring>
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

static const int64_t kEos = 5;
// ids that must not match: neighbours, the eos with high bits, negatives
static const int64_t kOther64[] = {0, 4, 6, kEos + (1ll << 32), -1,
                                   kEos - (1ll << 32), INT64_MIN, INT64_MAX};
static const int32_t kOther32[] = {0, 4, 6, -1, INT32_MIN, INT32_MAX,
                                   (int32_t)(kEos - (1ll << 31)), 70000};

static int64_t read_el(const std::vector<uint8_t>& d, uint64_t e, uint32_t ds) {
  if (ds == 8) {
    int64_t v;
    std::memcpy(&v, d.data() + e * 8, 8);
    return v;
  }
  int32_t v;
  std::memcpy(&v, d.data() + e * 4, 4);
  return v;
}

// eos[r * T + t] says where the eos sit; `outs` bit 0: position_ids, bit 1:
// doc_ids, bit 2: cu_seqlens
static void sweep_one(uint32_t dt, uint64_t rows, uint64_t T,
                      const std::vector<uint8_t>& eos, unsigned outs,
                      uint32_t seed) {
  uint32_t ds = cast_itemsize(dt);
  uint64_t n = rows * T;
  std::vector<uint8_t> x(n * ds), pos(n * ds, 0xAB), doc(n * ds, 0xAB);
  std::vector<int32_t> cu(n + 1, (int32_t)0xABABABAB);
  for (uint64_t i = 0; i < n; ++i) {
    if (ds == 8) {
      int64_t v = eos[i] ? kEos : kOther64[(seed + i * 5u) % 8u];
      std::memcpy(x.data() + i * 8, &v, 8);
    } else {
      int32_t v = eos[i] ? (int32_t)kEos : kOther32[(seed + i * 5u) % 8u];
      std::memcpy(x.data() + i * 4, &v, 4);
    }
  }
  uint64_t n_seqs = ~0ull, max_seqlen = ~0ull;
  token_docs_host(x.data(), rows, T, ds, (uint64_t)kEos,
                  (outs & 1) ? pos.data() : nullptr,
                  (outs & 2) ? doc.data() : nullptr,
                  (outs & 4) ? cu.data() : nullptr, n_seqs, max_seqlen);
  // the reference, from the definitions
  std::vector<int64_t> starts;
  uint64_t longest = 0;
  int64_t sent = ds == 8 ? (int64_t)0xABABABABABABABABull
                         : (int64_t)(int32_t)0xABABABAB;
  for (uint64_t r = 0; r < rows; ++r)
    for (uint64_t t = 0; t < T; ++t) {
      uint64_t docs = 0, start = 0;
      for (uint64_t s = 0; s < t; ++s)
        if (eos[r * T + s]) {
          docs++;
          start = s + 1;
        }
      if (t == 0 || eos[r * T + t - 1]) starts.push_back((int64_t)(r * T + t));
      check(read_el(pos, r * T + t, ds) ==
                ((outs & 1) ? (int64_t)(t - start) : sent), "pos", T, r, t);
      check(read_el(doc, r * T + t, ds) ==
                ((outs & 2) ? (int64_t)docs : sent), "doc", T, r, t);
    }
  starts.push_back((int64_t)n);
  for (size_t k = 1; k < starts.size(); ++k)
    if ((uint64_t)(starts[k] - starts[k - 1]) > longest)
      longest = (uint64_t)(starts[k] - starts[k - 1]);
  check(n_seqs == starts.size() - 1, "n_seqs", T, n_seqs, starts.size() - 1);
  check(max_seqlen == longest, "max_seqlen", T, max_seqlen, longest);
  for (uint64_t k = 0; k <= n; ++k) {
    int32_t e = (outs & 4) && k < starts.size() ? (int32_t)starts[k]
                                                : (int32_t)0xABABABAB;
    check(cu[k] == e, "cu", T, k, (uint64_t)(int64_t)cu[k]);
  }
}

int main() {
  uint32_t seed = 1;
  for (uint32_t dt : {(uint32_t)DT_I32, (uint32_t)DT_I64}) {
    for (uint64_t rows = 1; rows <= 3; ++rows)
      for (uint64_t T = 1; T <= 20; ++T) {
        uint64_t bits = T < 10 ? T : 10;
        for (uint64_t m = 0; m < (1ull << bits); ++m) {
          std::vector<uint8_t> eos(rows * T);
          for (uint64_t r = 0; r < rows; ++r)
            for (uint64_t t = 0; t < T; ++t)
              eos[r * T + t] = ((m * (r + 1) + r) >> (t % bits)) & 1u;
          sweep_one(dt, rows, T, eos, (unsigned)((m + T) % 8u), seed++);
        }
        std::vector<uint8_t> all(rows * T, 1), none(rows * T, 0);
        for (unsigned outs = 0; outs < 8; ++outs) {
          sweep_one(dt, rows, T, all, outs, seed++);
          sweep_one(dt, rows, T, none, outs, seed++);
        }
      }
    // rows longer than a chunk: eos around the chunk edge and at the row end
    for (uint64_t T : {(uint64_t)TOKEN_DOC_CHUNK, (uint64_t)TOKEN_DOC_CHUNK + 1})
      for (unsigned outs : {7u, 4u, 1u}) {
        std::vector<uint8_t> eos(2 * T);
        eos[TOKEN_DOC_CHUNK - 1] = 1;
        eos[T + 3] = 1;
        eos[2 * T - 1] = 1;
        sweep_one(dt, 2, T, eos, outs, seed++);
      }
  }
  std::printf("%llu checks, %d failures\n", (unsigned long long)checks,
              failures);
  return failures ? 1 : 0;
}

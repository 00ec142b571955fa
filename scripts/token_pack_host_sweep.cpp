// Host-side sanitizer sweep for the host twins of csrc/token_pack.hip,
// randomised against naive loops written here.
//
// token_eos_host: all three source dtypes, one to three spans of random
// lengths at random byte offsets of a heap block of exactly the bytes the
// spans need, random eos density, every capacity from 0 to total + 1.
//
// token_pack_host: every supported dtype pair, random batches: rows of
// random segments (source segments with and without TOKEN_SEG_NEXT, pad
// segments, gaps that nothing covers), every source segment cut into random
// pieces that sit apart at random byte offsets, pieces left out at random,
// every subset of the optional outputs, with and without a vocabulary.  The
// outputs are heap blocks of exactly rows * T elements (cu_seqlens exactly
// n_segments + 1), so AddressSanitizer sees any byte read or written outside
// them, and columns nothing covers must keep their sentinel.
//
// Host code only, never run on a GPU machine:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 \
//     -Xarch_host -fsanitize=address,undefined \
//     scripts/token_pack_host_sweep.cpp -o /tmp/token_pack_host_sweep && \
//     /tmp/token_pack_host_sweep

#include "../csrc/tensor_cast.hip"
#include "../csrc/token_gather.hip"
#include "../csrc/token_docs.hip"
#include "../csrc/token_pack.hip"

#include <cstdio>
#include <cstring>
#include <random>
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

static std::mt19937_64 rng(12345);

static uint64_t below(uint64_t n) { return rng() % n; }

// the value of a raw source token, as the destination sees it
static int64_t naive_widen(uint32_t bits, uint32_t sdt) {
  if (sdt == DT_U16) return (int64_t)(bits & 0xFFFFu);
  if (sdt == DT_U32) return (int64_t)bits;
  return (int64_t)(int32_t)bits;
}

static uint32_t random_token(uint32_t sdt, bool small) {
  static const uint32_t special[] = {0, 5, 0x7FFF, 0x8000, 0xFFFF, 0x7FFFFFFF,
                                     0x80000000u, 0xFFFFFFFFu, 0x80000005u};
  uint32_t v = small ? (uint32_t)below(8)
               : below(3) == 0 ? special[below(9)] : (uint32_t)rng();
  return sdt == DT_U16 ? (v & 0xFFFFu) : v;
}

static void put_token(uint8_t* p, uint32_t bits, uint32_t ss) {
  std::memcpy(p, &bits, ss);
}

// ------------------------------------------------------------------ eos index

static void sweep_eos(uint32_t sdt) {
  uint32_t ss = cast_itemsize(sdt);
  uint64_t n_spans = 1 + below(3), bytes = 0, tok = below(50);
  std::vector<TokenSpan> spans;
  for (uint64_t i = 0; i < n_spans; ++i) {
    uint64_t n = 1 + below(below(4) == 0 ? 600 : 20);
    bytes += below(5);                          // any byte offset
    spans.push_back({bytes, tok, n});
    bytes += n * ss;
    tok += n + below(30);
  }
  std::vector<uint8_t> src(bytes, 0xCD);
  bool small = below(2);
  uint64_t eos = small ? below(8)
                 : (uint64_t)naive_widen(random_token(sdt, false), sdt);
  if ((int64_t)eos < 0) eos = 5;               // a negative id is no eos
  std::vector<int64_t> want;
  for (auto& g : spans)
    for (uint64_t i = 0; i < g.n; ++i) {
      uint32_t bits = below(6) == 0 ? (uint32_t)eos : random_token(sdt, small);
      if (sdt == DT_U16) bits &= 0xFFFFu;
      put_token(src.data() + g.src_off + i * ss, bits, ss);
      if (naive_widen(bits, sdt) == (int64_t)eos)
        want.push_back((int64_t)(g.tok0 + i));
    }
  for (uint64_t cap = 0; cap <= want.size() + 1; ++cap) {
    std::vector<int64_t> out(cap, -77);
    uint64_t total = 0;
    for (auto& g : spans)
      total = token_eos_host(src.data(), g, sdt, eos, out.data(), cap, total);
    check(total == want.size(), "eos total", sdt, total, want.size());
    for (uint64_t r = 0; r < cap; ++r)
      check(out[r] == (r < want.size() ? want[r] : -77), "eos entry", sdt, r,
            cap);
    if (cap > 40 && cap + 2 < want.size()) cap = want.size() - 2;
  }
}

// ----------------------------------------------------------------------- pack

static const int64_t kSentinel = (int64_t)0xABABABABABABABABull;

struct Expect {
  std::vector<int64_t> x, y, pos, doc;
};

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

// the sentinel as an element of ds bytes reads
static int64_t sentinel(uint32_t ds) {
  return ds == 8 ? kSentinel : (int64_t)(int32_t)0xABABABABu;
}

static void sweep_pack(uint32_t sdt, uint32_t ddt) {
  uint32_t ss = cast_itemsize(sdt), ds = cast_itemsize(ddt);
  uint64_t rows = 1 + below(3), T = 1 + below(below(3) == 0 ? 70 : 12);
  unsigned outs = (unsigned)below(16);          // y, pos, doc, cu
  uint64_t vocab = below(2) ? 1 + below(70000) : 0;
  int64_t pad = (int64_t)below(2000) - 1000, ignore = (int64_t)below(400) - 200;
  Expect e;
  e.x.assign(rows * T, sentinel(ds));
  e.y = e.pos = e.doc = e.x;
  std::vector<TokenSeg> segs;
  std::vector<TokenPackPiece> items;
  std::vector<uint8_t> src;
  uint64_t bad = 0;
  for (uint64_t r = 0; r < rows; ++r)
    for (uint64_t col = 0; col < T;) {
      uint64_t n = 1 + below(T - col);
      unsigned kind = (unsigned)below(5);       // 0: gap, 1: pad, else source
      if (kind == 0) { col += n; continue; }
      TokenSeg s{r, col, n, below(1000), (int64_t)below(9), 0, 0};
      uint64_t at = r * T + col;
      if (kind == 1) {
        s.flags = TOKEN_SEG_PAD;
        for (uint64_t i = 0; i < n; ++i) {
          e.x[at + i] = pad;
          e.y[at + i] = ignore;
          e.pos[at + i] = (int64_t)i;
          e.doc[at + i] = -1;
        }
        segs.push_back(s);
        col += n;
        continue;
      }
      bool next = below(2);
      s.flags = next ? TOKEN_SEG_NEXT : 0;
      uint64_t tok = n + (next ? 1 : 0);
      for (uint64_t a = 0; a < tok;) {          // random pieces
        uint64_t k = 1 + below(tok - a);
        if (below(6) != 0) {                    // the piece is passed
          for (uint64_t pad_b = below(4); pad_b; --pad_b) src.push_back(0xCD);
          uint64_t off = src.size();
          src.resize(off + k * ss);
          for (uint64_t i = 0; i < k; ++i) {
            uint64_t j = a + i;
            uint32_t bits = random_token(sdt, false);
            put_token(src.data() + off + i * ss, bits, ss);
            int64_t v = naive_widen(bits, sdt);
            if (vocab && (v < 0 || (uint64_t)v >= vocab)) bad++;
            if (j < n) {
              e.x[at + j] = v;
              e.pos[at + j] = (int64_t)(s.pos0 + j);
              e.doc[at + j] = s.doc;
            }
            if (j >= 1) e.y[at + j - 1] = v;
          }
          if (!next && a <= n - 1 && n - 1 < a + k) e.y[at + n - 1] = ignore;
          items.push_back({off, segs.size(), a, k});
        }
        a += k;
      }
      segs.push_back(s);
      col += n;
    }
  // seq: a random permutation of the segments' entries
  std::vector<uint32_t> seq(segs.size());
  for (size_t i = 0; i < seq.size(); ++i) seq[i] = (uint32_t)i;
  for (size_t i = seq.size(); i > 1; --i) std::swap(seq[i - 1], seq[below(i)]);
  for (size_t i = 0; i < segs.size(); ++i) segs[i].seq = seq[i];
  for (size_t i = 0; i < segs.size(); ++i)
    if (segs[i].flags & TOKEN_SEG_PAD) items.push_back({0, i, 0, segs[i].n});
  // exact-size blocks; the source too, so a read past a piece is seen
  std::vector<uint8_t> x(rows * T * ds, 0xAB), y(outs & 1 ? rows * T * ds : 0, 0xAB),
      pos(outs & 2 ? rows * T * ds : 0, 0xAB),
      doc(outs & 4 ? rows * T * ds : 0, 0xAB);
  std::vector<int32_t> cu(outs & 8 ? segs.size() + 1 : 0, -77);
  std::vector<uint8_t> exact(src.begin(), src.end());
  exact.shrink_to_fit();
  TokenPackOut out{x.data(), outs & 1 ? y.data() : nullptr,
                   outs & 2 ? pos.data() : nullptr,
                   outs & 4 ? doc.data() : nullptr};
  uint64_t got = token_pack_host(exact.data(), segs, items, out,
                                 outs & 8 ? cu.data() : nullptr, rows, T, sdt,
                                 ddt, pad, ignore, vocab);
  check(got == bad, "pack count", sdt, got, bad);
  auto fit = [&](int64_t v) { return ds == 8 ? v : (int64_t)(int32_t)v; };
  for (uint64_t i = 0; i < rows * T; ++i) {
    check(read_el(x, i, ds) == fit(e.x[i]), "x", sdt * 16 + ddt, i, T);
    if (outs & 1) check(read_el(y, i, ds) == fit(e.y[i]), "y", sdt * 16 + ddt, i, T);
    if (outs & 2) check(read_el(pos, i, ds) == fit(e.pos[i]), "pos", sdt * 16 + ddt, i, T);
    if (outs & 4) check(read_el(doc, i, ds) == fit(e.doc[i]), "doc", sdt * 16 + ddt, i, T);
  }
  if (outs & 8) {
    for (auto& s : segs)
      check(cu[s.seq] == (int32_t)(s.row * T + s.col), "cu", s.seq, s.row, s.col);
    check(cu[segs.size()] == (int32_t)(rows * T), "cu end", rows, T, 0);
  }
}

int main() {
  const uint32_t sources[] = {DT_U16, DT_U32, DT_I32};
  for (int round = 0; round < 1500; ++round)
    for (uint32_t sdt : sources) sweep_eos(sdt);
  const uint32_t pairs[][2] = {{DT_U16, DT_I32}, {DT_U16, DT_I64},
                               {DT_U32, DT_I64}, {DT_I32, DT_I32},
                               {DT_I32, DT_I64}};
  for (int round = 0; round < 3000; ++round)
    for (auto& p : pairs) sweep_pack(p[0], p[1]);
  std::printf("token_pack_host_sweep: %llu checks, %d failures\n",
              (unsigned long long)checks, failures);
  return failures ? 1 : 0;
}

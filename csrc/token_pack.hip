// Document-packed token batches for curvine_amd: rows made of whole
// documents (or T-token chunks of long ones) instead of windows cut wherever
// a stride lands.  Two pieces of device code:
//
// 1. The eos index of a token file: the ascending list of file token indices
//    whose value equals the end-of-document id, found where the bytes live.
//    A span is `n` source tokens (U16 / U32 / I32) at arena byte `src_off`,
//    which are tokens tok0 .. tok0+n-1 of the file; spans come in ascending
//    tok0 and are tiled into TOKEN_EOS_TILE tokens.  A token matches when its
//    widened value equals eos, which is non-negative and fits the dtype, so a
//    negative I32 never matches.  Three launches on one stream, as in
//    token_docs.hip; no workgroup ever waits on another inside a launch:
//      token_eos_count_kernel    per tile: its number of hits
//      token_eos_offsets_kernel  one workgroup turns the counts into
//                                exclusive prefixes with a running carry, in
//                                place, and leaves the total
//      token_eos_write_kernel    per tile: re-reads it, scans lane -> wave ->
//                                LDS and stores each hit at its rank; ranks
//                                >= capacity are not written
//
// 2. The pack kernel: a batch is [rows, T].  A segment covers columns
//    col .. col+n-1 of one row: n tokens d[0 .. n-1] of one document (plus
//    d[n] when TOKEN_SEG_NEXT says the document goes on), or padding
//    (TOKEN_SEG_PAD).  For a source segment and i in 0 .. n-1:
//      x[row, col+i]            = d[i], widened as token_windows widens it
//      y[row, col+i]            = d[i+1] when i+1 < n or NEXT, else ignore
//      position_ids[row, col+i] = pos0 + i
//      doc_ids[row, col+i]      = doc
//    and for a pad segment x = pad, y = ignore, position_ids = i, doc_ids =
//    -1.  cu_seqlens[seq] = row*T + col for every segment, and
//    cu_seqlens[n_segments] = rows*T.
//    A piece is `k` source tokens at arena byte `src_off`: tokens
//    j0 .. j0+k-1 of its segment's n (+1) tokens.  Token j goes to x when
//    j < n and to y one column to the left when j >= 1, the TokenPiece rule
//    of token_gather.hip, so a block boundary may cut a segment anywhere.
//    Every source token is read once; one launch does all five outputs.
//
// Sources may sit at any byte alignment, destinations are aligned to their
// itemsize only.  16-byte accesses are used where an address is on the
// 16-byte grid (for y, which runs one element out of phase with x, a
// 16-byte store declared with the itemsize's alignment), element accesses
// at the edges.  Both kernels are memory-bound.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

// ---------------------------------------------------------------------------
// eos index
// ---------------------------------------------------------------------------

// tokens per workgroup tile: WG threads of TOKEN_EOS_PER consecutive tokens
#define TOKEN_EOS_PER 8
#define TOKEN_EOS_TILE (WG * TOKEN_EOS_PER)

struct TokenSpan {
  uint64_t src_off;     // bytes into the arena, any alignment
  uint64_t tok0;        // file index of the span's first token
  uint64_t n;           // tokens
};

// the ONE comparison (host + device)
__host__ __device__ inline bool token_eos_match(uint32_t bits, uint32_t sdt,
                                                uint64_t eos) {
  return token_widen(bits, sdt) == eos;
}

// hit bits of up to TOKEN_EOS_PER tokens at p; `left` tokens lie between p
// and the end of the span.  Nothing past the span's last byte is read: the
// shifted loads over-read up to 3 bytes, which then belong to the two
// tokens behind the thread's own.
template <uint32_t SDT>
__device__ __forceinline__ uint32_t token_eos_flags(const uint8_t* p,
                                                    uint64_t left,
                                                    uint64_t eos) {
  constexpr int SS = SDT == DT_U16 ? 2 : 4;
  constexpr int Q = TOKEN_EOS_PER * SS / 16;     // 16-byte groups per thread
  constexpr int KQ = 16 / SS;                    // tokens per group
  uint32_t nv = left < TOKEN_EOS_PER ? (uint32_t)left : TOKEN_EOS_PER;
  uint32_t m = 0;
  int mode = ((uintptr_t)p & 15) == 0 ? 0 : (((uintptr_t)p & 3) == 0 ? 1 : 2);
  if (nv == TOKEN_EOS_PER && (mode != 2 || left >= TOKEN_EOS_PER + 2)) {
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      uint32_t w[4];
      cast_load_words<4>(p + 16 * q, mode, w);
#pragma unroll
      for (int k = 0; k < KQ; ++k) {
        uint32_t bits;
        if constexpr (SS == 4) bits = w[k];
        else bits = (w[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu;
        m |= (token_eos_match(bits, SDT, eos) ? 1u : 0u) << (q * KQ + k);
      }
    }
    return m;
  }
#pragma unroll
  for (int j = 0; j < TOKEN_EOS_PER; ++j)
    if ((uint32_t)j < nv)
      m |= (token_eos_match(token_load(p + j * SS, SS), SDT, eos) ? 1u : 0u)
           << j;
  return m;
}

// the calling thread's tokens of tile `tile`: hit bits, and the file index
// of its first token in `first`
__device__ __forceinline__ uint32_t token_eos_tile_flags(
    const uint8_t* base, const TokenSpan* spans, const uint32_t* tile_span,
    const uint64_t* tile_off, uint32_t tile, uint32_t sdt, uint64_t eos,
    uint64_t& first) {
  TokenSpan g = spans[tile_span[tile]];
  uint64_t i = tile_off[tile] + (uint64_t)threadIdx.x * TOKEN_EOS_PER;
  first = g.tok0 + i;
  if (i >= g.n) return 0;               // no address is formed past the span
  uint32_t ss = sdt == DT_U16 ? 2u : 4u;
  const uint8_t* p = base + g.src_off + i * ss;
  switch (sdt) {
    case DT_U16: return token_eos_flags<DT_U16>(p, g.n - i, eos);
    case DT_U32: return token_eos_flags<DT_U32>(p, g.n - i, eos);
    default: return token_eos_flags<DT_I32>(p, g.n - i, eos);
  }
}

// grid-stride over tiles.  counts[tile]: hits among the tile's tokens.
extern "C" __global__ __launch_bounds__(WG) void token_eos_count_kernel(
    const uint8_t* __restrict__ base, const TokenSpan* __restrict__ spans,
    const uint32_t* __restrict__ tile_span,
    const uint64_t* __restrict__ tile_off, uint32_t n_tiles, uint32_t sdt,
    uint64_t eos, uint64_t* __restrict__ counts) {
  __shared__ uint32_t lds[WG / 64];
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    uint64_t first;
    uint32_t cnt = __popc(token_eos_tile_flags(base, spans, tile_span,
                                               tile_off, tile, sdt, eos,
                                               first));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint64_t c = 0;
#pragma unroll
      for (int w = 0; w < WG / 64; ++w) c += lds[w];
      counts[tile] = c;
    }
    __syncthreads();                     // lds is reused by the next tile
  }
}

// one workgroup: counts of n tiles become their exclusive prefix sum, in
// place (a thread reads and writes its own entries only); result[0] = total
extern "C" __global__ __launch_bounds__(WG) void token_eos_offsets_kernel(
    uint64_t* __restrict__ counts, uint64_t n,
    unsigned long long* __restrict__ result) {
  __shared__ uint64_t lds[2 * (WG / 64)];
  uint64_t carry = 0;
  for (uint64_t at = 0; at < n; at += WG) {       // uniform trip count
    uint64_t i = at + threadIdx.x;
    uint64_t sum = i < n ? counts[i] : 0, mx = 0;
    uint64_t ex_sum, ex_mx, tot_sum, tot_mx;
    token_doc_scan(sum, mx, ex_sum, ex_mx, tot_sum, tot_mx, lds);
    if (i < n) counts[i] = carry + ex_sum;
    carry += tot_sum;
  }
  if (threadIdx.x == 0) result[0] = carry;
}

// grid-stride over tiles, after token_eos_offsets_kernel: hit number r of
// the call (in file order) is stored at out[r] when r < capacity
extern "C" __global__ __launch_bounds__(WG) void token_eos_write_kernel(
    const uint8_t* __restrict__ base, const TokenSpan* __restrict__ spans,
    const uint32_t* __restrict__ tile_span,
    const uint64_t* __restrict__ tile_off, uint32_t n_tiles, uint32_t sdt,
    uint64_t eos, const uint64_t* __restrict__ counts,
    int64_t* __restrict__ out, uint64_t capacity) {
  __shared__ uint64_t lds[2 * (WG / 64)];
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    uint64_t first;
    uint32_t m = token_eos_tile_flags(base, spans, tile_span, tile_off, tile,
                                      sdt, eos, first);
    uint64_t sum = __popc(m), mx = 0, ex_sum, ex_mx, tot_sum, tot_mx;
    token_doc_scan(sum, mx, ex_sum, ex_mx, tot_sum, tot_mx, lds);
    uint64_t rank = counts[tile] + ex_sum;
#pragma unroll
    for (int j = 0; j < TOKEN_EOS_PER; ++j)
      if ((m >> j) & 1u) {
        if (rank < capacity) out[rank] = (int64_t)(first + j);
        rank++;
      }
  }
}

// host memory: the same comparison, a plain loop; returns the total
static uint64_t token_eos_host(const uint8_t* base, const TokenSpan& g,
                               uint32_t sdt, uint64_t eos, int64_t* out,
                               uint64_t capacity, uint64_t rank) {
  uint32_t ss = cast_itemsize(sdt);
  for (uint64_t i = 0; i < g.n; ++i)
    if (token_eos_match(token_load(base + g.src_off + i * ss, ss), sdt, eos)) {
      if (rank < capacity) out[rank] = (int64_t)(g.tok0 + i);
      rank++;
    }
  return rank;
}

// ---------------------------------------------------------------------------
// pack
// ---------------------------------------------------------------------------

// tokens (pad segments: columns) per workgroup tile
#define TOKEN_PACK_TILE 1024

// segment flags
#define TOKEN_SEG_NEXT 1u   // the document goes on: token n exists (y only)
#define TOKEN_SEG_PAD 2u    // padding: no source

struct TokenSeg {
  uint64_t row, col;    // first column of the segment
  uint64_t n;           // columns
  uint64_t pos0;        // position id of its first token
  int64_t doc;          // document id of its tokens
  uint32_t seq;         // its entry of cu_seqlens
  uint32_t flags;
};

// a source piece, or (seg a pad segment) the whole of a pad segment
struct TokenPackPiece {
  uint64_t src_off;     // bytes into the arena, any alignment
  uint64_t seg;         // index into the segment table
  uint64_t j0;          // index of the piece's first token in its segment
  uint64_t k;           // tokens, j0 + k <= n + NEXT
};

// the outputs, or inside a segment the addresses of its column 0; y, pos
// and doc may be null
struct TokenPackOut {
  uint8_t* x;
  uint8_t* y;
  uint8_t* pos;
  uint8_t* doc;
};

// ---- scalar routines (the ONE definition; host + device) ----

__host__ __device__ inline TokenPackOut token_pack_at(const TokenPackOut& o,
                                                      const TokenSeg& s,
                                                      uint64_t T, uint32_t ds) {
  uint64_t at = (s.row * T + s.col) * ds;
  TokenPackOut r;
  r.x = o.x + at;
  r.y = o.y ? o.y + at : nullptr;
  r.pos = o.pos ? o.pos + at : nullptr;
  r.doc = o.doc ? o.doc + at : nullptr;
  return r;
}

// token j of source segment s, byte loads, element stores; o = the
// segment's column 0; returns its count
__host__ __device__ inline uint32_t token_pack_one(
    const uint8_t* src, const TokenPackOut& o, const TokenSeg& s, uint64_t j,
    uint32_t sdt, uint32_t ss, uint32_t ds, uint64_t vocab) {
  uint32_t bits = token_load(src, ss);
  uint64_t v = token_widen(bits, sdt);
  if (j < s.n) {
    token_store(o.x + j * ds, v, ds);
    if (o.pos) token_store(o.pos + j * ds, s.pos0 + j, ds);
    if (o.doc) token_store(o.doc + j * ds, (uint64_t)s.doc, ds);
  }
  if (j >= 1 && o.y) token_store(o.y + (j - 1) * ds, v, ds);
  return vocab && token_out_of_range(bits, sdt, vocab) ? 1u : 0u;
}

// the target of segment s' last token when the document ends there
__host__ __device__ inline void token_pack_end(const TokenPackOut& o,
                                               const TokenSeg& s,
                                               int64_t ignore, uint32_t ds) {
  if (o.y) token_store(o.y + (s.n - 1) * ds, (uint64_t)ignore, ds);
}

// column i of a pad segment
__host__ __device__ inline void token_pack_pad_one(const TokenPackOut& o,
                                                   uint64_t i, int64_t pad,
                                                   int64_t ignore, uint32_t ds) {
  token_store(o.x + i * ds, (uint64_t)pad, ds);
  if (o.y) token_store(o.y + i * ds, (uint64_t)ignore, ds);
  if (o.pos) token_store(o.pos + i * ds, i, ds);
  if (o.doc) token_store(o.doc + i * ds, (uint64_t)(int64_t)-1, ds);
}

// ---- kernel ----

// elements e in [0, n) at p become a + b*e, all WG threads cooperating:
// 16-byte stores from the first address on the grid, element stores around
template <int DS>
__device__ __forceinline__ void token_pack_ramp(uint8_t* p, uint64_t n,
                                                uint64_t a, uint64_t b) {
  constexpr int K = 16 / DS;
  uint64_t hd = ((0 - (uintptr_t)p) & (uintptr_t)15) / DS;
  if (hd > n) hd = n;
  uint64_t nb = (n - hd) / K;
  for (uint64_t u = threadIdx.x; u < nb; u += WG) {
    uint64_t e = hd + u * K;
    uint4 o;
    if constexpr (DS == 8) {
      uint64_t v0 = a + b * e, v1 = a + b * (e + 1);
      o = make_uint4((uint32_t)v0, (uint32_t)(v0 >> 32), (uint32_t)v1,
                     (uint32_t)(v1 >> 32));
    } else {
      o = make_uint4((uint32_t)(a + b * e), (uint32_t)(a + b * (e + 1)),
                     (uint32_t)(a + b * (e + 2)), (uint32_t)(a + b * (e + 3)));
    }
    *reinterpret_cast<uint4*>(p + e * DS) = o;
  }
  uint64_t tail0 = hd + nb * K;
  uint64_t edge = hd + (n - tail0);              // fewer than 2*K elements
  for (uint64_t i = threadIdx.x; i < edge; i += WG) {
    uint64_t e = i < hd ? i : tail0 + (i - hd);
    token_store(p + e * DS, a + b * e, DS);
  }
}

// columns [t0, t1) of pad segment s
template <int DS>
__device__ __forceinline__ void token_pack_pad_tile(
    const TokenPackOut& o, uint64_t t0, uint64_t t1, int64_t pad,
    int64_t ignore) {
  uint64_t n = t1 - t0;
  token_pack_ramp<DS>(o.x + t0 * DS, n, (uint64_t)pad, 0);
  if (o.y) token_pack_ramp<DS>(o.y + t0 * DS, n, (uint64_t)ignore, 0);
  if (o.pos) token_pack_ramp<DS>(o.pos + t0 * DS, n, t0, 1);
  if (o.doc) token_pack_ramp<DS>(o.doc + t0 * DS, n, (uint64_t)(int64_t)-1, 0);
}

// tokens [t0, t1) of piece g of source segment s, all WG threads
// cooperating; o = the segment's column 0.  The access pattern is
// token_tile's (token_gather.hip) with the segment in the place of the
// window.  Returns the lane's count of out-of-range tokens.
template <uint32_t SDT, uint32_t DDT>
__device__ __forceinline__ uint32_t token_pack_tile(
    const uint8_t* base, const TokenPackOut& o, const TokenSeg& s,
    const TokenPackPiece& g, uint64_t t0, uint64_t t1, int64_t ignore,
    uint64_t vocab) {
  constexpr int SS = SDT == DT_U16 ? 2 : 4;
  constexpr int DS = DDT == DT_I64 ? 8 : 4;
  constexpr int K = 16 / DS;                    // tokens per unit
  constexpr int W = K * SS / 4;                 // source dwords per unit
  const uint8_t* src = base + g.src_off;        // token i of the piece: + i*SS
  uint32_t bad = 0;

  // the body holds tokens that go to both x and y: token 0 of a segment and
  // token n stay out
  uint64_t b0 = (g.j0 + t0 == 0) ? t0 + 1 : t0;
  uint64_t b1 = (g.j0 + t1 - 1 == s.n) ? t1 - 1 : t1;
  if (b1 < b0) b1 = b0;                         // a tile of one token
  // head: up to the first x address on the 16-byte grid
  uint64_t hd = ((0 - (uintptr_t)(o.x + (g.j0 + b0) * DS)) & (uintptr_t)15) / DS;
  if (hd > b1 - b0) hd = b1 - b0;
  uint64_t u0 = b0 + hd;                        // first body token
  uint64_t nb = (b1 - u0) / K;
  const uint8_t* sb = src + u0 * SS;
  int mode = ((uintptr_t)sb & (W * 4 - 1)) == 0 ? 0
             : (((uintptr_t)sb & 3) == 0 ? 1 : 2);
  // the shifted loads over-read up to 3 bytes past their unit: keep the
  // last unit out of the body, so those bytes belong to the tokens after it
  // and nothing past the tile's last byte is read
  if (mode == 2 && nb > 0) nb--;
  uint64_t tail0 = u0 + nb * K;

  for (uint64_t u = threadIdx.x; u < nb; u += WG) {
    uint32_t w[W], q[4];
    cast_load_words<W>(sb + u * (K * SS), mode, w);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      uint32_t bits;
      if constexpr (SS == 4) bits = w[k];
      else bits = (w[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu;
      if (vocab && token_out_of_range(bits, SDT, vocab)) bad++;
      uint64_t v = token_widen(bits, SDT);
      if constexpr (DS == 8) {
        q[2 * k] = (uint32_t)v;
        q[2 * k + 1] = (uint32_t)(v >> 32);
      } else {
        q[k] = (uint32_t)v;
      }
    }
    uint64_t j = g.j0 + u0 + u * K;             // 1 <= j, j + K - 1 < n
    *reinterpret_cast<uint4*>(o.x + j * DS) = make_uint4(q[0], q[1], q[2], q[3]);
    if (o.y) {
      if constexpr (DS == 8) {
        TokenQuadA8 t = {{q[0], q[1], q[2], q[3]}};
        *reinterpret_cast<TokenQuadA8*>(o.y + (j - 1) * DS) = t;
      } else {
        TokenQuadA4 t = {{q[0], q[1], q[2], q[3]}};
        *reinterpret_cast<TokenQuadA4*>(o.y + (j - 1) * DS) = t;
      }
    }
  }
  // position and document ids of the body, on 16-byte grids of their own
  uint64_t jb = g.j0 + u0;
  if (o.pos) token_pack_ramp<DS>(o.pos + jb * DS, tail0 - u0, s.pos0 + jb, 1);
  if (o.doc) token_pack_ramp<DS>(o.doc + jb * DS, tail0 - u0, (uint64_t)s.doc, 0);
  // edges: token 0, head, tail, token n: at most 3*K + 1 tokens
  uint64_t n_lo = u0 - t0;
  uint64_t edge = n_lo + (t1 - tail0);
  for (uint64_t e = threadIdx.x; e < edge; e += WG) {
    uint64_t i = e < n_lo ? t0 + e : tail0 + (e - n_lo);
    bad += token_pack_one(src + i * SS, o, s, g.j0 + i, SDT, SS, DS, vocab);
  }
  // the document ends with the segment and this tile holds its last token
  if (!(s.flags & TOKEN_SEG_NEXT) && threadIdx.x == 0 &&
      g.j0 + t0 <= s.n - 1 && s.n - 1 < g.j0 + t1)
    token_pack_end(o, s, ignore, DS);
  return bad;
}

template <uint32_t SDT, uint32_t DDT>
__device__ __forceinline__ uint32_t token_pack_tiles(
    const uint8_t* base, const TokenSeg* segs, const TokenPackPiece* items,
    const uint32_t* tile_item, const uint64_t* tile_off, uint32_t n_tiles,
    const TokenPackOut& out, uint64_t T, int64_t pad, int64_t ignore,
    uint64_t vocab) {
  constexpr int DS = DDT == DT_I64 ? 8 : 4;
  uint32_t bad = 0;
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    TokenPackPiece g = items[tile_item[tile]];
    TokenSeg s = segs[g.seg];
    TokenPackOut o = token_pack_at(out, s, T, DS);
    uint64_t t0 = tile_off[tile];
    uint64_t t1 = min(t0 + (uint64_t)TOKEN_PACK_TILE, g.k);
    if (s.flags & TOKEN_SEG_PAD)
      token_pack_pad_tile<DS>(o, t0, t1, pad, ignore);
    else
      bad += token_pack_tile<SDT, DDT>(base, o, s, g, t0, t1, ignore, vocab);
  }
  return bad;
}

// Tile table over `items`: the source pieces, then one item per pad segment
// (k = its columns); grid-stride over tiles.  cu (may be null) takes one
// entry per segment and rows*T at n_segs, whatever the pieces cover.
// `counter` receives the out-of-range tokens of the call and is touched only
// when vocab > 0.
extern "C" __global__ __launch_bounds__(WG) void token_pack_kernel(
    const uint8_t* __restrict__ base, const TokenSeg* __restrict__ segs,
    uint32_t n_segs, const TokenPackPiece* __restrict__ items,
    const uint32_t* __restrict__ tile_item,
    const uint64_t* __restrict__ tile_off, uint32_t n_tiles, TokenPackOut out,
    int32_t* __restrict__ cu, uint64_t rows, uint64_t T, uint32_t src_dt,
    uint32_t dst_dt, int64_t pad, int64_t ignore, uint64_t vocab,
    unsigned long long* __restrict__ counter) {
  __shared__ uint32_t lds[WG / 64];
  uint32_t bad = 0;
#define TOKEN_PACK_CASE(S, D)                                                 \
  case (S) * 16u + (D):                                                       \
    bad = token_pack_tiles<S, D>(base, segs, items, tile_item, tile_off,      \
                                 n_tiles, out, T, pad, ignore, vocab);        \
    break;
  switch (src_dt * 16u + dst_dt) {
    TOKEN_PACK_CASE(DT_U16, DT_I32) TOKEN_PACK_CASE(DT_U16, DT_I64)
    TOKEN_PACK_CASE(DT_U32, DT_I64)
    TOKEN_PACK_CASE(DT_I32, DT_I32) TOKEN_PACK_CASE(DT_I32, DT_I64)
    default: break;   // host rejects every other pair before launch
  }
#undef TOKEN_PACK_CASE
  if (cu)
    for (uint64_t i = (uint64_t)blockIdx.x * WG + threadIdx.x; i <= n_segs;
         i += (uint64_t)gridDim.x * WG) {
      if (i < n_segs)
        cu[segs[i].seq] = (int32_t)(segs[i].row * T + segs[i].col);
      else
        cu[n_segs] = (int32_t)(rows * T);
    }
  if (!vocab) return;                           // kernel-uniform
  // lanes -> wave (cross-lane) -> workgroup (LDS) -> one atomicAdd
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
  if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = bad;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t total = 0;
#pragma unroll
    for (int w = 0; w < WG / 64; ++w) total += lds[w];
    if (total) atomicAdd(counter, (unsigned long long)total);
  }
}

// host arena + host destinations: the same tables, the same scalar
// routines, plain loops; returns the count
static uint64_t token_pack_host(const uint8_t* base,
                                const std::vector<TokenSeg>& segs,
                                const std::vector<TokenPackPiece>& items,
                                const TokenPackOut& out, int32_t* cu,
                                uint64_t rows, uint64_t T, uint32_t sdt,
                                uint32_t ddt, int64_t pad, int64_t ignore,
                                uint64_t vocab) {
  uint32_t ss = cast_itemsize(sdt), ds = cast_itemsize(ddt);
  uint64_t bad = 0;
  for (auto& g : items) {
    const TokenSeg& s = segs[g.seg];
    TokenPackOut o = token_pack_at(out, s, T, ds);
    if (s.flags & TOKEN_SEG_PAD) {
      for (uint64_t i = 0; i < g.k; ++i)
        token_pack_pad_one(o, i, pad, ignore, ds);
      continue;
    }
    for (uint64_t i = 0; i < g.k; ++i)
      bad += token_pack_one(base + g.src_off + i * ss, o, s, g.j0 + i, sdt,
                            ss, ds, vocab);
    if (!(s.flags & TOKEN_SEG_NEXT) && g.j0 + g.k == s.n)
      token_pack_end(o, s, ignore, ds);
  }
  if (cu) {
    for (auto& s : segs) cu[s.seq] = (int32_t)(s.row * T + s.col);
    cu[segs.size()] = (int32_t)(rows * T);
  }
  return bad;
}

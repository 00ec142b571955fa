// Token-window gather for curvine_amd: flat files of token ids (uint16,
// uint32 or int32) living in the arena -> the two tensors an LLM training
// step consumes.  A window is T+1 consecutive tokens w; the step wants
// x = w[:-1] and y = w[1:], widened.  token_windows_kernel reads every
// source token once and writes it to both, so no full-size temporary and no
// separate widen / slice kernels exist.
//
// One piece = `n` consecutive source tokens at arena byte `src_off`, which
// are tokens j0 .. j0+n-1 of window `row`.  Token j carrying v lands at
// x[row*T + j] when j < T and at y[row*T + j - 1] when j >= 1.  A window
// that crosses cache blocks arrives as several pieces; a piece may be the
// single token 0 (x only) or the single token T (y only).
//
// The source may sit at ANY byte alignment (a header of any length, a block
// boundary at an odd offset).  x and y are aligned to the destination
// itemsize only: rows start at row*T elements and y runs one element out
// of phase with x, so the two can never both be on the 16-byte grid.
//
// Access pattern (memory-bound, LDS only for the count): a unit is the
// token group whose widened form is 16 B, one unit per lane per pass, so the
// load and both stores of a wave are contiguous.  The body starts where x
// reaches the 16-byte grid: x takes aligned 16-byte stores, y takes 16-byte
// stores declared with the itemsize's alignment only.  Source tiers are
// cast_load_words' (tensor_cast.hip, included first): vector load, aligned
// dwords, aligned dwords + byte shift, byte loads for the edges.
//
// Vocabulary check: with vocab > 0 every token read that lies outside
// [0, vocab) is counted, lane -> wave -> workgroup -> at most one atomicAdd
// per workgroup.  Offending tokens are still written.

#include <hip/hip_runtime.h>
#include <stdint.h>

// source tokens per workgroup tile
#define TOKEN_TILE 1024

struct TokenPiece {
  uint64_t src_off;     // bytes into the arena, any alignment
  uint64_t row;         // window (row of x and y)
  uint64_t j0;          // index of the piece's first token in its window
  uint64_t n;           // tokens, j0 + n <= T + 1
};

// U16 / U32 zero-extend, I32 sign-extends; I32 -> I32 keeps its bits
__host__ __device__ inline bool token_pair_supported(uint32_t s, uint32_t d) {
  if (d == DT_I64) return s == DT_U16 || s == DT_U32 || s == DT_I32;
  if (d == DT_I32) return s == DT_U16 || s == DT_I32;
  return false;
}

// ---------------------------------------------------------------------------
// Scalar routines on raw bit patterns (the ONE definition; host + device)
// ---------------------------------------------------------------------------

__host__ __device__ inline uint64_t token_widen(uint32_t bits, uint32_t sdt) {
  if (sdt == DT_I32) return (uint64_t)(int64_t)(int32_t)bits;
  return bits;
}

// vocab > 0
__host__ __device__ inline bool token_out_of_range(uint32_t bits, uint32_t sdt,
                                                   uint64_t vocab) {
  if (sdt == DT_I32 && (int32_t)bits < 0) return true;
  return (uint64_t)bits >= vocab;
}

__host__ __device__ inline uint32_t token_load(const uint8_t* s, uint32_t ss) {
  uint32_t bits = 0;
  for (uint32_t i = 0; i < ss; ++i) bits |= (uint32_t)s[i] << (8u * i);
  return bits;
}

__host__ __device__ inline void token_store(uint8_t* d, uint64_t v,
                                            uint32_t ds) {
  if (ds == 8) *reinterpret_cast<uint64_t*>(d) = v;
  else *reinterpret_cast<uint32_t*>(d) = (uint32_t)v;
}

// token j of window `row`, byte loads, element stores; returns its count
__host__ __device__ inline uint32_t token_one(
    const uint8_t* s, uint8_t* x, uint8_t* y, uint64_t row, uint64_t j,
    uint64_t T, uint32_t sdt, uint32_t ss, uint32_t ds, uint64_t vocab) {
  uint32_t bits = token_load(s, ss);
  uint64_t v = token_widen(bits, sdt);
  if (j < T) token_store(x + (row * T + j) * ds, v, ds);
  if (j >= 1) token_store(y + (row * T + j - 1) * ds, v, ds);
  return vocab && token_out_of_range(bits, sdt, vocab) ? 1u : 0u;
}

// ---------------------------------------------------------------------------
// Kernel
// ---------------------------------------------------------------------------

// 16 bytes that promise the destination itemsize's alignment and no more
struct __attribute__((packed, aligned(4))) TokenQuadA4 { uint32_t w[4]; };
struct __attribute__((packed, aligned(8))) TokenQuadA8 { uint32_t w[4]; };

// tokens [t0, t1) of piece g, all WG threads cooperating; returns the
// lane's count of out-of-range tokens
template <uint32_t SDT, uint32_t DDT>
__device__ __forceinline__ uint32_t token_tile(
    const uint8_t* base, uint8_t* x, uint8_t* y, const TokenPiece& g,
    uint64_t t0, uint64_t t1, uint64_t T, uint64_t vocab) {
  constexpr int SS = SDT == DT_U16 ? 2 : 4;
  constexpr int DS = DDT == DT_I64 ? 8 : 4;
  constexpr int K = 16 / DS;                    // tokens per unit
  constexpr int W = K * SS / 4;                 // source dwords per unit
  const uint8_t* s = base + g.src_off;          // token i of the piece: s + i*SS
  uint8_t* xr = x + g.row * T * DS;             // element j of the row: + j*DS
  uint8_t* yr = y + g.row * T * DS;
  uint32_t bad = 0;

  // the body holds tokens that go to both x and y: token 0 of a window and
  // token T stay out
  uint64_t b0 = (g.j0 + t0 == 0) ? t0 + 1 : t0;
  uint64_t b1 = (g.j0 + t1 - 1 == T) ? t1 - 1 : t1;
  if (b1 < b0) b1 = b0;                         // a tile of one token
  // head: up to the first x address on the 16-byte grid
  uint64_t hd = ((0 - (uintptr_t)(xr + (g.j0 + b0) * DS)) & (uintptr_t)15) / DS;
  if (hd > b1 - b0) hd = b1 - b0;
  uint64_t u0 = b0 + hd;                        // first body token
  uint64_t nb = (b1 - u0) / K;
  const uint8_t* sb = s + u0 * SS;
  int mode = ((uintptr_t)sb & (W * 4 - 1)) == 0 ? 0
             : (((uintptr_t)sb & 3) == 0 ? 1 : 2);
  // the shifted loads over-read up to 3 bytes past their unit: keep the
  // last unit out of the body, so those bytes belong to the tokens after it
  // and nothing past the tile's last byte is read
  if (mode == 2 && nb > 0) nb--;
  uint64_t tail0 = u0 + nb * K;

  for (uint64_t u = threadIdx.x; u < nb; u += WG) {
    uint32_t w[W], o[4];
    cast_load_words<W>(sb + u * (K * SS), mode, w);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      uint32_t bits;
      if constexpr (SS == 4) bits = w[k];
      else bits = (w[k >> 1] >> ((k & 1) * 16)) & 0xFFFFu;
      if (vocab && token_out_of_range(bits, SDT, vocab)) bad++;
      uint64_t v = token_widen(bits, SDT);
      if constexpr (DS == 8) {
        o[2 * k] = (uint32_t)v;
        o[2 * k + 1] = (uint32_t)(v >> 32);
      } else {
        o[k] = (uint32_t)v;
      }
    }
    uint64_t j = g.j0 + u0 + u * K;             // 1 <= j, j + K - 1 < T
    *reinterpret_cast<uint4*>(xr + j * DS) = make_uint4(o[0], o[1], o[2], o[3]);
    if constexpr (DS == 8) {
      TokenQuadA8 q = {{o[0], o[1], o[2], o[3]}};
      *reinterpret_cast<TokenQuadA8*>(yr + (j - 1) * DS) = q;
    } else {
      TokenQuadA4 q = {{o[0], o[1], o[2], o[3]}};
      *reinterpret_cast<TokenQuadA4*>(yr + (j - 1) * DS) = q;
    }
  }
  // edges: token 0, head, tail, token T: at most 3*K + 1 tokens
  uint64_t n_lo = u0 - t0;
  uint64_t edge = n_lo + (t1 - tail0);
  for (uint64_t e = threadIdx.x; e < edge; e += WG) {
    uint64_t i = e < n_lo ? t0 + e : tail0 + (e - n_lo);
    bad += token_one(s + i * SS, x, y, g.row, g.j0 + i, T, SDT, SS, DS, vocab);
  }
  return bad;
}

template <uint32_t SDT, uint32_t DDT>
__device__ __forceinline__ uint32_t token_tiles(
    const uint8_t* base, const TokenPiece* pieces, const uint32_t* tile_piece,
    const uint64_t* tile_off, uint32_t n_tiles, uint8_t* x, uint8_t* y,
    uint64_t T, uint64_t vocab) {
  uint32_t bad = 0;
  for (uint32_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    TokenPiece g = pieces[tile_piece[tile]];
    uint64_t t0 = tile_off[tile];
    uint64_t t1 = min(t0 + (uint64_t)TOKEN_TILE, g.n);
    bad += token_tile<SDT, DDT>(base, x, y, g, t0, t1, T, vocab);
  }
  return bad;
}

// Tile table as in convert_segments_kernel: tile -> piece, tile -> first
// token of the piece; grid-stride over tiles.  `counter` receives the
// out-of-range tokens of the call and is touched only when vocab > 0.
extern "C" __global__ __launch_bounds__(WG) void token_windows_kernel(
    const uint8_t* __restrict__ base, const TokenPiece* __restrict__ pieces,
    const uint32_t* __restrict__ tile_piece,
    const uint64_t* __restrict__ tile_off, uint32_t n_tiles,
    uint8_t* __restrict__ x, uint8_t* __restrict__ y, uint64_t T,
    uint32_t src_dt, uint32_t dst_dt, uint64_t vocab,
    unsigned long long* __restrict__ counter) {
  __shared__ uint32_t lds[WG / 64];
  uint32_t bad = 0;
#define TOKEN_CASE(S, D)                                                      \
  case (S) * 16u + (D):                                                       \
    bad = token_tiles<S, D>(base, pieces, tile_piece, tile_off, n_tiles, x,   \
                            y, T, vocab);                                     \
    break;
  switch (src_dt * 16u + dst_dt) {
    TOKEN_CASE(DT_U16, DT_I32) TOKEN_CASE(DT_U16, DT_I64)
    TOKEN_CASE(DT_U32, DT_I64)
    TOKEN_CASE(DT_I32, DT_I32) TOKEN_CASE(DT_I32, DT_I64)
    default: break;   // host rejects every other pair before launch
  }
#undef TOKEN_CASE
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

// host arena + host destinations: the same pieces, the same scalar
// routines, plain loops; returns the count
static uint64_t token_windows_host(const uint8_t* base, const TokenPiece& g,
                                   uint8_t* x, uint8_t* y, uint64_t T,
                                   uint32_t sdt, uint32_t ddt, uint64_t vocab) {
  uint32_t ss = cast_itemsize(sdt), ds = cast_itemsize(ddt);
  uint64_t bad = 0;
  for (uint64_t i = 0; i < g.n; ++i)
    bad += token_one(base + g.src_off + i * ss, x, y, g.row, g.j0 + i, T, sdt,
                     ss, ds, vocab);
  return bad;
}

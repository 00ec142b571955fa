// Document structure of a token batch for curvine_amd: from the finished
// x tensor of a token window batch ([rows, T] of int32 / int64) and the
// end-of-document id to the three tensors a trainer derives from them:
// position ids that restart after every eos, a document index per token, and
// cu_seqlens / max_seqlen for variable-length attention.
//
// Definitions (row r, column t; a token equal to eos ends its document and
// belongs to it):
//   doc_ids[r, t]      = #{s < t : x[r, s] == eos}
//   position_ids[r, t] = t - start, start = 1 + the largest s < t with
//                        x[r, s] == eos, or 0 when there is none
//   flat index r*T + t starts a sequence iff position_ids[r, t] == 0, that is
//   t == 0 or x[r, t-1] == eos; cu_seqlens is the ascending list of starts
//   followed by rows*T; max_seqlen the largest gap between neighbours.
// A sequence never crosses a row, so a start at (r, t) is entry
//   r + #{eos in columns < T-1 of rows < r} + doc_ids[r, t]
// of cu_seqlens, and a sequence ends at every eos and at column T-1, where
// its length is position_ids + 1.
//
// A row can be far longer than a workgroup holds, so the scan is chunked
// into TOKEN_DOC_CHUNK columns and split over three launches on one stream;
// no workgroup ever waits on another inside a launch:
//   token_doc_summary_kernel  one workgroup per chunk: its eos count (column
//                             T-1 left out) and the key of its last eos
//   token_doc_offsets_kernel  one workgroup walks the chunk table in
//                             row-major order with a running carry and turns
//                             both columns into exclusive prefixes, in place
//   token_doc_write_kernel    one workgroup per chunk re-reads it, scans
//                             lane -> wave -> LDS and writes the outputs
// Keys make the per-row reset a plain maximum: the eos at column s of row r
// has key r*(T+1) + s + 1, keys grow in row-major order, and a carried key
// below r*(T+1) + 1 belongs to an earlier row: no eos yet in this one.
//
// x and the outputs are aligned to their itemsize only (odd T: rows start
// at every 16-byte phase).  A thread owns 8 consecutive columns; 16-byte
// accesses are used where the thread's address is on the 16-byte grid and
// element accesses for the columns in front of and behind it.

#include <hip/hip_runtime.h>
#include <stdint.h>

// columns per workgroup: WG threads of TOKEN_DOC_PER consecutive columns
#define TOKEN_DOC_PER 8
#define TOKEN_DOC_CHUNK (WG * TOKEN_DOC_PER)

// ---------------------------------------------------------------------------
// Scalar routines (the ONE definition; host + device)
// ---------------------------------------------------------------------------

// element of `ds` bytes at full width, zero-extended: eos is non-negative
// and fits the dtype, so a negative id or one with high bits never matches
__host__ __device__ inline uint64_t token_doc_load(const uint8_t* p,
                                                   uint32_t ds) {
  if (ds == 8) return *reinterpret_cast<const uint64_t*>(p);
  return *reinterpret_cast<const uint32_t*>(p);
}

__host__ __device__ inline bool token_is_eos(uint64_t bits, uint64_t eos) {
  return bits == eos;
}

// running state inside one row: where the current document started and how
// many documents ended before the current column
struct TokenDocState {
  uint64_t start;
  uint64_t docs;
};

// key of the eos at column `col` of row `row`
__host__ __device__ inline uint64_t token_doc_key(uint64_t row, uint64_t col,
                                                  uint64_t T) {
  return row * (T + 1) + col + 1;
}

// document start carried into row `row` by key `key` (0: no eos so far)
__host__ __device__ inline uint64_t token_doc_start(uint64_t key, uint64_t row,
                                                    uint64_t T) {
  uint64_t base = row * (T + 1);
  return key > base ? key - base : 0;
}

// column `col` under state `st`: its position id and document index; advances
// the state past the column.  `seq_len` becomes the length of the sequence
// that ends here, or 0 when none does.
__host__ __device__ inline void token_doc_one(TokenDocState& st, uint64_t col,
                                              bool eos, uint64_t T,
                                              uint64_t& pos, uint64_t& doc,
                                              uint64_t& seq_len) {
  pos = col - st.start;
  doc = st.docs;
  seq_len = (eos || col == T - 1) ? pos + 1 : 0;
  if (eos) {
    st.start = col + 1;
    st.docs++;
  }
}

// ---------------------------------------------------------------------------
// Kernels
// ---------------------------------------------------------------------------

// eos bits of up to 8 columns at p (nv of them exist)
template <int DS>
__device__ __forceinline__ uint32_t token_doc_flags(const uint8_t* p,
                                                    uint32_t nv, uint64_t eos) {
  uint32_t m = 0;
  if (nv == TOKEN_DOC_PER && ((uintptr_t)p & 15) == 0) {
#pragma unroll
    for (int q = 0; q < TOKEN_DOC_PER * DS / 16; ++q) {
      uint4 v = *reinterpret_cast<const uint4*>(p + 16 * q);
      if constexpr (DS == 8) {
        uint64_t a = (uint64_t)v.x | ((uint64_t)v.y << 32);
        uint64_t b = (uint64_t)v.z | ((uint64_t)v.w << 32);
        m |= (token_is_eos(a, eos) ? 1u : 0u) << (2 * q);
        m |= (token_is_eos(b, eos) ? 1u : 0u) << (2 * q + 1);
      } else {
        m |= (token_is_eos(v.x, eos) ? 1u : 0u) << (4 * q);
        m |= (token_is_eos(v.y, eos) ? 1u : 0u) << (4 * q + 1);
        m |= (token_is_eos(v.z, eos) ? 1u : 0u) << (4 * q + 2);
        m |= (token_is_eos(v.w, eos) ? 1u : 0u) << (4 * q + 3);
      }
    }
    return m;
  }
#pragma unroll
  for (int j = 0; j < TOKEN_DOC_PER; ++j)
    if ((uint32_t)j < nv)
      m |= (token_is_eos(token_doc_load(p + j * DS, DS), eos) ? 1u : 0u) << j;
  return m;
}

// v[0 : nv] to p, HD elements in front of the 16-byte grid
template <int DS, int HD>
__device__ __forceinline__ void token_doc_store_at(
    uint8_t* p, const uint64_t (&v)[TOKEN_DOC_PER], uint32_t nv) {
  constexpr int K = 16 / DS;
#pragma unroll
  for (int e = 0; e < HD; ++e)
    if ((uint32_t)e < nv) token_store(p + e * DS, v[e], DS);
#pragma unroll
  for (int e = HD; e < TOKEN_DOC_PER; e += K) {
    if (e + K <= TOKEN_DOC_PER && (uint32_t)(e + K) <= nv) {
      uint4 o;
      if constexpr (DS == 8) {
        // e + K <= TOKEN_DOC_PER holds here; the modulo keeps the indices
        // inside the array where the unrolled branch is compiled out
        o = make_uint4((uint32_t)v[e], (uint32_t)(v[e] >> 32),
                       (uint32_t)v[(e + 1) % TOKEN_DOC_PER],
                       (uint32_t)(v[(e + 1) % TOKEN_DOC_PER] >> 32));
      } else {
        o = make_uint4((uint32_t)v[e], (uint32_t)v[e + 1],
                       (uint32_t)v[(e + 2) % TOKEN_DOC_PER],
                       (uint32_t)v[(e + 3) % TOKEN_DOC_PER]);
      }
      *reinterpret_cast<uint4*>(p + e * DS) = o;
    } else {
#pragma unroll
      for (int k = 0; k < K; ++k)
        if (e + k < TOKEN_DOC_PER && (uint32_t)(e + k) < nv)
          token_store(p + (e + k) * DS, v[(e + k) % TOKEN_DOC_PER], DS);
    }
  }
}

// the phase is the same for every thread of a chunk: threads are 32 / 64
// bytes apart
template <int DS>
__device__ __forceinline__ void token_doc_store(
    uint8_t* p, const uint64_t (&v)[TOKEN_DOC_PER], uint32_t nv) {
  uint32_t hd = (uint32_t)((0 - (uintptr_t)p) & (uintptr_t)15) / DS;
  if constexpr (DS == 8) {
    if (hd == 0) token_doc_store_at<8, 0>(p, v, nv);
    else token_doc_store_at<8, 1>(p, v, nv);
  } else {
    switch (hd) {
      case 0: token_doc_store_at<4, 0>(p, v, nv); break;
      case 1: token_doc_store_at<4, 1>(p, v, nv); break;
      case 2: token_doc_store_at<4, 2>(p, v, nv); break;
      default: token_doc_store_at<4, 3>(p, v, nv); break;
    }
  }
}

// Inclusive sum and inclusive max over the workgroup's threads in thread
// order, lane -> wave (__shfl_up) -> LDS.  On return `sum` / `mx` hold the
// inclusive values, ex_sum / ex_mx the exclusive ones (0 for thread 0) and
// tot_sum / tot_mx the workgroup's totals, the same in every thread.  Every
// thread of the workgroup calls it; `lds` holds 2 * WG / 64 words and is
// free again on return.
__device__ __forceinline__ void token_doc_scan(
    uint64_t& sum, uint64_t& mx, uint64_t& ex_sum, uint64_t& ex_mx,
    uint64_t& tot_sum, uint64_t& tot_mx, uint64_t* lds) {
  constexpr int NW = WG / 64;
  uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
  uint64_t own_sum = sum;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    uint64_t a = __shfl_up((unsigned long long)sum, d);
    uint64_t b = __shfl_up((unsigned long long)mx, d);
    if (lane >= (uint32_t)d) {
      sum += a;
      mx = b > mx ? b : mx;
    }
  }
  ex_sum = sum - own_sum;
  ex_mx = __shfl_up((unsigned long long)mx, 1);
  if (lane == 0) ex_mx = 0;
  if (lane == 63) {
    lds[w] = sum;
    lds[NW + w] = mx;
  }
  __syncthreads();
  tot_sum = 0;
  tot_mx = 0;
#pragma unroll
  for (int k = 0; k < NW; ++k) {
    uint64_t s = lds[k], m = lds[NW + k];
    if ((uint32_t)k < w) {
      sum += s;
      ex_sum += s;
      mx = m > mx ? m : mx;
      ex_mx = m > ex_mx ? m : ex_mx;
    }
    tot_sum += s;
    tot_mx = m > tot_mx ? m : tot_mx;
  }
  __syncthreads();
}

// a thread's columns of chunk `chunk`: row, first column, how many exist
struct TokenDocSpan {
  uint64_t row, col;
  uint32_t nv;
};

__device__ __forceinline__ TokenDocSpan token_doc_span(uint64_t chunk,
                                                       uint64_t cpr,
                                                       uint64_t T) {
  TokenDocSpan s;
  s.row = chunk / cpr;
  s.col = (chunk % cpr) * TOKEN_DOC_CHUNK + (uint64_t)threadIdx.x * TOKEN_DOC_PER;
  s.nv = s.col >= T ? 0u
         : (T - s.col < TOKEN_DOC_PER ? (uint32_t)(T - s.col) : TOKEN_DOC_PER);
  return s;
}

template <int DS>
__device__ __forceinline__ uint32_t token_doc_span_flags(
    const uint8_t* x, const TokenDocSpan& s, uint64_t T, uint64_t eos) {
  if (!s.nv) return 0;                 // no address is formed past the row
  return token_doc_flags<DS>(x + (s.row * T + s.col) * DS, s.nv, eos);
}

// grid = rows * cpr chunks.  counts[chunk]: eos in the chunk's columns
// below T-1 (each starts a sequence); keys[chunk]: key of its last eos, 0
// without one.
extern "C" __global__ __launch_bounds__(WG) void token_doc_summary_kernel(
    const uint8_t* __restrict__ x, uint64_t T, uint64_t cpr, uint32_t ds,
    uint64_t eos, uint64_t* __restrict__ counts, uint64_t* __restrict__ keys) {
  __shared__ uint64_t lds[2 * (WG / 64)];
  uint64_t chunk = blockIdx.x;
  TokenDocSpan s = token_doc_span(chunk, cpr, T);
  uint32_t m = ds == 8 ? token_doc_span_flags<8>(x, s, T, eos)
                       : token_doc_span_flags<4>(x, s, T, eos);
  uint64_t key = m ? token_doc_key(s.row, s.col + (31u - __clz(m)), T) : 0;
  // column T-1 is the last column of the thread that holds it
  if (s.nv && s.col + s.nv == T) m &= ~(1u << (s.nv - 1));
  uint64_t cnt = __popc(m);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor((unsigned long long)cnt, o);
    uint64_t k = __shfl_xor((unsigned long long)key, o);
    key = k > key ? k : key;
  }
  if ((threadIdx.x & 63u) == 0) {
    lds[threadIdx.x >> 6] = cnt;
    lds[WG / 64 + (threadIdx.x >> 6)] = key;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t c = 0, k = 0;
#pragma unroll
    for (int w = 0; w < WG / 64; ++w) {
      c += lds[w];
      k = lds[WG / 64 + w] > k ? lds[WG / 64 + w] : k;
    }
    counts[chunk] = c;
    keys[chunk] = k;
  }
}

// one workgroup: counts / keys of n chunks in row-major order become their
// exclusive prefix sum / prefix maximum, in place (a thread reads and writes
// its own entries only).  result[0] = rows + the total count = n_seqs.
extern "C" __global__ __launch_bounds__(WG) void token_doc_offsets_kernel(
    uint64_t* __restrict__ counts, uint64_t* __restrict__ keys, uint64_t n,
    uint64_t rows, unsigned long long* __restrict__ result) {
  __shared__ uint64_t lds[2 * (WG / 64)];
  uint64_t carry_sum = 0, carry_mx = 0;
  for (uint64_t base = 0; base < n; base += WG) {   // uniform trip count
    uint64_t i = base + threadIdx.x;
    uint64_t sum = i < n ? counts[i] : 0, mx = i < n ? keys[i] : 0;
    uint64_t ex_sum, ex_mx, tot_sum, tot_mx;
    token_doc_scan(sum, mx, ex_sum, ex_mx, tot_sum, tot_mx, lds);
    if (i < n) {
      counts[i] = carry_sum + ex_sum;
      keys[i] = ex_mx > carry_mx ? ex_mx : carry_mx;
    }
    carry_sum += tot_sum;
    carry_mx = tot_mx > carry_mx ? tot_mx : carry_mx;
  }
  if (threadIdx.x == 0) result[0] = rows + carry_sum;
}

template <int DS>
__device__ __forceinline__ uint64_t token_doc_write(
    const uint8_t* x, uint64_t T, uint64_t cpr, uint64_t eos,
    const uint64_t* counts, const uint64_t* keys, uint8_t* pos_out,
    uint8_t* doc_out, int32_t* cu, uint64_t* lds) {
  uint64_t chunk = blockIdx.x;
  TokenDocSpan s = token_doc_span(chunk, cpr, T);
  uint32_t m = token_doc_span_flags<DS>(x, s, T, eos);
  uint64_t sum = __popc(m);
  uint64_t mx = m ? s.col + (31u - __clz(m)) + 1 : 0;   // start after my last eos
  uint64_t ex_sum, ex_mx, tot_sum, tot_mx;
  token_doc_scan(sum, mx, ex_sum, ex_mx, tot_sum, tot_mx, lds);
  uint64_t row_base = counts[s.row * cpr];     // starts of the rows before
  uint64_t start_in = token_doc_start(keys[chunk], s.row, T);
  TokenDocState st;
  st.docs = counts[chunk] - row_base + ex_sum;
  st.start = ex_mx > start_in ? ex_mx : start_in;
  uint64_t seq0 = s.row + row_base;            // cu entry of the row's column 0
  uint64_t pos[TOKEN_DOC_PER], doc[TOKEN_DOC_PER], longest = 0;
#pragma unroll
  for (int j = 0; j < TOKEN_DOC_PER; ++j) {
    uint64_t len;
    token_doc_one(st, s.col + j, (m >> j) & 1u, T, pos[j], doc[j], len);
    if ((uint32_t)j < s.nv) {
      longest = len > longest ? len : longest;
      if (cu && pos[j] == 0)
        cu[seq0 + doc[j]] = (int32_t)(s.row * T + s.col + j);
    }
  }
  if (s.nv) {
    uint64_t at = (s.row * T + s.col) * DS;
    if (pos_out) token_doc_store<DS>(pos_out + at, pos, s.nv);
    if (doc_out) token_doc_store<DS>(doc_out + at, doc, s.nv);
  }
  return longest;
}

// grid = rows * cpr chunks, after token_doc_offsets_kernel.  pos_out,
// doc_out and cu may each be null.  result[0] = n_seqs (read), result[1] =
// max_seqlen (zeroed before the launch; at most one atomicMax per workgroup).
extern "C" __global__ __launch_bounds__(WG) void token_doc_write_kernel(
    const uint8_t* __restrict__ x, uint64_t rows, uint64_t T, uint64_t cpr,
    uint32_t ds, uint64_t eos, const uint64_t* __restrict__ counts,
    const uint64_t* __restrict__ keys, uint8_t* __restrict__ pos_out,
    uint8_t* __restrict__ doc_out, int32_t* __restrict__ cu,
    unsigned long long* __restrict__ result) {
  __shared__ uint64_t lds[2 * (WG / 64)];
  uint64_t longest =
      ds == 8 ? token_doc_write<8>(x, T, cpr, eos, counts, keys, pos_out,
                                   doc_out, cu, lds)
              : token_doc_write<4>(x, T, cpr, eos, counts, keys, pos_out,
                                   doc_out, cu, lds);
  // lanes -> wave (cross-lane) -> workgroup (LDS) -> one atomicMax
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    uint64_t v = __shfl_xor((unsigned long long)longest, o);
    longest = v > longest ? v : longest;
  }
  if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = longest;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t v = 0;
#pragma unroll
    for (int w = 0; w < WG / 64; ++w) v = lds[w] > v ? lds[w] : v;
    if (v) atomicMax(result + 1, (unsigned long long)v);
    if (cu && blockIdx.x == 0) cu[result[0]] = (int32_t)(rows * T);
  }
}

// host memory: the same scalar routines, plain loops.  Outputs may be null.
static void token_docs_host(const uint8_t* x, uint64_t rows, uint64_t T,
                            uint32_t ds, uint64_t eos, uint8_t* pos_out,
                            uint8_t* doc_out, int32_t* cu, uint64_t& n_seqs,
                            uint64_t& max_seqlen) {
  n_seqs = 0;
  max_seqlen = 0;
  for (uint64_t r = 0; r < rows; ++r) {
    TokenDocState st{0, 0};
    for (uint64_t t = 0; t < T; ++t) {
      uint64_t at = r * T + t, pos, doc, len;
      bool e = token_is_eos(token_doc_load(x + at * ds, ds), eos);
      token_doc_one(st, t, e, T, pos, doc, len);
      if (pos == 0) {
        if (cu) cu[n_seqs] = (int32_t)at;
        n_seqs++;
      }
      if (pos_out) token_store(pos_out + at * ds, pos, ds);
      if (doc_out) token_store(doc_out + at * ds, doc, ds);
      if (len > max_seqlen) max_seqlen = len;
    }
  }
  if (cu) cu[n_seqs] = (int32_t)(rows * T);
}

// LZ4 block codec: host compress/decompress + gfx950 device compress and
// decompress.
//
// Covers the reference's lz4 sites (raft snapshot streams,
// RocksDB block compression; new-engine kernel "lz4_decompress_stream").
// Container "CVLZ" = raw_size u64 | chunk_size u32 | n_chunks u32 |
// comp_size[n] u32 | chunk payloads.  Chunks compress independently so the
// GPU decompresses them in parallel (one workgroup per chunk; the
// sequential nature of LZ4 keeps per-chunk work serial — parallelism comes
// from chunk count, which saturates the chip for multi-MB streams).
//
// Block format per LZ4 spec: token(4b lit|4b match), ext lens (255...),
// literals, 2B little-endian offset, match >= 4.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <vector>

static const uint32_t LZ4_MAGIC = 0x435A4C34u;  // "4LZC"
static const int LZ4_CHUNK = 64 * 1024;

// ---------------------------------------------------------------------------
// host compress (greedy hash table, LZ4-block compatible)
// ---------------------------------------------------------------------------

static inline uint32_t lz4_hash(uint32_t v) {
  return (v * 2654435761u) >> 19;   // 13-bit table
}

static size_t lz4_compress_block(const uint8_t* src, size_t n, uint8_t* dst) {
  uint32_t table[1 << 13];
  memset(table, 0xFF, sizeof(table));
  size_t si = 0, di = 0, anchor = 0;
  if (n >= 13) {
    while (si + 12 < n) {
      uint32_t seq;
      memcpy(&seq, src + si, 4);
      uint32_t h = lz4_hash(seq);
      uint32_t cand = table[h];
      table[h] = (uint32_t)si;
      uint32_t ref_seq = 0;
      if (cand != 0xFFFFFFFFu && si - cand <= 65535) {
        memcpy(&ref_seq, src + cand, 4);
      }
      if (cand == 0xFFFFFFFFu || si - cand > 65535 || ref_seq != seq) {
        si++;
        continue;
      }
      // extend match (leave 5 bytes for the closing literals-only sequence)
      size_t mlen = 4;
      while (si + mlen < n - 5 && src[si + mlen] == src[cand + mlen]) mlen++;
      size_t lit = si - anchor;
      // token
      uint8_t* tok = dst + di++;
      *tok = 0;
      if (lit >= 15) {
        *tok |= 0xF0;
        size_t rest = lit - 15;
        while (rest >= 255) { dst[di++] = 255; rest -= 255; }
        dst[di++] = (uint8_t)rest;
      } else {
        *tok |= (uint8_t)(lit << 4);
      }
      memcpy(dst + di, src + anchor, lit);
      di += lit;
      uint16_t off = (uint16_t)(si - cand);
      dst[di++] = off & 0xFF;
      dst[di++] = off >> 8;
      size_t mrest = mlen - 4;
      if (mrest >= 15) {
        *tok |= 0x0F;
        mrest -= 15;
        while (mrest >= 255) { dst[di++] = 255; mrest -= 255; }
        dst[di++] = (uint8_t)mrest;
      } else {
        *tok |= (uint8_t)mrest;
      }
      si += mlen;
      anchor = si;
    }
  }
  // final literals
  size_t lit = n - anchor;
  uint8_t* tok = dst + di++;
  *tok = 0;
  if (lit >= 15) {
    *tok |= 0xF0;
    size_t rest = lit - 15;
    while (rest >= 255) { dst[di++] = 255; rest -= 255; }
    dst[di++] = (uint8_t)rest;
  } else {
    *tok |= (uint8_t)(lit << 4);
  }
  memcpy(dst + di, src + anchor, lit);
  di += lit;
  return di;
}

static size_t lz4_decompress_block_host(const uint8_t* src, size_t comp_n,
                                        uint8_t* dst, size_t cap) {
  size_t si = 0, di = 0;
  while (si < comp_n) {
    uint8_t tok = src[si++];
    size_t lit = tok >> 4;
    if (lit == 15) {
      uint8_t b;
      do {
        if (si >= comp_n) return (size_t)-1;
        b = src[si++]; lit += b;
      } while (b == 255);
    }
    if (di + lit > cap || si + lit > comp_n) return (size_t)-1;
    memcpy(dst + di, src + si, lit);
    di += lit; si += lit;
    if (si >= comp_n) break;   // last sequence has no match
    if (si + 2 > comp_n) return (size_t)-1;
    uint16_t off = src[si] | (src[si + 1] << 8);
    si += 2;
    size_t mlen = (tok & 0xF);
    if (mlen == 15) {
      uint8_t b;
      do {
        if (si >= comp_n) return (size_t)-1;
        b = src[si++]; mlen += b;
      } while (b == 255);
    }
    mlen += 4;
    if (off == 0 || off > di || di + mlen > cap) return (size_t)-1;
    // overlapping copy byte-by-byte
    for (size_t i = 0; i < mlen; ++i) { dst[di] = dst[di - off]; di++; }
  }
  return di;
}

// ---------------------------------------------------------------------------
// device decompress: one workgroup per chunk; lane 0 walks the sequences,
// the full wave does the literal copies (match copies are wave-wide when
// offset allows, serial otherwise).
// ---------------------------------------------------------------------------

extern "C" __global__ __launch_bounds__(64) void lz4_decompress_kernel(
    const uint8_t* __restrict__ comp, const uint32_t* __restrict__ chunk_off,
    const uint32_t* __restrict__ chunk_len, uint8_t* __restrict__ out,
    uint32_t chunk_size, uint64_t raw_size, uint32_t n_chunks,
    int* __restrict__ error_flag) {
  for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const uint8_t* src = comp + chunk_off[c];
    uint32_t comp_n = chunk_len[c];
    uint8_t* dst = out + (uint64_t)c * chunk_size;
    uint64_t cap = min((uint64_t)chunk_size,
                       raw_size - (uint64_t)c * chunk_size);
    uint32_t si = 0, di = 0;
    int lane = threadIdx.x;
    // The checks are those of lz4_decompress_block_host, in the same
    // order.  Every lane parses the same bytes, so each check, and the
    // return it leads to, is wave-uniform.  Lengths are summed in 64 bits:
    // a run of 255s cannot wrap a bound.
    bool bad = false;
    while (si < comp_n) {
      // every lane parses the same header (uniform addresses broadcast)
      uint8_t tok = src[si++];
      uint64_t lit = tok >> 4;
      if (lit == 15) {
        uint8_t b;
        do {
          if (si >= comp_n) { bad = true; break; }
          b = src[si++]; lit += b;
        } while (b == 255);
      }
      if (bad || (uint64_t)di + lit > cap || (uint64_t)si + lit > comp_n) {
        bad = true;
        break;
      }
      for (uint32_t i = lane; i < (uint32_t)lit; i += 64)
        dst[di + i] = src[si + i];
      __threadfence_block();   // cross-lane visibility of the writes
      di += (uint32_t)lit; si += (uint32_t)lit;
      if (si >= comp_n) break;
      if ((uint64_t)si + 2 > comp_n) { bad = true; break; }
      uint32_t off = src[si] | (src[si + 1] << 8);
      si += 2;
      uint64_t mlen = (tok & 0xF);
      if (mlen == 15) {
        uint8_t b;
        do {
          if (si >= comp_n) { bad = true; break; }
          b = src[si++]; mlen += b;
        } while (b == 255);
      }
      mlen += 4;
      if (bad || off == 0 || off > di || (uint64_t)di + mlen > cap) {
        bad = true;
        break;
      }
      // match bytes are periodic with period `off`: every lane reads only
      // PRE-MATCH data (dst[di-off .. di)), so there is no intra-match
      // hazard for any offset
      for (uint32_t i = lane; i < (uint32_t)mlen; i += 64)
        dst[di + i] = dst[di - off + (i % off)];
      __threadfence_block();
      di += (uint32_t)mlen;
    }
    // a chunk that decodes short leaves stale bytes in the block: the host
    // decoder's `got != cap`
    if (bad || di != cap) {
      if (lane == 0) atomicExch(error_flag, 1 + (int)c);
      return;
    }
  }
}

// ---------------------------------------------------------------------------
// device compress: one wave per 64 KiB chunk.  The chunk is staged into LDS
// (global reads are then one coalesced pass), the wave hashes 64 candidate
// positions per step, and extension/emission are wave-cooperative.  All
// control flow is wave-uniform: pos/anchor/di hold the same value in every
// lane, exactly like the sequence walk of the decompress kernel.
//
// Determinism: the position table is only ever updated with atomicMax of
// (position + 1), so when several lanes hash to one entry the LAST position
// wins by rule, not by store order; the in-step table uses atomicMin of the
// lane id (FIRST lane wins).  Entries are never trusted: every candidate is
// checked for cand < pos and for the 4 matching bytes.
//
// LDS: 64 KiB + 16 chunk image, 32 KiB position table (8192 x u32, 0 =
// empty), 8 KiB in-step table = ~104 KiB, i.e. one wave per CU, which is
// what a 16 MiB call (256 chunks over 256 CUs) needs.
// ---------------------------------------------------------------------------

// worst-case LZ4 block for one chunk, rounded up to 64 B
static const uint32_t LZ4_SLOT_STRIDE =
    ((LZ4_CHUNK + LZ4_CHUNK / 255 + 16 + 63) / 64) * 64;
static const uint64_t LZ4_DEVICE_MAX_N = 16ull << 20;   // per compress call

#define LZ4C_TABLE 8192     // position table entries (13-bit hash)
#define LZ4C_STEP 2048      // in-step table entries

__device__ __forceinline__ uint32_t lz4c_read32(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

// token-extension bytes for a length field >= 15: (len-15)/255 bytes of 255
// then one byte of (len-15)%255; lanes write them 64 at a time
__device__ __forceinline__ uint32_t lz4c_emit_ext(uint8_t* dst, uint32_t len,
                                                  int lane) {
  uint32_t rest = len - 15;
  uint32_t nb = rest / 255 + 1;
  for (uint32_t i = lane; i < nb; i += 64)
    dst[i] = (i + 1 == nb) ? (uint8_t)(rest % 255) : (uint8_t)255;
  return nb;
}

// copy len literal bytes LDS -> global: 16 B per lane once dst is aligned
__device__ __forceinline__ void lz4c_emit_lits(uint8_t* dst,
                                               const uint8_t* src,
                                               uint32_t len, int lane) {
  uint32_t head = 0;
  if (len >= 256) {
    head = (uint32_t)((16 - ((uintptr_t)dst & 15)) & 15);
    uint32_t body = (len - head) / 16;
    for (uint32_t i = lane; i < body; i += 64) {
      uint4 v;
      __builtin_memcpy(&v, src + head + i * 16, 16);
      *reinterpret_cast<uint4*>(dst + head + i * 16) = v;
    }
    for (uint32_t i = lane; i < head; i += 64) dst[i] = src[i];
    head += body * 16;
  }
  for (uint32_t i = head + lane; i < len; i += 64) dst[i] = src[i];
}

extern "C" __global__ __launch_bounds__(64) void lz4_compress_kernel(
    const uint8_t* __restrict__ base, uint64_t off, uint64_t n,
    uint32_t chunk_size, uint8_t* __restrict__ slot_base,
    uint32_t slot_stride, uint32_t* __restrict__ out_len, uint32_t n_chunks,
    int* __restrict__ error_flag) {
  __shared__ __attribute__((aligned(16))) uint8_t img[LZ4_CHUNK + 16];
  __shared__ uint32_t table[LZ4C_TABLE];
  __shared__ uint32_t step_tab[LZ4C_STEP];
  const int lane = threadIdx.x;
  if (chunk_size > (uint32_t)LZ4_CHUNK) {   // the LDS image holds one chunk
    if (lane == 0 && blockIdx.x == 0) atomicExch(error_flag, 1);
    return;
  }
  for (uint32_t i = lane; i < LZ4C_STEP; i += 64) step_tab[i] = 0xFFFFFFFFu;
  for (uint32_t c = blockIdx.x; c < n_chunks; c += gridDim.x) {
    const uint8_t* g = base + off + (uint64_t)c * chunk_size;
    const uint32_t cn =
        (uint32_t)min((uint64_t)chunk_size, n - (uint64_t)c * chunk_size);
    uint8_t* dst = slot_base + (uint64_t)c * slot_stride;
    __syncthreads();   // previous chunk's LDS reads are done
    // stage the chunk at the same 16 B misalignment it has in memory, so
    // the body is aligned uint4 loads; head and tail go byte-wise and no
    // byte outside [g, g + cn) is read
    const uint32_t mis = (uint32_t)((uintptr_t)g & 15);
    const uint8_t* src = img + mis;
    {
      uint32_t head = min((16 - mis) & 15, cn);
      uint32_t body = (cn - head) / 16;
      for (uint32_t i = lane; i < head; i += 64) img[mis + i] = g[i];
      const uint4* g4 = reinterpret_cast<const uint4*>(g + head);
      uint4* l4 = reinterpret_cast<uint4*>(img + mis + head);
      for (uint32_t i = lane; i < body; i += 64) l4[i] = g4[i];
      for (uint32_t i = head + body * 16 + lane; i < cn; i += 64)
        img[mis + i] = g[i];
    }
    for (uint32_t i = lane; i < LZ4C_TABLE; i += 64) table[i] = 0;
    __syncthreads();

    uint32_t pos = 0, anchor = 0, di = 0;
    bool overflow = false;
    // a match may start only where pos + 12 < cn (end-of-block rule)
    const uint32_t mflimit = cn >= 13 ? cn - 12 : 0;
    const uint32_t mend = cn >= 5 ? cn - 5 : 0;     // matches end here
    while (pos < mflimit) {
      const uint32_t p = pos + lane;
      const bool valid = p < mflimit;
      const uint32_t seq = lz4c_read32(src + (valid ? p : 0));
      const uint32_t h = (seq * 2654435761u) >> 19;
      // candidate from earlier steps; entry = position + 1, 0 = empty
      const uint32_t e = valid ? table[h] : 0;
      uint32_t cand = e - 1;
      bool ok = valid && e != 0 && cand < p &&
                lz4c_read32(src + cand) == seq;
      unsigned long long mask = __ballot(ok);
      if (mask == 0) {
        // nothing in the history: look inside this step.  The lowest lane
        // with the same table slot is the candidate for every higher lane.
        const uint32_t s = h & (LZ4C_STEP - 1);
        if (valid) atomicMin(&step_tab[s], (uint32_t)lane);
        __syncthreads();
        const uint32_t j = valid ? step_tab[s] : (uint32_t)lane;
        const uint32_t jseq = __shfl(seq, (int)(j & 63));
        ok = valid && j < (uint32_t)lane && jseq == seq;
        cand = pos + j;
        __syncthreads();
        if (valid) step_tab[s] = 0xFFFFFFFFu;   // every writer: same value
        mask = __ballot(ok);
      }
      const int f = mask ? __ffsll((long long)mask) - 1 : 63;
      // insert the positions up to and including the match start
      if (valid && lane <= f) atomicMax(&table[h], p + 1);
      if (mask == 0) {
        pos += 64;
        __syncthreads();
        continue;
      }
      const uint32_t mp = pos + f;                       // match start
      const uint32_t mc = __shfl(cand, f);               // its candidate
      // extend: 4 bytes per lane, 256 per step, never past mend
      const uint32_t maxlen = mend - mp;                 // >= 7
      uint32_t mlen = 4;
      while (mlen < maxlen) {
        uint32_t k = mlen + 4 * lane;
        // reads clamped inside the chunk; anything past maxlen is cut below
        uint32_t ia = min(mp + k, cn - 4), ib = min(mc + k, cn - 4);
        uint32_t d = lz4c_read32(src + ia) ^ lz4c_read32(src + ib);
        unsigned long long diff = __ballot(d != 0);
        if (diff == 0) { mlen += 256; continue; }
        int fl = __ffsll((long long)diff) - 1;
        uint32_t dd = __shfl(d, fl);
        mlen += 4 * fl + ((uint32_t)__ffs((int)dd) - 1) / 8;
        break;
      }
      mlen = min(mlen, maxlen);
      const uint32_t lit = mp - anchor;
      // a slot holds the LZ4 worst case, so this never fires; it guards
      // the stores below all the same
      if (di + 1 + lit / 255 + 1 + lit + 2 + mlen / 255 + 1 > slot_stride) {
        overflow = true;
        break;
      }
      const uint32_t mrest = mlen - 4;
      if (lane == 0)
        dst[di] = (uint8_t)((lit >= 15 ? 15 : lit) << 4 |
                            (mrest >= 15 ? 15 : mrest));
      di += 1;
      if (lit >= 15) di += lz4c_emit_ext(dst + di, lit, lane);
      lz4c_emit_lits(dst + di, src + anchor, lit, lane);
      di += lit;
      const uint32_t moff = mp - mc;
      if (lane == 0) {
        dst[di] = (uint8_t)(moff & 0xFF);
        dst[di + 1] = (uint8_t)(moff >> 8);
      }
      di += 2;
      if (mrest >= 15) di += lz4c_emit_ext(dst + di, mrest, lane);
      pos = mp + mlen;
      anchor = pos;
      __syncthreads();   // table inserts land before the next lookups
    }
    // closing literals-only sequence
    const uint32_t lit = cn - anchor;
    if (!overflow && di + 1 + lit / 255 + 1 + lit > slot_stride)
      overflow = true;
    if (overflow) {
      if (lane == 0) {
        atomicExch(error_flag, 1 + (int)c);
        out_len[c] = 0;
      }
      continue;
    }
    if (lane == 0) dst[di] = (uint8_t)((lit >= 15 ? 15 : lit) << 4);
    di += 1;
    if (lit >= 15) di += lz4c_emit_ext(dst + di, lit, lane);
    lz4c_emit_lits(dst + di, src + anchor, lit, lane);
    di += lit;
    if (lane == 0) out_len[c] = di;
  }
}

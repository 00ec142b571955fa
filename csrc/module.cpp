// curvine_amd native data plane: HBM block arenas, pinned staging
// pipelines, and CDNA4 kernel wrappers (kernels.hip).
//
// This is the MI355X-era equivalent of the reference's native layer
// (/root/reference/crates/core/curvine-sys: sendfile/splice/fadvise are the
// CPU fallback path there; here the hot path is hipMemcpyAsync through a
// pinned ring + device kernels).  Torch-free on purpose: consumers pass raw
// device pointers (e.g. torch tensor.data_ptr()) for GPU-to-GPU reads.
//
// Arena model: one big hipMalloc per (device, arena) — the HBM tier of the
// worker block store (BdevLayout/BdevOffsetAllocator analog,
// /root/reference/crates/adapters/curvine-storage-local/src/layout/
// bdev_layout.rs:30-111); offset allocation lives in Python
// (curvine_amd/worker/arena_alloc.py), this layer moves bytes.

#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <sys/mman.h>

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <memory>
#include <mutex>
#include <stdexcept>
#include <string>
#include <variant>
#include <vector>

#include <hip/hip_runtime.h>

namespace py = pybind11;

// Kernels live in this translation unit (device symbols + hipMemcpyToSymbol
// need no -fgpu-rdc this way).  kernels.hip comes first: it owns WG and
// CRC_SUB, which the host CRC tables below are built from.
#include "kernels.hip"

#define HIP_CHECK(expr)                                                        \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess)                                                      \
      throw std::runtime_error(std::string(#expr) + ": " +                     \
                               hipGetErrorString(_e));                         \
  } while (0)

// ---------------------------------------------------------------------------
// CRC32C (Castagnoli): host tables, SW slice-by-8, GF(2) combine
// ---------------------------------------------------------------------------

static uint32_t crc_tab[8][256];
static uint32_t comb_mat[24][32];  // shift by (CRC_SUB << k) bytes
static const uint32_t CRC_POLY = 0x82F63B78u;  // reflected Castagnoli

static void gf2_square(uint32_t dst[32], const uint32_t src[32]) {
  for (int i = 0; i < 32; ++i) {
    uint32_t v = src[i], out = 0;
    for (int b = 0; b < 32; ++b)
      if ((v >> b) & 1) out ^= src[b];
    dst[i] = out;
  }
}

static uint32_t gf2_apply(const uint32_t mat[32], uint32_t crc) {
  uint32_t out = 0;
  for (int i = 0; i < 32; ++i)
    if ((crc >> i) & 1) out ^= mat[i];
  return out;
}

static void crc_init_tables() {
  for (uint32_t i = 0; i < 256; ++i) {
    uint32_t c = i;
    for (int k = 0; k < 8; ++k) c = (c >> 1) ^ ((c & 1) ? CRC_POLY : 0);
    crc_tab[0][i] = c;
  }
  for (int t = 1; t < 8; ++t)
    for (uint32_t i = 0; i < 256; ++i)
      crc_tab[t][i] = (crc_tab[t - 1][i] >> 8) ^ crc_tab[0][crc_tab[t - 1][i] & 0xFF];

  // M1 = append-one-zero-bit operator; comb_mat[0] = M1^(8*CRC_SUB)
  uint32_t m[32], tmp[32];
  m[0] = CRC_POLY;
  for (int i = 1; i < 32; ++i) m[i] = 1u << (i - 1);
  // raise to 8*CRC_SUB = 2^15 -> square 15 times
  int shift_bits_log2 = 0;
  {
    uint64_t bits = 8ull * CRC_SUB;  // 32768 = 2^15
    while ((1ull << shift_bits_log2) < bits) shift_bits_log2++;
  }
  for (int s = 0; s < shift_bits_log2; ++s) {
    gf2_square(tmp, m);
    std::memcpy(m, tmp, sizeof(m));
  }
  std::memcpy(comb_mat[0], m, sizeof(m));
  for (int k = 1; k < 24; ++k) gf2_square(comb_mat[k], comb_mat[k - 1]);
}

// built once, before the first reader: every host CRC goes through
// crc32c_sw, and the device upload calls this before it copies the tables
static void crc_host_tables() {
  static std::once_flag once;
  std::call_once(once, crc_init_tables);
}

static uint32_t crc32c_sw(const uint8_t* p, size_t n, uint32_t crc_in) {
  crc_host_tables();
  uint32_t crc = crc_in ^ 0xFFFFFFFFu;
  while (n && ((uintptr_t)p & 7)) { crc = (crc >> 8) ^ crc_tab[0][(crc ^ *p++) & 0xFF]; --n; }
#if defined(__SSE4_2__)
  while (n >= 8) {
    crc = (uint32_t)__builtin_ia32_crc32di(crc, *(const uint64_t*)p);
    p += 8; n -= 8;
  }
  while (n) { crc = __builtin_ia32_crc32qi(crc, *p++); --n; }
#else
  while (n >= 8) {
    uint64_t v = *(const uint64_t*)p;
    uint32_t lo = (uint32_t)v ^ crc, hi = (uint32_t)(v >> 32);
    crc = crc_tab[7][lo & 0xFF] ^ crc_tab[6][(lo >> 8) & 0xFF] ^
          crc_tab[5][(lo >> 16) & 0xFF] ^ crc_tab[4][lo >> 24] ^
          crc_tab[3][hi & 0xFF] ^ crc_tab[2][(hi >> 8) & 0xFF] ^
          crc_tab[1][(hi >> 16) & 0xFF] ^ crc_tab[0][hi >> 24];
    p += 8; n -= 8;
  }
  while (n) { crc = (crc >> 8) ^ crc_tab[0][(crc ^ *p++) & 0xFF]; --n; }
#endif
  return crc ^ 0xFFFFFFFFu;
}

// shift a finalized crc over `len` zero bytes (zlib crc32_combine algebra)
static uint32_t crc32c_shift(uint32_t crc, uint64_t len) {
  if (!len) return crc;
  uint32_t m[32], sq[32];
  m[0] = CRC_POLY;
  for (int i = 1; i < 32; ++i) m[i] = 1u << (i - 1);
  // m = M1 (one bit). apply for each set bit of 8*len.
  uint64_t bits = 8ull * len;
  while (bits) {
    if (bits & 1) crc = gf2_apply(m, crc);
    bits >>= 1;
    if (bits) { gf2_square(sq, m); std::memcpy(m, sq, sizeof(m)); }
  }
  return crc;
}

static uint32_t crc32c_combine(uint32_t crc1, uint32_t crc2, uint64_t len2) {
  return crc32c_shift(crc1, len2) ^ crc2;
}

#include "lz4.hip"
#include "tensor_cast.hip"
#include "mx_cast.hip"
#include "block_cast.hip"
#include "token_gather.hip"
#include "token_docs.hip"
#include "token_pack.hip"
#include "array_gather.hip"

// ---------------------------------------------------------------------------
// GPU availability
// ---------------------------------------------------------------------------

static int cached_device_count = -2;
static int device_count() {
  if (cached_device_count == -2) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    cached_device_count = n;
  }
  return cached_device_count;
}

// ---------------------------------------------------------------------------
// Arena
// ---------------------------------------------------------------------------

struct Arena {
  void* base = nullptr;
  size_t cap = 0;
  int device = -1;       // -1 = host memory (CPU fallback / MEM tier)
  bool pinned = false;   // host arena allocated with hipHostMalloc
  hipStream_t stream = nullptr;       // copy stream
  hipStream_t kstream = nullptr;      // kernel stream
  // pinned staging ring (device arenas)
  std::vector<void*> pin;
  std::vector<hipEvent_t> ev;
  size_t pin_sz = 0;
  // device scratch for gather/crc results
  void* scratch = nullptr;
  size_t scratch_sz = 0;
  // true when base came from hipIpcOpenMemHandle (another process's
  // arena): destroy closes the mapping instead of freeing
  bool ipc_imported = false;
  std::mutex mu;

  Arena(int device_, size_t cap_) : cap(cap_), device(device_) {}
  Arena(const Arena&) = delete;
  Arena& operator=(const Arena&) = delete;

  bool is_dev() const { return device >= 0; }

  void open_streams() {
    HIP_CHECK(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    HIP_CHECK(hipStreamCreateWithFlags(&kstream, hipStreamNonBlocking));
  }

  // frees whatever exists, so an arena that failed half-way through its
  // construction unwinds through here too
  ~Arena() {
    if (is_dev()) {
      hipSetDevice(device);
      if (stream) hipStreamSynchronize(stream);
      for (auto* p : pin) if (p) hipHostFree(p);
      for (auto e : ev) if (e) hipEventDestroy(e);
      if (scratch) hipFree(scratch);
      if (base) {
        if (ipc_imported) hipIpcCloseMemHandle(base);
        else hipFree(base);
      }
      if (stream) hipStreamDestroy(stream);
      if (kstream) hipStreamDestroy(kstream);
    } else if (pinned) {
      hipHostFree(base);
    } else {
      std::free(base);
    }
  }
};

static std::vector<Arena*> g_arenas;
static std::mutex g_arenas_mu;

static Arena* get_arena(int h) {
  std::lock_guard<std::mutex> g(g_arenas_mu);
  if (h < 0 || h >= (int)g_arenas.size() || !g_arenas[h])
    throw std::runtime_error("bad arena handle");
  return g_arenas[h];
}

// hand a finished arena to the handle table (first free slot)
static int arena_register(std::unique_ptr<Arena> a) {
  std::lock_guard<std::mutex> g(g_arenas_mu);
  size_t i = 0;
  while (i < g_arenas.size() && g_arenas[i]) ++i;
  if (i == g_arenas.size()) g_arenas.push_back(nullptr);
  g_arenas[i] = a.release();
  return (int)i;
}

static int arena_create(int device, size_t cap, size_t staging_bytes,
                        int staging_count, bool host_pinned) {
  if (device >= 0 && device >= device_count())
    throw std::runtime_error("no such GPU device");
  auto a = std::make_unique<Arena>(device, cap);
  if (device >= 0) {
    HIP_CHECK(hipSetDevice(device));
    HIP_CHECK(hipMalloc(&a->base, cap));
    a->open_streams();
    a->pin_sz = staging_bytes;
    a->pin.resize(staging_count);
    a->ev.resize(staging_count);
    for (int i = 0; i < staging_count; ++i) {
      HIP_CHECK(hipHostMalloc(&a->pin[i], staging_bytes, hipHostMallocDefault));
      HIP_CHECK(hipEventCreateWithFlags(&a->ev[i], hipEventDisableTiming));
    }
  } else {
    if (host_pinned && device_count() > 0) {
      HIP_CHECK(hipHostMalloc(&a->base, cap, hipHostMallocDefault));
      a->pinned = true;   // pinning faults every page in
    } else {
      // 2 MiB-aligned + MADV_HUGEPAGE BEFORE the faulting memset: plain
      // malloc starts on 4 KiB pages and copies run TLB-bound at ~2
      // GiB/s until khugepaged collapses them (~7.6 GiB/s after);
      // faulting straight onto huge pages gets the fast path from the
      // first write
      size_t aligned = (cap + ((2u << 20) - 1)) & ~size_t((2u << 20) - 1);
      void* p = nullptr;
      if (posix_memalign(&p, 2u << 20, aligned) != 0) throw std::bad_alloc();
      a->base = p;
#ifdef MADV_HUGEPAGE
      madvise(a->base, aligned, MADV_HUGEPAGE);
#endif
      std::memset(a->base, 0, cap);
    }
  }
  return arena_register(std::move(a));
}

static void arena_destroy(int h) {
  Arena* a;
  {
    std::lock_guard<std::mutex> g(g_arenas_mu);
    if (h < 0 || h >= (int)g_arenas.size() || !g_arenas[h]) return;
    a = g_arenas[h];
    g_arenas[h] = nullptr;
  }
  delete a;
}

// ---- cross-process arena sharing (hipIpc, dmabuf mode) ----
//
// A worker exports its device arena once; a colocated client process
// (FUSE daemon, another engine) opens the handle and reads published
// extents with direct D2H DMA in ITS OWN process — the production
// short-circuit for the one-process-per-GPU deployment shape.

static py::bytes arena_ipc_handle(int h) {
  Arena* a = get_arena(h);
  if (!a->is_dev())
    throw std::runtime_error("ipc export: device arenas only");
  hipIpcMemHandle_t ih;
  HIP_CHECK(hipSetDevice(a->device));
  HIP_CHECK(hipIpcGetMemHandle(&ih, a->base));
  return py::bytes((const char*)&ih, sizeof(ih));
}

static int arena_ipc_open(py::bytes handle, size_t cap, int device) {
  std::string hb = handle;
  if (hb.size() != sizeof(hipIpcMemHandle_t))
    throw std::runtime_error("ipc open: bad handle size");
  if (device < 0 || device >= device_count())
    throw std::runtime_error("ipc open: bad device");
  hipIpcMemHandle_t ih;
  std::memcpy(&ih, hb.data(), sizeof(ih));
  auto a = std::make_unique<Arena>(device, cap);
  a->ipc_imported = true;
  HIP_CHECK(hipSetDevice(device));
  hipError_t e = hipIpcOpenMemHandle(&a->base, ih,
                                     hipIpcMemLazyEnablePeerAccess);
  if (e != hipSuccess) {
    a->base = nullptr;   // nothing was mapped: nothing to close
    throw std::runtime_error(std::string("hipIpcOpenMemHandle: ") +
                             hipGetErrorString(e));
  }
  a->open_streams();
  // no staging ring: reads ride the pooled bounce pairs / pinned dests
  return arena_register(std::move(a));
}

static void ensure_scratch(Arena* a, size_t n) {
  if (a->scratch_sz >= n) return;
  if (a->scratch) {
    // forget the old block before freeing it, so a failing hipMalloc
    // below leaves no dangling pointer for ~Arena to free again
    void* old = a->scratch;
    a->scratch = nullptr;
    a->scratch_sz = 0;
    HIP_CHECK(hipFree(old));
  }
  HIP_CHECK(hipMalloc(&a->scratch, n));
  a->scratch_sz = n;
}

// Bump carver over the arena's device scratch: sized once up front (the
// only ensure_scratch of a call, so no pointer outlives a regrow), then
// hands out typed sub-ranges.  Byte regions start on 64 B, tables on their
// natural alignment; room<T>() is what take<T>() can cost at worst.
// Caller holds a->mu.
struct Scratch {
  uint8_t* p;
  uint8_t* end;
  Scratch(Arena* a, size_t bytes) {
    ensure_scratch(a, bytes);
    p = (uint8_t*)a->scratch;
    end = p + bytes;
  }
  // carve device memory the caller owns (calls not tied to an arena)
  Scratch(void* base, size_t bytes) : p((uint8_t*)base), end(p + bytes) {}
  template <class T> static constexpr size_t align() {
    return sizeof(T) == 1 ? 64 : alignof(T);
  }
  template <class T> static size_t room(size_t n) {
    return n * sizeof(T) + align<T>() - 1;
  }
  template <class T> T* take(size_t n) {
    uintptr_t at = ((uintptr_t)p + align<T>() - 1) & ~(uintptr_t)(align<T>() - 1);
    p = (uint8_t*)at + n * sizeof(T);
    if (p > end) throw std::logic_error("scratch carve exceeds its sizing");
    return (T*)at;
  }
};

// device memory of one call that is not tied to an arena, carved the same
// way: allocated here, freed when the call returns (after its last sync)
struct CallScratch : Scratch {
  void* mem;
  static void* alloc(size_t bytes) {
    void* p = nullptr;
    HIP_CHECK(hipMalloc(&p, bytes));
    return p;
  }
  explicit CallScratch(size_t bytes) : Scratch(alloc(bytes), bytes), mem(p) {}
  CallScratch(const CallScratch&) = delete;
  CallScratch& operator=(const CallScratch&) = delete;
  ~CallScratch() { (void)hipFree(mem); }
};

// g_crc_tab / g_comb_mat are per-device symbols: upload once per device,
// under a lock of their own, so no arena re-uploads them under another
// arena's running CRC kernel.  Caller has set the device.
static void ensure_crc_tables(int device) {
  static std::mutex mu;
  static std::vector<char> uploaded;
  std::lock_guard<std::mutex> g(mu);
  if ((size_t)device < uploaded.size() && uploaded[device]) return;
  crc_host_tables();
  HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_crc_tab), crc_tab, sizeof(crc_tab)));
  HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_comb_mat), comb_mat, sizeof(comb_mat)));
  if ((size_t)device >= uploaded.size()) uploaded.resize(device + 1);
  uploaded[device] = 1;
}

// ---- host<->arena copies with pinned-ring pipelining ----

static void check_range(Arena* a, uint64_t off, uint64_t n) {
  if (off + n > a->cap) throw std::runtime_error("arena range out of bounds");
}

static bool is_pinned_host(const void* p) {
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, p) != hipSuccess) {
    (void)hipGetLastError();   // clear the error
    return false;
  }
  return at.type == hipMemoryTypeHost;
}

// small or pinned-destination copies skip the ring: one hipMemcpyAsync on
// the caller's thread stream (parallel across caller threads, no global lock)
static const uint64_t RING_THRESHOLD = 2u << 20;

// ------------------------------------------------------- pinned bounce pool

// hipHostMalloc costs ~1 ms: a per-device free-list of double-buffer
// bounce pairs makes HBM stream opens O(microseconds) after warmup
struct BouncePair {
  void* pin[2] = {nullptr, nullptr};
  hipEvent_t ev[2] = {};
  int device = -1;
};

static constexpr size_t kBounceSz = 8 << 20;

struct BouncePool {
  std::mutex mu;
  std::unordered_map<int, std::vector<BouncePair*>> free_by_dev;
};
static BouncePool g_bounce;

static BouncePair* bounce_acquire(int device) {
  {
    std::lock_guard<std::mutex> g(g_bounce.mu);
    auto& v = g_bounce.free_by_dev[device];
    if (!v.empty()) {
      BouncePair* b = v.back();
      v.pop_back();
      return b;
    }
  }
  auto* b = new BouncePair();
  b->device = device;
  HIP_CHECK(hipSetDevice(device));
  HIP_CHECK(hipHostMalloc(&b->pin[0], kBounceSz, hipHostMallocDefault));
  HIP_CHECK(hipHostMalloc(&b->pin[1], kBounceSz, hipHostMallocDefault));
  HIP_CHECK(hipEventCreateWithFlags(&b->ev[0], hipEventDisableTiming));
  HIP_CHECK(hipEventCreateWithFlags(&b->ev[1], hipEventDisableTiming));
  return b;
}

static void bounce_release(BouncePair* b) {
  std::lock_guard<std::mutex> g(g_bounce.mu);
  auto& v = g_bounce.free_by_dev[b->device];
  if (v.size() >= 32) {
    hipEventDestroy(b->ev[0]);
    hipEventDestroy(b->ev[1]);
    hipHostFree(b->pin[0]);
    hipHostFree(b->pin[1]);
    delete b;
    return;
  }
  v.push_back(b);
}

// per-caller-thread stream: zero contention for concurrent small copies
// (the 4K-IOPS path).  hipMemcpy on the null stream and ROCm's internal
// pageable-staging lock both serialize; a thread_local stream does not.
// A thread that exits parks its streams on a per-device free list (bounded:
// no leak under thread churn) and the next new thread takes one from there,
// so short-lived reader threads pay no stream create/destroy — except
// during process teardown, when the HIP runtime may already be gone.
static std::atomic<bool> g_process_exiting{false};
static struct ExitFlagSetter {
  ~ExitFlagSetter() { g_process_exiting.store(true); }
} g_exit_flag_setter;

// counters behind hip_pool_stats()
static std::atomic<uint64_t> g_st_pinned_created{0}, g_st_pinned_reused{0},
    g_st_streams_created{0}, g_st_streams_reused{0}, g_st_reader_pread{0};

static constexpr int kMaxDevices = 64;
static constexpr size_t kStreamPoolPerDev = 64;

struct StreamPool {
  std::mutex mu;
  std::vector<hipStream_t> free_by_dev[kMaxDevices];
};

// leaked on purpose: thread_local destructors of late-exiting threads run
// after static destructors would have torn a plain static down
static StreamPool& stream_pool() {
  static StreamPool* p = new StreamPool();
  return *p;
}

struct TlsStreams {
  hipStream_t s[kMaxDevices] = {};
  ~TlsStreams() {
    if (g_process_exiting.load()) return;
    for (int d = 0; d < kMaxDevices; ++d) {
      hipStream_t x = s[d];
      if (!x) continue;
      // a parked stream must be idle: its next owner syncs on it
      if (hipStreamQuery(x) != hipSuccess) {
        (void)hipGetLastError();
        (void)hipStreamSynchronize(x);
      }
      StreamPool& p = stream_pool();
      {
        std::lock_guard<std::mutex> g(p.mu);
        if (p.free_by_dev[d].size() < kStreamPoolPerDev) {
          p.free_by_dev[d].push_back(x);
          x = nullptr;
        }
      }
      if (x) (void)hipStreamDestroy(x);
    }
  }
};

static hipStream_t thread_stream(int device) {
  thread_local TlsStreams tls;
  if (device < 0 || device >= kMaxDevices)
    throw std::runtime_error("bad device");
  if (!tls.s[device]) {
    StreamPool& p = stream_pool();
    {
      std::lock_guard<std::mutex> g(p.mu);
      auto& v = p.free_by_dev[device];
      if (!v.empty()) {
        tls.s[device] = v.back();
        v.pop_back();
      }
    }
    if (tls.s[device]) {
      g_st_streams_reused.fetch_add(1, std::memory_order_relaxed);
    } else {
      HIP_CHECK(hipSetDevice(device));
      HIP_CHECK(hipStreamCreateWithFlags(&tls.s[device],
                                         hipStreamNonBlocking));
      g_st_streams_created.fetch_add(1, std::memory_order_relaxed);
    }
  }
  return tls.s[device];
}

static void dev_read_direct(Arena* a, uint64_t off, uint8_t* dst, uint64_t n) {
  HIP_CHECK(hipSetDevice(a->device));
  hipStream_t s = thread_stream(a->device);
  HIP_CHECK(hipMemcpyAsync(dst, (const uint8_t*)a->base + off, n,
                           hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
}

static void dev_write_direct(Arena* a, uint64_t off, const uint8_t* src,
                             uint64_t n) {
  HIP_CHECK(hipSetDevice(a->device));
  hipStream_t s = thread_stream(a->device);
  HIP_CHECK(hipMemcpyAsync((uint8_t*)a->base + off, src, n,
                           hipMemcpyHostToDevice, s));
  HIP_CHECK(hipStreamSynchronize(s));
}

// A pooled bounce pair on the caller's thread stream.  Going out of scope
// drains the stream first: no in-flight DMA may outlive the pair's turn.
struct BounceLease {
  hipStream_t s;
  BouncePair* bp;
  explicit BounceLease(int device)
      : s(thread_stream(device)), bp(bounce_acquire(device)) {}
  BounceLease(const BounceLease&) = delete;
  BounceLease& operator=(const BounceLease&) = delete;
  ~BounceLease() {
    (void)hipStreamSynchronize(s);
    bounce_release(bp);
  }
};

// device -> host in chunks of `cs` (<= kBounceSz) through a POOLED pinned
// double-buffer on the caller's stream: the D2H DMA of chunk k overlaps
// sink(pinned, offset, len) of chunk k-1, and concurrent readers do not
// serialize on one arena ring.  Chunks reach the sink in order; a sink
// returning false stops the pipeline, which then returns false.
template <class Sink>
static bool d2h_pipeline(Arena* a, const uint8_t* src, uint64_t n, uint64_t cs,
                         Sink&& sink) {
  HIP_CHECK(hipSetDevice(a->device));
  BounceLease l(a->device);
  uint64_t nchunks = (n + cs - 1) / cs;
  for (uint64_t c = 0; c <= nchunks; ++c) {
    if (c < nchunks) {
      uint64_t coff = c * cs;
      HIP_CHECK(hipMemcpyAsync(l.bp->pin[c & 1], src + coff,
                               std::min<uint64_t>(cs, n - coff),
                               hipMemcpyDeviceToHost, l.s));
      HIP_CHECK(hipEventRecord(l.bp->ev[c & 1], l.s));
    }
    if (c > 0) {
      // drain the previous chunk while this one is in flight
      uint64_t poff = (c - 1) * cs;
      HIP_CHECK(hipEventSynchronize(l.bp->ev[(c - 1) & 1]));
      if (!sink((const uint8_t*)l.bp->pin[(c - 1) & 1], poff,
                std::min<uint64_t>(cs, n - poff)))
        return false;
    }
  }
  return true;
}

// device -> unpinned host through the bounce pipeline, memcpy as the sink
static void dev_read(Arena* a, uint64_t off, uint8_t* dst, uint64_t n) {
  if (n <= RING_THRESHOLD || is_pinned_host(dst)) {
    dev_read_direct(a, off, dst, n);
    return;
  }
  uint64_t cs = std::min<uint64_t>(kBounceSz,
                                   std::max<uint64_t>(1u << 20, (n + 1) / 2));
  d2h_pipeline(a, (const uint8_t*)a->base + off, n, cs,
               [dst](const uint8_t* pin, uint64_t coff, uint64_t clen) {
                 std::memcpy(dst + coff, pin, clen);
                 return true;
               });
}

// host -> device, chunked through a POOLED pinned double-buffer on the
// caller's stream: concurrent writers (multi-file ingest, replication
// pushes) each pipeline their own H2D DMAs instead of serializing on
// one arena-wide staging ring.
static void dev_write(Arena* a, uint64_t off, const uint8_t* src, uint64_t n) {
  if (n <= RING_THRESHOLD || is_pinned_host(src)) {
    dev_write_direct(a, off, src, n);
    return;
  }
  HIP_CHECK(hipSetDevice(a->device));
  BounceLease l(a->device);
  uint8_t* dst = (uint8_t*)a->base + off;
  // chunk so every call gets >= 2 chunks: the staging memcpy of chunk
  // k overlaps the H2D DMA of chunk k-1 even for a single 4 MiB write
  uint64_t cs = std::min<uint64_t>(kBounceSz,
                                   std::max<uint64_t>(1u << 20, (n + 1) / 2));
  uint64_t nchunks = (n + cs - 1) / cs;
  for (uint64_t c = 0; c < nchunks; ++c) {
    uint64_t coff = c * cs;
    uint64_t clen = std::min<uint64_t>(cs, n - coff);
    int slot = (int)(c & 1);
    if (c >= 2) HIP_CHECK(hipEventSynchronize(l.bp->ev[slot]));
    std::memcpy(l.bp->pin[slot], src + coff, clen);
    HIP_CHECK(hipMemcpyAsync(dst + coff, l.bp->pin[slot], clen,
                             hipMemcpyHostToDevice, l.s));
    HIP_CHECK(hipEventRecord(l.bp->ev[slot], l.s));
  }
  HIP_CHECK(hipStreamSynchronize(l.s));   // reports a failed copy; the lease
                                          // only drains
}

static void arena_read(int h, uint64_t off, py::buffer buf, uint64_t buf_off,
                       uint64_t n) {
  Arena* a = get_arena(h);
  py::buffer_info info = buf.request(true);
  uint64_t cap = (uint64_t)info.size * (uint64_t)info.itemsize;
  if (buf_off + n > cap) throw std::runtime_error("dst buffer too small");
  check_range(a, off, n);
  uint8_t* dst = (uint8_t*)info.ptr + buf_off;
  py::gil_scoped_release rel;
  if (a->is_dev()) dev_read(a, off, dst, n);
  else std::memcpy(dst, (uint8_t*)a->base + off, n);
}

static void arena_write(int h, uint64_t off, py::buffer buf, uint64_t buf_off,
                        uint64_t n) {
  Arena* a = get_arena(h);
  py::buffer_info info = buf.request(false);
  uint64_t cap = (uint64_t)info.size * (uint64_t)info.itemsize;
  if (buf_off + n > cap) throw std::runtime_error("src buffer too small");
  check_range(a, off, n);
  const uint8_t* src = (const uint8_t*)info.ptr + buf_off;
  py::gil_scoped_release rel;
  if (a->is_dev()) dev_write(a, off, src, n);
  else std::memcpy((uint8_t*)a->base + off, src, n);
}

// raw-pointer variants (torch tensors, pinned reply buffers, other arenas'
// memory).  Copies ride the caller's thread_stream(device): concurrent FUSE
// channel threads each have their own stream, so large D2H copies overlap
// instead of serializing.
static void arena_read_ptr(int h, uint64_t off, uintptr_t dst, uint64_t n,
                           bool dst_is_device) {
  Arena* a = get_arena(h);
  check_range(a, off, n);
  py::gil_scoped_release rel;
  if (a->is_dev()) {
    HIP_CHECK(hipSetDevice(a->device));
    hipStream_t s = thread_stream(a->device);
    HIP_CHECK(hipMemcpyAsync((void*)dst, (uint8_t*)a->base + off, n,
                             dst_is_device ? hipMemcpyDeviceToDevice
                                           : hipMemcpyDeviceToHost, s));
    HIP_CHECK(hipStreamSynchronize(s));
  } else if (dst_is_device) {
    HIP_CHECK(hipMemcpy((void*)dst, (uint8_t*)a->base + off, n,
                        hipMemcpyHostToDevice));
  } else {
    std::memcpy((void*)dst, (uint8_t*)a->base + off, n);
  }
}

static void arena_write_ptr(int h, uint64_t off, uintptr_t src, uint64_t n,
                            bool src_is_device) {
  Arena* a = get_arena(h);
  check_range(a, off, n);
  py::gil_scoped_release rel;
  if (a->is_dev()) {
    HIP_CHECK(hipSetDevice(a->device));
    hipStream_t s = thread_stream(a->device);
    HIP_CHECK(hipMemcpyAsync((uint8_t*)a->base + off, (const void*)src, n,
                             src_is_device ? hipMemcpyDeviceToDevice
                                           : hipMemcpyHostToDevice, s));
    HIP_CHECK(hipStreamSynchronize(s));
  } else if (src_is_device) {
    HIP_CHECK(hipMemcpy((uint8_t*)a->base + off, (const void*)src, n,
                        hipMemcpyDeviceToHost));
  } else {
    std::memcpy((uint8_t*)a->base + off, (const void*)src, n);
  }
}

// arena -> arena (same or cross device / host tiers)
static void arena_copy(int dst_h, uint64_t dst_off, int src_h, uint64_t src_off,
                       uint64_t n) {
  Arena* d = get_arena(dst_h);
  Arena* s = get_arena(src_h);
  check_range(d, dst_off, n);
  check_range(s, src_off, n);
  py::gil_scoped_release rel;
  uint8_t* dp = (uint8_t*)d->base + dst_off;
  uint8_t* sp = (uint8_t*)s->base + src_off;
  if (!d->is_dev() && !s->is_dev()) {
    std::memcpy(dp, sp, n);
    return;
  }
  Arena* deva = d->is_dev() ? d : s;
  std::lock_guard<std::mutex> g(deva->mu);
  HIP_CHECK(hipSetDevice(deva->device));
  hipMemcpyKind kind =
      d->is_dev() ? (s->is_dev() ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice)
                  : hipMemcpyDeviceToHost;
  if (d->is_dev() && s->is_dev() && d->device != s->device) {
    HIP_CHECK(hipMemcpyPeerAsync(dp, d->device, sp, s->device, n, deva->stream));
  } else {
    HIP_CHECK(hipMemcpyAsync(dp, sp, n, kind, deva->stream));
  }
  HIP_CHECK(hipStreamSynchronize(deva->stream));
}

// ---- kernels ----

// every launch: clear the thread's stale last error, launch, and surface a
// launch failure here instead of at some later call
template <class... P, class... A>
static void launch(void (*kernel)(P...), unsigned grid, unsigned block,
                   hipStream_t s, A... args) {
  (void)hipGetLastError();
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, s, args...);
  HIP_CHECK(hipGetLastError());
}

static int grid_for(uint64_t work_items) {
  // >> 256 workgroups to fill 8 XCDs; cap for grid-stride loops
  uint64_t g = (work_items + WG - 1) / WG;
  if (g > 8192) g = 8192;
  if (g < 1) g = 1;
  return (int)g;
}

static void arena_fill(int h, uint64_t off, uint64_t n, int value) {
  Arena* a = get_arena(h);
  check_range(a, off, n);
  py::gil_scoped_release rel;
  if (!a->is_dev()) {
    std::memset((uint8_t*)a->base + off, value, n);
    return;
  }
  std::lock_guard<std::mutex> g(a->mu);
  HIP_CHECK(hipSetDevice(a->device));
  launch(fill_kernel, grid_for(n / 16 + 1), WG, a->kstream,
         (uint8_t*)a->base + off, (uint8_t)value, n);
  HIP_CHECK(hipStreamSynchronize(a->kstream));
}

// crc32c of n device bytes at an 8 B-aligned p (the kernel reads 8 B words);
// caller holds a->mu and has set the device
static uint32_t dev_crc32c_aligned(Arena* a, const uint8_t* p, uint64_t n) {
  uint64_t n_sub = n / CRC_SUB;
  uint64_t tail = n - n_sub * CRC_SUB;
  uint32_t result = 0;
  if (n_sub) {
    uint32_t n_wg = (uint32_t)((n_sub + WG - 1) / WG);
    Scratch sc(a, n_wg * sizeof(uint32_t) + a->pin_sz);
    uint32_t* d_out = sc.take<uint32_t>(n_wg);
    launch(crc32c_kernel, n_wg, WG, a->kstream, p, n_sub, d_out);
    std::vector<uint32_t> host_out(n_wg);
    HIP_CHECK(hipMemcpyAsync(host_out.data(), d_out, n_wg * sizeof(uint32_t),
                             hipMemcpyDeviceToHost, a->kstream));
    HIP_CHECK(hipStreamSynchronize(a->kstream));
    // combine per-workgroup crcs (each covers WG*CRC_SUB except the last)
    uint64_t remain = n_sub;
    result = host_out[0];
    uint64_t covered0 = std::min<uint64_t>(WG, remain);
    remain -= covered0;
    for (uint32_t w = 1; w < n_wg; ++w) {
      uint64_t cov = std::min<uint64_t>(WG, remain);
      remain -= cov;
      result = crc32c_combine(result, host_out[w], cov * CRC_SUB);
    }
  }
  if (tail) {
    // read the tail back through a pinned slot and crc on host
    uint8_t* pin0 = (uint8_t*)(a->pin.empty() ? nullptr : a->pin[0]);
    std::vector<uint8_t> tmp;
    uint8_t* dst;
    if (pin0 && tail <= a->pin_sz) dst = pin0;
    else { tmp.resize(tail); dst = tmp.data(); }
    HIP_CHECK(hipMemcpyAsync(dst, p + n_sub * CRC_SUB, tail,
                             hipMemcpyDeviceToHost, a->kstream));
    HIP_CHECK(hipStreamSynchronize(a->kstream));
    uint32_t tail_crc = crc32c_sw(dst, tail, 0);
    result = n_sub ? crc32c_combine(result, tail_crc, tail) : tail_crc;
  }
  return result;
}

static uint32_t arena_crc32c(int h, uint64_t off, uint64_t n) {
  Arena* a = get_arena(h);
  check_range(a, off, n);
  if (!a->is_dev()) {
    const uint8_t* p = (const uint8_t*)a->base + off;
    py::gil_scoped_release rel;
    return crc32c_sw(p, n, 0);
  }
  py::gil_scoped_release rel;
  std::lock_guard<std::mutex> g(a->mu);
  HIP_CHECK(hipSetDevice(a->device));
  ensure_crc_tables(a->device);
  const uint8_t* p = (const uint8_t*)a->base + off;
  // any byte offset: the up-to-7 bytes before the next 8 B boundary are
  // read back and checksummed here, the aligned rest goes to the kernel
  uint64_t head = std::min<uint64_t>((8 - ((uintptr_t)p & 7)) & 7, n);
  if (!head) return dev_crc32c_aligned(a, p, n);
  uint8_t hb[8];
  HIP_CHECK(hipMemcpyAsync(hb, p, head, hipMemcpyDeviceToHost, a->kstream));
  HIP_CHECK(hipStreamSynchronize(a->kstream));
  uint32_t head_crc = crc32c_sw(hb, head, 0);
  if (head == n) return head_crc;
  return crc32c_combine(head_crc, dev_crc32c_aligned(a, p + head, n - head),
                        n - head);
}

static uint32_t crc32c_buf(py::buffer buf, uint32_t init) {
  py::buffer_info info = buf.request(false);
  const uint8_t* p = (const uint8_t*)info.ptr;
  size_t n = (size_t)info.size * info.itemsize;
  py::gil_scoped_release rel;
  return crc32c_sw(p, n, init);
}

// ---- tile tables ----
//
// The tiled kernels (copy_extents_kernel, convert_segments_kernel) take an
// item table plus, per tile, the item it belongs to and its offset inside
// that item, so one grid is load-balanced whatever the items' sizes.

struct Tiles {
  std::vector<uint32_t> item;
  std::vector<uint64_t> off;
  bool empty() const { return item.empty(); }
  // scratch needed for `n_items` Items and up to `n_tiles` tiles
  template <class Item> static size_t room(size_t n_items, size_t n_tiles) {
    return Scratch::room<Item>(n_items) + Scratch::room<uint64_t>(n_tiles) +
           Scratch::room<uint32_t>(n_tiles);
  }
  template <class Item> size_t room(size_t n_items) const {
    return room<Item>(n_items, item.size());
  }
};

// item i, len(i) units long, is cut into tiles of step(i) units
template <class Len, class Step>
static Tiles build_tiles(size_t n_items, Len len, Step step, const char* who) {
  Tiles t;
  for (size_t i = 0; i < n_items; ++i)
    for (uint64_t o = 0, n = len(i), s = step(i); o < n; o += s) {
      t.item.push_back((uint32_t)i);
      t.off.push_back(o);
    }
  if (t.item.size() > 0xFFFFFFFFull)   // the kernels count tiles in uint32_t
    throw std::invalid_argument(std::string(who) +
                                ": too many tiles in one call");
  return t;
}

// most workgroups a tiled kernel (or scale_slots_kernel) is launched with;
// past it a workgroup strides over tiles blockIdx.x, + TILE_GRID_CAP, ...
static constexpr uint32_t TILE_GRID_CAP = 8192;

template <class Item> struct DevTiles {
  const Item* items;
  const uint32_t* tile_item;
  const uint64_t* tile_off;
  uint32_t n_tiles;
  unsigned grid() const { return std::min<uint32_t>(n_tiles, TILE_GRID_CAP); }
};

// carve the three tables (8-byte fields first) and upload them on `s`
template <class Item>
static DevTiles<Item> upload_tiles(hipStream_t s, Scratch& sc,
                                   const std::vector<Item>& items,
                                   const Tiles& t) {
  Item* d_items = sc.take<Item>(items.size());
  uint64_t* d_off = sc.take<uint64_t>(t.off.size());
  uint32_t* d_item = sc.take<uint32_t>(t.item.size());
  HIP_CHECK(hipMemcpyAsync(d_items, items.data(), items.size() * sizeof(Item),
                           hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(d_off, t.off.data(), t.off.size() * sizeof(uint64_t),
                           hipMemcpyHostToDevice, s));
  HIP_CHECK(hipMemcpyAsync(d_item, t.item.data(),
                           t.item.size() * sizeof(uint32_t),
                           hipMemcpyHostToDevice, s));
  return {d_items, d_item, d_off, (uint32_t)t.item.size()};
}

// the arena's own scratch and kstream
template <class Item>
static DevTiles<Item> upload_tiles(Arena* a, Scratch& sc,
                                   const std::vector<Item>& items,
                                   const Tiles& t) {
  return upload_tiles(a->kstream, sc, items, t);
}

static Tiles extent_tiles(const std::vector<Extent>& exts, const char* who) {
  return build_tiles(exts.size(), [&](size_t i) { return exts[i].len; },
                     [](size_t) { return (uint64_t)TILE; }, who);
}

// copy exts[i] = (src_off, dst_off, len) from src_base to dst_base on
// kstream; `tiles` is extent_tiles(exts) and not empty, `sc` has
// tiles.room<Extent>() left.  The caller syncs.
static void launch_copy_extents(Arena* a, Scratch& sc, const uint8_t* src_base,
                                uint8_t* dst_base,
                                const std::vector<Extent>& exts,
                                const Tiles& tiles) {
  DevTiles<Extent> d = upload_tiles(a, sc, exts, tiles);
  launch(copy_extents_kernel, d.grid(), WG, a->kstream, src_base, dst_base,
         d.items, d.tile_item, d.tile_off, d.n_tiles);
}

// gather device extents into a host buffer: kernel packs extents into
// contiguous scratch on-device, then one pipelined D2H.
static void arena_gather(int h, std::vector<std::pair<uint64_t, uint64_t>> ext,
                         py::buffer out, uint64_t out_off) {
  Arena* a = get_arena(h);
  py::buffer_info info = out.request(true);
  uint64_t total = 0;
  for (auto& e : ext) { check_range(a, e.first, e.second); total += e.second; }
  if (out_off + total > (uint64_t)info.size * info.itemsize)
    throw std::runtime_error("gather dst too small");
  uint8_t* dst = (uint8_t*)info.ptr + out_off;
  py::gil_scoped_release rel;
  if (!a->is_dev()) {
    uint64_t o = 0;
    for (auto& e : ext) {
      std::memcpy(dst + o, (uint8_t*)a->base + e.first, e.second);
      o += e.second;
    }
    return;
  }
  std::lock_guard<std::mutex> g(a->mu);
  HIP_CHECK(hipSetDevice(a->device));
  std::vector<Extent> exts(ext.size());
  uint64_t o = 0;
  for (size_t i = 0; i < ext.size(); ++i) {
    exts[i] = {ext[i].first, o, ext[i].second};
    o += ext[i].second;
  }
  Tiles tiles = extent_tiles(exts, "gather");
  if (tiles.empty()) return;   // nothing to copy: no grid-0 launch
  // the packed region sits at the scratch base, tables behind it
  Scratch sc(a, Scratch::room<uint8_t>(total) + tiles.room<Extent>(exts.size()));
  uint8_t* d_pack = sc.take<uint8_t>(total);
  launch_copy_extents(a, sc, (const uint8_t*)a->base, d_pack, exts, tiles);
  HIP_CHECK(hipStreamSynchronize(a->kstream));
  // pipelined D2H of the packed region
  size_t nb = a->pin.size();
  uint64_t nchunks = (total + a->pin_sz - 1) / a->pin_sz;
  for (uint64_t c = 0; c < nchunks; ++c) {
    uint64_t coff = c * a->pin_sz;
    uint64_t clen = std::min<uint64_t>(a->pin_sz, total - coff);
    size_t slot = c % nb;
    if (c >= nb) HIP_CHECK(hipEventSynchronize(a->ev[slot]));
    HIP_CHECK(hipMemcpyAsync(a->pin[slot], d_pack + coff, clen,
                             hipMemcpyDeviceToHost, a->stream));
    HIP_CHECK(hipEventRecord(a->ev[slot], a->stream));
    if (c + 1 == nchunks || ((c + 1) % nb) == 0) {
      uint64_t first = (c / nb) * nb;
      for (uint64_t d2 = first; d2 <= c; ++d2) {
        size_t ds = d2 % nb;
        HIP_CHECK(hipEventSynchronize(a->ev[ds]));
        uint64_t doff = d2 * a->pin_sz;
        std::memcpy(dst + doff, a->pin[ds],
                    std::min<uint64_t>(a->pin_sz, total - doff));
      }
    }
  }
}

// gather arena extents into a caller-supplied pointer with per-extent dst
// offsets.  Device arena + device dst = pure on-chip D2D via
// copy_extents_kernel (no host hop — the training-ingest fast path: tar
// sample payloads living in the HBM cache land directly in a torch
// device tensor).  Host arena = plain memcpy scatter into a host dst.
static void arena_gather_ptr(
    int h, std::vector<std::tuple<uint64_t, uint64_t, uint64_t>> ext,
    uintptr_t dst_ptr) {
  Arena* a = get_arena(h);
  for (auto& e : ext) check_range(a, std::get<0>(e), std::get<2>(e));
  uint8_t* dst = (uint8_t*)dst_ptr;
  py::gil_scoped_release rel;
  if (!a->is_dev()) {
    for (auto& e : ext)
      std::memcpy(dst + std::get<1>(e), (uint8_t*)a->base + std::get<0>(e),
                  std::get<2>(e));
    return;
  }
  std::lock_guard<std::mutex> g(a->mu);
  HIP_CHECK(hipSetDevice(a->device));
  std::vector<Extent> exts(ext.size());
  for (size_t i = 0; i < ext.size(); ++i)
    exts[i] = {std::get<0>(ext[i]), std::get<1>(ext[i]), std::get<2>(ext[i])};
  Tiles tiles = extent_tiles(exts, "gather");
  if (tiles.empty()) return;   // nothing to copy: no grid-0 launch
  Scratch sc(a, tiles.room<Extent>(exts.size()));
  launch_copy_extents(a, sc, (const uint8_t*)a->base, dst, exts, tiles);
  HIP_CHECK(hipStreamSynchronize(a->kstream));
}

// typed tensor load, store and scales over tensor_cast.hip, mx_cast.hip and
// block_cast.hip, and check_device_range (needs the plumbing above)
#include "typed_io.cpp"

// ---- token windows (token_gather.hip) ----
//
// Pieces: (src_off, row, j0, n): n source tokens at arena byte src_off are
// tokens j0 .. j0+n-1 of window `row` of `batch` windows of seq_len + 1
// tokens; token j lands at x[row*seq_len + j] (j < seq_len) and at
// y[row*seq_len + j - 1] (j >= 1), widened src_dtype -> dst_dtype.  Returns
// the tokens read that lie outside [0, vocab_size) (0 when vocab_size is 0).
// Every argument error is raised here, on the host, before anything runs.
typedef std::tuple<uint64_t, uint64_t, uint64_t, uint64_t> TokenPieceTuple;

static uint64_t arena_token_windows(int h, std::vector<TokenPieceTuple> pieces_in,
                                    uintptr_t x_ptr, uintptr_t y_ptr,
                                    uint64_t batch, uint64_t seq_len,
                                    uint64_t sdt, uint64_t ddt,
                                    uint64_t vocab) {
  Arena* a = get_arena(h);
  if (sdt >= DT_COUNT || ddt >= DT_COUNT)
    throw std::invalid_argument("token windows: unknown dtype code");
  if (!token_pair_supported((uint32_t)sdt, (uint32_t)ddt))
    throw std::invalid_argument("token windows: unsupported dtype pair");
  if (batch == 0 || seq_len == 0)
    throw std::invalid_argument("token windows: batch and seq_len must be positive");
  uint64_t ss = cast_itemsize((uint32_t)sdt), ds = cast_itemsize((uint32_t)ddt);
  uint64_t win, n_el, dst_b, x_end, y_end;
  if (__builtin_add_overflow(seq_len, (uint64_t)1, &win) ||
      __builtin_mul_overflow(batch, seq_len, &n_el) ||
      __builtin_mul_overflow(n_el, ds, &dst_b) ||
      __builtin_add_overflow((uint64_t)x_ptr, dst_b, &x_end) ||
      __builtin_add_overflow((uint64_t)y_ptr, dst_b, &y_end))
    throw std::invalid_argument("token windows: destination size overflows");
  if (x_ptr == 0 || x_ptr % ds)
    throw std::invalid_argument("token windows: x_ptr null or misaligned");
  if (y_ptr == 0 || y_ptr % ds)
    throw std::invalid_argument("token windows: y_ptr null or misaligned");
  std::vector<TokenPiece> pieces;
  pieces.reserve(pieces_in.size());
  for (auto& t : pieces_in) {
    TokenPiece g{std::get<0>(t), std::get<1>(t), std::get<2>(t), std::get<3>(t)};
    uint64_t last, src_b, end;
    if (g.n == 0)
      throw std::invalid_argument("token windows: piece without tokens");
    if (g.row >= batch)
      throw std::invalid_argument("token windows: piece row outside the batch");
    if (__builtin_add_overflow(g.j0, g.n, &last) ||
        __builtin_mul_overflow(g.n, ss, &src_b) ||
        __builtin_add_overflow(g.src_off, src_b, &end))
      throw std::invalid_argument("token windows: piece range overflows");
    if (last > win)
      throw std::invalid_argument("token windows: piece runs past its window");
    if (end > a->cap)
      throw std::invalid_argument("token windows: arena range out of bounds");
    pieces.push_back(g);
  }
  py::gil_scoped_release rel;
  uint8_t* x = (uint8_t*)x_ptr;
  uint8_t* y = (uint8_t*)y_ptr;
  if (!a->is_dev()) {
    // a host arena scatters with the CPU: device memory is the wrong side
    for (uintptr_t p : {x_ptr, y_ptr}) {
      hipPointerAttribute_t at;
      if (hipPointerGetAttributes(&at, (const void*)p) != hipSuccess) {
        (void)hipGetLastError();   // plain host memory, or no runtime
        continue;
      }
      if (at.type == hipMemoryTypeDevice)
        throw std::invalid_argument(
            "token windows: device destination on a host arena");
    }
    uint64_t bad = 0;
    for (auto& g : pieces)
      bad += token_windows_host((const uint8_t*)a->base, g, x, y, seq_len,
                                (uint32_t)sdt, (uint32_t)ddt, vocab);
    return bad;
  }
  Tiles tiles = build_tiles(
      pieces.size(), [&](size_t i) { return pieces[i].n; },
      [](size_t) { return (uint64_t)TOKEN_TILE; }, "token windows");
  std::lock_guard<std::mutex> g(a->mu);
  HIP_CHECK(hipSetDevice(a->device));
  std::vector<std::pair<uint64_t, uint64_t>> known;
  check_device_range(a->device, x_ptr, x_end, "token windows", "x_ptr",
                     "destination", known);
  check_device_range(a->device, y_ptr, y_end, "token windows", "y_ptr",
                     "destination", known);
  if (tiles.empty()) return 0;   // nothing to gather: no grid-0 launch
  Scratch sc(a, Scratch::room<unsigned long long>(1) +
                    tiles.room<TokenPiece>(pieces.size()));
  unsigned long long* d_count = sc.take<unsigned long long>(1);
  if (vocab) HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(*d_count), a->kstream));
  DevTiles<TokenPiece> d = upload_tiles(a, sc, pieces, tiles);
  launch(token_windows_kernel, d.grid(), WG, a->kstream,
         (const uint8_t*)a->base, d.items, d.tile_item, d.tile_off, d.n_tiles,
         x, y, seq_len, (uint32_t)sdt, (uint32_t)ddt, vocab, d_count);
  unsigned long long bad = 0;
  if (vocab)
    HIP_CHECK(hipMemcpyAsync(&bad, d_count, sizeof(bad), hipMemcpyDeviceToHost,
                             a->kstream));
  HIP_CHECK(hipStreamSynchronize(a->kstream));
  return bad;
}

// host widening of `n` packed tokens (the slow path of the token reader:
// file-tier spans and the token that straddles a block boundary go through
// the kernel's own scalar routine)
static py::bytes token_convert_host(py::buffer src, uint64_t sdt, uint64_t ddt,
                                    uint64_t n) {
  py::buffer_info bi = src.request();
  if (sdt >= DT_COUNT || ddt >= DT_COUNT)
    throw std::invalid_argument("token convert: unknown dtype code");
  if (!token_pair_supported((uint32_t)sdt, (uint32_t)ddt))
    throw std::invalid_argument("token convert: unsupported dtype pair");
  uint32_t ss = cast_itemsize((uint32_t)sdt), ds = cast_itemsize((uint32_t)ddt);
  uint64_t src_b, out_b;
  if (__builtin_mul_overflow(n, (uint64_t)ss, &src_b) ||
      __builtin_mul_overflow(n, (uint64_t)ds, &out_b) || out_b > (1ull << 40))
    throw std::invalid_argument("token convert: size overflows");
  if (src_b > (uint64_t)bi.size * bi.itemsize)
    throw std::invalid_argument("token convert: source shorter than n tokens");
  // 8-byte words: aligned for both destination itemsizes
  std::vector<uint64_t> out(out_b / 8 + 1);
  const uint8_t* s = (const uint8_t*)bi.ptr;
  uint8_t* d = (uint8_t*)out.data();
  for (uint64_t i = 0; i < n; ++i)
    token_store(d + i * ds, token_widen(token_load(s + i * ss, ss), (uint32_t)sdt),
                ds);
  return py::bytes((const char*)out.data(), out_b);
}

// ---- document structure of a token batch (token_docs.hip) ----
//
// x is a dense [rows, seq_len] array of I32 / I64 at x_ptr; pos_ptr and
// doc_ptr receive position_ids and doc_ids in x's dtype, cu_ptr the int32
// cu_seqlens (rows * seq_len + 1 entries of room, n_seqs + 1 written); each
// of the three may be 0, which skips that output.  Returns (n_seqs,
// max_seqlen).  device >= 0: summary, offsets and write kernels on the
// caller's thread stream, the chunk table in memory of this call, one D2H
// copy of the two result words; device == -1: the host loop.  Every
// argument error is raised before anything runs.
static std::pair<uint64_t, uint64_t> token_docs(
    int device, uintptr_t x_ptr, uint64_t rows, uint64_t seq_len, uint64_t dt,
    int64_t eos_id, uintptr_t pos_ptr, uintptr_t doc_ptr, uintptr_t cu_ptr) {
  if (device < -1) throw std::invalid_argument("token docs: bad device");
  if (dt >= DT_COUNT)
    throw std::invalid_argument("token docs: unknown dtype code");
  if (dt != DT_I32 && dt != DT_I64)
    throw std::invalid_argument("token docs: dtype is not I32 / I64");
  if (rows == 0 || seq_len == 0)
    throw std::invalid_argument("token docs: rows and seq_len must be positive");
  uint64_t ds = cast_itemsize((uint32_t)dt);
  uint64_t n_el, bytes, x_end, pos_end, doc_end, cu_b, cu_end, key_top;
  // positions and document indices fit the dtype; row keys fit 64 bits
  if ((dt == DT_I32 && seq_len > (uint64_t)INT32_MAX) ||
      __builtin_mul_overflow(rows, seq_len, &n_el) ||
      __builtin_add_overflow(n_el, rows, &key_top) ||
      __builtin_mul_overflow(n_el, ds, &bytes) ||
      __builtin_add_overflow((uint64_t)x_ptr, bytes, &x_end) ||
      __builtin_add_overflow((uint64_t)pos_ptr, bytes, &pos_end) ||
      __builtin_add_overflow((uint64_t)doc_ptr, bytes, &doc_end) ||
      __builtin_mul_overflow(n_el + 1, (uint64_t)4, &cu_b) ||
      __builtin_add_overflow((uint64_t)cu_ptr, cu_b, &cu_end))
    throw std::invalid_argument("token docs: size overflows");
  uint64_t cpr = (seq_len + TOKEN_DOC_CHUNK - 1) / TOKEN_DOC_CHUNK, n_chunks;
  if (__builtin_mul_overflow(rows, cpr, &n_chunks) ||
      n_chunks > (uint64_t)INT32_MAX)
    throw std::invalid_argument("token docs: size overflows");
  if (cu_ptr && n_el >= (1ull << 31))
    throw std::invalid_argument(
        "token docs: cu_seqlens needs rows * seq_len below 2^31");
  if (x_ptr == 0 || x_ptr % ds)
    throw std::invalid_argument("token docs: x_ptr null or misaligned");
  if (pos_ptr % ds)
    throw std::invalid_argument("token docs: pos_ptr misaligned");
  if (doc_ptr % ds)
    throw std::invalid_argument("token docs: doc_ptr misaligned");
  if (cu_ptr % 4)
    throw std::invalid_argument("token docs: cu_ptr misaligned");
  if (eos_id < 0 || (dt == DT_I32 && eos_id > (int64_t)INT32_MAX))
    throw std::invalid_argument(
        "token docs: eos_id negative or outside the dtype");
  uint64_t eos = (uint64_t)eos_id;
  const uint8_t* x = (const uint8_t*)x_ptr;
  uint8_t* pos = (uint8_t*)pos_ptr;
  uint8_t* doc = (uint8_t*)doc_ptr;
  int32_t* cu = (int32_t*)cu_ptr;
  py::gil_scoped_release rel;
  unsigned long long result[2] = {0, 0};
  if (device < 0) {
    // the host loop dereferences all four: device memory is the wrong side
    for (uintptr_t p : {x_ptr, pos_ptr, doc_ptr, cu_ptr}) {
      hipPointerAttribute_t at;
      if (!p) continue;
      if (hipPointerGetAttributes(&at, (const void*)p) != hipSuccess) {
        (void)hipGetLastError();   // plain host memory, or no runtime
        continue;
      }
      if (at.type == hipMemoryTypeDevice)
        throw std::invalid_argument(
            "token docs: device pointer with device -1");
    }
    uint64_t n_seqs, max_seqlen;
    token_docs_host(x, rows, seq_len, (uint32_t)ds, eos, pos, doc, cu, n_seqs,
                    max_seqlen);
    return {n_seqs, max_seqlen};
  }
  HIP_CHECK(hipSetDevice(device));
  std::vector<std::pair<uint64_t, uint64_t>> known;
  check_device_range(device, x_ptr, x_end, "token docs", "x_ptr", "source",
                     known);
  if (pos_ptr)
    check_device_range(device, pos_ptr, pos_end, "token docs", "pos_ptr",
                       "destination", known);
  if (doc_ptr)
    check_device_range(device, doc_ptr, doc_end, "token docs", "doc_ptr",
                       "destination", known);
  if (cu_ptr)
    check_device_range(device, cu_ptr, cu_end, "token docs", "cu_ptr",
                       "destination", known);
  hipStream_t s = thread_stream(device);
  CallScratch sc(Scratch::room<unsigned long long>(2) +
                 2 * Scratch::room<uint64_t>(n_chunks));
  unsigned long long* d_result = sc.take<unsigned long long>(2);
  uint64_t* d_counts = sc.take<uint64_t>(n_chunks);
  uint64_t* d_keys = sc.take<uint64_t>(n_chunks);
  HIP_CHECK(hipMemsetAsync(d_result, 0, sizeof(result), s));
  launch(token_doc_summary_kernel, (unsigned)n_chunks, WG, s, x, seq_len, cpr,
         (uint32_t)ds, eos, d_counts, d_keys);
  launch(token_doc_offsets_kernel, 1u, WG, s, d_counts, d_keys, n_chunks, rows,
         d_result);
  launch(token_doc_write_kernel, (unsigned)n_chunks, WG, s, x, rows, seq_len,
         cpr, (uint32_t)ds, eos, (const uint64_t*)d_counts,
         (const uint64_t*)d_keys, pos, doc, cu, d_result);
  HIP_CHECK(hipMemcpyAsync(result, d_result, sizeof(result),
                           hipMemcpyDeviceToHost, s));
  // the outputs are complete and the table freed once this returns
  HIP_CHECK(hipStreamSynchronize(s));
  return {result[0], result[1]};
}

// ---- document-packed token batches (token_pack.hip) ----

// a host arena works with the CPU: device memory is the wrong side
static void token_check_host_side(std::initializer_list<uintptr_t> ptrs,
                                  const char* msg) {
  for (uintptr_t p : ptrs) {
    hipPointerAttribute_t at;
    if (!p) continue;
    if (hipPointerGetAttributes(&at, (const void*)p) != hipSuccess) {
      (void)hipGetLastError();   // plain host memory, or no runtime
      continue;
    }
    if (at.type == hipMemoryTypeDevice) throw std::invalid_argument(msg);
  }
}

// eos_id as the widened value a token is compared with
static uint64_t token_eos_value(int64_t eos_id, uint64_t sdt, const char* who) {
  int64_t top = sdt == DT_U16 ? 0xFFFF
                : sdt == DT_U32 ? (int64_t)0xFFFFFFFFll : (int64_t)INT32_MAX;
  if (eos_id < 0 || eos_id > top)
    throw std::invalid_argument(std::string(who) +
                                ": eos_id negative or outside the dtype");
  return (uint64_t)eos_id;
}

// Spans: (src_off, tok0, n): n src_dtype tokens at arena byte src_off are
// tokens tok0 .. tok0+n-1 of a file, in ascending tok0 without overlap.  The
// file indices of the tokens equal to eos_id go to out_ptr (int64, room for
// `capacity`), ascending; hits past `capacity` are counted, not written.
// Returns the number of hits.  capacity 0 is a pure count (out_ptr may be 0).
// Device arena: count, offsets and (capacity > 0) write kernels on kstream
// and one D2H copy of the total; host arena: the host loop.  Every argument
// error is raised here, on the host, before anything runs.
typedef std::tuple<uint64_t, uint64_t, uint64_t> TokenSpanTuple;

static uint64_t arena_token_eos_index(int h, std::vector<TokenSpanTuple> spans_in,
                                      uint64_t sdt, int64_t eos_id,
                                      uintptr_t out_ptr, uint64_t capacity) {
  const char* who = "token eos index";
  Arena* a = get_arena(h);
  if (sdt >= DT_COUNT)
    throw std::invalid_argument("token eos index: unknown dtype code");
  if (!token_pair_supported((uint32_t)sdt, DT_I64))
    throw std::invalid_argument("token eos index: unsupported dtype");
  uint64_t eos = token_eos_value(eos_id, sdt, who);
  uint64_t ss = cast_itemsize((uint32_t)sdt), out_b, out_end;
  if (__builtin_mul_overflow(capacity, (uint64_t)8, &out_b) ||
      __builtin_add_overflow((uint64_t)out_ptr, out_b, &out_end))
    throw std::invalid_argument("token eos index: size overflows");
  if ((capacity && out_ptr == 0) || out_ptr % 8)
    throw std::invalid_argument("token eos index: out_ptr null or misaligned");
  std::vector<TokenSpan> spans;
  spans.reserve(spans_in.size());
  uint64_t next_tok = 0;
  for (auto& t : spans_in) {
    TokenSpan g{std::get<0>(t), std::get<1>(t), std::get<2>(t)};
    uint64_t last, src_b, end;
    if (g.n == 0)
      throw std::invalid_argument("token eos index: span without tokens");
    if (__builtin_add_overflow(g.tok0, g.n, &last) || last > (1ull << 62) ||
        __builtin_mul_overflow(g.n, ss, &src_b) ||
        __builtin_add_overflow(g.src_off, src_b, &end))
      throw std::invalid_argument("token eos index: size overflows");
    if (g.tok0 < next_tok)
      throw std::invalid_argument(
          "token eos index: spans not ascending, or overlapping");
    if (end > a->cap)
      throw std::invalid_argument("token eos index: arena range out of bounds");
    next_tok = last;
    spans.push_back(g);
  }
  py::gil_scoped_release rel;
  int64_t* out = (int64_t*)out_ptr;
  if (!a->is_dev()) {
    token_check_host_side({out_ptr},
                          "token eos index: device destination on a host arena");
    uint64_t total = 0;
    for (auto& g : spans)
      total = token_eos_host((const uint8_t*)a->base, g, (uint32_t)sdt, eos,
                             out, capacity, total);
    return total;
  }
  Tiles tiles = build_tiles(
      spans.size(), [&](size_t i) { return spans[i].n; },
      [](size_t) { return (uint64_t)TOKEN_EOS_TILE; }, who);
  std::lock_guard<std::mutex> g(a->mu);
  HIP_CHECK(hipSetDevice(a->device));
  std::vector<std::pair<uint64_t, uint64_t>> known;
  if (capacity)
    check_device_range(a->device, out_ptr, out_end, who, "out_ptr",
                       "destination", known);
  if (tiles.empty()) return 0;   // nothing to scan: no grid-0 launch
  size_t n_tiles = tiles.item.size();
  Scratch sc(a, Scratch::room<unsigned long long>(1) +
                    Scratch::room<uint64_t>(n_tiles) +
                    tiles.room<TokenSpan>(spans.size()));
  unsigned long long* d_total = sc.take<unsigned long long>(1);
  uint64_t* d_counts = sc.take<uint64_t>(n_tiles);
  DevTiles<TokenSpan> d = upload_tiles(a, sc, spans, tiles);
  const uint8_t* base = (const uint8_t*)a->base;
  launch(token_eos_count_kernel, d.grid(), WG, a->kstream, base, d.items,
         d.tile_item, d.tile_off, d.n_tiles, (uint32_t)sdt, eos, d_counts);
  launch(token_eos_offsets_kernel, 1u, WG, a->kstream, d_counts,
         (uint64_t)n_tiles, d_total);
  if (capacity)
    launch(token_eos_write_kernel, d.grid(), WG, a->kstream, base, d.items,
           d.tile_item, d.tile_off, d.n_tiles, (uint32_t)sdt, eos,
           (const uint64_t*)d_counts, out, capacity);
  unsigned long long total = 0;
  HIP_CHECK(hipMemcpyAsync(&total, d_total, sizeof(total),
                           hipMemcpyDeviceToHost, a->kstream));
  HIP_CHECK(hipStreamSynchronize(a->kstream));
  return total;
}

// host scan of `n` packed tokens, tokens tok0 .. tok0+n-1 of a file (the
// slow path of the reader's eos index): the hits' file indices as int64
static py::bytes token_eos_index_host(py::buffer src, uint64_t sdt,
                                      int64_t eos_id, uint64_t tok0,
                                      uint64_t n) {
  py::buffer_info bi = src.request();
  if (sdt >= DT_COUNT)
    throw std::invalid_argument("token eos index: unknown dtype code");
  if (!token_pair_supported((uint32_t)sdt, DT_I64))
    throw std::invalid_argument("token eos index: unsupported dtype");
  uint64_t eos = token_eos_value(eos_id, sdt, "token eos index");
  uint64_t ss = cast_itemsize((uint32_t)sdt), src_b, last;
  if (__builtin_mul_overflow(n, ss, &src_b) ||
      __builtin_add_overflow(tok0, n, &last) || last > (1ull << 62))
    throw std::invalid_argument("token eos index: size overflows");
  if (src_b > (uint64_t)bi.size * bi.itemsize)
    throw std::invalid_argument(
        "token eos index: source shorter than n tokens");
  TokenSpan g{0, tok0, n};
  const uint8_t* s = (const uint8_t*)bi.ptr;
  uint64_t total = token_eos_host(s, g, (uint32_t)sdt, eos, nullptr, 0, 0);
  std::vector<int64_t> out(total + 1);
  token_eos_host(s, g, (uint32_t)sdt, eos, out.data(), total, 0);
  return py::bytes((const char*)out.data(), total * 8);
}

// sentinels of a packed batch have to be values of the destination dtype
static void token_check_fits(int64_t v, uint64_t ddt, const char* what) {
  if (ddt == DT_I32 && (v < (int64_t)INT32_MIN || v > (int64_t)INT32_MAX))
    throw std::invalid_argument(std::string("token pack: ") + what +
                                " does not fit the dtype");
}

// One segment (row, col, n, pos0, doc, seq, flags) and the checks every
// caller shares; flags: TOKEN_SEG_NEXT, or TOKEN_SEG_PAD alone
typedef std::tuple<uint64_t, uint64_t, uint64_t, uint64_t, uint64_t, uint64_t,
                   uint64_t> TokenSegTuple;

static TokenSeg token_seg_checked(const TokenSegTuple& t, uint64_t rows,
                                  uint64_t seq_len, uint64_t n_segs,
                                  uint64_t ddt) {
  TokenSeg s{std::get<0>(t), std::get<1>(t), std::get<2>(t), std::get<3>(t),
             (int64_t)std::get<4>(t), (uint32_t)std::get<5>(t),
             (uint32_t)std::get<6>(t)};
  uint64_t last, pos_top;
  uint64_t top = ddt == DT_I32 ? (uint64_t)INT32_MAX : (uint64_t)INT64_MAX;
  if (s.n == 0)
    throw std::invalid_argument("token pack: segment without columns");
  if (s.row >= rows)
    throw std::invalid_argument("token pack: segment row outside the batch");
  if (__builtin_add_overflow(s.col, s.n, &last) || last > seq_len)
    throw std::invalid_argument("token pack: segment runs past its row");
  if (std::get<5>(t) >= n_segs)
    throw std::invalid_argument("token pack: seq outside the segment list");
  if (std::get<6>(t) > TOKEN_SEG_PAD)
    throw std::invalid_argument("token pack: unknown segment flags");
  if (__builtin_add_overflow(s.pos0, s.n, &pos_top) || pos_top - 1 > top ||
      std::get<4>(t) > top)
    throw std::invalid_argument(
        "token pack: position or document id overflows the dtype");
  return s;
}

// Segments: (row, col, n, pos0, doc, seq, flags); pieces: (src_off, segment,
// j0, k): k source tokens at arena byte src_off are tokens j0 .. j0+k-1 of
// source segment `segment` (see token_pack.hip).  x, y, position_ids and
// doc_ids are dense [rows, seq_len] arrays of dst_dtype, cu_seqlens int32
// with n_segments + 1 entries; every pointer but x_ptr may be 0, which skips
// that output.  Pad segments are filled and cu_seqlens written whatever the
// pieces cover.  Returns the tokens read that lie outside [0, vocab_size) (0
// when vocab_size is 0).  Device arena: the tables are uploaded and
// token_pack_kernel launched once on kstream; host arena: the host loop.
// Every argument error is raised here, on the host, before anything runs.
static uint64_t arena_token_pack(int h, std::vector<TokenSegTuple> segs_in,
                                 std::vector<TokenPieceTuple> pieces_in,
                                 uintptr_t x_ptr, uintptr_t y_ptr,
                                 uintptr_t pos_ptr, uintptr_t doc_ptr,
                                 uintptr_t cu_ptr, uint64_t rows,
                                 uint64_t seq_len, uint64_t sdt, uint64_t ddt,
                                 int64_t pad_id, int64_t ignore_index,
                                 uint64_t vocab) {
  const char* who = "token pack";
  Arena* a = get_arena(h);
  if (sdt >= DT_COUNT || ddt >= DT_COUNT)
    throw std::invalid_argument("token pack: unknown dtype code");
  if (!token_pair_supported((uint32_t)sdt, (uint32_t)ddt))
    throw std::invalid_argument("token pack: unsupported dtype pair");
  if (rows == 0 || seq_len == 0)
    throw std::invalid_argument("token pack: rows and seq_len must be positive");
  uint64_t ss = cast_itemsize((uint32_t)sdt), ds = cast_itemsize((uint32_t)ddt);
  uint64_t n_segs = segs_in.size();
  uint64_t n_el, dst_b, x_end, y_end, pos_end, doc_end, cu_end;
  if (n_segs >= 0xFFFFFFFFull || pieces_in.size() >= 0xFFFFFFFFull ||
      __builtin_mul_overflow(rows, seq_len, &n_el) ||
      __builtin_mul_overflow(n_el, ds, &dst_b) ||
      __builtin_add_overflow((uint64_t)x_ptr, dst_b, &x_end) ||
      __builtin_add_overflow((uint64_t)y_ptr, dst_b, &y_end) ||
      __builtin_add_overflow((uint64_t)pos_ptr, dst_b, &pos_end) ||
      __builtin_add_overflow((uint64_t)doc_ptr, dst_b, &doc_end) ||
      __builtin_add_overflow((uint64_t)cu_ptr, (n_segs + 1) * 4, &cu_end))
    throw std::invalid_argument("token pack: size overflows");
  if (cu_ptr && n_el >= (1ull << 31))
    throw std::invalid_argument(
        "token pack: cu_seqlens needs rows * seq_len below 2^31");
  if (x_ptr == 0 || x_ptr % ds)
    throw std::invalid_argument("token pack: x_ptr null or misaligned");
  if (y_ptr % ds) throw std::invalid_argument("token pack: y_ptr misaligned");
  if (pos_ptr % ds)
    throw std::invalid_argument("token pack: pos_ptr misaligned");
  if (doc_ptr % ds)
    throw std::invalid_argument("token pack: doc_ptr misaligned");
  if (cu_ptr % 4) throw std::invalid_argument("token pack: cu_ptr misaligned");
  token_check_fits(pad_id, ddt, "pad_id");
  token_check_fits(ignore_index, ddt, "ignore_index");
  std::vector<TokenSeg> segs;
  segs.reserve(n_segs);
  for (auto& t : segs_in)
    segs.push_back(token_seg_checked(t, rows, seq_len, n_segs, ddt));
  // the items of the launch: the source pieces, then the pad segments
  std::vector<TokenPackPiece> items;
  items.reserve(pieces_in.size());
  for (auto& t : pieces_in) {
    TokenPackPiece g{std::get<0>(t), std::get<1>(t), std::get<2>(t),
                     std::get<3>(t)};
    uint64_t last, src_b, end;
    if (g.seg >= n_segs)
      throw std::invalid_argument("token pack: piece of an unknown segment");
    const TokenSeg& s = segs[g.seg];
    if (s.flags & TOKEN_SEG_PAD)
      throw std::invalid_argument("token pack: piece on a pad segment");
    if (g.k == 0)
      throw std::invalid_argument("token pack: piece without tokens");
    if (__builtin_add_overflow(g.j0, g.k, &last) ||
        __builtin_mul_overflow(g.k, ss, &src_b) ||
        __builtin_add_overflow(g.src_off, src_b, &end))
      throw std::invalid_argument("token pack: size overflows");
    if (last > s.n + (s.flags & TOKEN_SEG_NEXT))
      throw std::invalid_argument("token pack: piece runs past its segment");
    if (end > a->cap)
      throw std::invalid_argument("token pack: arena range out of bounds");
    items.push_back(g);
  }
  for (size_t i = 0; i < segs.size(); ++i)
    if (segs[i].flags & TOKEN_SEG_PAD)
      items.push_back(TokenPackPiece{0, (uint64_t)i, 0, segs[i].n});
  py::gil_scoped_release rel;
  TokenPackOut out{(uint8_t*)x_ptr, (uint8_t*)y_ptr, (uint8_t*)pos_ptr,
                   (uint8_t*)doc_ptr};
  int32_t* cu = (int32_t*)cu_ptr;
  if (!a->is_dev()) {
    token_check_host_side({x_ptr, y_ptr, pos_ptr, doc_ptr, cu_ptr},
                          "token pack: device destination on a host arena");
    return token_pack_host((const uint8_t*)a->base, segs, items, out, cu, rows,
                           seq_len, (uint32_t)sdt, (uint32_t)ddt, pad_id,
                           ignore_index, vocab);
  }
  Tiles tiles = build_tiles(
      items.size(), [&](size_t i) { return items[i].k; },
      [](size_t) { return (uint64_t)TOKEN_PACK_TILE; }, who);
  std::lock_guard<std::mutex> g(a->mu);
  HIP_CHECK(hipSetDevice(a->device));
  std::vector<std::pair<uint64_t, uint64_t>> known;
  check_device_range(a->device, x_ptr, x_end, who, "x_ptr", "destination",
                     known);
  if (y_ptr)
    check_device_range(a->device, y_ptr, y_end, who, "y_ptr", "destination",
                       known);
  if (pos_ptr)
    check_device_range(a->device, pos_ptr, pos_end, who, "pos_ptr",
                       "destination", known);
  if (doc_ptr)
    check_device_range(a->device, doc_ptr, doc_end, who, "doc_ptr",
                       "destination", known);
  if (cu_ptr)
    check_device_range(a->device, cu_ptr, cu_end, who, "cu_ptr", "destination",
                       known);
  if (tiles.empty() && !cu) return 0;   // nothing to write: no launch
  Scratch sc(a, Scratch::room<unsigned long long>(1) +
                    Scratch::room<TokenSeg>(segs.size()) +
                    tiles.room<TokenPackPiece>(items.size()));
  unsigned long long* d_count = sc.take<unsigned long long>(1);
  TokenSeg* d_segs = sc.take<TokenSeg>(segs.size());
  if (vocab) HIP_CHECK(hipMemsetAsync(d_count, 0, sizeof(*d_count), a->kstream));
  if (!segs.empty())
    HIP_CHECK(hipMemcpyAsync(d_segs, segs.data(), segs.size() * sizeof(TokenSeg),
                             hipMemcpyHostToDevice, a->kstream));
  DevTiles<TokenPackPiece> d{nullptr, nullptr, nullptr, 0};
  if (!tiles.empty()) d = upload_tiles(a, sc, items, tiles);
  launch(token_pack_kernel, std::max(d.grid(), 1u), WG, a->kstream,
         (const uint8_t*)a->base, (const TokenSeg*)d_segs, (uint32_t)n_segs,
         d.items, d.tile_item, d.tile_off, d.n_tiles, out, cu, rows, seq_len,
         (uint32_t)sdt, (uint32_t)ddt, pad_id, ignore_index, vocab, d_count);
  unsigned long long bad = 0;
  if (vocab)
    HIP_CHECK(hipMemcpyAsync(&bad, d_count, sizeof(bad), hipMemcpyDeviceToHost,
                             a->kstream));
  // the tables are host vectors of this call: wait before they go
  HIP_CHECK(hipStreamSynchronize(a->kstream));
  return bad;
}

// One piece on the host (the slow path of the reader's packed batches: file
// tier, cross-side arenas, holes and the token a block boundary cuts), with
// the pack kernel's own scalar routines.  `src` holds tokens j0 .. j0+k-1 of
// a source segment (n, pos0, doc, flags); a pad segment has no source and
// is done whole (j0 = 0, k = n).  Returns (x, y, pos, doc, bad) as bytes of
// dst_dtype: x / pos / doc for the segment's columns j0 .. min(j0+k, n)-1,
// y for its columns max(j0, 1)-1 onwards (pad: all n), ignore_index at
// column n-1 included when the document ends inside the piece.
static py::tuple token_pack_piece_host(py::buffer src, uint64_t n,
                                       uint64_t pos0, uint64_t doc,
                                       uint64_t flags, uint64_t j0, uint64_t k,
                                       uint64_t sdt, uint64_t ddt,
                                       int64_t pad_id, int64_t ignore_index,
                                       uint64_t vocab) {
  py::buffer_info bi = src.request();
  if (sdt >= DT_COUNT || ddt >= DT_COUNT)
    throw std::invalid_argument("token pack: unknown dtype code");
  if (!token_pair_supported((uint32_t)sdt, (uint32_t)ddt))
    throw std::invalid_argument("token pack: unsupported dtype pair");
  token_check_fits(pad_id, ddt, "pad_id");
  token_check_fits(ignore_index, ddt, "ignore_index");
  // the segment alone in a row of its own
  TokenSeg s = token_seg_checked(
      TokenSegTuple{0, 0, n, pos0, doc, 0, flags}, 1, n, 1, ddt);
  bool is_pad = s.flags & TOKEN_SEG_PAD;
  uint32_t ss = cast_itemsize((uint32_t)sdt), ds = cast_itemsize((uint32_t)ddt);
  uint64_t last, src_b;
  if (k == 0) throw std::invalid_argument("token pack: piece without tokens");
  if (__builtin_add_overflow(j0, k, &last) ||
      __builtin_mul_overflow(k, (uint64_t)ss, &src_b) || k > (1ull << 36))
    throw std::invalid_argument("token pack: size overflows");
  if (is_pad ? (j0 != 0 || k != n) : last > s.n + (s.flags & TOKEN_SEG_NEXT))
    throw std::invalid_argument("token pack: piece runs past its segment");
  if (!is_pad && src_b > (uint64_t)bi.size * bi.itemsize)
    throw std::invalid_argument("token pack: source shorter than k tokens");
  // the columns from c on as a segment of their own: token j becomes j - c,
  // and a piece that begins past token 0 keeps j - c >= 1 (it still goes to
  // y).  k + 1 elements of 8-byte words, aligned for both itemsizes.
  uint64_t c = !is_pad && j0 >= 1 ? j0 - 1 : 0;
  s.n -= c;
  s.pos0 += c;
  j0 -= c;
  last -= c;
  size_t words = (size_t)((k + 1) * ds / 8 + 1);
  std::vector<uint64_t> bx(words), by(words), bp(words), bd(words);
  TokenPackOut o{(uint8_t*)bx.data(), (uint8_t*)by.data(), (uint8_t*)bp.data(),
                 (uint8_t*)bd.data()};
  uint64_t bad = 0, x1 = std::min(last, s.n), y1 = last;
  if (is_pad) {
    for (uint64_t i = 0; i < k; ++i)
      token_pack_pad_one(o, i, pad_id, ignore_index, ds);
  } else {
    const uint8_t* p = (const uint8_t*)bi.ptr;
    for (uint64_t i = 0; i < k; ++i)
      bad += token_pack_one(p + i * ss, o, s, j0 + i, (uint32_t)sdt, ss, ds,
                            vocab);
    y1 = last - 1;
    if (!(s.flags & TOKEN_SEG_NEXT) && last == s.n) {
      token_pack_end(o, s, ignore_index, ds);
      y1 = s.n;
    }
  }
  auto cut = [&](const uint8_t* b, uint64_t c0, uint64_t c1) {
    return py::bytes((const char*)b + c0 * ds, c1 > c0 ? (c1 - c0) * ds : 0);
  };
  return py::make_tuple(cut(o.x, j0, x1), cut(o.y, 0, y1), cut(o.pos, j0, x1),
                        cut(o.doc, j0, x1), bad);
}

static uintptr_t arena_base_ptr(int h) {
  return (uintptr_t)get_arena(h)->base;
}

// ---- array samples (array_gather.hip) ----
//
// Pieces: (src_off, row, e0, n): n source bytes at arena byte src_off are
// bytes e0 .. e0+n-1 of sample `row` of `batch` samples of H*W*C uint8, HWC
// order.  rows[b] = (dy, dx, flip) places the hc x wc crop of sample b; the
// element of output row r, column q, channel c is source pixel (dy + r,
// dx + (flip ? wc-1-q : q)) times scale[c] plus bias[c], as dst_dt, in a
// dense NCHW (layout 0) or NHWC (layout 1) array at out_ptr.  Every argument
// error is raised here, on the host, before anything runs.
typedef std::tuple<uint64_t, uint64_t, uint64_t, uint64_t> ArrayPieceTuple;
typedef std::tuple<uint64_t, uint64_t, uint64_t> ArrayRowTuple;
typedef std::tuple<uint64_t, uint64_t, uint64_t> ArrayDims;
typedef std::tuple<uint64_t, uint64_t> ArrayCrop;

// shape, crop, normalisation, dtype and layout of a call; returns the bytes
// of one sample, sets `out_el` to the elements of one sample's output
static uint64_t array_check_shape(const char* who_is, ArrayDims shape,
                                  ArrayCrop crop,
                                  const std::vector<double>& scale,
                                  const std::vector<double>& bias,
                                  uint64_t ddt, uint64_t layout,
                                  ArrayShape& p, uint64_t& out_el) {
  const std::string who = who_is;
  if (ddt >= DT_COUNT)
    throw std::invalid_argument(who + ": unknown dtype code");
  if (!array_dst_supported((uint32_t)ddt))
    throw std::invalid_argument(who + ": unsupported destination dtype");
  if (layout != ARRAY_NCHW && layout != ARRAY_NHWC)
    throw std::invalid_argument(who + ": unknown layout");
  uint64_t H = std::get<0>(shape), W = std::get<1>(shape),
           C = std::get<2>(shape);
  uint64_t hc = std::get<0>(crop), wc = std::get<1>(crop);
  if (C < 1 || C > 4)
    throw std::invalid_argument(who + ": channels outside 1..4");
  if (H == 0 || W == 0 || hc == 0 || wc == 0)
    throw std::invalid_argument(who + ": zero dimension");
  if (hc > H || wc > W)
    throw std::invalid_argument(who + ": crop larger than the source");
  uint64_t sb;
  if (__builtin_mul_overflow(H, W, &sb) || __builtin_mul_overflow(sb, C, &sb) ||
      sb >= (1ull << 31))
    throw std::invalid_argument(who + ": sample size overflows");
  if (scale.size() != C || bias.size() != C)
    throw std::invalid_argument(who + ": scale and bias need one entry per channel");
  p = ArrayShape{(uint32_t)H, (uint32_t)W, (uint32_t)C, (uint32_t)hc,
                 (uint32_t)wc, (uint32_t)layout, {0, 0, 0, 0}, {0, 0, 0, 0}};
  for (uint64_t c = 0; c < C; ++c) {
    // finite as f32 too: checked before the narrowing
    if (!(std::fabs(scale[c]) <= FLT_MAX) || !(std::fabs(bias[c]) <= FLT_MAX))
      throw std::invalid_argument(who + ": scale or bias is not finite");
    p.scale[c] = (float)scale[c];
    p.bias[c] = (float)bias[c];
  }
  out_el = hc * wc * C;                          // <= sb
  return sb;
}

static ArrayRow array_check_row(const char* who_is, const ArrayRowTuple& t,
                                const ArrayShape& p) {
  const std::string who = who_is;
  uint64_t dy = std::get<0>(t), dx = std::get<1>(t), flip = std::get<2>(t);
  if (dy > p.H - p.h || dx > p.W - p.w)
    throw std::invalid_argument(who + ": crop runs past the sample");
  if (flip > 1)
    throw std::invalid_argument(who + ": flip is not 0 or 1");
  return ArrayRow{(uint32_t)dy, (uint32_t)dx, (uint32_t)flip};
}

static void arena_array_samples(int h, std::vector<ArrayPieceTuple> pieces_in,
                                std::vector<ArrayRowTuple> rows_in,
                                uintptr_t out_ptr, uint64_t batch,
                                ArrayDims shape, ArrayCrop crop,
                                std::vector<double> scale,
                                std::vector<double> bias, uint64_t ddt,
                                uint64_t layout) {
  const char* who = "array samples";
  Arena* a = get_arena(h);
  ArrayShape p;
  uint64_t out_el;
  uint64_t sb = array_check_shape(who, shape, crop, scale, bias, ddt, layout,
                                  p, out_el);
  if (batch == 0)
    throw std::invalid_argument("array samples: batch must be positive");
  if (rows_in.size() != batch)
    throw std::invalid_argument("array samples: one (dy, dx, flip) per sample");
  uint64_t ds = cast_itemsize((uint32_t)ddt), n_el, dst_b, out_end;
  if (__builtin_mul_overflow(batch, out_el, &n_el) ||
      __builtin_mul_overflow(n_el, ds, &dst_b) ||
      __builtin_add_overflow((uint64_t)out_ptr, dst_b, &out_end))
    throw std::invalid_argument("array samples: destination size overflows");
  if (out_ptr == 0 || out_ptr % ds)
    throw std::invalid_argument("array samples: out_ptr null or misaligned");
  std::vector<ArrayRow> rows;
  rows.reserve(rows_in.size());
  for (auto& t : rows_in) rows.push_back(array_check_row(who, t, p));
  std::vector<ArrayPiece> pieces;
  pieces.reserve(pieces_in.size());
  for (auto& t : pieces_in) {
    ArrayPiece g{std::get<0>(t), std::get<1>(t), std::get<2>(t), std::get<3>(t)};
    uint64_t last, end;
    if (g.n == 0)
      throw std::invalid_argument("array samples: piece without bytes");
    if (g.row >= batch)
      throw std::invalid_argument("array samples: piece row outside the batch");
    if (__builtin_add_overflow(g.e0, g.n, &last) ||
        __builtin_add_overflow(g.src_off, g.n, &end))
      throw std::invalid_argument("array samples: piece range overflows");
    if (last > sb)
      throw std::invalid_argument("array samples: piece runs past its sample");
    if (end > a->cap)
      throw std::invalid_argument("array samples: arena range out of bounds");
    pieces.push_back(g);
  }
  py::gil_scoped_release rel;
  uint8_t* out = (uint8_t*)out_ptr;
  if (!a->is_dev()) {
    // a host arena scatters with the CPU: device memory is the wrong side
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, (const void*)out_ptr) != hipSuccess)
      (void)hipGetLastError();   // plain host memory, or no runtime
    else if (at.type == hipMemoryTypeDevice)
      throw std::invalid_argument(
          "array samples: device destination on a host arena");
    for (auto& g : pieces)
      array_samples_host((const uint8_t*)a->base, g, rows.data(), out, p,
                         (uint32_t)ddt);
    return;
  }
  Tiles tiles = build_tiles(
      pieces.size(), [&](size_t i) { return pieces[i].n; },
      [](size_t) { return (uint64_t)ARRAY_TILE; }, who);
  std::lock_guard<std::mutex> g(a->mu);
  HIP_CHECK(hipSetDevice(a->device));
  std::vector<std::pair<uint64_t, uint64_t>> known;
  check_device_range(a->device, out_ptr, out_end, who, "out_ptr",
                     "destination", known);
  if (tiles.empty()) return;   // nothing to gather: no grid-0 launch
  Scratch sc(a, Scratch::room<ArrayRow>(rows.size()) +
                    tiles.room<ArrayPiece>(pieces.size()));
  DevTiles<ArrayPiece> d = upload_tiles(a, sc, pieces, tiles);
  ArrayRow* d_rows = sc.take<ArrayRow>(rows.size());
  HIP_CHECK(hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(ArrayRow),
                           hipMemcpyHostToDevice, a->kstream));
  launch(array_samples_kernel, d.grid(), WG, a->kstream,
         (const uint8_t*)a->base, d.items, d.tile_item, d.tile_off, d.n_tiles,
         (const ArrayRow*)d_rows, out, p, (uint32_t)ddt);
  HIP_CHECK(hipStreamSynchronize(a->kstream));
}

// one whole sample on the host (the slow path of the array reader: samples
// with a part in the file tier, across sides or in a hole go through the
// kernel's own scalar routine): its dense hc*wc*C output as bytes
static py::bytes array_sample_host_py(py::buffer src, uint64_t dy, uint64_t dx,
                                      uint64_t flip, ArrayDims shape,
                                      ArrayCrop crop, std::vector<double> scale,
                                      std::vector<double> bias, uint64_t ddt,
                                      uint64_t layout) {
  const char* who = "array sample";
  py::buffer_info bi = src.request();
  ArrayShape p;
  uint64_t out_el;
  uint64_t sb = array_check_shape(who, shape, crop, scale, bias, ddt, layout,
                                  p, out_el);
  ArrayRow a = array_check_row(who, ArrayRowTuple(dy, dx, flip), p);
  if (sb > (uint64_t)bi.size * bi.itemsize)
    throw std::invalid_argument("array sample: source shorter than the sample");
  uint64_t out_b = out_el * cast_itemsize((uint32_t)ddt);
  std::vector<uint32_t> out(out_b / 4 + 1);    // aligned for both itemsizes
  array_sample_host((const uint8_t*)bi.ptr, a, (uint8_t*)out.data(), p,
                    (uint32_t)ddt);
  return py::bytes((const char*)out.data(), out_b);
}

// batched small reads (the fio iodepth>1 analog): issue every copy async
// on the caller's thread-local stream, sync ONCE — amortizes launch+sync
// cost over the batch (4K random-read IOPS path)
static void arena_read_batch(int h, const std::vector<uint64_t>& offs,
                             const std::vector<uint64_t>& dsts, uint64_t n) {
  Arena* a = get_arena(h);
  if (offs.size() != dsts.size())
    throw std::runtime_error("arena_read_batch: offs/dsts mismatch");
  for (uint64_t off : offs) check_range(a, off, n);
  py::gil_scoped_release rel;
  if (!a->is_dev()) {
    for (size_t i = 0; i < offs.size(); ++i)
      std::memcpy((uint8_t*)dsts[i], (uint8_t*)a->base + offs[i], n);
    return;
  }
  HIP_CHECK(hipSetDevice(a->device));
  hipStream_t s = thread_stream(a->device);
  for (size_t i = 0; i < offs.size(); ++i)
    HIP_CHECK(hipMemcpyAsync((void*)dsts[i], (uint8_t*)a->base + offs[i], n,
                             hipMemcpyDeviceToHost, s));
  HIP_CHECK(hipStreamSynchronize(s));
}

// ---------------------------------------------------------------------------
// Registered readers: a file's arena extent table pinned in C++ so batched
// random preads resolve + issue + sync entirely GIL-free (the 4 KiB IOPS
// path; the client-side sibling of the native FUSE read registration).
// Safety contract (curvine_amd/client/reader.py): the SyncLocalReader
// holds its store readers open (block refcounts defer delete/demote) for
// the registration's whole lifetime and unregisters before closing them.
// ---------------------------------------------------------------------------

struct RdExt { uint64_t file_off, len; int arena; uint64_t arena_off; };
struct RdReader { uint64_t length; std::vector<RdExt> exts; };
static std::mutex g_rd_mu;
// shared_ptr: a read keeps its reader alive past the lock, whatever the map
// does meanwhile (rehash, a racing unregister)
static std::unordered_map<int64_t, std::shared_ptr<const RdReader>> g_rd;
static int64_t g_rd_next = 1;

static int64_t reader_register(
    std::vector<std::tuple<uint64_t, uint64_t, int, uint64_t>> exts,
    uint64_t length) {
  auto r = std::make_shared<RdReader>();
  r->length = length;
  r->exts.reserve(exts.size());
  uint64_t prev = 0;
  for (auto& e : exts) {
    if (std::get<0>(e) < prev)
      throw std::runtime_error("reader_register: extents must be sorted");
    prev = std::get<0>(e);
    get_arena(std::get<2>(e));   // validate handle
    r->exts.push_back({std::get<0>(e), std::get<1>(e), std::get<2>(e),
                       std::get<3>(e)});
  }
  std::lock_guard<std::mutex> g(g_rd_mu);
  int64_t rid = g_rd_next++;
  g_rd[rid] = std::move(r);
  return rid;
}

static void reader_unregister(int64_t rid) {
  std::lock_guard<std::mutex> g(g_rd_mu);
  g_rd.erase(rid);
}

static std::shared_ptr<const RdReader> rd_get(int64_t rid) {
  std::lock_guard<std::mutex> g(g_rd_mu);
  auto it = g_rd.find(rid);
  if (it == g_rd.end()) throw std::runtime_error("bad reader id");
  return it->second;
}

// the extent search shared by reader_pread_batch and reader_pread: the
// extent that holds file offset `off`, or nullptr when `off` lies in a hole
// or past the last extent
static const RdExt* rd_ext_at(const std::vector<RdExt>& exts, uint64_t off) {
  // binary search: last extent with file_off <= off
  size_t lo = 0, hi = exts.size();
  while (lo < hi) {
    size_t mid = (lo + hi) / 2;
    if (exts[mid].file_off <= off) lo = mid + 1; else hi = mid;
  }
  if (lo == 0) return nullptr;
  const RdExt* e = &exts[lo - 1];
  return off - e->file_off < e->len ? e : nullptr;
}

// devices whose thread streams carry copies of the current call: one
// hipStreamSynchronize each at the end
struct RdDevSet {
  int dev[8];
  int n = 0;
  void add(int d) {
    for (int i = 0; i < n; i++) if (dev[i] == d) return;
    if (n < 8) { dev[n++] = d; return; }
    // a ninth device: drain it now, the set stays exact
    HIP_CHECK(hipStreamSynchronize(thread_stream(d)));
  }
  void sync() {
    for (int i = 0; i < n; i++) {
      HIP_CHECK(hipSetDevice(dev[i]));
      HIP_CHECK(hipStreamSynchronize(thread_stream(dev[i])));
    }
  }
};

// one arena -> host piece: memcpy, or an async D2H on the thread stream
static void rd_issue(Arena* a, uint64_t aoff, uint8_t* dst, uint64_t n,
                     RdDevSet& devs) {
  const uint8_t* src = (const uint8_t*)a->base + aoff;
  if (!a->is_dev()) {
    std::memcpy(dst, src, n);
    return;
  }
  HIP_CHECK(hipSetDevice(a->device));
  HIP_CHECK(hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost,
                           thread_stream(a->device)));
  devs.add(a->device);
}

// fixed-size batched preads: for each file offset, land n bytes at
// dst_ptr + i*stride.  Returns the indices it could NOT serve (reads
// spanning extent boundaries or past EOF) so the caller falls back for
// exactly those.
static py::list reader_pread_batch(int64_t rid,
                                   const std::vector<uint64_t>& offs,
                                   uint64_t n, uintptr_t dst_ptr,
                                   uint64_t stride) {
  std::shared_ptr<const RdReader> r = rd_get(rid);
  std::vector<uint32_t> skipped;
  {
    py::gil_scoped_release rel;
    RdDevSet devs;
    for (size_t i = 0; i < offs.size(); ++i) {
      uint64_t off = offs[i];
      const RdExt* e = nullptr;
      if (off + n <= r->length) {
        e = rd_ext_at(r->exts, off);
        if (e && off - e->file_off + n > e->len) e = nullptr;
      }
      if (e == nullptr) {
        skipped.push_back((uint32_t)i);
        continue;
      }
      rd_issue(get_arena(e->arena), e->arena_off + (off - e->file_off),
               (uint8_t*)dst_ptr + i * stride, n, devs);
    }
    devs.sync();
  }
  py::list out;
  for (uint32_t i : skipped) out.append(i);
  return out;
}

// one ranged pread, GIL-free: [off, off+n) clamped to the reader's length
// lands at dst_ptr, one copy per extent the range covers (a read across a
// block boundary stays native) and one synchronise per device used.
// Returns the bytes served, or -1 with nothing issued when any part of the
// range is not covered by a registered extent (hole, sparse tail): the
// caller's Python loop serves those.
static int64_t reader_pread(int64_t rid, uint64_t off, uint64_t n,
                            uintptr_t dst_ptr) {
  std::shared_ptr<const RdReader> r = rd_get(rid);
  g_st_reader_pread.fetch_add(1, std::memory_order_relaxed);
  if (off >= r->length) return 0;
  n = std::min<uint64_t>(n, r->length - off);
  if (n == 0) return 0;
  py::gil_scoped_release rel;
  struct Piece { Arena* a; uint64_t aoff, n; };
  std::vector<Piece> pieces;
  pieces.reserve(2);
  // resolve and validate the whole range first: -1 must issue nothing
  for (uint64_t got = 0; got < n;) {
    const RdExt* e = rd_ext_at(r->exts, off + got);
    if (e == nullptr) return -1;
    uint64_t boff = off + got - e->file_off;
    uint64_t len = std::min<uint64_t>(n - got, e->len - boff);
    Arena* a = get_arena(e->arena);
    check_range(a, e->arena_off + boff, len);
    pieces.push_back({a, e->arena_off + boff, len});
    got += len;
  }
  RdDevSet devs;
  uint8_t* dst = (uint8_t*)dst_ptr;
  for (const Piece& p : pieces) {
    rd_issue(p.a, p.aoff, dst, p.n, devs);
    dst += p.n;
  }
  devs.sync();
  return (int64_t)n;
}

// ---------------------------------------------------------------------------
// LZ4 container: compress/decompress (host) + compress-from-arena and
// decompress-into-arena (GPU)
// ---------------------------------------------------------------------------

// CVLZ: magic u32 | raw size u64 | chunk size u32 | n_chunks u32 |
// sizes u32[n_chunks] | chunk payloads back to back
static uint32_t lz4_chunk_count(uint64_t n) {
  return (uint32_t)((n + LZ4_CHUNK - 1) / LZ4_CHUNK);
}
static size_t lz4_header_size(uint32_t n_chunks) { return 20 + 4ull * n_chunks; }

static void lz4_write_header(uint8_t* h, uint64_t raw,
                             const std::vector<uint32_t>& sizes) {
  uint32_t ck = LZ4_CHUNK, n_chunks = (uint32_t)sizes.size();
  memcpy(h, &LZ4_MAGIC, 4);
  memcpy(h + 4, &raw, 8);
  memcpy(h + 12, &ck, 4);
  memcpy(h + 16, &n_chunks, 4);
  memcpy(h + 20, sizes.data(), 4ull * n_chunks);
}

// host codec: compress src[0, n) chunk by chunk, appending the payloads to
// `out` and recording sizes[c]
static void lz4_compress_host(const uint8_t* src, size_t n,
                              std::vector<uint32_t>& sizes,
                              std::vector<uint8_t>& out) {
  std::vector<uint8_t> tmp(LZ4_CHUNK + LZ4_CHUNK / 128 + 64);
  for (size_t c = 0; c < sizes.size(); ++c) {
    size_t cn = std::min<size_t>(LZ4_CHUNK, n - c * LZ4_CHUNK);
    size_t cs = lz4_compress_block(src + c * LZ4_CHUNK, cn, tmp.data());
    sizes[c] = (uint32_t)cs;
    out.insert(out.end(), tmp.data(), tmp.data() + cs);
  }
}

static py::bytes lz4_compress_py(py::buffer buf) {
  py::buffer_info info = buf.request(false);
  const uint8_t* src = (const uint8_t*)info.ptr;
  size_t n = (size_t)info.size * info.itemsize;
  std::vector<uint32_t> sizes(lz4_chunk_count(n));
  std::vector<uint8_t> out;
  out.reserve(n / 2 + 1024);
  out.resize(lz4_header_size(sizes.size()));
  {
    py::gil_scoped_release rel;
    lz4_compress_host(src, n, sizes, out);
    lz4_write_header(out.data(), n, sizes);
  }
  return py::bytes((const char*)out.data(), out.size());
}

struct Lz4Header {
  uint64_t raw_size;
  uint32_t chunk_size, n_chunks;
  const uint32_t* sizes;
  const uint8_t* payload;
};

static Lz4Header lz4_parse(const uint8_t* p, size_t n) {
  if (n < 20) throw std::runtime_error("lz4: short container");
  uint32_t magic;
  memcpy(&magic, p, 4);
  if (magic != LZ4_MAGIC) throw std::runtime_error("lz4: bad magic");
  Lz4Header h;
  memcpy(&h.raw_size, p + 4, 8);
  memcpy(&h.chunk_size, p + 12, 4);
  memcpy(&h.n_chunks, p + 16, 4);
  if (n < 20 + 4ull * h.n_chunks) throw std::runtime_error("lz4: truncated");
  h.sizes = (const uint32_t*)(p + 20);
  h.payload = p + 20 + 4ull * h.n_chunks;
  // the decoders walk sizes[] over the payload and index chunk c at
  // c * chunk_size: both must stay inside what the header announces
  uint64_t payload_n = 0;
  for (uint32_t c = 0; c < h.n_chunks; ++c) payload_n += h.sizes[c];
  if (payload_n > n - 20 - 4ull * h.n_chunks)
    throw std::runtime_error("lz4: truncated");
  if ((uint64_t)h.n_chunks * h.chunk_size < h.raw_size ||
      (h.n_chunks && (uint64_t)(h.n_chunks - 1) * h.chunk_size >= h.raw_size))
    throw std::runtime_error("lz4: chunk table does not match raw size");
  return h;
}

// host codec: decompress a parsed container into dst[0, raw_size)
static void lz4_decompress_host(const Lz4Header& h, uint8_t* dst) {
  const uint8_t* p = h.payload;
  for (uint32_t c = 0; c < h.n_chunks; ++c) {
    uint64_t at = (uint64_t)c * h.chunk_size;
    size_t cap = std::min<uint64_t>(h.chunk_size, h.raw_size - at);
    size_t got = lz4_decompress_block_host(p, h.sizes[c], dst + at, cap);
    if (got != cap) throw std::runtime_error("lz4: corrupt chunk");
    p += h.sizes[c];
  }
}

static py::bytes lz4_decompress_py(py::buffer buf) {
  py::buffer_info info = buf.request(false);
  const uint8_t* src = (const uint8_t*)info.ptr;
  size_t n = (size_t)info.size * info.itemsize;
  Lz4Header h = lz4_parse(src, n);
  std::string out(h.raw_size, '\0');
  {
    py::gil_scoped_release rel;
    lz4_decompress_host(h, (uint8_t*)out.data());
  }
  return py::bytes(out);
}

// decompress a CVLZ container directly into an arena (GPU kernel on device
// arenas: one workgroup per 64K chunk)
static uint64_t arena_lz4_decompress(int ah, uint64_t dst_off, py::buffer buf) {
  Arena* a = get_arena(ah);
  py::buffer_info info = buf.request(false);
  const uint8_t* src = (const uint8_t*)info.ptr;
  size_t n = (size_t)info.size * info.itemsize;
  Lz4Header h = lz4_parse(src, n);
  check_range(a, dst_off, h.raw_size);
  if (h.n_chunks == 0) return 0;   // empty container: no grid-0 launch
  py::gil_scoped_release rel;
  if (!a->is_dev()) {
    lz4_decompress_host(h, (uint8_t*)a->base + dst_off);
    return h.raw_size;
  }
  std::lock_guard<std::mutex> g(a->mu);
  HIP_CHECK(hipSetDevice(a->device));
  std::vector<uint32_t> offs(h.n_chunks);
  uint32_t acc = 0;
  for (uint32_t c = 0; c < h.n_chunks; ++c) {
    offs[c] = acc;
    acc += h.sizes[c];
  }
  size_t payload_n = acc;
  Scratch sc(a, Scratch::room<uint8_t>(payload_n) +
                    Scratch::room<uint32_t>(2ull * h.n_chunks + 1));
  uint8_t* d_comp = sc.take<uint8_t>(payload_n);
  uint32_t* d_off = sc.take<uint32_t>(h.n_chunks);
  uint32_t* d_len = sc.take<uint32_t>(h.n_chunks);
  int* d_err = (int*)sc.take<uint32_t>(1);
  HIP_CHECK(hipMemcpyAsync(d_comp, h.payload, payload_n,
                           hipMemcpyHostToDevice, a->kstream));
  HIP_CHECK(hipMemcpyAsync(d_off, offs.data(), 4ull * h.n_chunks,
                           hipMemcpyHostToDevice, a->kstream));
  HIP_CHECK(hipMemcpyAsync(d_len, h.sizes, 4ull * h.n_chunks,
                           hipMemcpyHostToDevice, a->kstream));
  HIP_CHECK(hipMemsetAsync(d_err, 0, 4, a->kstream));
  launch(lz4_decompress_kernel, std::min<uint32_t>(h.n_chunks, 16384), 64,
         a->kstream, d_comp, d_off, d_len, (uint8_t*)a->base + dst_off,
         h.chunk_size, h.raw_size, h.n_chunks, d_err);
  int err_host = 0;
  HIP_CHECK(hipMemcpyAsync(&err_host, d_err, 4, hipMemcpyDeviceToHost,
                           a->kstream));
  HIP_CHECK(hipStreamSynchronize(a->kstream));
  if (err_host) throw std::runtime_error(
      "lz4: corrupt chunk " + std::to_string(err_host - 1) + " (device)");
  return h.raw_size;
}

// compress arena bytes [off, off+n) into a CVLZ container.  Device arenas:
// one wave per 64K chunk compresses into fixed-stride scratch slots, the
// chunk lengths come back in one small D2H, copy_extents_kernel packs the
// payloads contiguously on the device and ONE D2H moves them — only
// compressed bytes cross the host link.
static py::bytes arena_lz4_compress(int ah, uint64_t off, uint64_t n) {
  Arena* a = get_arena(ah);
  check_range(a, off, n);
  if (n > LZ4_DEVICE_MAX_N)
    throw std::runtime_error(
        "lz4: compress of " + std::to_string(n) + " bytes exceeds the " +
        std::to_string(LZ4_DEVICE_MAX_N) + "-byte per-call limit; segment it");
  uint32_t n_chunks = lz4_chunk_count(n);
  size_t header = lz4_header_size(n_chunks);
  std::vector<uint32_t> sizes(n_chunks);
  std::vector<uint8_t> out(header);
  {
    py::gil_scoped_release rel;
    if (!a->is_dev()) {
      lz4_compress_host((const uint8_t*)a->base + off, n, sizes, out);
    } else if (n_chunks) {
      std::lock_guard<std::mutex> g(a->mu);
      HIP_CHECK(hipSetDevice(a->device));
      // scratch: slots | packed payload | lens + err | extent + tile tables
      // (a slot spans at most 2 tiles); the slot stride is a multiple of
      // 64, so both byte regions start where they always did
      size_t slots_n = (size_t)n_chunks * LZ4_SLOT_STRIDE;
      Scratch sc(a, 2 * Scratch::room<uint8_t>(slots_n) +
                        Scratch::room<uint32_t>(n_chunks + 1) +
                        Tiles::room<Extent>(n_chunks, 2ull * n_chunks));
      uint8_t* d_slots = sc.take<uint8_t>(slots_n);
      uint8_t* d_pack = sc.take<uint8_t>(slots_n);
      uint32_t* d_len = sc.take<uint32_t>(n_chunks + 1);
      int* d_err = (int*)(d_len + n_chunks);
      HIP_CHECK(hipMemsetAsync(d_err, 0, 4, a->kstream));
      launch(lz4_compress_kernel, std::min<uint32_t>(n_chunks, 16384), 64,
             a->kstream, (const uint8_t*)a->base, off, n, (uint32_t)LZ4_CHUNK,
             d_slots, LZ4_SLOT_STRIDE, d_len, n_chunks, d_err);
      // lens + error flag are adjacent: one small D2H
      std::vector<uint32_t> lens(n_chunks + 1);
      HIP_CHECK(hipMemcpyAsync(lens.data(), d_len, 4ull * (n_chunks + 1),
                               hipMemcpyDeviceToHost, a->kstream));
      HIP_CHECK(hipStreamSynchronize(a->kstream));
      if (lens[n_chunks]) throw std::runtime_error(
          "lz4: compress slot overflow in chunk " +
          std::to_string(lens[n_chunks] - 1) + " (device)");
      std::vector<Extent> exts(n_chunks);
      uint64_t total = 0;
      for (uint32_t c = 0; c < n_chunks; ++c) {
        if (lens[c] == 0 || lens[c] > LZ4_SLOT_STRIDE)
          throw std::runtime_error("lz4: bad device chunk length");
        sizes[c] = lens[c];
        exts[c] = {(uint64_t)c * LZ4_SLOT_STRIDE, total, lens[c]};
        total += lens[c];
      }
      launch_copy_extents(a, sc, d_slots, d_pack, exts,
                          extent_tiles(exts, "lz4"));
      out.resize(header + total);
      HIP_CHECK(hipMemcpyAsync(out.data() + header, d_pack, total,
                               hipMemcpyDeviceToHost, a->kstream));
      HIP_CHECK(hipStreamSynchronize(a->kstream));
    }
    lz4_write_header(out.data(), n, sizes);
  }
  return py::bytes((const char*)out.data(), out.size());
}

// ---------------------------------------------------------------------------
// DLPack export: zero-copy torch tensors over arena memory (uint8, 1-D).
// Lets RCCL collectives (torch.distributed "nccl" on ROCm) broadcast
// HBM-resident cache blocks over xGMI without a staging copy, and lets
// DataLoaders consume cached bytes as device tensors.
// ABI structs per dlpack v0.8 (stable).
// ---------------------------------------------------------------------------

extern "C" {
typedef struct { int32_t device_type; int32_t device_id; } DLDevice;
typedef struct { uint8_t code; uint8_t bits; uint16_t lanes; } DLDataType;
typedef struct {
  void* data; DLDevice device; int32_t ndim; DLDataType dtype;
  int64_t* shape; int64_t* strides; uint64_t byte_offset;
} DLTensor;
typedef struct DLManagedTensor {
  DLTensor dl_tensor; void* manager_ctx;
  void (*deleter)(struct DLManagedTensor*);
} DLManagedTensor;
}
static const int kDLCPU = 1, kDLROCM = 10;

struct DLWrap { DLManagedTensor mt; int64_t shape[1]; };

static void dl_deleter(DLManagedTensor* mt) {
  delete reinterpret_cast<DLWrap*>(mt->manager_ctx);
}

static void dl_capsule_destructor(PyObject* cap) {
  // torch renames the capsule to "used_dltensor" after consuming it
  if (PyCapsule_IsValid(cap, "dltensor")) {
    auto* mt = (DLManagedTensor*)PyCapsule_GetPointer(cap, "dltensor");
    if (mt && mt->deleter) mt->deleter(mt);
  }
}

static py::object arena_dlpack(int h, uint64_t off, uint64_t n) {
  Arena* a = get_arena(h);
  check_range(a, off, n);
  auto* w = new DLWrap();
  w->shape[0] = (int64_t)n;
  w->mt.dl_tensor.data = (uint8_t*)a->base + off;
  w->mt.dl_tensor.device = {a->is_dev() ? kDLROCM : kDLCPU,
                            a->is_dev() ? a->device : 0};
  w->mt.dl_tensor.ndim = 1;
  w->mt.dl_tensor.dtype = {0 /*kDLInt? 0=int*/, 8, 1};
  w->mt.dl_tensor.dtype.code = 1;  // kDLUInt
  w->mt.dl_tensor.shape = w->shape;
  w->mt.dl_tensor.strides = nullptr;
  w->mt.dl_tensor.byte_offset = 0;
  w->mt.manager_ctx = w;
  w->mt.deleter = dl_deleter;
  PyObject* cap = PyCapsule_New(&w->mt, "dltensor", dl_capsule_destructor);
  return py::reinterpret_steal<py::object>(cap);
}

static py::memoryview arena_host_view(int h, uint64_t off, uint64_t n) {
  Arena* a = get_arena(h);
  if (a->is_dev()) throw std::runtime_error("arena_host_view: device arena");
  check_range(a, off, n);
  return py::memoryview::from_memory((uint8_t*)a->base + off, n, false);
}

// ---------------------------------------------------------------------------
// Pinned host buffers (FUSE reply/request buffers: DMA lands directly in
// the buffer that is writev'd to /dev/fuse — no staging-ring hop)
// ---------------------------------------------------------------------------

struct PinnedBuf { void* ptr = nullptr; size_t n = 0; bool pinned = false; };
static std::vector<PinnedBuf> g_pins;
static std::mutex g_pins_mu;

// hipHostMalloc costs ~1 ms and hipHostFree waits on the device, so freed
// buffers park on a free list and the next pinned_alloc of exactly that
// byte size takes the newest one back (malloc'd buffers without a GPU go
// the same way).  Bounded by count and by total bytes: what no longer fits
// is freed as before, oldest parked buffer first, so sizes nobody asks for
// any more cannot hold the pool.  A buffer above the per-buffer cap is never
// parked.  Contract: a caller frees a buffer only after its reads into it
// have returned — parking does no device sync, and the contents of a fresh
// buffer are unspecified, as they always were.  Parked buffers live until
// they are evicted or the process exits.
static constexpr size_t kPinPoolMaxBuf = 64u << 20;
static constexpr size_t kPinPoolMaxCount = 64;
static constexpr size_t kPinPoolMaxBytes = 512u << 20;
static std::vector<PinnedBuf> g_pin_pool;   // oldest first; g_pins_mu
static size_t g_pin_pool_bytes = 0;         // g_pins_mu

static int pinned_publish(const PinnedBuf& b) {   // g_pins_mu held
  for (size_t i = 0; i < g_pins.size(); ++i)
    if (!g_pins[i].ptr) { g_pins[i] = b; return (int)i; }
  g_pins.push_back(b);
  return (int)g_pins.size() - 1;
}

static void pinned_release(const PinnedBuf& b) {
  if (b.pinned) hipHostFree(b.ptr);
  else std::free(b.ptr);
}

static int pinned_alloc(size_t n) {
  {
    std::lock_guard<std::mutex> g(g_pins_mu);
    for (size_t i = g_pin_pool.size(); i-- > 0;) {
      if (g_pin_pool[i].n != n) continue;
      PinnedBuf b = g_pin_pool[i];
      g_pin_pool.erase(g_pin_pool.begin() + i);
      g_pin_pool_bytes -= b.n;
      g_st_pinned_reused.fetch_add(1, std::memory_order_relaxed);
      return pinned_publish(b);
    }
  }
  PinnedBuf b;
  b.n = n;
  if (device_count() > 0) {
    HIP_CHECK(hipHostMalloc(&b.ptr, n, hipHostMallocDefault));
    b.pinned = true;
  } else {
    b.ptr = std::malloc(n ? n : 1);
    if (!b.ptr) throw std::bad_alloc();
  }
  g_st_pinned_created.fetch_add(1, std::memory_order_relaxed);
  std::lock_guard<std::mutex> g(g_pins_mu);
  return pinned_publish(b);
}

static void pinned_free(int id) {
  std::vector<PinnedBuf> drop;   // freed outside the lock: hipHostFree
                                 // waits on the device
  {
    std::lock_guard<std::mutex> g(g_pins_mu);
    if (id < 0 || id >= (int)g_pins.size() || !g_pins[id].ptr) return;
    PinnedBuf b = g_pins[id];
    g_pins[id] = PinnedBuf{};
    if (b.n > kPinPoolMaxBuf) {
      drop.push_back(b);
    } else {
      g_pin_pool.push_back(b);
      g_pin_pool_bytes += b.n;
      while (g_pin_pool.size() > kPinPoolMaxCount ||
             g_pin_pool_bytes > kPinPoolMaxBytes) {
        drop.push_back(g_pin_pool.front());
        g_pin_pool_bytes -= g_pin_pool.front().n;
        g_pin_pool.erase(g_pin_pool.begin());
      }
    }
  }
  for (const PinnedBuf& b : drop) pinned_release(b);
}

static py::dict hip_pool_stats() {
  py::dict d;
  d["pinned_created"] = g_st_pinned_created.load();
  d["pinned_reused"] = g_st_pinned_reused.load();
  {
    std::lock_guard<std::mutex> g(g_pins_mu);
    d["pinned_parked_bytes"] = g_pin_pool_bytes;
    d["pinned_parked_count"] = g_pin_pool.size();
  }
  d["pinned_pool_max_count"] = kPinPoolMaxCount;
  d["pinned_pool_max_bytes"] = kPinPoolMaxBytes;
  d["pinned_pool_max_buffer"] = kPinPoolMaxBuf;
  d["streams_created"] = g_st_streams_created.load();
  d["streams_reused"] = g_st_streams_reused.load();
  d["reader_pread_calls"] = g_st_reader_pread.load();
  return d;
}

static py::memoryview pinned_view(int id) {
  std::lock_guard<std::mutex> g(g_pins_mu);
  if (id < 0 || id >= (int)g_pins.size() || !g_pins[id].ptr)
    throw std::runtime_error("bad pinned buffer id");
  return py::memoryview::from_memory(g_pins[id].ptr, g_pins[id].n, false);
}

static uintptr_t pinned_ptr(int id) {
  std::lock_guard<std::mutex> g(g_pins_mu);
  if (id < 0 || id >= (int)g_pins.size() || !g_pins[id].ptr)
    throw std::runtime_error("bad pinned buffer id");
  return (uintptr_t)g_pins[id].ptr;
}

static py::dict arena_info(int h) {
  Arena* a = get_arena(h);
  py::dict d;
  d["capacity"] = a->cap;
  d["device"] = a->device;
  d["pinned"] = a->pinned;
  d["staging_bytes"] = a->pin_sz;
  d["staging_count"] = a->pin.size();
  return d;
}

// raw host->device copy for staged remote reads into consumer tensors
static void memcpy_h2d(uintptr_t dst, uintptr_t src, uint64_t n) {
  py::gil_scoped_release rel;
  HIP_CHECK(hipMemcpy((void*)dst, (const void*)src, n, hipMemcpyHostToDevice));
}

// raw device->host copy: the scales of a dequantising load whose extent
// takes the host convert path
static void memcpy_d2h(uintptr_t dst, uintptr_t src, uint64_t n) {
  py::gil_scoped_release rel;
  HIP_CHECK(hipMemcpy((void*)dst, (const void*)src, n, hipMemcpyDeviceToHost));
}

static void device_sync(int device) {
  py::gil_scoped_release rel;
  HIP_CHECK(hipSetDevice(device));
  HIP_CHECK(hipDeviceSynchronize());
}

// native FUSE data loop (needs Arena/get_arena/thread_stream above)
#include "fuse_loop.hip"

// native metadata RPC frontend (pure epoll/C++, no GPU involvement)
#include "meta_server.cpp"
#include "data_server.cpp"
#include "sdk_abi.cpp"

static py::dict device_mem_info(int device) {
  size_t free_b = 0, total_b = 0;
  HIP_CHECK(hipSetDevice(device));
  HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
  py::dict d;
  d["free"] = free_b;
  d["total"] = total_b;
  return d;
}

PYBIND11_MODULE(_native, m) {
  m.doc() = "curvine_amd native data plane (HIP/CDNA4, gfx950)";
  m.def("device_count", &device_count);
  m.def("device_sync", &device_sync);
  m.def("memcpy_h2d", &memcpy_h2d);
  m.def("memcpy_d2h", &memcpy_d2h);
  m.def("device_mem_info", &device_mem_info);
  m.def("arena_ipc_handle", &arena_ipc_handle);
  m.def("arena_ipc_open", &arena_ipc_open);
  m.def("arena_create", &arena_create, py::arg("device"), py::arg("capacity"),
        py::arg("staging_bytes") = 4 << 20, py::arg("staging_count") = 8,
        py::arg("host_pinned") = false);
  m.def("arena_destroy", &arena_destroy);
  m.def("arena_read", &arena_read);
  m.def("arena_write", &arena_write);
  m.def("arena_read_ptr", &arena_read_ptr);
  m.def("arena_write_ptr", &arena_write_ptr);
  m.def("arena_copy", &arena_copy);
  m.def("arena_fill", &arena_fill);
  m.def("arena_crc32c", &arena_crc32c);
  m.def("arena_gather", &arena_gather);
  m.def("arena_gather_ptr", &arena_gather_ptr);
  m.def("arena_convert_ptr", &arena_convert_ptr);
  m.def("arena_store_ptr", &arena_store_ptr);
  m.def("convert_host", &convert_host, py::arg("src"), py::arg("src_dtype"),
        py::arg("dst_dtype"), py::arg("n"), py::arg("scales") = py::none(),
        py::arg("scale_every") = 0, py::arg("scale_e0") = 0);
  m.def("arena_token_windows", &arena_token_windows);
  m.def("token_convert_host", &token_convert_host);
  m.def("arena_array_samples", &arena_array_samples);
  m.def("array_sample_host", &array_sample_host_py);
  m.def("absmax_scales", &absmax_scales);
  m.def("token_docs", &token_docs);
  m.def("arena_token_eos_index", &arena_token_eos_index);
  m.def("token_eos_index_host", &token_eos_index_host);
  m.def("arena_token_pack", &arena_token_pack);
  m.def("token_pack_piece_host", &token_pack_piece_host);
  m.def("arena_mx_store_ptr", &arena_mx_store_ptr);
  m.def("arena_mx_convert_ptr", &arena_mx_convert_ptr);
  m.def("mx_scales", &mx_scales);
  m.def("mx_convert_host", &mx_convert_host);
  m.def("arena_block_store_ptr", &arena_block_store_ptr);
  m.def("arena_block_convert_ptr", &arena_block_convert_ptr);
  m.def("block_absmax_scales", &block_absmax_scales);
  m.def("block_convert_host", &block_convert_host, py::arg("src"),
        py::arg("src_dtype"), py::arg("dst_dtype"), py::arg("n"),
        py::arg("scales"), py::arg("scale_e0"), py::arg("M"), py::arg("K"),
        py::arg("bm"), py::arg("bn"), py::arg("scale_g0") = 0);
  m.def("arena_base_ptr", &arena_base_ptr);
  m.def("arena_read_batch", &arena_read_batch);
  m.def("reader_register", &reader_register);
  m.def("reader_unregister", &reader_unregister);
  m.def("reader_pread_batch", &reader_pread_batch);
  m.def("reader_pread", &reader_pread);
  m.def("hip_pool_stats", &hip_pool_stats);
  m.def("arena_info", &arena_info);
  m.def("arena_dlpack", &arena_dlpack);
  m.def("arena_host_view", &arena_host_view);
  m.def("pinned_alloc", &pinned_alloc);
  m.def("pinned_free", &pinned_free);
  m.def("pinned_view", &pinned_view);
  m.def("pinned_ptr", &pinned_ptr);
  m.def("fuse_loop_create", &fuse_loop_create);
  m.def("fuse_loop_add_channel", &fuse_loop_add_channel);
  m.def("fuse_loop_register", &fuse_loop_register);
  m.def("fuse_loop_unregister", &fuse_loop_unregister);
  m.def("fuse_loop_register_write", &fuse_loop_register_write);
  m.def("fuse_loop_unregister_write", &fuse_loop_unregister_write);
  m.def("fuse_loop_write_state", &fuse_loop_write_state);
  m.def("fuse_loop_next_forward", &fuse_loop_next_forward);
  m.def("fuse_loop_stats", &fuse_loop_stats);
  m.def("fuse_loop_stop", &fuse_loop_stop);
  m.def("meta_create", &meta_create);
  m.def("meta_stop", &meta_stop_srv);
  m.def("meta_set_serving", &meta_set_serving);
  m.def("meta_upsert", &meta_upsert);
  m.def("meta_upsert_node", &meta_upsert_node);
  m.def("meta_touch", &meta_touch);
  m.def("meta_upsert_with_children", &meta_upsert_with_children);
  m.def("meta_add_child", &meta_add_child);
  m.def("meta_remove_child", &meta_remove_child);
  m.def("meta_drop", &meta_drop);
  m.def("meta_clear", &meta_clear);
  m.def("meta_forward_pop", &meta_forward_pop);
  m.def("meta_eventfd", &meta_eventfd);
  m.def("meta_send", &meta_send);
  m.def("meta_stats", &meta_stats);
  m.def("meta_worker_upsert", &meta_worker_upsert);
  m.def("meta_block_add_loc", &meta_block_add_loc);
  m.def("meta_block_remove_loc", &meta_block_remove_loc);
  m.def("meta_block_drop", &meta_block_drop);
  m.def("meta_take_access", &meta_take_access);
  m.def("data_create", &data_create);
  m.def("data_stop", &data_stop_srv);
  m.def("data_block_publish", &data_block_publish, py::arg("sid"),
        py::arg("block_id"), py::arg("kind"), py::arg("arena"),
        py::arg("aoff"), py::arg("len"), py::arg("path"),
        py::arg("direct") = false);
  m.def("data_block_drop", &data_block_drop);
  m.def("data_block_refs", &data_block_refs);
  m.def("data_write_register", &data_write_register);
  m.def("data_write_unregister", &data_write_unregister);
  m.def("data_forward_pop", &data_forward_pop);
  m.def("data_eventfd", &data_eventfd);
  m.def("data_send", &data_send);
  m.def("data_stats", &data_stats);
  m.def("data_read_into", &data_read_into);
  m.def("data_write_from", &data_write_from);
  m.def("dw_open", &dw_open);
  m.def("dw_write", &dw_write);
  m.def("dw_drain", &dw_drain);
  m.def("dw_commit", &dw_commit);
  m.def("dw_abort", &dw_abort);
  m.def("lz4_compress", &lz4_compress_py);
  m.def("lz4_decompress", &lz4_decompress_py);
  m.def("arena_lz4_decompress", &arena_lz4_decompress);
  m.def("arena_lz4_compress", &arena_lz4_compress);
  m.def("crc32c", &crc32c_buf, py::arg("buf"), py::arg("init") = 0);
  m.def("crc32c_combine", &crc32c_combine);
  m.attr("CRC_SUB") = CRC_SUB;
  m.attr("CAST_TILE") = CAST_TILE;
  m.attr("TILE_GRID_CAP") = TILE_GRID_CAP;
  m.attr("TOKEN_TILE") = TOKEN_TILE;
  m.attr("ARRAY_TILE") = ARRAY_TILE;
  m.attr("TOKEN_DOC_CHUNK") = TOKEN_DOC_CHUNK;
  m.attr("TOKEN_EOS_TILE") = TOKEN_EOS_TILE;
  m.attr("TOKEN_PACK_TILE") = TOKEN_PACK_TILE;
  m.attr("TOKEN_SEG_NEXT") = TOKEN_SEG_NEXT;
  m.attr("TOKEN_SEG_PAD") = TOKEN_SEG_PAD;
  m.attr("__hip_arch__") = "gfx950";
}

// MI355X (gfx950) batch Ed25519 verifier for PBFT prepare/commit quorums:
// kernels + the C ABI declared in include/pbft_verify.h.
//
// Data layout in HBM (one context = one GPU):
//   tabB   comb table of the base point, plan PLB (10 positions of 25/26-bit
//          signed windows, 128-B entries)
//   tabA   one comb table of -A per replica key, same geometry with WA
//   keys   raw 32-byte key encodings (hashed as given) + key_ok bytes
//   batch  SoA: R[N][32], S[N][32], key_idx[N] u16, msg[N][stride]
//   bitmap ceil(N/64) u64 words, one per wavefront (ballot)
#include <dlfcn.h>
#include <sched.h>
#include <hip/hip_runtime.h>
#include <sys/mman.h>
#include <rccl/rccl.h>  // types only: librccl.so.1 is dlopen'ed by pbft_multi_create
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <mutex>
#include <random>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/pbft_verify.h"
#include "../../include/pbft_wire.h"
#include "../../include/pbft_replica.h"  // pbft_envelope
#include "digest_kernels.h"
#include "verify_core.h"

using namespace pbft;
#include "verify_kernels.h"
#include "tally_kernels.h"
#include "admit_kernels.h"
#include "group_kernels.h"
#include "wire_decode_kernels.h"
#include "wire_index_kernels.h"
#include "wire_pp_kernels.h"
#include "egress_kernels.h"
#include "propose_kernels.h"
#include "reply_kernels.h"
#include "accept_kernels.h"
#include "anykey_kernels.h"
#include "sign_host.h"
// Finish configuration by batch size (signatures per lane, product tree, waves per SIMD), measured on MI355X
// with the lane-parallel wave inversion (profiles/r03/ab_finish.txt): 131k 0.2115 -> 0.1906 ms (width 2),
// 262k 0.3628 -> 0.3429 (width 4), 2^20 finish kernel 118.6 -> 91.4 us (width 8, tree, 2 waves per SIMD).
#ifndef PBFT_FIN_SMALL_UPTO
#define PBFT_FIN_SMALL_UPTO (1u << 17)
#endif
#ifndef PBFT_FIN_FM_SMALL
#define PBFT_FIN_FM_SMALL 2  // finish signatures per lane for N <= PBFT_FIN_SMALL_UPTO
#endif
#ifndef PBFT_FIN_TINY_UPTO
#define PBFT_FIN_TINY_UPTO (1u << 16)  // one signature per finish lane up to here (r04: 2^16 0.1097 -> 0.1064 ms,
#endif                                 // 2^17 +3 %: profiles/r04/ab_fin_shard.txt)
#ifndef PBFT_FIN_FM_MID
#define PBFT_FIN_FM_MID 4  // ... for PBFT_FIN_SMALL_UPTO < N < 2^19
#endif
#ifndef PBFT_FIN_FM_BIG
#define PBFT_FIN_FM_BIG 8  // ... for N >= 2^19
#endif
#ifndef PBFT_FIN_TREE_MAX_FM
#define PBFT_FIN_TREE_MAX_FM 8  // finish widths up to this use the cross-lane product tree (one inversion per wave)
#endif
#ifndef PBFT_FIN_W_BIG
#define PBFT_FIN_W_BIG 2  // waves per SIMD of the product-tree finish for N >= 2^19
#endif


// ------------------------------------------------------------------ errors
static thread_local std::string g_last_error;
static int set_err(int code, const char* what) {
  g_last_error = what;
  return code;
}
#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t _e = (expr);                                                             \
    if (_e != hipSuccess) {                                                             \
      char _b[256];                                                                     \
      snprintf(_b, sizeof _b, "%s: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
               __LINE__);                                                               \
      return set_err(PBFT_EHIP, _b);                                                    \
    }                                                                                   \
  } while (0)

// One grow-only device buffer: at least `bytes` afterwards, its contents not kept.  A failed allocation leaves it empty
// and consistent (null, capacity 0) and returns PBFT_ENOMEM with the caller's text.
static int grow_device(uint8_t** p, size_t* cap, size_t bytes, const char* what) {
  if (bytes <= *cap) return PBFT_OK;
  if (*p) HIP_TRY(hipFree(*p));  // (waits for the device: an earlier call may still use it)
  *p = nullptr;
  *cap = 0;
  if (hipMalloc(p, bytes) != hipSuccess) return set_err(PBFT_ENOMEM, what);
  *cap = bytes;
  return PBFT_OK;
}

// ------------------------------------------------------------------ kernels



// Request digests: one byte string per lane (offsets/lens into a packed buffer).
template <int KIND>  // 0 = Blake2b-512, 1 = SHA-256
__global__ void __launch_bounds__(BLOCK) digest_kernel(const uint8_t* __restrict__ data,
                                                       const uint64_t* __restrict__ offsets,
                                                       const uint32_t* __restrict__ lens, uint64_t N,
                                                       uint8_t* __restrict__ out) {
  const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (i >= N) return;
  const uint8_t* m = data + offsets[i];
  if (KIND == 0) {
    uint8_t d[64];
    blake2b512(d, m, lens[i]);
#pragma unroll
    for (int j = 0; j < 64; ++j) out[64 * i + j] = d[j];
  } else {
    uint8_t d[32];
    sha256(d, m, lens[i]);
#pragma unroll
    for (int j = 0; j < 32; ++j) out[32 * i + j] = d[j];
  }
}

// ------------------------------------------------------------------ context
// A replica key set on one device: raw encodings, key_ok bytes and the -A comb
// tables.  Reference-counted so that contexts cloned for extra streams
// (pbft_verify_ctx_clone) serve batches from the same tables.
struct keyset {
  std::atomic<int> refs{1};
  uint32_t* d_tabA = nullptr;
  uint32_t* d_keys = nullptr;
  uint8_t* d_key_ok = nullptr;
  uint32_t n = 0;
  uint32_t cap = 0;      // keys d_keys / d_key_ok hold
  size_t tab_bytes = 0;  // bytes of d_tabA (a later set_keys whose plan's tables fit reuses the buffers)
  int pa = 0;  // positions of the key plan (identifies PLA_HUGE / PLA_BIG / PLA_MID / PLA_SMALL)
  // the encodings as installed, host side, and a number that changes whenever one of them does: the PeerId table of
  // pbft_accept_reserve is built from the first and is stale once the second has moved on
  std::vector<uint8_t> h_keys;
  uint64_t gen = 0;
};
static std::atomic<uint64_t> g_keyset_gen{0};
static size_t plan_table_words(int pa) {
  return pa == PLA_HUGE::P ? PLA_HUGE::TABLE_WORDS
       : pa == PLA_BIG::P  ? PLA_BIG::TABLE_WORDS
       : pa == PLA_MID::P  ? PLA_MID::TABLE_WORDS
                           : PLA_SMALL::TABLE_WORDS;
}
static void keyset_release(keyset* k) {
  if (k && --k->refs == 0) {
    (void)hipFree(k->d_tabA); (void)hipFree(k->d_keys); (void)hipFree(k->d_key_ok);
    delete k;
  }
}

// device staging buffers of the votes chunks (chunk c uses buffer c % VOTES_BUFS; its copy waits for the kernels
// of chunk c - VOTES_BUFS)
static constexpr int VOTES_BUFS = 4;
#ifndef PBFT_VOTES_TWO_STREAMS
#define PBFT_VOTES_TWO_STREAMS 1
#endif

struct pbft_ctx {
  int device = -1;
  hipStream_t stream = nullptr;
  uint32_t* d_tabB = nullptr;
  keyset* ks = nullptr;
  // cached from ks (null / 0 without a key set)
  uint32_t* d_tabA = nullptr;
  uint32_t* d_keys = nullptr;
  uint8_t* d_key_ok = nullptr;
  uint32_t n_keys = 0;
  int pa = 0;  // comb positions of the installed key tables' plan (PLA_HUGE, PLA_BIG, PLA_MID or PLA_SMALL)
  uint64_t split_below = SPLIT_BELOW;  // latency mode below this batch size (env PBFT_SPLIT_BELOW)
  int fin_m = 0;                       // finish-kernel signatures per lane (0 = by batch size)
  int fin_tree = -1;                   // finish cross-lane tree (0: none; 4 / 6: the compiled tree; -1 = by batch size)
  int fin_waves = 0;                   // product-tree finish compiled for 1 or 2 waves per SIMD (0 = by batch size)
  int lat_split = 0;                   // latency-mode lanes per signature (4 / 8; 0 = by batch size)
  int comb_pair = -1;                  // comb_pair_kernel: 1 on, 0 off, -1 by batch size (PBFT_OPT_COMB_PAIR)
  int comb_prio = -1;                  // 8-wave comb blocks with paired wave priorities: 1, 0, -1 by batch size
                                       // (PBFT_OPT_COMB_PRIO)
  int comb_balance = -1;               // 4-wave comb with priorities falling with each wave's progress: 1, 0, -1 by
                                       // batch size (PBFT_OPT_COMB_BALANCE)
  int cus = 0;                         // compute units of the device
  // ev0 / ev1 around every launch (pbft_last_kernel_ms).  Off by default since r05: the two event records cost 7.5 us
  // per comb + finish pair, 4.5 % of the 131k shard (profiles/r05/shard/timing_events.txt)
  bool timing = false;
  uint64_t key_budget_mb = 0;          // key-table budget override (0 = env / default)
  pbft_key_stats kstats{};             // the last pbft_verify_set_keys / _update_keys (pbft_verify_key_stats)
  int fault_inject = 0;                // PBFT_OPT_FAULT_INJECT (tests): fail the next pbft_verify_update_keys
  void adopt(keyset* k) {
    keyset_release(ks);
    ks = k;
    d_tabA = k ? k->d_tabA : nullptr; d_keys = k ? k->d_keys : nullptr; d_key_ok = k ? k->d_key_ok : nullptr;
    n_keys = k ? k->n : 0; pa = k ? k->pa : 0;
  }
  // staging for the host-buffer API
  uint8_t* d_stage = nullptr;
  size_t stage_cap = 0;
  uint64_t* d_bitmap = nullptr;
  size_t bitmap_cap = 0;
  // verify workspace: R' limbs [30][N] u32 + flags[N]
  uint8_t* d_work = nullptr;
  size_t work_cap = 0;
  // votes form: per-envelope block-2 SHA-512 schedule (W[t] + K[t], t = 16..79; 512 B per envelope)
  uint64_t* d_wk = nullptr;
  uint64_t wk_cap = 0;  // envelopes
  uint64_t work_n = 0;     // signatures the workspace layout is sized for (offsets use this, not the batch N)
  bool work_two = false;   // two xyz/flags halves (pipelined form)
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_done = nullptr;
  // pipelined device form: comb on the caller's stream, finish on a second stream, two workspace halves
  hipEvent_t ev_comb = nullptr, ev_fin[2] = {nullptr, nullptr};
  bool fin_pending[2] = {false, false};
  int half = 0;
  // host-buffer pipeline: H2D of chunk c+1 (copy stream) overlaps the kernels of chunk c; VOTES_BUFS device
  // staging buffers (the per-signature form uses 2)
  hipStream_t cstream = nullptr;
  hipEvent_t ev_copied[VOTES_BUFS] = {}, ev_consumed[VOTES_BUFS] = {};
  // votes chunks alternate between the context stream and stream2, each with its own workspace, so that the
  // kernels of consecutive chunks may overlap (PBFT_VOTES_TWO_STREAMS)
  hipStream_t stream2 = nullptr;
  hipEvent_t ev_env = nullptr, ev_s2 = nullptr;
  uint8_t* d_work2 = nullptr;
  size_t work2_cap = 0;
  uint64_t work2_n = 0;
  bool v_two = false;
  bool v_s2_ready = false;  // stream2 has waited for this batch's envelope table and schedule (ev_env)
  bool two_streams = PBFT_VOTES_TWO_STREAMS;  // env PBFT_VOTES_TWO_STREAMS
  bool in_flight = false;
  uint64_t* async_out = nullptr;
  uint64_t* h_bitmap = nullptr;      // pinned, fine-grained
  uint64_t* h_bitmap_dev = nullptr;  // the same memory as the kernels address it (export_words)
  uint64_t async_words = 0;
  float last_ms = 0.f;
  // pinned host staging of the non-blocking host-buffer forms (pageable caller buffers are copied here,
  // then DMA'd asynchronously; pbft_verify_votes_stage hands it out for in-place filling)
  uint8_t* h_stage = nullptr;
  uint8_t* h_stage_dev = nullptr;  // the same memory as the kernels address it (the import kernels)
  size_t h_stage_cap = 0;
  uint64_t staged_n = 0;   // pbft_verify_votes_stage: the batch the staging is laid out for
  uint32_t staged_env = 0;
  bool staged = false;
  // votes batch being launched chunk by chunk (stage_votes_and_launch, pbft_verify_votes_submit_begin / _rows)
  uint64_t v_n = 0, v_next = 0, v_chunk = 0;  // batch rows, first row not launched, chunks launched
  uint32_t v_env = 0;
  size_t v_env_bytes = 0;
  const uint64_t* v_wk = nullptr;
  bool v_open = false;      // begun, not every chunk launched
  bool v_readback = false;  // progressive: each chunk's bitmap words come back on their own (ev_rows)
  std::vector<hipEvent_t> ev_rows;  // per chunk: its bitmap words are in h_bitmap
  std::vector<uint64_t> v_ends;     // per launched chunk: its end row
  uint32_t v_env_cap = 0;           // a batch opened in pieces (pbft_verify_votes_open): its envelope capacity
  hipEvent_t ev_envp = nullptr;     // a piece's envelopes copied
  bool v_short_tail = false;        // the batch's schedule ends with a VOTES_TAIL-row chunk (votes_chunk_end)
  uint64_t rows_out = 0;            // rows whose bitmap words are in the caller's bitmap
  uint64_t chunk_out = 0;           // chunks whose bitmap words are in the caller's bitmap
  // pbft_verify_votes_tally: signer sets [n_env][W] then counts [n_env] of the batch (grow-only); t_signers is set
  // only while that call launches its chunks (votes_chunk then tallies each chunk's rows), null otherwise
  uint64_t* d_tally = nullptr;
  size_t tally_cap = 0;  // bytes
  uint64_t* t_signers = nullptr;
  // pbft_verify_frames: the frames the host parser settled, as (index, record, head) patches (grow-only)
  uint8_t* d_fpatch = nullptr;
  size_t fpatch_cap = 0;  // bytes
  // pbft_group_envelopes_device: table, slots, marks and their prefix (grow-only; pbft_group_reserve), the hash
  // seed (drawn at first use unless PBFT_OPT_GROUP_SEED set it) and the hash bits kept (PBFT_OPT_GROUP_HASH_BITS)
  uint8_t* d_group = nullptr;
  size_t group_cap = 0;  // bytes
  uint64_t group_seed = 0;
  bool group_seeded = false;
  uint32_t group_hash_bits = 64;
  // pbft_wire_index_streams_device: tables and starts (grow-only; pbft_index_reserve) and the tile bytes
  // (PBFT_OPT_INDEX_TILE)
  uint8_t* d_index = nullptr;
  size_t index_cap = 0;  // bytes
  uint32_t index_tile = INDEX_TILE_DEFAULT;
  // pbft_admit_device: the two key planes, the residue marks and their prefix (grow-only; pbft_admit_reserve)
  uint8_t* d_admit = nullptr;
  size_t admit_cap = 0;  // bytes
  // pbft_sign_set_seed: the expanded signing key a | prefix | A and the replica index (egress_kernels.h), device
  // resident; the signing kernel's form (PBFT_OPT_EGRESS_BLOCK / _DIRECT)
  uint32_t* d_sign_key = nullptr;
  bool sign_set = false;
  uint32_t sign_replica = 0;
  int egress_block = 64;
  bool egress_direct = false;
  // The tile sums of pbft_sign_votes_frames_device, pbft_sign_preprepares_frames_device and pbft_sign_replies_device
  // (grow-only; pbft_egress_reserve, pbft_propose_reserve, pbft_reply_reserve).  One each: the device forms run on the
  // caller's stream, so two of them may be in flight at once.
  uint8_t* d_egress = nullptr;
  size_t egress_cap = 0;  // bytes
  uint8_t* d_propose = nullptr;
  size_t propose_cap = 0;  // bytes
  uint8_t* d_reply = nullptr;
  size_t reply_cap = 0;  // bytes
  // The device staging of the three blocking forms pbft_sign_votes_frames, pbft_sign_preprepares_frames and
  // pbft_sign_replies: inputs, outputs and the written bytes (sign_host.h's sign_layout; grow-only).  One for all: each
  // of them refuses to start while in_flight is set and synchronises `stream` before it returns, so no two hold it at
  // once (all three use `stream` alone: a call that failed half way is still ordered before the next); the device
  // forms never touch it.
  uint8_t* d_sign_io = nullptr;
  size_t sign_io_cap = 0;  // bytes
  int propose_width = PROPOSE_WIDTH_DEFAULT;
  // the installed identity's PeerId text (reply_core.h), also at word REPLY_KEY_PEER_ID of d_sign_key
  char sign_peer_id[pbft::RP_PEER_ID_B58] = {0};
  // pbft_accept_reserve: the installed keys' PeerId texts [n_keys][52] and the key set generation they were made from
  // (0: none); pbft_accept_replies: its staging and the settled replies' patches (grow-only)
  uint8_t* d_accept_pid = nullptr;
  uint32_t accept_pid_cap = 0;  // keys
  uint64_t accept_gen = 0;
  uint8_t* d_accept_io = nullptr;
  size_t accept_io_cap = 0;  // bytes
  uint8_t* d_accept_patch = nullptr;
  size_t accept_patch_cap = 0;  // bytes
};

#ifndef PBFT_ENV_SCHED
#define PBFT_ENV_SCHED 1  // A/B: 0 = every signature expands its own block-2 schedule
#endif

// Bitmap words [lo, lo + n) to the pinned host copy, written by a kernel over PCIe.  A hipMemcpyAsync D2H of these
// few KB blocked the calling thread for 6-8 ms at times on MI355X (PBFT_LAUNCH_TRACE in the replica's flush:
// profiles/r04/launch_stalls.txt), stalling the launch loop behind it; a kernel launch returns at once.  The host
// copy is fine-grained memory: the stores reach it without a cache writeback, and the event recorded after the
// kernel orders them before the host's read.
__global__ void export_words_kernel(const uint64_t* __restrict__ src, uint64_t* __restrict__ dst, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
  __threadfence_system();
}
static hipError_t export_words(pbft_ctx* c, uint64_t lo, uint64_t n, hipStream_t st);
// 16-byte words from host memory the kernels can address (the mapped staging) to device memory: one launch on the
// consuming stream instead of a copy-stream hipMemcpyAsync + event + cross-stream wait (~0.14 ms of host time per
// votes batch, PBFT_LAUNCH_TRACE=30)
__global__ void import16_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

// Pinned host staging (grow-only: hipHostMalloc costs milliseconds).  Never while a batch is in flight.
// Every user of the staging calls this first: whatever pbft_verify_votes_stage handed out is void from here on
// (a later pbft_verify_votes_submit must not launch what another path wrote there).
static int ensure_host_stage(pbft_ctx* c, size_t bytes) {
  c->staged = false;
  if (bytes <= c->h_stage_cap) return PBFT_OK;
  if (c->h_stage) HIP_TRY(hipHostFree(c->h_stage));
  c->h_stage = nullptr;
  c->h_stage_dev = nullptr;
  c->h_stage_cap = 0;
  const size_t cap = bytes + (bytes >> 2) + 4096;
  // fine-grained: kernels that read it in place see every host write, with no stale L2 lines
  if (hipHostMalloc(&c->h_stage, cap, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) {
    (void)hipGetLastError();
    c->h_stage = nullptr;
    return set_err(PBFT_ENOMEM, "pinned host staging alloc");
  }
  if (hipHostGetDevicePointer((void**)&c->h_stage_dev, c->h_stage, 0) != hipSuccess) {
    (void)hipGetLastError();
    c->h_stage_dev = nullptr;  // (kernels then never read it in place)
  }
  c->h_stage_cap = cap;
  return PBFT_OK;
}

// True if p is host memory the DMA engines can read in place (hipHostMalloc / hipHostRegister).  A pageable
// pointer makes the query fail; the error is cleared so that the next launch's hipGetLastError is clean.
static bool host_pinned(const void* p) {
  if (!p) return true;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return a.type == hipMemoryTypeHost;
}
// The address kernels read pinned host memory p at, or null (pageable, or no device mapping).
static const uint8_t* host_dev(const void* p) {
  if (!p) return nullptr;
  hipPointerAttribute_t a;
  if (hipPointerGetAttributes(&a, p) != hipSuccess) {
    (void)hipGetLastError();
    return nullptr;
  }
  if (a.type != hipMemoryTypeHost || !a.devicePointer || !a.hostPointer) return nullptr;
  return (const uint8_t*)a.devicePointer + ((const uint8_t*)p - (const uint8_t*)a.hostPointer);
}

// Host-buffer batches up to one chunk: R, S, key_idx and the messages reach the device staging through ONE kernel
// that reads the pinned host memory over PCIe (16 B per lane, line-contiguous per wave), instead of four
// hipMemcpyAsync.  VERDICT r04 item 2: config #5's back-to-back leg had one 7.5-9.4 ms maximum in every bench line;
// PBFT_LAUNCH_TRACE put it inside hipMemcpyAsync H2D of a 4k batch's columns (profiles/r05/stall_probe.txt: the
// calling thread blocked 7-30 ms in h2d_R / h2d_M while a kernel launch never did), the same signature as the D2H
// stalls r04 removed from the votes path.  PBFT_HOST_IMPORT=0 restores the copies (A/B).
struct import_segs {
  const uint8_t* src[4];
  uint64_t dst_off[4];   // 16-B aligned offsets into the destination
  uint64_t len[4];       // bytes
  uint64_t first[5];     // first 16-B piece of each segment; first[4] = total pieces
};
__global__ void __launch_bounds__(256) import_segs_kernel(import_segs s, uint8_t* __restrict__ dst) {
  const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= s.first[4]) return;
  const int k = c >= s.first[2] ? (c >= s.first[3] ? 3 : 2) : (c >= s.first[1] ? 1 : 0);
  const uint64_t o = (c - s.first[k]) * 16;
  const uint8_t* src = s.src[k] + o;
  uint8_t* d = dst + s.dst_off[k] + o;
  const uint64_t rem = s.len[k] - o;
  if (rem >= 16 && ((uintptr_t)src & 15) == 0) {
    *(uint4*)d = *(const uint4*)src;
  } else if (rem >= 16 && ((uintptr_t)src & 3) == 0) {
    const uint32_t* q = (const uint32_t*)src;
    *(uint4*)d = uint4{q[0], q[1], q[2], q[3]};
  } else {
    const int m = rem < 16 ? (int)rem : 16;
    for (int b = 0; b < m; ++b) d[b] = src[b];
  }
}
static bool host_import_enabled() {
  static const bool on = [] {
    const char* e = getenv("PBFT_HOST_IMPORT");
    return !e || strtol(e, nullptr, 10) != 0;
  }();
  return on;
}
// Launch the import of up to 4 host segments (device-readable addresses) into dst; false if a source has no device
// mapping (the caller then copies).
static bool launch_import(const uint8_t* const* src_host, const uint64_t* dst_off, const uint64_t* len, int n,
                          uint8_t* dst, hipStream_t st) {
  if (!host_import_enabled()) return false;
  import_segs s{};
  uint64_t pieces = 0;
  for (int k = 0; k < 4; ++k) {
    s.first[k] = pieces;
    if (k < n && len[k]) {
      s.src[k] = host_dev(src_host[k]);
      if (!s.src[k]) return false;
      s.dst_off[k] = dst_off[k];
      s.len[k] = len[k];
      pieces += (len[k] + 15) / 16;
    }
  }
  s.first[4] = pieces;
  if (pieces == 0) return true;
  hipLaunchKernelGGL(import_segs_kernel, dim3((unsigned)((pieces + 255) / 256)), dim3(256), 0, st, s, dst);
  return true;
}

// Pinned layout of a staged votes batch (pbft_verify_votes_stage): n rows of PBFT_VOTES_ROW_BYTES, then the
// envelopes.
static constexpr uint32_t ROW = PBFT_VOTES_ROW_BYTES;
static_assert(PBFT_VOTES_ROW_BYTES % 8 == 0 && PBFT_VOTES_ROW_KEY == 64 && PBFT_VOTES_ROW_ENV % 4 == 0 &&
                  PBFT_VOTES_ROW_ENV + 4 <= PBFT_VOTES_ROW_BYTES, "votes row layout");
struct host_votes_layout {
  size_t offE, bytes;
  host_votes_layout(uint64_t n, uint32_t n_env) {
    offE = (ROW * (size_t)n + 255) & ~(size_t)255;
    bytes = offE + (size_t)PBFT_ENVELOPE_LEN * n_env + 64;  // + read slack of the envelope loads
  }
};
struct host_batch_layout {
  size_t offS, offK, offM, bytes;
  host_batch_layout(uint64_t n, uint32_t msg_stride) {
    offS = 32 * n;
    offK = 64 * n;
    offM = (offK + 2 * n + 255) & ~(size_t)255;
    bytes = offM + (size_t)msg_stride * n + 64;
  }
};

static hipError_t export_words(pbft_ctx* c, uint64_t lo, uint64_t n, hipStream_t st) {
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(export_words_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, c->d_bitmap + lo,
                     c->h_bitmap_dev + lo, n);
  return hipGetLastError();
}

static int ensure_stage(pbft_ctx* c, size_t bytes, size_t words) {
  if (bytes > c->stage_cap) {
    if (c->d_stage) HIP_TRY(hipFree(c->d_stage));
    c->d_stage = nullptr;
    size_t cap = bytes + (bytes >> 2) + 4096;
    if (hipMalloc(&c->d_stage, cap) != hipSuccess) { c->stage_cap = 0; return set_err(PBFT_ENOMEM, "staging alloc"); }
    c->stage_cap = cap;
  }
  if (words > c->bitmap_cap) {
    if (c->d_bitmap) HIP_TRY(hipFree(c->d_bitmap));
    if (c->h_bitmap) HIP_TRY(hipHostFree(c->h_bitmap));
    c->d_bitmap = nullptr; c->h_bitmap = nullptr; c->h_bitmap_dev = nullptr;
    size_t cap = words + 64;
    if (hipMalloc(&c->d_bitmap, cap * 8) != hipSuccess) return set_err(PBFT_ENOMEM, "bitmap alloc");
    if (hipHostMalloc(&c->h_bitmap, cap * 8, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
      return set_err(PBFT_ENOMEM, "pinned bitmap alloc");
    HIP_TRY(hipHostGetDevicePointer((void**)&c->h_bitmap_dev, c->h_bitmap, 0));
    c->bitmap_cap = cap;
  }
  return PBFT_OK;
}

// Grow the verify workspace (never inside a stream capture: call
// pbft_verify_reserve first when capturing launches into a graph).
// Workspace per launch of N signatures (Npad = N rounded up to BLOCK):
//   xyz   [30][N] u32   R' limbs, comb -> finish            120 B/sig
//   flags [N] u8                                              1 B/sig
//   eidx  [steps][Npad] u32  per-step table entry indices    4 x steps B/sig
static constexpr int MAX_STEPS = steps<PLB, PLA_SMALL>::N;  // the smallest key plan has the most steps
static_assert(steps<PLB, PLA_SMALL>::N >= steps<PLB, PLA_MID>::N && steps<PLB, PLA_MID>::N >= steps<PLB, PLA_BIG>::N,
              "");
static inline size_t eidx_offset(uint64_t N) { return (121 * (size_t)N + 255) & ~(size_t)255; }
static inline size_t eidx_bytes(uint64_t N) {
  const uint64_t Npad = (N + 2 * BLOCK - 1) / (2 * BLOCK) * (2 * BLOCK);  // (8-wave comb blocks: PBFT_OPT_COMB_PRIO)
  // (latency mode: 4 or 8 lanes per signature, 8-byte entry addresses, ceil(steps / lanes) per lane)
  const size_t split4 = 8 * (size_t)((MAX_STEPS + 3) / 4) * (Npad * 4 + BLOCK);
  const size_t split8 = 8 * (size_t)((MAX_STEPS + 7) / 8) * (Npad * 8 + BLOCK);
  const size_t split = split4 > split8 ? split4 : split8;
  const size_t comb = 4 * (size_t)MAX_STEPS * Npad;
  return ((comb > split ? comb : split) + 255) & ~(size_t)255;
}
// PBFT_LAUNCH_TRACE=1: every HIP call of a votes chunk launch that blocks the host for more than 0.3 ms is reported
// on stderr (the replica's flush timeline showed 6-7 ms stalls inside pbft_verify_votes_submit_rows)
// (PBFT_LAUNCH_TRACE=<n> with n > 1: report calls longer than n microseconds instead)
static double launch_trace_ms() {
  static const double ms = [] {
    const char* e = getenv("PBFT_LAUNCH_TRACE");
    if (!e) return -1.0;
    const double v = strtod(e, nullptr);
    return v > 1 ? v / 1000.0 : 0.3;
  }();
  return ms;
}
static bool launch_trace() { return launch_trace_ms() >= 0; }
#define LT(name, ...)                                                                                              \
  do {                                                                                                             \
    const auto lt_t0 = std::chrono::steady_clock::now();                                                           \
    __VA_ARGS__;                                                                                                   \
    if (launch_trace()) {                                                                                          \
      const double lt_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - lt_t0).count(); \
      if (lt_ms > launch_trace_ms())                                                                            \
        fprintf(stderr, "launch-stall %s chunk %u: %.3f ms\n", name, (unsigned)c->v_chunk, lt_ms);             \
    }                                                                                                              \
  } while (0)

// second xyz/flags half (pipelined form) after the entry-index region
static inline size_t half1_offset(uint64_t N) { return eidx_offset(N) + eidx_bytes(N); }
// the whole workspace: half 0, the entry indices and (pipelined form) half 1
static inline size_t work_bytes(uint64_t W, bool two) {
  return ((two ? half1_offset(W) + eidx_offset(W) : half1_offset(W)) + 255) & ~(size_t)255;
}
// The layout is a function of c->work_n only, never of the batch at hand: a smaller batch must not move
// the entry-index region onto the xyz/flags half a pipelined finish may still be reading.
static int ensure_work(pbft_ctx* c, uint64_t N, bool two_halves = false) {
  if (N <= c->work_n && (!two_halves || c->work_two)) return PBFT_OK;
  const uint64_t W = N > c->work_n ? N : c->work_n;
  const bool two = two_halves || c->work_two;
  const size_t need = work_bytes(W, two);
  // nothing may still read the old workspace: the finishes of earlier pipelined launches, then this stream
  for (int h = 0; h < 2; ++h)
    if (c->fin_pending[h]) { HIP_TRY(hipEventSynchronize(c->ev_fin[h])); c->fin_pending[h] = false; }
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (c->d_work) HIP_TRY(hipDeviceSynchronize());  // a device-form launch may run on a caller's stream
  if (c->d_work) HIP_TRY(hipFree(c->d_work));
  c->d_work = nullptr;
  c->work_cap = 0;
  c->work_n = 0;
  c->work_two = false;
  if (hipMalloc(&c->d_work, need) != hipSuccess) return set_err(PBFT_ENOMEM, "verify workspace alloc");
  c->work_cap = need;
  c->work_n = W;
  c->work_two = two;
  return PBFT_OK;
}

// The second workspace (votes chunks on stream2): one half, same layout.
static int ensure_work2(pbft_ctx* c, uint64_t N) {
  if (N <= c->work2_n) return PBFT_OK;
  const uint64_t W = N;
  const size_t need = work_bytes(W, false);
  if (c->d_work2) {
    HIP_TRY(hipStreamSynchronize(c->stream2));
    HIP_TRY(hipFree(c->d_work2));
  }
  c->d_work2 = nullptr;
  c->work2_cap = 0;
  c->work2_n = 0;
  if (hipMalloc(&c->d_work2, need) != hipSuccess) return set_err(PBFT_ENOMEM, "verify workspace alloc");
  c->work2_cap = need;
  c->work2_n = W;
  return PBFT_OK;
}

// The finish behind a one-lane-per-signature kernel (the comb, or anykey_kernel): signatures per finish lane, product
// tree and waves per SIMD by batch size (PBFT_FIN_* above).
static hipError_t launch_finish_by_n(const pbft_ctx* c, const uint8_t* dR, uint32_t rs_stride, const uint32_t* xyz,
                                     const uint8_t* flags, uint64_t N, uint64_t* dB, hipStream_t st) {
  const bool big = N >= ((uint64_t)1 << 19);
  int fm = big ? PBFT_FIN_FM_BIG : N > PBFT_FIN_SMALL_UPTO ? PBFT_FIN_FM_MID
                                 : N > PBFT_FIN_TINY_UPTO  ? PBFT_FIN_FM_SMALL : 1;
  // cross-lane product tree (one variable-time inversion per 16-lane row since r04, per wave before) where few
  // signatures share a lane: 131k 0.2106 -> 0.2061 ms at fm 4, 0.2467 -> 0.2160 at fm 1; no gain at fm 16
  // (profiles/r02_ab_log.md); lv is a flag here, finish.hip compiles the tree depth (PBFT_FIN_LV)
  int lv = fm <= PBFT_FIN_TREE_MAX_FM ? PBFT_FIN_LV : 0;
  if (c->fin_m) fm = c->fin_m;
  if (c->fin_tree >= 0) lv = c->fin_tree;
  const int fw = c->fin_waves ? c->fin_waves : (big ? PBFT_FIN_W_BIG : 1);
  return launch_finish(fm, lv, fw, dR, rs_stride, xyz, flags, N, dB, st);
}

// fst != null: pipelined form -- the finish runs on fst after an event, on one of two
// workspace halves, so the next launch's comb (on st) overlaps it.  slot 1: the second workspace (votes chunks
// on stream2; no timing events, never pipelined).
static int launch_verify(pbft_ctx* c, const uint8_t* dR, const uint8_t* dS, const uint16_t* dK, const uint8_t* dM,
                         uint32_t msg_len, uint32_t msg_stride, uint64_t N, uint64_t* dB, hipStream_t st,
                         uint32_t rs_stride = 32, uint32_t k_stride = 2, hipStream_t fst = nullptr,
                         const uint32_t* dMI = nullptr, uint32_t n_msg = 0, const uint64_t* dWK = nullptr,
                         uint32_t mi_stride = 1, int slot = 0) {
  if (N == 0) return PBFT_OK;
  const uint64_t blocks = (N + BLOCK - 1) / BLOCK;
  if (blocks > 0x7fffffffull) return set_err(PBFT_EINVAL, "N too large for one launch");
  int rc = slot ? ensure_work2(c, N) : ensure_work(c, N, fst != nullptr);
  if (rc) return rc;
  uint8_t* const wbase = slot ? c->d_work2 : c->d_work;
  const bool timing = c->timing && slot == 0;
  int h = 0;
  if (fst) {
    h = c->half;
    c->half ^= 1;
  }
  if (slot == 0 && c->fin_pending[h]) HIP_TRY(hipStreamWaitEvent(st, c->ev_fin[h], 0));  // a pipelined finish still reading half h
  if (timing) LT("rec_ev0", HIP_TRY(hipEventRecord(c->ev0, st)));
  const uint64_t W = slot ? c->work2_n : c->work_n;  // layout (>= N)
  uint8_t* hw = wbase + (h ? half1_offset(W) : 0);
  const bool latency_mode = N < c->split_below;
  comb_launch_args a;
  a.R = dR; a.S = dS; a.K = (const uint8_t*)dK; a.rs_stride = rs_stride; a.k_stride = k_stride;
  a.M = dM; a.msg_len = msg_len; a.msg_stride = msg_stride; a.N = N;
  a.tabB = c->d_tabB; a.tabA = c->d_tabA; a.keys = c->d_keys; a.key_ok = c->d_key_ok; a.n_keys = c->n_keys;
  a.xyz = (uint32_t*)hw;
  a.flags = hw + 120 * N;  // within the half's 121 W bytes
  a.eidx = (uint32_t*)(wbase + eidx_offset(W));
  a.bitmap = dB; a.msg_idx = dMI; a.n_msg = n_msg; a.mi_stride = mi_stride; a.latency_mode = latency_mode; a.lat_split = c->lat_split; a.st = st;
  a.pair = c->comb_pair;
  a.cus = c->cus;
  a.prio = c->comb_prio;
  a.balance = c->comb_balance;
  a.wk = (PBFT_ENV_SCHED && dMI && msg_len == PBFT_ENVELOPE_LEN) ? dWK : nullptr;
  uint32_t* xyz = a.xyz;
  uint8_t* flags = a.flags;
  LT("comb", HIP_TRY(c->pa == PLA_HUGE::P  ? launch_comb_huge(a)
                     : c->pa == PLA_BIG::P ? launch_comb_big(a)
                     : c->pa == PLA_MID::P ? launch_comb_mid(a)
                                           : launch_comb_small(a)));
  HIP_TRY(hipGetLastError());
  if (fst) {
    if (timing) HIP_TRY(hipEventRecord(c->ev1, st));  // pipelined form: last_kernel_ms = the comb (or latency) kernel
    HIP_TRY(hipEventRecord(c->ev_comb, st));
    HIP_TRY(hipStreamWaitEvent(fst, c->ev_comb, 0));
    st = fst;
  }
  if (!latency_mode) {  // (the latency kernel writes the bitmap itself)
    LT("finish", HIP_TRY(launch_finish_by_n(c, dR, rs_stride, xyz, flags, N, dB, st)));
    HIP_TRY(hipGetLastError());
  }
  if (fst) {
    HIP_TRY(hipEventRecord(c->ev_fin[h], fst));
    c->fin_pending[h] = true;
    return PBFT_OK;
  }
  if (timing) LT("rec_ev1", HIP_TRY(hipEventRecord(c->ev1, st)));
  return PBFT_OK;
}

static bool check_batch_args(const void* R, const void* S, const void* K, const void* M, uint32_t msg_len,
                             uint32_t msg_stride, uint64_t N, const void* out) {
  if (N == 0) return out != nullptr || true;
  if (!R || !S || !K || !out) return false;
  if (msg_len > 0 && !M) return false;
  if (msg_stride < msg_len) return false;
  if (msg_len > (1u << 24)) return false;
  return true;
}

// Staging layout of n signatures: R | S | key_idx | msg (+ slack for unaligned message reads).
struct stage_layout {
  size_t offS, offK, offM, bytes;
  stage_layout(uint64_t n, uint32_t msg_stride) {
    offS = 32 * n;
    offK = 64 * n;
    offM = (offK + 2 * n + 255) & ~(size_t)255;
    bytes = (offM + (size_t)msg_stride * n + 64 + 255) & ~(size_t)255;
  }
};

// Host batches above this many signatures are copied and verified in chunks on two
// staging halves: the H2D copy of chunk c+1 (context copy stream) overlaps the
// kernels of chunk c (context stream).  A multiple of 64: chunks own whole
// bitmap words.  2^18 keeps every chunk in the one-lane-per-signature mode.
#ifndef PBFT_PIPE_CHUNK_LOG2
#define PBFT_PIPE_CHUNK_LOG2 18
#endif
#define PBFT_VOTES_CHUNK_LOG2 18  // PBFT_VOTES_CHUNK_ROWS (include/pbft_verify.h: the replica follows the schedule)
static_assert(PBFT_VOTES_CHUNK_ROWS == (1u << PBFT_VOTES_CHUNK_LOG2) && PBFT_VOTES_FIRST_ROWS % 64 == 0, "");
// chunks own whole 64-bit bitmap words (the kernels write d_bitmap + lo / 64, readbacks copy (n + 63) / 64 words)
static_assert(PBFT_PIPE_CHUNK_LOG2 >= 6 && PBFT_VOTES_CHUNK_LOG2 >= 6, "chunks must be multiples of 64 rows");
static constexpr uint64_t PIPE_CHUNK = 1ull << PBFT_PIPE_CHUNK_LOG2;
// the votes form moves 70 B per signature instead of 151: its copies are about as long as the kernels, so a
// smaller chunk shortens the pipeline's fill and drain (PBFT_VOTES_CHUNK_LOG2)
static constexpr uint64_t VOTES_CHUNK = 1ull << PBFT_VOTES_CHUNK_LOG2;

// Copy a host batch into the staging buffer and launch.  Result: the device bitmap.
static int stage_and_launch(pbft_ctx* c, const uint8_t* R, const uint8_t* S, const uint16_t* K, const uint8_t* M,
                            uint32_t msg_len, uint32_t msg_stride, uint64_t N) {
  const uint64_t words = (N + 63) / 64;
  if (N <= PIPE_CHUNK) {
    const stage_layout L(N, msg_stride);
    int rc = ensure_stage(c, L.bytes, words);
    if (rc) return rc;
    const uint8_t* src[4] = {R, S, (const uint8_t*)K, M};
    const uint64_t off[4] = {0, L.offS, L.offK, L.offM};
    const uint64_t len[4] = {32 * N, 32 * N, 2 * N, (uint64_t)msg_stride * N};
    bool imported = false;
    LT("import", imported = launch_import(src, off, len, 4, c->d_stage, c->stream));
    if (imported) {
      HIP_TRY(hipGetLastError());
    } else {
      LT("h2d_R", HIP_TRY(hipMemcpyAsync(c->d_stage, R, 32 * N, hipMemcpyHostToDevice, c->stream)));
      LT("h2d_S", HIP_TRY(hipMemcpyAsync(c->d_stage + L.offS, S, 32 * N, hipMemcpyHostToDevice, c->stream)));
      LT("h2d_K", HIP_TRY(hipMemcpyAsync(c->d_stage + L.offK, K, 2 * N, hipMemcpyHostToDevice, c->stream)));
      if ((size_t)msg_stride * N)
        LT("h2d_M", HIP_TRY(hipMemcpyAsync(c->d_stage + L.offM, M, (size_t)msg_stride * N, hipMemcpyHostToDevice,
                                           c->stream)));
    }
    return launch_verify(c, c->d_stage, c->d_stage + L.offS, (const uint16_t*)(c->d_stage + L.offK),
                         c->d_stage + L.offM, msg_len, msg_stride, N, c->d_bitmap, c->stream);
  }
  const stage_layout L(PIPE_CHUNK, msg_stride);
  int rc = ensure_stage(c, 2 * L.bytes, words);
  if (rc) return rc;
  uint64_t chunk = 0;
  for (uint64_t lo = 0; lo < N; lo += PIPE_CHUNK, ++chunk) {
    const uint64_t n = N - lo < PIPE_CHUNK ? N - lo : PIPE_CHUNK;
    const int b = (int)(chunk & 1);
    uint8_t* base = c->d_stage + (size_t)b * L.bytes;
    if (chunk >= 2) HIP_TRY(hipStreamWaitEvent(c->cstream, c->ev_consumed[b], 0));  // kernels of chunk-2 done
    HIP_TRY(hipMemcpyAsync(base, R + 32 * lo, 32 * n, hipMemcpyHostToDevice, c->cstream));
    HIP_TRY(hipMemcpyAsync(base + L.offS, S + 32 * lo, 32 * n, hipMemcpyHostToDevice, c->cstream));
    HIP_TRY(hipMemcpyAsync(base + L.offK, K + lo, 2 * n, hipMemcpyHostToDevice, c->cstream));
    if ((size_t)msg_stride * n)
      HIP_TRY(hipMemcpyAsync(base + L.offM, M + (size_t)msg_stride * lo, (size_t)msg_stride * n,
                             hipMemcpyHostToDevice, c->cstream));
    HIP_TRY(hipEventRecord(c->ev_copied[b], c->cstream));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_copied[b], 0));
    rc = launch_verify(c, base, base + L.offS, (const uint16_t*)(base + L.offK), base + L.offM, msg_len, msg_stride,
                       n, c->d_bitmap + lo / 64, c->stream);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(c->ev_consumed[b], c->stream));
  }
  return PBFT_OK;
}

// Votes form, once per call: the block-2 SHA-512 schedule of every 85-byte envelope (sha512.h
// sha512_env_sched), read by each signature's challenge hash instead of expanding it again.
__global__ void __launch_bounds__(BLOCK) env_sched_kernel(const uint8_t* __restrict__ env, uint32_t n_env,
                                                          uint64_t* __restrict__ wk) {
  const uint64_t e = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (e >= n_env) return;
  sha512_env_sched(wk + (size_t)SHA_ENV_WORDS * e, env + (size_t)PBFT_ENVELOPE_LEN * e);
}

// (the buffer grows on first use for a bigger table: not inside a stream capture)
static int ensure_wk(pbft_ctx* c, uint32_t n_env) {
  if (n_env > c->wk_cap) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->d_wk) {
      HIP_TRY(hipDeviceSynchronize());  // a device-form launch may still read it on a caller's stream
      HIP_TRY(hipFree(c->d_wk));
    }
    c->d_wk = nullptr;
    c->wk_cap = 0;
    if (hipMalloc(&c->d_wk, (size_t)SHA_ENV_WORDS * 8 * n_env) != hipSuccess)
      return set_err(PBFT_ENOMEM, "envelope schedule alloc");
    c->wk_cap = n_env;
  }
  return PBFT_OK;
}
static int prepare_env_sched(pbft_ctx* c, const uint8_t* dENV, uint32_t n_env, hipStream_t st, const uint64_t** out) {
  int rc = ensure_wk(c, n_env);
  if (rc) return rc;
  hipLaunchKernelGGL(env_sched_kernel, dim3((n_env + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, st, dENV, n_env, c->d_wk);
  HIP_TRY(hipGetLastError());
  *out = c->d_wk;
  return PBFT_OK;
}

// Votes form (include/pbft_verify.h pbft_verify_votes): R, S, key_idx and a 4-byte envelope index per
// signature (70 B instead of 151 B over PCIe; 72 B as staged rows) + the batch's table of distinct 85-byte
// envelopes.
// One chunk's device staging: R | S | key_idx | env_idx columns (caller columns), or the chunk's rows as staged
// (PBFT_VOTES_ROW_BYTES each, one copy).
struct votes_layout {
  size_t offS, offK, offI, bytes;
  explicit votes_layout(uint64_t n) {
    offS = 32 * n;
    offK = 64 * n;
    offI = (offK + 2 * n + 15) & ~(size_t)15;
    const size_t cols = (offI + 4 * n + 255) & ~(size_t)255, rows = (ROW * (size_t)n + 255) & ~(size_t)255;
    bytes = cols > rows ? cols : rows;
  }
};

// The kernels' address of [p, p + bytes) in the context's mapped staging, else null.
static const uint8_t* zc_map(const pbft_ctx* c, const void* p, size_t bytes) {
  const uint8_t* q = (const uint8_t*)p;
  if (!c->h_stage_dev || q < c->h_stage || q + bytes > c->h_stage + c->h_stage_cap) return nullptr;
  return c->h_stage_dev + (q - c->h_stage);
}

// rs_stride 32: R and S are separate [N][32] host columns (key_idx, env_idx columns too); PBFT_VOTES_ROW_BYTES: R
// = the staged rows (S = R + 32, key_idx at + 64, env_idx at + 68 of each row).
// votes_begin copies the envelope table and launches its schedule; votes_launch then launches every whole chunk
// inside rows [0, rows) (all the rest once rows >= N): the kernels of chunk c run on the context stream after
// its copies (copy stream), overlapping the copies of chunk c+1.
// Chunk schedule of a votes batch: PBFT_VOTES_CHUNK_END, or (v_short_tail: rows that are all in host memory when
// the batch starts, pbft_verify_votes_submit_host) the same with its last chunk cut down to ~VOTES_TAIL rows -- what
// is left once the last copy lands is that chunk's kernels and the caller's application of its rows
// (r05: the replica's flush ended with 64k rows of both).
static constexpr uint64_t VOTES_TAIL = 16384;
static uint64_t votes_chunk_end(const pbft_ctx* c, uint64_t lo, uint64_t N) {
  const uint64_t e = PBFT_VOTES_CHUNK_END(lo, N);
  if (c->v_short_tail && e == N && N > VOTES_CHUNK && N - lo > VOTES_TAIL + 64) return lo + ((N - lo - VOTES_TAIL) & ~(uint64_t)63);
  return e;
}

static int votes_begin(pbft_ctx* c, const uint8_t* ENV, uint32_t n_env, uint64_t N, bool readback,
                       bool short_tail = false) {
  c->v_short_tail = short_tail;
  c->v_env_cap = 0;  // (not a batch in pieces)
  c->v_ends.clear();
  const uint64_t words = (N + 63) / 64;
  const size_t env_bytes = ((size_t)PBFT_ENVELOPE_LEN * n_env + 64 + 255) & ~(size_t)255;  // + read slack
  const uint64_t ch = N < VOTES_CHUNK ? N : VOTES_CHUNK;
  const votes_layout L(ch);
  int rc = ensure_stage(c, env_bytes + (N > VOTES_CHUNK ? VOTES_BUFS : 1) * L.bytes, words);
  if (rc) return rc;
  // more than one chunk: odd chunks' kernels on stream2 (their own workspace), so consecutive chunks' kernels may
  // overlap -- the small first chunks and the last big one leave most of the GPU idle on one stream
  const bool two = c->two_streams && N > PBFT_VOTES_FIRST_ROWS;
  if (two && !c->stream2) {
    HIP_TRY(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&c->ev_env, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&c->ev_s2, hipEventDisableTiming));
  }
  if (readback) {
    uint64_t chunks = 0;
    for (uint64_t lo = 0; lo < N; lo = votes_chunk_end(c, lo, N)) ++chunks;
    while (c->ev_rows.size() < chunks) {
      hipEvent_t e;
      HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      c->ev_rows.push_back(e);
    }
  }
  const size_t env_len = (size_t)PBFT_ENVELOPE_LEN * n_env;
  const uint8_t* zenv = zc_map(c, ENV, env_len + 15);
  if (zenv && ((uintptr_t)zenv & 15) == 0) {  // the table sits in the mapped staging: copied by a kernel
    const uint64_t n16 = (env_len + 15) / 16;
    hipLaunchKernelGGL(import16_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, c->stream,
                       (const uint4*)zenv, (uint4*)c->d_stage, n16);
    LT("import_env", HIP_TRY(hipGetLastError()));
  } else {
    LT("h2d_env", HIP_TRY(hipMemcpyAsync(c->d_stage, ENV, env_len, hipMemcpyHostToDevice, c->cstream)));
    // the envelopes' block-2 schedule on the context stream once the table has landed (ev_copied[0] is
    // re-recorded by chunk 0)
    LT("rec_env", HIP_TRY(hipEventRecord(c->ev_copied[0], c->cstream)));
    LT("wait_env", HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_copied[0], 0)));
  }
  LT("env_sched", rc = prepare_env_sched(c, c->d_stage, n_env, c->stream, &c->v_wk));
  if (rc) return rc;
  // stream2's chunks read the envelope table and its schedule too (it waits at its first chunk: votes_launch)
  if (two) HIP_TRY(hipEventRecord(c->ev_env, c->stream));
  c->v_s2_ready = false;
  c->v_two = two;
  c->v_n = N;
  c->v_next = 0;
  c->v_chunk = 0;
  c->v_env_bytes = env_bytes;
  c->v_env = n_env;
  c->v_open = true;
  c->v_readback = readback;
  c->rows_out = 0;
  c->chunk_out = 0;
  return PBFT_OK;
}

// One chunk of a votes batch: rows [lo, lo + n) -- their copy (or the mapped staging read in place), the kernels
// on the chunk's stream, its bitmap words back (progressive form) -- then v_next / v_chunk advance.
static int votes_chunk(pbft_ctx* c, const uint8_t* R, const uint8_t* S, const uint16_t* K, const uint32_t* IDX,
                       uint32_t rs_stride, uint64_t lo, uint64_t n) {
  const uint64_t N = c->v_n;
  const votes_layout L(N < VOTES_CHUNK ? N : VOTES_CHUNK);
  const int b = (int)(c->v_chunk % VOTES_BUFS);
  const int slot = c->v_two ? (int)(c->v_chunk & 1) : 0;
  hipStream_t st = slot ? c->stream2 : c->stream;
  if (slot && !c->v_s2_ready) {
    LT("wait_env2", HIP_TRY(hipStreamWaitEvent(c->stream2, c->ev_env, 0)));
    c->v_s2_ready = true;
  }
  if (c->v_readback && c->ev_rows.size() <= c->v_chunk) {  // (pieces: the chunk count is not known up front)
    hipEvent_t e;
    HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    c->ev_rows.push_back(e);
  }
  c->v_ends.push_back(lo + n);
  const bool rows_form = rs_stride == ROW;
  const uint32_t ks = rows_form ? ROW : 2, mis = rows_form ? ROW / 4 : 1;
  uint8_t* base = c->d_stage + c->v_env_bytes + (size_t)b * L.bytes;
  if (c->v_chunk >= VOTES_BUFS) LT("wait_consumed", HIP_TRY(hipStreamWaitEvent(c->cstream, c->ev_consumed[b], 0)));
  if (rows_form) {  // the chunk's rows: one copy
    LT("h2d_rows", HIP_TRY(hipMemcpyAsync(base, R + (size_t)ROW * lo, (size_t)ROW * n, hipMemcpyHostToDevice,
                                          c->cstream)));
  } else {
    HIP_TRY(hipMemcpyAsync(base, R + 32 * lo, 32 * n, hipMemcpyHostToDevice, c->cstream));
    HIP_TRY(hipMemcpyAsync(base + L.offS, S + 32 * lo, 32 * n, hipMemcpyHostToDevice, c->cstream));
    LT("h2d_key", HIP_TRY(hipMemcpyAsync(base + L.offK, K + lo, 2 * n, hipMemcpyHostToDevice, c->cstream)));
    LT("h2d_idx", HIP_TRY(hipMemcpyAsync(base + L.offI, IDX + lo, 4 * n, hipMemcpyHostToDevice, c->cstream)));
  }
  LT("rec_copied", HIP_TRY(hipEventRecord(c->ev_copied[b], c->cstream)));
  LT("wait_copied", HIP_TRY(hipStreamWaitEvent(st, c->ev_copied[b], 0)));
  int rc = 0;
  LT("kernels", rc = launch_verify(c, base, base + (rows_form ? 32 : L.offS),
                                   (const uint16_t*)(base + (rows_form ? PBFT_VOTES_ROW_KEY : L.offK)), c->d_stage,
                                   PBFT_ENVELOPE_LEN, PBFT_ENVELOPE_LEN, n, c->d_bitmap + lo / 64, st,
                                   rs_stride, ks, nullptr,
                                   (const uint32_t*)(base + (rows_form ? PBFT_VOTES_ROW_ENV : L.offI)), c->v_env,
                                   c->v_wk, mis, slot));
  if (rc) return rc;
  // pbft_verify_votes_tally: the chunk's rows join the batch's signer sets while its columns are still in the
  // staging buffer (lo is a multiple of 64: the chunk's bitmap words are its own)
  if (c->t_signers)
    LT("tally", HIP_TRY(launch_tally(c->d_bitmap + lo / 64, base + (rows_form ? PBFT_VOTES_ROW_KEY : L.offK), ks,
                                     base + (rows_form ? PBFT_VOTES_ROW_ENV : L.offI), 4 * mis, n, c->v_env,
                                     c->n_keys, c->t_signers, st)));
  LT("rec_consumed", HIP_TRY(hipEventRecord(c->ev_consumed[b], st)));
  if (c->v_readback) {  // this chunk's bitmap words (a few KB) back on their own, for the caller to apply early
    LT("export_bitmap", HIP_TRY(export_words(c, lo / 64, (n + 63) / 64, st)));
    LT("rec_rows", HIP_TRY(hipEventRecord(c->ev_rows[c->v_chunk], st)));
  }
  c->v_next += n;
  ++c->v_chunk;
  return PBFT_OK;
}

// The context stream (ev_done, the final bitmap export) follows stream2's last chunk too
static int votes_join_streams(pbft_ctx* c) {
  if (c->v_two) {
    HIP_TRY(hipEventRecord(c->ev_s2, c->stream2));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_s2, 0));
  }
  return PBFT_OK;
}

static int votes_launch(pbft_ctx* c, const uint8_t* R, const uint8_t* S, const uint16_t* K, const uint32_t* IDX,
                        uint32_t rs_stride, uint64_t rows) {
  const uint64_t N = c->v_n;
  while (c->v_next < N && (rows >= N || votes_chunk_end(c, c->v_next, N) <= rows)) {
    const uint64_t lo = c->v_next;
    const int rc = votes_chunk(c, R, S, K, IDX, rs_stride, lo, votes_chunk_end(c, lo, N) - lo);
    if (rc) return rc;
  }
  if (c->v_next >= N) {
    c->v_open = false;
    return votes_join_streams(c);
  }
  return PBFT_OK;
}

static int stage_votes_and_launch(pbft_ctx* c, const uint8_t* R, const uint8_t* S, const uint16_t* K,
                                  const uint32_t* IDX, const uint8_t* ENV, uint32_t n_env, uint64_t N,
                                  uint32_t rs_stride = 32) {
  int rc = votes_begin(c, ENV, n_env, N, false);
  if (rc) return rc;
  rc = votes_launch(c, R, S, K, IDX, rs_stride, N);
  c->v_open = false;
  return rc;
}

// The base-point comb table is a constant of the curve: one copy per device,
// shared by every context on it (reference-counted; 30 GB with the default plan).
static std::mutex g_tabB_mu;
static uint32_t* g_tabB[64] = {};
static int g_tabB_refs[64] = {};

static int acquire_base_table(int device, hipStream_t st, uint32_t** out) {
  std::lock_guard<std::mutex> lk(g_tabB_mu);
  if (device < 0 || device >= 64) return set_err(PBFT_ENODEV, "device ordinal >= 64");
  if (!g_tabB[device]) {
    // base point B = (x, 4/5), x even
    const uint32_t benc[8] = {0x66666658u, 0x66666666u, 0x66666666u, 0x66666666u,
                              0x66666666u, 0x66666666u, 0x66666666u, 0x66666666u};
    uint32_t* d_benc = nullptr;
    uint32_t* tab = nullptr;
    HIP_TRY(hipMalloc(&d_benc, 32));
    if (hipMalloc(&tab, PLB::TABLE_WORDS * 4) != hipSuccess) {
      (void)hipFree(d_benc);
      return set_err(PBFT_ENOMEM, "base-point table alloc");
    }
    HIP_TRY(hipMemcpyAsync(d_benc, benc, 32, hipMemcpyHostToDevice, st));
    int rc = build_comb_tables(0, d_benc, 1u, 0, tab, nullptr, st) == hipSuccess ? PBFT_OK : set_err(PBFT_EHIP, "base table build");
    (void)hipFree(d_benc);
    if (rc) { (void)hipFree(tab); return rc; }
    g_tabB[device] = tab;
  }
  ++g_tabB_refs[device];
  *out = g_tabB[device];
  return PBFT_OK;
}

static void release_base_table(int device) {
  std::lock_guard<std::mutex> lk(g_tabB_mu);
  if (device < 0 || device >= 64 || g_tabB_refs[device] == 0) return;
  if (--g_tabB_refs[device] == 0) {
    (void)hipFree(g_tabB[device]);
    g_tabB[device] = nullptr;
  }
}

extern "C" {

const char* pbft_last_error(void) { return g_last_error.c_str(); }

const char* pbft_build_info(void) {
  static char buf[256];
  snprintf(buf, sizeof buf,
           "pbft_verify gfx950 PB=%d PA=%d|%d|%d|%d block=%d entry=128B tabB=%zuB tabA/key=%zuB|%zuB|%zuB|%zuB",
           PLB::P, PLA_HUGE::P, PLA_BIG::P, PLA_MID::P, PLA_SMALL::P, BLOCK, PLB::TABLE_WORDS * 4,
           PLA_HUGE::TABLE_WORDS * 4, PLA_BIG::TABLE_WORDS * 4, PLA_MID::TABLE_WORDS * 4, PLA_SMALL::TABLE_WORDS * 4);
  return buf;
}

int pbft_verify_ctx_create(int device, pbft_ctx** out) {
  if (!out) return set_err(PBFT_EINVAL, "out is null");
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
    return set_err(PBFT_ENODEV, "no HIP device at that ordinal");
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    char b[128];
    snprintf(b, sizeof b, "device %d is %s, this library is built for gfx950", device, prop.gcnArchName);
    return set_err(PBFT_ENODEV, b);
  }
  HIP_TRY(hipSetDevice(device));
  pbft_ctx* c = new pbft_ctx();
  c->device = device;
  c->cus = prop.multiProcessorCount;
  if (const char* e = getenv("PBFT_COMB_PRIO")) {
    const long v = strtol(e, nullptr, 10);
    c->comb_prio = (v == 0 || v == 1) ? (int)v : -1;
  }
  HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  if (const char* e = getenv("PBFT_SPLIT_BELOW")) c->split_below = strtoull(e, nullptr, 10);
  if (const char* e = getenv("PBFT_VOTES_TWO_STREAMS")) c->two_streams = strtol(e, nullptr, 10) != 0;
  if (const char* e = getenv("PBFT_COMB_PAIR")) {
    const long v = strtol(e, nullptr, 10);
    c->comb_pair = (v == 0 || v == 1) ? (int)v : -1;
  }
  HIP_TRY(hipEventCreate(&c->ev0));
  HIP_TRY(hipEventCreate(&c->ev1));
  HIP_TRY(hipEventCreateWithFlags(&c->ev_done, hipEventDisableTiming));
  HIP_TRY(hipStreamCreateWithFlags(&c->cstream, hipStreamNonBlocking));
  HIP_TRY(hipEventCreateWithFlags(&c->ev_comb, hipEventDisableTiming));
  for (int b = 0; b < 2; ++b) HIP_TRY(hipEventCreateWithFlags(&c->ev_fin[b], hipEventDisableTiming));
  for (int b = 0; b < VOTES_BUFS; ++b) {
    HIP_TRY(hipEventCreateWithFlags(&c->ev_copied[b], hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&c->ev_consumed[b], hipEventDisableTiming));
  }
  int rc = acquire_base_table(device, c->stream, &c->d_tabB);
  if (rc) {
    (void)hipEventDestroy(c->ev0); (void)hipEventDestroy(c->ev1); (void)hipEventDestroy(c->ev_done);
    for (int b = 0; b < 2; ++b) (void)hipEventDestroy(c->ev_fin[b]);
    for (int b = 0; b < VOTES_BUFS; ++b) { (void)hipEventDestroy(c->ev_copied[b]); (void)hipEventDestroy(c->ev_consumed[b]); }
    (void)hipEventDestroy(c->ev_comb);
    (void)hipStreamDestroy(c->cstream);
    (void)hipStreamDestroy(c->stream);
    delete c;
    return rc;
  }
  *out = c;
  return PBFT_OK;
}

int pbft_verify_ctx_destroy(pbft_ctx* c) {
  if (!c) return PBFT_OK;
  // teardown: errors are ignored (nothing useful to report from a destructor)
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  release_base_table(c->device);
  c->adopt(nullptr);
  (void)hipFree(c->d_stage); (void)hipFree(c->d_bitmap); (void)hipFree(c->d_work); (void)hipFree(c->d_wk);
  (void)hipFree(c->d_tally);
  (void)hipFree(c->d_fpatch);
  (void)hipFree(c->d_group);
  (void)hipFree(c->d_index);
  (void)hipFree(c->d_admit);
  if (c->d_sign_key) {
    (void)hipMemset(c->d_sign_key, 0, 4 * EGRESS_KEY_WORDS);
    (void)hipFree(c->d_sign_key);
  }
  (void)hipFree(c->d_egress);
  (void)hipFree(c->d_propose);
  (void)hipFree(c->d_reply);
  (void)hipFree(c->d_sign_io);
  (void)hipFree(c->d_accept_pid);
  (void)hipFree(c->d_accept_io);
  (void)hipFree(c->d_accept_patch);
  if (c->h_bitmap) (void)hipHostFree(c->h_bitmap);
  if (c->h_stage) (void)hipHostFree(c->h_stage);
  if (c->ev0) (void)hipEventDestroy(c->ev0);
  if (c->ev1) (void)hipEventDestroy(c->ev1);
  if (c->ev_done) (void)hipEventDestroy(c->ev_done);
  for (int b = 0; b < 2; ++b) {
    if (c->fin_pending[b]) (void)hipEventSynchronize(c->ev_fin[b]);
    if (c->ev_fin[b]) (void)hipEventDestroy(c->ev_fin[b]);
  }
  for (int b = 0; b < VOTES_BUFS; ++b) {
    if (c->ev_copied[b]) (void)hipEventDestroy(c->ev_copied[b]);
    if (c->ev_consumed[b]) (void)hipEventDestroy(c->ev_consumed[b]);
  }
  if (c->stream2) { (void)hipStreamSynchronize(c->stream2); (void)hipStreamDestroy(c->stream2); }
  if (c->ev_env) (void)hipEventDestroy(c->ev_env);
  if (c->ev_s2) (void)hipEventDestroy(c->ev_s2);
  (void)hipFree(c->d_work2);
  if (c->ev_comb) (void)hipEventDestroy(c->ev_comb);
  for (hipEvent_t e : c->ev_rows) (void)hipEventDestroy(e);
  if (c->ev_envp) (void)hipEventDestroy(c->ev_envp);
  if (c->cstream) { (void)hipStreamSynchronize(c->cstream); (void)hipStreamDestroy(c->cstream); }
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
  return PBFT_OK;
}

static double ms_since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// Install a key set.  Where the time of a re-key went: hipMalloc itself is ~0.3 ms even for
// 172 GB, but VRAM that was written and then freed is wiped by the driver (~22 GB/s, tools/microbench/alloc_h2d:
// re-allocating 202 GB right after freeing it took 9.3 s) and the next allocation waits for that -- a plan change
// that freed 69 GB of tables paid 6.2 s in hipMalloc, the table build itself ~0.25 s.  So a key set whose tables
// fit the current allocation (same plan and at most as many keys, or a smaller plan) is rebuilt IN PLACE -- no
// hipFree, no hipMalloc -- when this context alone holds it; pbft_verify_key_stats reports the phases of the
// last call.
int pbft_verify_set_keys(pbft_ctx* c, const uint8_t* A, uint32_t n, uint8_t* key_ok) {
  if (!c || (!A && n)) return set_err(PBFT_EINVAL, "null argument");
  if (n == 0 || n > 65535) return set_err(PBFT_EINVAL, "key count must be 1..65535");
  if (c->in_flight) return set_err(PBFT_EBUSY, "async batch in flight");
  const auto t_all = std::chrono::steady_clock::now();
  pbft_key_stats ks{};
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  // this context's key set, if no clone shares it: its tables may be overwritten in place
  keyset* own = (c->ks && c->ks->refs.load() == 1) ? c->ks : nullptr;
  const size_t own_bytes = own ? own->tab_bytes : 0;
  // The widest key plan whose tables fit the budget (PBFT_OPT_KEY_TABLE_BUDGET_MB / env, default 70 % of the HBM
  // free once the old key set is gone: ~180 GB on a 288-GB MI355X after the 30-GB base-point table) and the free
  // memory.  Entry indices are 32-bit (n * entries per key < 2^32).
  auto t = std::chrono::steady_clock::now();
  size_t free_b = 0, total_b = 0;
  HIP_TRY(hipMemGetInfo(&free_b, &total_b));
  ks.meminfo_ms = ms_since(t);
  const size_t avail = free_b + own_bytes;  // (a key set shared with clones stays allocated for them)
  size_t budget_mb = avail / 1048576 * 7 / 10;
  if (const char* e = getenv("PBFT_KEY_TABLE_BUDGET_MB")) budget_mb = strtoull(e, nullptr, 10);
  if (c->key_budget_mb) budget_mb = c->key_budget_mb;
  auto fits = [&](size_t table_words, uint64_t entries_per_key) {
    const size_t bytes = table_words * 4 * (size_t)n;
    return (uint64_t)n * entries_per_key < (1ull << 32) && bytes <= budget_mb * (size_t)1048576 &&
           bytes + ((size_t)4 << 30) < avail;
  };
  int pa = PLA_SMALL::P;
  if (fits(PLA_HUGE::TABLE_WORDS, PLA_HUGE::ENTRIES)) pa = PLA_HUGE::P;
  else if (fits(PLA_BIG::TABLE_WORDS, PLA_BIG::ENTRIES)) pa = PLA_BIG::P;
  else if (fits(PLA_MID::TABLE_WORDS, PLA_MID::ENTRIES)) pa = PLA_MID::P;
  const size_t tab_words = plan_table_words(pa);
  keyset* k = nullptr;
  if (own && n <= own->cap && tab_words * 4 * (size_t)n <= own->tab_bytes) {
    // the tables fit the allocation: rebuild in place.  Launches on callers' streams (device forms) may still
    // read the old tables.
    k = own;
    k->pa = pa;
    ks.reused = 1;
    HIP_TRY(hipDeviceSynchronize());
  } else {
    t = std::chrono::steady_clock::now();
    c->adopt(nullptr);  // (hipFree of an own key set: the slow part of a plan change)
    ks.free_ms = ms_since(t);
    t = std::chrono::steady_clock::now();
    k = new keyset();
    k->pa = pa;
    k->cap = n;
    k->tab_bytes = tab_words * 4 * (size_t)n;
    if (hipMalloc(&k->d_tabA, k->tab_bytes) != hipSuccess ||
        hipMalloc(&k->d_keys, 32 * (size_t)n) != hipSuccess || hipMalloc(&k->d_key_ok, n) != hipSuccess) {
      (void)hipGetLastError();
      keyset_release(k);
      c->kstats = ks;
      return set_err(PBFT_ENOMEM, "key table alloc");
    }
    ks.alloc_ms = ms_since(t);
  }
  k->n = n;
  t = std::chrono::steady_clock::now();
  int rc = PBFT_OK;
  if (hipMemcpyAsync(k->d_keys, A, 32 * (size_t)n, hipMemcpyHostToDevice, c->stream) != hipSuccess)
    rc = set_err(PBFT_EHIP, "key upload");
  if (!rc)
    rc = build_comb_tables(pa, k->d_keys, n, 1, k->d_tabA, k->d_key_ok, c->stream) == hipSuccess
             ? PBFT_OK
             : set_err(PBFT_EHIP, "key table build");
  if (!rc && key_ok && hipMemcpyAsync(key_ok, k->d_key_ok, n, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
    rc = set_err(PBFT_EHIP, "key_ok download");
  if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = set_err(PBFT_EHIP, "key table build");
  ks.build_ms = ms_since(t);
  ks.keys_built = n;
  if (rc) {
    if (k == c->ks) c->adopt(nullptr);  // half-rebuilt tables: no key set rather than a wrong one
    else keyset_release(k);
    c->kstats = ks;
    return rc;
  }
  k->h_keys.assign(A, A + 32 * (size_t)n);
  k->gen = ++g_keyset_gen;
  if (k != c->ks) c->adopt(k);
  else c->n_keys = k->n, c->pa = k->pa;  // rebuilt in place: same buffers, new count (and maybe plan)
  ks.table_bytes = k->tab_bytes;
  ks.total_ms = ms_since(t_all);
  c->kstats = ks;
  return PBFT_OK;
}

// Replace m keys of the installed set in place (the reference admits peers one at a time,
// src/behavior.rs:45-61 add_peer via src/network_behaviour_composer.rs:24-33): only their tables are rebuilt.
// The key set is shared by every clone of this context, so is the update.  Failure handling: a failure
// before any table is written (scratch allocation, key upload) changes nothing; one after the build kernels were
// launched clears key_ok of the updated slots in the SHARED key set -- every context that holds it then rejects
// those keys (their tables may be half-written) instead of verifying against them, the other keys keep working.
__global__ void clear_key_ok_kernel(uint8_t* key_ok, const uint32_t* slots, uint32_t m) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) key_ok[slots[i]] = 0;
}
int pbft_verify_update_keys(pbft_ctx* c, const uint32_t* idx, const uint8_t* A, uint32_t m, uint8_t* key_ok) {
  if (!c || (m && (!idx || !A))) return set_err(PBFT_EINVAL, "null argument");
  if (c->in_flight) return set_err(PBFT_EBUSY, "async batch in flight");
  if (!c->ks) return set_err(PBFT_ENOKEYS, "pbft_verify_set_keys not called");
  std::vector<uint32_t> sorted(idx, idx + m);
  std::sort(sorted.begin(), sorted.end());
  for (uint32_t i = 0; i < m; ++i)
    if (sorted[i] >= c->n_keys || (i && sorted[i] == sorted[i - 1]))
      return set_err(PBFT_EINVAL, "key index out of range or repeated");
  const auto t_all = std::chrono::steady_clock::now();
  pbft_key_stats ks{};
  ks.reused = 1;
  if (m == 0) { c->kstats = ks; return PBFT_OK; }
  const int inject = c->fault_inject;
  c->fault_inject = 0;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());  // no launch (this context's, a clone's, a device form's) reads the old tables
  keyset* k = c->ks;
  uint8_t* d_tmp = nullptr;  // [m] slots (u32) then [m][32] encodings
  const size_t off_enc = ((size_t)4 * m + 255) & ~(size_t)255;
  if (inject == 1 || hipMalloc(&d_tmp, off_enc + 32 * (size_t)m) != hipSuccess) {
    (void)hipGetLastError();
    return set_err(PBFT_ENOMEM, "update staging alloc");  // nothing written: the key set is unchanged
  }
  int rc = PBFT_OK, wrote = 0;
  if (hipMemcpyAsync(d_tmp, idx, 4 * (size_t)m, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
      hipMemcpyAsync(d_tmp + off_enc, A, 32 * (size_t)m, hipMemcpyHostToDevice, c->stream) != hipSuccess)
    rc = set_err(PBFT_EHIP, "key upload");
  if (!rc && build_comb_tables(k->pa, (const uint32_t*)(d_tmp + off_enc), m, 1, k->d_tabA, k->d_key_ok, c->stream,
                               (const uint32_t*)d_tmp, k->d_keys, &wrote) != hipSuccess)
    rc = set_err(PBFT_EHIP, wrote ? "key table build" : "key table build scratch alloc");
  if (!rc && inject == 2) rc = set_err(PBFT_EHIP, "key table build (injected fault)");
  std::vector<uint8_t> ok_all;
  if (!rc && key_ok) {
    ok_all.resize(k->n);
    if (hipMemcpyAsync(ok_all.data(), k->d_key_ok, k->n, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
      rc = set_err(PBFT_EHIP, "key_ok download");
  }
  if (!rc && hipStreamSynchronize(c->stream) != hipSuccess) rc = set_err(PBFT_EHIP, "key table build");
  if (rc && (wrote || inject == 2)) {
    // the updated slots' tables may be half-written: reject them everywhere the key set is used
    const std::string why = g_last_error;
    (void)hipGetLastError();
    hipLaunchKernelGGL(clear_key_ok_kernel, dim3((m + 255) / 256), dim3(256), 0, c->stream, k->d_key_ok,
                       (const uint32_t*)d_tmp, m);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
      c->adopt(nullptr);  // could not even mark them: drop the key set from this context rather than trust it
    g_last_error = why;
  }
  (void)hipStreamSynchronize(c->stream);
  (void)hipFree(d_tmp);
  if (rc) return rc;
  if (k->h_keys.size() == 32 * (size_t)k->n)
    for (uint32_t i = 0; i < m; ++i) memcpy(k->h_keys.data() + 32 * (size_t)idx[i], A + 32 * (size_t)i, 32);
  k->gen = ++g_keyset_gen;
  if (key_ok)
    for (uint32_t i = 0; i < m; ++i) key_ok[i] = ok_all[idx[i]];
  ks.keys_built = m;
  ks.build_ms = ks.total_ms = ms_since(t_all);
  ks.table_bytes = plan_table_words(k->pa) * 4 * (size_t)k->cap;
  c->kstats = ks;
  return PBFT_OK;
}

// Slots idx[0..m) of the context's key set reject every signature from now on (key_ok cleared; the tables stay):
// pbft_replica_update_keys uses it to leave no context of a replica verifying a key its PeerId map does not hold
// after an update failed on one of them.  A later set_keys / update_keys of a slot admits it again.
int pbft_verify_revoke_keys(pbft_ctx* c, const uint32_t* idx, uint32_t m) {
  if (!c || (m && !idx)) return set_err(PBFT_EINVAL, "null argument");
  if (c->in_flight) return set_err(PBFT_EBUSY, "async batch in flight");
  if (!c->ks) return set_err(PBFT_ENOKEYS, "pbft_verify_set_keys not called");
  for (uint32_t i = 0; i < m; ++i)
    if (idx[i] >= c->n_keys) return set_err(PBFT_EINVAL, "key index out of range");
  if (m == 0) return PBFT_OK;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());  // (no launch of a clone is reading key_ok while it changes)
  uint32_t* d_idx = nullptr;
  HIP_TRY(hipMalloc(&d_idx, 4 * (size_t)m));
  int rc = PBFT_OK;
  if (hipMemcpyAsync(d_idx, idx, 4 * (size_t)m, hipMemcpyHostToDevice, c->stream) != hipSuccess)
    rc = set_err(PBFT_EHIP, "revoke upload");
  if (!rc) {
    hipLaunchKernelGGL(clear_key_ok_kernel, dim3((m + 255) / 256), dim3(256), 0, c->stream, c->ks->d_key_ok,
                       (const uint32_t*)d_idx, m);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess)
      rc = set_err(PBFT_EHIP, "revoke kernel");
  }
  (void)hipStreamSynchronize(c->stream);
  (void)hipFree(d_idx);
  return rc;
}

// An identity of the key set the context verifies against (shared by its clones: pbft_verify_ctx_clone); 0 = none.
int pbft_verify_key_set_id(pbft_ctx* c, uint64_t* id) {
  if (!c || !id) return set_err(PBFT_EINVAL, "null argument");
  *id = (uint64_t)(uintptr_t)c->ks;
  return PBFT_OK;
}

int pbft_verify_key_stats(pbft_ctx* c, pbft_key_stats* out) {
  if (!c || !out) return set_err(PBFT_EINVAL, "null argument");
  *out = c->kstats;
  return PBFT_OK;
}

int pbft_verify_ctx_clone(pbft_ctx* parent, pbft_ctx** out) {
  if (!parent || !out) return set_err(PBFT_EINVAL, "null argument");
  *out = nullptr;
  pbft_ctx* c = nullptr;
  int rc = pbft_verify_ctx_create(parent->device, &c);
  if (rc) return rc;
  if (parent->ks) {
    ++parent->ks->refs;
    c->adopt(parent->ks);
  }
  // the parent's tuning options (pbft_verify_set_option)
  c->split_below = parent->split_below;
  c->fin_m = parent->fin_m;
  c->fin_tree = parent->fin_tree;
  c->fin_waves = parent->fin_waves;
  c->lat_split = parent->lat_split;
  c->timing = parent->timing;
  c->two_streams = parent->two_streams;
  c->comb_pair = parent->comb_pair;
  c->comb_prio = parent->comb_prio;
  c->comb_balance = parent->comb_balance;
  c->key_budget_mb = parent->key_budget_mb;
  *out = c;
  return PBFT_OK;
}

int pbft_verify_batch(pbft_ctx* c, const uint8_t* R, const uint8_t* S, const uint16_t* K, const uint8_t* M,
                      uint32_t msg_len, uint32_t msg_stride, uint64_t N, uint64_t* out) {
  int rc = pbft_verify_batch_async(c, R, S, K, M, msg_len, msg_stride, N, out);
  if (rc) return rc;
  return pbft_verify_wait(c);
}

int pbft_verify_batch_async(pbft_ctx* c, const uint8_t* R, const uint8_t* S, const uint16_t* K, const uint8_t* M,
                            uint32_t msg_len, uint32_t msg_stride, uint64_t N, uint64_t* out) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (c->in_flight) return set_err(PBFT_EBUSY, "async batch in flight");
  if (!check_batch_args(R, S, K, M, msg_len, msg_stride, N, out)) return set_err(PBFT_EINVAL, "bad batch arguments");
  if (c->n_keys == 0) return set_err(PBFT_ENOKEYS, "pbft_verify_set_keys not called");
  if (N == 0) return PBFT_OK;
  HIP_TRY(hipSetDevice(c->device));
  bool pinned = false;
  LT("pinned_query", pinned = host_pinned(R) && host_pinned(S) && host_pinned(K) && host_pinned(M));
  if (!pinned) {
    // pageable: copy into the pinned staging first, so the DMA below is asynchronous (a pageable
    // hipMemcpyAsync stages through the runtime's buffers and returns only when the copy is done)
    const host_batch_layout L(N, msg_stride);
    int rc = ensure_host_stage(c, L.bytes);
    if (rc) return rc;
    uint8_t* h = c->h_stage;
    memcpy(h, R, 32 * N);
    memcpy(h + L.offS, S, 32 * N);
    memcpy(h + L.offK, K, 2 * N);
    if (M && msg_stride) memcpy(h + L.offM, M, (size_t)msg_stride * N);
    R = h; S = h + L.offS; K = (const uint16_t*)(h + L.offK); M = M ? h + L.offM : M;
  }
  int rc = stage_and_launch(c, R, S, K, M, msg_len, msg_stride, N);
  if (rc) return rc;
  const uint64_t words = (N + 63) / 64;
  LT("export_bitmap", HIP_TRY(export_words(c, 0, words, c->stream)));
  LT("rec_done", HIP_TRY(hipEventRecord(c->ev_done, c->stream)));
  c->in_flight = true;
  c->v_readback = false;
  c->async_out = out;
  c->async_words = words;
  return PBFT_OK;
}

// Wait for an event by polling hipEventQuery instead of hipEventSynchronize.  VERDICT r04 item 2: with the H2D
// copies of a 4k host batch replaced by the import kernel, the back-to-back leg's stall moved into
// hipEventSynchronize (10.8 ms once in 5 one-second reps, profiles/r05/stall_probe.txt): the runtime's blocking
// wait (spin briefly, then sleep on the completion interrupt) sometimes wakes milliseconds late.  A serving
// thread that waits for its batch is latency-critical, so it polls (yielding the core between polls) -- the same
// thing the replica's flush_poll and the bench's poll loops do.  PBFT_SPIN_WAIT=0 restores hipEventSynchronize.
// The core is yielded only once a wait has lasted 2 ms: a sched_yield that lets another runnable thread in gives the
// core back a scheduler tick later, and the back-to-back leg's 1.05-ms maxima were exactly that (interleaved
// processes on one box, profiles/r05/stream_spin.txt: yielding every 64 polls, max 0.37-1.05 ms; never, 0.21-0.53).
// PBFT_SPIN_WAIT=2: never yield; =3: yield every 64 polls (the first r05 form).
static hipError_t wait_event(hipEvent_t e) {
  static const long spin = [] {
    const char* v = getenv("PBFT_SPIN_WAIT");
    return v ? strtol(v, nullptr, 10) : 1L;
  }();
  if (!spin) return hipEventSynchronize(e);
  const auto t0 = std::chrono::steady_clock::now();
  bool polite = spin == 3;
  for (uint32_t k = 0;; ++k) {
    const hipError_t q = hipEventQuery(e);
    if (q != hipErrorNotReady) return q;
    if ((k & 63) == 63) {
      if (!polite && spin == 1 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) polite = true;
      if (polite) sched_yield();
    }
  }
}

static int finish_async(pbft_ctx* c) {
  memcpy(c->async_out, c->h_bitmap, c->async_words * 8);
  c->in_flight = false;
  c->rows_out = c->async_words * 64;
  // (only with timing events: on events never recorded the call fails and would leave an error that the next
  // launch's hipGetLastError reports; a failure here is cleared for the same reason)
  if (c->timing && hipEventElapsedTime(&c->last_ms, c->ev0, c->ev1) != hipSuccess) (void)hipGetLastError();
  return PBFT_OK;
}

int pbft_verify_poll(pbft_ctx* c) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (!c->in_flight) return 1;
  if (c->v_open) return 0;  // progressive batch: not every chunk launched yet
  hipError_t e;
  LT("poll_query", e = hipEventQuery(c->ev_done));
  if (e == hipErrorNotReady) return 0;
  if (e != hipSuccess) {
    c->in_flight = false;  // the batch is lost; the context stays usable for the next submit
    HIP_TRY(e);
  }
  finish_async(c);
  return 1;
}

int pbft_verify_wait(pbft_ctx* c) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (!c->in_flight) return PBFT_OK;
  if (c->v_open) return set_err(PBFT_EBUSY, "progressive votes batch not fully submitted");
  hipError_t e;
  LT("wait_sync", e = wait_event(c->ev_done));
  if (e != hipSuccess) {
    c->in_flight = false;
    HIP_TRY(e);
  }
  return finish_async(c);
}

// ---- votes form, non-blocking (include/pbft_verify.h) ----
static int votes_submit_from(pbft_ctx* c, const uint8_t* R, const uint8_t* S, const uint16_t* K, const uint32_t* I,
                             const uint8_t* E, uint32_t n_env, uint64_t N, uint64_t* out, uint32_t rs_stride = 32) {
  int rc = stage_votes_and_launch(c, R, S, K, I, E, n_env, N, rs_stride);
  if (rc) return rc;
  const uint64_t words = (N + 63) / 64;
  HIP_TRY(export_words(c, 0, words, c->stream));
  HIP_TRY(hipEventRecord(c->ev_done, c->stream));
  c->in_flight = true;
  c->v_readback = false;
  c->async_out = out;
  c->async_words = words;
  return PBFT_OK;
}

int pbft_verify_votes_stage(pbft_ctx* c, uint64_t N, uint32_t n_env, pbft_votes_staging* out) {
  if (!c || !out) return set_err(PBFT_EINVAL, "null argument");
  if (c->in_flight) return set_err(PBFT_EBUSY, "async batch in flight");
  if (N && n_env == 0) return set_err(PBFT_EINVAL, "votes batch without envelopes");
  HIP_TRY(hipSetDevice(c->device));
  const host_votes_layout L(N, n_env);
  int rc = ensure_host_stage(c, L.bytes);
  if (rc) return rc;
  uint8_t* h = c->h_stage;
  out->sig = h;
  out->key_idx = (uint16_t*)(h + PBFT_VOTES_ROW_KEY);
  out->env_idx = (uint32_t*)(h + PBFT_VOTES_ROW_ENV);
  out->envelopes = h + L.offE;
  out->row_stride = ROW;
  c->staged = true;
  c->staged_n = N;
  c->staged_env = n_env;
  return PBFT_OK;
}

int pbft_verify_votes_submit(pbft_ctx* c, uint64_t N, uint32_t n_env, uint64_t* out) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (c->in_flight) return set_err(PBFT_EBUSY, "async batch in flight");
  if (!c->staged || N != c->staged_n || n_env != c->staged_env)
    return set_err(PBFT_EINVAL, "pbft_verify_votes_stage was not called for this batch");
  if (N && !out) return set_err(PBFT_EINVAL, "null bitmap");
  if (c->n_keys == 0) return set_err(PBFT_ENOKEYS, "pbft_verify_set_keys not called");
  c->staged = false;
  if (N == 0) return PBFT_OK;
  HIP_TRY(hipSetDevice(c->device));
  const host_votes_layout L(N, n_env);
  uint8_t* h = c->h_stage;
  return votes_submit_from(c, h, h + 32, (const uint16_t*)(h + PBFT_VOTES_ROW_KEY),
                           (const uint32_t*)(h + PBFT_VOTES_ROW_ENV), h + L.offE, n_env, N, out, ROW);
}

// Progressive form: the caller fills the staging front to back and launches as it goes.
int pbft_verify_votes_submit_begin(pbft_ctx* c, uint64_t N, uint32_t n_env, uint64_t* out) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (c->in_flight) return set_err(PBFT_EBUSY, "async batch in flight");
  if (!c->staged || N != c->staged_n || n_env != c->staged_env)
    return set_err(PBFT_EINVAL, "pbft_verify_votes_stage was not called for this batch");
  if (N == 0 || !out) return set_err(PBFT_EINVAL, "empty batch or null bitmap");
  if (c->n_keys == 0) return set_err(PBFT_ENOKEYS, "pbft_verify_set_keys not called");
  c->staged = false;
  HIP_TRY(hipSetDevice(c->device));
  const host_votes_layout L(N, n_env);
  int rc = votes_begin(c, c->h_stage + L.offE, n_env, N, true);
  if (rc) return rc;
  c->in_flight = true;  // (pbft_verify_poll reports "running" until every chunk is launched and done)
  c->async_out = out;
  c->async_words = (N + 63) / 64;
  return PBFT_OK;
}

int pbft_verify_votes_submit_rows(pbft_ctx* c, uint64_t rows) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (!c->in_flight || !c->v_open) return set_err(PBFT_EINVAL, "no progressive votes batch open");
  HIP_TRY(hipSetDevice(c->device));
  uint8_t* h = c->h_stage;
  int rc = votes_launch(c, h, h + 32, (const uint16_t*)(h + PBFT_VOTES_ROW_KEY), (const uint32_t*)(h + PBFT_VOTES_ROW_ENV),
                        ROW, rows);
  if (rc == PBFT_OK && !c->v_open)
    rc = hipEventRecord(c->ev_done, c->stream) == hipSuccess ? PBFT_OK : set_err(PBFT_EHIP, "event record");
  if (rc) {  // the batch is lost: drain what was launched, the context stays usable
    (void)hipStreamSynchronize(c->stream);
    if (c->stream2) (void)hipStreamSynchronize(c->stream2);
    (void)hipStreamSynchronize(c->cstream);
    c->in_flight = false;
    c->v_open = false;
  }
  return rc;
}

int pbft_verify_votes_submit_host(pbft_ctx* c, const uint8_t* rows, uint64_t N, const uint8_t* env, uint32_t n_env,
                                  uint64_t* out) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (c->in_flight) return set_err(PBFT_EBUSY, "async batch in flight");
  if (N == 0 || !rows || !env || n_env == 0 || !out) return set_err(PBFT_EINVAL, "empty batch or null argument");
  if (c->n_keys == 0) return set_err(PBFT_ENOKEYS, "pbft_verify_set_keys not called");
  c->staged = false;  // (as every host-buffer submit: a pending stage is void)
  HIP_TRY(hipSetDevice(c->device));
  int rc = votes_begin(c, env, n_env, N, true, true);
  if (rc) return rc;
  c->in_flight = true;
  c->async_out = out;
  c->async_words = (N + 63) / 64;
  rc = votes_launch(c, rows, rows + 32, (const uint16_t*)(rows + PBFT_VOTES_ROW_KEY),
                    (const uint32_t*)(rows + PBFT_VOTES_ROW_ENV), ROW, N);
  if (rc == PBFT_OK)
    rc = hipEventRecord(c->ev_done, c->stream) == hipSuccess ? PBFT_OK : set_err(PBFT_EHIP, "event record");
  if (rc) {  // the batch is lost: drain what was launched, the context stays usable
    (void)hipStreamSynchronize(c->stream);
    if (c->stream2) (void)hipStreamSynchronize(c->stream2);
    (void)hipStreamSynchronize(c->cstream);
    c->in_flight = false;
    c->v_open = false;
  }
  return rc;
}

// Anonymous pages pinned with hipHostRegister rather than hipHostMalloc: on the MI355X boxes the copy engine reads
// them at 56.5 GB/s wherever they are placed, while hipHostMalloc buffers after a process's first one read at 46-50
// GB/s (tools/microbench/pinned_write.cpp, numa_h2d.cpp; profiles/r05/pinned_h2d.txt).  One header page in front
// holds the mapping's length for pbft_host_free.
static constexpr size_t HOST_HDR = 4096;
// ---- votes batch in pieces (pbft_verify_votes_open / _piece / _close): the caller's rows and envelopes are
// written while earlier pieces are already being copied and verified (pbft_replica_push_many: r05) ----
int pbft_verify_votes_open(pbft_ctx* c, uint64_t n_cap, uint32_t env_cap, uint64_t* out) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (c->in_flight) return set_err(PBFT_EBUSY, "async batch in flight");
  if (n_cap == 0 || env_cap == 0 || !out) return set_err(PBFT_EINVAL, "empty batch or null bitmap");
  if (c->n_keys == 0) return set_err(PBFT_ENOKEYS, "pbft_verify_set_keys not called");
  c->staged = false;
  HIP_TRY(hipSetDevice(c->device));
  const uint64_t words = (n_cap + 63) / 64;
  const size_t env_bytes = ((size_t)PBFT_ENVELOPE_LEN * env_cap + 64 + 255) & ~(size_t)255;
  const votes_layout L(n_cap < VOTES_CHUNK ? n_cap : VOTES_CHUNK);
  int rc = ensure_stage(c, env_bytes + VOTES_BUFS * L.bytes, words);
  if (rc) return rc;
  rc = ensure_wk(c, env_cap);
  if (rc) return rc;
  const bool two = c->two_streams;
  if (two && !c->stream2) {
    HIP_TRY(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&c->ev_env, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&c->ev_s2, hipEventDisableTiming));
  }
  if (!c->ev_envp) HIP_TRY(hipEventCreateWithFlags(&c->ev_envp, hipEventDisableTiming));
  c->v_short_tail = false;
  c->v_ends.clear();
  c->v_s2_ready = true;  // (stream2 waits for every piece's envelopes itself: votes_piece)
  c->v_two = two;
  c->v_n = n_cap;
  c->v_next = 0;
  c->v_chunk = 0;
  c->v_env_bytes = env_bytes;
  c->v_env = 0;
  c->v_env_cap = env_cap;
  c->v_wk = c->d_wk;
  c->v_open = true;
  c->v_readback = true;
  c->rows_out = 0;
  c->chunk_out = 0;
  c->in_flight = true;
  c->async_out = out;
  c->async_words = words;
  return PBFT_OK;
}

static int votes_drop(pbft_ctx* c, int rc) {  // a failed piece: drain what was launched, the batch is lost
  (void)hipStreamSynchronize(c->stream);
  if (c->stream2) (void)hipStreamSynchronize(c->stream2);
  (void)hipStreamSynchronize(c->cstream);
  c->in_flight = false;
  c->v_open = false;
  c->v_env_cap = 0;
  return rc;
}

int pbft_verify_votes_piece(pbft_ctx* c, const uint8_t* rows, uint64_t row_lo, uint64_t row_hi, const uint8_t* envs,
                            uint32_t env_lo, uint32_t env_hi) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (!c->in_flight || !c->v_open || c->v_env_cap == 0) return set_err(PBFT_EINVAL, "no votes batch open in pieces");
  if (!rows || row_lo != c->v_next || row_hi < row_lo || row_hi > c->v_n || (row_lo & 63) ||
      env_lo != c->v_env || env_hi < env_lo || env_hi > c->v_env_cap || (env_hi > env_lo && !envs))
    return set_err(PBFT_EINVAL, "piece out of order or out of the opened bounds");
  HIP_TRY(hipSetDevice(c->device));
  if (env_hi > env_lo) {  // the piece's new envelopes and their block-2 schedules, ahead of its rows' kernels
    const uint32_t ne = env_hi - env_lo;
    if (hipMemcpyAsync(c->d_stage + (size_t)PBFT_ENVELOPE_LEN * env_lo, envs + (size_t)PBFT_ENVELOPE_LEN * env_lo,
                       (size_t)PBFT_ENVELOPE_LEN * ne, hipMemcpyHostToDevice, c->cstream) != hipSuccess ||
        hipEventRecord(c->ev_envp, c->cstream) != hipSuccess || hipStreamWaitEvent(c->stream, c->ev_envp, 0) != hipSuccess)
      return votes_drop(c, set_err(PBFT_EHIP, "piece envelopes"));
    hipLaunchKernelGGL(env_sched_kernel, dim3((ne + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream,
                       c->d_stage + (size_t)PBFT_ENVELOPE_LEN * env_lo, ne, c->d_wk + (size_t)SHA_ENV_WORDS * env_lo);
    if (hipGetLastError() != hipSuccess) return votes_drop(c, set_err(PBFT_EHIP, "piece envelope schedule"));
    if (c->v_two && (hipEventRecord(c->ev_env, c->stream) != hipSuccess ||
                     hipStreamWaitEvent(c->stream2, c->ev_env, 0) != hipSuccess))
      return votes_drop(c, set_err(PBFT_EHIP, "piece envelope event"));
    c->v_env = env_hi;
  }
  for (uint64_t lo = row_lo; lo < row_hi;) {
    const uint64_t n = row_hi - lo > VOTES_CHUNK ? VOTES_CHUNK : row_hi - lo;
    const int rc = votes_chunk(c, rows, rows + 32, (const uint16_t*)(rows + PBFT_VOTES_ROW_KEY),
                               (const uint32_t*)(rows + PBFT_VOTES_ROW_ENV), ROW, lo, n);
    if (rc) return votes_drop(c, rc);
    lo += n;
  }
  return PBFT_OK;
}

int pbft_verify_votes_close(pbft_ctx* c, uint64_t n) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (!c->in_flight || !c->v_open || c->v_env_cap == 0) return set_err(PBFT_EINVAL, "no votes batch open in pieces");
  if (n != c->v_next || n == 0) return votes_drop(c, set_err(PBFT_EINVAL, "close: rows submitted differ"));
  HIP_TRY(hipSetDevice(c->device));
  c->v_open = false;
  c->v_env_cap = 0;
  c->v_n = n;
  c->async_words = (n + 63) / 64;
  int rc = votes_join_streams(c);
  if (rc == PBFT_OK && hipEventRecord(c->ev_done, c->stream) != hipSuccess) rc = set_err(PBFT_EHIP, "event record");
  return rc ? votes_drop(c, rc) : PBFT_OK;
}

int pbft_host_alloc(pbft_ctx* c, size_t bytes, void** out) {
  if (!out) return set_err(PBFT_EINVAL, "null argument");
  *out = nullptr;
  if (!c || bytes == 0) return set_err(PBFT_EINVAL, "null context or empty allocation");
  HIP_TRY(hipSetDevice(c->device));
  const size_t len = HOST_HDR + ((bytes + 4095) & ~(size_t)4095);
  void* m = mmap(nullptr, len, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS, -1, 0);
  if (m == MAP_FAILED) return set_err(PBFT_ENOMEM, "host mmap");
  memcpy(m, &len, sizeof len);
  uint8_t* p = (uint8_t*)m + HOST_HDR;
  if (hipHostRegister(p, len - HOST_HDR, hipHostRegisterPortable) != hipSuccess) {
    (void)hipGetLastError();
    munmap(m, len);
    return set_err(PBFT_ENOMEM, "pinned host register");
  }
  *out = p;
  return PBFT_OK;
}

int pbft_host_free(pbft_ctx* c, void* p) {
  if (!p) return PBFT_OK;
  if (c) HIP_TRY(hipSetDevice(c->device));
  uint8_t* m = (uint8_t*)p - HOST_HDR;
  size_t len;
  memcpy(&len, m, sizeof len);
  HIP_TRY(hipHostUnregister(p));
  munmap(m, len);
  return PBFT_OK;
}

int pbft_verify_poll_rows(pbft_ctx* c, uint64_t* rows_done) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (c->in_flight && c->v_readback) {
    while (c->rows_out < c->v_next) {  // launched chunks whose bitmap words have landed, in order
      const hipError_t e = hipEventQuery(c->ev_rows[c->chunk_out]);
      if (e == hipErrorNotReady) break;
      if (e != hipSuccess) {
        c->in_flight = false;
        c->v_open = false;
        HIP_TRY(e);
      }
      const uint64_t hi = c->v_ends[c->chunk_out];
      memcpy(c->async_out + c->rows_out / 64, c->h_bitmap + c->rows_out / 64, (hi - c->rows_out + 63) / 64 * 8);
      c->rows_out = hi;
      ++c->chunk_out;
    }
    if (c->v_open || c->rows_out < c->v_n) {
      if (rows_done) *rows_done = c->rows_out;
      return 0;
    }
  }
  const bool progressive = c->in_flight && c->v_readback;
  const int st = pbft_verify_poll(c);
  if (rows_done) *rows_done = st == 1 ? c->rows_out : progressive ? c->rows_out : 0;
  return st;
}

int pbft_verify_votes_async(pbft_ctx* c, const uint8_t* R, const uint8_t* S, const uint16_t* K, const uint32_t* I,
                            const uint8_t* E, uint32_t n_env, uint64_t N, uint64_t* out) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (c->in_flight) return set_err(PBFT_EBUSY, "async batch in flight");
  if (N && (!R || !S || !K || !I || !out || !E || n_env == 0)) return set_err(PBFT_EINVAL, "bad votes arguments");
  if (c->n_keys == 0) return set_err(PBFT_ENOKEYS, "pbft_verify_set_keys not called");
  if (N == 0) return PBFT_OK;
  HIP_TRY(hipSetDevice(c->device));
  if (host_pinned(R) && host_pinned(S) && host_pinned(K) && host_pinned(I) && host_pinned(E))
    return votes_submit_from(c, R, S, K, I, E, n_env, N, out);
  pbft_votes_staging st;
  int rc = pbft_verify_votes_stage(c, N, n_env, &st);
  if (rc) return rc;
  for (uint64_t i = 0; i < N; ++i) {
    uint8_t* row = st.sig + (size_t)ROW * i;
    memcpy(row, R + 32 * i, 32);
    memcpy(row + 32, S + 32 * i, 32);
    const uint32_t kp = K[i];  // key_idx, two zero bytes
    memcpy(row + PBFT_VOTES_ROW_KEY, &kp, 4);
    memcpy(row + PBFT_VOTES_ROW_ENV, I + i, 4);
  }
  memcpy(st.envelopes, E, (size_t)PBFT_ENVELOPE_LEN * n_env);
  return pbft_verify_votes_submit(c, N, n_env, out);
}

// One host batch over several contexts (GPUs of this process, or cloned contexts
// of one GPU): contiguous 64-aligned shards, one async launch per context, each
// writing its own bitmap words in place (no exchange needed when
// the bitmaps return to one host process).
int pbft_verify_batch_multi(pbft_ctx* const* ctxs, uint32_t n_ctx, const uint8_t* R, const uint8_t* S,
                            const uint16_t* K, const uint8_t* M, uint32_t msg_len, uint32_t msg_stride, uint64_t N,
                            uint64_t* out) {
  if (!ctxs || n_ctx == 0) return set_err(PBFT_EINVAL, "no contexts");
  for (uint32_t i = 0; i < n_ctx; ++i)
    for (uint32_t j = 0; j < i; ++j)
      if (!ctxs[i] || ctxs[i] == ctxs[j]) return set_err(PBFT_EINVAL, "contexts must be distinct and non-null");
  if (!check_batch_args(R, S, K, M, msg_len, msg_stride, N, out)) return set_err(PBFT_EINVAL, "bad batch arguments");
  if (N == 0) return PBFT_OK;
  const uint64_t words = (N + 63) / 64, per = (words + n_ctx - 1) / n_ctx;
  int rc = PBFT_OK;
  uint32_t launched = 0;
  for (; launched < n_ctx; ++launched) {
    const uint64_t lo = launched * per * 64;
    if (lo >= N) break;
    const uint64_t hi = lo + per * 64 < N ? lo + per * 64 : N;
    rc = pbft_verify_batch_async(ctxs[launched], R + 32 * lo, S + 32 * lo, K + lo, M ? M + (size_t)msg_stride * lo : M,
                                 msg_len, msg_stride, hi - lo, out + lo / 64);
    if (rc) break;
  }
  for (uint32_t i = 0; i < launched; ++i) {
    const int w = pbft_verify_wait(ctxs[i]);
    if (!rc) rc = w;
  }
  return rc;
}

}  // extern "C"

// ---- single-process multi-GPU round, bitmap all-gather on RCCL (include/pbft_verify.h) ----
// RCCL is resolved at run time (dlopen), so the verifier loads on hosts and in processes without it; in a
// process that already loaded torch's bundled librccl.so.1 the same object is reused (SONAME match).
namespace {
struct rccl_api {
  bool ok = false;
  decltype(&ncclCommInitAll) CommInitAll = nullptr;
  decltype(&ncclCommDestroy) CommDestroy = nullptr;
  decltype(&ncclAllGather) AllGather = nullptr;
  decltype(&ncclGroupStart) GroupStart = nullptr;
  decltype(&ncclGroupEnd) GroupEnd = nullptr;
  decltype(&ncclGetErrorString) GetErrorString = nullptr;
};
rccl_api* rccl() {
  static rccl_api api;
  static std::once_flag once;
  std::call_once(once, [] {
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) return;
    api.CommInitAll = (decltype(api.CommInitAll))dlsym(h, "ncclCommInitAll");
    api.CommDestroy = (decltype(api.CommDestroy))dlsym(h, "ncclCommDestroy");
    api.AllGather = (decltype(api.AllGather))dlsym(h, "ncclAllGather");
    api.GroupStart = (decltype(api.GroupStart))dlsym(h, "ncclGroupStart");
    api.GroupEnd = (decltype(api.GroupEnd))dlsym(h, "ncclGroupEnd");
    api.GetErrorString = (decltype(api.GetErrorString))dlsym(h, "ncclGetErrorString");
    api.ok = api.CommInitAll && api.CommDestroy && api.AllGather && api.GroupStart && api.GroupEnd &&
             api.GetErrorString;
  });
  return api.ok ? &api : nullptr;
}
int rccl_err(ncclResult_t r, const char* what) {
  char b[256];
  snprintf(b, sizeof b, "%s: %s", what, rccl() ? rccl()->GetErrorString(r) : "RCCL unavailable");
  return set_err(PBFT_EHIP, b);
}
}  // namespace

struct pbft_multi {
  std::vector<pbft_ctx*> ctx;
  std::vector<ncclComm_t> comm;
};

extern "C" {

int pbft_multi_create(pbft_ctx* const* ctxs, uint32_t n_ctx, pbft_multi** out) {
  if (!ctxs || !out || n_ctx == 0) return set_err(PBFT_EINVAL, "no contexts");
  *out = nullptr;
  std::vector<int> devs(n_ctx);
  for (uint32_t i = 0; i < n_ctx; ++i) {
    if (!ctxs[i]) return set_err(PBFT_EINVAL, "null context");
    devs[i] = ctxs[i]->device;
    for (uint32_t j = 0; j < i; ++j)
      if (devs[j] == devs[i]) return set_err(PBFT_EINVAL, "one context per device (distinct devices)");
  }
  rccl_api* api = rccl();
  if (!api) return set_err(PBFT_ENODEV, "librccl.so.1 not loadable");
  pbft_multi* m = new pbft_multi();
  m->ctx.assign(ctxs, ctxs + n_ctx);
  m->comm.assign(n_ctx, nullptr);
  const ncclResult_t r = api->CommInitAll(m->comm.data(), (int)n_ctx, devs.data());
  if (r != ncclSuccess) {
    delete m;
    return rccl_err(r, "ncclCommInitAll");
  }
  *out = m;
  return PBFT_OK;
}

int pbft_multi_destroy(pbft_multi* m) {
  if (!m) return PBFT_OK;
  (void)pbft_multi_sync(m);
  if (rccl_api* api = rccl())
    for (ncclComm_t c : m->comm)
      if (c) (void)api->CommDestroy(c);
  delete m;
  return PBFT_OK;
}

int pbft_multi_sync(pbft_multi* m) {
  if (!m) return set_err(PBFT_EINVAL, "null multi");
  for (pbft_ctx* c : m->ctx) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  return PBFT_OK;
}

int pbft_verify_batch_device_multi(pbft_multi* m, const uint8_t* const* dR, const uint8_t* const* dS,
                                   const uint16_t* const* dK, const uint8_t* const* dM, uint32_t msg_len,
                                   uint32_t msg_stride, const uint64_t* n, uint64_t wpr, uint64_t* const* dB) {
  if (!m || !dR || !dS || !dK || !dM || !n || !dB) return set_err(PBFT_EINVAL, "null argument");
  const uint32_t G = (uint32_t)m->ctx.size();
  for (uint32_t r = 0; r < G; ++r) {
    if ((n[r] + 63) / 64 > wpr) return set_err(PBFT_EINVAL, "words_per_rank < ceil(n[r] / 64)");
    if (!dB[r] || !check_batch_args(dR[r], dS[r], dK[r], dM[r], msg_len, msg_stride, n[r], dB[r]))
      return set_err(PBFT_EINVAL, "bad shard arguments");
    if (m->ctx[r]->n_keys == 0) return set_err(PBFT_ENOKEYS, "pbft_verify_set_keys not called");
  }
  for (uint32_t r = 0; r < G; ++r) {
    pbft_ctx* c = m->ctx[r];
    HIP_TRY(hipSetDevice(c->device));
    uint64_t* mine = dB[r] + (size_t)r * wpr;
    const uint64_t words = (n[r] + 63) / 64;
    if (wpr > words) HIP_TRY(hipMemsetAsync(mine + words, 0, (wpr - words) * 8, c->stream));
    int rc = launch_verify(c, dR[r], dS[r], dK[r], dM[r], msg_len, msg_stride, n[r], mine, c->stream);
    if (rc) return rc;
  }
  rccl_api* api = rccl();
  ncclResult_t e = api->GroupStart();
  if (e != ncclSuccess) return rccl_err(e, "ncclGroupStart");
  for (uint32_t r = 0; r < G; ++r) {
    pbft_ctx* c = m->ctx[r];
    e = api->AllGather(dB[r] + (size_t)r * wpr, dB[r], wpr, ncclUint64, m->comm[r], c->stream);
    if (e != ncclSuccess) break;
  }
  const ncclResult_t e2 = api->GroupEnd();
  if (e != ncclSuccess) return rccl_err(e, "ncclAllGather");
  if (e2 != ncclSuccess) return rccl_err(e2, "ncclGroupEnd");
  return PBFT_OK;
}

int pbft_verify_batch_device(pbft_ctx* c, const uint8_t* dR, const uint8_t* dS, const uint16_t* dK,
                             const uint8_t* dM, uint32_t msg_len, uint32_t msg_stride, uint64_t N, uint64_t* dB,
                             void* stream) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (!check_batch_args(dR, dS, dK, dM, msg_len, msg_stride, N, dB)) return set_err(PBFT_EINVAL, "bad batch arguments");
  if (c->n_keys == 0) return set_err(PBFT_ENOKEYS, "pbft_verify_set_keys not called");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  return launch_verify(c, dR, dS, dK, dM, msg_len, msg_stride, N, dB, st);
}

// ---- verification under uninstalled keys (include/pbft_verify.h pbft_verify_batch_keys) ----
// Two kernel nodes on st: anykey_kernel (anykey.hip: every lane decompresses its own key and computes
// R' = [s]B + [k](-A) with 4-bit windows), then the finish the one-lane comb has behind it, chosen by N in the same
// way.  The hand-off lies where the comb's does: xyz and flags of workspace half 0.  No key set is read.
static int launch_verify_keys(pbft_ctx* c, const uint8_t* dR, const uint8_t* dS, const uint8_t* dA, const uint8_t* dM,
                              uint32_t msg_len, uint32_t msg_stride, uint64_t N, uint64_t* dB, hipStream_t st) {
  if (N == 0) return PBFT_OK;
  if ((N + BLOCK - 1) / BLOCK > 0x7fffffffull) return set_err(PBFT_EINVAL, "N too large for one launch");
  int rc = ensure_work(c, N);
  if (rc) return rc;
  if (c->fin_pending[0]) HIP_TRY(hipStreamWaitEvent(st, c->ev_fin[0], 0));  // a pipelined finish still reading half 0
  uint32_t* xyz = (uint32_t*)c->d_work;
  uint8_t* flags = c->d_work + 120 * N;  // within the half's 121 work_n bytes
  HIP_TRY(launch_anykey(dR, dS, dA, dM, msg_len, msg_stride, N, c->d_tabB, xyz, flags, st));
  HIP_TRY(launch_finish_by_n(c, dR, 32, xyz, flags, N, dB, st));
  return PBFT_OK;
}

int pbft_verify_batch_keys_device(pbft_ctx* c, const uint8_t* dR, const uint8_t* dS, const uint8_t* dA,
                                  const uint8_t* dM, uint32_t msg_len, uint32_t msg_stride, uint64_t N, uint64_t* dB,
                                  void* stream) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (!check_batch_args(dR, dS, dA, dM, msg_len, msg_stride, N, dB)) return set_err(PBFT_EINVAL, "bad batch arguments");
  HIP_TRY(hipSetDevice(c->device));
  return launch_verify_keys(c, dR, dS, dA, dM, msg_len, msg_stride, N, dB, stream ? (hipStream_t)stream : c->stream);
}

// Device staging of one chunk: R | S | A | msg (+ slack for the message reads past the end)
struct keys_stage_layout {
  size_t offS, offA, offM, bytes;
  keys_stage_layout(uint64_t n, uint32_t msg_stride) {
    offS = 32 * n;
    offA = 64 * n;
    offM = 96 * n;
    bytes = (offM + (size_t)msg_stride * n + 64 + 255) & ~(size_t)255;
  }
};

// Blocking.  Chunks of PIPE_CHUNK signatures, one after the other on the context's stream through one staging buffer
// (the kernels take several times as long as the copies: nothing to overlap).
int pbft_verify_batch_keys(pbft_ctx* c, const uint8_t* R, const uint8_t* S, const uint8_t* A, const uint8_t* M,
                           uint32_t msg_len, uint32_t msg_stride, uint64_t N, uint64_t* out) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (c->in_flight) return set_err(PBFT_EBUSY, "async batch in flight");
  if (!check_batch_args(R, S, A, M, msg_len, msg_stride, N, out)) return set_err(PBFT_EINVAL, "bad batch arguments");
  if (N == 0) return PBFT_OK;
  HIP_TRY(hipSetDevice(c->device));
  const uint64_t words = (N + 63) / 64;
  const keys_stage_layout L(N < PIPE_CHUNK ? N : PIPE_CHUNK, msg_stride);
  int rc = ensure_stage(c, L.bytes, words);
  if (rc) return rc;
  uint8_t* d = c->d_stage;
  for (uint64_t lo = 0; lo < N; lo += PIPE_CHUNK) {
    const uint64_t n = N - lo < PIPE_CHUNK ? N - lo : PIPE_CHUNK;
    HIP_TRY(hipMemcpyAsync(d, R + 32 * lo, 32 * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d + L.offS, S + 32 * lo, 32 * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d + L.offA, A + 32 * lo, 32 * n, hipMemcpyHostToDevice, c->stream));
    if ((size_t)msg_stride * n)
      HIP_TRY(hipMemcpyAsync(d + L.offM, M + (size_t)msg_stride * lo, (size_t)msg_stride * n, hipMemcpyHostToDevice,
                             c->stream));
    rc = launch_verify_keys(c, d, d + L.offS, d + L.offA, d + L.offM, msg_len, msg_stride, n, c->d_bitmap + lo / 64,
                            c->stream);
    if (rc) return rc;
  }
  HIP_TRY(hipMemcpyAsync(out, c->d_bitmap, words * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return PBFT_OK;
}

// Test hook (not declared in include/, like pbft_debug_invert): n triples (s, k, A) of 32 bytes each -> the encoding
// of [s]B + [k](-A) and the key_ok byte, through anykey_core.h's per-lane sum on the context's base-point table.  The
// hash is outside it, so a test can place the digits of k (< 2^253).  Host memory; blocking.
extern "C" int pbft_debug_anykey_point(pbft_ctx* c, const uint8_t* s, const uint8_t* k, const uint8_t* A, uint32_t n,
                                       uint8_t* enc_out, uint8_t* key_ok_out) {
  if (!c || !s || !k || !A || !enc_out || !key_ok_out || n == 0 || n > (1u << 20))
    return set_err(PBFT_EINVAL, "bad arguments");
  HIP_TRY(hipSetDevice(c->device));
  const size_t col = (size_t)32 * n;
  uint8_t* d = nullptr;
  if (hipMalloc(&d, 4 * col + n) != hipSuccess) return set_err(PBFT_ENOMEM, "point hook alloc");
  hipError_t e = hipMemcpyAsync(d, s, col, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d + col, k, col, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d + 2 * col, A, col, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess)
    e = launch_anykey_point((const uint32_t*)d, (const uint32_t*)(d + col), (const uint32_t*)(d + 2 * col), n, c->d_tabB,
                            (uint32_t*)(d + 3 * col), d + 4 * col, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(enc_out, d + 3 * col, col, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(key_ok_out, d + 4 * col, n, hipMemcpyDeviceToHost, c->stream);
  const hipError_t es = hipStreamSynchronize(c->stream);
  (void)hipFree(d);
  HIP_TRY(e);
  HIP_TRY(es);
  return PBFT_OK;
}

int pbft_verify_batch_device_pipelined(pbft_ctx* c, const uint8_t* dR, const uint8_t* dS, const uint16_t* dK,
                                       const uint8_t* dM, uint32_t msg_len, uint32_t msg_stride, uint64_t N,
                                       uint64_t* dB, void* stream, void* finish_stream) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (!stream || !finish_stream || stream == finish_stream)
    return set_err(PBFT_EINVAL, "two distinct non-null streams required");
  if (!check_batch_args(dR, dS, dK, dM, msg_len, msg_stride, N, dB)) return set_err(PBFT_EINVAL, "bad batch arguments");
  if (c->n_keys == 0) return set_err(PBFT_ENOKEYS, "pbft_verify_set_keys not called");
  HIP_TRY(hipSetDevice(c->device));
  return launch_verify(c, dR, dS, dK, dM, msg_len, msg_stride, N, dB, (hipStream_t)stream, 32, 2,
                       (hipStream_t)finish_stream);
}

int pbft_verify_votes(pbft_ctx* c, const uint8_t* R, const uint8_t* S, const uint16_t* K, const uint32_t* env_idx,
                      const uint8_t* envelopes, uint32_t n_env, uint64_t N, uint64_t* out) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (c->in_flight) return set_err(PBFT_EBUSY, "async batch in flight");
  if (N && (!R || !S || !K || !env_idx || !out || !envelopes || n_env == 0))
    return set_err(PBFT_EINVAL, "bad votes arguments");
  if (c->n_keys == 0) return set_err(PBFT_ENOKEYS, "pbft_verify_set_keys not called");
  if (N == 0) return PBFT_OK;
  int rc = pbft_verify_votes_async(c, R, S, K, env_idx, envelopes, n_env, N, out);
  if (rc) return rc;
  return pbft_verify_wait(c);
}

int pbft_verify_votes_device(pbft_ctx* c, const uint8_t* dR, const uint8_t* dS, const uint16_t* dK,
                             const uint32_t* d_env_idx, const uint8_t* d_envelopes, uint32_t n_env, uint64_t N,
                             uint64_t* dB, void* stream) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (N && (!dR || !dS || !dK || !d_env_idx || !d_envelopes || !dB || n_env == 0))
    return set_err(PBFT_EINVAL, "bad votes arguments");
  if (c->n_keys == 0) return set_err(PBFT_ENOKEYS, "pbft_verify_set_keys not called");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  if (N == 0) return PBFT_OK;
  const uint64_t* dWK = nullptr;
  int rc = prepare_env_sched(c, d_envelopes, n_env, st, &dWK);
  if (rc) return rc;
  return launch_verify(c, dR, dS, dK, d_envelopes, PBFT_ENVELOPE_LEN, PBFT_ENVELOPE_LEN, N, dB, st, 32, 2, nullptr,
                       d_env_idx, n_env, dWK);
}

// ---- vote tally (include/pbft_verify.h; kernels: tally.hip) ----
// Three launches (two when accumulating) on the caller's stream: no allocation, no synchronisation.
int pbft_tally_device(pbft_ctx* c, const uint64_t* dB, const uint16_t* dK, uint32_t key_stride, const uint32_t* dI,
                      uint32_t env_stride, uint64_t N, uint32_t n_env, uint32_t n_signers, uint32_t flags,
                      uint64_t* d_signers, uint32_t* d_count, void* stream) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (flags & ~PBFT_TALLY_ACCUMULATE) return set_err(PBFT_EINVAL, "unknown tally flags");
  if (n_signers == 0 || n_signers > 65535) return set_err(PBFT_EINVAL, "n_signers out of range");
  if (key_stride < 2 || (key_stride & 1) || env_stride < 4 || (env_stride & 3))
    return set_err(PBFT_EINVAL, "bad tally strides");
  if (N && (!dB || !dK || !dI)) return set_err(PBFT_EINVAL, "null tally input");
  if (n_env && (!d_signers || !d_count)) return set_err(PBFT_EINVAL, "null tally output");
  if (((uintptr_t)dB & 7) || ((uintptr_t)dK & 1) || ((uintptr_t)dI & 3) || ((uintptr_t)d_signers & 7) ||
      ((uintptr_t)d_count & 3))
    return set_err(PBFT_EINVAL, "misaligned tally pointer");
  if ((N + TALLY_BLOCK - 1) / TALLY_BLOCK > 0x7fffffffull) return set_err(PBFT_EINVAL, "N too large for one launch");
  if (n_env == 0) return PBFT_OK;  // nothing to write
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  if (!(flags & PBFT_TALLY_ACCUMULATE)) HIP_TRY(launch_tally_zero(d_signers, n_env, n_signers, st));
  if (N)
    HIP_TRY(launch_tally(dB, (const uint8_t*)dK, key_stride, (const uint8_t*)dI, env_stride, N, n_env, n_signers,
                         d_signers, st));
  HIP_TRY(launch_tally_count(d_signers, n_env, n_signers, d_count, st));
  return PBFT_OK;
}

// ---- envelope grouping (include/pbft_verify.h; kernels: group.hip) ----
static int ensure_group(pbft_ctx* c, uint64_t N) {
  return grow_device(&c->d_group, &c->group_cap, group_ws_bytes(N), "group workspace alloc");
}

static int check_group_args(const void* d_msg, uint32_t msg_stride, const void* dK, uint32_t key_stride, uint64_t N,
                            uint32_t env_cap, const void* d_env_idx, const void* d_envelopes, const void* d_n_env) {
  if (N > GROUP_MAX_ROWS) return set_err(PBFT_EINVAL, "more than 2^31 rows to group");
  if (msg_stride < PBFT_ENVELOPE_LEN || key_stride < 2 || (key_stride & 1))
    return set_err(PBFT_EINVAL, "bad group strides");
  if (N && env_cap == 0) return set_err(PBFT_EINVAL, "env_cap is 0");
  if (!d_n_env || (N && (!d_msg || !d_env_idx)) || (env_cap && !d_envelopes))
    return set_err(PBFT_EINVAL, "null group argument");
  if (((uintptr_t)d_env_idx & 3) || ((uintptr_t)d_n_env & 3) || ((uintptr_t)dK & 1))
    return set_err(PBFT_EINVAL, "misaligned group pointer");
  return PBFT_OK;
}

// Five launches on the caller's stream.  The workspace grows here only when the call is larger than every one before
// it and than pbft_group_reserve.
int pbft_group_envelopes_device(pbft_ctx* c, const uint8_t* d_msg, uint32_t msg_stride, const uint16_t* dK,
                                uint32_t key_stride, uint64_t N, uint32_t env_cap, uint32_t* d_env_idx,
                                uint8_t* d_envelopes, uint32_t* d_n_env, void* stream) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  int rc = check_group_args(d_msg, msg_stride, dK, key_stride, N, env_cap, d_env_idx, d_envelopes, d_n_env);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  rc = ensure_group(c, N);
  if (rc) return rc;
  if (!c->group_seeded) {  // drawn on the host, once: a peer cannot aim its envelopes at one probe chain
    std::random_device rd;
    c->group_seed = ((uint64_t)rd() << 32) ^ rd() ^ (uint64_t)std::chrono::steady_clock::now().time_since_epoch().count();
    c->group_seeded = true;
  }
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  HIP_TRY(launch_group(d_msg, msg_stride, (const uint8_t*)dK, key_stride, N, env_cap, c->group_seed,
                       c->group_hash_bits, c->d_group, d_env_idx, d_envelopes, d_n_env, st));
  return PBFT_OK;
}

int pbft_group_reserve(pbft_ctx* c, uint64_t max_n) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (max_n > GROUP_MAX_ROWS) return set_err(PBFT_EINVAL, "more than 2^31 rows to group");
  HIP_TRY(hipSetDevice(c->device));
  return ensure_group(c, max_n);
}

// pbft_verify_votes with every chunk tallied on its own stream while its columns are resident (the staging keeps
// VOTES_BUFS chunks, a batch may have more), all into one zeroed set -- OR is idempotent, so the chunks fold like
// PBFT_TALLY_ACCUMULATE pieces; then the counts and the copies back on the context stream, which follows both.
int pbft_verify_votes_tally(pbft_ctx* c, const uint8_t* R, const uint8_t* S, const uint16_t* K,
                            const uint32_t* env_idx, const uint8_t* envelopes, uint32_t n_env, uint64_t N,
                            uint64_t* out, uint64_t* signers_out, uint32_t* count_out) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (c->in_flight) return set_err(PBFT_EBUSY, "async batch in flight");
  if (N && (!R || !S || !K || !env_idx || !out || !envelopes || n_env == 0))
    return set_err(PBFT_EINVAL, "bad votes arguments");
  if (c->n_keys == 0) return set_err(PBFT_ENOKEYS, "pbft_verify_set_keys not called");
  if (n_env && (!signers_out || !count_out)) return set_err(PBFT_EINVAL, "null tally output");
  if (n_env == 0) return PBFT_OK;
  const size_t set_bytes = (size_t)n_env * tally_words(c->n_keys) * 8, cnt_bytes = (size_t)n_env * 4;
  if (N == 0) {
    memset(signers_out, 0, set_bytes);
    memset(count_out, 0, cnt_bytes);
    return PBFT_OK;
  }
  HIP_TRY(hipSetDevice(c->device));
  if (set_bytes + cnt_bytes > c->tally_cap) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->d_tally) HIP_TRY(hipFree(c->d_tally));
    c->d_tally = nullptr;
    c->tally_cap = 0;
    if (hipMalloc(&c->d_tally, set_bytes + cnt_bytes) != hipSuccess) return set_err(PBFT_ENOMEM, "tally alloc");
    c->tally_cap = set_bytes + cnt_bytes;
  }
  // zeroed on the context stream ahead of the batch: stream2's chunks wait for the envelope schedule behind it
  HIP_TRY(launch_tally_zero(c->d_tally, n_env, c->n_keys, c->stream));
  c->t_signers = c->d_tally;
  int rc = pbft_verify_votes_async(c, R, S, K, env_idx, envelopes, n_env, N, out);
  c->t_signers = nullptr;
  if (rc) return rc;
  uint32_t* d_count = (uint32_t*)((uint8_t*)c->d_tally + set_bytes);
  hipError_t e = launch_tally_count(c->d_tally, n_env, c->n_keys, d_count, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(signers_out, c->d_tally, set_bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(count_out, d_count, cnt_bytes, hipMemcpyDeviceToHost, c->stream);
  rc = pbft_verify_wait(c);  // (the bitmap; also ends the batch when a step above failed)
  HIP_TRY(e);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  return PBFT_OK;
}

// Binary wire records (include/pbft_wire.h): R at +0, S at +32, envelope at +64,
// key index at +150, stride 160 -- read in place by the same kernels.
int pbft_verify_records_device(pbft_ctx* c, const uint8_t* d_rec, uint64_t N, uint64_t* dB, void* stream) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (N && (!d_rec || !dB)) return set_err(PBFT_EINVAL, "bad batch arguments");
  if (((uintptr_t)d_rec & 15) != 0) return set_err(PBFT_EINVAL, "records must be 16-byte aligned");
  if (c->n_keys == 0) return set_err(PBFT_ENOKEYS, "pbft_verify_set_keys not called");
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  return launch_verify(c, d_rec, d_rec + 32, (const uint16_t*)(d_rec + 150), d_rec + 64, PBFT_ENVELOPE_LEN,
                       PBFT_RECORD_BYTES, N, dB, st, PBFT_RECORD_BYTES, PBFT_RECORD_BYTES);
}

int pbft_verify_records(pbft_ctx* c, const uint8_t* rec, uint64_t N, uint64_t* out) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (c->in_flight) return set_err(PBFT_EBUSY, "async batch in flight");
  if (N && (!rec || !out)) return set_err(PBFT_EINVAL, "bad batch arguments");
  if (c->n_keys == 0) return set_err(PBFT_ENOKEYS, "pbft_verify_set_keys not called");
  if (N == 0) return PBFT_OK;
  HIP_TRY(hipSetDevice(c->device));
  const uint64_t words = (N + 63) / 64;
  int rc = ensure_stage(c, PBFT_RECORD_BYTES * N + 256, words);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c->d_stage, rec, PBFT_RECORD_BYTES * N, hipMemcpyHostToDevice, c->stream));
  rc = pbft_verify_records_device(c, c->d_stage, N, c->d_bitmap, c->stream);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(out, c->d_bitmap, words * 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return PBFT_OK;
}

// ---- JSON frames decoded on the device (include/pbft_wire.h; kernels: wire_decode.hip) ----
static_assert(sizeof(pbft_frame_head) == 24, "pbft_frame_head is 24 bytes");
static int check_frames_args(const void* d_stream, const void* d_off, const void* d_len, const void* d_peer,
                             uint32_t n_replicas, uint64_t N, const void* d_records, const void* d_heads) {
  if (n_replicas == 0 || n_replicas > 65535) return set_err(PBFT_EINVAL, "n_replicas out of range");
  if (N > ((uint64_t)1 << 32)) return set_err(PBFT_EINVAL, "more than 2^32 frames");
  if (N && (!d_stream || !d_off || !d_len || !d_records || !d_heads))
    return set_err(PBFT_EINVAL, "null frames argument");
  if (((uintptr_t)d_stream & 15) || ((uintptr_t)d_off & 7) || ((uintptr_t)d_len & 3) || ((uintptr_t)d_peer & 1) ||
      ((uintptr_t)d_records & 15) || ((uintptr_t)d_heads & 7))
    return set_err(PBFT_EINVAL, "misaligned frames pointer");
  return PBFT_OK;
}

int pbft_wire_decode_frames_device(pbft_ctx* c, const uint8_t* d_stream, uint64_t stream_bytes, const uint64_t* d_off,
                                   const uint32_t* d_len, const uint16_t* d_peer, uint32_t n_replicas, uint64_t N,
                                   uint8_t* d_records, pbft_frame_head* d_heads, void* stream) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  int rc = check_frames_args(d_stream, d_off, d_len, d_peer, n_replicas, N, d_records, d_heads);
  if (rc) return rc;
  if (N == 0) return PBFT_OK;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  HIP_TRY(launch_decode_frames(d_stream, stream_bytes, d_off, d_len, d_peer, n_replicas, N, d_records, d_heads, st));
  return PBFT_OK;
}

int pbft_verify_frames_device(pbft_ctx* c, const uint8_t* d_stream, uint64_t stream_bytes, const uint64_t* d_off,
                              const uint32_t* d_len, const uint16_t* d_peer, uint32_t n_replicas, uint64_t N,
                              uint8_t* d_records, pbft_frame_head* d_heads, uint64_t* dB, void* stream) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  int rc = check_frames_args(d_stream, d_off, d_len, d_peer, n_replicas, N, d_records, d_heads);
  if (rc) return rc;
  if (N && !dB) return set_err(PBFT_EINVAL, "null bitmap");
  if ((uintptr_t)dB & 7) return set_err(PBFT_EINVAL, "misaligned frames pointer");
  if (c->n_keys == 0) return set_err(PBFT_ENOKEYS, "pbft_verify_set_keys not called");
  if (N == 0) return PBFT_OK;
  rc = pbft_wire_decode_frames_device(c, d_stream, stream_bytes, d_off, d_len, d_peer, n_replicas, N, d_records,
                                      d_heads, stream);
  if (rc) return rc;
  return pbft_verify_records_device(c, d_records, N, dB, stream);
}

// Device staging of the host form: records | heads | off | len | peer | (16-byte aligned) stream
struct frames_layout {
  size_t heads, off, len, peer, stream, total;
  frames_layout(uint64_t N, uint64_t stream_bytes) {
    heads = PBFT_RECORD_BYTES * (size_t)N;
    off = heads + sizeof(pbft_frame_head) * (size_t)N;
    len = off + 8 * (size_t)N;
    peer = len + 4 * (size_t)N;
    stream = (peer + 2 * (size_t)N + 15) & ~(size_t)15;
    total = stream + (((size_t)stream_bytes + 15) & ~(size_t)15);
  }
};

// The argument checks of the host forms (pbft_verify_frames, pbft_verify_frames_tally)
static int check_host_frames_args(pbft_ctx* c, const uint8_t* stream, uint64_t stream_bytes, const uint64_t* off,
                                  const uint32_t* flen, const uint16_t* peer, uint32_t n_replicas, uint64_t N,
                                  const uint64_t* out, const pbft_frame_head* heads_out) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (c->in_flight) return set_err(PBFT_EBUSY, "async batch in flight");
  if (n_replicas == 0 || n_replicas > 65535) return set_err(PBFT_EINVAL, "n_replicas out of range");
  if (N > ((uint64_t)1 << 32)) return set_err(PBFT_EINVAL, "more than 2^32 frames");
  if (N && (!stream || !off || !flen || !out || !heads_out)) return set_err(PBFT_EINVAL, "null frames argument");
  if (((uintptr_t)off & 7) || ((uintptr_t)flen & 3) || ((uintptr_t)peer & 1) || ((uintptr_t)out & 7) ||
      ((uintptr_t)heads_out & 7))
    return set_err(PBFT_EINVAL, "misaligned frames pointer");
  for (uint64_t f = 0; f < N; ++f)
    if (flen[f] > stream_bytes || off[f] > stream_bytes - flen[f])
      return set_err(PBFT_EINVAL, "frame beyond the end of the stream");
  if (c->n_keys == 0) return set_err(PBFT_ENOKEYS, "pbft_verify_set_keys not called");
  return PBFT_OK;
}

static int frames_settle(pbft_ctx* c, const uint8_t* stream, const uint64_t* off, const uint32_t* flen,
                         const uint16_t* peer, uint32_t n_replicas, uint64_t N, pbft_frame_head* heads_out,
                         uint8_t* d, pbft_frame_head* d_heads);

// The front half of the host forms, N > 0: stream and index into the device staging (laid out by `lay`, with `extra`
// bytes behind it for the caller), the decode, the heads back, the host's word on every deferred frame, and the
// patch of those that became OK.  Returns with all N records and heads settled on the device and the stream idle.
static int frames_stage_decode(pbft_ctx* c, const uint8_t* stream, uint64_t stream_bytes, const uint64_t* off,
                               const uint32_t* flen, const uint16_t* peer, uint32_t n_replicas, uint64_t N,
                               pbft_frame_head* heads_out, const frames_layout& lay, size_t extra) {
  const uint64_t words = (N + 63) / 64;
  int rc = ensure_stage(c, lay.total + extra + 256, words);
  if (rc) return rc;
  uint8_t* const d = c->d_stage;
  pbft_frame_head* const d_heads = (pbft_frame_head*)(d + lay.heads);
  HIP_TRY(hipMemcpyAsync(d + lay.stream, stream, stream_bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d + lay.off, off, 8 * N, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d + lay.len, flen, 4 * N, hipMemcpyHostToDevice, c->stream));
  if (peer) HIP_TRY(hipMemcpyAsync(d + lay.peer, peer, 2 * N, hipMemcpyHostToDevice, c->stream));
  rc = pbft_wire_decode_frames_device(c, d + lay.stream, stream_bytes, (const uint64_t*)(d + lay.off),
                                      (const uint32_t*)(d + lay.len), peer ? (const uint16_t*)(d + lay.peer) : nullptr,
                                      n_replicas, N, d, d_heads, c->stream);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(heads_out, d_heads, sizeof(pbft_frame_head) * N, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return frames_settle(c, stream, off, flen, peer, n_replicas, N, heads_out, d, d_heads);
}

// The host's word on every frame the device deferred (heads_out holds the device's heads; off / flen / peer are
// read for those frames only), and the patch of those that became OK into the N records at d and heads at d_heads.
static int frames_settle(pbft_ctx* c, const uint8_t* stream, const uint64_t* off, const uint32_t* flen,
                         const uint16_t* peer, uint32_t n_replicas, uint64_t N, pbft_frame_head* heads_out,
                         uint8_t* d, pbft_frame_head* d_heads) {
  // the frames the device deferred: the general parser, and the status rules of pbft_wire_decode_votes
  std::vector<uint32_t> pidx;
  std::vector<uint8_t> prec;
  std::vector<pbft_frame_head> phead;
  static thread_local char arena[1 << 16];  // (as pbft_wire_decode_votes: votes carry no operation)
  for (uint64_t f = 0; f < N; ++f) {
    pbft_frame_head& h = heads_out[f];
    if (h.status != PBFT_WIRE_EDEFER) continue;
    pbft_wire_msg m;
    uint8_t st = PBFT_WIRE_OK;
    if (pbft_wire_decode_json((const char*)stream + off[f], flen[f], &m, arena, sizeof arena) != 0)
      st = PBFT_WIRE_EJSON;
    else if (m.kind == PBFT_MSG_CLIENT_REQUEST) st = PBFT_WIRE_EKIND;
    else if (!m.digest_ok) st = PBFT_WIRE_EDIGEST;
    else if (!m.has_sig) st = PBFT_WIRE_EUNSIGNED;
    else if (m.replica >= n_replicas) st = PBFT_WIRE_ESIGNER;
    else if (peer && m.kind != PBFT_MSG_PREPREPARE && m.replica != peer[f]) st = PBFT_WIRE_ESIGNER;
    h.status = st;
    if (st != PBFT_WIRE_OK) continue;
    h.view = m.view;
    h.seq = m.seq;
    h.key_idx = (uint16_t)m.replica;
    h.kind = (uint8_t)m.kind;
    uint8_t env[PBFT_ENVELOPE_BYTES];
    pbft_envelope(env, (uint8_t)m.kind, m.view, m.seq, m.digest);
    const uint16_t k = (uint16_t)m.replica;
    prec.resize(prec.size() + PBFT_RECORD_BYTES);
    uint8_t* const rec = prec.data() + prec.size() - PBFT_RECORD_BYTES;
    pbft_records_pack(m.sig, m.sig + 32, &k, env, PBFT_ENVELOPE_BYTES, 1, rec);
    pidx.push_back((uint32_t)f);
    phead.push_back(h);
  }
  if (!pidx.empty()) {  // one H2D copy: indices | records | heads, then a scatter on the device
    const size_t P = pidx.size();
    const size_t o_rec = (4 * P + 15) & ~(size_t)15, o_head = o_rec + PBFT_RECORD_BYTES * P;
    const size_t bytes = o_head + sizeof(pbft_frame_head) * P;
    if (bytes > c->fpatch_cap) {
      if (c->d_fpatch) HIP_TRY(hipFree(c->d_fpatch));
      c->d_fpatch = nullptr;
      c->fpatch_cap = 0;
      const size_t cap = bytes + (bytes >> 2) + 4096;
      if (hipMalloc(&c->d_fpatch, cap) != hipSuccess) return set_err(PBFT_ENOMEM, "frame patch alloc");
      c->fpatch_cap = cap;
    }
    std::vector<uint8_t> buf(bytes, 0);
    memcpy(buf.data(), pidx.data(), 4 * P);
    memcpy(buf.data() + o_rec, prec.data(), PBFT_RECORD_BYTES * P);
    memcpy(buf.data() + o_head, phead.data(), sizeof(pbft_frame_head) * P);
    HIP_TRY(hipMemcpyAsync(c->d_fpatch, buf.data(), bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_patch_frames((const uint32_t*)c->d_fpatch, c->d_fpatch + o_rec, c->d_fpatch + o_head, (uint32_t)P,
                                N, d, d_heads, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // (buf is pageable and dies with this scope)
  }
  return PBFT_OK;
}

int pbft_verify_frames(pbft_ctx* c, const uint8_t* stream, uint64_t stream_bytes, const uint64_t* off,
                       const uint32_t* flen, const uint16_t* peer, uint32_t n_replicas, uint64_t N, uint64_t* out,
                       pbft_frame_head* heads_out, uint8_t* records_out) {
  int rc = check_host_frames_args(c, stream, stream_bytes, off, flen, peer, n_replicas, N, out, heads_out);
  if (rc) return rc;
  if (N == 0) return PBFT_OK;
  HIP_TRY(hipSetDevice(c->device));
  const uint64_t words = (N + 63) / 64;
  const frames_layout lay(N, stream_bytes);
  rc = frames_stage_decode(c, stream, stream_bytes, off, flen, peer, n_replicas, N, heads_out, lay, 0);
  if (rc) return rc;
  uint8_t* const d = c->d_stage;
  rc = pbft_verify_records_device(c, d, N, c->d_bitmap, c->stream);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(out, c->d_bitmap, words * 8, hipMemcpyDeviceToHost, c->stream));
  if (records_out) HIP_TRY(hipMemcpyAsync(records_out, d, PBFT_RECORD_BYTES * N, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return PBFT_OK;
}

// ---- frames in, quorums out: decode, group, verify, tally on one stream ----
int pbft_verify_frames_tally_device(pbft_ctx* c, const uint8_t* d_stream, uint64_t stream_bytes, const uint64_t* d_off,
                                    const uint32_t* d_len, const uint16_t* d_peer, uint32_t n_replicas, uint64_t N,
                                    uint8_t* d_records, pbft_frame_head* d_heads, uint64_t* dB, uint32_t env_cap,
                                    uint32_t* d_env_idx, uint8_t* d_envelopes, uint32_t* d_n_env, uint64_t* d_signers,
                                    uint32_t* d_count, void* stream) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  // every check of every step first: a refused call has written nothing
  int rc = check_frames_args(d_stream, d_off, d_len, d_peer, n_replicas, N, d_records, d_heads);
  if (rc) return rc;
  if (N && !dB) return set_err(PBFT_EINVAL, "null bitmap");
  if ((uintptr_t)dB & 7) return set_err(PBFT_EINVAL, "misaligned frames pointer");
  rc = check_group_args(d_records, PBFT_RECORD_BYTES, d_records, PBFT_RECORD_BYTES, N, env_cap, d_env_idx,
                        d_envelopes, d_n_env);
  if (rc) return rc;
  if (env_cap && (!d_signers || !d_count)) return set_err(PBFT_EINVAL, "null tally output");
  if (((uintptr_t)d_signers & 7) || ((uintptr_t)d_count & 3)) return set_err(PBFT_EINVAL, "misaligned tally pointer");
  if (c->n_keys == 0) return set_err(PBFT_ENOKEYS, "pbft_verify_set_keys not called");
  const uint16_t* const d_key = (const uint16_t*)(d_records + 150);
  if (N) {
    rc = pbft_wire_decode_frames_device(c, d_stream, stream_bytes, d_off, d_len, d_peer, n_replicas, N, d_records,
                                        d_heads, stream);
    if (rc) return rc;
  }
  rc = pbft_group_envelopes_device(c, d_records + 64, PBFT_RECORD_BYTES, d_key, PBFT_RECORD_BYTES, N, env_cap,
                                   d_env_idx, d_envelopes, d_n_env, stream);
  if (rc) return rc;
  if (N) {
    rc = pbft_verify_records_device(c, d_records, N, dB, stream);
    if (rc) return rc;
  }
  return pbft_tally_device(c, dB, d_key, PBFT_RECORD_BYTES, d_env_idx, 4, N, env_cap, c->n_keys, 0, d_signers,
                           d_count, stream);
}

int pbft_verify_frames_tally(pbft_ctx* c, const uint8_t* stream, uint64_t stream_bytes, const uint64_t* off,
                             const uint32_t* flen, const uint16_t* peer, uint32_t n_replicas, uint64_t N,
                             uint32_t env_cap, uint64_t* out, pbft_frame_head* heads_out, uint32_t* env_idx_out,
                             uint8_t* envelopes_out, uint32_t* n_env_out, uint64_t* signers_out,
                             uint32_t* count_out) {
  int rc = check_host_frames_args(c, stream, stream_bytes, off, flen, peer, n_replicas, N, out, heads_out);
  if (rc) return rc;
  if (N && env_cap == 0) return set_err(PBFT_EINVAL, "env_cap is 0");
  if (!n_env_out || (env_cap && (!envelopes_out || !signers_out || !count_out)))
    return set_err(PBFT_EINVAL, "null tally output");
  if (N > GROUP_MAX_ROWS) return set_err(PBFT_EINVAL, "more than 2^31 rows to group");
  const uint32_t W = tally_words(c->n_keys);
  const size_t env_bytes = (size_t)env_cap * PBFT_ENVELOPE_LEN, set_bytes = (size_t)env_cap * W * 8,
               cnt_bytes = (size_t)env_cap * 4;
  if (N == 0) {  // no frame: no envelope, empty sets
    n_env_out[0] = n_env_out[1] = 0;
    if (env_cap) {
      memset(envelopes_out, 0, env_bytes);
      memset(signers_out, 0, set_bytes);
      memset(count_out, 0, cnt_bytes);
    }
    return PBFT_OK;
  }
  HIP_TRY(hipSetDevice(c->device));
  const uint64_t words = (N + 63) / 64;
  const frames_layout lay(N, stream_bytes);
  // behind the frames staging: env_idx | envelopes (+16) | n_env | signer sets | counts
  const size_t o_idx = lay.total, o_env = o_idx + ((4 * (size_t)N + 15) & ~(size_t)15),
               o_n = o_env + ((env_bytes + 16 + 15) & ~(size_t)15), o_set = o_n + 16, o_cnt = o_set + set_bytes,
               extra = o_cnt + cnt_bytes - lay.total;
  rc = frames_stage_decode(c, stream, stream_bytes, off, flen, peer, n_replicas, N, heads_out, lay, extra);
  if (rc) return rc;
  uint8_t* const d = c->d_stage;
  uint32_t* const d_idx = (uint32_t*)(d + o_idx);
  const uint16_t* const d_key = (const uint16_t*)(d + 150);
  rc = pbft_group_envelopes_device(c, d + 64, PBFT_RECORD_BYTES, d_key, PBFT_RECORD_BYTES, N, env_cap, d_idx,
                                   d + o_env, (uint32_t*)(d + o_n), c->stream);
  if (rc) return rc;
  rc = pbft_verify_records_device(c, d, N, c->d_bitmap, c->stream);
  if (rc) return rc;
  rc = pbft_tally_device(c, c->d_bitmap, d_key, PBFT_RECORD_BYTES, d_idx, 4, N, env_cap, c->n_keys, 0,
                         (uint64_t*)(d + o_set), (uint32_t*)(d + o_cnt), c->stream);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(out, c->d_bitmap, words * 8, hipMemcpyDeviceToHost, c->stream));
  if (env_idx_out) HIP_TRY(hipMemcpyAsync(env_idx_out, d_idx, 4 * N, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(envelopes_out, d + o_env, env_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(n_env_out, d + o_n, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(signers_out, d + o_set, set_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(count_out, d + o_cnt, cnt_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return PBFT_OK;
}

// ---- the replica's admission pass (include/pbft_wire.h; kernels: admit.hip) ----
static_assert(sizeof(pbft_frame_head) == sizeof(pbft::admit_head) && sizeof(pbft_admit_residue) == sizeof(admit_residue),
              "admit.hip reads pbft_frame_head and writes pbft_admit_residue");
static_assert(PBFT_ADMIT_CLEAN == pbft::ADMIT_CLEAN && PBFT_ADMIT_CONTESTED == pbft::ADMIT_CONTESTED &&
                  PBFT_ADMIT_REJ_VIEW == pbft::ADMIT_REJ_VIEW && PBFT_ADMIT_REJ_WATERMARK == pbft::ADMIT_REJ_WATERMARK &&
                  PBFT_ADMIT_REJ_SIGNER == pbft::ADMIT_REJ_SIGNER && PBFT_ADMIT_HOST == pbft::ADMIT_HOST &&
                  PBFT_ADMIT_PAD == pbft::ADMIT_PAD && PBFT_ADMIT_CLASSES == pbft::ADMIT_CLASSES,
              "PBFT_ADMIT_* are admit_core.h's classes");
static int ensure_admit(pbft_ctx* c, uint64_t plane_bits, uint64_t N) {
  return grow_device(&c->d_admit, &c->admit_cap, admit_ws(plane_bits, N).total, "admit workspace alloc");
}

static int check_admit_shape(uint64_t log_window, uint32_t n_keys, uint64_t N) {
  if (N > ADMIT_MAX_ROWS) return set_err(PBFT_EINVAL, "more than 2^31 rows to admit");
  if (n_keys == 0 || n_keys > 65535) return set_err(PBFT_EINVAL, "n_keys out of range");
  if (log_window == 0 || pbft::admit_plane_bits(log_window, n_keys) == 0)
    return set_err(PBFT_EINVAL, "2 * log_window * n_keys must be in [1, 2^30]");
  return PBFT_OK;
}

// Five launches on the caller's stream.  The workspace grows here only when the call is larger than every one before
// it and than pbft_admit_reserve.
int pbft_admit_device(pbft_ctx* c, const pbft_frame_head* d_heads, uint8_t* d_records, const uint64_t* d_off,
                      const uint32_t* d_len, const uint32_t* d_n_frames, uint64_t N, uint64_t view, uint64_t h,
                      uint64_t log_window, uint32_t n_keys, uint32_t residue_cap, uint8_t* d_class, uint32_t* d_counts,
                      uint64_t* d_clean, pbft_admit_residue* d_res, uint32_t* d_n_res, void* stream) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  int rc = check_admit_shape(log_window, n_keys, N);
  if (rc) return rc;
  if (!d_counts || !d_n_res || (N && (!d_heads || !d_records || !d_class || !d_clean)) || (residue_cap && !d_res))
    return set_err(PBFT_EINVAL, "null admit argument");
  if (((uintptr_t)d_heads & 7) || ((uintptr_t)d_records & 1) || ((uintptr_t)d_off & 7) || ((uintptr_t)d_len & 3) ||
      ((uintptr_t)d_n_frames & 3) || ((uintptr_t)d_counts & 3) || ((uintptr_t)d_clean & 7) || ((uintptr_t)d_res & 7) ||
      ((uintptr_t)d_n_res & 3))
    return set_err(PBFT_EINVAL, "misaligned admit pointer");
  HIP_TRY(hipSetDevice(c->device));
  rc = ensure_admit(c, pbft::admit_plane_bits(log_window, n_keys), N);
  if (rc) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  HIP_TRY(launch_admit((const pbft::admit_head*)d_heads, d_records, d_off, d_len, d_n_frames, N, view, h, log_window,
                       n_keys, residue_cap, c->d_admit, d_class, d_counts, d_clean, (admit_residue*)d_res, d_n_res,
                       st));
  return PBFT_OK;
}

int pbft_admit_reserve(pbft_ctx* c, uint64_t log_window, uint32_t n_keys, uint64_t max_n) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  const int rc = check_admit_shape(log_window, n_keys, max_n);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  return ensure_admit(c, pbft::admit_plane_bits(log_window, n_keys), max_n);
}

// ---- connection streams in: the frame index made on the device (include/pbft_wire.h; kernels: wire_index.hip) ----
static_assert(sizeof(pbft_seg_head) == 24, "pbft_seg_head is 24 bytes");
static int ensure_index(pbft_ctx* c, uint64_t stream_bytes, uint32_t S) {
  return grow_device(&c->d_index, &c->index_cap, index_ws(stream_bytes, S, c->index_tile).total,
                     "index workspace alloc");
}

static int check_index_args(const void* d_stream, uint64_t stream_bytes, const void* d_seg_off, const void* d_seg_len,
                            const void* d_seg_peer, uint64_t S, uint64_t frame_cap, const void* d_off,
                            const void* d_len, const void* d_peer, const void* d_seg_heads, const void* d_n_frames) {
  if (S > pbft::IX_MAX_SEGMENTS) return set_err(PBFT_EINVAL, "more than 65536 segments");
  if (frame_cap > ((uint64_t)1 << 31)) return set_err(PBFT_EINVAL, "frame_cap above 2^31");
  if (stream_bytes > pbft::IX_MAX_STREAM) return set_err(PBFT_EINVAL, "more than 2^31 stream bytes to index");
  if (!d_n_frames || (stream_bytes && !d_stream) || (S && (!d_seg_off || !d_seg_len || !d_seg_heads)) ||
      (frame_cap && (!d_off || !d_len)) || (frame_cap && S && !d_peer != !d_seg_peer))
    return set_err(PBFT_EINVAL, "null index argument");
  if (((uintptr_t)d_stream & 15) || ((uintptr_t)d_seg_off & 7) || ((uintptr_t)d_seg_len & 7) ||
      ((uintptr_t)d_seg_peer & 1) || ((uintptr_t)d_off & 7) || ((uintptr_t)d_len & 3) || ((uintptr_t)d_peer & 1) ||
      ((uintptr_t)d_seg_heads & 7) || ((uintptr_t)d_n_frames & 3))
    return set_err(PBFT_EINVAL, "misaligned index pointer");
  return PBFT_OK;
}

int pbft_wire_index_streams_device(pbft_ctx* c, const uint8_t* d_stream, uint64_t stream_bytes,
                                   const uint64_t* d_seg_off, const uint64_t* d_seg_len, const uint16_t* d_seg_peer,
                                   uint32_t S, uint64_t frame_cap, uint64_t* d_off, uint32_t* d_len, uint16_t* d_peer,
                                   pbft_seg_head* d_seg_heads, uint32_t* d_n_frames, void* stream) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  int rc = check_index_args(d_stream, stream_bytes, d_seg_off, d_seg_len, d_seg_peer, S, frame_cap, d_off, d_len,
                            d_peer, d_seg_heads, d_n_frames);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  rc = ensure_index(c, stream_bytes, S);
  if (rc) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  HIP_TRY(launch_index_streams(d_stream, stream_bytes, d_seg_off, d_seg_len, d_seg_peer, S, frame_cap, c->index_tile,
                               c->d_index, d_off, d_len, frame_cap ? d_peer : nullptr, d_seg_heads, d_n_frames, st));
  return PBFT_OK;
}

int pbft_index_reserve(pbft_ctx* c, uint64_t max_stream_bytes, uint32_t max_segments) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (max_segments > pbft::IX_MAX_SEGMENTS) return set_err(PBFT_EINVAL, "more than 65536 segments");
  if (max_stream_bytes > pbft::IX_MAX_STREAM) return set_err(PBFT_EINVAL, "more than 2^31 stream bytes to index");
  HIP_TRY(hipSetDevice(c->device));
  return ensure_index(c, max_stream_bytes, max_segments);
}

int pbft_verify_streams_tally_device(pbft_ctx* c, const uint8_t* d_stream, uint64_t stream_bytes,
                                     const uint64_t* d_seg_off, const uint64_t* d_seg_len, const uint16_t* d_seg_peer,
                                     uint32_t S, uint32_t n_replicas, uint64_t frame_cap, uint64_t* d_off,
                                     uint32_t* d_len, uint16_t* d_peer, pbft_seg_head* d_seg_heads,
                                     uint32_t* d_n_frames, uint8_t* d_records, pbft_frame_head* d_heads, uint64_t* dB,
                                     uint32_t env_cap, uint32_t* d_env_idx, uint8_t* d_envelopes, uint32_t* d_n_env,
                                     uint64_t* d_signers, uint32_t* d_count, void* stream) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  // every check of every step first: a refused call has written nothing
  int rc = check_index_args(d_stream, stream_bytes, d_seg_off, d_seg_len, d_seg_peer, S, frame_cap, d_off, d_len,
                            d_peer, d_seg_heads, d_n_frames);
  if (rc) return rc;
  const uint64_t N = frame_cap;
  rc = check_frames_args(d_stream, d_off, d_len, d_peer, n_replicas, N, d_records, d_heads);
  if (rc) return rc;
  if (N && !dB) return set_err(PBFT_EINVAL, "null bitmap");
  if ((uintptr_t)dB & 7) return set_err(PBFT_EINVAL, "misaligned frames pointer");
  rc = check_group_args(d_records, PBFT_RECORD_BYTES, d_records, PBFT_RECORD_BYTES, N, env_cap, d_env_idx,
                        d_envelopes, d_n_env);
  if (rc) return rc;
  if (env_cap && (!d_signers || !d_count)) return set_err(PBFT_EINVAL, "null tally output");
  if (((uintptr_t)d_signers & 7) || ((uintptr_t)d_count & 3)) return set_err(PBFT_EINVAL, "misaligned tally pointer");
  if (c->n_keys == 0) return set_err(PBFT_ENOKEYS, "pbft_verify_set_keys not called");
  rc = pbft_wire_index_streams_device(c, d_stream, stream_bytes, d_seg_off, d_seg_len, d_seg_peer, S, frame_cap, d_off,
                                      d_len, d_peer, d_seg_heads, d_n_frames, stream);
  if (rc) return rc;
  return pbft_verify_frames_tally_device(c, d_stream, stream_bytes, d_off, d_len, d_peer, n_replicas, N, d_records,
                                         d_heads, dB, env_cap, d_env_idx, d_envelopes, d_n_env, d_signers, d_count,
                                         stream);
}

int pbft_verify_streams_tally(pbft_ctx* c, const uint8_t* stream, uint64_t stream_bytes, const uint64_t* seg_off,
                              const uint64_t* seg_len, const uint16_t* seg_peer, uint32_t S, uint32_t n_replicas,
                              uint64_t frame_cap, uint32_t env_cap, uint64_t* out, pbft_frame_head* heads_out,
                              uint32_t* env_idx_out, uint8_t* envelopes_out, uint32_t* n_env_out,
                              uint64_t* signers_out, uint32_t* count_out, pbft_seg_head* seg_heads_out,
                              uint32_t* n_frames_out, uint64_t* off_out, uint32_t* flen_out) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (c->in_flight) return set_err(PBFT_EBUSY, "async batch in flight");
  if (n_replicas == 0 || n_replicas > 65535) return set_err(PBFT_EINVAL, "n_replicas out of range");
  if (S > pbft::IX_MAX_SEGMENTS) return set_err(PBFT_EINVAL, "more than 65536 segments");
  if (frame_cap > ((uint64_t)1 << 31)) return set_err(PBFT_EINVAL, "frame_cap above 2^31");
  if (stream_bytes > pbft::IX_MAX_STREAM) return set_err(PBFT_EINVAL, "more than 2^31 stream bytes to index");
  if (!n_frames_out || (stream_bytes && !stream) || (S && (!seg_off || !seg_len || !seg_heads_out)) ||
      (frame_cap && (!out || !heads_out)))
    return set_err(PBFT_EINVAL, "null streams argument");
  if (((uintptr_t)seg_off & 7) || ((uintptr_t)seg_len & 7) || ((uintptr_t)seg_peer & 1) || ((uintptr_t)out & 7) ||
      ((uintptr_t)heads_out & 7) || ((uintptr_t)seg_heads_out & 7) || ((uintptr_t)n_frames_out & 3) ||
      ((uintptr_t)off_out & 7) || ((uintptr_t)flen_out & 3))
    return set_err(PBFT_EINVAL, "misaligned streams pointer");
  if (frame_cap && env_cap == 0) return set_err(PBFT_EINVAL, "env_cap is 0");
  if (!n_env_out || (env_cap && (!envelopes_out || !signers_out || !count_out)))
    return set_err(PBFT_EINVAL, "null tally output");
  if (c->n_keys == 0) return set_err(PBFT_ENOKEYS, "pbft_verify_set_keys not called");
  HIP_TRY(hipSetDevice(c->device));
  const uint32_t W = tally_words(c->n_keys);
  const size_t env_bytes = (size_t)env_cap * PBFT_ENVELOPE_LEN, set_bytes = (size_t)env_cap * W * 8,
               cnt_bytes = (size_t)env_cap * 4;
  // the frames staging for frame_cap frames; behind it the segment table, the segment heads and the totals, then
  // env_idx | envelopes (+16) | n_env | signer sets | counts as in pbft_verify_frames_tally
  const frames_layout lay(frame_cap, stream_bytes);
  const size_t o_soff = (lay.total + 15) & ~(size_t)15, o_slen = o_soff + 8 * (size_t)S, o_shead = o_slen + 8 * (size_t)S,
               o_nfr = o_shead + sizeof(pbft_seg_head) * (size_t)S, o_speer = o_nfr + 8,
               o_idx = (o_speer + 2 * (size_t)S + 15) & ~(size_t)15,
               o_env = o_idx + ((4 * (size_t)frame_cap + 15) & ~(size_t)15),
               o_n = o_env + ((env_bytes + 16 + 15) & ~(size_t)15), o_set = o_n + 16, o_cnt = o_set + set_bytes;
  int rc = ensure_stage(c, o_cnt + cnt_bytes + 256, (frame_cap + 63) / 64);
  if (rc) return rc;
  uint8_t* const d = c->d_stage;
  pbft_frame_head* const d_heads = (pbft_frame_head*)(d + lay.heads);
  uint64_t* const d_off = (uint64_t*)(d + lay.off);
  uint32_t* const d_len = (uint32_t*)(d + lay.len);
  uint16_t* const d_peer = seg_peer ? (uint16_t*)(d + lay.peer) : nullptr;
  if (stream_bytes) HIP_TRY(hipMemcpyAsync(d + lay.stream, stream, stream_bytes, hipMemcpyHostToDevice, c->stream));
  if (S) {
    HIP_TRY(hipMemcpyAsync(d + o_soff, seg_off, 8 * (size_t)S, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d + o_slen, seg_len, 8 * (size_t)S, hipMemcpyHostToDevice, c->stream));
    if (seg_peer) HIP_TRY(hipMemcpyAsync(d + o_speer, seg_peer, 2 * (size_t)S, hipMemcpyHostToDevice, c->stream));
  }
  rc = pbft_wire_index_streams_device(c, d + lay.stream, stream_bytes, (const uint64_t*)(d + o_soff),
                                      (const uint64_t*)(d + o_slen), seg_peer ? (const uint16_t*)(d + o_speer) : nullptr,
                                      S, frame_cap, d_off, d_len, frame_cap ? d_peer : nullptr,
                                      (pbft_seg_head*)(d + o_shead), (uint32_t*)(d + o_nfr), c->stream);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(n_frames_out, d + o_nfr, 8, hipMemcpyDeviceToHost, c->stream));
  if (S) HIP_TRY(hipMemcpyAsync(seg_heads_out, d + o_shead, sizeof(pbft_seg_head) * (size_t)S, hipMemcpyDeviceToHost,
                                c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const uint64_t N = n_frames_out[0] < frame_cap ? n_frames_out[0] : frame_cap;
  if (N == 0) {  // no frame: no envelope, empty sets
    n_env_out[0] = n_env_out[1] = 0;
    if (env_cap) {
      memset(envelopes_out, 0, env_bytes);
      memset(signers_out, 0, set_bytes);
      memset(count_out, 0, cnt_bytes);
    }
    return PBFT_OK;
  }
  rc = pbft_wire_decode_frames_device(c, d + lay.stream, stream_bytes, d_off, d_len, d_peer, n_replicas, N, d,
                                      d_heads, c->stream);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(heads_out, d_heads, sizeof(pbft_frame_head) * N, hipMemcpyDeviceToHost, c->stream));
  if (off_out) HIP_TRY(hipMemcpyAsync(off_out, d_off, 8 * N, hipMemcpyDeviceToHost, c->stream));
  if (flen_out) HIP_TRY(hipMemcpyAsync(flen_out, d_len, 4 * N, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  bool deferred = false;
  for (uint64_t f = 0; f < N && !deferred; ++f) deferred = heads_out[f].status == PBFT_WIRE_EDEFER;
  if (deferred) {  // the index comes back only now, and only for the host parser's sake
    std::vector<uint64_t> h_off;
    std::vector<uint32_t> h_len;
    std::vector<uint16_t> h_peer;
    const uint64_t* off = off_out;
    const uint32_t* flen = flen_out;
    if (!off) {
      h_off.resize(N);
      HIP_TRY(hipMemcpy(h_off.data(), d_off, 8 * N, hipMemcpyDeviceToHost));
      off = h_off.data();
    }
    if (!flen) {
      h_len.resize(N);
      HIP_TRY(hipMemcpy(h_len.data(), d_len, 4 * N, hipMemcpyDeviceToHost));
      flen = h_len.data();
    }
    if (seg_peer) {  // frame f's peer is its segment's: the heads say which frames a segment has
      h_peer.assign(N, 0xFFFF);
      for (uint32_t s = 0; s < S; ++s) {
        const uint64_t lo = seg_heads_out[s].first, hi = lo + seg_heads_out[s].n_frames;
        for (uint64_t f = lo; f < hi && f < N; ++f) h_peer[f] = seg_peer[s];
      }
    }
    rc = frames_settle(c, stream, off, flen, seg_peer ? h_peer.data() : nullptr, n_replicas, N, heads_out, d, d_heads);
    if (rc) return rc;
  }
  uint32_t* const d_idx = (uint32_t*)(d + o_idx);
  const uint16_t* const d_key = (const uint16_t*)(d + 150);
  rc = pbft_group_envelopes_device(c, d + 64, PBFT_RECORD_BYTES, d_key, PBFT_RECORD_BYTES, N, env_cap, d_idx,
                                   d + o_env, (uint32_t*)(d + o_n), c->stream);
  if (rc) return rc;
  rc = pbft_verify_records_device(c, d, N, c->d_bitmap, c->stream);
  if (rc) return rc;
  rc = pbft_tally_device(c, c->d_bitmap, d_key, PBFT_RECORD_BYTES, d_idx, 4, N, env_cap, c->n_keys, 0,
                         (uint64_t*)(d + o_set), (uint32_t*)(d + o_cnt), c->stream);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(out, c->d_bitmap, (N + 63) / 64 * 8, hipMemcpyDeviceToHost, c->stream));
  if (env_idx_out) HIP_TRY(hipMemcpyAsync(env_idx_out, d_idx, 4 * N, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(envelopes_out, d + o_env, env_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(n_env_out, d + o_n, 8, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(signers_out, d + o_set, set_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(count_out, d + o_cnt, cnt_bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return PBFT_OK;
}

// ---- connection streams in, signer sets out: the device half of pbft_replica_push_streams ----
// One staging, one enqueue of the whole chain over N = frame_cap rows (the index pads what the streams do not fill),
// one synchronisation.
struct admit_layout {
  frames_layout lay;
  uint32_t W;
  size_t env_bytes, set_bytes, o_soff, o_slen, o_shead, o_nfr, o_speer, o_idx, o_env, o_n, o_present, o_valid, o_cnt,
      o_cls, o_counts, o_clean, o_res, o_nres, o_pp, total;
  admit_layout(uint64_t stream_bytes, uint32_t S, uint64_t frame_cap, uint32_t env_cap, uint32_t residue_cap,
               uint32_t n_replicas)
      : lay(frame_cap, stream_bytes) {
    auto up = [](size_t x) { return (x + 15) & ~(size_t)15; };
    W = tally_words(n_replicas);
    env_bytes = (size_t)env_cap * PBFT_ENVELOPE_LEN;
    set_bytes = (size_t)env_cap * W * 8;
    o_soff = up(lay.total);
    o_slen = o_soff + 8 * (size_t)S;
    o_shead = o_slen + 8 * (size_t)S;
    o_nfr = o_shead + sizeof(pbft_seg_head) * (size_t)S;
    o_speer = o_nfr + 8;
    o_idx = up(o_speer + 2 * (size_t)S);
    o_env = o_idx + up(4 * (size_t)frame_cap);
    o_n = o_env + up(env_bytes + 16);
    o_present = o_n + 16;
    o_valid = o_present + up(set_bytes);
    o_cnt = o_valid + up(set_bytes);
    o_cls = o_cnt + up(4 * (size_t)env_cap);
    o_counts = o_cls + up((size_t)frame_cap);
    o_clean = o_counts + 32;
    o_res = o_clean + up(8 * (((size_t)frame_cap + 63) / 64));
    o_nres = o_res + sizeof(pbft_admit_residue) * (size_t)residue_cap;
    o_pp = o_nres + 16;  // (8-byte aligned: the PrePrepare heads of pbft_verify_streams_admit_pp)
    total = o_pp + sizeof(pbft_pp_head) * (size_t)residue_cap + 256;
  }
};

static int check_streams_admit_shape(pbft_ctx* c, uint64_t stream_bytes, uint32_t S, uint32_t n_replicas,
                                     uint64_t frame_cap, uint32_t env_cap, uint64_t log_window) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (n_replicas == 0 || n_replicas > 65535) return set_err(PBFT_EINVAL, "n_replicas out of range");
  if (S > pbft::IX_MAX_SEGMENTS) return set_err(PBFT_EINVAL, "more than 65536 segments");
  if (frame_cap == 0 || frame_cap > ((uint64_t)1 << 31)) return set_err(PBFT_EINVAL, "frame_cap out of range");
  if (env_cap == 0) return set_err(PBFT_EINVAL, "env_cap is 0");
  if (stream_bytes > pbft::IX_MAX_STREAM) return set_err(PBFT_EINVAL, "more than 2^31 stream bytes to index");
  return check_admit_shape(log_window, n_replicas, frame_cap);
}

int pbft_streams_admit_reserve(pbft_ctx* c, uint64_t max_stream_bytes, uint32_t max_segments, uint32_t n_replicas,
                               uint64_t frame_cap, uint32_t env_cap, uint32_t residue_cap, uint64_t log_window) {
  int rc = check_streams_admit_shape(c, max_stream_bytes, max_segments, n_replicas, frame_cap, env_cap, log_window);
  if (rc) return rc;
  if (c->in_flight) return set_err(PBFT_EBUSY, "async batch in flight");
  HIP_TRY(hipSetDevice(c->device));
  const admit_layout L(max_stream_bytes, max_segments, frame_cap, env_cap, residue_cap, n_replicas);
  if ((rc = ensure_stage(c, L.total, (frame_cap + 63) / 64)) != PBFT_OK) return rc;
  if ((rc = ensure_index(c, max_stream_bytes, max_segments)) != PBFT_OK) return rc;
  if ((rc = ensure_group(c, frame_cap)) != PBFT_OK) return rc;
  if ((rc = ensure_admit(c, pbft::admit_plane_bits(log_window, n_replicas), frame_cap)) != PBFT_OK) return rc;
  return ensure_work(c, frame_cap, true);
}

int pbft_wire_decode_preprepares_device(pbft_ctx* c, const uint8_t* d_stream, uint64_t stream_bytes,
                                        const pbft_admit_residue* d_res, const uint32_t* d_n_res, uint32_t residue_cap,
                                        pbft_pp_head* d_pp, void* stream) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (!d_res || !d_pp || (stream_bytes && !d_stream)) return set_err(PBFT_EINVAL, "null PrePrepare argument");
  if (((uintptr_t)d_stream & 15) || ((uintptr_t)d_res & 7) || ((uintptr_t)d_pp & 7) || ((uintptr_t)d_n_res & 3))
    return set_err(PBFT_EINVAL, "misaligned PrePrepare pointer");
  if (stream_bytes > pbft::IX_MAX_STREAM) return set_err(PBFT_EINVAL, "more than 2^31 stream bytes");
  if (residue_cap == 0) return PBFT_OK;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(launch_pp(d_stream, stream_bytes, d_res, d_n_res, residue_cap, d_pp, stream ? (hipStream_t)stream : c->stream));
  return PBFT_OK;
}

static int streams_admit(pbft_ctx* c, const uint8_t* stream, uint64_t stream_bytes, const uint64_t* seg_off,
                         const uint64_t* seg_len, const uint16_t* seg_peer, uint32_t S, uint32_t n_replicas,
                         uint64_t frame_cap, uint32_t env_cap, uint32_t residue_cap, uint64_t view, uint64_t h,
                         uint64_t log_window, pbft_seg_head* seg_heads_out, uint32_t* n_frames_out,
                         uint32_t* counts_out, uint8_t* envelopes_out, uint32_t* n_env_out, uint64_t* present_out,
                         uint64_t* valid_out, pbft_admit_residue* res_out, uint32_t* n_res_out, pbft_pp_head* pp_out) {
  int rc = check_streams_admit_shape(c, stream_bytes, S, n_replicas, frame_cap, env_cap, log_window);
  if (rc) return rc;
  if (c->in_flight) return set_err(PBFT_EBUSY, "async batch in flight");
  if (!n_frames_out || !counts_out || !envelopes_out || !n_env_out || !present_out || !valid_out || !n_res_out ||
      (residue_cap && !res_out) || (stream_bytes && !stream) || (S && (!seg_off || !seg_len || !seg_peer || !seg_heads_out)))
    return set_err(PBFT_EINVAL, "null streams argument");
  if (c->n_keys < n_replicas) return set_err(PBFT_ENOKEYS, "fewer keys installed than replicas");
  HIP_TRY(hipSetDevice(c->device));
  const admit_layout L(stream_bytes, S, frame_cap, env_cap, residue_cap, n_replicas);
  rc = ensure_stage(c, L.total, (frame_cap + 63) / 64);
  if (rc) return rc;
  uint8_t* const d = c->d_stage;
  const uint64_t N = frame_cap;
  pbft_frame_head* const d_heads = (pbft_frame_head*)(d + L.lay.heads);
  uint64_t* const d_off = (uint64_t*)(d + L.lay.off);
  uint32_t* const d_len = (uint32_t*)(d + L.lay.len);
  uint16_t* const d_peer = (uint16_t*)(d + L.lay.peer);
  uint32_t* const d_nfr = (uint32_t*)(d + L.o_nfr);
  uint32_t* const d_idx = (uint32_t*)(d + L.o_idx);
  const uint16_t* const d_key = (const uint16_t*)(d + 150);
  uint64_t* const d_clean = (uint64_t*)(d + L.o_clean);
  hipStream_t st = c->stream;
  if (stream_bytes) HIP_TRY(hipMemcpyAsync(d + L.lay.stream, stream, stream_bytes, hipMemcpyHostToDevice, st));
  if (S) {
    HIP_TRY(hipMemcpyAsync(d + L.o_soff, seg_off, 8 * (size_t)S, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d + L.o_slen, seg_len, 8 * (size_t)S, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d + L.o_speer, seg_peer, 2 * (size_t)S, hipMemcpyHostToDevice, st));
  }
  // with S = 0 the index still pads every row; its peer pointers must then both be null or both set: a dummy table
  rc = pbft_wire_index_streams_device(c, d + L.lay.stream, stream_bytes, (const uint64_t*)(d + L.o_soff),
                                      (const uint64_t*)(d + L.o_slen), (const uint16_t*)(d + L.o_speer), S, N, d_off,
                                      d_len, d_peer, (pbft_seg_head*)(d + L.o_shead), d_nfr, st);
  if (rc) return rc;
  rc = pbft_wire_decode_frames_device(c, d + L.lay.stream, stream_bytes, d_off, d_len, d_peer, n_replicas, N, d,
                                      d_heads, st);
  if (rc) return rc;
  rc = pbft_admit_device(c, d_heads, d, d_off, d_len, d_nfr, N, view, h, log_window, n_replicas, residue_cap,
                         d + L.o_cls, (uint32_t*)(d + L.o_counts), d_clean, (pbft_admit_residue*)(d + L.o_res),
                         (uint32_t*)(d + L.o_nres), st);
  if (rc) return rc;
  rc = pbft_group_envelopes_device(c, d + 64, PBFT_RECORD_BYTES, d_key, PBFT_RECORD_BYTES, N, env_cap, d_idx,
                                   d + L.o_env, (uint32_t*)(d + L.o_n), st);
  if (rc) return rc;
  rc = pbft_verify_records_device(c, d, N, c->d_bitmap, st);
  if (rc) return rc;
  rc = pbft_tally_device(c, d_clean, d_key, PBFT_RECORD_BYTES, d_idx, 4, N, env_cap, n_replicas, 0,
                         (uint64_t*)(d + L.o_present), (uint32_t*)(d + L.o_cnt), st);
  if (rc) return rc;
  rc = pbft_tally_device(c, c->d_bitmap, d_key, PBFT_RECORD_BYTES, d_idx, 4, N, env_cap, n_replicas, 0,
                         (uint64_t*)(d + L.o_valid), (uint32_t*)(d + L.o_cnt), st);
  if (rc) return rc;
  if (S) HIP_TRY(hipMemcpyAsync(seg_heads_out, d + L.o_shead, sizeof(pbft_seg_head) * (size_t)S, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(n_frames_out, d_nfr, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(counts_out, d + L.o_counts, 32, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(envelopes_out, d + L.o_env, L.env_bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(n_env_out, d + L.o_n, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(present_out, d + L.o_present, L.set_bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(valid_out, d + L.o_valid, L.set_bytes, hipMemcpyDeviceToHost, st));
  if (residue_cap)
    HIP_TRY(hipMemcpyAsync(res_out, d + L.o_res, sizeof(pbft_admit_residue) * (size_t)residue_cap,
                           hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(n_res_out, d + L.o_nres, 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  // The PrePrepares of the residue, where it lies: only now is it known whether there can be one, and how many entries
  // there are.  A call without a deferred frame ends here, as it always did.
  const uint32_t k = n_res_out[0] < residue_cap ? n_res_out[0] : residue_cap;
  if (pp_out && counts_out[PBFT_ADMIT_HOST] && k) {
    HIP_TRY(launch_pp(d + L.lay.stream, stream_bytes, d + L.o_res, nullptr, k, d + L.o_pp, st));
    HIP_TRY(hipMemcpyAsync(pp_out, d + L.o_pp, sizeof(pbft_pp_head) * (size_t)k, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
  }
  return PBFT_OK;
}

int pbft_verify_streams_admit(pbft_ctx* c, const uint8_t* stream, uint64_t stream_bytes, const uint64_t* seg_off,
                              const uint64_t* seg_len, const uint16_t* seg_peer, uint32_t S, uint32_t n_replicas,
                              uint64_t frame_cap, uint32_t env_cap, uint32_t residue_cap, uint64_t view, uint64_t h,
                              uint64_t log_window, pbft_seg_head* seg_heads_out, uint32_t* n_frames_out,
                              uint32_t* counts_out, uint8_t* envelopes_out, uint32_t* n_env_out, uint64_t* present_out,
                              uint64_t* valid_out, pbft_admit_residue* res_out, uint32_t* n_res_out) {
  return streams_admit(c, stream, stream_bytes, seg_off, seg_len, seg_peer, S, n_replicas, frame_cap, env_cap,
                       residue_cap, view, h, log_window, seg_heads_out, n_frames_out, counts_out, envelopes_out,
                       n_env_out, present_out, valid_out, res_out, n_res_out, nullptr);
}

int pbft_verify_streams_admit_pp(pbft_ctx* c, const uint8_t* stream, uint64_t stream_bytes, const uint64_t* seg_off,
                                 const uint64_t* seg_len, const uint16_t* seg_peer, uint32_t S, uint32_t n_replicas,
                                 uint64_t frame_cap, uint32_t env_cap, uint32_t residue_cap, uint64_t view, uint64_t h,
                                 uint64_t log_window, pbft_seg_head* seg_heads_out, uint32_t* n_frames_out,
                                 uint32_t* counts_out, uint8_t* envelopes_out, uint32_t* n_env_out,
                                 uint64_t* present_out, uint64_t* valid_out, pbft_admit_residue* res_out,
                                 uint32_t* n_res_out, pbft_pp_head* pp_out) {
  return streams_admit(c, stream, stream_bytes, seg_off, seg_len, seg_peer, S, n_replicas, frame_cap, env_cap,
                       residue_cap, view, h, log_window, seg_heads_out, n_frames_out, counts_out, envelopes_out,
                       n_env_out, present_out, valid_out, res_out, n_res_out, pp_out);
}

static int run_digest(pbft_ctx* c, int kind, const uint8_t* data, const uint64_t* offsets, const uint32_t* lens,
                      uint64_t N, uint8_t* out) {
  if (!c || (N && (!offsets || !lens || !out))) return set_err(PBFT_EINVAL, "null argument");
  if (c->in_flight) return set_err(PBFT_EBUSY, "async batch in flight");
  if (N == 0) return PBFT_OK;
  uint64_t total = 0;
  for (uint64_t i = 0; i < N; ++i) {
    const uint64_t end = offsets[i] + lens[i];
    if (end > total) total = end;
  }
  if (total && !data) return set_err(PBFT_EINVAL, "null data");
  HIP_TRY(hipSetDevice(c->device));
  const size_t outb = (kind == 0 ? 64 : 32) * N;
  const size_t offO = (total + 64 + 255) & ~(size_t)255;
  const size_t offL = offO + ((8 * N + 255) & ~(size_t)255);
  const size_t offOut = offL + ((4 * N + 255) & ~(size_t)255);
  int rc = ensure_stage(c, offOut + outb, 1);
  if (rc) return rc;
  if (total) HIP_TRY(hipMemcpyAsync(c->d_stage, data, total, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->d_stage + offO, offsets, 8 * N, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->d_stage + offL, lens, 4 * N, hipMemcpyHostToDevice, c->stream));
  const unsigned blocks = (unsigned)((N + BLOCK - 1) / BLOCK);
  if (kind == 0)
    hipLaunchKernelGGL(digest_kernel<0>, dim3(blocks), dim3(BLOCK), 0, c->stream, c->d_stage,
                       (const uint64_t*)(c->d_stage + offO), (const uint32_t*)(c->d_stage + offL), N,
                       c->d_stage + offOut);
  else
    hipLaunchKernelGGL(digest_kernel<1>, dim3(blocks), dim3(BLOCK), 0, c->stream, c->d_stage,
                       (const uint64_t*)(c->d_stage + offO), (const uint32_t*)(c->d_stage + offL), N,
                       c->d_stage + offOut);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, c->d_stage + offOut, outb, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return PBFT_OK;
}

int pbft_digest_blake2b512(pbft_ctx* c, const uint8_t* data, const uint64_t* offsets, const uint32_t* lens,
                           uint64_t N, uint8_t* out) {
  return run_digest(c, 0, data, offsets, lens, N, out);
}

int pbft_digest_sha256(pbft_ctx* c, const uint8_t* data, const uint64_t* offsets, const uint32_t* lens, uint64_t N,
                       uint8_t* out) {
  return run_digest(c, 1, data, offsets, lens, N, out);
}

int pbft_sign_batch(pbft_ctx* c, const uint8_t* seeds, uint32_t n_seeds, const uint16_t* seed_idx,
                    const uint8_t* msg, uint32_t msg_len, uint32_t msg_stride, uint64_t N, uint8_t* R, uint8_t* S,
                    uint8_t* pub) {
  if (!c || !seeds || n_seeds == 0 || (N && (!seed_idx || !R || !S)) || (msg_len && !msg) || msg_stride < msg_len)
    return set_err(PBFT_EINVAL, "bad sign arguments");
  if (c->in_flight) return set_err(PBFT_EBUSY, "async batch in flight");
  for (uint64_t i = 0; i < N; ++i)
    if (seed_idx[i] >= n_seeds) return set_err(PBFT_EINVAL, "seed index out of range");
  HIP_TRY(hipSetDevice(c->device));
  const size_t offI = (32 * (size_t)n_seeds + 255) & ~(size_t)255;
  const size_t offM = offI + ((2 * N + 255) & ~(size_t)255);
  const size_t offR = offM + (((size_t)msg_stride * N + 64 + 255) & ~(size_t)255);
  const size_t offS = offR + 32 * N;
  const size_t offP = offS + 32 * N;
  int rc = ensure_stage(c, offP + 32 * (size_t)n_seeds, 1);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c->d_stage, seeds, 32 * (size_t)n_seeds, hipMemcpyHostToDevice, c->stream));
  if (N) HIP_TRY(hipMemcpyAsync(c->d_stage + offI, seed_idx, 2 * N, hipMemcpyHostToDevice, c->stream));
  if (N && msg_len) HIP_TRY(hipMemcpyAsync(c->d_stage + offM, msg, (size_t)msg_stride * N, hipMemcpyHostToDevice, c->stream));
  uint64_t n_launch = N;
  const uint16_t* d_idx = (const uint16_t*)(c->d_stage + offI);
  std::vector<uint16_t> all;
  if (pub && N == 0) n_launch = 0;
  if (n_launch) {
    const unsigned blocks = (unsigned)((n_launch + BLOCK - 1) / BLOCK);
    if (msg_len == PBFT_ENVELOPE_LEN)
      launch_sign(PBFT_ENVELOPE_LEN, dim3(blocks), dim3(BLOCK), 0, c->stream,
                         (const uint32_t*)c->d_stage, d_idx, c->d_stage + offM, msg_len, msg_stride, n_launch,
                         c->d_tabB, (uint32_t*)(c->d_stage + offR), (uint32_t*)(c->d_stage + offS),
                         pub ? (uint32_t*)(c->d_stage + offP) : nullptr, n_seeds);
    else
      launch_sign(-1, dim3(blocks), dim3(BLOCK), 0, c->stream, (const uint32_t*)c->d_stage,
                         d_idx, c->d_stage + offM, msg_len, msg_stride, n_launch, c->d_tabB,
                         (uint32_t*)(c->d_stage + offR), (uint32_t*)(c->d_stage + offS),
                         pub ? (uint32_t*)(c->d_stage + offP) : nullptr, n_seeds);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(R, c->d_stage + offR, 32 * N, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(S, c->d_stage + offS, 32 * N, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (pub) {
    // public keys of seeds that no lane used are derived by a one-lane-per-seed pass
    std::vector<uint16_t> idx(n_seeds);
    for (uint32_t j = 0; j < n_seeds; ++j) idx[j] = (uint16_t)j;
    uint16_t* d_i2 = nullptr;
    uint32_t *d_r2 = nullptr, *d_s2 = nullptr;
    HIP_TRY(hipMalloc(&d_i2, 2 * (size_t)n_seeds));
    HIP_TRY(hipMalloc(&d_r2, 64 * (size_t)n_seeds));
    d_s2 = d_r2 + 8 * (size_t)n_seeds;
    HIP_TRY(hipMemcpyAsync(d_i2, idx.data(), 2 * (size_t)n_seeds, hipMemcpyHostToDevice, c->stream));
    launch_sign(0, dim3((n_seeds + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, c->stream,
                       (const uint32_t*)c->d_stage, (const uint16_t*)d_i2, (const uint8_t*)nullptr, 0u, 0u,
                       (uint64_t)n_seeds, c->d_tabB, d_r2, d_s2, (uint32_t*)(c->d_stage + offP), n_seeds);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(pub, c->d_stage + offP, 32 * (size_t)n_seeds, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    (void)hipFree(d_i2);
    (void)hipFree(d_r2);
  }
  return PBFT_OK;
}

// ---- replica egress: the round's own votes signed and framed on the device (include/pbft_wire.h; egress.hip) ----
int pbft_sign_set_seed(pbft_ctx* c, const uint8_t* seed, uint32_t replica, uint8_t* pub_out) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (seed && replica > pbft::EG_MAX_REPLICA) return set_err(PBFT_EINVAL, "replica index above 65535");
  if (c->in_flight) return set_err(PBFT_EBUSY, "async batch in flight");
  HIP_TRY(hipSetDevice(c->device));
  if (!seed) {
    c->sign_set = false;
    if (c->d_sign_key) {
      HIP_TRY(hipMemsetAsync(c->d_sign_key, 0, 4 * EGRESS_KEY_WORDS, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
    }
    return PBFT_OK;
  }
  if (!c->d_sign_key) {
    if (hipMalloc(&c->d_sign_key, 4 * EGRESS_KEY_WORDS) != hipSuccess) return set_err(PBFT_ENOMEM, "signing key alloc");
    HIP_TRY(hipMemsetAsync(c->d_sign_key, 0, 4 * EGRESS_KEY_WORDS, c->stream));
  }
  c->sign_set = false;
  HIP_TRY(hipMemcpyAsync(c->d_sign_key + EGRESS_KEY_SEED, seed, 32, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(launch_egress_seed(c->d_sign_key, replica, c->d_tabB, c->stream));  // (zeroes the staged seed)
  uint8_t pub[32];
  HIP_TRY(hipMemcpyAsync(pub, c->d_sign_key + 16, 32, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  // the identity's PeerId text for the client replies (reply.hip reads it; base58 is host work, once per seed)
  if (pbft::rp_peer_id_b58(pub, (uint8_t*)c->sign_peer_id) != pbft::RP_PEER_ID_B58)  // (sign_set stays false)
    return set_err(PBFT_EINVAL, "peer id text is not 52 characters");
  HIP_TRY(hipMemcpyAsync(c->d_sign_key + REPLY_KEY_PEER_ID, c->sign_peer_id, pbft::RP_PEER_ID_B58,
                         hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (pub_out) memcpy(pub_out, pub, 32);
  c->sign_set = true;
  c->sign_replica = replica;
  return PBFT_OK;
}

static int ensure_egress(pbft_ctx* c, uint64_t N) {
  return grow_device(&c->d_egress, &c->egress_cap, egress_ws_bytes(N ? N : 1), "egress workspace alloc");
}

int pbft_egress_reserve(pbft_ctx* c, uint64_t max_n) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (max_n > pbft::EG_MAX_N) return set_err(PBFT_EINVAL, "more than 2^24 votes to sign");
  HIP_TRY(hipSetDevice(c->device));
  return ensure_egress(c, max_n);
}

int pbft_sign_votes_frames_device(pbft_ctx* c, const uint8_t* d_env, uint32_t env_stride, uint64_t N, uint8_t* d_out,
                                  uint64_t out_cap, uint64_t* d_frame_off, uint8_t* d_sigs, void* stream) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (!c->sign_set) return set_err(PBFT_EINVAL, "no signing seed (pbft_sign_set_seed)");
  if (N > pbft::EG_MAX_N) return set_err(PBFT_EINVAL, "more than 2^24 votes to sign");
  if (!d_frame_off || (N && !d_env) || (out_cap && !d_out) || (N && env_stride < pbft::EG_ENV_BYTES))
    return set_err(PBFT_EINVAL, "bad egress argument");
  if (((uintptr_t)d_frame_off & 7) || ((uintptr_t)d_sigs & 3)) return set_err(PBFT_EINVAL, "misaligned egress pointer");
  HIP_TRY(hipSetDevice(c->device));
  int rc = ensure_egress(c, N);
  if (rc) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  HIP_TRY(launch_egress(d_env, env_stride, N, c->d_sign_key, c->d_tabB, (uint64_t*)c->d_egress, d_out, out_cap,
                        d_frame_off, d_sigs, c->egress_block, c->egress_direct, st));
  return PBFT_OK;
}

int pbft_sign_votes_frames(pbft_ctx* c, const uint8_t* envelopes, uint32_t env_stride, uint64_t N, uint8_t* out,
                           size_t cap, size_t* len, uint64_t* frame_off, uint8_t* sigs) {
  if (!c || !len) return set_err(PBFT_EINVAL, "null egress argument");
  *len = 0;
  if (!c->sign_set) return set_err(PBFT_EINVAL, "no signing seed (pbft_sign_set_seed)");
  if (N > pbft::EG_MAX_N) return set_err(PBFT_EINVAL, "more than 2^24 votes to sign");
  if ((N && (!envelopes || env_stride < pbft::EG_ENV_BYTES)) || (cap && !out))
    return set_err(PBFT_EINVAL, "bad egress argument");
  if (c->in_flight) return set_err(PBFT_EBUSY, "async batch in flight");
  size_t need = 0;  // the layout is a function of the envelopes and the replica index: known before anything runs
  for (uint64_t i = 0; i < N; ++i) need += pbft::eg_env_frame_len(envelopes + (size_t)env_stride * i, c->sign_replica);
  *len = need;
  if (need > cap) return set_err(PBFT_EINVAL, "output buffer too small for the frames");
  if (N == 0) {
    if (frame_off) frame_off[0] = 0;
    return PBFT_OK;
  }
  HIP_TRY(hipSetDevice(c->device));
  const sign_layout L = sign_votes_layout(env_stride, N, need);
  int rc = grow_device(&c->d_sign_io, &c->sign_io_cap, L.total, "egress buffers alloc");
  if (rc) return rc;
  rc = ensure_egress(c, N);
  if (rc) return rc;
  uint8_t* d = c->d_sign_io;
  HIP_TRY(hipMemcpyAsync(d, envelopes, sign_votes_env_bytes(env_stride, N), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(launch_egress(d, env_stride, N, c->d_sign_key, c->d_tabB, (uint64_t*)c->d_egress, d + L.out, need,
                        (uint64_t*)(d + L.out_off), sigs ? d + L.sig : nullptr, c->egress_block, c->egress_direct,
                        c->stream));
  if (need) HIP_TRY(hipMemcpyAsync(out, d + L.out, need, hipMemcpyDeviceToHost, c->stream));
  if (frame_off)
    HIP_TRY(hipMemcpyAsync(frame_off, d + L.out_off, 8 * (size_t)(N + 1), hipMemcpyDeviceToHost, c->stream));
  if (sigs) HIP_TRY(hipMemcpyAsync(sigs, d + L.sig, 64 * (size_t)N, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return PBFT_OK;
}

// ---- what the blocking proposal and reply forms share: N items (payload bytes, offsets, lengths, timestamps, clients)
// up, the device's packed bytes, digests and signatures back, the general items completed on the host (sign_host.h) ----
static int sign_upload(pbft_ctx* c, const sign_layout& L, const uint8_t* payload, uint64_t payload_bytes,
                       const uint64_t* off, const uint32_t* len, const uint64_t* timestamp, const char* clients,
                       uint64_t N) {
  uint8_t* d = c->d_sign_io;
  if (payload_bytes) HIP_TRY(hipMemcpyAsync(d, payload, payload_bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d + L.off, off, 8 * (size_t)N, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d + L.len, len, 4 * (size_t)N, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d + L.ts, timestamp, 8 * (size_t)N, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d + L.cl, clients, 64 * (size_t)N, hipMemcpyHostToDevice, c->stream));
  return PBFT_OK;
}

// Where the device's results go on the host.  All items the device's: its packed bytes are the answer and go straight
// to `out`.  With general items they go to a temporary for the merge, and so does each output the merge reads
// (signatures; digests too where merge_digests) that the caller left null.
struct sign_back {
  std::vector<uint8_t> tmp_stream, tmp_d, tmp_s;
  uint8_t *stream, *digests, *sigs;
  sign_back(uint64_t N, const sign_split& s, bool merge_digests, uint8_t* out, uint8_t* digests_, uint8_t* sigs_)
      : stream(out), digests(digests_), sigs(sigs_) {
    if (!s.n_general) return;
    tmp_stream.resize(s.dev_bytes ? s.dev_bytes : 1);
    stream = tmp_stream.data();
    if (merge_digests && !digests) { tmp_d.resize(64 * (size_t)N); digests = tmp_d.data(); }
    if (!sigs) { tmp_s.resize(64 * (size_t)N); sigs = tmp_s.data(); }
  }
  sign_back(const sign_back&) = delete;  // (the pointers may be into the temporaries)
};

// What was asked for, copied back; returns with the stream idle.
static int sign_read_back(pbft_ctx* c, const sign_layout& L, uint64_t N, size_t dev_bytes, const sign_back& to) {
  const uint8_t* d = c->d_sign_io;
  if (dev_bytes) HIP_TRY(hipMemcpyAsync(to.stream, d + L.out, dev_bytes, hipMemcpyDeviceToHost, c->stream));
  if (to.digests) HIP_TRY(hipMemcpyAsync(to.digests, d + L.dig, 64 * (size_t)N, hipMemcpyDeviceToHost, c->stream));
  if (to.sigs) HIP_TRY(hipMemcpyAsync(to.sigs, d + L.sig, 64 * (size_t)N, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return PBFT_OK;
}

// ---- the primary's proposals: requests hashed, PrePrepares signed and framed on the device (include/pbft_wire.h;
// propose.hip) ----
static int ensure_propose(pbft_ctx* c, uint64_t N) {
  return grow_device(&c->d_propose, &c->propose_cap, propose_ws_bytes(N ? N : 1), "propose workspace alloc");
}

int pbft_propose_reserve(pbft_ctx* c, uint64_t max_n) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (max_n > pbft::PR_MAX_N) return set_err(PBFT_EINVAL, "more than 2^24 requests to propose");
  HIP_TRY(hipSetDevice(c->device));
  return ensure_propose(c, max_n);
}

int pbft_sign_preprepares_frames_device(pbft_ctx* c, const uint8_t* d_ops, uint64_t ops_bytes, const uint64_t* d_op_off,
                                        const uint32_t* d_op_len, const uint64_t* d_timestamp, const uint8_t* d_clients,
                                        uint64_t view, uint64_t first_seq, uint64_t N, uint8_t* d_out, uint64_t out_cap,
                                        uint64_t* d_frame_off, uint8_t* d_digests, uint8_t* d_sigs, uint8_t* d_status,
                                        void* stream) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (!c->sign_set) return set_err(PBFT_EINVAL, "no signing seed (pbft_sign_set_seed)");
  if (N > pbft::PR_MAX_N) return set_err(PBFT_EINVAL, "more than 2^24 requests to propose");
  if (N && first_seq + (N - 1) < first_seq) return set_err(PBFT_EINVAL, "sequence numbers wrap");
  if (!d_frame_off || (ops_bytes && !d_ops) || (out_cap && !d_out) ||
      (N && (!d_op_off || !d_op_len || !d_timestamp || !d_clients || !d_digests || !d_sigs || !d_status)))
    return set_err(PBFT_EINVAL, "bad propose argument");
  if (((uintptr_t)d_ops & 15) || ((uintptr_t)d_op_off & 7) || ((uintptr_t)d_op_len & 3) || ((uintptr_t)d_timestamp & 7) ||
      ((uintptr_t)d_frame_off & 7) || ((uintptr_t)d_digests & 3) || ((uintptr_t)d_sigs & 3))
    return set_err(PBFT_EINVAL, "misaligned propose pointer");
  HIP_TRY(hipSetDevice(c->device));
  int rc = ensure_propose(c, N);
  if (rc) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  HIP_TRY(launch_propose(d_ops, ops_bytes, d_op_off, d_op_len, d_timestamp, d_clients, view, first_seq, N,
                         c->d_sign_key, c->d_tabB, (uint64_t*)c->d_propose, d_out, out_cap, d_frame_off, d_digests,
                         d_sigs, d_status, c->propose_width, st));
  return PBFT_OK;
}

int pbft_sign_preprepares_frames(pbft_ctx* c, const uint8_t* ops, uint64_t ops_bytes, const uint64_t* op_off,
                                 const uint32_t* op_len, const uint64_t* timestamp, const char* clients, uint64_t view,
                                 uint64_t first_seq, uint64_t N, uint8_t* out, size_t cap, size_t* len,
                                 uint64_t* frame_off, uint8_t* digests, uint8_t* sigs, uint8_t* status) {
  if (!c || !len) return set_err(PBFT_EINVAL, "null propose argument");
  *len = 0;
  if (!c->sign_set) return set_err(PBFT_EINVAL, "no signing seed (pbft_sign_set_seed)");
  if (N > pbft::PR_MAX_N) return set_err(PBFT_EINVAL, "more than 2^24 requests to propose");
  if ((N && (!op_off || !op_len || !timestamp || !clients)) || (ops_bytes && !ops) || (cap && !out))
    return set_err(PBFT_EINVAL, "bad propose argument");
  if (N && first_seq + (N - 1) < first_seq) return set_err(PBFT_EINVAL, "sequence numbers wrap");
  if (c->in_flight) return set_err(PBFT_EBUSY, "async batch in flight");
  if (!sign_spans_inside(op_off, op_len, N, ops_bytes)) return set_err(PBFT_EINVAL, "an operation outside ops_bytes");
  // the layout is a function of the requests and the replica index: known before anything runs
  std::vector<uint64_t> h_off(N + 1);
  std::vector<uint8_t> h_st(N ? N : 1);
  size_t need = 0;
  int rc = pbft_wire_encode_preprepares(N, view, first_seq, ops, op_off, op_len, timestamp, clients, c->sign_replica,
                                        nullptr, nullptr, nullptr, 0, &need, h_off.data(), h_st.data());
  if (rc) return set_err(PBFT_EINVAL, "bad propose argument");
  *len = need;
  if (need > cap) return set_err(PBFT_EINVAL, "output buffer too small for the frames");
  if (frame_off) memcpy(frame_off, h_off.data(), 8 * (size_t)(N + 1));
  if (N == 0) return PBFT_OK;
  const sign_split split = sign_count(h_off.data(), h_st.data(), N, PBFT_PROPOSE_OK);  // the device writes the OK ones
  if (status) memcpy(status, h_st.data(), N);
  HIP_TRY(hipSetDevice(c->device));
  const sign_layout L(N, ops_bytes, split.dev_bytes);
  rc = grow_device(&c->d_sign_io, &c->sign_io_cap, L.total, "propose buffers alloc");
  if (rc) return rc;
  rc = ensure_propose(c, N);
  if (rc) return rc;
  rc = sign_upload(c, L, ops, ops_bytes, op_off, op_len, timestamp, clients, N);
  if (rc) return rc;
  uint8_t* d = c->d_sign_io;
  HIP_TRY(launch_propose(d, ops_bytes, (const uint64_t*)(d + L.off), (const uint32_t*)(d + L.len),
                         (const uint64_t*)(d + L.ts), d + L.cl, view, first_seq, N, c->d_sign_key, c->d_tabB,
                         (uint64_t*)c->d_propose, d + L.out, split.dev_bytes, (uint64_t*)(d + L.out_off), d + L.dig,
                         d + L.sig, d + L.st, c->propose_width, c->stream));
  const sign_back back(N, split, /*merge_digests=*/true, out, digests, sigs);
  rc = sign_read_back(c, L, N, split.dev_bytes, back);
  if (rc) return rc;
  if (!split.n_general) return PBFT_OK;
  // the complete stream, on the host: the device's frames in order, the others from the general encoder
  const uint64_t off1 = 0;
  auto general = [&](uint64_t i, uint8_t* to, size_t fl, size_t* got) {
    return pbft_wire_encode_preprepares(1, view, first_seq + i, ops + op_off[i], &off1, op_len + i, timestamp + i,
                                        clients + 64 * i, c->sign_replica, back.digests + 64 * i, back.sigs + 64 * i, to,
                                        fl, got, nullptr, nullptr);
  };
  if (!sign_merge(N, h_off.data(), h_st.data(), PBFT_PROPOSE_OK, back.stream, out, general))
    return set_err(PBFT_EINVAL, "general frame encode");
  return PBFT_OK;
}

// ---- client replies: results hashed with their clients, the replies signed and written on the device
// (include/pbft_wire.h; reply.hip) ----
static int ensure_reply(pbft_ctx* c, uint64_t N) {
  return grow_device(&c->d_reply, &c->reply_cap, reply_ws_bytes(N ? N : 1), "reply workspace alloc");
}

int pbft_reply_reserve(pbft_ctx* c, uint64_t max_n) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (max_n > pbft::RP_MAX_N) return set_err(PBFT_EINVAL, "more than 2^24 replies");
  HIP_TRY(hipSetDevice(c->device));
  return ensure_reply(c, max_n);
}

int pbft_sign_replies_device(pbft_ctx* c, const uint8_t* d_results, uint64_t results_bytes, const uint64_t* d_res_off,
                             const uint32_t* d_res_len, const uint64_t* d_timestamp, const uint8_t* d_clients,
                             uint64_t view, uint64_t N, uint8_t* d_out, uint64_t out_cap, uint64_t* d_reply_off,
                             uint8_t* d_digests, uint8_t* d_sigs, uint8_t* d_status, void* stream) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (!c->sign_set) return set_err(PBFT_EINVAL, "no signing seed (pbft_sign_set_seed)");
  if (N > pbft::RP_MAX_N) return set_err(PBFT_EINVAL, "more than 2^24 replies");
  if (!d_reply_off || (results_bytes && !d_results) || (out_cap && !d_out) ||
      (N && (!d_res_off || !d_res_len || !d_timestamp || !d_clients || !d_digests || !d_sigs || !d_status)))
    return set_err(PBFT_EINVAL, "bad reply argument");
  if (((uintptr_t)d_results & 15) || ((uintptr_t)d_res_off & 7) || ((uintptr_t)d_res_len & 3) ||
      ((uintptr_t)d_timestamp & 7) || ((uintptr_t)d_reply_off & 7) || ((uintptr_t)d_digests & 3) || ((uintptr_t)d_sigs & 3))
    return set_err(PBFT_EINVAL, "misaligned reply pointer");
  HIP_TRY(hipSetDevice(c->device));
  int rc = ensure_reply(c, N);
  if (rc) return rc;
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  HIP_TRY(launch_reply(d_results, results_bytes, d_res_off, d_res_len, d_timestamp, d_clients, view, N, c->d_sign_key,
                       c->d_tabB, (uint64_t*)c->d_reply, d_out, out_cap, d_reply_off, d_digests, d_sigs, d_status, st));
  return PBFT_OK;
}

int pbft_sign_replies(pbft_ctx* c, const uint8_t* results, uint64_t results_bytes, const uint64_t* res_off,
                      const uint32_t* res_len, const uint64_t* timestamp, const char* clients, uint64_t view, uint64_t N,
                      uint8_t* out, size_t cap, size_t* len, uint64_t* reply_off, uint8_t* digests, uint8_t* sigs,
                      uint8_t* status) {
  if (!c || !len) return set_err(PBFT_EINVAL, "null reply argument");
  *len = 0;
  if (!c->sign_set) return set_err(PBFT_EINVAL, "no signing seed (pbft_sign_set_seed)");
  if (N > pbft::RP_MAX_N) return set_err(PBFT_EINVAL, "more than 2^24 replies");
  if ((N && (!res_off || !res_len || !timestamp || !clients)) || (results_bytes && !results) || (cap && !out))
    return set_err(PBFT_EINVAL, "bad reply argument");
  if (c->in_flight) return set_err(PBFT_EBUSY, "async batch in flight");
  if (!sign_spans_inside(res_off, res_len, N, results_bytes))
    return set_err(PBFT_EINVAL, "a result outside results_bytes");
  // the layout is a function of the results, the timestamps and the replica index: known before anything runs
  std::vector<uint64_t> h_off(N + 1);
  std::vector<uint8_t> h_st(N ? N : 1);
  size_t need = 0;
  int rc = pbft_wire_encode_replies(N, view, timestamp, results, res_off, res_len, c->sign_replica, nullptr, nullptr,
                                    nullptr, 0, &need, h_off.data(), h_st.data());
  if (rc) return set_err(PBFT_EINVAL, "bad reply argument");
  *len = need;
  if (reply_off) memcpy(reply_off, h_off.data(), 8 * (size_t)(N + 1));
  if (status && N) memcpy(status, h_st.data(), N);
  if (!out && cap == 0) return PBFT_OK;  // the size query
  if (need > cap) return set_err(PBFT_EINVAL, "output buffer too small for the replies");
  if (N == 0) return PBFT_OK;
  const sign_split split = sign_count(h_off.data(), h_st.data(), N, PBFT_REPLY_OK);  // the device writes the OK ones
  HIP_TRY(hipSetDevice(c->device));
  const sign_layout L(N, results_bytes, split.dev_bytes);
  rc = grow_device(&c->d_sign_io, &c->sign_io_cap, L.total, "reply buffers alloc");
  if (rc) return rc;
  rc = ensure_reply(c, N);
  if (rc) return rc;
  rc = sign_upload(c, L, results, results_bytes, res_off, res_len, timestamp, clients, N);
  if (rc) return rc;
  uint8_t* d = c->d_sign_io;
  HIP_TRY(launch_reply(d, results_bytes, (const uint64_t*)(d + L.off), (const uint32_t*)(d + L.len),
                       (const uint64_t*)(d + L.ts), d + L.cl, view, N, c->d_sign_key, c->d_tabB, (uint64_t*)c->d_reply,
                       d + L.out, split.dev_bytes, (uint64_t*)(d + L.out_off), d + L.dig, d + L.sig, d + L.st,
                       c->stream));
  const sign_back back(N, split, /*merge_digests=*/false, out, digests, sigs);  // (a reply's text holds no digest)
  rc = sign_read_back(c, L, N, split.dev_bytes, back);
  if (rc) return rc;
  if (!split.n_general) return PBFT_OK;
  // the complete stream, on the host: the device's texts in order, the others from the general encoder
  const uint64_t off1 = 0;
  auto general = [&](uint64_t i, uint8_t* to, size_t tl, size_t* got) {
    return pbft_wire_encode_replies(1, view, timestamp + i, results + res_off[i], &off1, res_len + i, c->sign_replica,
                                    c->sign_peer_id, back.sigs + 64 * i, to, tl, got, nullptr, nullptr);
  };
  if (!sign_merge(N, h_off.data(), h_st.data(), PBFT_REPLY_OK, back.stream, out, general))
    return set_err(PBFT_EINVAL, "general reply encode");
  return PBFT_OK;
}

// ---- the client's side: signed replies in, certificates out (include/pbft_wire.h; accept.hip; rule: accept_core.h) ----
static_assert(sizeof(pbft_accept_head) == sizeof(pbft::accept_head) && sizeof(pbft_accept_cert) == sizeof(pbft::accept_cert),
              "accept.hip writes pbft_accept_head and pbft_accept_cert");

// Device staging of pbft_accept_replies: records | heads | off | len | client_idx | clients | env_idx | envelopes | n_env
// | signer sets | counts | certs | (16-byte aligned) texts
struct accept_layout {
  size_t heads, off, len, ci, cl, idx, env, n_env, set, cnt, cert, text, total;
  accept_layout(uint64_t N, uint64_t text_bytes, uint32_t n_clients, uint32_t env_cap, uint32_t W) {
    auto up = [](size_t b) { return (b + 15) & ~(size_t)15; };
    heads = PBFT_RECORD_BYTES * (size_t)N;
    off = heads + sizeof(pbft_accept_head) * (size_t)N;
    len = off + up(8 * (size_t)N);
    ci = len + up(4 * (size_t)N);
    cl = ci + up(4 * (size_t)N);
    idx = cl + up(64 * (size_t)n_clients);
    env = idx + up(4 * (size_t)N);
    n_env = env + up((size_t)env_cap * PBFT_ENVELOPE_LEN + 16);
    set = n_env + 16;
    cnt = set + up((size_t)env_cap * W * 8);
    cert = cnt + up((size_t)env_cap * 4);
    text = cert + up((size_t)env_cap * sizeof(pbft_accept_cert));
    total = text + up((size_t)text_bytes) + 16;
  }
};

static int ensure_accept_io(pbft_ctx* c, size_t bytes) {
  return grow_device(&c->d_accept_io, &c->accept_io_cap, bytes, "accept staging alloc");
}

// The PeerId texts of the installed keys, from the key set's host copy; blocking.
static int accept_build_table(pbft_ctx* c) {
  keyset* k = c->ks;
  if (!k || c->n_keys == 0) return set_err(PBFT_ENOKEYS, "pbft_verify_set_keys not called");
  if (k->h_keys.size() != 32 * (size_t)k->n) return set_err(PBFT_EINVAL, "the key set holds no host copy of its keys");
  if (c->accept_gen == k->gen && c->d_accept_pid && c->accept_pid_cap >= k->n) return PBFT_OK;
  if (c->accept_pid_cap < k->n) {
    if (c->d_accept_pid) HIP_TRY(hipFree(c->d_accept_pid));
    c->d_accept_pid = nullptr;
    c->accept_pid_cap = 0;
    c->accept_gen = 0;
    if (hipMalloc(&c->d_accept_pid, (size_t)pbft::RP_PEER_ID_B58 * k->n) != hipSuccess)
      return set_err(PBFT_ENOMEM, "peer id table alloc");
    c->accept_pid_cap = k->n;
  }
  std::vector<uint8_t> t((size_t)pbft::RP_PEER_ID_B58 * k->n);
  for (uint32_t i = 0; i < k->n; ++i)
    if (pbft::rp_peer_id_b58(k->h_keys.data() + 32 * (size_t)i, t.data() + (size_t)pbft::RP_PEER_ID_B58 * i) !=
        pbft::RP_PEER_ID_B58)
      return set_err(PBFT_EINVAL, "peer id text");
  c->accept_gen = 0;
  HIP_TRY(hipStreamSynchronize(c->stream));  // (no launch of this context still reads the old table)
  HIP_TRY(hipMemcpy(c->d_accept_pid, t.data(), t.size(), hipMemcpyHostToDevice));
  c->accept_gen = k->gen;
  return PBFT_OK;
}

int pbft_accept_reserve(pbft_ctx* c, uint64_t max_n) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (max_n > pbft::AC_MAX_N) return set_err(PBFT_EINVAL, "more than 2^24 replies");
  if (c->in_flight) return set_err(PBFT_EBUSY, "async batch in flight");
  HIP_TRY(hipSetDevice(c->device));
  int rc = accept_build_table(c);
  if (rc) return rc;
  // the blocking form's staging for max_n replies of the shortest text, one client and max_n envelopes: a call that
  // needs more grows it
  const accept_layout lay(max_n, pbft::RP_TEXT_MIN * max_n, 1, (uint32_t)max_n, tally_words(c->n_keys));
  return ensure_accept_io(c, lay.total);
}

static int check_accept_decode_args(pbft_ctx* c, const void* d_text, uint64_t text_bytes, const void* d_off,
                                    const void* d_len, const void* d_ci, const void* d_clients, uint32_t n_clients,
                                    uint64_t N, const void* d_records, const void* d_heads) {
  if (N > pbft::AC_MAX_N) return set_err(PBFT_EINVAL, "more than 2^24 replies");
  if (text_bytes > pbft::AC_MAX_TEXT_BYTES) return set_err(PBFT_EINVAL, "more than 2^31 bytes of texts");
  if (N && (!d_off || !d_len || !d_records || !d_heads || (text_bytes && !d_text) || (n_clients && !d_clients)))
    return set_err(PBFT_EINVAL, "null accept argument");
  if (((uintptr_t)d_text & 15) || ((uintptr_t)d_off & 7) || ((uintptr_t)d_len & 3) || ((uintptr_t)d_ci & 3) ||
      ((uintptr_t)d_records & 15) || ((uintptr_t)d_heads & 7))
    return set_err(PBFT_EINVAL, "misaligned accept pointer");
  if (c->n_keys == 0 || !c->ks) return set_err(PBFT_ENOKEYS, "pbft_verify_set_keys not called");
  if (!c->d_accept_pid || c->accept_gen != c->ks->gen || c->accept_pid_cap < c->n_keys)
    return set_err(PBFT_EINVAL, "no PeerId table for the installed key set: call pbft_accept_reserve");
  return PBFT_OK;
}

int pbft_wire_decode_replies_device(pbft_ctx* c, const uint8_t* d_text, uint64_t text_bytes, const uint64_t* d_off,
                                    const uint32_t* d_len, const uint32_t* d_client_idx, const uint8_t* d_clients,
                                    uint32_t n_clients, uint64_t N, uint8_t* d_records, pbft_accept_head* d_heads,
                                    void* stream) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  int rc = check_accept_decode_args(c, d_text, text_bytes, d_off, d_len, d_client_idx, d_clients, n_clients, N,
                                    d_records, d_heads);
  if (rc) return rc;
  if (N == 0) return PBFT_OK;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t st = stream ? (hipStream_t)stream : c->stream;
  HIP_TRY(launch_accept_decode(d_text, text_bytes, d_off, d_len, d_client_idx, d_clients, n_clients, c->d_accept_pid,
                               c->n_keys, N, d_records, d_heads, st));
  return PBFT_OK;
}

// group, verify, tally and certify over N settled records: the back half of both forms
static int accept_back_half(pbft_ctx* c, const uint32_t* d_client_idx, uint64_t N, uint32_t need, uint8_t* d_records,
                            uint64_t* dB, uint32_t env_cap, uint32_t* d_env_idx, uint8_t* d_envelopes,
                            uint32_t* d_n_env, uint64_t* d_signers, uint32_t* d_count, pbft_accept_cert* d_certs,
                            void* stream) {
  const uint16_t* const d_key = (const uint16_t*)(d_records + 150);
  int rc = pbft_group_envelopes_device(c, d_records + 64, PBFT_RECORD_BYTES, d_key, PBFT_RECORD_BYTES, N, env_cap,
                                       d_env_idx, d_envelopes, d_n_env, stream);
  if (rc) return rc;
  if (N) {
    rc = pbft_verify_records_device(c, d_records, N, dB, stream);
    if (rc) return rc;
  }
  rc = pbft_tally_device(c, dB, d_key, PBFT_RECORD_BYTES, d_env_idx, 4, N, env_cap, c->n_keys, 0, d_signers, d_count,
                         stream);
  if (rc) return rc;
  if (env_cap) {
    hipStream_t st = stream ? (hipStream_t)stream : c->stream;
    HIP_TRY(launch_accept_certify(dB, d_env_idx, d_client_idx, N, d_envelopes, d_n_env, d_count, env_cap, need, d_certs,
                                  st));
  }
  return PBFT_OK;
}

int pbft_accept_replies_device(pbft_ctx* c, const uint8_t* d_text, uint64_t text_bytes, const uint64_t* d_off,
                               const uint32_t* d_len, const uint32_t* d_client_idx, const uint8_t* d_clients,
                               uint32_t n_clients, uint64_t N, uint32_t need, uint8_t* d_records,
                               pbft_accept_head* d_heads, uint64_t* dB, uint32_t env_cap, uint32_t* d_env_idx,
                               uint8_t* d_envelopes, uint32_t* d_n_env, uint64_t* d_signers, uint32_t* d_count,
                               pbft_accept_cert* d_certs, void* stream) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  // every check of every step first: a refused call has enqueued nothing
  if (need == 0) return set_err(PBFT_EINVAL, "need is 0");
  int rc = check_accept_decode_args(c, d_text, text_bytes, d_off, d_len, d_client_idx, d_clients, n_clients, N,
                                    d_records, d_heads);
  if (rc) return rc;
  if (N && !dB) return set_err(PBFT_EINVAL, "null bitmap");
  if ((uintptr_t)dB & 7) return set_err(PBFT_EINVAL, "misaligned accept pointer");
  rc = check_group_args(d_records, PBFT_RECORD_BYTES, d_records, PBFT_RECORD_BYTES, N, env_cap, d_env_idx, d_envelopes,
                        d_n_env);
  if (rc) return rc;
  if (env_cap && (!d_signers || !d_count || !d_certs)) return set_err(PBFT_EINVAL, "null accept output");
  if (((uintptr_t)d_signers & 7) || ((uintptr_t)d_count & 3) || ((uintptr_t)d_certs & 15))
    return set_err(PBFT_EINVAL, "misaligned accept pointer");
  if (N) {
    rc = pbft_wire_decode_replies_device(c, d_text, text_bytes, d_off, d_len, d_client_idx, d_clients, n_clients, N,
                                         d_records, d_heads, stream);
    if (rc) return rc;
  }
  return accept_back_half(c, d_client_idx, N, need, d_records, dB, env_cap, d_env_idx, d_envelopes, d_n_env, d_signers,
                          d_count, d_certs, stream);
}

int pbft_accept_replies(pbft_ctx* c, const uint8_t* texts, uint64_t text_bytes, const uint64_t* off, const uint32_t* len,
                        const uint32_t* client_idx, const char* clients, uint32_t n_clients, uint64_t N, uint32_t need,
                        uint32_t env_cap, uint64_t* out, pbft_accept_head* heads_out, uint32_t* env_idx_out,
                        uint8_t* envelopes_out, uint32_t* n_env_out, uint64_t* signers_out, uint32_t* count_out,
                        pbft_accept_cert* certs_out) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (c->in_flight) return set_err(PBFT_EBUSY, "async batch in flight");
  if (c->n_keys == 0) return set_err(PBFT_ENOKEYS, "pbft_verify_set_keys not called");
  if (need == 0) return set_err(PBFT_EINVAL, "need is 0");
  if (N > pbft::AC_MAX_N) return set_err(PBFT_EINVAL, "more than 2^24 replies");
  if (text_bytes > pbft::AC_MAX_TEXT_BYTES) return set_err(PBFT_EINVAL, "more than 2^31 bytes of texts");
  if (N && env_cap == 0) return set_err(PBFT_EINVAL, "env_cap is 0");
  if (N && (!off || !len || !out || !heads_out || (text_bytes && !texts) || (n_clients && !clients)))
    return set_err(PBFT_EINVAL, "null accept argument");
  if (!n_env_out || (env_cap && (!envelopes_out || !signers_out || !count_out || !certs_out)))
    return set_err(PBFT_EINVAL, "null accept output");
  for (uint64_t i = 0; i < N; ++i)
    if (len[i] > text_bytes || off[i] > text_bytes - len[i]) return set_err(PBFT_EINVAL, "a text outside text_bytes");
  const uint32_t W = tally_words(c->n_keys);
  const size_t env_bytes = (size_t)env_cap * PBFT_ENVELOPE_LEN, set_bytes = (size_t)env_cap * W * 8,
               cnt_bytes = (size_t)env_cap * 4, cert_bytes = (size_t)env_cap * sizeof(pbft_accept_cert);
  if (N == 0) {  // no reply: no envelope, empty sets, no certificate
    n_env_out[0] = n_env_out[1] = 0;
    if (env_cap) {
      memset(envelopes_out, 0, env_bytes);
      memset(signers_out, 0, set_bytes);
      memset(count_out, 0, cnt_bytes);
      memset(certs_out, 0, cert_bytes);
      for (uint32_t e = 0; e < env_cap; ++e) certs_out[e].first = PBFT_ACCEPT_NO_REPLY;
    }
    return PBFT_OK;
  }
  HIP_TRY(hipSetDevice(c->device));
  int rc = accept_build_table(c);  // (blocking anyway: a stale table is rebuilt here)
  if (rc) return rc;
  const accept_layout lay(N, text_bytes, n_clients, env_cap, W);
  rc = ensure_accept_io(c, lay.total);
  if (rc) return rc;
  uint8_t* const d = c->d_accept_io;
  pbft_accept_head* const d_heads = (pbft_accept_head*)(d + lay.heads);
  const uint32_t* const d_ci = client_idx ? (const uint32_t*)(d + lay.ci) : nullptr;
  uint64_t* const dB = (uint64_t*)(d + lay.off);  // (the offsets are dead once the decode has run: its words hold the bitmap)
  if (text_bytes) HIP_TRY(hipMemcpyAsync(d + lay.text, texts, text_bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d + lay.off, off, 8 * (size_t)N, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(d + lay.len, len, 4 * (size_t)N, hipMemcpyHostToDevice, c->stream));
  if (client_idx) HIP_TRY(hipMemcpyAsync(d + lay.ci, client_idx, 4 * (size_t)N, hipMemcpyHostToDevice, c->stream));
  if (n_clients) HIP_TRY(hipMemcpyAsync(d + lay.cl, clients, 64 * (size_t)n_clients, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(launch_accept_decode(d + lay.text, text_bytes, (const uint64_t*)(d + lay.off), (const uint32_t*)(d + lay.len),
                               d_ci, d + lay.cl, n_clients, c->d_accept_pid, c->n_keys, N, d, d_heads, c->stream));
  HIP_TRY(hipMemcpyAsync(heads_out, d_heads, sizeof(pbft_accept_head) * (size_t)N, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));

  // the host's word on every reply the device deferred
  std::vector<uint32_t> pidx;
  std::vector<uint8_t> prec;
  std::vector<pbft_accept_head> phead;
  std::vector<char> arena;
  const keyset* const ks = c->ks;
  for (uint64_t i = 0; i < N; ++i) {
    pbft_accept_head& h = heads_out[i];
    if (h.status != PBFT_ACCEPT_EDEFER) continue;
    h = pbft_accept_head{0, 0, 0, 0, 0, PBFT_ACCEPT_EJSON};
    if (arena.size() < (size_t)len[i] + 1) arena.resize((size_t)len[i] + 1);
    pbft_reply_head rh;
    const int rl = pbft_wire_decode_reply_json(texts + off[i], len[i], &rh, arena.data(), arena.size());
    if (rl < 0) continue;
    char pid[pbft::RP_PEER_ID_B58];
    if (rh.replica >= c->n_keys ||
        pbft::rp_peer_id_b58(ks->h_keys.data() + 32 * (size_t)rh.replica, (uint8_t*)pid) != pbft::RP_PEER_ID_B58 ||
        memcmp(pid, rh.peer_id, sizeof pid) != 0) {
      h.status = PBFT_ACCEPT_ESIGNER;
      continue;
    }
    const uint32_t ci = client_idx ? client_idx[i] : 0;
    if (ci >= n_clients) {
      h.status = PBFT_ACCEPT_ECLIENT;
      continue;
    }
    uint8_t D[64], env[PBFT_ENVELOPE_BYTES];
    const uint64_t o0 = 0;
    const uint32_t l0 = (uint32_t)rl;
    if (pbft_reply_digests(1, clients + 64 * (size_t)ci, (const uint8_t*)arena.data(), l0, &o0, &l0, D) != 0)
      return set_err(PBFT_EINVAL, "reply digest");
    pbft_reply_envelope(env, rh.view, rh.timestamp, D);
    const uint16_t key = (uint16_t)rh.replica;
    prec.resize(prec.size() + PBFT_RECORD_BYTES);
    pbft_records_pack(rh.sig, rh.sig + 32, &key, env, PBFT_ENVELOPE_BYTES, 1, prec.data() + prec.size() - PBFT_RECORD_BYTES);
    const bool escaped = memchr(texts + off[i] + rh.result_off, '\\', rh.result_len) != nullptr;
    h = pbft_accept_head{rh.view, rh.timestamp, rh.result_off, rh.result_len, rh.replica,
                         PBFT_ACCEPT_OK | (escaped ? (uint32_t)PBFT_ACCEPT_ESCAPED : 0u)};
    pidx.push_back((uint32_t)i);
    phead.push_back(h);
  }
  std::vector<uint8_t> buf;  // (pageable: it has to outlive the copy, so it lives to the end of the call)
  if (!pidx.empty()) {  // one H2D copy: indices | records | heads, then a scatter on the device
    const size_t P = pidx.size();
    const size_t o_rec = (4 * P + 15) & ~(size_t)15, o_head = o_rec + PBFT_RECORD_BYTES * P;
    const size_t bytes = o_head + sizeof(pbft_accept_head) * P;
    if (bytes > c->accept_patch_cap) {
      if (c->d_accept_patch) HIP_TRY(hipFree(c->d_accept_patch));
      c->d_accept_patch = nullptr;
      c->accept_patch_cap = 0;
      const size_t cap = bytes + (bytes >> 2) + 4096;
      if (hipMalloc(&c->d_accept_patch, cap) != hipSuccess) return set_err(PBFT_ENOMEM, "accept patch alloc");
      c->accept_patch_cap = cap;
    }
    buf.assign(bytes, 0);
    memcpy(buf.data(), pidx.data(), 4 * P);
    memcpy(buf.data() + o_rec, prec.data(), PBFT_RECORD_BYTES * P);
    memcpy(buf.data() + o_head, phead.data(), sizeof(pbft_accept_head) * P);
    HIP_TRY(hipMemcpyAsync(c->d_accept_patch, buf.data(), bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(launch_accept_patch((const uint32_t*)c->d_accept_patch, c->d_accept_patch + o_rec,
                                c->d_accept_patch + o_head, (uint32_t)P, N, d, d_heads, c->stream));
  }
  rc = accept_back_half(c, d_ci, N, need, d, dB, env_cap, (uint32_t*)(d + lay.idx), d + lay.env,
                        (uint32_t*)(d + lay.n_env), (uint64_t*)(d + lay.set), (uint32_t*)(d + lay.cnt),
                        (pbft_accept_cert*)(d + lay.cert), c->stream);
  if (rc) {
    (void)hipStreamSynchronize(c->stream);  // (buf)
    return rc;
  }
  const uint64_t words = (N + 63) / 64;
  hipError_t e = hipMemcpyAsync(out, dB, words * 8, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess && env_idx_out) e = hipMemcpyAsync(env_idx_out, d + lay.idx, 4 * (size_t)N, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(envelopes_out, d + lay.env, env_bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(n_env_out, d + lay.n_env, 8, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(signers_out, d + lay.set, set_bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(count_out, d + lay.cnt, cnt_bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(certs_out, d + lay.cert, cert_bytes, hipMemcpyDeviceToHost, c->stream);
  const hipError_t es = hipStreamSynchronize(c->stream);
  HIP_TRY(e);
  HIP_TRY(es);
  return PBFT_OK;
}

int pbft_verify_reserve(pbft_ctx* c, uint64_t max_n) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  HIP_TRY(hipSetDevice(c->device));
  return ensure_work(c, max_n, true);  // both halves: either device form can then be captured
}

int pbft_verify_set_option(pbft_ctx* c, int option, uint64_t value) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  switch (option) {
    case PBFT_OPT_SPLIT_BELOW: c->split_below = value; return PBFT_OK;
    case PBFT_OPT_FINISH_WIDTH:
      if (value != 0 && value != 1 && value != 2 && value != 4 && value != 8 && value != 16)
        return set_err(PBFT_EINVAL, "finish width");
      c->fin_m = (int)value;
      return PBFT_OK;
    case PBFT_OPT_FINISH_TREE:
      // the one compiled tree depth (PBFT_FIN_LV) or none; the other depth is a build-time A/B (-DPBFT_FIN_LV)
      if ((value == 4 || value == 6) && value != PBFT_FIN_LV) return set_err(PBFT_EINVAL, "finish tree depth not compiled");
      c->fin_tree = (value == 0 || value == PBFT_FIN_LV) ? (int)value : -1;
      return PBFT_OK;
    case PBFT_OPT_FINISH_WAVES: c->fin_waves = (value == 1 || value == 2) ? (int)value : 0; return PBFT_OK;
    case PBFT_OPT_LAT_SPLIT: c->lat_split = (value == 4 || value == 8) ? (int)value : 0; return PBFT_OK;
    case PBFT_OPT_KERNEL_TIMING: c->timing = value != 0; return PBFT_OK;
    case PBFT_OPT_COMB_PAIR: c->comb_pair = value <= 1 ? (int)value : -1; return PBFT_OK;
    case PBFT_OPT_KEY_TABLE_BUDGET_MB: c->key_budget_mb = value; return PBFT_OK;
    case PBFT_OPT_COMB_PRIO: c->comb_prio = value <= 1 ? (int)value : -1; return PBFT_OK;
    case PBFT_OPT_COMB_BALANCE: c->comb_balance = value <= 1 ? (int)value : -1; return PBFT_OK;
    case PBFT_OPT_FAULT_INJECT:
      if (value > 2) return set_err(PBFT_EINVAL, "fault injection point");
      c->fault_inject = (int)value;
      return PBFT_OK;
    case PBFT_OPT_GROUP_SEED:
      c->group_seed = value;
      c->group_seeded = true;
      return PBFT_OK;
    case PBFT_OPT_GROUP_HASH_BITS:
      if (value > 64) return set_err(PBFT_EINVAL, "group hash bits");
      c->group_hash_bits = (uint32_t)value;
      return PBFT_OK;
    case PBFT_OPT_INDEX_TILE:
      if (value == 0) value = INDEX_TILE_DEFAULT;
      if (value < pbft::IX_TILE_MIN || value > INDEX_TILE_DEFAULT || (value & (value - 1)))
        return set_err(PBFT_EINVAL, "index tile bytes");
      c->index_tile = (uint32_t)value;
      return PBFT_OK;
    case PBFT_OPT_EGRESS_BLOCK:
      if (value != 0 && value != 64 && value != 256) return set_err(PBFT_EINVAL, "egress block is 64 or 256");
      c->egress_block = value ? (int)value : 64;
      return PBFT_OK;
    case PBFT_OPT_EGRESS_DIRECT:
      if (value > 1) return set_err(PBFT_EINVAL, "egress direct is 0 or 1");
      c->egress_direct = value == 1;
      return PBFT_OK;
    case PBFT_OPT_PROPOSE_WIDTH:
      if (value != 0 && value != 1 && value != 4 && value != 16) return set_err(PBFT_EINVAL, "propose width is 1, 4 or 16");
      c->propose_width = value ? (int)value : PROPOSE_WIDTH_DEFAULT;
      return PBFT_OK;
  }
  return set_err(PBFT_EINVAL, "unknown option");
}

int pbft_verify_ctx_info(pbft_ctx* c, uint32_t* pb, uint32_t* pa, uint32_t* n_keys) {
  if (!c) return set_err(PBFT_EINVAL, "null context");
  if (pb) *pb = (uint32_t)PLB::P;
  if (pa) *pa = (uint32_t)c->pa;
  if (n_keys) *n_keys = c->n_keys;
  return PBFT_OK;
}

float pbft_last_kernel_ms(pbft_ctx* c) {
  if (!c || !c->timing) return -1.f;
  float ms = -1.f;
  if (hipEventSynchronize(c->ev1) != hipSuccess) { (void)hipGetLastError(); return -1.f; }
  if (hipEventElapsedTime(&ms, c->ev0, c->ev1) != hipSuccess) { (void)hipGetLastError(); return -1.f; }
  c->last_ms = ms;
  return ms;
}

}  // extern "C"

// Client acceptance (include/pbft_wire.h pbft_accept_replies_device): signed replies' texts matched, their results hashed
// together with their clients and the 160-byte verifier records written on the device; and, behind grouping,
// verification and tally, one certificate per envelope.  Its own translation unit.  The rule is accept_core.h's; the
// aligned-dword reader, the client field's words and the Blake2b over C | result are sign_tile.h's, shared with
// reply.hip.  Plain HIP C++.
#include "accept_kernels.h"

#include "../../include/pbft_wire.h"
#include "sign_tile.h"

using namespace pbft;

static_assert(AC_OK == PBFT_ACCEPT_OK && AC_EDEFER == PBFT_ACCEPT_EDEFER && AC_ESIGNER == PBFT_ACCEPT_ESIGNER &&
                  AC_ECLIENT == PBFT_ACCEPT_ECLIENT && AC_EJSON == PBFT_ACCEPT_EJSON && AC_ESCAPED == PBFT_ACCEPT_ESCAPED &&
                  AC_NO_REPLY == PBFT_ACCEPT_NO_REPLY,
              "the core's values are the header's");
static_assert(sizeof(pbft_accept_head) == sizeof(accept_head) && sizeof(pbft_accept_cert) == sizeof(accept_cert), "");
static constexpr uint32_t AC_ENVELOPE_LEN = 85;  // "PBFT" | kind | view | timestamp | D
static_assert(PBFT_RECORD_BYTES == 160 && 64 + AC_ENVELOPE_LEN + 1 == 150, "ten 16-byte stores per record; the key index at byte 150");

// LDS rows of one reply, in dwords: the aligned dwords that hold the text's first AC_HEAD_WIN and last AC_TAIL_WIN bytes
// (up to three bytes in front of each); odd, so that the 64 lanes' reads at one row position fall into different banks
static constexpr uint32_t AC_HEAD_DWORDS = 37, AC_TAIL_DWORDS = 43;
static constexpr uint32_t AC_HEAD_LOADS = (3 + AC_HEAD_WIN + 3) / 4, AC_TAIL_LOADS = (3 + AC_TAIL_WIN + 3) / 4;
static_assert(AC_HEAD_LOADS <= AC_HEAD_DWORDS && AC_TAIL_LOADS <= AC_TAIL_DWORDS && AC_TAIL_LOADS <= 64, "");
static_assert(AC_HEAD_DWORDS % 2 == 1 && AC_TAIL_DWORDS % 2 == 1, "odd rows");
static_assert(RP_TEXT_MIN >= AC_HEAD_WIN + 4 && RP_TEXT_MIN >= AC_TAIL_WIN, "every staged dword holds a byte of the text");

// Byte k of a text of n bytes from its two LDS rows: k < AC_HEAD_WIN from the head's, k >= n - AC_TAIL_WIN from the tail's
struct ac_lds_reader {
  const uint8_t* head;  // the row's byte that is the text's byte 0
  const uint8_t* tail;  // the row's byte that is the text's byte n - AC_TAIL_WIN
  uint32_t tail_from;   // n - AC_TAIL_WIN
  __device__ __forceinline__ uint32_t operator()(uint32_t k) const {
    return k < AC_HEAD_WIN ? head[k] : tail[k - tail_from];
  }
};

// One wave per 64-reply tile, one wave per workgroup.
//  1. Lane l decides from off / len alone whether reply l may be read: RP_TEXT_MIN <= len <= RP_TEXT_MAX and
//     off + len <= text_bytes, before any address is formed.  Any other reply is AC_EDEFER and none of its bytes are read.
//  2. The wave stages reply after reply: lane j loads aligned dword j of the text's first AC_HEAD_WIN bytes and aligned
//     dword j of its last AC_TAIL_WIN into the reply's two LDS rows.  Every such dword holds a byte of the text.
//  3. Each lane matches its own rows (ac_match_frame: the head forwards, the tail backwards from the text's end).
//  4. The results that are still candidates are tested against the alphabet by the whole wave, 256 bytes per step
//     (one aligned dword per lane) with one ballot per reply: at most RP_RESULT_MAX / 256 steps a reply.
//  5. Each lane applies the signer's and the client's rule, hashes C | result where the result lies, and stores its
//     record as ten 16-byte stores and its head as four 8-byte stores.
__global__ void __launch_bounds__(64) accept_decode_kernel(const uint8_t* __restrict__ text, uint64_t text_bytes,
                                                           const uint64_t* __restrict__ off,
                                                           const uint32_t* __restrict__ len,
                                                           const uint32_t* __restrict__ client_idx,
                                                           const uint8_t* __restrict__ clients, uint32_t n_clients,
                                                           const uint8_t* __restrict__ pid, uint32_t n_keys, uint64_t N,
                                                           uint4* __restrict__ records, uint2* __restrict__ heads) {
  __shared__ __attribute__((aligned(16))) uint32_t s_head[ACCEPT_TILE][AC_HEAD_DWORDS];
  __shared__ __attribute__((aligned(16))) uint32_t s_tail[ACCEPT_TILE][AC_TAIL_DWORDS];
  const int lane = threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * ACCEPT_TILE + lane;
  const bool live = i < N;
  uint64_t o = 0;
  uint32_t n = 0, ci = 0;
  bool cand = false;
  if (live) {
    const uint32_t l = len[i];
    if (l >= RP_TEXT_MIN && l <= RP_TEXT_MAX && l <= text_bytes) {
      const uint64_t at = off[i];
      if (at <= text_bytes - l) {
        cand = true;
        o = at;
        n = l;
      }
    }
    if (client_idx) ci = client_idx[i];
  }

  for (int r = 0; r < (int)ACCEPT_TILE; ++r) {
    if (!__shfl((int)cand, r, 64)) continue;  // (wave-uniform)
    const uint64_t ro = shfl64(o, r);
    const uint64_t re = ro + __shfl(n, r, 64);
    const uint64_t a0 = ro & ~(uint64_t)3, b0 = (re - AC_TAIL_WIN) & ~(uint64_t)3;
    if (lane < (int)AC_HEAD_LOADS) s_head[r][lane] = *(const uint32_t*)(text + a0 + 4 * (uint32_t)lane);
    if (lane < (int)AC_TAIL_LOADS && b0 + 4 * (uint32_t)lane < re)
      s_tail[r][lane] = *(const uint32_t*)(text + b0 + 4 * (uint32_t)lane);
  }
  __syncthreads();

  accept_frame f{};
  uint32_t sg[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) sg[j] = 0;
  const uint64_t e = o + n;
  const ac_lds_reader rd{(const uint8_t*)s_head[lane] + ((uint32_t)o & 3u),
                         (const uint8_t*)s_tail[lane] + ((uint32_t)(e - AC_TAIL_WIN) & 3u), n - AC_TAIL_WIN};
  bool ok = false;
  if (cand) ok = ac_match_frame(rd, n, f, sg);

  bool res_ok = true;
  for (int r = 0; r < (int)ACCEPT_TILE; ++r) {
    if (!__shfl((int)ok, r, 64)) continue;  // (wave-uniform)
    const uint8_t* m = text + shfl64(o, r) + __shfl(f.result_off, r, 64);
    const uint32_t l = __shfl(f.result_len, r, 64);  // (at most RP_RESULT_MAX)
    bool bad = false;
    for (uint32_t k = 4 * (uint32_t)lane; k < l; k += 4 * 64) {
      const uint32_t w = load32_span(m, l, k);
      const uint32_t nb = l - k < 4 ? l - k : 4;
#pragma unroll
      for (uint32_t b = 0; b < 4; ++b) bad = bad || (b < nb && !pr_alphabet((w >> (8 * b)) & 0xFFu));
    }
    const bool any = __ballot(bad) != 0;
    if (lane == r) res_ok = !any;
  }

  uint32_t st = AC_EDEFER;
  if (ok && res_ok) st = !ac_signer_ok(rd, f, pid, n_keys) ? AC_ESIGNER : ci >= n_clients ? AC_ECLIENT : AC_OK;

  uint32_t rec[40];
  if (st == AC_OK) {
    uint64_t cw[8];
    client_words(cw, clients + (size_t)RP_CLIENT_FIELD * ci);
    uint32_t dg[16];
    blake2b512_span<true>(dg, cw, text + o + f.result_off, f.result_len);  // (at most RP_RESULT_MAX / 128 + 1 blocks)
    ac_record(rec, sg, f.view, f.timestamp, dg, f.replica);
  } else {
    ac_record_none(rec);
    f = accept_frame{};
  }
  if (!live) return;
  uint4* dst = records + i * 10;
#pragma unroll
  for (int k = 0; k < 10; ++k) dst[k] = make_uint4(rec[4 * k], rec[4 * k + 1], rec[4 * k + 2], rec[4 * k + 3]);
  uint2* hd = heads + i * 4;
  hd[0] = make_uint2((uint32_t)f.view, (uint32_t)(f.view >> 32));
  hd[1] = make_uint2((uint32_t)f.timestamp, (uint32_t)(f.timestamp >> 32));
  hd[2] = make_uint2(f.result_off, f.result_len);
  hd[3] = make_uint2(f.replica, st);
}

// ---- certificates ----
__global__ void __launch_bounds__(256) accept_cert_init_kernel(uint4* __restrict__ certs, uint32_t env_cap) {
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e >= env_cap) return;
  certs[2 * e] = make_uint4(0, 0, 0, 0);
  certs[2 * e + 1] = make_uint4(AC_NO_REPLY, 0, 0, 0);
}

// first = the least reply index of the envelope whose bit is set: atomicMin, exact whatever order the atomics land in
__global__ void __launch_bounds__(256) accept_cert_first_kernel(const uint64_t* __restrict__ bitmap,
                                                                const uint32_t* __restrict__ env_idx, uint64_t N,
                                                                const uint32_t* __restrict__ n_env, uint32_t env_cap,
                                                                accept_cert* __restrict__ certs) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const uint32_t e = env_idx[i];
  const uint32_t live = n_env[0] < env_cap ? n_env[0] : env_cap;
  if (e >= live) return;  // (0xFFFFFFFF: a row without an envelope)
  if (!((bitmap[i >> 6] >> (i & 63)) & 1)) return;
  atomicMin(&certs[e].first, (uint32_t)i);
}

__global__ void __launch_bounds__(256) accept_cert_fill_kernel(const uint8_t* __restrict__ envelopes,
                                                               const uint32_t* __restrict__ n_env,
                                                               const uint32_t* __restrict__ count,
                                                               const uint32_t* __restrict__ client_idx, uint32_t env_cap,
                                                               uint32_t need, accept_cert* __restrict__ certs) {
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  const uint32_t live = n_env[0] < env_cap ? n_env[0] : env_cap;
  if (e >= live) return;
  const uint8_t* env = envelopes + (size_t)AC_ENVELOPE_LEN * e;
  uint64_t view = 0, ts = 0;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    view |= (uint64_t)env[5 + j] << (8 * j);
    ts |= (uint64_t)env[13 + j] << (8 * j);
  }
  const uint32_t first = certs[e].first;
  const uint32_t cnt = count[e];
  certs[e].view = view;
  certs[e].timestamp = ts;
  certs[e].count = cnt;
  certs[e].client = (first != AC_NO_REPLY && client_idx) ? client_idx[first] : 0u;
  certs[e].accepted = cnt >= need ? 1u : 0u;
}

// 14 lanes per patch: ten 16-byte granules of the record, four 8-byte words of the head
__global__ void __launch_bounds__(256) accept_patch_kernel(const uint32_t* __restrict__ idx,
                                                           const uint4* __restrict__ prec,
                                                           const uint2* __restrict__ phead, uint32_t P, uint64_t N,
                                                           uint4* __restrict__ records, uint2* __restrict__ heads) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  const uint64_t p = t / 14;
  const uint32_t k = (uint32_t)(t - p * 14);
  if (p >= P) return;
  const uint64_t f = idx[p];
  if (f >= N) return;
  if (k < 10) records[f * 10 + k] = prec[p * 10 + k];
  else heads[f * 4 + (k - 10)] = phead[p * 4 + (k - 10)];
}

hipError_t launch_accept_decode(const uint8_t* d_text, uint64_t text_bytes, const uint64_t* d_off, const uint32_t* d_len,
                                const uint32_t* d_client_idx, const uint8_t* d_clients, uint32_t n_clients,
                                const uint8_t* d_pid, uint32_t n_keys, uint64_t N, uint8_t* d_records, void* d_heads,
                                hipStream_t st) {
  hipLaunchKernelGGL(accept_decode_kernel, dim3((unsigned)((N + ACCEPT_TILE - 1) / ACCEPT_TILE)), dim3(ACCEPT_TILE), 0,
                     st, d_text, text_bytes, d_off, d_len, d_client_idx, d_clients, n_clients, d_pid, n_keys, N,
                     (uint4*)d_records, (uint2*)d_heads);
  return hipGetLastError();
}

hipError_t launch_accept_certify(const uint64_t* d_bitmap, const uint32_t* d_env_idx, const uint32_t* d_client_idx,
                                 uint64_t N, const uint8_t* d_envelopes, const uint32_t* d_n_env,
                                 const uint32_t* d_count, uint32_t env_cap, uint32_t need, void* d_certs,
                                 hipStream_t st) {
  const unsigned eb = (env_cap + 255) / 256;
  hipLaunchKernelGGL(accept_cert_init_kernel, dim3(eb), dim3(256), 0, st, (uint4*)d_certs, env_cap);
  if (N)
    hipLaunchKernelGGL(accept_cert_first_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, d_bitmap, d_env_idx,
                       N, d_n_env, env_cap, (accept_cert*)d_certs);
  hipLaunchKernelGGL(accept_cert_fill_kernel, dim3(eb), dim3(256), 0, st, d_envelopes, d_n_env, d_count, d_client_idx,
                     env_cap, need, (accept_cert*)d_certs);
  return hipGetLastError();
}

hipError_t launch_accept_patch(const uint32_t* d_idx, const uint8_t* d_prec, const void* d_phead, uint32_t P, uint64_t N,
                               uint8_t* d_records, void* d_heads, hipStream_t st) {
  const uint64_t threads = (uint64_t)P * 14;
  hipLaunchKernelGGL(accept_patch_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, d_idx,
                     (const uint4*)d_prec, (const uint2*)d_phead, P, N, (uint4*)d_records, (uint2*)d_heads);
  return hipGetLastError();
}

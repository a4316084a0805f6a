/*
 * pbft_wire.h — wire codec of the PBFT messages that feed the GPU verifier
 * (SURVEY.md §8f row 3).  Host C++ (pbft_amd/csrc/host/wire.cpp), compiled into
 * pbft_amd/libpbft_verify.so.
 *
 * Reference interfaces mirrored (ameya-deshmukh/pbft):
 *   pbft_uvi_encode / pbft_uvi_decode  unsigned-varint length prefix of the
 *       UviBytes framing (src/protocol_config.rs:51, :82 `UviBytes::default()`,
 *       unsigned-varint crate; max frame 128 MiB as its codec default)
 *   pbft_wire_encode_json              message_to_json src/protocol_config.rs:116-123
 *       = serde_json::to_string of the externally tagged `Message` enum
 *       (src/message.rs:7-31; structs :34-38, :105-115, :174-179, :214-219):
 *         {"Prepare":{"view":1,"sequence_number":2,"digest":"<128 hex>"}}
 *   pbft_wire_decode_json              bytes_to_message src/protocol_config.rs:125-129
 *       -> `impl From<Vec<u8>> for Message` (src/message.rs:15-19), which panics
 *       on bad input; here an error code is returned instead.
 *   pbft_wire_decode_votes             the ingress path PbftHandler ->
 *       message_to_handler_event (src/handler.rs:533-548): a byte stream of
 *       UviBytes frames straight into the verifier's struct-of-arrays batch.
 *
 * Signed-envelope extension (BASELINE north_star "a signed-message envelope in
 * message.rs"): PrePrepare / Prepare / Commit may carry two more fields after
 * the reference's ones, "replica" (u16 signer index = position in
 * network.json's "nodes") and "signature" (128 lowercase hex chars = R || S of
 * the Ed25519 signature over the 85-byte envelope of pbft_replica.h).  Messages
 * without them encode byte-identically to the reference.
 *
 * Binary record (zero-copy alternative to JSON, 160 bytes, 16-B aligned fields):
 *   [0,32) R  [32,64) S  [64,149) envelope  [149] pad  [150,152) key_idx LE
 *   [152,160) pad — consumed directly by pbft_verify_records_device.
 */
#ifndef PBFT_WIRE_H
#define PBFT_WIRE_H

#include <stddef.h>
#include <stdint.h>

#include "pbft_verify.h"

#ifdef __cplusplus
extern "C" {
#endif

#define PBFT_MSG_PREPREPARE 0
#define PBFT_MSG_PREPARE 1
#define PBFT_MSG_COMMIT 2
#define PBFT_MSG_CLIENT_REQUEST 3

#define PBFT_UVI_MAX_FRAME (128u * 1024u * 1024u)
#define PBFT_RECORD_BYTES 160

/* Frame decode status (pbft_wire_decode_votes) */
#define PBFT_WIRE_OK 0        /* signed PrePrepare/Prepare/Commit -> one SoA row */
#define PBFT_WIRE_EJSON 1     /* not a JSON Message of the reference schema */
#define PBFT_WIRE_EDIGEST 2   /* digest is not 128 hex chars               */
#define PBFT_WIRE_EUNSIGNED 3 /* no replica/signature fields               */
#define PBFT_WIRE_EKIND 4     /* ClientRequest (not signed by a replica)     */
#define PBFT_WIRE_ESIGNER 5   /* replica index >= n_replicas               */

typedef struct {
  uint32_t kind;     /* PBFT_MSG_* */
  uint64_t view;     /* PrePrepare / Prepare / Commit */
  uint64_t seq;      /* "sequence_number" */
  uint8_t digest[64];
  uint32_t digest_ok; /* 1: "digest" was 128 hex chars and is in digest[] */
  /* signed-envelope extension */
  uint32_t has_sig;
  uint32_t replica;
  uint8_t sig[64]; /* R || S */
  /* ClientRequest (standalone, or the PrePrepare's "message") */
  const char *operation; /* UTF-8, not NUL-terminated; decode: points into the arena */
  uint32_t operation_len;
  uint64_t timestamp;
  char client[64]; /* SocketAddr as serialized by serde ("127.0.0.1:8080"), NUL-terminated */
} pbft_wire_msg;

/* LEB128 unsigned varint.  encode: returns bytes written (1..10).
 * decode: 0 ok, 1 need more bytes, PBFT_EINVAL if overlong / non-minimal / > u64. */
size_t pbft_uvi_encode(uint64_t v, uint8_t out[10]);
int pbft_uvi_decode(const uint8_t *buf, size_t len, uint64_t *value, size_t *header_bytes);

/* serde_json encoding of m (compact, reference field order).  Writes at most cap
 * bytes, sets *len to the full length; returns 0, or PBFT_EINVAL if cap is too
 * small (nothing useful written) or the message is malformed. */
int pbft_wire_encode_json(const pbft_wire_msg *m, char *out, size_t cap, size_t *len);

/* One UviBytes frame (varint length + JSON) of m. Same conventions. */
int pbft_wire_encode_frame(const pbft_wire_msg *m, uint8_t *out, size_t cap, size_t *len);

/* Parse one JSON Message (any field order / whitespace, unknown fields ignored,
 * as serde does).  Unescaped strings go into arena (operation points there).
 * Returns 0 or PBFT_EINVAL. */
int pbft_wire_decode_json(const char *json, size_t len, pbft_wire_msg *out, char *arena, size_t arena_cap);

/* Decode a byte stream of UviBytes frames into the verifier's SoA batch.
 * Stops at the first incomplete frame, after max_rows signed votes, or after
 * max_frames frames.  For every decoded frame f: status[f] = PBFT_WIRE_*;
 * each OK frame appends row r: R[r], S[r], key_idx[r] = replica, msg[r] = the
 * 85-byte envelope (stride 85), kind[r] (0 PrePrepare, 1 Prepare, 2 Commit),
 * view[r], seq[r].  A PrePrepare row checks the primary's signature over the
 * CLAIMED digest only: the caller still recomputes the digest of its operation
 * (validate_digest, src/message.rs:139-145), as pbft_replica_push_frames does,
 * and checks that key_idx is the view's primary; key_idx of a vote must be the
 * authenticated connection's peer (src/behavior.rs:346, :380).  Outputs: *n_frames,
 * *n_rows, *consumed (bytes of whole frames).  Returns 0, or PBFT_EINVAL on a
 * framing error (bad varint / frame > PBFT_UVI_MAX_FRAME) at *consumed. */
int pbft_wire_decode_votes(const uint8_t *stream, size_t len, uint32_t n_replicas, uint64_t max_frames,
                           uint64_t max_rows, uint8_t *status, uint8_t *R, uint8_t *S, uint16_t *key_idx,
                           uint8_t *msg, uint8_t *kind, uint64_t *view, uint64_t *seq, uint64_t *n_frames,
                           uint64_t *n_rows, uint64_t *consumed);

/* N signed votes (kind[i] Prepare / Commit, view, seq, digest[64], replica, sig = R || S) as consecutive UviBytes
 * frames of their JSON Messages -- what a replica's connection carries when it multicasts its votes (the egress side
 * of pbft_replica_push_frames).  *len = the stream's full length; returns 0, or PBFT_EINVAL if cap is too small
 * (then *len still tells the length needed) or a kind is not a vote. */
int pbft_wire_encode_votes(uint64_t N, const uint8_t *kind, const uint64_t *view, const uint64_t *seq,
                           const uint8_t *digests, const uint32_t *replica, const uint8_t *sigs, uint8_t *out,
                           size_t cap, size_t *len);

/* Pack SoA rows into 160-byte binary records (layout above) and back. */
int pbft_records_pack(const uint8_t *R, const uint8_t *S, const uint16_t *key_idx, const uint8_t *msg,
                      uint32_t msg_stride, uint64_t N, uint8_t *records);

/* Verify N binary records resident on the device (zero-copy from the wire:
 * R, S, key index and envelope read in place with a 160-byte stride). */
int pbft_verify_records_device(pbft_ctx *ctx, const uint8_t *d_records, uint64_t N, uint64_t *d_bitmap,
                               void *stream);
/* Same from host records (one H2D copy of N x 160 bytes). Blocking. */
int pbft_verify_records(pbft_ctx *ctx, const uint8_t *records, uint64_t N, uint64_t *bitmap_out);

/* ---- JSON frames decoded on the device (kernel: pbft_amd/csrc/wire_decode.hip) ----
 * The canonical form of a signed vote, exactly what serde_json and pbft_wire_encode_json write,
 *   {"Prepare":{"view":V,"sequence_number":N,"digest":"<128 hex>","replica":R,"signature":"<128 hex>"}}
 * (or "Commit"; PBFT_FRAME_MIN..PBFT_FRAME_MAX bytes), is parsed by one GPU lane per frame into the 160-byte record
 * above and a 24-byte head.  Frame f is record f, head f and bit f: no compaction.  Any other frame -- a PrePrepare,
 * a ClientRequest, whitespace, another field order, an escape, an invalid number or hex digit -- is marked
 * PBFT_WIRE_EDEFER on the device: the general parser decides about it, with serde's rules (pbft_verify_frames does
 * that).  The signer of a vote is the connection's authenticated peer, never a frame field: with a peer array,
 * frame f is PBFT_WIRE_ESIGNER unless its "replica" equals peer[f] (tested on Prepare and Commit only).
 * A frame whose status is not PBFT_WIRE_OK has an all-zero record with key index 0xFFFF (bit 0 under any key set),
 * and view = seq = kind = 0, key_idx = 0xFFFF in its head. */
#define PBFT_WIRE_EDEFER 6 /* not the canonical vote form: pbft_wire_decode_json decides (device form only) */
#define PBFT_FRAME_MIN 336
#define PBFT_FRAME_MAX 379
typedef struct {
  uint64_t view, seq; /* of an OK frame */
  uint16_t key_idx;   /* the signer ("replica") of an OK frame */
  uint8_t kind;       /* PBFT_MSG_* of an OK frame */
  uint8_t status;     /* PBFT_WIRE_* */
  uint32_t frame_len; /* the frame's body length as given */
} pbft_frame_head;

/* Host: the varint scan of a stream of whole frames -> body offset and length of each (the framing loop of
 * pbft_wire_decode_votes: stops at the first incomplete frame or after max_frames; PBFT_EINVAL on a framing error
 * at *consumed).  off / flen hold max_frames entries. */
int pbft_wire_frame_index(const uint8_t *stream, size_t len, uint64_t max_frames, uint64_t *off, uint32_t *flen,
                          uint64_t *n_frames, uint64_t *consumed);

/* Device, enqueue only (one kernel node: no allocation, copy or synchronisation; capturable): frame f = bytes
 * [d_off[f], d_off[f] + d_len[f]) of d_stream -> d_records[f], d_heads[f].  d_stream must be 16-byte aligned and
 * readable up to stream_bytes rounded up to 16 (whole 16-byte granules of that range are read, nothing beyond
 * it); d_records 16-byte aligned, the others naturally.  A frame that does not lie inside stream_bytes is
 * PBFT_WIRE_EDEFER and is not read.  d_peer: NULL or one authenticated replica index per frame.
 * PBFT_EINVAL: null / misaligned pointer, n_replicas 0 or > 65535, N > 2^32. */
int pbft_wire_decode_frames_device(pbft_ctx *ctx, const uint8_t *d_stream, uint64_t stream_bytes,
                                   const uint64_t *d_off, const uint32_t *d_len, const uint16_t *d_peer,
                                   uint32_t n_replicas, uint64_t N, uint8_t *d_records, pbft_frame_head *d_heads,
                                   void *stream);

/* Device, enqueue only: the decode, then pbft_verify_records_device of d_records on the same stream.  Every frame
 * that is not PBFT_WIRE_OK (PBFT_WIRE_EDEFER included) has bit 0.  Call pbft_verify_reserve(N) before a capture. */
int pbft_verify_frames_device(pbft_ctx *ctx, const uint8_t *d_stream, uint64_t stream_bytes, const uint64_t *d_off,
                              const uint32_t *d_len, const uint16_t *d_peer, uint32_t n_replicas, uint64_t N,
                              uint8_t *d_records, pbft_frame_head *d_heads, uint64_t *d_bitmap, void *stream);

/* Host, blocking, the complete form: stream and index to the device, decode there, the heads back; every
 * PBFT_WIRE_EDEFER frame then goes through pbft_wire_decode_json on the host and gets the status
 * pbft_wire_decode_votes would give it (a signed PrePrepare that passes is a kind-0 record), plus the peer rule; the
 * records and heads of those that became OK are patched on the device, and all N records are verified.
 * heads_out[f].status is never PBFT_WIRE_EDEFER.  records_out: NULL or N x 160 bytes.  bitmap_out: ceil(N / 64) words.
 * PBFT_EINVAL also for a frame with off + flen beyond stream_bytes; PBFT_ENOKEYS / PBFT_EBUSY as
 * pbft_verify_records. */
int pbft_verify_frames(pbft_ctx *ctx, const uint8_t *stream, uint64_t stream_bytes, const uint64_t *off,
                       const uint32_t *flen, const uint16_t *peer, uint32_t n_replicas, uint64_t N,
                       uint64_t *bitmap_out, pbft_frame_head *heads_out, uint8_t *records_out);

/* Frames in, quorums out.  Device, enqueue only, one stream: the decode; pbft_group_envelopes_device over d_records
 * in place (envelope at +64, key index at +150, stride 160: a frame that is not PBFT_WIRE_OK has key index 0xFFFF and
 * is skipped), which writes d_env_idx [N], d_envelopes [env_cap][85] and d_n_env [2]; pbft_verify_records_device, so
 * d_bitmap is word for word what pbft_verify_frames_device writes for the same input; and pbft_tally_device with the
 * records' key indices, the new d_env_idx, n_env = env_cap and n_signers = the installed key count, which writes
 * d_signers [env_cap][ceil(n_keys / 64)] and d_count [env_cap] (table entries >= d_n_env[0] have empty sets and count
 * 0).  No per-vote data has to leave the device between the socket's bytes and "these envelopes have 2f / 2f + 1
 * distinct valid signers".  An env_cap below the number of distinct envelopes loses the later envelopes' votes (their
 * rows get env_idx 0xFFFFFFFF, counted in d_n_env[1]), never miscounts.  Call pbft_verify_reserve(N) and
 * pbft_group_reserve(N) before a capture.  PBFT_EINVAL as pbft_verify_frames_device and pbft_group_envelopes_device
 * (env_cap = 0 with N > 0, N > 2^31), and for a null or misaligned output; a refused call has enqueued nothing.
 * N = 0 writes d_n_env = {0, 0} and zeroes the table, the sets and the counts. */
int pbft_verify_frames_tally_device(pbft_ctx *ctx, const uint8_t *d_stream, uint64_t stream_bytes,
                                    const uint64_t *d_off, const uint32_t *d_len, const uint16_t *d_peer,
                                    uint32_t n_replicas, uint64_t N, uint8_t *d_records, pbft_frame_head *d_heads,
                                    uint64_t *d_bitmap, uint32_t env_cap, uint32_t *d_env_idx, uint8_t *d_envelopes,
                                    uint32_t *d_n_env, uint64_t *d_signers, uint32_t *d_count, void *stream);

/* Host, blocking: pbft_verify_frames' staging, its host settlement of the PBFT_WIRE_EDEFER frames and its patch, then
 * group, verify and tally as above on the settled records.  Back per frame: heads_out, bitmap_out (both as
 * pbft_verify_frames gives them) and, unless NULL, env_idx_out [N]; back per envelope: envelopes_out [env_cap][85],
 * n_env_out [2], signers_out [env_cap][ceil(n_keys / 64)] and count_out [env_cap].  The 160-byte records stay on the
 * device.  Argument checks and codes of pbft_verify_frames; PBFT_EINVAL also for env_cap = 0 with N > 0, N > 2^31 and
 * a null output.  N = 0 zeroes the per-envelope outputs. */
int pbft_verify_frames_tally(pbft_ctx *ctx, const uint8_t *stream, uint64_t stream_bytes, const uint64_t *off,
                             const uint32_t *flen, const uint16_t *peer, uint32_t n_replicas, uint64_t N,
                             uint32_t env_cap, uint64_t *bitmap_out, pbft_frame_head *heads_out,
                             uint32_t *env_idx_out, uint8_t *envelopes_out, uint32_t *n_env_out,
                             uint64_t *signers_out, uint32_t *count_out);

/* ---- Connection streams in: the frame index made on the device (kernels: pbft_amd/csrc/wire_index.hip) ----
 * What upgrade_inbound has is one buffer of bytes per authenticated connection.  Here they are S segments of one
 * stream: segment s = bytes [seg_off[s], seg_off[s] + seg_len[s]) at any alignment, with gaps between segments as
 * they come; it begins at a frame boundary and may end inside a varint or a body.  For every segment the device
 * computes what pbft_wire_frame_index(stream + seg_off[s], seg_len[s], unlimited, ...) computes, value for value: the
 * same frames, the same flen, off shifted by seg_off[s] (an absolute body offset, as
 * pbft_wire_decode_frames_device consumes it), the same consumed, and "framing error" exactly where that function
 * returns PBFT_EINVAL (the frames in front of the error are delivered).  Frames are numbered by segment, then by
 * position in the segment; peer[f] is its segment's peer.  No byte outside a segment influences its result. */
typedef struct {
  uint64_t consumed; /* bytes of whole frames, counted from seg_off[s] */
  uint32_t first;    /* number of the segment's first frame = the frames of the segments in front of it */
  uint32_t n_frames;
  uint32_t status;   /* PBFT_SEG_* */
  uint32_t pad;      /* 0 */
} pbft_seg_head;
#define PBFT_SEG_OK 0
#define PBFT_SEG_EFRAMING 1 /* framing error at consumed (pbft_wire_frame_index: PBFT_EINVAL) */
/* The segment is not read, n_frames = consumed = 0: it does not lie inside stream_bytes, or the lengths of the
 * segments up to and including it that do lie inside add up to more than stream_bytes (segments that overlap). */
#define PBFT_SEG_EOUTSIDE 2

/* Device, enqueue only (kernel nodes on one stream: no allocation, copy, memset or synchronisation, no lane waits for
 * another block; capturable after pbft_index_reserve).  d_stream as for pbft_wire_decode_frames_device: 16-byte
 * aligned, readable up to stream_bytes rounded up to 16, and only 16-byte granules of that range are read.
 * d_seg_peer: NULL or one authenticated replica index per segment; d_peer must be NULL iff it is.
 * Outputs: d_off / d_len / d_peer [frame_cap]; frames numbered >= frame_cap are not written and are counted in
 * d_n_frames[1] (later frames are lost, none is miscounted); entries [min(total, frame_cap), frame_cap) are padding:
 * off 0, len 0, peer 0xFFFF, which the decoder marks PBFT_WIRE_EDEFER without reading and the grouping skips, so the
 * whole chain can be enqueued with N = frame_cap.  d_seg_heads [S] is complete whatever frame_cap is.
 * d_n_frames [2] = {total, not written}.  S = 0 or frame_cap = 0 is legal.
 * PBFT_EINVAL: a null pointer that would be used or a misaligned one, S > 65536, frame_cap > 2^31, stream_bytes >
 * 2^31; a refused call has enqueued nothing.  The workspace (tile tables: ~0.19 bytes per stream byte at the default
 * tile, plus ~3 KB per segment) grows on first use of a larger call, which is then not capturable. */
int pbft_wire_index_streams_device(pbft_ctx *ctx, const uint8_t *d_stream, uint64_t stream_bytes,
                                   const uint64_t *d_seg_off, const uint64_t *d_seg_len, const uint16_t *d_seg_peer,
                                   uint32_t S, uint64_t frame_cap, uint64_t *d_off, uint32_t *d_len, uint16_t *d_peer,
                                   pbft_seg_head *d_seg_heads, uint32_t *d_n_frames, void *stream);

/* Pre-size the index workspace for calls of up to max_stream_bytes and max_segments at the current tile size
 * (PBFT_OPT_INDEX_TILE): required before a capture. */
int pbft_index_reserve(pbft_ctx *ctx, uint64_t max_stream_bytes, uint32_t max_segments);

/* Device, enqueue only, one stream: the index, then pbft_verify_frames_tally_device with N = frame_cap over the
 * index it wrote.  Every buffer is the caller's, as for that function; the per-frame and per-envelope outputs are
 * word for word what it writes when handed the same padded index.  Call pbft_verify_reserve(frame_cap),
 * pbft_group_reserve(frame_cap) and pbft_index_reserve before a capture.  Argument checks of both functions, all in
 * front of the first launch. */
int pbft_verify_streams_tally_device(pbft_ctx *ctx, const uint8_t *d_stream, uint64_t stream_bytes,
                                     const uint64_t *d_seg_off, const uint64_t *d_seg_len, const uint16_t *d_seg_peer,
                                     uint32_t S, uint32_t n_replicas, uint64_t frame_cap, uint64_t *d_off,
                                     uint32_t *d_len, uint16_t *d_peer, pbft_seg_head *d_seg_heads,
                                     uint32_t *d_n_frames, uint8_t *d_records, pbft_frame_head *d_heads,
                                     uint64_t *d_bitmap, uint32_t env_cap, uint32_t *d_env_idx, uint8_t *d_envelopes,
                                     uint32_t *d_n_env, uint64_t *d_signers, uint32_t *d_count, void *stream);

/* Host, blocking: the stream and the segment table go up, the index is made on the device, the totals and the segment
 * heads come back; then the front half of pbft_verify_frames_tally runs on N = min(total, frame_cap) frames with the
 * index where it is (it comes back only if a frame is PBFT_WIRE_EDEFER, for the host parser, or if off_out /
 * flen_out are not NULL), then group, verify and tally.  Outputs as pbft_verify_frames_tally (the per-frame ones hold
 * frame_cap entries, N are written) plus seg_heads_out [S], n_frames_out [2] and, unless NULL, off_out / flen_out
 * [frame_cap]: equal to that function fed with the host index of every segment and a per-frame peer array. */
int pbft_verify_streams_tally(pbft_ctx *ctx, const uint8_t *stream, uint64_t stream_bytes, const uint64_t *seg_off,
                              const uint64_t *seg_len, const uint16_t *seg_peer, uint32_t S, uint32_t n_replicas,
                              uint64_t frame_cap, uint32_t env_cap, uint64_t *bitmap_out, pbft_frame_head *heads_out,
                              uint32_t *env_idx_out, uint8_t *envelopes_out, uint32_t *n_env_out,
                              uint64_t *signers_out, uint32_t *count_out, pbft_seg_head *seg_heads_out,
                              uint32_t *n_frames_out, uint64_t *off_out, uint32_t *flen_out);

/* ---- The replica's admission pass on the device (kernels: pbft_amd/csrc/admit.hip; rule: admit_core.h) ----
 * What pbft_replica_push_frames does with a frame before it touches a round window, for N decoded frames at once,
 * from their heads and the replica's (view, h, log_window).  The view is tested before the window, as
 * pbft_replica_push does; the window is seq in (h, h + log_window] (seq - h <= log_window: a window that reaches past
 * 2^64 - 1 ends there).  Frame f gets one class: */
#define PBFT_ADMIT_CLEAN 0         /* an OK Prepare / Commit of this view inside the window, the only such row of its
                                      (kind, seq, signer) in the call: what becomes of it is a function of the
                                      window's state and of two signer sets per envelope */
#define PBFT_ADMIT_CONTESTED 1     /* ... that shares its (kind, seq, signer) with another such row (found exactly) */
#define PBFT_ADMIT_REJ_VIEW 2      /* an OK vote of another view */
#define PBFT_ADMIT_REJ_WATERMARK 3 /* an OK vote of this view outside the window */
#define PBFT_ADMIT_REJ_SIGNER 4    /* PBFT_WIRE_ESIGNER (also an OK vote whose key index is >= n_keys) */
#define PBFT_ADMIT_HOST 5          /* every other status that is not PBFT_WIRE_OK (PBFT_WIRE_EDEFER: a PrePrepare, a
                                      ClientRequest, a non-canonical vote), and an OK head of kind 0 */
#define PBFT_ADMIT_PAD 6           /* f >= min(d_n_frames[0], N): the index's padding */
#define PBFT_ADMIT_CLASSES 8       /* entries of d_counts (entry 7 is 0) */
typedef struct {
  uint64_t off;   /* d_off[frame]: the body's absolute offset in the stream */
  uint32_t frame; /* the frame's number */
  uint32_t len;   /* d_len[frame] */
} pbft_admit_residue;

/* Device, enqueue only (five kernel nodes on one stream: no allocation, copy, memset or synchronisation, no lane waits
 * for another block; capturable after pbft_admit_reserve).  d_heads [N] and d_records [N][160] as the frame decoder
 * wrote them; d_off / d_len [N]: the index (NULL: the residue's off / len are 0); d_n_frames: NULL (all N rows are
 * frames) or the index's {total, not written}, read on the device.  Outputs: d_class [N] bytes; d_counts
 * [PBFT_ADMIT_CLASSES] rows per class; d_clean [ceil(N / 64)] bit f = frame f is clean; d_res [residue_cap] the frames
 * of class CONTESTED or HOST in frame order (entries from min(total, residue_cap) on are zero) and d_n_res [2] =
 * {total, not written}; and, in place, key index 0xFFFF at byte 150 of the record of every row that is not clean, so
 * that pbft_group_envelopes_device, pbft_verify_records_device and pbft_tally_device skip it without change.
 * PBFT_EINVAL: a null pointer that would be used or a misaligned one, N > 2^31, n_keys 0 or > 65535, log_window 0 or
 * 2 * log_window * n_keys > 2^30 (the two key planes have one bit per (kind, seq, signer) of the window); a refused
 * call has enqueued nothing.  The workspace (2 * log_window * n_keys / 4 bytes, plus 1.5 bits per row) grows on first
 * use of a larger call, which is then not capturable. */
int pbft_admit_device(pbft_ctx *ctx, const pbft_frame_head *d_heads, uint8_t *d_records, const uint64_t *d_off,
                      const uint32_t *d_len, const uint32_t *d_n_frames, uint64_t N, uint64_t view, uint64_t h,
                      uint64_t log_window, uint32_t n_keys, uint32_t residue_cap, uint8_t *d_class, uint32_t *d_counts,
                      uint64_t *d_clean, pbft_admit_residue *d_res, uint32_t *d_n_res, void *stream);

/* Pre-size the admission workspace for calls of up to max_n rows at (log_window, n_keys): required before a capture. */
int pbft_admit_reserve(pbft_ctx *ctx, uint64_t log_window, uint32_t n_keys, uint64_t max_n);

/* Host, blocking: connection streams in, signer sets out -- the device half of pbft_replica_push_streams
 * (include/pbft_replica.h).  The stream and the segment table go up; then, enqueued once over N = frame_cap rows on
 * the context's stream: pbft_wire_index_streams_device, pbft_wire_decode_frames_device (peer = the segment's,
 * n_replicas), pbft_admit_device (n_keys = n_replicas), pbft_group_envelopes_device, pbft_verify_records_device,
 * pbft_tally_device over the clean bitmap (present_out: who sent each envelope) and pbft_tally_device over the verify
 * bitmap (valid_out: whose signature verified); rows that are not clean carry key index 0xFFFF and take part in
 * neither.  Back: seg_heads_out [S], n_frames_out [2], counts_out [PBFT_ADMIT_CLASSES], envelopes_out [env_cap][85],
 * n_env_out [2], present_out / valid_out [env_cap][ceil(n_replicas / 64)], res_out [residue_cap], n_res_out [2];
 * nothing per clean vote.  The caller compares n_frames_out[0] with frame_cap, n_env_out[0] with env_cap and
 * n_res_out[0] with residue_cap: beyond a cap the outputs are incomplete (never wrong for what they hold).
 * PBFT_EINVAL: a null argument, frame_cap or env_cap 0, and the range checks of the functions above; PBFT_ENOKEYS with
 * fewer than n_replicas keys installed; PBFT_EBUSY while an asynchronous batch is in flight. */
int pbft_verify_streams_admit(pbft_ctx *ctx, const uint8_t *stream, uint64_t stream_bytes, const uint64_t *seg_off,
                              const uint64_t *seg_len, const uint16_t *seg_peer, uint32_t S, uint32_t n_replicas,
                              uint64_t frame_cap, uint32_t env_cap, uint32_t residue_cap, uint64_t view, uint64_t h,
                              uint64_t log_window, pbft_seg_head *seg_heads_out, uint32_t *n_frames_out,
                              uint32_t *counts_out, uint8_t *envelopes_out, uint32_t *n_env_out, uint64_t *present_out,
                              uint64_t *valid_out, pbft_admit_residue *res_out, uint32_t *n_res_out);
/* Size the staging (the PrePrepare heads' residue_cap x sizeof(pbft_pp_head) included) and the index, grouping,
 * admission and verification workspaces of the call above and of pbft_verify_streams_admit_pp for these caps. */
int pbft_streams_admit_reserve(pbft_ctx *ctx, uint64_t max_stream_bytes, uint32_t max_segments, uint32_t n_replicas,
                               uint64_t frame_cap, uint32_t env_cap, uint32_t residue_cap, uint64_t log_window);

/* ---- The residue's PrePrepares parsed and digested on the device (kernels: pbft_amd/csrc/wire_pp.hip; rule:
 * wire_pp_core.h) ----
 * The canonical signed PrePrepare, exactly what pbft_wire_encode_json writes,
 *   {"PrePrepare":{"view":V,"sequence_number":N,"digest":"<128 hex>","message":{"operation":"OP","timestamp":T,
 *   "client":"C"},"replica":R,"signature":"<128 hex>"}}
 * with V, N, T serde u64, R <= 65535, lowercase hex, OP of 0 .. PBFT_PP_OP_MAX and C of 1 .. 63 bytes in 0x20 .. 0x7E
 * other than '"' and '\', nothing behind "}}" (PBFT_PP_FRAME_MIN .. PBFT_PP_FRAME_MAX bytes), is PBFT_PP_OK.  Anything
 * else -- a vote, a ClientRequest, whitespace, another field order, an escape, a non-ASCII or oversize operation -- is
 * PBFT_PP_NONE: pbft_wire_decode_json decides.  PBFT_PP_OK implies that pbft_wire_decode_json accepts the frame as a
 * PrePrepare with digest_ok and has_sig, the same view, seq, replica, timestamp, digest and signature, and an
 * operation equal to bytes [op_off, op_off + op_len) of the body. */
#define PBFT_PP_OP_MAX 3072
#define PBFT_PP_FRAME_MIN 394
#define PBFT_PP_FRAME_MAX (517 + PBFT_PP_OP_MAX)
#define PBFT_PP_NONE 0
#define PBFT_PP_OK 1
typedef struct {
  uint64_t view, seq, timestamp;
  uint32_t op_off, op_len; /* the operation's bytes, counted from the body's first byte */
  uint16_t replica;
  uint8_t status; /* PBFT_PP_* */
  uint8_t pad[5];
  uint8_t claimed[64];  /* the frame's "digest" */
  uint8_t computed[64]; /* Blake2b-512 of the operation */
  uint8_t sig[64];
} pbft_pp_head; /* all zero when status is PBFT_PP_NONE */

/* Host, one frame, no context and no GPU: the rule above and the digest.  Returns 0 (the answer is out->status), or
 * PBFT_EINVAL for a null argument. */
int pbft_wire_decode_preprepare(const uint8_t *body, size_t len, pbft_pp_head *out);

/* Device, enqueue only (two kernel nodes on one stream: no allocation, copy, memset or synchronisation, no lane waits
 * for another block, every loop is bounded; capturable).  Entry i < min(d_n_res[0], residue_cap) of d_res (as
 * pbft_admit_device wrote it; d_n_res NULL: all residue_cap entries are live) -> d_pp[i]; the entries behind that are
 * zeroed.  d_stream as for pbft_wire_decode_frames_device: 16-byte aligned, readable up to stream_bytes rounded up to
 * 16, only granules of that range are read; an entry that does not lie inside stream_bytes is PBFT_PP_NONE and is not
 * read.  PBFT_EINVAL: a null or misaligned pointer (d_res, d_pp 8 bytes, d_n_res 4), stream_bytes > 2^31; a refused
 * call has enqueued nothing.  residue_cap = 0 enqueues nothing. */
int pbft_wire_decode_preprepares_device(pbft_ctx *ctx, const uint8_t *d_stream, uint64_t stream_bytes,
                                        const pbft_admit_residue *d_res, const uint32_t *d_n_res, uint32_t residue_cap,
                                        pbft_pp_head *d_pp, void *stream);

/* pbft_verify_streams_admit with one more output, pp_out [residue_cap]; pp_out NULL is that call.  After the chain's one
 * synchronisation, and only if counts_out[PBFT_ADMIT_HOST] is not 0, the two kernels above run over the
 * k = min(n_res_out[0], residue_cap) residue entries where they lie on the device and pp_out[0 .. k) comes back: one
 * more launch pair, copy and synchronisation.  Otherwise (no frame of the call can be a PrePrepare) pp_out is not
 * touched and the call enqueues, copies and synchronises exactly as pbft_verify_streams_admit. */
int pbft_verify_streams_admit_pp(pbft_ctx *ctx, const uint8_t *stream, uint64_t stream_bytes, const uint64_t *seg_off,
                                 const uint64_t *seg_len, const uint16_t *seg_peer, uint32_t S, uint32_t n_replicas,
                                 uint64_t frame_cap, uint32_t env_cap, uint32_t residue_cap, uint64_t view, uint64_t h,
                                 uint64_t log_window, pbft_seg_head *seg_heads_out, uint32_t *n_frames_out,
                                 uint32_t *counts_out, uint8_t *envelopes_out, uint32_t *n_env_out,
                                 uint64_t *present_out, uint64_t *valid_out, pbft_admit_residue *res_out,
                                 uint32_t *n_res_out, pbft_pp_head *pp_out);

/* ---- egress: the replica's own votes signed and framed on the device (kernels: pbft_amd/csrc/egress.hip) ----
 * The other direction of everything above.  Envelope i = the 85 bytes at env + i * env_stride (env_stride >= 85,
 * pbft_envelope: "PBFT" | kind | view LE | seq LE | digest[64]) is both the signed message and everything its frame
 * holds except the signer.  The context signs it with the identity of pbft_sign_set_seed (include/pbft_verify.h;
 * PBFT_EINVAL without one) and writes the canonical frame of that vote, with "replica" = the index given there.  The
 * output is the concatenation of the N frames, byte for byte what pbft_wire_encode_votes writes for the same votes with
 * RFC 8032 signatures (which are deterministic): frame i occupies [frame_off[i], frame_off[i + 1]) and frame_off[N] is
 * the total.  An envelope whose magic is wrong or whose kind is not 1 (Prepare) or 2 (Commit) has no frame: length 0,
 * signature 64 zero bytes; its neighbours are unaffected.  sigs (optional) receives R || S of every envelope.
 *
 * Device form, enqueue only on `stream` (NULL = the context's): three kernel nodes -- the frame lengths and their scan
 * inside each 64-envelope tile, the scan over the tiles, one signature per lane and the frames -- with no allocation,
 * copy, memset or synchronisation once pbft_egress_reserve(max_n >= N) has sized the workspace (8 bytes per 64
 * envelopes); capturable as a plain chain.  N <= 2^24.  d_out may have any alignment; d_frame_off [N + 1] is 8-byte
 * aligned, d_sigs [N][64] 4-byte.  Nothing is read beyond envelope N - 1's 85 bytes.  When the stream would exceed
 * out_cap, the frames that do not fit entirely are not written, none is written in part, nothing at or beyond
 * d_out + out_cap is touched, and d_frame_off (and d_sigs) are still complete.  Calls of one context share the
 * workspace and must be ordered, like its verify launches. */
/* Measuring (pbft_verify_set_option): the form of the signing kernel: lanes per workgroup, 64 (default; 0 restores
 * it) or 256, and 1 = every lane stores its own frame bytewise instead of the wave staging its 64 frames in LDS and
 * storing the span with 16-byte stores (default 0).  The output does not depend on either. */
#define PBFT_OPT_EGRESS_BLOCK 20
#define PBFT_OPT_EGRESS_DIRECT 21
int pbft_egress_reserve(pbft_ctx *ctx, uint64_t max_n);
int pbft_sign_votes_frames_device(pbft_ctx *ctx, const uint8_t *d_env, uint32_t env_stride, uint64_t N,
                                  uint8_t *d_out, uint64_t out_cap, uint64_t *d_frame_off, uint8_t *d_sigs,
                                  void *stream);
/* Blocking, host buffers.  *len = the bytes needed, computed on the host before anything runs; when cap is smaller:
 * PBFT_EINVAL, nothing written and nothing launched (out = NULL, cap = 0 asks for the length).  frame_off [N + 1]
 * and sigs [N][64] are optional.  PBFT_EBUSY while an async batch is in flight on the context. */
int pbft_sign_votes_frames(pbft_ctx *ctx, const uint8_t *envelopes, uint32_t env_stride, uint64_t N, uint8_t *out,
                           size_t cap, size_t *len, uint64_t *frame_off, uint8_t *sigs);

/* ---- the primary's proposals: client requests in, signed PrePrepare frames out (kernels: pbft_amd/csrc/propose.hip;
 * frame rule: propose_core.h) ----
 * What Pbft::add_client_request does with a ClientRequest (src/behavior.rs:63-98): the next sequence number, the
 * operation's Blake2b-512 digest, the PrePrepare, its multicast.  Request i = operation bytes
 * [op_off[i], op_off[i] + op_len[i]) of `ops`, timestamp[i] and the client's address in the 64-byte field
 * clients + 64 * i (up to its first NUL); its sequence number is first_seq + i.  A request is canonical when its
 * operation has 0 .. PBFT_PP_OP_MAX bytes and its client 1 .. 63, all of them 0x20 .. 0x7E other than '"' and '\': its
 * frame needs no escaping, is PBFT_PP_FRAME_MIN .. PBFT_PP_FRAME_MAX bytes plus a two-byte varint, and is exactly what
 * pbft_wire_decode_preprepare (and the device path behind pbft_replica_push_streams) answers with PBFT_PP_OK. */
#define PBFT_PROPOSE_OK 0      /* canonical: the core's frame                                                       */
#define PBFT_PROPOSE_GENERAL 1 /* any other request: the frame pbft_wire_encode_frame writes (escapes, long operations,
                                  an empty or 64-byte client); the device forms write none                          */

/* Host, no context and no GPU: the N signed PrePrepares as consecutive UviBytes frames, for each i byte for byte
 * pbft_wire_encode_frame of {PrePrepare, view, first_seq + i, digests[i], request i, replica, sigs[i]} -- the analogue of
 * pbft_wire_encode_votes and the reference form of the functions below.  *len = the stream's full length; returns 0, or
 * PBFT_EINVAL if cap is too small (then *len still tells the length needed), first_seq + N - 1 wraps, replica > 65535
 * or an argument is null.  digests and sigs may be NULL for the length query (out = NULL, cap = 0): no frame's length
 * depends on them.  frame_off [N + 1] (frame i occupies [frame_off[i], frame_off[i + 1])) and status [N]
 * (PBFT_PROPOSE_*) are optional and complete whatever cap is. */
int pbft_wire_encode_preprepares(uint64_t N, uint64_t view, uint64_t first_seq, const uint8_t *ops,
                                 const uint64_t *op_off, const uint32_t *op_len, const uint64_t *timestamp,
                                 const char *clients /* [N][64] */, uint32_t replica,
                                 const uint8_t *digests /* [N][64] */, const uint8_t *sigs /* [N][64] */, uint8_t *out,
                                 size_t cap, size_t *len, uint64_t *frame_off, uint8_t *status);

/* Device form, enqueue only on `stream` (NULL = the context's): three kernel nodes -- the canonical test, the frame
 * lengths and their scan inside each 64-request tile; the scan over the tiles; one digest and one signature per lane and
 * the frames -- with no allocation, copy, memset or synchronisation once pbft_propose_reserve(max_n >= N) has sized the
 * workspace (8 bytes per 64 requests); every loop is bounded; capturable as a plain chain.  The signer is the identity
 * of pbft_sign_set_seed (PBFT_EINVAL without one), "replica" the index given there.  N <= 2^24.
 * Per request i, whatever its form: d_digests[i] = Blake2b-512 of the operation where it lies, d_sigs[i] = the RFC 8032
 * signature over pbft_envelope(0, view, first_seq + i, digest).  A request whose operation does not lie inside
 * ops_bytes is not read: digest and signature zero, status PBFT_PROPOSE_GENERAL.
 * A canonical request has status PBFT_PROPOSE_OK and its frame at d_out + d_frame_off[i]; any other has status
 * PBFT_PROPOSE_GENERAL and frame length 0; d_frame_off[N] is the total.  The frames equal
 * pbft_wire_encode_preprepares restricted to the OK requests.  When the stream would exceed out_cap, the frames that do
 * not fit entirely are not written, none is written in part, nothing at or beyond d_out + out_cap is touched, and
 * d_frame_off, d_digests, d_sigs and d_status are still complete.
 * d_out may have any alignment; d_ops is 16-byte aligned and nothing outside [d_ops, round_up(ops_bytes, 16)) is read;
 * d_op_off, d_timestamp, d_frame_off 8-byte aligned, d_op_len, d_digests, d_sigs 4-byte.  PBFT_EINVAL: a null or
 * misaligned pointer, N > 2^24, first_seq + N - 1 wraps; a refused call has enqueued nothing.  Calls of one context share
 * the workspace and must be ordered, like its other launches. */
/* Measuring (pbft_verify_set_option): bytes per store when the wave copies a frame to d_out: 1, 4 (default; 0 restores
 * it) or 16 (the output's aligned dwords / 16-byte granules with one store each).  The output does not depend on it. */
#define PBFT_OPT_PROPOSE_WIDTH 22
int pbft_propose_reserve(pbft_ctx *ctx, uint64_t max_n);
int pbft_sign_preprepares_frames_device(pbft_ctx *ctx, const uint8_t *d_ops, uint64_t ops_bytes,
                                        const uint64_t *d_op_off, const uint32_t *d_op_len,
                                        const uint64_t *d_timestamp, const uint8_t *d_clients, uint64_t view,
                                        uint64_t first_seq, uint64_t N, uint8_t *d_out, uint64_t out_cap,
                                        uint64_t *d_frame_off, uint8_t *d_digests, uint8_t *d_sigs, uint8_t *d_status,
                                        void *stream);
/* Blocking, host buffers; the complete form: its output equals pbft_wire_encode_preprepares for every input, with the
 * digests and signatures made on the device.  *len = the bytes needed, computed on the host before anything runs; when
 * cap is smaller: PBFT_EINVAL, nothing written and nothing launched (out = NULL, cap = 0 asks for the length).  The
 * device form runs over all N requests; if any status is PBFT_PROPOSE_GENERAL the stream is completed on the host: the
 * device's frames in order, the others encoded by pbft_wire_encode_frame from the digest and signature that came back.
 * frame_off [N + 1], digests, sigs [N][64] and status [N] are optional.  PBFT_EINVAL also for an operation outside
 * ops_bytes; PBFT_EBUSY while an async batch is in flight on the context. */
int pbft_sign_preprepares_frames(pbft_ctx *ctx, const uint8_t *ops, uint64_t ops_bytes, const uint64_t *op_off,
                                 const uint32_t *op_len, const uint64_t *timestamp, const char *clients, uint64_t view,
                                 uint64_t first_seq, uint64_t N, uint8_t *out, size_t cap, size_t *len,
                                 uint64_t *frame_off, uint8_t *digests, uint8_t *sigs, uint8_t *status);

/* ---- client replies: committed requests in, signed replies out (kernels: pbft_amd/csrc/reply.hip; text rule:
 * reply_core.h) ----
 * What inject_node_event does behind committed_local (src/behavior.rs:382-411) once the request is executed: the
 * ClientReply (src/message.rs:54-103), here signed.  Reply i = result bytes [res_off[i], res_off[i] + res_len[i]) of
 * `results`, timestamp[i] and the client's 64-byte field clients + 64 * i (as pbft_wire_encode_preprepares takes it).
 * Its text is the reference's serialization in the reference's field order, then the two fields of every signed message:
 *   {"view":V,"timestamp":T,"peer_id":"<52 base58 chars>","result":"R","replica":I,"signature":"<128 hex>"}
 * with no varint in front: the reference writes reply.to_string() raw, one reply per connection
 * (src/client_handler.rs:75-84).  The signature is RFC 8032 over pbft_reply_envelope(view, timestamp, D),
 *   "PBFT" | 3 | view LE | timestamp LE | D,   D = Blake2b-512(C[64] | result bytes),
 * where C is the client field with everything from its first NUL on replaced by zeros (a field without a NUL is taken
 * whole).  The serialized reply does not carry the client; D binds it, so f + 1 replies to one client cannot be replayed
 * to another whose request has the same timestamp.  Kind 3 cannot be replayed as a vote or a PrePrepare: the egress rule
 * (eg_env_kind) answers 0 for it and the admission path knows kinds 0 .. 2 only.
 * A reply is canonical when its result has 0 .. PBFT_REPLY_RESULT_MAX bytes, all of them 0x20 .. 0x7E other than '"'
 * and '\': its text needs no escaping. */
#define PBFT_KIND_REPLY 3
#define PBFT_REPLY_RESULT_MAX 3072
#define PBFT_REPLY_PEER_ID_CHARS 52
#define PBFT_REPLY_OK 0            /* canonical: the core's text                                                    */
#define PBFT_REPLY_GENERAL 1       /* any other result: the serde-exact string escaper; the device forms write none */
#define PBFT_REPLY_STALE 2         /* pbft_replica_reply only: timestamp <= last_timestamp, no text                 */
#define PBFT_REPLY_NOT_COMMITTED 3 /* pbft_replica_reply only: (view, seq) is not committed-local, no text          */

/* Host, no context and no GPU: digests_out[i] = D of reply i as defined above.  PBFT_EINVAL: a null argument, a result
 * outside results_bytes. */
int pbft_reply_digests(uint64_t N, const char *clients /* [N][64] */, const uint8_t *results, uint64_t results_bytes,
                       const uint64_t *res_off, const uint32_t *res_len, uint8_t *digests_out /* [N][64] */);

/* Host, no context and no GPU: the N signed replies' texts back to back, the reference form of the functions below.  A
 * canonical result takes the core's writer (PBFT_REPLY_OK); any other goes through the codec's serde-exact string
 * escaper (PBFT_REPLY_GENERAL).  A result that is not valid UTF-8 is treated as pbft_wire_encode_preprepares treats such
 * an operation: its bytes >= 0x80 are written as they are and nothing is validated (serde could not have produced such a
 * String; a JSON parser will refuse the text).  *len = the full length; returns 0, or PBFT_EINVAL if cap is too small
 * (then *len, reply_off and status are still set), replica > 65535 or an argument is null.  sigs may be NULL for the
 * length query (out = NULL, cap = 0): no text's length depends on it; peer_id may then be NULL too.  reply_off [N + 1]
 * (reply i occupies [reply_off[i], reply_off[i + 1])) and status [N] are optional and complete whatever cap is. */
int pbft_wire_encode_replies(uint64_t N, uint64_t view, const uint64_t *timestamp, const uint8_t *results,
                             const uint64_t *res_off, const uint32_t *res_len, uint32_t replica,
                             const char *peer_id /* [52] */, const uint8_t *sigs /* [N][64] */, uint8_t *out, size_t cap,
                             size_t *len, uint64_t *reply_off, uint8_t *status);

/* The reader-side twin, for clients and tests: a byte-for-byte matcher of the canonical text, one reply, no context.
 * PBFT_RH_OK implies that the writer, given the same fields, writes the same bytes.  Anything else -- whitespace, another
 * field order, an escape, a 51-character peer id, an uppercase hex digit, a trailing byte, a result above
 * PBFT_REPLY_RESULT_MAX -- is PBFT_RH_NONE (a general JSON parser decides).  peer_id is the text as it stands
 * (pbft_key_from_peer_id_b58 gives the key).  Returns 0 (the answer is out->status) or PBFT_EINVAL for a null argument. */
#define PBFT_RH_NONE 0
#define PBFT_RH_OK 1
typedef struct {
  uint64_t view, timestamp;
  uint32_t result_off, result_len; /* the result's bytes, counted from the text's first byte */
  uint32_t replica;
  uint32_t status; /* PBFT_RH_* */
  char peer_id[PBFT_REPLY_PEER_ID_CHARS];
  uint8_t sig[64];
  uint8_t pad[4];
} pbft_reply_head; /* all zero when status is PBFT_RH_NONE */
int pbft_wire_decode_reply(const uint8_t *text, size_t len, pbft_reply_head *out);

/* Device form, enqueue only on `stream` (NULL = the context's): three kernel nodes -- the canonical test, the text
 * lengths and their scan inside each 64-reply tile; the scan over the tiles; one digest and one signature per lane and
 * the texts -- with no allocation, copy, memset or synchronisation once pbft_reply_reserve(max_n >= N) has sized the
 * workspace (8 bytes per 64 replies); every loop is bounded; no lane waits for another block; capturable as a plain
 * chain.  The signer and the "peer_id" are the identity of pbft_sign_set_seed (PBFT_EINVAL without one), "replica" the
 * index given there.  N <= 2^24.
 * Per reply i, whatever its form: d_digests[i] = D, d_sigs[i] = the signature over the kind-3 envelope.  A result that
 * does not lie inside results_bytes is not read: digest and signature zero, status PBFT_REPLY_GENERAL.
 * A canonical reply has status PBFT_REPLY_OK and its text at d_out + d_reply_off[i]; any other has status
 * PBFT_REPLY_GENERAL and length 0; d_reply_off[N] is the total.  The texts equal pbft_wire_encode_replies restricted to
 * the OK replies.  When the stream would exceed out_cap, the replies that do not fit entirely are not written, none is
 * written in part, nothing at or beyond d_out + out_cap is touched, and d_reply_off, d_digests, d_sigs and d_status are
 * still complete.
 * d_out may have any alignment; d_results is 16-byte aligned and nothing outside [d_results, round_up(results_bytes, 4))
 * is read; d_res_off, d_timestamp, d_reply_off 8-byte aligned, d_res_len, d_digests, d_sigs 4-byte.  PBFT_EINVAL: a null
 * or misaligned pointer, N > 2^24; a refused call has enqueued nothing.  Calls of one context share the workspace and
 * must be ordered, like its other launches. */
int pbft_reply_reserve(pbft_ctx *ctx, uint64_t max_n);
int pbft_sign_replies_device(pbft_ctx *ctx, const uint8_t *d_results, uint64_t results_bytes, const uint64_t *d_res_off,
                             const uint32_t *d_res_len, const uint64_t *d_timestamp, const uint8_t *d_clients,
                             uint64_t view, uint64_t N, uint8_t *d_out, uint64_t out_cap, uint64_t *d_reply_off,
                             uint8_t *d_digests, uint8_t *d_sigs, uint8_t *d_status, void *stream);
/* Blocking, host buffers; the complete form: its output equals pbft_wire_encode_replies for every input, with the
 * digests and signatures made on the device.  *len = the bytes needed and the status, computed on the host before
 * anything runs; when cap is smaller: PBFT_EINVAL, nothing written and nothing launched; out = NULL with cap = 0 is
 * the size query and returns 0, as pbft_wire_encode_replies and pbft_replica_reply do.  If any status is
 * PBFT_REPLY_GENERAL the stream is completed on the host: the device's replies in order, the others written by the
 * host encoder from the signature that came back.  reply_off [N + 1], digests, sigs [N][64] and status [N] are
 * optional.  PBFT_EINVAL also for a result outside results_bytes; PBFT_EBUSY while an async batch is in flight on the
 * context. */
int pbft_sign_replies(pbft_ctx *ctx, const uint8_t *results, uint64_t results_bytes, const uint64_t *res_off,
                      const uint32_t *res_len, const uint64_t *timestamp, const char *clients, uint64_t view, uint64_t N,
                      uint8_t *out, size_t cap, size_t *len, uint64_t *reply_off, uint8_t *digests, uint8_t *sigs,
                      uint8_t *status);

/* ---- the client's side: signed replies in, f + 1 results out (kernels: pbft_amd/csrc/accept.hip; rule:
 * accept_core.h) ----
 * A client acts on a result once f + 1 distinct replicas have sent it matching signed replies.  A batch holds N reply
 * texts, reply i = bytes [off[i], off[i] + len[i]) of one buffer, raw as they arrive (one per connection, no varint);
 * clients [n_clients][64] are the client address fields these replies were sent to, in the form pbft_reply_digests takes,
 * and client_idx[i] names reply i's (NULL: every reply is client 0's).
 * Replies arrive on unauthenticated connections, so the signer is what the text claims and the signature is the
 * authentication.  Both claims must name the same installed key: "replica":I must be below the installed key count and
 * "peer_id" must equal, byte for byte, the 52-character PeerId text of installed key I (a per-context device table
 * built on the host by pbft_accept_reserve: there is no base58 on the device).
 * The status of reply i, decided in this order: */
#define PBFT_ACCEPT_OK 0      /* canonical (exactly pbft_wire_decode_reply -> PBFT_RH_OK), the signer's claim holds and
                                 client_idx[i] < n_clients                                                             */
#define PBFT_ACCEPT_EDEFER 1  /* not canonical, or not inside text_bytes (then not read); device forms only           */
#define PBFT_ACCEPT_ESIGNER 2 /* replica >= the installed key count, or the peer id is not that key's                 */
#define PBFT_ACCEPT_ECLIENT 3 /* client_idx[i] >= n_clients (decided before any address of the table is formed)       */
#define PBFT_ACCEPT_EJSON 4   /* pbft_accept_replies only: not a ClientReply with the two signed fields               */
/* A flag beside PBFT_ACCEPT_OK in the status of a reply pbft_accept_replies settled on the host (status & 0xFF is the
 * value above): the result between the quotes holds a JSON escape; result_off / result_len give that raw span. */
#define PBFT_ACCEPT_ESCAPED 0x100
#define PBFT_ACCEPT_NO_REPLY 0xFFFFFFFFu
/* An OK reply's record is the 160-byte record above: R | S from the hex, pbft_reply_envelope(view, timestamp, D) with
 * D = Blake2b-512(C | result), the result hashed where it lies in the text, and key index I.  Every other reply has the
 * all-zero record with key index 0xFFFF, as the frame decoder marks a frame that is not OK, and all-zero head fields
 * beside its status.
 * Two replies match iff their 85-byte kind-3 envelopes are equal: the same view, timestamp, client field and result
 * bytes.  The view is in the match, so replies of different views do not combine; the reference's view is constant and
 * view change is out of scope. */
typedef struct {
  uint64_t view, timestamp;
  uint32_t result_off, result_len; /* the result's bytes, counted from the text's first byte */
  uint32_t replica;
  uint32_t status; /* PBFT_ACCEPT_* (| PBFT_ACCEPT_ESCAPED) */
} pbft_accept_head;
/* One per envelope e < min(n_env[0], env_cap): first = the least reply index i with env_idx[i] == e whose signature
 * verified (that reply's text holds the result the client reads; PBFT_ACCEPT_NO_REPLY when there is none), count = the
 * tally's distinct-signer count, client = client_idx[first] (0 without one), accepted = count >= need.  Entries at or
 * beyond the number of envelopes are zero with first = PBFT_ACCEPT_NO_REPLY. */
typedef struct {
  uint64_t view, timestamp;
  uint32_t first, count, client, accepted;
} pbft_accept_cert;
#ifdef __cplusplus
static_assert(sizeof(pbft_accept_head) == 32 && sizeof(pbft_accept_cert) == 32, "32 bytes each");
#endif

/* Host, one text, no context and no GPU: the general reader pbft_wire_decode_reply leaves to "a general JSON parser".
 * A serde-exact parse of the signed ClientReply with pbft_wire_decode_json's tokenizer: any whitespace and field order,
 * unknown fields ignored, a duplicate field an error, "view", "timestamp" and "replica" by serde's u64 rules (replica
 * <= 65535), "peer_id" exactly 52 base58 characters, "signature" exactly 128 lowercase hex characters (upper case is
 * refused, as pbft_wire_decode_json refuses it in a vote's signature), all six fields present, valid UTF-8, nothing
 * behind the closing brace.  The result's JSON escapes are decoded: its bytes are arena[0, return value).
 * On a text pbft_wire_decode_reply answers PBFT_RH_OK for, head_out is what that function writes.  On any other text that
 * parses, status is PBFT_RH_GENERAL and result_off / result_len give the raw span between the result's quotes.
 * Returns the result's length (>= 0), or PBFT_EINVAL (head_out zeroed) for a text that does not parse, an arena that
 * is too small (len bytes always suffice) or a null argument. */
#define PBFT_RH_GENERAL 2
int pbft_wire_decode_reply_json(const uint8_t *text, size_t len, pbft_reply_head *head_out, char *arena,
                                size_t arena_cap);

/* Build the context's PeerId table [n_keys][52] from the installed key set (PBFT_ENOKEYS without one) and size the
 * staging of pbft_accept_replies for max_n replies.  Blocking.  The table follows the key set: after
 * pbft_verify_set_keys or pbft_verify_update_keys (on this context or one that shares its key set) it is stale, the
 * device forms below answer PBFT_EINVAL until this function is called again, and pbft_accept_replies rebuilds it
 * itself.  pbft_verify_revoke_keys leaves it as it is: a revoked slot verifies nothing. */
int pbft_accept_reserve(pbft_ctx *ctx, uint64_t max_n);

/* Device, enqueue only (one kernel node: no allocation, copy, memset or synchronisation, every loop is bounded, no lane
 * waits for another block; capturable): reply i -> d_records[i], d_heads[i].  d_text is 16-byte aligned and nothing
 * outside [d_text, round_up(text_bytes, 16)) is read; no byte outside a reply's own [off, off + len) enters its head,
 * its record or D.  d_records 16-byte aligned, d_off and d_heads 8, d_len and d_client_idx 4.  PBFT_EINVAL: a null or
 * misaligned pointer, N > 2^24, text_bytes > 2^31, a stale or missing PeerId table; PBFT_ENOKEYS without a key set; a
 * refused call has enqueued nothing.  N = 0 enqueues nothing. */
int pbft_wire_decode_replies_device(pbft_ctx *ctx, const uint8_t *d_text, uint64_t text_bytes, const uint64_t *d_off,
                                    const uint32_t *d_len, const uint32_t *d_client_idx, const uint8_t *d_clients,
                                    uint32_t n_clients, uint64_t N, uint8_t *d_records, pbft_accept_head *d_heads,
                                    void *stream);

/* Replies in, certificates out.  Device, enqueue only, one stream: the decode above; pbft_group_envelopes_device over
 * d_records in place (envelope at +64, key index at +150, stride 160), which writes d_env_idx [N], d_envelopes
 * [env_cap][85] and d_n_env [2]; pbft_verify_records_device into d_bitmap; pbft_tally_device with n_signers = the
 * installed key count into d_signers [env_cap][ceil(n_keys / 64)] and d_count [env_cap]; and the certificates d_certs
 * [env_cap] (three kernel nodes: an initialising one, not a memset; atomicMin on first; the rest).  After
 * pbft_verify_reserve(N), pbft_group_reserve(N) and pbft_accept_reserve it does no allocation, copy, memset or
 * synchronisation and is capturable as a plain chain of kernel nodes.  An env_cap below the number of distinct envelopes
 * loses the later envelopes' replies (counted in d_n_env[1]) and never miscounts.  PBFT_EINVAL as the decode above and
 * for need = 0, env_cap = 0 with N > 0, a null or misaligned output; a refused call has enqueued nothing.  N = 0 writes
 * d_n_env = {0, 0} and zeroes the per-envelope outputs (first = PBFT_ACCEPT_NO_REPLY). */
int pbft_accept_replies_device(pbft_ctx *ctx, const uint8_t *d_text, uint64_t text_bytes, const uint64_t *d_off,
                               const uint32_t *d_len, const uint32_t *d_client_idx, const uint8_t *d_clients,
                               uint32_t n_clients, uint64_t N, uint32_t need, uint8_t *d_records,
                               pbft_accept_head *d_heads, uint64_t *d_bitmap, uint32_t env_cap, uint32_t *d_env_idx,
                               uint8_t *d_envelopes, uint32_t *d_n_env, uint64_t *d_signers, uint32_t *d_count,
                               pbft_accept_cert *d_certs, void *stream);

/* Host, blocking, the complete form.  Texts, index and clients go to the device, the decode runs there and the heads
 * come back; every PBFT_ACCEPT_EDEFER reply then goes through pbft_wire_decode_reply_json on the host: one that parses
 * gets the signer's and the client's rule, D from the host's Blake2b over the unescaped result, and its record and head
 * are patched on the device (PBFT_ACCEPT_OK, with PBFT_ACCEPT_ESCAPED when the raw span holds an escape); any other is
 * PBFT_ACCEPT_EJSON.  Then group, verify, tally and certify run on the settled records.  No status that comes back is
 * PBFT_ACCEPT_EDEFER.  Back per reply: bitmap_out [ceil(N / 64)], heads_out [N] and, unless NULL, env_idx_out [N]; per
 * envelope: envelopes_out [env_cap][85], n_env_out [2], signers_out [env_cap][ceil(n_keys / 64)], count_out [env_cap]
 * and certs_out [env_cap].  PBFT_EINVAL: a text outside text_bytes, need = 0, env_cap = 0 with N > 0, N > 2^24,
 * text_bytes > 2^31, a null output; PBFT_ENOKEYS without a key set; PBFT_EBUSY while an async batch is in flight. */
int pbft_accept_replies(pbft_ctx *ctx, const uint8_t *texts, uint64_t text_bytes, const uint64_t *off,
                        const uint32_t *len, const uint32_t *client_idx, const char *clients /* [n_clients][64] */,
                        uint32_t n_clients, uint64_t N, uint32_t need, uint32_t env_cap, uint64_t *bitmap_out,
                        pbft_accept_head *heads_out, uint32_t *env_idx_out, uint8_t *envelopes_out, uint32_t *n_env_out,
                        uint64_t *signers_out, uint32_t *count_out, pbft_accept_cert *certs_out);

#ifdef __cplusplus
}
#endif
#endif /* PBFT_WIRE_H */

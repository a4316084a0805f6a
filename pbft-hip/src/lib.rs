//! pbft-hip: the MI355X batch verifier that gates PBFT's Prepare / Commit quorums
//! (BASELINE.json north_star), as the crate ameya-deshmukh/pbft would depend on.
//!
//! * [`BatchVerifier`]: the trait of SURVEY.md §8(b) -- non-blocking `submit` + `poll`
//!   (fits `NetworkBehaviour::poll`, /root/reference/src/behavior.rs:416-426) and a
//!   blocking `verify`.  An invalid signature is a 0 bit, never an error (the reference
//!   panics through `.unwrap()`, src/behavior.rs:345, :371).
//! * [`GpuVerifier`]: the HIP implementation (libpbft_verify.so, gfx950).
//! * [`CpuVerifier`] (feature `cpu`): ed25519-dalek 1.0.1 `PublicKey::verify_strict` per
//!   signature -- the reference's own crypto (libp2p-core 0.31.1 -> ed25519-dalek 1.0.1,
//!   Cargo.lock:668-679).  UNTESTED: there is no Rust toolchain in the build image, so this
//!   implementation has never been compiled or run; the GPU path's bit-exactness is established
//!   against the repository's C and Python restatements of verify_strict (tests/golden), not
//!   against this code.
//! * [`Replica`]: the native round batcher + quorum state machine
//!   (include/pbft_replica.h) that replaces `validate_prepare` / `validate_commit`
//!   (src/behavior.rs:159-195) and keys votes by the authenticated peer
//!   (src/behavior.rs:346, :380); any `BatchVerifier` can back it.
//! * [`key_from_peer_id`]: libp2p PeerId -> Ed25519 key (src/main.rs:39-40).
//!
//! NOT COMPILED IN THIS REPOSITORY: the build image has no Rust toolchain.  Every C entry
//! point used here is exercised through ctypes by tests/ (CPU) and tests/ -m gpu (MI355X).
use std::ffi::CStr;
use std::fmt;
use std::marker::PhantomData;
use std::os::raw::{c_char, c_int, c_void};
use std::ptr;

pub mod ffi;

/// The 85-byte signed envelope: "PBFT" || kind || view LE || seq LE || digest[64].
pub type Envelope = [u8; ffi::PBFT_ENVELOPE_BYTES];

#[derive(Debug, Clone, PartialEq, Eq)]
pub struct Error {
    pub code: i32,
    pub message: String,
}

impl fmt::Display for Error {
    fn fmt(&self, f: &mut fmt::Formatter<'_>) -> fmt::Result {
        write!(f, "pbft-hip error {}: {}", self.code, self.message)
    }
}
impl std::error::Error for Error {}

pub type Result<T> = std::result::Result<T, Error>;

fn check(rc: c_int) -> Result<c_int> {
    if rc >= 0 {
        return Ok(rc);
    }
    let message = unsafe { CStr::from_ptr(ffi::pbft_last_error()) }.to_string_lossy().into_owned();
    Err(Error { code: rc, message })
}

/// Encode the signed envelope (the bytes every Prepare / Commit / PrePrepare signature covers).
pub fn envelope(kind: u8, view: u64, seq: u64, digest: &[u8; 64]) -> Envelope {
    let mut out = [0u8; ffi::PBFT_ENVELOPE_BYTES];
    unsafe { ffi::pbft_envelope(out.as_mut_ptr(), kind, view, seq, digest.as_ptr()) };
    out
}

/// Struct-of-arrays batch of one or more (view, seq) round windows.
#[derive(Clone, Default)]
pub struct SigBatch {
    pub r: Vec<[u8; 32]>,
    pub s: Vec<[u8; 32]>,
    pub key_idx: Vec<u16>,
    pub msg: Vec<Envelope>,
}

impl SigBatch {
    pub fn push(&mut self, key_idx: u16, envelope: Envelope, sig: &[u8; 64]) {
        let mut r = [0u8; 32];
        let mut s = [0u8; 32];
        r.copy_from_slice(&sig[..32]);
        s.copy_from_slice(&sig[32..]);
        self.r.push(r);
        self.s.push(s);
        self.key_idx.push(key_idx);
        self.msg.push(envelope);
    }
    pub fn len(&self) -> usize {
        self.r.len()
    }
    pub fn is_empty(&self) -> bool {
        self.r.is_empty()
    }
}

/// Votes form of a round batch: signature i signs `envelopes[env_idx[i]]` (a window's Prepares / Commits
/// all sign the same (kind, view, seq, digest) envelope), 70 bytes per signature over PCIe instead of 151.
#[derive(Clone, Default)]
pub struct VotesBatch {
    pub r: Vec<[u8; 32]>,
    pub s: Vec<[u8; 32]>,
    pub key_idx: Vec<u16>,
    pub env_idx: Vec<u32>,
    pub envelopes: Vec<Envelope>,
}

impl VotesBatch {
    pub fn len(&self) -> usize {
        self.r.len()
    }
    pub fn is_empty(&self) -> bool {
        self.r.is_empty()
    }
    /// Err(PBFT_EINVAL) unless `s`, `key_idx` and `env_idx` have one entry per signature (`r`).
    pub fn check_columns(&self) -> Result<()> {
        let n = self.r.len();
        if self.s.len() != n || self.key_idx.len() != n || self.env_idx.len() != n {
            return Err(Error { code: ffi::PBFT_EINVAL, message: "VotesBatch: column lengths differ".into() });
        }
        Ok(())
    }
    /// The per-signature form (every signature carrying its own envelope), for verifiers without a votes form.
    pub fn to_sig_batch(&self) -> Result<SigBatch> {
        self.check_columns()?;
        let mut b = SigBatch::default();
        for i in 0..self.len() {
            let e = self.envelopes.get(self.env_idx[i] as usize).copied().unwrap_or([0u8; ffi::PBFT_ENVELOPE_BYTES]);
            let mut sig = [0u8; 64];
            sig[..32].copy_from_slice(&self.r[i]);
            sig[32..].copy_from_slice(&self.s[i]);
            // an out-of-range envelope index is a 0 bit: an out-of-range key index gives the same
            let k = if (self.env_idx[i] as usize) < self.envelopes.len() { self.key_idx[i] } else { u16::MAX };
            b.push(k, e, &sig);
        }
        Ok(b)
    }
}

/// Accept bits, LSB-first in u64 words; bits past the batch length are 0.
#[derive(Clone, Debug, Default, PartialEq, Eq)]
pub struct Bitmap(pub Vec<u64>);

impl Bitmap {
    pub fn zeros(n: usize) -> Self {
        Bitmap(vec![0u64; (n + 63) / 64])
    }
    pub fn get(&self, i: usize) -> bool {
        (self.0[i / 64] >> (i % 64)) & 1 == 1
    }
    pub fn set(&mut self, i: usize) {
        self.0[i / 64] |= 1u64 << (i % 64);
    }
}

/// Per-envelope result of a votes batch (pbft_verify_votes_tally): which replicas have a valid vote under each
/// envelope, and how many.  What Pbft::prepared / committed_local (src/behavior.rs:177-182, :214-223) count.
#[derive(Clone, Debug, Default, PartialEq, Eq)]
pub struct Tally {
    /// `[n_env][words_per_env]`: bit (k % 64) of word k / 64 of envelope e's row = replica k voted validly for e.
    pub signers: Vec<u64>,
    /// Distinct valid signers per envelope.
    pub counts: Vec<u32>,
    pub words_per_env: usize,
}

impl Tally {
    /// At least `need` distinct replicas signed envelope `env` (2f for prepared, 2f + 1 for committed-local).
    pub fn has_quorum(&self, env: usize, need: u32) -> bool {
        self.counts.get(env).map_or(false, |&c| c >= need)
    }
    /// The replica indices with a valid vote under envelope `env`, ascending.
    pub fn signers_of(&self, env: usize) -> Vec<u16> {
        let mut out = Vec::new();
        if env >= self.counts.len() {
            return out;
        }
        let row = &self.signers[env * self.words_per_env..(env + 1) * self.words_per_env];
        for (w, &word) in row.iter().enumerate() {
            let mut m = word;
            while m != 0 {
                out.push((w * 64 + m.trailing_zeros() as usize) as u16);
                m &= m - 1;
            }
        }
        out
    }
}

/// Head of one decoded frame (ffi::pbft_frame_head): status, and view / seq / kind / signer of an OK frame.
pub type FrameHead = ffi::pbft_frame_head;

/// Result of `GpuVerifier::verify_frames_tally`: per frame the bitmap and the heads, per envelope -- in order of
/// first appearance in the stream -- its 85 bytes with its signer set and count (`tally`, indexed like `envelopes`).
#[derive(Clone, Debug)]
pub struct FramesTally {
    pub bitmap: Bitmap,
    pub heads: Vec<FrameHead>,
    /// The distinct envelopes kept: min(envelopes_found, env_cap) of them.
    pub envelopes: Vec<[u8; 85]>,
    pub tally: Tally,
    /// Distinct envelopes in the stream (may exceed env_cap).
    pub envelopes_found: u32,
    /// OK frames whose envelope did not fit env_cap: their votes are in no set.
    pub rows_lost: u32,
    /// Bytes of whole frames (an incomplete last frame stays with the caller).
    pub consumed: usize,
}

/// Head of one connection segment (ffi::pbft_seg_head): frames, bytes consumed, framing status.
pub type SegHead = ffi::pbft_seg_head;

/// Result of `GpuVerifier::verify_streams_tally`: `FramesTally` over the frames of every connection, numbered by
/// connection and then by position, plus one head per connection.
#[derive(Clone, Debug)]
pub struct StreamsTally {
    pub bitmap: Bitmap,
    pub heads: Vec<FrameHead>,
    pub envelopes: Vec<[u8; 85]>,
    pub tally: Tally,
    pub envelopes_found: u32,
    pub rows_lost: u32,
    /// Per connection: `first` (number of its first frame), `n_frames`, `consumed` and `status`.
    pub segments: Vec<SegHead>,
    /// Whole frames in all connections (may exceed frame_cap).
    pub frames_found: u32,
    /// Frames numbered >= frame_cap: not decoded, not verified.
    pub frames_lost: u32,
}

/// Handle of one submitted batch.
#[derive(Debug, PartialEq, Eq)]
pub struct Ticket(pub u64);

/// the verifier behind the round batcher.
pub trait BatchVerifier {
    /// Install the replica key set (libp2p identity keys of network.json's nodes);
    /// returns key_ok per key (false: bad encoding or small order -> every signature under it is 0).
    fn set_keys(&mut self, keys: &[[u8; 32]]) -> Result<Vec<bool>>;
    /// Non-blocking: enqueue the batch.
    fn submit(&mut self, batch: SigBatch) -> Result<Ticket>;
    /// Ok(Some(bitmap)) once the batch is verified, Ok(None) while it runs.
    fn poll(&mut self, ticket: &Ticket) -> Result<Option<Bitmap>>;
    /// Blocking verify.
    fn verify(&mut self, batch: SigBatch) -> Result<Bitmap> {
        let t = self.submit(batch)?;
        loop {
            if let Some(bm) = self.poll(&t)? {
                return Ok(bm);
            }
            std::thread::yield_now();
        }
    }
}

/// One HIP context (one MI355X).  Not `Sync`: one per thread; `try_clone` for more streams.
pub struct GpuVerifier {
    ctx: *mut ffi::pbft_ctx,
    // the library copies pageable batches into its pinned staging before the DMA, so only the output
    // bitmap (written when the batch completes) has to outlive the call
    inflight: Option<(u64, Bitmap)>,
    next: u64,
}

unsafe impl Send for GpuVerifier {}

impl GpuVerifier {
    pub fn new(device: i32) -> Result<Self> {
        let mut ctx = ptr::null_mut();
        check(unsafe { ffi::pbft_verify_ctx_create(device, &mut ctx) })?;
        Ok(GpuVerifier { ctx, inflight: None, next: 0 })
    }
    /// Non-blocking votes-form submit (pbft_verify_votes_async); complete it with `poll`.
    pub fn submit_votes(&mut self, batch: &VotesBatch) -> Result<Ticket> {
        if self.inflight.is_some() {
            return Err(Error { code: ffi::PBFT_EBUSY, message: "one batch in flight per context".into() });
        }
        batch.check_columns()?; // the C side reads n entries of every column
        let n = batch.len();
        let mut out = Bitmap::zeros(n);
        check(unsafe {
            ffi::pbft_verify_votes_async(self.ctx, batch.r.as_ptr() as *const u8, batch.s.as_ptr() as *const u8,
                                         batch.key_idx.as_ptr(), batch.env_idx.as_ptr(),
                                         batch.envelopes.as_ptr() as *const u8, batch.envelopes.len() as u32,
                                         n as u64, out.0.as_mut_ptr())
        })?;
        self.next += 1;
        self.inflight = Some((self.next, out));
        Ok(Ticket(self.next))
    }
    /// Blocking votes-form verify with the per-envelope tally of its result over the installed keys
    /// (pbft_verify_votes_tally): the bitmap `submit_votes` would give, and who signed each envelope.
    pub fn verify_votes_tally(&mut self, batch: &VotesBatch) -> Result<(Bitmap, Tally)> {
        if self.inflight.is_some() {
            return Err(Error { code: ffi::PBFT_EBUSY, message: "one batch in flight per context".into() });
        }
        batch.check_columns()?;
        let (mut wb, mut wa, mut n_keys) = (0u32, 0u32, 0u32);
        check(unsafe { ffi::pbft_verify_ctx_info(self.ctx, &mut wb, &mut wa, &mut n_keys) })?;
        let n = batch.len();
        let n_env = batch.envelopes.len();
        let words_per_env = (n_keys as usize + 63) / 64;
        let mut out = Bitmap::zeros(n);
        let mut tally = Tally { signers: vec![0u64; n_env * words_per_env], counts: vec![0u32; n_env], words_per_env };
        check(unsafe {
            ffi::pbft_verify_votes_tally(self.ctx, batch.r.as_ptr() as *const u8, batch.s.as_ptr() as *const u8,
                                         batch.key_idx.as_ptr(), batch.env_idx.as_ptr(),
                                         batch.envelopes.as_ptr() as *const u8, n_env as u32, n as u64,
                                         out.0.as_mut_ptr(), tally.signers.as_mut_ptr(), tally.counts.as_mut_ptr())
        })?;
        Ok((out, tally))
    }
    /// The whole frames of one connection's byte stream (UviBytes + serde_json, what `upgrade_inbound` reads)
    /// decoded on the GPU and verified (pbft_wire_frame_index + pbft_verify_frames).  `peer`: the connection's
    /// authenticated replica index -- a vote naming another replica is PBFT_WIRE_ESIGNER.  Returns the bitmap (bit f:
    /// frame f is a signed message whose signature verifies), one head per frame with the status
    /// pbft_wire_decode_votes would give it, and the bytes consumed (an incomplete last frame stays with the caller).
    pub fn verify_frames(&mut self, stream: &[u8], peer: Option<u16>,
                         n_replicas: u32) -> Result<(Bitmap, Vec<FrameHead>, usize)> {
        if self.inflight.is_some() {
            return Err(Error { code: ffi::PBFT_EBUSY, message: "one batch in flight per context".into() });
        }
        let cap = stream.len(); // a frame is at least its one varint byte
        let (mut off, mut flen) = (vec![0u64; cap], vec![0u32; cap]);
        let (mut n, mut used) = (0u64, 0u64);
        check(unsafe {
            ffi::pbft_wire_frame_index(stream.as_ptr(), stream.len(), cap as u64, off.as_mut_ptr(), flen.as_mut_ptr(),
                                       &mut n, &mut used)
        })?;
        let n = n as usize;
        let peers = peer.map(|p| vec![p; n]);
        let mut out = Bitmap::zeros(n);
        let mut heads = vec![FrameHead::default(); n];
        check(unsafe {
            ffi::pbft_verify_frames(self.ctx, stream.as_ptr(), stream.len() as u64, off.as_ptr(), flen.as_ptr(),
                                    peers.as_ref().map_or(ptr::null(), |p| p.as_ptr()), n_replicas, n as u64,
                                    out.0.as_mut_ptr(), heads.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok((out, heads, used as usize))
    }
    /// `verify_frames` with the frames grouped by envelope and tallied on the GPU (pbft_verify_frames_tally): from
    /// the bytes a socket delivered to "these envelopes have 2f / 2f + 1 distinct valid signers" in one call.  Nothing
    /// per vote comes back but the heads and the bitmap; per envelope come its 85 bytes, its signer set and its count.
    /// `env_cap`: room for that many distinct envelopes -- later ones lose their votes (`rows_lost`), none is miscounted.
    pub fn verify_frames_tally(&mut self, stream: &[u8], peer: Option<u16>, n_replicas: u32,
                               env_cap: u32) -> Result<FramesTally> {
        if self.inflight.is_some() {
            return Err(Error { code: ffi::PBFT_EBUSY, message: "one batch in flight per context".into() });
        }
        let (mut wb, mut wa, mut n_keys) = (0u32, 0u32, 0u32);
        check(unsafe { ffi::pbft_verify_ctx_info(self.ctx, &mut wb, &mut wa, &mut n_keys) })?;
        let cap = stream.len(); // a frame is at least its one varint byte
        let (mut off, mut flen) = (vec![0u64; cap], vec![0u32; cap]);
        let (mut n, mut used) = (0u64, 0u64);
        check(unsafe {
            ffi::pbft_wire_frame_index(stream.as_ptr(), stream.len(), cap as u64, off.as_mut_ptr(), flen.as_mut_ptr(),
                                       &mut n, &mut used)
        })?;
        let n = n as usize;
        let peers = peer.map(|p| vec![p; n]);
        let words_per_env = (n_keys as usize + 63) / 64;
        let cap_env = env_cap as usize;
        let mut bitmap = Bitmap::zeros(n);
        let mut heads = vec![FrameHead::default(); n];
        let mut envelopes = vec![[0u8; 85]; cap_env];
        let mut n_env = [0u32; 2];
        let mut tally = Tally { signers: vec![0u64; cap_env * words_per_env], counts: vec![0u32; cap_env],
                                words_per_env };
        check(unsafe {
            ffi::pbft_verify_frames_tally(self.ctx, stream.as_ptr(), stream.len() as u64, off.as_ptr(), flen.as_ptr(),
                                          peers.as_ref().map_or(ptr::null(), |p| p.as_ptr()), n_replicas, n as u64,
                                          env_cap, bitmap.0.as_mut_ptr(), heads.as_mut_ptr(), ptr::null_mut(),
                                          envelopes.as_mut_ptr() as *mut u8, n_env.as_mut_ptr(),
                                          tally.signers.as_mut_ptr(), tally.counts.as_mut_ptr())
        })?;
        let kept = (n_env[0] as usize).min(cap_env);
        envelopes.truncate(kept);
        tally.signers.truncate(kept * words_per_env);
        tally.counts.truncate(kept);
        Ok(FramesTally { bitmap, heads, envelopes, tally, envelopes_found: n_env[0], rows_lost: n_env[1],
                         consumed: used as usize })
    }
    /// `verify_frames_tally` of what `upgrade_inbound` has: one buffer of bytes per authenticated connection, each
    /// with its peer's replica index (pbft_verify_streams_tally).  The buffers are laid end to end (each at a 16-byte
    /// boundary) into one stream; the varint walk, the decode, the grouping, the verify and the tally all run on the
    /// GPU.  Frames are numbered by connection, then by position.  `frame_cap`: room for that many frames -- later
    /// ones are not verified (`frames_lost`).  `segments[i]`: what connection i consumed, how many frames it had and
    /// whether its framing broke (status PBFT_SEG_EFRAMING at `consumed`: close that connection).
    pub fn verify_streams_tally(&mut self, conns: &[(&[u8], u16)], n_replicas: u32, frame_cap: usize,
                                env_cap: u32) -> Result<StreamsTally> {
        if self.inflight.is_some() {
            return Err(Error { code: ffi::PBFT_EBUSY, message: "one batch in flight per context".into() });
        }
        let (mut wb, mut wa, mut n_keys) = (0u32, 0u32, 0u32);
        check(unsafe { ffi::pbft_verify_ctx_info(self.ctx, &mut wb, &mut wa, &mut n_keys) })?;
        let mut stream: Vec<u8> = Vec::new();
        let (mut seg_off, mut seg_len, mut seg_peer) = (Vec::new(), Vec::new(), Vec::new());
        for (bytes, peer) in conns {
            stream.resize((stream.len() + 15) & !15, 0);
            seg_off.push(stream.len() as u64);
            seg_len.push(bytes.len() as u64);
            seg_peer.push(*peer);
            stream.extend_from_slice(bytes);
        }
        let words_per_env = (n_keys as usize + 63) / 64;
        let cap_env = env_cap as usize;
        let mut bitmap = Bitmap::zeros(frame_cap);
        let mut heads = vec![FrameHead::default(); frame_cap];
        let mut envelopes = vec![[0u8; 85]; cap_env];
        let mut n_env = [0u32; 2];
        let mut n_frames = [0u32; 2];
        let mut segments = vec![SegHead::default(); conns.len()];
        let mut tally = Tally { signers: vec![0u64; cap_env * words_per_env], counts: vec![0u32; cap_env],
                                words_per_env };
        check(unsafe {
            ffi::pbft_verify_streams_tally(self.ctx, stream.as_ptr(), stream.len() as u64, seg_off.as_ptr(),
                                           seg_len.as_ptr(), seg_peer.as_ptr(), conns.len() as u32, n_replicas,
                                           frame_cap as u64, env_cap, bitmap.0.as_mut_ptr(), heads.as_mut_ptr(),
                                           ptr::null_mut(), envelopes.as_mut_ptr() as *mut u8, n_env.as_mut_ptr(),
                                           tally.signers.as_mut_ptr(), tally.counts.as_mut_ptr(),
                                           segments.as_mut_ptr(), n_frames.as_mut_ptr(), ptr::null_mut(),
                                           ptr::null_mut())
        })?;
        let n = (n_frames[0] as usize).min(frame_cap);
        heads.truncate(n);
        bitmap.0.truncate((n + 63) / 64);
        let kept = (n_env[0] as usize).min(cap_env);
        envelopes.truncate(kept);
        tally.signers.truncate(kept * words_per_env);
        tally.counts.truncate(kept);
        Ok(StreamsTally { bitmap, heads, envelopes, tally, envelopes_found: n_env[0], rows_lost: n_env[1], segments,
                          frames_found: n_frames[0], frames_lost: n_frames[1] })
    }
    /// Another context on the same GPU sharing this one's tables (own HIP stream).
    pub fn try_clone(&self) -> Result<Self> {
        let mut ctx = ptr::null_mut();
        check(unsafe { ffi::pbft_verify_ctx_clone(self.ctx, &mut ctx) })?;
        Ok(GpuVerifier { ctx, inflight: None, next: 0 })
    }
    /// Replace keys `idx[i]` of the installed set by `keys[i]` in place (only their tables are rebuilt): a peer
    /// admitted later (Pbft::add_peer, src/behavior.rs:45-61) fills the slot its replica id reserves.
    /// Returns key_ok of the new keys.
    pub fn update_keys(&mut self, idx: &[u32], keys: &[[u8; 32]]) -> Result<Vec<bool>> {
        if idx.len() != keys.len() {
            return Err(Error { code: ffi::PBFT_EINVAL, message: "update_keys: idx and keys lengths differ".into() });
        }
        let mut ok = vec![0u8; keys.len()];
        check(unsafe {
            ffi::pbft_verify_update_keys(self.ctx, idx.as_ptr(), keys.as_ptr() as *const u8, keys.len() as u32,
                                         ok.as_mut_ptr())
        })?;
        Ok(ok.into_iter().map(|b| b == 1).collect())
    }
    /// Verify `(public key, envelope, signature)` triples under keys that are not installed: no `set_keys` first,
    /// and an installed set is neither read nor disturbed (pbft_verify_batch_keys).  A key that does not decode
    /// or is of small order is bit 0, like a bad signature.  Blocking.
    pub fn verify_with_keys(&mut self, items: &[([u8; 32], Envelope, [u8; 64])]) -> Result<Bitmap> {
        let n = items.len();
        let mut r = Vec::with_capacity(32 * n);
        let mut s = Vec::with_capacity(32 * n);
        let mut a = Vec::with_capacity(32 * n);
        let mut msg = Vec::with_capacity(ffi::PBFT_ENVELOPE_BYTES * n);
        for (key, env, sig) in items {
            r.extend_from_slice(&sig[..32]);
            s.extend_from_slice(&sig[32..]);
            a.extend_from_slice(key);
            msg.extend_from_slice(env);
        }
        let mut out = Bitmap::zeros(n);
        check(unsafe {
            ffi::pbft_verify_batch_keys(self.ctx, r.as_ptr(), s.as_ptr(), a.as_ptr(), msg.as_ptr(),
                                        ffi::PBFT_ENVELOPE_BYTES as u32, ffi::PBFT_ENVELOPE_BYTES as u32, n as u64,
                                        out.0.as_mut_ptr())
        })?;
        Ok(out)
    }
    /// Where the last set_keys / update_keys spent its time.
    pub fn key_stats(&self) -> ffi::pbft_key_stats {
        let mut s = ffi::pbft_key_stats::default();
        unsafe { ffi::pbft_verify_key_stats(self.ctx, &mut s) };
        s
    }
    pub fn set_option(&mut self, option: i32, value: u64) -> Result<()> {
        check(unsafe { ffi::pbft_verify_set_option(self.ctx, option, value) }).map(|_| ())
    }
    /// Blake2b-512 request digests (src/message.rs:209-212), one per item.
    pub fn blake2b512(&mut self, items: &[&[u8]]) -> Result<Vec<[u8; 64]>> {
        let (data, offs, lens) = pack(items);
        let mut out = vec![[0u8; 64]; items.len()];
        check(unsafe {
            ffi::pbft_digest_blake2b512(self.ctx, data.as_ptr(), offs.as_ptr(), lens.as_ptr(), items.len() as u64,
                                        out.as_mut_ptr() as *mut u8)
        })?;
        Ok(out)
    }
    /// RFC 8032 signatures of this replica's own envelopes.
    pub fn sign(&mut self, seed: &[u8; 32], msgs: &[Envelope]) -> Result<Vec<[u8; 64]>> {
        let n = msgs.len();
        let idx = vec![0u16; n];
        let mut r = vec![[0u8; 32]; n];
        let mut s = vec![[0u8; 32]; n];
        check(unsafe {
            ffi::pbft_sign_batch(self.ctx, seed.as_ptr(), 1, idx.as_ptr(), msgs.as_ptr() as *const u8,
                                 ffi::PBFT_ENVELOPE_BYTES as u32, ffi::PBFT_ENVELOPE_BYTES as u32, n as u64,
                                 r.as_mut_ptr() as *mut u8, s.as_mut_ptr() as *mut u8, ptr::null_mut())
        })?;
        Ok(r.iter().zip(s.iter()).map(|(r, s)| {
            let mut sig = [0u8; 64];
            sig[..32].copy_from_slice(r);
            sig[32..].copy_from_slice(s);
            sig
        }).collect())
    }
    /// Install this context's signing identity (pbft_sign_set_seed): the seed is expanded once on the device;
    /// `replica` is the index the frames carry.  Returns the public key.  `None` clears it.
    pub fn set_signing_seed(&mut self, seed: Option<&[u8; 32]>, replica: u32) -> Result<[u8; 32]> {
        let mut public = [0u8; 32];
        check(unsafe {
            ffi::pbft_sign_set_seed(self.ctx, seed.map_or(ptr::null(), |s| s.as_ptr()), replica, public.as_mut_ptr())
        })?;
        Ok(public)
    }
    /// The envelopes signed with the installed seed and written as UviBytes/JSON vote frames on the GPU
    /// (pbft_sign_votes_frames): (stream, frame offsets [n + 1], signatures).
    pub fn sign_votes_frames(&mut self, envelopes: &[Envelope]) -> Result<(Vec<u8>, Vec<u64>, Vec<[u8; 64]>)> {
        let n = envelopes.len();
        let env = envelopes.as_ptr() as *const u8;
        let stride = ffi::PBFT_ENVELOPE_BYTES as u32;
        let mut len = 0usize;
        unsafe {
            // the size query: PBFT_EINVAL with the length needed, unless there is nothing to write
            ffi::pbft_sign_votes_frames(self.ctx, env, stride, n as u64, ptr::null_mut(), 0, &mut len, ptr::null_mut(),
                                        ptr::null_mut());
        }
        let mut out = vec![0u8; len];
        let mut off = vec![0u64; n + 1];
        let mut sigs = vec![[0u8; 64]; n];
        check(unsafe {
            ffi::pbft_sign_votes_frames(self.ctx, env, stride, n as u64, out.as_mut_ptr(), out.len(), &mut len,
                                        off.as_mut_ptr(), sigs.as_mut_ptr() as *mut u8)
        })?;
        out.truncate(len);
        Ok((out, off, sigs))
    }
    /// The primary's side of a round (pbft_sign_preprepares_frames): the requests hashed, their PrePrepares with
    /// sequence numbers first_seq, first_seq + 1, ... signed with the installed seed and written as UviBytes/JSON
    /// frames; requests that are not of the canonical form are completed on the host.
    pub fn sign_preprepares_frames(&mut self, view: u64, first_seq: u64, requests: &[ClientRequest]) -> Result<Proposal> {
        let p = PackedRequests::new(requests);
        let n = requests.len();
        let mut len = 0usize;
        unsafe {
            // the size query: PBFT_EINVAL with the length needed, unless there is nothing to write
            ffi::pbft_sign_preprepares_frames(self.ctx, p.ops.as_ptr(), p.ops_bytes, p.off.as_ptr(), p.len.as_ptr(),
                                              p.ts.as_ptr(), p.clients.as_ptr() as *const c_char, view, first_seq,
                                              n as u64, ptr::null_mut(), 0, &mut len, ptr::null_mut(), ptr::null_mut(),
                                              ptr::null_mut(), ptr::null_mut());
        }
        let mut out = Proposal { stream: vec![0u8; len], frame_off: vec![0u64; n + 1], digests: vec![[0u8; 64]; n],
                                 sigs: vec![[0u8; 64]; n], status: vec![0u8; n] };
        check(unsafe {
            ffi::pbft_sign_preprepares_frames(self.ctx, p.ops.as_ptr(), p.ops_bytes, p.off.as_ptr(), p.len.as_ptr(),
                                              p.ts.as_ptr(), p.clients.as_ptr() as *const c_char, view, first_seq,
                                              n as u64, out.stream.as_mut_ptr(), out.stream.len(), &mut len,
                                              out.frame_off.as_mut_ptr(), out.digests.as_mut_ptr() as *mut u8,
                                              out.sigs.as_mut_ptr() as *mut u8, out.status.as_mut_ptr())
        })?;
        out.stream.truncate(len);
        Ok(out)
    }
    /// The client's side (pbft_accept_replies): signed replies as they arrived, one text each, `client_idx[i]` naming
    /// the entry of `clients` reply i was sent to -> one certificate per distinct (view, timestamp, client, result),
    /// `accepted` once `need` (f + 1) distinct installed replicas signed it; `texts[cert.first]` holds the result.
    /// Texts that are not canonical are settled by the host's serde-exact reader, so no status is PBFT_ACCEPT_EDEFER.
    pub fn accept_replies(&mut self, texts: &[&[u8]], client_idx: &[u32], clients: &[&str], need: u32,
                          env_cap: u32) -> Result<Accepted> {
        if self.inflight.is_some() {
            return Err(Error { code: ffi::PBFT_EBUSY, message: "one batch in flight per context".into() });
        }
        if client_idx.len() != texts.len() {
            return Err(Error { code: ffi::PBFT_EINVAL, message: "one client index per reply".into() });
        }
        let (mut wb, mut wa, mut n_keys) = (0u32, 0u32, 0u32);
        check(unsafe { ffi::pbft_verify_ctx_info(self.ctx, &mut wb, &mut wa, &mut n_keys) })?;
        let n = texts.len();
        let (mut buf, mut off, mut len) = (Vec::new(), Vec::with_capacity(n), Vec::with_capacity(n));
        for t in texts {
            off.push(buf.len() as u64);
            len.push(t.len() as u32);
            buf.extend_from_slice(t);
        }
        let mut fields = vec![0u8; 64 * clients.len()];
        for (i, c) in clients.iter().enumerate() {
            let b = c.as_bytes();
            let k = b.len().min(64);
            fields[64 * i..64 * i + k].copy_from_slice(&b[..k]);
        }
        let words_per_env = (n_keys as usize + 63) / 64;
        let cap_env = env_cap as usize;
        let mut bitmap = Bitmap::zeros(n);
        let mut heads = vec![ffi::pbft_accept_head::default(); n];
        let mut envelopes = vec![[0u8; 85]; cap_env];
        let mut n_env = [0u32; 2];
        let mut tally = Tally { signers: vec![0u64; cap_env * words_per_env], counts: vec![0u32; cap_env],
                                words_per_env };
        let mut certs = vec![ffi::pbft_accept_cert::default(); cap_env];
        check(unsafe {
            ffi::pbft_accept_replies(self.ctx, buf.as_ptr(), buf.len() as u64, off.as_ptr(), len.as_ptr(),
                                     client_idx.as_ptr(), fields.as_ptr() as *const c_char, clients.len() as u32,
                                     n as u64, need, env_cap, bitmap.0.as_mut_ptr(), heads.as_mut_ptr(),
                                     ptr::null_mut(), envelopes.as_mut_ptr() as *mut u8, n_env.as_mut_ptr(),
                                     tally.signers.as_mut_ptr(), tally.counts.as_mut_ptr(), certs.as_mut_ptr())
        })?;
        let kept = (n_env[0] as usize).min(cap_env);
        envelopes.truncate(kept);
        tally.signers.truncate(kept * words_per_env);
        tally.counts.truncate(kept);
        certs.truncate(kept);
        Ok(Accepted { bitmap, heads, envelopes, tally, certs, envelopes_found: n_env[0], rows_lost: n_env[1] })
    }
    pub fn raw(&self) -> *mut ffi::pbft_ctx {
        self.ctx
    }
}

/// What accept_replies returns: per reply its head and verify bit; per envelope found (at most env_cap) the envelope,
/// its signer set and count, and its certificate.
#[derive(Clone, Debug)]
pub struct Accepted {
    pub bitmap: Bitmap,
    pub heads: Vec<ffi::pbft_accept_head>,
    pub envelopes: Vec<Envelope>,
    pub tally: Tally,
    pub certs: Vec<ffi::pbft_accept_cert>,
    pub envelopes_found: u32,
    pub rows_lost: u32,
}

/// One client request as the primary receives it (the reference's ClientRequest, src/message.rs:174-179).
#[derive(Clone, Copy, Debug)]
pub struct ClientRequest<'a> {
    pub operation: &'a [u8],
    pub timestamp: u64,
    /// The client's address as serde writes it ("127.0.0.1:8080"); at most 64 bytes are used.
    pub client: &'a str,
}

/// What sign_preprepares_frames returns: the frames, frame i at [frame_off[i], frame_off[i + 1]), and per request the
/// operation's Blake2b-512 digest, R || S over the PrePrepare's envelope and PBFT_PROPOSE_OK / _GENERAL.
#[derive(Clone, Debug, Default)]
pub struct Proposal {
    pub stream: Vec<u8>,
    pub frame_off: Vec<u64>,
    pub digests: Vec<[u8; 64]>,
    pub sigs: Vec<[u8; 64]>,
    pub status: Vec<u8>,
}

// The arrays the proposal entry points take: operations back to back (padded to 16 bytes), 64-byte client fields.
struct PackedRequests {
    ops: Vec<u8>,
    ops_bytes: u64,
    off: Vec<u64>,
    len: Vec<u32>,
    ts: Vec<u64>,
    clients: Vec<[u8; 64]>,
}

impl PackedRequests {
    fn new(requests: &[ClientRequest]) -> Self {
        let mut p = PackedRequests { ops: Vec::new(), ops_bytes: 0, off: Vec::new(), len: Vec::new(), ts: Vec::new(),
                                     clients: Vec::new() };
        for r in requests {
            p.off.push(p.ops.len() as u64);
            p.len.push(r.operation.len() as u32);
            p.ops.extend_from_slice(r.operation);
            p.ts.push(r.timestamp);
            let mut c = [0u8; 64];
            let b = r.client.as_bytes();
            let k = b.len().min(64);
            c[..k].copy_from_slice(&b[..k]);
            p.clients.push(c);
        }
        p.ops_bytes = p.ops.len() as u64;
        let padded = (p.ops.len() + 16) / 16 * 16;
        p.ops.resize(padded, 0);
        p
    }
}

fn pack(items: &[&[u8]]) -> (Vec<u8>, Vec<u64>, Vec<u32>) {
    let mut data = Vec::new();
    let mut offs = Vec::with_capacity(items.len());
    let mut lens = Vec::with_capacity(items.len());
    for it in items {
        offs.push(data.len() as u64);
        lens.push(it.len() as u32);
        data.extend_from_slice(it);
    }
    data.extend_from_slice(&[0u8; 16]); // the digest kernels read aligned dwords past each item
    (data, offs, lens)
}

impl BatchVerifier for GpuVerifier {
    fn set_keys(&mut self, keys: &[[u8; 32]]) -> Result<Vec<bool>> {
        let mut ok = vec![0u8; keys.len()];
        check(unsafe {
            ffi::pbft_verify_set_keys(self.ctx, keys.as_ptr() as *const u8, keys.len() as u32, ok.as_mut_ptr())
        })?;
        Ok(ok.into_iter().map(|b| b == 1).collect())
    }
    fn submit(&mut self, batch: SigBatch) -> Result<Ticket> {
        if self.inflight.is_some() {
            return Err(Error { code: ffi::PBFT_EBUSY, message: "one batch in flight per context".into() });
        }
        let n = batch.len();
        let mut out = Bitmap::zeros(n);
        // pageable Vec buffers: copied into the context's pinned staging by the call, then DMA'd asynchronously
        check(unsafe {
            ffi::pbft_verify_batch_async(self.ctx, batch.r.as_ptr() as *const u8, batch.s.as_ptr() as *const u8,
                                         batch.key_idx.as_ptr(), batch.msg.as_ptr() as *const u8,
                                         ffi::PBFT_ENVELOPE_BYTES as u32, ffi::PBFT_ENVELOPE_BYTES as u32,
                                         n as u64, out.0.as_mut_ptr())
        })?;
        self.next += 1;
        self.inflight = Some((self.next, out));
        Ok(Ticket(self.next))
    }
    fn poll(&mut self, ticket: &Ticket) -> Result<Option<Bitmap>> {
        match &self.inflight {
            Some((id, _)) if *id == ticket.0 => {}
            _ => return Err(Error { code: ffi::PBFT_EINVAL, message: "unknown ticket".into() }),
        }
        match check(unsafe { ffi::pbft_verify_poll(self.ctx) }) {
            Ok(1) => Ok(Some(self.inflight.take().unwrap().1)),
            Ok(_) => Ok(None),
            Err(e) => {
                self.inflight = None; // the library dropped the failed batch
                Err(e)
            }
        }
    }
}

impl Drop for GpuVerifier {
    fn drop(&mut self) {
        unsafe {
            if self.inflight.is_some() {
                ffi::pbft_verify_wait(self.ctx);
            }
            ffi::pbft_verify_ctx_destroy(self.ctx);
        }
    }
}

/// The reference's CPU crypto path: ed25519-dalek 1.0.1 `verify_strict`, one signature at a time.
#[cfg(feature = "cpu")]
pub struct CpuVerifier {
    keys: Vec<Option<ed25519_dalek::PublicKey>>,
    done: Option<(u64, Bitmap)>,
    next: u64,
}

#[cfg(feature = "cpu")]
impl CpuVerifier {
    pub fn new() -> Self {
        CpuVerifier { keys: Vec::new(), done: None, next: 0 }
    }
}

#[cfg(feature = "cpu")]
impl BatchVerifier for CpuVerifier {
    fn set_keys(&mut self, keys: &[[u8; 32]]) -> Result<Vec<bool>> {
        // libp2p decodes the identity key once per peer (PublicKey::from_bytes = decompress);
        // verify_strict additionally rejects a small-order A at every verification
        self.keys = keys.iter().map(|k| ed25519_dalek::PublicKey::from_bytes(k).ok()).collect();
        Ok(self.keys.iter().map(|k| k.is_some()).collect())
    }
    fn submit(&mut self, batch: SigBatch) -> Result<Ticket> {
        use std::convert::TryFrom;
        let mut bm = Bitmap::zeros(batch.len());
        for i in 0..batch.len() {
            let mut sig = [0u8; 64];
            sig[..32].copy_from_slice(&batch.r[i]);
            sig[32..].copy_from_slice(&batch.s[i]);
            let ok = match (self.keys.get(batch.key_idx[i] as usize), ed25519_dalek::Signature::try_from(&sig[..])) {
                (Some(Some(pk)), Ok(sig)) => pk.verify_strict(&batch.msg[i], &sig).is_ok(),
                _ => false,
            };
            if ok {
                bm.set(i);
            }
        }
        self.next += 1;
        self.done = Some((self.next, bm));
        Ok(Ticket(self.next))
    }
    fn poll(&mut self, ticket: &Ticket) -> Result<Option<Bitmap>> {
        match self.done.take() {
            Some((id, bm)) if id == ticket.0 => Ok(Some(bm)),
            other => {
                self.done = other;
                Err(Error { code: ffi::PBFT_EINVAL, message: "unknown ticket".into() })
            }
        }
    }
}

/// libp2p PeerId (38 bytes: 00 24 08 01 12 20 || A) -> the Ed25519 key A.
pub fn key_from_peer_id(peer_id: &[u8]) -> Result<[u8; 32]> {
    let mut a = [0u8; 32];
    check(unsafe { ffi::pbft_key_from_peer_id(peer_id.as_ptr(), peer_id.len(), a.as_mut_ptr()) })?;
    Ok(a)
}

/// One frame body against the canonical signed-PrePrepare rule, on the host (pbft_wire_decode_preprepare): `Some(head)`
/// with the fields, where the operation lies in `body` and its Blake2b-512, or `None`: the general parser decides.
pub fn decode_preprepare(body: &[u8]) -> Result<Option<ffi::pbft_pp_head>> {
    let mut h = std::mem::MaybeUninit::<ffi::pbft_pp_head>::zeroed();
    check(unsafe { ffi::pbft_wire_decode_preprepare(body.as_ptr(), body.len(), h.as_mut_ptr()) })?;
    let h = unsafe { h.assume_init() };
    Ok(if h.status == ffi::PBFT_PP_OK { Some(h) } else { None })
}

/// Round events reported by [`Replica::flush`].
#[derive(Clone, Copy, Debug, PartialEq, Eq)]
pub enum RoundEvent {
    /// The PrePrepare's signature verified: multicast this replica's Prepare.
    PrePrepared { view: u64, seq: u64 },
    /// prepared(m, v, n): 2f matching Prepares from distinct backups: multicast the Commit.
    Prepared { view: u64, seq: u64 },
    /// committed-local: 2f+1 matching Commits: execute and reply to the client.
    CommittedLocal { view: u64, seq: u64 },
}

/// The round batcher + quorum state machine of one replica (include/pbft_replica.h).  It borrows the
/// `GpuVerifier` whose context it submits to (`'a`): the context must outlive the replica, whose Drop may
/// still wait on a batch in flight there.
pub struct Replica<'a> {
    raw: *mut ffi::pbft_replica,
    // a Rust BatchVerifier installed as the replica's asynchronous votes verifier (None: the GPU context)
    verifier: Option<Box<Backend>>,
    // event buffer reused by every flush_poll / flush (the event loop polls ~1,500 times per 2^20 round)
    events: Vec<ffi::pbft_round_event>,
    _gpu: PhantomData<&'a GpuVerifier>,
}

// A BatchVerifier behind the replica's submit / poll callbacks (pbft_replica_set_votes_verifier).
struct Backend {
    v: Box<dyn BatchVerifier>,
    pending: Option<(Ticket, *mut u64, usize)>,
}

extern "C" fn votes_submit_trampoline(user: *mut c_void, sig: *const u8, key_idx: *const u16,
                                      env_idx: *const u32, envelopes: *const u8, n_env: u32, n: u64,
                                      bitmap_out: *mut u64) -> c_int {
    let b = unsafe { &mut *(user as *mut Backend) };
    let n = n as usize;
    let mut vb = VotesBatch::default();
    unsafe {
        for row in std::slice::from_raw_parts(sig as *const [u8; 64], n) {
            let mut r = [0u8; 32];
            let mut s = [0u8; 32];
            r.copy_from_slice(&row[..32]);
            s.copy_from_slice(&row[32..]);
            vb.r.push(r);
            vb.s.push(s);
        }
        vb.key_idx.extend_from_slice(std::slice::from_raw_parts(key_idx, n));
        vb.env_idx.extend_from_slice(std::slice::from_raw_parts(env_idx, n));
        vb.envelopes.extend_from_slice(std::slice::from_raw_parts(envelopes as *const Envelope, n_env as usize));
    }
    let batch = match vb.to_sig_batch() {
        Ok(batch) => batch,
        Err(e) => return e.code,
    };
    match b.v.submit(batch) {
        Ok(t) => {
            b.pending = Some((t, bitmap_out, (n + 63) / 64));
            0
        }
        Err(e) => e.code,
    }
}

extern "C" fn votes_poll_trampoline(user: *mut c_void) -> c_int {
    let b = unsafe { &mut *(user as *mut Backend) };
    let (t, out, words) = match b.pending.take() {
        Some(p) => p,
        None => return 1,
    };
    match b.v.poll(&t) {
        Ok(Some(bm)) => {
            unsafe { ptr::copy_nonoverlapping(bm.0.as_ptr(), out, words.min(bm.0.len())) };
            1
        }
        Ok(None) => {
            b.pending = Some((t, out, words));
            0
        }
        Err(e) => e.code,
    }
}

fn round_events(ev: &[ffi::pbft_round_event]) -> Vec<RoundEvent> {
    ev.iter().filter_map(|e| match e.kind {
        ffi::PBFT_EVENT_PRE_PREPARED => Some(RoundEvent::PrePrepared { view: e.view, seq: e.seq }),
        ffi::PBFT_EVENT_PREPARED => Some(RoundEvent::Prepared { view: e.view, seq: e.seq }),
        ffi::PBFT_EVENT_COMMITTED_LOCAL => Some(RoundEvent::CommittedLocal { view: e.view, seq: e.seq }),
        _ => None,
    }).collect()
}

impl<'a> Replica<'a> {
    /// `gpu`: the context whose key set is `keys` (pbft_verify_set_keys); replica ids are
    /// positions in `keys` (network.json's "nodes" order); f = (n - 1) / 3.
    pub fn new(gpu: Option<&'a GpuVerifier>, self_id: u32, keys: &[[u8; 32]]) -> Result<Self> {
        let mut raw = ptr::null_mut();
        let ctx = gpu.map(|g| g.raw()).unwrap_or(ptr::null_mut());
        check(unsafe {
            ffi::pbft_replica_create(ctx, keys.len() as u32, self_id, keys.as_ptr() as *const u8, &mut raw)
        })?;
        Ok(Replica { raw, verifier: None, events: vec![ffi::pbft_round_event::default(); 4096], _gpu: PhantomData })
    }
    /// One replica over several GPU contexts (one per GPU of the node, each with `keys` installed;
    /// pbft_replica_create_multi): a large flush is cut into one slice per context, staged and launched
    /// on every GPU's own PCIe link at once, and applied in row order as each slice's bitmap lands.
    pub fn new_multi(gpus: &[&'a GpuVerifier], self_id: u32, keys: &[[u8; 32]]) -> Result<Self> {
        let ctxs: Vec<*mut ffi::pbft_ctx> = gpus.iter().map(|g| g.raw()).collect();
        let mut raw = ptr::null_mut();
        check(unsafe {
            ffi::pbft_replica_create_multi(ctxs.as_ptr(), ctxs.len() as u32, keys.len() as u32, self_id,
                                           keys.as_ptr() as *const u8, &mut raw)
        })?;
        Ok(Replica { raw, verifier: None, events: vec![ffi::pbft_round_event::default(); 4096], _gpu: PhantomData })
    }
    /// Back the batcher with any BatchVerifier (e.g. CpuVerifier) instead of the GPU context; its
    /// submit / poll become the replica's flush_submit / flush_poll.
    pub fn set_verifier(&mut self, v: Box<dyn BatchVerifier>) -> Result<()> {
        let mut boxed = Box::new(Backend { v, pending: None });
        let user = &mut *boxed as *mut Backend as *mut c_void;
        check(unsafe {
            ffi::pbft_replica_set_votes_verifier(self.raw, votes_submit_trampoline, votes_poll_trampoline, user)
        })?;
        self.verifier = Some(boxed);
        Ok(())
    }
    /// Peers admitted after start-up (Pbft::add_peer, src/behavior.rs:45-61): replica `idx[i]` gets `keys[i]`
    /// (its PeerId resolves through `peer_index` from now on; with a GPU context only its tables are rebuilt).
    pub fn update_keys(&mut self, idx: &[u32], keys: &[[u8; 32]]) -> Result<Vec<bool>> {
        if idx.len() != keys.len() {
            return Err(Error { code: ffi::PBFT_EINVAL, message: "update_keys: idx and keys lengths differ".into() });
        }
        let mut ok = vec![0u8; keys.len()];
        check(unsafe {
            ffi::pbft_replica_update_keys(self.raw, idx.as_ptr(), keys.as_ptr() as *const u8, keys.len() as u32,
                                          ok.as_mut_ptr())
        })?;
        Ok(ok.into_iter().map(|b| b == 1).collect())
    }
    /// PrePrepare ingress (validate_pre_prepare, src/behavior.rs:126-157, plus the signature TODO :127) from
    /// replica `peer` -- the AUTHENTICATED connection's replica index (`peer_index` of inject_node_event's
    /// peer_id, src/behavior.rs:304); dropped unless it is the view's primary.
    pub fn on_pre_prepare(&mut self, peer: u32, view: u64, seq: u64, operation: &[u8], digest: &[u8; 64],
                          primary_sig: &[u8; 64]) -> Result<bool> {
        let rc = check(unsafe {
            ffi::pbft_replica_on_pre_prepare(self.raw, peer, view, seq, operation.as_ptr(), operation.len() as u32,
                                             digest.as_ptr(), primary_sig.as_ptr(), ptr::null_mut())
        })?;
        Ok(rc == 1)
    }
    /// Many pushes at once (e.g. one decoded read of every connection); returns how many were queued.
    pub fn push_many(&mut self, kind: &[u8], view: &[u64], seq: &[u64], digests: &[[u8; 64]], signer: &[u32],
                     sigs: &[[u8; 64]]) -> Result<u64> {
        let n = kind.len();
        if view.len() != n || seq.len() != n || digests.len() != n || signer.len() != n || sigs.len() != n {
            return Err(Error { code: ffi::PBFT_EINVAL, message: "push_many: column lengths differ".into() });
        }
        let mut q = 0u64;
        check(unsafe {
            ffi::pbft_replica_push_many(self.raw, n as u64, kind.as_ptr(), view.as_ptr(), seq.as_ptr(),
                                        digests.as_ptr() as *const u8, signer.as_ptr(), sigs.as_ptr() as *const u8,
                                        &mut q)
        })?;
        Ok(q)
    }
    /// A Prepare / Commit from the AUTHENTICATED peer `signer` (inject_node_event's peer_id).
    pub fn push(&mut self, kind: u8, view: u64, seq: u64, digest: &[u8; 64], signer: u32, sig: &[u8; 64])
                -> Result<bool> {
        let rc = check(unsafe {
            ffi::pbft_replica_push(self.raw, kind, view, seq, digest.as_ptr(), signer, sig.as_ptr())
        })?;
        Ok(rc == 1)
    }
    /// Raw UviBytes/JSON frames read from peer `peer_idx`'s connection; returns bytes consumed
    /// (keep the rest for the next read).
    pub fn push_frames(&mut self, peer_idx: u32, stream: &[u8]) -> Result<usize> {
        let (mut used, mut pushed, mut dropped) = (0u64, 0u64, 0u64);
        check(unsafe {
            ffi::pbft_replica_push_frames(self.raw, peer_idx, stream.as_ptr(), stream.len(), &mut used,
                                          &mut pushed, &mut dropped)
        })?;
        Ok(used as usize)
    }
    /// Every connection's bytes at once (pbft_replica_push_streams): `segments[i]` = (offset, length, authenticated
    /// peer) of one connection's bytes in `stream`, from a frame boundary on.  Equivalent to a forced flush, one
    /// `push_frames` per segment and another forced flush, with the index, the decode, the admission, the grouping, the
    /// verification and the tallies on the GPU.  Returns the per-segment heads (`consumed`: keep the rest for the next
    /// read), the votes pushed, the frames dropped and the round events sorted by (view, seq, kind).
    pub fn push_streams(&mut self, stream: &[u8], segments: &[(u64, u64, u16)], max_events: usize)
                        -> Result<(Vec<ffi::pbft_seg_head>, u64, u64, Vec<ffi::pbft_round_event>)> {
        let off: Vec<u64> = segments.iter().map(|s| s.0).collect();
        let len: Vec<u64> = segments.iter().map(|s| s.1).collect();
        let peer: Vec<u16> = segments.iter().map(|s| s.2).collect();
        let mut heads = vec![ffi::pbft_seg_head::default(); segments.len()];
        let mut events = vec![ffi::pbft_round_event::default(); max_events];
        let (mut pushed, mut dropped, mut n_events) = (0u64, 0u64, 0u32);
        check(unsafe {
            ffi::pbft_replica_push_streams(self.raw, stream.as_ptr(), stream.len() as u64, off.as_ptr(), len.as_ptr(),
                                           peer.as_ptr(), segments.len() as u32, heads.as_mut_ptr(), &mut pushed,
                                           &mut dropped, events.as_mut_ptr(), max_events as u32, &mut n_events)
        })?;
        events.truncate(n_events as usize);
        Ok((heads, pushed, dropped, events))
    }
    /// Caps and buffers of the next `push_streams` calls (pbft_replica_reserve_streams).
    pub fn reserve_streams(&mut self, max_stream_bytes: u64, max_segments: u32, frame_cap: u64, env_cap: u32,
                           residue_cap: u32) -> Result<()> {
        check(unsafe {
            ffi::pbft_replica_reserve_streams(self.raw, max_stream_bytes, max_segments, frame_cap, env_cap, residue_cap)
        }).map(|_| ())
    }
    pub fn streams_stats(&self) -> ffi::pbft_replica_streams_stats {
        let mut s = ffi::pbft_replica_streams_stats::default();
        unsafe { ffi::pbft_replica_get_streams_stats(self.raw, &mut s) };
        s
    }
    /// Whether `push_streams` applies the residue's canonical PrePrepares from the heads the front half brings
    /// (pbft_replica_set_streams_pp; default on).  Off: every PrePrepare goes through the general parser.
    pub fn set_streams_pp(&mut self, on: bool) -> Result<()> {
        check(unsafe { ffi::pbft_replica_set_streams_pp(self.raw, on as c_int) }).map(|_| ())
    }
    /// The replica signs its own votes on the GPU (pbft_replica_set_signing_seed): the seed's public key must be
    /// keys[self_id]; turns the outbox on.  `None` clears the seed.
    pub fn set_signing_seed(&mut self, seed: Option<&[u8; 32]>) -> Result<()> {
        check(unsafe {
            ffi::pbft_replica_set_signing_seed(self.raw, seed.map_or(ptr::null(), |s| s.as_ptr()))
        }).map(|_| ())
    }
    /// Sign and encode every vote the decided events oblige this replica to send (pbft_replica_emit_frames): the
    /// bytes to write to every connected peer, and the number of votes.  `loopback`: the votes are also pushed as
    /// this replica's own (verified in the next flush).
    pub fn emit_frames(&mut self, loopback: bool) -> Result<(Vec<u8>, u64)> {
        let flags = if loopback { ffi::PBFT_EMIT_LOOPBACK } else { 0 };
        let (mut len, mut votes) = (0usize, 0u64);
        check(unsafe { ffi::pbft_replica_emit_frames(self.raw, 0, ptr::null_mut(), 0, &mut len, &mut votes) })?;
        let mut out = vec![0u8; len];
        if len > 0 {
            check(unsafe {
                ffi::pbft_replica_emit_frames(self.raw, flags, out.as_mut_ptr(), out.len(), &mut len, &mut votes)
            })?;
            out.truncate(len);
        }
        Ok((out, votes))
    }
    /// The primary's add_client_request for a batch (pbft_replica_propose): the requests that fit the window get the
    /// next sequence numbers and come back as signed PrePrepare frames, the bytes to write to every connected peer.
    /// Returns (frames, first sequence number, requests proposed); the rest are the caller's to offer again.
    /// `loopback`: each PrePrepare is also applied as this replica's own (verified in the next flush).
    pub fn propose(&mut self, requests: &[ClientRequest], loopback: bool) -> Result<(Vec<u8>, u64, u64)> {
        let flags = if loopback { ffi::PBFT_PROPOSE_LOOPBACK } else { 0 };
        let p = PackedRequests::new(requests);
        let (mut len, mut first, mut n) = (0usize, 0u64, 0u64);
        check(unsafe {
            ffi::pbft_replica_propose(self.raw, requests.len() as u64, p.ops.as_ptr(), p.ops_bytes, p.off.as_ptr(),
                                      p.len.as_ptr(), p.ts.as_ptr(), p.clients.as_ptr() as *const c_char, 0,
                                      ptr::null_mut(), 0, &mut len, &mut first, &mut n)
        })?;
        let mut out = vec![0u8; len];
        if len > 0 {
            check(unsafe {
                ffi::pbft_replica_propose(self.raw, requests.len() as u64, p.ops.as_ptr(), p.ops_bytes, p.off.as_ptr(),
                                          p.len.as_ptr(), p.ts.as_ptr(), p.clients.as_ptr() as *const c_char, flags,
                                          out.as_mut_ptr(), out.len(), &mut len, &mut first, &mut n)
            })?;
            out.truncate(len);
        }
        Ok((out, first, n))
    }
    /// The next sequence number a proposal gets (pbft_replica_set_next_seq; 1 at creation).
    pub fn set_next_seq(&mut self, seq: u64) -> Result<()> {
        check(unsafe { ffi::pbft_replica_set_next_seq(self.raw, seq) }).map(|_| ())
    }
    pub fn propose_stats(&self) -> ffi::pbft_replica_propose_stats {
        let mut s = ffi::pbft_replica_propose_stats::default();
        unsafe { ffi::pbft_replica_get_propose_stats(self.raw, &mut s) };
        s
    }
    /// The client's side of a round (pbft_replica_reply): after the events loop the caller executes the requests whose
    /// (view, seq) reported COMMITTED_LOCAL and passes them in execution order: `seqs[i]` with the request's timestamp
    /// and client in `executed[i]` and the result in its `operation` field.  Entries that are not committed-local or
    /// whose timestamp is not above the last reply's are skipped (exactly-once, src/behavior.rs:391-398).  Returns the
    /// signed replies' texts back to back, where each lies (reply i at [reply_off[i], reply_off[i + 1]), empty when
    /// skipped) and the per-entry status (ffi::PBFT_REPLY_*); each text goes to its client's connection.
    pub fn reply(&mut self, seqs: &[u64], executed: &[ClientRequest]) -> Result<(Vec<u8>, Vec<u64>, Vec<u8>)> {
        assert_eq!(seqs.len(), executed.len());
        let p = PackedRequests::new(executed);
        let n = seqs.len();
        let (mut len, mut made) = (0usize, 0u64);
        check(unsafe {
            ffi::pbft_replica_reply(self.raw, n as u64, seqs.as_ptr(), p.ts.as_ptr(), p.clients.as_ptr() as *const c_char,
                                    p.ops.as_ptr(), p.ops_bytes, p.off.as_ptr(), p.len.as_ptr(), 0, ptr::null_mut(), 0,
                                    &mut len, ptr::null_mut(), ptr::null_mut(), &mut made)
        })?;
        let mut out = vec![0u8; len.max(1)];
        let mut off = vec![0u64; n + 1];
        let mut status = vec![0u8; n];
        check(unsafe {
            ffi::pbft_replica_reply(self.raw, n as u64, seqs.as_ptr(), p.ts.as_ptr(), p.clients.as_ptr() as *const c_char,
                                    p.ops.as_ptr(), p.ops_bytes, p.off.as_ptr(), p.len.as_ptr(), 0, out.as_mut_ptr(),
                                    len, &mut len, off.as_mut_ptr(), status.as_mut_ptr(), &mut made)
        })?;
        out.truncate(len);
        Ok((out, off, status))
    }
    /// The timestamp of the last reply (State::last_timestamp; 0 at creation), to save and restore over a restart.
    pub fn last_timestamp(&self) -> u64 {
        let mut t = 0u64;
        unsafe { ffi::pbft_replica_last_timestamp(self.raw, &mut t) };
        t
    }
    pub fn set_last_timestamp(&mut self, timestamp: u64) -> Result<()> {
        check(unsafe { ffi::pbft_replica_set_last_timestamp(self.raw, timestamp) }).map(|_| ())
    }
    pub fn reply_stats(&self) -> ffi::pbft_replica_reply_stats {
        let mut s = ffi::pbft_replica_reply_stats::default();
        unsafe { ffi::pbft_replica_get_reply_stats(self.raw, &mut s) };
        s
    }
    pub fn egress_stats(&self) -> ffi::pbft_replica_egress_stats {
        let mut s = ffi::pbft_replica_egress_stats::default();
        unsafe { ffi::pbft_replica_get_egress_stats(self.raw, &mut s) };
        s
    }
    pub fn pp_stats(&self) -> ffi::pbft_replica_pp_stats {
        let mut s = ffi::pbft_replica_pp_stats::default();
        unsafe { ffi::pbft_replica_get_pp_stats(self.raw, &mut s) };
        s
    }
    /// 160-byte binary records (pbft_wire.h PBFT_RECORD_BYTES) read from peer `peer_idx`'s connection;
    /// returns (bytes consumed, votes pushed, records dropped) -- keep the unconsumed tail for the next read.
    pub fn push_records(&mut self, peer_idx: u32, stream: &[u8]) -> Result<(usize, u64, u64)> {
        let (mut used, mut pushed, mut dropped) = (0u64, 0u64, 0u64);
        check(unsafe {
            ffi::pbft_replica_push_records(self.raw, peer_idx, stream.as_ptr(), stream.len(), &mut used,
                                           &mut pushed, &mut dropped)
        })?;
        Ok((used as usize, pushed, dropped))
    }
    /// Where the last push_many and the last flush spent their time (host clock, ns).
    pub fn timings(&self) -> Result<ffi::pbft_replica_timings> {
        let mut t = ffi::pbft_replica_timings::default();
        check(unsafe { ffi::pbft_replica_get_timings(self.raw, &mut t) })?;
        Ok(t)
    }
    /// Launch one batch of every ready sub-window (force = the deadline: everything pending) without
    /// waiting for it; returns its signatures (0: nothing launched).  Err(PBFT_EBUSY) while one is in flight.
    pub fn flush_submit(&mut self, force: bool) -> Result<u64> {
        let mut n = 0u64;
        check(unsafe { ffi::pbft_replica_flush_submit(self.raw, force as c_int, &mut n) })?;
        Ok(n)
    }
    /// Call from NetworkBehaviour::poll (src/behavior.rs:416-426): None while the GPU works, else the round
    /// events decided by the finished batch (and any still queued).
    pub fn flush_poll(&mut self) -> Result<Option<Vec<RoundEvent>>> {
        let mut n = 0u32;
        let rc = check(unsafe {
            ffi::pbft_replica_flush_poll(self.raw, self.events.as_mut_ptr(), self.events.len() as u32, &mut n)
        })?;
        if rc == 0 {
            return Ok(None);
        }
        Ok(Some(round_events(&self.events[..n as usize])))
    }
    /// Blocking: verify every ready sub-window in one batch and report new round events.
    pub fn flush(&mut self, force: bool) -> Result<Vec<RoundEvent>> {
        let mut n = 0u32;
        check(unsafe {
            ffi::pbft_replica_flush(self.raw, force as c_int, self.events.as_mut_ptr(), self.events.len() as u32,
                                    &mut n)
        })?;
        Ok(round_events(&self.events[..n as usize]))
    }
    /// The replica index of an authenticated connection's PeerId (None: not a replica).
    pub fn peer_index(&self, peer_id: &[u8]) -> Option<u32> {
        let rc = unsafe { ffi::pbft_replica_peer_index(self.raw, peer_id.as_ptr(), peer_id.len()) };
        if rc >= 0 { Some(rc as u32) } else { None }
    }
    pub fn stable_checkpoint(&mut self, seq: u64) -> Result<()> {
        check(unsafe { ffi::pbft_replica_stable_checkpoint(self.raw, seq) }).map(|_| ())
    }
    pub fn stats(&self) -> ffi::pbft_replica_stats {
        let mut s = ffi::pbft_replica_stats::default();
        unsafe { ffi::pbft_replica_get_stats(self.raw, &mut s) };
        s
    }
}

impl Drop for Replica<'_> {
    fn drop(&mut self) {
        // destroy completes a batch in flight (through the installed verifier) before `verifier` is dropped
        unsafe { ffi::pbft_replica_destroy(self.raw) };
    }
}

/// Several GPUs of this process with the round's bitmap words all-gathered on RCCL
/// (pbft_multi_create / pbft_verify_batch_device_multi).  Borrows its `GpuVerifier`s (`'a`):
/// their contexts must outlive it (Drop synchronises their streams).
pub struct MultiGpu<'a> {
    raw: *mut ffi::pbft_multi,
    _gpus: PhantomData<&'a GpuVerifier>,
}

impl<'a> MultiGpu<'a> {
    /// One context per device, in rank order.
    pub fn new(gpus: &[&'a GpuVerifier]) -> Result<Self> {
        let ctxs: Vec<*mut ffi::pbft_ctx> = gpus.iter().map(|g| g.raw()).collect();
        let mut raw = ptr::null_mut();
        check(unsafe { ffi::pbft_multi_create(ctxs.as_ptr(), ctxs.len() as u32, &mut raw) })?;
        Ok(MultiGpu { raw, _gpus: PhantomData })
    }
    /// Enqueue: rank r verifies its device-resident shard; every rank's `d_bitmap[r]` then holds the round
    /// (rank-major, `words_per_rank` words per rank).  # Safety: device pointers as in include/pbft_verify.h.
    pub unsafe fn verify_device(&mut self, d_r: &[*const u8], d_s: &[*const u8], d_key_idx: &[*const u16],
                                d_msg: &[*const u8], n: &[u64], words_per_rank: u64,
                                d_bitmap: &[*mut u64]) -> Result<()> {
        check(ffi::pbft_verify_batch_device_multi(self.raw, d_r.as_ptr(), d_s.as_ptr(), d_key_idx.as_ptr(),
                                                  d_msg.as_ptr(), ffi::PBFT_ENVELOPE_BYTES as u32,
                                                  ffi::PBFT_ENVELOPE_BYTES as u32, n.as_ptr(), words_per_rank,
                                                  d_bitmap.as_ptr())).map(|_| ())
    }
    pub fn sync(&mut self) -> Result<()> {
        check(unsafe { ffi::pbft_multi_sync(self.raw) }).map(|_| ())
    }
}

impl Drop for MultiGpu<'_> {
    fn drop(&mut self) {
        unsafe { ffi::pbft_multi_destroy(self.raw) };
    }
}

/*
 * edv.h -- C-ABI of the MI355X (gfx950) batch Ed25519 verifier (libedv.so).
 *
 * Drop-in boundary for Plenum's client-request authentication hot path.  In the
 * reference every request signature ends in ONE call:
 *
 *   stp_core/crypto/nacl_wrappers.py:232-242  Verifier.verify(signature, msg)
 *       -> VerifyKey.verify(signature + msg)           nacl_wrappers.py:86-108
 *       -> libnacl.crypto_sign_open(sm, pk)            (libsodium 1.0.18)
 *
 * made once per signature from NaclAuthNr.authenticate_multi
 * (plenum/server/client_authn.py:83-113) through DidVerifier.verify
 * (plenum/common/verifier.py:54-55).  edv_verify_batch replaces a whole batch of
 * those calls; the Python shim (indy-plenum_amd/nacl_wrappers.py, client_authn.py,
 * req_authenticator.py) keeps the reference's per-request semantics above it.
 *
 * Verdict contract: accept[i] == 1 iff libsodium 1.0.18
 * crypto_sign_ed25519_verify_detached(sig_i, msg_i, len_i, pk_i) == 0, bit for
 * bit (strict S < L, small-order R/A blocklist, canonical A, cofactorless
 * equation).  The reference's positional sig||msg split (crypto_sign_open on
 * signature + msg) is applied by the caller before this layer (see
 * INTEGRATION.md); every sig here is exactly 64 bytes.
 *
 * All entry points return 0 on success or a negative EDV_E_* code, never
 * throw, and keep no pointer to caller memory after returning (except
 * edv_verify_batch_async, until edv_wait_async -- or edv_query_async returning
 * anything but EDV_PENDING -- for that batch).
 */
#ifndef EDV_H
#define EDV_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EDV_OK 0
#define EDV_E_ARG -1   /* bad argument (null pointer with n > 0, bad offsets) */
#define EDV_E_NODEV -2 /* no usable gfx950 device in device_mask */
#define EDV_E_HIP -3   /* HIP runtime error (text: edv_last_error) */
#define EDV_E_OOM -4   /* device or pinned allocation failed */
#define EDV_E_BUSY -5  /* edv_trim / edv_release: batches not yet handed over still own caller buffers */
#define EDV_E_SELFTEST -6 /* edv_self_test / edv_prepare: a verdict differs from libsodium's (text: edv_last_error) */

/*
 * Verify n detached signatures held in HOST memory; synchronous.
 * A device's shard of up to one chunk (2^18 requests, edv_set_chunk) is
 * copied field by field: signatures, keys and offsets first (the point sides
 * of the prep kernel start on them), then the messages (their hash side
 * starts as each slice lands), then the main kernel, which writes the
 * verdicts straight into page-locked host memory (no D2H copy).  A larger
 * shard alternates two streams of half-chunk sub-batches, so the copies of
 * one overlap the kernels of the other.  A shard of at most 16,384 requests
 * (a Node's prod, one Verifier.verify) takes the latency path instead
 * (edv_set_latency_path): one kernel launch with sixteen lanes per signature
 * (eight above 4,096 requests);
 * pinned inputs are copied by DMA straight from the caller's buffers (one copy
 * when sigs, pks and msg_off lie in one region in that order, then the
 * messages), pageable ones are packed into the library's pinned staging and
 * read there by the kernel.  On the batch path, inputs in pinned memory (e.g.
 * from edv_host_alloc) are copied to the device directly; pageable inputs are
 * first staged through the library's pinned buffers by a parallel memcpy
 * (EDV_COPY_THREADS threads, default 8).
 *   sigs     n x 64 bytes (R || S), contiguous
 *   pks      n x 32 bytes (A), contiguous
 *   msgs     concatenated messages; message i = msgs[msg_off[i] .. msg_off[i+1])
 *   msg_off  n + 1 non-decreasing byte offsets
 *   accept   out: n bytes, 1 = accept, 0 = reject
 *   device_mask  bit d selects device d; 0 = all visible devices.  The batch is
 *            split by request index into contiguous shards, one per device and
 *            one host thread each (edv_shard_split: equal counts, or equal
 *            estimated cost when SHA-512 block counts differ); no inter-device
 *            traffic; each shard's accept bytes land in its slice.
 * Replaces: a loop of nacl_wrappers.Verifier.verify (nacl_wrappers.py:232-242).
 */
int edv_verify_batch(const uint8_t *sigs, const uint8_t *pks, const uint8_t *msgs, const uint64_t *msg_off,
                     uint64_t n, uint8_t *accept, uint32_t device_mask);

/*
 * Asynchronous form of edv_verify_batch on one device (the batched call site of
 * plenum/server/client_authn.py:92-112 when the Node verifies one batch per prod
 * and keeps going): queues the H2D copies, the kernels and the D2H of the
 * verdicts and returns a ticket at once.  Batches take eight slots in turn,
 * so batch k+1's copies (and, for pageable inputs, its staging memcpy, done in
 * this call) run while batch k computes: back to back, the host path then runs
 * at the kernels' rate rather than copy + kernels.  The caller's buffers must
 * stay valid and unchanged, and `accept` unread, until edv_wait_async(device,
 * ticket) (or edv_query_async) returns 0; a submission waits for the batch eight submissions back
 * (completing it as edv_wait_async would) before reusing its slot.  Same
 * verdicts, arguments and alignment rules as edv_verify_batch.
 */
int edv_verify_batch_async(const uint8_t *sigs, const uint8_t *pks, const uint8_t *msgs, const uint64_t *msg_off,
                           uint64_t n, uint8_t *accept, int device, int64_t *ticket);
/* Wait for batch `ticket` of `device` and hand over its verdicts (0 at once if
 * it already was); EDV_E_ARG for a ticket never issued.  Fails closed: `accept`
 * is zeroed at submission (an unfilled buffer rejects), and once a batch has
 * failed, every wait for a ticket at or below it that is no longer pending
 * returns EDV_E_HIP, however many batches fail later. */
int edv_wait_async(int device, int64_t ticket);
/* edv_wait_async without the wait: EDV_PENDING while batch `ticket` of `device`
 * is still on the GPU (nothing changes), else exactly what edv_wait_async
 * returns, with the verdicts handed over.  Lets a Node hand a prod's batch over
 * in the same prod when the GPU is already done, and at its next prod if not. */
#define EDV_PENDING 1
int edv_query_async(int device, int64_t ticket);
/*
 * edv_verify_batch_async that also returns, when `digests` is not NULL, the
 * SHA-256 of every message (digests: n x 32 bytes, same lifetime rules as
 * `accept`), computed on the device from the bytes already copied for the
 * verify.  For a request whose signing bytes are its signingState's
 * serialization these are Request.getDigest (plenum/common/request.py:71-72),
 * which the Node computes per request next to the signature check
 * (plenum/server/node.py:2093-2147); the caller decides which requests that
 * holds for.  Ticket and wait as for edv_verify_batch_async.
 */
int edv_verify_digest_batch_async(const uint8_t *sigs, const uint8_t *pks, const uint8_t *msgs,
                                  const uint64_t *msg_off, uint64_t n, uint8_t *accept, uint8_t *digests, int device,
                                  int64_t *ticket);

/*
 * Same verdicts for inputs already resident in device memory of `device`;
 * asynchronous on `stream` (a hipStream_t, NULL = the library's own stream of
 * that device, which is then synchronised before returning).  Offsets are
 * absolute into d_msgs minus msg_base (so a shard may pass the global offset
 * array slice unchanged).
 * Alignment (EDV_E_ARG otherwise): d_sigs and d_pks 16-byte aligned (read as
 * 16-byte vectors), d_msg_off 8-byte aligned.  d_msgs may have any alignment:
 * message bytes are read as aligned 32-bit words, so the kernels touch up to
 * 3 bytes before a message start (never across a page) and up to 16 bytes past
 * the last message byte, which must be readable.
 * Launches on different streams never share the library's per-device scratch
 * concurrently: each one is ordered after the previous user of the scratch.
 */
int edv_verify_batch_dev(const uint8_t *d_sigs, const uint8_t *d_pks, const uint8_t *d_msgs,
                         const uint64_t *d_msg_off, uint64_t msg_base, uint64_t n, uint8_t *d_accept,
                         int device, void *stream);

/* Per-call SHA-512 length-bucket hint for the device paths (overrides the
 * device mode of edv_set_length_buckets for this call only). */
#define EDV_FLAG_UNIFORM_LENGTH 1u /* every message has the same SHA-512 block count: no buckets */
#define EDV_FLAG_BUCKETS 2u        /* always bucket by block count */
#define EDV_FLAG_SPLIT_PREP 4u     /* edv_verify_batch_dev_pipelined only: the hash side of batch k+1's
                                      prep runs beside batch k's main kernel, the point sides after it */
int edv_verify_batch_dev_flags(const uint8_t *d_sigs, const uint8_t *d_pks, const uint8_t *d_msgs,
                               const uint64_t *d_msg_off, uint64_t msg_base, uint64_t n, uint8_t *d_accept,
                               int device, void *stream, uint32_t flags);

/*
 * Batch SHA-256: out[32 i .. 32 i + 32) = SHA-256 of message i
 * (msgs/msg_off as in edv_verify_batch).  Host buffers, synchronous, sharded over
 * device_mask like edv_verify_batch.  Replaces, per request,
 * plenum/common/request.py:71-72 Request.getDigest (sha256 of the signing bytes,
 * hex-encoded by the caller) and plenum/server/domain_req_handler.py:166-167
 * nym_to_state_key (sha256 of the DID string).
 */
int edv_sha256_batch(const uint8_t *msgs, const uint64_t *msg_off, uint64_t n, uint8_t *out, uint32_t device_mask);
/* Device-resident form, async on `stream` (NULL = library stream, synchronised);
 * d_msgs readable 8 bytes past the last message byte; d_out n x 32 bytes.
 * Offsets are absolute into d_msgs minus msg_base, as for edv_verify_batch_dev.
 * EDV_E_ARG, with nothing launched: d_msg_off not 8-byte or d_out not 16-byte
 * aligned (the offsets are read as 64-bit words, each digest is stored as two
 * 16-byte vectors; d_msgs may have any alignment), or n > 0 with d_msgs,
 * d_msg_off or d_out NULL.  A NULL d_msgs is refused whenever n > 0, even if
 * every message is empty: the offsets live in device memory, so the library
 * cannot know that without reading them. */
int edv_sha256_batch_dev(const uint8_t *d_msgs, const uint64_t *d_msg_off, uint64_t msg_base, uint64_t n,
                         uint8_t *d_out, int device, void *stream);

/*
 * Ledger Merkle tree (row f-5): extend a compact RFC 6962 tree by a batch of
 * leaves in one call, bit-exact with n successive appends of the reference's
 * CompactMerkleTree (ledger/compact_merkle_tree.py:155-191 over
 * ledger/tree_hasher.py:20-28, called per transaction by
 * ledger/ledger.py:145-148).  Leaf hash SHA-256(0x00 | leaf), node hash
 * SHA-256(0x01 | left | right), empty root SHA-256("").
 *
 * A tree is (size, hashes): the roots of the full subtrees of the binary
 * decomposition of size, largest first, popcount(size) x 32 bytes.  With
 * new = old_size + n the call writes
 *   leaf_hashes  n x 32 bytes, in order (NULL: not wanted)
 *   node_hashes  the interior nodes in the order the appends create them
 *                (leaf s, 1-based, writes heights 1 .. ctz(s), ascending):
 *                (new - popcount(new)) - (old - popcount(old)) x 32 bytes, the
 *                node-store positions after the old tree's (NULL: not wanted)
 *   new_hashes   popcount(new) x 32 bytes (at most 63 entries)
 *   root         32 bytes
 * n = 0 is valid (hashes copied, root folded).  leaves / leaf_off are laid out
 * as msgs / msg_off everywhere else: n + 1 non-decreasing offsets.
 * EDV_E_ARG before anything is launched or written: n above
 * EDV_MERKLE_MAX_LEAVES, old_size + n above 2^62, old_size > 0 with NULL
 * old_hashes, NULL new_hashes / root, NULL leaf_off (or leaves, unless every
 * leaf is empty) with n > 0, offsets that decrease.
 * Host form: synchronous on `device`, staged in buffers of its own; only the
 * outputs asked for are copied back.  The scratch (tile roots handed from one
 * pass of eight heights to the next) and the staging grow by use, count in
 * edv_context_memory out[2], and are freed by edv_trim (what a batch of
 * keep_batch leaves does not need; all for 0) and edv_release.  A process that
 * never calls these two allocates nothing for them.
 */
#define EDV_MERKLE_MAX_LEAVES (1ull << 22)
int edv_merkle_extend(uint64_t old_size, const uint8_t *old_hashes,
                      const uint8_t *leaves, const uint64_t *leaf_off, uint64_t n,
                      uint8_t *leaf_hashes, uint8_t *node_hashes,
                      uint8_t *new_hashes, uint8_t *root, int device);
/* Device-resident form, async on `stream` (NULL = library stream, synchronised
 * before returning); offsets are absolute into d_leaves minus leaf_base.
 * d_leaves may have any alignment and must be readable 8 bytes past the last
 * leaf byte; nothing below the aligned 32-bit word holding a leaf's first byte
 * is read.  Also EDV_E_ARG, with nothing launched: d_leaf_off not 8-byte
 * aligned, any hash buffer (d_old_hashes, d_leaf_hashes, d_node_hashes,
 * d_new_hashes, d_root) not 16-byte aligned, n > 0 with NULL d_leaves or
 * d_leaf_off (the offsets live in device memory and are not checked).  The
 * output buffers must not overlap d_old_hashes.  Calls on different streams
 * are ordered on the shared scratch by an event, as the verify launches are. */
int edv_merkle_extend_dev(uint64_t old_size, const uint8_t *d_old_hashes,
                          const uint8_t *d_leaves, const uint64_t *d_leaf_off, uint64_t leaf_base, uint64_t n,
                          uint8_t *d_leaf_hashes, uint8_t *d_node_hashes,
                          uint8_t *d_new_hashes, uint8_t *d_root, int device, void *stream);

/*
 * Batched append (row f-6): edv_merkle_extend that also returns what each of
 * the n `append` calls of the reference returns (ledger/ledger.py:145-155 over
 * ledger/compact_merkle_tree.py:155-160, called once per transaction by
 * plenum/common/ledger.py:71-96, commitTxns), for every leaf i (0-based):
 *   roots        n x 32 bytes: the root hash of the tree of old_size + i + 1
 *                leaves; roots[n - 1] equals root (NULL: not wanted)
 *   audit_paths  leaf i's audit path: the hashes of the tree of old_size + i
 *                leaves, smallest subtree first (the reference's
 *                reversed(hashes)), popcount(old_size + i) x 32 bytes, packed
 *                one path after another: leaf i's starts at entry
 *                edv_merkle_path_entries(old_size, i, ..), the whole output is
 *                edv_merkle_path_entries(old_size, n, ..) x 32 bytes
 *                (NULL: not wanted)
 * Every other argument, limit, alignment rule and EDV_E_ARG case is
 * edv_merkle_extend[_dev]'s; d_roots and d_audit_paths are hash buffers
 * (16-byte aligned, not overlapping the inputs).  With roots and audit_paths
 * both NULL the call is edv_merkle_extend.  n = 0 writes neither.  One more
 * kernel after the passes, one lane per leaf: the lane folds popcount(s) - 1
 * node hashes, s = old_size + i + 1, and gathers its path.  It reads the leaf
 * and node hashes on the device, so they are kept there whether wanted or
 * not: the host form stages them with its other outputs and skips the copy
 * back, the device form puts a NULL d_leaf_hashes / d_node_hashes into context
 * scratch, ordered across streams with the tile-root scratch.  All of it is
 * counted in edv_context_memory out[2] and freed by edv_trim and edv_release.
 * The packed paths of a maximal call are gigabytes: a failed allocation of the
 * host form's staging returns EDV_E_OOM with nothing written.
 */
int edv_merkle_append_batch(uint64_t old_size, const uint8_t *old_hashes,
                            const uint8_t *leaves, const uint64_t *leaf_off, uint64_t n,
                            uint8_t *leaf_hashes, uint8_t *node_hashes,
                            uint8_t *new_hashes, uint8_t *root,
                            uint8_t *roots, uint8_t *audit_paths, int device);
int edv_merkle_append_batch_dev(uint64_t old_size, const uint8_t *d_old_hashes,
                                const uint8_t *d_leaves, const uint64_t *d_leaf_off, uint64_t leaf_base, uint64_t n,
                                uint8_t *d_leaf_hashes, uint8_t *d_node_hashes,
                                uint8_t *d_new_hashes, uint8_t *d_root,
                                uint8_t *d_roots, uint8_t *d_audit_paths, int device, void *stream);
/* Host only (no device is touched): *entries = the number of audit-path
 * entries of the first n appends to a tree of old_size leaves, the sum of
 * popcount(old_size + i) over i < n.  EDV_E_ARG: NULL entries, old_size + n
 * above 2^62.  (An int result with an out-parameter, like every entry point
 * here.) */
int edv_merkle_path_entries(uint64_t old_size, uint64_t n, uint64_t *entries);

/*
 * Batched proof verification (row f-7): what the reference's MerkleVerifier
 * (ledger/merkle_verifier.py) checks one proof at a time for a client
 * (plenum/client/client.py:846-873, verifyMerkleProof) and for a node in
 * catch-up (plenum/common/ledger_manager.py:564-609), for n proofs in one
 * call: RFC 6962 section 2.1.1 audit paths and 2.1.2 consistency proofs, one
 * lane per proof.  Every uint64_t tree size is valid (a walk is at most 64
 * levels).
 *   proofs      packed 32-byte entries, lowest level first
 *   proof_off   n + 1 non-decreasing offsets IN ENTRIES: proof i is entries
 *               [proof_off[i], proof_off[i + 1]).  This is the layout
 *               edv_merkle_append_batch writes: its audit_paths and roots, with
 *               offsets from edv_merkle_path_entries(old_size, i, ..), feed the
 *               device form unchanged (leaf i has index old_size + i in the
 *               tree of old_size + i + 1 leaves)
 *   leaves / leaf_off   the leaf bytes, laid out as msgs / msg_off everywhere
 *               else and readable 8 bytes past the end; the lane hashes its
 *               leaf itself.  Or
 *   leaf_hashes n x 32 bytes.  Exactly one of leaves and leaf_hashes is given
 *   roots       n x 32 bytes: the root hash each proof must arrive at
 *   status      n bytes, one EDV_PROOF_* each (0 never means good)
 *   computed    NULL, or n x 32 bytes: the root the walk calculated where it
 *               ran to its end (OK, LONG, ROOT), zeros otherwise.  Consistency:
 *               n x 64 bytes, the calculated old root, then the new one
 *               (zeros where no walk is made: RANGE, SHORT, equal sizes,
 *               old_size 0)
 * Inclusion, in this order: RANGE, SHORT, LONG, ROOT.  Consistency: old > new
 * is RANGE; equal sizes are OK if the roots are equal, else INCONSISTENT, and
 * old_size 0 is OK (the proof is ignored in both); else SHORT, ROOT (the new
 * root differs), INCONSISTENT (only the old one does); surplus entries after
 * the walk are accepted.
 * n = 0 is valid and writes nothing.  EDV_E_ARG with nothing launched or
 * written: n above EDV_MERKLE_MAX_LEAVES; both leaves and leaf_hashes; with
 * n > 0 neither of them, or NULL leaf_off (with leaves), leaf_index,
 * tree_size / old_size / new_size, roots, proofs, proof_off or status; host
 * offsets that decrease.
 * Host form: fills status with EDV_PROOF_UNVERIFIED, stages in buffers of its
 * own, synchronous.  The staging counts in edv_context_memory out[2]; edv_trim
 * frees what a batch of keep_batch proofs of at most 64 entries would not
 * need (all for 0), edv_release all of it.  A process that never calls the
 * host forms allocates nothing for them.
 */
#define EDV_PROOF_UNVERIFIED 0   /* never written by a kernel: what the host form fills the buffer with first */
#define EDV_PROOF_OK 1
#define EDV_PROOF_RANGE 2        /* leaf_index >= tree_size (tree_size 0 included) / old_size > new_size */
#define EDV_PROOF_SHORT 3        /* the walk needed an entry past the proof's end */
#define EDV_PROOF_LONG 4         /* inclusion only: entries left over after the walk */
#define EDV_PROOF_ROOT 5         /* the computed root (inclusion) / new root (consistency) differs */
#define EDV_PROOF_INCONSISTENT 6 /* consistency only: the new root matches and the old one does not */
int edv_merkle_verify_inclusion(const uint8_t *leaves, const uint64_t *leaf_off, const uint8_t *leaf_hashes,
                                const uint64_t *leaf_index, const uint64_t *tree_size, const uint8_t *roots,
                                const uint8_t *proofs, const uint64_t *proof_off, uint64_t n,
                                uint8_t *status, uint8_t *computed, int device);
int edv_merkle_verify_consistency(const uint64_t *old_size, const uint64_t *new_size, const uint8_t *old_roots,
                                  const uint8_t *new_roots, const uint8_t *proofs, const uint64_t *proof_off,
                                  uint64_t n, uint8_t *status, uint8_t *computed, int device);
/* Device-resident forms, async on `stream` (NULL = library stream,
 * synchronised before returning); offsets are absolute minus leaf_base /
 * proof_base, as in edv_verify_batch_dev.  They use no context memory, so
 * calls on any streams are ordered by their streams alone.  Also EDV_E_ARG,
 * with nothing launched: a 64-bit array (offsets, indices, sizes) not 8-byte
 * aligned, a hash buffer (d_leaf_hashes, d_roots, d_old_roots, d_new_roots,
 * d_proofs, d_computed) not 16-byte aligned; d_status and d_leaves may have
 * any alignment.  The offsets live in device memory and are not checked. */
int edv_merkle_verify_inclusion_dev(const uint8_t *d_leaves, const uint64_t *d_leaf_off, uint64_t leaf_base,
                                    const uint8_t *d_leaf_hashes, const uint64_t *d_leaf_index,
                                    const uint64_t *d_tree_size, const uint8_t *d_roots,
                                    const uint8_t *d_proofs, const uint64_t *d_proof_off, uint64_t proof_base, uint64_t n,
                                    uint8_t *d_status, uint8_t *d_computed, int device, void *stream);
int edv_merkle_verify_consistency_dev(const uint64_t *d_old_size, const uint64_t *d_new_size,
                                      const uint8_t *d_old_roots, const uint8_t *d_new_roots,
                                      const uint8_t *d_proofs, const uint64_t *d_proof_off, uint64_t proof_base, uint64_t n,
                                      uint8_t *d_status, uint8_t *d_computed, int device, void *stream);

/*
 * Batched proof generation (row f-8): what the reference's CompactMerkleTree
 * reads out of its hash store one proof at a time (ledger/compact_merkle_tree.py
 * merkle_tree_hash / inclusion_proof / consistency_proof) for every reply
 * (ledger/ledger.py:197-206 merkleInfo, called by plenum/server/node.py:3024-3034
 * getReplyFromLedger) and in catch-up (plenum/common/ledger_manager.py:448-452,
 * :995-998, :1117-1120), for n proofs in one call, one lane per proof, from a
 * hash store in device memory.
 *   leaf_store  the leaf hashes in order, store_leaves x 32 bytes
 *   node_store  the interior nodes in the order the appends create them (what
 *               edv_merkle_extend writes as node_hashes, tree after tree):
 *               (store_leaves - popcount(store_leaves)) x 32 bytes
 *   leaf_index / tree_size   inclusion: PATH(leaf_index, D[0:tree_size])
 *   first / second           consistency: PROOF(first, D[0:second])
 *   proof_off   n + 1 offsets IN ENTRIES: proof i is written to entries
 *               [proof_off[i], proof_off[i + 1]) of `proofs`, lowest level
 *               first: the layout edv_merkle_verify_* reads
 *   status      n bytes: EDV_PROOF_RANGE (inclusion: leaf_index >= tree_size or
 *               tree_size > store_leaves; consistency: first == 0, first >
 *               second or second > store_leaves), else EDV_PROOF_SPACE (the
 *               slot's length is not the proof's), else EDV_PROOF_OK, and only
 *               then is the slot written.  first == second is OK and empty
 *   roots       NULL, or n x 32 bytes: MTH(D[0:tree_size])
 *   leaf_hashes_out   NULL, or n x 32 bytes: the stored hash of the leaf; with
 *               it one call yields every input of edv_merkle_verify_inclusion
 *   old_roots / new_roots   NULL, or n x 32 bytes: MTH(D[0:first]), MTH(D[0:second])
 *               These outputs hold zeros where the status is not OK.
 * A proof's entries are stored hashes, copied, but at most one, which the fold
 * of the tree head yields on its way: a lane hashes popcount(tree_size) - 1
 * nodes with or without roots wanted (fewer without), and popcount(first) - 1
 * more for old_roots.  Audit paths have at most 62 entries, consistency proofs
 * 63.  No store position at or past the counts is read, nothing outside a
 * proof's own slot is written.
 * The offset helpers touch no device: they fill the n + 1 packed offsets from
 * 0 that fit the proofs exactly (a pair that gets RANGE takes no entries).
 * EDV_E_ARG: a NULL pointer.
 * n = 0 is valid and writes nothing.  EDV_E_ARG with nothing launched or
 * written: n above EDV_MERKLE_MAX_LEAVES; store_leaves above 2^62; with n > 0 a
 * NULL index array, proof_off, proofs or status; NULL leaf_store with
 * store_leaves > 0, NULL node_store with store_leaves > 1; host offsets that
 * decrease.
 * Device forms: async on `stream` (NULL = library stream, synchronised before
 * returning), offsets absolute minus proof_base; no context memory, so calls
 * are ordered by their streams alone.  Alignment as edv_merkle_verify_*_dev:
 * 64-bit arrays on 8 bytes, hash buffers and both stores on 16, d_status any.
 * The outputs must not overlap the stores.
 * Host forms: fill status with EDV_PROOF_UNVERIFIED, synchronous.  THEY COPY
 * THE STORE TO THE DEVICE ON EVERY CALL: the prefix the largest valid tree size
 * reads, 64 bytes per leaf of it.  They exist for small stores and for callers
 * without device memory; a ledger keeps its store on the device and uses the
 * device forms.  Their staging grows by use, counts in edv_context_memory
 * out[2], is cut by edv_trim to what keep_batch proofs of 64 entries need (all
 * of it for 0) and freed by edv_release; only these calls allocate it.
 */
#define EDV_PROOF_SPACE 7 /* proof generation only: the slot's length is not the proof's; nothing else written */
int edv_merkle_inclusion_offsets(const uint64_t *leaf_index, const uint64_t *tree_size, uint64_t n,
                                 uint64_t store_leaves, uint64_t *proof_off);
int edv_merkle_consistency_offsets(const uint64_t *first, const uint64_t *second, uint64_t n,
                                   uint64_t store_leaves, uint64_t *proof_off);
int edv_merkle_prove_inclusion(const uint8_t *leaf_store, const uint8_t *node_store, uint64_t store_leaves,
                               const uint64_t *leaf_index, const uint64_t *tree_size,
                               const uint64_t *proof_off, uint64_t n, uint8_t *proofs,
                               uint8_t *status, uint8_t *roots, uint8_t *leaf_hashes_out, int device);
int edv_merkle_prove_consistency(const uint8_t *leaf_store, const uint8_t *node_store, uint64_t store_leaves,
                                 const uint64_t *first, const uint64_t *second,
                                 const uint64_t *proof_off, uint64_t n, uint8_t *proofs,
                                 uint8_t *status, uint8_t *old_roots, uint8_t *new_roots, int device);
int edv_merkle_prove_inclusion_dev(const uint8_t *d_leaf_store, const uint8_t *d_node_store, uint64_t store_leaves,
                                   const uint64_t *d_leaf_index, const uint64_t *d_tree_size,
                                   const uint64_t *d_proof_off, uint64_t proof_base, uint64_t n, uint8_t *d_proofs,
                                   uint8_t *d_status, uint8_t *d_roots, uint8_t *d_leaf_hashes_out,
                                   int device, void *stream);
int edv_merkle_prove_consistency_dev(const uint8_t *d_leaf_store, const uint8_t *d_node_store, uint64_t store_leaves,
                                     const uint64_t *d_first, const uint64_t *d_second,
                                     const uint64_t *d_proof_off, uint64_t proof_base, uint64_t n, uint8_t *d_proofs,
                                     uint8_t *d_status, uint8_t *d_old_roots, uint8_t *d_new_roots,
                                     int device, void *stream);

/*
 * Auditing and repairing a hash store (row f-9): what nothing in the
 * reference checks.  Its Ledger.recoverTree (ledger/ledger.py:70-114) trusts a
 * store that has leaves, and CompactMerkleTree.verify_consistency
 * (ledger/compact_merkle_tree.py) compares two counts; a store with one wrong
 * byte passes both and yields wrong proofs from then on.  The store's
 * invariant is local, so it is checked one lane per stored entry:
 *   edv_merkle_audit_nodes   every node of the slice [node_lo, node_lo + count)
 *               of the node store (0-based positions) is SHA-256(0x01 | left |
 *               right) of its two children as they are stored: leaf-store
 *               entries for a node of height 1, earlier node-store entries above
 *   edv_merkle_audit_leaves  leaf-store entry leaf_lo + i is SHA-256(0x00 |
 *               leaf i) for the n leaves at leaves / leaf_off (laid out as
 *               msgs / msg_off everywhere else, readable 8 bytes past the end)
 *   status      NULL, or one EDV_AUDIT_* byte per entry of the slice (0 never
 *               means good)
 *   summary     two words: the number of bad entries, and the lowest bad
 *               position (0-based, in the store; UINT64_MAX: none).  A caller
 *               needs these 16 bytes back, not one byte per node
 * leaf_store / node_store are laid out as for edv_merkle_prove_*:
 * store_leaves x 32 and (store_leaves - popcount(store_leaves)) x 32 bytes.  A
 * node's children come before it, so a slice reads no position at or past its
 * own end and no leaf the append of its last node had not seen; nothing at or
 * past the counts is read.  A flipped bit in a node makes the node and its
 * parent bad; one in a leaf hash makes its parent bad (and, with the leaf
 * bytes given, the leaf).
 * count / n are at most EDV_MERKLE_MAX_LEAVES per call: a larger store is
 * audited in slices.  count = 0 / n = 0 are valid and write nothing but the
 * host forms' initial summary.  EDV_E_ARG with nothing launched or written:
 * count / n above EDV_MERKLE_MAX_LEAVES; store_leaves above 2^62; a slice that
 * reaches past store_leaves - popcount(store_leaves) nodes / store_leaves
 * leaves; NULL summary; with entries to read a NULL store, leaf_off or (unless
 * every leaf is empty) leaves; host offsets that decrease.
 * Device forms: async on `stream` (NULL = library stream, synchronised before
 * returning), offsets absolute minus leaf_base; no context memory, so calls are
 * ordered by their streams alone.  They ADD into the caller's d_summary, which
 * the caller sets to {0, UINT64_MAX} first: several slices accumulate into one
 * summary.  Alignment as edv_merkle_prove_*_dev: d_summary and d_leaf_off on 8
 * bytes, both stores on 16, d_status and d_leaves any.
 * Host forms: set summary to {0, UINT64_MAX} themselves, fill status with
 * EDV_AUDIT_UNCHECKED, synchronous.  THEY COPY THE STORE TO THE DEVICE ON
 * EVERY CALL: for nodes the prefix the slice reads (every node below its end
 * and the leaves below the append of its last node), for leaves the slice's
 * hashes and the leaf bytes.  They stage where the prove and verify host forms
 * stage: counted in edv_context_memory out[2], cut by edv_trim, freed by
 * edv_release; a ledger keeps its store on the device and uses the device forms.
 *
 * edv_merkle_extend_hashed is edv_merkle_extend from the n leaves' hashes
 * instead of their bytes (a store loaded from disk, a catch-up peer that sends
 * hashes): the same passes, the first of which reads its items as every later
 * one does.  node_hashes (NULL: not wanted), new_hashes and root are
 * byte-identical to edv_merkle_extend's on the leaves those hashes belong to;
 * every limit, alignment rule and EDV_E_ARG case is edv_merkle_extend[_dev]'s,
 * with leaf_hashes (n x 32 bytes, a hash buffer; NULL with n > 0 is
 * EDV_E_ARG) in place of leaves / leaf_off.  It shares the extend's scratch
 * and its ordering across streams.  From an empty tree over a store's leaf
 * hashes it rebuilds the node store without the transaction log.
 */
#define EDV_AUDIT_UNCHECKED 0 /* never written by a kernel: what the host forms fill status with first */
#define EDV_AUDIT_OK 1
#define EDV_AUDIT_BAD 2
int edv_merkle_audit_nodes(const uint8_t *leaf_store, const uint8_t *node_store, uint64_t store_leaves,
                           uint64_t node_lo, uint64_t count, uint8_t *status, uint64_t summary[2], int device);
int edv_merkle_audit_leaves(const uint8_t *leaf_store, uint64_t store_leaves, uint64_t leaf_lo,
                            const uint8_t *leaves, const uint64_t *leaf_off, uint64_t n,
                            uint8_t *status, uint64_t summary[2], int device);
int edv_merkle_audit_nodes_dev(const uint8_t *d_leaf_store, const uint8_t *d_node_store, uint64_t store_leaves,
                               uint64_t node_lo, uint64_t count, uint8_t *d_status, uint64_t *d_summary,
                               int device, void *stream);
int edv_merkle_audit_leaves_dev(const uint8_t *d_leaf_store, uint64_t store_leaves, uint64_t leaf_lo,
                                const uint8_t *d_leaves, const uint64_t *d_leaf_off, uint64_t leaf_base, uint64_t n,
                                uint8_t *d_status, uint64_t *d_summary, int device, void *stream);
int edv_merkle_extend_hashed(uint64_t old_size, const uint8_t *old_hashes, const uint8_t *leaf_hashes, uint64_t n,
                             uint8_t *node_hashes, uint8_t *new_hashes, uint8_t *root, int device);
int edv_merkle_extend_hashed_dev(uint64_t old_size, const uint8_t *d_old_hashes, const uint8_t *d_leaf_hashes, uint64_t n,
                                 uint8_t *d_node_hashes, uint8_t *d_new_hashes, uint8_t *d_root,
                                 int device, void *stream);

/*
 * Catch-up (row f-10): verify and apply the replies of a catch-up in one call.
 * A joining node (plenum/common/ledger_manager.py:505-609 hasValidCatchupReplies
 * / _add_txn) builds a temporary tree over each reply's transactions, walks one
 * consistency proof from it to the catch-up target and then appends the
 * transactions one by one: every transaction is hashed twice, one reply at a
 * time.  Here the n leaves are the transactions of `replies` in-order replies,
 * laid out as for edv_merkle_extend; the extend's passes hash them once, and
 * one lane per reply folds the root of the tree at the reply's end and walks
 * the reply's proof to (final_size, final_root).
 *
 *   reply_end   replies words: leaves of the call in replies 0 .. k (never
 *               falling; an empty reply repeats the end before it; the last is n)
 *   final_size / final_root   the catch-up target (the reference's catchUpTill)
 *   proofs / proof_off   packed 32-byte entries and replies + 1 offsets in
 *               entries, as for edv_merkle_verify_consistency
 *   leaf_hashes / node_hashes   as edv_merkle_extend's, NULL: not wanted (the
 *               lanes read them either way: the device form keeps them in
 *               context scratch then)
 *   reply_roots NULL, or replies x 32 bytes: the tree head at each reply's end
 *               (zeros where the status is EDV_PROOF_RANGE)
 *   status      replies bytes: EDV_PROOF_RANGE where reply_end[k] > n or
 *               old_size + reply_end[k] > final_size, else what
 *               edv_merkle_verify_consistency gives for (old_size + reply_end[k],
 *               final_size, that head, final_root, proof k)
 *
 * The replies a caller may apply are the leading ones with EDV_PROOF_OK: a
 * status after the first failure is computed over rejected transactions.
 * EDV_E_ARG (host form) before anything is launched or written: every case of
 * edv_merkle_extend; replies = 0 with n > 0; replies > n + 1; reply_end
 * falling or not ending at n; proof_off falling; final_root, status, reply_end
 * or proof_off NULL.  The device form's arrays live on the device and are not
 * checked: an end past n is EDV_PROOF_RANGE, other inconsistencies are the
 * caller's.  Alignment: hash buffers (d_final_root and d_proofs included) on
 * 16 bytes, d_leaf_off, d_reply_end and d_proof_off on 8.  The device form
 * shares the extend's scratch and its ordering across streams; the host form
 * fills status with EDV_PROOF_UNVERIFIED, stages where the extend and verify
 * host forms stage (edv_context_memory out[2], edv_trim, edv_release) and is
 * synchronous.
 */
int edv_merkle_catchup(uint64_t old_size, const uint8_t *old_hashes, const uint8_t *leaves, const uint64_t *leaf_off,
                       uint64_t n, const uint64_t *reply_end, uint64_t replies, uint64_t final_size,
                       const uint8_t *final_root, const uint8_t *proofs, const uint64_t *proof_off,
                       uint8_t *leaf_hashes, uint8_t *node_hashes, uint8_t *reply_roots, uint8_t *status, int device);
int edv_merkle_catchup_dev(uint64_t old_size, const uint8_t *d_old_hashes, const uint8_t *d_leaves,
                           const uint64_t *d_leaf_off, uint64_t leaf_base, uint64_t n, const uint64_t *d_reply_end,
                           uint64_t replies, uint64_t final_size, const uint8_t *d_final_root, const uint8_t *d_proofs,
                           const uint64_t *d_proof_off, uint64_t proof_base, uint8_t *d_leaf_hashes,
                           uint8_t *d_node_hashes, uint8_t *d_reply_roots, uint8_t *d_status, int device, void *stream);

/*
 * Pipelined submission of device-resident batches (a continuous stream of
 * client batches, e.g. one per Node prod): enqueues the batch and returns
 * without waiting.  Consecutive submissions alternate between two internal
 * state sets, with the prep kernel (checks, decompression, SHA-512, table) of
 * batch k+1 on one library stream and the main kernel (the joint walk) of
 * batch k on another, so both can run on the SIMDs at once (measured on
 * MI355X at C2 after round 5's kernels it is slower than sequential batches,
 * 91.8-92.3 M against 98.3-98.6 M verifies/s: profiles/r05/ab_modes_s16.jsonl;
 * with EDV_FLAG_SPLIT_PREP it pays at C4's long messages).  Work
 * already queued on the library stream (edv_stream) is ordered before the
 * batch; inputs must stay unchanged and each batch's d_accept must not be
 * reused or read until edv_pipeline_sync(device) returns.  Same verdicts as
 * edv_verify_batch_dev.
 */
int edv_verify_batch_dev_pipelined(const uint8_t *d_sigs, const uint8_t *d_pks, const uint8_t *d_msgs,
                                   const uint64_t *d_msg_off, uint64_t msg_base, uint64_t n, uint8_t *d_accept,
                                   int device, uint32_t flags);
/* Wait until every pipelined batch submitted on `device` has its verdicts. */
int edv_pipeline_sync(int device);

/* (Kernel timing and fault injection are not part of this ABI: they live in
 * the benchmark build libedv_measure.so, include/edv_measure.h.) */

/* Signatures per prep/main kernel pair on `device` (0 = default 2^18; rounded
 * down to a multiple of 256).  Tuning/testing knob: verdicts never depend on it. */
int edv_set_chunk(int device, uint64_t chunk);

/* Message slices of a synchronous edv_verify_batch shard that fits one chunk
 * (1..8; 0 = default: one per 65,536 requests, so one at C2): the messages are
 * copied in that many slices by request, and each slice's SHA-512 / scalar
 * side runs as soon as it has landed, so only the last slice's remains after
 * the copy.  Tuning knob: verdicts never depend on it. */
int edv_set_host_slices(int device, int slices);

/* The latency path: every batch of at most max_requests requests (default and
 * at most 16,384; 0 = never) on `device` -- synchronous, asynchronous and
 * device-resident calls alike -- runs as ONE kernel launch with several lanes
 * per signature (edv_quad.hip; each point doubling and addition split over a
 * quad of lanes, operands exchanged by DPP): up to 4,096 requests sixteen lanes
 * (per scalar a doubler wave running the 16^j P chain and an adder wave
 * summing per-digit buckets), above that eight (two table walks).  Below one
 * wave per SIMD the batch kernels (one signature per lane) take a lane's whole
 * serial chain whatever n is; this path divides that chain instead (0.18-0.21
 * ms of kernel on MI355X against ~0.55 ms).  Tuning knob: verdicts never
 * depend on it. */
int edv_set_latency_path(int device, uint64_t max_requests);

/* SHA-512 length buckets of the device paths (a counting sort of each chunk by
 * block count, so a wave of the prep kernel hashes equally long messages):
 * 0 = never (a caller whose messages all have one length saves three small
 * launches per chunk), 1 = always, 2 = auto (default: on for device-resident
 * batches; the host path buckets only when lengths differ).  Tuning knob:
 * verdicts never depend on it. */
int edv_set_length_buckets(int device, int mode);

/*
 * Batch Ed25519 signing for synthetic load generation,
 * device-resident: seeds n x 32 B -> pks n x 32 B and detached sigs n x 64 B
 * over the given messages; RFC 8032 deterministic, byte-identical to libsodium
 * crypto_sign_seed_keypair + crypto_sign_detached.  Counterpart of the
 * reference's client-side signing (stp_core/crypto/nacl_wrappers.py:162-176
 * SigningKey.sign, plenum/common/signer_did.py:122-129).  Async on `stream`
 * (NULL = library stream, synchronised before returning).
 */
int edv_sign_batch_dev(const uint8_t *d_seeds, const uint8_t *d_msgs, const uint64_t *d_msg_off, uint64_t msg_base,
                       uint64_t n, uint8_t *d_pks, uint8_t *d_sigs, int device, void *stream);

/* The library's own HIP stream of `device` (so callers can enqueue several
 * edv_*_dev calls asynchronously on it) and a wait for everything on it. */
int edv_stream(int device, void **out);
int edv_sync(int device);

/* Number of visible gfx950 devices (0 if none).  EDV_VIRTUAL_DEVICES=k (a
 * testing knob) presents k logical devices mapped round-robin onto the physical
 * ones, each with its own context, so the multi-device path runs on one GPU. */
int edv_device_count(void);

/*
 * Device placement on a multi-GPU node.  edv_verify_batch / edv_sha256_batch
 * split a batch only into shards of at least 65,536 requests (one wave per SIMD
 * of a whole MI355X: a smaller shard takes as long as a full one; EDV_MIN_SHARD
 * overrides), so a Node-sized batch (a prod of a few hundred requests, or one
 * Verifier.verify) runs whole on ONE device, on the calling thread, and no
 * other device is initialised.  Devices are chosen the same way for one shard
 * and for 2..7 shards of a mid-sized batch: initialised devices with nothing
 * running first, then devices not yet initialised (order starting at pid mod
 * devices), then the least-loaded (load = synchronous calls placed there +
 * asynchronous batches still running on the GPU, waited for or not); concurrent
 * calls see each other's choices.  edv_pick_device returns that choice for one
 * shard; the Node's asynchronous path asks it for the device of each
 * submission (edv_verify_batch_async takes the device explicitly).
 * edv_pick_device returns that device's index (or a negative EDV_E_* code);
 * edv_context_count: devices whose context (streams, scratch, [S]B tables) exists.
 * Reference: the per-request call being placed, nacl_wrappers.py:232-242, made
 * per prod (plenum/server/node.py:1026-1049, stp_core/config.py:28).
 */
int edv_pick_device(uint32_t device_mask);

/*
 * Accept bytes -> accept bitmask on the device: d_bits[i / 8] bit (i % 8) =
 * (d_accept[i] != 0), ceil(n / 8) bytes (numpy.packbits(..., bitorder="little")).
 * What a multi-GPU run gathers to the host: N/8 bytes per shard.
 * Asynchronous on `stream` if given, else synchronous on the library stream;
 * either way ordered after every verify already launched on `device` (any
 * stream, pipelined submissions included).
 */
int edv_pack_bits_dev(const uint8_t *d_accept, uint64_t n, uint8_t *d_bits, int device, void *stream);
int edv_context_count(void);

/*
 * Device memory the library holds for `device` in this process, in bytes:
 * out[0] total, out[1] the [S]B tables (shared by the logical devices of one
 * GPU), out[2] chunk scratch of the ordinary paths and the Merkle-tree
 * extension's scratch and staging, out[3] the asynchronous
 * slots (inputs and small-batch scratch), out[4] the pipelined state sets,
 * out[5] input buffers of the synchronous path, out[6] the signer's comb
 * table.  Scratch grows with the largest batch seen (up to one chunk), so a
 * Node that verifies prods of a few hundred requests holds a few hundred MB;
 * 0 for a device whose context does not exist yet.  (What a Node process
 * costs a GPU it shares with other Node processes: scripts/start_plenum_node
 * runs one Node per process.)
 */
int edv_context_memory(int device, uint64_t out[7]);

/*
 * ---- Context lifecycle.  A Node is one long-lived process (scripts/
 * start_plenum_node; several may share a GPU), and its first client request is
 * authenticated by the same call as every later one (plenum/server/
 * client_authn.py:83-113).  Without the calls below a device's context (HIP
 * runtime, streams, the [S]B table set, scratch) is created inside the first
 * verify, only ever grows, and lives until the process exits.  None of them
 * changes a verdict or a default; a process that never calls them behaves as
 * before.  `device` is a logical device index as everywhere else; they return
 * EDV_E_NODEV for one that does not exist.
 */

/*
 * Which [S]B table set the batches of `device` run against; takes effect with
 * the next batch, builds nothing and frees nothing by itself (edv_trim frees).
 * Starts as the EDV_SB_TABLES environment variable says (auto / compact /
 * large; default auto) and survives edv_release.
 *   EDV_TABLES_AUTO     the compact set (64 MiB); the large one (3 GiB) is built
 *                       by the first batch of at least 65,536 requests and then
 *                       used for every batch, small ones included
 *   EDV_TABLES_COMPACT  always the compact set (built if the context holds only
 *                       the large one): what a Node verifying prods wants
 *   EDV_TABLES_LARGE    always the large set (built by the next batch if the
 *                       context holds only the compact one)
 * EDV_E_ARG for any other value.  Clears the failed flag of edv_table_state.
 */
#define EDV_TABLES_AUTO 0
#define EDV_TABLES_COMPACT 1
#define EDV_TABLES_LARGE 2
int edv_set_table_policy(int device, int policy);
/*
 * out[0] the policy, out[1] / out[2] bytes of the compact / large set this
 * context holds (0: not held; a GPU's sets are shared by its logical devices
 * and freed when the last context holding one drops it), out[3] 1 if a build
 * of the large set has failed and is not being retried.  That flag is sticky:
 * the batch that hit the failure runs on the compact set and returns 0 with
 * the allocation's error left in edv_last_error, and later batches use the
 * compact set without another 3 GiB allocation, until edv_set_table_policy,
 * edv_trim or edv_release clears it.  Works before the context exists (zeros).
 */
int edv_table_state(int device, uint64_t out[4]);

/*
 * Power-on known-answer test: do the kernels on this GPU give libsodium's
 * verdicts?  (The reference trusts libsodium's own build-time tests; a Node
 * calls this before it authenticates its first request.)  The cases are part of
 * the library (RFC 8032 section 7.1 vectors 1-3; a rejecting case for each
 * strictness rule -- S >= L, small-order R, non-canonical A, small-order A, A
 * off the curve --, a valid signature over a changed message, a mixed-order A
 * that libsodium accepts) and run through the synchronous path of
 * edv_verify_batch, tiled to the smallest batch that takes each family:
 *   EDV_SELFTEST_RTL       16 requests, the right-to-left latency kernel
 *   EDV_SELFTEST_TWO_WALK  4,097 requests, the two-walk latency kernel
 *   EDV_SELFTEST_BATCH     256 requests on the prep + main kernels (the latency
 *                          path bypassed for this call only; the setting of
 *                          edv_set_latency_path is neither read nor changed)
 * on the table set the device's policy picks for such a batch (so never the
 * large set unless the policy or an earlier batch asked for it).  Creates the
 * context if needed.  0 when every verdict matches; EDV_E_SELFTEST otherwise,
 * with the family and the case in edv_last_error; EDV_E_ARG for an empty or
 * unknown mask; the synchronous path's other errors as they are.
 */
#define EDV_SELFTEST_RTL 1u
#define EDV_SELFTEST_TWO_WALK 2u
#define EDV_SELFTEST_BATCH 4u
int edv_self_test(int device, uint32_t families);

/*
 * Start-up step of a Node (in place of paying for all of it inside the first
 * prod's verify): creates the context of `device`; builds the table set(s) the
 * policy uses for batches of up to max_batch requests; grows scratch, input
 * buffers and pinned staging of the synchronous path -- and of every slot of
 * the asynchronous path with EDV_PREPARE_ASYNC -- to what such batches need, by
 * running warm-up batches of max_batch requests (and of 4,096 and the latency
 * path's limit where those are smaller: one per kernel family) with 512-byte
 * messages, from pageable and from page-locked memory; then runs edv_self_test
 * for the families such batches take (RTL up to 4,096 requests, RTL and
 * TWO_WALK up to the device's latency-path limit, all three above it).  After
 * it returns 0, a verify of at most max_batch requests whose messages average
 * at most 512 bytes allocates and builds nothing.  The warm-up batches use
 * tickets of the asynchronous path's ledger; a caller's ticket whose slot they
 * reuse is handed over as a later submission would.  Call it again after
 * changing a setting it depends on (policy, chunk, latency path).
 * EDV_E_ARG for max_batch 0 or above 2^20 or unknown flags; EDV_E_OOM /
 * EDV_E_HIP from allocations and launches (a failed build of the large set
 * included); EDV_E_SELFTEST as edv_self_test.
 */
#define EDV_PREPARE_ASYNC 1u
int edv_prepare(int device, uint64_t max_batch, uint32_t flags);

/*
 * Gives memory back without giving up the context (a Node after a catch-up
 * burst of large batches).  Waits for everything queued on the context's
 * streams, then frees every scratch set, asynchronous slot buffer, pinned
 * staging and input buffer larger than a batch of keep_batch requests needs
 * (messages of up to 4,096 bytes allowed for; 0 frees all of them) and drops
 * the table sets the policy would not pick for a batch of keep_batch in a fresh
 * context: under EDV_TABLES_AUTO with keep_batch below 65,536 the large set,
 * which a later batch of 65,536 builds again.  What is freed regrows by use.
 * EDV_E_BUSY, with nothing changed, while an asynchronous batch of this device
 * has not been handed over by edv_wait_async / edv_query_async or pipelined
 * batches have not been synced (edv_pipeline_sync): those still own caller
 * buffers.  Nothing happens for a device without a context.  Clears the failed
 * flag of edv_table_state.
 */
int edv_trim(int device, uint64_t keep_batch);

/*
 * Destroys the context of `device` (a Node leaving a GPU, or rebuilding its
 * context after an EDV_E_HIP): same wait and EDV_E_BUSY rule as edv_trim, then
 * every stream, event, device and pinned buffer goes and the table sets are
 * dropped; edv_context_count falls by one and edv_context_memory reports
 * zeros.  The device's settings (edv_set_*) are kept, and so is the ticket
 * count of the asynchronous path: a ticket issued before the release still
 * answers as settled (or failed), never as a later batch.  Device memory from
 * edv_dev_alloc and streams obtained from edv_stream are the caller's to free
 * and forget first.  The next call on the device creates a fresh context.
 */
int edv_release(int device);

/*
 * The shard split edv_verify_batch uses (host only, no GPU needed): bounds[0..g]
 * with shard k = requests [bounds[k], bounds[k+1]).  Equal request counts
 * (n*k/g) when every message has the same SHA-512 block count; otherwise equal
 * estimated cost, sum over the shard of (40 + SHA-512 blocks of R||A||M), where
 * 40 blocks is the fixed per-verify work of SURVEY.md section 8d's W(m).
 */
int edv_shard_split(const uint64_t *msg_off, uint64_t n, uint32_t g, uint64_t *bounds);

/* Pinned (page-locked, portable) host memory: inputs packed here are copied to
 * the device by DMA without the staging memcpy. */
int edv_host_alloc(uint64_t bytes, void **out);
int edv_host_free(void *p);

/* Device memory helpers so a host without PyTorch can stage inputs. */
int edv_dev_alloc(int device, uint64_t bytes, void **out);
int edv_dev_free(int device, void *p);
int edv_h2d(int device, void *dst, const void *src, uint64_t bytes);
int edv_d2h(int device, void *dst, const void *src, uint64_t bytes);

/* Library/version string, e.g. "edv 0.1.0 gfx950". */
const char *edv_version(void);

/* Text of the last error raised on the calling thread ("" if none). */
const char *edv_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* EDV_H */

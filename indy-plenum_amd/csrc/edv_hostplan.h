// edv_hostplan.h -- the arithmetic of the host paths (edv_runtime.hip): the
// packed layout of a batch, the single-copy test, slices and sub-batches of a
// shard, how far buffers grow and what a trim keeps, the Merkle buffers' sizes.
// Plain C++, no HIP types: libedv_hostcheck.so and tools/ubsan_hostplan.cpp
// check what the library runs.
#pragma once
#include <stdint.h>
#include <array>
#include "edv_merkle.h"

namespace edv {

// Message slices of the synchronous field-ordered path (edv_set_host_slices):
// the hash side of slice k runs while slice k+1 copies.
constexpr int kSlices = 8;
constexpr uint64_t kMinSliceReqs = 65536;
constexpr uint64_t kTrimMsgBytes = 4096;  // message bytes per request of keep_batch a buffer may hold and survive edv_trim
constexpr uint64_t kReadSlack = 64;       // bytes readable past the last message (the kernels read whole aligned words)
constexpr uint64_t kSpanGapMax = 4096;    // padding a single-copy span may carry between its three regions

// One block per batch of n requests: signatures (at 0) | keys | offsets |
// messages; signatures and keys stay 16-byte aligned, offsets 8-byte aligned.
struct PackedLayout {
  uint64_t pks, off, msgs;  // byte offsets of the parts
  uint64_t bytes, padded;   // ... of the end of the messages, and of the read slack behind them
};
inline PackedLayout packed_layout(uint64_t n, uint64_t mbytes) {
  const uint64_t msgs = 96 * n + 8 * (n + 1);
  return {64 * n, 96 * n, msgs, msgs + mbytes, msgs + mbytes + kReadSlack};
}

// Signatures, keys and offsets of n requests at host addresses as, ap, ao go
// to the device in ONE copy of `span` bytes from `as` when they lie in that
// order without overlap, with little padding, aligned relative to the
// signatures: the device block then has the keys at gp, the offsets at go.
// Otherwise gp, go and span are the packed layout's (three copies, one block).
struct OneSpan {
  bool one;
  uint64_t gp, go, span;
};
inline OneSpan one_span(uint64_t as, uint64_t ap, uint64_t ao, uint64_t n) {
  const uint64_t gp = ap - as, go = ao - as, span = go + 8 * (n + 1);
  if (ap >= as + 64 * n && ao >= ap + 32 * n && span <= 104 * n + 8 + kSpanGapMax && gp % 16 == 0 && go % 8 == 0)
    return {true, gp, go, span};
  const PackedLayout l = packed_layout(n, 0);
  return {false, l.pks, l.off, l.msgs};
}

// Signatures a chunk state set holds once grown to `need`: powers of two from 4,096, at most `limit` (the chunk).
inline uint64_t chunk_capacity(uint64_t need, uint64_t limit) {
  uint64_t c = 4096;
  while (c < need) c <<= 1;
  return c <= limit ? c : (limit > need ? limit : need);
}
// What a pinned buffer asked for `bytes` is allocated with (headroom: message bytes vary from call to call).
inline uint64_t pinned_capacity(uint64_t bytes) { return bytes + bytes / 4 + 4096; }

// The field path's K message slices of a shard, slice k = requests [rb[k],
// rb[k+1]), every bound but the last a multiple of `block`: one per
// kMinSliceReqs requests (below that a slice's hash side takes a whole wave's
// latency, so smaller slices only add copy gaps: profiles/r05/trace_sync_s1.json),
// at most kSlices; host_slices > 0 overrides; a bucketed shard is one slice.
inline int field_slices(uint64_t n, int host_slices, bool bucketed, uint64_t block, uint64_t rb[kSlices + 1]) {
  uint64_t K = bucketed ? 1 : (host_slices > 0 ? uint64_t(host_slices) : n / kMinSliceReqs);
  if (K < 1) K = 1;
  if (K > uint64_t(kSlices)) K = kSlices;
  if (K * block > n) K = n / block > 1 ? n / block : 1;
  for (uint64_t k = 0; k <= K; k++) rb[k] = k == K ? n : (n * k / K) / block * block;
  return int(K);
}

// A shard larger than one chunk: nsub sub-batches of P requests alternate over
// Q streams, stream q on scratch slots [q pmax, (q + 1) pmax); else one sub-batch.
struct SubSplit {
  uint64_t Q, pmax, P, nsub;
};
inline SubSplit sub_split(uint64_t n, uint64_t chunk, uint64_t block) {
  const uint64_t Q = (n > chunk && chunk >= 2 * block) ? 2 : 1, pmax = chunk / Q;
  uint64_t P = ((n + Q - 1) / Q + 63) / 64 * 64;
  if (P > pmax) P = pmax;
  return {Q, pmax, P, P ? (n + P - 1) / P : 0};
}

// What edv_trim keeps: a buffer larger than a batch of `keep` requests with
// kTrimMsgBytes of message each needs is freed (keep == 0: every buffer).
struct TrimLimits {
  uint64_t slots;                      // chunk state sets, in signatures (what such a batch grows a set to)
  uint64_t sigs, pks, acc, dig;
  uint64_t msgs, off, slot_off;        // the context's messages and offsets (a window per sub-batch); a slot's offsets
  uint64_t packed, blob;               // signatures | keys | offsets in one span; ... and the messages
  uint64_t stage, acc_host, dig_host;  // pinned buffers, with their headroom
};
inline TrimLimits trim_limits(uint64_t keep, uint64_t chunk) {
  const uint64_t k = keep, msgs = k * kTrimMsgBytes + kReadSlack;  // at keep == 0 too: a buffer of the bare slack stays
  if (!k) return {0, 0, 0, 0, 0, msgs, 0, 0, 0, 0, 0, 0, 0};
  const uint64_t packed = 104 * k + 8 + kSpanGapMax, blob = packed + msgs;
  return {chunk_capacity(k < chunk ? k : chunk, chunk), 64 * k, 32 * k, k, 32 * k, msgs,
          8 * (k + k / (chunk / 2 ? chunk / 2 : 1) + 2), 8 * (k + 1), packed, blob,
          pinned_capacity(blob), pinned_capacity(k), pinned_capacity(32 * k)};
}

// ---- the Merkle buffers of a context (edv_runtime.hip: MerkleBufs).  mk_*: the
// extension and the batched append.  mk_roots (the tile roots the passes hand
// on) and mk_fleafh / mk_fnodeh (the hashes the per-leaf fold reads) are scratch
// of every stream; the others are the host form's staging: leaf bytes, offsets,
// old entries | new entries | root, leaf and node hashes, per-leaf roots, packed
// paths.  mv_*: the host verify forms' staging: leaf bytes or hashes, every
// 64-bit array in turn, given roots, proof entries, computed roots | statuses.
// mp_*: the host prove forms' staging (row f-8): the prefix of the leaf store
// and of the node store the call reads, every 64-bit array in turn, the proof
// entries, roots (consistency: old | new) | leaf hashes | statuses.  The
// earlier buffers keep their places: kMerkleBufsV7 of them.
enum MerkleBuf {
  mk_roots, mk_leaves, mk_off, mk_hashes, mk_leafh, mk_nodeh, mk_fleafh, mk_fnodeh, mk_aroots, mk_paths,
  mv_leaves, mv_words, mv_roots, mv_proofs, mv_out,
  mp_leaves, mp_nodes, mp_words, mp_proofs, mp_out, kMerkleBufs
};
constexpr int kMerkleBufsV7 = mp_leaves;
using MerkleSizes = std::array<uint64_t, kMerkleBufs>;  // bytes, by MerkleBuf
constexpr uint64_t kMerkleHashesBytes = 32 * (2 * kMerkleMaxHashes + 2);  // mk_hashes: old entries | new entries | root
// What one extend or append of n leaves (mbytes of them) onto old_size needs of
// each (0: not touched); want_*: the outputs asked for.  The per-leaf fold reads
// the leaf and node hashes, so with roots or paths wanted they are kept anyway:
// staged (host form), in the fold scratch (device form without a buffer for them).
inline MerkleSizes merkle_extend_needs(uint64_t old_size, uint64_t n, uint64_t mbytes, bool host_form, bool want_leaf,
                                       bool want_node, bool want_roots, bool want_paths) {
  const uint64_t nodes = merkle_node_count(old_size + n) - merkle_node_count(old_size);
  const bool per_leaf = n != 0 && (want_roots || want_paths);
  MerkleSizes s = {};
  s[mk_roots] = 32 * merkle_scratch_hashes(old_size, old_size + n);
  if (host_form) {
    s[mk_leaves] = mbytes + 64;
    s[mk_off] = 8 * (n + 1);
    s[mk_hashes] = kMerkleHashesBytes;
    s[mk_leafh] = want_leaf || per_leaf ? 32 * n : 0;
    s[mk_nodeh] = want_node || per_leaf ? 32 * nodes : 0;
    s[mk_aroots] = want_roots ? 32 * n : 0;
    s[mk_paths] = want_paths ? 32 * merkle_path_entries(old_size, n) : 0;
  } else {
    s[mk_fleafh] = per_leaf && !want_leaf ? 32 * n : 0;
    s[mk_fnodeh] = per_leaf && !want_node ? 32 * nodes : 0;
  }
  return s;
}
// ... and one host verify call of n proofs of `entries` entries in all; lbytes:
// the leaves' bytes (inclusion by leaf hash: 32 n).  mv_proofs is never empty.
inline MerkleSizes merkle_verify_needs(bool inclusion, uint64_t n, uint64_t lbytes, uint64_t entries, bool want_computed) {
  const uint64_t rbytes = inclusion ? 32 * n : 64 * n;  // one root per proof, or two
  MerkleSizes s = {};
  s[mv_leaves] = inclusion ? lbytes + kReadSlack : 0;
  s[mv_words] = 8 * (4 * n + 2);
  s[mv_roots] = rbytes;
  s[mv_proofs] = entries ? 32 * entries : 32;
  s[mv_out] = (want_computed ? rbytes : 0) + n;
  return s;
}
// What edv_trim lets each keep (t: trim_limits of `keep`): what extending any tree by `keep` leaves of kTrimMsgBytes
// (paths of at most kMerkleMaxHashes entries) or verifying as many proofs of at most 64 entries can need (mv_out: 64
// computed bytes and the status, rounded up to 16); for the prove forms (mp_*) as many proofs of 64 entries: the
// entries, as many store hashes of either kind as the lanes can read, two roots, a leaf hash and the status.
inline MerkleSizes merkle_trim_limits(uint64_t keep, const TrimLimits& t) {
  const uint64_t k = keep, h = 32 * k, msgs = k ? t.msgs : 0;
  return {k ? 32 * (k / (kMerkleT - 1) + 16) : 0, msgs, t.slot_off, k ? kMerkleHashesBytes : 0, h, h, h, h, h,  // MerkleBuf's order
          h * kMerkleMaxHashes, msgs, k ? 8 * (4 * k + 2) : 0, 64 * k, 64 * h, 80 * k,
          64 * h, 64 * h, k ? 8 * (3 * k + 1) : 0, 64 * h, 112 * k};
}

// ---- proof generation (row f-8).  What the host forms stage of the store: the
// prefix the largest valid tree size reads, in leaves (0: every pair is RANGE).
// size_of_pair: the pair's tree size (tree_size[i] / second[i]) if the pair is
// in range, else 0.
inline uint64_t merkle_prove_inclusion_size(uint64_t idx, uint64_t size, uint64_t store_leaves) {
  return idx < size && size <= store_leaves ? size : 0;
}
inline uint64_t merkle_prove_consistency_size(uint64_t first, uint64_t second, uint64_t store_leaves) {
  return first != 0 && first <= second && second <= store_leaves ? second : 0;
}
inline uint64_t merkle_prove_prefix(bool consistency, const uint64_t* a, const uint64_t* b, uint64_t n,
                                    uint64_t store_leaves) {
  uint64_t top = 0;
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t s = consistency ? merkle_prove_consistency_size(a[i], b[i], store_leaves)
                                   : merkle_prove_inclusion_size(a[i], b[i], store_leaves);
    if (s > top) top = s;
  }
  return top;
}
// The slots a batch needs, packed: n + 1 offsets in entries from 0; a pair that
// would get RANGE takes none.
inline void merkle_prove_offsets(bool consistency, const uint64_t* a, const uint64_t* b, uint64_t n,
                                 uint64_t store_leaves, uint64_t* proof_off) {
  uint64_t at = 0;
  for (uint64_t i = 0; i < n; i++) {
    proof_off[i] = at;
    if (consistency ? merkle_prove_consistency_size(a[i], b[i], store_leaves) != 0
                    : merkle_prove_inclusion_size(a[i], b[i], store_leaves) != 0)
      at += consistency ? merkle_consistency_length(a[i], b[i]) : merkle_inclusion_length(a[i], b[i]);
  }
  proof_off[n] = at;
}
// Offsets inside mp_out: the first roots, the second (consistency: the new
// roots; inclusion: the leaf hashes), the statuses.  A part not wanted is left
// out, so the statuses follow whatever is there.
struct MerkleProveOut {
  uint64_t first, second, status, bytes;  // byte offsets; first / second are valid where wanted
};
inline MerkleProveOut merkle_prove_out(uint64_t n, bool want_first, bool want_second) {
  const uint64_t f = 0, s = want_first ? 32 * n : 0, st = s + (want_second ? 32 * n : 0);
  return {f, s, st, st + n};
}
// What one host prove call of n proofs over `entries` slot entries needs:
// `prefix` leaves of the store (merkle_prove_prefix).  mp_proofs is never empty.
inline MerkleSizes merkle_prove_needs(uint64_t n, uint64_t prefix, uint64_t entries, bool want_first, bool want_second) {
  MerkleSizes s = {};
  s[mp_leaves] = prefix ? 32 * prefix : 32;
  s[mp_nodes] = prefix > 1 ? 32 * merkle_node_count(prefix) : 32;
  s[mp_words] = 8 * (3 * n + 1);
  s[mp_proofs] = entries ? 32 * entries : 32;
  s[mp_out] = merkle_prove_out(n, want_first, want_second).bytes;
  return s;
}

// ---- auditing a stored tree (row f-9).  The host forms stage in the buffers
// the prove forms stage in (and the leaf bytes where the verify forms put
// theirs): no buffer of their own, so edv_trim and edv_release cut and free
// them as before.  mp_out: the summary's two words, then the statuses.
constexpr uint64_t kAuditSummaryBytes = 16;
// The store prefixes a node slice [node_lo, node_lo + count) reads, count > 0:
// every node below its end, and the leaves below the append that wrote its
// last node (merkle_node_children: children come before their parent).
struct MerkleAuditPrefix {
  uint64_t leaves, nodes;
};
inline MerkleAuditPrefix merkle_audit_nodes_prefix(uint64_t node_lo, uint64_t count) {
  uint64_t s;
  int h;
  merkle_store_node_at(node_lo + count - 1, &s, &h);
  return {s, node_lo + count};
}
inline MerkleSizes merkle_audit_nodes_needs(uint64_t node_lo, uint64_t count) {
  MerkleSizes s = {};
  if (!count) return s;
  const MerkleAuditPrefix p = merkle_audit_nodes_prefix(node_lo, count);
  s[mp_leaves] = 32 * p.leaves;
  s[mp_nodes] = 32 * p.nodes;
  s[mp_out] = kAuditSummaryBytes + count;
  return s;
}
// ... and a leaf slice of n leaves, lbytes of them: the n stored hashes, the
// leaf bytes, the n + 1 offsets.
inline MerkleSizes merkle_audit_leaves_needs(uint64_t n, uint64_t lbytes) {
  MerkleSizes s = {};
  if (!n) return s;
  s[mp_leaves] = 32 * n;
  s[mv_leaves] = lbytes + kReadSlack;
  s[mp_words] = 8 * (n + 1);
  s[mp_out] = kAuditSummaryBytes + n;
  return s;
}
// ... and an extend from n leaf hashes (host form): the extend's staging
// without leaf bytes and offsets; mk_leafh holds the hashes that come in.
inline MerkleSizes merkle_extend_hashed_needs(uint64_t old_size, uint64_t n, bool host_form, bool want_node) {
  MerkleSizes s = merkle_extend_needs(old_size, n, 0, host_form, host_form, want_node, false, false);
  s[mk_leaves] = s[mk_off] = 0;
  return s;
}

// ---- catch-up (row f-10).  One call of n leaves (mbytes of them) in `replies`
// replies with `entries` proof entries in all.  No buffer of its own: the
// leaves, offsets and old entries stage where the extend's do, the reply ends
// and proof offsets (mv_words: ends, then offsets), the target root
// (mv_roots), the proof entries (mv_proofs, never empty) and the outputs
// (mv_out: the reply roots if wanted, then the statuses) where the verify
// forms' do.  The lanes read the leaf and node hashes, so they are kept
// whether wanted or not: staged (host form), in the fold scratch (device form
// without a buffer for them).  The passes write the new tree's entries, which
// no catch-up output takes: they go to the front of mk_fnodeh in both forms.
constexpr uint64_t kCatchupNewBytes = 32 * kMerkleMaxHashes;
inline MerkleSizes merkle_catchup_needs(uint64_t old_size, uint64_t n, uint64_t mbytes, uint64_t replies,
                                        uint64_t entries, bool host_form, bool want_leaf, bool want_node,
                                        bool want_roots) {
  const uint64_t nodes = merkle_node_count(old_size + n) - merkle_node_count(old_size);
  MerkleSizes s = {};
  s[mk_roots] = 32 * merkle_scratch_hashes(old_size, old_size + n);
  s[mk_fnodeh] = kCatchupNewBytes + (!host_form && !want_node ? 32 * nodes : 0);
  if (host_form) {
    s[mk_leaves] = mbytes + 64;
    s[mk_off] = 8 * (n + 1);
    s[mk_hashes] = kMerkleHashesBytes;
    s[mk_leafh] = 32 * n;
    s[mk_nodeh] = 32 * nodes;
    s[mv_words] = 8 * (2 * replies + 1);
    s[mv_roots] = 32;
    s[mv_proofs] = entries ? 32 * entries : 32;
    s[mv_out] = (want_roots ? 32 * replies : 0) + replies;
  } else {
    s[mk_fleafh] = want_leaf ? 0 : 32 * n;
  }
  return s;
}

}  // namespace edv

// edv_merkle.h -- extending a compact RFC 6962 Merkle tree by a batch of leaves
// (SURVEY.md section 8f row f-5), and what each of the appends returns: the
// root after it and its audit path (row f-6), and the checking of such proofs:
// audit paths and consistency proofs, a batch at a time (row f-7, at the end of
// this file; ledger/merkle_verifier.py MerkleVerifier), and the making of them
// from the stored hashes (row f-8, after it; CompactMerkleTree.inclusion_proof
// / consistency_proof / merkle_tree_hash(0, n)), and the auditing of those
// stored hashes, entry by entry (row f-9, after that), and the verifying and
// applying of catch-up replies in one call (row f-10, at the very end).
//
// Replaces, per batch of transactions:
//   ledger/ledger.py:145-148              Ledger._addToTree (one append per txn)
//   ledger/compact_merkle_tree.py:155-191 CompactMerkleTree.append / extend
//   ledger/tree_hasher.py:20-28           hash_leaf = sha256(0x00 | leaf),
//                                         hash_children = sha256(0x01 | l | r)
//
// A tree of `size` leaves is (size, hashes): the roots of the full subtrees of
// the binary decomposition of size, largest first.  Extending `old` leaves by n
// gives, for every height h >= 1, the new aligned blocks k in
// [old >> h, new >> h) (block k covers leaves [k 2^h, (k + 1) 2^h)); the only
// child of a new block that is not itself new is the left child of block
// old >> h when bit h - 1 of old is set: the old tree's entry for that bit.
//
// The work is cut into passes of kMerkleLogT heights.  Pass p works on items
// of height h0 = p kMerkleLogT (leaves in pass 0, the roots of the previous
// pass's complete tiles after it); a tile is kMerkleT consecutive item indices
// aligned to kMerkleT, reduced level by level in a pair of buffers (LDS on the
// device).  What a lane runs is __host__ __device__: the kernels
// (edv_merkle.hip) and the CPU harness (edv_hostcheck.cpp, hc_merkle_extend)
// are loops over these functions under one host-side pass schedule and
// argument builders (merkle_for_each_pass, merkle_*_args), so the
// straddling-tile and multi-pass logic is tested without a GPU.
//
// Hashes in memory are their 32 bytes (read and written as little-endian
// words); in the level buffers they are the eight big-endian state words.
#pragma once
#include <stdint.h>

#include "edv_sha256.h"

namespace edv {

constexpr int kMerkleLogT = 8;
constexpr int kMerkleT = 1 << kMerkleLogT;     // items per tile = lanes per workgroup
constexpr int kMerkleMaxHashes = 63;           // popcount(size), size <= 2^62
constexpr uint64_t kMerkleMaxSize = uint64_t(1) << 62;

EDV_HD int popc64(uint64_t x) { return __builtin_popcountll(x); }
// x >> h for any h >= 0 (a pass's top level can reach height 64)
EDV_HD uint64_t shr64(uint64_t x, int h) { return h >= 64 ? 0 : x >> h; }

// ---- index arithmetic
// interior nodes of a tree of s leaves
EDV_HD uint64_t merkle_node_count(uint64_t s) { return s - uint64_t(popc64(s)); }
// 1-based position in the node store of block k at height h >= 1: the appends
// write heights 1 .. ctz(s) when leaf s = (k + 1) 2^h (1-based) arrives
EDV_HD uint64_t merkle_store_pos(int h, uint64_t k) {
  const uint64_t s = (k + 1) << h;
  return merkle_node_count(s - 1) + uint64_t(h);
}
// new blocks at height h: [lo, hi)
EDV_HD uint64_t merkle_block_lo(uint64_t old_size, int h) { return shr64(old_size, h); }
EDV_HD uint64_t merkle_block_hi(uint64_t new_size, int h) { return shr64(new_size, h); }
// index in `hashes` (largest first) of the entry for bit b of size
EDV_HD int merkle_hashes_index(uint64_t size, int b) { return popc64(shr64(size, b + 1)); }
// is the left child of new block k at height h the old tree's entry for bit h - 1?
EDV_HD bool merkle_left_is_old(uint64_t old_size, int h, uint64_t k) {
  return ((old_size >> (h - 1)) & 1) != 0 && k == shr64(old_size, h);
}
// is block k at height h (h = 0: a leaf) an entry of the new tree's hashes?
EDV_HD bool merkle_is_frontier(uint64_t new_size, int h, uint64_t k) {
  return h < 64 && ((new_size >> h) & 1) != 0 && k + 1 == (new_size >> h);
}
// does the new tree's entry for bit b come unchanged from the old tree?
EDV_HD bool merkle_frontier_is_old(uint64_t old_size, uint64_t new_size, int b) {
  return (new_size >> b) == (old_size >> b);
}
// items of pass p (height h0): global indices [old >> h0, new >> h0); its
// tiles: [first, first + count)
EDV_HD uint64_t merkle_pass_items(uint64_t old_size, uint64_t new_size, int h0) {
  return shr64(new_size, h0) - shr64(old_size, h0);
}
EDV_HD uint64_t merkle_pass_first_tile(uint64_t old_size, int h0) { return shr64(old_size, h0) >> kMerkleLogT; }
EDV_HD uint64_t merkle_pass_tiles(uint64_t old_size, uint64_t new_size, int h0) {
  if (merkle_pass_items(old_size, new_size, h0) == 0) return 0;
  return ((shr64(new_size, h0) - 1) >> kMerkleLogT) - merkle_pass_first_tile(old_size, h0) + 1;
}
// does pass h0 have anything to do?  Pass 0 hashes the leaves; a later pass
// runs only if it has a block one height up (without one there is none higher
// either: its items are then entries of the new hashes, which the pass before
// has already written)
EDV_HD bool merkle_pass_runs(uint64_t old_size, uint64_t new_size, int h0) {
  return h0 < 64 && merkle_pass_items(old_size, new_size, h0 == 0 ? 0 : h0 + 1) != 0;
}
// tile roots every pass after the first reads, all passes together (the scratch)
EDV_HD uint64_t merkle_scratch_hashes(uint64_t old_size, uint64_t new_size) {
  uint64_t t = 0;
  for (int h0 = kMerkleLogT; merkle_pass_runs(old_size, new_size, h0); h0 += kMerkleLogT)
    t += merkle_pass_items(old_size, new_size, h0);
  return t;
}

// ---- hashing
EDV_HD void merkle_store_hash(uint32_t* dst, const uint32_t H[8]) {  // dst 16-byte aligned on the device
#if defined(__HIP_DEVICE_COMPILE__)
  uint4* p = reinterpret_cast<uint4*>(dst);
  p[0] = make_uint4(bswap32(H[0]), bswap32(H[1]), bswap32(H[2]), bswap32(H[3]));
  p[1] = make_uint4(bswap32(H[4]), bswap32(H[5]), bswap32(H[6]), bswap32(H[7]));
#else
  for (int i = 0; i < 8; i++) dst[i] = bswap32(H[i]);
#endif
}
EDV_HD void merkle_load_hash(uint32_t H[8], const uint32_t* src) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* p = reinterpret_cast<const uint4*>(src);
  const uint4 a = p[0], b = p[1];
  H[0] = bswap32(a.x); H[1] = bswap32(a.y); H[2] = bswap32(a.z); H[3] = bswap32(a.w);
  H[4] = bswap32(b.x); H[5] = bswap32(b.y); H[6] = bswap32(b.z); H[7] = bswap32(b.w);
#else
  for (int i = 0; i < 8; i++) H[i] = bswap32(src[i]);
#endif
}
EDV_HD void sha256_init(uint32_t H[8]) {
  H[0] = 0x6a09e667u; H[1] = 0xbb67ae85u; H[2] = 0x3c6ef372u; H[3] = 0xa54ff53au;
  H[4] = 0x510e527fu; H[5] = 0x9b05688cu; H[6] = 0x1f83d9abu; H[7] = 0x5be0cd19u;
}

// The 16 big-endian words of block [q0, q0 + 64) of the message P | M, P one
// byte held in a register: msg_words32_tail's loads and masks over the virtual
// message that starts one byte before m, except that nothing below the
// 4-byte-aligned word holding m[0] is loaded (m may be the first byte of an
// allocation): only word 0 of block 0 could reach there, for its P byte alone,
// and that byte is put in from the register.  Readable 8 bytes past m + mlen,
// as sha256_msg asks.
EDV_HD void msg_words32_prefixed(uint32_t W[16], uint32_t prefix, const uint8_t* m, uint64_t mlen, uint64_t q0) {
  const uintptr_t m0 = reinterpret_cast<uintptr_t>(m);
  const uintptr_t a = m0 - 1 + q0;                 // where byte q0 of P | M would sit
  const uint32_t sh = uint32_t(a & 3);
  const uintptr_t base = a - sh;
  const uintptr_t low = m0 & ~uintptr_t(3);
  const uintptr_t last = (m0 + mlen) & ~uintptr_t(3);  // the word holding the 0x80 pad byte
  const uint64_t plen = mlen + 1;
  uint32_t d[17];
  if (q0 + 64 <= plen) {  // whole block inside P | M: no clamp to the end, no pad
#pragma unroll
    for (int t = 0; t < 17; t++) {
      const uintptr_t p = base + 4 * uintptr_t(t);
      d[t] = *reinterpret_cast<const uint32_t*>(t == 0 && p < low ? low : p);
    }
#pragma unroll
    for (int t = 0; t < 16; t++) W[t] = bswap32(uint32_t(((uint64_t(d[t + 1]) << 32) | d[t]) >> (8 * sh)));
  } else {
    const int32_t lim = int32_t(int64_t(last) - int64_t(base));  // < 0 for a block wholly past the end
#pragma unroll
    for (int t = 0; t < 17; t++) {
      const int32_t back = lim - 4 * t;
      uintptr_t p = last - uintptr_t(uint32_t(back > 0 ? back : 0));  // min(base + 4 t, last)
      if (t == 0 && p < low) p = low;
      d[t] = *reinterpret_cast<const uint32_t*>(p);
    }
    const int32_t rem0 = int32_t(int64_t(plen) - int64_t(q0));
#pragma unroll
    for (int t = 0; t < 16; t++) {
      const int32_t r = rem0 - 4 * t;
      const int32_t nv = r < 0 ? 0 : (r > 4 ? 4 : r);
      const int32_t nv1 = r + 1 < 0 ? 0 : (r + 1 > 4 ? 4 : r + 1);
      const uint32_t keep = ((1u << (4 * nv)) << (4 * nv)) - 1u;   // low nv bytes (nv = 4: all)
      const uint32_t keep1 = ((1u << (4 * nv1)) << (4 * nv1)) - 1u;
      uint32_t v = uint32_t(((uint64_t(d[t + 1]) << 32) | d[t]) >> (8 * sh));  // little-endian byte order
      if (t == 0 && q0 == 0) v = (v & ~0xffu) | prefix;
      v = (v & keep) | ((keep ^ keep1) & 0x80808080u);
      W[t] = bswap32(v);
    }
    return;
  }
  if (q0 == 0) W[0] = (W[0] & 0x00ffffffu) | (prefix << 24);
}

// SHA-256(P | M) -> the eight state words (big-endian order)
EDV_HD void sha256_prefixed(uint32_t H[8], uint32_t prefix, const uint8_t* m, uint64_t mlen) {
  sha256_init(H);
  const uint64_t plen = mlen + 1;
  const uint64_t nb = (plen + 8 + 1 + 63) / 64;
  uint32_t W[16];
#pragma unroll 1
  for (uint64_t b = 0; b < nb; b++) {
    msg_words32_prefixed(W, prefix, m, mlen, 64 * b);
    if (b == nb - 1) {
      W[14] = uint32_t(plen >> 29);
      W[15] = uint32_t(plen << 3);
    }
    sha256_compress(H, W);
  }
}
// RFC 6962 leaf hash, SHA-256(0x00 | leaf)
EDV_HD void merkle_leaf_hash(uint32_t H[8], const uint8_t* leaf, uint64_t len) { sha256_prefixed(H, 0u, leaf, len); }

// RFC 6962 node hash, SHA-256(0x01 | l | r): 65 bytes, two blocks spelt out.
// Block 1 is 0x01, l, r[0..31); block 2 is r[31], 0x80, zeros and the bit
// length 520.
EDV_HD void merkle_node_hash(uint32_t H[8], const uint32_t l[8], const uint32_t r[8]) {
  uint32_t W[16];
  W[0] = 0x01000000u | (l[0] >> 8);
#pragma unroll
  for (int i = 1; i < 8; i++) W[i] = (l[i - 1] << 24) | (l[i] >> 8);
  W[8] = (l[7] << 24) | (r[0] >> 8);
#pragma unroll
  for (int i = 1; i < 8; i++) W[8 + i] = (r[i - 1] << 24) | (r[i] >> 8);
  const uint32_t tail = (r[7] << 24) | 0x00800000u;
  sha256_init(H);
  sha256_compress(H, W);
  W[0] = tail;
#pragma unroll
  for (int i = 1; i < 15; i++) W[i] = 0;
  W[15] = 520;
  sha256_compress(H, W);
}
EDV_HD void merkle_empty_hash(uint32_t H[8]) {  // SHA-256("")
  uint32_t W[16];
  W[0] = 0x80000000u;
#pragma unroll
  for (int i = 1; i < 16; i++) W[i] = 0;
  sha256_init(H);
  sha256_compress(H, W);
}
// Root of (size, hashes): fold from the right
EDV_HD void merkle_fold(uint32_t root[8], const uint32_t* hashes, int count) {
  if (count == 0) {
    merkle_empty_hash(root);
    return;
  }
  merkle_load_hash(root, hashes + 8 * (count - 1));
#pragma unroll 1
  for (int i = count - 2; i >= 0; i--) {
    uint32_t l[8], r[8];
    merkle_load_hash(l, hashes + 8 * i);
    for (int w = 0; w < 8; w++) r[w] = root[w];
    merkle_node_hash(root, l, r);
  }
}

// ---- one pass
struct MerklePass {
  uint64_t old_size, new_size;  // the call's
  int h0;                       // height of this pass's items
  const uint32_t* old_hashes;   // popcount(old_size) entries
  const uint32_t* in;           // h0 > 0: the items' hashes, item j at 8 (j - (old_size >> h0))
  uint32_t* leaf_out;           // h0 = 0: leaf hashes, or null
  uint32_t* node_out;           // node store positions node_count(old) + 1 ..., or null
  uint32_t* new_hashes;         // the new tree's entries that are new
  uint32_t* roots_out;          // roots of complete tiles: block k of height h0 + kMerkleLogT at 8 (k - lo), or null
};

// what becomes of a new hash at height h (0: a leaf), block k
EDV_HD void merkle_emit(const MerklePass& a, int h, uint64_t k, const uint32_t H[8]) {
  if (h == 0) {
    if (a.leaf_out) merkle_store_hash(a.leaf_out + 8 * (k - a.old_size), H);
  } else if (a.node_out) {
    merkle_store_hash(a.node_out + 8 * (merkle_store_pos(h, k) - 1 - merkle_node_count(a.old_size)), H);
  }
  if (merkle_is_frontier(a.new_size, h, k)) merkle_store_hash(a.new_hashes + 8 * merkle_hashes_index(a.new_size, h), H);
}

// The level buffers hold word w of local item j at [w kMerkleT + j].
// Item stage of lane j of a tile (pass 0: H is the lane's leaf hash, by the
// caller; later passes: loaded here).  False: no such item.
EDV_HD bool merkle_item_index(const MerklePass& a, uint64_t tile, uint32_t j, uint64_t* g) {
  *g = (tile << kMerkleLogT) + j;
  return *g >= shr64(a.old_size, a.h0) && *g < shr64(a.new_size, a.h0);
}
EDV_HD void merkle_item_put(const MerklePass& a, uint64_t g, uint32_t j, const uint32_t H[8], uint32_t* cur) {
  for (int w = 0; w < 8; w++) cur[w * kMerkleT + j] = H[w];
  if (a.h0 == 0) merkle_emit(a, 0, g, H);  // later passes' items were emitted as the pass before's tile roots
}
// Level hl (1 .. kMerkleLogT) of a tile, local block j < kMerkleT >> hl: reads
// level hl - 1 from cur, writes nxt.
EDV_HD void merkle_level(const MerklePass& a, uint64_t tile, int hl, uint32_t j, const uint32_t* cur, uint32_t* nxt) {
  const int h = a.h0 + hl;
  const uint64_t k = (tile << (kMerkleLogT - hl)) + j;
  if (k < merkle_block_lo(a.old_size, h) || k >= merkle_block_hi(a.new_size, h)) return;
  uint32_t l[8], r[8], H[8];
  if (merkle_left_is_old(a.old_size, h, k)) {
    merkle_load_hash(l, a.old_hashes + 8 * merkle_hashes_index(a.old_size, h - 1));
  } else {
    for (int w = 0; w < 8; w++) l[w] = cur[w * kMerkleT + 2 * j];
  }
  for (int w = 0; w < 8; w++) r[w] = cur[w * kMerkleT + 2 * j + 1];
  merkle_node_hash(H, l, r);
  for (int w = 0; w < 8; w++) nxt[w * kMerkleT + j] = H[w];
  merkle_emit(a, h, k, H);
  if (hl == kMerkleLogT && a.roots_out) merkle_store_hash(a.roots_out + 8 * (k - merkle_block_lo(a.old_size, h)), H);
}

// A call's passes (host side): what every pass of it shares (hashes at any
// pointer type), and the schedule: run_pass(a) once per pass that runs, lowest
// first, with a.h0, a.in and a.roots_out set.  A pass that another follows
// writes its tiles' roots to the scratch at roots_base (merkle_scratch_hashes
// entries in all) behind those of the passes before it.  Returns the first
// nonzero result of run_pass (an int or an error code), or zero.
inline MerklePass merkle_pass_args(uint64_t old_size, uint64_t new_size, const void* old_hashes, void* leaf_out,
                                   void* node_out, void* new_hashes) {
  using H = uint32_t*;
  return {old_size, new_size, 0, static_cast<const uint32_t*>(old_hashes), nullptr, H(leaf_out), H(node_out),
          H(new_hashes), nullptr};
}
// leaf_in (row f-9, extend from hashes): the n leaf hashes instead of leaf
// bytes; pass 0 then loads its items from them, as every later pass loads its.
template <class F>
inline auto merkle_for_each_pass(uint64_t old_size, uint64_t new_size, uint32_t* roots_base, MerklePass& a, F run_pass,
                                 const uint32_t* leaf_in = nullptr) {
  a.in = leaf_in;
  for (int h0 = 0; merkle_pass_runs(old_size, new_size, h0); h0 += kMerkleLogT) {
    const uint64_t next_items =
        merkle_pass_runs(old_size, new_size, h0 + kMerkleLogT) ? merkle_pass_items(old_size, new_size, h0 + kMerkleLogT) : 0;
    a.h0 = h0;
    a.roots_out = next_items ? roots_base : nullptr;
    if (const auto rc = run_pass(a)) return rc;
    a.in = roots_base;
    roots_base += 8 * next_items;
  }
  return decltype(run_pass(a))();
}

// Finish: the entries of the new tree's hashes that the old tree already had
// (same index in both), then the root.
EDV_HD void merkle_finish(uint64_t old_size, uint64_t new_size, const uint32_t* old_hashes, uint32_t* new_hashes,
                          uint32_t* root) {
  for (int b = 62; b >= 0; b--) {
    if (!((new_size >> b) & 1) || !merkle_frontier_is_old(old_size, new_size, b)) continue;
    const int i = merkle_hashes_index(new_size, b);
    for (int w = 0; w < 8; w++) new_hashes[8 * i + w] = old_hashes[8 * i + w];
  }
  uint32_t R[8];
  merkle_fold(R, new_hashes, popc64(new_size));
  merkle_store_hash(root, R);
}

// ---- per-leaf roots and audit paths (row f-6: what n calls of `append` return)
// Leaf i (0-based) of a call extending `old` by n gives the tree of size
// s = old + i + 1.  The entry of hashes(s) for set bit b is block
// k = (s >> b) - 1 at height b.  If that block ends at or before `old`
// ((k + 1) << b <= old) then old >> b == s >> b, so it is the old tree's entry
// for the same bit, at the same index; otherwise the call made it: a leaf hash
// (b = 0) or a node at its node-store position.  Nothing is hashed twice: the
// passes have written every entry before the append kernel reads it.
struct MerkleAppend {
  uint64_t old_size, n;
  uint64_t path_base;           // merkle_popc_prefix(old_size)
  const uint32_t* old_hashes;   // popcount(old_size) entries
  const uint32_t* leaf_hashes;  // the call's n leaf hashes
  const uint32_t* node_hashes;  // the call's nodes, node-store order
  uint32_t* roots;              // root after leaf i at 8 i, or null
  uint32_t* paths;              // packed audit paths, or null
};

// P(x) = sum of popcount(t) over t < x, modulo 2^64 (x <= 2^62; P(2^62) is
// above 2^64, differences over one call are not): bit b is set in
// (x >> (b + 1)) 2^b numbers below x, plus the part of x's last period of
// 2^(b + 1) past its first half.
EDV_HD uint64_t merkle_popc_prefix(uint64_t x) {
  uint64_t p = 0;
#pragma unroll 1
  for (int b = 0; b < 63 && (x >> b) != 0; b++) {
    const uint64_t half = uint64_t(1) << b;
    const uint64_t rem = x & ((half << 1) - 1);
    p += ((x >> (b + 1)) << b) + (rem > half ? rem - half : 0);
  }
  return p;
}
// the append kernel's arguments from the call's, field by field (host side; hashes at any pointer type)
inline MerkleAppend merkle_append_args(uint64_t old_size, uint64_t n, const void* old_hashes, const void* leaf_hashes,
                                       const void* node_hashes, void* roots, void* paths) {
  using H = const uint32_t*;
  return {old_size, n, merkle_popc_prefix(old_size), H(old_hashes), H(leaf_hashes), H(node_hashes),
          static_cast<uint32_t*>(roots), static_cast<uint32_t*>(paths)};
}
// audit-path entries of the first n appends to a tree of old_size leaves
// (leaf i's path has popcount(old_size + i) entries)
EDV_HD uint64_t merkle_path_entries(uint64_t old_size, uint64_t n) {
  return merkle_popc_prefix(old_size + n) - merkle_popc_prefix(old_size);
}
// the entry of hashes(s) for set bit b of s, old_size <= s <= old_size + n
EDV_HD const uint32_t* merkle_entry(const MerkleAppend& a, uint64_t s, int b) {
  const uint64_t k = (s >> b) - 1;
  if (((k + 1) << b) <= a.old_size) return a.old_hashes + 8 * merkle_hashes_index(a.old_size, b);
  if (b == 0) return a.leaf_hashes + 8 * (k - a.old_size);
  return a.node_hashes + 8 * (merkle_store_pos(b, k) - 1 - merkle_node_count(a.old_size));
}
EDV_HD void merkle_copy_hash(uint32_t* dst, const uint32_t* src) {  // both 16-byte aligned on the device
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* p = reinterpret_cast<const uint4*>(src);
  const uint4 x = p[0], y = p[1];
  uint4* q = reinterpret_cast<uint4*>(dst);
  q[0] = x;
  q[1] = y;
#else
  for (int w = 0; w < 8; w++) dst[w] = src[w];
#endif
}
// The root of the tree of s leaves inside the call, 1 <= s, a.old_size <= s <=
// a.old_size + a.n: merkle_fold's order over the entries of hashes(s), from the
// lowest set bit up.
EDV_HD void merkle_fold_entries(uint32_t acc[8], const MerkleAppend& a, uint64_t s) {
  uint64_t bits = s;
  int b = __builtin_ctzll(bits);
  merkle_load_hash(acc, merkle_entry(a, s, b));
  bits &= bits - 1;
#pragma unroll 1
  while (bits) {
    b = __builtin_ctzll(bits);
    bits &= bits - 1;
    uint32_t l[8], r[8];
    merkle_load_hash(l, merkle_entry(a, s, b));
    for (int w = 0; w < 8; w++) r[w] = acc[w];
    merkle_node_hash(acc, l, r);
  }
}
// Leaf i of the call, i < a.n: the root of the tree after it (merkle_fold_entries)
// and its audit path (the entries of hashes(s - 1), lowest bit first, at entry
// P(old + i) - P(old) of the packed output).
EDV_HD void merkle_append_leaf(const MerkleAppend& a, uint64_t i) {
  const uint64_t s = a.old_size + i + 1;
  if (a.roots) {
    uint32_t acc[8];
    merkle_fold_entries(acc, a, s);
    merkle_store_hash(a.roots + 8 * i, acc);
  }
  if (a.paths) {
    uint32_t* out = a.paths + 8 * (merkle_popc_prefix(s - 1) - a.path_base);
    uint64_t bits = s - 1;
#pragma unroll 1
    while (bits) {
      const int b = __builtin_ctzll(bits);
      bits &= bits - 1;
      merkle_copy_hash(out, merkle_entry(a, s - 1, b));
      out += 8;
    }
  }
}

// ---- proof verification (row f-7: what MerkleVerifier checks, one lane per proof)
// Written from RFC 6962 sections 2.1.1 (audit paths) and 2.1.2 (consistency
// proofs).  A proof is `count` 32-byte entries, lowest level first; a walk
// never reads an entry at or past `count`.  One status byte per proof; 0 is
// never written by a walk, so a buffer nothing wrote rejects.
constexpr uint8_t kProofUnverified = 0;    // EDV_PROOF_* of include/edv.h
constexpr uint8_t kProofOk = 1;
constexpr uint8_t kProofRange = 2;         // leaf_index >= tree_size / old_size > new_size
constexpr uint8_t kProofShort = 3;         // the walk needed an entry past the proof's end
constexpr uint8_t kProofLong = 4;          // inclusion: entries left over after the walk
constexpr uint8_t kProofRoot = 5;          // the computed (new) root differs
constexpr uint8_t kProofInconsistent = 6;  // consistency: new root matches, old root does not
// did the walk run to its end (`computed` holds what it calculated)?
EDV_HD bool merkle_proof_walked(uint8_t st) { return st == kProofOk || st >= kProofLong; }
EDV_HD bool merkle_hash_equal(const uint32_t a[8], const uint32_t b[8]) {
  uint32_t d = 0;
#pragma unroll
  for (int w = 0; w < 8; w++) d |= a[w] ^ b[w];
  return d == 0;
}

// Audit path of leaf `leaf_index` in the tree of `tree_size` leaves (any
// uint64_t size, at most 64 levels): node = leaf_index, last = tree_size - 1,
// upwards while last > 0.  An odd node has a left sibling, an even node below
// `last` a right one, an even node that is the last of its level none (no
// entry, no hash).  Both kinds of sibling go through one node hash with the
// operands selected, so lanes on different sides of their parents stay
// together.  acc: the leaf hash in, the calculated root out (when the walk
// ran to its end).  Precedence: RANGE, SHORT, LONG, ROOT.
EDV_HD uint8_t merkle_verify_inclusion_one(uint32_t acc[8], uint64_t leaf_index, uint64_t tree_size,
                                           const uint32_t* path, uint64_t count, const uint32_t root[8]) {
  if (leaf_index >= tree_size) return kProofRange;
  uint64_t node = leaf_index, last = tree_size - 1, used = 0;
#pragma unroll 1
  while (last > 0) {
    const bool odd = (node & 1) != 0;
    if (odd || node < last) {
      if (used == count) return kProofShort;
      uint32_t e[8], l[8], r[8];
      merkle_load_hash(e, path + 8 * used);
      used++;
#pragma unroll
      for (int w = 0; w < 8; w++) {
        l[w] = odd ? e[w] : acc[w];
        r[w] = odd ? acc[w] : e[w];
      }
      merkle_node_hash(acc, l, r);
    }
    node >>= 1;
    last >>= 1;
  }
  if (used != count) return kProofLong;
  return merkle_hash_equal(acc, root) ? kProofOk : kProofRoot;
}

// Consistency of the trees of old_size and new_size leaves.  old > new: RANGE;
// equal sizes: the roots decide, the proof is ignored; old = 0: OK, anything is
// consistent with the empty tree.  Otherwise node = old - 1, last = new - 1,
// both shifted right while node is odd (that part is in both trees); the seed
// of both accumulators is the first entry, or old_root when node is 0 (old is
// a power of two).  Then upwards while last > 0: an odd node's left sibling
// goes into both accumulators, an even node's right sibling (node < last) into
// the new one only, an even last node has none.  Once node is 0 it stays even
// and below last, so the same loop is the rest of the path up to the new
// root.  Entries after the walk are accepted.  walked: false where no walk was
// made (then oldr / newr hold nothing).  ROOT before INCONSISTENT.
EDV_HD uint8_t merkle_verify_consistency_one(uint32_t oldr[8], uint32_t newr[8], bool* walked, uint64_t old_size,
                                             uint64_t new_size, const uint32_t old_root[8], const uint32_t new_root[8],
                                             const uint32_t* proof, uint64_t count) {
  *walked = false;
  if (old_size > new_size) return kProofRange;
  if (old_size == new_size) return merkle_hash_equal(old_root, new_root) ? kProofOk : kProofInconsistent;
  if (old_size == 0) return kProofOk;
  uint64_t node = old_size - 1, last = new_size - 1, used = 0;
  while (node & 1) {
    node >>= 1;
    last >>= 1;
  }
  if (node != 0) {
    if (count == 0) return kProofShort;
    merkle_load_hash(newr, proof);
    used = 1;
  } else {
#pragma unroll
    for (int w = 0; w < 8; w++) newr[w] = old_root[w];
  }
#pragma unroll
  for (int w = 0; w < 8; w++) oldr[w] = newr[w];
#pragma unroll 1
  while (last > 0) {
    const bool odd = (node & 1) != 0;
    if (odd || node < last) {
      if (used == count) return kProofShort;
      uint32_t e[8], l[8], r[8];
      merkle_load_hash(e, proof + 8 * used);
      used++;
      if (odd) {
#pragma unroll
        for (int w = 0; w < 8; w++) r[w] = oldr[w];
        merkle_node_hash(oldr, e, r);
      }
#pragma unroll
      for (int w = 0; w < 8; w++) {
        l[w] = odd ? e[w] : newr[w];
        r[w] = odd ? newr[w] : e[w];
      }
      merkle_node_hash(newr, l, r);
    }
    node >>= 1;
    last >>= 1;
  }
  *walked = true;
  if (!merkle_hash_equal(newr, new_root)) return kProofRoot;
  return merkle_hash_equal(oldr, old_root) ? kProofOk : kProofInconsistent;
}

// One batch of inclusion proofs.  Proof i is entries [proof_off[i],
// proof_off[i + 1]) - proof_base of `proofs` (the layout the batched append
// writes); its leaf is bytes [leaf_off[i], leaf_off[i + 1]) - leaf_base of
// `leaves` (kLeaves), or hash i of leaf_hashes.
struct MerkleVerifyInclusion {
  uint64_t n;
  const uint8_t* leaves;        // kLeaves: readable 8 bytes past the last leaf byte
  const uint64_t* leaf_off;
  uint64_t leaf_base;
  const uint32_t* leaf_hashes;  // !kLeaves
  const uint64_t* leaf_index;
  const uint64_t* tree_size;
  const uint32_t* roots;
  const uint32_t* proofs;
  const uint64_t* proof_off;
  uint64_t proof_base;
  uint8_t* status;
  uint32_t* computed;           // 8 words per proof, or null
};
// ... from the call's arguments (host side; hashes at any pointer type): leaves or leaf_hashes, the other null
inline MerkleVerifyInclusion merkle_verify_inclusion_args(
    uint64_t n, const uint8_t* leaves, const uint64_t* leaf_off, uint64_t leaf_base, const void* leaf_hashes,
    const uint64_t* leaf_index, const uint64_t* tree_size, const void* roots, const void* proofs,
    const uint64_t* proof_off, uint64_t proof_base, uint8_t* status, void* computed) {
  using H = const uint32_t*;
  return {n, leaves, leaf_off, leaf_base, H(leaf_hashes), leaf_index, tree_size, H(roots), H(proofs), proof_off,
          proof_base, status, static_cast<uint32_t*>(computed)};
}
// Lane i < a.n.  A lane out of range hashes no leaf.
template <bool kLeaves>
EDV_HD void merkle_verify_inclusion_lane(const MerkleVerifyInclusion& a, uint64_t i) {
  const uint64_t idx = a.leaf_index[i], size = a.tree_size[i];
  const uint64_t p0 = a.proof_off[i], p1 = a.proof_off[i + 1];
  uint32_t acc[8], root[8];
  uint8_t st = kProofRange;
  if (idx < size) {
    if (kLeaves) {
      const uint64_t o0 = a.leaf_off[i] - a.leaf_base, o1 = a.leaf_off[i + 1] - a.leaf_base;
      merkle_leaf_hash(acc, a.leaves + o0, o1 - o0);
    } else {
      merkle_load_hash(acc, a.leaf_hashes + 8 * i);
    }
    merkle_load_hash(root, a.roots + 8 * i);
    st = merkle_verify_inclusion_one(acc, idx, size, a.proofs + 8 * (p0 - a.proof_base), p1 - p0, root);
  }
  a.status[i] = st;
  if (a.computed) {
    if (!merkle_proof_walked(st)) {
#pragma unroll
      for (int w = 0; w < 8; w++) acc[w] = 0;
    }
    merkle_store_hash(a.computed + 8 * i, acc);
  }
}

struct MerkleVerifyConsistency {
  uint64_t n;
  const uint64_t* old_size;
  const uint64_t* new_size;
  const uint32_t* old_roots;
  const uint32_t* new_roots;
  const uint32_t* proofs;
  const uint64_t* proof_off;
  uint64_t proof_base;
  uint8_t* status;
  uint32_t* computed;  // 16 words per proof (old, then new), or null
};
inline MerkleVerifyConsistency merkle_verify_consistency_args(
    uint64_t n, const uint64_t* old_size, const uint64_t* new_size, const void* old_roots, const void* new_roots,
    const void* proofs, const uint64_t* proof_off, uint64_t proof_base, uint8_t* status, void* computed) {
  using H = const uint32_t*;
  return {n, old_size, new_size, H(old_roots), H(new_roots), H(proofs), proof_off, proof_base, status,
          static_cast<uint32_t*>(computed)};
}
EDV_HD void merkle_verify_consistency_lane(const MerkleVerifyConsistency& a, uint64_t i) {
  const uint64_t p0 = a.proof_off[i], p1 = a.proof_off[i + 1];
  uint32_t ro[8], rn[8], oldr[8], newr[8];
  merkle_load_hash(ro, a.old_roots + 8 * i);
  merkle_load_hash(rn, a.new_roots + 8 * i);
  bool walked;
  const uint8_t st = merkle_verify_consistency_one(oldr, newr, &walked, a.old_size[i], a.new_size[i], ro, rn,
                                                   a.proofs + 8 * (p0 - a.proof_base), p1 - p0);
  a.status[i] = st;
  if (a.computed) {
    if (!walked) {
#pragma unroll
      for (int w = 0; w < 8; w++) oldr[w] = newr[w] = 0;
    }
    merkle_store_hash(a.computed + 16 * i, oldr);
    merkle_store_hash(a.computed + 16 * i + 8, newr);
  }
}

// ---- proof generation from a stored tree (row f-8: what CompactMerkleTree.
// inclusion_proof / consistency_proof / merkle_tree_hash(0, n) read out of the
// hash store, one lane per proof).  Written from RFC 6962 sections 2.1.1 and
// 2.1.2: the walks above run backwards.  The store is the appends': leaf hash
// k (0-based) at byte 32 k of the leaf store, block k of height h >= 1 at byte
// 32 (merkle_store_pos(h, k) - 1) of the node store.  Every proof entry is
// MTH(D[a:b]) of a sibling on the way up; all of them are complete aligned
// subtrees, which are stored, but at most one: a right sibling cut off by the
// tree's end, [a, n) with a = (n >> h) << h, whose leaves are the subtrees of
// the set bits of n below h.  Folding the root of the n leaves in merkle_fold's
// order (lowest set bit first), the accumulator is that entry at the moment the
// bits below h are consumed, so it costs no hash beyond the root's.  (With one
// set bit below h the range is itself a complete subtree and is read.)
constexpr uint8_t kProofSpace = 7;  // EDV_PROOF_SPACE: the slot's length is not the proof's
constexpr int kMerkleMaxProof = 63; // entries: an audit path has at most 62, a consistency proof 63 (sizes <= 2^62)
constexpr uint8_t kEntryLeaf = 0, kEntryNode = 1, kEntryFold = 2;  // where an entry comes from

// The walk of one proof over a tree of n leaves, 1 <= n <= 2^62: entries come
// out lowest level first.  seed: a consistency proof's first entry, the subtree
// (h, node) that ends at `first`, when first is no power of two.
struct MerkleProofWalk {
  uint64_t node, last, n;
  int h;
  bool seed;
};
EDV_HD MerkleProofWalk merkle_inclusion_walk(uint64_t m, uint64_t n) { return {m, n - 1, n, 0, false}; }
// 1 <= first <= second; first == second: no entries
EDV_HD MerkleProofWalk merkle_consistency_walk(uint64_t first, uint64_t second) {
  if (first == second) return {0, 0, second, 0, false};
  uint64_t node = first - 1, last = second - 1;
  int h = 0;
  while (node & 1) {
    node >>= 1;
    last >>= 1;
    h++;
  }
  return {node, last, second, h, node != 0};
}
// store offset in bytes of the complete subtree of height h, block k
EDV_HD uint8_t merkle_subtree_pos(int h, uint64_t k, uint64_t* off) {
  if (h == 0) {
    *off = 32 * k;
    return kEntryLeaf;
  }
  *off = 32 * (merkle_store_pos(h, k) - 1);
  return kEntryNode;
}
// The next entry: false when the walk is over.  kEntryLeaf / kEntryNode: *off
// is its byte offset into that store; kEntryFold: *off is the height h of the
// cut-off sibling, the fold's accumulator once the set bits of n below h are in.
EDV_HD bool merkle_walk_next(MerkleProofWalk& w, uint8_t* kind, uint64_t* off) {
  if (w.seed) {
    w.seed = false;
    *kind = merkle_subtree_pos(w.h, w.node, off);
    return true;
  }
  while (w.last > 0) {
    const uint64_t node = w.node, last = w.last;
    const int h = w.h;
    w.node >>= 1;
    w.last >>= 1;
    w.h++;
    if (node & 1) {
      *kind = merkle_subtree_pos(h, node - 1, off);
      return true;
    }
    if (node < last) {
      const uint64_t k = node + 1, start = k << h, rem = w.n - start;  // (k + 1) << h <= n + 2^h: no overflow
      if (((k + 1) << h) <= w.n) {
        *kind = merkle_subtree_pos(h, k, off);
      } else if ((rem & (rem - 1)) == 0) {  // one subtree of height ctz(rem), aligned: start is a multiple of 2^h
        const int j = __builtin_ctzll(rem);
        *kind = merkle_subtree_pos(j, start >> j, off);
      } else {
        *kind = kEntryFold;
        *off = uint64_t(h);
      }
      return true;
    }
  }
  return false;
}
EDV_HD uint64_t merkle_walk_length(MerkleProofWalk w) {
  uint64_t len = w.seed ? 1 : 0;
  for (; w.last > 0; w.node >>= 1, w.last >>= 1)
    if ((w.node & 1) || w.node < w.last) len++;
  return len;
}
// entries of PATH(m, D[n]), m < n, and of PROOF(first, D[second]), 1 <= first <= second
EDV_HD uint64_t merkle_inclusion_length(uint64_t m, uint64_t n) { return merkle_walk_length(merkle_inclusion_walk(m, n)); }
EDV_HD uint64_t merkle_consistency_length(uint64_t first, uint64_t second) {
  return merkle_walk_length(merkle_consistency_walk(first, second));
}
// The positions of a proof's entries in output order (the pair as above): kind
// and byte offset (kEntryFold: the height) per entry, at most kMerkleMaxProof.
// Returns the count.  Pure index arithmetic: any size up to 2^62 without a store.
EDV_HD int merkle_proof_positions(bool consistency, uint64_t a, uint64_t n, uint8_t* kind, uint64_t* off) {
  MerkleProofWalk w = consistency ? merkle_consistency_walk(a, n) : merkle_inclusion_walk(a, n);
  int e = 0;
  while (merkle_walk_next(w, kind + e, off + e)) e++;
  return e;
}
// the stored entry of hashes(n) for set bit b of n
EDV_HD const uint32_t* merkle_store_entry(const uint32_t* leaf_store, const uint32_t* node_store, uint64_t n, int b) {
  const uint64_t k = (n >> b) - 1;
  return b == 0 ? leaf_store + 8 * k : node_store + 8 * (merkle_store_pos(b, k) - 1);
}
// MTH(D[0:n]) into acc, n >= 1, folded from the lowest set bit up; fold_slot
// (or null) takes the accumulator before the first bit at or above fold_h goes
// in.  Without want_root the fold stops there.
EDV_HD void merkle_fold_store(uint32_t acc[8], const uint32_t* leaf_store, const uint32_t* node_store, uint64_t n,
                              int fold_h, uint32_t* fold_slot, bool want_root) {
  uint64_t bits = n;
  int b = __builtin_ctzll(bits);
  merkle_load_hash(acc, merkle_store_entry(leaf_store, node_store, n, b));
  bits &= bits - 1;
#pragma unroll 1
  while (bits) {
    b = __builtin_ctzll(bits);
    bits &= bits - 1;
    if (fold_slot && b >= fold_h) {
      merkle_store_hash(fold_slot, acc);
      fold_slot = nullptr;
      if (!want_root) return;
    }
    uint32_t l[8], r[8];
    merkle_load_hash(l, merkle_store_entry(leaf_store, node_store, n, b));
    for (int w = 0; w < 8; w++) r[w] = acc[w];
    merkle_node_hash(acc, l, r);
  }
}
// One proof's entries into out (the walk's length of them, checked by the
// caller) and, with want_root, MTH(D[0:w.n]) into root: the stored entries are
// copied, the cut-off one comes out of the root's fold (which runs without
// want_root only up to it).
EDV_HD void merkle_prove_one(uint32_t root[8], const uint32_t* leaf_store, const uint32_t* node_store, MerkleProofWalk w,
                             uint32_t* out, bool want_root) {
  const uint64_t n = w.n;
  uint32_t* fold_slot = nullptr;
  int fold_h = 64;
  uint8_t kind;
  uint64_t off;
#pragma unroll 1
  while (merkle_walk_next(w, &kind, &off)) {
    if (kind == kEntryFold) {
      fold_slot = out;
      fold_h = int(off);
    } else {
      merkle_copy_hash(out, (kind == kEntryLeaf ? leaf_store : node_store) + off / 4);
    }
    out += 8;
  }
  if (want_root || fold_slot) merkle_fold_store(root, leaf_store, node_store, n, fold_h, fold_slot, want_root);
}
EDV_HD void merkle_store_hash_or_zero(uint32_t* dst, uint32_t H[8], bool ok) {
  if (!ok) {
#pragma unroll
    for (int w = 0; w < 8; w++) H[w] = 0;
  }
  merkle_store_hash(dst, H);
}

// One batch of inclusion proofs out of a store of store_leaves leaves (and
// merkle_node_count(store_leaves) nodes).  Proof i goes to entries
// [proof_off[i], proof_off[i + 1]) - proof_base of `proofs`, the layout the
// verify kernels read.  RANGE, then SPACE (the slot is not the proof's length:
// nothing written there), then OK.  No store position at or past the counts is
// read: every entry of a proof in the tree of tree_size <= store_leaves leaves
// is a subtree that ends at or before tree_size.
struct MerkleProveInclusion {
  uint64_t n;
  const uint32_t* leaf_store;
  const uint32_t* node_store;
  uint64_t store_leaves;
  const uint64_t* leaf_index;
  const uint64_t* tree_size;
  const uint64_t* proof_off;
  uint64_t proof_base;
  uint32_t* proofs;
  uint8_t* status;
  uint32_t* roots;            // MTH(D[0:tree_size]) at 8 i, zeros unless OK; or null
  uint32_t* leaf_hashes_out;  // the leaf's stored hash at 8 i, zeros unless OK; or null
};
inline MerkleProveInclusion merkle_prove_inclusion_args(const void* leaf_store, const void* node_store,
                                                        uint64_t store_leaves, const uint64_t* leaf_index,
                                                        const uint64_t* tree_size, const uint64_t* proof_off,
                                                        uint64_t proof_base, uint64_t n, void* proofs, uint8_t* status,
                                                        void* roots, void* leaf_hashes_out) {
  using H = uint32_t*;
  return {n, static_cast<const uint32_t*>(leaf_store), static_cast<const uint32_t*>(node_store), store_leaves,
          leaf_index, tree_size, proof_off, proof_base, H(proofs), status, H(roots), H(leaf_hashes_out)};
}
EDV_HD uint8_t merkle_prove_inclusion_status(uint64_t idx, uint64_t size, uint64_t store_leaves, uint64_t slot) {
  if (idx >= size || size > store_leaves) return kProofRange;
  return slot == merkle_inclusion_length(idx, size) ? kProofOk : kProofSpace;
}
EDV_HD void merkle_prove_inclusion_lane(const MerkleProveInclusion& a, uint64_t i) {
  const uint64_t idx = a.leaf_index[i], size = a.tree_size[i];
  const uint64_t p0 = a.proof_off[i], p1 = a.proof_off[i + 1];
  const uint8_t st = merkle_prove_inclusion_status(idx, size, a.store_leaves, p1 - p0);
  const bool ok = st == kProofOk;
  uint32_t root[8];
  if (ok)
    merkle_prove_one(root, a.leaf_store, a.node_store, merkle_inclusion_walk(idx, size),
                     a.proofs + 8 * (p0 - a.proof_base), a.roots != nullptr);
  a.status[i] = st;
  if (a.roots) merkle_store_hash_or_zero(a.roots + 8 * i, root, ok);
  if (a.leaf_hashes_out) {
    if (ok)
      merkle_copy_hash(a.leaf_hashes_out + 8 * i, a.leaf_store + 8 * idx);
    else
      merkle_store_hash_or_zero(a.leaf_hashes_out + 8 * i, root, false);
  }
}

// ... and of consistency proofs PROOF(first, D[second]).  RANGE: first == 0
// (the recursive definition never ends there), first > second, second >
// store_leaves; first == second is OK with no entries.  The old root is a fold
// of its own over the same store, popcount(first) - 1 hashes.
struct MerkleProveConsistency {
  uint64_t n;
  const uint32_t* leaf_store;
  const uint32_t* node_store;
  uint64_t store_leaves;
  const uint64_t* first;
  const uint64_t* second;
  const uint64_t* proof_off;
  uint64_t proof_base;
  uint32_t* proofs;
  uint8_t* status;
  uint32_t* old_roots;  // MTH(D[0:first]) at 8 i, zeros unless OK; or null
  uint32_t* new_roots;  // MTH(D[0:second])
};
inline MerkleProveConsistency merkle_prove_consistency_args(const void* leaf_store, const void* node_store,
                                                            uint64_t store_leaves, const uint64_t* first,
                                                            const uint64_t* second, const uint64_t* proof_off,
                                                            uint64_t proof_base, uint64_t n, void* proofs,
                                                            uint8_t* status, void* old_roots, void* new_roots) {
  using H = uint32_t*;
  return {n, static_cast<const uint32_t*>(leaf_store), static_cast<const uint32_t*>(node_store), store_leaves,
          first, second, proof_off, proof_base, H(proofs), status, H(old_roots), H(new_roots)};
}
EDV_HD uint8_t merkle_prove_consistency_status(uint64_t first, uint64_t second, uint64_t store_leaves, uint64_t slot) {
  if (first == 0 || first > second || second > store_leaves) return kProofRange;
  return slot == merkle_consistency_length(first, second) ? kProofOk : kProofSpace;
}
EDV_HD void merkle_prove_consistency_lane(const MerkleProveConsistency& a, uint64_t i) {
  const uint64_t first = a.first[i], second = a.second[i];
  const uint64_t p0 = a.proof_off[i], p1 = a.proof_off[i + 1];
  const uint8_t st = merkle_prove_consistency_status(first, second, a.store_leaves, p1 - p0);
  const bool ok = st == kProofOk;
  uint32_t root[8];
  if (ok)
    merkle_prove_one(root, a.leaf_store, a.node_store, merkle_consistency_walk(first, second),
                     a.proofs + 8 * (p0 - a.proof_base), a.new_roots != nullptr);
  a.status[i] = st;
  if (a.new_roots) merkle_store_hash_or_zero(a.new_roots + 8 * i, root, ok);
  if (a.old_roots) {
    if (ok) merkle_fold_store(root, a.leaf_store, a.node_store, first, 64, nullptr, true);
    merkle_store_hash_or_zero(a.old_roots + 8 * i, root, ok);
  }
}

// ---- auditing a stored tree (row f-9: what nothing in ledger/ledger.py:70-114
// recoverTree or compact_merkle_tree.py verify_consistency checks, one lane per
// stored entry).  The store's invariant is local: the node at position q is
// SHA-256(0x01 | left | right) of two entries that are stored too, and leaf
// hash k is SHA-256(0x00 | leaf k).  One status byte per entry; 0 is never
// written by a lane.
constexpr uint8_t kAuditUnchecked = 0;  // EDV_AUDIT_* of include/edv.h
constexpr uint8_t kAuditOk = 1;
constexpr uint8_t kAuditBad = 2;

// The inverse of merkle_store_pos: the append that wrote 0-based node-store
// position q, as the 1-based leaf count s, and the node's height h in
// 1 .. ctz(s) (its block is (s >> h) - 1).  With f = merkle_node_count, s is
// the smallest value with f(s) > q and h = q - f(s - 1) + 1.  f never falls
// (f(s + 1) - f(s) = ctz(s + 1)) and s - 63 <= f(s) <= s - 1 for s <= 2^62, so
// s lies in [q + 2, q + 64]: six halvings.  Exact for q < merkle_node_count(2^62).
EDV_HD void merkle_store_node_at(uint64_t q, uint64_t* s, int* h) {
  uint64_t lo = q + 2, hi = q + 64;
#pragma unroll 1
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (merkle_node_count(mid) > q)
      hi = mid;
    else
      lo = mid + 1;
  }
  *s = lo;
  *h = int(q - merkle_node_count(lo - 1)) + 1;
}
// The two children of block k at height h >= 1: leaf-store entries 2k and
// 2k + 1 (h = 1, *leaves), else 0-based node-store positions.  Both are below
// the node's own append: a node at position q reads no node at or past q and
// no leaf at or past its s.
EDV_HD void merkle_node_children(int h, uint64_t k, bool* leaves, uint64_t* left, uint64_t* right) {
  *leaves = h == 1;
  if (h == 1) {
    *left = 2 * k;
    *right = 2 * k + 1;
  } else {
    *left = merkle_store_pos(h - 1, 2 * k) - 1;
    *right = merkle_store_pos(h - 1, 2 * k + 1) - 1;
  }
}

// One slice of the node store: positions [node_lo, node_lo + count), 0-based.
struct MerkleAuditNodes {
  const uint32_t* leaf_store;
  const uint32_t* node_store;
  uint64_t node_lo, count;
  uint8_t* status;  // one byte per position of the slice, or null
};
inline MerkleAuditNodes merkle_audit_nodes_args(const void* leaf_store, const void* node_store, uint64_t node_lo,
                                                uint64_t count, uint8_t* status) {
  return {static_cast<const uint32_t*>(leaf_store), static_cast<const uint32_t*>(node_store), node_lo, count, status};
}
// Lane i < a.count: is the node at position node_lo + i not the hash of its stored children?
EDV_HD bool merkle_audit_node_lane(const MerkleAuditNodes& a, uint64_t i) {
  const uint64_t q = a.node_lo + i;
  uint64_t s, left, right;
  int h;
  bool leaves;
  merkle_store_node_at(q, &s, &h);
  merkle_node_children(h, (s >> h) - 1, &leaves, &left, &right);
  const uint32_t* from = leaves ? a.leaf_store : a.node_store;
  uint32_t l[8], r[8], H[8], stored[8];
  merkle_load_hash(l, from + 8 * left);
  merkle_load_hash(r, from + 8 * right);
  merkle_load_hash(stored, a.node_store + 8 * q);
  merkle_node_hash(H, l, r);
  const bool bad = !merkle_hash_equal(H, stored);
  if (a.status) a.status[i] = bad ? kAuditBad : kAuditOk;
  return bad;
}

// One slice of the leaf store against the leaves' bytes: leaf i of the call is
// bytes [leaf_off[i], leaf_off[i + 1]) - leaf_base of `leaves` (the verify
// kernel's layout and rules: any alignment, readable 8 bytes past the end) and
// must hash to leaf-store entry leaf_lo + i, which is at 8 (leaf_lo + i -
// store_base) of leaf_store (store_base: the entry leaf_store points at; 0 for
// a whole store, leaf_lo where only the slice is at hand).
struct MerkleAuditLeaves {
  const uint32_t* leaf_store;
  uint64_t store_base, leaf_lo, n;
  const uint8_t* leaves;
  const uint64_t* leaf_off;
  uint64_t leaf_base;
  uint8_t* status;  // one byte per leaf of the slice, or null
};
inline MerkleAuditLeaves merkle_audit_leaves_args(const void* leaf_store, uint64_t store_base, uint64_t leaf_lo,
                                                  uint64_t n, const uint8_t* leaves, const uint64_t* leaf_off,
                                                  uint64_t leaf_base, uint8_t* status) {
  return {static_cast<const uint32_t*>(leaf_store), store_base, leaf_lo, n, leaves, leaf_off, leaf_base, status};
}
EDV_HD bool merkle_audit_leaf_lane(const MerkleAuditLeaves& a, uint64_t i) {
  const uint64_t o0 = a.leaf_off[i] - a.leaf_base, o1 = a.leaf_off[i + 1] - a.leaf_base;
  uint32_t H[8], stored[8];
  merkle_leaf_hash(H, a.leaves + o0, o1 - o0);
  merkle_load_hash(stored, a.leaf_store + 8 * (a.leaf_lo + i - a.store_base));
  const bool bad = !merkle_hash_equal(H, stored);
  if (a.status) a.status[i] = bad ? kAuditBad : kAuditOk;
  return bad;
}
// A launch's summary: the number of bad entries and the lowest bad position
// (0-based; UINT64_MAX: none).  Empty: {0, UINT64_MAX}; adding is commutative,
// so slices and workgroups accumulate into one in any order.
EDV_HD void merkle_audit_summary_init(uint64_t summary[2]) {
  summary[0] = 0;
  summary[1] = ~uint64_t(0);
}
// (host side) a slice's lanes one after another into summary
template <class Args, class Lane>
inline void merkle_audit_run(const Args& a, uint64_t count, uint64_t first_pos, uint64_t summary[2], Lane lane) {
  for (uint64_t i = 0; i < count; i++) {
    if (!lane(a, i)) continue;
    summary[0]++;
    if (first_pos + i < summary[1]) summary[1] = first_pos + i;
  }
}

// ---- catch-up (row f-10: what plenum/common/ledger_manager.py:505-609
// hasValidCatchupReplies / _add_txn do one reply at a time).  The call's n
// leaves are the transactions of `replies` replies in order: reply k ends at
// leaf reply_end[k] of the call (ends never fall; an empty reply repeats the
// end before it) and carries a consistency proof from the tree at its end,
// s = old_size + reply_end[k], to the catch-up target (final_size,
// final_root).  One lane per reply, after the extend's passes: the root of the
// tree of s leaves is a fold of hashes(s), every entry of which the old tree
// or the passes have (merkle_entry), so a transaction is hashed once and the
// replies' proofs are walked side by side.  The status is the walk's; RANGE
// also where the arrays do not describe the call (an end past n).
struct MerkleCatchup {
  MerkleAppend t;             // old_size, n and the three sources of merkle_entry; roots / paths unused
  uint64_t replies, final_size;
  const uint64_t* reply_end;  // leaves of the call in replies 0 .. k
  const uint32_t* final_root;
  const uint32_t* proofs;     // proof k: entries [proof_off[k], proof_off[k + 1]) - proof_base
  const uint64_t* proof_off;
  uint64_t proof_base;
  uint32_t* reply_roots;      // the root at reply k's end at 8 k, zeros where RANGE; or null
  uint8_t* status;
};
// ... from the call's arguments (host side; hashes at any pointer type)
inline MerkleCatchup merkle_catchup_args(uint64_t old_size, uint64_t n, const void* old_hashes, const void* leaf_hashes,
                                         const void* node_hashes, const uint64_t* reply_end, uint64_t replies,
                                         uint64_t final_size, const void* final_root, const void* proofs,
                                         const uint64_t* proof_off, uint64_t proof_base, void* reply_roots,
                                         uint8_t* status) {
  using H = const uint32_t*;
  return {{old_size, n, 0, H(old_hashes), H(leaf_hashes), H(node_hashes), nullptr, nullptr},
          replies, final_size, reply_end, H(final_root), H(proofs), proof_off, proof_base,
          static_cast<uint32_t*>(reply_roots), status};
}
// Lane k < a.replies.  The end is checked against n before it is added to
// old_size (old_size + n <= 2^62: no wrap below that); an end or a size out of
// range reads neither offsets nor hashes.
EDV_HD void merkle_catchup_lane(const MerkleCatchup& a, uint64_t k) {
  const uint64_t e = a.reply_end[k];
  uint32_t root[8];
  uint8_t st = kProofRange;
  if (e <= a.t.n && a.t.old_size + e <= a.final_size) {
    const uint64_t s = a.t.old_size + e;
    if (s == 0)
      merkle_empty_hash(root);
    else
      merkle_fold_entries(root, a.t, s);
    const uint64_t p0 = a.proof_off[k], p1 = a.proof_off[k + 1];
    uint32_t target[8], oldr[8], newr[8];
    bool walked;
    merkle_load_hash(target, a.final_root);
    st = merkle_verify_consistency_one(oldr, newr, &walked, s, a.final_size, root, target,
                                       a.proofs + 8 * (p0 - a.proof_base), p1 - p0);
  }
  a.status[k] = st;
  if (a.reply_roots) merkle_store_hash_or_zero(a.reply_roots + 8 * k, root, st != kProofRange);
}

}  // namespace edv

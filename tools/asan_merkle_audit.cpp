// asan_merkle_audit.cpp -- the store audit's header code (edv_merkle.h, row
// f-9: merkle_store_node_at, merkle_node_children, the two lane functions,
// and the extend from hashes) under AddressSanitizer and UBSan on the CPU, as
// a program of its own (tools/asan_merkle_audit.sh).  A tree is built with
// hc_merkle_extend; its two stores are heap blocks of exactly store_leaves and
// merkle_node_count(store_leaves) hashes, and hc_merkle_audit_* copies them
// into exact-size blocks of its own, so a lane that reads one entry at or past
// the counts is an ASan report.  Each store is then damaged (the table of
// tests/merkle_audit_cases.py) and what the lanes report is compared with the
// invariant restated forwards: every block (h, k) of the tree, by
// merkle_store_pos, against the hash of its two stored children.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "edv_hostcheck.cpp"

namespace {

uint64_t rng_state = 0x6962f9ull;
uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return uint32_t(rng_state >> 33);
}

int fails = 0;
void expect(bool ok, const char* what, uint64_t a, uint64_t b, uint64_t i) {
  if (ok) return;
  fails++;
  fprintf(stderr, "FAIL %s: %llu %llu at %llu\n", what, (unsigned long long)a, (unsigned long long)b,
          (unsigned long long)i);
}

struct Block {  // exact size; never null (size 0: one byte that nothing may touch)
  uint8_t* p;
  uint64_t bytes;
  explicit Block(uint64_t n) : p(static_cast<uint8_t*>(malloc(n ? n : 1))), bytes(n) {}
  Block(const Block& o) : Block(o.bytes) { memcpy(p, o.p, bytes); }
  ~Block() { free(p); }
};

// the bad positions of a store of s leaves, forwards
std::vector<uint64_t> forward_bad(const uint8_t* leaf_store, const uint8_t* node_store, uint64_t s) {
  std::vector<uint64_t> bad;
  for (int h = 1; (uint64_t(1) << h) <= s; h++)
    for (uint64_t k = 0; k < (s >> h); k++) {
      const uint64_t q = merkle_store_pos(h, k) - 1;
      const uint8_t *l, *r;
      if (h == 1) {
        l = leaf_store + 64 * k;
        r = l + 32;
      } else {
        l = node_store + 32 * (merkle_store_pos(h - 1, 2 * k) - 1);
        r = node_store + 32 * (merkle_store_pos(h - 1, 2 * k + 1) - 1);
      }
      uint32_t lw[8], rw[8], L[8], R[8], H[8], o[8];
      memcpy(lw, l, 32);
      memcpy(rw, r, 32);
      merkle_load_hash(L, lw);
      merkle_load_hash(R, rw);
      merkle_node_hash(H, L, R);
      merkle_store_hash(o, H);
      if (memcmp(o, node_store + 32 * q, 32)) bad.push_back(q);
    }
  std::sort(bad.begin(), bad.end());
  return bad;
}

void check_nodes(const char* what, const Block& leaf_store, const Block& node_store, uint64_t s, bool must_be_bad) {
  const uint64_t nodes = merkle_node_count(s);
  const std::vector<uint64_t> bad = forward_bad(leaf_store.p, node_store.p, s);
  if (must_be_bad) expect(!bad.empty(), what, s, 0, 0);
  // the whole store, and slices whose starts and lengths are no multiples of 64
  // (a large store: the whole, one odd slice and the last node, to keep the run short)
  const bool large = nodes > 4096;
  const std::vector<uint64_t> los = large ? std::vector<uint64_t>{0, 191, nodes - 1}
                                          : std::vector<uint64_t>{0, 1, nodes / 3, uint64_t(nodes > 191 ? 191 : 0),
                                                                  nodes ? nodes - 1 : 0};
  for (uint64_t lo : los) {
    if (lo > nodes) continue;
    const std::vector<uint64_t> counts = large ? std::vector<uint64_t>{lo == 191 ? nodes - lo - 65 : nodes - lo}
                                               : std::vector<uint64_t>{nodes - lo, (nodes - lo) / 2,
                                                                       uint64_t(nodes - lo ? 1 : 0)};
    for (uint64_t count : counts) {
      Block status(count);
      uint64_t summary[2] = {7, 7};
      expect(hc_merkle_audit_nodes(leaf_store.p, node_store.p, s, lo, count, status.p, summary) == 0, what, s, lo, count);
      uint64_t want_n = 0, want_first = ~uint64_t(0);
      for (uint64_t i = 0; i < count; i++) {
        const bool is_bad = std::binary_search(bad.begin(), bad.end(), lo + i);
        expect(status.p[i] == (is_bad ? kAuditBad : kAuditOk), what, s, lo, i);
        if (is_bad && !want_n++) want_first = lo + i;
      }
      expect(summary[0] == want_n && summary[1] == want_first, "summary", s, lo, count);
    }
  }
}

void flip(Block& b, uint64_t entry, int bit) { b.p[32 * entry + bit / 8] ^= uint8_t(1u << (bit % 8)); }

void run_tree(uint64_t s) {
  const uint64_t nodes = merkle_node_count(s);
  std::vector<uint64_t> off(s + 1, 0);
  for (uint64_t i = 0; i < s; i++) off[i + 1] = off[i] + rnd() % (s > 4096 ? 19 : 67);
  Block leaves(off[s] + 8), leaf_store(32 * s), node_store(32 * nodes), hashes(32 * 64), root(32);
  for (uint64_t k = 0; k < off[s] + 8; k++) leaves.p[k] = uint8_t(rnd());
  expect(hc_merkle_extend(0, nullptr, leaves.p, off.data(), s, leaf_store.p, node_store.p, hashes.p, root.p) == 0, "extend",
         s, 0, 0);
  check_nodes("clean", leaf_store, node_store, s, false);
  expect(forward_bad(leaf_store.p, node_store.p, s).empty(), "a clean store has no bad node", s, 0, 0);
  if (nodes) {
    int top = 0;
    while ((uint64_t(2) << top) <= s) top++;
    const uint64_t targets[] = {0, nodes - 1, merkle_store_pos(top, 0) - 1, merkle_store_pos(1, (s / 2) / 2) - 1};
    const char* names[] = {"first", "last", "highest", "height1"};
    for (int t = 0; t < 4; t++) {
      Block dam(node_store);
      flip(dam, targets[t], 5 + 60 * t);
      check_nodes(names[t], leaf_store, dam, s, true);
    }
    {
      Block dam(leaf_store);
      flip(dam, s > 3 ? ((s / 3) | 1) : 0, 9);
      check_nodes("leafhash", dam, node_store, s, true);
    }
    if (nodes >= 2) {
      Block dam(node_store);
      const uint64_t i = nodes / 3, j = nodes - 1;
      memcpy(dam.p + 32 * i, node_store.p + 32 * j, 32);
      memcpy(dam.p + 32 * j, node_store.p + 32 * i, 32);
      check_nodes("swap", leaf_store, dam, s, true);
    }
  }
  // a store cut short or lengthened by one node is the store of another count to these entry points: the slice
  // past the counts is refused, and the last slice that fits reads nothing behind the exact-size blocks
  uint64_t summary[2] = {7, 7};
  expect(hc_merkle_audit_nodes(leaf_store.p, node_store.p, s, nodes, 1, nullptr, summary) == -1, "past the counts", s, 0, 0);
  expect(hc_merkle_audit_nodes(leaf_store.p, node_store.p, s, 0, nodes + 1, nullptr, summary) == -1, "past the counts", s, 1, 0);
  expect(summary[0] == 7 && summary[1] == 7, "a refused call writes nothing", s, 0, 0);
  // the leaf store against the leaves' bytes, whole and in a slice, one hash damaged
  if (s) {
    Block dam(leaf_store), status(s);
    const uint64_t hit = s / 2;
    flip(dam, hit, 100);
    expect(hc_merkle_audit_leaves(leaf_store.p, s, 0, leaves.p, off.data(), s, status.p, summary) == 0, "audit leaves", s, 0, 0);
    expect(summary[0] == 0 && summary[1] == ~uint64_t(0), "clean leaves", s, 0, 0);
    expect(hc_merkle_audit_leaves(dam.p, s, 0, leaves.p, off.data(), s, status.p, summary) == 0, "audit leaves", s, 1, 0);
    expect(summary[0] == 1 && summary[1] == hit, "one bad leaf", s, hit, 0);
    for (uint64_t i = 0; i < s; i++) expect(status.p[i] == (i == hit ? kAuditBad : kAuditOk), "leaf status", s, hit, i);
    const uint64_t lo = s / 3, n = s - lo;
    expect(hc_merkle_audit_leaves(dam.p, s, lo, leaves.p, off.data() + lo, n, nullptr, summary) == 0, "audit leaves", s, 2, 0);
    expect(summary[0] == 1 && summary[1] == hit, "one bad leaf in a slice", s, hit, lo);
  }
  // extend from hashes: byte-identical to the extend, onto an empty tree and onto a prefix
  for (uint64_t old : {uint64_t(0), s / 3}) {
    const uint64_t n = s - old, span = nodes - merkle_node_count(old);
    Block oh(32 * 64), oroot(32), nh(32 * span), nnew(32 * 64), nroot(32);
    expect(hc_merkle_extend(0, nullptr, leaves.p, off.data(), old, nullptr, nullptr, oh.p, oroot.p) == 0, "prefix", s, old, 0);
    expect(hc_merkle_extend_hashed(old, oh.p, leaf_store.p + 32 * old, n, nh.p, nnew.p, nroot.p) == 0, "extend hashed", s,
           old, 0);
    expect(!memcmp(nh.p, node_store.p + 32 * merkle_node_count(old), 32 * span), "hashed nodes", s, old, 0);
    expect(!memcmp(nnew.p, hashes.p, 32 * size_t(popc64(s))) && !memcmp(nroot.p, root.p, 32), "hashed head", s, old, 0);
  }
}

// the inverse position function at sizes no store has
void run_positions() {
  const uint64_t top = uint64_t(1) << 62;
  for (uint64_t size : {top, top - 1, (uint64_t(1) << 40) + 1}) {
    const uint64_t nodes = merkle_node_count(size);
    for (int k = 0; k < 1002; k++) {
      const uint64_t q = k == 0 ? 0 : k == 1 ? nodes - 1 : ((uint64_t(rnd()) << 32) | rnd()) % nodes;
      uint64_t s;
      int32_t h;
      expect(hc_merkle_store_node_at(q, &s, &h) == 1, "node_at", size, q, 0);
      expect(h >= 1 && h <= 62 && s <= size && (s & ((uint64_t(1) << h) - 1)) == 0, "node_at range", size, q, s);
      expect(merkle_store_pos(h, (s >> h) - 1) - 1 == q, "node_at inverts store_pos", size, q, s);
    }
  }
  uint64_t s;
  int32_t h;
  expect(hc_merkle_store_node_at(merkle_node_count(top), &s, &h) == 0, "past the largest store", 0, 0, 0);
}

}  // namespace

int main() {
  const uint64_t t = kMerkleT;
  for (uint64_t s : {uint64_t(0), uint64_t(1), uint64_t(2), uint64_t(3), uint64_t(4), uint64_t(5), uint64_t(7), uint64_t(8),
                     uint64_t(9), t - 1, t, t + 1, uint64_t(1000), 2 * t * t + 3})
    run_tree(s);
  run_positions();
  if (fails) {
    fprintf(stderr, "%d failures\n", fails);
    return 1;
  }
  printf("asan_merkle_audit ok\n");
  return 0;
}

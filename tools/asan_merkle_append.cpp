// asan_merkle_append.cpp -- the batched append's header code (edv_merkle.h:
// merkle_popc_prefix, merkle_entry, merkle_append_leaf) under AddressSanitizer
// and UBSan on the CPU, as a program of its own (tools/asan_merkle_append.sh).
// Every buffer handed to hc_merkle_append_batch is a heap block of exactly the
// documented size, so a read or a store one hash too far is an ASan report.
// Results are checked against the extend itself: the root after leaf i is the
// root of extending by i + 1 leaves, and leaf i's audit path is the new hashes
// of extending by i leaves, reversed.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "edv_hostcheck.cpp"

namespace {

uint64_t rng_state = 0x6962f6ull;
uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return uint32_t(rng_state >> 33);
}

int fails = 0;
void expect(bool ok, const char* what, uint64_t old_size, uint64_t n, uint64_t i) {
  if (ok) return;
  fails++;
  fprintf(stderr, "FAIL %s: old %llu n %llu leaf %llu\n", what, (unsigned long long)old_size, (unsigned long long)n,
          (unsigned long long)i);
}

// exact-size heap blocks (never a null data() for size 0: one byte that nothing may touch)
struct Block {
  uint8_t* p;
  explicit Block(uint64_t bytes) : p(static_cast<uint8_t*>(malloc(bytes ? bytes : 1))) {}
  ~Block() { free(p); }
};

void run_case(uint64_t old_size, uint64_t n, int combo) {
  const bool want_roots = combo & 1, want_paths = combo & 2, want_leaf = combo & 4, want_node = combo & 8;
  const int nold = popc64(old_size);
  Block old_hashes(32 * uint64_t(nold));
  for (int k = 0; k < 32 * nold; k++) old_hashes.p[k] = uint8_t(rnd());
  std::vector<uint64_t> off(n + 1, 0);
  for (uint64_t i = 0; i < n; i++) off[i + 1] = off[i] + rnd() % 131;
  Block leaves(off[n] + 8);  // readable 8 bytes past the last leaf byte
  for (uint64_t k = 0; k < off[n] + 8; k++) leaves.p[k] = uint8_t(rnd());
  const uint64_t nodes = merkle_node_count(old_size + n) - merkle_node_count(old_size);
  const uint64_t entries = hc_merkle_path_entries(old_size, n);
  Block lh(32 * n), nh(32 * nodes), new_hashes(32 * uint64_t(popc64(old_size + n))), root(32), roots(32 * n),
      paths(32 * entries);
  const int rc = hc_merkle_append_batch(old_size, nold ? old_hashes.p : nullptr, leaves.p, off.data(), n,
                                        want_leaf ? lh.p : nullptr, want_node ? nh.p : nullptr, new_hashes.p, root.p,
                                        want_roots ? roots.p : nullptr, want_paths ? paths.p : nullptr);
  expect(rc == 0, "return code", old_size, n, 0);
  uint64_t at = 0, sum = 0;
  for (uint64_t i = 0; i < n; i++) {
    // the tree before leaf i and after it, by the extend alone
    Block before(32 * uint64_t(popc64(old_size + i))), r0(32), after(32 * uint64_t(popc64(old_size + i + 1))), r1(32);
    hc_merkle_extend(old_size, nold ? old_hashes.p : nullptr, leaves.p, off.data(), i, nullptr, nullptr, before.p, r0.p);
    hc_merkle_extend(old_size, nold ? old_hashes.p : nullptr, leaves.p, off.data(), i + 1, nullptr, nullptr, after.p,
                     r1.p);
    if (want_roots) expect(!memcmp(roots.p + 32 * i, r1.p, 32), "root", old_size, n, i);
    const int cnt = popc64(old_size + i);
    expect(hc_merkle_path_entries(old_size, i) == at, "path offset", old_size, n, i);
    if (want_paths)
      for (int e = 0; e < cnt; e++)
        expect(!memcmp(paths.p + 32 * (at + uint64_t(e)), before.p + 32 * (cnt - 1 - e), 32), "path", old_size, n, i);
    at += uint64_t(cnt);
    sum += uint64_t(cnt);
  }
  expect(sum == entries, "entry count", old_size, n, n);
  if (n && want_roots) expect(!memcmp(roots.p + 32 * (n - 1), root.p, 32), "last root", old_size, n, n - 1);
}

}  // namespace

int main() {
  const uint64_t olds[] = {0, 1, 2, 3, 255, 256, 257, 65535, 65536, (uint64_t(1) << 32) - 1,
                           (uint64_t(1) << 40) + (uint64_t(1) << 20) + 5, (uint64_t(1) << 62) - 600,
                           (uint64_t(1) << 62) - 65};
  const uint64_t ns[] = {0, 1, 2, 3, 63, 64, 65};
  for (uint64_t old_size : olds)
    for (uint64_t n : ns) run_case(old_size, n, 15);
  for (int combo = 0; combo < 16; combo++) {
    run_case(255, 130, combo);
    run_case((uint64_t(1) << 32) - 1, 67, combo);
  }
  run_case(255, 600, 3);  // three tiles: entries that are tile roots, hashes kept by the harness
  // the closed form where P itself wraps
  expect(hc_merkle_path_entries(0, 4) == 4, "P(4)", 0, 4, 0);
  expect(hc_merkle_path_entries((uint64_t(1) << 62) - 1, 1) == 62, "popcount(2^62 - 1)", 0, 1, 0);
  if (fails) {
    fprintf(stderr, "%d failures\n", fails);
    return 1;
  }
  printf("asan_merkle_append ok\n");
  return 0;
}

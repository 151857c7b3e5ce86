// asan_merkle_verify.cpp -- the proof verification's header code (edv_merkle.h:
// merkle_verify_inclusion_one, merkle_verify_consistency_one and the two lane
// functions) under AddressSanitizer and UBSan on the CPU, as a program of its
// own (tools/asan_merkle_verify.sh).  Every buffer handed to
// hc_merkle_verify_inclusion / hc_merkle_verify_consistency is a heap block of
// exactly the documented size (the leaves: 8 bytes more, their read-ahead
// allowance), and the harness copies them into exact-size blocks of its own, so
// a read past a proof's last entry or past a leaf's allowance is an ASan
// report.  Proofs are built from real trees (hc_merkle_append_batch's audit
// paths and roots), then shortened, lengthened and altered; statuses are
// checked against what each change must give.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "edv_hostcheck.cpp"

namespace {

uint64_t rng_state = 0x6962f7ull;
uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return uint32_t(rng_state >> 33);
}

int fails = 0;
void expect(bool ok, const char* what, uint64_t a, uint64_t b, uint64_t i) {
  if (ok) return;
  fails++;
  fprintf(stderr, "FAIL %s: %llu %llu proof %llu\n", what, (unsigned long long)a, (unsigned long long)b,
          (unsigned long long)i);
}

// exact-size heap blocks (never a null pointer for size 0: one byte that nothing may touch)
struct Block {
  uint8_t* p;
  explicit Block(uint64_t bytes) : p(static_cast<uint8_t*>(malloc(bytes ? bytes : 1))) {}
  ~Block() { free(p); }
};

uint64_t path_length(uint64_t index, uint64_t size) {
  uint64_t len = 0;
  for (uint64_t last = size - 1; last > 0; index >>= 1, last >>= 1)
    if ((index & 1) || index < last) len++;
  return len;
}

// The n appends onto a tree of old_size leaves with an arbitrary frontier: leaf
// i is leaf old_size + i of the tree of old_size + i + 1 leaves, its audit path
// and that tree's root are what the batched append returns.  All n proofs in
// one call: intact (OK), and per proof one change chosen by i % 5.
void run_appended(uint64_t old_size, uint64_t n, bool by_hash, bool want_computed) {
  const int nold = popc64(old_size);
  Block old_hashes(32 * uint64_t(nold));
  for (int k = 0; k < 32 * nold; k++) old_hashes.p[k] = uint8_t(rnd());
  std::vector<uint64_t> off(n + 1, 0);
  for (uint64_t i = 0; i < n; i++) off[i + 1] = off[i] + rnd() % 131;
  Block leaves(off[n] + 8);
  for (uint64_t k = 0; k < off[n] + 8; k++) leaves.p[k] = uint8_t(rnd());
  const uint64_t entries = hc_merkle_path_entries(old_size, n);
  Block lh(32 * n), new_hashes(32 * uint64_t(popc64(old_size + n))), root(32), roots(32 * n), paths(32 * entries);
  expect(hc_merkle_append_batch(old_size, nold ? old_hashes.p : nullptr, leaves.p, off.data(), n, lh.p, nullptr,
                                new_hashes.p, root.p, roots.p, paths.p) == 0,
         "append", old_size, n, 0);
  std::vector<uint64_t> index(n), size(n), poff(n + 1);
  for (uint64_t i = 0; i < n; i++) {
    index[i] = old_size + i;
    size[i] = old_size + i + 1;
    poff[i] = hc_merkle_path_entries(old_size, i);
    expect(path_length(index[i], size[i]) == uint64_t(popc64(old_size + i)), "path length", old_size, n, i);
  }
  poff[n] = entries;
  Block status(n), computed(32 * n);
  auto call = [&](const uint8_t* pr, const uint64_t* po, const uint8_t* rt, const uint64_t* ix) {
    return hc_merkle_verify_inclusion(by_hash ? nullptr : leaves.p, by_hash ? nullptr : off.data(),
                                      by_hash ? lh.p : nullptr, ix, size.data(), rt, pr, po, n, status.p,
                                      want_computed ? computed.p : nullptr);
  };
  expect(call(paths.p, poff.data(), roots.p, index.data()) == 0, "verify", old_size, n, 0);
  for (uint64_t i = 0; i < n; i++) {
    expect(status.p[i] == kProofOk, "intact proof", old_size, n, i);
    if (want_computed) expect(!memcmp(computed.p + 32 * i, roots.p + 32 * i, 32), "computed root", old_size, n, i);
  }
  if (n == 0) return;
  // changed: every proof re-packed into an exact-size block of its own layout
  std::vector<uint64_t> moff(n + 1, 0), mindex(index);
  std::vector<uint8_t> want(n);
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t len = poff[i + 1] - poff[i];
    uint64_t mlen = len;
    switch (i % 5) {
      case 0: want[i] = kProofOk; break;
      case 1: mlen = len ? len - 1 : 1; want[i] = len ? kProofShort : kProofLong; break;
      case 2: mlen = len + 1; want[i] = kProofLong; break;
      case 3: want[i] = kProofRoot; break;                        // a flipped bit, below
      default: mindex[i] = size[i]; want[i] = kProofRange; break;
    }
    moff[i + 1] = moff[i] + mlen;
  }
  Block mpaths(32 * moff[n]), mroots(32 * n);
  memcpy(mroots.p, roots.p, 32 * n);
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t len = poff[i + 1] - poff[i], mlen = moff[i + 1] - moff[i];
    for (uint64_t e = 0; e < mlen; e++) {
      if (e < len)
        memcpy(mpaths.p + 32 * (moff[i] + e), paths.p + 32 * (poff[i] + e), 32);
      else
        memset(mpaths.p + 32 * (moff[i] + e), 0x5a, 32);
    }
    if (i % 5 == 3) {
      if (len)
        mpaths.p[32 * moff[i] + rnd() % (32 * len)] ^= 0x10;
      else
        mroots.p[32 * i + 9] ^= 0x10;
    }
  }
  expect(call(mpaths.p, moff.data(), mroots.p, mindex.data()) == 0, "verify changed", old_size, n, 0);
  for (uint64_t i = 0; i < n; i++) expect(status.p[i] == want[i], "changed proof", old_size, n, i);
}

// Consistency of (old, new) without a tree: arbitrary entries of the right
// count; the roots the walk calculates make the proof good, and each change has
// its status.
void run_consistency(uint64_t old_size, uint64_t new_size) {
  uint64_t node = old_size - 1, last = new_size - 1, len = 0;
  while (node & 1) {
    node >>= 1;
    last >>= 1;
  }
  if (node) len = 1;
  for (; last > 0; node >>= 1, last >>= 1)
    if ((node & 1) || node < last) len++;
  const uint64_t n = 6;
  // proof k: 0 intact, 1 one entry short, 2 one entry more (accepted), 3 wrong new root, 4 wrong old root, 5 swapped sizes
  std::vector<uint64_t> poff(n + 1, 0), os(n, old_size), ns(n, new_size);
  for (uint64_t k = 0; k < n; k++) poff[k + 1] = poff[k] + (k == 1 ? len - 1 : k == 2 ? len + 1 : len);
  Block proofs(32 * poff[n]), old_roots(32 * n), new_roots(32 * n), status(n), computed(64 * n);
  Block base(32 * (len + 1));
  for (uint64_t k = 0; k < 32 * (len + 1); k++) base.p[k] = uint8_t(rnd());
  for (uint64_t k = 0; k < n; k++) memcpy(proofs.p + 32 * poff[k], base.p, 32 * (poff[k + 1] - poff[k]));
  for (uint64_t k = 0; k < 32 * n; k++) old_roots.p[k] = new_roots.p[k] = uint8_t(17 + k % 32);   // power of two: the seed
  // first pass: learn the roots the intact proof calculates
  expect(hc_merkle_verify_consistency(os.data(), ns.data(), old_roots.p, new_roots.p, proofs.p, poff.data(), 1, status.p,
                                      computed.p) == 0, "consistency", old_size, new_size, 0);
  expect(status.p[0] == kProofRoot, "arbitrary new root", old_size, new_size, 0);
  for (uint64_t k = 0; k < n; k++) {
    memcpy(old_roots.p + 32 * k, computed.p, 32);
    memcpy(new_roots.p + 32 * k, computed.p + 32, 32);
  }
  new_roots.p[32 * 3 + 4] ^= 1;
  old_roots.p[32 * 4 + 4] ^= 1;
  os[5] = new_size;
  ns[5] = old_size;
  expect(hc_merkle_verify_consistency(os.data(), ns.data(), old_roots.p, new_roots.p, proofs.p, poff.data(), n, status.p,
                                      computed.p) == 0, "consistency", old_size, new_size, 1);
  // a flipped old root that is the seed (old a power of two) moves the new root too
  const bool seed_is_root = (old_size & (old_size - 1)) == 0;
  const uint8_t want[6] = {kProofOk, kProofShort, kProofOk, kProofRoot,
                           seed_is_root ? kProofRoot : kProofInconsistent, kProofRange};
  for (uint64_t k = 0; k < n; k++) expect(status.p[k] == want[k], "consistency status", old_size, new_size, k);
  expect(!memcmp(computed.p, old_roots.p, 32) && !memcmp(computed.p + 32, new_roots.p, 32), "computed roots", old_size,
         new_size, 0);
}

}  // namespace

int main() {
  const uint64_t olds[] = {0, 1, 2, 3, 255, 256, 257, 65535, (uint64_t(1) << 32) - 1,
                           (uint64_t(1) << 40) + (uint64_t(1) << 20) + 5, (uint64_t(1) << 62) - 600};
  const uint64_t ns[] = {0, 1, 2, 63, 64, 65};
  for (uint64_t old_size : olds)
    for (uint64_t n : ns) {
      run_appended(old_size, n, false, true);
      run_appended(old_size, n, true, (n & 1) != 0);
    }
  run_appended(255, 257, false, false);
  const uint64_t top = ~uint64_t(0);
  const uint64_t pairs[][2] = {{1, 2}, {2, 3}, {3, 4}, {4, 7}, {6, 7}, {7, 8}, {255, 256}, {256, 257}, {192, 257},
                               {1, top}, {top - 1, top}, {uint64_t(1) << 32, (uint64_t(1) << 63) + 5},
                               {(uint64_t(1) << 63) + 4, (uint64_t(1) << 63) + 5}, {(uint64_t(3) << 61), top}};
  for (const auto& p : pairs) run_consistency(p[0], p[1]);
  // inclusion at the largest sizes, arbitrary entries: the walk takes exactly path_length entries
  {
    const uint64_t size[3] = {top, top, (uint64_t(1) << 63) + 5}, index[3] = {top - 1, 0, (uint64_t(1) << 63) + 4};
    uint64_t poff[4] = {0, 0, 0, 0};
    for (int k = 0; k < 3; k++) poff[k + 1] = poff[k] + path_length(index[k], size[k]);
    Block proofs(32 * poff[3]), lh(96), roots(96), status(3), computed(96);
    for (uint64_t k = 0; k < 32 * poff[3]; k++) proofs.p[k] = uint8_t(rnd());
    for (int k = 0; k < 96; k++) lh.p[k] = roots.p[k] = uint8_t(rnd());
    hc_merkle_verify_inclusion(nullptr, nullptr, lh.p, index, size, roots.p, proofs.p, poff, 3, status.p, computed.p);
    for (int k = 0; k < 3; k++) expect(status.p[k] == kProofRoot, "arbitrary root", index[k], size[k], uint64_t(k));
    hc_merkle_verify_inclusion(nullptr, nullptr, lh.p, index, size, computed.p, proofs.p, poff, 3, status.p, nullptr);
    for (int k = 0; k < 3; k++) expect(status.p[k] == kProofOk, "calculated root", index[k], size[k], uint64_t(k));
    expect(poff[1] == 63 && poff[2] - poff[1] == 64, "path lengths at 2^64 - 1", 0, 0, 0);
  }
  if (fails) {
    fprintf(stderr, "%d failures\n", fails);
    return 1;
  }
  printf("asan_merkle_verify ok\n");
  return 0;
}

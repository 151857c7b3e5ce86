// asan_merkle_prove.cpp -- the proof generation's header code (edv_merkle.h, row
// f-8: merkle_walk_next, merkle_prove_one, merkle_fold_store and the two lane
// functions) under AddressSanitizer and UBSan on the CPU, as a program of its
// own (tools/asan_merkle_prove.sh).  A tree is built with hc_merkle_extend; its
// two stores are heap blocks of exactly store_leaves and
// merkle_node_count(store_leaves) hashes, the slots one of exactly the proofs'
// entries, and hc_merkle_prove_* copies them into exact-size blocks of its own,
// so a lane that reads a store position at or past the counts, or writes an
// entry outside its slot, is an ASan report.  What comes out is then checked by
// the verification lanes (hc_merkle_verify_*): every proof made must verify
// against the roots made with it.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "edv_hostcheck.cpp"

namespace {

uint64_t rng_state = 0x6962f8ull;
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

struct Block {  // exact size; never null (size 0: one byte that nothing may touch)
  uint8_t* p;
  explicit Block(uint64_t bytes) : p(static_cast<uint8_t*>(malloc(bytes ? bytes : 1))) {}
  ~Block() { free(p); }
};

// every pair of a tree of s leaves whose store is exactly that tree
void run_tree(uint64_t s) {
  std::vector<uint64_t> off(s + 1, 0);
  for (uint64_t i = 0; i < s; i++) off[i + 1] = off[i] + rnd() % 67;
  Block leaves(off[s] + 8), leaf_store(32 * s), node_store(32 * merkle_node_count(s)), hashes(32 * 64), root(32);
  for (uint64_t k = 0; k < off[s] + 8; k++) leaves.p[k] = uint8_t(rnd());
  expect(hc_merkle_extend(0, nullptr, leaves.p, off.data(), s, leaf_store.p, node_store.p, hashes.p, root.p) == 0, "extend",
         s, 0, 0);
  // inclusion: all (m, n), n <= s, with exact slots; then verified
  std::vector<uint64_t> idx, size;
  for (uint64_t n = 1; n <= s; n++)
    for (uint64_t m = 0; m < n; m++) {
      idx.push_back(m);
      size.push_back(n);
    }
  idx.push_back(s);  // RANGE: no slot
  size.push_back(s);
  idx.push_back(0);
  size.push_back(s + 1);
  const uint64_t n = idx.size();
  std::vector<uint64_t> poff(n + 1);
  hc_merkle_prove_offsets(0, idx.data(), size.data(), n, s, poff.data());
  {
    Block proofs(32 * poff[n]), status(n), roots(32 * n), lh(32 * n), vstatus(n);
    expect(hc_merkle_prove_inclusion(leaf_store.p, node_store.p, s, idx.data(), size.data(), poff.data(), n, proofs.p,
                                     status.p, roots.p, lh.p) == 0, "prove inclusion", s, n, 0);
    expect(hc_merkle_verify_inclusion(nullptr, nullptr, lh.p, idx.data(), size.data(), roots.p, proofs.p, poff.data(), n,
                                      vstatus.p, nullptr) == 0, "verify made", s, n, 0);
    for (uint64_t i = 0; i < n; i++) {
      const bool bad = i + 2 >= n;
      expect(status.p[i] == (bad ? kProofRange : kProofOk), "inclusion status", idx[i], size[i], i);
      if (!bad) expect(vstatus.p[i] == kProofOk, "made proof verifies", idx[i], size[i], i);
      if (!bad && size[i] == s) expect(!memcmp(roots.p + 32 * i, root.p, 32), "tree head", idx[i], size[i], i);
    }
    // every slot one entry short or long: SPACE, nothing written; without roots
    std::vector<uint64_t> moff(n + 1, 0);
    for (uint64_t i = 0; i < n; i++) {
      const uint64_t len = poff[i + 1] - poff[i];
      moff[i + 1] = moff[i] + ((i & 1) && len ? len - 1 : len + 1);
    }
    Block mproofs(32 * moff[n]);
    memset(mproofs.p, 0x5a, 32 * moff[n]);
    expect(hc_merkle_prove_inclusion(leaf_store.p, node_store.p, s, idx.data(), size.data(), moff.data(), n, mproofs.p,
                                     status.p, nullptr, nullptr) == 0, "prove misfit", s, n, 0);
    for (uint64_t i = 0; i + 2 < n; i++) expect(status.p[i] == kProofSpace, "misfit status", idx[i], size[i], i);
    for (uint64_t k = 0; k < 32 * moff[n]; k++)
      if (mproofs.p[k] != 0x5a) {
        expect(false, "misfit slot written", s, k, 0);
        break;
      }
  }
  // consistency: all (a, b), 1 <= a <= b <= s
  std::vector<uint64_t> first, second;
  for (uint64_t b = 1; b <= s; b++)
    for (uint64_t a = 1; a <= b; a++) {
      first.push_back(a);
      second.push_back(b);
    }
  first.push_back(0);  // RANGE
  second.push_back(s);
  const uint64_t nc = first.size();
  std::vector<uint64_t> coff(nc + 1);
  hc_merkle_prove_offsets(1, first.data(), second.data(), nc, s, coff.data());
  Block proofs(32 * coff[nc]), status(nc), old_roots(32 * nc), new_roots(32 * nc), vstatus(nc);
  expect(hc_merkle_prove_consistency(leaf_store.p, node_store.p, s, first.data(), second.data(), coff.data(), nc, proofs.p,
                                     status.p, old_roots.p, new_roots.p) == 0, "prove consistency", s, nc, 0);
  expect(hc_merkle_verify_consistency(first.data(), second.data(), old_roots.p, new_roots.p, proofs.p, coff.data(), nc,
                                      vstatus.p, nullptr) == 0, "verify made", s, nc, 1);
  for (uint64_t i = 0; i + 1 < nc; i++) {
    expect(status.p[i] == kProofOk, "consistency status", first[i], second[i], i);
    expect(vstatus.p[i] == kProofOk, "made consistency proof verifies", first[i], second[i], i);
  }
  expect(status.p[nc - 1] == kProofRange, "first == 0", 0, s, nc - 1);
}

// the walk alone at sizes no store has: entry counts and kinds stay in bounds
void run_walks() {
  const uint64_t top = uint64_t(1) << 62;
  const uint64_t sizes[] = {top, top - 1, (uint64_t(1) << 32) + 1, (uint64_t(1) << 61) + (uint64_t(1) << 33) + 5};
  for (uint64_t n : sizes)
    for (int k = 0; k < 62; k++)
      for (uint64_t a : {(uint64_t(1) << k) - 1, (uint64_t(1) << k) + 1, n - 1 - uint64_t(k)}) {
        if (a >= n) continue;
        Block kind(kMerkleMaxProof), off(8 * kMerkleMaxProof);
        const int ci = hc_merkle_proof_positions(0, a, n, kind.p, reinterpret_cast<uint64_t*>(off.p));
        expect(ci >= 0 && uint64_t(ci) == hc_merkle_inclusion_length(a, n), "inclusion positions", a, n, 0);
        const int cc = hc_merkle_proof_positions(1, a + 1, n, kind.p, reinterpret_cast<uint64_t*>(off.p));
        expect(cc >= 0 && uint64_t(cc) == hc_merkle_consistency_length(a + 1, n), "consistency positions", a + 1, n, 0);
      }
}

}  // namespace

int main() {
  for (uint64_t s : {1, 2, 3, 7, 8, 11, 33, 64, 65, 100}) run_tree(s);
  run_walks();
  if (fails) {
    fprintf(stderr, "%d failures\n", fails);
    return 1;
  }
  printf("asan_merkle_prove ok\n");
  return 0;
}

// asan_merkle_catchup.cpp -- the catch-up lane's header code (edv_merkle.h:
// merkle_fold_entries, merkle_entry, merkle_catchup_lane over the extend's
// passes) under AddressSanitizer and UBSan on the CPU, as a program of its own
// (tools/asan_merkle_catchup.sh).  Leaves, reply ends, proofs and outputs
// handed to hc_merkle_catchup are heap blocks of exactly the documented sizes
// (the leaves: 8 bytes more, their read-ahead allowance), and the harness copies
// them into exact-size blocks of its own, so a lane reading an entry past its
// proof, a hash past the call's or storing a root too far is an ASan report.
// Proofs come from real trees (hc_merkle_prove_consistency over the stores
// hc_merkle_extend wrote), then are shortened and lengthened, a transaction is
// altered and the target moved; statuses are checked against what each change
// must give.  A tree of 2^40 + 5 leaves with arbitrary entries runs for its
// addresses alone.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "edv_hostcheck.cpp"

namespace {

uint64_t rng_state = 0xf10ca7ull;
uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return uint32_t(rng_state >> 33);
}

int fails = 0;
void expect(bool ok, const char* what, uint64_t a, uint64_t b, uint64_t i) {
  if (ok) return;
  fails++;
  fprintf(stderr, "FAIL %s: %llu %llu reply %llu\n", what, (unsigned long long)a, (unsigned long long)b,
          (unsigned long long)i);
}

// exact-size heap blocks (never a null pointer for size 0: one byte that nothing may touch)
struct Block {
  uint8_t* p;
  explicit Block(uint64_t bytes) : p(static_cast<uint8_t*>(malloc(bytes ? bytes : 1))) {}
  ~Block() { free(p); }
};

enum Change { kIntact, kCut, kExtra, kTxn, kBelow };

// The tree of old_size + sum(counts) + extra random leaves; the replies are
// counts[k] leaves each from leaf old_size on; change applies to reply j.
void run_real(uint64_t old_size, const std::vector<uint64_t>& counts, uint64_t extra, Change change, uint64_t j) {
  const uint64_t replies = counts.size();
  uint64_t n = 0;
  std::vector<uint64_t> ends(replies);
  for (uint64_t k = 0; k < replies; k++) ends[k] = (n += counts[k]);
  const uint64_t total = old_size + n + extra;
  std::vector<uint64_t> off(total + 1, 0);
  for (uint64_t i = 0; i < total; i++) off[i + 1] = off[i] + 1 + rnd() % 130;
  Block leaves(off[total] + 8);
  for (uint64_t k = 0; k < off[total] + 8; k++) leaves.p[k] = uint8_t(rnd());
  Block leaf_store(32 * total), node_store(32 * merkle_node_count(total)), top(32 * uint64_t(popc64(total))), final_root(32);
  expect(hc_merkle_extend(0, nullptr, leaves.p, off.data(), total, leaf_store.p, node_store.p, top.p, final_root.p) == 0,
         "whole tree", old_size, n, 0);
  Block old_hashes(32 * uint64_t(popc64(old_size))), old_root(32);
  expect(hc_merkle_extend(0, nullptr, leaves.p, off.data(), old_size, nullptr, nullptr, old_hashes.p, old_root.p) == 0,
         "old tree", old_size, n, 0);
  // the proofs, packed; a reply that ends at size 0 or at the target has none
  uint64_t final_size = total;
  std::vector<uint64_t> poff(replies + 1, 0), len(replies);
  for (uint64_t k = 0; k < replies; k++) {
    const uint64_t s = old_size + ends[k];
    len[k] = s && s < total ? merkle_consistency_length(s, total) : 0;
    uint64_t mlen = len[k];
    if (k == j && change == kCut && mlen) mlen--;
    if (k == j && change == kExtra) mlen++;
    poff[k + 1] = poff[k] + mlen;
  }
  Block proofs(32 * poff[replies]), heads(32 * replies);
  for (uint64_t k = 0; k < replies; k++) {
    const uint64_t s = old_size + ends[k], mlen = poff[k + 1] - poff[k];
    Block whole(32 * (len[k] + 1)), st(1);
    memset(whole.p, 0x5a, 32 * (len[k] + 1));
    if (len[k]) {
      const uint64_t po[2] = {0, len[k]};
      expect(hc_merkle_prove_consistency(leaf_store.p, node_store.p, total, &s, &total, po, 1, whole.p, st.p, heads.p + 32 * k,
                                         nullptr) == 0 && st.p[0] == kProofOk, "prove", s, total, k);
    } else if (s == 0) {
      uint32_t H[8], bytes[8];
      merkle_empty_hash(H);
      merkle_store_hash(bytes, H);
      memcpy(heads.p + 32 * k, bytes, 32);
    } else {
      memcpy(heads.p + 32 * k, final_root.p, 32);
    }
    memcpy(proofs.p + 32 * poff[k], whole.p, 32 * mlen);
  }
  if (change == kTxn) leaves.p[off[old_size + ends[j] - 1]] ^= 0x20;  // the first byte of reply j's last leaf
  if (change == kBelow) final_size = old_size + ends[j] - 1;
  Block lh(32 * n), nh(32 * (merkle_node_count(old_size + n) - merkle_node_count(old_size))), rr(32 * replies), status(replies);
  expect(hc_merkle_catchup(old_size, old_size ? old_hashes.p : nullptr, leaves.p, off.data() + old_size, n, ends.data(),
                           replies, final_size, final_root.p, proofs.p, poff.data(), lh.p, nh.p, rr.p, status.p) == 0,
         "catchup", old_size, n, 0);
  for (uint64_t k = 0; k < replies; k++) {
    const uint64_t s = old_size + ends[k];
    uint8_t want = kProofOk;
    bool exact = true;
    if (change == kCut && k == j && len[k]) want = kProofShort;
    if (change == kTxn && k >= j) exact = false;  // ROOT or INCONSISTENT by the size: the Python model tells them apart
    if (change == kBelow) {
      // a reply that ends at or below the moved target walks its proof against a size it was not made for:
      // where the two sizes ask for the same siblings the walk still arrives (the size is not hashed), so
      // only the statuses past the target are known here
      if (s <= final_size) continue;
      want = kProofRange;
    }
    if (exact)
      expect(status.p[k] == want, "status", old_size, n, k);
    else
      expect(status.p[k] != kProofOk && status.p[k] != kProofUnverified, "rejection", old_size, n, k);
    if (change != kTxn && change != kBelow) expect(!memcmp(rr.p + 32 * k, heads.p + 32 * k, 32), "reply root", old_size, n, k);
  }
  if (change != kTxn) {
    expect(!memcmp(lh.p, leaf_store.p + 32 * old_size, 32 * n), "leaf hashes", old_size, n, 0);
    expect(!memcmp(nh.p, node_store.p + 32 * merkle_node_count(old_size),
                   32 * (merkle_node_count(old_size + n) - merkle_node_count(old_size))), "node hashes", old_size, n, 0);
  }
  // the optional outputs left out: the lanes' hashes are kept by the harness
  Block status2(replies);
  expect(hc_merkle_catchup(old_size, old_size ? old_hashes.p : nullptr, leaves.p, off.data() + old_size, n, ends.data(),
                           replies, final_size, final_root.p, proofs.p, poff.data(), nullptr, nullptr, nullptr,
                           status2.p) == 0 && !memcmp(status.p, status2.p, replies), "without outputs", old_size, n, 0);
}

// An old tree far above 2^32 with arbitrary entries and arbitrary proofs of the
// walk's exact length, then one entry short: addresses only, no status is OK.
void run_synthetic(uint64_t old_size, const std::vector<uint64_t>& counts, uint64_t extra, bool cut) {
  const uint64_t replies = counts.size();
  uint64_t n = 0;
  std::vector<uint64_t> ends(replies), poff(replies + 1, 0), off;
  for (uint64_t k = 0; k < replies; k++) ends[k] = (n += counts[k]);
  off.assign(n + 1, 0);
  for (uint64_t i = 0; i < n; i++) off[i + 1] = off[i] + rnd() % 70;
  const uint64_t final_size = old_size + n + extra, nold = uint64_t(popc64(old_size));
  for (uint64_t k = 0; k < replies; k++)
    poff[k + 1] = poff[k] + merkle_consistency_length(old_size + ends[k], final_size) - (cut ? 1 : 0);
  Block leaves(off[n] + 8), old_hashes(32 * nold), proofs(32 * poff[replies]), root(32), status(replies), rr(32 * replies);
  for (uint64_t k = 0; k < off[n] + 8; k++) leaves.p[k] = uint8_t(rnd());
  for (uint64_t k = 0; k < 32 * nold; k++) old_hashes.p[k] = uint8_t(rnd());
  for (uint64_t k = 0; k < 32 * poff[replies]; k++) proofs.p[k] = uint8_t(rnd());
  for (int k = 0; k < 32; k++) root.p[k] = uint8_t(rnd());
  expect(hc_merkle_catchup(old_size, old_hashes.p, leaves.p, off.data(), n, ends.data(), replies, final_size, root.p, proofs.p,
                           poff.data(), nullptr, nullptr, rr.p, status.p) == 0, "synthetic", old_size, n, 0);
  for (uint64_t k = 0; k < replies; k++)
    expect(status.p[k] == (cut ? kProofShort : kProofRoot), "synthetic status", old_size, n, k);
}

}  // namespace

int main() {
  const std::vector<std::vector<uint64_t>> shapes0 = {{1}, {0, 1}, {3, 1, 4}}, shapes1 = {{1}, {3, 0, 4}, {8}};
  for (uint64_t extra : {uint64_t(0), uint64_t(37)}) {
    for (const auto& c : shapes0) run_real(0, c, extra, kIntact, 0);
    for (uint64_t old_size : {uint64_t(1), uint64_t(5), uint64_t(8)})
      for (const auto& c : shapes1) run_real(old_size, c, extra, kIntact, 0);
    for (uint64_t old_size : {uint64_t(255), uint64_t(256), uint64_t(257)}) {
      run_real(old_size, {256, 2, 255}, extra, kIntact, 0);
      for (uint64_t j = 0; j < 3; j++)
        for (Change ch : {kCut, kExtra, kTxn, kBelow}) run_real(old_size, {256, 2, 255}, extra, ch, j);
    }
    for (uint64_t j = 0; j < 3; j++)
      for (Change ch : {kCut, kExtra, kTxn, kBelow}) {
        run_real(0, {3, 1, 4}, extra, ch, j);
        if (j != 1) run_real(5, {3, 0, 4}, extra, ch, j);  // reply 1 is empty: it has no transaction to alter
      }
  }
  run_synthetic((uint64_t(1) << 40) + 5, {2, 3}, 3, false);
  run_synthetic((uint64_t(1) << 40) + 5, {2, 3}, 3, true);
  run_synthetic((uint64_t(1) << 62) - 600, {1, 256, 7}, 1, false);
  if (fails) {
    fprintf(stderr, "%d failures\n", fails);
    return 1;
  }
  printf("asan_merkle_catchup ok\n");
  return 0;
}

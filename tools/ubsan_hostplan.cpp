// ubsan_hostplan.cpp -- TESTS ONLY (tests/test_hostplan_cpu.py).  The host
// paths' arithmetic of edv_hostplan.h on the CPU over the sweeps of that test,
// for a build with
//   g++ -std=c++17 -fsanitize=undefined,address -fno-sanitize-recover=all
// The header's functions index rb[] and shift and divide by what they are
// given: the sanitizers abort the run on a write past rb[kSlices], a division
// by zero or an overflowing shift, and the properties a caller relies on (the
// slices and sub-batches partition the shard, nothing exceeds its scratch, the
// Merkle buffers hold what a call of either form reads and writes, for tree
// sizes up to 2^62) are checked here.  Prints "ok <cases> <checksum>" over every result.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <initializer_list>
#include "../indy-plenum_amd/csrc/edv_hostplan.h"

using namespace edv;

namespace {
constexpr uint64_t kN[] = {0,    1,    255,   256,   257,   511,    512,
                           513,  4096, 4097,  65535, 65536, 65537,  262144, (uint64_t(1) << 32) + 1};
constexpr uint64_t kChunks[] = {256, 512, 768, uint64_t(1) << 18};
constexpr uint64_t kBlock = 256;
uint64_t sum = 0, cases = 0;
void eat(uint64_t v) { sum = sum * 0x100000001b3ULL ^ v; }
void must(bool ok, const char* what, uint64_t n, uint64_t x) {
  if (ok) return;
  fprintf(stderr, "%s: n = %llu, %llu\n", what, (unsigned long long)n, (unsigned long long)x);
  exit(1);
}
}  // namespace

int main() {
  for (uint64_t n : kN) {
    const PackedLayout l = packed_layout(n, 700 * n + 3);
    must(l.pks == 64 * n && l.off == 96 * n && l.msgs == 104 * n + 8 && l.padded == l.bytes + 64, "layout", n, 0);
    eat(l.padded);
    cases++;
    // the single-copy test: gaps from exact fit to past the limit, aligned and not, and the regions swapped
    const uint64_t s = 0x7F0000001000ULL, p = s + 64 * n, o = s + 96 * n;
    for (uint64_t gap : {0, 4, 8, 16, 24, 4096, 4104}) {
      const OneSpan a = one_span(s, p, o + gap, n), b = one_span(s, p + gap, o + gap, n), c = one_span(p, s, o, n),
                    d = one_span(s, o, p, n), e = one_span(o + gap, p, s, n);
      must(a.one == (gap % 8 == 0 && gap <= 4096), "span: gap before the offsets", n, gap);
      must(b.one == (gap % 16 == 0 && gap <= 4096), "span: gap before the keys", n, gap);
      must(n == 0 || (!c.one && !d.one && !e.one), "span: swapped regions", n, gap);
      for (const OneSpan& x : {a, b, c, d, e}) {
        must(x.one || (x.gp == 64 * n && x.go == 96 * n && x.span == 104 * n + 8), "span: packed fallback", n, gap);
        must(x.gp >= 64 * n && x.go >= x.gp + 32 * n && x.span == x.go + 8 * (n + 1), "span: order", n, gap);
        eat(x.span);
        cases++;
      }
    }
    for (int hs = 0; hs < 10; hs++)
      for (int bucketed = 0; bucketed < 2; bucketed++) {
        uint64_t rb[kSlices + 1];
        const int K = field_slices(n, hs, bucketed != 0, kBlock, rb);
        must(K >= 1 && K <= kSlices && (!bucketed || K == 1), "slices: K", n, uint64_t(K));
        must(rb[0] == 0 && rb[K] == n, "slices: ends", n, uint64_t(K));
        for (int k = 0; k < K; k++) must(rb[k] <= rb[k + 1] && rb[k] % kBlock == 0, "slices: bounds", n, uint64_t(k));
        eat(uint64_t(K));
        cases++;
      }
    for (uint64_t chunk : kChunks) {
      const SubSplit sp = sub_split(n, chunk, kBlock);
      must(uint64_t(sp.Q) * sp.pmax <= chunk && sp.P <= sp.pmax, "split: scratch", n, chunk);
      must(n == 0 || ((sp.nsub - 1) * sp.P < n && n <= sp.nsub * sp.P), "split: partition", n, chunk);
      must(n == 0 || (sp.nsub == 1) == (n <= chunk), "split: one chunk is one sub-batch", n, chunk);
      const uint64_t cap = chunk_capacity(n < chunk ? n : chunk, chunk);
      must(cap >= (n < chunk ? n : chunk) && cap <= chunk, "capacity", n, chunk);
      const TrimLimits t = trim_limits(n, chunk);
      must(t.slots == (n ? cap : 0) && t.msgs == n * kTrimMsgBytes + 64, "trim: slots / msgs", n, chunk);
      must(n == 0 || (t.stage == pinned_capacity(t.blob) && t.blob >= packed_layout(n, n * kTrimMsgBytes).padded &&
                      t.off >= 8 * (n + sp.nsub)),
           "trim: a batch of keep requests survives", n, chunk);
      eat(sp.nsub ^ cap ^ t.stage ^ t.off);
      cases++;
    }
  }
  // the Merkle buffers' sizes: tree sizes up to old + n = 2^62, every combination of the outputs, both forms
  for (uint64_t old : {uint64_t(0), uint64_t(1), uint64_t(255), uint64_t(256), uint64_t(257), (uint64_t(1) << 20) + 12345,
                       kMerkleMaxSize - 300})
    for (uint64_t n : {0, 1, 255, 256, 257, 300})
      for (int bits = 0; bits < 32; bits++) {
        const bool host = bits & 16, leaf = bits & 1, node = bits & 2, roots = bits & 4, paths = bits & 8;
        const MerkleSizes s = merkle_extend_needs(old, n, 700 * n + 3, host, leaf, node, roots, paths);
        const uint64_t nodes = merkle_node_count(old + n) - merkle_node_count(old);
        must(s[mk_roots] == 32 * merkle_scratch_hashes(old, old + n) && s[mk_roots] <= 32 * (n / (kMerkleT - 1) + 16),
             "merkle: tile-root scratch", old, n);
        must(host ? s[mk_fleafh] == 0 && s[mk_fnodeh] == 0 && s[mk_off] == 8 * (n + 1) && s[mk_paths] <= 32 * 63 * n
                  : s[mk_leaves] == 0 && s[mk_leafh] == 0 && s[mk_nodeh] == 0 && s[mk_aroots] == 0 && s[mk_paths] == 0,
             "merkle: a form touches the other's buffers", old, n);
        // with per-leaf outputs the fold finds the leaf and node hashes somewhere: the caller's buffer or one of these
        if (n && (roots || paths))
          must((host ? s[mk_leafh] : leaf ? 32 * n : s[mk_fleafh]) == 32 * n &&
                   (host ? s[mk_nodeh] : node ? 32 * nodes : s[mk_fnodeh]) == 32 * nodes,
               "merkle: the fold's hashes", old, n);
        for (int i = mv_leaves; i < kMerkleBufs; i++) must(s[i] == 0, "merkle: an extend touches a verify buffer", old, n);
        for (uint64_t v : s) eat(v);
        cases++;
      }
  for (uint64_t n : {1, 255, 256, 257, 300, 4097})
    for (uint64_t entries : {uint64_t(0), uint64_t(1), 64 * n})
      for (int bits = 0; bits < 4; bits++) {
        const MerkleSizes s = merkle_verify_needs(bits & 1, n, 300 * n + 1, entries, bits & 2);
        must(s[mv_proofs] >= 32 && s[mv_proofs] >= 32 * entries && s[mv_out] >= n && s[mv_words] >= 8 * (3 * n + 1 + (bits & 1) * (n + 1)),
             "merkle verify: staging", n, entries);
        for (int i = 0; i < mv_leaves; i++) must(s[i] == 0, "merkle verify: touches an extend buffer", n, entries);
        for (uint64_t v : s) eat(v);
        cases++;
      }
  for (uint64_t keep : {uint64_t(0), uint64_t(1), uint64_t(254), uint64_t(255), uint64_t(256), uint64_t(400), uint64_t(1) << 20}) {
    const MerkleSizes t = merkle_trim_limits(keep, trim_limits(keep, uint64_t(1) << 18));
    // what extending a tree by `keep` leaves of kTrimMsgBytes, or verifying as many proofs of 64 entries, needs survives
    // (but for the node hashes, limited to 32 keep: n leaves make up to n + popcount(old) - 1 nodes)
    const uint64_t old = (uint64_t(1) << 20) + 12345;
    for (int host = 0; host < 2; host++) {
      const MerkleSizes s = merkle_extend_needs(old, keep, kTrimMsgBytes * keep, host, false, false, true, true);
      for (int i = 0; i < kMerkleBufs; i++) {
        const uint64_t slack = i == mk_nodeh || i == mk_fnodeh ? 32 * uint64_t(popc64(old)) : 0;
        must(!keep ? t[i] == 0 : s[i] <= t[i] + slack, "merkle trim: an extend of keep leaves", keep, i);
      }
    }
    for (int incl = 0; incl < 2; incl++) {
      const MerkleSizes s = merkle_verify_needs(incl, keep, kTrimMsgBytes * keep, 64 * keep, true);
      for (int i = 0; i < kMerkleBufs; i++) must(!keep || s[i] <= t[i], "merkle trim: a verify of keep proofs", keep, i);
    }
    for (uint64_t v : t) eat(v);
    cases++;
  }
  printf("ok %llu %016llx\n", (unsigned long long)cases, (unsigned long long)sum);
  return 0;
}

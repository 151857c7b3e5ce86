// edv_hostcheck.cpp -- TEST HARNESS ONLY.  Builds the kernel's own math and
// per-signature algorithm (edv_math.h, edv_verify_core.h) as plain C++ so the
// CPU test suite can check them against the oracle and Python big integers
// without a GPU.  Nothing in the product path (libedv.so, the Python shim)
// loads this library; it is not a fallback.  fe_sq_floor is built as the prep
// kernel builds it, with its columns chained (edv_math.h).
#define EDV_CHAIN_FLOOR 1
#include <stdint.h>
#include <string.h>
#include <vector>
#include "edv_verify_core.h"
#include "edv_sha256.h"
#include "edv_merkle.h"
#include "edv_ledger.h"
#include "edv_tables.h"
#include "edv_hostplan.h"
#include "edv_selftest_cases.h"
#include "edv_probe_ops.h"

using namespace edv;

namespace {
struct HostATab {
  ge_cached t[kAEntries];
  int staged = 0;
  void store(int e, const ge_cached& c) { t[e] = c; }
  ge_cached load(int e) const { return t[e]; }
  void stage(int e) { staged = e; }
  ge_cached fetch() const { return t[staged]; }
};
// The R side's view of an [S]B table set (large or compact): each entry
// computed when asked for, by the device table's own btab_entry (the sets'
// millions of entries would take minutes to build on one core; a verify needs
// 12 or 16 of them).
struct HostBTab {
  SbShape sh;
  ge_p3 base[kBTablesCompact];
  explicit HostBTab(SbShape s) : sh(s) {
    for (int t = 0; t < sh.tables; t++) base[t] = base_point(t * sh.bits);
  }
  ge_precomp entry(int t, int j) const {
    int32_t w[kBStride];
    btab_entry(w, j, base[t]);
    return precomp_from_words(w);
  }
};
struct HostBStage {
  const HostBTab& b;
  int t = 0, j = 0;
  ge_cached stash;
  SbShape shape() const { return b.sh; }
  void stage(int tt, int jj) { t = tt; j = jj; }
  ge_precomp fetch() const { return b.entry(t, j); }
  void put(const ge_cached& c) { stash = c; }
  ge_cached get() const { return stash; }
};
struct HostComb {
  std::vector<int32_t> w;
  HostComb() : w(kCombRows * kCombEntries * kBStride) {
    for (int i = 0; i < kCombRows; i++)
      for (int j = 0; j < kCombEntries; j++) comb_entry(w.data() + (i * kCombEntries + j) * kBStride, i, j);
  }
  ge_precomp entry(int i, int j) const { return precomp_from_words(w.data() + (i * kCombEntries + j) * kBStride); }
};
const HostComb& comb() {
  static HostComb c;
  return c;
}
static_assert(kBTablesCompact >= kBTables, "base[] holds the larger table count");
const HostBTab& btab(int bits = kBBits) {
  static HostBTab large(sb_large()), compact(sb_compact());
  return bits == kBBitsCompact ? compact : large;
}
void load_words(uint32_t* w, const uint8_t* b, int n) {
  for (int i = 0; i < n; i++) w[i] = uint32_t(b[4 * i]) | uint32_t(b[4 * i + 1]) << 8 | uint32_t(b[4 * i + 2]) << 16 | uint32_t(b[4 * i + 3]) << 24;
}
void store_words(uint8_t* b, const uint32_t* w, int n) {
  for (int i = 0; i < n; i++)
    for (int j = 0; j < 4; j++) b[4 * i + j] = uint8_t(w[i] >> (8 * j));
}
fe to_fe(const int32_t* l) { fe f; for (int i = 0; i < 10; i++) f.v[i] = l[i]; return f; }
void from_fe(int32_t* l, const fe& f) { for (int i = 0; i < 10; i++) l[i] = f.v[i]; }
}  // namespace

extern "C" {
void hc_fe_mul(const int32_t* f, const int32_t* g, int32_t* h) { from_fe(h, fe_mul(to_fe(f), to_fe(g))); }
void hc_fe_sq(const int32_t* f, int32_t* h) { from_fe(h, fe_sq(to_fe(f))); }
void hc_fe_sq_floor(const int32_t* f, int32_t* h) { from_fe(h, fe_sq_floor(to_fe(f))); }
void hc_fe_sq2(const int32_t* f, int32_t* h) { from_fe(h, fe_sq2(to_fe(f))); }
void hc_fe_sqn(const int32_t* f, int n, int32_t* h) { from_fe(h, fe_sqn(to_fe(f), n)); }
void hc_fe_carry32(const int32_t* f, int32_t* h) { from_fe(h, fe_carry32(to_fe(f))); }
void hc_fe_invert(const int32_t* f, int32_t* h) { from_fe(h, fe_invert(to_fe(f))); }
void hc_fe_invert_safegcd(const int32_t* f, int32_t* h) { from_fe(h, fe_invert_safegcd(to_fe(f))); }
void hc_fe_pow22523(const int32_t* f, int32_t* h) { from_fe(h, fe_pow22523(to_fe(f))); }
void hc_fe_tobytes(const int32_t* f, uint8_t* out) { uint32_t w[8]; fe_tobytes(w, to_fe(f)); store_words(out, w, 8); }
void hc_fe_frombytes(const uint8_t* in, int32_t* h) { uint32_t w[8]; load_words(w, in, 8); from_fe(h, fe_frombytes(w)); }
void hc_sc_reduce(const uint8_t* in64, uint8_t* out32) {
  uint32_t w[16], o[8];
  load_words(w, in64, 16);
  sc_reduce(o, w);
  store_words(out32, o, 8);
}
void hc_hram(const uint8_t* R, const uint8_t* A, const uint8_t* m, uint64_t mlen, uint8_t* out64) {
  uint32_t r[8], a[8], o[16];
  load_words(r, R, 8);
  load_words(a, A, 8);
  // msg_word reads whole aligned words up to 12 bytes past the end: pad a copy
  std::vector<uint8_t> buf(mlen + 32, 0);
  if (mlen) memcpy(buf.data() + 16, m, mlen);
  hram(o, r, a, buf.data() + 16, mlen);
  store_words(out64, o, 16);
}
int hc_decompress_negate(const uint8_t* in, uint8_t* out) {
  uint32_t w[8], o[8];
  load_words(w, in, 8);
  ge_p3 p;
  const bool ok = ge_frombytes_negate(p, w);
  ge_p2_tobytes(o, ge_p3_to_p2(p));
  store_words(out, o, 8);
  return ok ? 0 : -1;
}
// SHA-256 of m at a chosen misalignment of the copy (the kernel reads aligned words)
void hc_sha256(const uint8_t* m, uint64_t mlen, int misalign, uint8_t* out32) {
  std::vector<uint8_t> buf(mlen + 48, 0xA5);
  if (mlen) memcpy(buf.data() + 16 + misalign, m, mlen);
  uint32_t o[8];
  sha256_msg(o, buf.data() + 16 + misalign, mlen);
  store_words(out32, o, 8);
}
// edv_sha256_batch's signature, the kernel's SHA-256 on the CPU (tests hand its
// address to _edvhost.request_digests)
int hc_sha256_batch(const uint8_t* msgs, const uint64_t* off, uint64_t n, uint8_t* out, uint32_t) {
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t mlen = off[i + 1] - off[i];
    std::vector<uint8_t> buf(mlen + 48, 0);
    if (mlen) memcpy(buf.data() + 16, msgs + off[i], mlen);
    uint32_t o[8];
    sha256_msg(o, buf.data() + 16, mlen);
    store_words(out + 32 * i, o, 8);
  }
  return 0;
}
// entries js[0..nj) of table t (j x 2^(bits t) B) of the set with `bits`
// (22 large, 16 compact), kBStride words each
int hc_btab_entries_of_bits(int bits, int t, const int32_t* js, int nj, int32_t* out) {
  if (bits != kBBits && bits != kBBitsCompact) return -1;
  const HostBTab& b = btab(bits);
  if (t < 0 || t >= b.sh.tables) return -1;
  for (int k = 0; k < nj; k++) {
    if (js[k] < 0 || js[k] >= b.sh.entries) return -1;
    btab_entry(out + size_t(k) * kBStride, js[k], b.base[t]);
  }
  return 0;
}
int hc_btab_entries_of(int t, const int32_t* js, int nj, int32_t* out) {
  return hc_btab_entries_of_bits(kBBits, t, js, nj, out);
}
// the R side's Q = [S]B - R against the table set with `bits`, encoded (0),
// or -1 if R is rejected
int hc_rside_point_bits(int bits, const uint8_t* R32, const uint8_t* S32, uint8_t* out32) {
  struct Keep {  // keeps entry 1 of the table: Q itself
    ge_cached q;
    void store(int e, const ge_cached& c) { if (e == 1) q = c; }
  } tab;
  uint32_t R[8], S[8], o[8];
  load_words(R, R32, 8);
  load_words(S, S32, 8);
  if (bits != kBBits && bits != kBBitsCompact) return -1;
  HostBStage bs{btab(bits)};
  if (!prep_rpoint(R, S, tab, bs)) return -1;
  // cached (Y+X, Y-X, Z, 2dT) -> (X : Y : Z)
  const fe two_y = fe_carry32(fe_add(tab.q.YpX, tab.q.YmX)), two_x = fe_carry32(fe_sub(tab.q.YpX, tab.q.YmX));
  ge_p2 p{two_x, two_y, fe_carry32(fe_add(tab.q.Z, tab.q.Z))};
  ge_p2_tobytes(o, p);
  store_words(out32, o, 8);
  return 0;
}
int hc_rside_point(const uint8_t* R32, const uint8_t* S32, uint8_t* out32) {
  return hc_rside_point_bits(kBBits, R32, S32, out32);
}
// the lattice reduction of the prep kernel: (a, u, neg) for h (32-byte scalars)
int hc_half_scalars(const uint8_t* h32, uint8_t* a32, uint8_t* u32) {
  uint32_t h[8], a[8], u[8];
  load_words(h, h32, 8);
  bool neg = false;
  half_scalars(h, a, u, neg);
  store_words(a32, a, 8);
  store_words(u32, u, 8);
  return neg ? 1 : 0;
}
// The one-lane math probes of include/edv_measure.h on the CPU build of the
// headers: edv_probe_math's ops and packed layout (edv_probe_ops.h), so the
// tests run one set of cases through both builds.  -1: not a one-lane op, or
// strides below the op's sizes.
int hc_probe_math(int op, const void* in, uint64_t in_stride, void* out, uint64_t out_stride, uint64_t n) {
  const ProbeSize sz = probe_size(op);
  if (!sz.in || probe_is_quad(op) || in_stride < sz.in || out_stride < sz.out || (in_stride & 3) || (out_stride & 3))
    return -1;
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t* x = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(in) + i * in_stride);
    uint32_t* y = reinterpret_cast<uint32_t*>(static_cast<uint8_t*>(out) + i * out_stride);
    switch (op) {
#define HC_PROBE_CASE(OP) case OP: probe_lane_op<OP>(x, y); break;
      HC_PROBE_CASE(EDV_PROBE_FE_MUL)
      HC_PROBE_CASE(EDV_PROBE_FE_SQ)
      HC_PROBE_CASE(EDV_PROBE_FE_SQ2)
      HC_PROBE_CASE(EDV_PROBE_FE_SQ_FLOOR)
      HC_PROBE_CASE(EDV_PROBE_FE_TOBYTES)
      HC_PROBE_CASE(EDV_PROBE_FE_FROMBYTES)
      HC_PROBE_CASE(EDV_PROBE_FE_INVERT_SAFEGCD)
      HC_PROBE_CASE(EDV_PROBE_FE_POW22523)
      HC_PROBE_CASE(EDV_PROBE_SC_REDUCE)
      HC_PROBE_CASE(EDV_PROBE_HALF_SCALARS)
      HC_PROBE_CASE(EDV_PROBE_RECODE5)
      HC_PROBE_CASE(EDV_PROBE_APPROX_DIV)
      HC_PROBE_CASE(EDV_PROBE_FDIV_FLOOR)
      HC_PROBE_CASE(EDV_PROBE_EUCLID_DIV)
      HC_PROBE_CASE(EDV_PROBE_GE_FROMBYTES)
      HC_PROBE_CASE(EDV_PROBE_SC_MULADD)
      HC_PROBE_CASE(EDV_PROBE_RECODE8)
      HC_PROBE_CASE(EDV_PROBE_GE_P3_TOBYTES)
#undef HC_PROBE_CASE
      case EDV_PROBE_SCALARMULT_BASE: probe_scalarmult_base(x, y, comb()); break;
      default: return -1;
    }
  }
  return 0;
}
// The stage probes of include/edv_measure.h on the CPU build of the headers,
// same state layout (dig[w cap + j], alive[k cap + j], atab / rtab 360 words
// per slot, accept by request): the caller pre-fills every array with the
// sentinel, these write what the kernels write.
//
// hc_stage_prep: prep_one, prep_point and prep_rpoint per slot, as
// edv_prep_kernel's sides side0 .. side0 + nsides - 1 (a split run is the same
// stores in another order).  buckets: perm = a stable counting sort by
// sha_bucket (the device's order within a bucket is its atomics'), the
// identity when every request shares one bucket.  bits: 16 or 22.
static_assert(kAEntries * 40 == 360, "a slot's table is 9 entries of 4 x 10 limbs");
int hc_stage_prep(const uint8_t* sigs, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, uint64_t n,
                  int bits, int side0, int nsides, int buckets, uint64_t cap, uint32_t* dig, uint8_t* alive,
                  int32_t* atab, int32_t* rtab, uint32_t* perm, uint8_t* accept) {
  if ((bits != kBBits && bits != kBBitsCompact) || n > cap || side0 < 0 || nsides < 1 || side0 + nsides > 3) return -1;
  const HostBTab& bt = btab(bits);
  if (buckets) {
    auto bucket = [&](uint64_t i) {
      const uint64_t nb = (64 + (off[i + 1] - off[i]) + 17 + 127) / 128;
      return nb < 63 ? nb : uint64_t(63);
    };
    uint64_t k = 0;
    bool one = true;
    for (uint64_t i = 1; i < n; i++) one = one && bucket(i) == bucket(0);
    for (uint64_t b = 0; b < 64 && !one; b++)
      for (uint64_t i = 0; i < n; i++)
        if (bucket(i) == b) perm[k++] = uint32_t(i);
    for (uint64_t i = 0; one && i < n; i++) perm[i] = uint32_t(i);
  }
  for (uint64_t j = 0; j < n; j++) {
    const uint64_t i = buckets ? perm[j] : j;
    uint32_t R[8], S[8], A[8];
    load_words(R, sigs + 64 * i, 8);
    load_words(S, sigs + 64 * i + 32, 8);
    load_words(A, pks + 32 * i, 8);
    for (int side = side0; side < side0 + nsides; side++) {
      bool ok;
      if (side == 0) {
        const uint64_t mlen = off[i + 1] - off[i];
        std::vector<uint8_t> buf(mlen + 32, 0);
        if (mlen) memcpy(buf.data() + 16, msgs + off[i], mlen);
        PrepDigits pd;
        ok = prep_one(R, S, A, buf.data() + 16, mlen, pd);
        if (ok) {
          for (int k = 0; k < 8; k++) {
            dig[uint64_t(k) * cap + j] = pd.da[k];
            dig[uint64_t(8 + k) * cap + j] = pd.db[k];
          }
          dig[16 * cap + j] = uint32_t(pd.nwin) | (pd.negR ? 0x100u : 0u);
        }
      } else {
        HostATab tab;
        if (side == 1) {
          ok = prep_point(A, tab);
        } else {
          HostBStage bs{bt};
          ok = prep_rpoint(R, S, tab, bs);
        }
        int32_t* o = (side == 1 ? atab : rtab) + j * 360;
        for (int e = 0; ok && e < kAEntries; e++) {
          from_fe(o + 40 * e, tab.t[e].YpX);
          from_fe(o + 40 * e + 10, tab.t[e].YmX);
          from_fe(o + 40 * e + 20, tab.t[e].Z);
          from_fe(o + 40 * e + 30, tab.t[e].T2d);
        }
      }
      alive[uint64_t(side) * cap + j] = ok ? 1 : 0;
      if (!ok) accept[i] = 0;
    }
  }
  return 0;
}
// hc_stage_main: main_one on an injected state through a HostATab filled from
// the buffers, as edv_main_kernel's body: a wave is 64 consecutive slots, its
// window count the maximum over its live slots, dead slots untouched, slot
// j's verdict at accept[perm ? perm[j] : j].
int hc_stage_main(uint64_t n, uint64_t cap, const uint32_t* dig, const uint8_t* alive, const int32_t* atab,
                  const int32_t* rtab, const uint32_t* perm, uint8_t* accept) {
  if (n > cap) return -1;
  auto live = [&](uint64_t j) { return j < n && alive[j] && alive[cap + j] && alive[2 * cap + j]; };
  for (uint64_t w0 = 0; w0 < n; w0 += 64) {
    int nwin = 0;
    for (uint64_t j = w0; j < w0 + 64; j++)
      if (live(j)) nwin = mx(nwin, int(dig[16 * cap + j] & 0xff));
    if (nwin > kAWindows) return -1;
    for (uint64_t j = w0; j < w0 + 64; j++) {
      if (!live(j)) continue;
      if (perm && perm[j] >= n) return -1;
      uint32_t da[8], db[8];
      for (int k = 0; k < 8; k++) {
        da[k] = dig[uint64_t(k) * cap + j];
        db[k] = dig[uint64_t(8 + k) * cap + j];
      }
      HostATab at, rt;
      for (int e = 0; e < kAEntries; e++) {
        const int32_t *a = atab + j * 360 + 40 * e, *r = rtab + j * 360 + 40 * e;
        at.t[e] = ge_cached{to_fe(a), to_fe(a + 10), to_fe(a + 20), to_fe(a + 30)};
        rt.t[e] = ge_cached{to_fe(r), to_fe(r + 10), to_fe(r + 20), to_fe(r + 30)};
      }
      accept[perm ? perm[j] : j] = main_one(da, db, nwin, (dig[16 * cap + j] >> 8) & 1, at, rt) ? 1 : 0;
    }
  }
  return 0;
}
// The latency probes of include/edv_measure.h on the CPU.  The latency
// kernels' quad code (edv_quad_body.h) has no CPU build, so these are
// REFERENCES, not the code under test: they prove the cases and the Python
// checkers here before the same families run on the device.  State layout
// [word][slot] with stride slots = n rounded up to ns (16 or 32):
// dig[w slots + j], pt[(k 40 + w) slots + j], ok[k slots + j].
//
// hc_stage_latency_phase1: what phase1<BITS, NS> leaves in LDS, from the
// one-lane header functions (prep_one; ge_is_canonical / has_small_order /
// ge_frombytes_negate; add_sb from the identity), with the kernels' padding
// rule: slots n .. 15 repeat the last request, later ones are not worked.
namespace {
void put_p3(int32_t* pt, int k, uint64_t slots, uint64_t j, const ge_p3& p) {
  const fe* c[4] = {&p.X, &p.Y, &p.Z, &p.T};
  for (int q = 0; q < 4; q++)
    for (int i = 0; i < 10; i++) pt[(uint64_t(k) * 40 + 10 * q + i) * slots + j] = c[q]->v[i];
}
ge_p3 get_p3(const int32_t* pt, int k, uint64_t slots, uint64_t j) {
  fe c[4];
  for (int q = 0; q < 4; q++)
    for (int i = 0; i < 10; i++) c[q].v[i] = pt[(uint64_t(k) * 40 + 10 * q + i) * slots + j];
  return ge_p3{c[0], c[1], c[2], c[3]};
}
ge_p3 p3_add(const ge_p3& p, const ge_p3& q) { return ge_p1p1_to_p3(ge_add(p, ge_p3_to_cached(q))); }
ge_p3 p3_neg(const ge_p3& p) { return ge_p3{fe_neg(p.X), p.Y, p.Z, fe_neg(p.T)}; }
// sum_k d_k 16^k P over the 64 signed 4-bit digits packed in d, most
// significant first: four doublings, then + d_k P
ge_p3 signed_digit_mult(const uint32_t d[8], bool negate, const ge_p3& P) {
  ge_p3 m[9];
  m[0] = ge_p3_identity();
  for (int e = 1; e < 9; e++) m[e] = p3_add(m[e - 1], P);
  ge_p3 acc = ge_p3_identity();
  for (int k = 63; k >= 0; k--) {
    for (int t = 0; t < 4; t++) acc = ge_p1p1_to_p3(ge_p2_dbl(ge_p3_to_p2(acc)));
    int dg = int(d[k / 8] >> (4 * (k % 8))) & 15;
    if (dg >= 8) dg -= 16;
    if (negate) dg = -dg;
    if (dg) acc = p3_add(acc, dg < 0 ? p3_neg(m[-dg]) : m[dg]);
  }
  return acc;
}
}  // namespace
int hc_stage_latency_phase1(const uint8_t* sigs, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off,
                            uint64_t n, int ns, int bits, uint32_t* dig, int32_t* pt, uint8_t* ok) {
  if ((bits != kBBits && bits != kBBitsCompact) || (ns != 16 && ns != 32) || n == 0) return -1;
  const HostBTab& bt = btab(bits);
  const uint64_t slots = (n + ns - 1) / ns * ns;
  for (uint64_t jl = 0; jl < slots; jl++) {
    const bool in = jl < n || jl < 16;
    const uint64_t i = jl < n ? jl : n - 1;
    bool ok0 = false, ok1 = false, ok2 = false;
    PrepDigits pd;
    ge_p3 pa = ge_p3_identity(), pr = ge_p3_identity(), sb = ge_p3_identity();
    if (in) {
      uint32_t R[8], S[8], A[8];
      load_words(R, sigs + 64 * i, 8);
      load_words(S, sigs + 64 * i + 32, 8);
      load_words(A, pks + 32 * i, 8);
      const uint64_t mlen = off[i + 1] - off[i];
      std::vector<uint8_t> buf(mlen + 32, 0);
      if (mlen) memcpy(buf.data() + 16, msgs + off[i], mlen);
      ok0 = prep_one(R, S, A, buf.data() + 16, mlen, pd);
      ok1 = ge_is_canonical(A) && !has_small_order(A) && ge_frombytes_negate(pa, A);
      if (!ok1) pa = ge_p3_identity();
      ok2 = ge_is_canonical(R) && !has_small_order(R) && ge_frombytes_negate(pr, R);
      if (!ok2) pr = ge_p3_identity();
      HostBStage bs{bt};
      add_sb(sb, S, bs);
    }
    for (int k = 0; k < 8; k++) {
      dig[uint64_t(k) * slots + jl] = ok0 ? pd.da[k] : 0u;
      dig[uint64_t(8 + k) * slots + jl] = ok0 ? pd.db[k] : 0u;
    }
    dig[16 * slots + jl] = ok0 ? (uint32_t(pd.nwin) | (pd.negR ? 0x100u : 0u)) : 0u;
    ok[jl] = ok0;
    ok[slots + jl] = ok1;
    ok[2 * slots + jl] = ok2;
    put_p3(pt, 0, slots, jl, pa);
    put_p3(pt, 1, slots, jl, pr);
    put_p3(pt, 2, slots, jl, sb);
  }
  return 0;
}
// hc_stage_latency_walk: the verdict of every slot below n from the injected
// state, [a]P1 + [+-b]([S]B + (-R)) == identity by plain signed-digit
// double-and-add with ge_* of edv_math.h over all 64 digits (a slot's digits
// past its window count are zero in the domain the probe accepts), with the
// kernels' alive / in / padding rules: a slot some side killed gets 0, slots
// n .. write nothing.
int hc_stage_latency_walk(uint64_t n, int ns, const uint32_t* dig, const int32_t* pt, const uint8_t* ok,
                          uint8_t* accept) {
  if ((ns != 16 && ns != 32) || n == 0) return -1;
  const uint64_t slots = (n + ns - 1) / ns * ns;
  for (uint64_t j = 0; j < n; j++) {
    const bool alive = ok[j] && ok[slots + j] && ok[2 * slots + j];
    if (!alive) {
      accept[j] = 0;
      continue;
    }
    const uint32_t wf = dig[16 * slots + j];
    if ((wf & 0xff) > uint32_t(kAWindows)) return -1;
    uint32_t da[8], db[8];
    for (int k = 0; k < 8; k++) {
      da[k] = dig[uint64_t(k) * slots + j];
      db[k] = dig[uint64_t(8 + k) * slots + j];
    }
    const ge_p3 q = p3_add(get_p3(pt, 2, slots, j), get_p3(pt, 1, slots, j));
    const ge_p3 r = p3_add(signed_digit_mult(da, false, get_p3(pt, 0, slots, j)),
                           signed_digit_mult(db, (wf >> 8) & 1, q));
    accept[j] = (fe_iszero(r.X) && fe_iszero(fe_sub(r.Y, r.Z))) ? 1 : 0;
  }
  return 0;
}
// entries (i, j) = ij[2 k], ij[2 k + 1] of the signer's comb (j x 256^i B), kBStride words each
int hc_comb_entries(const int32_t* ij, int n, int32_t* out) {
  const HostComb& ct = comb();
  for (int k = 0; k < n; k++) {
    if (ij[2 * k] < 0 || ij[2 * k] >= kCombRows || ij[2 * k + 1] < 0 || ij[2 * k + 1] >= kCombEntries) return -1;
    memcpy(out + size_t(k) * kBStride, ct.w.data() + (ij[2 * k] * kCombEntries + ij[2 * k + 1]) * kBStride,
           kBStride * sizeof(int32_t));
  }
  return 0;
}
// single-case forms of the ops the harness had no entry point for
double hc_approx_div(double a, double b) { return approx_div(a, b); }
double hc_fdiv_floor(double a, double b) { return fdiv_floor(a, b); }
// r0, t0 <- one Euclidean step against r1, t1 (8 words each, in place)
void hc_euclid_div(uint32_t* r0, uint32_t* t0, const uint32_t* r1, const uint32_t* t1) { euclid_div(r0, t0, r1, t1); }
// recode5 digits of a 32-byte scalar < 2^253; returns digits5_windows of them
int hc_recode5_windows(const uint8_t* in32, uint32_t* out8) {
  uint32_t w[8];
  load_words(w, in32, 8);
  recode5(out8, w);
  return digits5_windows(out8);
}
// ge_frombytes_negate's point as limbs (X Y Z T); returns ge_is_canonical |
// has_small_order << 1 | ge_frombytes_negate << 2
int hc_ge_frombytes_negate_limbs(const uint8_t* in32, int32_t* out40) {
  uint32_t w[8];
  load_words(w, in32, 8);
  ge_p3 p;
  const bool ok = ge_frombytes_negate(p, w);
  from_fe(out40, p.X);
  from_fe(out40 + 10, p.Y);
  from_fe(out40 + 20, p.Z);
  from_fe(out40 + 30, p.T);
  return int(ge_is_canonical(w)) | int(has_small_order(w)) << 1 | int(ok) << 2;
}
// plain (one-lane) group arithmetic on limb vectors, the CPU check of the quad
// formulas' references: p3 = X Y Z T (40 limbs)
void hc_ge_add_p3(const int32_t* p40, const int32_t* q40, int32_t* out40) {
  const ge_p3 p{to_fe(p40), to_fe(p40 + 10), to_fe(p40 + 20), to_fe(p40 + 30)};
  const ge_p3 q{to_fe(q40), to_fe(q40 + 10), to_fe(q40 + 20), to_fe(q40 + 30)};
  const ge_p3 r = ge_p1p1_to_p3(ge_add(p, ge_p3_to_cached(q)));
  from_fe(out40, r.X); from_fe(out40 + 10, r.Y); from_fe(out40 + 20, r.Z); from_fe(out40 + 30, r.T);
}
void hc_ge_dbl_p3(const int32_t* p40, int32_t* out40) {
  const ge_p3 p{to_fe(p40), to_fe(p40 + 10), to_fe(p40 + 20), to_fe(p40 + 30)};
  const ge_p3 r = ge_p1p1_to_p3(ge_p2_dbl(ge_p3_to_p2(p)));
  from_fe(out40, r.X); from_fe(out40 + 10, r.Y); from_fe(out40 + 20, r.Z); from_fe(out40 + 30, r.T);
}
// the walk's layout constants: kAWin, kAEntries, kBBits, kBTables
void hc_layout(int32_t* out4) {
  const int32_t v[4] = {kAWin, kAEntries, kBBits, kBTables};
  memcpy(out4, v, sizeof v);
}
int hc_btab_entries() { return kBEntries; }
// the asynchronous path's ticket ledger (edv_ledger.h): issue n tickets, fail
// the listed ones, then report settled() for each query
void hc_ledger(int64_t n, const int64_t* failed, int nf, const int64_t* queries, int nq, int* out) {
  AsyncLedger l;
  for (int64_t i = 0; i < n; i++) l.issue();
  for (int k = 0; k < nf; k++) l.fail(failed[k]);
  for (int k = 0; k < nq; k++) out[k] = l.settled(queries[k]);
}
// the table-set decision the runtime makes per batch (edv_tables.h): out = use, build, failed
void hc_choose_tables(int policy, uint64_t n, int have_compact, int have_large, int failed, int* out3) {
  const TableChoice c = choose_tables(policy, n, have_compact != 0, have_large != 0, failed != 0);
  out3[0] = c.use;
  out3[1] = c.build;
  out3[2] = c.failed ? 1 : 0;
}
// the host paths' arithmetic (edv_hostplan.h), as the runtime computes it
// out: pks, off, msgs, bytes, padded
void hc_packed_layout(uint64_t n, uint64_t mbytes, uint64_t* out5) {
  const PackedLayout l = packed_layout(n, mbytes);
  const uint64_t v[5] = {l.pks, l.off, l.msgs, l.bytes, l.padded};
  memcpy(out5, v, sizeof v);
}
// out: gp, go, span; returns one
int hc_one_span(uint64_t as, uint64_t ap, uint64_t ao, uint64_t n, uint64_t* out3) {
  const OneSpan s = one_span(as, ap, ao, n);
  out3[0] = s.gp;
  out3[1] = s.go;
  out3[2] = s.span;
  return s.one ? 1 : 0;
}
uint64_t hc_chunk_capacity(uint64_t need, uint64_t limit) { return chunk_capacity(need, limit); }
uint64_t hc_pinned_capacity(uint64_t bytes) { return pinned_capacity(bytes); }
// rb: kSlices + 1 = 9 bounds; returns K
int hc_field_slices(uint64_t n, int host_slices, int bucketed, uint64_t block, uint64_t* rb) {
  return field_slices(n, host_slices, bucketed != 0, block, rb);
}
// out: Q, pmax, P, nsub
void hc_sub_split(uint64_t n, uint64_t chunk, uint64_t block, uint64_t* out4) {
  const SubSplit s = sub_split(n, chunk, block);
  const uint64_t v[4] = {uint64_t(s.Q), s.pmax, s.P, s.nsub};
  memcpy(out4, v, sizeof v);
}
// out: slots, sigs, pks, acc, dig, msgs, off, slot_off, packed, blob, stage, acc_host, dig_host
void hc_trim_limits(uint64_t keep, uint64_t chunk, uint64_t* out13) {
  const TrimLimits t = trim_limits(keep, chunk);
  const uint64_t v[13] = {t.slots, t.sigs, t.pks,  t.acc,   t.dig,      t.msgs,    t.off,
                          t.slot_off, t.packed, t.blob, t.stage, t.acc_host, t.dig_host};
  memcpy(out13, v, sizeof v);
}
// the Merkle buffers' sizes, out: one row of kMerkleBufs = 15 in MerkleBuf's order (no Merkle limit depends on the chunk)
static void put_sizes(uint64_t* out15, const MerkleSizes& s) { memcpy(out15, s.data(), 8 * kMerkleBufsV7); }
// ... and whole rows of kMerkleBufs = 20, the prove forms' staging (mp_*, row f-8) after the 15
void hc_merkle_prove_needs(uint64_t n, uint64_t prefix, uint64_t entries, int want_first, int want_second, uint64_t* out20) {
  const MerkleSizes s = merkle_prove_needs(n, prefix, entries, want_first, want_second);
  memcpy(out20, s.data(), sizeof s);
}
void hc_merkle_trim_limits_all(uint64_t keep, uint64_t* out20) {
  const MerkleSizes s = merkle_trim_limits(keep, trim_limits(keep, uint64_t(1) << 18));
  memcpy(out20, s.data(), sizeof s);
}
uint64_t hc_merkle_prove_prefix(int consistency, const uint64_t* a, const uint64_t* b, uint64_t n, uint64_t store_leaves) {
  return merkle_prove_prefix(consistency, a, b, n, store_leaves);
}
void hc_merkle_prove_offsets(int consistency, const uint64_t* a, const uint64_t* b, uint64_t n, uint64_t store_leaves,
                             uint64_t* proof_off) {
  merkle_prove_offsets(consistency, a, b, n, store_leaves, proof_off);
}
// out: first, second, status, bytes
void hc_merkle_prove_out(uint64_t n, int want_first, int want_second, uint64_t* out4) {
  const MerkleProveOut o = merkle_prove_out(n, want_first, want_second);
  const uint64_t v[4] = {o.first, o.second, o.status, o.bytes};
  memcpy(out4, v, sizeof v);
}
void hc_merkle_extend_needs(uint64_t old_size, uint64_t n, uint64_t mbytes, int host_form, int want_leaf, int want_node,
                            int want_roots, int want_paths, uint64_t* out15) {
  put_sizes(out15, merkle_extend_needs(old_size, n, mbytes, host_form, want_leaf, want_node, want_roots, want_paths));
}
void hc_merkle_verify_needs(int inclusion, uint64_t n, uint64_t lbytes, uint64_t entries, int want_computed, uint64_t* out15) {
  put_sizes(out15, merkle_verify_needs(inclusion, n, lbytes, entries, want_computed));
}
void hc_merkle_trim_limits(uint64_t keep, uint64_t* out15) {
  put_sizes(out15, merkle_trim_limits(keep, trim_limits(keep, uint64_t(1) << 18)));
}
// the known answers of edv_self_test (edv_selftest_cases.h), as the library holds them
int hc_selftest_count() { return kSelfTestCases; }
int hc_selftest_case(int i, uint8_t* sig64, uint8_t* pk32, uint8_t* msg, uint64_t* mlen, int* accept, int* rule) {
  if (i < 0 || i >= kSelfTestCases) return -1;
  const SelfTestCase& t = selftest_cases()[i];
  memcpy(sig64, t.sig, 64);
  memcpy(pk32, t.pk, 32);
  memcpy(msg, t.msg, sizeof t.msg);
  *mlen = t.mlen;
  *accept = t.accept;
  *rule = t.rule;
  return int(sizeof t.msg);
}
// windows the packed radix-2^kAWin digits need (the prep kernel's per-lane count)
int hc_digits_windows(const uint32_t* d8) { return digits5_windows(d8); }
// packed signed digits of a 32-byte scalar at radix 2^bits: 4 (64 digits: the main
// loop's windows at kAWin = 4), 5 (51 digits), 8 -> recode8 (signer)
int hc_recode(const uint8_t* in32, int bits, uint32_t* out8) {
  uint32_t w[8];
  load_words(w, in32, 8);
  if (bits == 4) recode4(out8, w);
  else if (bits == 5) recode5_fixed(out8, w);
  else if (bits == 8) recode8(out8, w);
  else return -1;
  return 0;
}
int hc_sign_batch(const uint8_t* seeds, const uint8_t* msgs, const uint64_t* off, uint64_t n, uint8_t* pks,
                  uint8_t* sigs) {
  const HostComb& ct = comb();
  for (uint64_t i = 0; i < n; i++) {
    uint32_t seed[8], pk[8], sig[16];
    load_words(seed, seeds + 32 * i, 8);
    const uint64_t mlen = off[i + 1] - off[i];
    std::vector<uint8_t> buf(mlen + 32, 0);
    if (mlen) memcpy(buf.data() + 16, msgs + off[i], mlen);
    sign_one(pk, sig, seed, buf.data() + 16, mlen, ct);
    store_words(pks + 32 * i, pk, 8);
    store_words(sigs + 64 * i, sig, 16);
  }
  return 0;
}
int hc_verify_batch(const uint8_t* sigs, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, uint64_t n,
                    uint8_t* accept) {
  const HostBTab& bt = btab();
  for (uint64_t i = 0; i < n; i++) {
    uint32_t R[8], S[8], A[8];
    load_words(R, sigs + 64 * i, 8);
    load_words(S, sigs + 64 * i + 32, 8);
    load_words(A, pks + 32 * i, 8);
    const uint64_t mlen = off[i + 1] - off[i];
    std::vector<uint8_t> buf(mlen + 32, 0);
    if (mlen) memcpy(buf.data() + 16, msgs + off[i], mlen);
    HostATab at, rt;
    HostBStage bs{bt};
    accept[i] = verify_one(R, S, A, buf.data() + 16, mlen, at, rt, bs) ? 1 : 0;
  }
  return 0;
}

// ---- the Merkle-tree extension (edv_merkle.h, row f-5)
// out: kMerkleLogT, kMerkleT, kMerkleMaxHashes
void hc_merkle_consts(int32_t* out) { out[0] = kMerkleLogT; out[1] = kMerkleT; out[2] = kMerkleMaxHashes; }
uint64_t hc_merkle_store_pos(int h, uint64_t k) { return merkle_store_pos(h, k); }
uint64_t hc_merkle_node_count(uint64_t s) { return merkle_node_count(s); }
// the prefixed loader on a leaf that starts `misalign` bytes into a word, the
// word before the leaf's first one not addressable through the buffer
void hc_merkle_leaf_hash(const uint8_t* m, uint64_t mlen, int misalign, uint8_t* out32) {
  std::vector<uint32_t> buf((mlen + 3 + 8) / 4 + 1, 0xA5A5A5A5u);
  uint8_t* p = reinterpret_cast<uint8_t*>(buf.data()) + (misalign & 3);
  if (mlen) memcpy(p, m, mlen);
  uint32_t H[8], o[8];
  merkle_leaf_hash(H, p, mlen);
  merkle_store_hash(o, H);
  store_words(out32, o, 8);
}
// edv_merkle_extend's signature minus `device`: the kernels' passes and tiles,
// lanes and levels run one after another (what __syncthreads() separates on
// the device is a finished loop here).  leaf_in (row f-9): the n leaf hashes
// instead of leaves / off, in a block of exactly 32 n bytes.
static int hc_extend(uint64_t old_size, const uint8_t* old_hashes, const uint8_t* leaves, const uint64_t* off,
                     const uint8_t* leaf_in, uint64_t n, uint8_t* leaf_hashes, uint8_t* node_hashes, uint8_t* new_hashes,
                     uint8_t* root) {
  if (old_size > kMerkleMaxSize || n > kMerkleMaxSize || old_size + n > kMerkleMaxSize) return -1;
  if ((old_size && !old_hashes) || !new_hashes || !root || (n && !off && !leaf_in)) return -1;
  for (uint64_t i = 0; i < n && !leaf_in; i++)
    if (off[i + 1] < off[i]) return -1;
  const uint64_t new_size = old_size + n;
  const uint64_t nodes = merkle_node_count(new_size) - merkle_node_count(old_size);
  const uint64_t mbase = n && !leaf_in ? off[0] : 0, mbytes = n && !leaf_in ? off[n] - off[0] : 0;
  std::vector<uint32_t> inw(leaf_in ? 8 * n : 0);
  if (leaf_in && n) memcpy(inw.data(), leaf_in, 32 * n);
  // the leaves keep their alignment relative to their offsets; 8 readable bytes past the end
  std::vector<uint32_t> lbuf((mbytes + 3 + 8) / 4 + 2, 0);
  uint8_t* lv = reinterpret_cast<uint8_t*>(lbuf.data()) + (mbase & 3);
  if (mbytes) memcpy(lv, leaves + mbase, mbytes);
  std::vector<uint32_t> oldw(8 * size_t(popc64(old_size)) + 8), neww(8 * size_t(popc64(new_size)) + 8), rootw(8);
  if (old_size) memcpy(oldw.data(), old_hashes, 32 * size_t(popc64(old_size)));
  std::vector<uint32_t> leafw(leaf_hashes ? 8 * n : 0), nodew(node_hashes ? 8 * nodes : 0);
  std::vector<uint32_t> roots(8 * merkle_scratch_hashes(old_size, new_size) + 8);
  MerklePass args = merkle_pass_args(old_size, new_size, oldw.data(), leaf_hashes ? leafw.data() : nullptr,
                                     node_hashes ? nodew.data() : nullptr, neww.data());
  std::vector<uint32_t> lvl0(8 * kMerkleT), lvl1(8 * kMerkleT);
  uint32_t* lvl[2] = {lvl0.data(), lvl1.data()};
  merkle_for_each_pass(old_size, new_size, roots.data(), args, [&](const MerklePass& a) {  // the runtime's schedule
    const int h0 = a.h0;
    const uint64_t tile0 = merkle_pass_first_tile(old_size, h0), tiles = merkle_pass_tiles(old_size, new_size, h0);
    for (uint64_t tile = tile0; tile < tile0 + tiles; tile++) {
      for (uint32_t w = 0; w < 8 * kMerkleT; w++) lvl0[w] = lvl1[w] = 0xDEADBEEFu;  // nothing stale may be read
      for (uint32_t j = 0; j < uint32_t(kMerkleT); j++) {
        uint64_t g;
        if (!merkle_item_index(a, tile, j, &g)) continue;
        uint32_t H[8];
        if (h0 == 0 && !a.in) {
          const uint64_t i = g - old_size;
          merkle_leaf_hash(H, lv + (off[i] - mbase), off[i + 1] - off[i]);
        } else {
          merkle_load_hash(H, a.in + 8 * (g - (old_size >> h0)));
        }
        merkle_item_put(a, g, j, H, lvl[0]);
      }
      for (int hl = 1; hl <= kMerkleLogT; hl++)
        for (uint32_t j = 0; j < (uint32_t(kMerkleT) >> hl); j++)
          merkle_level(a, tile, hl, j, lvl[(hl - 1) & 1], lvl[hl & 1]);
    }
    return 0;
  }, leaf_in && n ? inw.data() : nullptr);
  merkle_finish(old_size, new_size, args.old_hashes, args.new_hashes, rootw.data());
  if (leaf_hashes && n) memcpy(leaf_hashes, leafw.data(), 32 * n);
  if (node_hashes && nodes) memcpy(node_hashes, nodew.data(), 32 * nodes);
  memcpy(new_hashes, neww.data(), 32 * size_t(popc64(new_size)));
  memcpy(root, rootw.data(), 32);
  return 0;
}
int hc_merkle_extend(uint64_t old_size, const uint8_t* old_hashes, const uint8_t* leaves, const uint64_t* off,
                     uint64_t n, uint8_t* leaf_hashes, uint8_t* node_hashes, uint8_t* new_hashes, uint8_t* root) {
  return hc_extend(old_size, old_hashes, leaves, off, nullptr, n, leaf_hashes, node_hashes, new_hashes, root);
}
// edv_merkle_extend_hashed's signature minus `device`
int hc_merkle_extend_hashed(uint64_t old_size, const uint8_t* old_hashes, const uint8_t* leaf_hashes, uint64_t n,
                            uint8_t* node_hashes, uint8_t* new_hashes, uint8_t* root) {
  if (n && !leaf_hashes) return -1;
  return hc_extend(old_size, old_hashes, nullptr, nullptr, leaf_hashes, n, nullptr, node_hashes, new_hashes, root);
}
// ---- the batched append (edv_merkle.h, row f-6)
uint64_t hc_merkle_path_entries(uint64_t old_size, uint64_t n) { return merkle_path_entries(old_size, n); }
// edv_merkle_append_batch's signature minus `device`: hc_merkle_extend, then
// the append kernel's lanes one after another over the hashes it wrote.
int hc_merkle_append_batch(uint64_t old_size, const uint8_t* old_hashes, const uint8_t* leaves, const uint64_t* off,
                           uint64_t n, uint8_t* leaf_hashes, uint8_t* node_hashes, uint8_t* new_hashes, uint8_t* root,
                           uint8_t* roots, uint8_t* audit_paths) {
  if (old_size > kMerkleMaxSize || n > kMerkleMaxSize || old_size + n > kMerkleMaxSize) return -1;
  const bool per_leaf = n != 0 && (roots || audit_paths);
  const uint64_t nodes = merkle_node_count(old_size + n) - merkle_node_count(old_size);
  // the fold reads the leaf and node hashes whether the caller wants them or not
  std::vector<uint8_t> lh(per_leaf && !leaf_hashes ? 32 * n : 0), nh(per_leaf && !node_hashes ? 32 * nodes + 1 : 0);
  uint8_t* lhp = leaf_hashes ? leaf_hashes : (per_leaf ? lh.data() : nullptr);
  uint8_t* nhp = node_hashes ? node_hashes : (per_leaf ? nh.data() : nullptr);
  if (const int rc = hc_merkle_extend(old_size, old_hashes, leaves, off, n, lhp, nhp, new_hashes, root)) return rc;
  if (!per_leaf) return 0;
  const uint64_t entries = merkle_path_entries(old_size, n);
  // exact sizes, here and below: a lane reading or storing a hash too far is ASan's to see
  std::vector<uint32_t> oldw(8 * size_t(popc64(old_size))), leafw(8 * n), nodew(8 * nodes);
  std::vector<uint32_t> rootsw(roots ? 8 * n : 0), pathsw(audit_paths ? 8 * entries : 0);
  if (old_size) memcpy(oldw.data(), old_hashes, 32 * size_t(popc64(old_size)));
  memcpy(leafw.data(), lhp, 32 * n);
  if (nodes) memcpy(nodew.data(), nhp, 32 * nodes);
  const MerkleAppend a = merkle_append_args(old_size, n, oldw.data(), leafw.data(), nodew.data(),
                                            roots ? rootsw.data() : nullptr, audit_paths ? pathsw.data() : nullptr);
  for (uint64_t i = 0; i < n; i++) merkle_append_leaf(a, i);
  if (roots) memcpy(roots, rootsw.data(), 32 * n);
  if (audit_paths && entries) memcpy(audit_paths, pathsw.data(), 32 * entries);
  return 0;
}
// ---- proof verification (edv_merkle.h, row f-7)
// The host C-ABI forms' signatures minus `device`: the kernels' lanes one after
// another.  Every input goes into a heap block of exactly its documented size
// (the leaves: 8 bytes more, their alignment relative to their offsets kept),
// so a lane reading past a proof's last entry is ASan's to see.
static bool hc_offsets_ok(const uint64_t* off, uint64_t n) {
  for (uint64_t i = 0; i < n; i++)
    if (off[i + 1] < off[i]) return false;
  return true;
}
int hc_merkle_verify_inclusion(const uint8_t* leaves, const uint64_t* leaf_off, const uint8_t* leaf_hashes,
                               const uint64_t* leaf_index, const uint64_t* tree_size, const uint8_t* roots,
                               const uint8_t* proofs, const uint64_t* proof_off, uint64_t n, uint8_t* status,
                               uint8_t* computed) {
  if (n > (uint64_t(1) << 22) || (leaves && leaf_hashes)) return -1;
  if (n == 0) return 0;
  if ((!leaves && !leaf_hashes) || (leaves && !leaf_off) || !leaf_index || !tree_size || !roots || !proofs || !proof_off ||
      !status)
    return -1;
  if ((leaves && !hc_offsets_ok(leaf_off, n)) || !hc_offsets_ok(proof_off, n)) return -1;
  memset(status, kProofUnverified, n);
  const uint64_t lbase = leaves ? leaf_off[0] : 0, lbytes = leaves ? leaf_off[n] - leaf_off[0] : 0;
  const uint64_t pbase = proof_off[0], entries = proof_off[n] - proof_off[0];
  std::vector<uint32_t> lbuf(leaves ? (lbytes + (lbase & 3) + 8 + 3) / 4 : 0), lhw(leaves ? 0 : 8 * n), rootw(8 * n),
      proofw(8 * entries), compw(computed ? 8 * n : 0);
  std::vector<uint64_t> loff(leaves ? n + 1 : 0), idx(leaf_index, leaf_index + n), size(tree_size, tree_size + n),
      poff(proof_off, proof_off + n + 1);
  uint8_t* lv = reinterpret_cast<uint8_t*>(lbuf.data()) + (lbase & 3);
  if (leaves) {
    memcpy(loff.data(), leaf_off, 8 * (n + 1));
    if (lbytes) memcpy(lv, leaves + lbase, lbytes);
  } else {
    memcpy(lhw.data(), leaf_hashes, 32 * n);
  }
  memcpy(rootw.data(), roots, 32 * n);
  if (entries) memcpy(proofw.data(), proofs + 32 * pbase, 32 * entries);
  std::vector<uint8_t> st(n);
  const MerkleVerifyInclusion a = merkle_verify_inclusion_args(
      n, leaves ? lv : nullptr, leaves ? loff.data() : nullptr, lbase, leaves ? nullptr : lhw.data(), idx.data(),
      size.data(), rootw.data(), proofw.data(), poff.data(), pbase, st.data(), computed ? compw.data() : nullptr);
  for (uint64_t i = 0; i < n; i++) {
    if (leaves)
      merkle_verify_inclusion_lane<true>(a, i);
    else
      merkle_verify_inclusion_lane<false>(a, i);
  }
  memcpy(status, st.data(), n);
  if (computed) memcpy(computed, compw.data(), 32 * n);
  return 0;
}
int hc_merkle_verify_consistency(const uint64_t* old_size, const uint64_t* new_size, const uint8_t* old_roots,
                                 const uint8_t* new_roots, const uint8_t* proofs, const uint64_t* proof_off, uint64_t n,
                                 uint8_t* status, uint8_t* computed) {
  if (n > (uint64_t(1) << 22)) return -1;
  if (n == 0) return 0;
  if (!old_size || !new_size || !old_roots || !new_roots || !proofs || !proof_off || !status) return -1;
  if (!hc_offsets_ok(proof_off, n)) return -1;
  memset(status, kProofUnverified, n);
  const uint64_t pbase = proof_off[0], entries = proof_off[n] - proof_off[0];
  std::vector<uint32_t> oldw(8 * n), neww(8 * n), proofw(8 * entries), compw(computed ? 16 * n : 0);
  std::vector<uint64_t> os(old_size, old_size + n), ns(new_size, new_size + n), poff(proof_off, proof_off + n + 1);
  memcpy(oldw.data(), old_roots, 32 * n);
  memcpy(neww.data(), new_roots, 32 * n);
  if (entries) memcpy(proofw.data(), proofs + 32 * pbase, 32 * entries);
  std::vector<uint8_t> st(n);
  const MerkleVerifyConsistency a =
      merkle_verify_consistency_args(n, os.data(), ns.data(), oldw.data(), neww.data(), proofw.data(), poff.data(), pbase,
                                     st.data(), computed ? compw.data() : nullptr);
  for (uint64_t i = 0; i < n; i++) merkle_verify_consistency_lane(a, i);
  memcpy(status, st.data(), n);
  if (computed) memcpy(computed, compw.data(), 64 * n);
  return 0;
}

// ---- proof generation (edv_merkle.h, row f-8)
// out: kProofSpace, kMerkleMaxProof, kMerkleBufs
void hc_merkle_prove_consts(int32_t* out) { out[0] = kProofSpace; out[1] = kMerkleMaxProof; out[2] = kMerkleBufs; }
uint64_t hc_merkle_inclusion_length(uint64_t m, uint64_t n) { return merkle_inclusion_length(m, n); }
uint64_t hc_merkle_consistency_length(uint64_t first, uint64_t second) { return merkle_consistency_length(first, second); }
// kind / off: room for kMerkleMaxProof entries; the pair must be in range (m < n, or 1 <= a <= n), n <= 2^62
int hc_merkle_proof_positions(int consistency, uint64_t a, uint64_t n, uint8_t* kind, uint64_t* off) {
  if (n == 0 || n > kMerkleMaxSize || (consistency ? (a == 0 || a > n) : a >= n)) return -1;
  return merkle_proof_positions(consistency, a, n, kind, off);
}
// The host C-ABI forms' signatures minus `device`: the kernels' lanes one after
// another.  The two stores go into heap blocks of exactly the sizes the counts
// give, the slots [proof_off[0], proof_off[n]) into one of exactly their
// entries (copied in first, so what no lane writes keeps the caller's bytes),
// so a lane reading or writing one hash too far is ASan's to see.
extern "C++" template <class Args, class Lane>
int hc_prove(const uint8_t* leaf_store, const uint8_t* node_store, uint64_t store_leaves, const uint64_t* a,
                    const uint64_t* b, const uint64_t* proof_off, uint64_t n, uint8_t* proofs, uint8_t* status,
                    uint8_t* out1, uint8_t* out2, Args make, Lane lane) {
  if (n > (uint64_t(1) << 22) || store_leaves > kMerkleMaxSize) return -1;
  if (n == 0) return 0;
  if (!a || !b || !proof_off || !proofs || !status || (store_leaves && !leaf_store) || (store_leaves > 1 && !node_store))
    return -1;
  if (!hc_offsets_ok(proof_off, n)) return -1;
  memset(status, kProofUnverified, n);
  const uint64_t nodes = merkle_node_count(store_leaves), pbase = proof_off[0], entries = proof_off[n] - proof_off[0];
  std::vector<uint32_t> leafw(8 * store_leaves), nodew(8 * nodes), proofw(8 * entries), o1(out1 ? 8 * n : 0),
      o2(out2 ? 8 * n : 0);
  std::vector<uint64_t> av(a, a + n), bv(b, b + n), poff(proof_off, proof_off + n + 1);
  if (store_leaves) memcpy(leafw.data(), leaf_store, 32 * store_leaves);
  if (nodes) memcpy(nodew.data(), node_store, 32 * nodes);
  if (entries) memcpy(proofw.data(), proofs + 32 * pbase, 32 * entries);
  std::vector<uint8_t> st(n);
  const auto args = make(leafw.data(), nodew.data(), store_leaves, av.data(), bv.data(), poff.data(), pbase, n,
                         proofw.data(), st.data(), out1 ? o1.data() : nullptr, out2 ? o2.data() : nullptr);
  for (uint64_t i = 0; i < n; i++) lane(args, i);
  if (entries) memcpy(proofs + 32 * pbase, proofw.data(), 32 * entries);
  memcpy(status, st.data(), n);
  if (out1) memcpy(out1, o1.data(), 32 * n);
  if (out2) memcpy(out2, o2.data(), 32 * n);
  return 0;
}
int hc_merkle_prove_inclusion(const uint8_t* leaf_store, const uint8_t* node_store, uint64_t store_leaves,
                              const uint64_t* leaf_index, const uint64_t* tree_size, const uint64_t* proof_off, uint64_t n,
                              uint8_t* proofs, uint8_t* status, uint8_t* roots, uint8_t* leaf_hashes_out) {
  return hc_prove(leaf_store, node_store, store_leaves, leaf_index, tree_size, proof_off, n, proofs, status, roots,
                  leaf_hashes_out, merkle_prove_inclusion_args, merkle_prove_inclusion_lane);
}
int hc_merkle_prove_consistency(const uint8_t* leaf_store, const uint8_t* node_store, uint64_t store_leaves,
                                const uint64_t* first, const uint64_t* second, const uint64_t* proof_off, uint64_t n,
                                uint8_t* proofs, uint8_t* status, uint8_t* old_roots, uint8_t* new_roots) {
  return hc_prove(leaf_store, node_store, store_leaves, first, second, proof_off, n, proofs, status, old_roots, new_roots,
                  merkle_prove_consistency_args, merkle_prove_consistency_lane);
}

// ---- auditing a stored tree (edv_merkle.h, row f-9)
// 0: q is a position no store of at most 2^62 leaves has
int hc_merkle_store_node_at(uint64_t q, uint64_t* s, int32_t* h) {
  if (q >= merkle_node_count(kMerkleMaxSize)) return 0;
  int hh;
  merkle_store_node_at(q, s, &hh);
  *h = hh;
  return 1;
}
// The host C-ABI forms' signatures minus `device`: the kernels' lanes one after
// another.  The stores go into heap blocks of exactly the sizes the counts give
// (leaves: the slice's entries alone, as the host form stages them; the leaf
// bytes 8 more, their alignment relative to their offsets kept), so a lane
// reading one entry past the counts is ASan's to see.
int hc_merkle_audit_nodes(const uint8_t* leaf_store, const uint8_t* node_store, uint64_t store_leaves, uint64_t node_lo,
                          uint64_t count, uint8_t* status, uint64_t* summary) {
  if (count > (uint64_t(1) << 22) || store_leaves > kMerkleMaxSize || !summary) return -1;
  const uint64_t nodes = merkle_node_count(store_leaves);
  if (node_lo > nodes || count > nodes - node_lo) return -1;
  if (count && (!leaf_store || !node_store)) return -1;
  merkle_audit_summary_init(summary);
  if (!count) return 0;
  std::vector<uint32_t> leafw(8 * store_leaves), nodew(8 * nodes);
  memcpy(leafw.data(), leaf_store, 32 * store_leaves);
  memcpy(nodew.data(), node_store, 32 * nodes);
  std::vector<uint8_t> st(count, kAuditUnchecked);
  const MerkleAuditNodes a = merkle_audit_nodes_args(leafw.data(), nodew.data(), node_lo, count, status ? st.data() : nullptr);
  merkle_audit_run(a, count, node_lo, summary, merkle_audit_node_lane);
  if (status) memcpy(status, st.data(), count);
  return 0;
}
int hc_merkle_audit_leaves(const uint8_t* leaf_store, uint64_t store_leaves, uint64_t leaf_lo, const uint8_t* leaves,
                           const uint64_t* leaf_off, uint64_t n, uint8_t* status, uint64_t* summary) {
  if (n > (uint64_t(1) << 22) || store_leaves > kMerkleMaxSize || !summary) return -1;
  if (leaf_lo > store_leaves || n > store_leaves - leaf_lo) return -1;
  if (n && (!leaf_store || !leaf_off || !hc_offsets_ok(leaf_off, n))) return -1;
  if (n && !leaves && leaf_off[n] != leaf_off[0]) return -1;
  merkle_audit_summary_init(summary);
  if (!n) return 0;
  const uint64_t lbase = leaf_off[0], lbytes = leaf_off[n] - leaf_off[0];
  std::vector<uint32_t> lbuf((lbytes + (lbase & 3) + 8 + 3) / 4), leafw(8 * n);
  std::vector<uint64_t> loff(leaf_off, leaf_off + n + 1);
  uint8_t* lv = reinterpret_cast<uint8_t*>(lbuf.data()) + (lbase & 3);
  if (lbytes) memcpy(lv, leaves + lbase, lbytes);
  memcpy(leafw.data(), leaf_store + 32 * leaf_lo, 32 * n);
  std::vector<uint8_t> st(n, kAuditUnchecked);
  const MerkleAuditLeaves a =
      merkle_audit_leaves_args(leafw.data(), leaf_lo, leaf_lo, n, lv, loff.data(), lbase, status ? st.data() : nullptr);
  merkle_audit_run(a, n, leaf_lo, summary, merkle_audit_leaf_lane);
  if (status) memcpy(status, st.data(), n);
  return 0;
}
// the host plan of the host forms, whole rows of kMerkleBufs = 20
void hc_merkle_audit_nodes_needs(uint64_t node_lo, uint64_t count, uint64_t* out20, uint64_t* prefix2) {
  const MerkleSizes s = merkle_audit_nodes_needs(node_lo, count);
  memcpy(out20, s.data(), sizeof s);
  prefix2[0] = prefix2[1] = 0;
  if (count) {
    const MerkleAuditPrefix p = merkle_audit_nodes_prefix(node_lo, count);
    prefix2[0] = p.leaves;
    prefix2[1] = p.nodes;
  }
}
void hc_merkle_audit_leaves_needs(uint64_t n, uint64_t lbytes, uint64_t* out20) {
  const MerkleSizes s = merkle_audit_leaves_needs(n, lbytes);
  memcpy(out20, s.data(), sizeof s);
}
void hc_merkle_extend_hashed_needs(uint64_t old_size, uint64_t n, int host_form, int want_node, uint64_t* out20) {
  const MerkleSizes s = merkle_extend_hashed_needs(old_size, n, host_form, want_node);
  memcpy(out20, s.data(), sizeof s);
}
// out: kAuditUnchecked, kAuditOk, kAuditBad
void hc_merkle_audit_consts(int32_t* out) { out[0] = kAuditUnchecked; out[1] = kAuditOk; out[2] = kAuditBad; }

// ---- catch-up (edv_merkle.h, row f-10)
// edv_merkle_catchup's signature minus `device`, and its EDV_E_ARG cases (-1):
// hc_merkle_extend, then the catch-up kernel's lanes one after another over the
// hashes it wrote.  Ends, offsets, hashes, proofs and outputs are heap blocks of
// exactly their documented sizes: a lane reading an entry past its proof or a
// hash past the call's is ASan's to see.
int hc_merkle_catchup(uint64_t old_size, const uint8_t* old_hashes, const uint8_t* leaves, const uint64_t* off,
                      uint64_t n, const uint64_t* reply_end, uint64_t replies, uint64_t final_size,
                      const uint8_t* final_root, const uint8_t* proofs, const uint64_t* proof_off, uint8_t* leaf_hashes,
                      uint8_t* node_hashes, uint8_t* reply_roots, uint8_t* status) {
  if (n > (uint64_t(1) << 22) || old_size > kMerkleMaxSize || old_size + n > kMerkleMaxSize) return -1;
  if ((old_size && !old_hashes) || !reply_end || !final_root || !proof_off || !status) return -1;
  if ((replies == 0 && n) || replies > n + 1) return -1;
  if (n && (!off || !hc_offsets_ok(off, n) || (!leaves && off[n] != off[0]))) return -1;
  if (replies == 0) return 0;
  if (!hc_offsets_ok(reply_end, replies - 1) || reply_end[replies - 1] != n || !hc_offsets_ok(proof_off, replies)) return -1;
  if (!proofs && proof_off[replies] != proof_off[0]) return -1;
  memset(status, kProofUnverified, replies);
  const uint64_t nodes = merkle_node_count(old_size + n) - merkle_node_count(old_size);
  const size_t nold = size_t(popc64(old_size));
  std::vector<uint8_t> lh(32 * n + 1), nh(32 * nodes + 1), newh(32 * size_t(popc64(old_size + n)) + 1), root(32);
  if (const int rc = hc_merkle_extend(old_size, old_hashes, leaves, off, n, lh.data(), nh.data(), newh.data(), root.data()))
    return rc;
  const uint64_t pbase = proof_off[0], entries = proof_off[replies] - proof_off[0];
  std::vector<uint32_t> oldw(8 * nold), leafw(8 * n), nodew(8 * nodes), targetw(8), proofw(8 * entries);
  std::vector<uint32_t> rootsw(reply_roots ? 8 * replies : 0);
  std::vector<uint64_t> ends(reply_end, reply_end + replies), poff(proof_off, proof_off + replies + 1);
  std::vector<uint8_t> st(replies);
  if (nold) memcpy(oldw.data(), old_hashes, 32 * nold);
  if (n) memcpy(leafw.data(), lh.data(), 32 * n);
  if (nodes) memcpy(nodew.data(), nh.data(), 32 * nodes);
  memcpy(targetw.data(), final_root, 32);
  if (entries) memcpy(proofw.data(), proofs + 32 * pbase, 32 * entries);
  const MerkleCatchup a = merkle_catchup_args(old_size, n, oldw.data(), leafw.data(), nodew.data(), ends.data(), replies,
                                              final_size, targetw.data(), proofw.data(), poff.data(), pbase,
                                              reply_roots ? rootsw.data() : nullptr, st.data());
  for (uint64_t k = 0; k < replies; k++) merkle_catchup_lane(a, k);
  memcpy(status, st.data(), replies);
  if (reply_roots) memcpy(reply_roots, rootsw.data(), 32 * replies);
  if (leaf_hashes && n) memcpy(leaf_hashes, lh.data(), 32 * n);
  if (node_hashes && nodes) memcpy(node_hashes, nh.data(), 32 * nodes);
  return 0;
}
// the host plan of both forms, a whole row of kMerkleBufs = 20
void hc_merkle_catchup_needs(uint64_t old_size, uint64_t n, uint64_t mbytes, uint64_t replies, uint64_t entries,
                             int host_form, int want_leaf, int want_node, int want_roots, uint64_t* out20) {
  const MerkleSizes s = merkle_catchup_needs(old_size, n, mbytes, replies, entries, host_form, want_leaf, want_node, want_roots);
  memcpy(out20, s.data(), sizeof s);
}
}

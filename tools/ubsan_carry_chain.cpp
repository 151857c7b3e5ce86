// ubsan_carry_chain.cpp -- TESTS ONLY (tests/test_carry_chain_cpu.py).  The
// field products of edv_math.h on the CPU over the inputs that push their
// 64-bit columns furthest, for a build with
//   g++ -std=c++17 -fsanitize=signed-integer-overflow,undefined -fno-sanitize-recover=all
// A column is a sum of up to ten products, its start (a rounding bias, or in
// fe_sq_floor the carry of the column before, which rides in as the first
// product's addend) and, in the rounding chain, the carry added at the end;
// the bound arguments in edv_math.h keep every column inside 2^62, and UBSan
// aborts the run if a sum leaves int64 anyway.  Prints "ok <cases> <checksum>"
// over every output limb: the same line with fe_sq_floor's columns chained
// (the default here, as in the prep kernel) and with -DEDV_CHAIN_FLOOR=0.
#ifndef EDV_CHAIN_FLOOR
#define EDV_CHAIN_FLOOR 1
#endif
#include <stdint.h>
#include <stdio.h>
#include "../indy-plenum_amd/csrc/edv_math.h"

using namespace edv;

namespace {
// the multiply's input bound: |f_i| <= 1.65 * 2^26 (even i), 1.65 * 2^25 (odd i)
constexpr int32_t kBound[2] = {110729625, 55364812};
// the largest limbs fe_sq_floor is specified for
constexpr int32_t kFloorTop[2] = {(1 << 26) - 1, (1 << 25) + (1 << 16)};
uint64_t sum = 0, cases = 0;
void eat(const fe& h) {
  for (int i = 0; i < 10; i++) sum = sum * 0x100000001b3ULL ^ uint32_t(h.v[i]);
  cases++;
}
// limb i = +-bound by bit i of `signs`, one inside the bound by bit i of `inside`
fe at_bound(uint32_t signs, uint32_t inside) {
  fe f;
  for (int i = 0; i < 10; i++) {
    const int32_t b = kBound[i & 1] - int32_t((inside >> i) & 1);
    f.v[i] = ((signs >> i) & 1) ? -b : b;
  }
  return f;
}
}  // namespace

int main() {
  // every sign pattern of f at the bound, against g in the patterns that line
  // the column's terms up with one sign: g's signs equal to f's, opposite,
  // f's reversed (term f_i g_(k-i)) and its opposite, all plus, all minus
  for (uint32_t s = 0; s < 1024; s++) {
    const fe f = at_bound(s, s * 7 & 1023);
    uint32_t rev = 0;
    for (int i = 0; i < 10; i++) rev |= ((s >> i) & 1) << (9 - i);
    const uint32_t gs[6] = {s, s ^ 1023, rev, rev ^ 1023, 0, 1023};
    for (uint32_t g : gs) eat(fe_mul(f, at_bound(g, 0)));
    eat(fe_sq(f));
    eat(fe_sq2(f));
    eat(fe_sq(at_bound(s, 0)));
    eat(fe_sq2(at_bound(s, 0)));
  }
  // floor squarings: each limb at its top or at zero, every pattern, and a run
  // from each of them
  for (uint32_t s = 0; s < 1024; s++) {
    fe f;
    for (int i = 0; i < 10; i++) f.v[i] = ((s >> i) & 1) ? kFloorTop[i & 1] : 0;
    eat(fe_sq_floor(f));
    eat(fe_sqn(f, 6));
  }
  // fe_pow22523 (every op above, chained 252 squarings deep) from the uniform sign patterns
  const uint32_t uniform[6] = {0, 1023, 0x155, 0x2aa, 1, 0x200};
  for (uint32_t s : uniform) eat(fe_pow22523(at_bound(s, 0)));
  printf("ok %llu %016llx\n", (unsigned long long)cases, (unsigned long long)sum);
  return 0;
}

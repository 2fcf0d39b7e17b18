// secp_step.hpp -- the fast ladder step of k_secp_mul (kernels_secp.hip): one wave-uniform test per point operation.
//
// secp256k1.hpp's field operations each end in their own test of a rare condition (Mul's borrow out of word 1,
// square's ripple mask, mul_small's exc and borrow, Add's / double's carry out of word 1 and Sub's borrow, the
// top word of all ones behind every reduce) and branch on it.  On random inputs none of these legs is ever taken, yet
// one ladder step paid ~80 compares and branches for asking.  Here the same arithmetic runs without asking:
//   * the generated field products with the _ACC suffix (tools/gen_field_asm.py) OR their rare lane masks into an
//     SGPR pair the caller owns, and Add / double / Sub (FEC_SECP_{ADD,DBL,SUB}_ACC_ASM) do the same with the carry
//     (borrow) out of word 1;
//   * the condition of every reduce -- a result's top word all ones (2^-32 per lane) -- is folded into the unsigned
//     maximum of the top words: one v_max3 per two results, one compare per point operation;
//   * carries that need a 32-bit word within a few units of 2^32 (Mul's first product of a column, the square's +1
//     inside a limb) are not computed at all: the words that decide them join the same maximum, which is tested
//     against RARE_WORD instead of all ones;
//   * the point operation tests both once, at its end.  If any lane of the wavefront met any of them, the whole
//     wavefront recomputes that operation from its LDS operands with the exact code (the caller's padd_slots +
//     secp::pdouble), which takes every leg where it must.  Otherwise every operation above computed exactly what the
//     exact code computes on its common legs.
// Identity operands (Z == 0: each wavefront's first steps, while a lane's leading scalar bits are zero) are found up
// front, on the one-word Z test, before any work.  The addition's u1 == u2 candidate (its one-word test) joins the
// accumulator.
//
// Device code only: the host emulation (FEC_HOST_EMUL) keeps secp256k1.hpp's portable forms.
#pragma once
#include "secp256k1.hpp"
#include "staging.hpp"

namespace fecgpu {
namespace secp_step {

using secp::pt;

// the rare conditions met so far in one point operation
struct Rare {
  lmask m = 0;   // lanes on which a field operation's rare leg would run
  u32 top = 0;   // unsigned maximum of the words that decide a rare leg by being close to 2^32 (RARE_WORD)
};
// One threshold for every word in Rare::top; each condition below is a subset of `word >= RARE_WORD`:
//   * the top word of a reduced result all ones (every reduce);
//   * Mul's a.w[0] or b.w[7] >= 2^32 - 9 (see mul());
//   * square's W[6], W[14] all ones, W[10] >= 0xFFFFFFFE, W[3] all ones (tools/gen_field_asm.py, secp_sqr).
// Rate on random input, 2^-28 per word and lane: an addition folds 56 words (12 Mul x 3, 4 squares x 5), a doubling
// 37 (2 Mul x 3, 2 mul_small, 5 squares x 5, 4 Add / double), so a wavefront flags 93 * 64 * 2^-28 = 2.2e-5 steps:
// about 93 of the 8.4 million point operations of a 2^20 launch are recomputed with the exact code.
constexpr u32 RARE_WORD = 0xFFFFFFF0u;
// (measured against it: note_top as `rr.m |= lanes_where(r.w[7] == 0xFFFFFFFFu)`, one v_cmp per result straight into
// m -- 12 more VALU and 27 more SALU per step, 28.30 against 28.23 ms at 2^20 on the same box, profiles/fast_step_r05/)
FEC_DEV void note_top(Rare& rr, const fe& r) { rr.top = rr.top > r.w[7] ? rr.top : r.w[7]; }
FEC_DEV void note_word(Rare& rr, u32 x, u32 y) {
  const u32 m = x > y ? x : y;
  rr.top = rr.top > m ? rr.top : m;
}
FEC_DEV bool met(const Rare& rr) { return (rr.m | lanes_where(rr.top >= RARE_WORD)) != 0; }

// Mul (442-507): secp::mul without its borrow continuation and reduce, and without the carry out of the first product
// of columns 2..13 of the product scanning.  That product is a.w[0] * b.w[k] (k <= 7) or a.w[k - 7] * b.w[7], added to a
// carry-in below 9 * 2^32: it passes 2^64 only if both factors are >= 2^32 - 9.  With a.w[0] and b.w[7] below RARE_WORD
// (= 2^32 - 16) no such carry exists, so both words join the maximum that met() tests.
FEC_DEV fe mul(const fe& a, const fe& b, Rare& rr) {
  fe r;
  lmask sc, sink;
  note_word(rr, a.w[0], b.w[7]);
  asm(FEC_SECP_MUL_ACC_ASM
      : "=v"(r.w[0]), "=v"(r.w[1]), "=v"(r.w[2]), "=v"(r.w[3]), "=v"(r.w[4]), "=v"(r.w[5]), "=v"(r.w[6]),
        "=v"(r.w[7]), "=&s"(sc), "=&s"(sink), "+s"(rr.m)
      : FEC_V8(a), FEC_V8(b), "s"(0xD2253531u), "s"(977u)
      : FEC_SECP_MUL_ACC_CLOBBERS);
  note_top(rr, r);
  return r;
}
// Mul by raw 3 / raw 8 (1523, 1533): secp::mul_small_k without its exc / borrow legs and reduce
template <u32 K>
FEC_DEV fe mul_small(const fe& a, Rare& rr) {
  static_assert(K == 3 || K == 8, "the ladder multiplies by 3 and 8 only");
  fe r;
  lmask sc, sink;
  if (K == 3) {
    asm(FEC_SECP_MUL3_ACC_ASM
        : "=v"(r.w[0]), "=v"(r.w[1]), "=v"(r.w[2]), "=v"(r.w[3]), "=v"(r.w[4]), "=v"(r.w[5]), "=v"(r.w[6]),
          "=v"(r.w[7]), "=&s"(sc), "=&s"(sink), "+s"(rr.m)
        : FEC_V8(a), "s"(0xD2253531u), "s"(977u)
        : FEC_SECP_MUL3_ACC_CLOBBERS);
  } else {
    asm(FEC_SECP_MUL8_ACC_ASM
        : "=v"(r.w[0]), "=v"(r.w[1]), "=v"(r.w[2]), "=v"(r.w[3]), "=v"(r.w[4]), "=v"(r.w[5]), "=v"(r.w[6]),
          "=v"(r.w[7]), "=&s"(sc), "=&s"(sink), "+s"(rr.m)
        : FEC_V8(a), "s"(0xD2253531u), "s"(977u)
        : FEC_SECP_MUL8_ACC_CLOBBERS);
  }
  note_top(rr, r);
  return r;
}
// square() (634-713): secp::sqr without its exc leg and reduce, and without the +1 chains' ripple inside the limb they
// enter.  The statement itself folds the four words that decide its rare legs (each against RARE_WORD or a weaker
// bound), and the result's top word, into the running maximum (tools/gen_field_asm.py, secp_sqr).
FEC_DEV fe sqr(const fe& a, Rare& rr) {
  fe r;
  lmask tmp;
  asm(FEC_SECP_SQR_ACC_ASM
      : "=v"(r.w[0]), "=v"(r.w[1]), "=v"(r.w[2]), "=v"(r.w[3]), "=&v"(r.w[4]), "=&v"(r.w[5]), "=&v"(r.w[6]),
        "=&v"(r.w[7]), "=&s"(tmp), "+v"(rr.top)
      : FEC_V8(a), "s"(977u)
      : FEC_SECP_SQR_ACC_CLOBBERS);
  return r;
}
// Add (353-393) and a + a: secp::add / secp::dbl without their top-word and carry legs
FEC_DEV fe add(const fe& a, const fe& b, Rare& rr) {
  fe x = a;
  u32 t0, t1;
  register lmask c asm("vcc");  // the carry (borrow) out of word 1, where the statement's last instruction leaves it
  asm(FEC_SECP_ADD_ACC_ASM : FEC_RW8(x), "=s"(c), "=&v"(t1), "=&v"(t0) : FEC_V8(b));
  rr.m |= c;
  note_top(rr, x);
  return x;
}
FEC_DEV fe dbl(const fe& a, Rare& rr) {
  fe x = a;
  u32 t0, t1;
  register lmask c asm("vcc");  // the carry (borrow) out of word 1, where the statement's last instruction leaves it
  asm(FEC_SECP_DBL_ACC_ASM : FEC_RW8(x), "=s"(c), "=&v"(t1), "=&v"(t0));
  rr.m |= c;
  note_top(rr, x);
  return x;
}
// Sub (395-440): secp::sub without its borrow leg
FEC_DEV fe sub(const fe& a, const fe& b, Rare& rr) {
  fe x = a;
  u32 t0, t1;
  register lmask c asm("vcc");  // the carry (borrow) out of word 1, where the statement's last instruction leaves it
  asm(FEC_SECP_SUB_ACC_ASM : FEC_RW8(x), "=s"(c), "=&v"(t1), "=&v"(t0) : FEC_V8(b));
  rr.m |= c;
  return x;
}

// The up-front identity tests need one word of Z; the operation needs the whole point right after.  Without this
// the compiler sinks the other loads below the test's branch (the fast path is their only user), and the step pays
// two LDS round trips in a row where one does: the empty statement takes the loaded words as inputs, so all of them
// are issued before the one wait the test needs.
FEC_DEV void in_registers(const fe& a, u32 b) { asm volatile("" : : FEC_V8(a), "v"(b)); }
FEC_DEV void in_registers(const fe& a, const fe& b) { asm volatile("" : : FEC_V8(a), FEC_V8(b)); }

// (A ladder point sits in its LDS slot: word w of the point at l[w * TPB].)
// The addition of padd_slots (kernels_secp.hip) -- the same products on the same operands, loaded where they are used,
// with the same sched_barrier placement -- on the common legs only.  False: some lane needs the exact code.
FEC_DEV bool padd_fast(const u32* lp, const u32* lq, pt& o) {
  const fe z1 = load_coord(lp, TPB, 2);
  const u32 z2w0 = lq[16 * TPB];
  in_registers(z1, z2w0);
  if (__builtin_expect(lanes_where((z1.w[0] < z2w0 ? z1.w[0] : z2w0) == 0u) != 0, 0)) return false;
  Rare rr;
  fe z1s, z1c, z2s, z2c;
  {
    z1s = sqr(z1, rr);
    z1c = mul(z1s, z1, rr);
  }
  __builtin_amdgcn_sched_barrier(0);  // keep the loads where they are used (register budget of three waves per SIMD)
  {
    const fe z2 = load_coord(lq, TPB, 2);
    z2s = sqr(z2, rr);
    z2c = mul(z2s, z2, rr);
  }
  __builtin_amdgcn_sched_barrier(0);
  const fe u1 = mul(load_coord(lp, TPB, 0), z2s, rr);
  const fe u2 = mul(load_coord(lq, TPB, 0), z1s, rr);
  __builtin_amdgcn_sched_barrier(0);
  const fe s1 = mul(load_coord(lp, TPB, 1), z2c, rr);
  const fe s2 = mul(load_coord(lq, TPB, 1), z1c, rr);
  __builtin_amdgcn_sched_barrier(0);
  rr.m |= lanes_where(u1.w[0] == u2.w[0]);  // u1 == u2 possible: equal points or their negatives
  const fe h = sub(u2, u1, rr);
  const fe r = sub(s2, s1, rr);
  const fe h2 = sqr(h, rr);
  const fe h3 = mul(h2, h, rr);
  const fe u1h2 = mul(u1, h2, rr);
  o.x = sub(sub(sub(sqr(r, rr), h3, rr), u1h2, rr), u1h2, rr);
  o.y = sub(mul(r, sub(u1h2, o.x, rr), rr), mul(s1, h3, rr), rr);
  o.z = mul(mul(h, load_coord(lp, TPB, 2), rr), load_coord(lq, TPB, 2), rr);
  return !met(rr);
}

// secp::pdouble of the point in slot l on the common legs only.  False: some lane needs the exact code.
FEC_DEV bool pdouble_fast(const u32* l, pt& r) {
  const pt p = {load_coord(l, TPB, 0), load_coord(l, TPB, 1), load_coord(l, TPB, 2)};
  in_registers(p.x, p.y);
  in_registers(p.z, 0u);
  if (__builtin_expect(lanes_where(p.z.w[0] == 0u) != 0, 0)) return false;
  Rare rr;
  const fe a = sqr(p.x, rr);
  const fe b = sqr(p.y, rr);
  const fe c = sqr(b, rr);
  const fe xpb2 = sqr(add(p.x, b, rr), rr);
  const fe d = dbl(sub(sub(xpb2, a, rr), c, rr), rr);
  const fe e = mul_small<3>(a, rr);
  const fe f = sqr(e, rr);
  r.x = sub(f, dbl(d, rr), rr);
  r.y = sub(mul(e, sub(d, r.x, rr), rr), mul_small<8>(c, rr), rr);
  r.z = dbl(mul(p.y, p.z, rr), rr);
  return !met(rr);
}

// One point operation of the ladder: the sum of the points in slots lp and lq (exact(): the exact code on the same
// slots) into slot dst, which may be one of them; the doubling of the point in slot l back into l.  The result is
// written only after the operation's test, so exact() still finds its operands.  (Reading the doubling's operand
// before the sum is written, as the exact step does, keeps both points live at once: 8 more v_mov per step.)
template <class Exact>
FEC_DEV void add_step(const u32* lp, const u32* lq, u32* dst, Exact exact) {
  pt o;
  if (__builtin_expect(!padd_fast(lp, lq, o), 0)) o = exact();
  store_pt(dst, TPB, o);
}
template <class Exact>
FEC_DEV void double_step(u32* l, Exact exact) {
  pt o;
  if (__builtin_expect(!pdouble_fast(l, o), 0)) o = exact();
  store_pt(l, TPB, o);
}

}  // namespace secp_step
}  // namespace fecgpu

// canon_msm.hpp -- CANONICAL-MATH MODE: the per-lane code of the bucket-method multi-scalar multiplication
// sum_i k_i * P_i (fec_canon_msm).  The kernels around it are in canon_msm_kernels.hpp; this file
// builds under FEC_HOST_EMUL (tests/cpp/canon_msm_host.cpp runs the same lane functions serially).
//
// The passes, per slice of the batch and window width c (W = ceil(257 / c) windows, B = 2^(c-1) buckets per window):
//   recode      one lane per element: on_curve, signed digits d_w in [-B, B] with the carry run through the top window,
//               key |d_w| and sign per window (a bad point: every key 0, one bit in the flag word)
//   sort        counting sort of the keys per window (histogram, exclusive scan, scatter): kernels only
//   accumulate  one lane per RUN consecutive sorted entries of one window (accumulate_run): a bucket that lies inside the
//               run is summed and stored; a bucket that crosses a run boundary leaves a partial sum in the next list, and
//               the same function runs on that list (RUN entries per lane again) until one lane holds a window's list
//   reduce      one lane per SEG buckets (reduce_segment): sum b * B_b by two running sums plus a short double-and-add
//   fold        FOLD partial sums per lane, repeated: the segments of a window, then the windows
//   combine     window w doubled w * c times (shift_window)
// Everything is exact for every input: the Weierstrass additions go through jadd_affine / jadd with their P = +-Q and
// infinity legs, Ed25519's formulas are complete.  Nothing here is constant-time.
#pragma once
#include "canon_curves.hpp"

namespace fecgpu {
namespace canon {
namespace msm {

constexpr int MIN_WINDOW = 2, MAX_WINDOW = 16;
constexpr int RUN = 16;    // sorted entries per accumulate lane: no lane adds more, however large a bucket is
constexpr int SEG = 16;    // buckets per reduce lane: the serial chain behind the last slice, kept short
constexpr int FOLD = 8;    // partial sums per fold lane
constexpr u32 EMPTY = 0x80000000u;   // a list entry that carries a key and no point
constexpr u32 NO_KEY = 0xFFFFFFFFu;  // what lies outside a list: never equal to a key

constexpr int windows(int c) { return (257 + c - 1) / c; }
constexpr u32 buckets(int c) { return 1u << (c - 1); }
constexpr size_t div_up(size_t a, size_t b) { return (a + b - 1) / b; }

// The curve-specific half: the accumulator type, its stored form (WORDS u32 each, 16-byte aligned) and the additions.
template <class C>
struct ops;
template <class P>
struct ops<wei<P>> {
  using C = wei<P>;
  using acc = jac;
  static constexpr int WORDS = 24;  // X, Y, Z; all-zero bytes are the point at infinity
  FEC_SDEV acc identity() { return jac_infinity(); }
  FEC_SDEV acc load(const u32* p) {
    acc a;
    a.x = ld8(p);
    a.y = ld8(p + 8);
    a.z = ld8(p + 16);
    return a;
  }
  FEC_SDEV void store(u32* p, const acc& a) {
    st8(p, a.x);
    st8(p + 8, a.y);
    st8(p + 16, a.z);
  }
  FEC_SDEV acc add_point(const acc& a, const aff& q, bool negate) {
    aff t;
    t.x = q.x;
    t.y = fe_select(q.y, C::neg(q.y), lanes_where(negate));
    return C::jadd_affine(a, t, 0);
  }
  // jadd's formulas (add-2007-bl) and jadd's results in every exceptional case -- either operand at infinity, P == Q,
  // P == -Q -- with those cases behind one wave-uniform branch: jadd itself computes its doubling on every call, which
  // table building can afford and the chains of full additions here cannot.
  FEC_SDEV acc add(const acc& p, const acc& q) {
    fe z1z1 = C::sqr(p.z), z2z2 = C::sqr(q.z);
    fe u1 = C::mul(p.x, z2z2), u2 = C::mul(q.x, z1z1);
    fe s1 = C::mul(C::mul(p.y, q.z), z2z2), s2 = C::mul(C::mul(q.y, p.z), z1z1);
    fe h = C::sub(u2, u1);
    fe i = C::sqr(C::dbl(h));
    fe j = C::mul(h, i);
    fe rr = C::dbl(C::sub(s2, s1));
    fe v = C::mul(u1, i);
    acc o;
    o.x = C::sub(C::sub(C::sqr(rr), j), C::dbl(v));
    o.y = C::sub(C::mul(rr, C::sub(v, o.x)), C::dbl(C::mul(s1, j)));
    o.z = C::mul(C::sub(C::sub(C::sqr(C::add(p.z, q.z)), z1z1), z2z2), h);
    const lmask pinf = fe_is_zero(p.z), qinf = fe_is_zero(q.z);
    const lmask hzero = fe_is_zero(h) & ~pinf & ~qinf;
    if (__builtin_expect((pinf | qinf | hzero) != 0, 0)) {
      if (hzero != 0) {   // the same x: P == Q (double) or P == -Q (infinity)
        const lmask same = hzero & fe_is_zero(rr);
        const acc d = C::jdouble(p);
        o = jac_select(o, jac_infinity(), hzero & ~same);
        o = jac_select(o, d, same);
      }
      o = jac_select(o, q, pinf);
      o = jac_select(o, p, qinf & ~pinf);
    }
    return o;
  }
  FEC_SDEV acc dbl(const acc& a) { return C::jdouble(a); }
  // what the batched normalisation takes: X, Y and Z apart
  FEC_SDEV void emit(const acc& a, u32* xy, u32* z) {
    st8(xy, a.x);
    st8(xy + 8, a.y);
    st8(z, a.z);
  }
};
template <>
struct ops<edw> {
  using C = edw;
  using acc = ext;
  static constexpr int WORDS = 32;  // X, Y, Z, T
  FEC_SDEV acc identity() { return edw::identity(); }
  FEC_SDEV acc load(const u32* p) {
    acc a;
    a.x = ld8(p);
    a.y = ld8(p + 8);
    a.z = ld8(p + 16);
    a.t = ld8(p + 24);
    return a;
  }
  FEC_SDEV void store(u32* p, const acc& a) {
    st8(p, a.x);
    st8(p + 8, a.y);
    st8(p + 16, a.z);
    st8(p + 24, a.t);
  }
  FEC_SDEV acc add_point(const acc& a, const aff& q, bool negate) {
    niels nq;
    nq.ypx = edw::add(q.y, q.x);
    nq.ymx = edw::sub(q.y, q.x);
    nq.t2d = edw::mul(edw::mul(q.x, q.y), edw::d2());
    return edw::add_niels(a, nq, lanes_where(negate), 0);
  }
  FEC_SDEV acc add(const acc& a, const acc& b) { return edw::add_pniels(a, edw::to_pniels(b), 0, 0); }
  FEC_SDEV acc dbl(const acc& a) { return edw::dbl<true>(a); }
  FEC_SDEV void emit(const acc& a, u32* xy, u32* z) {
    st8(xy, a.x);
    st8(xy + 8, a.y);
    st8(z, a.z);
  }
};

// k = sum_w d_w 2^(c w), |d_w| <= 2^(c-1), for any 256-bit k (8 words at k): emit(w, |d_w|, d_w < 0) for w = 0 .. W-1.
// Window w reads bits [c w, c w + c) plus the carry from below; a value above 2^(c-1) becomes value - 2^c and carries.
// W * c >= 257, so the top window holds bit 256 (zero) and its value is at most 2^(c-1): nothing is carried out of it.
template <class Emit>
FEC_DEV void recode(const u32* k, int c, Emit&& emit) {
  const int W = windows(c);
  const u32 half = 1u << (c - 1), full = 1u << c;
  u32 carry = 0;
#pragma unroll 1
  for (int w = 0; w < W; ++w) {
    const int bit = w * c;
    u32 raw = 0;
    if (bit < 256) {
      const int wd = bit >> 5;
      u64 two = k[wd];
      if (wd + 1 < 8) two |= (u64)k[wd + 1] << 32;
      raw = (u32)(two >> (bit & 31)) & (full - 1u);
    }
    raw += carry;
    carry = raw > half ? 1u : 0u;
    emit(w, carry ? full - raw : raw, carry);
  }
}

// One lane of the accumulate pass: entries [run * RUN, run * RUN + RUN) of one window's list of `len` entries, whose keys
// are non-decreasing.  LEVEL0: the list is the sorted slice -- keys[pos] the bucket (0: no contribution), src[pos] =
// element << 1 | sign, the element's affine point at points + 16 * element; a bucket that begins in this run starts from
// its stored value.  Otherwise the list holds partial sums: keys[pos] = key, or key | EMPTY for an entry without a point,
// the point at src + WORDS * pos; the sum starts from nothing.
// A segment (the entries of one key) that neither continues from the run before nor into the run after belongs to this
// lane alone and is stored to bucket[key - 1]: because the run that holds a bucket's first entry has taken the stored value
// in, every store is the bucket's whole new value, and no two lanes ever write one bucket in one pass.  The first and the
// last segment may cross: they go to the next list, entries 2 * run and 2 * run + 1, in order, and whichever of the two
// is not needed is written as EMPTY with its segment's key, so the next list is again dense and sorted.
// out_keys == nullptr: one lane holds the whole list, nothing crosses, nothing is written out.
template <class C, bool LEVEL0>
FEC_DEV void accumulate_run(const u32* keys, const u32* src, const u32* points, size_t len, size_t run, u32* bucket,
                            u32* out_keys, u32* out_pts) {
  using O = ops<C>;
  using A = typename O::acc;
  const size_t lo = run * (size_t)RUN, hi = lo + RUN < len ? lo + RUN : len;
  if (lo >= hi) return;
  const u32 before = lo == 0 ? NO_KEY : keys[lo - 1] & ~EMPTY;
  const u32 after = hi == len ? NO_KEY : keys[hi] & ~EMPTY;
  u32 cur = NO_KEY;
  bool have = false, open_left = false, first_seg = true;
  A a = O::identity();
  // closes the segment of key `cur`; closed_right: it does not continue into the next run; last: no segment follows
  auto flush = [&](bool closed_right, bool last) {
    const bool owned = !open_left && closed_right;
    if (owned && have) O::store(bucket + (size_t)(cur - 1u) * O::WORDS, a);
    if (out_keys) {
      const bool carry = !owned && have;
      if (first_seg) {
        out_keys[2 * run] = carry ? cur : (cur | EMPTY);
        if (carry) O::store(out_pts + (2 * run) * O::WORDS, a);
      }
      if (last) {
        const bool here = carry && !first_seg;
        out_keys[2 * run + 1] = here ? cur : (cur | EMPTY);
        if (here) O::store(out_pts + (2 * run + 1) * O::WORDS, a);
      }
    }
    first_seg = false;
  };
#pragma unroll 1
  for (size_t pos = lo; pos < hi; ++pos) {
    const u32 kw = keys[pos], key = kw & ~EMPTY;
    if (key != cur) {
      if (cur != NO_KEY) flush(true, false);
      cur = key;
      a = O::identity();
      have = false;
      open_left = pos == lo && before == key;
      if (LEVEL0 && key != 0 && !open_left) {
        a = O::load(bucket + (size_t)(key - 1u) * O::WORDS);
        have = true;
      }
    }
    if (LEVEL0) {
      if (key != 0) {
        const u32 e = src[pos];
        aff q;
        q.x = ld8(points + (size_t)(e >> 1) * 16);
        q.y = ld8(points + (size_t)(e >> 1) * 16 + 8);
        a = O::add_point(a, q, (e & 1u) != 0);
        have = true;
      }
    } else if (!(kw & EMPTY)) {
      const A q = O::load(src + pos * O::WORDS);
      a = have ? O::add(a, q) : q;
      have = true;
    }
  }
  flush(after != cur, true);
}

// One lane of the reduce pass: sum over the buckets b in (lo, hi], lo = seg * SEG, hi = min(lo + SEG, B), of b * B_b.
// Walking down from hi, run = sum of the buckets seen and sum = sum of the runs = sum (b - lo) * B_b; then lo * run by
// double-and-add (lo < 2^15).  Empty buckets, infinity and run == sum (a doubling) all go through the complete addition.
template <class C>
FEC_DEV typename ops<C>::acc reduce_segment(const u32* bucket, u32 B, u32 seg) {
  using O = ops<C>;
  using A = typename O::acc;
  const u32 lo = seg * (u32)SEG, hi = lo + SEG < B ? lo + SEG : B;
  A run = O::identity(), sum = O::identity();
#pragma unroll 1
  for (u32 b = hi; b > lo; --b) {
    run = O::add(run, O::load(bucket + (size_t)(b - 1u) * O::WORDS));
    sum = O::add(sum, run);
  }
  if (lo != 0) {
    A t = O::identity();
#pragma unroll 1
    for (int bit = MAX_WINDOW - 2; bit >= 0; --bit) {
      t = O::dbl(t);
      if ((lo >> bit) & 1u) t = O::add(t, run);
    }
    sum = O::add(sum, t);
  }
  return sum;
}

// One lane of a fold: the sum of entries [lane * FOLD, lane * FOLD + FOLD) of `cnt` stored accumulators.
template <class C>
FEC_DEV typename ops<C>::acc fold_group(const u32* in, size_t cnt, size_t lane) {
  using O = ops<C>;
  const size_t lo = lane * (size_t)FOLD, hi = lo + FOLD < cnt ? lo + FOLD : cnt;
  typename ops<C>::acc s = O::load(in + lo * O::WORDS);
#pragma unroll 1
  for (size_t j = lo + 1; j < hi; ++j) s = O::add(s, O::load(in + j * O::WORDS));
  return s;
}

// 2^(c w) * S_w: window w's sum on its place
template <class C>
FEC_DEV typename ops<C>::acc shift_window(typename ops<C>::acc s, int doublings) {
#pragma unroll 1
  for (int i = 0; i < doublings; ++i) s = ops<C>::dbl(s);
  return s;
}

}  // namespace msm
}  // namespace canon
}  // namespace fecgpu

// canon_bip32_kernels.hpp -- kernels of the canonical-mode tweak-add and BIP-32 derivation (canon_bip32.hpp), included by
// canon.hip.  One element per lane, no LDS.  The public kernels take public inputs; for k_canon_seckey_tweak_add and
// k_canon_bip32_priv what canon_sign.hpp says about secrets holds: addresses depend on the element's index only, branches on
// the index, on the call's uniform arguments and on nothing else.
#pragma once
#include "canon_kernels.hpp"
#include "canon_sign_kernels.hpp"
#include "canon_bip32.hpp"

namespace fecgpu {

// What k_canon_bip32_parent leaves for a batch that shares one parent, as words: the parent's affine x, y (16), the two HMAC
// states of its chain code (16 + 16, high word first), whether the key decoded (1).
constexpr int BIP32_SHARED_WORDS = 64;
FEC_DEV void bip32_store_mid(u32* w, const canon::hmac_mid& m) {
  FEC_UNROLL for (int j = 0; j < 8; ++j) {
    w[2 * j] = (u32)(m.inner.h[j] >> 32);
    w[2 * j + 1] = (u32)m.inner.h[j];
    w[16 + 2 * j] = (u32)(m.outer.h[j] >> 32);
    w[16 + 2 * j + 1] = (u32)m.outer.h[j];
  }
}
FEC_DEV canon::hmac_mid bip32_load_mid(const u32* w) {
  canon::hmac_mid m;
  FEC_UNROLL for (int j = 0; j < 8; ++j) {
    m.inner.h[j] = ((u64)w[2 * j] << 32) | w[2 * j + 1];
    m.outer.h[j] = ((u64)w[16 + 2 * j] << 32) | w[16 + 2 * j + 1];
  }
  return m;
}

// fec_canon_pubkey_tweak_add, before the multiplication: key i in `form` (33, 65 or 32), tweak i as 32 big-endian bytes ->
// t as limbs, the affine key, the flag (canon::tweak_prepare).  P = SecpParams / P256Params.
template <class P>
__global__ __launch_bounds__(TPB, 2) void k_canon_tweak_prepare(const unsigned char* __restrict__ pks, int form,
                                                                const u32* __restrict__ tweaks, u32* __restrict__ ts,
                                                                u32* __restrict__ qxy, unsigned char* __restrict__ flag, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  canon::aff Q;
  const lmask ok = canon::tweak_key<P>(pks, i, form, Q);
  fe t = canon::be_integer(canon::ld8(tweaks + i * 8));
  flag[i] = canon::tweak_prepare<P>(ok, t, Q);
  canon::st8(ts + i * 8, t);
  canon::st8(qxy + i * 16, Q.x);
  canon::st8(qxy + i * 16 + 8, Q.y);
}

// One parent for the whole batch: decoded once, its chain code's two HMAC states computed once.  One lane.
template <class P>
__global__ __launch_bounds__(64) void k_canon_bip32_parent(const unsigned char* __restrict__ pk, const u32* __restrict__ cc,
                                                           u32* __restrict__ shared) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  canon::aff K;
  const bool ok = lane_of(canon::sec1_record<P>(pk, 0, false, K));
  if (!ok) K = canon::wei<P>::generator();
  u32 key[8];
  canon::chain_code_key(canon::ld8(cc), key);
  canon::st8(shared, K.x);
  canon::st8(shared + 8, K.y);
  bip32_store_mid(shared + 16, canon::hmac_sha512_midstates(key));
  shared[48] = ok ? 1u : 0u;
}

// CKDpub before the multiplication.  SHARED = false: parent i and chain code i, four compressions; true: the block
// k_canon_bip32_parent left, two compressions, the parent read by every lane at one address.  Writes IL as limbs, the parent
// (or G) as affine x, y, the child chain code to out_cc and the flag; k_canon_tweak_finish clears a refused element's chain code.
template <class P, bool SHARED>
__global__ __launch_bounds__(TPB, 2) void k_canon_bip32_pub_prepare(const unsigned char* __restrict__ pks, const u32* __restrict__ ccs,
                                                                    const u32* __restrict__ shared, const u32* __restrict__ indices,
                                                                    u32* __restrict__ ils, u32* __restrict__ qxy,
                                                                    u32* __restrict__ out_cc, unsigned char* __restrict__ flag,
                                                                    size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  canon::aff K;
  canon::hmac_mid mid;
  lmask ok;
  if constexpr (SHARED) {
    K.x = canon::ld8(shared);
    K.y = canon::ld8(shared + 8);
    mid = bip32_load_mid(shared + 16);
    ok = lanes_where(shared[48] != 0);
  } else {
    ok = canon::sec1_record<P>(pks, i, false, K);
    u32 key[8];
    canon::chain_code_key(canon::ld8(ccs + i * 8), key);
    mid = canon::hmac_sha512_midstates(key);
  }
  fe il, ir;
  flag[i] = canon::bip32_pub_prepare<P>(mid, ok, K, indices[i], il, ir);
  canon::st8(ils + i * 8, il);
  canon::st8(qxy + i * 16, K.x);
  canon::st8(qxy + i * 16 + 8, K.y);
  canon::st8(out_cc + i * 8, ir);
}

// (xy[i], zbuf[i]) += the affine point qxy[i]: the step between the comb (finish = false) and the batched normalisation.
// The normalisation reads the point status this leaves and finds infinity from Z itself.
template <class W>
__global__ __launch_bounds__(TPB, 2) void k_canon_add_affine(u32* __restrict__ xy, u32* __restrict__ zbuf, const u32* __restrict__ qxy,
                                                             unsigned char* __restrict__ status, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  canon::jac a;
  a.x = canon::ld8(xy + i * 16);
  a.y = canon::ld8(xy + i * 16 + 8);
  a.z = canon::ld8(zbuf + i * 8);
  canon::aff q;
  q.x = canon::ld8(qxy + i * 16);
  q.y = canon::ld8(qxy + i * 16 + 8);
  const canon::jac r = canon::add_affine_step<W>(a, q);
  canon::st8(xy + i * 16, r.x);
  canon::st8(xy + i * 16 + 8, r.y);
  canon::st8(zbuf + i * 8, r.z);
  status[i] = CANON_FINITE;
}

// The end of both public calls: flags and point status fold into status[i]; the point is encoded, or zeros are written.
// ccs (BIP-32 only, else null): the child chain codes the prepare kernel wrote, cleared where the status is not 0.
template <int FORM>
__global__ __launch_bounds__(TPB) void k_canon_tweak_finish(const u32* __restrict__ xy, const unsigned char* __restrict__ flag,
                                                            const unsigned char* __restrict__ point_status,
                                                            unsigned char at_infinity, unsigned char* __restrict__ out,
                                                            u32* __restrict__ ccs, unsigned char* __restrict__ status, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const unsigned char st = canon::tweak_finish<FORM>(canon::ld8(xy + i * 16), canon::ld8(xy + i * 16 + 8), flag[i], point_status[i],
                                                     at_infinity, out + i * (size_t)FORM);
  if (ccs && st != 0) canon::st8(ccs + i * 8, fe_zero());
  status[i] = st;
}

// fec_canon_seckey_tweak_add: 32 big-endian bytes each way
template <class N>
__global__ __launch_bounds__(TPB) void k_canon_seckey_tweak_add(const u32* __restrict__ keys, const u32* __restrict__ tweaks,
                                                                u32* __restrict__ out, unsigned char* __restrict__ status, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  fe r;
  status[i] = canon::seckey_tweak_add<N>(canon::be_integer(canon::ld8(keys + i * 8)), canon::be_integer(canon::ld8(tweaks + i * 8)), r);
  canon::st8(out + i * 8, canon::be_bytes(r));
}

// CKDpriv behind k_canon_key_limbs and, with COMB, the secret comb over the parent keys: ds = the parents' limbs, kst their
// status, pxy = k G affine.  per_elem = 1: parent i and chain code i; 0: one parent for all.  COMB = false
// (FEC_CANON_BIP32_NO_COMB): pxy is not read, a non-hardened lane gets BIP32_BAD_INDEX.
template <bool COMB>
__global__ __launch_bounds__(TPB, 2) void k_canon_bip32_priv(const u32* __restrict__ ds, const unsigned char* __restrict__ kst,
                                                             const u32* __restrict__ pxy, const u32* __restrict__ ccs,
                                                             size_t per_elem, const u32* __restrict__ indices,
                                                             u32* __restrict__ out_keys, u32* __restrict__ out_ccs,
                                                             unsigned char* __restrict__ status, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const size_t p = i * per_elem;
  const fe k = canon::ld8(ds + p * 8);
  fe px = fe_zero(), py = fe_zero();
  if constexpr (COMB) {
    px = canon::ld8(pxy + p * 16);
    py = canon::ld8(pxy + p * 16 + 8);
  }
  u32 key[8];
  canon::chain_code_key(canon::ld8(ccs + p * 8), key);
  fe child, ir;
  status[i] = canon::bip32_priv(canon::hmac_sha512_midstates(key), kst[p], k, px, py, indices[i], !COMB, child, ir);
  canon::st8(out_keys + i * 8, canon::be_bytes(child));
  canon::st8(out_ccs + i * 8, ir);
}

}  // namespace fecgpu

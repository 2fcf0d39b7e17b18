// canon_wallet_kernels.hpp -- kernels of the canonical-mode RIPEMD-160 / HASH160 calls, the Taproot output key and CKDpub
// along a path (ripemd160.hpp, canon_wallet.hpp), included by canon.hip.  One element per lane, no LDS.  Every input is
// public.
#pragma once
#include "canon_bip32_kernels.hpp"
#include "canon_wallet.hpp"

namespace fecgpu {

// 20 digest bytes as 5 words at a 4-byte-aligned record
FEC_DEV void wallet_store20(u32* o, const ripemd160::state& d, bool keep) {
  FEC_UNROLL for (int j = 0; j < 5; ++j) o[j] = keep ? d.h[j] : 0u;
}

// fec_canon_ripemd160 (DOUBLE = false) and fec_canon_hash160 (true): message i -> 20 bytes.  Every lane checks its own range;
// a bad one gets a zero digest and, where status is not null, 4.
template <bool DOUBLE>
__global__ __launch_bounds__(TPB, 4) void k_canon_ripemd160(Messages m, u32* __restrict__ out, unsigned char* __restrict__ status,
                                                            size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const unsigned char* msg;
  u64 len;
  const bool in_range = message_at(m, i, msg, len);
  ripemd160::state d = ripemd160::init();
  if (in_range) d = DOUBLE ? ripemd160::hash160(msg, len) : ripemd160::hash(msg, len);
  wallet_store20(out + i * 5, d, in_range);
  if (status) status[i] = in_range ? 0 : 4;
}

// fec_canon_pubkey_hash160: HASH160 of record i, pk_len bytes as they lie (33 or 65; any alignment)
__global__ __launch_bounds__(TPB, 4) void k_canon_pubkey_hash160(const unsigned char* __restrict__ pks, size_t pk_len,
                                                                 u32* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  wallet_store20(out + i * 5, ripemd160::hash160(pks + i * pk_len, pk_len), true);
}

// fec_canon_taproot_output_key, before the multiplication: internal key i in `form` (32 or 33), root i as 32 bytes or no roots
// at all (null) -> t as limbs, P affine, the flag (canon::taproot_prepare).
template <class P>
__global__ __launch_bounds__(TPB, 2) void k_canon_taproot_prepare(const unsigned char* __restrict__ pks, int form,
                                                                  const u32* __restrict__ roots, u32* __restrict__ ts,
                                                                  u32* __restrict__ qxy, unsigned char* __restrict__ flag, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  canon::aff Q;
  fe x, t;
  const lmask ok = canon::taproot_key<P>(pks, i, form, x, Q);
  const bool has_root = roots != nullptr;
  const fe root = has_root ? canon::ld8(roots + i * 8) : fe_zero();
  flag[i] = canon::taproot_prepare<P>(ok, x, has_root, root, t, Q);
  canon::st8(ts + i * 8, t);
  canon::st8(qxy + i * 16, Q.x);
  canon::st8(qxy + i * 16 + 8, Q.y);
}

// ... and behind the normalisation: x(Q), the parity of y(Q), the status
__global__ __launch_bounds__(TPB) void k_canon_taproot_finish(const u32* __restrict__ xy, const unsigned char* __restrict__ flag,
                                                              const unsigned char* __restrict__ point_status,
                                                              unsigned char* __restrict__ out, unsigned char* __restrict__ parity,
                                                              unsigned char* __restrict__ status, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  unsigned char par;
  status[i] = canon::taproot_finish(canon::ld8(xy + i * 16), canon::ld8(xy + i * 16 + 8), flag[i], point_status[i], out + i * 32, par);
  parity[i] = par;
}

// Column `level` of the row-major index matrix, for the first level's prepare kernel, which reads one index per element
__global__ __launch_bounds__(TPB) void k_canon_path_indices(const u32* __restrict__ indices, size_t depth, size_t level,
                                                            u32* __restrict__ out, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i < n) out[i] = indices[i * depth + level];
}

// A path of one level: the fingerprint of the given parent, from the affine point the prepare kernel left in qxy
__global__ __launch_bounds__(TPB, 2) void k_canon_path_fingerprint(const u32* __restrict__ qxy, u32* __restrict__ fp, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  canon::aff K;
  K.x = canon::ld8(qxy + i * 16);
  K.y = canon::ld8(qxy + i * 16 + 8);
  fp[i] = canon::bip32_fingerprint(K);
}

// One level of a path behind the first: the previous level's child (xy, affine, with its point status) is this level's parent,
// ccs holds the running chain code and takes the next.  Writes IL, the addend, the merged flag (canon::bip32_path_step).
// fp (the last level only, and only where fingerprints are asked for; else null): the parent's fingerprint.
template <class P>
__global__ __launch_bounds__(TPB, 2) void k_canon_bip32_path_step(const u32* __restrict__ xy, const unsigned char* __restrict__ point_status,
                                                                  const u32* __restrict__ indices, size_t depth, size_t level,
                                                                  u32* __restrict__ ils, u32* __restrict__ qxy, u32* __restrict__ ccs,
                                                                  unsigned char* __restrict__ flag, u32* __restrict__ fp, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  canon::aff K;
  K.x = canon::ld8(xy + i * 16);
  K.y = canon::ld8(xy + i * 16 + 8);
  if (fp) fp[i] = canon::bip32_fingerprint(K);
  u32 key[8];
  canon::chain_code_key(canon::ld8(ccs + i * 8), key);
  fe il, ir;
  flag[i] = canon::bip32_path_step<P>(canon::hmac_sha512_midstates(key), flag[i], point_status[i], indices[i * depth + level], K, il, ir);
  canon::st8(ils + i * 8, il);
  canon::st8(qxy + i * 16, K.x);
  canon::st8(qxy + i * 16 + 8, K.y);
  canon::st8(ccs + i * 8, ir);
}

// The end of a path: the child's 33 bytes and status; chain code, fingerprint and HASH160 cleared where the status is not 0.
// fp, h160: null where the caller did not ask.
__global__ __launch_bounds__(TPB, 2) void k_canon_bip32_path_finish(const u32* __restrict__ xy, const unsigned char* __restrict__ flag,
                                                                    const unsigned char* __restrict__ point_status,
                                                                    unsigned char* __restrict__ out, u32* __restrict__ ccs,
                                                                    u32* __restrict__ fp, u32* __restrict__ h160,
                                                                    unsigned char* __restrict__ status, size_t n) {
  const size_t i = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (i >= n) return;
  const unsigned char st = canon::bip32_path_finish(canon::ld8(xy + i * 16), canon::ld8(xy + i * 16 + 8), flag[i], point_status[i],
                                                    out + i * 33, h160 ? h160 + i * 5 : nullptr);
  if (st != 0) {
    canon::st8(ccs + i * 8, fe_zero());
    if (fp) fp[i] = 0u;
  }
  status[i] = st;
}

}  // namespace fecgpu

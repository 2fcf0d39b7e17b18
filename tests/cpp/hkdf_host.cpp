// Host build of forge_ec_amd/csrc/hkdf.hpp (FEC_HOST_EMUL): the per-element code of k_derive_key as a C function, so that
// tests/test_hkdf_host.py can compare it with the fixture and with hashlib over the same grid.  Test infrastructure only.
// With -DHKDF_HOST_MAIN the same file is a stand-alone program that runs the grid with every input ending at the last
// byte of its allocation and every key row inside an exact-size allocation behind its neighbours, and compares the two
// load paths and every store class with a byte-wise model of the same chain: what a sanitizer build
// (-fsanitize=address,undefined) is run on.
#define FEC_HOST_EMUL 1
#include "../../forge_ec_amd/csrc/hkdf.hpp"

#include <string.h>

using namespace fecgpu;

extern "C" {
// keys[i] = derive_key(secrets[i], info, out_len) for i < n, rows packed; xor_form: P256's placeholder, else HKDF.
// `keys` must be 16-byte aligned (as the ABI asks of d_keys).  Returns 0, or -1 for lengths the ABI refuses.
int hh_derive_key(int xor_form, const uint8_t* secrets, size_t secret_len, const uint8_t* info, size_t info_len, size_t out_len,
                  uint8_t* keys, size_t n) {
  if (secret_len > hkdf::MAX_SECRET || info_len > hkdf::MAX_INFO || out_len > hkdf::MAX_OUT) return -1;
  const hkdf::Params p = hkdf::make_params(xor_form != 0, info, info_len, secret_len, out_len);
  const bool words = (secret_len & 3u) == 0 && ((uintptr_t)secrets & 3u) == 0;
  for (size_t i = 0; i < n; ++i) {
    u32 sec[16];
    hkdf::load_secret(secrets + i * secret_len, (u32)secret_len, words, sec);
    if (xor_form) hkdf::derive_key<true>(p, sec, false, keys + i * out_len);
    else hkdf::derive_key<false>(p, sec, false, keys + i * out_len);
  }
  return 0;
}
}

#ifdef HKDF_HOST_MAIN
#include <stdio.h>
#include <stdlib.h>

#include <vector>

namespace {

// SHA-256 and HMAC over byte strings, on the header's own compress: the model the chain is compared with
std::vector<uint8_t> sha256_bytes(const std::vector<uint8_t>& m) {
  std::vector<uint8_t> b(m);
  b.push_back(0x80);
  while (b.size() % 64 != 56) b.push_back(0);
  const uint64_t bits = (uint64_t)m.size() * 8;
  for (int k = 7; k >= 0; --k) b.push_back((uint8_t)(bits >> (8 * k)));
  sha256::state st = sha256::init();
  for (size_t o = 0; o < b.size(); o += 64) {
    u32 w[16];
    for (int j = 0; j < 16; ++j) w[j] = (u32)b[o + 4 * j] << 24 | (u32)b[o + 4 * j + 1] << 16 | (u32)b[o + 4 * j + 2] << 8 | b[o + 4 * j + 3];
    sha256::compress(st, w);
  }
  std::vector<uint8_t> d(32);
  for (int j = 0; j < 8; ++j)
    for (int k = 0; k < 4; ++k) d[4 * j + k] = (uint8_t)(st.h[j] >> (24 - 8 * k));
  return d;
}
std::vector<uint8_t> hmac(const std::vector<uint8_t>& key, const std::vector<uint8_t>& data) {
  std::vector<uint8_t> in(64, 0x36), outer(64, 0x5c);
  for (size_t k = 0; k < key.size(); ++k) {
    in[k] ^= key[k];
    outer[k] ^= key[k];
  }
  in.insert(in.end(), data.begin(), data.end());
  const std::vector<uint8_t> d = sha256_bytes(in);
  outer.insert(outer.end(), d.begin(), d.end());
  return sha256_bytes(outer);
}
std::vector<uint8_t> model(bool xor_form, const uint8_t* sec, size_t sl, const uint8_t* info, size_t il, size_t L) {
  std::vector<uint8_t> okm;
  if (xor_form) {
    okm.assign(L, 0);
    for (size_t i = 0; i < sl && i < L; ++i) okm[i] ^= sec[i];
    for (size_t i = 0; i < il && i < L; ++i) okm[i] ^= info[i];
    return okm;
  }
  const std::vector<uint8_t> prk = hmac(std::vector<uint8_t>(32, 0), std::vector<uint8_t>(sec, sec + sl));
  std::vector<uint8_t> t;
  uint8_t counter = 1;
  while (okm.size() < L) {
    std::vector<uint8_t> d(t);
    d.insert(d.end(), info, info + il);
    d.push_back(counter);
    t = hmac(prk, d);
    for (size_t k = 0; k < 32 && okm.size() < L; ++k) okm.push_back(t[k]);
    ++counter;
  }
  return okm;
}

}  // namespace

int main() {
  const size_t sls[] = {0, 1, 22, 32, 55, 56, 64}, ils[] = {0, 1, 22, 23, 54, 55, 86, 87, 118, 119, 1024},
               ols[] = {0, 1, 31, 32, 33, 48, 56, 60, 64, 65, 8128};
  const size_t n = 5;   // rows at five different alignments when out_len is odd
  unsigned long checked = 0;
  uint32_t x = 0x2545F491u;
  for (int xor_form = 0; xor_form < 2; ++xor_form)
    for (size_t sl : sls)
      for (size_t il : ils)
        for (size_t ol : ols) {
          if (ol == 8128 && !(sl == 32 && (il == 23 || il == 1024))) continue;
          // exact-size allocations: a read or a write one byte past either end is a heap-buffer-overflow
          uint8_t* sec = (uint8_t*)malloc(n * sl ? n * sl : 1);
          uint8_t* info = il ? (uint8_t*)malloc(il) : nullptr;
          uint8_t* keys = (uint8_t*)aligned_alloc(16, (n * ol + 15) / 16 * 16 ? (n * ol + 15) / 16 * 16 : 16);
          for (size_t k = 0; k < n * sl; ++k) sec[k] = (uint8_t)((x = x * 1664525u + 1013904223u) >> 24);
          for (size_t k = 0; k < il; ++k) info[k] = (uint8_t)((x = x * 1664525u + 1013904223u) >> 24);
          const size_t cap = (n * ol + 15) / 16 * 16;
          for (size_t k = 0; k < cap; ++k) keys[k] = 0xA5;
          if (hh_derive_key(xor_form, sl ? sec : nullptr, sl, info, il, ol, keys, n) != 0) return 2;
          for (size_t i = 0; i < n; ++i) {
            const std::vector<uint8_t> want = model(xor_form != 0, sec + i * sl, sl, info, il, ol);
            if (ol && memcmp(keys + i * ol, want.data(), ol) != 0) {
              printf("MISMATCH form %d secret_len %zu info_len %zu out_len %zu row %zu\n", xor_form, sl, il, ol, i);
              return 1;
            }
            ++checked;
          }
          for (size_t k = n * ol; k < cap; ++k)
            if (keys[k] != 0xA5) {
              printf("WROTE PAST THE ROWS form %d secret_len %zu info_len %zu out_len %zu\n", xor_form, sl, il, ol);
              return 1;
            }
          free(sec);
          free(info);
          free(keys);
        }
  if (hh_derive_key(0, nullptr, 65, nullptr, 0, 32, nullptr, 0) != -1 || hh_derive_key(0, nullptr, 0, nullptr, 1025, 32, nullptr, 0) != -1 ||
      hh_derive_key(1, nullptr, 0, nullptr, 0, 8129, nullptr, 0) != -1)
    return 3;
  printf("hkdf_host: %lu rows equal the byte-wise model\n", checked);
  return 0;
}
#endif

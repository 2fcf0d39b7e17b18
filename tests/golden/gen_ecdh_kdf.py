"""
Generates tests/golden/ecdh_kdf_vectors.json: KeyExchange::derive_key, derive_shared_secret + derive_key and
KeyExchange::exchange fixtures from the restatement tests/ecdh_kdf_ref.py over oracle/py_model.py
(restatement-derived; not reference-executed).

  python tests/golden/gen_ecdh_kdf.py

{"a3": RFC 5869 test case A.3 (the one standard vector: a zero-length salt is 32 zero bytes),
 "secret_pool", "info_pool": 64 and 1024 seeded bytes; a derive_key case uses their first secret_len / info_len bytes,
 "derive_key": [curve, secret_len, info_len, out_len, okm hex] over SECRET_LENS x INFO_LENS x OUT_LENS per curve -- the
   info lengths are the ones at which the padding of T(1)'s input (65 + info_len bytes with the pad block) and of a later
   block's (97 + info_len) spills into another compression -- plus one case at out_len 8128, the longest the u8 counter
   of the reference allows,
 "exchange": the cases of ecdh_vectors.json (sk = 0, an infinite peer, P-256 points the reference rejects among them)
   through ecdh_derive_key and exchange with two info strings: status, key, public_xy, public_inf}.
"""
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import ecdh_kdf_ref as K  # noqa: E402

EXCHANGE_INFOS = ((b"", 32), (b"forge-ec ecdh fixture 1", 33))   # (info, out_len): 0 and 23 bytes


def main():
    rng = random.Random(0x4B4446)
    secret_pool = bytes(rng.getrandbits(8) for _ in range(K.MAX_SECRET))
    info_pool = bytes(rng.getrandbits(8) for _ in range(K.MAX_INFO))
    out = {"provenance": "restatement-derived by tests/ecdh_kdf_ref.py over oracle/py_model.py; not reference-executed; a3 is RFC 5869 A.3",
           "a3": {"ikm": K.A3_IKM.hex(), "info": "", "out_len": K.A3_L, "okm": K.hkdf_zero_salt(K.A3_IKM, b"", K.A3_L).hex()},
           "secret_pool": secret_pool.hex(), "info_pool": info_pool.hex(), "derive_key": [], "exchange": []}
    assert out["a3"]["okm"] == K.A3_OKM.hex()
    for curve in (0, 1):
        grid = [(s, i, o) for s in K.SECRET_LENS for i in K.INFO_LENS for o in K.OUT_LENS] + [(32, 23, K.MAX_OUT)]
        for s, i, o in grid:
            out["derive_key"].append([curve, s, i, o, K.derive_key(curve, secret_pool[:s], info_pool[:i], o).hex()])
    ecdh = json.load(open(os.path.join(HERE, "ecdh_vectors.json")))["cases"]
    for info, out_len in EXCHANGE_INFOS:
        for c in ecdh:
            xy, inf, keys, st = K.exchange(None, c["curve"], [c["sk"]], [c["pk"]], [c["pk_inf"]], info, out_len)
            assert int(st[0]) == c["status"]
            out["exchange"].append({"curve": c["curve"], "note": c["note"], "sk": c["sk"], "pk": c["pk"], "pk_inf": c["pk_inf"],
                                    "info": info.hex(), "out_len": out_len, "status": int(st[0]), "key": bytes(keys[0]).hex(),
                                    "public_xy": [int(v) for v in xy[0]], "public_inf": int(inf[0])})
    path = os.path.join(HERE, "ecdh_kdf_vectors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0)
    print(len(out["derive_key"]), "derive_key cases,", len(out["exchange"]), "exchange cases,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()

"""
Writes tests/golden/canon_adversarial_vectors.json from tests/canon_adversarial.py with a fixed seed:

    python tests/golden/gen_canon_adversarial.py

Three lists.  "msg": signatures from the message (scheme, curve, pk_len, class, name, msg, sig, pk, want) and, where the
signature is in range and the key decodes, "dm": the double multiplication the verifier does (u1, u2, q and the point
u1 G + u2 q; Ed25519: u1 = S, u2 = h, q = -A; the 65-byte twin of an ECDSA case shares its 33-byte case's).  "hash":
ECDSA after the hash with z free (z, r, s, q and the point u1 G + u2 q for u1 = z / s, u2 = r / s).  "double_mul": u1, u2, q and the point alone.  There a
256-bit integer is 64 hex digits, a point x then y, and the point null for infinity; the tests split them into limbs.
"want_parent" is the verdict of the equation S B + (l - h) A == R that the verifier used to test.
"ossl" is what the `openssl` program on the generating machine answered for an ECDSA or Ed25519 case from the message
(null for BIP-340, which it lacks, after-the-hash cases, and when there is no such program); the generator fails when
OpenSSL contradicts the model outside the classes of OPENSSL_OWN_POLICY.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

import canon_adversarial as A  # noqa: E402
import openssl_cli as O  # noqa: E402

# OpenSSL decodes a point encoding without asking that y < p or that x = 0 comes without the sign bit (RFC 8032 5.1.3 asks both)
OPENSSL_OWN_POLICY = ("non-canonical A",)


def build():
    fix = A.build()
    if O.OPENSSL:
        cli = O.Cli()
        try:
            for c in fix["msg"]:
                if c["scheme"] in ("ecdsa", "ed25519"):
                    c["ossl"] = cli.verify(c["scheme"], c["curve"], bytes.fromhex(c["msg"]), bytes.fromhex(c["sig"]), bytes.fromhex(c["pk"]))
                    assert c["ossl"] == c["want"] or c["class"] in OPENSSL_OWN_POLICY, (c["class"], c["name"], c["want"], c["ossl"])
        finally:
            cli.close()
    return fix


if __name__ == "__main__":
    out = os.path.join(HERE, "canon_adversarial_vectors.json")
    fix = build()
    with open(out, "w") as f:   # one case per line
        f.write('{"note": %s' % json.dumps(fix["note"]))
        for name in ("msg", "hash", "double_mul"):
            f.write(',\n"%s": [\n%s\n]' % (name, ",\n".join(json.dumps(c, sort_keys=True, separators=(",", ":")) for c in fix[name])))
        f.write("}\n")
    print(out, {k: len(v) for k, v in fix.items() if isinstance(v, list)})

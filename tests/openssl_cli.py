"""
The `openssl` command-line program as a second opinion on the model (tests/test_canon_model_vs_openssl.py, and the
"ossl" field that tests/golden/gen_canon_adversarial.py records): subprocess and DER assembled by hand, nothing else.
"""
import os
import shutil
import subprocess
import tempfile

OPENSSL = shutil.which("openssl")
OID_EC_PUBLIC_KEY = bytes.fromhex("06072a8648ce3d0201")
OID_CURVE = {"p256": bytes.fromhex("06082a8648ce3d030107"), "secp256k1": bytes.fromhex("06052b8104000a")}
ED25519_ALGORITHM = bytes.fromhex("300506032b6570")


def der(tag, content):
    n = len(content)
    head = bytes([n]) if n < 128 else bytes([0x80 | ((n.bit_length() + 7) // 8)]) + n.to_bytes((n.bit_length() + 7) // 8, "big")
    return bytes([tag]) + head + content


def der_int(v):
    return der(0x02, v.to_bytes(v.bit_length() // 8 + 1, "big"))


def ec_spki(curve, sec1_point):
    """SubjectPublicKeyInfo of a SEC 1 encoded point (33 or 65 bytes)"""
    return der(0x30, der(0x30, OID_EC_PUBLIC_KEY + OID_CURVE[curve]) + der(0x03, b"\0" + sec1_point))


def ed25519_spki(pk32):
    return der(0x30, ED25519_ALGORITHM + der(0x03, b"\0" + pk32))


def ed25519_pkcs8(seed32):
    return der(0x30, der_int(0) + ED25519_ALGORITHM + der(0x04, der(0x04, seed32)))


def ec_private_key(curve, d32):
    """SEC 1 appendix C.4 ECPrivateKey with the curve's name"""
    return der(0x30, der_int(1) + der(0x04, d32) + der(0xA0, OID_CURVE[curve]))


def ecdsa_sig(sig64):
    return der(0x30, der_int(int.from_bytes(sig64[:32], "big")) + der_int(int.from_bytes(sig64[32:], "big")))


EMPTY_INPUT = b"Could not allocate 0 bytes"   # pkeyutl -rawin of OpenSSL 3.0 on an empty message: the tool's limit, not the library's


class Cli:
    """runs `openssl` on files in a directory of its own"""

    def __init__(self):
        self.dir = tempfile.mkdtemp(prefix="ossl")

    def close(self):
        shutil.rmtree(self.dir, ignore_errors=True)

    def path(self, name, data=None):
        p = os.path.join(self.dir, name)
        if data is not None:
            with open(p, "wb") as f:
                f.write(data)
        return p

    def run(self, *args):
        return subprocess.run([OPENSSL] + list(args), capture_output=True)

    def ecdsa_verify(self, curve, msg, sig64, sec1_point):
        """1 / 0: SHA-256 ECDSA; a key that OpenSSL does not load counts as refused"""
        out = self.run("dgst", "-sha256", "-verify", self.path("pk", ec_spki(curve, sec1_point)), "-keyform", "DER",
                       "-signature", self.path("sig", ecdsa_sig(sig64)), self.path("msg", msg))
        return 1 if out.returncode == 0 and b"Verified OK" in out.stdout else 0

    def ed25519_verify(self, msg, sig64, pk32):
        """1 / 0, or None where the program cannot take the (empty) message at all"""
        out = self.run("pkeyutl", "-verify", "-pubin", "-inkey", self.path("pk", ed25519_spki(pk32)), "-keyform", "DER", "-rawin",
                       "-in", self.path("msg", msg), "-sigfile", self.path("sig", sig64))
        if not msg and EMPTY_INPUT in out.stderr:
            return None
        return 1 if out.returncode == 0 and b"Signature Verified Successfully" in out.stdout else 0

    def ed25519_sign(self, seed32, msg):
        out = self.run("pkeyutl", "-sign", "-inkey", self.path("sk", ed25519_pkcs8(seed32)), "-keyform", "DER", "-rawin",
                       "-in", self.path("msg", msg), "-out", self.path("sig"))
        if not msg and EMPTY_INPUT in out.stderr:
            return None
        assert out.returncode == 0, out.stderr
        return open(self.path("sig"), "rb").read()

    def public_key(self, private_der):
        """the SubjectPublicKeyInfo OpenSSL derives from a private key"""
        out = self.run("pkey", "-inform", "DER", "-in", self.path("sk", private_der), "-pubout", "-outform", "DER")
        assert out.returncode == 0, out.stderr
        return out.stdout

    def ecdh_x(self, curve, d32, sec1_point):
        out = self.run("pkeyutl", "-derive", "-inkey", self.path("sk", ec_private_key(curve, d32)), "-keyform", "DER",
                       "-peerkey", self.path("pk", ec_spki(curve, sec1_point)), "-peerform", "DER")
        assert out.returncode == 0, out.stderr
        return out.stdout

    def verify(self, scheme, curve, msg, sig, pk):
        return self.ecdsa_verify(curve, msg, sig, pk) if scheme == "ecdsa" else self.ed25519_verify(msg, sig, pk)

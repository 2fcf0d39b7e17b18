"""
CPU checks of the batch-verification model (tests/canon_batch_ref.py) and of its fixture (tests/golden/canon_batch_vectors.json):
the coefficient's known answers, the model's verdict against the per-signature model, the cancelling pair that only the
coefficients catch, and the Ed25519 torsion cases that only the cofactored equation accepts.
"""
import hashlib
import struct

import canon_adversarial as ADV
import canon_batch_ref as B
import canon_msg_ref as R
import gen_canon_batch as G

FX = B.load_fixture()
SEED = bytes(range(32))


def test_the_fixture_is_what_the_generator_writes():
    assert G.build() == FX.doc


def test_the_fixture_covers_the_block_edges():
    for scheme in B.SCHEMES:
        rows = FX.triples(scheme)
        assert len(rows) == 80
        assert sorted({len(m) for m, _, _ in rows}) == sorted(B.MSG_LENGTHS)
        assert all(B.single(scheme, *row) == 1 for row in rows[:16])


def test_coefficient_known_answers():
    """the definition, spelt out: the tag hash twice, the seed, the index as eight little-endian bytes"""
    t = hashlib.sha256(b"fecgpu/batch-coefficient").digest()
    assert t.hex() == "f86bbbbb0c6022bea19afef7e8e28fc8f89a06b7ea74122a15e40827b7419459"
    for i, le in ((0, bytes(8)), (2**32 + 1, bytes([1, 0, 0, 0, 1, 0, 0, 0]))):
        d = hashlib.sha256(t + t + SEED + le).digest()
        assert B.coefficient(SEED, i) == int(d[:16].hex(), 16) != 0
        assert struct.pack("<Q", i) == le
    assert B.coefficient(SEED, 0) == 0x9b51619cf6e9036c696c896ab017b3ab
    assert B.coefficient(SEED, 2**32 + 1) == 0xc5abea5d81ab0f07e9e1c02dc0f5d204
    assert B.coefficient(SEED, 0) != B.coefficient(SEED, 1) != B.coefficient(SEED, 2**32 + 1)
    assert B.coefficient(SEED, 0) != B.coefficient(bytes(32), 0)


def test_the_midstate_is_the_state_after_the_tag_block():
    """one more compression from the midstate gives hashlib's digest"""
    mid = B.tag_midstate()
    assert ["%08x" % v for v in mid] == ["d5369972", "dfc3fb5d", "72673496", "495c809e", "eaecdd36", "bb5e980e", "bba65ef9", "0e5dc54c"]
    t = hashlib.sha256(B.TAG).digest()
    for i in (0, 1, 2**32 + 1, 2**64 - 1):
        block = SEED + struct.pack("<Q", i) + b"\x80" + bytes(15) + struct.pack(">Q", 104 * 8)
        digest = b"".join(struct.pack(">I", v) for v in B.sha256_compress(mid, block))
        assert digest == hashlib.sha256(t + t + SEED + struct.pack("<Q", i)).digest()


def test_a_zero_coefficient_becomes_one():
    """no seed whose digest starts with 16 zero bytes turns up in a bounded search (2^-128 each), so the rule is tested on the
    function that applies it"""
    found = [c for c in range(4096) if hashlib.sha256(struct.pack("<I", c)).digest()[:16] == bytes(16)]
    assert not found
    assert B.coefficient_from_digest(bytes(16) + b"\xff" * 16) == 1
    assert B.coefficient_from_digest(bytes(15) + b"\x02" + bytes(16)) == 2
    assert B.coefficient_from_digest(b"\x80" + bytes(31)) == 2**127


def test_verdict_equals_every_signature_valid():
    for scheme in B.SCHEMES:
        rows = FX.triples(scheme)[:24]
        msgs, sigs, pks = [list(v) for v in zip(*rows)]
        assert B.batch(scheme, msgs, sigs, pks, SEED) == (True, [0] * 24, 1)
        for at, part in ((0, "sig"), (11, "msg"), (23, "pk")):
            m, s, p = list(msgs), list(sigs), list(pks)
            if part == "sig":
                s[at] = s[at][:40] + bytes([s[at][40] ^ 4]) + s[at][41:]
            elif part == "msg":
                m[at] = m[at] + b"!"
            else:
                p[at] = pks[(at + 1) % 24] if pks[(at + 1) % 24] != pks[at] else pks[(at + 2) % 24]
            each = [B.single(scheme, *row) for row in zip(m, s, p)]
            ok, status, verdict = B.batch(scheme, m, s, p, SEED)
            assert each.count(0) == 1 and ok == all(each) and not ok and verdict == 0 and status == [0] * 24, (scheme, part)


def test_refused_elements_leave_the_verdict_to_the_rest():
    for scheme in B.SCHEMES:
        msgs, sigs, pks = FX.tiled(scheme, 6)
        for name, msg, sig, pk, status in FX.refused(scheme):
            ok, st, verdict = B.batch(scheme, msgs[:3] + [msg] + msgs[3:], sigs[:3] + [sig] + sigs[3:], pks[:3] + [pk] + pks[3:], SEED)
            assert (ok, st, verdict) == (False, [0, 0, 0, status, 0, 0, 0], 1), (scheme, name)
            assert B.single(scheme, msg, sig, pk) == 0


def test_the_cancelling_pair_is_caught_by_the_coefficients_alone():
    for scheme in B.SCHEMES:
        msgs, sigs, pks = FX.tiled(scheme, 5)
        sigs[1], sigs[3] = B.cancelling_pair(scheme, sigs[1], sigs[3], 0x1234567)
        assert [B.single(scheme, *row) for row in zip(msgs, sigs, pks)] == [1, 0, 1, 0, 1]
        assert B.batch(scheme, msgs, sigs, pks, SEED, coeff=B.ones) == (True, [0] * 5, 1)   # the sum without coefficients accepts
        for k in range(2):
            assert B.batch(scheme, msgs, sigs, pks, B.fixed_seed(k)) == (False, [0] * 5, 0)


def test_torsion_defects_pass_the_cofactored_equation_only():
    assert sorted(name for name, *_ in FX.torsion()) == sorted("%s + T of order %d" % (w, o) for w in "RA" for o in (2, 4, 8))
    msgs, sigs, pks = FX.tiled("ed25519", 2)
    for name, msg, sig, pk in FX.torsion():
        assert R.ed25519_verify(msg, sig, pk) == 0, name
        A, Rp = R.ed_decode(pk), R.ed_decode(sig[:32])
        h, S = R.ed25519_challenge(sig[:32], pk, msg), int.from_bytes(sig[32:], "little")
        defect = ADV.E.add(ADV.E.mul(S, ADV.E.G), ADV.E.neg(ADV.E.add(ADV.E.mul(h, A), Rp)))
        assert defect != ADV.E.IDENTITY and ADV.order_of(defect) == int(name.split()[-1]), name
        seed = B.seed_with_odd(name, [1])
        m, s, p = [msgs[0], msg, msgs[1]], [sigs[0], sig, sigs[1]], [pks[0], pk, pks[1]]
        assert B.batch("ed25519", m, s, p, seed) == (True, [0, 0, 0], 1), name
        assert B.batch("ed25519", m, s, p, seed, cofactor=1) == (False, [0, 0, 0], 0), name   # a cofactorless sum refuses it for certain

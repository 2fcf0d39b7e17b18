"""
The Python mirror of schnorr::batch_verify maps the C result byte to its verdict without a GPU: a stub library stands
in for libfecgpu.so and writes the result.  fec_schnorr_batch_verify writes 2 for Ed25519 when the reference panics in
to_affine (k_schnorr_fold_compare); that is not a verified batch, so the boolean forms must not report True.
"""
import ctypes

import numpy as np
import pytest

import forge_ec_amd as F


class _StubLib:
    """Each entry point stores `result` at the result pointer and the given sides, then returns FEC_OK."""

    def __init__(self, result):
        self.result = result
        self.calls = []

    def _write(self, name, res_ptr, sides_ptr, sinf_ptr, dbg_ptr=None):
        self.calls.append(name)
        ctypes.c_uint8.from_address(res_ptr.value).value = self.result
        (ctypes.c_uint64 * 16).from_address(sides_ptr.value)[:] = list(range(1, 17))
        (ctypes.c_uint8 * 2).from_address(sinf_ptr.value)[:] = [0, 0]
        if dbg_ptr is not None:
            ctypes.c_uint8.from_address(dbg_ptr.value).value = 0
        return 0

    def fec_schnorr_batch_verify(self, h, curve, pk, pi, r, ri, s, a, e, n, res, sides, sinf):
        return self._write("fec_schnorr_batch_verify", res, sides, sinf)

    def fec_schnorr_batch_verify_secp256k1(self, h, pk, pi, r, ri, s, a, e, n, res, sides, sinf):
        return self._write("fec_schnorr_batch_verify_secp256k1", res, sides, sinf)

    def fec_schnorr_batch_verify_ed25519(self, h, pk, pi, r, ri, s, a, e, n, res, sides, sinf, dbg):
        return self._write("fec_schnorr_batch_verify_ed25519", res, sides, sinf, dbg)


def _stub_ctx(result):
    ctx = F.Context.__new__(F.Context)   # no fec_ctx: the stub is the whole library
    ctx._lib = _StubLib(result)
    ctx._h = None
    ctx.device = 0
    return ctx


def _inputs(n=3):
    pt = np.ones((n, 8), dtype=np.uint64)
    sc = np.ones((n, 4), dtype=np.uint64)
    return pt, pt.copy(), sc, sc.copy(), sc.copy()


@pytest.mark.parametrize("result, verdict", [(0, False), (1, True), (2, False)])
def test_generic_schnorr_batch_verify_mirror_is_true_only_for_1(result, verdict):
    ctx = _stub_ctx(result)
    got, sides, sinf = ctx.schnorr_batch_verify(F.ED25519, *_inputs())
    assert ctx._lib.calls == ["fec_schnorr_batch_verify"]
    assert got is verdict
    assert [int(v) for v in sides] == list(range(1, 17)) and list(sinf) == [0, 0]


@pytest.mark.parametrize("result, verdict", [(0, False), (1, True), (2, False)])
def test_secp256k1_schnorr_batch_verify_mirror_is_true_only_for_1(result, verdict):
    ctx = _stub_ctx(result)
    got, _, _ = ctx.schnorr_batch_verify_secp256k1(*_inputs())
    assert ctx._lib.calls == ["fec_schnorr_batch_verify_secp256k1"]
    assert got is verdict


def test_ed25519_schnorr_batch_verify_mirror_keeps_the_tri_state():
    ctx = _stub_ctx(2)
    res, _, _, dbg = ctx.schnorr_batch_verify_ed25519(*_inputs())
    assert ctx._lib.calls == ["fec_schnorr_batch_verify_ed25519"]
    assert res == 2 and dbg is False

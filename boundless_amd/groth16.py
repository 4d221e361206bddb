"""Python mirror of include/bx_groth16.h: the BN254 Groth16 prover (snarkjs / rapidsnark conventions) and its MSMs.

    key = Groth16Key(hal, "circuit.zkey")      # or the zkey's bytes; parsed, uploaded and checked once
    proof = key.prove(witness)                 # witness: ints, or n_vars x 32 bytes little-endian (what a .wtns holds)
    proof.to_json(), proof.seal(selector)      # snarkjs proof JSON; the 260-byte on-chain seal
    verify(key.vk(), proof)                    # the library's host verifier: returns, or raises HalError naming the failed check
    verify_seal(VerifyingKey.from_json(text), seal, claim_digest)

A thin ctypes binding: the proving arithmetic runs in the library's HIP kernels, and there is no CPU fallback.  Verification
(VerifyingKey, verify, verify_seal, pairing_check, Proof.from_seal / from_json) is host C++ in the same library and needs no GPU.
"""
import ctypes as C
import struct

import numpy as np

from .hal import BxBuf, HalError, load_library

Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
MAX_PUBLIC = 64


class Info(C.Structure):
    _fields_ = [("n_vars", C.c_uint32), ("n_public", C.c_uint32), ("domain_size", C.c_uint32), ("n_coefs", C.c_uint64), ("bytes", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class _Proof(C.Structure):
    _fields_ = [("a", C.c_uint32 * 16), ("b", C.c_uint32 * 32), ("c", C.c_uint32 * 16), ("n_public", C.c_uint32),
                ("public_signals", C.c_uint32 * (MAX_PUBLIC * 8))]


class _Vk(C.Structure):
    _fields_ = [("alpha1", C.c_uint32 * 16), ("beta2", C.c_uint32 * 32), ("gamma2", C.c_uint32 * 32), ("delta2", C.c_uint32 * 32),
                ("n_public", C.c_uint32), ("ic", C.c_uint32 * ((MAX_PUBLIC + 1) * 16))]


_declared = False


def _lib():
    global _declared
    L = load_library()
    if not _declared:
        vp, sz, cp, u32p = C.c_void_p, C.c_size_t, C.c_char_p, C.POINTER(C.c_uint32)
        sigs = {
            "bx_groth16_zkey_inspect": [cp, C.POINTER(Info)],
            "bx_groth16_zkey_inspect_mem": [vp, sz, C.POINTER(Info)],
            "bx_groth16_key_load": [vp, cp, C.POINTER(vp)],
            "bx_groth16_key_load_mem": [vp, vp, sz, C.POINTER(vp)],
            "bx_groth16_key_info": [vp, C.POINTER(Info)],
            "bx_groth16_key_free": [vp, vp],
            "bx_groth16_prove": [vp, vp, vp, sz, vp, C.POINTER(_Proof)],
            "bx_groth16_proof_json": [C.POINTER(_Proof), C.c_char_p, sz],
            "bx_groth16_public_json": [C.POINTER(_Proof), C.c_char_p, sz],
            "bx_groth16_zkey_vk": [cp, C.POINTER(_Vk)],
            "bx_groth16_zkey_vk_mem": [vp, sz, C.POINTER(_Vk)],
            "bx_groth16_key_vk": [vp, C.POINTER(_Vk)],
            "bx_groth16_vk_json": [C.POINTER(_Vk), C.c_char_p, sz],
            "bx_groth16_vk_from_json": [cp, sz, C.POINTER(_Vk)],
            "bx_groth16_proof_from_json": [cp, sz, cp, sz, C.POINTER(_Proof)],
            "bx_groth16_seal_encode": [C.POINTER(_Proof), cp, C.c_char_p],
            "bx_groth16_seal_decode": [cp, sz, C.POINTER(_Proof)],
            "bx_groth16_verify": [C.POINTER(_Vk), C.POINTER(_Proof)],
            "bx_groth16_verify_seal": [C.POINTER(_Vk), cp, sz, cp],
            "bx_bn254_pairing_check": [u32p, u32p, sz],
            "bx_bn254_msm_g1": [vp, BxBuf, BxBuf, sz, u32p],
            "bx_bn254_msm_g2": [vp, BxBuf, BxBuf, sz, u32p],
        }
        for name, args in sigs.items():
            fn = getattr(L, name)
            fn.argtypes = args
            fn.restype = cp
        _declared = True
    return L


def _check(msg):
    if msg:
        raise HalError(msg.decode())


def _int(words):
    return int.from_bytes(np.asarray(words, dtype="<u4").tobytes(), "little")


def _words(x, n=8):
    return np.frombuffer(int(x).to_bytes(4 * n, "little"), dtype="<u4")


def inspect(src):
    """bx_groth16_zkey_inspect: header facts of a zkey (path or bytes), host only.  Raises HalError for a malformed key."""
    L, info = _lib(), Info()
    if isinstance(src, (bytes, bytearray, memoryview)):
        b = bytes(src)
        _check(L.bx_groth16_zkey_inspect_mem(b, len(b), C.byref(info)))
    else:
        _check(L.bx_groth16_zkey_inspect(str(src).encode(), C.byref(info)))
    return info.as_dict()


def read_wtns(path_or_bytes):
    """the values of a snarkjs .wtns file ("wtns", version, sections; 1: n8, prime, count; 2: values) as ints"""
    b = path_or_bytes if isinstance(path_or_bytes, (bytes, bytearray)) else open(path_or_bytes, "rb").read()
    if b[:4] != b"wtns":
        raise ValueError("not a wtns file")
    _ver, nsec = struct.unpack_from("<II", b, 4)
    at, secs = 12, {}
    for _ in range(nsec):
        t, size = struct.unpack_from("<IQ", b, at)
        secs[t] = b[at + 12:at + 12 + size]
        at += 12 + size
    n8, = struct.unpack_from("<I", secs[1], 0)
    prime = int.from_bytes(secs[1][4:4 + n8], "little")
    count, = struct.unpack_from("<I", secs[1], 4 + n8)
    if prime != R:
        raise ValueError("wtns prime is not BN254's r")
    return [int.from_bytes(secs[2][i * n8:(i + 1) * n8], "little") for i in range(count)]


def witness_bytes(witness):
    if isinstance(witness, (bytes, bytearray)):
        return bytes(witness)
    return b"".join(int(x).to_bytes(32, "little") for x in witness)


class Proof:
    """A (G1), B (G2, ((x.c0, x.c1), (y.c0, y.c1))), C (G1) as integer affine coordinates (None = infinity), public signals."""

    def __init__(self, raw):
        self._raw = raw
        aff = lambda w: (_int(w[0:8]), _int(w[8:16]))
        nz = lambda p: None if p == (0, 0) else p
        self.a = nz(aff(raw.a))
        x, y = ((_int(raw.b[0:8]), _int(raw.b[8:16])), (_int(raw.b[16:24]), _int(raw.b[24:32])))
        self.b = None if x == (0, 0) and y == (0, 0) else (x, y)
        self.c = nz(aff(raw.c))
        self.public = [_int(raw.public_signals[8 * i:8 * i + 8]) for i in range(raw.n_public)]

    def as_tuple(self):
        return self.a, self.b, self.c

    @classmethod
    def from_seal(cls, seal, public=()):
        """bx_groth16_seal_decode: a 260-byte seal (or 256 without its selector) back to a proof; the seal carries no public signals,
        so they are re-attached here"""
        raw, b = _Proof(), bytes(seal)
        _check(_lib().bx_groth16_seal_decode(b, len(b), C.byref(raw)))
        return cls(raw).with_public(public)

    @classmethod
    def from_json(cls, proof_json, public_json=None):
        """bx_groth16_proof_from_json: what to_json() and public_json() write"""
        raw = _Proof()
        pj = proof_json.encode() if isinstance(proof_json, str) else bytes(proof_json)
        uj = None if public_json is None else (public_json.encode() if isinstance(public_json, str) else bytes(public_json))
        _check(_lib().bx_groth16_proof_from_json(pj, len(pj), uj, 0 if uj is None else len(uj), C.byref(raw)))
        return cls(raw)

    def with_public(self, public):
        """the same A, B, C with other public signals (ints below 2^256; verification refuses those not below r)"""
        public = [int(x) for x in public]
        if len(public) > MAX_PUBLIC:
            raise ValueError("more public signals than BX_GROTH16_MAX_PUBLIC")
        raw = _Proof.from_buffer_copy(self._raw)
        C.memset(raw.public_signals, 0, C.sizeof(raw.public_signals))
        for i, x in enumerate(public):
            raw.public_signals[8 * i:8 * i + 8] = [int(w) for w in _words(x)]
        raw.n_public = len(public)
        return Proof(raw)

    def to_json(self):
        buf = C.create_string_buffer(2048)
        _check(_lib().bx_groth16_proof_json(C.byref(self._raw), buf, len(buf)))
        return buf.value.decode()

    def public_json(self):
        buf = C.create_string_buffer(100 * (MAX_PUBLIC + 1))
        _check(_lib().bx_groth16_public_json(C.byref(self._raw), buf, len(buf)))
        return buf.value.decode()

    def seal(self, selector):
        """the on-chain seal: 4-byte selector, A.x, A.y, B.x.c1, B.x.c0, B.y.c1, B.y.c0, C.x, C.y (32-byte big-endian each)"""
        sel = bytes(selector)
        if len(sel) != 4:
            raise ValueError("selector must be 4 bytes")
        out = C.create_string_buffer(260)
        _check(_lib().bx_groth16_seal_encode(C.byref(self._raw), sel, out))
        return out.raw


def _g1(w):
    p = (_int(w[0:8]), _int(w[8:16]))
    return None if p == (0, 0) else p


def _g2(w):
    x, y = (_int(w[0:8]), _int(w[8:16])), (_int(w[16:24]), _int(w[24:32]))
    return None if x == (0, 0) and y == (0, 0) else (x, y)


class VerifyingKey:
    """bx_groth16_vk: alpha1 (G1), beta2, gamma2, delta2 (G2) and IC_0 .. IC_n_public (G1) as integer affine coordinates.  Every
    constructor goes through the library, which checks ranges, curves and the G2 subgroup and raises HalError otherwise."""

    def __init__(self, raw):
        self._raw = raw
        self.n_public = int(raw.n_public)
        self.alpha1, self.beta2, self.gamma2, self.delta2 = _g1(raw.alpha1), _g2(raw.beta2), _g2(raw.gamma2), _g2(raw.delta2)
        self.ic = [_g1(raw.ic[16 * i:16 * i + 16]) for i in range(self.n_public + 1)]

    @classmethod
    def from_zkey(cls, src):
        """the verifying key a zkey carries (path or bytes): bx_groth16_zkey_vk(_mem)"""
        L, raw = _lib(), _Vk()
        if isinstance(src, (bytes, bytearray, memoryview)):
            b = bytes(src)
            _check(L.bx_groth16_zkey_vk_mem(b, len(b), C.byref(raw)))
        else:
            _check(L.bx_groth16_zkey_vk(str(src).encode(), C.byref(raw)))
        return cls(raw)

    @classmethod
    def from_json(cls, text):
        """snarkjs verification_key.json: bx_groth16_vk_from_json"""
        raw = _Vk()
        b = text.encode() if isinstance(text, str) else bytes(text)
        _check(_lib().bx_groth16_vk_from_json(b, len(b), C.byref(raw)))
        return cls(raw)

    def to_json(self):
        buf = C.create_string_buffer(1024 + 200 * (MAX_PUBLIC + 1))
        _check(_lib().bx_groth16_vk_json(C.byref(self._raw), buf, len(buf)))
        return buf.value.decode()

    def as_dict(self):
        return {"alpha1": self.alpha1, "beta2": self.beta2, "gamma2": self.gamma2, "delta2": self.delta2, "ic": list(self.ic)}

    def __eq__(self, other):
        return isinstance(other, VerifyingKey) and self.as_dict() == other.as_dict()


def verify(vk, proof):
    """bx_groth16_verify: returns None when the proof is accepted, raises HalError with the library's message (the failed check by
    name, or "pairing check failed") otherwise"""
    _check(_lib().bx_groth16_verify(C.byref(vk._raw), C.byref(proof._raw)))


def verify_seal(vk, seal, claim_digest):
    """bx_groth16_verify_seal: the reference's verify_seal — one public input, the 32-byte claim digest as a big-endian number mod r"""
    s, d = bytes(seal), bytes(claim_digest)
    if len(d) != 32:
        raise ValueError("claim digest must be 32 bytes")
    _check(_lib().bx_groth16_verify_seal(C.byref(vk._raw), s, len(s), d))


def pairing_check(g1s, g2s):
    """bx_bn254_pairing_check: prod e(g1s[i], g2s[i]) == 1 for integer affine points (None = infinity).  True / False; a malformed
    point (off its curve, outside the subgroup, a coordinate not below q) raises HalError"""
    if len(g1s) != len(g2s):
        raise ValueError("as many G1 as G2 points")
    a, b = np.zeros((len(g1s), 16), np.uint32), np.zeros((len(g2s), 32), np.uint32)
    for i, p in enumerate(g1s):
        if p is not None:
            a[i, :8], a[i, 8:] = _words(p[0], 8), _words(p[1], 8)
    for i, p in enumerate(g2s):
        if p is not None:
            for j, v in enumerate((p[0][0], p[0][1], p[1][0], p[1][1])):
                b[i, 8 * j:8 * j + 8] = _words(v, 8)
    u32p = C.POINTER(C.c_uint32)
    msg = _lib().bx_bn254_pairing_check(a.ctypes.data_as(u32p), b.ctypes.data_as(u32p), len(g1s))
    if msg and msg.decode().endswith("pairing check failed"):
        return False
    _check(msg)
    return True


class Groth16Key:
    """bx_groth16_key_load(_mem): a proving key on one HipHal's ctx.  .info holds n_vars, n_public, domain_size, n_coefs, bytes."""

    def __init__(self, hal, src):
        self.hal, self.L = hal, _lib()
        k = C.c_void_p()
        if isinstance(src, (bytes, bytearray, memoryview)):
            b = bytes(src)
            _check(self.L.bx_groth16_key_load_mem(hal.ctx, b, len(b), C.byref(k)))
        else:
            _check(self.L.bx_groth16_key_load(hal.ctx, str(src).encode(), C.byref(k)))
        self.key = k
        info = Info()
        _check(self.L.bx_groth16_key_info(k, C.byref(info)))
        self.info = info.as_dict()

    def prove(self, witness, r=None, s=None):
        w = witness_bytes(witness)
        rs = None if r is None and s is None else int(r).to_bytes(32, "little") + int(s).to_bytes(32, "little")
        raw = _Proof()
        _check(self.L.bx_groth16_prove(self.hal.ctx, self.key, w, len(w) // 32, rs, C.byref(raw)))
        return Proof(raw)

    def vk(self):
        """bx_groth16_key_vk: the verifying key of this proving key, from what the load kept on the host (no device access)"""
        raw = _Vk()
        _check(self.L.bx_groth16_key_vk(self.key, C.byref(raw)))
        return VerifyingKey(raw)

    def free(self):
        """bx_groth16_key_free; after hal.close() there is nothing left to free (bx_free released the ctx's keys)"""
        if getattr(self, "key", None):
            key, self.key = self.key, None
            if self.hal.ctx:
                _check(self.L.bx_groth16_key_free(self.hal.ctx, key))

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def g1_words(points):
    """affine int points (None = infinity) -> device layout: Montgomery x, y little-endian, 16 words each"""
    out = np.zeros((len(points), 16), np.uint32)
    for i, p in enumerate(points):
        if p is not None:
            out[i, :8], out[i, 8:] = _words(p[0] * (1 << 256) % Q), _words(p[1] * (1 << 256) % Q)
    return out.ravel()


def g2_words(points):
    out = np.zeros((len(points), 32), np.uint32)
    for i, p in enumerate(points):
        if p is not None:
            for j, v in enumerate((p[0][0], p[0][1], p[1][0], p[1][1])):
                out[i, 8 * j:8 * j + 8] = _words(v * (1 << 256) % Q)
    return out.ravel()


def scalar_words(scalars):
    return np.frombuffer(b"".join(int(k).to_bytes(32, "little") for k in scalars), dtype="<u4").copy()


def _msm(hal, fn, pts_buf, sc_buf, n, words):
    out = np.zeros(words, np.uint32)
    _check(fn(hal.ctx, pts_buf.raw, sc_buf.raw, n, out.ctypes.data_as(C.POINTER(C.c_uint32))))
    return out


def msm_g1(hal, points, scalars, n=None):
    """sum k_i P_i over G1.  points / scalars: device Buffers in the layout of bx_bn254_msm_g1, or Python lists (uploaded here).
    Returns (x, y) ints or None for infinity."""
    pb = points if hasattr(points, "raw") else hal.copy_from(g1_words(points))
    sb = scalars if hasattr(scalars, "raw") else hal.copy_from(scalar_words(scalars))
    n = pb.size() // 16 if n is None else n
    o = _msm(hal, _lib().bx_bn254_msm_g1, pb, sb, n, 16)
    p = (_int(o[:8]), _int(o[8:]))
    return None if p == (0, 0) else p


def msm_g2(hal, points, scalars, n=None):
    pb = points if hasattr(points, "raw") else hal.copy_from(g2_words(points))
    sb = scalars if hasattr(scalars, "raw") else hal.copy_from(scalar_words(scalars))
    n = pb.size() // 32 if n is None else n
    o = _msm(hal, _lib().bx_bn254_msm_g2, pb, sb, n, 32)
    x, y = (_int(o[0:8]), _int(o[8:16])), (_int(o[16:24]), _int(o[24:32]))
    return None if x == (0, 0) and y == (0, 0) else (x, y)


__all__ = ["Groth16Key", "Proof", "VerifyingKey", "verify", "verify_seal", "pairing_check", "inspect", "read_wtns", "msm_g1", "msm_g2", "g1_words", "g2_words", "scalar_words", "Q", "R"]

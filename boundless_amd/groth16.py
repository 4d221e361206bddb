"""Python mirror of include/bx_groth16.h: the BN254 Groth16 prover (snarkjs / rapidsnark conventions) and its MSMs.

    key = Groth16Key(hal, "circuit.zkey")      # or the zkey's bytes; parsed, uploaded and checked once
    proof = key.prove(witness)                 # witness: ints, or n_vars x 32 bytes little-endian (what a .wtns holds)
    proof.to_json(), proof.seal(selector)      # snarkjs proof JSON; the 260-byte on-chain seal

A thin ctypes binding: the arithmetic runs in the library's HIP kernels, and there is no CPU fallback.
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
        a, b, c = self.a or (0, 0), self.b or ((0, 0), (0, 0)), self.c or (0, 0)
        nums = [a[0], a[1], b[0][1], b[0][0], b[1][1], b[1][0], c[0], c[1]]
        return sel + b"".join(x.to_bytes(32, "big") for x in nums)


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


__all__ = ["Groth16Key", "Proof", "inspect", "read_wtns", "msm_g1", "msm_g2", "g1_words", "g2_words", "scalar_words", "Q", "R"]

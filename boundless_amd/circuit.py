"""ctypes mirror of include/bx_circuit.h: the circuit half of the segment prover as a plug-in table.

Reference: below `ProverServer::prove_segment` (bento/crates/workflow/src/tasks/prove.rs:41-49) the prover reaches
`risc0_zkp::hal::CircuitHal` (eval_check, accumulate) and the circuit crate's witness generation; `bx_circuit_ops` is that
boundary as a C table.  `CircuitOps.from_object` adapts a Python object with the same method names (used by the tests to plug a
circuit written outside the library into bx_prove_segment / bx_verify_segment); production circuits are native tables.
"""
import ctypes as C

from .hal import BxBuf, load_library
from .prover import SegmentParams


MAX_TAPS = 8  # BX_MAX_TAPS (include/bx_circuit.h)


class TapReader(C.Structure):
    pass


_TAP_AT = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_int, C.c_uint32, C.c_int, C.POINTER(C.c_uint32))
TapReader._fields_ = [("ctx", C.c_void_p), ("at", _TAP_AT)]

_NORMALIZE = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.POINTER(SegmentParams))
_TAPS = C.CFUNCTYPE(C.c_uint32, C.c_void_p, C.POINTER(SegmentParams), C.c_int, C.c_uint32, C.POINTER(C.c_uint32))
_NGLOBALS = C.CFUNCTYPE(C.c_uint32, C.c_void_p, C.POINTER(SegmentParams))
_CREATE = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(SegmentParams), C.POINTER(C.c_void_p))
_DESTROY = C.CFUNCTYPE(None, C.c_void_p, C.c_void_p)
_CODE = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, BxBuf)
_WITGEN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, BxBuf, BxBuf, C.POINTER(C.c_uint8), C.c_size_t, BxBuf, C.POINTER(C.c_uint32))
_ACCUM = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, BxBuf, C.POINTER(C.c_uint32))
_CHECK_CODE = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.POINTER(SegmentParams), C.POINTER(C.c_uint32))
_EVAL = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, BxBuf, BxBuf, BxBuf, BxBuf, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                    C.POINTER(C.c_uint32))
_CONS = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.POINTER(SegmentParams), C.POINTER(TapReader), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32),
                    C.POINTER(C.c_uint32), C.POINTER(C.c_uint32))


class CircuitOps(C.Structure):
    _fields_ = [("user", C.c_void_p), ("name", C.c_char_p), ("normalize", _NORMALIZE), ("taps", _TAPS), ("n_globals", _NGLOBALS), ("create", _CREATE),
                ("destroy", _DESTROY), ("code_group", _CODE), ("witgen", _WITGEN), ("accumulate", _ACCUM), ("eval_check", _EVAL),
                ("constraints_at", _CONS),
                ("set_noise_seed", C.c_void_p),  # optional (include/bx_circuit.h); NULL for circuits written in Python
                ("check_code", _CHECK_CODE)]

    @staticmethod
    def from_object(obj, name=b"python-circuit"):
        """obj provides normalize(shape), taps(shape, group, col) -> list of rows back (first 0), n_globals(shape),
        code_group(ctx, code) (fills the public code group: a function of the shape alone),
        witgen(ctx, code, data, segment_bytes, segment_dev) -> list of the n_globals public words, accumulate(ctx, accum, mix),
        optionally check_code(shape, root_words) (raise to refuse a code root; without it seals of this circuit verify only
        against an explicit VerifierContext),
        eval_check(ctx, check, code_eval, data_eval, accum_eval, poly_mix, mix, globals) and
        constraints_at(shape, tap, poly_mix, mix, globals) -> 4 words; ctx is the raw bx_ctx pointer, buffers are BxBuf, mixes are lists of 4 Montgomery words, tap(group, col, back)
        returns 4 Montgomery words.  Exceptions become the error string of the call."""
        errs = []

        def guard(fn):
            def wrapped(*a):
                try:
                    fn(*a)
                    return None
                except Exception as e:  # noqa: BLE001 - crosses the ABI as a string
                    errs.append(C.create_string_buffer(f"{type(e).__name__}: {e}".encode()))
                    return C.cast(errs[-1], C.c_void_p).value
            return wrapped

        def w4(p):
            return [p[i] for i in range(4)]

        n_glob = {}

        def n_globals(_u, shape):
            n_glob["n"] = int(obj.n_globals(shape.contents)) if hasattr(obj, "n_globals") else 0
            return n_glob["n"]

        def witgen(_u, _s, ctx, code, data, seg, seg_len, seg_dev, globals_out):
            g = list(obj.witgen(ctx, code, data, C.string_at(seg, seg_len), seg_dev) or [])
            # the C side hands over an array of n_globals words: more would be written past it before any check could run
            if len(g) > n_glob.get("n", 0):
                raise ValueError(f"witgen returned {len(g)} public words, the circuit declared {n_glob.get('n', 0)}")
            for i, v in enumerate(g):
                globals_out[i] = int(v)

        def glist(p):
            return [p[i] for i in range(n_glob.get("n", 0))]

        def constraints_at(_u, shape, reader, poly_mix, mix, globals_, out):
            def tap(group, col, back):
                buf = (C.c_uint32 * 4)()
                msg = reader.contents.at(reader.contents.ctx, group, col, back, buf)
                if msg:
                    raise RuntimeError(C.cast(msg, C.c_char_p).value.decode())
                return list(buf)

            r = obj.constraints_at(shape.contents, tap, w4(poly_mix), w4(mix), glist(globals_))
            for i in range(4):
                out[i] = int(r[i])

        def taps(_u, shape, g, c, out):
            backs = list(obj.taps(shape.contents, g, c))  # e.g. [0] or [0, 1, 3]: the rows back the column is opened at
            # `out` is a BX_MAX_TAPS-word array on the caller's stack: report an oversized set by its length (the C side refuses
            # k > BX_MAX_TAPS) without writing past the array
            for i, b in enumerate(backs[:MAX_TAPS]):
                out[i] = int(b)
            return len(backs)

        ops = CircuitOps(None, name,
                         _NORMALIZE(guard(lambda _u, shape: obj.normalize(shape.contents))),
                         _TAPS(taps), _NGLOBALS(n_globals),
                         _CREATE(), _DESTROY(),
                         _CODE(guard(lambda _u, _s, ctx, code: obj.code_group(ctx, code))),
                         _WITGEN(guard(witgen)),
                         _ACCUM(guard(lambda _u, _s, ctx, accum, mix: obj.accumulate(ctx, accum, w4(mix)))),
                         _EVAL(guard(lambda _u, _s, ctx, check, ce, de, ae, pm, mix, gl: obj.eval_check(ctx, check, ce, de, ae, w4(pm), w4(mix), glist(gl)))),
                         _CONS(guard(constraints_at)), None,
                         _CHECK_CODE(guard(lambda _u, shape, root: obj.check_code(shape.contents, [root[i] for i in range(8)])))
                         if hasattr(obj, "check_code") else _CHECK_CODE())
        ops._keepalive = (obj, errs)
        return ops


def synthetic_circuit():
    """Pointer to the library's built-in table (bx_synthetic_circuit)."""
    lib = load_library()
    lib.bx_synthetic_circuit.restype = C.POINTER(CircuitOps)
    return lib.bx_synthetic_circuit()


def lookup_circuit():
    """Pointer to the library's lookup circuit (bx_lookup_circuit, include/bx_lookup.h): a range check proved with LogUp running sums."""
    lib = load_library()
    lib.bx_lookup_circuit.restype = C.POINTER(CircuitOps)
    return lib.bx_lookup_circuit()


def builtin_circuit(name):
    """"synthetic" or "lookup" -> pointer to the library's table"""
    if name == "synthetic":
        return synthetic_circuit()
    if name == "lookup":
        return lookup_circuit()
    raise ValueError(f"unknown built-in circuit {name!r} (\"synthetic\" or \"lookup\")")


def encode_cell_records(records):
    """The payload of a lookup-circuit segment (include/bx_lookup.h, "segment"): an iterable of (col, row, value) -> 12 bytes each,
    little endian.  `value` is the field value the data cell (col, row) is to hold (not its Montgomery word)."""
    out = bytearray()
    for col, row, value in records:
        for v in (col, row, value):
            out += int(v).to_bytes(4, "little")
    return bytes(out)


# ---- constraint programs (include/bx_program.h): a circuit's eval_check and constraints_at from one description ----
class ConsStep(C.Structure):
    _fields_ = [("op", C.c_uint32), ("a", C.c_uint32), ("b", C.c_uint32), ("c", C.c_uint32), ("d", C.c_uint32)]


class ConsTap(C.Structure):
    _fields_ = [("group", C.c_uint32), ("col", C.c_uint32), ("back", C.c_uint32)]


class ConsProgramDesc(C.Structure):
    _fields_ = [("steps", C.POINTER(ConsStep)), ("n_steps", C.c_size_t), ("taps", C.POINTER(ConsTap)), ("n_taps", C.c_size_t),
                ("n_globals", C.c_uint32), ("ret", C.c_uint32)]


class ConsProgramInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("steps", "constraints", "degree", "narrow", "wide", "instructions", "taps", "n_globals")]


(OP_CONST, OP_CONST_EXT, OP_GET, OP_GET_GLOBAL, OP_ADD, OP_SUB, OP_MUL, OP_TRUE, OP_AND_EQZ, OP_AND_COND) = range(10)  # enum bx_cons_op
CONS_MAX_STEPS, CONS_MAX_DEGREE, CONS_MAX_NARROW, CONS_MAX_WIDE = 65536, 5, 32, 24  # BX_CONS_MAX_*


def _cons_lib():
    lib = load_library()
    if not getattr(lib, "_cons_bound", False):
        u32p, vp = C.POINTER(C.c_uint32), C.c_void_p
        lib.bx_cons_program_create.argtypes = [C.POINTER(ConsProgramDesc), C.POINTER(vp)]
        lib.bx_cons_program_destroy.argtypes = [vp]
        lib.bx_cons_program_destroy.restype = None
        lib.bx_cons_program_info_get.argtypes = [vp, C.POINTER(ConsProgramInfo)]
        lib.bx_cons_program_taps.argtypes = [vp, C.c_int, C.c_uint32, u32p]
        lib.bx_cons_program_taps.restype = C.c_uint32
        lib.bx_cons_program_constraints_at.argtypes = [vp, C.POINTER(TapReader), u32p, u32p, u32p, u32p]
        lib.bx_cons_program_load.argtypes = [vp, vp, C.POINTER(vp)]
        lib.bx_cons_program_unload.argtypes = [vp]
        lib.bx_cons_program_eval_check.argtypes = [vp, vp, C.c_uint32, BxBuf, BxBuf, C.c_uint32, BxBuf, C.c_uint32, BxBuf, C.c_uint32, u32p, u32p, u32p,
                                                   C.c_uint32]
        lib.bx_cons_circuit_create.argtypes = [vp, vp, C.POINTER(vp)]
        lib.bx_cons_circuit_ops.argtypes = [vp]
        lib.bx_cons_circuit_ops.restype = C.POINTER(CircuitOps)
        lib.bx_cons_circuit_destroy.argtypes = [vp]
        lib.bx_cons_circuit_destroy.restype = None
        lib.bx_cons_program_digest.argtypes = [vp, u32p]
        lib.bx_cons_program_emit_hip.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
        lib.bx_cons_program_attach_kernel.argtypes = [vp, C.c_char_p, C.c_size_t]
        lib.bx_cons_program_detach_kernel.argtypes = [vp]
        lib.bx_cons_program_kernel_attached.argtypes = [vp]
        lib.bx_cons_program_kernel_attached.restype = C.c_int
        lib.bx_cons_circuit_set_kernel.argtypes = [vp, C.c_char_p, C.c_size_t]
        for name in ("bx_cons_program_create", "bx_cons_program_info_get", "bx_cons_program_constraints_at", "bx_cons_program_load", "bx_cons_program_unload",
                     "bx_cons_program_eval_check", "bx_cons_circuit_create", "bx_cons_program_digest", "bx_cons_program_emit_hip",
                     "bx_cons_program_attach_kernel", "bx_cons_program_detach_kernel", "bx_cons_circuit_set_kernel"):
            getattr(lib, name).restype = C.c_char_p
        lib._cons_bound = True
    return lib


def _u32x(words, n=None):
    words = [int(w) for w in words]
    assert n is None or len(words) == n
    return (C.c_uint32 * max(len(words), 1))(*words)


class _CompiledProgram:
    """What the compiled handles of the three program kinds share (bx_<kind>_program): host only until `load`ed on a HipHal.  A
    subclass names its kind, its info structure and its loaded class."""

    _KIND = _INFO = _LOADED = None

    def _fn(self, name):
        return getattr(self.lib, f"bx_{self._KIND}_program_{name}")

    def info(self):
        out = self._INFO()
        msg = self._fn("info_get")(self.handle, C.byref(out))
        assert not msg, msg
        return {n: int(getattr(out, n)) for n, _ in self._INFO._fields_}

    def load(self, hal):
        dev = C.c_void_p()
        hal._check(self._fn("load")(hal.ctx, self.handle, C.byref(dev)))
        return self._LOADED(self, hal, dev)

    def close(self):
        if self.handle:
            self._fn("destroy")(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _EmitsKernel:
    """... of the kinds a kernel can be generated for: the digest a generated kernel carries, and its text"""

    def digest(self):
        """bx_<kind>_program_digest as 64 hex digits (the 32 bytes in order): what a generated kernel carries and attach compares"""
        from .hal import HalError

        out = (C.c_uint32 * 8)()
        msg = self._fn("digest")(self.handle, out)
        if msg:
            raise HalError(msg.decode())
        return b"".join(int(w).to_bytes(4, "little") for w in out).hex()

    def emit_hip(self):
        """bx_<kind>_program_emit_hip: the generated translation unit as text (boundless_amd.consgen compiles it)"""
        from .hal import HalError

        need = C.c_size_t(0)
        msg = self._fn("emit_hip")(self.handle, None, 0, C.byref(need))
        if msg:
            raise HalError(msg.decode())
        buf = C.create_string_buffer(need.value)
        msg = self._fn("emit_hip")(self.handle, buf, need.value, C.byref(need))
        if msg:
            raise HalError(msg.decode())
        return buf.value.decode()


class _LoadedProgram:
    """What the loaded handles share (bx_<kind>_program_dev)."""

    def __init__(self, program, hal, dev):
        self.program, self.hal, self.dev = program, hal, dev

    def unload(self):
        if self.dev:
            dev, self.dev = self.dev, None
            self.hal._check(self.program._fn("unload")(dev))


class _AttachesKernel:
    """... of the kinds a kernel can be generated for"""

    def attach_kernel(self, path_or_bytes):
        """bx_<kind>_program_attach_kernel: a code object built by boundless_amd.consgen for THIS program (a path, or its bytes); the
        program's launches then run it instead of the interpreter.  A refusal raises HalError."""
        image = _kernel_image(path_or_bytes)
        self.hal._check(self.program._fn("attach_kernel")(self.dev, image, len(image)))

    def detach_kernel(self):
        self.hal._check(self.program._fn("detach_kernel")(self.dev))

    @property
    def kernel_attached(self):
        return bool(self.dev) and bool(self.program._fn("kernel_attached")(self.dev))


def _kernel_image(path_or_bytes):
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        return bytes(path_or_bytes)
    with open(path_or_bytes, "rb") as f:
        return f.read()


class LoadedConsProgram(_LoadedProgram, _AttachesKernel):
    """A constraint program on a ctx (bx_cons_program_dev); hal.cons_program_eval_check runs it."""


class CompiledConsProgram(_CompiledProgram, _EmitsKernel):
    """A compiled constraint program (bx_cons_program): host only until `load`ed on a HipHal."""

    _KIND, _INFO, _LOADED = "cons", ConsProgramInfo, LoadedConsProgram

    def __init__(self, lib, handle, n_globals):
        self.lib, self.handle, self.n_globals = lib, handle, n_globals

    info = property(_CompiledProgram.info)

    def taps(self, group, col):
        out = (C.c_uint32 * MAX_TAPS)()
        n = self.lib.bx_cons_program_taps(self.handle, int(group), int(col), out)
        return list(out[:n])

    def constraints_at(self, tap, poly_mix, mix, globals_=()):
        """tap(group, col, back) -> 4 Montgomery words (raise to refuse); poly_mix, mix: 4 Montgomery words; -> 4 Montgomery words.
        A refused tap reads as zero and its message is raised as HalError once the evaluation is through."""
        from .hal import HalError

        errs = []

        def at(_ctx, group, col, back, out):
            try:
                v = tap(group, col, back)
                for i in range(4):
                    out[i] = int(v[i])
                return None
            except Exception as e:  # noqa: BLE001 - crosses the ABI as a string
                errs.append(C.create_string_buffer(f"{type(e).__name__}: {e}".encode()))
                return C.cast(errs[-1], C.c_void_p).value

        reader = TapReader(None, _TAP_AT(at))
        out = (C.c_uint32 * 4)()
        g = list(globals_)
        assert len(g) >= self.n_globals, "fewer globals than the program names"
        msg = self.lib.bx_cons_program_constraints_at(self.handle, C.byref(reader), _u32x(poly_mix, 4), _u32x(mix, 4), _u32x(g), out)
        if msg:
            raise HalError(msg.decode())
        return list(out)


class ConsProgram:
    """Builder of a constraint program (include/bx_program.h, "Values"): every method appends one step and returns the index of the
    fp var or mix var it made, which later steps take as operands.

        p = ConsProgram(n_globals=1)
        x = p.get(1, 0, 0)
        top = p.and_eqz(p.true(), p.sub(p.mul(x, x), p.get(1, 1, 0)))
        prog = p.compile(ret=top)
    """

    def __init__(self, n_globals=0):
        self.n_globals = n_globals
        self.steps, self.tap_list, self._tap_index = [], [], {}
        self.n_fp = self.n_mix = 0

    def _fp(self, op, a=0, b=0, c=0, d=0):
        self.steps.append((op, a, b, c, d))
        self.n_fp += 1
        return self.n_fp - 1

    def _mix(self, op, a=0, b=0, c=0):
        self.steps.append((op, a, b, c, 0))
        self.n_mix += 1
        return self.n_mix - 1

    def const(self, a):
        return self._fp(OP_CONST, a)

    def const_ext(self, a, b, c, d):
        return self._fp(OP_CONST_EXT, a, b, c, d)

    def tap(self, group, col, back=0):
        """index of (group, col, back) in the tap list (added on first use)"""
        key = (int(group), int(col), int(back))
        if key not in self._tap_index:
            self._tap_index[key] = len(self.tap_list)
            self.tap_list.append(key)
        return self._tap_index[key]

    def get(self, group, col, back=0):
        return self._fp(OP_GET, self.tap(group, col, back))

    def get_tap(self, index):
        """GET of a raw tap-list index (not checked here: bx_cons_program_create is the judge)"""
        return self._fp(OP_GET, index)

    def global_(self, index):
        return self._fp(OP_GET_GLOBAL, 0, index)

    def mix(self, component):
        return self._fp(OP_GET_GLOBAL, 1, component)

    def add(self, a, b):
        return self._fp(OP_ADD, a, b)

    def sub(self, a, b):
        return self._fp(OP_SUB, a, b)

    def mul(self, a, b):
        return self._fp(OP_MUL, a, b)

    def true(self):
        return self._mix(OP_TRUE)

    def and_eqz(self, x, y):
        return self._mix(OP_AND_EQZ, x, y)

    def and_cond(self, x, cond, inner):
        return self._mix(OP_AND_COND, x, cond, inner)

    def compile(self, ret=None):
        """-> CompiledConsProgram; ret = the mix var whose tot is the result (default: the last one).  A refusal raises HalError."""
        from .hal import HalError

        lib = _cons_lib()
        steps = (ConsStep * max(len(self.steps), 1))(*[ConsStep(*s) for s in self.steps])
        taps = (ConsTap * max(len(self.tap_list), 1))(*[ConsTap(*t) for t in self.tap_list])
        desc = ConsProgramDesc(steps, len(self.steps), taps, len(self.tap_list), self.n_globals, (self.n_mix - 1 if ret is None else ret) & 0xFFFFFFFF)
        handle = C.c_void_p()
        msg = lib.bx_cons_program_create(C.byref(desc), C.byref(handle))
        if msg:
            raise HalError(msg.decode())
        return CompiledConsProgram(lib, handle, self.n_globals)


def _from_program(program, base, kernel=None, witness=None, witness_kernel=None, accumulate=None):
    """CircuitOps.from_program(program, base, kernel=None, witness=None, witness_kernel=None, accumulate=None): the table whose taps, eval_check and constraints_at come from
    `program` (a CompiledConsProgram) and everything else from `base` (a CircuitOps: from_object, lookup_circuit() or synthetic_circuit()).
    kernel: a code object generated from `program` (boundless_amd.consgen; a path or its bytes) that eval_check launches instead of
    the interpreter; a prover's creation fails with attach_kernel's message if it is not this program's.
    witness: a CompiledWitnessProgram; `base`'s witgen then only has to place the free cells, the program derives the other data columns
    on the device and its global cells become public words (bx_cons_circuit_set_witness).
    witness_kernel: a code object generated from `witness` (boundless_amd.consgen --witness; a path or its bytes) that witgen launches
    instead of the interpreter; a prover's creation fails with attach_kernel's message if it is not that program's, and by name if
    there is no `witness`.
    accumulate: a CompiledAccumulateProgram; the table's accumulate then calls `base`'s (if it has one: it owns filler and the accum
    columns at or above 4 S) and writes the program's running sums and products into accum columns [0, 4 S) on the device
    (bx_cons_circuit_set_accumulate).  A prover's creation refuses by name a program that does not fit the shape.
    The result is used like any other table (HipProverServer(circuit=...), verify_seal(circuit=...)); it keeps program, base and witness alive."""
    import weakref

    from .hal import HalError

    lib = _cons_lib()
    base_ptr = C.addressof(base) if isinstance(base, C.Structure) else C.cast(base, C.c_void_p).value
    cc = C.c_void_p()
    msg = lib.bx_cons_circuit_create(base_ptr, program.handle, C.byref(cc))
    if msg:
        raise HalError(msg.decode())
    if kernel is not None:
        image = _kernel_image(kernel)
        msg = lib.bx_cons_circuit_set_kernel(cc, image, len(image))
        if msg:
            lib.bx_cons_circuit_destroy(cc)
            raise HalError(msg.decode())
    if witness is not None:
        msg = _wit_lib().bx_cons_circuit_set_witness(cc, witness.handle)
        if msg:
            lib.bx_cons_circuit_destroy(cc)
            raise HalError(msg.decode())
    if witness_kernel is not None:
        image = _kernel_image(witness_kernel)
        msg = _wit_lib().bx_cons_circuit_set_witness_kernel(cc, image, len(image))
        if msg:
            lib.bx_cons_circuit_destroy(cc)
            raise HalError(msg.decode())
    if accumulate is not None:
        msg = _acc_lib().bx_cons_circuit_set_accumulate(cc, accumulate.handle)
        if msg:
            lib.bx_cons_circuit_destroy(cc)
            raise HalError(msg.decode())
    ops = lib.bx_cons_circuit_ops(cc).contents
    ops._keepalive = (program, base, witness, accumulate)
    weakref.finalize(ops, lib.bx_cons_circuit_destroy, cc)
    return ops


# ---- witness programs (include/bx_program.h, "Witness programs"): a circuit's derived data columns from one description ----
OP_SET = 10  # BX_CONS_SET


class WitGlobalCell(C.Structure):
    _fields_ = [("global_", C.c_uint32), ("col", C.c_uint32), ("row", C.c_uint32)]


class WitProgramDesc(C.Structure):
    _fields_ = [("steps", C.POINTER(ConsStep)), ("n_steps", C.c_size_t), ("taps", C.POINTER(ConsTap)), ("n_taps", C.c_size_t),
                ("cells", C.POINTER(WitGlobalCell)), ("n_cells", C.c_size_t)]


class WitCount(C.Structure):
    _fields_ = [("col", C.c_uint32), ("bins", C.c_uint32), ("rows", C.c_uint32), ("n_sources", C.c_uint32), ("sources", C.POINTER(C.c_uint32))]


class WitSort(C.Structure):
    _fields_ = [("rows", C.c_uint32), ("n_keys", C.c_uint32), ("n_cols", C.c_uint32), ("bits", C.POINTER(C.c_uint32)), ("sources", C.POINTER(C.c_uint32)),
                ("dests", C.POINTER(C.c_uint32))]


class WitProgramInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("steps", "sets", "narrow", "instructions", "taps", "cells")]


def _wit_lib():
    lib = load_library()
    if not getattr(lib, "_wit_bound", False):
        u32p, vp = C.POINTER(C.c_uint32), C.c_void_p
        lib.bx_wit_program_create.argtypes = [C.POINTER(WitProgramDesc), C.POINTER(vp)]
        lib.bx_wit_program_create_counted.argtypes = [C.POINTER(WitProgramDesc), C.POINTER(WitCount), C.c_size_t, C.POINTER(vp)]
        lib.bx_wit_program_counts.argtypes = [vp]
        lib.bx_wit_program_counts.restype = C.c_uint32
        lib.bx_wit_program_count_get.argtypes = [vp, C.c_uint32, u32p, u32p, u32p, u32p, C.c_uint32, u32p]
        lib.bx_wit_program_create_sorted.argtypes = [C.POINTER(WitProgramDesc), C.POINTER(WitCount), C.c_size_t, C.POINTER(WitSort), C.c_size_t, C.POINTER(vp)]
        lib.bx_wit_program_sorts.argtypes = [vp]
        lib.bx_wit_program_sorts.restype = C.c_uint32
        lib.bx_wit_program_sort_get.argtypes = [vp, C.c_uint32, u32p, u32p, u32p, u32p, u32p, C.c_uint32, u32p]
        for name in ("bx_wit_program_create_sorted", "bx_wit_program_sort_get"):
            getattr(lib, name).restype = C.c_char_p
        lib.bx_wit_program_destroy.argtypes = [vp]
        lib.bx_wit_program_destroy.restype = None
        lib.bx_wit_program_info_get.argtypes = [vp, C.POINTER(WitProgramInfo)]
        lib.bx_wit_program_derives.argtypes = [vp, C.c_uint32]
        lib.bx_wit_program_derives.restype = C.c_int
        lib.bx_wit_program_run_host.argtypes = [vp, C.c_uint32, u32p, C.c_uint32, u32p, C.c_uint32]
        lib.bx_wit_program_load.argtypes = [vp, vp, C.POINTER(vp)]
        lib.bx_wit_program_unload.argtypes = [vp]
        lib.bx_wit_program_run.argtypes = [vp, vp, C.c_uint32, BxBuf, C.c_uint32, BxBuf, C.c_uint32]
        lib.bx_cons_circuit_set_witness.argtypes = [vp, vp]
        lib.bx_wit_program_digest.argtypes = [vp, u32p]
        lib.bx_wit_program_emit_hip.argtypes = [vp, C.c_char_p, C.c_size_t, C.POINTER(C.c_size_t)]
        lib.bx_wit_program_attach_kernel.argtypes = [vp, C.c_char_p, C.c_size_t]
        lib.bx_wit_program_detach_kernel.argtypes = [vp]
        lib.bx_wit_program_kernel_attached.argtypes = [vp]
        lib.bx_wit_program_kernel_attached.restype = C.c_int
        lib.bx_cons_circuit_set_witness_kernel.argtypes = [vp, C.c_char_p, C.c_size_t]
        for name in ("bx_wit_program_create", "bx_wit_program_create_counted", "bx_wit_program_count_get", "bx_wit_program_info_get", "bx_wit_program_run_host", "bx_wit_program_load", "bx_wit_program_unload",
                     "bx_wit_program_run", "bx_cons_circuit_set_witness", "bx_wit_program_digest", "bx_wit_program_emit_hip",
                     "bx_wit_program_attach_kernel", "bx_wit_program_detach_kernel", "bx_cons_circuit_set_witness_kernel"):
            getattr(lib, name).restype = C.c_char_p
        lib._wit_bound = True
    return lib


class LoadedWitnessProgram(_LoadedProgram, _AttachesKernel):
    """A witness program on a ctx (bx_wit_program_dev); hal.wit_program_run runs it."""

    def run(self, po2, code, w_code, data, w_data):
        self.hal.wit_program_run(self, po2, code, w_code, data, w_data)


class CompiledWitnessProgram(_CompiledProgram, _EmitsKernel):
    """A compiled witness program (bx_wit_program): host only until `load`ed on a HipHal."""

    _KIND, _INFO, _LOADED = "wit", WitProgramInfo, LoadedWitnessProgram

    def __init__(self, lib, handle):
        self.lib, self.handle = lib, handle

    def derives(self, col):
        return bool(self.lib.bx_wit_program_derives(self.handle, int(col)))

    def counts(self):
        """the multiplicity columns as dicts {"col", "bins", "rows", "sources"}, in list order (bx_wit_program_count_get)"""
        from .hal import HalError

        out = []
        col, bins, rows, n_src = C.c_uint32(), C.c_uint32(), C.c_uint32(), C.c_uint32()
        src = (C.c_uint32 * 64)()  # BX_WIT_MAX_COUNT_SOURCES
        for i in range(self.lib.bx_wit_program_counts(self.handle)):
            msg = self.lib.bx_wit_program_count_get(self.handle, i, C.byref(col), C.byref(bins), C.byref(rows), src, 64, C.byref(n_src))
            if msg:
                raise HalError(msg.decode())
            out.append({"col": int(col.value), "bins": int(bins.value), "rows": int(rows.value), "sources": [int(v) for v in src[:n_src.value]]})
        return out

    def sorts(self):
        """the sorted columns as dicts {"rows", "keys": [(col, bits), ...], "payload", "dests"}, in list order (bx_wit_program_sort_get)"""
        from .hal import HalError

        out = []
        rows, n_keys, n_cols = C.c_uint32(), C.c_uint32(), C.c_uint32()
        bits, src, dst = (C.c_uint32 * 4)(), (C.c_uint32 * 16)(), (C.c_uint32 * 16)()  # BX_WIT_MAX_SORT_KEYS, BX_WIT_MAX_SORT_COLS
        for i in range(self.lib.bx_wit_program_sorts(self.handle)):
            msg = self.lib.bx_wit_program_sort_get(self.handle, i, C.byref(rows), C.byref(n_keys), bits, src, dst, 16, C.byref(n_cols))
            if msg:
                raise HalError(msg.decode())
            nk, nc = int(n_keys.value), int(n_cols.value)
            out.append({"rows": int(rows.value), "keys": [(int(src[q]), int(bits[q])) for q in range(nk)], "payload": [int(v) for v in src[nk:nc]],
                        "dests": [int(v) for v in dst[:nc]]})
        return out

    def run_host(self, po2, code, w_code, data, w_data):
        """bx_wit_program_run_host: code (w_code x N) and data (w_data x N) are C-contiguous uint32 numpy arrays of Montgomery words;
        the derived columns of `data` are written in place.  A refusal raises HalError."""
        import numpy as np

        from .hal import HalError

        for a, w in ((code, w_code), (data, w_data)):
            assert a.dtype == np.uint32 and a.flags.c_contiguous and a.size == w << po2, "a group is a C-contiguous uint32 array of width x N words"
        assert data.flags.writeable
        u32p = C.POINTER(C.c_uint32)
        msg = self.lib.bx_wit_program_run_host(self.handle, po2, code.ctypes.data_as(u32p), w_code, data.ctypes.data_as(u32p), w_data)
        if msg:
            raise HalError(msg.decode())


class WitnessProgram:
    """Builder of a witness program (include/bx_program.h, "Witness programs"): const / get / add / sub / mul append one step and
    return the index of the fp var it made; set(col, var) stores a var into a data column, which makes that column derived;
    count(col, sources, bins, rows=0) makes `col` a multiplicity column ("multiplicity columns"): after every row has run,
    data[col][r] = how many cells of the `sources` columns, rows [0, rows), hold the integer r, for r < bins (rows = 0: all rows);
    sort(keys, payload, dests, rows=0) writes a stably sorted copy of columns ("sorted columns"), after every row and before the counts.

        w = WitnessProgram()
        x = w.get(1, 0)
        w.set(1, w.add(w.mul(x, x), w.get(0, 0)))
        w.global_cell(0, 1, 0)  # public word 0 = data[1][0]
        prog = w.compile()
    """

    def __init__(self):
        self.steps, self.tap_list, self._tap_index, self.cells = [], [], {}, []
        self.count_list = []
        self.sort_list = []
        self.n_fp = 0

    def _fp(self, op, a=0, b=0):
        self.steps.append((op, a, b, 0, 0))
        self.n_fp += 1
        return self.n_fp - 1

    def const(self, a):
        return self._fp(OP_CONST, a)

    def tap(self, group, col, back=0):
        """index of (group, col, back) in the tap list (added on first use)"""
        key = (int(group), int(col), int(back))
        if key not in self._tap_index:
            self._tap_index[key] = len(self.tap_list)
            self.tap_list.append(key)
        return self._tap_index[key]

    def get(self, group, col, back=0):
        return self._fp(OP_GET, self.tap(group, col, back))

    def add(self, a, b):
        return self._fp(OP_ADD, a, b)

    def sub(self, a, b):
        return self._fp(OP_SUB, a, b)

    def mul(self, a, b):
        return self._fp(OP_MUL, a, b)

    def set(self, col, var):
        self.steps.append((OP_SET, col, var, 0, 0))

    def global_cell(self, index, col, row):
        self.cells.append((int(index), int(col), int(row)))

    def count(self, col, sources, bins, rows=0):
        entry = (int(col), [int(s) for s in sources], int(bins), int(rows))
        for v in (entry[0], entry[2], entry[3], *entry[1]):
            if not 0 <= v < 1 << 32:  # the library takes 32-bit words: a value that would wrap into a valid one is an error here
                raise ValueError(f"WitnessProgram.count: {v} is not a 32-bit unsigned value")
        self.count_list.append(entry)

    def sort(self, keys, payload=(), dests=(), rows=0):
        """after every row has run and before the counts ("sorted columns"): rows [0, rows) of the key columns `keys` = [(col, bits), ...]
        (most significant first) and of the `payload` columns, stably sorted by the low `bits` bits of the keys, go to `dests`, one per
        key and payload column in that order (rows = 0: all rows)"""
        entry = ([(int(c), int(b)) for c, b in keys], [int(c) for c in payload], [int(c) for c in dests], int(rows))
        if len(entry[2]) != len(entry[0]) + len(entry[1]):
            raise ValueError(f"WitnessProgram.sort: {len(entry[2])} dests for {len(entry[0]) + len(entry[1])} key and payload columns")
        for v in (entry[3], *[v for kb in entry[0] for v in kb], *entry[1], *entry[2]):
            if not 0 <= v < 1 << 32:
                raise ValueError(f"WitnessProgram.sort: {v} is not a 32-bit unsigned value")
        self.sort_list.append(entry)

    def compile(self):
        """-> CompiledWitnessProgram.  A refusal raises HalError."""
        from .hal import HalError

        lib = _wit_lib()
        steps = (ConsStep * max(len(self.steps), 1))(*[ConsStep(*s) for s in self.steps])
        taps = (ConsTap * max(len(self.tap_list), 1))(*[ConsTap(*t) for t in self.tap_list])
        cells = (WitGlobalCell * max(len(self.cells), 1))(*[WitGlobalCell(*g) for g in self.cells])
        desc = WitProgramDesc(steps, len(self.steps), taps, len(self.tap_list), cells, len(self.cells))
        handle = C.c_void_p()
        u32p = C.POINTER(C.c_uint32)
        srcs = [(C.c_uint32 * max(len(s), 1))(*s) for _, s, _, _ in self.count_list]
        counts = (WitCount * max(len(self.count_list), 1))(*[WitCount(col, bins, rows, len(s), C.cast(a, u32p)) for (col, s, bins, rows), a in zip(self.count_list, srcs)])
        if self.sort_list:
            keep, sorts = [], (WitSort * len(self.sort_list))()
            for k, (keys, payload, dests, rows) in enumerate(self.sort_list):
                cols = [c for c, _ in keys] + payload
                arrays = [(C.c_uint32 * max(len(v), 1))(*v) for v in ([b for _, b in keys], cols, dests)]
                keep.append(arrays)
                sorts[k] = WitSort(rows, len(keys), len(cols), *[C.cast(a, u32p) for a in arrays])
            msg = lib.bx_wit_program_create_sorted(C.byref(desc), counts if self.count_list else None, len(self.count_list), sorts, len(self.sort_list), C.byref(handle))
        elif not self.count_list:
            msg = lib.bx_wit_program_create(C.byref(desc), C.byref(handle))
        else:
            msg = lib.bx_wit_program_create_counted(C.byref(desc), counts, len(self.count_list), C.byref(handle))
        if msg:
            raise HalError(msg.decode())
        return CompiledWitnessProgram(lib, handle)


# ---- accumulate programs (include/bx_program.h, "Accumulate programs"): a circuit's running sums and products from one description ----
OP_SUM, OP_PROD = 11, 12  # BX_CONS_SUM, BX_CONS_PROD
OP_RATIO = 16  # BX_CONS_RATIO (13, 14 and 15 are no ops)
ACC_MAX_SEQS = 1024  # BX_ACC_MAX_SEQS


class AccProgramDesc(C.Structure):
    _fields_ = [("steps", C.POINTER(ConsStep)), ("n_steps", C.c_size_t), ("taps", C.POINTER(ConsTap)), ("n_taps", C.c_size_t), ("n_globals", C.c_uint32)]


class AccProgramInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("steps", "sequences", "sums", "instructions", "narrow", "wide", "taps", "kept", "n_globals")]


def _acc_lib():
    lib = load_library()
    if not getattr(lib, "_acc_bound", False):
        u32p, vp = C.POINTER(C.c_uint32), C.c_void_p
        lib.bx_acc_program_create.argtypes = [C.POINTER(AccProgramDesc), C.POINTER(vp)]
        lib.bx_acc_program_destroy.argtypes = [vp]
        lib.bx_acc_program_destroy.restype = None
        lib.bx_acc_program_info_get.argtypes = [vp, C.POINTER(AccProgramInfo)]
        lib.bx_acc_program_kept.argtypes = [vp, C.c_uint32, u32p, u32p]
        lib.bx_acc_program_run_host.argtypes = [vp, C.c_uint32, u32p, C.c_uint32, u32p, C.c_uint32, u32p, u32p, u32p, C.c_uint32]
        lib.bx_acc_program_load.argtypes = [vp, vp, C.POINTER(vp)]
        lib.bx_acc_program_unload.argtypes = [vp]
        lib.bx_acc_program_keep.argtypes = [vp, vp, C.c_uint32, BxBuf, C.c_uint32, BxBuf, C.c_uint32, BxBuf]
        lib.bx_acc_program_run.argtypes = [vp, vp, C.c_uint32, BxBuf, u32p, u32p, BxBuf, BxBuf, BxBuf, C.c_uint32]
        lib.bx_cons_circuit_set_accumulate.argtypes = [vp, vp]
        lib.bx_acc_program_ratios.argtypes = [vp, u32p]
        for name in ("bx_acc_program_create", "bx_acc_program_info_get", "bx_acc_program_kept", "bx_acc_program_ratios", "bx_acc_program_run_host", "bx_acc_program_load",
                     "bx_acc_program_unload", "bx_acc_program_keep", "bx_acc_program_run", "bx_cons_circuit_set_accumulate"):
            getattr(lib, name).restype = C.c_char_p
        lib._acc_bound = True
    return lib


class LoadedAccumulateProgram(_LoadedProgram):
    """An accumulate program on a ctx (bx_acc_program_dev); hal.acc_program_keep / hal.acc_program_run run it."""

    def keep(self, po2, code, w_code, data, w_data, kept):
        self.hal.acc_program_keep(self, po2, code, w_code, data, w_data, kept)

    def run(self, po2, kept, globals_, mix, run_ext, mults, accum, w_accum):
        self.hal.acc_program_run(self, po2, kept, globals_, mix, run_ext, mults, accum, w_accum)


class CompiledAccumulateProgram(_CompiledProgram):
    """A compiled accumulate program (bx_acc_program): host only until `load`ed on a HipHal."""

    _KIND, _INFO, _LOADED = "acc", AccProgramInfo, LoadedAccumulateProgram

    def __init__(self, lib, handle, n_globals):
        self.lib, self.handle, self.n_globals = lib, handle, n_globals

    def kept(self):
        """the kept columns as (group, col), in kept order: what `keep` copies and the taps read"""
        out = []
        g, c = C.c_uint32(), C.c_uint32()
        for i in range(self.info()["kept"]):
            msg = self.lib.bx_acc_program_kept(self.handle, i, C.byref(g), C.byref(c))
            assert not msg, msg
            out.append((int(g.value), int(c.value)))
        return out

    def ratios(self):
        """R, the number of RATIO sequences: the last R of info()["sequences"] (bx_acc_program_ratios).  run_ext of `run` holds
        4 N (S + R) words."""
        r = C.c_uint32()
        msg = self.lib.bx_acc_program_ratios(self.handle, C.byref(r))
        assert not msg, msg
        return int(r.value)

    def run_host(self, po2, code, w_code, data, w_data, globals_, mix, accum, w_accum):
        """bx_acc_program_run_host: code (w_code x N), data (w_data x N) and accum (w_accum x N) are C-contiguous uint32 numpy arrays of
        Montgomery words; globals_ the program's public words, mix four words.  Columns [0, 4 S) of `accum` are written in place.  A
        refusal raises HalError."""
        import numpy as np

        from .hal import HalError

        for a, w in ((code, w_code), (data, w_data), (accum, w_accum)):
            assert a.dtype == np.uint32 and a.flags.c_contiguous and a.size == w << po2, "a group is a C-contiguous uint32 array of width x N words"
        assert accum.flags.writeable
        g = list(globals_)
        assert len(g) >= self.n_globals, "fewer globals than the program names"
        u32p = C.POINTER(C.c_uint32)
        msg = self.lib.bx_acc_program_run_host(self.handle, po2, code.ctypes.data_as(u32p), w_code, data.ctypes.data_as(u32p), w_data, _u32x(g), _u32x(mix, 4),
                                               accum.ctypes.data_as(u32p), w_accum)
        if msg:
            raise HalError(msg.decode())


class AccumulateProgram(ConsProgram):
    """Builder of an accumulate program (include/bx_program.h, "Accumulate programs"): const / const_ext / get / global_ / mix / add / sub /
    mul append one step and return the index of the fp var it made; sum_(s, m, d) makes sequence s the running sum of m / d, prod(s, a)
    the running product of a, ratio(s, a, b) the running product of a / b.  Sums are numbered before products, products before ratios;
    sequence s is accum columns 4 s .. 4 s + 3.

        p = AccumulateProgram()
        alpha = p.add(p.const_ext(0, 1, 0, 0), p.mix(0))   # an ext value built from a mix component
        p.sum_(0, p.const(1), p.sub(alpha, p.get(1, 0)))
        prog = p.compile()
    """

    def sum_(self, s, m, d):
        self.steps.append((OP_SUM, s, m, d, 0))

    def prod(self, s, a):
        self.steps.append((OP_PROD, s, a, 0, 0))

    def ratio(self, s, a, b):
        """sequence s is the running product of a / b (a zero b contributes the factor 0); ratios are numbered after all products"""
        self.steps.append((OP_RATIO, s, a, b, 0))

    def compile(self):
        """-> CompiledAccumulateProgram.  A refusal raises HalError."""
        from .hal import HalError

        lib = _acc_lib()
        steps = (ConsStep * max(len(self.steps), 1))(*[ConsStep(*s) for s in self.steps])
        taps = (ConsTap * max(len(self.tap_list), 1))(*[ConsTap(*t) for t in self.tap_list])
        desc = AccProgramDesc(steps, len(self.steps), taps, len(self.tap_list), self.n_globals)
        handle = C.c_void_p()
        msg = lib.bx_acc_program_create(C.byref(desc), C.byref(handle))
        if msg:
            raise HalError(msg.decode())
        return CompiledAccumulateProgram(lib, handle, self.n_globals)


CircuitOps.from_program = staticmethod(_from_program)


# ---- trace layouts (include/bx_layout.h): a circuit's code group and free cells from one description — the base of from_program ----
(LAYOUT_CONST, LAYOUT_FIRST, LAYOUT_LAST, LAYOUT_ACTIVE, LAYOUT_ROW, LAYOUT_PERIODIC, LAYOUT_WORD) = range(7)  # enum bx_layout_code_kind
LAYOUT_MAX_STRIDE = 128  # BX_LAYOUT_MAX_STRIDE
SEGMENT_WIRE_BYTES = 28  # BX_SEGMENT_WIRE_BYTES


class LayoutCodeCol(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("a", C.c_uint32), ("b", C.c_uint32)]


class LayoutField(C.Structure):
    _fields_ = [("col", C.c_uint32), ("word", C.c_uint32), ("shift", C.c_uint32), ("bits", C.c_uint32), ("pad", C.c_uint32)]


class TraceLayoutDesc(C.Structure):
    _fields_ = [("code", C.POINTER(LayoutCodeCol)), ("n_code", C.c_uint32), ("table", C.POINTER(C.c_uint32)), ("n_table", C.c_uint32),
                ("fields", C.POINTER(LayoutField)), ("n_fields", C.c_uint32), ("stride", C.c_uint32), ("noise_rows", C.c_uint32), ("n_globals", C.c_uint32)]


class TraceLayoutInfo(C.Structure):
    _fields_ = [(n, C.c_uint32) for n in ("n_code", "n_table", "n_fields", "stride", "noise_rows", "n_globals", "min_w_data")]


def _layout_lib():
    lib = load_library()
    if not getattr(lib, "_layout_bound", False):
        u32p, vp = C.POINTER(C.c_uint32), C.c_void_p
        lib.bx_trace_layout_create.argtypes = [C.POINTER(TraceLayoutDesc), C.POINTER(vp)]
        lib.bx_trace_layout_destroy.argtypes = [vp]
        lib.bx_trace_layout_destroy.restype = None
        lib.bx_trace_layout_info_get.argtypes = [vp, C.POINTER(TraceLayoutInfo)]
        lib.bx_trace_layout_ops.argtypes = [vp]
        lib.bx_trace_layout_ops.restype = C.POINTER(CircuitOps)
        lib.bx_trace_layout_code_host.argtypes = [vp, C.c_uint32, u32p]
        lib.bx_trace_layout_data_host.argtypes = [vp, C.c_uint32, C.c_char_p, C.c_size_t, C.POINTER(C.c_uint64), u32p, C.c_uint32]
        lib.bx_trace_layout_control_id_host_hashfn.argtypes = [vp, C.c_uint32, C.c_char_p, u32p]
        lib.bx_trace_layout_load.argtypes = [vp, vp, C.POINTER(vp)]
        lib.bx_trace_layout_unload.argtypes = [vp]
        lib.bx_trace_layout_code.argtypes = [vp, vp, C.c_uint32, BxBuf]
        lib.bx_trace_layout_place.argtypes = [vp, vp, C.c_uint32, BxBuf, C.c_size_t, C.c_uint64, BxBuf, C.c_uint32]
        for name in ("bx_trace_layout_create", "bx_trace_layout_info_get", "bx_trace_layout_code_host", "bx_trace_layout_data_host",
                     "bx_trace_layout_control_id_host_hashfn", "bx_trace_layout_load", "bx_trace_layout_unload", "bx_trace_layout_code", "bx_trace_layout_place"):
            getattr(lib, name).restype = C.c_char_p
        lib._layout_bound = True
    return lib


def encode_records(records):
    """The payload of a trace-layout segment (include/bx_layout.h, "data"): a 2-D array-like of R records x stride 32-bit words ->
    the R * stride words as little-endian bytes, record after record."""
    import numpy as np

    a = np.asarray(records)
    if a.ndim != 2:
        raise ValueError("encode_records: a 2-D array of records x stride words is needed")
    if a.size and (a.min() < 0 or a.max() > 0xFFFFFFFF):
        raise ValueError("encode_records: a word is not a 32-bit unsigned value")
    return np.ascontiguousarray(a, dtype="<u4").tobytes()


class LoadedTraceLayout:
    """A trace layout on a ctx (bx_trace_layout_dev): the two kernels outside a proof."""

    def __init__(self, layout, hal, dev):
        self.layout, self.hal, self.dev = layout, hal, dev

    def code(self, po2, code):
        """bx_trace_layout_code: fills the N x n_code group `code` (a hal Buffer)"""
        self.hal.trace_layout_code(self, po2, code)

    def place(self, po2, segment_dev, segment_len, noise_seed, data, w_data):
        """bx_trace_layout_place: the free cells of the N x w_data group `data` from the segment's bytes in `segment_dev` (header
        included; segment_len bytes); noise_seed is the noise seed itself"""
        self.hal.trace_layout_place(self, po2, segment_dev, segment_len, noise_seed, data, w_data)

    def unload(self):
        if self.dev:
            dev, self.dev = self.dev, None
            self.hal._check(self.layout.lib.bx_trace_layout_unload(dev))


class CompiledTraceLayout:
    """A compiled trace layout (bx_trace_layout): host only until `load`ed on a HipHal or made a circuit's base with `ops`."""

    def __init__(self, lib, handle):
        self.lib, self.handle = lib, handle

    def info(self):
        out = TraceLayoutInfo()
        msg = self.lib.bx_trace_layout_info_get(self.handle, C.byref(out))
        assert not msg, msg
        return {n: int(getattr(out, n)) for n, _ in TraceLayoutInfo._fields_}

    def ops(self):
        """bx_trace_layout_ops: the layout as a CircuitOps, usable as `base` of CircuitOps.from_program (it keeps the layout alive)"""
        ops = self.lib.bx_trace_layout_ops(self.handle).contents
        ops._keepalive = self
        return ops

    def code_host(self, po2):
        """bx_trace_layout_code_host -> the code group as a (n_code, N) uint32 array of Montgomery words.  A refusal raises HalError."""
        import numpy as np

        from .hal import HalError

        out = np.zeros((self.info()["n_code"], 1 << po2), np.uint32)
        msg = self.lib.bx_trace_layout_code_host(self.handle, po2, out.ctypes.data_as(C.POINTER(C.c_uint32)))
        if msg:
            raise HalError(msg.decode())
        return out

    def data_host(self, po2, segment_bytes, w_data, noise_seed=None, out=None):
        """bx_trace_layout_data_host -> the data group's free cells as a (w_data, N) uint32 array; segment_bytes = header + payload
        (prover.Segment(...).to_bytes()); noise_seed None = derived from the segment's seed.  out: a C-contiguous (w_data, N) uint32
        array to fill instead of a new one (a refusal leaves it untouched).  A refusal raises HalError."""
        import numpy as np

        from .hal import HalError

        if out is None:
            out = np.zeros((w_data, 1 << po2), np.uint32)
        assert out.dtype == np.uint32 and out.flags.c_contiguous and out.size == w_data << po2
        seed = None if noise_seed is None else C.byref(C.c_uint64(int(noise_seed)))
        msg = self.lib.bx_trace_layout_data_host(self.handle, po2, bytes(segment_bytes), len(segment_bytes), seed, out.ctypes.data_as(C.POINTER(C.c_uint32)), w_data)
        if msg:
            raise HalError(msg.decode())
        return out

    def control_id_host(self, po2, hashfn="poseidon2"):
        """bx_trace_layout_control_id_host_hashfn -> the 8 words of the control ID of a circuit over this layout at po2"""
        import numpy as np

        from .hal import HalError

        out = np.zeros(8, np.uint32)
        msg = self.lib.bx_trace_layout_control_id_host_hashfn(self.handle, po2, hashfn.encode(), out.ctypes.data_as(C.POINTER(C.c_uint32)))
        if msg:
            raise HalError(msg.decode())
        return out

    def load(self, hal):
        dev = C.c_void_p()
        hal._check(self.lib.bx_trace_layout_load(hal.ctx, self.handle, C.byref(dev)))
        return LoadedTraceLayout(self, hal, dev)

    def close(self):
        if self.handle:
            self.lib.bx_trace_layout_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TraceLayout:
    """Builder of a trace layout (include/bx_layout.h): the code_* methods append one code column each and return its index;
    field(col, word, ...) names the record word a free data column comes from.

        t = TraceLayout(stride=2, noise_rows=0)
        t.code_first()
        t.code_last()
        t.field(0, 0, bits=8)            # data column 0 = the low 8 bits of record word 0
        t.field(1, 1, bits=30)
        layout = t.compile()
        ops = CircuitOps.from_program(cons, layout.ops(), witness=wit, accumulate=acc)
    """

    def __init__(self, stride=1, noise_rows=1994, n_globals=0):
        self.stride, self.noise_rows, self.n_globals = stride, noise_rows, n_globals
        self.code, self.table, self.fields = [], [], []

    def _code(self, kind, a=0, b=0):
        self.code.append((int(kind), int(a), int(b)))
        return len(self.code) - 1

    def code_const(self, value):
        return self._code(LAYOUT_CONST, value)

    def code_first(self):
        return self._code(LAYOUT_FIRST)

    def code_last(self, back=0):
        """1 at row A - 1 - back"""
        return self._code(LAYOUT_LAST, back)

    def code_active(self, back=0):
        """1 on rows below A - back"""
        return self._code(LAYOUT_ACTIVE, back)

    def code_row(self, below=0):
        """the value r on rows below `below` (0 = every row), else 0"""
        return self._code(LAYOUT_ROW, below)

    def code_periodic(self, values):
        """the values repeat with period len(values), a power of two up to 4096; they are appended to the layout's table"""
        values = [int(v) for v in values]
        bits = len(values).bit_length() - 1
        if not values or 1 << bits != len(values):
            raise ValueError("TraceLayout.code_periodic: the period must be a power of two")
        at = len(self.table)
        self.table += values
        return self._code(LAYOUT_PERIODIC, bits, at)

    def code_word(self, seed):
        """the pseudo-random words word(seed, c, r) of bx_prover.h"""
        return self._code(LAYOUT_WORD, int(seed) & 0xFFFFFFFF, (int(seed) >> 32) & 0xFFFFFFFF)

    def field(self, col, word, shift=0, bits=30, pad=0):
        self.fields.append((int(col), int(word), int(shift), int(bits), int(pad)))

    def compile(self):
        """-> CompiledTraceLayout.  A refusal raises HalError."""
        from .hal import HalError

        for v in [self.stride, self.noise_rows, self.n_globals, *self.table, *[v for c in self.code for v in c], *[v for f in self.fields for v in f]]:
            if not 0 <= int(v) < 1 << 32:  # the library takes 32-bit words: a value that would wrap into a valid one is an error here
                raise ValueError(f"TraceLayout.compile: {v} is not a 32-bit unsigned value")
        lib = _layout_lib()
        code = (LayoutCodeCol * max(len(self.code), 1))(*[LayoutCodeCol(*c) for c in self.code])
        table = (C.c_uint32 * max(len(self.table), 1))(*self.table)
        fields = (LayoutField * max(len(self.fields), 1))(*[LayoutField(*f) for f in self.fields])
        desc = TraceLayoutDesc(code, len(self.code), table, len(self.table), fields, len(self.fields), self.stride, self.noise_rows, self.n_globals)
        handle = C.c_void_p()
        msg = lib.bx_trace_layout_create(C.byref(desc), C.byref(handle))
        if msg:
            raise HalError(msg.decode())
        return CompiledTraceLayout(lib, handle)

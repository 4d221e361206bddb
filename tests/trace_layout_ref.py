"""Definition-level reference of trace layouts (include/bx_layout.h, "Trace layouts"), written from that text and sharing no code
with the library: code kinds, record decoding, pad, noise rows and the accum filler, with numpy uint64 and Python integers.  Words are
Montgomery words, canonical in [0, P).

Also here: the named layouts the tests run, the helper that hands a layout to the library's builder, and segments."""
import numpy as np

P = 2013265921
GOLDEN = 0x9E3779B97F4A7C15
M64 = (1 << 64) - 1
U = np.uint64
CONST, FIRST, LAST, ACTIVE, ROW, PERIODIC, WORD = range(7)
MAX_STRIDE, MAX_GLOBALS = 128, 64
POISON = 0xDEADBEEF  # not a field element: a cell that holds it was not written
LOOKUP_CODE_SEED, SYNTH_CODE_SEED = 0x4C4F4F4B55502121, 0x434F4E54524F4C21  # "LOOKUP!!", "CONTROL!"


def splitmix64(x):
    """on a Python integer"""
    z = (x + GOLDEN) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def words(seed, col, rows):
    """word(seed, col, r) for every r of the integer array `rows` -> uint32"""
    with np.errstate(over="ignore"):
        x = U(seed & M64) ^ (U(col << 32) | np.asarray(rows, U))
        z = x + U(GOLDEN)
        z = (z ^ (z >> U(30))) * U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> U(27))) * U(0x94D049BB133111EB)
        v = (z ^ (z >> U(31))) >> U(33)
    return np.where(v >= P, v - U(P), v).astype(np.uint32)


def encode(values):
    """the Montgomery words x * 2^32 mod P of values below 2^32"""
    return ((np.asarray(values, U) << U(32)) % U(P)).astype(np.uint32)


class Layout:
    def __init__(self, stride=1, noise_rows=1994, n_globals=0):
        self.stride, self.noise_rows, self.n_globals = stride, noise_rows, n_globals
        self.code, self.table, self.fields = [], [], []  # (kind, a, b); values; (col, word, shift, bits, pad)

    def col(self, kind, a=0, b=0):
        self.code.append((kind, a, b))
        return self

    def periodic(self, values):
        self.code.append((PERIODIC, len(values).bit_length() - 1, len(self.table)))
        self.table += list(values)
        return self

    def word(self, seed):
        return self.col(WORD, seed & 0xFFFFFFFF, seed >> 32)

    def field(self, col, word, shift=0, bits=30, pad=0):
        self.fields.append((col, word, shift, bits, pad))
        return self

    def min_w_data(self):
        return max([f[0] + 1 for f in self.fields], default=0)


def active_rows(po2, noise_rows):
    n = 1 << po2
    return n - min(noise_rows, n // 4)


def code_group(layout, po2):
    """-> (n_code, N) uint32"""
    n, act = 1 << po2, active_rows(po2, layout.noise_rows)
    r = np.arange(n)
    out = np.zeros((len(layout.code), n), np.uint32)
    one = int(encode(1))
    for c, (kind, a, b) in enumerate(layout.code):
        if kind in (LAST, ACTIVE):
            assert a < act, "refused where the shape is known"
        if kind == CONST:
            out[c] = encode(a)
        elif kind == FIRST:
            out[c, 0] = one
        elif kind == LAST:
            out[c, act - 1 - a] = one
        elif kind == ACTIVE:
            out[c, :act - a] = one
        elif kind == ROW:
            below = min(n, a if a else n)
            out[c, :below] = encode(r[:below])
        elif kind == PERIODIC:
            out[c] = encode(np.array(layout.table, U)[b + (r % (1 << a))])
        elif kind == WORD:
            out[c] = words(a | b << 32, c, r)
        else:
            raise ValueError(kind)
    return out


def segment_bytes(po2, seed, records, index=0):
    """the "BXSYNSEG" header followed by the records (a 2-D array of R x stride words, or raw payload bytes)"""
    payload = records if isinstance(records, (bytes, bytearray)) else np.ascontiguousarray(records, "<u4").tobytes()
    return b"BXSYNSEG" + index.to_bytes(8, "little") + po2.to_bytes(4, "little") + seed.to_bytes(8, "little") + bytes(payload)


class Refused(Exception):
    pass


def data_group(layout, po2, segment, w_data, noise_seed=None):
    """-> (w_data, N) uint32: the free cells; raises Refused for the two payload refusals"""
    n, act = 1 << po2, active_rows(po2, layout.noise_rows)
    assert segment[:8] == b"BXSYNSEG" and int.from_bytes(segment[16:20], "little") == po2
    seed = int.from_bytes(segment[20:28], "little")
    payload = segment[28:]
    if len(payload) % (4 * layout.stride):
        raise Refused("not a whole number of")
    recs = np.frombuffer(payload, "<u4").reshape(-1, layout.stride).astype(U)
    if len(recs) > act:
        raise Refused("active rows")
    noise = splitmix64(seed ^ 0x5A4B4E4F49534521) if noise_seed is None else noise_seed
    nseed = (noise + 2 * GOLDEN) & M64
    out = np.zeros((w_data, n), np.uint32)
    for col, word, shift, bits, pad in layout.fields:
        out[col, :len(recs)] = encode((recs[:, word] >> U(shift)) & U((1 << bits) - 1))
        out[col, len(recs):act] = int(encode(pad))
    for c in range(w_data):
        out[c, act:] = words(nseed, c, np.arange(act, n))
    return out


def filler(seed, mix, po2, w_accum):
    """the accum group before an accumulate program has run: every column word(filler_seed(seed, mix), c, r)"""
    fseed = ((seed + 3 * GOLDEN) & M64) ^ ((int(mix[0]) << 32) | int(mix[1]))
    return np.stack([words(fseed, c, np.arange(1 << po2)) for c in range(w_accum)]) if w_accum else np.zeros((0, 1 << po2), np.uint32)


def to_builder(layout):
    from boundless_amd.circuit import TraceLayout

    t = TraceLayout(stride=layout.stride, noise_rows=layout.noise_rows, n_globals=layout.n_globals)
    t.code, t.table, t.fields = list(layout.code), list(layout.table), list(layout.fields)
    return t


def compile_ref(layout):
    return to_builder(layout).compile()


def to_description(layout):
    """the JSON form boundless_amd.consgen.layout_of takes"""
    names = ("const", "first", "last", "active", "row", "periodic", "word")
    return {"layout": {"stride": layout.stride, "noise_rows": layout.noise_rows, "n_globals": layout.n_globals, "table": list(layout.table),
                       "code": [[names[k], a, b] for k, a, b in layout.code],
                       "fields": [dict(zip(("col", "word", "shift", "bits", "pad"), f)) for f in layout.fields]}}


# ---- layouts ----
def every_kind(noise_rows=1994, stride=3):
    """every code kind, LAST / ACTIVE with and without an offset, a ROW with and without a bound, two PERIODIC windows"""
    t = Layout(stride, noise_rows)
    t.col(CONST, 0).col(CONST, P - 1).col(CONST, 12345).col(FIRST).col(LAST).col(LAST, 1).col(ACTIVE).col(ACTIVE, 1).col(ROW).col(ROW, 1).col(ROW, 5)
    t.periodic([7]).periodic([1, 2, P - 1, 0]).word(SYNTH_CODE_SEED).word(1)
    t.field(0, 0, 0, 8, 3).field(2, stride - 1, 2, 30, (1 << 30) - 1)
    return t


def lookup_code(w_code=4, noise_rows=1994, po2=9):
    """the lookup circuit's code group (include/bx_lookup.h, "code") restated as a layout: first, last, the table below B, control words"""
    t = Layout(1, noise_rows)
    t.col(FIRST).col(LAST).col(ROW, 1 << min(15, po2 - 1))
    for _ in range(3, w_code):
        t.word(LOOKUP_CODE_SEED)
    return t


def synthetic_code(w_code=4):
    """the synthetic circuit's code group (include/bx_prover.h, "code") restated as a layout"""
    t = Layout(1, 1994)
    t.col(FIRST).col(LAST)
    for _ in range(2, w_code):
        t.word(SYNTH_CODE_SEED)
    return t


def no_fields(noise_rows=1994, stride=1):
    return Layout(stride, noise_rows).col(FIRST)


def every_column(w_data, stride, noise_rows=1994, seed=0):
    """a field on every column of a data group of w_data columns, words, shifts, widths and pads drawn from `seed`; shift + bits = 32,
    bits 1 and bits 30 are among them"""
    rng = np.random.default_rng([seed, w_data, stride])
    t = Layout(stride, noise_rows).col(FIRST).col(LAST)
    for c in range(w_data):
        bits = (1, 30, 16)[c] if c < 3 else int(rng.integers(1, 31))
        shift = 32 - bits if c % 2 == 0 else int(rng.integers(0, 33 - bits))
        t.field(c, int(rng.integers(0, stride)), shift, bits, int(rng.integers(0, 1 << bits)))
    return t


def one_word_three_fields(stride=2):
    """a record word feeding three fields (two of them overlapping), and a column between them that no field names"""
    return Layout(stride, 1994).col(FIRST).field(0, stride - 1, 0, 12).field(1, stride - 1, 12, 20, 5).field(3, stride - 1, 4, 16, 65535)


STRIDES = (1, 2, 3, 31, 32, 33, 128)


def records(kind, count, stride, seed=0):
    """`count` records: "random" 32-bit words, "zero", or "ones" (every word 0xFFFFFFFF)"""
    if kind == "zero":
        return np.zeros((count, stride), np.uint32)
    if kind == "ones":
        return np.full((count, stride), 0xFFFFFFFF, np.uint32)
    return np.random.default_rng([seed, count, stride]).integers(0, 1 << 32, (count, stride), dtype=np.uint64).astype(np.uint32)

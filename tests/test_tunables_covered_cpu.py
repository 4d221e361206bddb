"""No GPU: every name bx_set_tunable accepts (csrc/hal.hip) is set by at least one GPU parity test and documented in DESIGN.md §9, so
the next tunable arrives with both.  A text search of the project's own source for its own option names.  And the property of the
C oracle the selectable-path tests lean on: its Horner loop takes a poly_size that is no power of two."""
import glob
import os
import re

import numpy as np

from oracle import np_oracle as npo
from oracle import oracle_lib as ol

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def tunable_names():
    src = open(os.path.join(ROOT, "boundless_amd", "csrc", "hal.hip")).read()
    body = src[src.index('extern "C" const char* bx_set_tunable('):]
    body = body[:body.index("BX_ABI_CATCH")]
    names = re.findall(r'strcmp\(name, "([a-z0-9_]+)"\)', body)
    assert len(names) >= 25 and len(set(names)) == len(names), names
    return names


def missing_from(names, text):
    return [n for n in names if not re.search(r"""["']%s["']""" % re.escape(n), text)]


def test_every_tunable_is_set_by_a_gpu_test():
    text = "".join(open(p).read() for p in sorted(glob.glob(os.path.join(ROOT, "tests", "test_*_gpu.py"))))
    assert missing_from(tunable_names(), text) == [], "tunables no tests/test_*_gpu.py names as a string literal"
    # the search itself: a name that no test sets is reported
    assert missing_from(["fold_quad_wg", "not_a_tunable"], text) == ["not_a_tunable"]


def test_every_tunable_is_in_the_design_table():
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    start = design.index("\n## 9. Tunables")
    section = design[start:design.index("\n## ", start + 1)]
    rows = [line for line in section.splitlines() if line.startswith("|")]
    assert rows and "tested by" in rows[0], "the table of §9 names the test of each tunable"
    undocumented = [n for n in tunable_names() if not any(f"`{n}`" in row.split("|")[1] for row in rows[2:])]
    assert undocumented == []
    assert all(re.search(r"`test_\w+", row.split("|")[-2]) for row in rows[2:]), "every row names a test"


def test_oracle_horner_evaluation_takes_a_ragged_size():
    """bxo_batch_evaluate_any at poly_size = 257 (no power of two, no multiple of anything) against big-integer Horner evaluation by
    the definition (oracle/np_oracle.py), on the second of two polynomials."""
    ol.build()
    size, rng = 257, np.random.default_rng(257)
    coeffs = ol.random_elems(rng, 2 * size)
    x = ol.random_elems(rng, 4)
    out = np.zeros(4, np.uint32)
    ol.lib().bxo_batch_evaluate_any(coeffs, size, np.array([1], np.uint32), x, out, 1)
    canon = [[int(v), 0, 0, 0] for v in ol.decode(coeffs[size:])]
    want = npo.f4_poly_eval(canon, [int(v) for v in ol.decode(x)])
    assert ol.decode(out).tolist() == want

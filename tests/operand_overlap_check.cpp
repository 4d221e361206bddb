// operand_overlap_check — csrc/operands.hpp alone, as a stand-alone host program (built plain and under AddressSanitizer +
// UndefinedBehaviorSanitizer by tests/test_operand_overlap_check_cpu.py): bufs_overlap over the placements the GPU suite puts device
// operands in — empty, touching, one word shared at either end, containment, exact alias — against a byte-by-byte model, and over
// buffers at the ends of the address space, where an implementation that forms `dptr + 4 * len` wraps.
#include <stdint.h>
#include <stdio.h>

#include "operands.hpp"

static int failures = 0;
static bx_buf buf(uintptr_t addr, size_t len) { return bx_buf{(void*)addr, len}; }
static void expect(bool got, bool want, const char* what, uintptr_t a, size_t al, uintptr_t b, size_t bl) {
    if (got != want) {
        printf("FAIL %s: [%#zx, +%zu words) against [%#zx, +%zu words): got %d, want %d\n", what, (size_t)a, al, (size_t)b, bl, (int)got, (int)want);
        ++failures;
    }
}
static void both(uintptr_t a, size_t al, uintptr_t b, size_t bl, bool want, const char* what) {
    expect(bx::bufs_overlap(buf(a, al), buf(b, bl)), want, what, a, al, b, bl);
    expect(bx::bufs_overlap(buf(b, bl), buf(a, al)), want, what, b, bl, a, al);  // symmetric
}
// the definition, in 128-bit arithmetic that cannot wrap: [a, a + 4 al) and [b, b + 4 bl) share a byte
static bool model(uintptr_t a, size_t al, uintptr_t b, size_t bl) {
    typedef unsigned __int128 u128;
    if (!al || !bl) return false;
    const u128 a0 = a, a1 = a0 + (u128)4 * al, b0 = b, b1 = b0 + (u128)4 * bl;
    return a0 < b1 && b0 < a1;
}

int main() {
    const uintptr_t base = 0x7f0000001000ull;
    // empty buffers overlap nothing: not each other, not a buffer they point into, not with a null pointer
    both(base, 0, base, 0, false, "empty / empty");
    both(base + 8, 0, base, 16, false, "empty inside");
    both(0, 0, base, 16, false, "null empty");
    both(base, 0, base, 16, false, "empty at the start");
    // touching: one ends where the other starts
    both(base, 16, base + 64, 16, false, "touching");
    both(base, 1, base + 4, 1, false, "touching single words");
    // one word shared at either end
    both(base, 16, base + 60, 16, true, "one word, upper end");
    both(base + 60, 16, base, 16, true, "one word, lower end");
    both(base, 17, base + 64, 16, true, "one word longer");
    // containment and exact alias
    both(base, 64, base + 16, 8, true, "containment");
    both(base, 64, base, 8, true, "containment at the start");
    both(base, 64, base + 4 * 56, 8, true, "containment at the end");
    both(base, 64, base, 64, true, "exact alias");
    expect(bx::bufs_same(buf(base, 64), buf(base, 64)), true, "same", base, 64, base, 64);
    expect(bx::bufs_same(buf(base, 64), buf(base, 63)), false, "same start, other length", base, 64, base, 63);
    expect(bx::bufs_same(buf(base, 64), buf(base + 4, 64)), false, "same length, other start", base, 64, base + 4, 64);
    // pointers that are not word aligned (never handed out, but the test must still be the interval test): 1 byte shared
    both(base, 1, base + 3, 1, true, "unaligned, one byte shared");
    // the top of the address space: a buffer whose end is 2^64 exactly, and lengths whose byte count wraps
    const uintptr_t top = ~(uintptr_t)0;
    both(top - 63, 16, top - 127, 16, false, "ends at 2^64, touching below");
    both(top - 63, 16, top - 127, 17, true, "ends at 2^64, one word");
    both(top - 63, 16, base, 16, false, "ends at 2^64, far away");
    both(top - 63, 16, top - 63, 16, true, "ends at 2^64, alias");
    both(top - 3, 1, top - 7, 1, false, "last word / the word before");
    both(base, (size_t)1 << 62, base + 4096, 4, true, "4 * len wraps to 0");
    both(base, ((size_t)1 << 62) + 1, base + 4096, 4, true, "4 * len wraps to 4");
    both(base + 4096, 4, base, ~(size_t)0, true, "len = SIZE_MAX");
    both(base, 4, base + 4096, ~(size_t)0, false, "len = SIZE_MAX above");
    // every placement of two short buffers around each other, near 0, in the middle and at the top, against the model
    const uintptr_t origins[] = {0, base, top - 255};
    long checked = 0;
    for (uintptr_t o : origins)
        for (size_t ao = 0; ao < 12; ++ao)
            for (size_t al = 0; al < 6; ++al)
                for (size_t bo = 0; bo < 12; ++bo)
                    for (size_t bl = 0; bl < 6; ++bl) {
                        const uintptr_t a = o + 4 * ao, b = o + 4 * bo;
                        both(a, al, b, bl, model(a, al, b, bl), "sweep");
                        ++checked;
                    }
    if (failures) {
        printf("operand_overlap_check: %d failures\n", failures);
        return 1;
    }
    printf("operand_overlap_check ok (%ld swept placements)\n", checked);
    return 0;
}

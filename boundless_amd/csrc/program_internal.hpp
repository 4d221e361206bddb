// program_internal.hpp — what the two host translation units of the program kinds share (program_compile.cpp: the step-list compiler;
// cons_program_host.cpp: the host executors, the shape checks and the small getters).  Plain C++, no HIP.
#pragma once
#include "cons_program.hpp"

namespace bx {
// A refusal: the formatted message in ONE thread-local buffer (program_compile.cpp), valid until the calling thread's next refusal.
// The compiler, the host executors and the *_check_widths / *_check_counts helpers all write here.
const char* refuse(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
}  // namespace bx

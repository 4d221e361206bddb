/*
 * bx_program.h — constraint programs: a circuit's constraints as DATA.  One description gives both halves a bx_circuit_ops
 * table needs of them: `eval_check` (a gfx950 kernel that interprets the program over the 4N domain, or one generated from the
 * program off line: "Generated kernels" below) and `constraints_at` (a host interpreter for the verifier), plus the tap sets.
 * No device code is written per circuit by hand.
 *
 * Where this comes from
 * ---------------------
 * Upstream's circuits (rv32im, recursion, keccak) ship their constraints as a `PolyExtStepDef`: a flat list of steps (`Const`,
 * `ConstExt`, `Get`, `GetGlobal`, `Add`, `Sub`, `Mul`, `True`, `AndEqz`, `AndCond`) and a return index, interpreted by the
 * verifier's `poly_ext` [EXT: risc0-zkp, recalled; not in the reference tree].  RECALLED AND UNVERIFIED: the step names, the two
 * separately numbered var lists, the operand order of AndEqz / AndCond and their (tot, mul) update rules, and GetGlobal's split
 * into a "global" and a "mix" table.  THE TEXT BELOW, not upstream's, is normative here; an upstream table is translated to
 * it, and any difference found on re-verification is a change to the translator, not to this header.
 *
 * Values (normative)
 * ------------------
 * A program is evaluated over a value field K: on the prover K = Fp at a domain point x = w_4N^row, on the verifier K = Fp4 at Z.
 * There are two separately numbered lists.  fp vars hold values of K (or Fp4 on the prover once an ext constant flowed in); mix
 * vars hold pairs (tot, mul) of Fp4.  Each step appends exactly one entry to exactly one list; operands name EARLIER entries.
 *
 *   step                appends  meaning
 *   CONST a             fp       the field element a (canonical integer < P)
 *   CONST_EXT a b c d   fp       the ext element a + b X + c X^2 + d X^3 (canonical integers < P)
 *   GET a               fp       tap a of the program's tap list: (group 0 code / 1 data / 2 accum, col, back) = that column at
 *                                x * w_N^-back; on the 4N domain this is row - 4 * back mod 4N
 *   GET_GLOBAL a b      fp       a = 0: the public word globals[b];  a = 1: component b < 4 of accumulate's `mix`, as a BASE-field
 *                                element (an ext challenge alpha is rebuilt as sum_k X^k * mix_k through CONST_EXT)
 *   ADD a b, SUB a b, MUL a b    fp       fp[a] + fp[b], fp[a] - fp[b], fp[a] * fp[b]
 *   TRUE                mix      (0, 1)
 *   AND_EQZ a b         mix      x = mix[a], y = fp[b]:                   (x.tot + x.mul * y,  x.mul * poly_mix)
 *   AND_COND a b c      mix      x = mix[a], cond = fp[b], inner = mix[c]: (x.tot + cond * inner.tot * x.mul,  x.mul * inner.mul)
 *
 * The result is mix[ret].tot.  A chain of AND_EQZ from TRUE is exactly sum_i poly_mix^i C_i.
 *
 * Compilation (bx_cons_program_create; host only, no ctx, no GPU)
 * ---------------------------------------------------------------
 *   validation   refused by name: an operand that names a later or missing var or the wrong list; a tap index, tap group, tap
 *                back, global index or mix component out of range; a constant >= P; `ret` not a mix var; more than BX_MAX_TAPS
 *                distinct backs on one column (0 always counts: every column is opened at Z); more than BX_CONS_MAX_STEPS steps.
 *   types        on the prover an fp var is BASE unless a CONST_EXT flows into it; on the verifier everything is ext.  Every
 *                arithmetic step is resolved to a base x base, ext x base or ext x ext opcode; the y of AND_EQZ and the cond of
 *                AND_COND may be either.
 *   mix powers   `mul` is always a statically known power of poly_mix: TRUE 0, AND_EQZ + 1, AND_COND + the inner's.  The
 *                compiler resolves every x.mul to an index into a table of powers; no executor computes a mul.  The exponent
 *                of `ret` is the program's constraint count.
 *   degree       const and global 0, tap 1, add / sub max, mul sum, AND_EQZ max(x, y), AND_COND max(x, cond + inner).  The check
 *                polynomial sum / ((3x)^N - 1) is committed as 4N evaluations: with columns of degree < N a sum of degree d has a
 *                quotient of degree <= d (N - 1) - N, which is below 4N exactly for d <= BX_CONS_MAX_DEGREE = 5 — the bound
 *                bx_prover.h already states for cons_degree.  A program above it is refused.
 *   slots        values live in two bounded files, allocated by last use and reused when freed: NARROW slots (one word; base
 *                values) and WIDE slots (four words; ext values and the tot of a mix var).  A program that needs more live values
 *                than BX_CONS_MAX_NARROW / BX_CONS_MAX_WIDE is refused with the number it needs and the limit.  On the device a
 *                narrow slot is 1 KiB and a wide slot 4 KiB of a workgroup's LDS: 32 + 4 * 24 = 128 KiB of the CU's 160.
 *   output       ONE instruction stream, read by the host executor and by the device kernel alike.
 *
 * Generated kernels (normative)
 * -----------------------------
 * The interpreter pays for every value with an LDS round trip and for every step with a fetch and a dispatch.  A program may
 * instead be given a kernel GENERATED from its compiled stream, built off line and attached to the loaded program; without one
 * the interpreter runs, exactly as before.  Nothing is compiled at run time.
 *
 *   digest       bx_cons_program_digest: SHA-256 over the bytes "bx-cons-program" and then, each as a little-endian 32-bit word,
 *                the ABI number (1), n_globals, the number of mix powers, the result's slot, the length of the stream in words
 *                and the stream, the number of constants and the constants (Montgomery words), the number of taps and
 *                (group, col, back) of every tap.  The 32 bytes are returned as eight little-endian words.  It depends on the
 *                description alone: the same on every machine, different after a change to one constant, tap, step or `ret`.
 *   text         bx_cons_program_emit_hip: one translation unit, a pure function of the compiled program (no time, no path, no
 *                address).  Straight-line code, one statement per instruction of the stream, in stream order: a narrow slot
 *                is a uint32_t local, a wide slot an Fp4 local, so the allocator's 32 + 4 * 24 = 128 live words bound the
 *                kernel's registers.  The arithmetic is the interpreter's (fp_add / fp_sub / fp_mul / fp_neg, f4_add / f4_sub /
 *                f4_scale / f4_mul_lz / f4_zero, same operand order): every value is canonical, canonical words are unique, so
 *                the two executors agree word for word.  Constants are Montgomery-word literals; globals and `mix` are read
 *                from a table of n_globals + 4 words written per call; mix powers from the canonical power table by literal
 *                index.  A tap is one load at group_base + (col << (po2 + 2)) + r_back with r_back = (i - 4 back) & (4N - 1)
 *                computed once per distinct back.  A program of more than 1024 instructions is written as segments of that many,
 *                each a device function of its own that is not inlined (the compiler's time on one function grows faster than
 *                linearly); between two segments the slots go through a struct in memory at fixed offsets.  Such a kernel is
 *                given the whole register file and runs at the lowest occupancy; shorter programs are one function and keep
 *                every slot in a register.  The text includes csrc/cons_program_gen.hpp, the frame: the argument
 *                struct, the accessors, the division by (3x)^N - 1, and two wrappers.  Under hipcc:
 *                    extern "C" __global__ __launch_bounds__(256) void bx_cp_eval(bx_cp_gen_args)
 *                one lane per domain point, lanes past 4N return, no LDS, with the device symbols bx_cp_abi (one word) and
 *                bx_cp_digest (eight).  Under a host compiler: a function that fills the four planes from host arrays.
 *   build        python -m boundless_amd.consgen DESC.json -o OUT.hsaco: hipcc, device only, the library's own flags.
 *   attach       bx_cons_program_attach_kernel.  Refused by name before anything reaches HIP: an image that starts with neither
 *                the ELF magic nor "__CLANG_OFFLOAD_BUNDLE__".  Refused by name with the module unloaded again: a code object
 *                without bx_cp_eval, bx_cp_abi or bx_cp_digest; another ABI number; a digest that is not the loaded program's; a
 *                second attach without a detach.  bx_cons_program_unload and bx_free detach what is still attached.
 *   launch       bx_cons_program_eval_check with a kernel attached: the same argument checks and the same table updates, then
 *                the attached kernel on the ctx's stream, ceil(4N / 256) workgroups of 256 lanes, no dynamic LDS, profiled as
 *                "cons_program_eval_check_gen".
 *
 * Witness programs (normative)
 * ----------------------------
 * The derived columns of a trace are the same kind of object as its constraints: "this data column equals this polynomial of other
 * cells of the same or earlier rows".  A WITNESS PROGRAM is a step list that derives data columns from free ones.  It is evaluated
 * once per trace row r, 0 <= r < N = 2^po2, over Fp only (the prover's K).  It has ONE list, of fp vars, and no mix vars.
 *
 *   step                appends  meaning
 *   CONST a             fp       as above
 *   GET a               fp       tap a of the program's tap list: (group 0 code / 1 data, col, back) = that column at row
 *                                (r - back) mod N, cyclic
 *   ADD a b, SUB a b, MUL a b    fp       as above
 *   SET a b             nothing  data[a][r] = fp[b]                                                   (BX_CONS_SET = 10)
 *
 * A data column the program SETs is DERIVED; every other data column is FREE and must be filled before the program runs.
 * Refused by name at bx_wit_program_create:
 *   ops          CONST_EXT, GET_GLOBAL, TRUE, AND_EQZ and AND_COND do not belong in a witness program.  (Conversely BX_CONS_SET is
 *                refused by bx_cons_program_create, as any unknown op is.)
 *   accum        tap group 2: the accum group does not exist yet when the witness is generated.
 *   one SET      a data column is SET at most once.
 *   forwarding   a GET of a derived column with back == 0, placed AFTER that column's SET, is not a memory read: the compiler
 *                forwards the fp var that was stored (it compiles to nothing).
 *   other rows   a GET of a derived column with back > 0 is refused: lanes are rows, and the other row's value may not have been
 *                written yet.
 *   order        a GET of a derived column placed BEFORE its SET is refused.
 *   limits       BX_CONS_MAX_STEPS, BX_CONS_MAX_TAPS, BX_CONS_MAX_BACK, BX_CONS_MAX_COL, constants < P, operands name earlier
 *                vars, and BX_CONS_MAX_NARROW = 32 live values: a program over it is refused with the number it needs and the
 *                limit.  There are no wide slots, no degree bound and no mix powers.
 * The three rules forwarding / other rows / order mean that no lane ever reads a word another lane of the same run writes.  That
 * is what makes the device kernel barrier-free and its result independent of how lanes, waves and workgroups are scheduled.
 *
 *   global cells an optional list of (global index, data column, row): after the program has run, public word `index` is
 *                data[column][row] as it stands in the buffer, a Montgomery word.  Index < BX_MAX_GLOBALS, each index at most once
 *                (refused at create).  `row` is checked against N when a prover is created: the list is the one shape-dependent
 *                part of a description.
 *   multiplicity columns (normative; bx_wit_program_create_counted)
 *                m(r) = "how many looked-up cells hold table entry r" is a histogram over whole columns: no step list can give it,
 *                because a lane may not read what other lanes write.  A witness program therefore has an optional list of at most
 *                BX_WIT_MAX_COUNTS = 16 COUNTS (col, bins, rows, sources[]):
 *                  col      the data column that receives the multiplicities
 *                  sources  1 .. BX_WIT_MAX_COUNT_SOURCES = 64 data columns.  With rows <= 2^24 a count is at most 2^30 < P: a
 *                           uint32_t bin never wraps and no reduction is needed
 *                  rows     only rows r < rows are counted and written; rows == 0 means all N.  Rows at or above `rows` are neither
 *                           read nor written: they keep what the base's witgen left (the lookup circuit's noise rows)
 *                  bins     B, 1 <= B <= rows, not necessarily a power of two, at most BX_WIT_MAX_COUNT_BINS = 2^24
 *                Meaning: let c(v) be the number of pairs (source column s, row j < rows) whose cell, decoded from Montgomery
 *                form, is the integer v.  After the run data[col][r] holds the value c(r) as a Montgomery word for r < B and the
 *                value 0 for B <= r < rows.  A source cell that decodes to a value >= B is not counted (bx_lookup.h's rule: the
 *                prover does not judge the witness).
 *                Order: all counts run after the per-row program, in list order, on the same stream; a source may therefore be a
 *                free column or a SET column.
 *                Refused by name at create: a count column that is also SET; a count column named by any GET (its value does not
 *                exist while the program runs); a count column that is a source of any count, or the column of two counts; `col` or
 *                a source above BX_CONS_MAX_COL; no sources, or more than 64; a source named twice within one count; bins == 0,
 *                bins > 2^24, rows > 2^24, or rows != 0 && bins > rows; more than 16 counts.
 *                A global cell may name a count column (cells are read after the counts), and an accumulate program may tap one
 *                (`keep` runs after the counts).  A program may consist of counts alone.
 *                `rows` and `bins` against N are shape-dependent, like a cell's row: rows > N, or bins > N with rows == 0, is
 *                refused by name when the program runs and when a prover is created, as is a count column or a source that is not
 *                below the data group's width.
 *                The counts are NOT hashed by bx_wit_program_digest and play no part in bx_wit_program_emit_hip, for the reason the
 *                global cells are not: the per-row kernel does not depend on them, so one code object serves a program under any
 *                count list.  With a kernel attached, bx_wit_program_run launches it and then runs the counts exactly as it does
 *                after the interpreter.
 *                Host: bx_wit_program_run_host runs the counts after the stream with plain loops; counts are integers, so there is
 *                no ordering question and host and device agree word for word.
 *                Device (csrc/wit_count.hip), per count and without blocking: (1) the count's bins are cleared; (2) a histogram
 *                directly over the source columns of `data`, rows [0, rows), with no gathered copy, profiled as
 *                "wit_program_count"; (3) a store to rows [0, rows) of `col`, profiled as "wit_program_count_store".  The histogram
 *                has two forms: for B <= 32 768 (4 B <= 128 KiB) per-workgroup bins in dynamic LDS, 1024 lanes, every non-zero bin
 *                flushed with one global atomic; above that, or with the ctx tunable lookup_hist_lds = 0, global atomics.  In both
 *                the lanes of a wave that hit the first live lane's bin are counted with one ballot and added by one lane.
 *                Out of scope: tables whose entries are not indexed by row (a tuple lookup supplies the index as a source column),
 *                weighted counts, counting code columns.
 *   sorted columns (normative; bx_wit_program_create_sorted)
 *                A permutation or memory-consistency argument (RATIO, "Accumulate programs" below) needs a sorted copy of some
 *                columns as its witness.  No step list can give it, for the reason no step list gives m(r).  A witness program
 *                therefore has an optional list of at most BX_WIT_MAX_SORTS = 8 SORTS (rows, n_keys, bits[], sources[], dests[]):
 *                  sources  1 .. BX_WIT_MAX_SORT_COLS = 16 data columns.  The first n_keys of them (1 .. BX_WIT_MAX_SORT_KEYS = 4) are the
 *                           key, most significant first; the others are payload carried along
 *                  dests    as many data columns as sources: dests[i] receives sources[i], permuted
 *                  bits[k]  1 .. 31: the key of a cell of key column k is the low bits[k] bits of its integer decoded from Montgomery
 *                           form; 31 is the whole value, since P < 2^31.  The prover does not judge the witness: a value at or above
 *                           2^bits is not an error, it sorts by its low bits and the circuit's constraints catch it.  The bits of
 *                           one sort sum to at most BX_WIT_MAX_SORT_BITS = 64
 *                  rows     as in a count: only rows [0, rows) are read and written, rows == 0 means all N, rows at or above
 *                           `rows` keep what they held
 *                Meaning: let pi be the stable sort of rows [0, rows) by the key tuple, lexicographic, ties by ascending row.  After
 *                the run data[dests[i]][r] = data[sources[i]][pi(r)] for r < rows; the source's Montgomery word is copied unchanged.
 *                pi is unique, so host and device agree word for word.
 *                Order, on the one stream: (1) the per-row program (interpreter or attached kernel), (2) all sorts in list order,
 *                (3) all counts.  A source may therefore be a free or a SET column, a count's source may be a dest, a global cell
 *                may name a dest, and an accumulate program may tap one.  A program without sorts enqueues exactly what it did.
 *                Refused by name at create: a dest that is SET, that is named by any GET, that is a count column, that is a source
 *                of any sort, or that is named twice (in one sort or in two); a source that is a count column; a source named
 *                twice within one sort; any column above BX_CONS_MAX_COL; n_keys == 0, n_keys > 4 or n_keys above the number of
 *                sources; no sources, or more than 16; a bits value of 0 or above 31; bits that sum to more than 64; rows > 2^24;
 *                more than 8 sorts.
 *                Shape-dependent, refused by name by bx_wit_program_run_host, by bx_wit_program_run and when a prover is created,
 *                with nothing written: rows > N; a source or dest that is not below the data group's width.
 *                Like counts and global cells the sorts are NOT hashed by bx_wit_program_digest and play no part in
 *                bx_wit_program_emit_hip: one code object serves a program under any sort list.  bx_wit_program_derives answers 1
 *                for a dest.
 *                Host: bx_wit_program_run_host runs the sorts after the stream and before the counts, std::stable_sort on the
 *                decoded, masked key tuples, gathered into a temporary before anything is written.
 *                Device (csrc/wit_sort.hip), per sort and without blocking, a stable LSD radix sort: (1) PACK, the key columns
 *                decoded once into one uint64_t composite key per row, most significant key in the high bits, with idx[r] = r,
 *                profiled as "wit_program_sort_pack"; (2) ceil(sum of bits / 8) stable passes of 8-bit digits, least significant
 *                first, over (key, idx) pairs, ping-pong between two buffers, profiled together as "wit_program_sort": a per-tile
 *                digit histogram (256 LDS bins, written digit-major [digit][tile]), an exclusive scan of that table, and a stable
 *                scatter to base[digit][tile] + rank (the rank within a wave from a ballot match on the digit's 8 bits, across waves
 *                and trips from per-wave counters in LDS taken in tile order); (3) GATHER, dests[i][r] = sources[i][idx[r]] for every
 *                source in one launch, profiled as "wit_program_sort_gather".  The pair buffers and the digit table belong to the
 *                loaded program: sized at the first run that needs more than is there, released by bx_wit_program_unload and
 *                bx_free; a second run at the same shape allocates nothing.
 *                Out of scope: a second per-row pass after the sorts (differences of sorted cells are the constraints' business,
 *                through `back`); descending order; keys in the code group; a built-in memory circuit.
 *   compiled     the instruction stream of a constraint program restricted to the narrow opcodes, plus one: a store of a
 *                narrow slot to a data column.  bx_wit_program_run_host and the device kernel read the same stream and use the
 *                same canonical arithmetic, so they give identical words.
 *   device       bx_wit_program_run: one lane per row, 256 per workgroup, the slot file in LDS (1 KiB per slot, at most 32 KiB),
 *                profiled as "wit_program_run".  A tap is col[(r - back) & (N - 1)]; a store is data[col * N + r].
 *   composite    bx_cons_circuit_set_witness: the table's witgen calls base->witgen (which fills the free cells; whatever it
 *                leaves in derived columns is overwritten), runs the program on `code` and `data`, and then reads the global
 *                cells back with one blocking gather into globals_out, overriding the base's words at those indices.
 * Out of scope: free-cell generators and code groups from data.  A column that depends on its own earlier rows is an accumulator and
 * belongs to an accumulate program ("Accumulate programs" below): prefix_products / logup_accumulate.
 *
 * Accumulate programs (normative)
 * -------------------------------
 * The third circuit-specific stage, bx_circuit_ops::accumulate, fills the accum group with running sums (LogUp) and running products
 * (grand products) of per-row terms.  The scans are the HAL's (bx_logup_accumulate, bx_batch_prefix_products); what differs per circuit
 * is the terms in front of them.  An ACCUMULATE PROGRAM is a step list that gives those terms.  It is evaluated once per trace row r,
 * 0 <= r < N = 2^po2, on the prover only, after the data commit, with accumulate's `mix` known.  It has ONE list, of fp vars, and no mix
 * vars.  Types are those of a constraint program on the prover: a var is BASE unless a CONST_EXT flows into it.
 *
 *   step                appends  meaning
 *   CONST a, CONST_EXT a b c d, ADD a b, SUB a b, MUL a b    fp    as in constraint programs (base x base, ext x base, ext x ext
 *                                resolved by the compiler)
 *   GET a               fp       tap a of the program's tap list: (group 0 code / 1 data, col, back) = that column at row
 *                                (r - back) mod N, cyclic, as in witness programs
 *   GET_GLOBAL 0 b / GET_GLOBAL 1 b    fp    public word b / base-field component b of `mix`, as in constraint programs
 *   SUM s m d           nothing  sequence s is a running sum: acc_s[r] = sum_{j <= r} fp[m](j) / fp[d](j).  m must be BASE (it becomes a
 *                                `mults` word of bx_logup_accumulate); d is base or ext.  A zero denominator contributes zero (the
 *                                HAL's rule).                                                              (BX_CONS_SUM = 11)
 *   PROD s a            nothing  sequence s is a running product: acc_s[r] = prod_{j <= r} fp[a](j); a is base or ext.
 *                                                                                                          (BX_CONS_PROD = 12)
 *   RATIO s a b         nothing  sequence s is a running product of ratios: acc_s[r] = prod_{j <= r} fp[a](j) / fp[b](j), what a
 *                                permutation or memory-consistency argument accumulates (z(N-1) = 1 iff the multisets agree).  a and b
 *                                are base or ext; a base value is promoted.  A zero denominator contributes the factor 0 (the HAL's
 *                                rule, bx_batch_ratio_products): the sequence is 0 from that row on.  The prover does not judge the
 *                                witness.                                      (BX_CONS_RATIO = 16; 13, 14 and 15 are no ops)
 * Operands in bx_cons_step: SUM has a = s, b = m, c = d; PROD has a = s, b = a; RATIO has a = s, b = the numerator, c = the denominator.
 * Sequence s, component k is accum column 4 s + k.  With S sequences the program does not touch accum columns at or above 4 S.
 * Refused by name at bx_acc_program_create:
 *   ops          TRUE, AND_EQZ, AND_COND and SET do not belong in an accumulate program.  (BX_CONS_SUM, BX_CONS_PROD and BX_CONS_RATIO
 *                stay unknown ops to bx_cons_program_create and bx_wit_program_create; 13, 14 and 15 are unknown to all three.)
 *   accum        tap group 2: the program produces the accum group, it does not read it.
 *   m            an ext-typed m of a SUM.
 *   sequences    a sequence defined twice; a gap (the sequences must be exactly 0 .. S-1); S = 0; a sequence number at or above
 *                BX_ACC_MAX_SEQS = 1024; a PROD sequence numbered below a SUM sequence; a RATIO sequence numbered below a SUM or a
 *                PROD sequence, i.e. a SUM or PROD numbered above a RATIO (all sums come first, then all products, then all ratios,
 *                so that each scan is ONE batched call over a contiguous range).  The rules for twice, gap and the bound cover all
 *                three kinds.
 *   limits       BX_CONS_MAX_STEPS, BX_CONS_MAX_TAPS, BX_CONS_MAX_BACK, BX_CONS_MAX_COL, n_globals <= BX_MAX_GLOBALS, constants < P,
 *                operands name earlier vars, and BX_CONS_MAX_NARROW / BX_CONS_MAX_WIDE live values: a program over one is refused
 *                with the number it needs and the limit.  There is no degree bound and there are no mix powers.
 *
 *   kept columns the prover interpolates `code` and `data` in place right after witgen (bx_circuit.h), so the columns a program taps
 *                are copied before that.  The compiler numbers the distinct (group, col) pairs of the tap list 0 .. K-1 in order of
 *                first appearance in that list; bx_acc_program_kept lists them; the compiled tap table names the kept index.
 *   compiled     the instruction stream of a constraint program without the mix opcodes, plus four appended after CP_ST (so that no
 *                existing stream, digest or generated text changes): a term store for a sum with a base or an ext denominator and for a
 *                product of base or ext factors, the sequence in `imm`.  `scal` = [globals | mix (4) | constants].  A generated kernel
 *                per program is not part of this; the stream is what it would be generated from, as for the other two kinds.
 *                Two more are appended after those four, for the same reason: the store of a RATIO's base or ext denominator.  A
 *                RATIO compiles to a product's term store for its numerator (imm = s) and a denominator store with imm = S + t,
 *                t the ratio's index among the R ratios.  The work space of the terms therefore holds S + R sequences: [0, S) are
 *                the terms, [S, S + R) the denominators of sequences [S - R, S).  bx_acc_program_ratios gives R; info.sequences
 *                counts all three kinds.  A program without RATIO compiles to exactly the stream it had.
 *   host         bx_acc_program_run_host, the definition-level twin: the terms of every row, then the Fp4 inverse with 0 -> 0 times m
 *                (a SUM) or times the numerator (a RATIO), the running sums and products, then columns 4 s + k.  Canonical arithmetic in the kernel's operand order, and canonical
 *                words are unique, so host and device agree word for word.
 *   device       bx_acc_program_keep: ONE launch that gathers the K kept columns into the caller's `kept` (K x N), profiled as
 *                "acc_program_keep".  bx_acc_program_run: (1) the interpreting kernel, one lane per row, 256 per workgroup, slot
 *                files in LDS, writes every term as ONE 16-byte store at run_ext[4 (s N + r)] (a base value is promoted to
 *                (v, 0, 0, 0)) and for a sum one word at mults[s N + r], profiled as "acc_program_run"; (2) ONE bx_logup_accumulate
 *                over sequences [0, sums), in place; (3) ONE bx_batch_prefix_products over [sums, S - R) and ONE
 *                bx_batch_ratio_products over [S - R, S), in place, with the denominators [S, S + R); (4) the transposition of the
 *                first S ext runs into accum columns [0, 4 S), profiled as "acc_program_store".  Columns at or above 4 S are not
 *                written.  run_ext holds 4 N (S + R) words.
 *                A tap is kept[k N + ((r - back) & (N - 1))].  Nothing blocks.
 *   composite    bx_cons_circuit_set_accumulate: the table's witgen ends with bx_acc_program_keep (after the witness program, if
 *                any) and remembers the public words; its accumulate calls base->accumulate when the base has one (that call owns
 *                filler and every column at or above 4 S; whatever it leaves below 4 S is overwritten) and then bx_acc_program_run.
 * Out of scope: a generated kernel per accumulate program; fusing the terms into the scan's tile load.
 *
 * Generated witness kernels (normative)
 * -------------------------------------
 * As a constraint program, a witness program may be given a kernel GENERATED from its compiled stream, built off line and attached
 * to the loaded program; without one the interpreter runs, exactly as before.  Nothing is compiled at run time.
 *
 *   digest       bx_wit_program_digest: SHA-256 over the bytes "bx-wit-program" and then, each as a little-endian 32-bit word, the
 *                ABI number BX_WP_ABI (1), the length of the stream in words and the stream, the number of constants and the
 *                constants (Montgomery words), the number of taps and (group, col, back) of every tap, the number of SETs and the
 *                SET columns in the order of their SETs.  Eight little-endian words.  The global cells are NOT hashed: the kernel
 *                does not depend on them (they are read back by the composite table after the run), so one code object serves a
 *                program under any cell list.
 *   text         bx_wit_program_emit_hip, with the contract of bx_cons_program_emit_hip: a NULL buffer asks for the size, a cap
 *                below it is refused and nothing is written.  One translation unit, a pure function of the compiled program.
 *                Straight-line code, one statement per instruction of the stream, in stream order; a narrow slot is a uint32_t
 *                local, so the allocator's 32 slots bound the kernel's registers.
 *                    CP_LD_B      a Montgomery-word literal: a witness program's `scal` table is its constants alone, so nothing is
 *                                 read per call
 *                    CP_TAP       at.code(col, r<back>) or at.data(col, r<back>), with r<back> = (r - back) & (N - 1) computed once
 *                                 per distinct back of a function
 *                    CP_ADD_BB, CP_SUB_BB, CP_MUL_BB   fp_add, fp_sub, fp_mul in the interpreter's operand order: canonical words,
 *                                 so the kernel, the interpreter and bx_wit_program_run_host agree word for word
 *                    CP_ST        at.store(col, n<a>)
 *                Any other opcode (the padding CP_NOP is no statement), a slot >= info.narrow, a tap or constant index outside
 *                the program's tables, a tap group other than 0 or 1, or a store to a column above the program's largest SET
 *                column is refused as "corrupt instruction stream".  A program of more than 1024 statements is
 *                written as segment functions that are not inlined, the narrow slots going through a struct in memory between
 *                two segments, exactly as for a constraint program.  The text includes csrc/wit_program_gen.hpp, the frame (a
 *                file of its own, so that no generated constraint text's include changes):
 *                    struct bx_wp_gen_args { uint32_t* data; const uint32_t* code; uint32_t n, po2; }  and BX_WP_ABI
 *                a device and a host accessor, and two wrappers.  Under hipcc:
 *                    extern "C" __global__ __launch_bounds__(256) void bx_wp_run(bx_wp_gen_args)
 *                one lane per row, lanes with r >= n return, no LDS, no barrier, with the device symbols bx_wp_abi (one word) and
 *                bx_wp_digest (eight).  Under a host compiler: bx_wp_run_host(args) over all rows.  Column offsets are
 *                (size_t)col << po2, wave-uniform.  No inline assembly, no per-lane array indexed at run time.
 *   aliasing     the three rules forwarding / other rows / order guarantee that no word a launch writes is read by any lane of it.
 *                The device accessor therefore reads taps through a const __restrict__ pointer and stores through a second
 *                __restrict__ pointer to the same buffer: every modified word is accessed through the store pointer only
 *                (the argument is written out in the frame).
 *   build        python -m boundless_amd.consgen --witness DESC.json -o OUT.hsaco: hipcc, device only, the library's own flags.
 *   attach       bx_wit_program_attach_kernel, in the order of bx_cons_program_attach_kernel.  Refused by name before anything
 *                reaches HIP: an image that starts with neither the ELF magic nor "__CLANG_OFFLOAD_BUNDLE__".  Refused by name with
 *                the module unloaded again: a code object without the kernel bx_wp_run, without bx_wp_abi or bx_wp_digest; another
 *                ABI number; a digest that is not the loaded program's ("digest mismatch"); a second attach without a detach
 *                ("already attached").  bx_wit_program_unload and bx_free unload what is still attached.
 *   launch       bx_wit_program_run with a kernel attached: the same argument checks in the same order with the same messages,
 *                then the attached kernel on the ctx's stream, ceil(N / 256) workgroups of 256 lanes, no dynamic LDS, not
 *                blocking, profiled as "wit_program_run_gen".
 *   composite    bx_cons_circuit_set_witness_kernel: the table copies the image; its create attaches it right after it has loaded
 *                the witness program and fails with attach's message if it is refused.  A kernel without a witness program is
 *                refused by name at create.
 */
#ifndef BX_PROGRAM_H
#define BX_PROGRAM_H
#include "bx_circuit.h"
#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

#define BX_CONS_MAX_STEPS 65536 /* steps of one program */
#define BX_CONS_MAX_TAPS 4096   /* entries of a program's tap list */
#define BX_CONS_MAX_BACK 65535  /* largest `back` of a tap */
#define BX_CONS_MAX_COL 65535   /* largest column of a tap (group widths are below 65536) */
#define BX_CONS_MAX_DEGREE 5    /* see "degree" above */
#define BX_CONS_MAX_NARROW 32   /* live base values */
#define BX_CONS_MAX_WIDE 24     /* live ext values and mix tots */
#define BX_ACC_MAX_SEQS 1024    /* sequences of one accumulate program */
#define BX_WIT_MAX_COUNTS 16    /* multiplicity columns of one witness program */
#define BX_WIT_MAX_COUNT_SOURCES 64       /* source columns of one count */
#define BX_WIT_MAX_COUNT_BINS (1u << 24) /* bins of one count */
#define BX_WIT_MAX_SORTS 8      /* sorts of one witness program */
#define BX_WIT_MAX_SORT_COLS 16 /* source columns (keys and payload) of one sort */
#define BX_WIT_MAX_SORT_KEYS 4  /* key columns of one sort */
#define BX_WIT_MAX_SORT_BITS 64 /* key bits of one sort, all keys together */

enum bx_cons_op {
    BX_CONS_CONST = 0,
    BX_CONS_CONST_EXT = 1,
    BX_CONS_GET = 2,
    BX_CONS_GET_GLOBAL = 3,
    BX_CONS_ADD = 4,
    BX_CONS_SUB = 5,
    BX_CONS_MUL = 6,
    BX_CONS_TRUE = 7,
    BX_CONS_AND_EQZ = 8,
    BX_CONS_AND_COND = 9,
    BX_CONS_SET = 10, /* witness programs only ("Witness programs" above) */
    BX_CONS_SUM = 11, /* accumulate programs only ("Accumulate programs" above) */
    BX_CONS_PROD = 12, /* likewise */
    /* 13, 14 and 15 are no ops: every compiler answers them "unknown op" */
    BX_CONS_RATIO = 16 /* accumulate programs only */
};

/* one step: `op` and its operands in the order of the table above (unused operands are ignored) */
typedef struct bx_cons_step {
    uint32_t op;
    uint32_t a, b, c, d;
} bx_cons_step;

typedef struct bx_cons_tap {
    uint32_t group; /* 0 code, 1 data, 2 accum */
    uint32_t col;
    uint32_t back;
} bx_cons_tap;

typedef struct bx_cons_program_desc {
    const bx_cons_step* steps;
    size_t n_steps;
    const bx_cons_tap* taps;
    size_t n_taps;
    uint32_t n_globals; /* public words the program may name: GET_GLOBAL 0 b needs b < n_globals <= BX_MAX_GLOBALS */
    uint32_t ret;       /* the mix var whose tot is the result */
} bx_cons_program_desc;

typedef struct bx_cons_program_info {
    uint32_t steps;
    uint32_t constraints; /* the exponent of poly_mix at `ret` */
    uint32_t degree;
    uint32_t narrow; /* slots used */
    uint32_t wide;
    uint32_t instructions; /* of the compiled stream */
    uint32_t taps;
    uint32_t n_globals;
} bx_cons_program_info;

typedef struct bx_cons_program bx_cons_program;         /* a compiled program (host) */
typedef struct bx_cons_program_dev bx_cons_program_dev; /* ... loaded on a ctx */
typedef struct bx_cons_circuit bx_cons_circuit;         /* a bx_circuit_ops made of a program and a base table */

/* Validates and compiles `desc` (nothing of it is referenced afterwards).  NULL = ok; the message of a refusal lives in a
 * thread-local buffer until the calling thread's next refusal. */
const char* bx_cons_program_create(const bx_cons_program_desc* desc, bx_cons_program** out);
void bx_cons_program_destroy(bx_cons_program* prog);
const char* bx_cons_program_info_get(const bx_cons_program* prog, bx_cons_program_info* out);
/* The tap set of a column in the form bx_circuit_ops::taps wants: strictly increasing, backs_out[0] == 0, {0} for a column the
 * program never names.  Returns the count, 1..BX_MAX_TAPS. */
uint32_t bx_cons_program_taps(const bx_cons_program* prog, int group, uint32_t col, uint32_t backs_out[BX_MAX_TAPS]);

/* Host executor (the verifier's side): the compiled stream over Fp4, tap values from `taps`.  `globals` holds the program's
 * n_globals Montgomery words (may be NULL when that is 0).  A tap the reader refuses reads as zero, evaluation goes on and the
 * reader's message is returned with the result.  No mutable global state: callable from several threads at once. */
const char* bx_cons_program_constraints_at(const bx_cons_program* prog, const bx_tap_reader* taps, const uint32_t poly_mix[4], const uint32_t mix[4],
                                           const uint32_t* globals, uint32_t out[4]);

/* Uploads the stream, the constant table and the tap descriptors once.  bx_free releases what is still loaded on its ctx. */
const char* bx_cons_program_load(bx_ctx* ctx, const bx_cons_program* prog, bx_cons_program_dev** out);
const char* bx_cons_program_unload(bx_cons_program_dev* dev);
/* The contract of bx_circuit_ops::eval_check: the four check planes (check.len = 16N) of result(x) / ((3x)^N - 1) over
 * x = w_4N^row, N = 2^po2, po2 in [1, 24].  The three evaluation buffers are 4N x width column-major.  Refused: lengths that do not
 * match, a tap column that is not below its group's width, n_globals below the program's.  `n_globals` is the length of `globals`
 * (the table's eval_check has no such argument; it is here so that a short array is refused, not read past its end).
 * Each call writes `globals`, `mix` and the powers of `poly_mix` into tables that belong to `dev`, on the ctx's stream: a loaded
 * program serves one stream, its calls in order (a ctx has one stream, so that holds for every caller today).  To run one program
 * from two ctxs, load it on each. */
const char* bx_cons_program_eval_check(bx_ctx* ctx, bx_cons_program_dev* dev, uint32_t po2, bx_buf check, bx_buf code_eval, uint32_t w_code,
                                       bx_buf data_eval, uint32_t w_data, bx_buf accum_eval, uint32_t w_accum, const uint32_t poly_mix[4],
                                       const uint32_t mix[4], const uint32_t* globals, uint32_t n_globals);

/* Generated kernels (see the section of that name above).  The digest of the compiled form, eight words. */
const char* bx_cons_program_digest(const bx_cons_program* prog, uint32_t out[8]);
/* The generated translation unit as NUL-terminated text.  *need receives its size with the NUL.  buf == NULL only asks for
 * that size.  A cap below *need is refused and nothing is written; nothing is ever written past cap. */
const char* bx_cons_program_emit_hip(const bx_cons_program* prog, char* buf, size_t cap, size_t* need);
/* Attaches the code object `image` (len bytes: an ELF code object or a clang offload bundle; not referenced afterwards) to a
 * loaded program, whose eval_check then launches it; detach drains the stream and unloads it, and is refused when nothing is
 * attached.  kernel_attached: 1 or 0. */
const char* bx_cons_program_attach_kernel(bx_cons_program_dev* dev, const void* image, size_t len);
const char* bx_cons_program_detach_kernel(bx_cons_program_dev* dev);
int bx_cons_program_kernel_attached(const bx_cons_program_dev* dev);

/* A bx_circuit_ops whose taps, eval_check and constraints_at come from `prog` and whose normalize, n_globals, create / destroy,
 * code_group, witgen, accumulate, set_noise_seed and check_code are forwarded to `base` with base->user (base's own taps,
 * eval_check and constraints_at may be NULL).  Its create loads the program on the ctx and checks it against the shape: tap
 * columns within the widths, the program's n_globals equal to the base's.  `base` and `prog` must outlive the table, the table
 * its provers.  It is a plug-in table: its code group is committed for every proof. */
const char* bx_cons_circuit_create(const bx_circuit_ops* base, const bx_cons_program* prog, bx_cons_circuit** out);
/* Copies a generated kernel's code object into the table: its create attaches it right after loading the program, and fails
 * with attach_kernel's message if it is refused.  len == 0 goes back to the interpreter.  Set before a prover is created. */
const char* bx_cons_circuit_set_kernel(bx_cons_circuit* cc, const void* image, size_t len);
const bx_circuit_ops* bx_cons_circuit_ops(bx_cons_circuit* cc);
void bx_cons_circuit_destroy(bx_cons_circuit* cc);

/* ---- witness programs (the section of that name above) ---- */
typedef struct bx_wit_global_cell {
    uint32_t global, col, row; /* public word `global` = data[col][row] after the program has run */
} bx_wit_global_cell;

typedef struct bx_wit_program_desc {
    const bx_cons_step* steps;
    size_t n_steps;
    const bx_cons_tap* taps;
    size_t n_taps;
    const bx_wit_global_cell* cells;
    size_t n_cells;
} bx_wit_program_desc;

typedef struct bx_wit_program_info {
    uint32_t steps;
    uint32_t sets;         /* derived columns */
    uint32_t narrow;       /* slots used */
    uint32_t instructions; /* of the compiled stream: a forwarded GET has none */
    uint32_t taps;
    uint32_t cells;
} bx_wit_program_info;

typedef struct bx_wit_program bx_wit_program;         /* a compiled witness program (host) */
typedef struct bx_wit_program_dev bx_wit_program_dev; /* ... loaded on a ctx */

/* Validates and compiles `desc` (nothing of it is referenced afterwards); host only.  NULL = ok; a refusal's message lives in a
 * thread-local buffer until the calling thread's next refusal. */
const char* bx_wit_program_create(const bx_wit_program_desc* desc, bx_wit_program** out);
void bx_wit_program_destroy(bx_wit_program* prog);
const char* bx_wit_program_info_get(const bx_wit_program* prog, bx_wit_program_info* out);
/* 1 if the program sets data column `col`, fills it as a multiplicity column or writes it as the dest of a sort, else 0 */
int bx_wit_program_derives(const bx_wit_program* prog, uint32_t col);
/* Multiplicity columns ("multiplicity columns" above).  One count: data[col][r] = the number of cells of the `sources` columns, rows
 * [0, rows), that hold the integer r, for r < bins; 0 for bins <= r < rows; rows == 0 means all N rows. */
typedef struct bx_wit_count {
    uint32_t col, bins, rows, n_sources;
    const uint32_t* sources;
} bx_wit_count;
/* bx_wit_program_create with a count list (nothing of it is referenced afterwards); with n_counts == 0 it is exactly
 * bx_wit_program_create. */
const char* bx_wit_program_create_counted(const bx_wit_program_desc* desc, const bx_wit_count* counts, size_t n_counts, bx_wit_program** out);
/* the number of counts */
uint32_t bx_wit_program_counts(const bx_wit_program* prog);
/* count i: its column, bins and rows, the number of its sources in *n_sources and the first min(cap, *n_sources) of them in
 * sources_out (which may be NULL when cap is 0) */
const char* bx_wit_program_count_get(const bx_wit_program* prog, uint32_t i, uint32_t* col, uint32_t* bins, uint32_t* rows, uint32_t* sources_out, uint32_t cap,
                                     uint32_t* n_sources);
/* Sorted columns ("sorted columns" above).  One sort: rows [0, rows) of the n_cols `sources` columns, stably sorted by the low bits[k]
 * bits of the first n_keys of them (most significant first), go to the `dests` columns; rows == 0 means all N rows. */
typedef struct bx_wit_sort {
    uint32_t rows, n_keys, n_cols;
    const uint32_t* bits;    /* n_keys */
    const uint32_t* sources; /* n_cols: keys first, then payload */
    const uint32_t* dests;   /* n_cols */
} bx_wit_sort;
/* bx_wit_program_create_counted with a sort list (nothing of it is referenced afterwards); with n_sorts == 0 it is exactly
 * bx_wit_program_create_counted. */
const char* bx_wit_program_create_sorted(const bx_wit_program_desc* desc, const bx_wit_count* counts, size_t n_counts, const bx_wit_sort* sorts, size_t n_sorts,
                                         bx_wit_program** out);
/* the number of sorts */
uint32_t bx_wit_program_sorts(const bx_wit_program* prog);
/* sort i: its rows, its n_keys bits in bits_out, the number of its columns in *n_cols and the first min(cap, *n_cols) sources and
 * dests in sources_out and dests_out (which may be NULL when cap is 0) */
const char* bx_wit_program_sort_get(const bx_wit_program* prog, uint32_t i, uint32_t* rows, uint32_t* n_keys, uint32_t bits_out[BX_WIT_MAX_SORT_KEYS],
                                    uint32_t* sources_out, uint32_t* dests_out, uint32_t cap, uint32_t* n_cols);
/* Host executor, the reference for the device kernel: the compiled stream over the N = 2^po2 rows of host arrays, column-major
 * (code: w_code x N, data: w_data x N Montgomery words), `data` in place; the sorts after the stream, the counts after the sorts.
 * po2 in [1, 24].  Refused with nothing written: a tap or SET column that is not below its group's width, a sort's source or dest
 * that is not below w_data, a sort's rows > N, a count column or source that is not below w_data, a count's rows > N, or bins > N
 * with rows == 0.  No mutable global state. */
const char* bx_wit_program_run_host(const bx_wit_program* prog, uint32_t po2, const uint32_t* code, uint32_t w_code, uint32_t* data, uint32_t w_data);
/* Uploads the stream, the constants, the tap descriptors and the counts' source table once, and allocates the counts' bins.
 * bx_free releases what is still loaded on its ctx. */
const char* bx_wit_program_load(bx_ctx* ctx, const bx_wit_program* prog, bx_wit_program_dev** out);
const char* bx_wit_program_unload(bx_wit_program_dev* dev);
/* Derives the program's columns of `data` on the ctx's stream, then writes its sorted columns, then fills its multiplicity columns;
 * does not block.  po2 in [1, 24], code.len == w_code * N, data.len == w_data * N.  Refused with nothing enqueued: lengths that do
 * not match, a tap or SET column that is not below its group's width, `code` and `data` sharing a byte ("Operand overlap",
 * bx_hal.h), and then a sort's source or dest that is not below w_data, a sort's rows > N, a count column or source that is not
 * below w_data, a count's rows > N, or bins > N with rows == 0.  The bins and the sorts' work space belong to `dev` (the work space
 * grows at the first run that needs more): a loaded program serves one stream, its calls in order. */
const char* bx_wit_program_run(bx_ctx* ctx, bx_wit_program_dev* dev, uint32_t po2, bx_buf code, uint32_t w_code, bx_buf data, uint32_t w_data);
/* The table's witgen then runs `wit` after base->witgen and takes the global cells from the trace ("composite" above); its create
 * loads the program on the ctx and refuses by name a SET or tap column beyond the shape's widths, a cell row >= N, a cell index
 * >= the base's n_globals, a count column or source beyond w_data, a count's rows or bins above N, a sort's source or dest beyond w_data and a sort's rows above N.  NULL goes back to forwarding witgen to `base` alone.  `wit` must outlive the table.  Set before a
 * prover is created. */
const char* bx_cons_circuit_set_witness(bx_cons_circuit* cc, const bx_wit_program* wit);

/* Generated witness kernels (see the section of that name above).  The digest of the compiled form, eight words. */
const char* bx_wit_program_digest(const bx_wit_program* prog, uint32_t out[8]);
/* The generated translation unit as NUL-terminated text, with the contract of bx_cons_program_emit_hip: *need receives its size
 * with the NUL, buf == NULL only asks for that size, a cap below *need is refused and nothing is written. */
const char* bx_wit_program_emit_hip(const bx_wit_program* prog, char* buf, size_t cap, size_t* need);
/* Attaches the code object `image` (len bytes; not referenced afterwards) to a loaded witness program, whose run then launches it;
 * detach drains the stream and unloads it, and is refused when nothing is attached.  kernel_attached: 1 or 0. */
const char* bx_wit_program_attach_kernel(bx_wit_program_dev* dev, const void* image, size_t len);
const char* bx_wit_program_detach_kernel(bx_wit_program_dev* dev);
int bx_wit_program_kernel_attached(const bx_wit_program_dev* dev);
/* Copies a generated witness kernel's code object into the table: its create attaches it right after loading the witness program,
 * and fails with attach_kernel's message if it is refused, or by name if no witness program is set.  len == 0 goes back to the
 * interpreter.  Set before a prover is created. */
const char* bx_cons_circuit_set_witness_kernel(bx_cons_circuit* cc, const void* image, size_t len);

/* ---- accumulate programs (the section of that name above) ---- */
typedef struct bx_acc_program_desc {
    const bx_cons_step* steps;
    size_t n_steps;
    const bx_cons_tap* taps;
    size_t n_taps;
    uint32_t n_globals; /* public words the program may name: GET_GLOBAL 0 b needs b < n_globals <= BX_MAX_GLOBALS */
} bx_acc_program_desc;

typedef struct bx_acc_program_info {
    uint32_t steps;
    uint32_t sequences;    /* S */
    uint32_t sums;         /* sequences [0, sums) are running sums, [sums, S) running products */
    uint32_t instructions; /* of the compiled stream */
    uint32_t narrow;       /* slots used */
    uint32_t wide;
    uint32_t taps;
    uint32_t kept; /* K: distinct tapped (group, col) pairs */
    uint32_t n_globals;
} bx_acc_program_info;

typedef struct bx_acc_program bx_acc_program;         /* a compiled accumulate program (host) */
typedef struct bx_acc_program_dev bx_acc_program_dev; /* ... loaded on a ctx */

/* Validates and compiles `desc` (nothing of it is referenced afterwards); host only.  NULL = ok; a refusal's message lives in a
 * thread-local buffer until the calling thread's next refusal. */
const char* bx_acc_program_create(const bx_acc_program_desc* desc, bx_acc_program** out);
void bx_acc_program_destroy(bx_acc_program* prog);
const char* bx_acc_program_info_get(const bx_acc_program* prog, bx_acc_program_info* out);
/* kept column i < info.kept: its group (0 code, 1 data) and column */
const char* bx_acc_program_kept(const bx_acc_program* prog, uint32_t i, uint32_t* group, uint32_t* col);
/* R, the number of RATIO sequences: sequences [S - R, S) of info.sequences (which counts all three kinds).  Not a field of
 * bx_acc_program_info, whose layout stays what it was. */
const char* bx_acc_program_ratios(const bx_acc_program* prog, uint32_t* out);
/* Host executor, the reference for the device path: host arrays, column-major (code: w_code x N, data: w_data x N, accum: w_accum x N
 * Montgomery words); `globals` holds the program's n_globals words (may be NULL when that is 0), `mix` four.  Writes accum columns
 * [0, 4 S) and nothing else.  po2 in [1, 24].  Refused: a kept column that is not below its group's width, w_accum < 4 S. */
const char* bx_acc_program_run_host(const bx_acc_program* prog, uint32_t po2, const uint32_t* code, uint32_t w_code, const uint32_t* data, uint32_t w_data,
                                    const uint32_t* globals, const uint32_t mix[4], uint32_t* accum, uint32_t w_accum);
/* Uploads the stream, the constants, the tap and kept tables once.  bx_free releases what is still loaded on its ctx. */
const char* bx_acc_program_load(bx_ctx* ctx, const bx_acc_program* prog, bx_acc_program_dev** out);
const char* bx_acc_program_unload(bx_acc_program_dev* dev);
/* Gathers the K kept columns of `code` (w_code x N) and `data` (w_data x N) into `kept` (K x N, kept column i at words [i N, i N + N));
 * one launch, does not block.  Refused with nothing enqueued: another ctx's program, po2 outside [1, 24], lengths that do not match,
 * a kept column that is not below its group's width, `kept` sharing a byte with `code` or `data`. */
const char* bx_acc_program_keep(bx_ctx* ctx, bx_acc_program_dev* dev, uint32_t po2, bx_buf code, uint32_t w_code, bx_buf data, uint32_t w_data, bx_buf kept);
/* The whole stage from `kept`: terms, scans, columns [0, 4 S) of `accum` (w_accum x N); does not block.  `globals` is a HOST array of the
 * program's n_globals words (may be NULL when that is 0).  run_ext (4 N (S + R) words, R = bx_acc_program_ratios, 16-byte aligned) and
 * mults (N sums words) are the caller's work space.  Refused with nothing enqueued: another ctx's program, po2 outside [1, 24],
 * kept.len != K N, run_ext.len != 4 N (S + R), mults.len != N sums, accum.len != N w_accum, w_accum < 4 S, a misaligned run_ext, any two of run_ext, mults, accum and kept sharing a
 * byte ("Operand overlap", bx_hal.h).  Each call writes `globals` and `mix` into a table that belongs to `dev`, on the ctx's stream: a
 * loaded program serves one stream, its calls in order. */
const char* bx_acc_program_run(bx_ctx* ctx, bx_acc_program_dev* dev, uint32_t po2, bx_buf kept, const uint32_t* globals, const uint32_t mix[4], bx_buf run_ext,
                               bx_buf mults, bx_buf accum, uint32_t w_accum);
/* The table's accumulate then comes from `acc` ("composite" above); its create loads the program on the ctx and refuses by name a kept
 * column beyond the shape's widths, 4 S > w_accum, a global count other than the base's, and a base without accumulate when
 * w_accum > 4 S.  NULL goes back to forwarding accumulate to `base` alone.  `acc` must outlive the table.  Set before a prover is created. */
const char* bx_cons_circuit_set_accumulate(bx_cons_circuit* cc, const bx_acc_program* acc);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif

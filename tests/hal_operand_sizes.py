"""What tests/test_hal_operands_gpu.py and tests/test_operand_overlap_check_cpu.py share: the names the overlap refusals carry, and the
sizes of the large-array cases with the thresholds they are derived from (the CPU test reads the same numbers out of the sources)."""

# the prefix of "<name>: <operand> and <operand> overlap", one per entry point that has an operand rule (include/bx_hal.h)
ENTRY_POINTS_WITH_A_RULE = [
    "fri_fold", "fri_fold_dev", "mix_poly_coeffs", "eltwise_sum_extelem", "hash_rows", "merkle_build", "hash_fold_indexed",
    "batch_evaluate_any", "batch_evaluate_ptrs", "scatter", "merkle_query_gather", "transcript_step", "poly_divide", "poly_divide_batch",
    "poly_divide_batch_indexed", "gather_sample", "eltwise_add_elem", "eltwise_copy_elem", "bx_d2d", "logup_accumulate",
    "batch_expand_into_evaluate_ntt",
]

DIVIDE_THIRD_LEVEL = 1 << 21  # DIV_DIRECT * DIV_L^2: above it divide_rec runs three chunked levels before its one-workgroup kernel
SCAN_THIRD_LEVEL = 1 << 23    # PP_DIRECT * PP_L^2: the same for three_phase_rec
ELTWISE_ONE_TRIP = 65536 * 256  # grid1d's block cap times its block size: above it a lane of the element-wise kernels loops
DIVIDE_N = DIVIDE_THIRD_LEVEL + 1
SCAN_N = SCAN_THIRD_LEVEL + 1
ELTWISE_WORDS = ELTWISE_ONE_TRIP + 5

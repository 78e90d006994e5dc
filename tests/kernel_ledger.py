"""The ledger of the library's gfx950 kernels: which GPU test launches each one, and which none can.

A kernel's name here is its demangled name without the namespace, the argument list and the blanks: `k_cmux<2,10>`,
`k_blind_rotate<2,10,false>`, `k_copy_words`.  ENTRIES maps a pattern over such names (re.fullmatch) to the GPU test that
launches every kernel the pattern matches -- file, test function, and what selects the instance there -- read from the
dispatch code: blind_rotate_kernel, launch_leveled, launch_keyswitch, ks_mfma_launch, the `p == 2 ? ... : ...` selections,
k_lin_modswitch<MAXT, BOOT>, k_seed_masks<MODE>, k_sample_add<V>, k_dot_init / k_conv_lists (engine.hip) and multi.hip's
k_copy_words.  UNLAUNCHED maps a kernel to the dispatch condition that makes it unreachable from every public call.

tests/test_kernel_ledger_cpu.py holds the built code objects against this file: every kernel matches exactly one entry or is in
UNLAUNCHED, every entry matches a kernel, every file and function exists -- a kernel added without an entry fails there.
tools/kernel_ledger.py holds a kernel trace of the GPU suite against it: the kernels with no dispatch are UNLAUNCHED's.  The
trace is per process, not per test: that the suite launches every kernel is measured, which test does it is read."""
import re

# the third template argument of the blind rotations: the rotation amounts read back by vector (false) or scalar (true) loads
_BR = "tests/test_gpu_br_instances.py", "test_instance_bit_exact_on_edge_inputs"
_ENC = "tests/test_gpu_lut2_instances.py", "test_instance_bit_exact_on_edge_inputs"
_ROUND = "tests/test_gpu_leveled_round_instances.py"
_INST = "one id per instance, named after the kernel"

# (pattern, file, test function, what picks the instance)
ENTRIES = [
    # -- blind rotations: blind_rotate_kernel(wide, l, Bgbit, sabar, tables_lds, family) ---------------------------------------
    (r"k_blind_rotate<[1234],(0|7|10),(true|false)>", *_BR, _INST),
    (r"k_blind_rotate_tv<[1234],(0|7|10),(true|false)>", *_BR, _INST),
    (r"k_lut_many<[1234],(0|7|10),(true|false)>", *_BR, _INST),
    (r"k_br_lds<2,(0|10),(true|false)>", *_BR, _INST + " (EOC_TFHE_BR_TABLES_LDS=1)"),
    (r"k_br_lds_tv<2,(0|10),(true|false)>", *_BR, _INST + " (EOC_TFHE_BR_TABLES_LDS=1)"),
    (r"k_br_lds_many<2,(0|10),(true|false)>", *_BR, _INST + " (EOC_TFHE_BR_TABLES_LDS=1)"),
    (r"k_blind_rotate_wide<(0|10),(true|false)>", *_BR, _INST + " (EOC_TFHE_BR_WIDE=1)"),
    (r"k_blind_rotate_wide_tv<(0|10),(true|false)>", *_BR, _INST + " (EOC_TFHE_BR_WIDE=1)"),
    (r"k_lut_many_wide<(0|10),(true|false)>", *_BR, _INST + " (EOC_TFHE_BR_WIDE=1)"),
    (r"k_br_enc<[1234],(0|7|10),(true|false)>", *_ENC, _INST),
    (r"k_br_enc_wide<(0|10),(true|false)>", *_ENC, _INST + " (EOC_TFHE_BR_WIDE=1)"),
    # -- leveled kernels: launch_leveled(family or its rounding twin, l, Bgbit) ------------------------------------------------
    (r"k_cmux<[1234],(0|7|10)>", "tests/test_gpu_cmux_instances.py", "test_instance_bit_exact_on_edge_inputs", _INST),
    (r"k_demux<[1234],(0|7|10)>", "tests/test_gpu_demux_instances.py", "test_instance_bit_exact_on_edge_inputs", _INST),
    (r"k_automaton_step<[1234],(0|7|10)>", "tests/test_gpu_automaton_instances.py", "test_instance_bit_exact_on_edge_inputs", _INST),
    (r"k_rcmux<[1234],(0|7|10)>", _ROUND, "test_rcmux_instance_bit_exact_on_edge_inputs", _INST),
    (r"k_rdemux<[1234],(0|7|10)>", _ROUND, "test_rdemux_instance_bit_exact_on_edge_inputs", _INST),
    (r"k_rstep<[1234],(0|7|10)>", _ROUND, "test_rstep_instance_bit_exact_on_edge_inputs", _INST),
    # -- key switch: launch_keyswitch ------------------------------------------------------------------------------------------
    (r"k_keyswitch_mfma<4>", "tests/test_gpu_ks_mfma.py", "test_stand_alone_key_switch_new_equals_old_equals_oracle",
     "EOC_TFHE_KS_MFMA=1; ks_mfma_plan's nwv is 4"),
    (r"k_ksk_limbs", "tests/test_gpu_ks_mfma.py", "test_stand_alone_key_switch_new_equals_old_equals_oracle",
     "the limb image, built when a key is loaded"),
    (r"k_keyswitch_waves<8,(8,16|8,32|4,64|8,64)>", "tests/test_gpu_ks_mfma.py",
     "test_stand_alone_key_switch_new_equals_old_equals_oracle", "EOC_TFHE_KS_MFMA=0 at n + 1 padded to 256, 512, 768, 1024 columns"),
    (r"k_keyswitch_generic", "tests/test_gpu_parity.py", "test_other_keyswitch_shapes", "(ks_basebit, ks_t) other than (2, 8)"),
    (r"k_ks_init", "tests/test_gpu_ks_mfma.py", "test_stand_alone_key_switch_new_equals_old_equals_oracle",
     "the stand-alone key switch and levels with a MUX: no blind rotation epilogue set the rows up"),
    # -- gate levels -----------------------------------------------------------------------------------------------------------
    (r"k_prepare", "tests/test_gpu_parity.py", "test_mixed_all_opcodes_run_as_one_level", "three-operand gates: no folded prologue"),
    (r"k_modswitch_coarse", "tests/test_gpu_lut_many.py", "test_set_a_pair_kernel_bit_exact", "theta > 0"),
    (r"k_free_gates", "tests/test_gpu_parity.py", "test_mux_not_copy_small", "NOT / COPY / CONSTANT runs"),
    (r"k_gather_rows", "tests/test_gpu_parity.py", "test_mixed_ops_arbitrary_order_large", "a mixed batch sorted by opcode"),
    (r"k_tv_gather", "tests/test_gpu_int_circuit.py", "test_mixed_two_level_circuit_bit_exact", "the tables of a level's nodes"),
    (r"k_lin_modswitch<[1234],(true|false)>", "tests/test_gpu_linear_stage_paths.py", "test_path_bit_exact_on_cell_edge_operands",
     "one id per (MAXT, BOOT) path"),
    # -- transforms, compact lists, extraction -----------------------------------------------------------------------------------
    (r"k_fft_fwd_polys", "tests/test_gpu_parity.py", "test_fft_forward_inverse_bit_exact", ""),
    (r"k_fft_inv_polys", "tests/test_gpu_parity.py", "test_fft_forward_inverse_bit_exact", ""),
    (r"k_compact_expand", "tests/test_gpu_compact.py", "test_expansion_equals_the_oracle_composition", ""),
    (r"k_tlwe_extract", "tests/test_gpu_cmux_instances.py", "test_instance_bit_exact_on_edge_inputs", "the table read's slots"),
    # -- packing -----------------------------------------------------------------------------------------------------------------
    (r"k_pack_gather", "tests/test_gpu_pack_edges.py", "test_pack_bit_exact_on_edge_words_and_shapes", ""),
    (r"k_pack_rows", "tests/test_gpu_pack_edges.py", "test_pack_bit_exact_on_edge_words_and_shapes", ""),
    (r"k_tvpack_cols<[248]>", "tests/test_gpu_pack_edges.py", "test_tv_pack_bit_exact_on_extreme_words", "p = 2, 4, 8"),
    (r"k_pks_limbs", "tests/test_gpu_tvpack_mm.py", "test_real_keys_word_for_word", "the limb image, built when a packing key is loaded"),
    (r"k_tvpack_mm<4>", "tests/test_gpu_tvpack_mm.py", "test_real_keys_word_for_word", ""),
    (r"k_tv_spread<[248]>", "tests/test_gpu_tvpack_mm.py", "test_real_keys_word_for_word", "p = 2, 4, 8"),
    # -- table updates, seeded expansion -------------------------------------------------------------------------------------------
    (r"k_sample_add<[14]>", "tests/test_gpu_table_update.py", "test_update_equals_the_composed_reference",
     "d = 0 (one list: the rotated value is the leaf); <4> where value and table are 16-byte aligned, <1> otherwise"),
    (r"k_seed_masks<[012]>", "tests/test_gpu_seeded.py", "test_cloud_key_images_equal_those_of_the_host_expanded_arrays",
     "SEED_LWE, SEED_KSK, SEED_RING"),
    (r"k_chacha20_blocks<16>", "tests/test_gpu_seeded.py", "test_block_function_equals_the_hosts", ""),
    # -- inner products and convolutions -------------------------------------------------------------------------------------------
    (r"k_dot_init<(true|false)>", "tests/test_gpu_dot.py", "test_linear_equals_reference_dot_plus_keyswitch",
     "<true> extracts for the key switch (eoc_linear_device), <false> keeps the list (eoc_dot_device)"),
    (r"k_dot_mask<8>", "tests/test_gpu_dot.py", "test_dot_equals_the_reference", ""),
    (r"k_conv_init<256>", "tests/test_gpu_conv.py", "test_conv_equals_the_reference", "more than one chunk per output"),
    (r"k_conv_lists<8,(true|false)>", "tests/test_gpu_conv.py", "test_conv_equals_the_reference",
     "<true> stores (one chunk per output), <false> adds behind k_conv_init"),
    (r"k_conv_extract<16>", "tests/test_gpu_conv.py", "test_extraction_and_key_switch_equal_the_reference", ""),
    # -- multi.hip -----------------------------------------------------------------------------------------------------------------
    (r"k_copy_words", "tests/test_gpu_multi.py", "test_pinned_io_and_steady_state_buffers",
     "result rows into the caller's pinned, device-mapped buffer"),
]

# kernel -> the dispatch condition that keeps every public call from it.  Empty: k_keyswitch_mfma<8>, which ks_mfma_launch took
# only under a plan width ks_mfma_plan never sets, is no longer compiled (tools/ubench_ks_mfma.hip instantiates it for its sweep).
UNLAUNCHED = {}


def short_name(name):
    """`void eoc::k_cmux<2, 10>(eoc::CmuxArgs, ...) [clone .kd]` -> `k_cmux<2,10>`"""
    name = re.sub(r"^void\s+", "", name.strip())
    name = re.sub(r"\.kd$", "", name)
    depth, cut = 0, len(name)
    for i, ch in enumerate(name):                               # the argument list: the first ( outside the template brackets
        depth += (ch == "<") - (ch == ">")
        if ch == "(" and depth == 0:
            cut = i
            break
    return re.sub(r"^(\w+::)+", "", name[:cut].strip()).replace(" ", "")


def entries_of(kernel):
    """the entries whose pattern matches the short name `kernel`"""
    return [e for e in ENTRIES if re.fullmatch(e[0], kernel)]

"""eoc_tfhe_amd -- Python host side of libeoc_tfhe_gpu.so (ctypes over the C ABI of
include/eoc_tfhe_gpu.h).

The product is the shared library; this module is the thin façade a Python host uses, in the way
ao-tfhe/tfhe.lua:1-53 wraps the Lua C module (`Tfhe.*` pass-throughs to `Tfhe.backend.*`).
Nothing here computes a gate on the CPU: every hot-path call goes to the HIP engine and raises
if the library or a GPU is missing.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EOC_TFHE_LIB") or os.path.join(_HERE, "libeoc_tfhe_gpu.so")
N = 1024

OPS = dict(NAND=0, AND=1, OR=2, NOR=3, XOR=4, XNOR=5, ANDNY=6, ANDYN=7, ORNY=8, ORYN=9,
           MUX=10, NOT=11, COPY=12, CONST0=13, CONST1=14,
           MAJ=15, XOR3=16)   # extension gates: majority / three-input parity, one bootstrap each (include/eoc_tfhe_gpu.h)


class EocError(RuntimeError):
    pass


class Params(C.Structure):
    """eoc_params (TFheGateBootstrappingParameterSet flattened)."""
    _fields_ = [("n", C.c_int32), ("l", C.c_int32), ("Bgbit", C.c_int32), ("ks_t", C.c_int32),
                ("ks_basebit", C.c_int32), ("ks_stdev", C.c_double), ("bk_stdev", C.c_double)]

    def copy(self):
        q = Params()
        C.memmove(C.byref(q), C.byref(self), C.sizeof(Params))
        return q


class Gate(C.Structure):
    """eoc_gate netlist entry."""
    _fields_ = [("op", C.c_int32), ("in0", C.c_int32), ("in1", C.c_int32), ("in2", C.c_int32),
                ("out", C.c_int32)]


class INode(C.Structure):
    """eoc_inode: a node of an integer netlist (include/eoc_tfhe_gpu.h)."""
    _fields_ = [("n_tables", C.c_int32), ("out", C.c_int32), ("tv", C.c_int32), ("n_terms", C.c_int32),
                ("in_", C.c_int32 * 4), ("w", C.c_int32 * 4), ("cst", C.c_int32)]


def _inode_array(nodes):
    arr = (INode * max(1, len(nodes)))()
    for k, q in enumerate(nodes):
        C.memmove(C.byref(arr[k]), C.byref(q), C.sizeof(INode))
    return arr


_lib = None


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch-ROCm bundles its own libamdhip64.so (SONAME
    libamdhip64.so.7); if our library pulled /opt/rocm's copy in first, a later `import torch`
    would load a second runtime and one of the two would see no device.  Pre-loading torch's copy
    (when torch is installed) makes both resolve to the same one, whatever the import order."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    """Load the C-ABI library (fails loudly when it has not been built)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EocError(f"{LIB_PATH} is missing: run `python -m eoc_tfhe_amd.build` "
                       "(there is no Python/CPU fallback for the gate path)")
    _share_hip_runtime_with_torch()
    L = C.CDLL(LIB_PATH)
    PP = C.POINTER(Params)
    vp, sz, u64 = C.c_void_p, C.c_size_t, C.c_uint64
    sig = {
        "eoc_default_params": (C.c_int, [C.c_int, PP]),
        "eoc_params_for_lambda": (C.c_int, [C.c_int, PP]),
        "eoc_keygen": (C.c_int, [PP, u64, C.c_int, C.POINTER(vp)]),
        "eoc_keygen_secure": (C.c_int, [PP, C.c_int, C.POINTER(vp)]),
        "eoc_keygen_from_master": (C.c_int, [PP, vp, C.c_int, C.POINTER(vp)]),
        "eoc_sk_is_secure": (C.c_int, [vp]),
        "eoc_encrypt_bits_keyed": (C.c_int, [vp, vp, u64, vp, sz, vp]),
        "eoc_dbg_chacha20_block": (None, [vp, C.c_uint32, vp, vp]),
        "eoc_secret_key_free": (None, [vp]),
        "eoc_sk_params": (PP, [vp]),
        "eoc_sk_lwe_key": (vp, [vp]),
        "eoc_sk_tlwe_key": (vp, [vp]),
        "eoc_sk_bk": (vp, [vp]),
        "eoc_sk_ksk": (vp, [vp]),
        "eoc_bk_len": (sz, [PP]),
        "eoc_ksk_len": (sz, [PP]),
        "eoc_encrypt_bits": (C.c_int, [vp, u64, u64, vp, sz, vp]),
        "eoc_decrypt_bits": (C.c_int, [vp, vp, sz, vp]),
        "eoc_lwe_encrypt": (C.c_int, [vp, u64, u64, C.c_int32, C.c_double, vp]),
        "eoc_lwe_phase": (C.c_int32, [vp, vp]),
        "eoc_host_threads": (C.c_int, []),
        "eoc_modswitch_to_torus32": (C.c_int32, [C.c_int32, C.c_int32]),
        "eoc_modswitch_from_torus32": (C.c_int32, [C.c_int32, C.c_int32]),
        "eoc_device_count": (C.c_int, []),
        "eoc_engine_create": (C.c_int, [C.c_int, PP, C.POINTER(vp)]),
        "eoc_engine_destroy": (None, [vp]),
        "eoc_last_error": (C.c_char_p, []),
        "eoc_device_alloc": (C.c_int, [vp, sz, C.POINTER(vp)]),
        "eoc_device_free": (C.c_int, [vp, vp]),
        "eoc_host_to_device": (C.c_int, [vp, vp, vp, sz]),
        "eoc_device_to_host": (C.c_int, [vp, vp, vp, sz]),
        "eoc_engine_synchronize": (C.c_int, [vp]),
        "eoc_bkfft_bytes": (sz, [PP]),
        "eoc_ksk_dev_bytes": (sz, [PP]),
        "eoc_ksk_row_stride": (sz, [PP]),
        "eoc_engine_load_cloud_key": (C.c_int, [vp, vp, vp]),
        "eoc_engine_set_cloud_key_device": (C.c_int, [vp, vp, vp]),
        "eoc_engine_build_cloud_key_device": (C.c_int, [vp, vp, vp, vp, vp]),
        "eoc_engine_set_profiling": (C.c_int, [vp, C.c_int]),
        "eoc_engine_kernel_times": (C.c_int, [vp, C.POINTER(C.c_double * 3), C.POINTER(u64 * 3), C.c_int]),
        "eoc_engine_cloud_key_device": (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp)]),
        "eoc_gate_batch_device": (C.c_int, [vp, C.c_int, vp, vp, vp, vp, vp, sz, vp]),
        "eoc_circuit_run_device": (C.c_int, [vp, vp, sz, vp, sz, sz, vp]),
        "eoc_circuit_bootstraps": (sz, [vp, sz]),
        "eoc_netlist_optimize": (C.c_int64, [vp, sz, vp, sz, vp]),
        "eoc_netlist_optimize_ex": (C.c_int64, [vp, sz, vp, sz, vp, C.c_uint]),
        "eoc_netlist_levels": (C.c_int64, [vp, sz, vp, vp]),
        "eoc_netlist_cost": (C.c_int64, [vp, sz, sz, sz]),
        "eoc_dbg_fft_fwd_device": (C.c_int, [vp, vp, vp, sz, vp]),
        "eoc_dbg_fft_inv_device": (C.c_int, [vp, vp, vp, sz, vp]),
        "eoc_blind_rotate_device": (C.c_int, [vp, vp, vp, sz, vp]),
        "eoc_keyswitch_device": (C.c_int, [vp, vp, vp, sz, vp]),
        "eoc_lut_batch_device": (C.c_int, [vp, vp, sz, vp, vp, sz, vp]),
        "eoc_encrypt_ints": (C.c_int, [vp, u64, u64, C.c_int, vp, sz, vp]),
        "eoc_decrypt_ints": (C.c_int, [vp, C.c_int, vp, sz, vp]),
        "eoc_lut_test_polynomial": (C.c_int, [C.c_int, vp, vp]),
        "eoc_lut_batch": (C.c_int, [C.c_int, vp, sz, vp, vp, sz]),
        "eoc_lut_many_test_polynomial": (C.c_int, [C.c_int, C.c_int, vp, vp]),
        "eoc_lut_many_batch_device": (C.c_int, [vp, C.c_int, vp, sz, vp, vp, sz, vp]),
        "eoc_lut_many_batch": (C.c_int, [C.c_int, C.c_int, vp, sz, vp, vp, sz]),
        "eoc_int_netlist_levels": (C.c_int64, [vp, sz, sz, sz, vp, vp]),
        "eoc_int_circuit_run_device": (C.c_int, [vp, vp, sz, vp, sz, vp, sz, sz, vp]),
        "eoc_int_circuit_run": (C.c_int, [vp, sz, vp, vp, vp, sz, vp, sz, sz]),
        "eoc_global_encrypt_ints": (C.c_int, [C.c_int, vp, sz, vp]),
        "eoc_global_decrypt_ints": (C.c_int, [C.c_int, vp, sz, vp]),
        "eoc_engine_stats": (C.c_int, [vp, C.POINTER(u64 * 3)]),
        "eoc_stats": (C.c_int, [C.POINTER(u64 * 3)]),
        "eoc_gpu_init": (C.c_int, [C.c_int, PP]),
        "eoc_gpu_init_multi": (C.c_int, [vp, C.c_int, PP]),
        "eoc_gpu_init_from_env": (C.c_int, [PP]),
        "eoc_gpu_set_devices": (C.c_int, [C.POINTER(C.c_int), C.c_int]),
        "eoc_gpu_engine_count": (C.c_int, []),
        "eoc_global_engine_at": (vp, [C.c_int]),
        "eoc_upload_cloud_key_arrays": (C.c_int, [vp, vp]),
        "eoc_stats_multi": (C.c_int, [vp, C.c_int, C.POINTER(C.c_double)]),
        "eoc_key_broadcast_method": (C.c_char_p, []),
        "eoc_host_path_buffer_grows": (u64, []),
        "eoc_rccl_origin": (C.c_char_p, []),
        "eoc_rccl_selftest": (C.c_int, [C.c_int, sz]),
        "eoc_worker_wakeups": (u64, [C.c_int]),
        "eoc_shard_range": (None, [sz, C.c_int, C.c_int, C.POINTER(sz), C.POINTER(sz)]),
        "eoc_gate_batch_submit": (C.c_int, [C.c_int, vp, vp, vp, vp, vp, sz, C.POINTER(u64)]),
        "eoc_gate_batch_wait": (C.c_int, [u64]),
        "eoc_global_gate_batch_submit": (C.c_int, [C.c_int, vp, vp, vp, vp, vp, sz, C.POINTER(u64)]),
        "eoc_host_alloc": (vp, [sz]),
        "eoc_host_free": (None, [vp]),
        "eoc_engine_reserve": (C.c_int, [vp, sz, sz, sz]),
        "eoc_engine_workspace_grows": (u64, [vp]),
        "eoc_engine_blind_rotate_launches": (u64, [vp]),
        "eoc_engine_blind_rotate_wide_launches": (u64, [vp]),
        "eoc_engine_keyswitch_mfma_launches": (u64, [vp]),
        "eoc_engine_resident_jobs": (C.c_size_t, [vp]),
        "eoc_engine_device": (C.c_int, [vp]),
        "eoc_engine_params": (PP, [vp]),
        "eoc_engine_adopt_cloud_key_device": (C.c_int, [vp, vp, vp]),
        "eoc_upload_cloud_key": (C.c_int, [vp]),
        "eoc_global_engine": (vp, []),
        "eoc_gpu_shutdown": (None, []),
        "eoc_gate_batch": (C.c_int, [C.c_int, vp, vp, vp, vp, vp, sz]),
        "eoc_circuit_run": (C.c_int, [vp, sz, vp, sz, sz]),
        "generateGateKey": (vp, [C.c_int, u64]),
        "resetGateKey": (None, []),
        "encryptBit": (vp, [C.c_int, C.c_char_p]),
        "decryptBit": (C.c_int, [C.c_char_p, C.c_char_p]),
        "constantBit": (vp, [C.c_int]),
        "gateNAND": (vp, [C.c_char_p, C.c_char_p, C.c_char_p]),
        "gateAND": (vp, [C.c_char_p, C.c_char_p, C.c_char_p]),
        "gateOR": (vp, [C.c_char_p, C.c_char_p, C.c_char_p]),
        "gateNOR": (vp, [C.c_char_p, C.c_char_p, C.c_char_p]),
        "gateXOR": (vp, [C.c_char_p, C.c_char_p, C.c_char_p]),
        "gateXNOR": (vp, [C.c_char_p, C.c_char_p, C.c_char_p]),
        "gateNOT": (vp, [C.c_char_p, C.c_char_p]),
        "gateMUX": (vp, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p]),
        "gateMAJ": (vp, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p]),
        "gateXOR3": (vp, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p]),
        # f1: the reference's 11 calls
        "generateSecretKey": (vp, [C.c_char_p, C.c_char_p]),
        "generatePublicKey": (vp, []),
        "encryptInteger": (vp, [C.c_int32, C.c_char_p]),
        "encryptInteger_dummy": (vp, [C.c_int32, C.c_char_p]),
        "decryptInteger": (C.c_int, [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p]),
        "addCiphertexts": (vp, [C.c_char_p, C.c_char_p, C.c_char_p]),
        "subtractCiphertexts": (vp, [C.c_char_p, C.c_char_p, C.c_char_p]),
        "encrypt8BitASCIIString": (vp, [C.c_char_p, C.c_int16, C.c_char_p]),
        "decrypt8BitASCIIString": (vp, [C.c_char_p, C.c_int16, C.c_char_p, C.c_char_p, C.c_char_p]),
        "info": (None, []),
        "testJWT": (None, []),
        # f2: key export / import
        "eoc_secret_key_export": (sz, [vp, vp, sz]),
        "eoc_secret_key_import": (C.c_int, [vp, sz, C.c_int, C.POINTER(vp)]),
        "eoc_cloud_key_blob_bytes": (sz, [PP]),
        "eoc_cloud_key_export": (C.c_int, [vp, vp, sz]),
        "eoc_cloud_key_blob_params": (C.c_int, [vp, sz, PP]),
        "eoc_engine_create_from_cloud_key_blob": (C.c_int, [C.c_int, vp, sz, C.POINTER(vp)]),
        "eoc_global_params": (C.c_int, [PP]),
        "eoc_global_encrypt_bits": (C.c_int, [vp, sz, vp]),
        "eoc_global_decrypt_bits": (C.c_int, [vp, sz, vp]),
        "eoc_global_gate_batch": (C.c_int, [C.c_int, vp, vp, vp, vp, vp, sz]),
        "eoc_global_circuit_run": (C.c_int, [vp, sz, vp, sz, sz]),
        "exportSecretKey": (vp, []),
        "importSecretKey": (C.c_int, [C.c_char_p]),
        # f2, server side: the cloud ("public") key on the global context
        "exportCloudKey": (vp, []),
        "importCloudKey": (C.c_int, [C.c_char_p]),
        "exportCloudKeyToFile": (C.c_int, [C.c_char_p]),
        "importCloudKeyFromFile": (C.c_int, [C.c_char_p]),
        "eoc_global_cloud_key_export": (sz, [vp, sz]),
        "eoc_global_import_cloud_key_blob": (C.c_int, [vp, sz]),
        "eoc_global_key_mode": (C.c_int, []),
        # compact public-key encryption
        "eoc_public_key_blob_bytes": (sz, [PP]),
        "eoc_public_key_export": (C.c_int, [vp, vp, sz]),
        "eoc_public_key_blob_params": (C.c_int, [vp, sz, PP]),
        "eoc_pk_encrypt_bits": (C.c_int, [vp, sz, u64, u64, vp, sz, vp]),
        "eoc_pk_encrypt_bits_keyed": (C.c_int, [vp, sz, vp, u64, vp, sz, vp]),
        "eoc_pk_encrypt_ints": (C.c_int, [vp, sz, u64, u64, C.c_int, vp, sz, vp]),
        "eoc_pk_encrypt_ints_keyed": (C.c_int, [vp, sz, vp, u64, C.c_int, vp, sz, vp]),
        "eoc_compact_expand_device": (C.c_int, [vp, vp, sz, vp, vp]),
        "eoc_compact_expand": (C.c_int, [vp, sz, vp]),
        "eoc_global_public_key_export": (sz, [vp, sz]),
        # leveled operations: selectors, CMux, encrypted-index table reads
        "eoc_tgsw_len": (sz, [PP]),
        "eoc_tgsw_encrypt_bits": (C.c_int, [vp, u64, u64, vp, sz, vp]),
        "eoc_tgsw_encrypt_bits_keyed": (C.c_int, [vp, vp, u64, vp, sz, vp]),
        "eoc_global_tgsw_encrypt_bits": (C.c_int, [vp, sz, vp]),
        "eoc_table_trivial": (C.c_int, [vp, sz, vp]),
        "eoc_tgsw_fft_bytes": (sz, [PP]),
        "eoc_tgsw_to_fft_device": (C.c_int, [vp, vp, sz, vp, vp]),
        "eoc_cmux_device": (C.c_int, [vp, vp, vp, vp, vp, sz, vp]),
        "eoc_table_read_device": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, sz, vp, vp]),
        "eoc_engine_cmux_launches": (u64, [vp]),
        "eoc_table_read": (C.c_int, [vp, C.c_int, C.c_int, vp, sz, vp]),
        # encrypted-index table updates
        "eoc_demux_device": (C.c_int, [vp, vp, vp, vp, vp, sz, C.c_int, vp]),
        "eoc_table_update_device": (C.c_int, [vp, vp, C.c_int, C.c_int, vp, vp, sz, vp]),
        "eoc_engine_demux_launches": (u64, [vp]),
        "eoc_table_update": (C.c_int, [vp, C.c_int, C.c_int, vp, vp, sz]),
        # finite automata on encrypted bit strings
        "eoc_automaton_step_device": (C.c_int, [vp, vp, sz, vp, sz, vp, sz, vp, sz, vp]),
        "eoc_automaton_run_device": (C.c_int, [vp, vp, sz, vp, vp, sz, vp, sz, C.c_int, vp, sz, vp]),
        "eoc_engine_automaton_launches": (u64, [vp]),
        "eoc_automaton_run": (C.c_int, [vp, sz, vp, vp, sz, vp, sz, C.c_int, vp, sz]),
        # rounding mode of the leveled calls
        "eoc_engine_set_leveled_rounding": (C.c_int, [vp, C.c_int]),
        "eoc_engine_leveled_rounding": (C.c_int, [vp]),
        "eoc_global_set_leveled_rounding": (C.c_int, [C.c_int]),
        # packing key switch: LWE samples -> compact lists
        "eoc_packing_key_blob_bytes": (sz, [PP]),
        "eoc_packing_key_export": (C.c_int, [vp, vp, sz]),
        "eoc_packing_key_blob_params": (C.c_int, [vp, sz, PP]),
        "eoc_engine_set_packing_key": (C.c_int, [vp, vp, sz]),
        "eoc_pack_device": (C.c_int, [vp, vp, sz, vp, vp]),
        "eoc_engine_pack_launches": (u64, [vp]),
        "eoc_engine_packed_samples": (u64, [vp]),
        "eoc_list_phases": (C.c_int, [vp, vp, sz, vp]),
        "eoc_decrypt_list_bits": (C.c_int, [vp, vp, sz, vp]),
        "eoc_decrypt_list_ints": (C.c_int, [vp, C.c_int, vp, sz, vp]),
        "eoc_global_list_phases": (C.c_int, [vp, sz, vp]),
        "eoc_global_decrypt_list_bits": (C.c_int, [vp, sz, vp]),
        "eoc_global_decrypt_list_ints": (C.c_int, [C.c_int, vp, sz, vp]),
        "eoc_global_packing_key_export": (sz, [vp, sz]),
        "eoc_global_import_packing_key_blob": (C.c_int, [vp, sz]),
        "eoc_pack": (C.c_int, [vp, sz, vp]),
        # two-input table lookups
        "eoc_lut2_test_polynomials": (C.c_int, [C.c_int, C.c_int, vp, vp]),
        "eoc_lut_enc_batch_device": (C.c_int, [vp, vp, sz, C.c_int, vp, vp, sz, vp]),
        "eoc_tv_pack_device": (C.c_int, [vp, C.c_int, vp, sz, sz, vp, vp]),
        "eoc_lut2_batch_device": (C.c_int, [vp, C.c_int, C.c_int, vp, sz, vp, vp, vp, sz, vp]),
        "eoc_lut2_batch": (C.c_int, [C.c_int, C.c_int, vp, sz, vp, vp, vp, sz]),
        "eoc_tv_pack_exact_device": (C.c_int, [vp, C.c_int, vp, sz, sz, vp, vp]),
        "eoc_lut_tree_test_polynomials": (C.c_int, [C.c_int, C.c_int, C.c_int, vp, vp]),
        "eoc_lut_tree_batch_device": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, vp, sz, vp, vp, sz, vp]),
        "eoc_lut_tree_batch": (C.c_int, [C.c_int, C.c_int, C.c_int, vp, sz, vp, vp, sz]),
        # seeded ciphertexts, selectors and cloud key
        "eoc_seeded_encrypt_bits": (C.c_int, [vp, vp, sz, vp, vp]),
        "eoc_seeded_encrypt_ints": (C.c_int, [vp, C.c_int, vp, sz, vp, vp]),
        "eoc_seeded_encrypt_bits_keyed": (C.c_int, [vp, vp, vp, u64, vp, sz, vp]),
        "eoc_seeded_encrypt_ints_keyed": (C.c_int, [vp, vp, vp, u64, C.c_int, vp, sz, vp]),
        "eoc_tgsw_seeded_encrypt_bits": (C.c_int, [vp, vp, sz, vp, vp]),
        "eoc_tgsw_seeded_encrypt_bits_keyed": (C.c_int, [vp, vp, vp, u64, vp, sz, vp]),
        "eoc_seeded_cloud_key_blob_bytes": (sz, [PP]),
        "eoc_seeded_cloud_key_export": (C.c_int, [vp, vp, sz]),
        "eoc_seeded_cloud_key_blob_params": (C.c_int, [vp, sz, PP]),
        "eoc_seeded_expand_host": (C.c_int, [PP, vp, u64, vp, sz, vp]),
        "eoc_tgsw_seeded_expand_host": (C.c_int, [PP, vp, u64, vp, sz, vp]),
        "eoc_seeded_cloud_key_expand": (C.c_int, [vp, sz, vp, vp]),
        "eoc_seeded_expand_device": (C.c_int, [vp, vp, u64, vp, sz, vp, vp]),
        "eoc_tgsw_seeded_to_fft_device": (C.c_int, [vp, vp, u64, vp, sz, vp, vp]),
        "eoc_engine_load_seeded_cloud_key": (C.c_int, [vp, vp, sz]),
        "eoc_engine_create_from_seeded_cloud_key_blob": (C.c_int, [C.c_int, vp, sz, C.POINTER(vp)]),
        "eoc_engine_seed_launches": (u64, [vp]),
        "eoc_dbg_chacha20_blocks_device": (C.c_int, [vp, vp, u64, u64, sz, vp, vp]),
        "eoc_seeded_expand": (C.c_int, [vp, u64, vp, sz, vp]),
        "eoc_global_import_seeded_cloud_key_blob": (C.c_int, [vp, sz]),
        # inner products with public integer weights on compact lists
        "eoc_weights_image_bytes": (sz, [sz, sz]),
        "eoc_weights_to_device": (C.c_int, [vp, vp, sz, sz, vp, vp]),
        "eoc_dot_device": (C.c_int, [vp, vp, sz, sz, vp, sz, vp, vp, vp]),
        "eoc_linear_device": (C.c_int, [vp, vp, sz, sz, vp, sz, vp, vp, vp]),
        "eoc_engine_dot_launches": (u64, [vp]),
        "eoc_linear": (C.c_int, [vp, sz, sz, vp, sz, vp, vp]),
        "eoc_pk_encrypt_torus": (C.c_int, [vp, sz, u64, u64, vp, sz, vp]),
        "eoc_pk_encrypt_torus_keyed": (C.c_int, [vp, sz, vp, u64, vp, sz, vp]),
        # convolutions with public int8 kernels on compact lists
        "eoc_conv_slots_to_device": (C.c_int, [vp, vp, sz, sz, vp, vp]),
        "eoc_conv_device": (C.c_int, [vp, vp, sz, sz, vp, sz, vp, vp, vp]),
        "eoc_conv_linear_device": (C.c_int, [vp, vp, sz, sz, vp, sz, vp, vp, sz, vp, vp]),
        "eoc_conv_extract_device": (C.c_int, [vp, vp, sz, sz, vp, sz, vp, vp]),
        "eoc_engine_conv_launches": (u64, [vp]),
        "eoc_conv_linear": (C.c_int, [vp, sz, sz, vp, sz, vp, vp, sz, vp]),
        # dense layers on LWE samples (include/eoc_tfhe_lwe.h)
        "eoc_lwe_weights_image_bytes": (sz, [sz, sz]),
        "eoc_lwe_weights_to_device": (C.c_int, [vp, vp, sz, sz, vp, vp]),
        "eoc_lwe_matmul_device": (C.c_int, [vp, vp, sz, sz, vp, sz, sz, vp, vp, vp]),
        "eoc_engine_lwe_matmul_launches": (u64, [vp]),
        "eoc_lwe_matmul": (C.c_int, [vp, sz, sz, vp, sz, sz, vp, vp]),
    }
    for name, (res, args) in sig.items():
        f = getattr(L, name)
        f.restype = res
        f.argtypes = args
    _lib = L
    return L


ABI_SYMBOLS = None  # filled lazily by abi_symbols()


def abi_symbols():
    """Every symbol include/eoc_tfhe_gpu.h declares (parsed from the header)."""
    import re
    hdr = os.path.join(os.path.dirname(_HERE), "include", "eoc_tfhe_gpu.h")
    text = open(hdr).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = re.findall(r"\b([A-Za-z_][A-Za-z0-9_]*)\s*\([^;{}]*\)\s*;", text)
    return sorted(set(names))


def _check(rc, what):
    if rc != 0:
        msg = lib().eoc_last_error()
        raise EocError(f"{what} failed (code {rc}): {msg.decode() if msg else ''}")


def default_params(pset=0):
    p = Params()
    _check(lib().eoc_default_params(pset, C.byref(p)), "eoc_default_params")
    return p


def _take_str(ptr):
    """Copy and free() a heap C string returned by the string API (NULL -> None, like Lua nil)."""
    if not ptr:
        return None
    s = C.string_at(ptr).decode()
    C.CDLL(None).free(C.c_void_p(ptr))
    return s


def _np_view(ptr, count, dtype):
    if not ptr:
        return None
    buf = (C.c_char * (count * np.dtype(dtype).itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype, count=count)


def _key32(key, what):
    k = np.frombuffer(bytes(key), np.uint8).copy() if key is not None else None
    if k is None or k.size != 32:
        raise EocError(f"{what} must be 32 bytes")
    return k


def _blob_u8(blob):
    return np.ascontiguousarray(np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray)) else blob, np.uint8)


def seeded_expand_host(params, seed, bodies, first_idx=0):
    """Host twin of Engine.seeded_expand_device (eoc_seeded_expand_host): (seed, bodies [count]) -> samples [count][n+1]"""
    s = _key32(seed, "seed")
    bodies = np.ascontiguousarray(np.asarray(bodies).ravel(), np.int32)
    out = np.empty((bodies.size, params.n + 1), np.int32)
    _check(lib().eoc_seeded_expand_host(C.byref(params), s.ctypes.data, int(first_idx), bodies.ctypes.data, bodies.size,
                                        out.ctypes.data), "eoc_seeded_expand_host")
    return out


def tgsw_seeded_expand_host(params, seed, bodies, first_idx=0):
    """(seed, bodies [count][2l][N]) -> selectors in torus form [count][2l][2][N] (eoc_tgsw_seeded_expand_host)"""
    s = _key32(seed, "seed")
    bodies = np.ascontiguousarray(bodies, np.int32).reshape(-1, 2 * params.l, N)
    out = np.empty((bodies.shape[0], 2 * params.l, 2, N), np.int32)
    _check(lib().eoc_tgsw_seeded_expand_host(C.byref(params), s.ctypes.data, int(first_idx), bodies.ctypes.data,
                                             bodies.shape[0], out.ctypes.data), "eoc_tgsw_seeded_expand_host")
    return out


def seeded_cloud_key_params(blob):
    blob = _blob_u8(blob)
    p = Params()
    _check(lib().eoc_seeded_cloud_key_blob_params(blob.ctypes.data, blob.size, C.byref(p)), "eoc_seeded_cloud_key_blob_params")
    return p


def seeded_cloud_key_expand(blob):
    """EOCCKS1 blob -> (bk [n][2l][2][N], ksk [N t (base - 1)][n+1]) in torus form, on the host: what Engine.load_cloud_key
    and the oracle accept (eoc_seeded_cloud_key_expand)"""
    blob = _blob_u8(blob)
    p = seeded_cloud_key_params(blob)
    L = lib()
    bk = np.empty(L.eoc_bk_len(C.byref(p)), np.int32)
    ksk = np.empty(L.eoc_ksk_len(C.byref(p)), np.int32)
    _check(L.eoc_seeded_cloud_key_expand(blob.ctypes.data, blob.size, bk.ctypes.data, ksk.ctypes.data),
           "eoc_seeded_cloud_key_expand")
    return bk.reshape(p.n, 2 * p.l, 2, N), ksk.reshape(-1, p.n + 1)


class SecretKey:
    """TFheGateBootstrappingSecretKeySet: LWE key, TLWE key and (optionally) the cloud key."""

    def __init__(self, params, seed, with_cloud_key=True, master=None):
        """seed: int -> reproducible test mode (PRNG v1, shared with the oracle; NOT secure);
        seed None -> secure mode (getrandom + ChaCha20), or from a 32-byte `master` key"""
        self.L = lib()
        self.h = C.c_void_p()
        self.params = params.copy()
        if master is not None:
            m = np.frombuffer(bytes(master), np.uint8)
            assert m.size == 32
            _check(self.L.eoc_keygen_from_master(C.byref(self.params), m.ctypes.data, int(with_cloud_key), C.byref(self.h)),
                   "eoc_keygen_from_master")
        elif seed is None:
            _check(self.L.eoc_keygen_secure(C.byref(self.params), int(with_cloud_key), C.byref(self.h)), "eoc_keygen_secure")
        else:
            _check(self.L.eoc_keygen(C.byref(self.params), seed, int(with_cloud_key), C.byref(self.h)), "eoc_keygen")
        self.n = params.n
        self.seed = seed

    def __del__(self):
        if getattr(self, "h", None):
            self.L.eoc_secret_key_free(self.h)
            self.h = None

    @property
    def lwe_key(self):
        return _np_view(self.L.eoc_sk_lwe_key(self.h), self.n, np.int32)

    @property
    def tlwe_key(self):
        return _np_view(self.L.eoc_sk_tlwe_key(self.h), N, np.int32)

    @property
    def bk(self):
        p = self.params
        v = _np_view(self.L.eoc_sk_bk(self.h), self.L.eoc_bk_len(C.byref(p)), np.int32)
        return None if v is None else v.reshape(p.n, 2 * p.l, 2, N)

    @property
    def ksk(self):
        p = self.params
        v = _np_view(self.L.eoc_sk_ksk(self.h), self.L.eoc_ksk_len(C.byref(p)), np.int32)
        return None if v is None else v.reshape(-1, p.n + 1)

    def export_bytes(self):
        """EOCSK1 blob (params | seed | key bits)."""
        need = self.L.eoc_secret_key_export(self.h, None, 0)
        buf = (C.c_ubyte * need)()
        self.L.eoc_secret_key_export(self.h, buf, need)
        return bytes(buf)

    @classmethod
    def from_bytes(cls, blob, with_cloud_key=True):
        self = cls.__new__(cls)
        self.L = lib()
        self.h = C.c_void_p()
        _check(self.L.eoc_secret_key_import(blob, len(blob), int(with_cloud_key), C.byref(self.h)),
               "eoc_secret_key_import")
        self.params = self.L.eoc_sk_params(self.h).contents.copy()
        self.n = self.params.n
        self.seed = None
        return self

    def export_cloud_key(self):
        """EOCCK1 blob (params | bk | ksk): everything a server needs, no secret material."""
        need = self.L.eoc_cloud_key_blob_bytes(C.byref(self.params))
        buf = np.empty(need, np.uint8)
        _check(self.L.eoc_cloud_key_export(self.h, buf.ctypes.data, need), "eoc_cloud_key_export")
        return buf

    def public_key_bytes(self):
        """EOCPK1 blob (params | A | B, 8 236 bytes): the compact public key of this secret key (PublicKey)"""
        need = self.L.eoc_public_key_blob_bytes(C.byref(self.params))
        buf = (C.c_ubyte * need)()
        _check(self.L.eoc_public_key_export(self.h, buf, need), "eoc_public_key_export")
        return bytes(buf)

    def packing_key_bytes(self):
        """EOCPKS1 blob (params | t, basebit | rows [n][4][2][N]; 16.4 MB on Set A, 20.6 MB on Set B): the packing key of this
        secret key, with which a server packs LWE samples into compact lists (Engine.load_packing_key)"""
        need = self.L.eoc_packing_key_blob_bytes(C.byref(self.params))
        buf = np.empty(need, np.uint8)
        _check(self.L.eoc_packing_key_export(self.h, buf.ctypes.data, need), "eoc_packing_key_export")
        return buf

    @staticmethod
    def _lists(lists):
        lists = np.ascontiguousarray(lists, np.int32)
        if lists.ndim == 2:
            lists = lists[None]
        if lists.ndim != 3 or lists.shape[1:] != (2, N):
            raise EocError(f"lists must be [L][2][{N}], got {lists.shape}")
        return lists

    def list_phases(self, lists):
        """phases c1 - c0 s' of every slot of compact lists [L][2][N] -> [L][N] int32 (eoc_list_phases)"""
        lists = self._lists(lists)
        out = np.empty((lists.shape[0], N), np.int32)
        _check(self.L.eoc_list_phases(self.h, lists.ctypes.data, lists.shape[0], out.ctypes.data), "eoc_list_phases")
        return out

    def _decrypt_list(self, lists, count, p):
        lists = self._lists(lists)
        count = lists.shape[0] * N if count is None else int(count)
        if count > lists.shape[0] * N:
            raise EocError(f"{lists.shape[0]} lists hold at most {lists.shape[0] * N} messages, not {count}")
        out = np.empty(count, np.uint8)
        if p is None:
            _check(self.L.eoc_decrypt_list_bits(self.h, lists.ctypes.data, count, out.ctypes.data), "eoc_decrypt_list_bits")
        else:
            _check(self.L.eoc_decrypt_list_ints(self.h, int(p), lists.ctypes.data, count, out.ctypes.data),
                   "eoc_decrypt_list_ints")
        return out

    def decrypt_list_bits(self, lists, count=None):
        """the first `count` slots of compact lists [L][2][N] as bits (phase > 0), count = L N unless given"""
        return self._decrypt_list(lists, count, None)

    def decrypt_list_ints(self, lists, p, count=None):
        """the first `count` slots of compact lists as integers of Z_p (decrypt_ints' rule)"""
        return self._decrypt_list(lists, count, p)

    def encrypt_bits(self, bits, enc_seed, first_idx=0):
        bits = np.ascontiguousarray(np.asarray(bits).ravel(), np.uint8)
        out = np.empty((bits.size, self.n + 1), np.int32)
        _check(self.L.eoc_encrypt_bits(self.h, enc_seed, first_idx, bits.ctypes.data, bits.size, out.ctypes.data),
               "eoc_encrypt_bits")
        return out

    def decrypt_bits(self, cts):
        cts = np.ascontiguousarray(cts, np.int32).reshape(-1, self.n + 1)
        out = np.empty(cts.shape[0], np.uint8)
        _check(self.L.eoc_decrypt_bits(self.h, cts.ctypes.data, cts.shape[0], out.ctypes.data), "eoc_decrypt_bits")
        return out

    def phase(self, ct):
        ct = np.ascontiguousarray(ct, np.int32)
        return self.L.eoc_lwe_phase(self.h, ct.ctypes.data)

    def encrypt_ints(self, values, p, enc_seed, first_idx=0):
        """Small integers for table lookups (eoc_encrypt_ints): m in Z_p, p in {2, 4, 8}, at phase m / (2p); the upper
        half of the torus is padding.  Sample s uses stream (enc_seed, first_idx + s), as encrypt_bits.

        Ciphertexts add as arrays: `cx + cy` on the int32 arrays -- a wrapping int32 addition -- encrypts x + y while
        the sum stays below p.  Example: x, y in Z_4 encrypted at p = 8, then one lookup:

            cx, cy = sk.encrypt_ints(x, 8, 1), sk.encrypt_ints(y, 8, 2)
            s = cx + cy                                             # x + y in Z_8 (x + y <= 6: no wrap-around)
            out = lut_batch(8, [[f(m) for m in range(8)]], s)       # f(m) as Torus32 output values
        At p = 8 a sum of two fresh ciphertexts has a decision margin of 4.9 sigma on Set A (5.7 on Set B): about one
        lookup in 10^6 decodes the wrong m on Set A (computed with noise.predict).  One input: 6.6 sigma."""
        values = np.ascontiguousarray(np.asarray(values).ravel(), np.uint8)
        out = np.empty((values.size, self.n + 1), np.int32)
        _check(self.L.eoc_encrypt_ints(self.h, enc_seed, first_idx, int(p), values.ctypes.data, values.size,
                                       out.ctypes.data), "eoc_encrypt_ints")
        return out

    def encrypt_selector_bits(self, bits, enc_seed, first_idx=0):
        """TGSW selectors of `bits` for Engine.cmux_device / table_read (eoc_tgsw_encrypt_bits): [len(bits)][2l][2][N] int32
        in torus form, the shape of one bootstrapping-key block.  enc_seed an int: the reproducible test streams (enc_seed,
        first_idx + s) -- NOT secure, refused for a secure-mode key.  enc_seed None: ChaCha20 streams under a fresh key from
        the OS, drawn per call (a repeated (key, index) pair repeats mask and noise)."""
        bits = np.ascontiguousarray(np.asarray(bits).ravel(), np.uint8)
        p = self.params
        out = np.empty((bits.size, 2 * p.l, 2, N), np.int32)
        if enc_seed is not None:
            _check(self.L.eoc_tgsw_encrypt_bits(self.h, int(enc_seed), int(first_idx), bits.ctypes.data, bits.size,
                                                out.ctypes.data), "eoc_tgsw_encrypt_bits")
            return out
        if first_idx:
            raise EocError("first_idx is a test-mode argument: secure encryption draws a fresh key per call")
        key = np.frombuffer(os.urandom(32), np.uint8).copy()
        try:
            _check(self.L.eoc_tgsw_encrypt_bits_keyed(self.h, key.ctypes.data, 0, bits.ctypes.data, bits.size,
                                                      out.ctypes.data), "eoc_tgsw_encrypt_bits_keyed")
        finally:
            key[:] = 0
        return out

    def encrypt_index(self, index, nbits, enc_seed, first_idx=0):
        """The selectors of an encrypted table index: bits of `index` LSB first, [nbits][2l][2][N] (table_read's order)"""
        index, nbits = int(index), int(nbits)
        if index < 0 or index >> nbits:
            raise EocError(f"encrypt_index: {index} does not fit {nbits} bits")
        return self.encrypt_selector_bits([(index >> k) & 1 for k in range(nbits)], enc_seed, first_idx)

    # -- seeded forms: a public 32-byte mask seed and the bodies; the receiver regenerates the masks ----------
    def _seeded_lwe(self, values, p, enc_key, mask_seed, first_idx):
        values = np.ascontiguousarray(np.asarray(values).ravel(), np.uint8)
        bodies = np.empty(values.size, np.int32)
        if enc_key is None and mask_seed is None:       # secure: seed AND noise key fresh from the OS, per call
            if first_idx:
                raise EocError("first_idx is a test-mode argument: secure seeded encryption draws a fresh seed per call")
            seed = np.zeros(32, np.uint8)
            rc = (self.L.eoc_seeded_encrypt_bits(self.h, values.ctypes.data, values.size, seed.ctypes.data, bodies.ctypes.data)
                  if p is None else
                  self.L.eoc_seeded_encrypt_ints(self.h, int(p), values.ctypes.data, values.size, seed.ctypes.data,
                                                 bodies.ctypes.data))
            _check(rc, "eoc_seeded_encrypt")
            return seed.tobytes(), bodies
        k, s = _key32(enc_key, "enc_key"), _key32(mask_seed, "mask_seed")
        rc = (self.L.eoc_seeded_encrypt_bits_keyed(self.h, k.ctypes.data, s.ctypes.data, int(first_idx), values.ctypes.data,
                                                   values.size, bodies.ctypes.data) if p is None else
              self.L.eoc_seeded_encrypt_ints_keyed(self.h, k.ctypes.data, s.ctypes.data, int(first_idx), int(p),
                                                   values.ctypes.data, values.size, bodies.ctypes.data))
        _check(rc, "eoc_seeded_encrypt_keyed")
        return s.tobytes(), bodies

    def encrypt_bits_seeded(self, bits, enc_key=None, mask_seed=None, first_idx=0):
        """bits -> (seed, bodies): a 32-byte PUBLIC mask seed and one int32 body per bit; Engine.seeded_expand_device,
        seeded_expand or seeded_expand_host turn them into encrypt_bits' samples [count][n+1].  By default the seed and the
        noise key are drawn fresh from the OS per call.  enc_key / mask_seed (32 bytes each) and first_idx are the TEST-ONLY
        keyed form: a (seed, index) pair must never mask two encryptions under one key."""
        return self._seeded_lwe(bits, None, enc_key, mask_seed, first_idx)

    def encrypt_ints_seeded(self, values, p, enc_key=None, mask_seed=None, first_idx=0):
        """small integers m < p (encrypt_ints' encoding) -> (seed, bodies); randomness as encrypt_bits_seeded"""
        return self._seeded_lwe(values, p, enc_key, mask_seed, first_idx)

    def encrypt_selector_bits_seeded(self, bits, enc_key=None, mask_seed=None, first_idx=0):
        """TGSW selectors of `bits` in seeded form -> (seed, bodies [len(bits)][2l][N]): half of encrypt_selector_bits'
        size; Engine.tgsw_seeded_to_fft_device converts them for cmux_device / table_read_device, tgsw_seeded_expand_host
        gives the torus form.  Randomness as encrypt_bits_seeded."""
        bits = np.ascontiguousarray(np.asarray(bits).ravel(), np.uint8)
        bodies = np.empty((bits.size, 2 * self.params.l, N), np.int32)
        if enc_key is None and mask_seed is None:
            if first_idx:
                raise EocError("first_idx is a test-mode argument: secure seeded encryption draws a fresh seed per call")
            seed = np.zeros(32, np.uint8)
            _check(self.L.eoc_tgsw_seeded_encrypt_bits(self.h, bits.ctypes.data, bits.size, seed.ctypes.data, bodies.ctypes.data),
                   "eoc_tgsw_seeded_encrypt_bits")
            return seed.tobytes(), bodies
        k, s = _key32(enc_key, "enc_key"), _key32(mask_seed, "mask_seed")
        _check(self.L.eoc_tgsw_seeded_encrypt_bits_keyed(self.h, k.ctypes.data, s.ctypes.data, int(first_idx), bits.ctypes.data,
                                                         bits.size, bodies.ctypes.data), "eoc_tgsw_seeded_encrypt_bits_keyed")
        return s.tobytes(), bodies

    def seeded_cloud_key_bytes(self):
        """EOCCKS1 blob (params | seed | BK bodies | KSK bodies; 8.3 MB on Set A, 15.6 MB on Set B): a fresh, independent
        encryption of this key's cloud key whose masks a server regenerates from the seed (Engine.from_seeded_cloud_key_blob,
        global_import_seeded_cloud_key_blob, seeded_cloud_key_expand).  Deterministic: every export gives the same bytes."""
        need = self.L.eoc_seeded_cloud_key_blob_bytes(C.byref(self.params))
        buf = np.empty(need, np.uint8)
        _check(self.L.eoc_seeded_cloud_key_export(self.h, buf.ctypes.data, need), "eoc_seeded_cloud_key_export")
        return buf

    def decrypt_ints(self, cts, p):
        """round(phase * 2p / 2^32) mod p (eoc_decrypt_ints)"""
        cts = np.ascontiguousarray(cts, np.int32).reshape(-1, self.n + 1)
        out = np.empty(cts.shape[0], np.uint8)
        _check(self.L.eoc_decrypt_ints(self.h, int(p), cts.ctypes.data, cts.shape[0], out.ctypes.data), "eoc_decrypt_ints")
        return out


class PublicKey:
    """Compact public key (EOCPK1 blob): anyone holding it encrypts into compact lists -- one TLWE sample
    [2][N] int32 carries N = 1024 messages -- which a server turns into LWE samples with the cloud key alone
    (Engine.compact_expand_device, compact_expand).  Encryption runs on the CPU."""

    def __init__(self, blob):
        self.L = lib()
        self.blob = bytes(blob)
        self.params = Params()
        _check(self.L.eoc_public_key_blob_params(self.blob, len(self.blob), C.byref(self.params)),
               "eoc_public_key_blob_params")
        self.n = self.params.n

    @classmethod
    def from_bytes(cls, blob):
        return cls(blob)

    def to_bytes(self):
        return self.blob

    @property
    def A(self):
        return np.frombuffer(self.blob, np.int32, N, len(self.blob) - 8 * N)

    @property
    def B(self):
        return np.frombuffer(self.blob, np.int32, N, len(self.blob) - 4 * N)

    @staticmethod
    def list_count(count):
        """lists that hold `count` messages"""
        return (int(count) + N - 1) // N

    def _encrypt(self, values, p, enc_seed, first_list):
        values = np.ascontiguousarray(np.asarray(values).ravel(), np.uint8)
        out = np.empty((self.list_count(values.size), 2, N), np.int32)
        if enc_seed is not None:            # reproducible test mode: NOT secure (include/eoc_tfhe_gpu.h)
            rc = (self.L.eoc_pk_encrypt_bits(self.blob, len(self.blob), enc_seed, first_list, values.ctypes.data, values.size,
                                             out.ctypes.data) if p is None else
                  self.L.eoc_pk_encrypt_ints(self.blob, len(self.blob), enc_seed, first_list, int(p), values.ctypes.data,
                                             values.size, out.ctypes.data))
            _check(rc, "eoc_pk_encrypt")
            return out
        if first_list:
            raise EocError("first_list is a test-mode argument: secure encryption draws a fresh key per call")
        key = np.frombuffer(os.urandom(32), np.uint8).copy()    # fresh per call (raises if the OS has no entropy): a
        try:                                                    # (key, list index) pair can never repeat
            rc = (self.L.eoc_pk_encrypt_bits_keyed(self.blob, len(self.blob), key.ctypes.data, 0, values.ctypes.data,
                                                   values.size, out.ctypes.data) if p is None else
                  self.L.eoc_pk_encrypt_ints_keyed(self.blob, len(self.blob), key.ctypes.data, 0, int(p), values.ctypes.data,
                                                   values.size, out.ctypes.data))
        finally:
            key[:] = 0
        _check(rc, "eoc_pk_encrypt_keyed")
        return out

    def encrypt_bits(self, bits, enc_seed=None, first_list=0):
        """bits -> compact lists [ceil(count / N)][2][N] (bits at +-2^29, the gates' encoding).  enc_seed=None: ChaCha20
        under a fresh key from the OS; an int: the reproducible test streams (enc_seed, first_list + L) -- NOT secure, and
        two calls must never cover the same (enc_seed, list index)."""
        return self._encrypt(bits, None, enc_seed, first_list)

    def encrypt_ints(self, values, p, enc_seed=None, first_list=0):
        """small integers m < p, p in {2, 4, 8} (SecretKey.encrypt_ints' encoding) -> compact lists; randomness as
        encrypt_bits"""
        return self._encrypt(values, p, enc_seed, first_list)

    def encrypt_torus(self, msgs, enc_seed=None, first_list=0):
        """arbitrary Torus32 messages (int32 per slot, e.g. x_k * Delta for Engine.linear_device) -> compact lists
        (eoc_pk_encrypt_torus); the same streams, u, e1 and e2 as encrypt_bits, randomness as encrypt_bits"""
        msgs = np.ascontiguousarray(np.asarray(msgs).ravel(), np.int32)
        out = np.empty((self.list_count(msgs.size), 2, N), np.int32)
        if enc_seed is not None:            # reproducible test mode: NOT secure (include/eoc_tfhe_gpu.h)
            _check(self.L.eoc_pk_encrypt_torus(self.blob, len(self.blob), enc_seed, first_list, msgs.ctypes.data, msgs.size,
                                               out.ctypes.data), "eoc_pk_encrypt_torus")
            return out
        if first_list:
            raise EocError("first_list is a test-mode argument: secure encryption draws a fresh key per call")
        key = np.frombuffer(os.urandom(32), np.uint8).copy()    # fresh per call, as _encrypt
        try:
            rc = self.L.eoc_pk_encrypt_torus_keyed(self.blob, len(self.blob), key.ctypes.data, 0, msgs.ctypes.data, msgs.size,
                                                   out.ctypes.data)
        finally:
            key[:] = 0
        _check(rc, "eoc_pk_encrypt_torus_keyed")
        return out


def trivial_table(messages):
    """Public data as a table for table_read (eoc_table_trivial): Torus32 messages -> trivial TLWE lists [L][2][N], c0 = 0,
    c1 = the messages, zero-padded to whole lists"""
    messages = np.ascontiguousarray(np.asarray(messages).ravel(), np.int32)
    out = np.empty((max(1, -(-messages.size // N)), 2, N), np.int32)
    if messages.size == 0:
        out[:] = 0
        return out
    _check(lib().eoc_table_trivial(messages.ctypes.data, messages.size, out.ctypes.data), "eoc_table_trivial")
    return out


def lut_test_polynomial(p, table):
    """Test polynomial [N] int32 of `table` (eoc_lut_test_polynomial): table[m], m < p in {2, 4, 8}, is the Torus32
    OUTPUT value for input m -- +-2^29 gives a bit ciphertext (the gates' encoding), k * 2^32 / (2p') an integer of
    Z_p'.  tv[k] = table[round(k p / N)] for k < N - N / (2p), -table[0] for the last N / (2p) coefficients; an input in
    the padding half (m in [p, 2p)) yields -table[m - p]."""
    table = np.ascontiguousarray(np.asarray(table, np.int64).astype(np.int32).ravel())
    if table.size != int(p):
        raise EocError(f"lut_test_polynomial: table has {table.size} entries, p = {p}")
    tv = np.empty(N, np.int32)
    _check(lib().eoc_lut_test_polynomial(int(p), table.ctypes.data, tv.ctypes.data), "eoc_lut_test_polynomial")
    return tv


def lut_many_test_polynomial(p, tables):
    """Packed test polynomial [N] int32 of T = len(tables) tables (eoc_lut_many_test_polynomial): tables
    [T][p] of Torus32 output values as in lut_test_polynomial, T in {2, 4, 8}, p T <= 16.  tv[kT + j] = table j's
    lut_test_polynomial coefficient kT: one blind rotation on the T-grid gives all T lookups (Engine.lut_many_batch_device)."""
    tables = np.ascontiguousarray(np.asarray(tables, np.int64).astype(np.int32))
    if tables.ndim != 2 or tables.shape[1] != int(p):
        raise EocError(f"lut_many_test_polynomial: tables must be [T][p], got {tables.shape} for p = {p}")
    tv = np.empty(N, np.int32)
    _check(lib().eoc_lut_many_test_polynomial(int(p), tables.shape[0], tables.ctypes.data, tv.ctypes.data),
           "eoc_lut_many_test_polynomial")
    return tv


def lut2_test_polynomials(p, table, n_tables=1):
    """Level-1 test polynomials [p / T][N] int32 of ONE two-input function (eoc_lut2_test_polynomials): table
    [p][p] of Torus32 output values, table[x][y]; T = max(n_tables, 1) in {1, 2, 4, 8} divides p, p T <= 16 for T > 1.
    Polynomial g holds the tables x -> F(x, y), y = g T .. g T + T - 1 (lut_many_test_polynomial's layout for T > 1)."""
    table = np.ascontiguousarray(np.asarray(table, np.int64).astype(np.int32))
    if table.shape != (int(p), int(p)):
        raise EocError(f"lut2_test_polynomials: table must be [p][p], got {table.shape} for p = {p}")
    T = max(int(n_tables), 1)
    tv = np.empty((max(int(p) // T, 1), N), np.int32)
    _check(lib().eoc_lut2_test_polynomials(int(p), int(n_tables), table.ctypes.data, tv.ctypes.data), "eoc_lut2_test_polynomials")
    return tv


def lut_tree_test_polynomials(p, d, table, n_tables=1):
    """Level-1 test polynomials [p^(d-1) / T][N] int32 of ONE function on Z_p^d (eoc_lut_tree_test_polynomials):
    table of p^d Torus32 output values (any shape), table[x_1]..[x_d].  Level-1 table J = j_2 + p j_3 + p^2 j_4 (j_2 fastest)
    is x_1 -> F(x_1, j_2, .., j_d); polynomial g holds the tables J = g T .. g T + T - 1."""
    p, d = int(p), int(d)
    table = np.ascontiguousarray(np.asarray(table, np.int64).astype(np.int32)).reshape(-1)
    if not 2 <= d <= 4 or table.size != p ** d:
        raise EocError(f"lut_tree_test_polynomials: table must hold p^d values with 2 <= d <= 4, got {table.size} for p = {p}, d = {d}")
    T = max(int(n_tables), 1)
    tv = np.empty((max(p ** (d - 1) // T, 1), N), np.int32)
    _check(lib().eoc_lut_tree_test_polynomials(p, d, int(n_tables), table.ctypes.data, tv.ctypes.data),
           "eoc_lut_tree_test_polynomials")
    return tv


class Engine:
    """One HIP engine (one GPU).  All array arguments are DEVICE pointers (ints) unless noted."""

    def __init__(self, params, device=0):
        self.L = lib()
        self.h = C.c_void_p()
        self.params = params.copy()
        _check(self.L.eoc_engine_create(device, C.byref(self.params), C.byref(self.h)), "eoc_engine_create")
        self.device = device
        self.n = params.n

    @classmethod
    def from_cloud_key_blob(cls, blob, device=0):
        """Server side: engine + key images from an EOCCK1 blob alone."""
        blob = np.ascontiguousarray(blob, np.uint8)
        self = cls.__new__(cls)
        self.L = lib()
        self.h = C.c_void_p()
        self.params = Params()
        _check(self.L.eoc_cloud_key_blob_params(blob.ctypes.data, blob.size, C.byref(self.params)),
               "eoc_cloud_key_blob_params")
        _check(self.L.eoc_engine_create_from_cloud_key_blob(device, blob.ctypes.data, blob.size, C.byref(self.h)),
               "eoc_engine_create_from_cloud_key_blob")
        self.device = device
        self.n = self.params.n
        return self

    @classmethod
    def borrow_global(cls, index=0):
        """Wrapper around engine `index` of the process-global context (eoc_gpu_init[_multi]): the same engine the
        host-buffer API drives, reachable through the device-pointer API too.  Not owned: close() leaves it alone."""
        self = cls.__new__(cls)
        self.L = lib()
        h = self.L.eoc_global_engine_at(index)
        if not h:
            raise EocError("borrow_global: no global engine (eoc_gpu_init not called)")
        self.h = C.c_void_p(h)
        self._borrowed = True
        self.params = self.L.eoc_engine_params(self.h).contents.copy()
        self.device = self.L.eoc_engine_device(self.h)
        self.n = self.params.n
        return self

    def close(self):
        if getattr(self, "h", None):
            if not getattr(self, "_borrowed", False):
                self.L.eoc_engine_destroy(self.h)
            self.h = None

    def __del__(self):
        self.close()

    # -- cloud key ---------------------------------------------------------------------------
    def load_cloud_key(self, sk_or_bk, ksk=None):
        """Host torus-form BK/KSK -> device images (forward transform runs on the GPU)."""
        if isinstance(sk_or_bk, SecretKey):
            bk, ksk = sk_or_bk.bk, sk_or_bk.ksk
        else:
            bk = sk_or_bk
        bk = np.ascontiguousarray(bk, np.int32)
        ksk = np.ascontiguousarray(ksk, np.int32)
        _check(self.L.eoc_engine_load_cloud_key(self.h, bk.ctypes.data, ksk.ctypes.data), "eoc_engine_load_cloud_key")

    def build_cloud_key_device(self, sk, d_bkfft, d_ksk):
        """Like load_cloud_key but into caller-owned device buffers (e.g. torch tensors)."""
        bk = np.ascontiguousarray(sk.bk, np.int32)
        ksk = np.ascontiguousarray(sk.ksk, np.int32)
        _check(self.L.eoc_engine_build_cloud_key_device(self.h, bk.ctypes.data, ksk.ctypes.data, d_bkfft, d_ksk),
               "eoc_engine_build_cloud_key_device")

    def set_profiling(self, on=True):
        _check(self.L.eoc_engine_set_profiling(self.h, int(on)), "eoc_engine_set_profiling")

    def kernel_times(self, reset=True):
        ms, cnt = (C.c_double * 3)(), (C.c_uint64 * 3)()
        _check(self.L.eoc_engine_kernel_times(self.h, C.byref(ms), C.byref(cnt), int(reset)), "eoc_engine_kernel_times")
        names = ("prepare", "blind_rotate", "keyswitch")
        return {k: dict(ms=ms[i], launches=cnt[i]) for i, k in enumerate(names)}

    def set_cloud_key_device(self, d_bkfft, d_ksk):
        _check(self.L.eoc_engine_set_cloud_key_device(self.h, d_bkfft, d_ksk), "eoc_engine_set_cloud_key_device")

    def cloud_key_device(self):
        a, b = C.c_void_p(), C.c_void_p()
        _check(self.L.eoc_engine_cloud_key_device(self.h, C.byref(a), C.byref(b)), "eoc_engine_cloud_key_device")
        return a.value, b.value

    def download(self, d_ptr, nbytes, dtype=np.uint8):
        """device -> host numpy copy of a raw buffer"""
        out = np.empty(nbytes // np.dtype(dtype).itemsize, dtype)
        _check(self.L.eoc_device_to_host(self.h, out.ctypes.data, d_ptr, nbytes), "eoc_device_to_host")
        return out

    def synchronize(self):
        _check(self.L.eoc_engine_synchronize(self.h), "eoc_engine_synchronize")

    @property
    def bkfft_bytes(self):
        return self.L.eoc_bkfft_bytes(C.byref(self.params))

    @property
    def ksk_dev_bytes(self):
        return self.L.eoc_ksk_dev_bytes(C.byref(self.params))

    # -- hot path ----------------------------------------------------------------------------
    def gate_batch_device(self, op, d_in0, d_in1, d_in2, d_out, count, ops=None, stream=None):
        ops_p = None
        if ops is not None:
            ops = np.ascontiguousarray(ops, np.uint8)
            ops_p = ops.ctypes.data
        _check(self.L.eoc_gate_batch_device(self.h, int(op), ops_p, d_in0, d_in1, d_in2, d_out, count, stream),
               "eoc_gate_batch_device")

    def circuit_run_device(self, gates, d_wires, n_wires, instances, stream=None):
        arr = (Gate * len(gates))(*gates)
        _check(self.L.eoc_circuit_run_device(self.h, C.addressof(arr), len(gates), d_wires, n_wires, instances, stream),
               "eoc_circuit_run_device")

    def fft_fwd_device(self, d_polys, d_specs, count, stream=None):
        _check(self.L.eoc_dbg_fft_fwd_device(self.h, d_polys, d_specs, count, stream), "eoc_dbg_fft_fwd_device")

    def fft_inv_device(self, d_specs, d_polys, count, stream=None):
        _check(self.L.eoc_dbg_fft_inv_device(self.h, d_specs, d_polys, count, stream), "eoc_dbg_fft_inv_device")

    def blind_rotate_device(self, d_t, d_u, count, stream=None):
        _check(self.L.eoc_blind_rotate_device(self.h, d_t, d_u, count, stream), "eoc_blind_rotate_device")

    def keyswitch_device(self, d_u, d_out, count, stream=None):
        _check(self.L.eoc_keyswitch_device(self.h, d_u, d_out, count, stream), "eoc_keyswitch_device")

    def lut_batch_device(self, d_tv, n_luts, d_in, d_out, count, stream=None):
        """Table lookups (eoc_lut_batch_device): d_tv [n_luts][N] test polynomials (lut_test_polynomial), d_in
        [count][n+1], d_out [n_luts][count][n+1]; every table on every row in one level of n_luts x count bootstraps.
        Encoding and supported p: SecretKey.encrypt_ints."""
        _check(self.L.eoc_lut_batch_device(self.h, d_tv, n_luts, d_in, d_out, count, stream), "eoc_lut_batch_device")

    def lut_many_batch_device(self, n_tables, d_tv, n_luts, d_in, d_out, count, stream=None):
        """Many-LUT lookups (eoc_lut_many_batch_device): d_tv [n_luts][N] packed polynomials of T = n_tables tables each
        (lut_many_test_polynomial), d_in [count][n+1], d_out [n_luts][T][count][n+1]; one blind rotation per (polynomial,
        row) and T key switches."""
        _check(self.L.eoc_lut_many_batch_device(self.h, int(n_tables), d_tv, n_luts, d_in, d_out, count, stream),
               "eoc_lut_many_batch_device")

    def int_circuit_run_device(self, nodes, d_tv, n_tv, d_wires, n_wires, instances, stream=None):
        """Integer circuit (eoc_int_circuit_run_device): nodes = list of INode (IntCircuit.nodes()), d_tv
        [n_tv][N] test polynomials, d_wires [n_wires][instances][n+1]; one blind rotation per (level, T) group of nodes."""
        arr = _inode_array(nodes)
        _check(self.L.eoc_int_circuit_run_device(self.h, C.addressof(arr), len(nodes), d_tv, n_tv, d_wires, n_wires,
                                                 instances, stream), "eoc_int_circuit_run_device")

    def compact_expand_device(self, d_lists, count, d_out, stream=None):
        """Compact lists -> LWE samples (eoc_compact_expand_device): d_lists [ceil(count / N)][2][N] (PublicKey.encrypt_*),
        d_out [count][n+1]; slot extraction and the key switch, with the key-switch key alone"""
        _check(self.L.eoc_compact_expand_device(self.h, d_lists, count, d_out, stream), "eoc_compact_expand_device")

    # -- seeded forms -----------------------------------------------------------
    @classmethod
    def from_seeded_cloud_key_blob(cls, blob, device=0):
        """Server side: engine + key images from an EOCCKS1 blob alone; the masks are expanded on the GPU."""
        blob = _blob_u8(blob)
        self = cls.__new__(cls)
        self.L = lib()
        self.h = C.c_void_p()
        self.params = seeded_cloud_key_params(blob)
        _check(self.L.eoc_engine_create_from_seeded_cloud_key_blob(device, blob.ctypes.data, blob.size, C.byref(self.h)),
               "eoc_engine_create_from_seeded_cloud_key_blob")
        self.device = device
        self.n = self.params.n
        return self

    def load_seeded_cloud_key(self, blob):
        """EOCCKS1 blob -> device images: bodies uploaded, masks expanded on the GPU, then load_cloud_key's transform"""
        blob = _blob_u8(blob)
        _check(self.L.eoc_engine_load_seeded_cloud_key(self.h, blob.ctypes.data, blob.size), "eoc_engine_load_seeded_cloud_key")

    def seeded_expand_device(self, seed, d_bodies, count, d_out, first_idx=0, stream=None):
        """(seed, d_bodies [count]) -> d_out [count][n+1] (eoc_seeded_expand_device): SecretKey.encrypt_*_seeded's samples,
        masks regenerated by k_seed_masks.  Needs no key; d_out must not overlap d_bodies."""
        s = _key32(seed, "seed")
        _check(self.L.eoc_seeded_expand_device(self.h, s.ctypes.data, int(first_idx), d_bodies, count, d_out, stream),
               "eoc_seeded_expand_device")

    def tgsw_seeded_to_fft_device(self, seed, d_bodies, count, d_fft, first_idx=0, stream=None):
        """(seed, d_bodies [count][2l][N]) -> converted selectors d_fft (tgsw_fft_bytes each), byte for byte what
        tgsw_to_fft_device gives for the host-expanded selectors (eoc_tgsw_seeded_to_fft_device)"""
        s = _key32(seed, "seed")
        _check(self.L.eoc_tgsw_seeded_to_fft_device(self.h, s.ctypes.data, int(first_idx), d_bodies, count, d_fft, stream),
               "eoc_tgsw_seeded_to_fft_device")

    @property
    def seed_launches(self):
        return self.L.eoc_engine_seed_launches(self.h)

    @property
    def tgsw_fft_bytes(self):
        """bytes of one converted selector (eoc_tgsw_fft_bytes): 64 KiB on Set A, 96 KiB on Set B"""
        return self.L.eoc_tgsw_fft_bytes(C.byref(self.params))

    def tgsw_to_fft_device(self, d_tgsw, count, d_fft, stream=None):
        """Selectors in torus form [count][2l][2][N] -> the form the kernels multiply by, [count][2l][2][512] complex
        (eoc_tgsw_to_fft_device; tgsw_fft_bytes each).  Needs no key."""
        _check(self.L.eoc_tgsw_to_fft_device(self.h, d_tgsw, count, d_fft, stream), "eoc_tgsw_to_fft_device")

    @property
    def leveled_rounding(self):
        """the rounding mode of the leveled calls (eoc_engine_set_leveled_rounding): False, the default, is the
        oracle's truncating gadget; True makes cmux_device, table_read_device, demux_device, table_update_device,
        automaton_step_device and automaton_run_device round, which removes the mean that bounds long leveled chains
        (noise.automaton_budget(rounding=True)).  Nothing else is governed by it.  Setting it while a graph capture holds
        leveled calls of this engine raises EocError."""
        return bool(self.L.eoc_engine_leveled_rounding(self.h))

    @leveled_rounding.setter
    def leveled_rounding(self, on):
        _check(self.L.eoc_engine_set_leveled_rounding(self.h, 1 if on else 0), "eoc_engine_set_leveled_rounding")

    def cmux_device(self, d_sel_fft, d_in0, d_in1, d_out, count, stream=None):
        """out[i] = in0[i] + C[i] (x) (in1[i] - in0[i]) on TLWE samples [count][2][N], one converted selector per item
        (eoc_cmux_device): in1 where the bit is 1, in0 otherwise.  Needs no key."""
        _check(self.L.eoc_cmux_device(self.h, d_sel_fft, d_in0, d_in1, d_out, count, stream), "eoc_cmux_device")

    def table_read_device(self, d_table, log2_lists, log2_width, d_sel_fft, queries, d_out, stream=None):
        """Entry idx_q of a table for each of `queries` encrypted indices (eoc_table_read_device): d_table [2^d][2][N], entries
        of W = 2^log2_width slots, d_sel_fft [queries][10 - log2_width + d] converted selectors (index bits LSB first), d_out
        [queries][W][n+1] -- ordinary gate / LUT inputs"""
        _check(self.L.eoc_table_read_device(self.h, d_table, int(log2_lists), int(log2_width), d_sel_fft, queries, d_out,
                                            stream), "eoc_table_read_device")

    def demux_device(self, d_sel_fft, d_in, d_out0, d_out1, count, accumulate=False, stream=None):
        """E = C[i] (x) in[i]; out1[i] = E, out0[i] = in[i] - E on TLWE samples [count][2][N], one converted selector per item
        (eoc_demux_device): in[i] goes to out1 where the bit is 1 and to out0 otherwise.  accumulate adds into the outputs
        (integer atomics) instead of storing.  Needs no key."""
        _check(self.L.eoc_demux_device(self.h, d_sel_fft, d_in, d_out0, d_out1, count, 1 if accumulate else 0, stream),
               "eoc_demux_device")

    def table_update_device(self, d_table, log2_lists, log2_width, d_sel_fft, d_vals, queries, stream=None):
        """table[idx_q] += value_q in place for each of `queries` encrypted indices (eoc_table_update_device): d_table
        [2^d][2][N], d_sel_fft as table_read_device's (None at d = 0, log2_width = 10), d_vals [queries][2][N] TLWE samples with
        the entry's W messages in slots 0 .. W-1 and 0 elsewhere.  Needs no key."""
        _check(self.L.eoc_table_update_device(self.h, d_table, int(log2_lists), int(log2_width), d_sel_fft, d_vals, queries,
                                              stream), "eoc_table_update_device")

    def load_packing_key(self, blob):
        """Install an EOCPKS1 blob (SecretKey.packing_key_bytes) as this engine's packing key (eoc_engine_set_packing_key);
        replaces an earlier one.  The blob's parameters must be the engine's."""
        blob = np.ascontiguousarray(np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray)) else blob, np.uint8)
        _check(self.L.eoc_engine_set_packing_key(self.h, blob.ctypes.data, blob.size), "eoc_engine_set_packing_key")

    def pack_device(self, d_in, count, d_lists, stream=None):
        """LWE samples -> compact lists (eoc_pack_device): d_in [count][n+1], d_lists [ceil(count / N)][2][N]; sample i goes
        to slot i mod N of list i / N.  Needs the packing key alone."""
        _check(self.L.eoc_pack_device(self.h, d_in, count, d_lists, stream), "eoc_pack_device")

    def lut_enc_batch_device(self, d_lists, n_groups, per_row, d_in, d_out, count, stream=None):
        """Blind rotation from ENCRYPTED polynomials (eoc_lut_enc_batch_device): d_lists TLWE samples [..][2][N]
        (pack_device / tv_pack_device outputs, PublicKey.encrypt_*, trivial_table), d_in [count][n+1], d_out
        [n_groups][count][n+1].  Job (g, s) starts from list g (per_row false) or list g x count + s (per_row true), is rotated
        by input row s, extracted and key-switched.  Needs the cloud key alone."""
        _check(self.L.eoc_lut_enc_batch_device(self.h, d_lists, n_groups, 1 if per_row else 0, d_in, d_out, count, stream),
               "eoc_lut_enc_batch_device")

    def automaton_step_device(self, trans, d_prev, prev_query_stride, d_sel_fft, sel_query_stride, d_next, queries, stream=None):
        """One backward step of a public automaton for every state and query (eoc_automaton_step_device):
        next[q] = A + C (x) (B - A), A = X^(-w0) prev[next0(q)], B = X^(-w1) prev[next1(q)].  trans: an Automaton or host
        records [states][4] = (next0, w0, next1, w1); d_prev [states][2][N] per query, prev_query_stride TLWE samples between
        the queries' vectors (0: one shared vector); the selector of query q lies sel_query_stride selectors behind query
        q - 1's; d_next [queries][states][2][N].  Needs no key."""
        t = _automaton_records(trans)
        _check(self.L.eoc_automaton_step_device(self.h, t.ctypes.data, t.shape[0], d_prev, int(prev_query_stride), d_sel_fft,
                                                int(sel_query_stride), d_next, queries, stream), "eoc_automaton_step_device")

    def automaton_run_device(self, trans, d_final, d_sel_fft, steps, starts, log2_width, d_out, queries, stream=None):
        """A public automaton over `queries` encrypted bit strings of `steps` bits (eoc_automaton_run_device):
        d_final [states][2][N] (trivial_table or encrypted lists), d_sel_fft [queries][steps] converted selectors (bit 0 is
        read first; None at steps = 0), starts: host state ids, d_out [queries][len(starts)][2^log2_width][n+1] ordinary
        LWE samples.  No bootstrap: mean and variance of the error grow linearly in `steps` (noise.automaton_budget says how
        far).  Only the key switch needs the cloud key."""
        t = _automaton_records(trans)
        st = np.ascontiguousarray(np.atleast_1d(starts), np.int32)
        _check(self.L.eoc_automaton_run_device(self.h, t.ctypes.data, t.shape[0], d_final, d_sel_fft, int(steps), st.ctypes.data,
                                               st.size, int(log2_width), d_out, queries, stream), "eoc_automaton_run_device")

    def weights_image_bytes(self, rows, cols):
        """bytes of the device image of a rows x cols model (eoc_weights_image_bytes)"""
        return int(self.L.eoc_weights_image_bytes(int(rows), int(cols)))

    def weights_to_device(self, weights, d_image, stream=None):
        """Public int8 weights [rows][cols], every value in [-127, 127] -> the device image at d_image
        (eoc_weights_to_device; weights_image_bytes(rows, cols) bytes: the spectra [rows][L][512] complex, then the zero-padded
        weights).  A model load: no key, synchronous.  Returns (rows, cols)."""
        w = np.asarray(weights)
        if w.ndim != 2 or w.size == 0 or not np.issubdtype(w.dtype, np.integer) or np.abs(w.astype(np.int64)).max() > 127:
            raise EocError(f"weights_to_device: weights must be a non-empty integer matrix [rows][cols] in [-127, 127], got "
                           f"{w.dtype} {w.shape}")
        w = np.ascontiguousarray(w, np.int8)
        _check(self.L.eoc_weights_to_device(self.h, w.ctypes.data, w.shape[0], w.shape[1], d_image, stream), "eoc_weights_to_device")
        return w.shape

    def dot_device(self, d_image, rows, cols, d_lists, batch, d_bias, d_u, stream=None):
        """Inner products with public weights (eoc_dot_device): d_lists [batch][ceil(cols / N)][2][N], d_bias
        [rows] Torus32 or None, d_u [batch][rows][N+1]: LWE samples under s' (keyswitch_device's input).  No key needed."""
        _check(self.L.eoc_dot_device(self.h, d_image, rows, cols, d_lists, batch, d_bias, d_u, stream), "eoc_dot_device")

    def linear_device(self, d_image, rows, cols, d_lists, batch, d_bias, d_out, stream=None):
        """dot_device followed by the key switch (eoc_linear_device): d_out [batch][rows][n+1], ordinary LWE samples of phase
        bias[r] + sum_k w[r][k] phase(slot k of vector b).  Needs the cloud key."""
        _check(self.L.eoc_linear_device(self.h, d_image, rows, cols, d_lists, batch, d_bias, d_out, stream), "eoc_linear_device")

    def dot_launches(self):
        """k_dot_mask launches so far (eoc_engine_dot_launches): one per slice of a call's input vectors"""
        return int(self.L.eoc_engine_dot_launches(self.h))

    def lwe_weights_image_bytes(self, rows, cols):
        """bytes of the device image of a rows x cols model of lwe_matmul_device (eoc_lwe_weights_image_bytes; 0 for a shape
        that is refused: rows in [1, 2^20], cols in [1, 2^16])"""
        return int(self.L.eoc_lwe_weights_image_bytes(int(rows), int(cols)))

    def lwe_weights_to_device(self, weights, d_image, stream=None):
        """Public int8 weights [rows][cols], every value in [-127, 127] -> the matrix-core operand image at d_image
        (eoc_lwe_weights_to_device; lwe_weights_image_bytes(rows, cols) bytes).  A model load: no key, synchronous.
        Returns (rows, cols)."""
        w = np.asarray(weights)
        if w.ndim != 2 or w.size == 0 or not np.issubdtype(w.dtype, np.integer) or np.abs(w.astype(np.int64)).max() > 127:
            raise EocError(f"lwe_weights_to_device: weights must be a non-empty integer matrix [rows][cols] in [-127, 127], got "
                           f"{w.dtype} {w.shape}")
        w = np.ascontiguousarray(w, np.int8)
        _check(self.L.eoc_lwe_weights_to_device(self.h, w.ctypes.data, w.shape[0], w.shape[1], d_image, stream),
               "eoc_lwe_weights_to_device")
        return w.shape

    def lwe_matmul_device(self, d_image, rows, cols, d_cts, width, batch, d_bias, d_out, stream=None):
        """A public int8 matrix on LWE samples (eoc_lwe_matmul_device): d_cts [batch][cols][width] int32, d_bias
        [rows] Torus32 or None, d_out [batch][rows][width]: out[b][r] = sum_k w[r][k] cts[b][k] word by word mod 2^32, the bias
        on the body (last) word -- samples under the same key.  No key, no workspace; legal under capture."""
        _check(self.L.eoc_lwe_matmul_device(self.h, d_image, rows, cols, d_cts, width, batch, d_bias, d_out, stream),
               "eoc_lwe_matmul_device")

    def lwe_matmul_launches(self):
        """k_lwe_matmul launches so far (eoc_engine_lwe_matmul_launches): one per call of up to 65 535 vectors"""
        return int(self.L.eoc_engine_lwe_matmul_launches(self.h))

    def conv_slots_to_device(self, slots, lists_per_vec, d_slots, stream=None):
        """A public slot table [n_slots] (entry s: slot s mod N of list s / N of a vector's lists_per_vec lists; any order,
        repeats allowed) -> the device table at d_slots, n_slots uint32 (eoc_conv_slots_to_device).  Every entry is checked
        here, once, on the host; the run calls take the device table as it is.  Synchronous.  Returns n_slots."""
        t = np.asarray(slots)
        if t.ndim != 1 or t.size == 0 or not np.issubdtype(t.dtype, np.integer) or t.min() < 0 or t.max() >= 2**32:
            raise EocError(f"conv_slots_to_device: slots must be a non-empty vector of slot numbers, got {t.dtype} {t.shape}")
        t = np.ascontiguousarray(t, np.uint32)
        _check(self.L.eoc_conv_slots_to_device(self.h, t.ctypes.data, t.size, int(lists_per_vec), d_slots, stream),
               "eoc_conv_slots_to_device")
        return t.size

    def conv_device(self, d_image, rows, cols, d_lists, batch, d_bias, d_out_lists, stream=None):
        """Convolutions with public int8 kernels (eoc_conv_device): the image of weights_to_device, rows = output
        channels, list l of d_lists [batch][ceil(cols / N)][2][N] = input channel l, w[r][l N + k] = tap k of filter (r, l);
        d_out_lists [batch][rows][2][N]: slot t of list (b, r) has phase bias[r] + sum_l sum_k w[r][l N + k] x_l[t + k]
        (negacyclic: terms past slot N - 1 enter negated).  No key needed; the output is compact lists."""
        _check(self.L.eoc_conv_device(self.h, d_image, rows, cols, d_lists, batch, d_bias, d_out_lists, stream), "eoc_conv_device")

    def conv_linear_device(self, d_image, rows, cols, d_lists, batch, d_bias, d_slots, n_slots, d_out, stream=None):
        """conv_device into a scratch buffer, then the samples of the slot table (conv_slots_to_device with lists_per_vec =
        rows) extracted and key-switched (eoc_conv_linear_device): d_out [batch][n_slots][n+1], ordinary LWE samples.  Needs
        the cloud key."""
        _check(self.L.eoc_conv_linear_device(self.h, d_image, rows, cols, d_lists, batch, d_bias, d_slots, n_slots, d_out, stream),
               "eoc_conv_linear_device")

    def conv_extract_device(self, d_lists, lists_per_vec, batch, d_slots, n_slots, d_out, stream=None):
        """the extraction and the key switch of conv_linear_device alone (eoc_conv_extract_device): d_lists
        [batch][lists_per_vec][2][N] -> d_out [batch][n_slots][n+1].  Needs the cloud key."""
        _check(self.L.eoc_conv_extract_device(self.h, d_lists, lists_per_vec, batch, d_slots, n_slots, d_out, stream),
               "eoc_conv_extract_device")

    def conv_launches(self):
        """k_conv_lists launches so far (eoc_engine_conv_launches): one per slice of a call's input vectors"""
        return int(self.L.eoc_engine_conv_launches(self.h))

    def automaton_launches(self):
        """k_automaton_step launches so far (eoc_engine_automaton_launches): `steps` per slice of a run's queries"""
        return int(self.L.eoc_engine_automaton_launches(self.h))

    def tv_pack_device(self, p, d_vals, n_funcs, count, d_lists, stream=None):
        """LWE samples -> encrypted test polynomials (eoc_tv_pack_device): d_vals [n_funcs][p][count][n+1], d_lists
        [n_funcs][count][2][N]; list (f, s) holds values 0 .. p - 1 of row s by lut_test_polynomial's rule.  Needs the packing
        key."""
        _check(self.L.eoc_tv_pack_device(self.h, int(p), d_vals, n_funcs, count, d_lists, stream), "eoc_tv_pack_device")

    def tv_pack_exact_device(self, p, d_vals, n_funcs, count, d_lists, stream=None):
        """tv_pack_device's arguments and layouts, evaluated EXACTLY in wrapping integers on the matrix cores
        (eoc_tv_pack_exact_device): the value tv_pack_device gives within the rounding of its transforms."""
        _check(self.L.eoc_tv_pack_exact_device(self.h, int(p), d_vals, n_funcs, count, d_lists, stream), "eoc_tv_pack_exact_device")

    def lut_tree_batch_device(self, p, d, n_tables, d_tv0, n_funcs, d_digits, d_out, count, stream=None):
        """d-digit lookups F(x_1, .., x_d) (eoc_lut_tree_batch_device): d_tv0 [n_funcs][p^(d-1) / T][N]
        (lut_tree_test_polynomials per function), d_digits [d][count][n+1] (x_1 first) at message space p, d_out
        [n_funcs][count][n+1].  Needs the cloud key and the packing key."""
        _check(self.L.eoc_lut_tree_batch_device(self.h, int(p), int(d), int(n_tables), d_tv0, n_funcs, d_digits, d_out, count, stream),
               "eoc_lut_tree_batch_device")

    def lut2_batch_device(self, p, n_tables, d_tv0, n_funcs, d_x, d_y, d_out, count, stream=None):
        """Two-input lookups F(x, y) (eoc_lut2_batch_device): d_tv0 [n_funcs][p / T][N] (lut2_test_polynomials
        per function), d_x, d_y [count][n+1] at message space p, d_out [n_funcs][count][n+1].  Needs the cloud key and the
        packing key."""
        _check(self.L.eoc_lut2_batch_device(self.h, int(p), int(n_tables), d_tv0, n_funcs, d_x, d_y, d_out, count, stream),
               "eoc_lut2_batch_device")

    def resident_jobs(self):
        """blind rotations that fill the device in one launch (8 x CUs where the one-wave-per-ciphertext kernel applies,
        4 x otherwise): cut long jobs at multiples of this"""
        return int(self.L.eoc_engine_resident_jobs(self.h))

    def stats(self):
        out = (C.c_uint64 * 3)()
        _check(self.L.eoc_engine_stats(self.h, C.byref(out)), "eoc_engine_stats")
        return dict(batches=out[0], bootstraps=out[1], keyswitches=out[2],
                    br_launches=int(self.L.eoc_engine_blind_rotate_launches(self.h)),
                    br_wide_launches=int(self.L.eoc_engine_blind_rotate_wide_launches(self.h)),
                    ks_mfma_launches=int(self.L.eoc_engine_keyswitch_mfma_launches(self.h)),
                    cmux_launches=int(self.L.eoc_engine_cmux_launches(self.h)),
                    demux_launches=int(self.L.eoc_engine_demux_launches(self.h)),
                    automaton_launches=int(self.L.eoc_engine_automaton_launches(self.h)),
                    pack_launches=int(self.L.eoc_engine_pack_launches(self.h)),
                    packed_samples=int(self.L.eoc_engine_packed_samples(self.h)))


def circuit_bootstraps(gates):
    arr = (Gate * len(gates))(*gates)
    return lib().eoc_circuit_bootstraps(C.addressof(arr), len(gates))


def netlist_optimize(gates, outputs, extension_gates=True):
    """eoc_netlist_optimize(_ex): constant / NOT / COPY folding, MUX and carry fusion, dead-gate removal in the native library
    (the same rewriting as circuits.optimize).  extension_gates=False keeps the result inside libtfhe's boots* family (the
    carry as MUX instead of MAJ, no XOR3).  Raises EocError for netlists that are not single-assignment."""
    arr = (Gate * max(1, len(gates)))(*gates)
    out = (Gate * max(1, len(gates)))()
    outs = (C.c_int32 * max(1, len(outputs)))(*outputs)
    n = lib().eoc_netlist_optimize_ex(C.addressof(arr), len(gates), C.addressof(outs), len(outputs), C.addressof(out),
                                      0 if extension_gates else 1)
    if n < 0:
        raise EocError(f"eoc_netlist_optimize failed ({n}): not a single-assignment netlist?")
    return [Gate(out[k].op, out[k].in0, out[k].in1, out[k].in2, out[k].out) for k in range(n)]


def netlist_levels(gates):
    """eoc_netlist_levels: (level of every gate, number of levels, levels that hold a blind rotation)"""
    arr = (Gate * max(1, len(gates)))(*gates)
    lev = (C.c_int32 * max(1, len(gates)))()
    depth = C.c_int64(0)
    n = lib().eoc_netlist_levels(C.addressof(arr), len(gates), C.addressof(lev), C.addressof(depth))
    if n < 0:
        raise EocError(f"eoc_netlist_levels failed ({n})")
    return list(lev[:len(gates)]), int(n), int(depth.value)


def int_netlist_levels(nodes, n_wires, n_tv):
    """eoc_int_netlist_levels: (level of every node, number of bootstrap levels, blind rotations per instance).  A free
    node's level is the one in whose pre-pass it runs.  Raises EocError for a malformed netlist."""
    arr = _inode_array(nodes)
    lev = (C.c_int32 * max(1, len(nodes)))()
    boots = C.c_int64(0)
    n = lib().eoc_int_netlist_levels(C.addressof(arr), len(nodes), int(n_wires), int(n_tv), C.addressof(lev), C.addressof(boots))
    if n < 0:
        msg = lib().eoc_last_error()
        raise EocError(f"eoc_int_netlist_levels failed ({n}): {msg.decode() if msg else ''}")
    return list(lev[:len(nodes)]), int(n), int(boots.value)


def netlist_cost(gates, instances, resident_jobs=0):
    """eoc_netlist_cost: estimated run time over `instances` instances in units of 0.1 ms (the native twin of
    circuits.netlist_cost)"""
    arr = (Gate * max(1, len(gates)))(*gates)
    c = lib().eoc_netlist_cost(C.addressof(arr), len(gates), int(instances), int(resident_jobs))
    if c < 0:
        raise EocError(f"eoc_netlist_cost failed ({c})")
    return int(c)


# ---- host-buffer batch API (global context: one key, any number of GPUs), numpy in / numpy out ---------
def gpu_init(params, device=0, devices=None):
    """eoc_gpu_init / eoc_gpu_init_multi: `devices` = list of device ordinals (a device may repeat: several engines
    then share it, the one-GPU rehearsal of the N-GPU path)"""
    if devices is None:
        _check(lib().eoc_gpu_init(device, C.byref(params)), "eoc_gpu_init")
    else:
        arr = (C.c_int * len(devices))(*devices)
        _check(lib().eoc_gpu_init_multi(C.addressof(arr), len(devices), C.byref(params)), "eoc_gpu_init_multi")


def gpu_engine_count():
    return lib().eoc_gpu_engine_count()


def shard_range(total, rank, world):
    lo, hi = C.c_size_t(), C.c_size_t()
    lib().eoc_shard_range(total, rank, world, C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def stats_multi():
    """per-engine counters, key replication seconds and method of the global context"""
    n = lib().eoc_gpu_engine_count()
    buf = (C.c_uint64 * (3 * max(1, n)))()
    secs = C.c_double()
    rc = lib().eoc_stats_multi(C.addressof(buf), n, C.byref(secs))
    if rc < 0:
        _check(rc, "eoc_stats_multi")
    per = [dict(batches=buf[3 * i], bootstraps=buf[3 * i + 1], keyswitches=buf[3 * i + 2]) for i in range(n)]
    return dict(engines=per, key_broadcast_s=secs.value, key_broadcast_method=lib().eoc_key_broadcast_method().decode(),
                host_buffer_grows=int(lib().eoc_host_path_buffer_grows()),
                rccl_origin=lib().eoc_rccl_origin().decode(),
                worker_wakeups=[int(lib().eoc_worker_wakeups(i)) for i in range(n)])


class PinnedArray:
    """numpy view of pinned host memory from eoc_host_alloc (true DMA source/target of the batch API)."""

    def __init__(self, shape, dtype=np.int32):
        self.nbytes = int(np.prod(shape)) * np.dtype(dtype).itemsize
        self.ptr = lib().eoc_host_alloc(self.nbytes)
        if not self.ptr:
            raise EocError("eoc_host_alloc failed")
        buf = (C.c_char * self.nbytes).from_address(self.ptr)
        self.array = np.frombuffer(buf, dtype=dtype).reshape(shape)

    def free(self):
        if self.ptr:
            self.array = None
            lib().eoc_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def gate_batch_submit(op, in0, in1=None, in2=None, ops=None, out=None):
    """eoc_gate_batch_submit on PinnedArray-backed numpy views (C-contiguous int32 [count][n+1]); returns the ticket.
    The arrays must stay alive and untouched until gate_batch_wait(ticket)."""
    for a in (in0, in1, in2, out):
        if a is not None and (a.dtype != np.int32 or not a.flags.c_contiguous):
            raise EocError("gate_batch_submit: operands are C-contiguous int32 arrays")
    if out is None or (in0 is not None and out.shape != in0.shape):
        raise EocError("gate_batch_submit: `out` must be given and have the operands' shape")
    opsc = None if ops is None else np.ascontiguousarray(ops, np.uint8)
    t = C.c_uint64()
    _check(lib().eoc_gate_batch_submit(int(op), None if opsc is None else opsc.ctypes.data,
                                       None if in0 is None else in0.ctypes.data, None if in1 is None else in1.ctypes.data,
                                       None if in2 is None else in2.ctypes.data, out.ctypes.data, out.shape[0], C.byref(t)),
           "eoc_gate_batch_submit")
    return t.value


def gate_batch_wait(ticket):
    _check(lib().eoc_gate_batch_wait(ticket), "eoc_gate_batch_wait")


def gpu_shutdown():
    lib().eoc_gpu_shutdown()


def stats():
    """eoc_stats: counters of the global engine (batches, bootstraps, key switches)"""
    out = (C.c_uint64 * 3)()
    _check(lib().eoc_stats(C.byref(out)), "eoc_stats")
    return dict(batches=out[0], bootstraps=out[1], keyswitches=out[2])


def upload_cloud_key(sk):
    _check(lib().eoc_upload_cloud_key(sk.h), "eoc_upload_cloud_key")


def gate_batch(op, in0, in1=None, in2=None, ops=None, out=None, count=None, rowlen=None):
    """eoc_gate_batch on host arrays [count][n+1] int32.  Operand shapes are checked here (the C ABI takes bare
    pointers): every supplied operand must have exactly in0's shape, `ops` one opcode per row.  CONST0/CONST1 take
    no input: pass in0=None with `count` and `rowlen`."""
    if in0 is None:
        if ops is not None or int(op) not in (OPS["CONST0"], OPS["CONST1"]) or count is None or rowlen is None:
            raise EocError("gate_batch: in0 may be omitted only for CONST0/CONST1 with count and rowlen given")
        shape = (int(count), int(rowlen))
    else:
        in0 = np.ascontiguousarray(in0, np.int32)
        if in0.ndim != 2:
            raise EocError("gate_batch: operands are 2-d arrays [count][n+1]")
        shape = in0.shape
    in1c = None if in1 is None else np.ascontiguousarray(in1, np.int32)
    in2c = None if in2 is None else np.ascontiguousarray(in2, np.int32)
    opsc = None if ops is None else np.ascontiguousarray(ops, np.uint8)
    for name, a in (("in1", in1c), ("in2", in2c)):
        if a is not None and a.shape != shape:
            raise EocError(f"gate_batch: {name} has shape {a.shape}, expected {shape}")
    if opsc is not None and opsc.shape != (shape[0],):
        raise EocError(f"gate_batch: ops has shape {opsc.shape}, expected ({shape[0]},)")
    e0 = lib().eoc_global_engine()
    if e0 and shape[1] != lib().eoc_engine_params(e0).contents.n + 1:
        raise EocError(f"gate_batch: rows have {shape[1]} words, the engine's samples have n + 1 = "
                       f"{lib().eoc_engine_params(e0).contents.n + 1}")
    if out is None:
        out = np.empty(shape, np.int32)
    elif out.shape != shape or out.dtype != np.int32 or not out.flags.c_contiguous:
        raise EocError("gate_batch: out must be a C-contiguous int32 array of the operands' shape")
    _check(lib().eoc_gate_batch(int(op), None if opsc is None else opsc.ctypes.data,
                                None if in0 is None else in0.ctypes.data,
                                None if in1c is None else in1c.ctypes.data,
                                None if in2c is None else in2c.ctypes.data, out.ctypes.data, shape[0]),
           "eoc_gate_batch")
    return out


def lut_batch(p, tables, cts):
    """eoc_lut_batch on the global context (gpu_init + upload_cloud_key, or a cloud key alone): tables [n_luts][p] Torus32
    output values (lut_test_polynomial), cts [count][n+1] encrypted at message space p in {2, 4, 8}
    (SecretKey.encrypt_ints, where the encoding, the addition of ciphertexts and the failure rates are stated).
    Returns [n_luts][count][n+1]."""
    tables = np.ascontiguousarray(np.asarray(tables, np.int64).astype(np.int32))
    if tables.ndim != 2 or tables.shape[1] != int(p):
        raise EocError(f"lut_batch: tables must be [n_luts][p], got {tables.shape} for p = {p}")
    cts = np.ascontiguousarray(cts, np.int32)
    if cts.ndim != 2:
        raise EocError("lut_batch: cts is a 2-d array [count][n+1]")
    out = np.empty((tables.shape[0],) + cts.shape, np.int32)
    _check(lib().eoc_lut_batch(int(p), tables.ctypes.data, tables.shape[0], cts.ctypes.data, out.ctypes.data,
                               cts.shape[0]), "eoc_lut_batch")
    return out


def lut_many_batch(p, tables, cts):
    """eoc_lut_many_batch on the global context: tables [T][p] or [n_luts][T][p] Torus32 output values
    (lut_many_test_polynomial), cts [count][n+1] encrypted at message space p (SecretKey.encrypt_ints), p T <= 16.
    Returns [n_luts][T][count][n+1]."""
    tables = np.asarray(tables, np.int64).astype(np.int32)
    if tables.ndim == 2:
        tables = tables[None]
    tables = np.ascontiguousarray(tables)
    if tables.ndim != 3 or tables.shape[2] != int(p):
        raise EocError(f"lut_many_batch: tables must be [T][p] or [n_luts][T][p], got {tables.shape} for p = {p}")
    cts = np.ascontiguousarray(cts, np.int32)
    if cts.ndim != 2:
        raise EocError("lut_many_batch: cts is a 2-d array [count][n+1]")
    n_luts, T = tables.shape[:2]
    out = np.empty((n_luts, T) + cts.shape, np.int32)
    _check(lib().eoc_lut_many_batch(int(p), T, tables.ctypes.data, n_luts, cts.ctypes.data, out.ctypes.data, cts.shape[0]),
           "eoc_lut_many_batch")
    return out


def lut2_batch(p, tables, x, y, n_tables=1):
    """eoc_lut2_batch on the global context (cloud key + packing key: global_import_packing_key_blob): tables [p][p] or
    [n_funcs][p][p] Torus32 output values, tables[f][x][y]; x, y [count][n+1] at message space p.  Returns
    [n_funcs][count][n+1]."""
    tables = np.asarray(tables, np.int64).astype(np.int32)
    if tables.ndim == 2:
        tables = tables[None]
    tables = np.ascontiguousarray(tables)
    if tables.ndim != 3 or tables.shape[1:] != (int(p), int(p)):
        raise EocError(f"lut2_batch: tables must be [p][p] or [n_funcs][p][p], got {tables.shape} for p = {p}")
    x, y = np.ascontiguousarray(x, np.int32), np.ascontiguousarray(y, np.int32)
    if x.ndim != 2 or x.shape != y.shape:
        raise EocError("lut2_batch: x and y are 2-d arrays [count][n+1] of one shape")
    out = np.empty((tables.shape[0],) + x.shape, np.int32)
    _check(lib().eoc_lut2_batch(int(p), int(n_tables), tables.ctypes.data, tables.shape[0], x.ctypes.data, y.ctypes.data,
                                out.ctypes.data, x.shape[0]), "eoc_lut2_batch")
    return out


def lut_tree_batch(p, d, tables, digits, n_tables=1):
    """eoc_lut_tree_batch on the global context (cloud key + packing key): tables [n_funcs][p^d] (or one function's p^d values,
    any shape with p^d entries per function given as [n_funcs][...]) Torus32 output values, tables[f][x_1]..[x_d]; digits
    [d][count][n+1] at message space p, x_1 first.  Returns [n_funcs][count][n+1]."""
    p, d = int(p), int(d)
    tables = np.asarray(tables, np.int64).astype(np.int32)
    if not 2 <= d <= 4 or tables.size == 0 or tables.size % (p ** d):
        raise EocError(f"lut_tree_batch: tables must hold n_funcs x p^d values with 2 <= d <= 4, got {tables.shape} for p = {p}, d = {d}")
    tables = np.ascontiguousarray(tables.reshape(-1, p ** d))
    digits = np.ascontiguousarray(digits, np.int32)
    if digits.ndim != 3 or digits.shape[0] != d:
        raise EocError("lut_tree_batch: digits is a 3-d array [d][count][n+1]")
    out = np.empty((tables.shape[0],) + digits.shape[1:], np.int32)
    _check(lib().eoc_lut_tree_batch(p, d, int(n_tables), tables.ctypes.data, tables.shape[0], digits.ctypes.data, out.ctypes.data,
                                    digits.shape[1]), "eoc_lut_tree_batch")
    return out


def int_circuit_run(nodes, tables, wires, instances=None):
    """eoc_int_circuit_run on the global context: nodes = list of INode, tables = one entry per test polynomial, each
    [T][p] (or [p] for one table) of Torus32 output values, wires [n_wires][instances][n+1] with the input wires' rows filled
    in.  Returns the array with every written wire's rows filled in (a copy when `wires` is not contiguous int32)."""
    wires = np.ascontiguousarray(wires, np.int32)
    if wires.ndim != 3:
        raise EocError("int_circuit_run: wires is a 3-d array [n_wires][instances][n+1]")
    entries = [np.atleast_2d(np.asarray(t, np.int32)) for t in tables]
    flat = np.ascontiguousarray(np.concatenate([t.ravel() for t in entries]) if entries else np.zeros(1, np.int32), np.int32)
    ps = np.array([t.shape[1] for t in entries] or [0], np.int32)
    Ts = np.array([t.shape[0] for t in entries] or [0], np.int32)
    arr = _inode_array(nodes)
    _check(lib().eoc_int_circuit_run(C.addressof(arr), len(nodes), flat.ctypes.data, ps.ctypes.data, Ts.ctypes.data,
                                     len(entries), wires.ctypes.data, wires.shape[0],
                                     wires.shape[1] if instances is None else int(instances)), "eoc_int_circuit_run")
    return wires


def _global_n(who):
    """n of the global context: from its key, else from its first GPU engine (a cloud key alone suffices)"""
    if lib().eoc_global_key_mode():
        return global_params().n
    e0 = lib().eoc_global_engine()
    if not e0:
        raise EocError(f"{who}: no key and no GPU engine on the global context")
    return lib().eoc_engine_params(e0).contents.n


def _table_call_args(who, table, log2_lists, log2_width, selectors, values=None):
    """The checks table_read and table_update share, under the caller's name `who`: table (an int32 array already)
    [2^log2_lists][2][N], log2_width in [0, 10], selectors [queries][depth][2l][2][N] with depth = log2_lists + 10 - log2_width.
    An update passes its `values`: they must be [queries][2][N], their count is the selectors', and depth 0 takes no
    selectors.  Returns (log2_lists, log2_width, selectors or None, values) as ints and contiguous int32 arrays."""
    d, lw = int(log2_lists), int(log2_width)
    if table.ndim != 3 or table.shape[1:] != (2, N) or not 0 <= d <= 12 or table.shape[0] != 1 << d:
        raise EocError(f"{who}: table must be [2^log2_lists][2][{N}] with log2_lists in [0, 12], got {table.shape}")
    if not 0 <= lw <= 10:
        raise EocError(f"{who}: log2_width = {lw} outside [0, 10]")
    depth = d + 10 - lw
    queries = "queries"
    if values is not None:
        values = np.ascontiguousarray(values, np.int32)
        if values.ndim != 3 or values.shape[1:] != (2, N):
            raise EocError(f"{who}: values must be [queries][2][{N}], got {values.shape}")
        queries = values.shape[0]
        if not depth:
            return d, lw, None, values
    selectors = np.ascontiguousarray(selectors, np.int32)
    if (selectors.ndim != 5 or selectors.shape[1] != depth or selectors.shape[3:] != (2, N)
            or (values is not None and selectors.shape[0] != queries)):
        raise EocError(f"{who}: selectors must be [{queries}][{depth}][2l][2][{N}], got {selectors.shape}")
    return d, lw, selectors, values


def compact_expand(lists, count=None):
    """eoc_compact_expand on the global context (a cloud key alone suffices): lists [L][2][N] (PublicKey.encrypt_*) ->
    [count][n+1] LWE samples, count = L N unless given (the messages the lists were made for)"""
    lists = np.ascontiguousarray(lists, np.int32)
    if lists.ndim != 3 or lists.shape[1:] != (2, N):
        raise EocError(f"compact_expand: lists must be [L][2][{N}], got {lists.shape}")
    count = lists.shape[0] * N if count is None else int(count)
    if count > lists.shape[0] * N:
        raise EocError(f"compact_expand: {lists.shape[0]} lists hold at most {lists.shape[0] * N} samples, not {count}")
    out = np.empty((count, _global_n("compact_expand") + 1), np.int32)
    _check(lib().eoc_compact_expand(lists.ctypes.data, count, out.ctypes.data), "eoc_compact_expand")
    return out


def set_leveled_rounding(on):
    """eoc_global_set_leveled_rounding: the rounding mode of the leveled calls (Engine.leveled_rounding) on every engine of the
    global context and on those it creates later; table_read, table_update and automaton_run follow it"""
    _check(lib().eoc_global_set_leveled_rounding(1 if on else 0), "eoc_global_set_leveled_rounding")


def table_read(table, log2_lists, log2_width, selectors):
    """eoc_table_read on the global context (a cloud key alone suffices): table [2^log2_lists][2][N] (trivial_table or
    PublicKey.encrypt_*), selectors [queries][10 - log2_width + log2_lists][2l][2][N] in torus form
    (SecretKey.encrypt_index per query) -> [queries][2^log2_width][n+1] LWE samples"""
    table = np.ascontiguousarray(table, np.int32)
    d, lw, selectors, _ = _table_call_args("table_read", table, log2_lists, log2_width, selectors)
    out = np.empty((selectors.shape[0], 1 << lw, _global_n("table_read") + 1), np.int32)
    _check(lib().eoc_table_read(table.ctypes.data, d, lw, selectors.ctypes.data, selectors.shape[0], out.ctypes.data),
           "eoc_table_read")
    return out


def table_update(table, log2_lists, log2_width, selectors, values):
    """eoc_table_update on the global context (no key is used; a cloud key alone brings the engines up): returns the table
    [2^log2_lists][2][N] with table[idx_q] += values[q] for every query.  selectors as table_read's (None or empty at
    log2_lists = 0, log2_width = 10), values [queries][2][N] TLWE samples (pack of W samples, PublicKey.encrypt_*,
    trivial_table) with the entry in slots 0 .. W-1 and 0 elsewhere"""
    table = np.array(table, np.int32, order="C")                              # a copy: the C call updates in place
    d, lw, selectors, values = _table_call_args("table_update", table, log2_lists, log2_width, selectors, values)
    sel_ptr = None if selectors is None else selectors.ctypes.data
    _check(lib().eoc_table_update(table.ctypes.data, d, lw, sel_ptr, values.ctypes.data, values.shape[0]), "eoc_table_update")
    return table


def _automaton_records(trans):
    """host records [states][4] int32 = (next0, w0, next1, w1) of an Automaton or of an array-like"""
    t = np.ascontiguousarray(trans.trans if isinstance(trans, Automaton) else trans, np.int32)
    if t.ndim != 2 or t.shape[1] != 4:
        raise EocError(f"automaton: transitions must be [states][4] = (next0, w0, next1, w1), got {t.shape}")
    return t


class Automaton:
    """A public deterministic (weighted) finite automaton over bits, in plain Python: state q goes to next0
    with weight w0 under input bit 0 and to next1 with weight w1 under bit 1; weights live in [0, 2N) and add up modulo 2N
    along a run.  `trans` [states][4] int32 = (next0, w0, next1, w1), `start` the start state, `accepting` the accepting
    states of an acceptor (empty for a weighted automaton whose final vector is a table).  Bit 0 of an input is read first.
    Evaluated on encrypted bits by Engine.automaton_run_device / automaton_run: no bootstrap, so the error's mean and
    variance both grow linearly in the number of input bits (noise.automaton_budget)."""

    def __init__(self, trans, start=0, accepting=()):
        self.trans = np.ascontiguousarray(trans, np.int32).reshape(-1, 4)
        self.start = int(start)
        self.accepting = tuple(int(a) for a in accepting)
        Q = self.states
        t = self.trans
        if not (1 <= Q <= 4096 and ((t[:, [0, 2]] >= 0) & (t[:, [0, 2]] < Q)).all() and ((t[:, [1, 3]] >= 0) & (t[:, [1, 3]] < 2 * N)).all()
                and 0 <= self.start < Q and all(0 <= a < Q for a in self.accepting)):
            raise EocError("Automaton: states in [1, 4096], successors and start inside the states, weights in [0, 2N)")

    @property
    def states(self):
        return self.trans.shape[0]

    def run_plain(self, bits, start=None):
        """(end state, sum of the weights mod 2N) of the run over `bits`, bit 0 first"""
        q, w = self.start if start is None else int(start), 0
        for b in bits:
            nxt, wt = self.trans[q, 2:] if int(b) else self.trans[q, :2]
            q, w = int(nxt), (w + int(wt)) % (2 * N)
        return q, w

    def evaluate_plain(self, bits, final=None, start=None):
        """what slot 0 of the encrypted run decodes to.  final None: 1 if the run ends in an accepting state, else 0.  final
        given: a public table [states][<= N] of integers -- final[end state][sum of weights], negated past N (X^N = -1)."""
        q, w = self.run_plain(bits, start)
        if final is None:
            return int(q in self.accepting)
        v = int(np.asarray(final)[q][w % N])
        return -v if w >= N else v

    def final_bits(self):
        """the acceptor's final vector in the clear: [states] of 0 / 1 (slot 0 of every state)"""
        f = np.zeros(self.states, np.uint8)
        f[list(self.accepting)] = 1
        return f

    @classmethod
    def contains(cls, pattern_bits):
        """accepts the strings that contain `pattern_bits` as a substring: the Knuth-Morris-Pratt automaton, len + 1 states,
        the last one absorbing"""
        pat = [int(b) & 1 for b in pattern_bits]
        m = len(pat)
        if m < 1:
            raise EocError("Automaton.contains: empty pattern")
        trans = np.zeros((m + 1, 4), np.int32)
        for q in range(m):
            for b in (0, 1):
                s = pat[:q] + [b]
                k = min(m, q + 1)
                while k and s[len(s) - k:] != pat[:k]:
                    k -= 1
                trans[q, 2 * b] = k
        trans[m, 0] = trans[m, 2] = m
        return cls(trans, 0, (m,))

    @classmethod
    def divisible_by(cls, m):
        """accepts the binary numbers divisible by m, MOST significant bit first: state = value so far mod m"""
        m = int(m)
        if m < 1:
            raise EocError("Automaton.divisible_by: m >= 1")
        trans = np.zeros((m, 4), np.int32)
        for q in range(m):
            trans[q, 0], trans[q, 2] = (2 * q) % m, (2 * q + 1) % m
        return cls(trans, 0, (0,))

    @classmethod
    def popcount(cls):
        """one state, weight 0 under bit 0 and 1 under bit 1: the run's weight is the number of set bits, and a final vector
        holding a table f in its slots turns slot 0 into f(count) (evaluate_plain(bits, final=[f]))"""
        return cls([[0, 0, 0, 1]], 0, ())


def automaton_run(trans, final, selectors, starts, log2_width=0):
    """eoc_automaton_run on the global context (a cloud key alone suffices): trans an Automaton or records [states][4], final
    [states][2][N] TLWE samples (trivial_table or PublicKey.encrypt_*), selectors [queries][steps][2l][2][N] in torus form
    (SecretKey.encrypt_selector_bits per query; bit 0 is read first), starts: state ids -> [queries][len(starts)]
    [2^log2_width][n+1] LWE samples.  No bootstrap: the error's mean and variance grow linearly in the number of steps
    (noise.automaton_budget)."""
    t = _automaton_records(trans)
    final = np.ascontiguousarray(final, np.int32)
    lw = int(log2_width)
    if final.ndim != 3 or final.shape != (t.shape[0], 2, N):
        raise EocError(f"automaton_run: final must be [{t.shape[0]}][2][{N}], got {final.shape}")
    if not 0 <= lw <= 10:
        raise EocError(f"automaton_run: log2_width = {lw} outside [0, 10]")
    selectors = np.ascontiguousarray(selectors, np.int32)
    if selectors.ndim != 5 or selectors.shape[3:] != (2, N):
        raise EocError(f"automaton_run: selectors must be [queries][steps][2l][2][{N}], got {selectors.shape}")
    st = np.ascontiguousarray(np.atleast_1d(starts), np.int32)
    queries, steps = selectors.shape[:2]
    out = np.empty((queries, st.size, 1 << lw, _global_n("automaton_run") + 1), np.int32)
    _check(lib().eoc_automaton_run(t.ctypes.data, t.shape[0], final.ctypes.data, selectors.ctypes.data if steps else None, steps,
                                   st.ctypes.data, st.size, lw, out.ctypes.data, queries), "eoc_automaton_run")
    return out


def linear(weights, lists, bias=None):
    """eoc_linear on the global context (a cloud key alone suffices): public int8 weights [rows][cols] in [-127, 127], lists
    [batch][ceil(cols / N)][2][N] (PublicKey.encrypt_*, pack), bias [rows] Torus32 or None -> LWE samples [batch][rows][n+1]
    of phase bias[r] + sum_k w[r][k] phase(slot k of vector b)"""
    w = np.asarray(weights)
    if w.ndim != 2 or w.size == 0 or not np.issubdtype(w.dtype, np.integer) or np.abs(w.astype(np.int64)).max() > 127:
        raise EocError(f"linear: weights must be a non-empty integer matrix [rows][cols] in [-127, 127], got {w.dtype} {w.shape}")
    w = np.ascontiguousarray(w, np.int8)
    rows, cols = w.shape
    L = -(-cols // N)
    lists = np.ascontiguousarray(lists, np.int32)
    if lists.ndim != 4 or lists.shape[1:] != (L, 2, N):
        raise EocError(f"linear: lists must be [batch][{L}][2][{N}], got {lists.shape}")
    if bias is not None:
        bias = np.ascontiguousarray(bias, np.int32)
        if bias.shape != (rows,):
            raise EocError(f"linear: bias must be [{rows}], got {bias.shape}")
    out = np.empty((lists.shape[0], rows, _global_n("linear") + 1), np.int32)
    _check(lib().eoc_linear(w.ctypes.data, rows, cols, lists.ctypes.data, lists.shape[0],
                            None if bias is None else bias.ctypes.data, out.ctypes.data), "eoc_linear")
    return out


def lwe_matmul(weights, cts, bias=None):
    """eoc_lwe_matmul on the global context (no key needed): public int8 weights [rows][cols] in [-127, 127], LWE samples
    cts [batch][cols][width], bias [rows] Torus32 or None -> [batch][rows][width], out[b][r] = sum_k w[r][k] cts[b][k] word
    by word mod 2^32, the bias on the body (last) word"""
    w = np.asarray(weights)
    if w.ndim != 2 or w.size == 0 or not np.issubdtype(w.dtype, np.integer) or np.abs(w.astype(np.int64)).max() > 127:
        raise EocError(f"lwe_matmul: weights must be a non-empty integer matrix [rows][cols] in [-127, 127], got {w.dtype} {w.shape}")
    w = np.ascontiguousarray(w, np.int8)
    rows, cols = w.shape
    cts = np.ascontiguousarray(cts, np.int32)
    if cts.ndim != 3 or cts.shape[1] != cols or cts.shape[2] < 1:
        raise EocError(f"lwe_matmul: cts must be [batch][{cols}][width], got {cts.shape}")
    if bias is not None:
        bias = np.ascontiguousarray(bias, np.int32)
        if bias.shape != (rows,):
            raise EocError(f"lwe_matmul: bias must be [{rows}], got {bias.shape}")
    out = np.empty((cts.shape[0], rows, cts.shape[2]), np.int32)
    _check(lib().eoc_lwe_matmul(w.ctypes.data, rows, cols, cts.ctypes.data, cts.shape[2], cts.shape[0],
                                None if bias is None else bias.ctypes.data, out.ctypes.data), "eoc_lwe_matmul")
    return out


def conv_linear(weights, lists, slots, bias=None):
    """eoc_conv_linear on the global context (a cloud key alone suffices): public int8 kernels [rows][cols] in [-127, 127]
    (rows = output channels, w[r][l N + k] = tap k of filter (r, l)), lists [batch][ceil(cols / N)][2][N] (list l = input
    channel l), slots [n_slots] (entry s: slot s mod N of output channel s / N), bias [rows] Torus32 or None -> LWE samples
    [batch][n_slots][n+1] of phase bias[r] + sum_l sum_k w[r][l N + k] x_l[t + k]"""
    w = np.asarray(weights)
    if w.ndim != 2 or w.size == 0 or not np.issubdtype(w.dtype, np.integer) or np.abs(w.astype(np.int64)).max() > 127:
        raise EocError(f"conv_linear: weights must be a non-empty integer matrix [rows][cols] in [-127, 127], got {w.dtype} {w.shape}")
    w = np.ascontiguousarray(w, np.int8)
    rows, cols = w.shape
    L = -(-cols // N)
    lists = np.ascontiguousarray(lists, np.int32)
    if lists.ndim != 4 or lists.shape[1:] != (L, 2, N):
        raise EocError(f"conv_linear: lists must be [batch][{L}][2][{N}], got {lists.shape}")
    t = np.asarray(slots)
    if t.ndim != 1 or (t.size and (not np.issubdtype(t.dtype, np.integer) or t.min() < 0 or t.max() >= rows * N)):
        raise EocError(f"conv_linear: slots must be a vector of slot numbers in [0, {rows * N}), got {t.dtype} {t.shape}")
    t = np.ascontiguousarray(t, np.uint32)
    if bias is not None:
        bias = np.ascontiguousarray(bias, np.int32)
        if bias.shape != (rows,):
            raise EocError(f"conv_linear: bias must be [{rows}], got {bias.shape}")
    out = np.empty((lists.shape[0], t.size, _global_n("conv_linear") + 1), np.int32)
    _check(lib().eoc_conv_linear(w.ctypes.data, rows, cols, lists.ctypes.data, lists.shape[0],
                                 None if bias is None else bias.ctypes.data, t.ctypes.data, t.size, out.ctypes.data), "eoc_conv_linear")
    return out


def pack(cts):
    """eoc_pack on the global context (the packing key alone suffices: global_import_packing_key_blob): LWE samples
    [count][n+1] -> compact lists [ceil(count / N)][2][N], sample i in slot i mod N of list i / N"""
    cts = np.ascontiguousarray(cts, np.int32)
    if cts.ndim != 2:
        raise EocError(f"pack: samples must be [count][n+1], got {cts.shape}")
    out = np.empty((max(1, -(-cts.shape[0] // N)), 2, N), np.int32)
    _check(lib().eoc_pack(cts.ctypes.data, cts.shape[0], out.ctypes.data), "eoc_pack")
    return out[:-(-cts.shape[0] // N)]


def global_import_packing_key_blob(blob):
    """Give the global context's engines an EOCPKS1 packing key (works behind a cloud key alone, key mode 2)"""
    blob = np.ascontiguousarray(np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray)) else blob, np.uint8)
    _check(lib().eoc_global_import_packing_key_blob(blob.ctypes.data, blob.size), "eoc_global_import_packing_key_blob")


def global_public_key_export():
    """EOCPK1 blob of the global secret key (key mode 1)"""
    need = lib().eoc_global_public_key_export(None, 0)
    if not need:
        raise EocError("eoc_global_public_key_export: no secret key on the global context")
    buf = (C.c_ubyte * need)()
    if lib().eoc_global_public_key_export(buf, need) != need:
        raise EocError("eoc_global_public_key_export failed")
    return bytes(buf)


def circuit_run(gates, wires, instances):
    wires = np.ascontiguousarray(wires, np.int32)
    arr = (Gate * len(gates))(*gates)
    _check(lib().eoc_circuit_run(C.addressof(arr), len(gates), wires.ctypes.data, wires.shape[0], instances),
           "eoc_circuit_run")
    return wires


# ---- raw-buffer calls on the string API's global key (what the Node / Lua batch wrappers use) ------------------
def global_key_mode():
    return lib().eoc_global_key_mode()


def global_params():
    p = Params()
    _check(lib().eoc_global_params(C.byref(p)), "eoc_global_params")
    return p


def global_import_cloud_key_blob(blob):
    """Server side: install an EOCCK1 blob (numpy uint8 / bytes) as the cloud-key-only global context."""
    blob = np.ascontiguousarray(np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray)) else blob, np.uint8)
    _check(lib().eoc_global_import_cloud_key_blob(blob.ctypes.data, blob.size), "eoc_global_import_cloud_key_blob")


def global_import_seeded_cloud_key_blob(blob):
    """Server side: install an EOCCKS1 blob as the cloud-key-only global context (key mode 2); every engine expands its own
    copy of the key on its device"""
    blob = _blob_u8(blob)
    _check(lib().eoc_global_import_seeded_cloud_key_blob(blob.ctypes.data, blob.size), "eoc_global_import_seeded_cloud_key_blob")


def seeded_expand(seed, bodies, first_idx=0):
    """eoc_seeded_expand on the global context (no key is used): (seed, bodies [count]) -> [count][n+1] LWE samples, cut over
    the engines"""
    s = _key32(seed, "seed")
    bodies = np.ascontiguousarray(np.asarray(bodies).ravel(), np.int32)
    if lib().eoc_global_key_mode():
        n = global_params().n
    else:
        e0 = lib().eoc_global_engine()
        if not e0:
            raise EocError("seeded_expand: no key and no GPU engine on the global context")
        n = lib().eoc_engine_params(e0).contents.n
    out = np.empty((bodies.size, n + 1), np.int32)
    _check(lib().eoc_seeded_expand(s.ctypes.data, int(first_idx), bodies.ctypes.data, bodies.size, out.ctypes.data),
           "eoc_seeded_expand")
    return out


def global_cloud_key_export():
    need = lib().eoc_global_cloud_key_export(None, 0)
    if not need:
        raise EocError("eoc_global_cloud_key_export: no key on the global context")
    buf = np.empty(need, np.uint8)
    if lib().eoc_global_cloud_key_export(buf.ctypes.data, need) != need:
        raise EocError("eoc_global_cloud_key_export failed")
    return buf


def global_encrypt_bits(bits):
    bits = np.ascontiguousarray(np.asarray(bits).ravel(), np.uint8)
    out = np.empty((bits.size, global_params().n + 1), np.int32)
    _check(lib().eoc_global_encrypt_bits(bits.ctypes.data, bits.size, out.ctypes.data), "eoc_global_encrypt_bits")
    return out


def global_decrypt_bits(cts):
    cts = np.ascontiguousarray(cts, np.int32).reshape(-1, global_params().n + 1)
    out = np.empty(cts.shape[0], np.uint8)
    _check(lib().eoc_global_decrypt_bits(cts.ctypes.data, cts.shape[0], out.ctypes.data), "eoc_global_decrypt_bits")
    return out


def global_encrypt_ints(values, p):
    """SecretKey.encrypt_ints on the global key, with secure-mode randomness (eoc_global_encrypt_ints)"""
    values = np.ascontiguousarray(np.asarray(values).ravel(), np.uint8)
    out = np.empty((values.size, global_params().n + 1), np.int32)
    _check(lib().eoc_global_encrypt_ints(int(p), values.ctypes.data, values.size, out.ctypes.data), "eoc_global_encrypt_ints")
    return out


def global_decrypt_ints(cts, p):
    cts = np.ascontiguousarray(cts, np.int32).reshape(-1, global_params().n + 1)
    out = np.empty(cts.shape[0], np.uint8)
    _check(lib().eoc_global_decrypt_ints(int(p), cts.ctypes.data, cts.shape[0], out.ctypes.data), "eoc_global_decrypt_ints")
    return out


def global_gate_batch(op, in0, in1=None, in2=None, ops=None):
    """eoc_global_gate_batch: brings the GPU engine(s) up behind the global key on first use."""
    in0 = np.ascontiguousarray(in0, np.int32)
    in1c = None if in1 is None else np.ascontiguousarray(in1, np.int32)
    in2c = None if in2 is None else np.ascontiguousarray(in2, np.int32)
    opsc = None if ops is None else np.ascontiguousarray(ops, np.uint8)
    for a in (in1c, in2c):
        if a is not None and a.shape != in0.shape:
            raise EocError("global_gate_batch: operand shapes differ")
    out = np.empty_like(in0)
    _check(lib().eoc_global_gate_batch(int(op), None if opsc is None else opsc.ctypes.data, in0.ctypes.data,
                                       None if in1c is None else in1c.ctypes.data,
                                       None if in2c is None else in2c.ctypes.data, out.ctypes.data, in0.shape[0]),
           "eoc_global_gate_batch")
    return out


def global_circuit_run(gates, wires, instances):
    wires = np.ascontiguousarray(wires, np.int32)
    arr = (Gate * len(gates))(*gates)
    _check(lib().eoc_global_circuit_run(C.addressof(arr), len(gates), wires.ctypes.data, wires.shape[0], instances),
           "eoc_global_circuit_run")
    return wires


class Tfhe:
    """String façade in the shape of ao-tfhe/tfhe.lua (Tfhe.* -> backend.*), for the Boolean path."""

    # ---- the reference's 11 functions (ao-tfhe/tfhe.lua:4-53), same names and argument order ----
    @staticmethod
    def info():
        return lib().info()

    @staticmethod
    def testJWT():
        return lib().testJWT()

    @staticmethod
    def generateSecretKey(jwtToken, jwksBase64):
        return _take_str(lib().generateSecretKey(jwtToken.encode(), jwksBase64.encode()))

    @staticmethod
    def generatePublicKey():
        return _take_str(lib().generatePublicKey())

    @staticmethod
    def encryptInteger(value, key=""):
        return _take_str(lib().encryptInteger(int(value), key.encode()))

    @staticmethod
    def encryptInteger_dummy(value, key=""):
        return _take_str(lib().encryptInteger_dummy(int(value), key.encode()))

    @staticmethod
    def decryptInteger(value, key, jwtToken, jwksBase64):
        return lib().decryptInteger(value.encode(), key.encode(), jwtToken.encode(), jwksBase64.encode())

    @staticmethod
    def addCiphertexts(c1, c2, public_key=""):
        return _take_str(lib().addCiphertexts(c1.encode(), c2.encode(), public_key.encode()))

    @staticmethod
    def subtractCiphertexts(c1, c2, public_key=""):
        # ao-tfhe/tfhe.lua:41-43 forwards subtract to backend.addCiphertexts; tests/tfhe.test.js:185
        # pins the result (50 "-" 8 = 58).  Kept for drop-in behaviour; the real one is below.
        return _take_str(lib().addCiphertexts(c1.encode(), c2.encode(), public_key.encode()))

    @staticmethod
    def subtractCiphertexts_backend(c1, c2, public_key=""):
        return _take_str(lib().subtractCiphertexts(c1.encode(), c2.encode(), public_key.encode()))

    @staticmethod
    def encryptASCIIString(value, length, key=""):
        return _take_str(lib().encrypt8BitASCIIString(value.encode(), int(length), key.encode()))

    @staticmethod
    def decryptASCIIString(value, length, key, jwtToken, jwksBase64):
        return _take_str(lib().decrypt8BitASCIIString(value.encode(), int(length), key.encode(),
                                                      jwtToken.encode(), jwksBase64.encode()))

    @staticmethod
    def exportSecretKey():
        return _take_str(lib().exportSecretKey())

    @staticmethod
    def importSecretKey(b64):
        return lib().importSecretKey(b64.encode())

    # ---- the cloud ("public") key: exported by the client, imported by a server that never sees the secret key ----
    @staticmethod
    def exportCloudKey():
        return _take_str(lib().exportCloudKey())

    @staticmethod
    def importCloudKey(b64):
        return lib().importCloudKey(b64.encode())

    @staticmethod
    def exportCloudKeyToFile(path):
        return lib().exportCloudKeyToFile(os.fsencode(path))

    @staticmethod
    def importCloudKeyFromFile(path):
        return lib().importCloudKeyFromFile(os.fsencode(path))

    @staticmethod
    def keyMode():
        """0 no key, 1 secret + cloud key (client / single host), 2 cloud key only (server)"""
        return lib().eoc_global_key_mode()

    # ---- Boolean path -----------------------------------------------------------------------------
    @staticmethod
    def generateGateKey(minimum_lambda=80, seed=1):
        return _take_str(lib().generateGateKey(minimum_lambda, seed))

    @staticmethod
    def resetGateKey():
        lib().resetGateKey()

    @staticmethod
    def encryptBit(bit, key=""):
        return _take_str(lib().encryptBit(int(bit), key.encode()))

    @staticmethod
    def constantBit(bit):
        """bootsCONSTANT: the noiseless trivial sample of `bit` as a ciphertext string"""
        return _take_str(lib().constantBit(int(bit)))

    @staticmethod
    def decryptBit(ct, key=""):
        return lib().decryptBit(ct.encode(), key.encode())

    @staticmethod
    def _g2(name, a, b, pk=""):
        return _take_str(getattr(lib(), name)(a.encode(), b.encode(), pk.encode()))

    nand = staticmethod(lambda a, b, pk="": Tfhe._g2("gateNAND", a, b, pk))
    and_ = staticmethod(lambda a, b, pk="": Tfhe._g2("gateAND", a, b, pk))
    or_ = staticmethod(lambda a, b, pk="": Tfhe._g2("gateOR", a, b, pk))
    nor = staticmethod(lambda a, b, pk="": Tfhe._g2("gateNOR", a, b, pk))
    xor = staticmethod(lambda a, b, pk="": Tfhe._g2("gateXOR", a, b, pk))
    xnor = staticmethod(lambda a, b, pk="": Tfhe._g2("gateXNOR", a, b, pk))

    @staticmethod
    def not_(a, pk=""):
        return _take_str(lib().gateNOT(a.encode(), pk.encode()))

    @staticmethod
    def mux(a, b, c, pk=""):
        return _take_str(lib().gateMUX(a.encode(), b.encode(), c.encode(), pk.encode()))

    @staticmethod
    def maj(a, b, c, pk=""):
        """extension gate: the majority of three bits in ONE bootstrap (a full adder's carry)"""
        return _take_str(lib().gateMAJ(a.encode(), b.encode(), c.encode(), pk.encode()))

    @staticmethod
    def xor3(a, b, c, pk=""):
        """extension gate: the parity of three bits in ONE bootstrap (a full adder's sum)"""
        return _take_str(lib().gateXOR3(a.encode(), b.encode(), c.encode(), pk.encode()))

    # ---- word-level circuits, one backend call each; the FORM is picked by the instance count (circuits.pick_form: ----
    # ---- fewest levels for a handful of instances, fewest bootstraps for thousands), like Tfhe.addBits in tfhe.js / .lua ----
    @staticmethod
    def _samples(cts):
        import base64
        n1 = global_params().n + 1
        return np.stack([np.frombuffer(base64.b64decode(c), "<i4", count=n1) for c in cts])[:, None, :]

    @staticmethod
    def _strings(planes):
        import base64
        return [base64.b64encode(np.ascontiguousarray(p[0], "<i4").tobytes() + bytes(8)).decode() for p in planes]

    @staticmethod
    def _run(built, a_planes, b_planes, instances, outputs):
        gates, n_wires, a, b = built[0], built[1], built[2], built[3]
        wires = np.zeros((n_wires, instances, a_planes.shape[-1]), np.int32)
        wires[a[0]: a[0] + len(a)] = a_planes
        wires[b[0]: b[0] + len(b)] = b_planes
        return global_circuit_run(gates, wires, instances)[list(outputs)]

    @staticmethod
    def addBitsBatch(A, B):
        """A, B: samples [nbits][instances][n+1] (LSB first) -> [nbits + 1][instances][n+1]"""
        from . import circuits
        A, B = np.ascontiguousarray(A, np.int32), np.ascontiguousarray(B, np.int32)
        built = circuits.adder(A.shape[0], A.shape[1])
        return Tfhe._run(built, A, B, A.shape[1], built[4])

    @staticmethod
    def lessThanBitsBatch(A, B):
        """A, B: samples [nbits][instances][n+1] -> [instances][n+1]: 1 iff A < B (unsigned)"""
        from . import circuits
        A, B = np.ascontiguousarray(A, np.int32), np.ascontiguousarray(B, np.int32)
        built = circuits.less_than_for(A.shape[0], A.shape[1])
        return Tfhe._run(built, A, B, A.shape[1], [built[4]])[0]

    @staticmethod
    def subtractBitsBatch(A, B):
        """A, B: samples [nbits][instances][n+1] -> [nbits + 1][instances][n+1]: difference bits, then the borrow (= A < B)"""
        from . import circuits
        A, B = np.ascontiguousarray(A, np.int32), np.ascontiguousarray(B, np.int32)
        built = circuits.subtractor_for(A.shape[0], A.shape[1])
        return Tfhe._run(built, A, B, A.shape[1], list(built[4]) + [built[5]])

    @staticmethod
    def multiplyBitsBatch(A, B):
        """A, B: samples [nbits][instances][n+1] -> [2 nbits][instances][n+1]: column compression + one prefix addition for
        small batches, the row-by-row form for wide ones (both through the netlist optimizer)"""
        from . import circuits
        A, B = np.ascontiguousarray(A, np.int32), np.ascontiguousarray(B, np.int32)
        built = circuits.multiplier_for(A.shape[0], A.shape[1])
        return Tfhe._run(built, A, B, A.shape[1], built[4])

    @staticmethod
    def minMaxBitsBatch(A, B):
        """A, B: samples [nbits][instances][n+1] -> (min, max), each [nbits][instances][n+1]"""
        from . import circuits
        A, B = np.ascontiguousarray(A, np.int32), np.ascontiguousarray(B, np.int32)
        built = circuits.min_max_for(A.shape[0], A.shape[1])
        out = Tfhe._run(built, A, B, A.shape[1], list(built[4]) + list(built[5]))
        return out[: A.shape[0]], out[A.shape[0]:]

    @staticmethod
    def addBits(A, B):
        """arrays of base64 bit ciphertexts (LSB first) -> len(A) + 1 ciphertext strings (the log-depth adder)"""
        return Tfhe._strings(Tfhe.addBitsBatch(Tfhe._samples(A), Tfhe._samples(B)))

    @staticmethod
    def lessThanBits(A, B):
        return Tfhe._strings(Tfhe.lessThanBitsBatch(Tfhe._samples(A), Tfhe._samples(B))[None])[0]


class Circuit:
    """Deferred gates: the reference's call style (one ciphertext operation per call, ao-tfhe/tfhe.lua:4-53) evaluated by ONE
    backend call.  A gate call on the string API costs a whole blind rotation's n sequential steps (1.8 ms) however little
    it computes; a Circuit records the same calls on wire handles and run() sends the recorded netlist through
    eoc_netlist_optimize and one eoc_global_circuit_run, where every LEVEL costs those 1.8 ms.  The twin of Tfhe.newCircuit
    in tfhe_gates.lua / tfhe.js.

        c = Circuit(); x, y = c.input(ct_x), c.input(ct_y)
        s, k = c.run([c.xor(x, y), c.and_(x, y)])          # base64 ciphertext strings, one backend call
    """

    def __init__(self):
        self.gates, self.n_wires, self.inputs, self.instances = [], 0, {}, None

    def _wire(self):
        self.n_wires += 1
        return self.n_wires - 1

    def _gate(self, name, a=-1, b=-1, c=-1):
        out = self._wire()
        self.gates.append(Gate(OPS[name], a, b, c, out))
        return out

    def _add_input(self, planes):
        if self.instances not in (None, planes.shape[0]):
            raise EocError("every input of a Circuit has the same instance count")
        self.instances = planes.shape[0]
        w = self._wire()
        self.inputs[w] = planes
        return w

    def input(self, ct):
        """one base64 ciphertext string"""
        return self._add_input(Tfhe._samples([ct])[0])

    def input_samples(self, samples):
        """raw samples [instances][n+1]"""
        return self._add_input(np.ascontiguousarray(samples, np.int32))

    def constant(self, bit):
        return self._gate("CONST1" if bit else "CONST0")

    def nand(self, a, b): return self._gate("NAND", a, b)
    def and_(self, a, b): return self._gate("AND", a, b)
    def or_(self, a, b): return self._gate("OR", a, b)
    def nor(self, a, b): return self._gate("NOR", a, b)
    def xor(self, a, b): return self._gate("XOR", a, b)
    def xnor(self, a, b): return self._gate("XNOR", a, b)
    def not_(self, a): return self._gate("NOT", a)
    def mux(self, a, b, c): return self._gate("MUX", a, b, c)
    def maj(self, a, b, c): return self._gate("MAJ", a, b, c)
    def xor3(self, a, b, c): return self._gate("XOR3", a, b, c)

    def run(self, outs):
        """outs: handles -> list of base64 strings (one instance) or of sample arrays [instances][n+1]"""
        instances = self.instances or 1
        rowlen = next(iter(self.inputs.values())).shape[-1] if self.inputs else global_params().n + 1
        wires = np.zeros((self.n_wires, instances, rowlen), np.int32)
        for w, planes in self.inputs.items():
            wires[w] = planes
        gates = netlist_optimize(self.gates, list(outs)) if self.gates else []
        if gates:
            global_circuit_run(gates, wires, instances)
        return Tfhe._strings([wires[w] for w in outs]) if instances == 1 else [wires[w] for w in outs]



from .int_circuits import IntCircuit, bit_function2, radix_add, radix_less_than  # noqa: E402,F401
from . import dinn  # noqa: E402,F401
from .dinn import DenseLayer, Network  # noqa: E402,F401

"""The ledger of the library's third code object, eoc_tfhe_amd/csrc/lwe_matmul.hip, as tests/
test_kernel_ledger_cpu.py keeps it for engine.hip and multi.hip (no GPU): the kernels hipcc emits are exactly the names listed
here, each beside the GPU test function that launches it; none spills or uses scratch; k_lwe_matmul runs on the int8 matrix
instruction.  A kernel added to the file without an entry fails here: that is the purpose."""
import os
import re
import subprocess
import tempfile

import pytest

import kernel_ledger as kl
from isa_lib import HIPCC, ISA_FLAGS, ROOT, demangled, kernel_bodies, kernel_meta

# kernel -> (file, GPU test function that launches it, what the function covers)
ENTRIES = {
    "k_lwe_matmul": ("tests/test_gpu_lwe_matmul.py", "test_words_equal_the_reference",
                     "every tail: rows, cols and width below, at and above a tile, several workgroups, with and without a bias"),
}


@pytest.fixture(scope="module")
def isa():
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    with tempfile.TemporaryDirectory(prefix="eoc_isa_") as tmp:
        out = os.path.join(tmp, "lwe_matmul.s")
        subprocess.run([HIPCC, *ISA_FLAGS, "-o", out, os.path.join(ROOT, "eoc_tfhe_amd", "csrc", "lwe_matmul.hip")], check=True, cwd=tmp)
        with open(out) as f:
            return f.read()


def test_the_kernels_are_exactly_the_listed_ones(isa):
    mangled = list(kernel_meta(isa))
    names = [kl.short_name(n) for n in demangled(mangled)]
    assert sorted(names) == sorted(ENTRIES), names


def test_every_named_file_and_gpu_test_function_exists():
    for kernel, (path, func, why) in ENTRIES.items():
        full = os.path.join(ROOT, path)
        assert os.path.isfile(full), (kernel, path)
        with open(full) as f:
            text = f.read()
        assert re.search(rf"^def {re.escape(func)}\(", text, flags=re.M), (kernel, path, func)
        assert "pytest.mark.gpu" in text and why, (kernel, path)


def test_no_kernel_spills_or_uses_scratch(isa):
    for name, m in kernel_meta(isa).items():
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] <= 256, (name, m)                          # two waves per SIMD, as its launch bounds ask


def test_the_matrix_product_is_the_int8_mfma(isa):
    bodies = {kl.short_name(d): b for d, b in zip(demangled(list(kernel_bodies(isa))), kernel_bodies(isa).values())}
    body = bodies["k_lwe_matmul"]
    mfma = [ln for ln in body if ln.startswith("v_mfma")]
    assert mfma and all(ln.startswith("v_mfma_i32_32x32x32_i8") for ln in mfma), mfma[:3]
    assert len(mfma) == 8                                                 # 2 row tiles x 4 limbs, one K step per loop pass
    assert any(ln.startswith("v_perm_b32") for ln in body)                # the byte transposition of the ciphertext words

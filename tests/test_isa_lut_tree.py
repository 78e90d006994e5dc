"""ISA guards of the exact test-polynomial pack (hipcc cross-compiles gfx950 here, no GPU), from the code
object's metadata and the instruction text: k_pks_limbs, k_tvpack_mm and the three k_tv_spread instances exist, the product
runs on v_mfma_i32_32x32x32_i8 (eight per K step: two row tiles x four limbs), nothing spills or uses scratch, results leave
through plain vector dword stores (no atomics: every word of S and of a list is written once), and the registers are the
ones DESIGN.md 22 states (hipcc 7.2)."""
import pytest

from isa_lib import engine_isa, kernel_bodies, kernel_meta

# mangled-name fragment -> (VGPRs, LDS bytes) as measured
KERNELS = {
    "11k_pks_limbsE": (10, 0),
    "11k_tvpack_mmILi4EE": (178, 8192),
    "11k_tv_spreadILi2EE": (34, 4112),
    "11k_tv_spreadILi4EE": (34, 4112),
    "11k_tv_spreadILi8EE": (34, 4112),
}


@pytest.fixture(scope="module")
def isa():
    text = engine_isa()
    return kernel_meta(text), kernel_bodies(text)


def one(table, sub):
    hits = [k for k in table if sub in k]
    assert len(hits) == 1, (sub, hits)
    return hits[0]


@pytest.mark.parametrize("sub", list(KERNELS))
def test_kernels_exist_without_scratch_and_with_the_stated_registers(isa, sub):
    meta, _ = isa
    m = meta[one(meta, sub)]
    print(sub, m)
    assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
    assert (m["vgpr_count"], m["group_segment_fixed_size"]) == KERNELS[sub] and m["agpr_count"] == 0, m
    assert m["vgpr_count"] + m["agpr_count"] <= 256                       # k_tvpack_mm: two waves per SIMD


def test_the_product_runs_on_the_int8_matrix_instruction(isa):
    _, bodies = isa
    ops = [ln.split()[0] for ln in bodies[one(bodies, "11k_tvpack_mmILi4EE")]]
    assert ops.count("v_mfma_i32_32x32x32_i8") == 8, ops.count("v_mfma_i32_32x32x32_i8")
    assert not [o for o in ops if "mfma" in o and o != "v_mfma_i32_32x32x32_i8"]


@pytest.mark.parametrize("sub", list(KERNELS))
def test_results_leave_through_plain_vector_dword_stores(isa, sub):
    _, bodies = isa
    ops = [ln.split()[0] for ln in bodies[one(bodies, sub)]]
    assert not [o for o in ops if "atomic" in o or o.startswith(("scratch_", "buffer_"))], sub
    assert {o for o in ops if "store" in o} == {"global_store_dword"}, sub


def test_earlier_kernel_counts_are_unchanged(isa):
    meta, _ = isa
    assert len([k for k in meta if "k_tvpack_cols" in k]) == 3 and len([k for k in meta if "k_ksk_limbs" in k]) == 1
    # k_keyswitch_mfma: one since the <8> instance no launch could reach is no longer compiled
    assert len([k for k in meta if "k_keyswitch_mfma" in k]) == 1 and len([k for k in meta if "k_pack_rows" in k]) == 1

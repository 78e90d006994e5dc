"""ISA guards of the two-input lookup's kernels (hipcc cross-compiles gfx950 here, no GPU), from the code
object's metadata and symbol names alone: the encrypted-seed family k_br_enc / k_br_enc_wide exists exactly once per (shape,
read-back form) with the register budgets of its _tv twins, the gather kernel k_tvpack_cols is small, and the new names stay
out of the kernel counts the other ISA tests rely on."""
import pytest

from isa_lib import engine_isa, kernel_meta

PAIR = ["8k_br_encILi1ELi0E", "8k_br_encILi2ELi0E", "8k_br_encILi3ELi0E", "8k_br_encILi4ELi0E", "8k_br_encILi2ELi10E",
        "8k_br_encILi3ELi7E"]
WIDE = ["13k_br_enc_wideILi10E", "13k_br_enc_wideILi0E"]
DEFAULT_SETS = ("8k_br_encILi2ELi10E", "8k_br_encILi3ELi7E", "13k_br_enc_wideILi10E")
RESERVED = ("k_blind_rotate", "k_lut_many", "keyswitch_waves", "k_cmux", "k_tlwe_extract", "k_pack_rows", "k_pack_gather",
            "k_tv_gather", "modswitch")


@pytest.fixture(scope="module")
def meta():
    return kernel_meta(engine_isa())


def test_encrypted_seed_kernels_exist_once_per_shape_and_form_and_fit_the_register_file(meta):
    family = [k for k in meta if "k_br_enc" in k]
    assert len(family) == 16 and len([k for k in family if "k_br_enc_wide" in k]) == 4, family
    for form in ("Lb0EE", "Lb1EE"):
        for sub in PAIR + WIDE:
            hits = [k for k in meta if sub + form in k]
            assert len(hits) == 1, (sub, form, hits)
            name, m = hits[0], meta[hits[0]]
            print(name, m)
            assert name.endswith("PKij"), name                # the _tv kernels' five arguments
            assert m["sgpr_spill_count"] == 0, (name, m)
            if sub in DEFAULT_SETS:
                assert m["vgpr_count"] + m["agpr_count"] <= 256, (name, m)
                assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
            elif sub == "13k_br_enc_wideILi0E":                # run-time base, wide: a few registers, as its twins
                assert m["vgpr_count"] <= 256 and m["vgpr_spill_count"] <= 8, (name, m)
            elif sub == "8k_br_encILi4ELi0E":                  # gadget length 4: the slow correctness path spills, as its twins
                assert m["vgpr_spill_count"] > 0, (name, m)
            else:
                assert m["vgpr_count"] <= 256, (name, m)


def test_gather_kernel_is_small(meta):
    hits = [k for k in meta if "k_tvpack_cols" in k]
    assert len(hits) == 3, hits                               # p = 2, 4, 8
    for k in hits:
        m = meta[k]
        print(k, m)
        assert m["vgpr_count"] <= 32 and m["agpr_count"] == 0, (k, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (k, m)
        assert m["group_segment_fixed_size"] == 0, (k, m)    # no LDS: no transpose


def test_new_names_contain_no_reserved_substring(meta):
    new = [k for k in meta if "k_br_enc" in k or "k_tvpack_cols" in k]
    assert len(new) == 19
    for k in new:
        assert not any(r in k for r in RESERVED), k

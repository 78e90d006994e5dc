"""ISA guards of the packing kernels (hipcc cross-compiles gfx950 here; no GPU), from the code object's metadata alone:
k_pack_rows fits the 256 registers of a wave at two waves per SIMD with no spill and no scratch, k_pack_gather is small, and
the new names leave the kernel counts that tests/test_isa_lut.py and tests/test_isa_cmux.py rely on as they were."""
import re

import pytest

from isa_lib import engine_isa, kernel_meta


@pytest.fixture(scope="module")
def isa():
    return engine_isa()


def one(meta, name):
    hits = [k for k in meta if name in k]
    assert len(hits) == 1, hits
    assert not any("blind_rotate" in k or "keyswitch_waves" in k for k in hits)   # the new names stay out of those counts
    return meta[hits[0]]


def test_pack_rows_fits_a_wave_without_spill_or_scratch(isa):
    m = one(kernel_meta(isa), "k_pack_rows")
    print("k_pack_rows", m)
    assert m["vgpr_count"] + m["agpr_count"] <= 256, m          # two waves per SIMD
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m


def test_pack_gather_is_small(isa):
    m = one(kernel_meta(isa), "k_pack_gather")
    print("k_pack_gather", m)
    assert m["vgpr_count"] <= 32 and m["agpr_count"] == 0, m
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m


def test_kernel_name_counts_are_unchanged(isa):
    names = re.findall(r"^(_Z\S*k_blind_rotate\S*):", isa, flags=re.M)
    assert len([k for k in names if "_tv" in k]) == len([k for k in names if "_tv" not in k]) == 16
    assert len(re.findall(r"^(_Z\S*keyswitch_waves\S*):", isa, flags=re.M)) == 4
    assert len([k for k in kernel_meta(isa) if "k_cmux" in k or "k_tlwe_extract" in k]) == 7

"""ISA guards of the table-update kernels (hipcc cross-compiles gfx950 here; no GPU), from the code object's metadata alone:
the six instances of k_demux exist, the two default-set ones fit the 256 registers of a wave at two waves per SIMD without
scratch (the second output is formed at store time from a reload of x, not held across the product), the run-time-base
instances up to gadget length 3 do not spill, k_sample_add is small, and no new name contains a substring by which the
other ISA tests count kernels.  Instruction text is not searched."""
import re

import pytest

from isa_lib import engine_isa, kernel_meta

RESERVED = ("k_cmux", "k_tlwe_extract", "blind_rotate", "keyswitch_waves", "k_br_enc", "k_tvpack_cols", "k_pack",
            "k_lin_modswitch", "k_tv_gather", "lut_many", "modswitch")
SHAPES = [("2", "10"), ("3", "7"), ("1", "0"), ("2", "0"), ("3", "0"), ("4", "0")]


@pytest.fixture(scope="module")
def meta():
    return kernel_meta(engine_isa())


def test_demux_instances_and_their_registers(meta):
    demux = {re.search(r"k_demuxILi(\d)ELi(\d+)E", k).groups(): m for k, m in meta.items() if "k_demux" in k}
    assert sorted(demux) == sorted(SHAPES), sorted(demux)
    for inst in (("2", "10"), ("3", "7")):
        m = demux[inst]
        print(inst, m)
        assert m["vgpr_count"] <= 256, (inst, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (inst, m)
    for inst in (("1", "0"), ("2", "0"), ("3", "0")):           # the run-time-base instances: only gadget length 4 may spill
        assert demux[inst]["vgpr_spill_count"] == 0 and demux[inst]["private_segment_fixed_size"] == 0, (inst, demux[inst])


def test_sample_add_is_small(meta):
    add = {k: m for k, m in meta.items() if "k_sample_add" in k}
    assert len(add) == 2, sorted(add)                           # 16 bytes per lane, and the word form for unaligned callers
    for k, m in add.items():
        print(k, m)
        assert m["vgpr_count"] <= 32 and m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, (k, m)


def test_new_names_contain_no_reserved_substring(meta):
    new = [k for k in meta if "k_demux" in k or "k_sample_add" in k]
    assert len(new) == 8
    assert not [(k, s) for k in new for s in RESERVED if s in k]

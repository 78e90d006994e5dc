"""ISA guards of the leveled kernels (hipcc cross-compiles gfx950 here; no GPU), from the code object's metadata: the two
default-set instances of k_cmux fit the 256 registers of a wave at two waves per SIMD without scratch, k_tlwe_extract stays as
small as its sibling k_compact_expand, and the new names leave the kernel counts tests/test_isa_lut.py and
tests/test_isa_int_circuit.py rely on as they were."""
import re

import pytest

from isa_lib import engine_isa, kernel_meta


@pytest.fixture(scope="module")
def isa():
    return engine_isa()


def test_cmux_instances_and_their_registers(isa):
    meta = kernel_meta(isa)
    cmux = {re.search(r"k_cmuxILi(\d)ELi(\d+)E", k).groups(): m for k, m in meta.items() if "k_cmux" in k}
    assert sorted(cmux) == sorted([("2", "10"), ("3", "7"), ("1", "0"), ("2", "0"), ("3", "0"), ("4", "0")]), sorted(cmux)
    for inst in (("2", "10"), ("3", "7")):
        m = cmux[inst]
        print(inst, m)
        assert m["vgpr_count"] <= 256, (inst, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (inst, m)
    for inst in (("1", "0"), ("2", "0"), ("3", "0")):           # the run-time-base instances: only gadget length 4 may spill
        assert cmux[inst]["vgpr_spill_count"] == 0 and cmux[inst]["private_segment_fixed_size"] == 0, (inst, cmux[inst])


def test_tlwe_extract_is_small(isa):
    meta = kernel_meta(isa)
    ext = [k for k in meta if "k_tlwe_extract" in k]
    assert len(ext) == 1
    m = meta[ext[0]]
    print(ext[0], m)
    assert m["vgpr_count"] <= 32 and m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0, m


def test_kernel_name_counts_are_unchanged(isa):
    """tests/test_isa_lut.py counts kernels by name: 16 gate and 16 _tv blind rotations, and the key switch's four shapes"""
    names = re.findall(r"^(_Z\S*k_blind_rotate\S*):", isa, flags=re.M)
    tv = [k for k in names if "_tv" in k]
    gate = [k for k in names if "_tv" not in k]
    assert len(tv) == len(gate) == 16
    assert len(re.findall(r"^(_Z\S*keyswitch_waves\S*):", isa, flags=re.M)) == 4
    new = [k for k in kernel_meta(isa) if "k_cmux" in k or "k_tlwe_extract" in k]
    assert len(new) == 7 and not any("k_blind_rotate" in k or "keyswitch_waves" in k for k in new)

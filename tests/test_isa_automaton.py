"""ISA guards of the automaton step kernel (hipcc cross-compiles gfx950 here; no GPU), from the code object's metadata alone:
the six instances of k_automaton_step exist, the two default-set ones fit the 256 registers of a wave at two waves per SIMD
without scratch (the first operand is gathered again at store time, not held across the product), the run-time-base instances
up to gadget length 3 do not spill, and the new name leaves the kernel counts of tests/test_isa_cmux.py,
tests/test_isa_demux.py and tests/test_isa_lut.py as they were.  Instruction text is not searched."""
import re

import pytest

from isa_lib import engine_isa, kernel_meta

RESERVED = ("k_cmux", "k_demux", "k_sample_add", "k_tlwe_extract", "k_blind_rotate", "keyswitch_waves", "_tv", "k_pack",
            "k_br_enc", "k_lut_many", "k_seed")
SHAPES = [("2", "10"), ("3", "7"), ("1", "0"), ("2", "0"), ("3", "0"), ("4", "0")]


@pytest.fixture(scope="module")
def isa():
    return engine_isa()


def test_automaton_instances_and_their_registers(isa):
    meta = kernel_meta(isa)
    step = {re.search(r"k_automaton_stepILi(\d)ELi(\d+)E", k).groups(): m for k, m in meta.items() if "k_automaton_step" in k}
    assert sorted(step) == sorted(SHAPES), sorted(step)
    for inst in (("2", "10"), ("3", "7")):
        m = step[inst]
        print(inst, m)
        assert m["vgpr_count"] <= 256, (inst, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (inst, m)
    for inst in (("1", "0"), ("2", "0"), ("3", "0")):           # the run-time-base instances: only gadget length 4 may spill
        assert step[inst]["vgpr_spill_count"] == 0 and step[inst]["private_segment_fixed_size"] == 0, (inst, step[inst])


def test_the_new_name_contains_no_reserved_substring(isa):
    new = [k for k in kernel_meta(isa) if "k_automaton" in k]
    assert len(new) == 6
    assert not [(k, s) for k in new for s in RESERVED if s in k]


def test_kernel_name_counts_are_unchanged(isa):
    """what tests/test_isa_cmux.py, tests/test_isa_demux.py and tests/test_isa_lut.py count by name"""
    meta = kernel_meta(isa)
    names = re.findall(r"^(_Z\S*k_blind_rotate\S*):", isa, flags=re.M)
    tv = [k for k in names if "_tv" in k]
    assert len(tv) == len(names) - len(tv) == 16
    assert len(re.findall(r"^(_Z\S*keyswitch_waves\S*):", isa, flags=re.M)) == 4
    assert len([k for k in meta if "k_cmux" in k or "k_tlwe_extract" in k]) == 7
    assert len([k for k in meta if "k_demux" in k or "k_sample_add" in k]) == 8

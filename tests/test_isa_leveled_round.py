"""ISA guards of the rounding twins of the leveled kernels (hipcc cross-compiles gfx950 here, no GPU), from the
code object's metadata: each of k_rcmux, k_rdemux and k_rstep has the six pair shapes, fits the registers its truncating twin
fits -- and takes no more of them --, and the new names stay out of every count the other guards make by name."""
import re

import pytest

from isa_lib import engine_isa, kernel_meta

SHAPES = sorted([("2", "10"), ("3", "7"), ("1", "0"), ("2", "0"), ("3", "0"), ("4", "0")])
TWINS = {"k_rcmux": "k_cmux", "k_rdemux": "k_demux", "k_rstep": "k_automaton_step"}
# substrings the existing guards count kernels by (tests/test_isa_*.py)
COUNTED = ("k_cmux", "k_demux", "k_automaton", "k_blind_rotate", "blind_rotate", "keyswitch_waves", "k_tlwe_extract", "k_sample_add",
           "k_br_enc", "br_lds", "lut_many", "modswitch", "k_pack_", "k_dot_", "k_conv_", "k_seed_masks", "k_tv_gather")


@pytest.fixture(scope="module")
def meta():
    return kernel_meta(engine_isa())


def family(meta, name):
    """(l, Bgbit) -> metadata of the instances of the kernel template `name` (the mangled name carries its length in front)"""
    pat = re.compile(rf"{len(name)}{name}ILi(\d)ELi(\d+)EEE")
    return {m.groups(): v for k, v in meta.items() for m in [pat.search(k)] if m}


@pytest.mark.parametrize("twin", sorted(TWINS))
def test_twin_instances_and_their_registers(meta, twin):
    new, old = family(meta, twin), family(meta, TWINS[twin])
    assert sorted(new) == SHAPES == sorted(old), (sorted(new), sorted(old))
    assert len([k for k in meta if twin in k]) == 6
    for inst in (("2", "10"), ("3", "7")):
        m = new[inst]
        print(twin, inst, m)
        assert m["vgpr_count"] <= 256, (inst, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (inst, m)
    for inst in (("1", "0"), ("2", "0"), ("3", "0")):           # the run-time-base instances: only gadget length 4 may spill
        assert new[inst]["vgpr_spill_count"] == 0 and new[inst]["sgpr_spill_count"] == 0, (inst, new[inst])
    for inst in SHAPES:
        print(twin, inst, "vgprs", new[inst]["vgpr_count"], "twin's", old[inst]["vgpr_count"])
        assert new[inst]["vgpr_count"] <= old[inst]["vgpr_count"], (inst, new[inst], old[inst])
        assert new[inst]["group_segment_fixed_size"] == old[inst]["group_segment_fixed_size"]


def test_new_names_stay_out_of_the_existing_counts(meta):
    new = [k for k in meta if any(t in k for t in TWINS)]
    assert len(new) == 18
    assert not [k for k in new if any(s in k for s in COUNTED)]
    # the counts themselves, as the other guards state them
    assert len([k for k in meta if "k_cmux" in k or "k_tlwe_extract" in k]) == 7
    assert len([k for k in meta if "k_demux" in k or "k_sample_add" in k]) == 8
    assert len([k for k in meta if "k_automaton_step" in k]) == 6

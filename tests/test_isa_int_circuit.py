"""ISA guards of the integer-circuit kernels (hipcc cross-compiles gfx950 here; no GPU), from the code object's metadata:
every instance of k_lin_modswitch (term counts 1..4, free and bootstrapped form) and k_tv_gather exists, uses no scratch, spills
nothing and stays small; their names leave the kernel counts tests/test_isa_lut.py relies on as they were."""
import re

import pytest

from isa_lib import engine_isa, kernel_meta


@pytest.fixture(scope="module")
def isa():
    return engine_isa()


def test_linear_stage_and_gather_kernels_are_small_and_spill_nothing(isa):
    meta = kernel_meta(isa)
    lin = [k for k in meta if "k_lin_modswitch" in k]
    assert sorted(re.search(r"ILi(\d)ELb(\d)E", k).groups() for k in lin) == \
        sorted((str(t), str(b)) for t in (1, 2, 3, 4) for b in (0, 1)), lin
    gather = [k for k in meta if "k_tv_gather" in k]
    assert len(gather) == 1
    for k in lin + gather:
        m = meta[k]
        print(k, m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (k, m)
        assert m["vgpr_count"] <= 32, (k, m)               # k_compact_expand, a kernel of the same kind, uses 22


def test_kernel_name_counts_are_unchanged(isa):
    """tests/test_isa_lut.py counts kernels by name: 16 gate and 16 _tv blind rotations, none of them new"""
    names = re.findall(r"^(_Z\S*k_blind_rotate\S*):", isa, flags=re.M)
    tv = [k for k in names if "_tv" in k]
    gate = [k for k in names if "_tv" not in k]
    assert len(tv) == len(gate) == 16
    new = [k for k in kernel_meta(isa) if "k_lin_modswitch" in k or "k_tv_gather" in k]
    assert new and not any("k_blind_rotate" in k or "keyswitch_waves" in k for k in new)

"""ISA guards of the programmable-bootstrapping kernels (hipcc cross-compiles gfx950 here; no GPU): the *_tv twins of the
shipped blind-rotation kernels exist for Set A (pair and wide kernel) and Set B, in both forms of the rotation-amount
read-back, and fit 256 VGPRs without scratch, like the kernels they share their body with (tests/test_isa_guard.py)."""
import re

import pytest

from isa_lib import engine_isa, kernel_meta


@pytest.fixture(scope="module")
def isa():
    return engine_isa()


def test_tv_kernels_fit_the_register_file_without_scratch(isa):
    meta = kernel_meta(isa)
    for form in ("Lb0EE", "Lb1EE"):
        for sub in ("17k_blind_rotate_tvILi2ELi10E", "17k_blind_rotate_tvILi3ELi7E", "22k_blind_rotate_wide_tvILi10E"):
            hits = [k for k in meta if sub + form in k]
            assert len(hits) == 1, (sub, form, hits)
            m = meta[hits[0]]
            assert m["vgpr_count"] <= 256 and m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (sub, m)
            assert m["sgpr_spill_count"] == 0, (sub, m)
    # every shape the launch policy can pick has its twin: pair kernel L = 1..4 (run-time base), wide kernel run-time base
    for sub in ("17k_blind_rotate_tvILi1ELi0E", "17k_blind_rotate_tvILi2ELi0E", "17k_blind_rotate_tvILi3ELi0E",
                "17k_blind_rotate_tvILi4ELi0E", "22k_blind_rotate_wide_tvILi0E"):
        assert any(sub in k for k in meta), sub


def test_tv_kernels_take_the_test_polynomial_and_the_gate_kernels_do_not(isa):
    """the twins' extra arguments come after the gate kernels' (BRArgs, twiddles, twist factors), so a gate kernel's
    argument block -- and the code that reads it -- is what it was"""
    names = re.findall(r"^(_Z\S*k_blind_rotate\S*):", isa, flags=re.M)
    tv = [k for k in names if "_tv" in k]
    gate = [k for k in names if "_tv" not in k]
    assert len(tv) == len(gate) == 16
    assert all(k.endswith("PKij") for k in tv) and not any(k.endswith("PKij") for k in gate)

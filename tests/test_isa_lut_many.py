"""ISA guards of the many-LUT kernels (hipcc cross-compiles gfx950 here; no GPU): k_lut_many / k_lut_many_wide exist for every
shape the launch policy picks, in both forms of the rotation-amount read-back, with the register budgets of the _tv twins
they share their body with, and their scalar read-back keeps the wait behind the scalar-cache invalidate
(tests/test_isa_guard.py's memory-model check only looks at kernels named *blind_rotate*).  k_modswitch_coarse exists."""
import re

import pytest

from isa_lib import engine_isa, kernel_meta


@pytest.fixture(scope="module")
def isa():
    return engine_isa()


PAIR = ["10k_lut_manyILi1ELi0E", "10k_lut_manyILi2ELi0E", "10k_lut_manyILi3ELi0E", "10k_lut_manyILi4ELi0E",
        "10k_lut_manyILi2ELi10E", "10k_lut_manyILi3ELi7E"]
WIDE = ["15k_lut_many_wideILi10E", "15k_lut_many_wideILi0E"]


def test_many_lut_kernels_exist_for_every_shape_and_fit_the_register_file(isa):
    meta = kernel_meta(isa)
    for form in ("Lb0EE", "Lb1EE"):
        for sub in PAIR + WIDE:
            hits = [k for k in meta if sub + form in k]
            assert len(hits) == 1, (sub, form, hits)
            name, m = hits[0], meta[hits[0]]
            assert name.endswith("PKijj"), name               # the _tv twin's arguments, then T
            assert m["sgpr_spill_count"] == 0, (name, m)
            if sub == "10k_lut_manyILi4ELi0E":                 # gadget length 4: the slow correctness path spills, as its twin
                assert m["vgpr_spill_count"] > 0
            elif sub == "15k_lut_many_wideILi0E":              # run-time base, wide: a few registers, as its twin
                assert m["vgpr_count"] <= 256 and m["vgpr_spill_count"] <= 8, (name, m)
            else:
                assert m["vgpr_count"] <= 256 and m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
            # the Set A / Set B instances use no more registers than their _tv twins
            twin = [k for k in meta if sub.replace("10k_lut_many", "17k_blind_rotate_tv")
                    .replace("15k_lut_many_wide", "22k_blind_rotate_wide_tv") + form in k]
            assert len(twin) == 1, (sub, twin)
            if sub in ("10k_lut_manyILi2ELi10E", "10k_lut_manyILi3ELi7E", "15k_lut_many_wideILi10E"):
                assert m["vgpr_count"] <= meta[twin[0]]["vgpr_count"], (name, m, meta[twin[0]])
    assert any("18k_modswitch_coarse" in k for k in meta)
    assert not any("blind_rotate" in k for k in meta if "lut_many" in k or "modswitch" in k)


def test_many_lut_rotation_amounts_stay_inside_the_memory_model_by_default(isa):
    """test_isa_guard.py's read-back check on the k_lut_many* kernels: no s_dcache_inv in the shipped (Lb0) form; the scalar
    form (Lb1) waits on lgkmcnt(0) directly behind every invalidate"""
    parts = re.split(r"^(_ZN3eoc\w+):[^\n]*$", isa, flags=re.M)
    seen = {"Lb0": 0, "Lb1": 0}
    for i in range(1, len(parts), 2):
        name = parts[i]
        if "k_lut_many" not in name:
            continue
        body = parts[i + 1][: parts[i + 1].rfind("s_endpgm")] if "s_endpgm" in parts[i + 1] else parts[i + 1]
        code = [ln.strip() for ln in body.splitlines() if ln.strip() and not ln.strip().startswith((";", "."))]
        form = "Lb1" if re.search(r"Lb1EE", name) else "Lb0"
        seen[form] += 1
        inv = [k for k, ln in enumerate(code) if ln.startswith("s_dcache_inv")]
        if form == "Lb0":
            assert not inv, name
        else:
            assert inv, name
            for k in inv:
                assert re.match(r"s_waitcnt .*lgkmcnt\(0\)", code[k + 1]), (name, code[k:k + 3])
    assert seen == {"Lb0": 8, "Lb1": 8}, seen

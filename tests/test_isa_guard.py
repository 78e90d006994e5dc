"""Guards on the SHIPPED kernels' ISA (hipcc cross-compiles gfx950 here; no GPU):

  * the register budgets DESIGN.md 5.1 states -- the hot kernels of both default parameter sets fit 256 VGPRs without
    scratch (a spill inside the step loop costs more than most optimisations gain);
  * no buffer store anywhere: hipcc 7.2 puts no wait state between `buffer_store_dwordx4 ..., sN offen` and a VALU write
    of the stored registers, and gfx950 then stores corrupted data now and then (found while bisecting the gadget-length-3
    prototype, DESIGN.md 5.1 / profiles/r05_wide_gadget3_attempt.txt).  The library's stores are global_store_*, which get
    their wait states; a change that introduces raw buffer stores has to bring its own (s_nop + sched_barrier) and this test.
"""
import re

import pytest

from isa_lib import engine_isa, kernel_meta


@pytest.fixture(scope="module")
def isa():
    return engine_isa()


def test_hot_kernels_fit_the_register_file_without_scratch(isa):
    meta = kernel_meta(isa)
    def find(sub):
        hits = [k for k in meta if sub in k]
        assert len(hits) == 1, (sub, hits)
        return meta[hits[0]]
    # both forms of the rotation-amount read-back (Lb0 = shipped: LDS copy; Lb1 = scalar loads, EOC_TFHE_SCALAR_ABAR=1)
    for form in ("Lb0EE", "Lb1EE"):
        for sub in ("14k_blind_rotateILi2ELi10E", "14k_blind_rotateILi3ELi7E", "19k_blind_rotate_wideILi10E",
                    "14k_blind_rotateILi1ELi0E", "14k_blind_rotateILi2ELi0E", "14k_blind_rotateILi3ELi0E"):
            m = find(sub + form)
            assert m["vgpr_count"] <= 256 and m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (sub, m)
            assert m["sgpr_spill_count"] == 0, (sub, m)
        # the documented exceptions: the run-time-base instance of the wide kernel spills a few registers, gadget length 4
        # is the slow correctness path (kernels.hip.h)
        assert find("19k_blind_rotate_wideILi0E" + form)["vgpr_spill_count"] <= 8
        assert find("14k_blind_rotateILi4ELi0E" + form)["vgpr_spill_count"] > 0
    for k, m in meta.items():
        if "k_keyswitch_waves" in k:
            assert m["vgpr_spill_count"] == 0 and m["vgpr_count"] <= 128, (k, m)   # four waves per SIMD


def test_no_buffer_stores_in_the_shipped_isa(isa):
    assert not re.search(r"^\s*buffer_store_", isa, flags=re.M)
    # and the wide global stores carry their wait states: no VALU write of the data registers in the next two instructions
    lines = [ln.strip() for ln in isa.splitlines()]
    bad = []
    for i, ln in enumerate(lines):
        m = re.match(r"global_store_dwordx[34] \S+ v\[(\d+):(\d+)\]", ln)
        if not m:
            continue
        data = set(range(int(m.group(1)), int(m.group(2)) + 1))
        seen = 0
        for nxt in lines[i + 1:i + 8]:
            if not nxt or nxt[0] in ";." or nxt.endswith(":"):
                continue
            if nxt.startswith("s_nop"):
                seen += 1 + int(nxt.split()[1])
                continue
            if seen >= 2:
                break
            if nxt.startswith("v_"):
                d = re.match(r"v_\S+ v\[(\d+):(\d+)\]|v_\S+ v(\d+)", nxt)
                if d:
                    regs = set(range(int(d.group(1)), int(d.group(2)) + 1)) if d.group(1) else {int(d.group(3))}
                    if regs & data:
                        bad.append((i, ln, nxt))
            seen += 1
    assert not bad, bad[:3]


def test_rotation_amounts_stay_inside_the_memory_model_by_default(isa):
    """VERDICT r5 task 4 / ADVICE r5: the shipped blind-rotation kernels (SABAR = false) read the folded prologue's row
    back through vector loads + LDS -- no s_dcache_inv anywhere in them; the scalar form keeps the invalidate and now waits
    on it (s_waitcnt lgkmcnt(0) directly behind s_dcache_inv) before any later scalar load can issue"""
    parts = re.split(r"^(_ZN3eoc\w+):[^\n]*$", isa, flags=re.M)
    seen = {"Lb0": 0, "Lb1": 0}
    for i in range(1, len(parts), 2):
        name = parts[i]
        if "blind_rotate" not in name:
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
    assert seen["Lb0"] >= 8 and seen["Lb1"] >= 8, seen

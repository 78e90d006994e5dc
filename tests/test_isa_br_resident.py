"""ISA guard of the gadget-length-2 pair kernels' step loop (hipcc cross-compiles gfx950 here; no GPU): the loop reads no
table.  Per wave-step it issues exactly 56 ds_read_b128 -- the 48 reads of the six transposes and the 8 of the chain
exchange; every loop-invariant table value (forward passes 1 and 2, inverse passes 1 and 0, the eight un-twist factors) is
held in registers -- 56 ds_write_b128, the 16 ds_bpermute_b32 of the rotation and the 32 key-row loads, and the tables are
not even copied into LDS: the kernel stores nothing 16 bytes wide to LDS ahead of the loop, so no read inside it can hit the
table regions.  Nothing is spilled to make room for that.  The earlier form (k_br_lds*, EOC_TFHE_BR_TABLES_LDS=1) is
compiled next to it and keeps its 72 reads: the difference, 16, is what SQ_INSTS_LDS per wave-step falls by.
"""
import re

import pytest

from isa_lib import engine_isa, kernel_meta


READS_RESIDENT = 56     # 6 transposes x 8 + the exchange's 8: all three remaining table sets are resident
READS_TABLES_LDS = 72   # + forward pass 1 (4), inverse pass 0 (4), un-twist factors (8)


@pytest.fixture(scope="module")
def isa():
    return engine_isa()


def kernel_text(text):
    """raw text per kernel, labels and indentation kept (step_loop finds the loop by its labels), up to the last s_endpgm"""
    parts = re.split(r"^(_ZN3eoc\w+):[^\n]*$", text, flags=re.M)
    return {parts[i]: parts[i + 1][: parts[i + 1].rfind("s_endpgm")] for i in range(1, len(parts), 2)
            if "s_endpgm" in parts[i + 1]}


def step_loop(body):
    """(lines ahead of the loop, lines of the loop): the loop is the longest span closed by a backward branch"""
    lines = body.splitlines()
    label = {m.group(1): i for i, ln in enumerate(lines) for m in [re.match(r"(\.LBB\d+_\d+):", ln)] if m}
    best = None
    for i, ln in enumerate(lines):
        m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", ln)
        if m and label.get(m.group(1), i) < i and (best is None or i - label[m.group(1)] > best[1] - best[0]):
            best = (label[m.group(1)], i)
    assert best, "no loop"
    return lines[:best[0]], lines[best[0]:best[1] + 1]


def count(lines, mnemonic):
    return sum(1 for ln in lines if re.match(r"\s+" + mnemonic + r"\b", ln))


FAMILIES = ("14k_blind_rotateILi2E", "17k_blind_rotate_tvILi2E", "10k_lut_manyILi2E")
OLD = ("8k_br_ldsILi2E", "11k_br_lds_tvILi2E", "13k_br_lds_manyILi2E")


def test_step_loop_of_gadget_length_2_reads_no_table(isa):
    meta, bodies = kernel_meta(isa), kernel_text(isa)
    seen = 0
    for fam in FAMILIES:
        for base in ("Li10E", "Li0E"):
            for form in ("Lb0EE", "Lb1EE"):
                hits = [k for k in bodies if fam + base + form in k]
                assert len(hits) == 1, (fam, base, form, hits)
                name = hits[0]
                head, loop = step_loop(bodies[name])
                assert len(loop) > 2000, (name, len(loop))                      # the step loop, not an epilogue loop
                assert count(loop, "ds_read_b128") == READS_RESIDENT, (name, count(loop, "ds_read_b128"))
                assert count(loop, "ds_write_b128") == 56, name
                assert count(loop, "ds_bpermute_b32") == 16, name
                assert count(loop, "buffer_load_dwordx4") == 32, name
                assert count(loop, "s_barrier") == 2, name
                # the rotation amount (LDS form only) is the one other LDS read; no table value is re-fetched from memory
                other = [ln.strip() for ln in loop if re.match(r"\s+ds_read", ln) and not re.match(r"\s+ds_read_b128\b", ln)]
                assert len(other) == (1 if form == "Lb0EE" else 0) and all(o.startswith("ds_read_u16") for o in other), (name, other)
                assert not [ln for ln in loop if re.match(r"\s+(global_load|scratch_|flat_load)", ln)], name
                # the tables never reach LDS: no 16-byte LDS store ahead of the loop (the earlier form has them, below)
                assert count(head, "ds_write_b128") == 0 and count(head, "ds_write2_b64") == 0, name
                m = meta[name]
                assert m["vgpr_count"] <= 256 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, (name, m)
                assert m["private_segment_fixed_size"] == 0, (name, m)
                seen += 1
    assert seen == 12


def test_earlier_form_is_compiled_next_to_it(isa):
    meta, bodies = kernel_meta(isa), kernel_text(isa)
    for fam in OLD:
        for base in ("Li10E", "Li0E"):
            for form in ("Lb0EE", "Lb1EE"):
                hits = [k for k in bodies if fam + base + form in k]
                assert len(hits) == 1, (fam, base, form, hits)
                head, loop = step_loop(bodies[hits[0]])
                assert count(loop, "ds_read_b128") == READS_TABLES_LDS, (hits[0], count(loop, "ds_read_b128"))
                assert count(head, "ds_write_b128") + count(head, "ds_write2_b64") > 0, hits[0]
                m = meta[hits[0]]
                assert m["vgpr_count"] <= 256 and m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (hits[0], m)
    # gadget lengths 1, 3, 4 have no second form
    assert not [k for k in bodies if "br_lds" in k and "ILi2E" not in k]

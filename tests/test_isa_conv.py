"""Guards on the ISA of the convolution kernels (hipcc cross-compiles gfx950 here; no GPU): both k_conv_lists
instances keep k_dot_mask's frame -- one spectral accumulator in registers, no spill or scratch, two workgroups per CU, one
barrier --, the storing instance has no atomics and the adding instance no plain stores, the helpers k_conv_init and
k_conv_extract are small, and the kernel families other guards count are unchanged."""
import re

import pytest

from isa_lib import engine_isa, kernel_bodies, kernel_meta


@pytest.fixture(scope="module")
def isa():
    return engine_isa()


def test_both_instances_fit_the_register_file_without_scratch(isa):
    hits = {k: m for k, m in kernel_meta(isa).items() if "k_conv_lists" in k}
    assert len(hits) == 2, list(hits)
    single = [k for k in hits if "ILi8ELb1E" in k]                       # <the format's chunk, SINGLE>
    adding = [k for k in hits if "ILi8ELb0E" in k]
    assert len(single) == len(adding) == 1, list(hits)
    bodies = kernel_bodies(isa)
    for k, m in hits.items():
        print(k, m, len(bodies[k]), "instructions")
        assert m["vgpr_count"] + m["agpr_count"] <= 256 and m["vgpr_count"] <= 128, m  # 128: two waves per SIMD, as launched
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m
        assert m["group_segment_fixed_size"] == 0                        # dynamic LDS only: tables + four transpose scratches
        assert sum(ln.startswith("s_barrier") for ln in bodies[k]) == 1  # the tables; none behind it
    s, a = bodies[single[0]], bodies[adding[0]]
    assert not any("atomic" in ln for ln in s) and sum(ln.startswith("global_store_dword") for ln in s) == 16
    assert not any(ln.startswith("global_store") for ln in a) and sum(ln.startswith("global_atomic_add") for ln in a) == 16


def test_helper_kernels_are_small(isa):
    meta, bodies = kernel_meta(isa), kernel_bodies(isa)
    hits = {k: m for k, m in meta.items() if "k_conv_init" in k or "k_conv_extract" in k}
    assert len(hits) == 2, list(hits)
    for k, m in hits.items():
        print(k, m, len(bodies[k]), "instructions")
        assert m["vgpr_count"] <= 32 and m["agpr_count"] == 0, (k, m)
        assert m["group_segment_fixed_size"] == (4096 if "k_conv_extract" in k else 0), (k, m)   # c0 of the list at hand
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (k, m)
        assert len(bodies[k]) < 400, k
        assert not any("atomic" in ln for ln in bodies[k]), k


def test_kernel_name_counts_are_unchanged(isa):
    meta = kernel_meta(isa)
    names = re.findall(r"^(_Z\S*k_blind_rotate\S*):", isa, flags=re.M)
    assert len([k for k in names if "_tv" in k]) == len([k for k in names if "_tv" not in k]) == 16
    assert len(re.findall(r"^(_Z\S*keyswitch_waves\S*):", isa, flags=re.M)) == 4
    assert len([k for k in meta if "k_cmux" in k or "k_tlwe_extract" in k]) == 7
    assert len([k for k in meta if "k_demux" in k or "k_sample_add" in k]) == 8
    assert len([k for k in meta if "k_pack_rows" in k]) == 1 and len([k for k in meta if "k_pack_gather" in k]) == 1
    assert len([k for k in meta if "k_dot_" in k]) == 3
    assert len([k for k in meta if "k_compact_expand" in k]) == 1 and len([k for k in meta if "k_tv_gather" in k]) == 1
    new = [k for k in meta if "k_conv_" in k]
    assert len(new) == 4 and not any(s in k for k in new for s in ("k_dot_", "k_pack", "k_compact_expand", "k_cmux", "k_tv_gather",
                                                                   "k_blind_rotate", "keyswitch_waves", "k_lin_modswitch"))

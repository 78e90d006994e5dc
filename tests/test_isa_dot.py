"""Guards on the ISA of the inner-product kernels (hipcc cross-compiles gfx950 here; no GPU): k_dot_mask keeps
its one spectral accumulator and a row pair of both spectra in registers without spill or scratch, two workgroups per CU; the
helper k_dot_init is small; and the kernel families other guards count are unchanged."""
import re

import pytest

from isa_lib import engine_isa, kernel_bodies, kernel_meta


@pytest.fixture(scope="module")
def isa():
    return engine_isa()


def test_mask_kernel_fits_the_register_file_without_scratch(isa):
    hits = {k: m for k, m in kernel_meta(isa).items() if "k_dot_mask" in k}
    assert len(hits) == 1, list(hits)
    (name, m), = hits.items()
    print("k_dot_mask", m)
    assert "ILi8E" in name                                               # the format's chunk: 8 lists per inverse transform
    assert m["vgpr_count"] + m["agpr_count"] <= 256 and m["vgpr_count"] <= 128, m      # 128: two waves per SIMD, as launched
    assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m
    assert m["group_segment_fixed_size"] == 0                            # dynamic LDS only: tables + four transpose scratches
    body = kernel_bodies(isa)[name]
    assert sum(ln.startswith("s_barrier") for ln in body) == 1          # the tables; none behind it
    assert sum(ln.startswith("global_atomic_add") for ln in body) == 16 and not any(ln.startswith("global_store") for ln in body)


def test_helper_kernel_is_small(isa):
    hits = {k: m for k, m in kernel_meta(isa).items() if "k_dot_init" in k}
    assert len(hits) == 2, list(hits)                                    # the sample form and the key-switch operand form
    for k, m in hits.items():
        print(k, m)
        assert m["vgpr_count"] <= 32 and m["agpr_count"] == 0 and m["group_segment_fixed_size"] <= 64, (k, m)
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (k, m)
        assert len(kernel_bodies(isa)[k]) < 400, k


def test_kernel_name_counts_are_unchanged(isa):
    meta = kernel_meta(isa)
    names = re.findall(r"^(_Z\S*k_blind_rotate\S*):", isa, flags=re.M)
    assert len([k for k in names if "_tv" in k]) == len([k for k in names if "_tv" not in k]) == 16
    assert len(re.findall(r"^(_Z\S*keyswitch_waves\S*):", isa, flags=re.M)) == 4
    assert len([k for k in meta if "k_cmux" in k or "k_tlwe_extract" in k]) == 7
    assert len([k for k in meta if "k_demux" in k or "k_sample_add" in k]) == 8
    assert len([k for k in meta if "k_pack_rows" in k]) == 1 and len([k for k in meta if "k_pack_gather" in k]) == 1
    new = [k for k in meta if "k_dot_" in k]
    assert len(new) == 3 and not any(s in k for k in new for s in ("k_blind_rotate", "keyswitch_waves", "k_cmux", "k_pack", "k_lin_modswitch"))
    assert not re.search(r"^\s*buffer_store_", isa, flags=re.M)

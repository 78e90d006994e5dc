"""ISA guards of the matrix-core key switch (hipcc cross-compiles gfx950 here; no GPU): k_keyswitch_mfma exists in the one
instance ks_mfma_launch dispatches (4 waves per workgroup: the shipped plan; the alternative of 8 is instantiated by tools/ubench_ks_mfma.hip alone), runs on v_mfma_i32_32x32x32_i8, keeps its 128 accumulator registers and everything else
in the register file (no spill, no scratch) at two waves per SIMD, and the limb-image builder k_ksk_limbs exists.
tests/test_isa_guard.py (unchanged) checks the whole library for the stores that must not be there."""
import re

import pytest

from isa_lib import engine_isa, kernel_bodies, kernel_meta


@pytest.fixture(scope="module")
def isa():
    return engine_isa()


def test_mfma_key_switch_exists_without_spill_or_scratch(isa):
    meta, bodies = kernel_meta(isa), kernel_bodies(isa)
    names = sorted(k for k in meta if "16k_keyswitch_mfma" in k)
    assert len(names) == 1 and "ILi4E" in names[0], names              # <8>: never dispatched, no longer compiled
    for name in names:
        m = meta[name]
        assert m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, (name, m)
        assert m["vgpr_count"] + m["agpr_count"] <= 256, (name, m)       # two waves per SIMD
        code = bodies[name]
        mf = [ln for ln in code if ln.startswith("v_mfma_i32_")]
        assert mf and all(ln.startswith("v_mfma_i32_32x32x32_i8") for ln in mf), (name, mf[:2])
        assert len(mf) >= 32, (name, len(mf))                           # 4 indices x (2 row tiles x 4 limbs) per staged step
        assert not any(ln.startswith(("scratch_", "buffer_store", "buffer_load")) for ln in code), name
        at = [ln for ln in code if "_atomic_" in ln]                     # integer adds into the output row, nothing returned
        assert at and all(re.match(r"(flat|global)_atomic_add \S+ \S+( off)?$", ln) for ln in at), (name, at[:3])
        assert any(ln.startswith("ds_read_b128") for ln in code) and any(ln.startswith("ds_write_b128") for ln in code), name


def test_limb_image_builder_exists(isa):
    meta = kernel_meta(isa)
    hits = [k for k in meta if "11k_ksk_limbs" in k]
    assert len(hits) == 1, hits
    m = meta[hits[0]]
    assert m["vgpr_spill_count"] == 0 and m["private_segment_fixed_size"] == 0, m


def test_shipped_key_switch_kernels_are_still_there(isa):
    meta = kernel_meta(isa)
    for sub in ("17k_keyswitch_wavesILi8ELi8ELi16E", "17k_keyswitch_wavesILi8ELi8ELi32E", "17k_keyswitch_wavesILi8ELi4ELi64E",
                "17k_keyswitch_wavesILi8ELi8ELi64E", "19k_keyswitch_generic", "9k_ks_init"):
        assert any(sub in k for k in meta), sub

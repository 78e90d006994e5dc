"""ISA guards of the mask-expansion kernels (hipcc cross-compiles gfx950 here, no GPU), from the code object's
metadata and the instruction text: k_seed_masks exists once per output shape with the registers DESIGN.md 16 states, keeps
everything in registers (no scratch, no spill), stores with plain vector global stores only -- dword stores for the LWE rows,
dwordx4 stores for the key image and the ring rows --, uses no atomics, and its names stay out of the kernel counts the other
ISA tests rely on."""
import pytest

from isa_lib import engine_isa, kernel_bodies, kernel_meta

# (mangled-name fragment, VGPRs as stated in DESIGN.md 16)
KERNELS = {"12k_seed_masksILi0E": 50, "12k_seed_masksILi1E": 45, "12k_seed_masksILi2E": 25}
RESERVED = ("k_blind_rotate", "k_lut_many", "keyswitch_waves", "k_cmux", "k_tlwe_extract", "k_pack_rows", "k_pack_gather",
            "k_tv_gather", "modswitch", "k_br_enc", "k_tvpack_cols", "k_demux", "k_sample_add", "_tv", "br_lds", "k_ksk_limbs",
            "k_keyswitch_mfma", "k_lin_modswitch")


@pytest.fixture(scope="module")
def isa():
    text = engine_isa()
    return kernel_meta(text), kernel_bodies(text)


def test_seed_kernels_exist_once_per_shape_without_scratch_and_with_the_stated_registers(isa):
    meta, _ = isa
    assert len([k for k in meta if "k_seed_masks" in k]) == 3 and len([k for k in meta if "k_chacha20_blocks" in k]) == 1
    for sub, vgprs in KERNELS.items():
        hits = [k for k in meta if sub in k]
        assert len(hits) == 1, (sub, hits)
        m = meta[hits[0]]
        print(hits[0], m)
        assert m["private_segment_fixed_size"] == 0 and m["vgpr_spill_count"] == 0 and m["sgpr_spill_count"] == 0, m
        assert m["agpr_count"] == 0 and m["vgpr_count"] == vgprs, (sub, m)
        assert m["group_segment_fixed_size"] == (8192 + 32 * 8) * 4, m       # the rows' image and their sub-keys
    dbg = meta[[k for k in meta if "k_chacha20_blocks" in k][0]]
    assert dbg["private_segment_fixed_size"] == 0 and dbg["vgpr_spill_count"] == 0 and dbg["group_segment_fixed_size"] == 0


def test_seed_kernels_store_with_plain_vector_global_stores_and_no_atomics(isa):
    _, bodies = isa
    for sub in list(KERNELS) + ["k_chacha20_blocks"]:
        name = [k for k in bodies if sub in k][0]
        ops = [ln.split()[0] for ln in bodies[name]]
        assert not [o for o in ops if "atomic" in o], name
        assert not [o for o in ops if o.startswith("scratch_")], name
        stores = {o for o in ops if "store" in o}
        print(name, sorted(stores), len(ops), "instructions")
        assert stores and all(o.startswith("global_store_dword") for o in stores), (name, stores)
        if sub == "12k_seed_masksILi0E":
            assert stores == {"global_store_dword"}, stores              # rows are 4-byte aligned only
        elif sub in KERNELS:
            assert stores == {"global_store_dwordx4"}, stores            # 16-byte aligned rows: 1 KiB per wave and instruction
        assert any(o == "v_alignbit_b32" for o in ops), name             # the rotates


def test_new_names_contain_no_reserved_substring(isa):
    meta, _ = isa
    new = [k for k in meta if "k_seed_masks" in k or "k_chacha20_blocks" in k]
    assert len(new) == 4
    for k in new:
        assert not any(r in k for r in RESERVED), k

"""kernel_bodies (tests/isa_lib.py) compares kernels modulo the function's number in the code object: synthetic assembly,
no compiler."""
from isa_lib import kernel_bodies


def _function(name, number, block=2, reg="v3", imm="0x80"):
    return (f"{name}:                                   ; @{name}\n"
            f"; %bb.0:\n"
            f"\ts_load_dwordx2 s[0:1], s[4:5], 0x0\n"
            f"\ts_cbranch_execz .LBB{number}_{block}\n"
            f"; %bb.1:\n"
            f"\tv_add_u32_e32 {reg}, {imm}, v0\n"
            f"\ts_getpc_b64 s[2:3]\n"
            f"\ts_add_u32 s2, s2, .LJTI{number}_0@rel32@lo+4\n"
            f"\tv_mov_b32_e32 v1, my.LBB{number}_7\n"
            f"\ts_branch .LBB{number}_{block}\n"
            f".LBB{number}_{block}:\n"
            f"\ts_endpgm\n"
            f".Lfunc_end{number}:\n")


def _body(**kw):
    return kernel_bodies(_function("_Z1kv", **kw))["_Z1kv"]


def test_function_number_is_dropped_and_nothing_else():
    a, b = _body(number=3), _body(number=41)
    # the jump-table label and the symbol that merely contains ".LBB" are no block labels: they keep their number
    assert a[1] == "s_cbranch_execz .LBB_2" and a[-2] == "s_branch .LBB_2"
    assert a[4] == "s_add_u32 s2, s2, .LJTI3_0@rel32@lo+4" and b[4] == "s_add_u32 s2, s2, .LJTI41_0@rel32@lo+4"
    assert a[5] == "v_mov_b32_e32 v1, my.LBB3_7" and b[5] == "v_mov_b32_e32 v1, my.LBB41_7"
    # apart from those two lines, two functions that differ only in their number compare equal
    assert a[:4] + a[6:] == b[:4] + b[6:]
    assert len(a) == 8


def test_two_functions_of_one_file_compare_equal():
    text = _function("_Z1av", 0) + _function("_Z1bv", 12)
    bodies = kernel_bodies(text)
    strip = lambda body: [ln for ln in body if ".LJTI" not in ln and "my.LBB" not in ln]
    assert set(bodies) == {"_Z1av", "_Z1bv"}
    assert strip(bodies["_Z1av"]) == strip(bodies["_Z1bv"])


def test_real_changes_still_differ():
    base = _body(number=5)
    assert _body(number=5, block=3) != base  # another block index
    assert _body(number=6, block=3) != _body(number=6)
    assert _body(number=5, reg="v4") != base  # another register
    assert _body(number=5, imm="0x81") != base  # another immediate

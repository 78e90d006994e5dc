"""The kernel ledger (tests/kernel_ledger.py) against the kernels hipcc emits for the library's two code objects
(engine.hip and multi.hip; no GPU): every kernel matches exactly one entry or is in UNLAUNCHED, every entry matches a kernel,
every named file and test function exists.  A kernel added without an entry fails here: that is the purpose."""
import os
import re

import pytest

import kernel_ledger as kl
from isa_lib import ROOT, demangled, engine_isa, kernel_meta, multi_isa


@pytest.fixture(scope="module")
def kernels():
    mangled = list(kernel_meta(engine_isa())) + list(kernel_meta(multi_isa()))
    names = [kl.short_name(n) for n in demangled(mangled)]
    assert len(set(names)) == len(names) == len(mangled) > 100, len(names)
    return names


def test_short_names():
    assert kl.short_name("void eoc::k_cmux<2, 10>(eoc::CmuxArgs, HIP_vector_type<double, 2u> const*)") == "k_cmux<2,10>"
    assert kl.short_name("void eoc::k_blind_rotate<2, 10, false>(eoc::BRArgs, double2 const*) [clone .kd]") == "k_blind_rotate<2,10,false>"
    assert kl.short_name("k_copy_words(int const*, int*, unsigned long)") == "k_copy_words"
    assert kl.short_name("eoc::k_prepare(eoc::GateDesc const*, int).kd") == "k_prepare"


def test_every_kernel_has_exactly_one_entry_or_is_listed_unlaunched(kernels):
    bad = {k: [e[0] for e in kl.entries_of(k)] for k in kernels
           if len(kl.entries_of(k)) != (0 if k in kl.UNLAUNCHED else 1)}
    assert not bad, bad


def test_every_entry_and_every_unlaunched_name_matches_a_kernel(kernels):
    assert not [e[0] for e in kl.ENTRIES if not any(re.fullmatch(e[0], k) for k in kernels)]
    assert not [k for k in kl.UNLAUNCHED if k not in kernels]
    assert all(isinstance(why, str) and why for why in kl.UNLAUNCHED.values())


def test_rounding_twins_and_their_siblings_are_all_there(kernels):
    for stem in ("k_cmux", "k_demux", "k_automaton_step", "k_rcmux", "k_rdemux", "k_rstep"):
        assert sorted(k for k in kernels if k.startswith(stem + "<")) == sorted(
            f"{stem}<{s}>" for s in ("2,10", "3,7", "1,0", "2,0", "3,0", "4,0")), stem


def test_every_named_file_and_test_function_exists():
    for pattern, path, func, _ in kl.ENTRIES:
        full = os.path.join(ROOT, path)
        assert os.path.isfile(full), (pattern, path)
        with open(full) as f:
            text = f.read()
        assert re.search(rf"^def {re.escape(func)}\(", text, flags=re.M), (pattern, path, func)
        assert "pytest.mark.gpu" in text, (pattern, path)

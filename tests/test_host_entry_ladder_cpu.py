"""The ladder of checks of every host-buffer entry of the global context, in a process with no key and no
engine: which code a null argument, an empty batch and a smallest well-formed call get, in that order, and which text
eoc_last_error holds behind a failure.  Entries differ on purpose (eoc_pack asks for engines before it looks at count,
eoc_table_read answers EOC_OK for zero queries before it looks for anything); the expected values are what the entries
returned before they moved into one file under one rule, so a change here is a change of the C ABI's behaviour.

The process-global state is the subject, so the thirty-nine calls run in ONE fresh child process (no test that ran earlier
in this one can have left a key or an engine behind); none reaches a HIP call, since no engine exists."""
import json
import os
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CHILD = textwrap.dedent("""
    import ctypes as C, json, sys
    sys.path.insert(0, %r)
    import numpy as np
    import eoc_tfhe_amd as eoc
    L = eoc.lib()
    buf = [np.zeros(1 << 16, np.int32) for _ in range(5)]
    a, b, c, d, e = (x.ctypes.data for x in buf)
    seed = np.arange(32, dtype=np.uint8)
    w8 = np.ones(1, np.int8)
    trans = np.zeros((1, 4), np.int32)              # one state, both successors itself, weights 0
    starts = np.zeros(1, np.int32)
    tab2 = np.zeros(16, np.int32)                   # a table of any of the shapes below, all zero
    two = np.array([2], np.int32)
    gate = eoc.Gate(eoc.OPS["NAND"], 0, 1, -1, 2)
    node = eoc.INode()                              # wire 1 = 1 * wire 0: a linear node, no table
    node.n_tables, node.out, node.tv, node.n_terms, node.cst = 0, 1, -1, 1, 0
    node.in_[0], node.w[0] = 0, 1
    g, nd = C.addressof(gate), C.addressof(node)
    t, tr, st, sd, w = tab2.ctypes.data, trans.ctypes.data, starts.ctypes.data, seed.ctypes.data, w8.ctypes.data
    NAND = eoc.OPS["NAND"]
    # entry -> (null argument, empty batch, smallest non-empty call)
    calls = {
        "eoc_compact_expand": [(None, 1, b), (a, 0, b), (a, 1, b)],
        "eoc_seeded_expand": [(None, 0, a, 1, b), (sd, 0, a, 0, b), (sd, 0, a, 1, b)],
        "eoc_linear": [(None, 1, 1, a, 1, None, b), (w, 1, 1, a, 0, None, b), (w, 1, 1, a, 1, None, b)],
        "eoc_pack": [(None, 1, b), (a, 0, b), (a, 1, b)],
        "eoc_lut2_batch": [(2, 2, None, 1, a, b, c, 1), (2, 2, t, 1, a, b, c, 0), (2, 2, t, 1, a, b, c, 1)],
        "eoc_table_read": [(None, 0, 10, b, 1, c), (a, 0, 10, b, 0, c), (a, 0, 10, b, 1, c)],
        "eoc_table_update": [(None, 0, 10, b, c, 1), (a, 0, 10, b, c, 0), (a, 0, 10, b, c, 1)],
        "eoc_automaton_run": [(tr, 1, None, b, 1, st, 1, 10, c, 1), (tr, 1, a, b, 1, st, 1, 10, c, 0),
                              (tr, 1, a, b, 1, st, 1, 10, c, 1)],
        "eoc_lut_batch": [(2, None, 1, a, b, 1), (2, t, 1, a, b, 0), (2, t, 1, a, b, 1)],
        "eoc_lut_many_batch": [(2, 2, None, 1, a, b, 1), (2, 2, t, 1, a, b, 0), (2, 2, t, 1, a, b, 1)],
        "eoc_int_circuit_run": [(nd, 1, None, None, None, 0, None, 2, 1), (nd, 1, None, None, None, 0, a, 2, 0),
                                (nd, 1, None, None, None, 0, a, 2, 1)],
        "eoc_circuit_run": [(g, 1, None, 3, 1), (g, 1, a, 3, 0), (g, 1, a, 3, 1)],
        "eoc_gate_batch": [(NAND, None, a, b, None, None, 1), (NAND, None, a, b, None, c, 0), (NAND, None, a, b, None, c, 1)],
    }
    out = {}
    for name, three in calls.items():
        out[name] = []
        for args in three:
            rc = getattr(L, name)(*args)
            out[name].append([rc, L.eoc_last_error().decode() if rc else None])
    print("RESULT" + json.dumps(out))
""") % ROOT

OK, ERR_ARG, ERR_NO_DEVICE, ERR_STATE = 0, -1, -2, -6


def no_engine(who):
    return ERR_NO_DEVICE, who + ": no GPU engine (eoc_gpu_init not called or failed); there is no CPU fallback"


def null_arg(who, rest=""):
    return ERR_ARG, who + ": null argument" + rest


def engines_first(who):
    """the entries that ask for engines before they look at anything else"""
    return [no_engine(who)] * 3


LEVELED = ", log2_lists = 0 outside [0, 12] or log2_width = 10 outside [0, 10]"
# entry -> (code, eoc_last_error text behind a failure) of the three calls, as returned before the entries moved
EXPECTED = {
    "eoc_compact_expand": [null_arg("eoc_compact_expand"), (OK, None), no_engine("eoc_compact_expand")],
    "eoc_seeded_expand": [null_arg("eoc_seeded_expand"), (OK, None),
                          (ERR_STATE, "eoc_seeded_expand: no engine (install a key or call eoc_gpu_init first)")],
    "eoc_linear": [null_arg("eoc_linear"), no_engine("eoc_linear"), no_engine("eoc_linear")],
    "eoc_pack": [null_arg("eoc_pack"), no_engine("eoc_pack"), no_engine("eoc_pack")],
    "eoc_lut2_batch": engines_first("eoc_lut2_batch"),
    "eoc_table_read": [null_arg("eoc_table_read", LEVELED), (OK, None), no_engine("eoc_table_read")],
    "eoc_table_update": [null_arg("eoc_table_update", LEVELED), (OK, None), no_engine("eoc_table_update")],
    "eoc_automaton_run": [null_arg("eoc_automaton_run", ", log2_width = 10 outside [0, 10] or 1 start states outside [1, 4096]"),
                          (OK, None), no_engine("eoc_automaton_run")],
    "eoc_lut_batch": engines_first("eoc_lut_batch"),
    "eoc_lut_many_batch": engines_first("eoc_lut_many_batch"),
    "eoc_int_circuit_run": engines_first("eoc_int_circuit_run"),
    "eoc_circuit_run": engines_first("eoc_circuit_run"),
    "eoc_gate_batch": engines_first("eoc_gate_batch"),
}


@pytest.fixture(scope="module")
def ladder(built_lib):
    r = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1]
    return json.loads(line[len("RESULT"):])


@pytest.mark.parametrize("entry", sorted(EXPECTED))
def test_entry_ladder(ladder, entry):
    got = [tuple(x) for x in ladder[entry]]
    print(entry, got)
    assert got == EXPECTED[entry]

"""Every device call family interleaved on ONE engine with ONE key set on the MI355X, word for word against the families' own
references (the steps and schedules are in tests/interleave_cases.py).  The family modules check each call in
isolation on engines of their own; this one asks whether a call gives the right words when another family ran on the same
engine just ahead of it and a third is queued behind it -- through the one workspace, the grow-only scratch buffers, the derived
key images, the two modes and the slice knobs they share.

Per configuration (A and B: the two parameter sets' shapes at n = 40 with the shipped knobs; A-sliced: every slicing knob set):

  cold     a fresh engine, nothing reserved; the schedule -- F^2 + 1 calls, every ordered pair of families adjacent once, every
           family narrow / wide / narrow -- queued in windows of 64 calls with NO host synchronisation inside a window, windows
           alternating between a side stream and the NULL stream.  The buffers grow mid-window with earlier calls queued.  After a
           window: every position's words equal its reference, no output is still poison, every guard row is intact, and every
           cumulative counter moved by the sum of what one call of each position's (step, width) moves on a fresh engine.  One
           window runs under profiling; the leveled-rounding mode is switched by the schedule between leveled calls, and a
           leveled position's reference is that of the mode in force when it was queued
  warm     the same schedule on the same engine: eoc_engine_workspace_grows does not move, the words are equal again
  key swap (A, B) a second key set on the same engine -- cloud key (on B through the seeded form), packing key -- one narrow
           call of every family whose words depend on a key image, against the second key set's references; then the first
           again, then the second again

Then one reduced pass at full size (the shipped Set A keys: two equal cycles, every family narrow then wide, the second cycle
growing nothing) and the host-buffer calls of the global context in an all-ordered-pairs schedule of their own, on one and on
two engines.  tests/test_interleave_cpu.py checks the schedules' properties for the seeds used here.

Every comparison is byte for byte; there is no tolerance in this module."""
import os

import numpy as np
import pytest

import capture_cases as cc
import interleave_cases as ic
from gpu_util import sync, torch_cuda

pytestmark = pytest.mark.gpu
WINDOW = 64
PROFILED_WINDOW = 1
N = 1024
SLICED = {                                                       # values of the families' own slicing tests
    "EOC_TFHE_SLICE_SAMPLES": "16",                              # test_gpu_lut_tree, test_gpu_slice_seams
    "EOC_TFHE_TABLE_WS_BYTES": str(2 * 3 * 8192 + 100),          # two queries' samples at log2_lists = 2 (capture_cases)
    "EOC_TFHE_PACK_WS_BYTES": str(40 * N * 4 + 100),             # one list's columns (test_gpu_pack)
    "EOC_TFHE_DOT_WS_BYTES": str(9 * 16384 + 3 * 8192 + 100),    # one vector of 9 lists and its 3 scratch lists (test_gpu_dot)
    "EOC_TFHE_INT_SLICE_ROWS": "2",                              # capture_cases.IntCircuitSliced
    "EOC_TFHE_BR_SLICE": "64",                                   # jobs per blind-rotation launch
}
CONFIGS = {"A": dict(pset=0, env={}), "B": dict(pset=1, env={}), "A-sliced": dict(pset=0, env=SLICED)}
KEY_SEEDS = (71, 72)


@pytest.fixture(scope="module")
def eoc(built_lib):
    torch_cuda()
    import eoc_tfhe_amd
    yield eoc_tfhe_amd
    for c in _CONFIGS.values():
        c.close()
    for ks, _ in _KEYS.values():
        ks.close()
    _CONFIGS.clear()
    _KEYS.clear()
    _HOST.clear()


_KEYS, _CONFIGS, _HOST = {}, {}, {}     # (pset, which, seeded) -> (key set, its steps); name -> Config; the host-buffer steps


def keyset(eoc, pset, which=0, seeded=False):
    """(key set, its steps): shared by the configurations of one parameter set, so every reference is computed once"""
    key = (pset, which, seeded)
    if key not in _KEYS:
        ks = ic.KeySet(eoc, pset, KEY_SEEDS[which], seeded=seeded)
        _KEYS[key] = (ks, ic.registry(ks))
    return _KEYS[key]


def fresh_engine(eoc, ks, env):
    with cc.knobs({}):                                           # clears every knob of cc.KNOBS
        saved = os.environ.pop("EOC_TFHE_DOT_WS_BYTES", None)
        os.environ.update(env)
        try:
            eng = eoc.Engine(ks.p)
        finally:
            for k in env:
                os.environ.pop(k, None)
            if saved is not None:
                os.environ["EOC_TFHE_DOT_WS_BYTES"] = saved
    ks.install(eng)
    return eng


class Config:
    def __init__(self, eoc, name):
        self.eoc, self.name, self.env = eoc, name, CONFIGS[name]["env"]
        self.ks, self.steps = keyset(eoc, CONFIGS[name]["pset"])
        self.sched = ic.schedule(ic.NAMES, ic.SCHEDULE_SEEDS[name])
        self.plan = ic.mode_plan(self.sched, ic.LEVELED)
        self.entries = [(n, k, w, m) for (n, k, w), m in zip(self.sched, self.plan)]
        self.eng = self.runner = None
        self.iso, self.done = {}, set()

    def prepare(self):
        """what a pass compares with, made ahead of it: every position's reference, and for every (step, width) the counters
        one call moves alone on a fresh engine of this configuration"""
        ic.precompute(self.steps, self.entries)
        for name, _, width in self.sched:
            self.isolated(name, width)
        return self

    def again(self):
        """this configuration on another fresh engine, with the same references and isolated deltas"""
        c = Config(self.eoc, self.name)
        c.iso = self.iso
        return c

    def engine(self):
        if self.eng is None:
            self.eng = fresh_engine(self.eoc, self.ks, self.env)
            self.runner = ic.Runner(self.steps, self.eng)
        return self.eng

    def isolated(self, name, width):
        """the counters one call of (step, width) moves on a fresh engine of this configuration"""
        if (name, width) not in self.iso:
            self.engine()
            eng = fresh_engine(self.eoc, self.ks, self.env)
            r = ic.Runner(self.steps, eng)
            r.dev, r.snap = self.runner.dev, self.runner.snap    # the shared read-only inputs
            before = ic.counters(eng)
            pos = r.window([(name, 0, width, False)], None)
            sync()
            self.iso[(name, width)] = ic.moved(before, ic.counters(eng))
            bad = r.failures(pos)
            eng.close()
            assert not bad, ("alone on a fresh engine", bad)
        return self.iso[(name, width)]

    def run_pass(self, warm):
        torch, L = torch_cuda(), self.eoc.lib()
        self.prepare()
        eng, entries = self.engine(), self.entries
        side = torch.cuda.Stream()
        grows = L.eoc_engine_workspace_grows(eng.h)
        prev = None
        for wi, at in enumerate(range(0, len(entries), WINDOW)):
            win = entries[at:at + WINDOW]
            profiled = wi == PROFILED_WINDOW
            if profiled:
                eng.set_profiling(True)
                eng.kernel_times()
            before = ic.counters(eng)
            sync()
            positions = self.runner.window(win, side.cuda_stream if wi % 2 == 0 else None, first_index=at)
            sync()
            after = ic.counters(eng)
            if profiled:
                times = eng.kernel_times()
                eng.set_profiling(False)
                assert sum(t["launches"] for t in times.values()) > 0 and all(t["ms"] >= 0 for t in times.values()), times
            bad = self.runner.failures(positions, prev)
            assert not bad, (self.name, "warm" if warm else "cold", f"window {wi}", bad[:6], len(bad))
            prev = win[-1][0]
            want = {c: sum(self.isolated(n, w)[c] for n, _, w, _ in win) for c in after}
            got = ic.moved(before, after)
            assert got == want, (self.name, f"window {wi}", {c: (got[c], want[c]) for c in got if got[c] != want[c]})
            if warm:
                assert L.eoc_engine_workspace_grows(eng.h) == grows, (self.name, f"window {wi}", "a warm call grew a buffer")
        assert self.runner.inputs_intact() == [], "a call wrote into its read-only inputs"
        if not warm:
            assert L.eoc_engine_workspace_grows(eng.h) > grows
        self.done.add("warm" if warm else "cold")

    def ensure(self, *passes):
        for p in passes:
            if p not in self.done:
                self.run_pass(p == "warm")

    def close(self):
        if self.eng is not None:
            self.eng.close()
            self.eng = None


def config(eoc, name):
    if name not in _CONFIGS:
        _CONFIGS[name] = Config(eoc, name)
    return _CONFIGS[name]


@pytest.fixture(scope="module", params=list(CONFIGS))
def cfg(eoc, request):
    """a configuration with its key set, references and isolated counter deltas ready: the passes' set-up, kept out of their
    own time.  Closed with the module, by `eoc`"""
    return config(eoc, request.param).prepare()


def test_cold_pass(eoc, cfg):
    assert set(CONFIGS) == set(ic.SCHEDULE_SEEDS)
    assert ic.switches(cfg.plan) >= 4
    if "cold" not in cfg.done:
        cfg.run_pass(False)
        return
    c = cfg.again()                                              # another id ran this configuration's cold pass already
    try:
        c.run_pass(False)
    finally:
        c.close()


def test_warm_pass(eoc, cfg):
    cfg.ensure("cold")
    cfg.run_pass(True)


def br(m):
    return m["br_launches"] + m["br_wide_launches"]


def test_sliced_configuration_runs_every_wide_call_as_two_slices_or_more(eoc):
    """from the launch counters, for every family that has one: a wide call makes at least twice the launches of the same
    call under the shipped knobs (compact-expand and conv-extract by their key switches: ks_mfma_launches, Set A's key
    switch at every width).  Not sliced at all, in any configuration: cmux, demux, demux-accumulate, automaton-step, the two
    tgsw conversions and seeded-expand -- no knob reaches them, their wide calls run whole"""
    a, s = config(eoc, "A"), config(eoc, "A-sliced")
    checked = []
    for step in ic.STEPS:
        if step.sliced_by is None:
            continue
        whole, cut = a.isolated(step.name, "wide"), s.isolated(step.name, "wide")
        w, c = (br(whole), br(cut)) if step.sliced_by == "br" else (whole[step.sliced_by], cut[step.sliced_by])
        print(f"SLICES {step.name}: {step.sliced_by} {w} -> {c}")
        assert w >= 1 and c >= 2 * w, (step.name, step.sliced_by, w, c)
        checked.append(step.name)
    assert len(checked) == 23, checked


@pytest.mark.parametrize("name", ["A", "B"])
def test_key_swap(eoc, name):
    """d_ksl, d_pks, d_pkl and the bootstrapping key follow the key that is installed: on the engine the two passes ran on"""
    c = config(eoc, name).prepare()
    c.ensure("cold", "warm")
    eng, pset = c.eng, CONFIGS[name]["pset"]
    ks2, steps2 = keyset(eoc, pset, 1, seeded=name == "B")
    assert not np.array_equal(ks2.orc.ksk, c.ks.orc.ksk) and not np.array_equal(ks2.pk_rows, c.ks.pk_rows)
    eng.leveled_rounding = False
    for ks, steps in ((ks2, steps2), (c.ks, c.steps), (ks2, steps2)):
        ks.install(eng)
        r = ic.Runner(steps, eng)
        for j, name_ in enumerate(ic.KEYED):
            pos = r.window([(name_, 0, "narrow", False)], None, first_index=j)
            sync()
            bad = r.failures(pos)
            assert not bad, (name, f"key seed {ks.seed}", bad)
        assert r.inputs_intact() == []
    c.ks.install(eng)


@pytest.fixture(scope="module")
def full(eoc):
    """the full-size key set, its steps and the references of the two cycles: set-up, as `cfg` is"""
    ks = ic.KeySet.shared(eoc, 0)
    steps = ic.registry(ks)
    cyc = ic.cycle(ic.NAMES, ic.FULL_SEED)
    plan = ic.mode_plan(cyc, ic.LEVELED, every=3)
    entries = [(n, k, w, m) for (n, k, w), m in zip(cyc, plan)]
    ic.precompute(steps, entries)
    yield ks, steps, plan, entries
    ks.close()


def test_full_size_pass(eoc, full):
    """the shipped Set A keys the family modules share (n = 630: the real n1p, K steps of the packs and key-row sizes): two
    equal cycles, each visiting every family narrow then wide in a seeded order with no repeated neighbour pair, queued in
    windows under the cold-pass protocol; the second cycle grows nothing.  The wide shapes are the steps' `full` ones where
    the reference's cost grows with n: wider than the narrow call, so the scratch still grows, but short of a key-switch tile"""
    torch, L = torch_cuda(), eoc.lib()
    ks, steps, plan, entries = full
    assert ic.switches(plan) >= 4
    eng = fresh_engine(eoc, ks, {})
    runner = ic.Runner(steps, eng)
    side = torch.cuda.Stream()
    try:
        for rnd in range(2):
            grows, prev = L.eoc_engine_workspace_grows(eng.h), None
            for wi, at in enumerate(range(0, len(entries), WINDOW)):
                win = entries[at:at + WINDOW]
                positions = runner.window(win, side.cuda_stream if wi % 2 == 0 else None, first_index=at)
                sync()
                bad = runner.failures(positions, prev)
                assert not bad, (f"cycle {rnd}", f"window {wi}", bad[:6], len(bad))
                prev = win[-1][0]
            if rnd:
                assert L.eoc_engine_workspace_grows(eng.h) == grows, "the second cycle grew a buffer"
        assert runner.inputs_intact() == []
    finally:
        eng.close()


@pytest.fixture(scope="module")
def host_steps(eoc):
    """the host-buffer steps of configuration A's key set (its device steps re-used, so their references too), the schedule,
    the mode plan and every reference: set-up, as `cfg` is"""
    ks, dev = keyset(eoc, 0)
    if not _HOST:
        _HOST.update(ic.host_registry(ks, dev))
    sched = ic.schedule(ic.HOST_NAMES, ic.GLOBAL_SEED)
    plan = ic.mode_plan(sched, ic.LEVELED, every=3)
    ic.precompute(_HOST, [(n, k, w, m) for (n, k, w), m in zip(sched, plan)])
    return ks, _HOST, sched, plan


@pytest.mark.parametrize("devices", [[0], [0, 0]], ids=["one-engine", "two-engines"])
def test_global_context_host_buffer_calls(eoc, host_steps, devices):
    """the host-buffer calls of csrc/multi.hip in an all-ordered-pairs schedule of their own: one staging area per slot, the
    persistent workers, the per-device block frame; eoc_global_set_leveled_rounding switched inside the schedule.  Two passes,
    the second without staging growth"""
    ks, steps, sched, plan = host_steps
    assert ic.switches(plan) >= 4 and len(sched) == len(ic.HOST_NAMES) ** 2 + 1
    try:
        eoc.gpu_shutdown()
        eoc.gpu_init(ks.p, devices=devices)
        eoc.upload_cloud_key(ks.sk)
        eoc.global_import_packing_key_blob(ks.blob)
        for rnd in range(2):
            grows, mode, prev = eoc.stats_multi()["host_buffer_grows"], None, None
            for j, ((name, k, width), m) in enumerate(zip(sched, plan)):
                if m != mode:
                    eoc.set_leveled_rounding(m)
                    mode = m
                step = steps[name]
                got, want = step.host_form(step.host(k, width)), step.want(k, width, m)
                for out, w in want.items():
                    g = np.asarray(got[out])
                    assert ic.same_words(g, np.asarray(w).reshape(g.shape)), (f"pass {rnd}", j, prev, name, k, width, m, out,
                                                                             np.argwhere(g != np.asarray(w).reshape(g.shape))[:3].tolist())
                prev = name
            if rnd:
                assert eoc.stats_multi()["host_buffer_grows"] == grows, "the second pass grew a staging buffer"
    finally:
        try:
            eoc.set_leveled_rounding(False)
        finally:
            eoc.gpu_shutdown()

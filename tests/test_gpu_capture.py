"""Every device call family of the engine captured into a hipGraph (torch.cuda.CUDAGraph) on the MI355X and replayed on new
inputs, word for word against the family's existing reference.  The cases are in tests/capture_cases.py; the protocol is the
same for all of them:

  1. eager     input set 0, one call on a side stream: sizes every buffer, loads the code objects; equals the reference
  2. capture   the same call into a graph; eoc_engine_workspace_grows does not move
  3. replay    for sets 1 and 2: the inputs are written IN PLACE into the captured buffers; disturb() runs eager calls of the
               same family on other live buffers with other inputs (the captured shape, six times, and one call of another
               width or opcode mix that fits the sized workspace: the descriptor ring advances, h_perm, the scratch buffers,
               the staging rows and W.d_u are rewritten, a table walk of another depth ends in the other ping-pong buffer); the
               outputs are filled with a poison word; the grow counter still has the value of step 2 -- asserted AHEAD of the
               replay, because a call that grew a buffer has freed memory the graph refers to and such a graph must never be
               replayed; then the replay
  4. compare   every replayed word with the reference (where the reference is slow: a fixed sample of rows with the first and
               the last) and the whole output with an eager call of a second engine on the same inputs

What a graph bakes: every pointer, count, shape, the seed and first_idx of the seeded calls, the slice bounds and buffer
parities of the table walks, and the descriptors (copied from the engine's never-re-used pinned arena at every replay, or
carried as kernel arguments).  A replay varies only what sits in the device buffers the call was captured on.  The contract the
test relies on: after a capture, no call on that engine may grow a buffer.

Every comparison is byte for byte; there is no tolerance in this module.
The families interleaved on one engine, eagerly, are tests/test_gpu_interleave.py's subject.

Sensitivity (not part of the suite): with push_descs sending captured descriptors through the ring instead of the arena, and
EOC_CAPTURE_TEST_SAME_SHAPE_CALLS=1100 in the environment -- disturb() then makes that many calls of the captured shape on its
two live buffer sets and nothing else, so the ring wraps and every slot holds a live descriptor of the captured type -- the ids
whose descriptors travel through memory fail at the first replay with the poison word still in the output."""
import numpy as np
import pytest

import capture_cases as cc
from gpu_util import sync, to_dev, torch_cuda

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def eoc(built_lib):
    torch_cuda()
    import eoc_tfhe_amd
    return eoc_tfhe_amd


def assert_words(got, want, case, what):
    for name, w in want.items():
        g = case.pick(name, got[name])
        assert cc.bytes_equal(g, w), (what, name, np.argwhere(np.asarray(g) != np.asarray(w))[:4].tolist())


def side_stream(torch):
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    return st


def capture(torch, st, run):
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=st):
        run(st.cuda_stream)
    return g


def still_poisoned(case):
    """the outputs (by position in outs()) that hold nothing but the poison word"""
    torch = torch_cuda()
    return [j for j, t in enumerate(case.outs(case.bufs)) if bool((t.view(torch.int32) == cc.POISON).all())]


@pytest.mark.parametrize("name", list(cc.CASES))
def test_captured_call_replays_the_reference_words(eoc, name):
    torch, L = torch_cuda(), eoc.lib()
    c = cc.CASES[name](eoc)
    eng = c.eng
    st = side_stream(torch)
    # 1. eager
    c.set_inputs(0)
    c.poison()
    sync()
    st.wait_stream(torch.cuda.current_stream())
    before = eng.stats()
    with torch.cuda.stream(st):
        c.run(st.cuda_stream)
    st.synchronize()
    after = eng.stats()
    for counter, delta in c.expect.items():
        assert after[counter] - before[counter] == delta, (name, counter)
    assert_words(c.fetch(), c.want(0), c, "eager")
    # 2. capture
    c.set_inputs(0)
    sync()
    grows = L.eoc_engine_workspace_grows(eng.h)
    g = capture(torch, st, c.run)
    assert L.eoc_engine_workspace_grows(eng.h) == grows
    # 3. replay
    got = {}
    for k in (1, 2):
        c.set_inputs(k)
        c.disturb()
        c.poison()
        sync()
        assert L.eoc_engine_workspace_grows(eng.h) == grows, "a call after the capture grew a buffer: the graph is void"
        g.replay()
        sync()
        got[k] = c.fetch()
        assert not still_poisoned(c), (name, k, "the replay left the poison word in outputs", still_poisoned(c))
        assert_words(got[k], c.want(k), c, f"replay {k}")           # at once: a wrong first replay is the finding
    if name == "table-update":
        # the update accumulates: a second replay WITHOUT the reset gives the reference's words for two updates
        assert L.eoc_engine_workspace_grows(eng.h) == grows
        g.replay()
        sync()
        assert cc.bytes_equal(c.fetch()["out"], c.updated(c.want(2)["out"], 2))
    # 4. the whole output against a second engine's eager call
    for k in (1, 2):
        second = c.second(k)
        for out, words in got[k].items():
            assert cc.bytes_equal(words, second[out]), (name, k, out)
    del g
    c.close()


# ---- arena exhaustion -------------------------------------------------------------------------------------------------------
GATES, WIRES_IN = 300, 8


def netlist(eoc):
    """one level of 300 independent two-input gates over 8 input wires"""
    ops = [eoc.OPS[o] for o in ("NAND", "XOR", "AND", "OR", "XNOR", "NOR")]
    return [eoc.Gate(ops[g % len(ops)], g % WIRES_IN, (3 * g + 1) % WIRES_IN, -1, WIRES_IN + g) for g in range(GATES)]


def netlist_oracle(orc, gates, wires):
    ref = wires.copy()
    for op in sorted({g.op for g in gates}):
        sel = [g for g in gates if g.op == op]
        out = orc.gate_batch(op, np.concatenate([wires[g.in0] for g in sel]), np.concatenate([wires[g.in1] for g in sel]))
        for j, g in enumerate(sel):
            ref[g.out] = out[j:j + 1]
    return ref


class Arena:
    """a reserved engine (descriptor ring of 1024, so an arena of 4096) and graphs of the netlist captured on one wire buffer
    until push_descs refuses: 13 graphs of 300 descriptors fit, the 14th capture is refused"""

    def __init__(self, eoc):
        torch, L = torch_cuda(), eoc.lib()
        self.eoc, self.torch, self.L = eoc, torch, L
        self.p, self.sk, self.orc, _ = cc.small_keys(eoc, 0, 40, 61)
        with cc.knobs({}):
            self.eng = eoc.Engine(self.p)
        self.eng.load_cloud_key(self.sk)
        self.rows_mixed = 2000
        assert L.eoc_engine_reserve(self.eng.h, 2048, 1024, self.rows_mixed) == 0
        self.gates = netlist(eoc)
        self.n_wires = WIRES_IN + GATES
        self.wires = torch.zeros((self.n_wires, 1, self.p.n + 1), dtype=torch.int32, device="cuda")
        self.st = side_stream(torch)
        self.set_inputs(0)
        with torch.cuda.stream(self.st):
            self.run(self.st.cuda_stream)
        self.st.synchronize()
        self.check("eager")
        self.grows = L.eoc_engine_workspace_grows(self.eng.h)
        self.graphs = []
        with pytest.raises(eoc.EocError, match=r"graph capture: descriptor arena exhausted \("):
            for _ in range(20):
                g = capture(torch, self.st, self.run)           # a refused capture is discarded with its CUDAGraph object
                self.graphs.append(g)
        sync()
        assert len(self.graphs) == 4096 // GATES == 13

    def run(self, stream):
        self.eng.circuit_run_device(self.gates, self.wires.data_ptr(), self.n_wires, 1, stream=stream)

    def set_inputs(self, k):
        rng = np.random.default_rng(70 + k)
        self.host = np.zeros((self.n_wires, 1, self.p.n + 1), np.int32)
        for w in range(WIRES_IN):
            self.host[w] = self.sk.encrypt_bits(rng.integers(0, 2, 1).astype(np.uint8), 1000 + 10 * k + w)
        self.wires.copy_(to_dev(self.host))
        self.wires[WIRES_IN:].fill_(cc.POISON)
        sync()

    def check(self, what):
        assert cc.bytes_equal(self.wires.cpu().numpy(), netlist_oracle(self.orc, self.gates, self.host)), what

    def replay_first_and_last(self):
        for k, g in ((1, self.graphs[0]), (2, self.graphs[-1])):
            self.set_inputs(k)
            assert self.L.eoc_engine_workspace_grows(self.eng.h) == self.grows
            g.replay()
            sync()
            self.check(f"replay of graph {k}")

    def close(self):
        self.graphs.clear()
        self.eng.close()


def test_arena_exhaustion_is_refused_and_earlier_graphs_still_replay(eoc):
    a = Arena(eoc)
    a.replay_first_and_last()
    a.set_inputs(3)                                             # an eager call afterwards works (the ring, not the arena)
    a.run(None)
    sync()
    a.check("eager call after the refusal")
    a.replay_first_and_last()                                   # ... and leaves the graphs alone
    a.close()


def test_arena_exhaustion_by_a_mixed_batch_permutation(eoc):
    """the second refusal site: 13 netlist graphs leave 196 arena slots, the permutation of a 2000-row mixed batch on the
    gather path wants 200"""
    torch = torch_cuda()
    a = Arena(eoc)
    S, n1 = a.rows_mixed, a.p.n + 1
    rng = np.random.default_rng(77)
    ops = rng.choice(np.array([0, 4, 1, 2, 11, 13], np.uint8), S)
    assert (np.diff(ops.astype(int)) != 0).sum() + 1 > 15       # the gather path
    c = [a.sk.encrypt_bits(rng.integers(0, 2, S).astype(np.uint8), 1100 + j) for j in range(2)]
    d = [to_dev(x) for x in c]
    out = torch.full((S, n1), cc.POISON, dtype=torch.int32, device="cuda")

    def mixed(stream):
        a.eng.gate_batch_device(0, d[0].data_ptr(), d[1].data_ptr(), None, out.data_ptr(), S, ops=ops, stream=stream)

    mixed(None)                                                 # outside capture: the shape is served
    sync()
    sample = np.r_[0:24, S // 2:S // 2 + 8, S - 24:S]
    want = a.orc.gate_batch(0, c[0][sample], c[1][sample], ops=ops[sample])
    assert cc.bytes_equal(out.cpu().numpy()[sample], want)
    assert a.L.eoc_engine_workspace_grows(a.eng.h) == a.grows
    with pytest.raises(eoc.EocError, match="descriptor arena exhausted by a mixed batch's permutation"):
        capture(torch, a.st, mixed)
    sync()
    a.replay_first_and_last()
    out.fill_(cc.POISON)
    mixed(None)                                                 # an eager call afterwards works
    sync()
    assert cc.bytes_equal(out.cpu().numpy()[sample], want)
    a.replay_first_and_last()
    a.close()

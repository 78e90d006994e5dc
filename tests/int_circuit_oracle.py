"""An integer netlist (eoc_inode list) evaluated on the CPU oracle: the byte-for-byte reference of
eoc_int_circuit_run_device.  The linear stage is wrapping-int32 numpy; a node with one table goes through
lut_oracle.bootstrap, a many-LUT node through lut_many_oracle.bootstrap_many.  Test-side only."""
import numpy as np

import lut_many_oracle as lmo
import lut_oracle as lo


def linear(node, wires):
    """t [instances][n+1] int32 of one node: sum_k w[k] wires[in[k]] + (0, ..., 0, cst), wrapping"""
    acc = np.zeros(wires.shape[1:], np.int64)
    for k in range(node.n_terms):
        acc += int(node.w[k]) * wires[node.in_[k]].astype(np.int64)
    acc[:, -1] += int(node.cst)
    return (acc & 0xFFFFFFFF).astype(np.uint32).view(np.int32)


def run(orc, nodes, tvs, wires):
    """wires [n_wires][instances][n+1] with the input wires' rows filled in -> a copy with every written wire filled in"""
    wires = np.array(wires, np.int32)
    for q in nodes:
        t = linear(q, wires)
        if q.n_tables == 0:
            wires[q.out] = t
        elif q.n_tables == 1:
            wires[q.out] = np.stack([lo.bootstrap(orc, tvs[q.tv], row) for row in t])
        else:
            res = np.stack([lmo.bootstrap_many(orc, tvs[q.tv], row, q.n_tables) for row in t])      # [instance][T][n+1]
            for j in range(q.n_tables):
                wires[q.out + j] = res[:, j]
    return wires

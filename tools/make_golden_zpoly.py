#!/usr/bin/env python3
"""tests/golden/g15_maxcut_diag.npz: MaxCut cost diagonals computed by the reference (run in the build container only; same
provenance rules as tools/make_golden.py, whose helpers it uses: the reference is RUN, never copied).

For n = 8, 10 and 12 nodes, with `random` and `np.random` seeded, the record is the edge list of the reference's
max_cut.build_graph -- (u, v, w) rows -- and the array of its max_cut.graph_to_diagonal_h.  Only these data are stored; the
largest array is 4096 doubles."""
import os
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402


def main():
  xg = mg.load_ref_xgates()
  sys.modules['libxgates'] = xg
  mg.install_absl_stub(tempfile.mkdtemp(prefix='qcc_golden_zpoly_'))
  sys.path.insert(0, mg.REF)
  from src import max_cut  # the reference
  out = {}
  for n in (8, 10, 12):
    random.seed(1500 + n)
    np.random.seed(1500 + n)
    nn, edges = max_cut.build_graph(n)
    assert nn == n
    diag = np.asarray(max_cut.graph_to_diagonal_h(n, edges), dtype=np.float64)
    assert diag.shape == (1 << n,)
    out[f'edges{n}'] = np.asarray([[float(u), float(v), float(w)] for u, v, w in edges], dtype=np.float64)
    out[f'diag{n}'] = diag
  path = os.path.join(mg.OUT, 'g15_maxcut_diag.npz')
  np.savez_compressed(path, nodes=np.array([8, 10, 12]), **out)
  print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
  main()

#!/usr/bin/env python3
"""Random programs over the whole device API against the NumPy model (run on the GPU box), for longer than the suite does.

The generator and the runner are the suite's (tests/program_model.py; tests/test_gpu_program_fuzz.py runs a fixed list):
queued gate bursts, barrier mutators (dense matrices, table-selected gates, diagonals, register permutations, scalings,
projections), readers, handle steps, two-state steps, Pauli-sum operators (qh_apply_pauli_sum / qh_pauli_sum_new), in-place Pauli
products (qh_apply_pauli_product), reduced density matrices (qh_reduced_density), Z-polynomials (qh_apply_zpoly /
qh_expect_zpoly) and layout steps, program after program, seeds SEED, SEED + 1, ...,
each at both widths, until SECONDS have passed.  It ENDS AT THE FIRST FAILURE of any kind -- a step the model disagrees
with, or an exception such as a QhError that wraps a HIP fault: no further program is started on a device that may have
faulted.  The failure prints one JSON line with the seed, the width, the mode, the index of the failing step and the step,
so that gen_program(seed, bw, mode) replays it (on tests.program_model.NumpyDevice first), then the summary line; the exit
status is then 1.
usage: fuzz_programs.py [SECONDS] [SEED] [MODE]     MODE: own (default) | shard | attached | mapped | all"""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import program_model as pm  # noqa: E402


def main(make_state=pm.make_device_state):
  budget = float(sys.argv[1]) if len(sys.argv) > 1 else 60.0
  seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
  mode = sys.argv[3] if len(sys.argv) > 3 else 'own'
  modes = ['own', 'shard', 'attached', 'mapped'] if mode == 'all' else [mode]
  t0 = time.time()
  programs = fails = 0
  while not fails and time.time() - t0 < budget:
    for md, bw in [(md, bw) for md in modes for bw in (128, 64)]:
      programs += 1
      where = {'FAIL': seed, 'bw': bw, 'mode': md, 'env': {k: v for k, v in os.environ.items() if k.startswith('QH_')}}
      try:
        pm.run_program(pm.gen_program(seed, bw, md), make_state, pm.Check(bw))
      except pm.StepFailure as e:
        fails += 1
        print(json.dumps(dict(where, step_index=e.index, step=pm.describe(e.step), what=e.what[:400])), flush=True)
      except Exception as e:  # pylint: disable=broad-except
        # the generator's own assertion, or anything the runner did not expect: still one line that names the seed
        fails += 1
        print(json.dumps(dict(where, step_index=None, step=None, what=f'{type(e).__name__}: {e}'[:400])), flush=True)
      if fails:
        break                                                # the first failure is the last program
    seed += 1
  print(json.dumps({'programs': programs, 'failures': fails, 'seconds': round(time.time() - t0, 1), 'next_seed': seed, 'mode': mode}))
  sys.exit(1 if fails else 0)


if __name__ == '__main__':
  main()

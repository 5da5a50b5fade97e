"""Every handler of every sweep island, run on the GPU against the oracle: the corpus of tests/handler_corpus.py, whose
coverage of the islands' branch tables tests/test_handler_coverage_cpu.py proves on planner-only handles.  Before a case
is flushed, the live handle must report the very handler words the planner-only handle reported (qh_plan_handlers): what
was proved on the CPU is then what runs.

Bounds.  complex128: TOL of tests/test_gpu_parity.py.  complex64: the oracle runs in complex64, as in the parity tests; the
bound is max(3e-6, 8 x max|oracle_c64 - oracle_c128|) per case, from the two reference runs alone -- 3e-6 is the parity
tests' bound, the factor 8 allows another summation order over at most ~40 gates."""
import numpy as np
import pytest

from qcc_amd import device, native
from tests import handler_corpus as hc
from tests.test_gpu_parity import TOL
from tests.test_handler_coverage_cpu import describe

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('island', hc.ISLANDS, ids=[hc.island_id(i) for i in hc.ISLANDS])
def test_island_handlers_vs_oracle(oracle, monkeypatch, island):
  bw = island[0]
  dt = np.complex128 if bw == 128 else np.complex64
  claims = hc.load_claims()
  cases = [c for c in hc.CASES if c.island == island]
  assert cases
  lib = native.load()
  states = {}
  worst_ratio, worst_case = 0.0, None
  try:
    for c in cases:
      what = (c.name, [describe(island, k) for k in sorted(claims[c.name])])
      dry_words, _ = hc.dry_plan(c)
      psi0 = hc.case_state(c)
      want = hc.oracle_apply(oracle, psi0.astype(dt), c)
      if bw == 128:
        bound = TOL
      else:
        want128 = hc.oracle_apply(oracle, psi0.astype(dt).astype(np.complex128), c)
        bound = max(3e-6, 8.0 * float(np.max(np.abs(want.astype(np.complex128) - want128))))
      key = (c.n, c.env.get('QH_RELAYOUT', '1'))      # (a handle decides once whether it re-lays out)
      if key not in states:
        states[key] = device.DeviceState(c.n, bw, fusion=native.QH_FUSE_SWEEP)
      st = states[key]
      st.upload(psi0.astype(dt))
      for k, v in c.env.items():
        monkeypatch.setenv(k, v)
      hc.queue_case(lib, st.h, c)
      live_words = hc.plan_handlers(lib, st.h)
      assert live_words == dry_words, ('the live handle plans other handlers than the planner-only handle', what)
      st.flush()
      for k in c.env:
        monkeypatch.delenv(k)
      got = st.download()
      err = float(np.max(np.abs(got.astype(np.complex128) - want.astype(np.complex128))))
      if err / bound > worst_ratio:
        worst_ratio, worst_case = err / bound, c.name
      assert err <= bound, ('GPU result differs from the oracle', err, bound, what)
  finally:
    for st in states.values():
      st.close()
  print(f'{hc.island_id(island)}: {len(cases)} cases, worst error / bound = {worst_ratio:.3g} ({worst_case})')

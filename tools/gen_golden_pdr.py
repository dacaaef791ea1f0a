#!/usr/bin/env python3
"""Golden fixtures for the priority-dispatch-rule baselines: run the REFERENCE's
`tester.pdrs.run_Rules_jointActions_withMinus_1217` (tester/pdrs.py:606-839) for all 12 rule pairs of test_all.py:484-540 on
  - the 16 instances of tests/golden/trace_j6m6e2_eval16_free.npz            -> tests/golden/pdr_j6m6e2_eval16.npz
  - 4 reference-generated J10M10E2 instances (M >= 8: numpy's pairwise row sum) -> tests/golden/pdr_j10m10e2_b4.npz
and record, per rule pair and instance, the dispatch plan (`operation_lst` as 0-based task indices, `machine_lst`), the five
cumulative reward sums and the four final costs (`untilNow`).  `random.seed(k)` (k = instance index) precedes every run, and the
column orders that MOR's `random.shuffle` produced are recorded, so that a test can replay them.

Build machine only: imports the reference through oracle/ref_harness/bootstrap.py, copies nothing of it; never imported by a
GPU test.  Usage: python tools/gen_golden_pdr.py
"""
import contextlib
import io
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "oracle", "ref_harness"))
from bootstrap import bootstrap, default_config  # noqa: E402

REF = bootstrap(models=True)
GOLDEN = os.path.join(ROOT, "tests", "golden")

with contextlib.redirect_stdout(io.StringIO()):
    try:
        import trainer.fig_kpi  # noqa: F401  (plotting; only its name is needed by tester.pdrs)
    except Exception:
        stand_in = types.ModuleType("trainer.fig_kpi")
        stand_in.result_box_plot = lambda *a, **k: None
        sys.modules["trainer.fig_kpi"] = stand_in
    import tester.pdrs as pdrs  # noqa: E402
    from gen_golden import ref_generate  # noqa: E402  (the reference generator with instance/config_ins.json's values)

M_NAMES = ["SPT", "SEC"]                                                              # pdrs.py:729
O_NAMES = ["FIFO", "MOR", "LWKR_T_o", "LWKR_PT_o", "MWKR_T_o", "MWKR_PT_o"]           # pdrs.py:730


_BASE = pdrs.FJSP_Rules


class Recorder(_BASE):
    """the reference's rules, keeping what each call returned (run_Rules only prints its two lists)"""
    last = {}

    def _keep(self, kind, val):
        Recorder.last[kind] = np.asarray(val).copy()
        return val


for _name, _kind in (("FIFO_o", "o"), ("MOR_o", "o"), ("LWKR_T_o_jointActor", "o"), ("LWKR_PT_o_jointActor", "o"),
                     ("SPT_m", "m"), ("SEC_m", "m")):
    def _wrap(self, *a, _n=_name, _k=_kind, **k):
        return self._keep(_k, getattr(_BASE, _n)(self, *a, **k))
    setattr(Recorder, _name, _wrap)
pdrs.FJSP_Rules = Recorder


def record(t, p, tt, edge, J, M, E):
    N, T = t.shape[0], J * M
    data = types.SimpleNamespace(t=t, p=p, transT=tt, edge=edge)
    cfg = default_config(J, M, E, 1)
    task = np.zeros((12, N, T), np.int32); mach = np.zeros((12, N, T), np.int32)
    cum = np.zeros((12, N, 5)); final4 = np.zeros((12, N, 4))
    mor = np.zeros((2, N, M, J), np.int32)
    names, o_rule, m_rule = [], [], []
    for o in range(6):
        for m in range(2):
            r = 2 * o + m
            names.append(f"{O_NAMES[o]}+{M_NAMES[m]}"); o_rule.append(o); m_rule.append(m)
            for k in range(N):
                random.seed(k)
                Recorder.last = {}
                with contextlib.redirect_stdout(io.StringIO()):
                    _, cost, until = pdrs.run_Rules_jointActions_withMinus_1217(cfg, o, m, data, k, None, None)
                task[r, k] = Recorder.last["o"].astype(np.int64) - 1
                mach[r, k] = Recorder.last["m"]
                cum[r, k] = [cost["opr_Gt"], cost["opr_mk"], cost["opr_idleT"], cost["opr_pt"], cost["opr_transT"]]
                final4[r, k] = until
                if o == 1:
                    mor[m, k] = (task[r, k] // M).reshape(M, J)
    assert np.array_equal(mor[0], mor[1]), "same seed, same shuffle for both machine rules"
    return {"meta": np.array([J, M, E, N], np.int32), "t": t, "p": p, "tt": tt, "edge": edge,
            "names": np.array(names), "o_rule": np.array(o_rule, np.int32), "m_rule": np.array(m_rule, np.int32),
            "task": task, "machine_lst": mach, "cum": cum, "final4": final4, "mor_order": mor[0],
            "cfg_w": np.array([cfg["weight_mk"], cfg["weight_ec"], cfg["weight_tt"]])}


def main():
    g = np.load(os.path.join(GOLDEN, "trace_j6m6e2_eval16_free.npz"))
    J, M, E = [int(x) for x in g["meta"][:3]]
    for name, d in (("pdr_j6m6e2_eval16", record(g["t"], g["p"], g["tt"], g["edge"], J, M, E)),
                    ("pdr_j10m10e2_b4", record(*ref_generate(4, 10, 10, 2, 21), 10, 10, 2))):
        path = os.path.join(GOLDEN, name + ".npz")
        np.savez_compressed(path, **d)
        print(f"wrote {path} ({os.path.getsize(path) / 1024:.0f} KiB)")


if __name__ == "__main__":
    main()

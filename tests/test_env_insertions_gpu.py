"""PARITY (GPU): every step kernel on the insertion branches and on exact ties, against the C oracle after EVERY step
(tests/env_parity.py).

The other every-step comparisons draw the job from the unmasked jobs; the round-robin job mask keeps all jobs in lockstep, and an
operation then almost never fits before or between the operations already on its machine: the front insertion and the gap insertion
— the parallel gap test reduced to the first hit in route order, the mid-route insert, the removed and merged edge with its two new
weights, the observation rows rewritten behind it — run in 0 to 4 steps per thousand.  Here the actions ignore the mask
(policy="blocks": a job is kept for a run of steps; "jobseq": one job after another), which sends 4 to 13 % of all steps down the front
path and 21 to 50 % down the gap path.

data="integer" makes times small integers.  The three comparisons that choose the path — lb_ft <= arrival(first),
lb_ft > arrival(next), gap < d — differ from their neighbours (< for <=, and so on) only where two times are exactly equal, which
products of uniform doubles never are.  Every row also runs on generated data in f32: the insertions without ties, to tell the two
defects apart.

The table names the kernel of every row and the GPU test asserts that the dispatch reaches it; tests/test_env_insertions_cpu.py walks
the same table without a GPU and proves on the oracle that every row reaches the paths and the ties it is about.  Shapes are the
smallest that reach each kernel path; every batch ends in a partly filled group.  Left shift is on everywhere.
"""
from collections import namedtuple

import pytest

from env_parity import run_parity

Row = namedtuple("Row", "family force J M E B kernel seed")
Case = namedtuple("Case", "row policy data obs_dtype")

J6M6, J8M8 = (6, 6, 2), (8, 8, 2)
J10M10, J11M11, J7M9 = (10, 10, 2), (11, 11, 1), (7, 9, 1)
J5M12, J13M10, J20M15 = (5, 12, 2), (13, 10, 2), (20, 15, 3)


def _rows(family, forces, shapes, B, seed=3):
    return [Row(family, f, *s, B, k, seed) for f, k in forces for s in shapes]


ROWS = (
    # one task slot per lane; B = 19: one full group of 16 + 3, four full groups of 4 + 3
    _rows("one_slot", [("grp16", "k_env_grp16"), ("grp4", "k_env_grp4"), ("reg1", "k_env_reg")], [J6M6, J8M8], 19)
    # two task slots per lane: T = 100, 121, and J7M9 (T = 63, M*M = 81: the second slot of every lane is empty)
    + _rows("two_slot", [("grp16", "k_env_grp16x2"), ("grp4", "k_env_grp4x2")], [J10M10, J11M11, J7M9], 19)
    # the grouped LDS kernel forced on a register-kernel shape; B = 11: one full group of 8 + 3
    + _rows("lds_forced", [("lds", "k_env_step_grp")], [J6M6], 11)
    # the grouped LDS kernel by the default dispatch: J5M12 (a single, partly filled wave of tasks), J13M10 (T = 130), J20M15
    # (T = 300: two reduction levels)
    + _rows("lds_default", [(None, "k_env_step_grp")], [J5M12, J13M10, J20M15], 11)
    # one instance per workgroup; seed 3 gives these three instances no tie at the gap test, seed 7 gives every kind
    + _rows("lds1", [("lds1", "k_env_step")], [J6M6], 3, seed=7)
)
FAMILIES = ("one_slot", "two_slot", "lds_forced", "lds_default", "lds1")
# one row per family also runs with the jobs one after another
JOBSEQ = {"one_slot": ("grp16", J6M6), "two_slot": ("grp4", J10M10), "lds_forced": ("lds", J6M6), "lds_default": (None, J13M10),
          "lds1": ("lds1", J6M6)}

CASES = ([Case(r, "blocks", "integer", d) for r in ROWS for d in ("f32", "f64")]
         + [Case(r, "blocks", "generated", "f32") for r in ROWS]
         + [Case(r, "jobseq", "integer", "f32") for r in ROWS if JOBSEQ[r.family] == (r.force, (r.J, r.M, r.E))])


def case_id(c):
    r = c.row
    return f"{r.family}-{r.force or 'default'}-J{r.J}M{r.M}E{r.E}-B{r.B}-{c.policy}-{c.data}-{c.obs_dtype}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_insertions_and_ties_equal_the_oracle_at_every_step(case, monkeypatch):
    r = case.row
    n = run_parity(r.J, r.M, r.E, r.B, case.obs_dtype, left_shift=True, seed=r.seed, force=r.force, monkeypatch=monkeypatch,
                   expect_kernel=r.kernel, policy=case.policy, data=case.data)
    assert n == r.J * r.M

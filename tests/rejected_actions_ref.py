"""Rejected actions in mixed batches (plain host module): the expected side and the schedule of actions.

include/mtfjsp.h promises that a step with a bad action — task already scheduled, job predecessor unscheduled, an index out of range —
leaves the instance untouched and sets MTFJSP_ST_INVALID.  The oracle's own schedule() mirrors the reference's behaviour on such an
action (it corrupts node attributes, env:1496-1528), so the expected side never makes that call:

  Expected   B OracleBatch objects of batch 1, one per instance.  An instance whose action is valid steps its own oracle (and calls
             job_mask_update); an instance whose action is rejected does nothing, so its state, observation, candidate, mask and its
             17 RewardScaling words are its oracle's current ones.  What a rejected step writes is stated here once: info row
             [0, d, 0, 0, 0, 0] with d = 1.0 iff all T tasks of the instance are scheduled, raw row zeros, status ST_INVALID exactly.
             Whether an action is rejected is decided from the oracle's scheduled flags alone (Expected.rejected), never from the
             kind the schedule meant to draw.

  Schedule   deterministic from a seed and drawn from the expected side's own state, the way env_parity.random_valid draws valid
             actions.  Per step and instance either a valid action or one rejection kind:
               a  task -1                       b  task T                  c  task 2**31-1 ("c+") or -2**31 ("c-")
               d  valid task, machine -1        e  valid task, machine M
               f  a task that is already scheduled, with a feasible machine
               g  the task after a candidate whose op is not the last one: its job predecessor is unscheduled
               h  any of a-f, or the instance's formerly valid last action ("h:last"), after the instance has finished
             Step 0 rejects the whole batch (nothing is scheduled: a-e and g); step GROUP_STEP rejects exactly the first `group`
             instances (the first workgroup of the kernel under test) and nobody else; step NOBODY_STEP rejects nobody; otherwise a
             running instance is rejected with probability 1/3.  The episode runs until every instance has finished plus
             EXTRA_STEPS steps on the all-finished batch, so instances finish at different steps and the early ones receive kind h
             beside running neighbours.
"""
from collections import namedtuple

import numpy as np

from oracle.env_oracle import OracleBatch

ST_INVALID, ST_INFEASIBLE = 0x100, 0x200           # include/mtfjsp.h (the CPU test holds them to capi's)
GROUP_STEP, NOBODY_STEP, EXTRA_STEPS = 3, 5, 2
P_REJECT = 1.0 / 3.0
INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
KINDS = ("a", "b", "c+", "c-", "d", "e", "f", "g", "h")
GROUP = {"k_env_grp16": 16, "k_env_grp16x2": 16, "k_env_grp4": 4, "k_env_grp4x2": 4, "k_env_step_grp": 8, "k_env_reg": 1, "k_env_step": 1}


class Expected:
    """B batch-1 oracles and, as [B, ...] arrays that a step updates only for the instances it stepped, everything the device is
    compared with: info, raw, status, the observation (tfea [B*T,12], mfea2, adj), cand, mask, vmask (valid_action_mask) and the
    state arrays of OracleBatch.state() (mach, sched, st, ft, routes, prev, scaler) plus w3."""

    def __init__(self, t, p, tt, edge, left_shift=True):
        self.B, self.T, self.M = t.shape
        self.J = self.T // self.M
        self.feas = t >= 0
        self.orc = [OracleBatch(t[b:b + 1], p[b:b + 1], tt[b:b + 1], edge[b:b + 1], left_shift=left_shift) for b in range(self.B)]
        self.last_valid = [None] * self.B

    def scaler_init(self):
        for o in self.orc:
            o.scaler_init()

    def scaler_reset_returns(self):
        for o in self.orc:
            o.scaler_reset_returns()
        self._refresh_state(range(self.B))

    def reset(self, w3):
        B, T, M, J = self.B, self.T, self.M, self.J
        self.w3 = np.ascontiguousarray(w3, np.float64).copy()
        self.info, self.raw, self.status = np.zeros((B, 6)), np.zeros((B, 5)), np.zeros(B, np.int32)
        self.tfea, self.mfea2, self.adj = np.zeros((B * T, 12)), np.zeros((B, M, 8)), np.zeros((B, T, T))
        self.cand, self.mask, self.vmask = np.zeros((B, J), np.int32), np.zeros((B, J), np.uint8), np.zeros((B, T), np.uint8)
        self.state = dict(mach=np.zeros((B, T), np.int32), sched=np.zeros((B, T), np.uint8), st=np.zeros((B, T)), ft=np.zeros((B, T)),
                          routes=np.zeros((B, M, T), np.int32), prev=np.zeros((B, 4)), scaler=np.zeros((B, 17)))
        for b, o in enumerate(self.orc):
            o.reset(self.w3[b:b + 1])
            self.cand[b], self.mask[b] = (x[0] for x in o.job_mask_state())
        self._refresh_obs(range(B)); self._refresh_state(range(B))
        self.last_valid = [None] * B

    def _refresh_obs(self, which):
        T = self.T
        for b in which:
            o = self.orc[b].observe()
            self.tfea[b * T:(b + 1) * T], self.mfea2[b], self.adj[b] = o["tfea"], o["mfea2"][0], o["adj"][0]
            self.vmask[b] = self.orc[b].valid_action_mask()[0]

    def _refresh_state(self, which):
        for b in which:
            for k, v in self.orc[b].state().items():
                self.state[k][b] = v[0]

    def finished(self):
        """[B] bool: all T tasks of the instance are scheduled"""
        return self.state["sched"].all(axis=1)

    def rejected(self, task, mach):
        """[B] bool: the header's rule — an index out of range, the task already scheduled, its job predecessor unscheduled"""
        T, M, sched = self.T, self.M, self.state["sched"]
        out = np.zeros(self.B, bool)
        for b in range(self.B):
            a, m = int(task[b]), int(mach[b])
            out[b] = not (0 <= a < T and 0 <= m < M) or bool(sched[b, a]) or (a % M != 0 and not sched[b, a - 1])
        return out

    def step(self, task, mach):
        """-> the [B] bool mask of rejected instances; every array of the expected side is then that of after the step"""
        rej = self.rejected(task, mach)
        done = self.finished()
        stepped = []
        for b in range(self.B):
            if rej[b]:
                self.info[b] = [0.0, 1.0 if done[b] else 0.0, 0.0, 0.0, 0.0, 0.0]
                self.raw[b] = 0.0
                self.status[b] = ST_INVALID
                continue
            a, m = np.array([task[b]], np.int32), np.array([mach[b]], np.int32)
            info, raw, paths = self.orc[b].step(a, m)
            cand, mask = self.orc[b].job_mask_update(a // self.M)
            self.info[b], self.raw[b], self.cand[b], self.mask[b] = info[0], raw[0], cand[0], mask[0]
            self.status[b] = int(paths[0]) | (0 if self.feas[b, a[0], m[0]] else ST_INFEASIBLE)
            self.last_valid[b] = (int(a[0]), int(m[0]))
            stepped.append(b)
        self._refresh_obs(stepped); self._refresh_state(stepped)
        return rej

    def rows_rewritten(self, task, rej):
        """flat tasks_fea rows a step is to rewrite in full: the acting task .. the end of its job, of the instances not rejected"""
        T, M = self.T, self.M
        rows = [b * T + np.arange(task[b], (task[b] // M + 1) * M) for b in range(self.B) if not rej[b]]
        return np.concatenate(rows) if rows else np.zeros(0, np.int64)


class Schedule:
    """draw() -> (task [B] int32, mach [B] int32, kinds [B]: None for an action meant to be valid, else one of KINDS, "h:<sub>" after
    the instance has finished) from the expected side's state BEFORE the step; the caller then steps the expected side.  over():
    every instance has finished and EXTRA_STEPS more steps were drawn."""

    def __init__(self, exp, seed, group):
        self.exp, self.rs, self.group, self.s, self.extra = exp, np.random.RandomState(seed), group, 0, 0

    def over(self):
        return self.extra >= EXTRA_STEPS

    def _valid(self, b):
        """a uniformly drawn valid (task, machine) of instance b: an unmasked job's candidate, a feasible machine (random_valid)"""
        e = self.exp
        j = self.rs.choice(np.flatnonzero(e.mask[b] == 0))
        a = int(e.cand[b, j])
        return a, int(self.rs.choice(np.flatnonzero(e.feas[b, a])))

    def _possible(self, b):
        e, M = self.exp, self.exp.M
        sched = e.state["sched"][b]
        nsj = sched.reshape(e.J, M).sum(axis=1, dtype=np.int64)
        kinds = ["a", "b", "c+", "c-"]
        if not sched.all():
            kinds += ["d", "e"]
        if sched.any():
            kinds.append("f")
        if (nsj < M - 1).any():
            kinds.append("g")
        return kinds

    def _bad(self, b, kind):
        e, rs, T, M = self.exp, self.rs, self.exp.T, self.exp.M
        sched = e.state["sched"][b]
        if kind in ("a", "b", "c+", "c-"):
            return {"a": -1, "b": T, "c+": INT_MAX, "c-": INT_MIN}[kind], int(rs.randint(M))
        if kind in ("d", "e"):
            a = self._valid(b)[0] if not sched.all() else int(rs.randint(T))
            return a, (-1 if kind == "d" else M)
        if kind == "f":
            a = int(rs.choice(np.flatnonzero(sched)))
        elif kind == "g":
            nsj = sched.reshape(e.J, M).sum(axis=1, dtype=np.int64)
            j = rs.choice(np.flatnonzero(nsj < M - 1))
            a = int(j * M + nsj[j] + 1)
        else:
            raise ValueError(kind)
        return a, int(rs.choice(np.flatnonzero(e.feas[b, a])))

    def draw(self):
        e, rs, B, s = self.exp, self.rs, self.exp.B, self.s
        done = e.finished()
        task, mach, kinds = np.zeros(B, np.int32), np.zeros(B, np.int32), [None] * B
        for b in range(B):
            if done[b]:
                sub = str(rs.choice(["a", "b", "c+", "c-", "d", "e", "f", "last"]))
                a, m = e.last_valid[b] if sub == "last" else self._bad(b, sub)
                kinds[b] = "h:" + sub
            else:
                if s == 0:
                    reject = True
                elif s == GROUP_STEP:
                    reject = b < self.group
                elif s == NOBODY_STEP:
                    reject = False
                else:
                    reject = rs.rand() < P_REJECT
                if reject:
                    kinds[b] = str(rs.choice(self._possible(b)))
                    a, m = self._bad(b, kinds[b])
                else:
                    a, m = self._valid(b)
            task[b], mach[b] = a, m
        self.s += 1
        if done.all():
            self.extra += 1
        return task, mach, kinds


def instances(J, M, E, B, seed):
    """the host-generated instances of a case, as tests/env_parity.py draws them"""
    from importlib import import_module
    import mtfjsp_amd  # noqa: F401
    inst = import_module("e2e-mappo-for-mt-fjsp_amd.instances")
    return inst.generate_instances(B, J, M, E, seed=1000 * seed + J * 100 + M)


def reward_weights(B, seed, episodes):
    """the reward weights of every reset of a case"""
    rs = np.random.RandomState(10_000 + seed)
    return [rs.dirichlet([1, 1, 1], B) for _ in range(episodes)]


class Census:
    """what the schedule did, counted from Expected.rejected (not from the kinds meant): kinds seen, launches, steps with a group
    holding both a rejected and a valid instance, and the three fixed steps"""

    def __init__(self, B, group):
        self.B, self.group = B, group
        self.kinds = {k: 0 for k in KINDS}
        self.launches = self.mixed_steps = 0
        self.fixed = {"all": False, "group": False, "nobody": False}
        self.finish_step = [None] * B

    def note(self, s, kinds, rej, finished_after):
        for b, k in enumerate(kinds):
            assert (k is not None) == bool(rej[b]), f"step {s} instance {b}: kind {k} but rejected = {rej[b]}"
            if k is not None:
                self.kinds["h" if k.startswith("h") else k] += 1
        g = self.group
        if g == 1:
            mixed = rej.any() and not rej.all()
        else:
            mixed = any(rej[i:i + g].any() and not rej[i:i + g].all() for i in range(0, self.B, g))
        self.mixed_steps += bool(mixed)
        if s == 0:
            self.fixed["all"] = bool(rej.all())
        if s == GROUP_STEP:
            self.fixed["group"] = bool(rej[:g].all() and not rej[g:].any())
        if s == NOBODY_STEP:
            self.fixed["nobody"] = not rej.any()
        for b in range(self.B):
            if finished_after[b] and self.finish_step[b] is None:
                self.finish_step[b] = s
        self.launches += 1


# ---------------------------------------------------------------------------------------------------------------------------------
# The table: every step kernel, forced through MTFJSP_ENV_KERNEL where the default dispatch would not reach it; every B ends in a
# partly filled group.  The GPU test runs every row with f32 and with f64 observations.
Case = namedtuple("Case", "family force J M E B kernel left_shift episodes seed")
SEED = 3


def _c(family, force, shape, B, kernel, left_shift=True, episodes=1, seed=SEED):
    return Case(family, force, *shape, B, kernel, left_shift, episodes, seed)


def _family(name, forces, shapes, B, noshift, second):
    """every (kernel, shape) of the family once, then its two variants on one row each: left_shift=False, and a second episode after
    scaler_reset_returns + reset over the dirty terminal state"""
    kern = dict(forces)
    rows = [_c(name, f, s, B, k) for f, k in forces for s in shapes]
    rows.append(_c(name, noshift[0], noshift[1], B, kern[noshift[0]], left_shift=False))
    rows.append(_c(name, second[0], second[1], B, kern[second[0]], episodes=2))
    return rows


J6M6, J8M8, J10M10, J3M11, J5M12, J13M10, J9M8 = (6, 6, 2), (8, 8, 2), (10, 10, 2), (3, 11, 1), (5, 12, 2), (13, 10, 2), (9, 8, 2)
CASES = (
    # one task slot per lane; J8M8: T = 64, every lane a task.  B = 19: one full group of 16 + 3, four full groups of 4 + 3
    _family("one_slot", [("grp16", "k_env_grp16"), ("grp4", "k_env_grp4"), ("reg1", "k_env_reg")], [J6M6, J8M8], 19,
            ("grp16", J8M8), ("grp4", J6M6))
    # two task slots per lane; J3M11 (T = 33): the second slot of every lane is empty
    + _family("two_slot", [("grp16", "k_env_grp16x2"), ("grp4", "k_env_grp4x2")], [J10M10, J3M11], 19, ("grp4", J3M11), ("grp16", J3M11))
    # the grouped LDS kernel forced on a register-kernel shape.  B = 11: one full group of 8 + 3
    + _family("lds_forced", [("lds", "k_env_step_grp")], [J6M6], 11, ("lds", J6M6), ("lds", J6M6))
    # the grouped LDS kernel by the default dispatch; J13M10: T = 130
    + _family("lds_default", [(None, "k_env_step_grp")], [J5M12, J13M10], 11, (None, J5M12), (None, J5M12))
    # one instance per workgroup
    + _family("lds1", [("lds1", "k_env_step")], [J6M6], 3, ("lds1", J6M6), ("lds1", J6M6))
)
FAMILIES = ("one_slot", "two_slot", "lds_forced", "lds_default", "lds1")
STEP_KERNELS = ("k_env_grp16", "k_env_grp4", "k_env_grp16x2", "k_env_grp4x2", "k_env_reg", "k_env_step_grp", "k_env_step")


def case_id(c):
    v = "noleftshift" if not c.left_shift else "plain" if c.episodes == 1 else "two_episodes"
    return f"{c.family}-{c.force or 'default'}-J{c.J}M{c.M}E{c.E}-B{c.B}-{v}"


def expected_side(c):
    """-> (Expected after scaler_init, the reward weights of the case's resets, the instances)"""
    t, p, tt, edge = instances(c.J, c.M, c.E, c.B, c.seed)
    exp = Expected(t, p, tt, edge, left_shift=c.left_shift)
    exp.scaler_init()
    return exp, reward_weights(c.B, c.seed, c.episodes), (t, p, tt, edge)


def begin_episode(exp, c, ep, w3):
    """the expected side's part of an episode's start (after the first: scaler_reset_returns, then the reset over the terminal
    state) -> the episode's Schedule"""
    if ep > 0:
        exp.scaler_reset_returns()
    exp.reset(w3[ep])
    return Schedule(exp, 100 * c.seed + ep, GROUP[c.kernel])

"""Priority-dispatch-rule baselines — the reference's `run_Rules_jointActions_withMinus_1217` (tester/pdrs.py:606-839) for all 12
rule pairs of test_all.py:484-540 (6 operation rules x 2 machine rules) and a whole instance set in ONE device rollout.

The reference runs rule by rule and instance by instance (~0.14 s per instance for MOR+SPT).  All 12 rules are
static — the order of the tasks and the machine of every task are fixed from t, p before the first step (pdrs:680-753) — so
`k_pdr_plan` (csrc/mtfjsp_pdr.hip) plans every instance's episode on the device from the handle's instance arrays, and the ordinary
step kernel replays the plans for all rule x instance pairs side by side, with left shift off as pdrs:669 has it.  The numbers
come back in the layout of `evaluate.validate_cost_batched`, so that policy and rules sit in one table.
"""
import ctypes as C

import numpy as np
import torch

from . import capi
from .batch_env import DeviceBatchEnv

M_RULE_NAMES = ["SPT", "SEC"]                                                        # pdrs:729
O_RULE_NAMES = ["FIFO", "MOR", "LWKR_T_o", "LWKR_PT_o", "MWKR_T_o", "MWKR_PT_o"]     # pdrs:730
# (name, o_rule, m_rule) in test_all.py's order: o_i outer, m_i inner
RULES = [(f"{O_RULE_NAMES[o]}+{M_RULE_NAMES[m]}", o, m) for o in range(6) for m in range(2)]
PLANS = "plans"          # key of pdr_baselines' result that holds {name: (task[N,T], mach[N,T])}; no rule is called that


def _rule_tensor(x, B, dev):
    if torch.is_tensor(x):
        assert x.is_cuda and x.dtype == torch.int32 and x.shape == (B,) and x.is_contiguous()
        return x
    a = np.asarray(x, np.int32)
    return torch.as_tensor(np.array(np.broadcast_to(a, (B,))), device=dev)                 # (a writable copy)


def pdr_plan(env, o_rule, m_rule, mor_order=None, seed=0):
    """Plan the whole episode of every instance of `env` under its dispatch rules (mtfjsp_pdr_plan; one launch).
    o_rule (0..5: FIFO, MOR, LWKR_T, LWKR_PT, MWKR_T, MWKR_PT), m_rule (0..1: SPT, SEC): an int for all instances, or [B] (host
    sequence or int32 device tensor).  mor_order [B,M,J] int32 (host or device): MOR's job order per column, used as is; None: drawn
    on the device (Philox keyed by (seed, instance, column)).  Reads t, p from the handle: works straight after
    `env.generate_instances`.  -> (task[B,T], mach[B,T]) int32 device tensors: the (task, machine) of step s."""
    B, T, dev = env.B, env.T, env.device
    o = _rule_tensor(o_rule, B, dev)
    m = _rule_tensor(m_rule, B, dev)
    mor = None
    if mor_order is not None:
        mor = mor_order if torch.is_tensor(mor_order) else torch.as_tensor(np.ascontiguousarray(mor_order, np.int32), device=dev)
        assert mor.is_cuda and mor.dtype == torch.int32 and mor.is_contiguous() and mor.shape == (B, env.M, env.J)
    task = torch.empty(B, T, dtype=torch.int32, device=dev)
    mach = torch.empty(B, T, dtype=torch.int32, device=dev)
    capi.check(env.L.mtfjsp_pdr_plan(env.h, o.data_ptr(), m.data_ptr(), C.c_void_p(mor.data_ptr() if mor is not None else None),
                                     int(seed), task.data_ptr(), mach.data_ptr()), env.h)
    return task, mach


def _rollout(env, w3, o_rule, m_rule, mor_order, seed):
    """reset with the config weights, plan, T steps -> (cumulative raw rewards [B,5], final costs [B,4], task, mach)"""
    T, dev = env.T, env.device
    env.reset(w3)                                                       # pdrs:675 reset(Random_weight_type="eval")
    task, mach = pdr_plan(env, o_rule, m_rule, mor_order, seed)
    ts, ms = task.t().contiguous(), mach.t().contiguous()               # [T,B]: row s = the actions of step s
    cum = torch.zeros(env.B, 5, dtype=torch.float64, device=dev)
    bad = torch.zeros(env.B, dtype=torch.int32, device=dev)
    for s in range(T):
        env.step(ts[s], ms[s])
        cum += env.raw                                                  # reward, r_mk, r_idle, r_pt, r_tt (pdrs:776-780), in step order
        bad |= env.status
    torch.cuda.synchronize(dev)
    n_bad = int((bad & (capi.ST_INVALID | capi.ST_INFEASIBLE)).ne(0).sum().item())
    if n_bad:
        raise RuntimeError(f"dispatch-rule rollout: {n_bad} instance(s) met an invalid action or an infeasible machine")
    if not bool(env.info[:, 1].all().item()):
        raise RuntimeError("dispatch-rule rollout: an episode did not finish after T steps")
    prev = env.read_state(capi.STATE_PREV_COSTS)                        # mk, e1, transT, idle of the finished schedule (pdrs:808-812)
    return cum.cpu().numpy(), prev, task.cpu().numpy(), mach.cpu().numpy()


def pdr_baselines(t, p, tt, edge, args, rules=RULES, mor_order=None, seed=0, device=0, env=None, obs_dtype="f32"):
    """The dispatch rules `rules` ((name, o_rule, m_rule) each; default: all 12) on the N instances t, p [N,T,M], tt [N,M,M],
    edge [N,E,M/E]; args: the reference's config dict (n_job, n_machine, n_edge, weight_mk, weight_ec, weight_tt).  One
    `DeviceBatchEnv(left_shift=False)` of len(rules)*N instances (block r = the N instances under rule r) and one T-step rollout.
    mor_order [N,M,J]: MOR's job order per column (every MOR block uses it); None: drawn on the device from `seed`.
    env: instead of t, p, tt, edge — a `DeviceBatchEnv(left_shift=False)` whose N instances are already loaded or generated
    on the device: the rules then run one after another on it (len(rules) rollouts of N), and no instance leaves the device.
    -> {name: (cost_dict_cumsum, Final_4cost, Objective)} with the per-instance arrays of `validate_cost_batched` (opr_Gt, opr_mk,
    opr_idleT, opr_pt, opr_transT; [N,4] makespan, e1 / T, transport, idle; pdrs:790-812 and test_all.py:536-538), and under
    PLANS ("plans") {name: (task[N,T], mach[N,T])}: what every rule dispatched."""
    J, M, E = int(args["n_job"]), int(args["n_machine"]), int(args["n_edge"])
    T, R = J * M, len(rules)
    w = (float(args["weight_mk"]), float(args["weight_ec"]), float(args["weight_tt"]))
    names = [r[0] for r in rules]
    if len(set(names)) != R or PLANS in names:
        raise ValueError("rule names must be distinct")
    if env is None:
        t = np.asarray(t, np.float64)
        N = t.shape[0]
        scal = args.get("reward_scaling", {}) or {}
        big = DeviceBatchEnv(J, M, E, R * N, left_shift=False, obs_dtype=obs_dtype, device=device, w_cfg=w,
                             scaling_divisor=float(scal.get("scaling_divisor", 1.0)))
        rep = lambda x: np.tile(np.asarray(x), (R,) + (1,) * (np.asarray(x).ndim - 1))      # noqa: E731
        big.load_instances(rep(t), rep(np.asarray(p, np.float64)), rep(np.asarray(tt, np.float64)), edge=rep(edge))
        big.scaler_init()                                               # the scaled components are produced but not used here
        w3 = torch.tensor([w], dtype=torch.float64, device=big.device).repeat(R * N, 1)
        o = np.repeat(np.array([r[1] for r in rules], np.int32), N)
        m = np.repeat(np.array([r[2] for r in rules], np.int32), N)
        mor = None
        if mor_order is not None:
            mor = mor_order.repeat(R, 1, 1).contiguous() if torch.is_tensor(mor_order) else np.tile(np.asarray(mor_order, np.int32), (R, 1, 1))
        try:
            cum, prev, task, mach = _rollout(big, w3, o, m, mor, seed)
        finally:
            big.close()
        parts = [(cum[r * N:(r + 1) * N], prev[r * N:(r + 1) * N], task[r * N:(r + 1) * N], mach[r * N:(r + 1) * N]) for r in range(R)]
    else:
        if (env.J, env.M) != (J, M):
            raise ValueError("env does not have the size args describes")
        if env.left_shift:
            raise ValueError("the dispatch rules run with left shift off (pdrs:669): create the env with left_shift=False")
        w3 = torch.tensor([w], dtype=torch.float64, device=env.device).repeat(env.B, 1)
        env.scaler_init()
        parts = [_rollout(env, w3, r[1], r[2], mor_order, seed) for r in rules]
    out, plans = {}, {}
    for name, (c, prev, task, mach) in zip(names, parts):
        cost = {"opr_Gt": c[:, 0], "opr_mk": c[:, 1], "opr_idleT": c[:, 2], "opr_pt": c[:, 3], "opr_transT": c[:, 4]}
        final4 = np.stack([prev[:, 0], prev[:, 1] / T, prev[:, 2], prev[:, 3]], 1)
        obj = w[0] * final4[:, 0] + w[1] * (final4[:, 1] + final4[:, 3]) + w[2] * final4[:, 2]
        out[name] = (cost, final4, obj)
        plans[name] = (task, mach)
    out[PLANS] = plans
    return out


# ---- one-step look-ahead rules (csrc/mtfjsp_lookahead.hip): the dynamic half of the table.  (name, column of the raw rewards whose
# one-step value decides: 2 idle time — the reference's LWKR_IT_o_jointActor, pdrs:465-540 —, 4 transport time, 1 makespan,
# 3 energy, 0 the scalar reward)
LOOKAHEAD_RULES = [("LA_IT", 2), ("LA_TT", 4), ("LA_MK", 1), ("LA_EC", 3), ("LA_R", 0)]


class Lookahead:
    """The scratch handle and buffers of one-step look-ahead decisions for `src` (a DeviceBatchEnv with loaded or generated
    instances): B*T copies, copy (b, j, m) tries job j's next task on machine m for instance b.  The constants are forked once,
    here; `decide(column)` is expand, one ordinary step of the scratch handle and the selection — five launches, no read-back."""

    def __init__(self, src):
        self.src, B, T, dev = src, src.B, src.T, src.device
        self.scratch = DeviceBatchEnv(src.J, src.M, src.E, B * T, left_shift=src.left_shift, obs_dtype="f32" if src.obs_f32 else "f64",
                                      device=dev.index or 0, gamma=src.gamma, w_cfg=src.w_cfg, scaling_divisor=src.scaling_divisor)
        self.scratch.fork_from(src, torch.arange(B * T, dtype=torch.int32, device=dev) // T, instance=True, state=False, obs=False)
        self.task_c = torch.empty(B * T, dtype=torch.int32, device=dev)
        self.mach_c = torch.empty(B * T, dtype=torch.int32, device=dev)
        self.task = torch.empty(B, dtype=torch.int32, device=dev)
        self.mach = torch.empty(B, dtype=torch.int32, device=dev)
        self.job = torch.empty(B, dtype=torch.int32, device=dev)
        self.best = torch.empty(B, dtype=torch.float64, device=dev)

    def expand(self):
        capi.check(self.src.L.mtfjsp_lookahead_expand(self.scratch.h, self.src.h, self.task_c.data_ptr(), self.mach_c.data_ptr()), self.scratch.h)

    def select(self, column):
        capi.check(self.src.L.mtfjsp_lookahead_select(self.scratch.h, self.src.h, int(column), self.task.data_ptr(), self.mach.data_ptr(),
                                                      self.job.data_ptr(), self.best.data_ptr()), self.scratch.h)

    def decide(self, column):
        """-> (task, mach) [B] int32 device tensors (overwritten by the next decision): the action whose one-step raw[column] is
        largest, ties to the lowest (job, machine); task -1 for a finished instance.  `self.best`: the winning values."""
        self.expand()
        self.scratch.step(self.task_c, self.mach_c)
        self.select(column)
        return self.task, self.mach

    def close(self):
        self.scratch.close()


def lookahead_baselines(t, p, tt, edge, args, rules=LOOKAHEAD_RULES, device=0, obs_dtype="f32", left_shift=False):
    """One-step look-ahead dispatch rules `rules` ((name, column) each) on the N instances t, p [N,T,M], tt [N,M,M],
    edge [N,E,M/E]; args as for `pdr_baselines`.  Per rule and step: fork the N instances into N*T copies, step every copy with its
    (job, machine), take per instance the copy with the largest raw[column] (the least added cost; ties: lowest (job, machine)),
    step the instance with it.  Unlike the reference's idle-time rule (pdrs:465-540) the tie is not drawn at random (pdrs:520) and
    the machine is not fixed beforehand by a machine rule: job and machine are chosen jointly.
    -> {name: (cost_dict_cumsum, Final_4cost, Objective)} in `pdr_baselines`' layout, and under PLANS {name: (task[N,T], mach[N,T])}."""
    J, M, E = int(args["n_job"]), int(args["n_machine"]), int(args["n_edge"])
    T = J * M
    w = (float(args["weight_mk"]), float(args["weight_ec"]), float(args["weight_tt"]))
    names = [r[0] for r in rules]
    if len(set(names)) != len(rules) or PLANS in names:
        raise ValueError("rule names must be distinct")
    if any(int(r[1]) not in range(5) for r in rules):
        raise ValueError("a look-ahead rule's column must be 0..4")
    t = np.asarray(t, np.float64)
    N = t.shape[0]
    scal = args.get("reward_scaling", {}) or {}
    env = DeviceBatchEnv(J, M, E, N, left_shift=left_shift, obs_dtype=obs_dtype, device=device, w_cfg=w,
                         scaling_divisor=float(scal.get("scaling_divisor", 1.0)))
    la = None
    out, plans = {}, {}
    try:
        env.load_instances(t, np.asarray(p, np.float64), np.asarray(tt, np.float64), edge=edge)
        la = Lookahead(env)
        dev = env.device
        w3 = torch.tensor([w], dtype=torch.float64, device=dev).repeat(N, 1)
        for name, column in rules:
            env.scaler_init()                                           # the scaled components are produced but not used here
            env.reset(w3)                                               # pdrs:675 reset(Random_weight_type="eval")
            task = torch.empty(T, N, dtype=torch.int32, device=dev)
            mach = torch.empty(T, N, dtype=torch.int32, device=dev)
            cum = torch.zeros(N, 5, dtype=torch.float64, device=dev)
            bad = torch.zeros(N, dtype=torch.int32, device=dev)
            for s in range(T):
                a, m = la.decide(column)
                task[s].copy_(a); mach[s].copy_(m)
                env.step(a, m)
                cum += env.raw                                          # reward, r_mk, r_idle, r_pt, r_tt, in step order
                bad |= env.status
            torch.cuda.synchronize(dev)
            n_bad = int((bad & (capi.ST_INVALID | capi.ST_INFEASIBLE)).ne(0).sum().item())
            if n_bad:
                raise RuntimeError(f"look-ahead rollout: {n_bad} instance(s) met an invalid action or an infeasible machine")
            if not bool(env.info[:, 1].all().item()):
                raise RuntimeError("look-ahead rollout: an episode did not finish after T steps")
            prev = env.read_state(capi.STATE_PREV_COSTS)
            c = cum.cpu().numpy()
            cost = {"opr_Gt": c[:, 0], "opr_mk": c[:, 1], "opr_idleT": c[:, 2], "opr_pt": c[:, 3], "opr_transT": c[:, 4]}
            final4 = np.stack([prev[:, 0], prev[:, 1] / T, prev[:, 2], prev[:, 3]], 1)
            obj = w[0] * final4[:, 0] + w[1] * (final4[:, 1] + final4[:, 3]) + w[2] * final4[:, 2]
            out[name] = (cost, final4, obj)
            plans[name] = (task.t().contiguous().cpu().numpy(), mach.t().contiguous().cpu().numpy())
    finally:
        if la is not None:
            la.close()
        env.close()
    out[PLANS] = plans
    return out

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
from .evaluate import COST_KEYS, CopyGroups, best_of_k_rollout, episode_results, config_w3, eval_reset, parse_args, replay_episode

M_RULE_NAMES = ["SPT", "SEC"]                                                        # pdrs:729
O_RULE_NAMES = ["FIFO", "MOR", "LWKR_T_o", "LWKR_PT_o", "MWKR_T_o", "MWKR_PT_o"]     # pdrs:730
# (name, o_rule, m_rule) in test_all.py's order: o_i outer, m_i inner
RULES = [(f"{O_RULE_NAMES[o]}+{M_RULE_NAMES[m]}", o, m) for o in range(6) for m in range(2)]
PLANS = "plans"          # key of pdr_baselines' result that holds {name: (task[N,T], mach[N,T])}; no rule is called that


def _rule_names(rules, kind=None):
    """the names of `rules` ((name, ...) each), checked; kind ("look-ahead", "beam"): element 1 is a column of the raw rewards"""
    names = [r[0] for r in rules]
    if len(set(names)) != len(rules) or PLANS in names:
        raise ValueError("rule names must be distinct")
    if kind and any(int(r[1]) not in range(5) for r in rules):
        raise ValueError(f"a {kind} rule's column must be 0..4")
    return names


def _results(names, parts, T, w):
    """{name: (cum, prev, task, mach)} host arrays per rule -> the *_baselines' result dict"""
    out = {name: episode_results(parts[name][0], parts[name][1], T, w) for name in names}
    out[PLANS] = {name: parts[name][2:] for name in names}
    return out


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
    env.reset(w3)                                                       # pdrs:675 reset(Random_weight_type="eval")
    task, mach = pdr_plan(env, o_rule, m_rule, mor_order, seed)
    ts, ms = task.t().contiguous(), mach.t().contiguous()               # [T,B]: row s = the actions of step s
    cum, prev = replay_episode(env, env.T, lambda s: (ts[s], ms[s]), "dispatch-rule")
    return cum, prev, task.cpu().numpy(), mach.cpu().numpy()


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
    J, M, E, T, w, kw = parse_args(args, left_shift=False, obs_dtype=obs_dtype, device=device)
    R, names = len(rules), _rule_names(rules)
    if env is None:
        t = np.asarray(t, np.float64)
        N = t.shape[0]
        big = DeviceBatchEnv(J, M, E, R * N, **kw)
        rep = lambda x: np.tile(np.asarray(x), (R,) + (1,) * (np.asarray(x).ndim - 1))      # noqa: E731
        big.load_instances(rep(t), rep(np.asarray(p, np.float64)), rep(np.asarray(tt, np.float64)), edge=rep(edge))
        big.scaler_init()                                               # the scaled components are produced but not used here
        w3 = config_w3(big, w)
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
        w3 = config_w3(env, w)
        env.scaler_init()
        parts = [_rollout(env, w3, r[1], r[2], mor_order, seed) for r in rules]
    return _results(names, dict(zip(names, parts)), T, w)


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
        self.scratch = DeviceBatchEnv.like(src, B * T)
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
    J, M, E, T, w, kw = parse_args(args, left_shift=left_shift, obs_dtype=obs_dtype, device=device)
    names = _rule_names(rules, "look-ahead")
    t = np.asarray(t, np.float64)
    N = t.shape[0]
    env = DeviceBatchEnv(J, M, E, N, **kw)
    la = None
    parts = {}
    try:
        env.load_instances(t, np.asarray(p, np.float64), np.asarray(tt, np.float64), edge=edge)
        la = Lookahead(env)
        dev = env.device
        w3 = config_w3(env, w)
        for name, column in rules:
            eval_reset(env, w3)
            task = torch.empty(T, N, dtype=torch.int32, device=dev)
            mach = torch.empty(T, N, dtype=torch.int32, device=dev)

            def decide(s):                                              # the choice of step s, recorded
                a, m = la.decide(column)
                task[s].copy_(a); mach[s].copy_(m)
                return a, m
            cum, prev = replay_episode(env, T, decide, "look-ahead")
            parts[name] = (cum, prev, task.t().contiguous().cpu().numpy(), mach.t().contiguous().cpu().numpy())
    finally:
        if la is not None:
            la.close()
        env.close()
    return _results(names, parts, T, w)


# ---- beam search (csrc/mtfjsp_beam.hip): the look-ahead's children, the W best of them kept per instance instead of one.  (name,
# column of the raw rewards whose running sum is the score: as LOOKAHEAD_RULES)
BEAM_RULES = [("BS_IT", 2), ("BS_TT", 4), ("BS_MK", 1), ("BS_EC", 3), ("BS_R", 0)]
BEAM_MAX_WIDTH, BEAM_MAX_CANDIDATES = 64, 8192
BEAM_SCRATCH_BATCH = 262144          # the chip-filling batch: what one pass of beam_baselines keeps in flight


def _backtrack(beam, N, W, s, hist, start_slot):
    """mtfjsp_beam_backtrack over the first s rows of `hist` (from_slot, task, mach: [cap, N*W] each) from slot start_slot[n] (None:
    slot 0) of the beam handle `beam` -> (task[N,s], mach[N,s]) int32 device tensors"""
    if s < 1:
        raise ValueError("no decision has been taken yet")
    dev = beam.device
    if start_slot is not None and not torch.is_tensor(start_slot):
        start_slot = torch.as_tensor(np.ascontiguousarray(start_slot, np.int32), device=dev)
    if start_slot is not None:
        assert start_slot.is_cuda and start_slot.dtype == torch.int32 and start_slot.is_contiguous() and start_slot.shape == (N,)
    task = torch.empty(N, s, dtype=torch.int32, device=dev)
    mach = torch.empty(N, s, dtype=torch.int32, device=dev)
    capi.check(beam.L.mtfjsp_beam_backtrack(beam.h, W, s, hist["from_slot"].data_ptr(), hist["task"].data_ptr(), hist["mach"].data_ptr(),
                                            C.c_void_p(start_slot.data_ptr() if start_slot is not None else None),
                                            task.data_ptr(), mach.data_ptr()), beam.h)
    return task, mach


class BeamSearch:
    """Beam search of width `width` from the states `src` (a reset DeviceBatchEnv of N instances) holds now: a beam handle of N*W
    instances (slot w of instance n = n*W + w) and a scratch handle of N*W*T (child (j, m) of every slot).  Constants and state are
    forked from `src` once, here (and again by `restart`); the scores start as [0, -inf, ...] per instance: one live slot.
    `advance(column)` is one decision — expand, one ordinary step of the scratch handle, the children's signatures (with `dedupe`:
    children that are the same partial schedule reached in another order are merged into the best of them), the selection of the
    W best children by score + raw[column] into row s of the history, and the fork of the winners into the beam — six launches,
    no read-back.  `run` drives whole episodes and reads the best plan out through the back-pointers."""

    def __init__(self, src, width, dedupe=True):
        W = int(width)
        if not 1 <= W <= BEAM_MAX_WIDTH or W * src.T > BEAM_MAX_CANDIDATES:
            raise ValueError(f"beam width must be 1..{BEAM_MAX_WIDTH} with width * n_job * n_machine <= {BEAM_MAX_CANDIDATES}")
        self.src, self.W, self.dedupe = src, W, bool(dedupe)
        N, T, dev = src.B, src.T, src.device
        self.N, self.T = N, T
        self.beam = DeviceBatchEnv.like(src, N * W)
        self.scratch = DeviceBatchEnv.like(src, N * W * T)
        self._beam_index = torch.arange(N * W, dtype=torch.int32, device=dev) // W
        self.scratch.fork_from(src, torch.arange(N * W * T, dtype=torch.int32, device=dev) // (W * T), instance=True, state=False, obs=False)
        self.task_c = torch.empty(N * W * T, dtype=torch.int32, device=dev)
        self.mach_c = torch.empty(N * W * T, dtype=torch.int32, device=dev)
        self.sig = torch.zeros(N * W * T, dtype=torch.int64, device=dev)        # (the 64-bit signatures, as int64 words)
        self.score = torch.empty(N * W, dtype=torch.float64, device=dev)
        self._score_next = torch.empty_like(self.score)
        self._alloc_history(T)
        self.restart()

    def _alloc_history(self, cap):
        dev, NW = self.src.device, self.N * self.W
        old = getattr(self, "hist", None)
        # rows of (parent, from_slot, task, mach): row s = what decision s's selection wrote
        self.hist = {k: torch.full((cap, NW), -1, dtype=torch.int32, device=dev) for k in ("parent", "from_slot", "task", "mach")}
        if old is not None:
            for k, v in old.items():
                self.hist[k][:v.shape[0]].copy_(v)

    def restart(self):
        """take `src`'s present state again: every slot a copy of its instance, one live slot, no history"""
        self.beam.fork_from(self.src, self._beam_index, instance=True, state=True, obs=False)
        self.score.fill_(float("-inf"))
        self.score.view(self.N, self.W)[:, 0] = 0.0
        self.s = 0

    def advance(self, column):
        """one decision of every instance; -> the step's history row index.  `self.score` [N*W] then holds the new scores."""
        L, s = self.src.L, self.s
        if s >= self.hist["task"].shape[0]:
            self._alloc_history(2 * s)
        capi.check(L.mtfjsp_lookahead_expand(self.scratch.h, self.beam.h, self.task_c.data_ptr(), self.mach_c.data_ptr()), self.scratch.h)
        self.scratch.step(self.task_c, self.mach_c)
        if self.dedupe:
            self.scratch.state_signature(self.sig)
        h = self.hist
        capi.check(L.mtfjsp_beam_select(self.scratch.h, self.beam.h, self.W, int(column), self.score.data_ptr(),
                                        C.c_void_p(self.sig.data_ptr() if self.dedupe else None), h["parent"][s].data_ptr(),
                                        h["from_slot"][s].data_ptr(), h["task"][s].data_ptr(), h["mach"][s].data_ptr(),
                                        self._score_next.data_ptr()), self.scratch.h)
        self.beam.fork_from(self.scratch, h["parent"][s], instance=False, state=True, obs=False)
        self.score, self._score_next = self._score_next, self.score
        self.s = s + 1
        return s

    def plans(self, start_slot=None):
        """-> (task[N,s], mach[N,s]) int32 device tensors: the decisions that led to slot start_slot[n] (host sequence or int32
        device tensor [N]; None: slot 0, the best) of the present beam, -1 where the slot is empty or the instance had finished"""
        return _backtrack(self.beam, self.N, self.W, self.s, self.hist, start_slot)

    def run(self, column, steps=None):
        """`steps` (default T: the whole episode) decisions -> (task[N,steps], mach[N,steps], score[N,W]): the best slot's plan and
        every slot's score (the running sum of raw[column]; -inf: empty)"""
        for _ in range(self.T if steps is None else int(steps)):
            self.advance(column)
        task, mach = self.plans()
        return task, mach, self.score.view(self.N, self.W)

    def close(self):
        self.scratch.close()
        self.beam.close()


def beam_baselines(t, p, tt, edge, args, rules=BEAM_RULES, width=8, dedupe=True, device=0, obs_dtype="f32", left_shift=False, chunk=None):
    """Beam search `rules` ((name, column) each) of width `width` on the N instances t, p [N,T,M], tt [N,M,M], edge [N,E,M/E]; args
    as for `pdr_baselines`.  Per rule: a `BeamSearch` over the whole episode (score = the running sum of raw[column]; ties to the
    lowest (slot, job, machine); with `dedupe`, children that are one partial schedule are merged), then the best plan is replayed on the plain handle step by
    step, as `lookahead_baselines` steps its choices.  chunk: source instances per pass (None: the largest with
    chunk * width * T <= BEAM_SCRATCH_BATCH); the results do not depend on it.
    -> {name: (cost_dict_cumsum, Final_4cost, Objective)} in `pdr_baselines`' layout, and under PLANS {name: (task[N,T], mach[N,T])}."""
    J, M, E, T, w, kw = parse_args(args, left_shift=left_shift, obs_dtype=obs_dtype, device=device)
    W, names = int(width), _rule_names(rules, "beam")
    t, p, tt, edge = np.asarray(t, np.float64), np.asarray(p, np.float64), np.asarray(tt, np.float64), np.asarray(edge)
    N = t.shape[0]
    chunk = max(1, BEAM_SCRATCH_BATCH // (W * T)) if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be at least 1")
    parts = {name: [] for name in names}
    for lo in range(0, N, chunk):
        hi = min(N, lo + chunk)
        n = hi - lo
        env = DeviceBatchEnv(J, M, E, n, **kw)
        bs = None
        try:
            env.load_instances(t[lo:hi], p[lo:hi], tt[lo:hi], edge=edge[lo:hi])
            w3 = config_w3(env, w)
            for name, column in rules:
                eval_reset(env, w3)
                if bs is None:
                    bs = BeamSearch(env, W, dedupe)
                else:
                    bs.restart()
                task, mach, _ = bs.run(int(column), T)
                ts, ms = task.t().contiguous(), mach.t().contiguous()   # [T,n]: row s = the actions of step s
                cum, prev = replay_episode(env, T, lambda s: (ts[s], ms[s]), "beam-search")
                parts[name].append((cum, prev, task.cpu().numpy(), mach.cpu().numpy()))
        finally:
            if bs is not None:
                bs.close()
            env.close()
    return _results(names, {name: tuple(np.concatenate([x[k] for x in parts[name]]) for k in range(4)) for name in names}, T, w)


# ---- policy-guided beam search (csrc/mtfjsp_policy_beam.hip): the beam's slots, scored by the actors' joint log-probability
PB_TOP, PB_BEST = "PB_TOP", "PB_BEST"
POLICY_BEAM_BATCH = 65536            # (slot, job) rows of the machine forward that one pass of policy_beam keeps in flight
_PB_HIST = ("parent", "from_slot", "job", "task", "mach", "child")


class PolicyBeamSearch:
    """Beam decoding of the trained actors from the states `src` (a reset DeviceBatchEnv of N instances) holds now: the W most
    probable partial schedules per instance, a slot's score being the running sum of log p(job) + log p(machine | job).  Two beam
    handles of N*W instances (slot w of instance n = n*W + w) take turns, both forked from `src` with constants, state and
    observation here (and again by `restart`), so every slot always holds some valid state; an `Encoder` of batch N*W runs the job
    forwards and one of batch N*W*J the machine forwards, both with per-instance BatchNorm (a slot's forward does not depend on its
    neighbours).  weights: (job actor, machine actor) state dicts.  The scores start as [0, -inf, ...] per instance.
    `advance()` is one decision: the job forward on the current beam (with the embedding every slot carries from the machine
    forward of its last decision; none at decision 0), m_fea1 of every job's candidate task, ONE machine forward over all (slot,
    job) rows, the two logarithms (torch.log of the binary64 probabilities), the selection of the W best (slot, job, machine) into
    row s of the history, the fork of the winners' slots into the other handle, its step with the chosen actions, the carried
    embedding and — with `dedupe` — the merge of slots that hold one partial schedule (the later, less probable one is emptied
    and refilled by the next selection).  Only the W kept children are stepped.  Nothing is read back; everything runs on the
    stream that was current at construction.  A rank without a candidate has parent -1 (the fork leaves its slot untouched) and
    task -1 (the step rejects it).  A forward that reports capi.ERR_RETRY raises MtfjspError: there is no retry loop.
    on_decision(s, tensors) (tests): called at the end of decision s with that decision's device tensors — inputs, probabilities,
    logarithms, outputs, signatures; they are overwritten by the next decision."""

    def __init__(self, src, weights, width, dedupe=True, on_decision=None):
        from .encoder import Encoder
        W = int(width)
        if not 1 <= W <= BEAM_MAX_WIDTH or W * src.T > BEAM_MAX_CANDIDATES:
            raise ValueError(f"beam width must be 1..{BEAM_MAX_WIDTH} with width * n_job * n_machine <= {BEAM_MAX_CANDIDATES}")
        self.src, self.W, self.dedupe, self.on_decision = src, W, bool(dedupe), on_decision
        N, T, J, M, dev = src.B, src.T, src.J, src.M, src.device
        self.N, self.T = N, T
        NW = N * W
        obs = "f32" if src.obs_f32 else "f64"
        self.cur = self.nxt = self.enc_job = self.enc_mach = None
        try:
            self.cur, self.nxt = DeviceBatchEnv.like(src, NW), DeviceBatchEnv.like(src, NW)
            self.enc_job = Encoder(J, M, NW, device=dev.index or 0, obs_dtype=obs)
            self.enc_mach = Encoder(J, M, NW * J, device=dev.index or 0, obs_dtype=obs)
            for e in (self.enc_job, self.enc_mach):
                e.load_weights(weights[0], weights[1])
                e.set_bn_mode(True)
        except Exception:
            self.close()
            raise
        self._beam_index = torch.arange(NW, dtype=torch.int32, device=dev) // W
        self._job_rows = torch.arange(NW * J, dtype=torch.int64, device=dev) // J         # (slot, job) row -> slot
        odt = torch.float32 if src.obs_f32 else torch.float64
        self.m_fea1 = torch.empty(NW, J, M, 6, dtype=odt, device=dev)
        self.mmask = torch.empty(NW, J, M, dtype=torch.uint8, device=dev)
        self.sig = torch.zeros(NW, dtype=torch.int64, device=dev)
        self.score = torch.empty(NW, dtype=torch.float64, device=dev)
        self._score_next = torch.empty_like(self.score)
        self.hist = {k: torch.full((T, NW), -1, dtype=torch.int32, device=dev) for k in _PB_HIST}
        self.restart()

    def restart(self):
        """take `src`'s present state again: every slot of both handles a copy of its instance, one live slot, no history"""
        for e in (self.cur, self.nxt):
            e.fork_from(self.src, self._beam_index, instance=True, state=True, obs=True)
        self.score.fill_(float("-inf"))
        self.score.view(self.N, self.W)[:, 0] = 0.0
        self.h_m = None                                                 # the embedding every slot carries ([N*W,128] f32)
        self.s = 0

    def advance(self):
        """one decision of every instance; -> the decision's history row index.  `self.score` [N*W] then holds the new scores and
        `self.cur` the new beam."""
        s, cur, nxt, W, J = self.s, self.cur, self.nxt, self.W, self.src.J
        if s >= self.hist["task"].shape[0]:
            old = self.hist
            self.hist = {k: torch.full((2 * s, v.shape[1]), -1, dtype=torch.int32, device=v.device) for k, v in old.items()}
            for k, v in old.items():
                self.hist[k][:s].copy_(v)
        ej, em = self.enc_job, self.enc_mach
        job_prob, h_o, _ = ej.job_actor_forward(cur.tasks_fea, cur.ell_col, cur.ell_val, cur.candidate, cur.job_mask, self.h_m)
        cur.observe_mfea1_jobs(self.m_fea1, self.mmask)
        m_fea2 = cur.m_fea2.index_select(0, self._job_rows)            # [N*W*J,M,8]: a slot's machines, once per job
        h_o_rows = h_o.index_select(0, self._job_rows)                 # [N*W*J,128]
        mch_prob, h_mach, _ = em.machine_actor_forward(self.m_fea1, m_fea2, h_o_rows, self.mmask)
        logp_job, logp_mach = torch.log(job_prob.double()), torch.log(mch_prob.double())
        h = {k: v[s] for k, v in self.hist.items()}
        capi.check(cur.L.mtfjsp_beam_select_policy(cur.h, W, self.score.data_ptr(), logp_job.data_ptr(), logp_mach.data_ptr(), self.mmask.data_ptr(),
                                                   *[h[k].data_ptr() for k in _PB_HIST], self._score_next.data_ptr()), cur.h)
        nxt.fork_from(cur, h["parent"], instance=False, state=True, obs=True)
        nxt.step(h["task"], h["mach"])
        h_m_prev, self.h_m = self.h_m, h_mach.index_select(0, h["child"].clamp(min=0).long())
        selected = self._score_next.clone() if self.on_decision is not None else None
        if self.dedupe:
            nxt.state_signature(self.sig)
            capi.check(cur.L.mtfjsp_beam_merge_slots(nxt.h, W, self.sig.data_ptr(), self._score_next.data_ptr()), nxt.h)
        if self.on_decision is not None:
            self.on_decision(s, dict(
                beam=cur, next=nxt, candidate=cur.candidate, job_mask=cur.job_mask, h_m_prev=h_m_prev, job_prob=job_prob, h_o=h_o,
                m_fea1=self.m_fea1, mmask=self.mmask, m_fea2=cur.m_fea2, m_fea2_rows=m_fea2, h_o_rows=h_o_rows, mch_prob=mch_prob,
                h_mach=h_mach, logp_job=logp_job, logp_mach=logp_mach, score_in=self.score, score_selected=selected,
                score_out=self._score_next, sig=self.sig if self.dedupe else None, h_m=self.h_m, **h))
        self.score, self._score_next = self._score_next, self.score
        self.cur, self.nxt = nxt, cur
        self.s = s + 1
        return s

    def plans(self, start_slot=None):
        """-> (task[N,s], mach[N,s]) int32 device tensors: the decisions that led to slot start_slot[n] (host sequence or int32
        device tensor [N]; None: slot 0, the most probable) of the present beam, -1 where the slot is empty"""
        return _backtrack(self.cur, self.N, self.W, self.s, self.hist, start_slot)

    def run(self, steps=None):
        """`steps` (default T: the whole episode) decisions -> (task[N,steps], mach[N,steps], score[N,W]): the most probable slot's
        plan and every slot's joint log-probability (-inf: empty)"""
        for _ in range(self.T if steps is None else int(steps)):
            self.advance()
        task, mach = self.plans()
        return task, mach, self.score.view(self.N, self.W)

    def close(self):
        for e in (self.enc_job, self.enc_mach):
            if e is not None:
                e.set_bn_mode(False)
                e.close()
        for e in (self.cur, self.nxt):
            if e is not None:
                e.close()
        self.cur = self.nxt = self.enc_job = self.enc_mach = None


def policy_beam(weights, t, p, tt, edge, args, width=8, dedupe=True, chunk=None, device=0, obs_dtype="f32", left_shift=True, on_decision=None):
    """Beam decoding of the policy `weights` ((job actor, machine actor) state dicts, as for `evaluate.validate_cost_batched`) on the
    N instances t, p [N,T,M], tt [N,M,M], edge [N,E,M/E]; args as for `pdr_baselines`; left shift on, as the policy's evaluations
    have it.  Per pass a `PolicyBeamSearch` of width `width` runs the T decisions of the episode; then `final_costs` of the last
    beam and `group_reduce(n, W)` over its live slots give every instance's finished slot with the smallest Objective.  Two plans
    per instance are read out through the back-pointers and replayed on the plain handle step by step, as `beam_baselines` replays
    its plan: PB_TOP, slot 0 — the most probable finished schedule the beam holds —, and PB_BEST, the cheapest one (lowest slot on
    ties).  width = 1 is the joint arg-max of p(job) * p(machine | job) at every decision, which is not the sequential greedy of
    `validate_cost_batched` (the most probable job first, then its most probable machine).
    chunk: bounds (source instances per pass) * width * n_job, the rows of the machine forward (None: POLICY_BEAM_BATCH).  The
    results are NOT promised to be bit-independent of chunk: which kernels the forwards run follows their batch.
    on_decision(s, tensors): handed to every pass's `PolicyBeamSearch` (tests).
    -> {"PB_TOP", "PB_BEST": (cost_dict_cumsum, Final_4cost, Objective)} in `pdr_baselines`' layout, under PLANS both plans
    {name: (task[N,T], mach[N,T])}, and "logp" [N,W]: every final slot's joint log-probability (descending; -inf: empty or merged)."""
    J, M, E, T, w, kw = parse_args(args, left_shift=left_shift, obs_dtype=obs_dtype, device=device)
    W = int(width)
    t, p, tt, edge = np.asarray(t, np.float64), np.asarray(p, np.float64), np.asarray(tt, np.float64), np.asarray(edge)
    N = t.shape[0]
    chunk = POLICY_BEAM_BATCH if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be at least 1")
    per_pass = max(1, chunk // (W * J))
    names = [PB_TOP, PB_BEST]
    parts, logp = {name: [] for name in names}, []
    for lo in range(0, N, per_pass):
        hi = min(N, lo + per_pass)
        n = hi - lo
        env = DeviceBatchEnv(J, M, E, n, **kw)
        pb = None
        try:
            env.load_instances(t[lo:hi], p[lo:hi], tt[lo:hi], edge=edge[lo:hi])
            w3 = config_w3(env, w)
            eval_reset(env, w3)
            pb = PolicyBeamSearch(env, weights, W, dedupe, on_decision=on_decision)
            top_t, top_m, score = pb.run(T)
            cost4, done = pb.cur.final_costs()
            done &= (score.reshape(-1) != float("-inf")).to(torch.uint8)            # an emptied slot is nobody's best
            _, best, _, _ = env.group_reduce(n, W, cost4, done, w, obj=False, best_obj=False, front=False)
            if int(best.min().item()) < 0:
                raise RuntimeError("policy-beam search: an instance has no finished slot")
            best_t, best_m = pb.plans(best - torch.arange(n, dtype=torch.int32, device=env.device) * W)
            logp.append(score.cpu().numpy().copy())
            for name, (task, mach) in ((PB_TOP, (top_t, top_m)), (PB_BEST, (best_t, best_m))):
                eval_reset(env, w3)
                ts, ms = task.t().contiguous(), mach.t().contiguous()   # [T,n]: row s = the actions of step s
                cum, prev = replay_episode(env, T, lambda s: (ts[s], ms[s]), "policy-beam")
                parts[name].append((cum, prev, task.cpu().numpy(), mach.cpu().numpy()))
        finally:
            if pb is not None:
                pb.close()
            env.close()
    out = _results(names, {name: tuple(np.concatenate([x[k] for x in parts[name]]) for k in range(4)) for name in names}, T, w)
    out["logp"] = np.concatenate(logp)
    return out


# ---- the random dispatch rule as best-of-K (csrc/mtfjsp_group.hip): K uniformly random episodes per instance, the best kept
RANDOM_BEST, RANDOM_MEAN = "RANDOM_BEST", "RANDOM_MEAN"


class _RandomPolicy:
    """`evaluate.best_of_k_rollout`'s policy without an encoder: `env.random_actions` (a uniform unmasked job, a uniform feasible
    machine; Philox keyed by (seed, step, index of the copy inside the handle))"""

    def __init__(self, seed):
        self.seed = int(seed)

    def open(self, batch):
        pass

    def begin(self):
        pass

    def decide(self, env, s, task_row, mach_row, job):
        env.random_actions(self.seed, s, task_row, mach_row, job)

    def close(self):
        pass


def random_baselines(t, p, tt, edge, args, K=1, seed=0, device=0, obs_dtype="f32", left_shift=False, chunk=None):
    """The random dispatch rule on the N instances t, p [N,T,M], tt [N,M,M], edge [N,E,M/E] (args as for `pdr_baselines`): K random
    episodes per instance side by side — the K-copy handle, final costs, best copy and fork of `evaluate.sample_best_of_k`, with the
    actions of `DeviceBatchEnv.random_actions(seed, step)` in place of the actors.  The stream is keyed by a copy's index inside
    the handle: the results are a function of (seed, K, chunk), chunk = instances per pass (None: all N).
    -> {"RANDOM_BEST": (cost_dict_cumsum, Final_4cost, Objective) of every instance's best episode (smallest Objective, lowest copy
    on ties), "RANDOM_MEAN": the same three as means over the K episodes (taken on the host)} in `pdr_baselines`' layout, and under
    PLANS {"RANDOM_BEST": (task[N,T], mach[N,T])}."""
    r = best_of_k_rollout(t, p, tt, edge, args, K, _RandomPolicy(seed), chunk=chunk, device=device, obs_dtype=obs_dtype, left_shift=left_shift,
                          what="random-rule")
    mean_cost = {key: r["cum"][:, :, i].mean(axis=1) for i, key in enumerate(COST_KEYS)}
    return {RANDOM_BEST: r["best"], RANDOM_MEAN: (mean_cost, r["final4"].mean(axis=1), r["obj"].mean(axis=1)),
            PLANS: {RANDOM_BEST: r["plans"]}}


# ---- local search on plans (csrc/mtfjsp_plan.hip): K neighbours of every instance's incumbent per round, replayed side by side
MOVE_SWAP, MOVE_INSERT, MOVE_REASSIGN = 1, 2, 4          # bits of `moves`; what "accepted" holds
ALL_MOVES = MOVE_SWAP | MOVE_INSERT | MOVE_REASSIGN
MOVE_CRIT_SWAP, MOVE_CRIT_REASSIGN = 8, 16               # moves a critical path of the incumbent's schedule directs
CRIT_MOVES = MOVE_CRIT_SWAP | MOVE_CRIT_REASSIGN


MOVE_NAMES = ("MOVE_SWAP", "MOVE_INSERT", "MOVE_REASSIGN", "MOVE_CRIT_SWAP", "MOVE_CRIT_REASSIGN")                  # bit i = MOVE_NAMES[i]
# what a plan search returns beside (name, PLANS): (key, dtype, rows) — rows None: per instance [N]; else per round [rounds + rows, N]
EVOLVE_RESULT = (("start_obj", np.float64, None), ("history", np.float64, 0))
LOCAL_RESULT = EVOLVE_RESULT + (("accepted", np.int8, 0),)
WALK_RESULT = EVOLVE_RESULT + (("current", np.float64, 0), ("accepted", np.int8, 0), ("why", np.int8, 0), ("barred", np.int32, 0))
PARETO_RESULT = EVOLVE_RESULT + (("front_size", np.int32, 1),)


def _check_copies(what, n):
    if not 1 <= n <= 4096:
        raise ValueError(f"{what} must be 1..4096")


def _check_rounds_moves(what, count, moves, allowed):
    if count < 0 or not 1 <= moves <= allowed:
        raise ValueError(f"{what} must be >= 0 and moves a non-empty mask of " + " | ".join(x for i, x in enumerate(MOVE_NAMES) if allowed >> i & 1))


def _check_name(name, table, *more):                                   # the entry `name` is none of the result's other keys
    _rule_names([(name,)] + [(key,) for key, _, _ in table] + [(key,) for key in more])


def _thresholds(p_cross, p_mut):
    """the probabilities of `evolve`, checked -> the thresholds round(p * 2**32) the device compares its draws with"""
    if not (0.0 <= float(p_cross) <= 1.0 and 0.0 <= float(p_mut) <= 1.0):
        raise ValueError("p_cross and p_mut must be probabilities")
    return int(round(float(p_cross) * 2 ** 32)), int(round(float(p_mut) * 2 ** 32))


def _start_plans(start, N, T):
    """`start` -> (task [N,T], mach [N,T]) int32, checked"""
    task, mach = np.ascontiguousarray(start[0], np.int32), np.ascontiguousarray(start[1], np.int32)
    if task.shape != (N, T) or mach.shape != (N, T):
        raise ValueError("start must be (task [N,T], mach [N,T])")
    return task, mach


def _start_population(start, P, N, T):
    """`start`: one (task [N,T], mach [N,T]) or a list of S <= P, checked -> the population (task, mach [N,P,T]): member c = start c % S"""
    starts = [start] if len(start) == 2 and np.ndim(start[0]) == 2 else list(start)
    starts = [(np.ascontiguousarray(s[0], np.int32), np.ascontiguousarray(s[1], np.int32)) for s in starts]
    if not 1 <= len(starts) <= P or any(s[0].shape != (N, T) or s[1].shape != (N, T) for s in starts):
        raise ValueError("start must be (task [N,T], mach [N,T]) or a list of 1..P of them")
    member = np.arange(P) % len(starts)
    return np.stack([s[0] for s in starts], 1)[:, member], np.stack([s[1] for s in starts], 1)[:, member]


def _search_result(g, name, table, rounds, **more):
    """`g.finish`'s parts -> a plan search's result: the entry `name`, its plans, `more`, and every key of `table` in its shape — where no
    pass recorded it (no rounds: a plain replay), start_obj is the replay's Objective and a per-round entry has no rows"""
    r = g.collect(last_axis=[key for key, _, rows in table if rows is not None])
    out = _results([name], {name: (r["cum"], r["prev"], r["task"], r["mach"])}, g.T, g.w)
    for key, dt, rows in table:
        if rows is None:
            out[key] = r[key] if key in r else out[name][2].copy()
        else:
            out[key] = r[key].reshape(rounds + rows, g.N) if key in r else np.zeros((rounds + rows, g.N), dt)
    out.update(more)
    return out


def local_search(t, p, tt, edge, args, start, K=16, rounds=32, seed=0, moves=ALL_MOVES, left_shift=False, chunk=None, device=0,
                 obs_dtype="f32", name="LS", replay="steps"):
    """Hill climbing from the plans `start` = (task [N,T], mach [N,T]) — any plan the library returns: PLANS of `pdr_baselines`,
    `lookahead_baselines`, `beam_baselines`, `random_baselines`, or `plans` of `evaluate.sample_best_of_k` — on the N instances t, p
    [N,T,M], tt [N,M,M], edge [N,E,M/E] (args as for `pdr_baselines`).  Per round every instance's incumbent becomes K neighbours
    (`DeviceBatchEnv.plan_neighbours`: copy 0 the incumbent itself, every other copy one SWAP / INSERT of the job string or one
    REASSIGN of a task's machine, drawn from `moves` by the Philox stream of (seed, instance, copy, round)); the K-copy handle
    replays them, and `group_reduce` keeps the best as the next incumbent: plan_neighbours, reset, T steps, final_costs,
    group_reduce — T + 4 launches a round, no torch kernel, nothing read back before the last round.  The incumbent is copy 0 and
    the reduction keeps the lowest copy among equal objectives: it survives ties, and the best Objective never rises.  The draws
    are keyed by the instance's number in the whole set: the results do not depend on `chunk` (instances per pass; None: all N).
    After the last round the best plans are replayed on an n-instance handle step by step, as `beam_baselines` replays its plans;
    a start plan that is no valid plan ends there (RuntimeError).  The handles, the passes, the round after the move kernel and
    that replay are `evaluate.CopyGroups`'.  rounds = 0 is a plain replay of `start`; K = 1 never moves.
    `moves` may also hold MOVE_CRIT_SWAP and MOVE_CRIT_REASSIGN (CRIT_MOVES: both; ALL_MOVES | CRIT_MOVES: all five kinds): a move
    changes the makespan only if it breaks an arc of a critical path, so these take one machine arc of the incumbent's critical
    path between two jobs and turn it round, or put one task of the path on another machine.  The path is read off the device
    state (`DeviceBatchEnv.critical_path`): of `start` after one replay on the n-instance handle before round 0, of every group's
    best copy after its `group_reduce`, while that state is still there — T + 5 launches a round, still nothing read back.
    replay="launch": the copies' replay of a round is `DeviceBatchEnv.replay_plans` — one launch instead of reset, T steps and
    final_costs, the same bits; it writes the copies' schedules only where the round reads a critical path.  The start plans' replay
    for the paths and the last replay stay step by step.  Any other value: ValueError.
    -> {name: (cost_dict_cumsum, Final_4cost, Objective)} in `pdr_baselines`' layout, under PLANS {name: (task[N,T], mach[N,T])}, and
       "start_obj" [N]: the Objective of `start`;  "history" [rounds, N]: the best Objective after every round;
       "accepted" [rounds, N] int8: the move that gave the round's best copy (MOVE_*, 8 and 16 included), -1 where the incumbent stayed."""
    N, T = CopyGroups.sizes(t, args)
    K, R, moves = int(K), int(rounds), int(moves)
    CopyGroups.check_mode(replay)
    _check_copies("K", K)
    _check_rounds_moves("rounds", R, moves, ALL_MOVES | CRIT_MOVES)
    _check_name(name, LOCAL_RESULT)
    st_task, st_mach = _start_plans(start, N, T)
    with CopyGroups(t, p, tt, edge, args, K, chunk, copies=R > 0, plans=True, left_shift=left_shift, obs_dtype=obs_dtype, device=device) as g:
        n, dev, env = g.n, g.dev, g.env
        path = None
        if R:
            obj0 = torch.empty(n * K, dtype=torch.float64, device=dev)
            best = torch.empty(R, n, dtype=torch.int32, device=dev)
            hist = torch.empty(R, n, dtype=torch.float64, device=dev)
            kind = torch.empty(R, n * K, dtype=torch.int8, device=dev)
            if moves & CRIT_MOVES:
                path = g.path_bufs()
        for lo, m in g.passes():
            cur_t, cur_m = g.upload(st_task), g.upload(st_mach)
            col = None
            if path is not None:                                        # the start plans' schedules, for round 0's directed moves
                g.prime_paths(cur_t, cur_m, path)
            for r in range(R):
                out_t, out_m = g.plan_bufs(r)
                env.plan_neighbours(K, cur_t, cur_m, col, seed, r, lo, moves, out_t, out_m, kind[r], critical=path)
                g.round(out_t, out_m, obj0 if r == 0 else False, best[r], hist[r], replay, path is not None)
                if path is not None:                                    # of the best copies, while their state is still there (-1: an empty path)
                    env.critical_path(best[r], None, *path)
                cur_t, cur_m, col = out_t, out_m, best[r]
            if R:
                acc = torch.where(best < 0, torch.full_like(best, -1), kind.gather(1, best.clamp(min=0).long()).to(torch.int32)).to(torch.int8)
                g.finish(cur_t, cur_m, col, f"{name} local-search", start_obj=obj0.view(n, K)[:, 0], history=hist, accepted=acc)
            else:
                g.finish(cur_t, cur_m, None, f"{name} local-search")
    return _search_result(g, name, LOCAL_RESULT, R)


# ---- a walk on plans (csrc/mtfjsp_walk.hip): the local search's round with an acceptance rule that can leave a local optimum
def walk_search(t, p, tt, edge, args, start, K=16, rounds=64, seed=0, moves=ALL_MOVES, tabu=0, slack=None, late=8, left_shift=False,
                chunk=None, device=0, obs_dtype="f32", name="WS", replay="steps"):
    """`local_search` that may step sideways and uphill: start, the instances, args, K, seed, moves (CRIT_MOVES included), left_shift and
    chunk are `local_search`'s, and so are the neighbours of a round (`DeviceBatchEnv.plan_neighbours`, draws keyed by (seed, instance,
    copy, round)) and their replay.  What differs is the acceptance (`DeviceBatchEnv.walk_accept`; include/mtfjsp.h has the rule): of the
    neighbours whose SCHEDULE (`state_signature`) is neither the incumbent's own nor one of the last `tabu` schedules the walk left
    (0..1024; 0: no ring) the best becomes the incumbent if it is strictly better, or within `slack` of the incumbent (None: off; one
    number; or a sequence of `rounds` numbers, a threshold schedule: 0.0 admits sideways steps, inf always moves — with a ring that is
    tabu search), or not above the incumbent's objective `late` rounds ago (0..4096; 0: off — late-acceptance hill climbing).  The
    incumbent can get worse, so the best plan met is kept on the device beside it and is what the result holds.
    A round: plan_neighbours, reset, T steps, final_costs, state_signature, walk_accept — T + 5 launches (T + 6 with directed moves:
    critical_path of the next incumbent), no torch kernel, nothing read back before the last round.  The state is per pass and the
    draws are keyed by the instance's number in the whole set: the results do not depend on `chunk`.  After the last round the best
    plans are replayed as `local_search` replays its plans.  rounds = 0 is a plain replay of `start`; K = 1 never moves.  With tabu = 0,
    slack = None, late = 0 the walk is `local_search`: a copy of the incumbent's schedule is never strictly better.
    The defaults are late acceptance alone: at J6M6E2 x 4096 it ends below the ring with slack = inf under both weightings.
    replay: `local_search`'s ("launch": one launch per round's replay, with the copies' schedules written: every round reads their signatures).
    -> {name: (cost_dict_cumsum, Final_4cost, Objective)} in `pdr_baselines`' layout for the best plans, under PLANS {name: (task[N,T],
       mach[N,T])}, and "start_obj" [N];  "history" [rounds, N]: the best Objective so far after every round (never rising);  "current"
       [rounds, N]: the incumbent's;  "accepted" [rounds, N] int8: the kind of the move taken (MOVE_*), -1 where the walk stayed;  "why"
       [rounds, N] int8: 0 no candidate, 1 refused, 2 better, 3 within the slack, 4 by the late ring, + 8 for a new best;  "barred"
       [rounds, N] int32: neighbours with an objective that were the incumbent's schedule again or in the ring."""
    N, T = CopyGroups.sizes(t, args)
    K, R, moves, tabu, late = int(K), int(rounds), int(moves), int(tabu), int(late)
    CopyGroups.check_mode(replay)
    _check_copies("K", K)
    _check_rounds_moves("rounds", R, moves, ALL_MOVES | CRIT_MOVES)
    if not 0 <= tabu <= 1024 or not 0 <= late <= 4096:
        raise ValueError("tabu must be 0..1024 and late 0..4096")
    if slack is None or np.ndim(slack) == 0:
        slacks = [None if slack is None else float(slack)] * R
    else:
        slacks = [float(x) for x in slack]
        if len(slacks) != R:
            raise ValueError("slack must be None, one number or a sequence of `rounds` numbers")
    _check_name(name, WALK_RESULT)
    st_task, st_mach = _start_plans(start, N, T)
    with CopyGroups(t, p, tt, edge, args, K, chunk, copies=R > 0, plans=True, left_shift=left_shift, obs_dtype=obs_dtype, device=device) as g:
        n, dev, env = g.n, g.dev, g.env
        path = None
        if R:
            obj0 = torch.empty(n * K, dtype=torch.float64, device=dev)
            sig = torch.empty(n * K, dtype=torch.int64, device=dev)
            col = torch.empty(R, n, dtype=torch.int32, device=dev)
            hist, cur = torch.empty(R, n, dtype=torch.float64, device=dev), torch.empty(R, n, dtype=torch.float64, device=dev)
            kind = torch.empty(R, n * K, dtype=torch.int8, device=dev)
            why, barred = torch.empty(R, n, dtype=torch.int8, device=dev), torch.empty(R, n, dtype=torch.int32, device=dev)
            state = env.walk_state(n, late, tabu)
            if moves & CRIT_MOVES:
                path = g.path_bufs()
        for lo, m in g.passes():
            cur_t, cur_m = g.upload(st_task), g.upload(st_mach)
            src = None
            if path is not None:                                        # the start plans' schedules, for round 0's directed moves
                g.prime_paths(cur_t, cur_m, path)
            for r in range(R):
                out_t, out_m = g.plan_bufs(r)
                env.plan_neighbours(K, cur_t, cur_m, src, seed, r, lo, moves, out_t, out_m, kind[r], critical=path)
                g.replay(out_t, out_m, g.cost4, g.done, replay, True)
                env.state_signature(sig)
                env.walk_accept(n, K, g.cost4, g.done, g.w, out_t, out_m, state, sig, r, r == 0, slacks[r], col[r], cur[r], hist[r], False,
                                why[r], barred[r], obj0 if r == 0 else False)
                if path is not None:                                    # of the next incumbents, while their state is still there (-1: an empty path)
                    env.critical_path(col[r], None, *path)
                cur_t, cur_m, src = out_t, out_m, col[r]
            if R:
                acc = torch.where((why & 7) < 2, torch.full_like(col, -1), kind.gather(1, col.clamp(min=0).long()).to(torch.int32)).to(torch.int8)
                g.finish(state["best_task"], state["best_mach"], None, f"{name} walk", start_obj=obj0.view(n, K)[:, 0], history=hist, current=cur,
                         accepted=acc, why=why, barred=barred)
            else:
                g.finish(cur_t, cur_m, None, f"{name} walk")
    return _search_result(g, name, WALK_RESULT, R)


# ---- evolutionary search on plans (csrc/mtfjsp_evolve.hip): a population of P plans per instance, recombined generation by generation
def evolve(t, p, tt, edge, args, start, P=32, generations=32, seed=0, p_cross=0.8, p_mut=0.3, moves=ALL_MOVES, left_shift=False, chunk=None,
           device=0, obs_dtype="f32", name="GA", replay="steps"):
    """A genetic algorithm on the (job string, machine per task) encoding, seeded with plans the library already has: `start` = one
    (task [N,T], mach [N,T]) or a list of S <= P of them — any PLANS entry of `pdr_baselines`, `lookahead_baselines`, `beam_baselines`,
    `random_baselines`, `local_search`, or `plans` of `evaluate.sample_best_of_k` — on the N instances t, p [N,T,M], tt [N,M,M], edge
    [N,E,M/E] (args as for `pdr_baselines`).  Generation 0's population is member c = start[c % S] word for word; the P-copy handle
    replays it and `group_reduce` gives every member's Objective and the best member, so "start_obj" is the best start's Objective.
    Every later generation g = 1..generations: `DeviceBatchEnv.plan_offspring` (child 0 the best member as it is; every other child
    two parents by binary tournaments, crossed with probability p_cross, one move of `moves` with probability p_mut — thresholds
    round(p * 2**32), draws keyed by (seed, instance, child, g)), reset, T steps, final_costs, group_reduce: T + 4 launches, no torch
    kernel, nothing read back before the last generation.  The replacement is generational with one elite: the best Objective never
    rises and is never above the best start's.  The draws are keyed by the instance's number in the whole set: the results do not
    depend on `chunk` (instances per pass; None: all N).  After the last generation the best plans are replayed on an n-instance
    handle step by step, as `local_search` replays its plans (`evaluate.CopyGroups`, which also holds the handles and the round);
    where no member is a valid plan the replay of member 0 ends there (RuntimeError).  generations = 0 is a replay of the best start.
    replay: `local_search`'s ("launch": every generation's replay is one launch; no schedule is read, none is written).
    -> {name: (cost_dict_cumsum, Final_4cost, Objective)} in `pdr_baselines`' layout, under PLANS {name: (task[N,T], mach[N,T])}, and
       "start_obj" [N]: the best start's Objective;  "history" [generations, N]: the best Objective after every generation."""
    N, T = CopyGroups.sizes(t, args)
    P, G, moves = int(P), int(generations), int(moves)
    CopyGroups.check_mode(replay)
    _check_copies("P", P)
    _check_rounds_moves("generations", G, moves, ALL_MOVES)
    cross_thr, mut_thr = _thresholds(p_cross, p_mut)
    _check_name(name, EVOLVE_RESULT)
    pop_task, pop_mach = _start_population(start, P, N, T)
    with CopyGroups(t, p, tt, edge, args, P, chunk, plans=True, left_shift=left_shift, obs_dtype=obs_dtype, device=device) as g:
        n, dev, env = g.n, g.dev, g.env
        obj = torch.empty(n * P, dtype=torch.float64, device=dev)
        best = torch.empty(G + 1, n, dtype=torch.int32, device=dev)
        hist = torch.empty(G + 1, n, dtype=torch.float64, device=dev)
        for lo, m in g.passes():
            cur_t, cur_m = g.plan_bufs(0)
            g.upload(pop_task, cur_t); g.upload(pop_mach, cur_m)
            for gen in range(G + 1):
                if gen:
                    out_t, out_m = g.plan_bufs(gen)
                    env.plan_offspring(P, cur_t, cur_m, obj, best[gen - 1], seed, gen, lo, cross_thr, mut_thr, moves, out_t, out_m, False, False)
                    cur_t, cur_m = out_t, out_m
                g.round(cur_t, cur_m, obj, best[gen], hist[gen], replay)
            g.finish(cur_t, cur_m, best[G], f"{name} evolve", start_obj=hist[0], history=hist[1:])
    return _search_result(g, name, EVOLVE_RESULT, G)


# ---- Pareto-front evolutionary search (csrc/mtfjsp_nsga.hip): parents and children ranked into fronts, the first P survive
def evolve_pareto(t, p, tt, edge, args, start, P=32, generations=32, seed=0, p_cross=0.8, p_mut=0.3, moves=ALL_MOVES, left_shift=False,
                  chunk=None, device=0, obs_dtype="f32", name="NSGA", replay="steps"):
    """`evolve` without collapsing the three objectives before it selects: an NSGA-II style search that returns one Pareto front of
    schedules in (makespan, energy + idle, transport) per instance.  `start`, the P-member generation 0 (member c = start[c % S]), the
    thresholds round(p * 2**32) and the draws keyed by (seed, instance, child, g) are `evolve`'s; 8 <= P <= 1024.
    Generation 0: the P-copy handle replays the population, `DeviceBatchEnv.front_rank` ranks it and `plan_survivors` stores it in
    selection order with fit = the position.  Every later generation g = 1..generations: `plan_offspring(P, pop, fit, None, ...)` — a
    binary tournament on the position is NSGA-II's crowded comparison: lower front first, then larger crowding distance — into a second
    buffer; reset, T steps, final_costs of the children; `front_rank` over parents and children together (K = 2P); `plan_survivors`
    keeps the first P of the order in a third buffer, and the three take turns: T + 5 launches, no torch kernel, nothing read back
    before the last generation.  Selection (include/mtfjsp.h has the rule): fronts by peeling, inside a front the larger crowding
    distance, and — the one addition to the textbook rule — the member of a front with its smallest Objective counts as +inf, so at
    most seven members of front 0 carry +inf and with P >= 8 and weights that are not negative the smallest Objective always survives:
    the best Objective never rises and is never above the best start's.  Ties go to the lower index; of exact duplicates the lowest
    index keeps its front and the others fall to later ones; there is no archive across generations.  The results do not depend on
    `chunk`.  After the last generation one `group_reduce` over the survivors gives the best-Objective member, which is replayed on
    an n-instance handle as `evolve` replays its best plan (RuntimeError where no member is a valid plan), and the population's
    plans, costs and ranks are read back once.  replay: `evolve`'s.
    -> {name: (cost_dict_cumsum, Final_4cost, Objective)} in `pdr_baselines`' layout and PLANS {name: (task[N,T], mach[N,T])} for the
       best-Objective member; "start_obj" [N]: the best start's Objective; "history" [generations, N]: the best Objective among
       parents and children of every generation; "front_size" [generations + 1, N] int32: the members of front 0 among the ranked
       candidates of every generation (generation 0 included); "fronts": a list of N dicts {"cost" [F,3] (mk, ec, tt), "final4"
       [F,4], "obj" [F], "task" [F,T], "mach" [F,T]}: the front-0 survivors in selection order."""
    N, T = CopyGroups.sizes(t, args)
    P, G, moves = int(P), int(generations), int(moves)
    CopyGroups.check_mode(replay)
    if not 8 <= P <= 1024:
        raise ValueError("P must be 8..1024 (the best Objective is only sure to survive among 8 or more)")
    _check_rounds_moves("generations", G, moves, ALL_MOVES)
    cross_thr, mut_thr = _thresholds(p_cross, p_mut)
    _check_name(name, PARETO_RESULT, "fronts")
    pop_task, pop_mach = _start_population(start, P, N, T)
    fronts = []
    with CopyGroups(t, p, tt, edge, args, P, chunk, plans=True, left_shift=left_shift, obs_dtype=obs_dtype, device=device) as g:
        n, dev, env = g.n, g.dev, g.env
        B = n * P
        plans = list(g.bufs) + [tuple(torch.empty(T, B, dtype=torch.int32, device=dev) for _ in range(2))]
        # three slots (task, mach, cost4, done) that take turns as parents, children and survivors
        slots = [pl + (torch.empty(B, 4, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.uint8, device=dev)) for pl in plans]
        rank, order = torch.empty(2 * B, dtype=torch.int32, device=dev), torch.empty(2 * B, dtype=torch.int32, device=dev)
        fit, pop_rank = torch.empty(B, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
        size = torch.empty(G + 1, n, dtype=torch.int32, device=dev)
        hist = torch.empty(G + 1, n, dtype=torch.float64, device=dev)
        obj, best = torch.empty(B, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
        for lo, m in g.passes():
            pop, child, spare = slots
            g.upload(pop_task, pop[0]); g.upload(pop_mach, pop[1])
            g.replay(*pop, replay)
            env.front_rank(n, pop[2], pop[3], None, None, g.w, rank[:B], False, order[:B], size[0], hist[0])
            env.plan_survivors(P, order[:B], rank[:B], pop, None, child[0], child[1], child[2], child[3], pop_rank, False, fit)
            pop, child = child, pop
            for gen in range(1, G + 1):
                env.plan_offspring(P, pop[0], pop[1], fit, None, seed, gen, lo, cross_thr, mut_thr, moves, child[0], child[1], False, False)
                g.replay(*child, replay)
                env.front_rank(n, pop[2], pop[3], child[2], child[3], g.w, rank, False, order, size[gen], hist[gen])
                env.plan_survivors(P, order, rank, pop, child, spare[0], spare[1], spare[2], spare[3], pop_rank, False, fit)
                pop, child, spare = spare, pop, child
            env.group_reduce(n, P, pop[2], pop[3], g.w, obj=obj, best=best, best_obj=False, front=False)
            g.finish(pop[0], pop[1], best, f"{name} evolve_pareto", start_obj=hist[0], history=hist[1:], front_size=size)
            h_task, h_mach = pop[0][:, :m * P].t().cpu().numpy(), pop[1][:, :m * P].t().cpu().numpy()   # the population, read back once
            h_c4, h_obj, h_rank = pop[2][:m * P].cpu().numpy(), obj[:m * P].cpu().numpy(), pop_rank[:m * P].cpu().numpy()
            for i in range(m):
                sel = np.flatnonzero(h_rank[i * P:(i + 1) * P] == 0) + i * P
                f4 = h_c4[sel]
                fronts.append({"cost": np.stack([f4[:, 0], f4[:, 1] + f4[:, 3], f4[:, 2]], 1), "final4": f4, "obj": h_obj[sel],
                               "task": np.ascontiguousarray(h_task[sel]), "mach": np.ascontiguousarray(h_mach[sel])})
    return _search_result(g, name, PARETO_RESULT, G, fronts=fronts)


def hypervolume(points, ref):
    """The volume that `points` [F,3] dominate below the reference point `ref` [3], all three axes minimised — one number per front
    (`evolve_pareto`'s "cost").  Exact slicing on the host: along the first axis the space falls into slabs between consecutive
    coordinates, and a slab's cross-section is the area the points met so far dominate in the other two axes, a staircase.
    Points that are not strictly below `ref` on every axis contribute nothing; dominated points and duplicates are harmless."""
    pts = np.asarray(points, np.float64).reshape(-1, 3)
    ref = np.asarray(ref, np.float64).reshape(3)
    pts = pts[(pts < ref).all(1)]
    if not len(pts):
        return 0.0
    pts = pts[np.argsort(pts[:, 0], kind="stable")]
    vol = 0.0
    for i in range(len(pts)):
        depth = (pts[i + 1, 0] if i + 1 < len(pts) else ref[0]) - pts[i, 0]
        if depth <= 0.0:
            continue
        area, low = 0.0, ref[2]                                         # the staircase of pts[:i + 1] in axes 1 and 2
        for y, z in sorted(map(tuple, pts[:i + 1, 1:])):
            if z < low:
                area += (ref[1] - y) * (low - z)
                low = z
        vol += depth * area
    return float(vol)

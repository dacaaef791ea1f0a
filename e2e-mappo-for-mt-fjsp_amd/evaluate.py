"""Batched greedy evaluation — the reference's `validate_cost_gcn_jointActor_GAT` (trainer/validate.py:60-297) for a
whole evaluation set in ONE device rollout.

The reference evaluates instance by instance with env_batch = 1 (Run.py:672-745: 100 serial episodes, ~60 s per
evaluation): fixed reward weights (`reset(Random_weight_type="eval")`, env:1262), no reward scaling, greedy decoding, and
— because its BatchNorms are always in training mode — statistics over the rows of the single instance.  Here the B
instances run side by side: `Encoder.set_bn_mode(True)` gives every instance its own BatchNorm statistics
(`k_gin_inst` / `k_gat_inst`, one workgroup per instance), the raw (unscaled) rewards of `mtfjsp_obs_t.raw` are summed
on the device, and the final costs are read from the `*_previous_step` state exactly as validate.py:277-287 does.
"""
import numpy as np
import torch

from . import capi
from .batch_env import DeviceBatchEnv


COST_KEYS = ("opr_Gt", "opr_mk", "opr_idleT", "opr_pt", "opr_transT")


def parse_args(args, **env_kw):
    """The reference's config dict `args` (n_job, n_machine, n_edge, weight_mk, weight_ec, weight_tt, reward_scaling) -> (J, M, E, T,
    w, kw): the sizes, the three weights as floats and `DeviceBatchEnv`'s keywords (w_cfg, scaling_divisor and `env_kw`)."""
    J, M, E = int(args["n_job"]), int(args["n_machine"]), int(args["n_edge"])
    w = (float(args["weight_mk"]), float(args["weight_ec"]), float(args["weight_tt"]))
    scal = args.get("reward_scaling", {}) or {}
    return J, M, E, J * M, w, dict(env_kw, w_cfg=w, scaling_divisor=float(scal.get("scaling_divisor", 1.0)))


def episode_results(cum, prev, T, w):
    """cum [N,5]: the summed raw step rewards (reward, r_mk, r_idle, r_pt, r_tt); prev [N,4]: mk, e1, transT, idle of the finished
    schedule (STATE_PREV_COSTS); w: (w_mk, w_ec, w_tt) -> (cost_dict_cumsum, Final_4cost [N,4], Objective [N]) as
    `validate_cost_batched` documents them (validate.py:277-297, test_all.py:536-538).  Pure numpy: no device, no state."""
    cost = {key: cum[:, i] for i, key in enumerate(COST_KEYS)}
    final4 = np.stack([prev[:, 0], prev[:, 1] / T, prev[:, 2], prev[:, 3]], 1)
    obj = w[0] * final4[:, 0] + w[1] * (final4[:, 1] + final4[:, 3]) + w[2] * final4[:, 2]
    return cost, final4, obj


def config_w3(env, w):
    """the config weights w = (w_mk, w_ec, w_tt) for every instance of `env`: the [B,3] device tensor an evaluation resets with"""
    return torch.tensor([w], dtype=torch.float64, device=env.device).repeat(env.B, 1)


def eval_reset(env, w3):
    """An evaluation's reset (pdrs:675, env:1262 Random_weight_type="eval"): a fresh reward scaler (its output is not used), then the weights w3"""
    env.scaler_init()
    env.reset(w3)


def replay_episode(env, T, actions, what):
    """T steps of the reset handle `env`, step s with the (task, mach) [B] int32 device tensors `actions(s)` returns, the raw rewards
    summed on the device; one synchronisation, then RuntimeError("<what> rollout: ...") if an instance met an invalid action or an
    infeasible machine, or did not finish.  -> (cum [B,5], prev [B,4]) host arrays: `episode_results`' inputs."""
    dev = env.device
    cum = torch.zeros(env.B, 5, dtype=torch.float64, device=dev)
    bad = torch.zeros(env.B, dtype=torch.int32, device=dev)
    for s in range(T):
        env.step(*actions(s))
        cum += env.raw                                                  # reward, r_mk, r_idle, r_pt, r_tt (env:1051-1171), in step order
        bad |= env.status
    torch.cuda.synchronize(dev)
    n_bad = int((bad & (capi.ST_INVALID | capi.ST_INFEASIBLE)).ne(0).sum().item())
    if n_bad:
        raise RuntimeError(f"{what} rollout: {n_bad} instance(s) met an invalid action or an infeasible machine")
    if not bool(env.info[:, 1].all().item()):
        raise RuntimeError(f"{what} rollout: an episode did not finish after T steps")
    prev = env.read_state(capi.STATE_PREV_COSTS)                        # mk, e1, transT, idle of the finished schedule (pdrs:808-812)
    return cum.cpu().numpy(), prev


def validate_cost_batched(weights, t, p, tt, edge, args, greedy=True, device=0, obs_dtype="f32", actor=None,
                          forced_actions=None, on_step=None, on_action=None):
    """weights: (job_actor_state_dict, machine_actor_state_dict) with the reference's key names (or an `ActorPair` via
    `actor=`); t, p [B,T,M], tt [B,M,M], edge [B,E,M/E]: the evaluation instances; args: the reference's config dict
    (n_job, n_machine, n_edge, weight_mk, weight_ec, weight_tt).
    forced_actions [B,T,2] (task, machine): replay these decisions (teacher forcing) — the forwards still run and
    on_step(s, job_prob, mch_prob) sees the policy's distributions in every visited state; used by the parity tests, because the
    reference's own greedy choice among machines whose scores tie is decided by f32 round-off (validate.py has many
    exactly-uniform machine distributions in its first steps).
    Returns, per instance and in the reference's order (validate.py:297):
      cost_dict_cumsum  dict of [B] arrays: opr_Gt, opr_mk, opr_idleT, opr_pt, opr_transT (sums of the raw step rewards)
      Final_4cost       [B,4]: makespan, mean processing energy, transport time, idle time of the finished schedule
      Objective         [B]:   w_mk*mk + w_ec*(pt + idle) + w_tt*transT
    """
    from . import encoder as enc_mod
    J, M, E, T, w, kw = parse_args(args, obs_dtype=obs_dtype, device=device)
    t = np.asarray(t, np.float64)
    B = t.shape[0]
    env = DeviceBatchEnv(J, M, E, B, **kw)
    env.load_instances(t, np.asarray(p, np.float64), np.asarray(tt, np.float64), edge=np.asarray(edge))
    env.scaler_init()                                               # the scaled components are produced but not used here
    dev = env.device
    if actor is None:
        actor = enc_mod.ActorPair(J, M, B, device=device, obs_dtype=obs_dtype, weights=weights, greedy=greedy, seed=0)
    actor.enc.set_bn_mode(True)
    try:
        w3 = torch.tensor([w], dtype=torch.float64, device=dev).repeat(B, 1)
        env.reset(w3)                                               # env:1262 Random_weight_type="eval"
        actor.begin_episode()
        task = torch.zeros(B, dtype=torch.int32, device=dev); mach = torch.zeros_like(task); job = torch.zeros_like(task)
        cum = torch.zeros(B, 5, dtype=torch.float64, device=dev)
        fa = None if forced_actions is None else torch.as_tensor(np.asarray(forced_actions), dtype=torch.int32, device=dev)
        for s in range(T):
            if fa is None:
                actor.act(env, s, task, mach, job)
            else:
                # the forwards run on the forced trajectory's states: job_prob is the policy's distribution in this state,
                # mch_prob its machine distribution for the FORCED task
                actor.act(env, s, task, mach, job, force=(fa[:, s, 0].contiguous(), fa[:, s, 1].contiguous()))
                if on_step is not None:
                    on_step(s, actor.enc.job_prob, actor.enc.mch_prob)
            if on_action is not None:
                on_action(s, task, mach)                            # the decisions about to be applied (tests)
            env.step(task, mach)
            cum += env.raw                                          # reward, r_mk, r_idle, r_pt, r_tt (env:1051-1171), unscaled
        torch.cuda.synchronize(dev)
        st = env.status
        if int((st & capi.ST_INVALID).sum().item()) != 0:
            raise RuntimeError("greedy evaluation produced an invalid action")
        assert bool(env.info[:, 1].all().item()), "evaluation episode did not finish"
        prev = env.read_state(capi.STATE_PREV_COSTS)                # mk, e1, transT, idle of the finished schedule (validate.py:277-281)
    finally:
        actor.enc.set_bn_mode(False)
    return episode_results(cum.cpu().numpy(), prev, T, w)



class CopyGroups:
    """What every search over groups of copies is built on (`best_of_k_rollout`, `baselines.local_search`, `baselines.evolve`, `baselines.evolve_pareto`): N
    instances, n = chunk or N of them per pass, K copies of each side by side.  Three handles: `src` with the N loaded instances, `env`
    with the n*K copies (copy c of group i = element i*K + c; None with copies=False) and `top` with n, for the best copy of every
    group; per pass both take their constants from `src` by the explicit-index fork.  The constructor validates `chunk` and builds the
    handles and index tensors (`copy_of`, `own`: every group's copy 0, `inst_of`, `w3_all`, `w3_top`: args' weights per element, or w3 [K,3]:
    copy c of every group resets with w3[c]); leaving the `with` block closes the handles.  `passes()` iterates; `host`,
    `parts` and `collect()` gather the per-pass results.  `sizes(t, args)` gives N and T before anything is built.
    For searches on plans (plans=True; [T, n*K] int32 histories, row s = the actions of step s): `upload()` brings host plans into one,
    `plan_bufs(i)` are two pairs of them that take turns, `round()` replays one on the copies (`replay()`) and reduces the groups,
    `path_bufs()` / `prime_paths()` hold and first fill the critical paths of directed moves, `finish()` replays every group's best plan on `top`."""

    @staticmethod
    def sizes(t, args):
        return np.shape(t)[0], parse_args(args)[3]

    def __init__(self, t, p, tt, edge, args, K, chunk=None, copies=True, plans=False, w3=None, **env_kw):
        J, M, E, self.T, self.w, kw = parse_args(args, **env_kw)
        t = np.asarray(t, np.float64)
        self.N, self.K = t.shape[0], int(K)
        n = self.N if chunk is None else int(chunk)
        if n < 1:
            raise ValueError("chunk must be at least 1")
        self.n = n = min(n, self.N)
        self.src = self.env = self.top = None
        self.parts = []
        try:
            self.src = DeviceBatchEnv(J, M, E, self.N, **kw)
            self.src.load_instances(t, np.asarray(p, np.float64), np.asarray(tt, np.float64), edge=np.asarray(edge))
            self.dev = dev = self.src.device
            self.top = DeviceBatchEnv(J, M, E, n, **kw)
            B = n * self.K
            if copies:                                                  # (every handle before the first tensor)
                self.env = DeviceBatchEnv(J, M, E, B, **kw)
            self.w3_top = config_w3(self.top, self.w)
            self.inst_of = torch.arange(n, dtype=torch.int32, device=dev)
            if copies:
                w3_k = torch.as_tensor(np.ascontiguousarray([self.w] if w3 is None else w3, np.float64), device=dev)
                if w3 is not None and tuple(w3_k.shape) != (self.K, 3):
                    raise ValueError("w3 must be [K,3]")
                self.w3_all = w3_k.repeat(B // w3_k.shape[0], 1).contiguous()
                self.copy_of = torch.arange(B, dtype=torch.int32, device=dev) // self.K
                self.own = self.inst_of * self.K
                if plans:
                    self.bufs = [tuple(torch.empty(self.T, B, dtype=torch.int32, device=dev) for _ in range(2)) for _ in range(2)]
                    self.cost4, self.done = torch.empty(B, 4, dtype=torch.float64, device=dev), torch.empty(B, dtype=torch.uint8, device=dev)
        except BaseException:
            self.close()
            raise

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        for e in (self.top, self.env, self.src):
            if e is not None:
                e.close()
        self.src = self.env = self.top = None

    def passes(self):
        """-> (lo, m) per pass: the pass holds instances lo .. lo + m - 1 (a last, smaller pass is padded with copies of its last
        instance); both handles have their instances (`top` first), the copies' scaler is initialised"""
        for lo in range(0, self.N, self.n):
            self.lo, self.m = lo, min(self.n, self.N - lo)
            self.top.fork_from(self.src, torch.clamp(self.inst_of + lo, max=self.N - 1), instance=True, state=False, obs=False)
            if self.env is not None:
                self.env.fork_from(self.src, torch.clamp(self.copy_of + lo, max=self.N - 1), instance=True, state=False, obs=False)
                self.env.scaler_init()                                  # the scaled components are produced but not used here
            yield lo, self.m

    def pad(self, x):                                                   # host array [N, ...] -> the rows of this pass's n instances
        return x[np.minimum(np.arange(self.n) + self.lo, self.N - 1)]

    def host(self, x):                                                  # device tensor [..., n] -> host array [..., m]
        return x[..., :self.m].cpu().numpy()

    def collect(self, last_axis=()):
        """the per-pass dicts of `parts` -> one dict, concatenated along the instances' axis: the first, or the last for keys in `last_axis`"""
        return {k: np.concatenate([x[k] for x in self.parts], axis=-1 if k in last_axis else 0) for k in self.parts[0]}

    # ---- searches on plans
    def plan_bufs(self, i):
        return self.bufs[i & 1]

    def upload(self, plans, out=None):
        """host plans [N,T] or [N,K,T] int32 -> this pass's device history [T,n] or [T,n*K], row s = the actions of step s (a new one, or `out`)"""
        host = torch.as_tensor(np.ascontiguousarray(self.pad(plans).reshape(-1, self.T).T))
        return host.to(self.dev) if out is None else out.copy_(host)

    def path_bufs(self):
        """every group's critical path, `DeviceBatchEnv.critical_path`'s outputs: (tasks [n,T] int32, arcs [n,T] int8, length [n] int32)"""
        n, T, dev = self.n, self.T, self.dev
        return torch.empty(n, T, dtype=torch.int32, device=dev), torch.empty(n, T, dtype=torch.int8, device=dev), torch.empty(n, dtype=torch.int32, device=dev)

    def prime_paths(self, task, mach, path):
        """the plans (task, mach) [T,n] replayed on `top` step by step, their schedules' critical paths into `path` (for round 0's directed moves)"""
        eval_reset(self.top, self.w3_top)
        for s in range(self.T):
            self.top.step(task[s], mach[s])
        self.top.critical_path(None, None, *path)

    REPLAY_MODES = ("steps", "launch")

    @classmethod
    def check_mode(cls, mode):
        if mode not in cls.REPLAY_MODES:
            raise ValueError('replay must be "steps" or "launch"')
        return mode

    def round(self, task, mach, obj, best, best_obj, mode="steps", state=False):
        """the copies replay the plans (task, mach) and every group is reduced into the tensors given (obj may be False): reset, T steps,
        final_costs, group_reduce — T + 3 launches (mode "launch": 2), no torch kernel, nothing read back; mode, state: `replay`'s"""
        self.replay(task, mach, self.cost4, self.done, mode, state)
        self.env.group_reduce(self.n, self.K, self.cost4, self.done, self.w, obj=obj, best=best, best_obj=best_obj, front=False)

    def replay(self, task, mach, cost4, done, mode="steps", state=False):
        """the copies replay the plans (task, mach), their final costs into the tensors given.  mode "steps": reset, T steps, final_costs
        — T + 2 launches; mode "launch": `DeviceBatchEnv.replay_plans`, one launch, the same costs (NaN for a copy that is not done),
        and the copies' schedules are there afterwards (`critical_path`, `state_signature`) only with state=True.  No torch kernel,
        nothing read back"""
        env = self.env
        if self.check_mode(mode) == "launch":
            env.replay_plans(task, mach, cost4, done, state=state)
            return
        env.reset(self.w3_all)
        for s in range(self.T):
            env.step(task[s], mach[s])
        env.final_costs(cost4, done)                                    # a rejected action leaves done = 0: the copy is not eligible

    def finish(self, task, mach, col, what, **extra):
        """the pass's result: column col[i] of (task, mach) for group i — its copy 0 where col[i] < 0, a group without an eligible copy,
        which the replay rejects; col None: column i — replayed on `top` step by step (`replay_episode`: RuntimeError for a plan that
        is none) -> appends dict(cum, prev, task [m,T], mach [m,T], **extra) to `parts`, the device tensors of `extra` through `host`"""
        if col is not None:
            pick = torch.where(col < 0, self.own, col).long()
            task, mach = task.index_select(1, pick).contiguous(), mach.index_select(1, pick).contiguous()
        eval_reset(self.top, self.w3_top)
        cum, prev = replay_episode(self.top, self.T, lambda s: (task[s], mach[s]), what)
        self.parts.append(dict(cum=cum[:self.m], prev=prev[:self.m], task=self.host(task).T.copy(), mach=self.host(mach).T.copy(),
                               **{k: self.host(x) for k, x in extra.items()}))


def best_of_k_rollout(t, p, tt, edge, args, K, policy, w3=None, chunk=None, device=0, obs_dtype="f32", left_shift=True, what="best-of-K",
                      on_event=None):
    """The K-copy rollout behind `sample_best_of_k` and `baselines.random_baselines`: N instances, K copies of each side by side in
    one handle of n*K (`CopyGroups`: n = chunk or N instances per pass; copy c of instance i = element i*K + c), every copy playing its own
    episode with the actions `policy.decide(env, s, task_row, mach_row, job)` writes into row s of the [T, n*K] histories; then the final
    costs, the best copy and the Pareto front per instance on the device (csrc/mtfjsp_group.hip) and a fork of the best copies into an
    n-instance handle, from which their schedules are read.  policy: `open(batch)` once before the first pass, `begin()` at every
    pass's reset, `decide(...)` per step, `close()` at the end.  on_event(event, env, first_instance, hist_task, hist_mach) (tests): called
    with "reset" after every pass's reset and with "end" after its last step, the handle of copies and the [T, n*K] device histories.
    -> the dict `sample_best_of_k` documents, plus `cum` [N,K,5]: every copy's summed raw rewards."""
    K = int(K)
    if not 1 <= K <= 4096:
        raise ValueError("K must be 1..4096")
    with CopyGroups(t, p, tt, edge, args, K, chunk, w3=w3, left_shift=left_shift, obs_dtype=obs_dtype, device=device) as g:
        n, T, w, dev, env, top = g.n, g.T, g.w, g.dev, g.env, g.top
        policy.open(n * K)
        try:
            hist_task = torch.empty(T, n * K, dtype=torch.int32, device=dev)
            hist_mach = torch.empty(T, n * K, dtype=torch.int32, device=dev)
            job = torch.zeros(n * K, dtype=torch.int32, device=dev)
            cum = torch.empty(n * K, 5, dtype=torch.float64, device=dev)
            bad = torch.empty(n * K, dtype=torch.int32, device=dev)
            for lo, m in g.passes():
                env.reset(g.w3_all)
                policy.begin()
                if on_event is not None:
                    on_event("reset", env, lo, hist_task, hist_mach)
                cum.zero_(); bad.zero_()
                for s in range(T):
                    policy.decide(env, s, hist_task[s], hist_mach[s], job)
                    env.step(hist_task[s], hist_mach[s])
                    bad |= env.status
                    cum += env.raw                                      # reward, r_mk, r_idle, r_pt, r_tt (env:1051-1171), unscaled
                if on_event is not None:
                    on_event("end", env, lo, hist_task, hist_mach)
                cost4, done = env.final_costs()
                obj, best, best_obj, front = env.group_reduce(n, K, cost4, done, w)
                top.fork_from(env, best, instance=False, state=True, obs=False)
                pick = best.clamp(min=0).long()
                best_cum, best_c4 = cum.index_select(0, pick), cost4.index_select(0, pick)
                plan_t, plan_m = hist_task.index_select(1, pick).t().contiguous(), hist_mach.index_select(1, pick).t().contiguous()
                torch.cuda.synchronize(dev)
                if int((bad[:m * K] & capi.ST_INVALID).ne(0).sum().item()) != 0:
                    raise RuntimeError(f"{what} evaluation produced an invalid action")
                if not bool(done[:m * K].all().item()) or int(best[:m].min().item()) < 0:
                    raise RuntimeError(f"{what} evaluation: an episode did not finish")
                host = lambda x, k=m: x[:k].cpu().numpy()               # noqa: E731
                g.parts.append(dict(
                    best_copy=host(best).astype(np.int64) + lo * K, best_obj=host(best_obj), best_cum=host(best_cum), best_c4=host(best_c4),
                    obj=host(obj, m * K).reshape(m, K), final4=host(cost4, m * K).reshape(m, K, 4), front=host(front, m * K).reshape(m, K).astype(bool),
                    cum=host(cum, m * K).reshape(m, K, 5), plan_t=host(plan_t), plan_m=host(plan_m),
                    machine=top.read_state(capi.STATE_MACHINE)[:m], start=top.read_state(capi.STATE_START)[:m],
                    finish=top.read_state(capi.STATE_FINISH)[:m]))
        finally:
            policy.close()
    r = g.collect()
    cost = {key: r["best_cum"][:, i] for i, key in enumerate(COST_KEYS)}
    return {"best": (cost, r["best_c4"], r["best_obj"]), "best_copy": r["best_copy"], "obj": r["obj"], "final4": r["final4"],
            "front": r["front"], "cum": r["cum"], "plans": (r["plan_t"], r["plan_m"]),
            "schedule": {"machine": r["machine"], "start": r["start"], "finish": r["finish"]}}


class _SampledPolicy:
    """`best_of_k_rollout`'s policy: one `ActorPair` of the copies' batch with per-instance BatchNorm"""

    def __init__(self, weights, J, M, greedy, seed, device, obs_dtype):
        self.cfg, self.actor = (weights, J, M, greedy, seed, device, obs_dtype), None

    def open(self, batch):
        from . import encoder as enc_mod
        weights, J, M, greedy, seed, device, obs_dtype = self.cfg
        self.actor = enc_mod.ActorPair(J, M, batch, device=device, obs_dtype=obs_dtype, weights=weights, greedy=greedy, seed=seed)
        self.actor.enc.set_bn_mode(True)

    def begin(self):
        self.actor.begin_episode()

    def decide(self, env, s, task_row, mach_row, job):
        self.actor.act(env, s, task_row, mach_row, job)                 # the actions land in the history rows: no copies

    def close(self):
        if self.actor is not None:
            self.actor.enc.set_bn_mode(False)
            self.actor.enc.close()


def sample_best_of_k(weights, t, p, tt, edge, args, K, seed=0, greedy=False, w3=None, chunk=None, device=0, obs_dtype="f32",
                     left_shift=True, on_event=None):
    """Best-of-K evaluation of the policy: K schedules per instance drawn from the actors (`greedy=False`; the Philox sampler of
    `ActorPair`, keyed by (seed, decision, index of the copy inside the handle)), the best of them kept — and, the policy being
    conditioned on the preference weights, the Pareto front of the K (makespan, energy, transport) points of every instance.
    The reference evaluates one greedy schedule per instance (validate.py:60-297).

    weights, t, p, tt, edge, args: as for `validate_cost_batched`; N instances.  The instances are loaded once; a handle of n*K
    copies (n = chunk or N instances per pass) takes its constants from them by the explicit-index fork, runs T decisions with
    per-instance BatchNorm (a copy's forward does not depend on its neighbours), and the reductions over the copies run on the
    device: only [n]- and [n*K]-sized scalars, the best plans and the n best schedules are read back per pass.
    w3 [K,3]: copy c is reset with the preference w3[c] — what the policy sees in columns 9-11 of tasks_fea — instead of args'
    weights; `best` and `obj` are measured with args' weights either way.
    Reproducibility: the sampler is keyed by a copy's index INSIDE THE HANDLE, so the samples — and with them every result — are a
    function of (seed, K, chunk), not of (seed, K) alone; the same (seed, K, chunk) gives the same results bit for bit.  With
    greedy=True all K copies of an instance are the same schedule (K = 1 is `validate_cost_batched`).
    Ties: the best copy is the lowest c among equal objectives; of exact duplicates only the lowest c is on the front.
    -> dict:
      best       (cost_dict_cumsum, Final_4cost [N,4], Objective [N]) of every instance's best copy, in `validate_cost_batched`'s layout
      best_copy  [N] int64: i*K + c of that copy (an index into the flattened [N,K] arrays)
      obj        [N,K] every copy's Objective;  final4 [N,K,4] its Final_4cost;  cum [N,K,5] its summed raw rewards
      front      [N,K] bool: the copy is not dominated in (makespan, energy + idle, transport) by another copy of its instance
      plans      (task [N,T], mach [N,T]) int32: the decisions of the best copy
      schedule   {"machine" [N,T] int32, "start" [N,T], "finish" [N,T]}: the best copy's schedule
    on_event: see `best_of_k_rollout` (tests)."""
    policy = _SampledPolicy(weights, int(args["n_job"]), int(args["n_machine"]), greedy, seed, device, obs_dtype)
    return best_of_k_rollout(t, p, tt, edge, args, K, policy, w3=w3, chunk=chunk, device=device, obs_dtype=obs_dtype, left_shift=left_shift,
                             what="best-of-K", on_event=on_event)

"""Host model of what a free-running Rollout(collect="full") leaves in its device TrajectoryBuffer (test infrastructure only).

Inputs: the shard's instances, the rollout's seed, the number of episodes, the RECORDED actions (a_operation = job, a = machine,
[S, B]), the observation dtype, left shift and the reward configuration.  Nothing else comes from the device.

Environment half (exact): TrajectoryModel drives oracle.env_oracle.OracleBatch as tests/env_parity.py does — scaler_init once,
scaler_reset_returns before every episode after the first, reset(draw_w3(B, seed, episode)) — and yields, slot by slot, every
environment-side field of the buffer in the buffer's own dtypes (FIELDS).  compare_slot / compare_record hold a record to it with
env_parity._same and name the field and the slot of the first difference.  The model is stateful (the reward scaler's running
statistics outlive a buffer): a second call of slots() models the next buffer of the same rollout.

Network half (bounded): slot_forward evaluates the two actors of oracle.encoder_oracle on one slot's own fields, given the previous
machine embedding and (optionally) the current job embedding; terminal_pair evaluates the post-terminal pair of Run.py:455-475 as
ActorPair.terminal_values states it.  compare_network holds a record's log-probabilities and critic values to such evaluations
under caller-given bounds and names the field and the slot.

The critics read pooled embeddings only, so the job mask of the terminal forward cannot show in a stored value (the CPU test
proves it on the fixture): records carry the mask that forward was given as their own field, `term_mask` [episodes, B, J]."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import device_streams_ref as streams  # noqa: E402
from env_parity import _same, ell_rows  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# environment-side fields of a slot, by the TrajectoryBuffer's attribute names (r4 = mk, idle, pt, tt: the step kernel's order)
OBS_FIELDS = ("tasks_fea", "tasks_fea_", "machine_fea1", "machine_fea2", "machine_fea2_")
ELL_FIELDS = (("ell_col", "ell_val"), ("ell_col_", "ell_val_"))
FIELDS = OBS_FIELDS + ("candidate", "mask_operation", "candidate_", "mask_operation_", "mask_machine_", "r_operation", "done_operation", "r4",
                       "random_weight") + tuple(k for pair in ELL_FIELDS for k in pair)
NET_FIELDS = ("a_logprob_operation", "a_logprob", "job_v", "machine_v", "job_v_", "machine_v_")
# the reference ReplayBuffer's tuple order (replaybuffer.py:141-204), as tests/test_rollout_handoff.py names it
TUPLE_NAMES = ("adj", "tasks_fea", "candidate", "mask_operation", "a_operation", "a_logprob_operation", "adj_", "tasks_fea_", "candidate_",
               "mask_operation_", "r_operation", "done_operation", "machine_fea2", "a", "a_logprob", "machine_fea2_", "mask_machine_",
               "mk", "pt", "tt", "it", "machine_fea1", "rw", "job_v", "machine_v", "job_v_", "machine_v_")


class TrajectoryModel:
    def __init__(self, instances, seed, obs_dtype="f32", left_shift=True, w_cfg=(0.4, 0.4, 0.2), divisor=1.0, gamma=0.99):
        from oracle.env_oracle import OracleBatch
        t, p, tt, edge = instances
        self.t = np.asarray(t, np.float64)
        self.B, self.T, self.M = self.t.shape
        self.E = np.asarray(edge).shape[1]
        self.feas = self.t >= 0
        self.seed = seed
        self.odt = {"f32": np.float32, "f64": np.float64}[obs_dtype]
        self.orc = OracleBatch(t, p, tt, edge, left_shift=left_shift, w_cfg=w_cfg, divisor=divisor, gamma=gamma)
        self.J = self.orc.J
        self.orc.scaler_init()
        self.episode = 0                                  # episodes replayed so far: the next one's number in the rollout's run

    def slots(self, a_operation, a, episodes, weights=None):
        """generator over the episodes * T slots of the next buffer: dict of FIELDS (one slot each, no leading axis) plus `task`,
        `legal` [B] (the recorded job is unmasked, the recorded machine feasible for its task) and `w3` (binary64).  An illegal
        action ends the replay after its slot (the oracle cannot take it).  weights [episodes, B, 3]: the reward weights, where
        they are given instead of drawn"""
        B, T, M, J, orc, odt = self.B, self.T, self.M, self.J, self.orc, self.odt
        jobs, machs = np.asarray(a_operation).astype(np.int64), np.asarray(a).astype(np.int64)
        assert jobs.shape == machs.shape == (episodes * T, B), (jobs.shape, machs.shape, episodes, T, B)
        rows = np.arange(B)
        obs = lambda x: np.asarray(x, np.float64).astype(odt)
        for e in range(episodes):
            w3 = streams.draw_w3(B, self.seed, self.episode) if weights is None else np.asarray(weights[e], np.float64)
            if self.episode > 0:
                orc.scaler_reset_returns()
            o = orc.reset(w3)
            self.episode += 1
            cand, mask = orc.job_mask_state()
            for k in range(T):
                s = e * T + k
                job, mach = jobs[s], machs[s]
                in_range = (job >= 0) & (job < J) & (mach >= 0) & (mach < M)
                jc, mc = np.clip(job, 0, J - 1), np.clip(mach, 0, M - 1)
                task = cand[rows, jc].astype(np.int32)
                legal = in_range & (mask[rows, jc] == 0) & self.feas[rows, task, mc]
                mm = ~self.feas[rows, task]
                out = dict(task=task, legal=legal, w3=w3,
                           tasks_fea=obs(o["tfea"]), ell_col=o["ell_col"].reshape(B * T, 2), ell_val=o["ell_val"].reshape(B * T, 2),
                           candidate=cand.astype(np.int32), mask_operation=mask.astype(bool), machine_fea2=obs(o["mfea2"]),
                           machine_fea1=obs(orc.mfea1(task, mm, o["tfea"])), mask_machine_=mm.reshape(B, 1, M),
                           random_weight=w3.astype(np.float32))
                if not legal.all():
                    yield out
                    return
                info, _, _ = orc.step(task, mach.astype(np.int32))
                cand, mask = orc.job_mask_update(job.astype(np.int32))
                o = orc.observe(dense=False)
                out.update(tasks_fea_=obs(o["tfea"]), ell_col_=o["ell_col"].reshape(B * T, 2), ell_val_=o["ell_val"].reshape(B * T, 2),
                           candidate_=cand.astype(np.int32), mask_operation_=mask.astype(bool), machine_fea2_=obs(o["mfea2"]),
                           r_operation=info[:, 0].astype(np.float32), done_operation=info[:, 1].astype(np.float32),
                           r4=np.ascontiguousarray(info[:, 2:6].T).astype(np.float32))
                yield out
            assert info[:, 1].all(), "the oracle's episode must be over after T steps"

    def record(self, a_operation, a, episodes, weights=None):
        """the whole buffer: dict of FIELDS with a leading slot axis, plus a_operation / a, `legal` and `term_mask` [episodes, B, J]"""
        out = [x for x in self.slots(a_operation, a, episodes, weights)]
        assert all(x["legal"].all() for x in out), "an illegal recorded action"
        rec = {k: np.stack([x[k] for x in out]) for k in FIELDS + ("legal",)}
        rec["a_operation"], rec["a"] = np.asarray(a_operation).astype(np.int32), np.asarray(a).astype(np.int32)
        rec["term_mask"] = rec["mask_operation"][self.T - 1::self.T].copy()
        return rec


def reference_tuple(rec):
    """the environment-side entries of the reference ReplayBuffer's 27-tuple from a record, by TUPLE_NAMES, in the dtypes
    numpy_to_tensor_operation casts to (float32 / int64 / bool); adj / adj_ dense float32 [S, B, T, T]"""
    S, B, J = rec["candidate"].shape
    T = rec["tasks_fea"].shape[1] // B
    f = np.float32

    def dense(col, val):
        out = np.zeros((S, B, T, T), f)
        out[:, :, np.arange(T), np.arange(T)] = 1
        c, v = col.reshape(S, B, T, 2), val.reshape(S, B, T, 2)
        for k in range(2):
            si, bi, ti = np.nonzero(c[..., k] >= 0)
            out[si, bi, ti, c[si, bi, ti, k]] = v[si, bi, ti, k]
        return out

    return dict(adj=dense(rec["ell_col"], rec["ell_val"]), tasks_fea=rec["tasks_fea"].astype(f), candidate=rec["candidate"].astype(np.int64),
                mask_operation=rec["mask_operation"], a_operation=rec["a_operation"].astype(np.int64),
                adj_=dense(rec["ell_col_"], rec["ell_val_"]), tasks_fea_=rec["tasks_fea_"].astype(f), candidate_=rec["candidate_"].astype(f),
                mask_operation_=rec["mask_operation_"], r_operation=rec["r_operation"], done_operation=rec["done_operation"],
                machine_fea2=rec["machine_fea2"].astype(f), a=rec["a"].astype(np.int64), machine_fea2_=rec["machine_fea2_"].astype(f),
                mask_machine_=rec["mask_machine_"], mk=rec["r4"][:, 0], pt=rec["r4"][:, 2], tt=rec["r4"][:, 3], it=rec["r4"][:, 1],
                machine_fea1=rec["machine_fea1"].astype(f), rw=rec["random_weight"])


# ------------------------------------------------------------------------------------------------------------- the comparator
def compare_slot(got, want, s):
    """one slot of a record (dict of FIELDS, no slot axis) against the model's: legal actions, then every field with env_parity._same,
    the adjacency as sets of rows; an AssertionError names the field and the slot"""
    assert want["legal"].all(), f"slot {s}: the recorded action of instance {int(np.argmin(want['legal']))} is not legal (job masked or machine infeasible)"
    for k in FIELDS:
        if k.startswith("ell_"):
            continue
        assert k in want, f"slot {s}: the model has no {k} (the replay ended early)"
        _same(got[k], want[k], f"slot {s} {k}")
    for ck, vk in ELL_FIELDS:
        g, w = ell_rows(got[ck], got[vk]), ell_rows(want[ck], want[vk])
        _same(g[0], w[0], f"slot {s} {ck} (rows as sets)")
        _same(g[1], w[1], f"slot {s} {vk} (rows as sets)")


def compare_record(got, want):
    """every slot of a whole record (leading slot axis) against a model record, then the masks the terminal forwards were given"""
    S = want["candidate"].shape[0]
    for s in range(S):
        compare_slot({k: got[k][s] for k in FIELDS}, {k: want[k][s] for k in FIELDS + ("legal",)}, s)
    T = S // want["term_mask"].shape[0]
    for e in range(want["term_mask"].shape[0]):
        _same(got["term_mask"][e], want["term_mask"][e], f"slot {e * T + T - 1} term_mask (the job mask of the post-terminal forward)")


# ------------------------------------------------------------------------------------------------------------- the network half
def slot_forward(ja, ma, slot, h_m_prev, h_o=None, dtype=torch.float32):
    """both actors on one slot's own fields.  h_m_prev [B, H]: the machine embedding of the previous step (None: an episode's first
    step, the learned `_input`); h_o [B, H]: the job embedding the machine actor reads (None: this evaluation's own).
    -> (job actor's dict, machine actor's dict) of oracle.encoder_oracle"""
    from oracle import encoder_oracle as eo
    B, J = slot["candidate"].shape
    M = slot["mask_machine_"].shape[-1]
    T = slot["tasks_fea"].shape[0] // B
    job = eo.job_actor_forward(ja, slot["tasks_fea"], slot["ell_col"], slot["ell_val"], slot["candidate"], slot["mask_operation"], h_m_prev, B, T, dtype=dtype)
    mach = eo.machine_actor_forward(ma, slot["machine_fea1"], slot["machine_fea2"], job["h_pooled"] if h_o is None else h_o, slot["mask_machine_"], B, M, dtype=dtype)
    return job, mach


def terminal_pair(ja, ma, last, h_m_last, dtype=torch.float32, job_mask=None):
    """the post-terminal pair (Run.py:455-475, ActorPair.terminal_values) on an episode's LAST slot: the job forward on the
    post-decision observation and candidates under the slot's PRE-decision job mask with the last machine embedding; the machine
    forward on the slot's m_fea1 and machine mask with the post-decision m_fea2 and that job forward's embedding.
    job_mask: another mask for the job forward (the slip tests).  -> (job actor's dict, machine actor's dict)"""
    from oracle import encoder_oracle as eo
    B, J = last["candidate"].shape
    M = last["mask_machine_"].shape[-1]
    T = last["tasks_fea"].shape[0] // B
    mask = last["mask_operation"] if job_mask is None else job_mask
    with np.errstate(invalid="ignore"):
        job = eo.job_actor_forward(ja, last["tasks_fea_"], last["ell_col_"], last["ell_val_"], last["candidate_"], mask, h_m_last, B, T, dtype=dtype)
    mach = eo.machine_actor_forward(ma, last["machine_fea1"], last["machine_fea2_"], job["h_pooled"], last["mask_machine_"], B, M, dtype=dtype)
    return job, mach


def record_network(ja, ma, rec, dtype=torch.float32):
    """the network half of a whole record, every embedding the model's own: dict of job_prob [S, B, J], mch_prob [S, B, M], h_o, h_m,
    job_v, machine_v, job_v_, machine_v_ [S, B, 2] (v_ of a slot = v of the next one, the terminal pair's at an episode's end),
    term_job_v_, term_machine_v_ [episodes, B, 2] and the log-probabilities of the recorded actions"""
    S, B, _ = rec["candidate"].shape
    eps = rec["term_mask"].shape[0]
    T = S // eps
    rows = np.arange(B)
    out = {k: [] for k in ("job_prob", "mch_prob", "h_o", "h_m", "job_v", "machine_v", "term_job_v_", "term_machine_v_")}
    for s in range(S):
        slot = {k: rec[k][s] for k in FIELDS}
        job, mach = slot_forward(ja, ma, slot, None if s % T == 0 else out["h_m"][-1], dtype=dtype)
        for k, v in (("job_prob", job["prob"]), ("mch_prob", mach["prob"]), ("h_o", job["h_pooled"]), ("h_m", mach["h_pooled"]), ("job_v", job["job_v"]),
                     ("machine_v", mach["mach_v"])):
            out[k].append(v)
        if s % T == T - 1:
            tj, tm = terminal_pair(ja, ma, slot, mach["h_pooled"], dtype=dtype, job_mask=rec["term_mask"][s // T])
            out["term_job_v_"].append(tj["job_v"]); out["term_machine_v_"].append(tm["mach_v"])
    out = {k: np.stack(v) for k, v in out.items()}
    for v, v_, term in (("job_v", "job_v_", "term_job_v_"), ("machine_v", "machine_v_", "term_machine_v_")):
        nxt = np.concatenate([out[v][1:], out[v][:1]])
        nxt[T - 1::T] = out[term]
        out[v_] = nxt
    with np.errstate(divide="ignore"):
        out["a_logprob_operation"] = np.log(out["job_prob"][np.arange(S)[:, None], rows, rec["a_operation"]]).astype(np.float32)
        out["a_logprob"] = np.log(out["mch_prob"][np.arange(S)[:, None], rows, rec["a"]]).astype(np.float32)
    return out


def compare_network(got, net, rec, bounds, slots=None):
    """the stored network half of a record against an evaluation (record_network's dict, or the same keys on the listed slots only):
    exp(a_logprob*) against the probability of the recorded action (absolute), the four value fields elementwise / (1 + |expected|);
    bounds: dict field -> bound.  An AssertionError names the field and the slot.  -> dict field -> worst figure"""
    S, B = rec["a_operation"].shape
    rows = np.arange(B)
    worst = {}
    for s in (range(S) if slots is None else slots):
        for k, pk, ak in (("a_logprob_operation", "job_prob", "a_operation"), ("a_logprob", "mch_prob", "a")):
            want = np.asarray(net[pk][s], np.float64)[rows, rec[ak][s]]
            err = np.abs(np.exp(np.asarray(got[k][s], np.float64)) - want).max()
            assert err <= bounds[k], f"slot {s} {k}: exp(stored) is {err:.3e} from the probability of the recorded action (bound {bounds[k]:.3e})"
            worst[k] = max(worst.get(k, 0.0), float(err))
        for k in ("job_v", "machine_v", "job_v_", "machine_v_"):
            want = np.asarray(net[k][s], np.float64)
            err = (np.abs(np.asarray(got[k][s], np.float64) - want) / (1.0 + np.abs(want))).max()
            assert err <= bounds[k], f"slot {s} {k}: {err:.3e} from the model (bound {bounds[k]:.3e})"
            worst[k] = max(worst.get(k, 0.0), float(err))
    return worst

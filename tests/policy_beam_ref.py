"""Host models of the policy-guided beam search (plain module; tests/test_policy_beam_cpu.py pins them on hand-written rows,
tests/test_beam_select_policy_gpu.py and tests/test_policy_beam_gpu.py hold the device to them).  The rules of include/mtfjsp.h
(mtfjsp_beam_select_policy, mtfjsp_beam_merge_slots) are applied literally, candidate by candidate, in Python: comparisons, and per
candidate the two binary64 additions (score + log p(job)) + log p(machine | job) in that order.  The whole-search model does not
run the actors: it is handed every decision's logarithms, masks, candidates and signatures as the device produced them, and
answers what the selection, the merge and the back-pointers must then be.
"""
import numpy as np

NEG = -np.inf


def values(score, logp_job, logp_mach):
    """score [S], logp_job [S,J], logp_mach [S,J,M] (f64) -> [S,J,M]: (score + logp_job) + logp_mach, two additions in this order"""
    score, logp_job, logp_mach = (np.asarray(x, np.float64) for x in (score, logp_job, logp_mach))
    with np.errstate(invalid="ignore"):
        return (score[:, None] + logp_job)[:, :, None] + logp_mach


def select(score, logp_job, logp_mach, job_mask, mmask, W):
    """the selection for ONE source instance: score [W], logp_job [W,J], logp_mach [W,J,M], job_mask [W,J], mmask [W,J,M]
    -> list of W picks, each (w, j, m, value) or None (a rank left without a candidate)"""
    v = values(score, logp_job, logp_mach)
    _, J, M = v.shape
    alive = []
    for w in range(W):
        for j in range(J):
            for m in range(M):
                x = v[w, j, m]
                if score[w] != NEG and job_mask[w, j] == 0 and mmask[w, j, m] == 0 and x == x and x != NEG:
                    alive.append((w, j, m))                                  # ascending c = w*T + j*M + m
    picks = []
    for _ in range(W):
        if not alive:
            picks.append(None)
            continue
        best = alive[0]
        for c in alive[1:]:
            if v[c] > v[best]:                                              # the lowest c among equals stays
                best = c
        picks.append(best + (v[best],))
        alive.remove(best)
    return picks


def select_batch(score, logp_job, logp_mach, job_mask, mmask, candidate, W):
    """N source instances: score [N*W], logp_job [N*W,J], logp_mach [N*W*J,M], job_mask [N*W,J], mmask [N*W*J,M], candidate [N*W,J]
    (the task of an unfinished job's next operation: what the device forms from its job records) -> dict of the seven outputs [N*W]"""
    NW, J = logp_job.shape
    M = logp_mach.shape[-1]
    N = NW // W
    lm, mm = np.asarray(logp_mach).reshape(NW, J, M), np.asarray(mmask).reshape(NW, J, M)
    out = {k: np.full(NW, -1, np.int32) for k in ("parent", "from_slot", "job", "task", "mach", "child")}
    out["score"] = np.full(NW, NEG)
    for n in range(N):
        sl = slice(n * W, (n + 1) * W)
        for k, pick in enumerate(select(np.asarray(score)[sl], np.asarray(logp_job)[sl], lm[sl], np.asarray(job_mask)[sl], mm[sl], W)):
            if pick is None:
                continue
            w, j, m, x = pick
            i, slot = n * W + k, n * W + w
            out["parent"][i], out["from_slot"][i], out["job"][i], out["mach"][i] = slot, w, j, m
            out["task"][i], out["child"][i], out["score"][i] = candidate[slot, j], slot * J + j, x
    return out


def merge(sig, score, W):
    """sig [N*W] uint64, score [N*W] f64 -> the merged scores: slot k is emptied iff a slot k' < k of its source has its signature
    and had a score other than -inf on entry"""
    sig, score = np.asarray(sig).view(np.uint64), np.asarray(score, np.float64)
    out = score.copy()
    for i in range(len(score)):
        lo = i - i % W
        if any(sig[q] == sig[i] and score[q] != NEG for q in range(lo, i)):
            out[i] = NEG
    return out


class Search:
    """the whole search: scores, back-pointers and plans, decision by decision from the device's own per-decision tensors"""

    def __init__(self, N, W, dedupe):
        self.N, self.W, self.dedupe = N, W, dedupe
        self.score = np.where(np.arange(N * W) % W == 0, 0.0, NEG)
        self.prefix = [[] if i % W == 0 else None for i in range(N * W)]
        self.rows = []

    def decide(self, logp_job, logp_mach, job_mask, mmask, candidate, sig_next=None):
        """-> the decision's record: the seven outputs of the selection ("score": as selected) and "merged": the scores after the merge
        (sig_next [N*W]: the signatures of the stepped children; needed with dedupe)"""
        rec = select_batch(self.score, logp_job, logp_mach, job_mask, mmask, candidate, self.W)
        rec["merged"] = merge(sig_next, rec["score"], self.W) if self.dedupe else rec["score"].copy()
        self.prefix = [None if rec["parent"][i] < 0 else self.prefix[rec["parent"][i]] + [(int(rec["task"][i]), int(rec["mach"][i]))]
                       for i in range(self.N * self.W)]
        self.score = rec["merged"]
        self.rows.append(rec)
        return rec

    def plan(self, slot):
        """(task, mach) lists of slot [N] -> arrays [N,s], -1 rows for an empty slot"""
        s = len(self.rows)
        task, mach = np.full((self.N, s), -1, np.int32), np.full((self.N, s), -1, np.int32)
        for n in range(self.N):
            x = self.prefix[n * self.W + int(slot[n])] if 0 <= slot[n] < self.W else None
            if x is not None:
                task[n], mach[n] = [a for a, _ in x], [m for _, m in x]
        return task, mach

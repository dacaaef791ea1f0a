"""Per-instance BatchNorm mode (Encoder.set_bn_mode(True): k_gin_inst and k_gat_inst, one workgroup per instance) at the machine counts
where k_gat_inst's code changes, to the bit and against binary64.  It is the path behind validate_cost_batched and sample_best_of_k.

k_gat_inst puts the 2 M (machine, node) rows of an instance into tiles of 16, one tile per wave; k_gin_inst walks ceil(T / 16) tiles with 8 waves:

  (3, 8, 2) x 11    2 M = 16: exactly one full GAT tile; T = 24
  (5, 9, 3) x 19    a second GAT tile with two live rows; T = 45, a ragged GIN tile; 19 instances: a ragged last group in the heads
  (7, 16, 2) x 9    two full GAT tiles; T = 112
  (2, 17, 1) x 9    three GAT waves: the first shape whose BatchNorm sums and pooled mean have more than two contributions; T = 34
  (3, 33, 3) x 6    five GAT waves, the last tile with two live rows; T = 99
  (9, 17, 1) x 10   T = 153: more than 8 GIN tiles (some waves take two), ragged
  (20, 20, 4) x 5   the BASELINE shape: T = 400, three GAT waves

(The number of edges E only shapes the instances — it has to divide M, instances.generate_instances — and does not reach the encoder.)
Inputs come from min(12, T // 3) rollout steps on the device with perturbed BatchNorm affine parameters; the machine-side inputs are the
environment's observation of the float32 oracle's greedy task.  The references are per instance (B = 1 calls of oracle/encoder_oracle.py) in
float32 and in binary64, computed once per case and shared.  Two sizes run with binary64 observations as well.

a. Run to run: eight forwards on one handle and one on a second handle with the same weights are one set of bits.  Every sum across waves or
   row groups in the two kernels is a fold of per-contributor partial sums in index order; floating-point atomics would make three or more
   contributions (M >= 17, any T in k_gin_inst) depend on the order in which the waves arrive.
b. A copy does not see its neighbours: the same instances gathered into other slots, instance 0 in several of them (two in one heads group, one
   in the next, one in the ragged last group), give every slot the bits its instance had in the unpermuted forward — kernel outputs and the
   heads' outputs alike.
c. Accuracy: tests/error_budget.check under max(hard cap of the tensor class, 2 x the float32 oracle's own distance from binary64 on the same
   inputs), the rule of tests/test_encoder_limits_gpu.py (_held); nothing is derived from the kernels' output.  The figures of a GPU run are in
   profiles/r05_encoder_errors.json under "per_instance:...".
"""
import functools
from importlib import import_module
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from test_encoder_limits_gpu import _held, _perturb

pytestmark = pytest.mark.gpu

SIZES = [(3, 8, 2, 11), (5, 9, 3, 19), (7, 16, 2, 9), (2, 17, 1, 9), (3, 33, 3, 6), (9, 17, 1, 10), (20, 20, 4, 5)]
F64_OBS = [(5, 9, 3, 19), (2, 17, 1, 9)]
CASES = [(s, "f32") for s in SIZES] + [(s, "f64") for s in F64_OBS]
RUNS = 8
OUTPUTS = ("prob", "h_pooled", "job_v", "h_nodes", "mprob", "h_pooled_m", "mach_v")


def _case_id(c):
    return "J%dM%dE%d-B%d" % c[0] + ("-f64obs" if c[1] == "f64" else "")


def _mods():
    import mtfjsp_amd  # noqa: F401
    return import_module("e2e-mappo-for-mt-fjsp_amd.encoder"), import_module("e2e-mappo-for-mt-fjsp_amd.rollout")


@functools.lru_cache(maxsize=None)
def _case(size, obs):
    """the rollout after min(12, T // 3) policy steps, device copies of what the two forwards read, and the per-instance references (float32
    oracle, binary64): computed once, read by every test of the case and never written"""
    enc_mod, rollout = _mods()
    from oracle import encoder_oracle as eo
    J, M, E, B = size
    T = J * M
    ja, ma = enc_mod.random_init_weights(seed=J * 100 + M)
    _perturb((ja, ma), 3)
    ro = rollout.Rollout(J, M, E, B, policy="actor", obs_dtype=obs, weights=(ja, ma), collect=False)
    for _ in range(min(12, T // 3)):
        ro.step()
    env, e = ro.env, ro.actor.enc
    torch.cuda.synchronize()
    c = SimpleNamespace(size=size, obs=obs, ro=ro, e=e, weights=(ja, ma), name="per_instance:%dx%dx%dx%d" % size + (":f64obs" if obs == "f64" else ""))
    inp = dict(tfea=env.tasks_fea.clone().view(B, T, 12), col=env.ell_col.clone().view(B, T, 2), val=env.ell_val.clone().view(B, T, 2),
               cand=env.candidate.clone().view(B, J), mask=env.job_mask.clone().view(B, J), hm=e.h_pooled_m.clone().view(B, 128))
    tf = inp["tfea"].cpu().numpy().reshape(B * T, 12)
    col, val = inp["col"].cpu().numpy(), inp["val"].cpu().numpy()
    cand, mask, hm = inp["cand"].cpu().numpy(), inp["mask"].cpu().numpy(), inp["hm"].cpu().numpy()

    def per_instance(fn, keys):
        outs = [fn(b) for b in range(B)]
        return {k: np.concatenate([x[k] for x in outs], 0) for k in keys}

    c.job = {dt: per_instance(lambda b: eo.job_actor_forward(ja, tf[b * T:(b + 1) * T], col[b:b + 1], val[b:b + 1], cand[b:b + 1], mask[b:b + 1], hm[b:b + 1], 1, T, dtype=dt),
                              ("prob", "h_nodes", "h_pooled", "job_v")) for dt in (torch.float32, torch.float64)}
    # the machine actor on the task each instance picks greedily by the float32 oracle, with the oracle's pooled embedding as its input
    o = c.job[torch.float32]
    task = torch.as_tensor(cand[np.arange(B), o["prob"].argmax(1)].astype(np.int32)).cuda()
    env.observe_mfea1(task)
    torch.cuda.synchronize()
    inp.update(f1=env.m_fea1.clone().view(B, M, 6), f2=env.m_fea2.clone().view(B, M, 8), mmask=env.mmask.clone().view(B, M), h_o=torch.as_tensor(o["h_pooled"]).cuda())
    f1, f2, mm = inp["f1"].cpu().numpy(), inp["f2"].cpu().numpy(), inp["mmask"].cpu().numpy()
    c.mach = {dt: per_instance(lambda b: eo.machine_actor_forward(ma, f1[b:b + 1], f2[b:b + 1], o["h_pooled"][b:b + 1], mm[b:b + 1], 1, M, dtype=dt), ("prob", "h_pooled", "mach_v"))
              for dt in (torch.float32, torch.float64)}
    c.inp = inp
    return c


def _forward(e, c, inp):
    """the job forward (with node embeddings) and the machine forward of handle e in per-instance mode -> copies of the seven outputs"""
    J, M, E, B = c.size
    T = J * M
    h_nodes = torch.zeros(B * T, 128, dtype=torch.float32, device="cuda")
    prob, h_o, job_v = e.job_actor_forward(inp["tfea"], inp["col"], inp["val"], inp["cand"], inp["mask"], inp["hm"], h_nodes=h_nodes)
    torch.cuda.synchronize()
    plan = e.gin_launches()
    assert plan["path"] == "per_instance", plan
    out = dict(prob=prob.clone(), h_pooled=h_o.clone(), job_v=job_v.clone(), h_nodes=h_nodes.view(B, T, 128))
    mprob, h_m, mach_v = e.machine_actor_forward(inp["f1"], inp["f2"], inp["h_o"], inp["mmask"])
    torch.cuda.synchronize()
    out.update(mprob=mprob.clone(), h_pooled_m=h_m.clone(), mach_v=mach_v.clone())
    assert e.range_fallbacks()[0] == 0
    return out


def _ulps(a, b):
    """largest distance of two float32 tensors in units of the last place (diagnostic of a failed bit comparison)"""
    def key(x):
        i = x.detach().cpu().contiguous().numpy().view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return int(np.abs(key(a) - key(b)).max())


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_run_to_run_one_set_of_bits(case):
    c = _case(*case)
    J, M, E, B = c.size
    enc_mod, _ = _mods()
    e = c.e
    e2 = enc_mod.Encoder(J, M, B, obs_dtype=c.obs)
    e2.load_weights(*c.weights)
    e.set_bn_mode(True); e2.set_bn_mode(True)
    try:
        first = _forward(e, c, c.inp)
        runs = [("run %d" % (i + 2), _forward(e, c, c.inp)) for i in range(RUNS - 1)] + [("second handle", _forward(e2, c, c.inp))]
        bad = ["%s %s: %d ulps" % (tag, k, _ulps(o[k], first[k])) for tag, o in runs for k in OUTPUTS if not torch.equal(o[k], first[k])]
        assert not bad, (c.name, bad)
    finally:
        e.set_bn_mode(False)
        e2.close()


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_a_copy_does_not_see_its_neighbours(case):
    """instance 0 in slots 0 and 7 (one heads group), 8 (the next group) and B - 1 (the ragged last group) where B allows, the other slots a
    permutation of other instances: every output row of a slot is, bit for bit, the row its instance had in the unpermuted forward (the
    copies of instance 0 therefore equal each other).  Probabilities and values are compared, sampled indices are not: the sampler is
    keyed by the slot."""
    c = _case(*case)
    J, M, E, B = c.size
    e = c.e
    copies = sorted({s for s in (0, 7, 8, B - 1) if s < B})
    assert len(copies) >= 2
    rest = [s for s in range(B) if s not in copies]
    src = np.zeros(B, np.int64)
    for seed in range(100):                                          # the first permutation that leaves none of the other slots its own instance
        src[rest] = np.random.RandomState(seed).permutation(np.arange(1, B))[:len(rest)]
        if (src[rest] != np.asarray(rest)).all():
            break
    assert (src[copies] == 0).all() and len(set(src.tolist())) == len(rest) + 1 and (src[rest] != np.asarray(rest)).all()
    idx = torch.as_tensor(src).cuda()
    moved = {k: v.index_select(0, idx).contiguous() for k, v in c.inp.items()}
    e.set_bn_mode(True)
    try:
        plain = _forward(e, c, c.inp)
        perm = _forward(e, c, moved)
        bad = []
        for k in OUTPUTS:
            want = plain[k].index_select(0, idx)
            if not torch.equal(perm[k], want):
                rows = sorted({int(r) for r in (perm[k] != want).nonzero()[:, 0].cpu()})
                bad.append("%s: slots %s, %d ulps" % (k, rows, _ulps(perm[k], want)))
        assert not bad, (c.name, src.tolist(), bad)
        for k in OUTPUTS:
            for s in copies[1:]:
                assert torch.equal(perm[k][s], perm[k][copies[0]]), (c.name, k, s)
    finally:
        e.set_bn_mode(False)


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_accuracy_against_binary64(case):
    c = _case(*case)
    e = c.e
    f32, f64 = torch.float32, torch.float64
    e.set_bn_mode(True)
    try:
        out = _forward(e, c, c.inp)
    finally:
        e.set_bn_mode(False)
    J, M, E, B = c.size
    o, o64, mo, mo64 = c.job[f32], c.job[f64], c.mach[f32], c.mach[f64]
    scale = max(1.0, float(np.abs(o["h_nodes"]).max()))
    mscale = max(1.0, float(np.abs(mo["h_pooled"]).max()))
    failed = []
    for tensor, hip, a, b, s in (("h_nodes", out["h_nodes"].reshape(B * J * M, 128), o["h_nodes"], o64["h_nodes"], scale),
                                 ("h_pooled_o", out["h_pooled"], o["h_pooled"], o64["h_pooled"], scale),
                                 ("job_prob", out["prob"], o["prob"], o64["prob"], None), ("job_v", out["job_v"], o["job_v"], o64["job_v"], None),
                                 ("mch_prob", out["mprob"], mo["prob"], mo64["prob"], None), ("h_pooled_m", out["h_pooled_m"], mo["h_pooled"], mo64["h_pooled"], mscale),
                                 ("mach_v", out["mach_v"], mo["mach_v"], mo64["mach_v"], None)):
        try:                                                         # every tensor is measured and printed before the case fails
            _held(c.name, tensor, hip, a, b, s)
        except AssertionError as ex:
            failed.append(str(ex))
    assert not failed, failed
    p, mp = out["prob"].cpu().numpy(), out["mprob"].cpu().numpy()
    assert (p[c.inp["mask"].cpu().numpy() != 0] == 0).all() and np.allclose(p.sum(1), 1.0, atol=1e-5)
    assert (mp[c.inp["mmask"].cpu().numpy() != 0] == 0).all() and np.allclose(mp.sum(1), 1.0, atol=1e-5)

"""Shared pieces of the weight-reload tests (tests/test_weight_reload_cpu.py, tests/test_weight_reload_gpu.py): inputs, weight sets, a
per-key perturbation, the list of tensors no output depends on, the oracle evaluation of every forward and the comparison rule.

The CPU test proves, in binary64, that every tensor outside UNOBSERVABLE moves at least one compared output by 1e-3 of its scale on these
inputs, alone (perturb) and between the two whole sets; the GPU tests hold a reloaded handle to 2e-6 of the same scale, so a derived image
that was not refreshed shows at 500 times the bound.  Test infrastructure only.
"""
import os
import zlib

import numpy as np

from error_budget import normalised

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
H = 128
PREFIXES = ("job_actor.", "machine_actor.", "global_critic.")
# compared outputs per forward ("first": job actor with h_m_prev = None, the learned `_input` row; "later": with a given h_m_prev)
FORWARDS = {"first": ("prob", "h_pooled_o", "job_v"), "later": ("prob", "h_pooled_o", "job_v"),
            "machine": ("mch_prob", "h_pooled_m", "mach_v"), "critic": ("global_v",)}
OBSERVABLE_AT = 1e-3          # least normalised change of an output that counts as "this tensor is read"
RELOAD_BOUND = 2e-6           # reloaded handle against a fresh one: summation-order noise (tests/test_encoder_sizes_gpu.py)

_GIN_BIASES = [f"encoder.feature_extract.mlps.{l}.linears.{i}.bias" for l in range(2) for i in range(3)]
# Tensors no compared output depends on — mathematically, not by accident of these inputs:
#   * a Linear bias in front of a training-mode BatchNorm cancels in (x - mean) (the six GIN Linears of each encoder);
#   * the last bias of a policy head shifts every score of a softmax alike;
#   * fcl_pooling.weight and encoder.feature_extract.bn.* belong to modules the reference's forwards never call (ac:357, gcn:66);
#   * `_input` is read only when h_m_prev is None: the entry with the "[later]" suffix names that form alone.
UNOBSERVABLE = sorted(
    ["job_actor." + k for k in _GIN_BIASES] + ["global_critic." + k for k in _GIN_BIASES] +
    ["job_actor.o_policy.linears.2.bias", "machine_actor.m_policy.linears.2.bias",
     "machine_actor.fcl_pooling.weight", "global_critic.fcl_pooling.weight",
     "job_actor.encoder.feature_extract.bn.weight", "job_actor.encoder.feature_extract.bn.bias",
     "global_critic.encoder.feature_extract.bn.weight", "global_critic.encoder.feature_extract.bn.bias",
     "job_actor._input[later]"])
# keys whose effect is small under the common perturbation — the global critic's attention vector and first projection (4 outputs behind two tanh
# layers), the job scorer's hidden biases (U(+-0.05) beside 384 and 128 products) and `_input` — get a stronger one, chosen on the CPU until
# OBSERVABLE_AT holds with a margin (tests/test_weight_reload_cpu.py prints the figures)
STRONG = ("global_critic.gat_layer.a", "global_critic.m_fea_1_fcl.weight", "job_actor.o_policy.linears.0.bias", "job_actor.o_policy.linears.1.bias",
          "job_actor._input")


def forwards_reading(key):
    """the forwards whose outputs depend on this (prefixed) tensor"""
    if key.startswith("machine_actor."):
        return ("machine",)
    if key.startswith("global_critic."):
        return ("critic",)
    return ("first",) if key == "job_actor._input" else ("first", "later")


def fixture_inputs():
    """J6M6E2 x 8: step 0 of tests/golden/encoder_j6m6e2_rand.npz (every job unmasked; step 9 has one-hot probabilities) + a synthetic h_m_prev"""
    from oracle import encoder_oracle as eo
    g = np.load(os.path.join(GOLDEN, "encoder_j6m6e2_rand.npz"))
    J, M, E, B = [int(x) for x in g["meta"]]
    T = J * M
    col, val = eo.ell_from_dense(g["s0_adj"])
    inp = dict(J=J, M=M, B=B, T=T, tfea=g["s0_tfea"].reshape(B * T, 12).astype(np.float32), col=col.astype(np.int32), val=val.astype(np.float32),
               cand=g["s0_cand"].astype(np.int32), mask=g["s0_mask"].astype(np.uint8), mfea1=g["s0_mfea1"].reshape(B, M, 6).astype(np.float32),
               mfea2=g["s0_mfea2"].reshape(B, M, 8).astype(np.float32), mmask=g["s0_mmask"].reshape(B, M).astype(np.uint8),
               h_o=g["s0_h_o"].astype(np.float32), hm=np.random.RandomState(11).uniform(-1, 1, (B, H)).astype(np.float32))
    check_inputs(inp)
    return inp


def synthetic_inputs(J=10, M=10, B=5, seed=5):
    """a shape the single-launch GIN kernel does not take (T = 100 > 65: streaming launches, 500 rows = 15 row tiles + 20 rows): random features in
    the environment's layout — job-chain and machine in-edges, candidates inside their job's block of rows, some jobs and machines masked"""
    rs = np.random.RandomState(seed)
    T = J * M
    col = -np.ones((B, T, 2), np.int32); val = np.zeros((B, T, 2), np.float32)
    for b in range(B):
        for v in range(T):
            if v % M:
                col[b, v, 0] = v - 1; val[b, v, 0] = 1.0                                   # previous operation of the job
            if rs.rand() < 0.5:
                u = rs.randint(T)
                if u != v and u != col[b, v, 0]:
                    col[b, v, 1] = u; val[b, v, 1] = 1.0                                   # previous operation on the machine
    mask = (rs.rand(B, J) < 0.3); mask[:, :3] = False
    mmask = (rs.rand(B, M) < 0.3); mmask[:, :2] = False
    inp = dict(J=J, M=M, B=B, T=T, tfea=rs.uniform(0, 1, (B * T, 12)).astype(np.float32), col=col, val=val,
               cand=(np.arange(J)[None, :] * M + rs.randint(0, M, (B, J))).astype(np.int32), mask=mask.astype(np.uint8),
               mfea1=rs.uniform(0, 1, (B, M, 6)).astype(np.float32), mfea2=rs.uniform(0, 1, (B, M, 8)).astype(np.float32),
               mmask=mmask.astype(np.uint8), h_o=rs.uniform(-1, 1, (B, H)).astype(np.float32), hm=rs.uniform(-1, 1, (B, H)).astype(np.float32))
    check_inputs(inp)
    return inp


def check_inputs(inp):
    """the condition under which the policy heads are observable: a softmax over one unmasked entry is 1 whatever the weights"""
    assert ((inp["mask"] == 0).sum(1) >= 3).all(), "every instance needs at least 3 unmasked jobs"
    assert ((inp["mmask"] == 0).sum(1) >= 2).all(), "every instance needs at least 2 unmasked machines"


def _with_unused_modules(ja, ma, gc, rs):
    """the tensors of a reference checkpoint that no forward reads (the library accepts and stores them)"""
    for d in (ja, gc):
        d["encoder.feature_extract.bn.weight"] = rs.uniform(0.5, 1.5, 12).astype(np.float32)
        d["encoder.feature_extract.bn.bias"] = rs.uniform(-0.5, 0.5, 12).astype(np.float32)
    for d in (ma, gc):
        d["fcl_pooling.weight"] = rs.uniform(-0.1, 0.1, (H, H)).astype(np.float32)


def _perturb_bn(dicts, seed):
    """non-trivial BatchNorm affine parameters (the default initialiser has gamma 1 / beta 0), as tests/test_encoder_sizes_gpu.py"""
    rs = np.random.RandomState(seed)
    for d in dicts:
        for k in d:
            if "batch_norms" in k or k.startswith("bn."):
                d[k] = (rs.uniform(0.5, 1.5, d[k].shape) if k.endswith("weight") else rs.uniform(-0.5, 0.5, d[k].shape)).astype(np.float32)


def weight_sets():
    """-> (W1, W2), each (job actor, machine actor, global critic) under the reference's state_dict keys.  W2: another seed, and every 128-wide
    Linear weight and gat_layer.W scaled by 0.3 / 3 alternately: max |W| lands in another binade, so the power-of-two scale of the f16 operand
    images and its inverse on the host change with the reload"""
    from importlib import import_module
    import mtfjsp_amd  # noqa: F401
    enc_mod = import_module("e2e-mappo-for-mt-fjsp_amd.encoder")
    sets = []
    for seed, bn_seed in ((101, 3), (202, 7)):
        w = [dict(d) for d in enc_mod.random_init_weights(seed, with_critic=True)]
        _perturb_bn(w, bn_seed)
        _with_unused_modules(*w, np.random.RandomState(seed))
        sets.append(tuple(w))
    n = 0
    for d in sets[1]:
        for k in sorted(d):
            if (k.endswith(".weight") and "linears" in k and d[k].size % (H * H) == 0) or k == "gat_layer.W":
                d[k] = (d[k] * (0.3 if n % 2 == 0 else 3.0)).astype(np.float32)
                n += 1
    assert n >= 20
    return sets[0], sets[1]


def all_keys(w):
    return [p + k for p, d in zip(PREFIXES, w) for k in d]


def get(w, key):
    p = next(p for p in PREFIXES if key.startswith(p))
    return w[PREFIXES.index(p)][key[len(p):]]


def replaced(w, key, value):
    """a copy of the set with one (prefixed) tensor replaced"""
    p = next(p for p in PREFIXES if key.startswith(p))
    out = [dict(d) for d in w]
    out[PREFIXES.index(p)][key[len(p):]] = np.asarray(value, np.float32)
    return tuple(out)


def perturb(key, value):
    """a tensor clearly different from `value` and from any other key's perturbation: x 1.5 plus noise of a quarter of its r.m.s. (deterministic per
    key; an all-zero tensor counts as r.m.s. 0.1); the STRONG keys: sign flipped, x 2, plus noise of four times its r.m.s."""
    rs = np.random.RandomState(zlib.crc32(key.encode()) & 0x7fffffff)
    v = np.asarray(value, np.float32)
    rms = max(float(np.sqrt(np.mean(np.square(v.astype(np.float64))))), 0.1)
    if key in STRONG:
        return (-2.0 * v + 4.0 * rms * rs.standard_normal(v.shape)).astype(np.float32)
    return (1.5 * v + 0.25 * rms * rs.standard_normal(v.shape)).astype(np.float32)


def walk(w):
    """the single-key walk: one observable tensor after another replaced by its perturbation, cumulatively -> (key, the set after this step)"""
    for key in all_keys(w):
        if key in UNOBSERVABLE:
            continue
        w = replaced(w, key, perturb(key, get(w, key)))
        yield key, w


def oracle_outputs(w, inp, which=None, per_instance=False):
    """every forward of `which` (default: all of FORWARDS) under the set w in binary64 -> {forward: {tensor: array}}.  per_instance: the two actors'
    BatchNorms over the rows of one instance (Encoder.set_bn_mode(True)); the global critic's stay batch-wide there, as in the library"""
    import torch
    from oracle import encoder_oracle as eo
    ja, ma, gc = w
    B, T, M = inp["B"], inp["T"], inp["M"]
    f64 = torch.float64
    out = {}

    def per_b(fn, names):
        outs = [fn(slice(b, b + 1), 1) for b in range(B)] if per_instance else [fn(slice(0, B), B)]
        return {k: np.concatenate([o[k] for o in outs], 0) for k in names}

    for f in which or FORWARDS:
        if f in ("first", "later"):
            o = per_b(lambda s, n: eo.job_actor_forward(ja, inp["tfea"][s.start * T:s.stop * T], inp["col"][s], inp["val"][s], inp["cand"][s], inp["mask"][s],
                                                        inp["hm"][s] if f == "later" else None, n, T, dtype=f64), ("prob", "h_pooled", "job_v"))
            out[f] = {"prob": o["prob"], "h_pooled_o": o["h_pooled"], "job_v": o["job_v"]}
        elif f == "machine":
            o = per_b(lambda s, n: eo.machine_actor_forward(ma, inp["mfea1"][s], inp["mfea2"][s], inp["h_o"][s], inp["mmask"][s], n, M, dtype=f64),
                      ("prob", "h_pooled", "mach_v"))
            out[f] = {"mch_prob": o["prob"], "h_pooled_m": o["h_pooled"], "mach_v": o["mach_v"]}
        else:
            out[f] = {"global_v": eo.global_critic_forward(gc, inp["tfea"], inp["col"], inp["val"], inp["mfea1"], inp["mfea2"], B, T, M, dtype=f64)}
    return out


def distance(tensor, got, want):
    """normalised as tests/error_budget.py records it: probabilities absolute, embeddings by max(1, max |want|), critic values elementwise by 1 + |want|"""
    if tensor.endswith("prob"):
        return normalised(got, want)
    if tensor.startswith("h_pooled"):
        return normalised(got, want, max(1.0, float(np.abs(want).max())))
    return normalised(got, want, relative=True)


def distances(got, want):
    """{(forward, tensor): distance} over the forwards both hold"""
    return {(f, t): distance(t, got[f][t], want[f][t]) for f in want if f in got for t in want[f]}

"""Binary64 host model of the rollout -> update hand-off: the GAE reverse scan, the global
normalisation with its value targets, and the slot / channel bookkeeping that wires eight scans and eight value tensors
together — plain numpy, with DERIVED bounds on what a correct binary32 evaluation may differ by.

Test infrastructure only.  Nothing here imports torch, a kernel or the product; the indexing of `compose64` is written
from the description of the reference in the module docstring of advantages.py (ppo:437-536, 628-703, Run.py:451-475),
not from the product's code.  The input generators of the kernel tests live here too, so that the CPU tests
(tests/test_handoff_ref_cpu.py) check the bounds on exactly the inputs the GPU tests (tests/test_handoff_kernels_gpu.py) use.
"""
import numpy as np

U = 2.0 ** -24                      # unit round-off of binary32 (round to nearest)


# ------------------------------------------------------------------------------------------------------- GAE
def gae_constants(gamma, lam):
    """gamma, lambda and their product as a binary32 kernel holds them (as binary64 numbers): the product gamma * lambda is
    ROUNDED to binary32 — the one place where a binary64 model silently differs from the kernel"""
    g32, l32 = np.float32(gamma), np.float32(lam)
    return float(g32), float(l32), float(np.float32(g32 * l32))


def gae64(r, v, vn, done, gamma, lam):
    """The recursion of ppo:444-457 on [S,B] inputs -> (g, E), both [S,B] binary64.

        delta_s = r_s + gamma * vn_s - v_s                      (NO (1 - done) factor on delta)
        g_s     = delta_s + gamma * lambda * (1 - d_s) * g_{s+1},   g_S = 0

    evaluated in binary64 on the binary32 inputs, with gamma and c = gamma * lambda taken as the kernel has them
    (`gae_constants`).  E is a running bound on |binary32 evaluation - g|, carried alongside:

        E_s = c (1 - d_s) E_{s+1} + 5 u (|r_s| + gamma |vn_s| + |v_s| + c (1 - d_s) |g_{s+1}|),   u = 2^-24.

    Derivation of the factor (derived, not measured).  Write A = |r| + gamma |vn| + |v| and P = c (1 - d) |g_{s+1}|.
      * delta takes three roundings (gamma * vn, + r, - v); each result is at most A in magnitude, so each rounding is at
        most u A: 3 u A.  (A fused multiply-add would only remove one of them.)
      * the product chain c * g * (1 - d) takes at most three roundings (the product gamma * lambda, times g, times (1 - d));
        (1 - d) is exact for d in {0, 1} and this model already holds c as rounded, so this over-counts: 3 u P.  The error the
        carried g_{s+1} already has passes through the chain scaled by c (1 - d): the first term of E_s.
      * the final add rounds a number of magnitude at most A + P: u (A + P).
    Together 4 u (A + P) to first order; the bound uses 5 u, which covers the second-order terms (products of two relative
    errors, and |g| of the binary32 evaluation standing in for |g| of this model) with a margin of u (A + P) where
    they are of the order of u^2 S (A + P)."""
    r, v, vn, d = [np.asarray(x, np.float64) for x in (r, v, vn, done)]
    gam, _, c = gae_constants(gamma, lam)
    S, B = d.shape
    g, E = np.zeros((S, B)), np.zeros((S, B))
    gn, En = np.zeros(B), np.zeros(B)
    for s in range(S - 1, -1, -1):
        keep = c * (1.0 - d[s])
        g[s] = (r[s] + gam * vn[s] - v[s]) + keep * gn
        E[s] = keep * En + 5.0 * U * (np.abs(r[s]) + gam * np.abs(vn[s]) + np.abs(v[s]) + keep * np.abs(gn))
        gn, En = g[s], E[s]
    return g, E


def gae32(r, v, vn, done, gamma, lam):
    """numpy binary32 restatement of the kernel's recursion, operation by operation (no fused multiply-add) -> [S,B] float32"""
    f = np.float32
    r, v, vn, d = [np.asarray(x, f) for x in (r, v, vn, done)]
    gam, lm = f(gamma), f(lam)
    c = f(gam * lm)
    S, B = d.shape
    out = np.zeros((S, B), f)
    g = np.zeros(B, f)
    for s in range(S - 1, -1, -1):
        delta = f(f(r[s] + f(gam * vn[s])) - v[s])
        g = f(delta + f(f(c * g) * f(f(1.0) - d[s])))
        out[s] = g
    return out


# ------------------------------------------------------------------------------------------------------- normalisation
def _stats64(x):
    """mean and unbiased standard deviation (torch.std, ppo:485,532) in binary64; one element: std 0 — the kernel's deliberate
    choice where torch's unbiased std is NaN"""
    x = np.asarray(x, np.float64)
    return float(x.mean()), (float(x.std(ddof=1)) if x.size > 1 else 0.0)


def normalise64(G, K, rank, eps, values):
    """G [world,Kt,S,B] (what the all-gather of the packed per-rank buffers leaves on every rank) -> dict of
        norm    [K,S,B]   (x - mean) / (std + eps) of rank's block, statistics over ALL world*S*B elements of tensor k, unbiased
                          std (ppo:485,532); eps as a binary32 kernel argument holds it
        targets [K,S,B]   norm + values[k] (ppo:668-671,689); NaN where values is shorter than K
        full    [Kt,S,world*B]  the single-process layout: rank-major column blocks, every one of the Kt tensors
        Bn, Bt  [K,S,B]   elementwise bounds on |binary32 evaluation - norm| and |... - targets|
        mean, std [K]

    Bn = 2 u (|mean| / (std + eps) + 6 |a|) for a binary32 evaluation that takes mean and std from a binary64 reduction, rounds
    both to binary32, and then computes a = (x - mean) * (1 / (std + eps)):
      * rounding the mean moves every a by at most u |mean| / (std + eps);
      * the subtraction, the rounding of std, the add of eps, the reciprocal and the multiply are five roundings, each at most
        u |a| to first order; 6 |a| leaves one u for the statistics themselves (below);
      * the factor 2 covers the second-order terms.
    Bt = Bn + u |target| for the one extra add.

    The statistics: a kernel that forms the variance in ONE pass, (sum x^2 - n mean^2) / (n - 1) in binary64, loses
    (mean / std)^2 of its 2^-53 to cancellation.  That is negligible against u only while |mean| / std <= 100 (1e4 * n * 2^-53
    stays below u / 2 for n up to 4e4 in the worst case); every generated input of the tests stays inside that range."""
    G = np.asarray(G, np.float64)
    world, Kt, S, B = G.shape
    e = float(np.float32(eps))
    full = np.concatenate([G[w] for w in range(world)], axis=2)                 # [Kt,S,world*B]
    norm, Bn = np.zeros((K, S, B)), np.zeros((K, S, B))
    targets, Bt = np.full((K, S, B), np.nan), np.full((K, S, B), np.nan)
    means, stds = np.zeros(K), np.zeros(K)
    for k in range(K):
        mean, std = _stats64(full[k])
        a = (G[rank, k] - mean) / (std + e)
        norm[k], means[k], stds[k] = a, mean, std
        Bn[k] = 2.0 * U * (abs(mean) / (std + e) + 6.0 * np.abs(a))
        if k < len(values) and values[k] is not None:
            targets[k] = a + np.asarray(values[k], np.float64)
            Bt[k] = Bn[k] + U * np.abs(targets[k])
    return dict(norm=norm, targets=targets, full=full, Bn=Bn, Bt=Bt, mean=means, std=stds)


def normalise32(G, K, rank, eps, values):
    """numpy binary32 restatement of the normalisation kernel's arithmetic: binary64 mean and std (here numpy's two-pass ones)
    rounded to binary32, then (x - mean) * (1 / (std + eps)) and + value in binary32 -> (norm, targets) [K,S,B] float32"""
    f = np.float32
    G = np.asarray(G, f)
    world, Kt, S, B = G.shape
    norm, targets = np.zeros((K, S, B), f), np.full((K, S, B), np.nan, f)
    for k in range(K):
        mean, std = _stats64(np.concatenate([G[w, k] for w in range(world)], axis=1))
        inv = f(f(1.0) / f(f(std) + f(eps)))
        norm[k] = f(f(G[rank, k] - f(mean)) * inv)
        if k < len(values) and values[k] is not None:
            targets[k] = f(norm[k] + np.asarray(values[k], f))
    return norm, targets


# ------------------------------------------------------------------------------------------------------- composition
def handoff_views(buf_r, buf_jv, buf_mv, multi_v=None, multi_v_=None):
    """Slot and channel bookkeeping of the hand-off, with plain indexing -> list of (r, v, v_next) [S,B] triples: the four global
    ones (when multi_v is given) and then the four local ones, each in the order mk, pt, tt, it (ppo:441-443).

    What the reference does (advantages.py's docstring; ppo:437-536, Run.py:451-475):
      * the rollout stores the four scaled reward components per step as buf_r [S,4,B] in the order mk, idle, pt, tt; the
        advantages are ordered mk, pt, tt, it — so advantage channel (mk, pt, tt, it) reads reward channel (0, 2, 3, 1);
      * the job critic's two outputs are (mk, it), the machine critic's (pt, tt): buf_jv / buf_mv [episodes, T+1, B, 2];
      * v of step t of an episode is slot t; v_ of step t is slot t+1 — the value at act time of the next step — and for the
        episode's last step slot T, the value of the terminal state from the post-terminal forward pair: NOT the value of the
        next episode's first state;
      * global channel i pairs reward (mk, pt, tt, it)[i] with multi_v[..., i] and multi_v_[..., i] ([S,B,4])."""
    buf_r, buf_jv, buf_mv = [np.asarray(x) for x in (buf_r, buf_jv, buf_mv)]
    eps, T1, B, _ = buf_jv.shape
    T = T1 - 1
    S = eps * T
    assert buf_r.shape == (S, 4, B) and buf_mv.shape == buf_jv.shape
    r_mk, r_it, r_pt, r_tt = buf_r[:, 0], buf_r[:, 1], buf_r[:, 2], buf_r[:, 3]

    def now(buf, c):            # slots 0 .. T-1 of every episode
        return np.concatenate([buf[e, 0:T, :, c] for e in range(eps)], axis=0)

    def nxt(buf, c):            # slots 1 .. T of every episode
        return np.concatenate([buf[e, 1:T + 1, :, c] for e in range(eps)], axis=0)

    out = []
    if multi_v is not None:
        mv, mv_ = np.asarray(multi_v), np.asarray(multi_v_)
        assert mv.shape == (S, B, 4) and mv_.shape == (S, B, 4)
        out += [(r, mv[:, :, i], mv_[:, :, i]) for i, r in enumerate((r_mk, r_pt, r_tt, r_it))]
    out += [(r_mk, now(buf_jv, 0), nxt(buf_jv, 0)), (r_pt, now(buf_mv, 0), nxt(buf_mv, 0)),
            (r_tt, now(buf_mv, 1), nxt(buf_mv, 1)), (r_it, now(buf_jv, 1), nxt(buf_jv, 1))]
    return out


def compose64(buf_r, buf_jv, buf_mv, buf_done, multi_v=None, multi_v_=None, gamma=0.99, lam=0.98, eps=1e-5, raw=None):
    """The whole single-rank hand-off from a rollout's stored buffers (buf_r [S,4,B], buf_jv / buf_mv [episodes,T+1,B,2],
    buf_done [S,B], multi_v / multi_v_ [S,B,4] or None for the local half alone) -> dict of [n,S,B] arrays, n = 8 (4 global, then
    4 local) or 4, each group in the order mk, pt, tt, it:
        raw, E               un-normalised advantages and their bound (gae64)
        adv, adv_bound       normalised advantages (normalise64 over the [S,B] tensor) and their bound
        targets, target_bound    adv + value at act time
        values               the value tensors the targets are built from

    raw=None: the normalisation runs on this model's own raw advantages.  An evaluation that normalised ITS raw advantages x' (with
    |x' - x| <= E) differs by what that perturbation does to (x - mean) / (std + eps) on top of Bn: the mean moves by at most
    mean(E), the unbiased std by at most rms(E) sqrt(n / (n - 1)) (the std is 1-Lipschitz in the root-mean-square norm), so
        adv_bound = Bn + 1.01 (E + mean(E) + |a| rms(E) sqrt(n / (n - 1))) / (std + eps)
    (1.01 for the second-order terms).  raw = [n,S,B] array: the normalisation runs on these stored numbers instead (a kernel's own
    raw advantages) and adv_bound is Bn unchanged."""
    views = handoff_views(buf_r, buf_jv, buf_mv, multi_v, multi_v_)
    n = len(views)
    done = np.asarray(buf_done, np.float64)
    S, B = done.shape
    g, E = np.zeros((n, S, B)), np.zeros((n, S, B))
    for k, (r, v, vn) in enumerate(views):
        g[k], E[k] = gae64(r, v, vn, done, gamma, lam)
    values = [np.asarray(v, np.float64) for _, v, _ in views]
    x = g if raw is None else np.asarray(raw, np.float64)
    N = normalise64(x[None], n, 0, eps, values)
    adv_bound = N["Bn"].copy()
    if raw is None:
        cnt = S * B
        for k in range(n):
            rms = np.sqrt((E[k] ** 2).mean()) * (np.sqrt(cnt / (cnt - 1.0)) if cnt > 1 else 1.0)
            adv_bound[k] += 1.01 * (E[k] + E[k].mean() + np.abs(N["norm"][k]) * rms) / (N["std"][k] + float(np.float32(eps)))
    target_bound = adv_bound + U * np.abs(N["targets"])
    return dict(raw=g, E=E, adv=N["norm"], adv_bound=adv_bound, targets=N["targets"], target_bound=target_bound,
                values=np.stack(values), std=N["std"], mean=N["mean"])


def compose32(buf_r, buf_jv, buf_mv, buf_done, multi_v=None, multi_v_=None, gamma=0.99, lam=0.98, eps=1e-5):
    """binary32 restatement of the same hand-off (gae32 + normalise32) -> (raw, adv, targets) [n,S,B] float32"""
    views = handoff_views(buf_r, buf_jv, buf_mv, multi_v, multi_v_)
    raw = np.stack([gae32(r, v, vn, buf_done, gamma, lam) for r, v, vn in views])
    adv, targets = normalise32(raw[None], len(views), 0, eps, [v for _, v, _ in views])
    return raw, adv, targets


# ------------------------------------------------------------------------------------------------------- test inputs
GAMMA, LAM, EPS = 0.99, 0.98, 1e-5
GAE_S = (1, 5, 11, 12, 13, 23, 24, 25, 100)
GAE_B = (1, 63, 64, 65, 130)
# (S, B, layout, done): every S x B in the product's layout with 10 % random dones, then the special ones
GAE_CASES = [(S, B, "product", "random") for S in GAE_S for B in GAE_B] + [
    (25, 65, "product", "zeros"), (25, 65, "product", "ones"), (25, 65, "transposed", "random"), (100, 63, "transposed", "random"),
    (25, 65, "contiguous", "random"), (13, 130, "contiguous", "random")]


def gae_case(S, B, layout, done):
    """One input set of the GAE kernel tests, as the BASE arrays of the layout (float32) — `gae_views` slices them:
      product     r = r4[:, ch] of [S,4,B]; v, vn = vv[:S,:,c], vv[1:,:,c] of [S+1,B,2] (what the rollout hands the kernel)
      transposed  r, v = transposed [B,S] tensors (stride_b > stride_s), vn a contiguous [S,B]
      contiguous  three contiguous [S,B]
    |r| ~ 1, |v| ~ 5; done: 10 % random ones plus the last row set, all zero, or all one."""
    rs = np.random.RandomState(100000 + 1000 * S + B + {"product": 0, "transposed": 300, "contiguous": 600}[layout])
    f = np.float32
    c = dict(S=S, B=B, layout=layout)
    if layout == "product":
        c.update(r4=rs.randn(S, 4, B).astype(f), vv=(5 * rs.randn(S + 1, B, 2)).astype(f), ch=(S + B) % 4, c=(S * B) % 2)
    elif layout == "transposed":
        c.update(rT=rs.randn(B, S).astype(f), vT=(5 * rs.randn(B, S)).astype(f), vn=(5 * rs.randn(S, B)).astype(f))
    else:
        c.update(r=rs.randn(S, B).astype(f), v=(5 * rs.randn(S, B)).astype(f), vn=(5 * rs.randn(S, B)).astype(f))
    if done == "random":
        d = (rs.rand(S, B) < 0.1).astype(f)
        d[-1] = 1
    else:
        d = np.full((S, B), 0 if done == "zeros" else 1, f)
    c["done"] = d
    return c


def gae_views(case, up=lambda a: a):
    """(r, v, vn, done) views of a `gae_case`; `up` moves a base array to where the views are wanted (identity: numpy; a host ->
    device copy: tensors with the same strides)"""
    if case["layout"] == "product":
        r4, vv = up(case["r4"]), up(case["vv"])
        S = r4.shape[0]
        return r4[:, case["ch"]], vv[:S, :, case["c"]], vv[1:, :, case["c"]], up(case["done"])
    if case["layout"] == "transposed":
        return up(case["rT"]).T, up(case["vT"]).T, up(case["vn"]), up(case["done"])
    return up(case["r"]), up(case["v"]), up(case["vn"]), up(case["done"])


# (world, rank, S, B, K, Kt): fewer elements than one workgroup; 20 000 elements; 40 000 > 32 768 with a ragged second sweep; odd
# shapes; K = Kt = 16
NORM_ROWS = [(1, 0, 1, 3, 1, 1), (1, 0, 100, 200, 8, 16), (2, 1, 100, 200, 8, 16), (3, 2, 13, 65, 4, 8), (2, 0, 36, 40, 16, 16)]
NORM_KINDS = ("randn", "offset", "constant", "outlier")


def norm_case(row, kind):
    """-> (G [world,Kt,S,B] float32, vals3 [S,B,2] float32; values[k] = vals3[..., k % 2], strided like job_v[..., 0])
      randn     3 N(0,1) + 0.7
      offset    mean 50, std 0.5001 per tensor (the sample is standardised first, so that |mean| / std stays just inside 100 after
                the rounding to float32, whatever the sample size)
      constant  one value everywhere (model and kernel both give exact zeros)
      outlier   N(0,1) with a single 1e4 in every tensor"""
    world, rank, S, B, K, Kt = row
    rs = np.random.RandomState(7000 + 100 * NORM_ROWS.index(row) + NORM_KINDS.index(kind))
    z = rs.randn(world, Kt, S, B)
    if kind == "randn":
        G = 3.0 * z + 0.7
    elif kind == "offset":
        m = z.mean(axis=(0, 2, 3), keepdims=True)
        s = z.std(axis=(0, 2, 3), ddof=1, keepdims=True)
        G = 50.0 + 0.5001 * (z - m) / s
    elif kind == "constant":
        G = np.full_like(z, 1.7)
    else:
        G = z
        G[world - 1, :, S // 2, B // 3] = 1e4
    vals3 = (2.0 * rs.randn(S, B, 2)).astype(np.float32)
    return G.astype(np.float32), vals3


# (T, B, episodes): the slot layouts of the rollout shapes of tests/test_handoff_rollout_gpu.py, filled with random numbers
BUFFER_SHAPES = [(100, 24, 1), (35, 19, 2), (12, 7, 3), (16, 65, 2)]


def random_buffers(T, B, episodes, seed=0):
    """stored buffers of a rollout with random contents -> dict(buf_r, buf_jv, buf_mv, buf_done, multi_v, multi_v_) float32"""
    rs = np.random.RandomState(9000 + seed + 10 * T + B)
    f = np.float32
    S = T * episodes
    done = np.zeros((S, B), f)
    done[T - 1::T] = 1
    return dict(buf_r=rs.randn(S, 4, B).astype(f), buf_jv=(5 * rs.randn(episodes, T + 1, B, 2)).astype(f),
                buf_mv=(5 * rs.randn(episodes, T + 1, B, 2)).astype(f), buf_done=done,
                multi_v=(5 * rs.randn(S, B, 4)).astype(f), multi_v_=(5 * rs.randn(S, B, 4)).astype(f))

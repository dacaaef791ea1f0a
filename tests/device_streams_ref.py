"""Host model of every random stream and of the action selection that run on the device (test infrastructure only).

Each function restates one piece of kernel text — integer arithmetic plus IEEE binary32 / binary64 adds, multiplies and divides,
one rounding per operation (the library is built without floating-point contraction) — so that a device result can be demanded
EQUAL to the model, element for element.  numpy, vectorised over instances; csrc/ = e2e-mappo-for-mt-fjsp_amd/csrc/.
tests/test_device_streams_cpu.py pins this file (Philox known answers, the sampler's distribution, structure of the generator)."""
import numpy as np

U64 = np.uint64
M32 = U64(0xFFFFFFFF)
TAG_SAMPLE, TAG_RANDOM, TAG_W3, TAG_MOR = 0x73616d70, 0x6d746a73, 0x77337733, 0x70647231
TAG_GEN = (0x67656e31, 0x67656e32, 0x67656e33, 0x67656e34, 0x67656e35)
DEFAULT_SCOPE = dict(t_low=1, t_high=99, p_low=1, p_high=20, transT_in_low=1, transT_in_high=10, transT_out_high=20,
                     weight_low=0.8, weight_high=1.2)          # = instances.DEFAULT_SCOPE (the fields the kernel reads)


def _w(x):
    """a 32-bit word (python int of any size, or an integer array) -> uint64 array holding its low 32 bits"""
    if isinstance(x, (int, np.integer)):
        return np.asarray(int(x) & 0xFFFFFFFF, U64)
    return np.asarray(x).astype(U64) & M32


def _lo_hi(x):
    """a 64-bit kernel argument (uint64_t seed / counter / episode) -> its ((uint32_t)x, (uint32_t)(x >> 32))"""
    x = int(x) & 0xFFFFFFFFFFFFFFFF
    return x & 0xFFFFFFFF, x >> 32


def philox4x32(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 (csrc/mtfjsp_env_dev.h:106-115) -> the four output words, uint64 arrays < 2^32"""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(_w(c0), _w(c1), _w(c2), _w(c3), _w(k0), _w(k1))
    for _ in range(10):
        p0, p1 = U64(0xD2511F53) * c0, U64(0xCD9E8D57) * c2               # 32 x 32 -> 64 bits: no wrap in uint64
        c0, c1, c2, c3 = (p1 >> U64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> U64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + U64(0x9E3779B9)) & M32, (k1 + U64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def pick_uniform(b, seed, counter):
    """binary32 u in [0,1) of instance b's draw (csrc/mtfjsp_encoder.hip:1521-1526)"""
    s0, s1 = _lo_hi(seed)
    n0, n1 = _lo_hi(counter)
    c = philox4x32(b, n0, n1, TAG_SAMPLE, s0, s1)
    return (c[0] >> U64(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def pick(prob, greedy, u=None):
    """pick_action_u (csrc/mtfjsp_encoder.hip:1528-1551) on prob [B,n] binary32, one column at a time: the kernel's left-to-right sums"""
    p = np.ascontiguousarray(prob, np.float32)
    B, n = p.shape
    if greedy:                                                           # the first maximum
        best, idx = p[:, 0].copy(), np.zeros(B, np.int32)
        for i in range(1, n):
            m = p[:, i] > best
            best[m] = p[m, i]
            idx[m] = i
        return idx
    tot = np.zeros(B, np.float32)
    for i in range(n):
        tot = tot + p[:, i]
    thr = np.asarray(u, np.float32) * tot
    acc, idx, last = np.zeros(B, np.float32), np.full(B, -1, np.int32), np.zeros(B, np.int32)
    for i in range(n):
        pos = p[:, i] > 0
        acc = np.where(pos, acc + p[:, i], acc)
        last[pos] = i
        idx[pos & (idx < 0) & (thr < acc)] = i
    return np.where(idx < 0, last, idx).astype(np.int32)


def _nth_true(ok, k):
    """index of the k-th (0-based) True of every row of ok [B,n] (0 where there is none)"""
    return np.argmax(ok & ((np.cumsum(ok, 1) - 1) == k[:, None]), 1).astype(np.int32)


def random_actions(t, cand, jmask, seed, counter):
    """k_random_actions (csrc/mtfjsp_env.hip:1497-1524) -> (task, mach, job) [B] int32"""
    t, cand = np.asarray(t), np.asarray(cand)
    B = t.shape[0]
    s0, s1 = _lo_hi(seed)
    n0, n1 = _lo_hi(counter)
    c = philox4x32(np.arange(B), n0, n1, TAG_RANDOM, s0, s1)
    free = np.asarray(jmask) == 0
    n = free.sum(1).astype(U64)
    jj = np.where(n > 0, _nth_true(free, ((c[0] * n) >> U64(32)).astype(np.int64)), 0).astype(np.int32)
    a = np.where(n > 0, cand[np.arange(B), jj], 0).astype(np.int32)
    ok = t[np.arange(B), a] >= 0
    nf = ok.sum(1).astype(U64)
    mm = np.where(nf > 0, _nth_true(ok, ((c[1] * nf) >> U64(32)).astype(np.int64)), 0).astype(np.int32)
    return a, mm, jj


def draw_w3(B, seed, episode):
    """draw_w3 (csrc/mtfjsp_env.hip:110-121) -> [B,3] binary64"""
    s0, s1 = _lo_hi(seed)
    e0, e1 = _lo_hi(episode)
    b = np.arange(B)
    x = philox4x32(b, e0, e1, TAG_W3, s0, s1)
    y = philox4x32(b, e0, e1, TAG_W3 + 2, s0, s1)

    def u53(a, c):
        return ((a >> U64(5)).astype(np.float64) * 67108864.0 + (c >> U64(6)).astype(np.float64)) * (1.0 / 9007199254740992.0)

    u0, u1, u2 = u53(x[0], x[1]), u53(x[2], x[3]), u53(y[0], y[1])
    s = (u0 + u1) + u2
    return np.stack([u0 / s, u1 / s, u2 / s], 1)


def u01(a, b):
    """csrc/mtfjsp_env.hip:1612"""
    return (((a << U64(21)) ^ (b >> U64(11))).astype(np.float64) + 0.5) * (1.0 / 9007199254740992.0)


def generate(B, J, M, E, seed, first_instance=0, scope=None):
    """k_generate (csrc/mtfjsp_env.hip:1613-1665) -> t, p [B,T,M] f64, tt [B,M,M] f64, shop [B,M] int32.
    (Streams 0x67656e33 / 0x67656e34 carry only the LOW word of the instance number beside task and machine / draw index.)"""
    S = dict(DEFAULT_SCOPE)
    if scope:
        S.update(scope)
    f = np.float64
    t_low, t_high, p_low, p_high = f(S["t_low"]), f(S["t_high"]), f(S["p_low"]), f(S["p_high"])
    w_low, w_high = f(S["weight_low"]), f(S["weight_high"])
    in_low, in_high, out_high = f(S["transT_in_low"]), f(S["transT_in_high"]), f(S["transT_out_high"])
    T = J * M
    s0, s1 = _lo_hi(seed)
    inst = (np.repeat(np.arange(B, dtype=U64), T) + U64(int(first_instance) & 0xFFFFFFFFFFFFFFFF))     # (wraps like uint64_t)
    i0, i1 = inst & M32, inst >> U64(32)
    v = np.tile(np.arange(T, dtype=U64), B)
    N = B * T
    c = philox4x32(i0, i1, v, TAG_GEN[0], s0, s1)                        # :1619-1622
    avg_t = t_low + (t_high - t_low) * u01(c[0], c[1])
    avg_p = p_low + (p_high - p_low) * u01(c[2], c[3])
    d = philox4x32(i0, i1, v, TAG_GEN[1], s0, s1)                        # :1625-1627
    k = (u01(d[0], d[1]) * M).astype(np.int64)
    perm = np.tile(np.arange(M), (N, 1))
    bad = np.zeros((N, M), bool)
    rows = np.arange(N)
    for j in range(int(k.max()) if N else 0):                            # :1631-1637 (ctr = j)
        e = philox4x32(i0, v, j, TAG_GEN[2], s0, s1)
        r = j + (u01(e[0], e[1]) * (M - j)).astype(np.int64)
        on = j < k
        pj, pr = perm[rows, j].copy(), perm[rows, r].copy()
        perm[rows[on], j] = pr[on]
        perm[rows[on], r[on]] = pj[on]
        bad[rows[on], perm[rows[on], j]] = True
    t, p = np.empty((N, M)), np.empty((N, M))
    for m in range(M):                                                   # :1639-1647
        e = philox4x32(i0, v, m, TAG_GEN[3], s0, s1)
        tv = avg_t * (w_low + (w_high - w_low) * u01(e[0], e[1]))
        pv = avg_p * (w_low + (w_high - w_low) * u01(e[2], e[3]))
        t[:, m] = np.where(bad[:, m], -tv, tv)
        p[:, m] = np.where(bad[:, m], -pv, pv)
    # transport times (:1649-1664)
    per = M // E
    sh = np.minimum(np.arange(M) // per, E - 1)
    r, cc = np.meshgrid(np.arange(M), np.arange(M), indexing="ij")
    lo, hi = np.minimum(r, cc), np.maximum(r, cc)
    ib = np.arange(B, dtype=U64) + U64(int(first_instance) & 0xFFFFFFFFFFFFFFFF)
    e = philox4x32((ib & M32)[:, None, None], (ib >> U64(32))[:, None, None], (lo * M + hi)[None], TAG_GEN[4], s0, s1)
    u = u01(e[0], e[1])
    dist = np.abs(sh[r] - sh[cc]).astype(np.float64)[None]
    near = in_low + (in_high - in_low) * u
    far = in_high * dist + (out_high * dist - in_high * dist) * u
    tt = np.where(dist == 0, near, far)
    tt[:, r == cc] = 0.0
    shop = np.tile(sh.astype(np.int32), (B, 1))
    return t.reshape(B, T, M), p.reshape(B, T, M), tt, shop


def mor_order(B, J, M, seed):
    """the MOR shuffle of k_pdr_plan (csrc/mtfjsp_pdr.hip:101-118) -> [B,M,J] int32: column c's job order of instance b
    (the planner's task order is order[b, c, i] * M + c at position c * J + i)"""
    s0, s1 = _lo_hi(seed)
    b, c = np.meshgrid(np.arange(B), np.arange(M), indexing="ij")
    b, c = b.ravel(), c.ravel()
    col = np.tile(np.arange(J), (B * M, 1))
    rows = np.arange(B * M)
    have, blk, r = 0, 0, None
    for i in range(J - 1, 0, -1):
        if not have:
            r = philox4x32(b, c, blk, TAG_MOR, s0, s1)
            blk += 1
            have = 4
        u = r[4 - have]
        have -= 1
        k = ((u * U64(i + 1)) >> U64(32)).astype(np.int64)               # uniform in [0, i]
        x, y = col[:, i].copy(), col[rows, k].copy()
        col[:, i] = y
        col[rows, k] = x
    return col.reshape(B, M, J).astype(np.int32)

"""The binary64 host model of the rollout -> update hand-off (tests/handoff_ref.py) checked without a GPU:
  * the model IS the reference: on the reference's own rollout (tests/golden/rollout_gae_j6m6e2_b4.npz) it reproduces all eight
    advantages and value targets;
  * its derived bounds E / Bn hold for a correct binary32 evaluation (numpy restatements of the kernels' arithmetic) on every input
    set tests/test_handoff_kernels_gpu.py uses — same generators, same seeds — so they are not too tight;
  * they catch what they are for: every listed mutant of the model leaves its bound somewhere on those inputs.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import handoff_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "rollout_gae_j6m6e2_b4.npz")
G, L, EPS = ref.GAMMA, ref.LAM, ref.EPS


def _fixture_buffers():
    """the reference rollout's stored numbers in the device rollout's slot layout: T+1 value slots per episode, slot T the
    post-terminal value; rewards in the step kernel's order mk, idle, pt, tt"""
    f = np.load(FIX)
    J, M, E, B, eps = [int(x) for x in f["meta"]]
    T = J * M
    buf_r = np.stack([f["out_mk"], f["out_it"], f["out_pt"], f["out_tt"]], axis=1)
    buf_jv, buf_mv = np.zeros((eps, T + 1, B, 2), np.float32), np.zeros((eps, T + 1, B, 2), np.float32)
    for e in range(eps):
        buf_jv[e, :T], buf_mv[e, :T] = f["out_job_v"][e * T:(e + 1) * T], f["out_machine_v"][e * T:(e + 1) * T]
        buf_jv[e, T], buf_mv[e, T] = f["term_job_v_"][e], f["term_machine_v_"][e]
    return f, dict(buf_r=buf_r, buf_jv=buf_jv, buf_mv=buf_mv, buf_done=f["out_done_operation"], multi_v=f["multi_v"], multi_v_=f["multi_v_"])


def _buffer_sets():
    """(name, buffers, gamma, lambda): the reference rollout and random contents in the slot layouts of the rollout tests"""
    f, fb = _fixture_buffers()
    g, lam = [float(x) for x in f["gamma_lambda"]]
    return [("fixture", fb, g, lam)] + [(f"random{T}x{B}x{e}", ref.random_buffers(T, B, e), G, L) for T, B, e in ref.BUFFER_SHAPES]


# ------------------------------------------------------------------------------------------- the model is the reference
def test_model_reproduces_the_reference_advantages_and_targets():
    f, fb = _fixture_buffers()
    g, lam = [float(x) for x in f["gamma_lambda"]]
    m = ref.compose64(gamma=g, lam=lam, **fb)
    tol = dict(rtol=1e-5, atol=1e-5)           # the tolerance of test_host_gae_and_normalisation_reproduce_the_reference_advantages
    for i in range(4):
        np.testing.assert_allclose(m["adv"][i], f["global_adv"][i], **tol)
        np.testing.assert_allclose(m["targets"][i], f["global_target"][i], **tol)
        np.testing.assert_allclose(m["adv"][4 + i], f["local_adv"][i], **tol)
        np.testing.assert_allclose(m["targets"][4 + i], f["local_target"][i], **tol)
    local = ref.compose64(fb["buf_r"], fb["buf_jv"], fb["buf_mv"], fb["buf_done"], gamma=g, lam=lam)      # the local half alone
    assert np.array_equal(local["adv"], m["adv"][4:]) and np.array_equal(local["raw"], m["raw"][4:])


def test_kernel_constants_differ_from_their_binary64_values():
    gam, lam, c = ref.gae_constants(G, L)
    assert gam == float(np.float32(0.99)) != 0.99 and c == float(np.float32(np.float32(0.99) * np.float32(0.98))) and c != gam * lam


# ------------------------------------------------------------------------------------------- bounds hold for binary32
@pytest.mark.parametrize("S,B,layout,done", ref.GAE_CASES)
def test_gae_bound_holds_for_a_binary32_evaluation(S, B, layout, done):
    r, v, vn, d = ref.gae_views(ref.gae_case(S, B, layout, done))
    assert r.shape == v.shape == vn.shape == d.shape == (S, B)
    g, E = ref.gae64(r, v, vn, d, G, L)
    g32 = ref.gae32(r, v, vn, d, G, L)
    assert (np.abs(g32 - g) <= E).all(), float((np.abs(g32 - g) / E).max())
    assert E.max() < 5e-4 and np.abs(g).max() > 3          # a rounding bound (5 u x 11 per step, summed with weights c^k <= 33 steps' worth)


@pytest.mark.parametrize("kind", ref.NORM_KINDS)
@pytest.mark.parametrize("row", ref.NORM_ROWS)
def test_normalisation_bound_holds_for_a_binary32_evaluation(row, kind):
    world, rank, S, B, K, Kt = row
    Gt, vals3 = ref.norm_case(row, kind)
    values = [vals3[..., k % 2] for k in range(K)]
    m = ref.normalise64(Gt, K, rank, EPS, values)
    if kind != "constant":
        assert (np.abs(m["mean"]) <= 100.0 * m["std"]).all()                 # the range the one-pass variance is negligible in
    n32, t32 = ref.normalise32(Gt, K, rank, EPS, values)
    assert (np.abs(n32 - m["norm"]) <= m["Bn"]).all(), float((np.abs(n32 - m["norm"]) / m["Bn"]).max())
    assert (np.abs(t32 - m["targets"]) <= m["Bt"]).all()
    if kind == "constant":
        assert not n32.any() and not m["norm"].any()
    for k in range(Kt):                                                          # rank-major column blocks
        for w in range(world):
            assert np.array_equal(m["full"][k][:, w * B:(w + 1) * B], Gt[w, k])
    short = ref.normalise64(Gt, K, rank, EPS, values[:K // 2])
    assert np.isnan(short["targets"][K // 2:]).all() and np.array_equal(short["targets"][:K // 2], m["targets"][:K // 2])


def test_one_element_normalises_to_zero():
    """the kernel's deliberate choice (std 0 for a single element), where torch's unbiased std is NaN"""
    m = ref.normalise64(np.full((1, 1, 1, 1), 3.25, np.float32), 1, 0, EPS, [])
    assert m["norm"].item() == 0.0 and m["std"].item() == 0.0


@pytest.mark.parametrize("name,bufs,g,lam", _buffer_sets(), ids=[b[0] for b in _buffer_sets()])
def test_composed_bounds_hold_for_a_binary32_evaluation(name, bufs, g, lam):
    raw32, adv32, tgt32 = ref.compose32(gamma=g, lam=lam, **bufs)
    m = ref.compose64(gamma=g, lam=lam, **bufs)
    assert (np.abs(raw32 - m["raw"]) <= m["E"]).all()
    assert (np.abs(adv32 - m["adv"]) <= m["adv_bound"]).all() and (np.abs(tgt32 - m["targets"]) <= m["target_bound"]).all()
    own = ref.compose64(gamma=g, lam=lam, raw=raw32, **bufs)                    # normalisation of the evaluation's OWN raw advantages: Bn unchanged
    assert (np.abs(adv32 - own["adv"]) <= own["adv_bound"]).all() and (np.abs(tgt32 - own["targets"]) <= own["target_bound"]).all()
    assert (own["adv_bound"] <= m["adv_bound"]).all() and (m["adv_bound"] <= 1e-4 * (1 + np.abs(m["adv"]))).all()


# ------------------------------------------------------------------------------------------- mutants of the GAE model
def _gae_mutant(r, v, vn, done, gamma, lam, mask_delta=False, mask_carry=True, tail=None, gamma64=False):
    """the recursion of gae64 in binary64 with one slip: (1-done) on delta as well; none on the carry; the S mod 12 steps the
    kernel's remainder loop handles (s = S mod 12 - 1 ... 0) skipped (left at zero) or restarted from g = 0; gamma, lambda in binary64"""
    r, v, vn, d = [np.asarray(x, np.float64) for x in (r, v, vn, done)]
    gam, _, c = (gamma, lam, gamma * lam) if gamma64 else ref.gae_constants(gamma, lam)
    S, B = d.shape
    rem = S % 12
    g, gn = np.zeros((S, B)), np.zeros(B)
    for s in range(S - 1, -1, -1):
        if s < rem and tail == "skip":
            break
        if s == rem - 1 and tail == "restart":
            gn = np.zeros(B)
        nd = 1.0 - d[s]
        delta = r[s] + gam * vn[s] - v[s]
        g[s] = delta * (nd if mask_delta else 1.0) + c * (nd if mask_carry else 1.0) * gn
        gn = g[s]
    return g


def _worst_ratio(mutant, cases):
    """largest |mutant - model| / E over the cases, per case"""
    out = {}
    for case in cases:
        r, v, vn, d = ref.gae_views(ref.gae_case(*case))
        g, E = ref.gae64(r, v, vn, d, G, L)
        out[case] = float((np.abs(mutant(r, v, vn, d) - g) / E).max())
    return out


RANDOM_DONE = [c for c in ref.GAE_CASES if c[3] == "random"]


def test_gae_mutant_done_on_delta_leaves_the_bound():
    w = _worst_ratio(lambda *a: _gae_mutant(*a, G, L, mask_delta=True), RANDOM_DONE)
    assert all(x > 10 for x in w.values()), w                                     # the last row is done in every one of them


def test_gae_mutant_no_done_on_the_carry_leaves_the_bound():
    w = _worst_ratio(lambda *a: _gae_mutant(*a, G, L, mask_carry=False), [c for c in RANDOM_DONE if c[0] >= 11 and c[1] >= 63])
    assert all(x > 10 for x in w.values()), w
    ones = _worst_ratio(lambda *a: _gae_mutant(*a, G, L, mask_carry=False), [(25, 65, "product", "ones")])
    assert all(x > 10 for x in ones.values())


@pytest.mark.parametrize("tail", ["skip", "restart"])
def test_gae_mutant_in_the_remainder_steps_leaves_the_bound(tail):
    """S = 13, 23, 25, 100 leave 1, 11, 1 and 4 steps to the kernel's remainder loop; a skipped one shows at any S that is not a
    multiple of 12, a restarted carry only where unrolled steps came before it"""
    long_ = [c for c in RANDOM_DONE if c[0] % 12 and c[0] > 12]
    w = _worst_ratio(lambda *a: _gae_mutant(*a, G, L, tail=tail), long_)
    for (S, B, _, _), x in w.items():
        if B >= 63:                                        # (a single column may hold a done exactly at the restart)
            assert x > 10, (S, B, x)
    assert max(x for (S, B, _, _), x in w.items() if B == 1) > 10
    if tail == "skip":
        short = _worst_ratio(lambda *a: _gae_mutant(*a, G, L, tail=tail), [c for c in RANDOM_DONE if c[0] < 12])
        assert all(x > 10 for x in short.values()), short
    same = _worst_ratio(lambda *a: _gae_mutant(*a, G, L, tail=tail), [c for c in RANDOM_DONE if c[0] % 12 == 0])
    assert all(x == 0 for x in same.values())              # multiples of 12: the remainder loop does not run — the gap this closes


def test_gae_mutant_vn_read_with_the_stride_of_v_leaves_the_bound():
    """v and vn of the product layout share their strides (two slices of one tensor); the transposed cases pair a [B,S] transposed
    v with a contiguous vn, where reading vn at v's strides (1, S) from vn's base takes element s + b S of its storage"""
    for case in [c for c in ref.GAE_CASES if c[2] == "transposed"]:
        S, B = case[0], case[1]
        c = ref.gae_case(*case)
        r, v, vn, d = ref.gae_views(c)
        assert v.strides != vn.strides and v.strides[1] > v.strides[0]
        vn_wrong = c["vn"].ravel().reshape(B, S).T
        g, E = ref.gae64(r, v, vn, d, G, L)
        assert float((np.abs(ref.gae64(r, v, vn_wrong, d, G, L)[0] - g) / E).max()) > 10


def test_gamma_in_binary64_stays_inside_the_bound_and_is_not_a_mutant_the_bound_can_catch():
    """DROPPED as a mutant, with the reason: binary32(0.99) differs from 0.99 by 9.5e-9 = 0.16 u relative and the rounded product
    gamma * lambda by 2.0e-8, so the mutant moves delta by 0.16 u gamma |vn| per step where E grants 5 u (|r| + gamma |vn| + |v|), and
    both accumulate through the same recursion: the ratio stays near 0.05 at every length, the long scans (S = 100) included.  E is
    a worst-case rounding bound and is not tightened for this; what the model does guarantee is that the KERNEL's constants are
    used on both sides, so this difference never eats into the bound."""
    w = _worst_ratio(lambda *a: _gae_mutant(*a, G, L, gamma64=True), RANDOM_DONE)
    worst_long = max(x for (S, _, _, _), x in w.items() if S >= 100)
    assert 0.0 < worst_long < 0.2 and max(w.values()) < 0.2, w


# ------------------------------------------------------------------------------------------- mutants of the normalisation
def _norm_mutant(Gt, K, rank, eps, biased=False, eps_inside=False):
    Gt = np.asarray(Gt, np.float64)
    world = Gt.shape[0]
    e = float(np.float32(eps))
    out = []
    for k in range(K):
        full = np.concatenate([Gt[w, k] for w in range(world)], axis=1)
        var = full.var(ddof=0 if biased else 1)
        out.append((Gt[rank, k] - full.mean()) / (np.sqrt(var + e) if eps_inside else np.sqrt(var) + e))
    return np.stack(out)


BIG_ROWS = [r for r in ref.NORM_ROWS if r[0] * r[2] * r[3] >= 20000]


@pytest.mark.parametrize("row", BIG_ROWS)
def test_normalisation_mutant_biased_variance_leaves_the_bound(row):
    """1 / (2 n) of |a| against 12 u |a|: visible up to n ~ 7e5 — at the 20 000 and 40 000 element rows by a factor 35 and 17"""
    world, rank, S, B, K, Kt = row
    for kind in ("randn", "offset", "outlier"):
        Gt, _ = ref.norm_case(row, kind)
        m = ref.normalise64(Gt, K, rank, EPS, [])
        assert float((np.abs(_norm_mutant(Gt, K, rank, EPS, biased=True) - m["norm"]) / m["Bn"]).max()) > 3, kind


@pytest.mark.parametrize("row", BIG_ROWS)
def test_normalisation_mutant_eps_under_the_square_root_leaves_the_bound(row):
    """sqrt(var + eps) against std + eps: 2.8e-6 relative at std 3 (47 u), the `randn` inputs; at std 0.5 the two happen to agree
    and at std 70 they differ by 2 u, so the other kinds cannot tell"""
    world, rank, S, B, K, Kt = row
    Gt, _ = ref.norm_case(row, "randn")
    m = ref.normalise64(Gt, K, rank, EPS, [])
    assert float((np.abs(_norm_mutant(Gt, K, rank, EPS, eps_inside=True) - m["norm"]) / m["Bn"]).max()) > 3


# ------------------------------------------------------------------------------------------- mutants of the bookkeeping
def _leaves_bounds(m, mutant, groups):
    """the mutant's raw advantages leave E, and its normalised advantages and targets their bounds, in every listed tensor"""
    for k in groups:
        assert (np.abs(mutant["raw"][k] - m["raw"][k]) > m["E"][k]).any(), k
        assert (np.abs(mutant["adv"][k] - m["adv"][k]) > m["adv_bound"][k]).any(), k
        assert (np.abs(mutant["targets"][k] - m["targets"][k]) > m["target_bound"][k]).any(), k


@pytest.mark.parametrize("name,bufs,g,lam", _buffer_sets(), ids=[b[0] for b in _buffer_sets()])
def test_bookkeeping_mutant_permuted_reward_channels_leaves_the_bounds(name, bufs, g, lam):
    """pt / tt / it read from one another's reward channel (r4 is ordered mk, idle, pt, tt; the advantages mk, pt, tt, it)"""
    m = ref.compose64(gamma=g, lam=lam, **bufs)
    for perm in ([0, 2, 3, 1], [0, 3, 1, 2], [0, 1, 3, 2]):
        mut = dict(bufs, buf_r=np.ascontiguousarray(bufs["buf_r"][:, perm]))
        moved = [i for i, ch in enumerate((0, 2, 3, 1)) if perm[ch] != ch]       # advantage channels whose reward changed
        _leaves_bounds(m, ref.compose64(gamma=g, lam=lam, **mut), moved + [4 + i for i in moved])


@pytest.mark.parametrize("name,bufs,g,lam", [b for b in _buffer_sets() if b[1]["buf_jv"].shape[0] > 1],
                         ids=[b[0] for b in _buffer_sets() if b[1]["buf_jv"].shape[0] > 1])
def test_bookkeeping_mutant_terminal_value_from_the_next_episode_leaves_the_bounds(name, bufs, g, lam):
    """v_ of an episode's last step taken from the next episode's first slot instead of the post-terminal slot (the last episode
    has no next one and keeps its own): the local advantages move, the global ones do not read these slots"""
    m = ref.compose64(gamma=g, lam=lam, **bufs)
    jv, mv = bufs["buf_jv"].copy(), bufs["buf_mv"].copy()
    jv[:-1, -1], mv[:-1, -1] = jv[1:, 0], mv[1:, 0]
    mut = ref.compose64(gamma=g, lam=lam, **dict(bufs, buf_jv=jv, buf_mv=mv))
    _leaves_bounds(m, mut, [4, 5, 6, 7])
    assert np.array_equal(mut["raw"][:4], m["raw"][:4])

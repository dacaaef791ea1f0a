"""Host model of mtfjsp_walk_accept and of baselines.walk_search (plain module; tests/test_walk_cpu.py pins it on hand-written rows,
tests/test_walk_accept_gpu.py and tests/test_walk_search_gpu.py hold the device to it bit for bit).  The rule of include/mtfjsp.h is
applied literally, group by group and copy by copy; `search` drives the C oracle, the host models of the moves
(tests/critical_path_ref.py), of the objectives (tests/group_reduce_ref.py) and of the signature (tests/beam_ref.py)."""
import numpy as np

import group_reduce_ref as gref

COST_KEYS = ("opr_Gt", "opr_mk", "opr_idleT", "opr_pt", "opr_transT")
CONFIG_W = (0.4, 0.4, 0.2)
SENT_F, SENT_I, SENT_U, SENT_B = -12345.5, -777, 0xDEADBEEFCAFEF00D, -99
_U = np.uint64


def new_state(N, T, late_len, tabu_len):
    """-> the state of N groups, every cell a sentinel: the first call (first=True) must not read it and fills what the rule names"""
    return dict(late=np.full((N, late_len), SENT_F), tabu=np.full((N, tabu_len), SENT_U, np.uint64), tabu_n=np.full(N, SENT_I, np.int32),
                best_obj=np.full(N, SENT_F), best_task=np.full((T, N), SENT_I, np.int32), best_mach=np.full((T, N), SENT_I, np.int32))


def accept(cost4, done, w, N, K, sig, task, mach, round, first, slack, state):
    """cost4 [N*K,4], done [N*K], w as `group_reduce_ref.group_reduce` takes them; sig [N*K] uint64 or None; task, mach [T, N*K] int32;
    slack: a float (negative or NaN: off) or None (off); state: dict of `new_state` — late_len and tabu_len are its shapes; it is not
    modified.  -> (out, state'): out = dict(next_col, pick, barred [N] int32, cur_obj, best_obj [N] f64, why [N] int8, obj [N*K] f64)"""
    cost4 = np.asarray(cost4, np.float64).reshape(N * K, 4)
    done = np.asarray(done).reshape(N * K)
    task, mach = np.asarray(task), np.asarray(mach)
    slack = np.float64(-1.0 if slack is None else slack)
    st = {k: v.copy() for k, v in state.items()}
    late, tabu, tabu_n, best_obj = st["late"], st["tabu"], st["tabu_n"], st["best_obj"]
    late_len, tabu_len = late.shape[1], tabu.shape[1]
    # 1 objectives
    mk, ec, tt, obj = gref.objectives(cost4, w)
    elig = (done != 0) & ~np.isnan(mk) & ~np.isnan(ec) & ~np.isnan(tt)
    obj = np.where(elig, obj, np.nan)
    out = dict(next_col=np.zeros(N, np.int32), pick=np.zeros(N, np.int32), barred=np.zeros(N, np.int32), cur_obj=np.zeros(N),
               best_obj=np.zeros(N), why=np.zeros(N, np.int8), obj=obj)
    for n in range(N):
        g0 = n * K
        go = obj[g0:g0 + K]
        cur = go[0]
        # 2 first call
        if first:
            late[n, :] = cur
            if tabu_len > 0:
                tabu_n[n] = 0
            best_obj[n] = cur
            st["best_task"][:, n], st["best_mach"][:, n] = task[:, g0], mach[:, g0]
        # 3 candidates
        ring = [int(x) for x in tabu[n, :min(max(int(tabu_n[n]), 0), tabu_len)]] if tabu_len > 0 else []
        cand, barred = [], 0
        for c in range(1, K):
            if go[c] != go[c]:
                continue
            if sig is not None and (int(sig[g0 + c]) == int(sig[g0]) or int(sig[g0 + c]) in ring):
                barred += 1
                continue
            cand.append(c)
        # 4 pick
        pick = -1
        for c in cand:                                                  # ascending, strict: ties stay with the lowest c
            if pick < 0 or go[c] < go[pick]:
                pick = c
        # 5 why
        slot = int(round) % late_len if late_len > 0 else 0
        if pick < 0:
            why = 0
        elif cur != cur or go[pick] < cur:
            why = 2
        elif slack >= 0 and go[pick] <= cur + slack:
            why = 3
        elif late_len > 0 and go[pick] <= late[n, slot]:
            why = 4
        else:
            why = 1
        # 6 move or stay
        if why >= 2:
            if tabu_len > 0:
                tabu[n, int(tabu_n[n]) % tabu_len] = _U(int(sig[g0]))
                tabu_n[n] += 1
            out["next_col"][n], now = g0 + pick, go[pick]
        else:
            out["next_col"][n], now = (g0 if cur == cur else -1), cur
        # 7 late ring
        if late_len > 0:
            late[n, slot] = now
        # 8 best so far
        if why >= 2 and (best_obj[n] != best_obj[n] or now < best_obj[n]):
            best_obj[n] = now
            st["best_task"][:, n], st["best_mach"][:, n] = task[:, g0 + pick], mach[:, g0 + pick]
            why += 8
        # 9 outputs
        out["cur_obj"][n], out["best_obj"][n], out["pick"][n], out["why"][n], out["barred"][n] = now, best_obj[n], pick, why, barred
    return out, st


# ---- constructed cases (tests/test_walk_cpu.py proves on the model that each shows what it is there for; tests/test_walk_accept_gpu.py
# runs them on the device)
# exact objectives: with these weights obj = (1.0*mk + -0.0*ec) + -0.0*tt is mk's own word for every finite mk, zeros of both signs
# included (x + -0.0 == x, -0.0 + -0.0 == -0.0), as long as ec and tt are +0.0; an infinite ec makes it NaN
W_EXACT = (1.0, -0.0, -0.0)
KINDS = ("random", "shared_min", "last_min", "second", "all_barred", "dead0", "zeros", "nan_obj", "slack_edge", "late_only", "no_new_best",
         "readmit")
SLACKS = (None, 0.0, 2.0, np.inf, -1.0, np.nan)


def _call(N, K, rows, slack, rest=(200.0, None)):
    """one call with exact objectives: rows = {c: (obj or None: not done, sig)}, every other copy `rest`; a sig of None is one no other copy
    has; group n's objectives are shifted by 1000 n (zeros stay zeros) and its signatures by n << 32"""
    cost4, done, sig = np.zeros((N * K, 4)), np.ones(N * K, np.uint8), np.zeros(N * K, np.uint64)
    for n in range(N):
        for c in range(K):
            o, s = rows.get(c, rest)
            g = n * K + c
            if o is None:
                done[g], o = 0, 7.0
            elif o == "nan":
                cost4[g, 1], o = np.inf, 7.0
            cost4[g, 0] = o if o == 0 else o + 1000.0 * n
            sig[g] = _U((n << 32) + (0x10000 + c if s is None else s))
    return dict(cost4=cost4, done=done, sig=sig, slack=slack, w=W_EXACT)


def synthetic(kind, N, K, seed, late_len=2, tabu_len=3, calls=None):
    """-> a list of calls, each dict(cost4 [N*K,4], done [N*K] uint8, sig [N*K] uint64, slack, w), to be run in order from first = 1 with
    rings of the given lengths.  "random": `calls` calls of objectives from a coarse grid (integer costs 0..3 under the weights 0.4, 0.4,
    0.2) with done = 0 and NaN scattered in, signatures from an alphabet of 2 tabu_len + 4 words and a slack that takes turns through
    SLACKS: frequent ties, ring hits and every `why`; the other kinds are a few scripted calls each (see the tests for what each shows) and
    need K >= 3 to show it"""
    rs = np.random.RandomState(seed)
    if kind == "random":
        out = []
        for i in range(calls or 8):
            cost4 = rs.randint(0, 4, (N * K, 4)).astype(np.float64)
            cost4[rs.uniform(size=(N * K, 4)) < 0.03] = np.nan
            done = (rs.uniform(size=N * K) > 0.1).astype(np.uint8) * rs.randint(1, 256, N * K).astype(np.uint8)
            sig = rs.randint(0, 2 * tabu_len + 4, N * K).astype(np.uint64) * _U(0x9E3779B97F4A7C15)
            for n in range(N):                                          # a random incumbent is beaten nearly always: half of them get the costs of their group's best copy
                o = np.where(done[n * K:(n + 1) * K] != 0, gref.objectives(cost4[n * K:(n + 1) * K], CONFIG_W)[3], np.nan)
                if rs.uniform() < 0.5 and not np.isnan(o).all():
                    cost4[n * K], done[n * K] = cost4[n * K + int(np.nanargmin(o))], 1
            out.append(dict(cost4=cost4, done=done, sig=sig, slack=SLACKS[rs.randint(len(SLACKS))] if calls is None else np.inf, w=CONFIG_W))
        return out
    last, mid = K - 1, min(64, K - 1)
    A, B, C, D = 1, 2, 3, 4                                             # signatures of schedules
    leave = _call(N, K, {0: (100.0, A), 1: (90.0, B)}, None)            # from A to B: the ring holds A afterwards
    if kind == "shared_min":                                            # the lowest of the equal minima
        return [_call(N, K, {0: (100.0, A), 1: (50.0, None), mid: (50.0, None), last: (50.0, None)}, None)]
    if kind == "last_min":
        return [_call(N, K, {0: (100.0, A), last: (50.0, None)}, None)]
    if kind == "second":                                                # the best is the schedule just left, the second best is taken
        return [leave, _call(N, K, {0: (90.0, B), 1: (50.0, A), last: (60.0, C)}, None)]
    if kind == "all_barred":                                            # every candidate is the incumbent's schedule or the one just left
        return [leave, _call(N, K, {0: (90.0, B)}, np.inf, rest=(50.0, A)), _call(N, K, {0: (90.0, B), 1: (50.0, A)}, np.inf, rest=(50.0, B))]
    if kind == "dead0":                                                 # an incumbent that is no plan: with candidates, without
        return [_call(N, K, {0: (None, A), last: (300.0, B)}, None), _call(N, K, {0: (None, A)}, np.inf, rest=(None, None)),
                _call(N, K, {0: (None, A), 1: (400.0, C)}, None)]
    if kind == "zeros":                                                 # equal zeros of both signs: no step without slack, a sideways step with slack 0
        return [_call(N, K, {0: (0.0, A), 1: (-0.0, B)}, None, rest=(5.0, None)), _call(N, K, {0: (0.0, A), 1: (-0.0, B)}, 0.0, rest=(5.0, None)),
                _call(N, K, {0: (-0.0, B), last: (0.0, C)}, 0.0, rest=(5.0, None))]
    if kind == "nan_obj":                                               # done, but 0 * inf: eligible and no candidate
        return [_call(N, K, {0: (100.0, A), 1: ("nan", B)}, np.inf, rest=(None, None)), _call(N, K, {0: (100.0, A), 1: ("nan", B), last: (150.0, C)}, np.inf)]
    if kind == "slack_edge":                                            # cur + slack itself, the next binary64 above it, anything under +inf
        edge = [np.float64(100.0 + 1000.0 * n) + np.float64(0.3) for n in range(N)]
        calls = [_call(N, K, {0: (100.0, A), 1: (100.0, B)}, 0.3, rest=(1e6, None)) for _ in range(2)]
        for n in range(N):
            calls[0]["cost4"][n * K + 1, 0], calls[1]["cost4"][n * K + 1, 0] = edge[n], np.nextafter(edge[n], np.inf)
        return calls + [_call(N, K, {0: (100.0, A), last: (1e300, B)}, np.inf, rest=(None, None))]
    if kind == "late_only":                                             # worse than the incumbent, not worse than it was late_len rounds ago
        return [_call(N, K, {0: (100.0, A), 1: (90.0, B)}, None), _call(N, K, {0: (90.0, B), last: (95.0, C)}, None),
                _call(N, K, {0: (95.0, C), 1: (99.0, D)}, None)]
    if kind == "no_new_best":                                           # an uphill step keeps the best plan
        return [leave, _call(N, K, {0: (90.0, B), 1: (95.0, C)}, np.inf)]
    if kind == "readmit":                                               # A is barred while it is in the ring and taken once tabu_len + 1 moves have passed
        out = [leave]
        for i in range(tabu_len + 1):
            out.append(_call(N, K, {0: (90.0 + i, B + i), 1: (50.0, A), last: (91.0 + i, B + i + 1)}, np.inf))
        return out
    raise ValueError(kind)


def run(calls, N, K, T, late_len, tabu_len, seed):
    """the calls of `synthetic` through `accept`, from a state of sentinels, with random words as plans
    -> (plans: [(task, mach)] per call, outs: [out] per call, states: [state after the call] per call)"""
    rs = np.random.RandomState(seed + 1)
    state = new_state(N, T, late_len, tabu_len)
    plans, outs, states = [], [], []
    for i, c in enumerate(calls):
        task, mach = rs.randint(-5, 1 << 20, (T, N * K)).astype(np.int32), rs.randint(-5, 1 << 20, (T, N * K)).astype(np.int32)
        out, state = accept(c["cost4"], c["done"], c["w"], N, K, c["sig"], task, mach, i, i == 0, c["slack"], state)
        plans.append((task, mach)); outs.append(out); states.append(state)
    return plans, outs, states


def search(data, start, K, rounds, seed, moves=7, left_shift=False, w=CONFIG_W, tabu=8, slack=np.inf, late=0, first_instance=0, trace=None):
    """baselines.walk_search on the host -> dict(start_obj [N], history, current [rounds,N], accepted, why [rounds,N] int8, barred
    [rounds,N] int32, plans (task, mach) [N,T], cost {key: [N]}, final4 [N,4], obj [N]).  trace: a list that gets one dict per round
    (sig [N*K], ring: the valid entries per group before the call, obj, pick, next_col) for the tests about the ring"""
    import beam_ref
    import critical_path_ref as cref
    t, tt = np.asarray(data[0]), np.asarray(data[2])
    N, T, M = t.shape
    J = T // M
    slacks = [slack] * rounds if slack is None or np.ndim(slack) == 0 else list(slack)
    assert len(slacks) == rounds
    task, mach = np.array(start[0], np.int32), np.array(start[1], np.int32)
    rep = tuple(np.repeat(np.asarray(x), K, axis=0) for x in data)
    state = new_state(N, T, late, tabu)
    keys = ("history", "current", "accepted", "why", "barred")
    rows = {k: [] for k in keys}
    start_obj, paths = None, None
    if rounds and moves & cref.CRIT_MOVES:
        paths = cref.path_rows(cref.replay(data, task, mach, left_shift, w)[4], tt, J, M)
    for r in range(rounds):
        if paths is None:
            nt, nm, kind = cref.pref.neighbours(t, task, mach, K, seed, r, first_instance, moves)
        else:
            nt, nm, kind = cref.neighbours(t, task, mach, K, seed, r, first_instance, moves, paths)
        _, final4, done, _, sched = cref.replay(rep, nt, nm, left_shift, w)
        sig = beam_ref.state_signature(sched)
        ring = [state["tabu"][n, :min(max(int(state["tabu_n"][n]), 0), tabu)].copy() if r else np.zeros(0, np.uint64) for n in range(N)]
        out, state = accept(final4, done, w, N, K, sig, np.ascontiguousarray(nt.T), np.ascontiguousarray(nm.T), r, r == 0, slacks[r], state)
        col = out["next_col"]
        assert (col >= 0).all()
        if r == 0:
            start_obj = out["obj"][::K].copy()
        if trace is not None:
            trace.append(dict(sig=sig, ring=ring, obj=out["obj"], pick=out["pick"].copy(), next_col=col.copy()))
        rows["history"].append(out["best_obj"]); rows["current"].append(out["cur_obj"]); rows["why"].append(out["why"])
        rows["barred"].append(out["barred"])
        rows["accepted"].append(np.where((out["why"] & 7) < 2, -1, kind[col]).astype(np.int8))
        task, mach = nt[col], nm[col]
        if paths is not None:
            paths = cref.path_rows(sched, rep[2], J, M, col)
    if rounds:
        task, mach = np.ascontiguousarray(state["best_task"].T), np.ascontiguousarray(state["best_mach"].T)
    cum, final4, done, obj, _ = cref.replay(data, task, mach, left_shift, w)
    assert done.all()
    dt = dict(history=np.float64, current=np.float64, accepted=np.int8, why=np.int8, barred=np.int32)
    res = {k: np.array(rows[k], dt[k]).reshape(rounds, N) for k in keys}
    res.update(start_obj=obj.copy() if start_obj is None else start_obj, plans=(task, mach), cost={key: cum[:, i] for i, key in enumerate(COST_KEYS)},
               final4=final4, obj=obj)
    return res

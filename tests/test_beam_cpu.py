"""No GPU: the host model of the beam search (tests/beam_ref.py) on J3M3 with W = 3 — the yardstick of tests/test_beam_gpu.py must
itself be right: every live slot's prefix is a valid action sequence, episodes finish in T steps, an independent enumeration (one
single-instance oracle per child, `sorted`) ranks the same survivors with the same value bits, merged beams hold no two equal
schedules, distinct schedules never share a signature on the test data, and the tie-rich data really makes duplicates."""
import numpy as np
import pytest

import beam_ref as ref
from oracle.env_oracle import OracleBatch

J, M, E, N, W = 3, 3, 3, 5, 3
T = J * M


def _state_key(state, i):
    return state["mach"][i].tobytes() + state["st"][i].tobytes() + state["routes"][i].tobytes()


def _slot_states(rec):
    """state key of every live slot after the step, from the children the slots were forked from"""
    return [None if g < 0 else _state_key(rec["children"], g) for g in rec["parent"]]


@pytest.mark.parametrize("dedupe", [True, False], ids=["dedupe", "plain"])
@pytest.mark.parametrize("column", [0, 2])
def test_prefixes_are_valid_and_episodes_finish(column, dedupe):
    data, recs = ref.cached_episode(J, M, E, N, W, column, dedupe, True)
    t, p, tt, edge, w3 = data
    assert len(recs) == T
    final, score = recs[-1]["prefixes"], recs[-1]["score"]
    for n in range(N):
        assert final[n * W] is not None, "slot 0 is never empty"
        live = [final[n * W + k] is not None for k in range(W)]
        assert live == sorted(live, reverse=True), "ranks come out in order: empty slots are the last ones"
        s = score[n * W:(n + 1) * W]
        assert all(s[k] >= s[k + 1] for k in range(W - 1)), "scores descend with the rank"
    for i, prefix in enumerate(final):
        if prefix is None:
            assert score[i] == -np.inf
            continue
        n = i // W
        one = lambda x: np.asarray(x)[n:n + 1]                          # noqa: E731
        orc = OracleBatch(one(t), one(p), one(tt), one(edge), w_cfg=ref.CONFIG_W); orc.scaler_init(); orc.reset(one(w3))
        cand, mask = orc.job_mask_state()
        total = 0.0
        assert len(prefix) == T
        for a, m in prefix:
            j = a // M
            assert mask[0, j] == 0 and cand[0, j] == a, f"slot {i}: not a candidate"
            assert t[n, a, m] >= 0, f"slot {i}: infeasible machine"
            info, raw, _ = orc.step(np.array([a], np.int32), np.array([m], np.int32))
            total = total + raw[0, column]
            orc.job_mask_update(np.array([j], np.int32))
            cand, mask = orc.job_mask_state()
        assert info[0, 1] == 1.0 and mask.all(), f"slot {i}: the episode finishes in T steps"
        assert np.float64(total).view(np.int64) == score[i].view(np.int64), "the score is the running sum of the one-step rewards"


@pytest.mark.parametrize("dedupe", [True, False], ids=["dedupe", "plain"])
@pytest.mark.parametrize("s", [0, 4, T - 1])
def test_an_independent_enumeration_ranks_the_same_survivors(s, dedupe):
    """every child of step s again, one at a time, each on an oracle of its own; ranking by `sorted` on (-value, c), duplicates
    told apart by comparing the state arrays themselves (no signature)"""
    column = 2
    data, recs = ref.cached_episode(J, M, E, N, W, column, dedupe, True)
    t, p, tt, edge, w3 = data
    prefixes, scores = recs[s]["before"]
    for n in range(N):
        one = lambda x: np.asarray(x)[n:n + 1]                          # noqa: E731
        seen = []
        for w in range(W):
            prefix = prefixes[n * W + w]
            if prefix is None:
                continue
            for r in range(T):
                orc = OracleBatch(one(t), one(p), one(tt), one(edge), w_cfg=ref.CONFIG_W); orc.scaler_init(); orc.reset(one(w3))
                for a, m in prefix:
                    orc.step(np.array([a], np.int32), np.array([m], np.int32)); orc.job_mask_update(np.array([a // M], np.int32))
                cand, mask = orc.job_mask_state()
                j, m = divmod(r, M)
                if mask[0, j] or t[n, cand[0, j], m] < 0:
                    continue
                _, raw, _ = orc.step(cand[:1, j], np.array([m], np.int32))
                value = scores[n * W + w] + raw[0, column]
                seen.append((-value, w * T + r, _state_key(orc.state(), 0), w, int(cand[0, j]), m))
        ranked, keys = [], set()
        for x in sorted(seen, key=lambda x: (x[0], x[1])):
            if dedupe and x[2] in keys:
                continue
            keys.add(x[2])
            ranked.append(x)
        ranked = ranked[:W]
        rec = recs[s]
        for k in range(W):
            i = n * W + k
            if k >= len(ranked):
                assert rec["parent"][i] == -1 and rec["from_slot"][i] == -1 and rec["task"][i] == -1 and rec["score"][i] == -np.inf
                continue
            neg, c, _, w, a, m = ranked[k]
            assert rec["parent"][i] == n * W * T + c and rec["from_slot"][i] == w and rec["task"][i] == a and rec["mach"][i] == m, f"instance {n} rank {k}"
            assert np.float64(-neg).view(np.int64) == rec["score"][i].view(np.int64), f"instance {n} rank {k}: value bits"


@pytest.mark.parametrize("ties", [False, True], ids=["generated", "tie_rich"])
def test_a_merged_beam_holds_no_two_equal_schedules(ties):
    _, recs = ref.cached_episode(J, M, E, N, W, 2, True, False, ties)
    for s, rec in enumerate(recs):
        keys = _slot_states(rec)
        for n in range(N):
            live = [k for k in keys[n * W:(n + 1) * W] if k is not None]
            assert len(live) == len(set(live)), f"step {s} instance {n}: two slots hold one schedule"


@pytest.mark.parametrize("ties", [False, True], ids=["generated", "tie_rich"])
@pytest.mark.parametrize("left_shift", [True, False], ids=["left_shift", "no_left_shift"])
def test_distinct_schedules_never_share_a_signature(left_shift, ties):
    """over every child of every step of an episode (all instances together: the task data differ, so do the start times)"""
    _, recs = ref.cached_episode(J, M, E, N, W, 2, True, left_shift, ties)
    n_equal = 0
    for rec in recs:
        for n in range(N):                                              # children of one instance: the only ones the selection compares
            by_sig = {}
            for g in range(n * W * T, (n + 1) * W * T):
                if not rec["eligible"][g]:
                    continue
                key = _state_key(rec["children"], g)
                other = by_sig.setdefault(int(rec["sigs"][g]), key)
                assert other == key, "two distinct schedules share a signature"
            keys = [_state_key(rec["children"], g) for g in range(n * W * T, (n + 1) * W * T) if rec["eligible"][g]]
            n_equal += len(keys) - len(set(keys))
            assert len(set(keys)) == len(by_sig), "equal schedules have equal signatures"
    if ties and not left_shift:
        assert n_equal > 0, "tie-rich data without left shift: some children are the same schedule reached in two orders"


def test_tie_rich_data_fills_a_plain_beam_with_duplicates():
    """a condition on the INPUTS of the GPU dedupe cases: without merging, the W = 4 beam on the tie-rich J3M3 instances holds two
    slots with equal states at some step, and merging changes the survivors — otherwise those cases would prove nothing"""
    _, plain = ref.cached_episode(J, M, E, N, 4, 2, False, False, True)
    _, merged = ref.cached_episode(J, M, E, N, 4, 2, True, False, True)
    dup = 0
    for rec in plain:
        keys = _slot_states(rec)
        for n in range(N):
            live = [k for k in keys[n * 4:(n + 1) * 4] if k is not None]
            dup += len(live) - len(set(live))
    assert dup > 0
    assert any(not np.array_equal(a["parent"], b["parent"]) for a, b in zip(plain, merged))


def test_signature_of_a_fresh_instance_is_zero_and_mix_is_splitmix64():
    # splitmix64's published test vector: the first output for seed 0 is mix(0 + 0x9e3779b97f4a7c15)
    assert int(ref.mix(np.array([0x9e3779b97f4a7c15], np.uint64))[0]) == 0xe220a8397b1dcdaf
    t, p, tt, edge, w3 = ref.cached_data(J, M, E, N)
    orc = OracleBatch(t, p, tt, edge, w_cfg=ref.CONFIG_W); orc.scaler_init(); orc.reset(w3)
    assert not ref.state_signature(orc.state()).any()

"""No GPU: the host model of the one-step look-ahead rules (tests/lookahead_ref.py) on J3M4 — the yardstick of
tests/test_lookahead_gpu.py must itself be right: every pick is valid, episodes finish in T steps, and at an independently replayed
step no valid candidate beats the pick (larger value, or equal value at a lower index).  The selection rule itself (`ref.select`) is
pinned on hand-written rows: ties across index 63 / 64, -inf, NaN, both zeros, a copy that does not count."""
import numpy as np
import pytest

import lookahead_ref as ref
from oracle.env_oracle import OracleBatch

J, M, E, B = 3, 4, 2, 4
T = J * M


@pytest.mark.parametrize("column", range(5))
def test_model_picks_are_valid_and_episodes_finish(column):
    (t, p, tt, edge, w3), task, mach, best = ref.cached_episode(J, M, E, B, column, True)
    assert task.shape == (T, B) and mach.shape == (T, B) and np.isfinite(best).all()
    orc = OracleBatch(t, p, tt, edge, w_cfg=ref.CONFIG_W); orc.scaler_init(); orc.reset(w3)
    cand, mask = orc.job_mask_state()
    for s in range(T):
        job = task[s] // M
        assert (mask[np.arange(B), job] == 0).all() and (cand[np.arange(B), job] == task[s]).all(), f"step {s}: not a candidate"
        assert (t[np.arange(B), task[s], mach[s]] >= 0).all(), f"step {s}: infeasible machine"
        info, raw, _ = orc.step(task[s], mach[s])
        assert np.array_equal(raw[:, column], best[s]), f"step {s}: the value of the pick is the value the model reported"
        orc.job_mask_update(job)
        cand, mask = orc.job_mask_state()                               # 1 = the job is finished (not the policy's column mask)
    assert info[:, 1].all() and mask.all()


@pytest.mark.parametrize("column", [0, 2, 4])
@pytest.mark.parametrize("s", [0, 5, T - 1])
def test_no_valid_candidate_beats_the_pick(column, s):
    """every candidate of step s again, one at a time, each on an oracle of its own (no replica batch, no masking arithmetic)"""
    (t, p, tt, edge, w3), task, mach, best = ref.cached_episode(J, M, E, B, column, True)
    for b in range(B):
        one = lambda x: np.asarray(x)[b:b + 1]                          # noqa: E731
        seen = []
        for c in range(T):
            orc = OracleBatch(one(t), one(p), one(tt), one(edge), w_cfg=ref.CONFIG_W); orc.scaler_init(); orc.reset(one(w3))
            for k in range(s):
                orc.step(task[k, b:b + 1], mach[k, b:b + 1]); orc.job_mask_update(task[k, b:b + 1] // M)
            cand, mask = orc.job_mask_state()
            j, m = divmod(c, M)
            if mask[0, j] or t[b, cand[0, j], m] < 0:
                continue
            _, raw, _ = orc.step(cand[:1, j], np.array([m], np.int32))
            seen.append((c, cand[0, j], m, raw[0, column]))
        pick = [x for x in seen if x[1] == task[s, b] and x[2] == mach[s, b]]
        assert len(pick) == 1 and pick[0][3] == best[s, b]
        for c, _, _, v in seen:
            assert v <= pick[0][3] and not (v == pick[0][3] and c < pick[0][0]), f"instance {b}: candidate {c} beats the pick"


def test_select_on_hand_written_rows():
    """the selection rule itself (ref.select), where no episode asks: ties across a pass boundary, -inf, NaN, both zeros, and a
    copy that does not count"""
    inf, nan = np.inf, np.nan
    # a tie across index 63 / 64: the lower index; with 63 not counting, the next one
    v = np.full(130, 1.0); v[[63, 64, 129]] = 7.5
    ok = np.ones(130, bool)
    assert ref.select(v, ok) == 63
    ok[63] = False
    assert ref.select(v, ok) == 64
    ok[64] = False
    assert ref.select(v, ok) == 129
    # only -inf counts: -inf is a value, the lowest COUNTING index wins (copy 0 does not count, whatever it holds)
    v = np.array([-inf, 3.0, -inf, -inf, 5.0]); ok = np.array([False, False, True, True, False])
    assert ref.select(v, ok) == 2 and v[ref.select(v, ok)] == -inf
    assert ref.select(np.full(4, -inf), np.array([False, True, True, True])) == 1
    # only NaN counts: nothing; a NaN beside values is passed over, also at index 0
    assert ref.select(np.array([nan, nan, 1.0]), np.array([True, True, False])) is None
    assert ref.select(np.array([nan, -2.0, nan, -2.0]), np.ones(4, bool)) == 1
    assert ref.select(np.array([nan, -inf]), np.ones(2, bool)) == 1
    # nothing counts, and the empty row
    assert ref.select(np.array([1.0, 2.0]), np.zeros(2, bool)) is None and ref.select(np.zeros(0), np.zeros(0, bool)) is None
    # the two zeros are equal: the lower index, and the value is that copy's own zero
    for lo, hi in ((-0.0, 0.0), (0.0, -0.0)):
        v = np.array([-1.0, lo, -3.0, hi, -1.0]); ok = np.ones(5, bool)
        c = ref.select(v, ok)
        assert c == 1 and np.signbit(v[c]) == np.signbit(lo)
    # a copy that does not count holds the largest value (+inf included)
    assert ref.select(np.array([9.0, 1.0, 2.0, inf]), np.array([False, True, True, False])) == 2
    assert ref.select(np.array([1.0, inf, inf]), np.ones(3, bool)) == 1

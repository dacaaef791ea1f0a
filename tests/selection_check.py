"""assert_selection_exact: the index a selecting launch wrote is the one the host model (tests/device_streams_ref.py) picks from the
probabilities THE SAME LAUNCH wrote — equality on every instance, no tolerance — and its log-probability is log of that stored binary32
probability.  Test infrastructure only.

The log-probability is the one figure that is not an equality: the kernels compute logf(p) in binary32, the expected value is the
binary64 log of the stored binary32 p.  Its error, in binary32 ulps of the expected value, is recorded per launch form — the ledger of
a test run is written to $MTFJSP_LEDGER_DIR/selection_logp_ulps_observed.json when the interpreter exits (only where that variable is
set; the file is replaced), and one GPU run's ledger is committed as profiles/selection_logp_ulps.json — and asserted against twice the
committed maximum of the form, never above 3 ulps (the OpenCL full-profile bound for log, which the ROCm device library implements; no OCML accuracy table ships with the toolchain to quote a tighter
one) and never below 1 ulp.  A form the committed ledger does not know is held to the 3 ulps.  -inf (a zero probability) is compared by
equality, and so is log(1) = 0."""
import atexit
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import device_streams_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEDGER_FILE = os.path.join(ROOT, "profiles", "selection_logp_ulps.json")
CAP_ULPS, FLOOR_ULPS, MARGIN = 3.0, 1.0, 2.0

try:
    _ledger = json.load(open(LEDGER_FILE))["max_ulps"]
except (OSError, ValueError, KeyError) as ex:
    raise RuntimeError(f"tests/selection_check.py: the committed ledger {LEDGER_FILE} is missing or unreadable ({ex})") from ex
_observed = {}


def _flush():
    out = os.environ.get("MTFJSP_LEDGER_DIR")
    if not _observed or not out:
        return
    try:
        os.makedirs(out, exist_ok=True)
        json.dump({"what": "max |logp - log(p)| in binary32 ulps of log(p) per launch form (p = the stored binary32 probability of the selected entry, "
                           "log in binary64), observed by tests/selection_check.assert_selection_exact in one GPU test run",
                   "max_ulps": _observed}, open(os.path.join(out, "selection_logp_ulps_observed.json"), "w"), indent=1, sort_keys=True)
    except OSError:
        pass


atexit.register(_flush)


def logp_bound(form):
    rec = _ledger.get(form)
    return CAP_ULPS if rec is None else min(CAP_ULPS, max(FLOOR_ULPS, MARGIN * float(rec)))


def _host(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def assert_selection_exact(prob, idx, logp, seed, counter, greedy, gather_from=None, gathered=None, mask=None, form="k_sample"):
    """prob [B,n] f32, idx [B] i32, logp [B] f32 (or None) as one launch left them; gather_from [B,n] / gathered [B]: the launch's
    gather of the selected entry; mask [B,n] bytes: the mask the launch selected under.  -> the largest log-probability error (ulps)"""
    prob, idx = np.ascontiguousarray(_host(prob), np.float32), _host(idx).astype(np.int64)
    B, n = prob.shape
    rows = np.arange(B)
    assert idx.shape == (B,) and (idx >= 0).all() and (idx < n).all(), f"{form}: index outside 0..{n - 1}"
    u = None if greedy else ref.pick_uniform(rows, seed, counter)
    want = ref.pick(prob, greedy, u)
    bad = np.flatnonzero(idx != want)
    assert bad.size == 0, (f"{form} (seed {seed}, counter {counter}, greedy {bool(greedy)}): {bad.size} of {B} instances picked another index than the model; "
                           f"first: instance {bad[0]}, device {idx[bad[0]]}, model {want[bad[0]]}, row {prob[bad[0]].tolist()}, u {None if u is None else float(u[bad[0]])}")
    if gather_from is not None:
        assert np.array_equal(_host(gathered), _host(gather_from)[rows, idx]), f"{form}: gathered entry is not gather_from[b, idx]"
    sel = prob[rows, idx]
    live = (prob > 0).any(1)
    assert (sel[live] > 0).all(), f"{form}: an entry of probability zero was selected"
    if mask is not None:
        m = _host(mask).reshape(B, n)
        assert (m[rows, idx][live] == 0).all(), f"{form}: a masked entry was selected"
        assert ((prob > 0) <= (m == 0)).all(), f"{form}: a masked entry has a positive probability"
    worst = 0.0
    if logp is not None:
        got = _host(logp).astype(np.float64)
        with np.errstate(divide="ignore"):
            exp = np.log(sel.astype(np.float64))
        exact = ~np.isfinite(exp) | (exp == 0.0)                         # log(0) = -inf, log(1) = 0: by equality
        assert np.array_equal(got[exact], exp[exact]), f"{form}: log-probability of a probability 0 or 1"
        if (~exact).any():
            err = np.abs(got[~exact] - exp[~exact]) / np.spacing(np.abs(exp[~exact]).astype(np.float32)).astype(np.float64)
            worst = float(err.max())
            _observed[form] = max(_observed.get(form, 0.0), worst)
            b = logp_bound(form)
            assert worst <= b, f"{form}: log-probability off by {worst:.3f} binary32 ulps (bound {b}, committed {_ledger.get(form)})"
    return worst

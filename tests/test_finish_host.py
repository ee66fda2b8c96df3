"""CPU test of what a fit computes behind the sampling (api._finish): for the option combinations default, pool_chains, predict_observation alone,
loo_predict and stack_chains, WHICH wrapper is called with WHICH arguments, in which order, and the Results fields that tell the paths apart
(BNRPrediction.draws, waic["pit_i"], stat_chains, the k-hat threshold's draw count).  No GPU: the chain set is a fake whose chains record the
Chain methods called on them, the _capi wrappers on lists of chains are replaced by recorders that return arrays of the right shapes, and
the device_* functions of api.py are wrapped (they still run) so that the list also shows through which of them a call went.

Every recorded call is (name, arguments in the order of the real function's parameters with its defaults filled in), so an argument passed
by position or by keyword reads the same; chains appear by name, arrays as "arr", the new rows as "X"."""
import inspect
import math

import numpy as np
import pytest

from bnr_amd import _capi, api
from bnr_amd.api import Results

N, V, R, TOT = 5, 3, 2, 10
Q = V * (V + 1) // 2
NB, NS = 4, 6                                  # burn-in and window: rows 5 .. 10
INTERVAL, PRED_SEED, R_EFF = 50, 99, 0.5
M = 4                                          # new rows


def _tag(v):
    if isinstance(v, FakeChain):
        return v.name
    if isinstance(v, (list, tuple)) and v and all(isinstance(c, FakeChain) for c in v):
        return tuple(c.name for c in v)
    if isinstance(v, _capi.XInput):
        return "X"
    if isinstance(v, np.ndarray):
        return "arr"
    return v


def _record(log, name, real, args, kwargs, this=None):
    """this: the chain of a Chain method (bound in place of self)"""
    b = inspect.signature(real).bind(*(((this,) if this is not None else ()) + tuple(args)), **kwargs)
    b.apply_defaults()
    log.append((name,) + tuple(_tag(v) for v in b.arguments.values()))


def _vec(n, base):
    return base + np.arange(n, dtype=np.float64) / 8.0


class FakeChain:
    def __init__(self, name, log):
        self.name, self.log = name, log
        self.n, self.q, self.V, self.R, self.tot = N, Q, V, R, TOT

    def fetch(self, *a, **k):
        self.log.append(("Chain.fetch", self.name, a[0], a[1]))

    def summary(self, *a, **k):
        _record(self.log, "Chain.summary", _capi.Chain.summary, a, k, this=self)
        return _vec(Q, 0.0), _vec(Q, -1.0), _vec(Q, 1.0), _vec(V, 0.25)

    def predict(self, *a, **k):
        _record(self.log, "Chain.predict", _capi.Chain.predict, a, k, this=self)
        return _vec(M, 0.0), _vec(M, -1.0), _vec(M, 1.0), _vec(M, -2.0), _vec(M, 0.5)

    def loglik_stats(self, *a, **k):
        _record(self.log, "Chain.loglik_stats", _capi.Chain.loglik_stats, a, k, this=self)
        return _vec(N, -2.0), _vec(N, 0.5)

    def loo(self, *a, **k):
        _record(self.log, "Chain.loo", _capi.Chain.loo, a, k, this=self)
        return _vec(N, -2.0), _vec(N, -2.5), _vec(N, 0.1)


class FakeChainSet:
    def __init__(self, log):
        self.log = log
        self.ids = [1, 2]
        self.chains = {c: FakeChain("c%d" % c, log) for c in self.ids}


def _fake_capi(log):
    K = 2

    def pooled_summary(*a, **k):
        return _vec(Q, 0.0), _vec(Q, -1.0), _vec(Q, 1.0), _vec(V, 0.25)

    def pooled_predict(chains, X, first_row, nsamp, k_lo, k_hi, y=None, x_transform=False, pred_seed=None, pit=False):
        two = (_vec(M, -3.0), _vec(M, 3.0)) if pred_seed is not None else (None, None)
        return (_vec(M, 0.0), _vec(M, -1.0), _vec(M, 1.0), _vec(M, -2.0), _vec(M, 0.5)) + two + (_vec(M, 0.3) / 2 if pit else None,)

    def pooled_loglik_stats(*a, **k):
        return _vec(N, -2.0), _vec(N, 0.5), _vec(N, 0.2) / 2

    def pooled_loo(*a, **k):
        return _vec(N, -2.0), _vec(N, -2.5), _vec(N, 0.1)

    def pooled_loo_predict(*a, **k):
        return (_vec(N, -2.0), _vec(N, -2.5), _vec(N, 0.1), _vec(N, 0.0), _vec(N, 1.0), _vec(N, 0.2) / 2, _vec(N, -2.0), _vec(N, 2.0))

    def chains_stack(*a, **k):
        return np.array([0.75, 0.25]), np.stack([_vec(N, -2.5)] * K), np.stack([_vec(N, 0.1)] * K), _vec(N, -2.4), 1e-10, 7

    def stacked_summary(*a, **k):
        return _vec(Q, 0.0), _vec(Q, -1.0), _vec(Q, 1.0), _vec(V, 0.25)

    def stacked_predict(*a, **k):
        return _vec(M, 0.0), _vec(M, -1.0), _vec(M, 1.0), _vec(M, -2.0), None, None

    fakes = {}
    for f in (pooled_summary, pooled_predict, pooled_loglik_stats, pooled_loo, pooled_loo_predict, chains_stack, stacked_summary, stacked_predict):
        def rec(*a, _f=f, _real=getattr(_capi, f.__name__), **k):
            _record(log, _f.__name__, _real, a, k)
            return _f(*a, **k)
        fakes[f.__name__] = rec
    return fakes


DEVICE_FUNCTIONS = ("device_summary", "device_predict", "device_summary_pooled", "device_predict_pooled", "device_loo_predict", "device_stack_chains",
                    "device_summary_stacked", "device_predict_stacked")


@pytest.fixture
def fit(monkeypatch):
    """finish(**options) -> (Results, the recorded calls) on a fake fit of two chains"""
    log = []
    for name, fake in _fake_capi(log).items():
        monkeypatch.setattr(_capi, name, fake)
    for name in DEVICE_FUNCTIONS:
        def wrap(*a, _name=name, _real=getattr(api, name), **k):
            _record(log, _name, _real, a, k)
            return _real(*a, **k)
        monkeypatch.setattr(api, name, wrap)
    rng = np.random.default_rng(3)
    xi = _capi.XInput(rng.random((M, Q)))
    y_new, y = rng.standard_normal(M), rng.standard_normal(N)

    def finish(pool_chains=False, predict_observation=False, loo_predict=False, stack_chains=False):
        cs = FakeChainSet(log)
        res = Results(None, np.ones(V), np.ones(Q), NB, NS)
        req = api._fit_requests(y, 2, X_new=_capi.XInput(rng.random((N, Q))), nsamp=NS, return_state=True, summary_interval=INTERVAL,
                                predict_X=xi, predict_y=y_new, predict_interval=INTERVAL, waic=True, loo=True, loo_r_eff=R_EFF,
                                pool_chains=pool_chains, predict_observation=predict_observation, pred_seed=PRED_SEED, loo_predict=loo_predict,
                                stack_chains=stack_chains)
        return api._finish(cs, res, req, seed=12345), log
    return finish


LW1, HI1 = api._summary_ranks(NS, INTERVAL)
LW2, HI2 = api._summary_ranks(2 * NS, INTERVAL)
ONE, TWO = ("c1",), ("c1", "c2")
# chain 1's window through the single-chain calls, as a fit without pool_chains / predict_observation makes them
DEFAULT_SUMMARY = [("device_summary", "c1", NB, NS, INTERVAL), ("Chain.summary", "c1", NB + 1, NS, LW1, HI1)]
DEFAULT_PREDICT = [("device_predict", "c1", NB, NS, "X", "arr", INTERVAL, False), ("Chain.predict", "c1", "X", NB + 1, NS, LW1, HI1, "arr", False)]
DEFAULT_WAIC = [("Chain.loglik_stats", "c1", NB + 1, NS)]
DEFAULT_LOO = [("Chain.loo", "c1", NB + 1, NS, R_EFF)]
FETCH = [("Chain.fetch", "c1", 1, TOT)]


def _thr(S):
    return min(1.0 - 1.0 / math.log10(S), 0.7)


def test_default_goes_through_the_single_chain_calls(fit):
    res, log = fit()
    assert log == FETCH + DEFAULT_SUMMARY + DEFAULT_PREDICT + DEFAULT_WAIC + DEFAULT_LOO
    assert res.state is not None and res.summary_device["interval"] == INTERVAL
    assert res.prediction.draws is None and res.prediction.pred_lower_bound is None and res.prediction.pit is None
    assert "pit_i" not in res.waic
    assert res.loo["khat_threshold"] == _thr(NS)
    assert res.stat_chains == 1
    assert res.loo_predictive is None and res.stacking is None and res.essgamma is None


def _pooled_calls(chains, lw, hi, observation):
    return [("device_summary_pooled", chains, NB, NS, INTERVAL), ("pooled_summary", chains, NB + 1, NS, lw, hi),
            ("device_predict_pooled", chains, NB, NS, "X", "arr", INTERVAL, PRED_SEED, False, observation),
            ("pooled_predict", chains, "X", NB + 1, NS, lw, hi, "arr", False, PRED_SEED if observation else None, observation),
            ("pooled_loglik_stats", chains, NB + 1, NS, True), ("pooled_loo", chains, NB + 1, NS, R_EFF)]


def test_pool_chains_goes_through_the_pooled_calls_over_every_chain(fit):
    res, log = fit(pool_chains=True)
    assert log == FETCH + _pooled_calls(TWO, LW2, HI2, False)
    assert res.prediction.draws == 2 * NS and res.prediction.pred_lower_bound is None and res.prediction.pit is None
    assert res.waic["pit_i"] is not None and res.waic["pit_i"].shape == (N,)
    assert res.loo["khat_threshold"] == _thr(2 * NS)
    assert res.stat_chains == 2


def test_predict_observation_alone_goes_through_the_pooled_calls_over_chain_1(fit):
    res, log = fit(predict_observation=True)
    assert log == FETCH + _pooled_calls(ONE, LW1, HI1, True)
    assert res.prediction.draws == NS and res.prediction.pred_lower_bound is not None and res.prediction.pit is not None
    assert res.waic["pit_i"] is not None
    assert res.loo["khat_threshold"] == _thr(NS)
    assert res.stat_chains == 1


def test_loo_predict_replaces_the_loo_call(fit):
    res, log = fit(loo_predict=True)
    p_lo, p_hi = api._loo_interval_probs(INTERVAL)
    assert log == FETCH + DEFAULT_SUMMARY + DEFAULT_PREDICT + DEFAULT_WAIC + [
        ("device_loo_predict", ONE, "arr", NB, NS, INTERVAL, R_EFF), ("pooled_loo_predict", ONE, NB + 1, NS, R_EFF, p_lo, p_hi, _capi.LOO_PREDICT_FIELDS)]
    assert res.loo_predictive is not None and res.loo_predictive.draws == NS
    assert np.array_equal(res.loo["elpd_loo_i"], res.loo_predictive.elpd_loo_i) and res.loo["khat_threshold"] == _thr(NS)
    assert res.prediction.draws is None and "pit_i" not in res.waic and res.stat_chains == 1


def test_stack_chains_adds_its_calls_in_front_and_leaves_the_default_ones(fit):
    res, log = fit(stack_chains=True)
    assert log == [("device_stack_chains", TWO, NB, NS, R_EFF, 100000, 1e-9), ("chains_stack", TWO, NB + 1, NS, R_EFF, 100000, 1e-9),
                   ("device_summary_stacked", TWO, "arr", NB, NS, INTERVAL), ("stacked_summary", TWO, "arr", NB + 1, NS, LW2, HI2),
                   ("device_predict_stacked", TWO, "arr", NB, NS, "X", "arr", INTERVAL, PRED_SEED, False, False),
                   ("stacked_predict", TWO, "arr", "X", NB + 1, NS, LW2, HI2, "arr", False, None)
                   ] + FETCH + DEFAULT_SUMMARY + DEFAULT_PREDICT + DEFAULT_WAIC + DEFAULT_LOO
    assert np.array_equal(res.stacking.weights, [0.75, 0.25]) and res.stacking.summary["interval"] == INTERVAL
    assert res.stacking.prediction.draws == 2 * NS
    assert res.prediction.draws is None and "pit_i" not in res.waic and res.stat_chains == 1


def test_pool_chains_with_loo_predict_is_one_pooled_call_for_both(fit):
    res, log = fit(pool_chains=True, loo_predict=True)
    p_lo, p_hi = api._loo_interval_probs(INTERVAL)
    assert log == FETCH + _pooled_calls(TWO, LW2, HI2, False)[:-1] + [
        ("device_loo_predict", TWO, "arr", NB, NS, INTERVAL, R_EFF), ("pooled_loo_predict", TWO, NB + 1, NS, R_EFF, p_lo, p_hi, _capi.LOO_PREDICT_FIELDS)]
    assert res.loo_predictive.draws == 2 * NS and res.loo["khat_threshold"] == _thr(2 * NS) and res.stat_chains == 2


# ------------------------------------------------------------------------------------------ the analysis options, stated once
# The analysis options of a fit are _fit_requests' parameters after x_transform.  Fit, generate_samples and generate_samples_dbl repeat them in
# their signatures and hand them on as one dict made from that list: these tests hold the four lists equal and follow every option, with a value
# of its own, from Fit down to _fit_requests.
_FIT_REQUESTS_PARAMETERS = list(inspect.signature(api._fit_requests).parameters.values())
OPTIONS = _FIT_REQUESTS_PARAMETERS[[p.name for p in _FIT_REQUESTS_PARAMETERS].index("x_transform") + 1:]
OPTION_NAMES = [p.name for p in OPTIONS]


def test_the_analysis_keywords_of_the_fit_functions_are_those_of_fit_requests():
    assert len(OPTIONS) == 30 and OPTION_NAMES[0] == "return_state" and OPTION_NAMES[-1] == "marginal_loo_predict"
    want = [(p.name, type(p.default), p.default) for p in OPTIONS]
    for fn in (api.Fit, api.generate_samples, api.generate_samples_dbl):
        got = [(p.name, type(p.default), p.default) for p in inspect.signature(fn).parameters.values() if p.name in OPTION_NAMES]
        assert got == want, fn.__name__


class _Marked:
    """a value of an option that is no default and equal to no other"""

    def __init__(self, name):
        self.name = name

    def __repr__(self):
        return "<%s>" % self.name


def _marked_options():
    return {name: _Marked(name) for name in OPTION_NAMES}


def _same_options(kwargs, given):
    return all(kwargs[name] is given[name] for name in OPTION_NAMES)


@pytest.mark.parametrize("doubling", [False, True])
def test_fit_hands_every_analysis_option_to_the_check_and_to_the_sampler(monkeypatch, doubling):
    calls = []

    def recorder(name):
        def f(*a, **k):
            calls.append((name, a, k))
            return name
        return f

    for name in ("_fit_requests", "generate_samples", "generate_samples_dbl"):
        monkeypatch.setattr(api, name, recorder(name))
    given = _marked_options()
    X, y = np.zeros((N, Q)), np.zeros(N)
    out = api.Fit(X, y, R, filename=None, seed=5, num_chains=3, **(dict(mingen=10, maxgen=20) if doubling else {}), **given)
    sampler = "generate_samples_dbl" if doubling else "generate_samples"
    assert out == sampler and [c[0] for c in calls] == ["_fit_requests", sampler]        # the check first, then the one sampler
    _, a, k = calls[0]
    assert len(a) == 2 and a[0] is y and a[1] == 3 and sorted(k) == sorted(OPTION_NAMES) and _same_options(k, given)
    _, a, k = calls[1]
    assert a[0] is X and a[1] is y and a[2] == R and _same_options(k, given)
    assert k["num_chains"] == 3 and k["seed"] == 5 and k["xi_weights"] == "log"


class _FakeRun:
    """what generate_samples / generate_samples_dbl need of a ChainSet that converged at once"""
    chains = {}

    def __init__(self, *a, **k):
        pass

    def init_prior(self):
        pass

    def run(self, *a, **k):
        pass

    def close(self):
        pass


@pytest.mark.parametrize("sampler, window, nsamp", [("generate_samples", dict(nburn=6, nsamp=4), 4), ("generate_samples_dbl", dict(mingen=9, maxgen=9), 5)])
def test_the_samplers_hand_every_analysis_option_to_fit_requests(monkeypatch, sampler, window, nsamp):
    calls, finished = [], []
    xin = object()
    monkeypatch.setattr(api, "XInput", lambda X, x_transform: xin)
    monkeypatch.setattr(api, "ChainSet", _FakeRun)
    monkeypatch.setattr(api, "return_psrf_VOI", lambda cs, stt, ns, **k: Results(None, np.ones(V), np.ones(Q), stt, ns))
    monkeypatch.setattr(api, "_fit_requests", lambda *a, **k: calls.append((a, k)) or "the requests")
    monkeypatch.setattr(api, "_finish", lambda cs, res, req, seed: finished.append((req, seed)) or res)
    given = _marked_options()
    y = np.zeros(N)
    res = getattr(api, sampler)(np.zeros((N, Q)), y, R, seed=5, num_chains=3, x_transform=False, suppress_timer=True, **window, **given)
    (a, k), = calls
    assert len(a) == 5 and a[0] is y and a[1] == 3 and a[2] is xin and a[3] == nsamp and a[4] is False
    assert sorted(k) == sorted(OPTION_NAMES) and _same_options(k, given)
    assert finished == [("the requests", 5)] and res.sampled == nsamp


# the six marginal options: (the option, the keyword of its draws, whether it takes predict_interval, what else the request needs)
MARGINAL_OPTIONS = [("marginal_loo", "marginal_loo_draws", False, {}), ("marginal_edges", "marginal_edges_draws", True, {}),
                    ("marginal_edge_cov", "marginal_edges_draws", False, {}), ("marginal_predict", "marginal_predict_draws", True, {"predict_X": "rows"}),
                    ("marginal_loo_predict", "marginal_loo_draws", True, {}), ("marginal_stack", "marginal_loo_draws", True, {})]
RANKS_MESSAGE = "%s needs every chain of the fit on one rank: the chains are spread over 2 torch.distributed ranks"
DRAWS_MESSAGE = "%s must be an integer >= 1, not %r"
INTERVAL_MESSAGE = "need 0 < p_lo < p_hi < 1, not p_lo = 0.0, p_hi = 1.0"
ROWS_MESSAGE = "%s takes at most 2048 training rows in this version, not 2049"


@pytest.mark.parametrize("option, draws, takes_interval, needs", MARGINAL_OPTIONS)
def test_the_refusals_of_a_marginal_option_and_their_order(monkeypatch, option, draws, takes_interval, needs):
    y = np.zeros(N)
    big = _capi.XInput(np.zeros((_capi.MLOO_MAX_N + 1, 3)))

    def refusal(ranks=1, **kw):
        with monkeypatch.context() as m:
            m.setattr(api, "_rank_world", lambda: (0, ranks))
            m.setattr(api, "_new_rows", lambda *a: "rows")                    # (predict_X is not what is under test)
            with pytest.raises(ValueError) as e:
                api._fit_requests(y, 2, **{option: True}, **needs, **kw)
        return str(e.value)

    for bad in (0, 1.5, True):
        assert refusal(**{draws: bad}) == DRAWS_MESSAGE % (draws, bad)
    assert refusal(ranks=2) == RANKS_MESSAGE % option
    assert refusal(X_new=big, x_transform=False) == ROWS_MESSAGE % option
    if takes_interval:
        assert refusal(predict_interval=100) == INTERVAL_MESSAGE
    # two at once: the ranks before the draws, the draws before the interval (or, without one, the rows), the interval before the rows
    assert refusal(ranks=2, **{draws: 0}) == RANKS_MESSAGE % option
    assert refusal(predict_interval=100, X_new=big, x_transform=False, **{draws: 0}) == DRAWS_MESSAGE % (draws, 0)
    if takes_interval:
        assert refusal(predict_interval=100, X_new=big, x_transform=False) == INTERVAL_MESSAGE
    # and what stands in front of the ranks
    if option == "marginal_predict":
        with monkeypatch.context() as m:
            m.setattr(api, "_rank_world", lambda: (0, 2))
            with pytest.raises(ValueError) as e:
                api._fit_requests(y, 2, marginal_predict=True)
        assert str(e.value) == "marginal_predict needs predict_X"
    if option == "marginal_stack":
        with monkeypatch.context() as m:
            m.setattr(api, "_rank_world", lambda: (0, 2))
            for chains, message in ((1, "marginal_stack needs num_chains >= 2: one chain has nothing to be weighted against"),
                                    (33, "marginal_stack takes at most 32 chains")):
                with pytest.raises(ValueError) as e:
                    api._fit_requests(y, chains, marginal_stack=True)
                assert str(e.value) == message

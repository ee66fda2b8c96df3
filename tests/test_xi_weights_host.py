"""CPU tests of the `xi_weights` model option (include/bnr_hip.h): the reference's node weight as the library computes it
(bnr_host_xi_weight, the kernel's own function) against a numpy restatement of gibbs.jl:349-351, the Python keyword and its
validation, and the Julia shim's switch.  No GPU needed."""
import inspect
import itertools
import os
import re

import numpy as np
import pytest

import bnr_amd
from test_julia_shim import _check_keywords, _fixture, _julia_keywords

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ELLS = [800.0, -800.0, 710.0, -710.0, -745.2, -744.0, -708.5, 0.0, -1.5, 3.0, np.inf, -np.inf, np.nan]
DELTAS = [0.0, 0.5, 1.0, 0.25]


def reference_weight(lt, lb, delta):
    """gibbs.jl:349-351: w_top = (1 - Delta) pdf(top), w_bot = Delta pdf(bot), w = w_top / (w_bot + w_top)"""
    with np.errstate(all="ignore"):
        lt, lb, delta = np.float64(lt), np.float64(lb), np.float64(delta)
        w_top = (np.float64(1.0) - delta) * np.exp(lt)
        w_bot = delta * np.exp(lb)
        return float(w_top / (w_bot + w_top))


def test_host_xi_weight_matches_the_reference_arithmetic():
    L = bnr_amd.lib()
    seen = {"nan": 0, "zero": 0, "one": 0, "subnormal": 0, "interior": 0}
    for lt, lb, delta in itertools.product(ELLS, ELLS, DELTAS):
        got, want = L.bnr_host_xi_weight(lt, lb, delta), reference_weight(lt, lb, delta)
        case = (lt, lb, delta, got, want)
        assert np.isnan(got) == np.isnan(want), case
        if np.isnan(want):
            seen["nan"] += 1
            continue
        assert (got == 0.0) == (want == 0.0) and (got == 1.0) == (want == 1.0), case
        if want == 0.0:
            seen["zero"] += 1
        elif want == 1.0:
            seen["one"] += 1
        else:
            # one exp() in the subnormal range keeps only the bits it has: compare those (a last-bit difference between two libm's exp)
            assert abs(got - want) <= 1e-13 * abs(want) + 2e-323, case
            seen["subnormal" if abs(want) < np.finfo(np.float64).tiny else "interior"] += 1
    assert all(v > 0 for v in seen.values()), seen


def test_host_xi_weight_edge_cases():
    """the outcomes update_xi (gibbs.jl:385-402) branches on, one by one"""
    w = bnr_amd.lib().bnr_host_xi_weight
    assert np.isnan(w(-800.0, -800.0, 0.5))              # both densities underflow: 0/0, the fair coin
    assert w(-800.0, -700.0, 0.5) == 0.0                  # only w_top underflows: xi = 1 without a draw
    assert w(-700.0, -800.0, 0.5) == 1.0                  # only w_bot underflows: xi = 0 without a draw
    assert np.isnan(w(800.0, 800.0, 0.5))                 # both overflow: Inf/Inf
    assert np.isnan(w(800.0, 0.0, 0.5)) and w(0.0, 800.0, 0.5) == 0.0    # w_top overflows: Inf/Inf; only w_bot does: finite/Inf
    assert w(-3.0, -1.0, 1.0) == 0.0 and w(-3.0, -1.0, 0.0) == 1.0    # Delta = 1 / 0 as in Julia
    assert np.isnan(w(-800.0, -800.0, 1.0)) and np.isnan(w(800.0, -1.0, 1.0))   # 0 * 0 / 0, 0 * Inf
    assert np.isnan(w(np.nan, -1.0, 0.5)) and np.isnan(w(-1.0, np.nan, 0.5))
    assert w(-2.0, -2.0, 0.5) == 0.5 and 0.0 < w(-710.0, 0.0, 0.5) < np.finfo(np.float64).tiny


def test_xi_weights_keyword_defaults_to_log():
    for fn in (bnr_amd.Fit, bnr_amd.generate_samples, bnr_amd.generate_samples_dbl, bnr_amd.Chain.__init__, bnr_amd.ChainSet.__init__):
        assert inspect.signature(fn).parameters["xi_weights"].default == "log", fn
    assert bnr_amd._capi.xi_weights_code("log") == 0 and bnr_amd._capi.xi_weights_code("reference") == 1


def test_unknown_xi_weights_is_refused_before_any_gpu_call(tmp_path):
    log = tmp_path / "parameters.log"
    X, y, _ = bnr_amd.make_synthetic(10, 4, 2, seed=1)
    for bad in ("bogus", "Reference", "", None, 1):
        with pytest.raises(ValueError):
            bnr_amd.Fit(X, y, 2, nburn=2, nsamples=2, x_transform=False, suppress_timer=True, seed=3, filename=str(log), xi_weights=bad)
        assert not log.exists()                       # refused before parameters.log is written
    with pytest.raises(ValueError):
        bnr_amd.generate_samples(X, y, 2, nburn=2, nsamp=2, x_transform=False, suppress_timer=True, seed=3, xi_weights="bogus")
    with pytest.raises(ValueError):
        bnr_amd.generate_samples_dbl(X, y, 2, mingen=4, maxgen=8, x_transform=False, suppress_timer=True, seed=3, xi_weights="bogus")
    with pytest.raises(ValueError):
        bnr_amd.Chain(X, y, 2, 3, 3, 1, xi_weights="bogus")


def test_fit_does_not_log_the_option(tmp_path):
    """parameters.log keeps the reference's lines: the option is not among them"""
    import bnr_amd.api as api
    src = inspect.getsource(api.Fit)
    body = src[src.index("with open(filename"):src.index("if mingen > 0 and maxgen > 0")]
    assert "xi_weights" not in body


def test_julia_shim_has_the_switch():
    src = open(os.path.join(ROOT, "julia", "BNRHip.jl"), encoding="utf-8").read()
    chain_kw = _julia_keywords(src, "Chain")
    assert chain_kw.get("xi_weights") == ":log"
    assert re.search(r"^const XI_WEIGHTS = Ref\(:log\)", src, flags=re.M)
    for fname, nxt in (("generate_samples!", "function generate_samples_dbl!("), ("generate_samples_dbl!", "function Fit!(")):
        body = src[src.index("function %s(" % fname):src.index(nxt)]
        creates = re.findall(r"Chain\(X, yv,[^\n]*", body)
        assert creates and all("xi_weights = XI_WEIGHTS[]" in c for c in creates), (fname, creates)
    fit = src[src.index("function Fit!("):]
    assert "XI_WEIGHTS[]" in fit[:fit.index("open(filename")]
    # the three entry points keep exactly the reference's keywords (no xi_weights among them)
    fx = _fixture()
    _check_keywords(src, fx)
    for fname in ("Fit!", "generate_samples!", "generate_samples_dbl!"):
        assert "xi_weights" not in _julia_keywords(src, fname)


def test_header_documents_the_model_option():
    hdr = open(os.path.join(ROOT, "include", "bnr_hip.h"), encoding="utf-8").read()
    assert int(re.search(r"#define BNR_ABI_VERSION (\d+)", hdr).group(1)) >= 7 and bnr_amd.lib().bnr_abi_version() >= 7
    model = hdr[hdr.index("model options (change results)"):hdr.index("tunables (performance only")]
    assert '"xi_weights"' in model
    assert '"xi_weights"' not in hdr[hdr.index("tunables (performance only"):hdr.index("int bnr_chain_set_option(")]

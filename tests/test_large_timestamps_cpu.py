"""What tests/test_large_timestamps_gpu.py relies on, checked without a GPU: at each scale every backbone's case really reaches the argument
range it is there for, and the float32 autograd oracles are usable references for gradients that carry a factor of dt up to 2.7e9."""
import numpy as np
import pytest

from tests import large_timestamp_cases as lt


@pytest.fixture(scope="module", params=lt.SCALES)
def base(request):
    return lt.scaled_case(request.param)


def test_the_scaled_graph_is_the_fixture_graph_with_other_times(base):
    from tests import golden_cases as gc
    d0, d = gc.build_case(lt.GRAPH)["data"], base["data"]
    assert np.array_equal(d.src_node_ids, d0.src_node_ids) and np.array_equal(d.node_interact_times, d0.node_interact_times * float(base["scale"]))
    assert len(base["src"]) == lt.B <= 40 and (base["times"][:2] == d.node_interact_times.min()).all()
    assert 2.6e6 * base["scale"] < d.node_interact_times.max() < 2.7e6 * base["scale"]


@pytest.mark.parametrize("name", list(lt.CASES))
def test_arguments_reach_the_range_the_scale_is_for(name, base):
    """x1000: a valid slot whose row of arguments lies on both sides of 3e7 (a wave that takes the libm call and the fast path at once);
    x10: an argument in (2.7e6, 3e7], the decade no fixture graph reaches"""
    c = lt.CASES[name](base)
    got = lt.require_ranges(base["scale"], c[lt.PARAMS[name]], lt.time_differences(name, c), f"{name} x{base['scale']}")
    print(name, base["scale"], got)
    assert got["rows"] >= 2 * lt.B


@pytest.mark.parametrize("name", list(lt.TRAINED))
def test_float32_oracle_agrees_with_its_float64_evaluation(name, base):
    """Every parameter gradient of the float32 oracle within a quarter of the close_scaled bar (1e-4 * max(1, max |g|)) of the same oracle
    evaluated in float64 behind the float32 argument of the time encoder: the float32 oracle is the GPU tests' reference, also for
    time_encoder.w.weight, whose terms carry dt.  Embeddings: within 1e-5."""
    build, run = lt.TRAINED[name]
    c = build(base)
    e32, g32 = run(c)
    e64, g64 = lt.oracle_float64(run, c)
    assert set(g32) == set(g64) and len(g64) > 4
    assert all(b.dtype == np.float64 for b in e64)                      # the second run really was a float64 run
    for a, b in zip(e32, e64):
        assert np.abs(a.astype(np.float64) - b).max() <= 1e-5, name
    ratio = lt.quarter_bar_agreement(g32, g64)
    worst = max(ratio, key=ratio.get)
    print(name, base["scale"], "worst", worst, ratio[worst], "time encoder", ratio.get(lt.TIME_W), ratio.get(lt.TIME_B))
    assert ratio[worst] <= 0.25, (worst, ratio[worst])
    if name != "graphmixer":                                            # GraphMixer's time encoder is frozen
        assert np.abs(g64[lt.TIME_W]).max() > 1e5 * base["scale"] / 10  # the factor of dt is there


@pytest.mark.parametrize("name", ["tgat", "tgn", "tcl", "cawn"])
def test_no_relu_of_the_oracle_sits_on_its_kink(name, base):
    """see lt.RELU_MARGIN: a pre-activation that float32 cannot tell from zero makes the reference itself machine-dependent"""
    build, run = lt.TRAINED[name]
    smallest, units = lt.relu_margin(run, build(base))
    print(name, base["scale"], smallest, units)
    assert units > 10_000 and smallest >= lt.RELU_MARGIN, (smallest, units)

"""tools/gpu_timing.py without a GPU: the order in which the variants of a comparison are launched, which rounds
count, and the record of a variant's timings."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gpu_timing  # noqa: E402


def test_interleaved_alternates_the_variants_and_drops_the_warmup():
    order = []

    def launch(v):
        order.append(v)
        return len(order)

    out = gpu_timing.interleaved(["a", "b", "c"], launch, warmup=2, reps=3)
    assert order == ["a", "b", "c"] * 5  # every variant once per round, in the order given
    assert out == {"a": [7, 10, 13], "b": [8, 11, 14], "c": [9, 12, 15]}  # rounds 3 to 5
    assert list(out) == ["a", "b", "c"]
    order.clear()
    assert gpu_timing.interleaved([("x", 1)], launch, warmup=0, reps=2) == {("x", 1): [1, 2]}
    assert gpu_timing.interleaved(["a"], launch, warmup=3, reps=0) == {"a": []} and len(order) == 5


def test_interleaved_keeps_whatever_launch_returns():
    out = gpu_timing.interleaved(["a"], lambda v: (1.5, 2.5), warmup=1, reps=2)
    assert out == {"a": [(1.5, 2.5), (1.5, 2.5)]}


def test_summary():
    assert gpu_timing.summary([3, 1, 2], 4) == {"reps": 3, "ms_median": 2, "ms_min": 1, "ms_max": 3, "spread": 1.0}
    assert gpu_timing.summary([4.0, 1.0], 4)["ms_median"] == 2.5  # an even count: the mean of the middle two
    s = gpu_timing.summary([1.23456, 1.23444, 1.5], 3)
    assert (s["ms_median"], s["ms_min"], s["ms_max"]) == (1.235, 1.234, 1.5)
    assert s["spread"] == round((1.5 - 1.23444) / 1.23456, 4)  # of the unrounded timings, to 4 places
    s = gpu_timing.summary([1.23456, 1.23444, 1.5], 5)
    assert (s["ms_median"], s["ms_min"], s["ms_max"]) == (1.23456, 1.23444, 1.5)

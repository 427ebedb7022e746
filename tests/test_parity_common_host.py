"""The shared parity functions (tests/parity_common.py) on inputs small enough to check by eye."""
import json
import math

import numpy as np
import torch

import helpers
import parity_common as P

INF, NAN = math.inf, math.nan
E = 2.0**-24


def test_distance_per_element():
    x = torch.tensor([1.0, 3.0, 0.0, 1.0, INF, NAN, 5.0], dtype=torch.float32)
    x64 = torch.tensor([1.0, 2.0, 0.0, 0.0, INF, NAN, 5.0], dtype=torch.float64)
    den = torch.tensor([4.0, 4.0, 0.0, 0.0, 1.0, 1.0, 0.0], dtype=torch.float64)
    # equal; 1 / 4; 0 over 0; nonzero over 0; x not finite though x64 is the same; NaN; equal over 0
    d = P.distance(x, x64, den)
    assert d.dtype == torch.float64 and d.tolist() == [0.0, 0.25, 0.0, INF, INF, INF, 0.0]
    dn = P.distance(x.numpy(), x64.numpy(), den.numpy())
    assert isinstance(dn, np.ndarray) and dn.dtype == np.float64 and dn.tolist() == d.tolist()
    frozen = den.numpy().copy()
    frozen.setflags(write=False)  # (the families share read-only arrays)
    assert P.distance(frozen, frozen, frozen).tolist() == [0.0] * 7
    assert float(P.distance(torch.tensor(1.5), torch.tensor(1.0, dtype=torch.float64), 2.0)) == 0.25  # scalars


def test_distance_per_row():
    x = torch.tensor([[3.0, 4.0], [0.0, 0.0], [1.0, 0.0], [1.0, NAN], [2.0, 2.0]])
    x64 = torch.zeros(5, 2, dtype=torch.float64)
    x64[4] = 2.0
    den = torch.tensor([[6.0, 8.0], [0.0, 0.0], [0.0, 0.0], [1.0, 1.0], [0.0, 0.0]], dtype=torch.float64)
    # |(3, 4)| / |(6, 8)|; zero over zero; nonzero over zero; not finite; equal over zero
    assert P.distance(x, x64, den, rows=True).tolist() == [0.5, 0.0, INF, INF, 0.0]
    # one axis: a row is its element; more than two: a row is everything behind the first axis
    assert P.distance(torch.tensor([1.0, 2.0]), torch.tensor([1.0, 1.0]), torch.tensor([2.0, 2.0]), rows=True).tolist() == [0.0, 0.5]
    assert P.distance(torch.ones(2, 2, 2), torch.zeros(2, 2, 2), torch.full((2, 2, 2), 2.0), rows=True).tolist() == [0.5, 0.5]


def test_exact_zero_rule_and_live_rows():
    x64 = torch.tensor([[0.0, -0.0], [0.0, 1.0], [0.0, 0.0], [0.0, 0.0]], dtype=torch.float64)
    x = torch.tensor([[-0.0, 0.0], [0.0, 1.0], [0.0, 1e-45], [NAN, 0.0]])
    assert P.zero_rows(x64).tolist() == [True, False, True, True] and P.exact_zero_rule(x, x64).tolist() == [False, False, True, True]
    assert P.zero_rows(torch.tensor([0.0, 2.0, -0.0])).tolist() == [True, False, True]  # one axis
    live = P.live_row_masks(["a", "b", "a", "c"], x64)
    assert list(live) == ["a", "b", "c"] and [m.tolist() for m in live.values()] == [[False] * 4, [False, True, False, False], [False] * 4]
    # rows that are exactly zero take no part: regime a has no live row -- the floor in the yardstick, absent from the ratios
    d = torch.tensor([9.0, 4 * E, 9.0, 9.0], dtype=torch.float64)
    e32 = P.yardstick(live, d, E)
    assert e32 == {"a": E, "b": 4 * E, "c": E}
    assert P.worst_ratios(live, d, e32) == {"b": (1.0, 1)}


def test_the_floor_applies_and_the_three_selection_forms_agree():
    d32 = torch.tensor([1 * E, 3 * E, 64 * E, 2 * E, 32 * E, 5 * E], dtype=torch.float64)
    d = torch.tensor([8 * E, 1 * E, 64 * E, 32 * E, 16 * E, 7 * E], dtype=torch.float64)
    names = ("low", "high", "none")
    by_index = P.masks_of_index(torch.tensor([0, 0, 1, 0, 1, 0]), names)
    by_label = P.masks_of_labels(["low", "low", "high", "low", "high", "low"])
    by_mask = {"low": torch.tensor([True, True, False, True, False, True]), "high": np.array([False, False, True, False, True, False])}
    assert list(by_index) == ["low", "high"]  # a regime without elements is absent
    want_e32 = {"low": 16 * E, "high": 64 * E}  # low: its largest is 5 E, below the floor of 16 E
    want = {"low": (2.0, 3), "high": (1.0, 2)}  # 32 E / 16 E at element 3; 64 E / 64 E at element 2
    for masks in (by_index, by_label, by_mask):
        e32 = P.yardstick(masks, d32, 16 * E)
        assert e32 == want_e32
        assert P.worst_ratios(masks, d, e32) == want
        assert P.worst_ratios(masks, d.numpy(), e32) == want
    # an empty mask passed as such: the floor in the yardstick, absent from the ratios (not a ratio of zero)
    masks = dict(by_mask, none=torch.zeros(6, dtype=torch.bool))
    assert P.yardstick(masks, d32, 16 * E)["none"] == 16 * E
    assert set(P.worst_ratios(masks, d, dict(want_e32, none=16 * E))) == {"low", "high"}
    assert {k: m.tolist() for k, m in P.restrict(by_index, torch.tensor([True, False, False, True, True, False])).items()} == {
        "low": [True, False, False, True, False, False], "high": [False, False, False, False, True, False]}  # fmt: skip


def test_not_finite_counts_as_inf():
    masks = {"a": torch.tensor([True, True, False]), "b": torch.tensor([False, False, True])}
    e32 = {"a": 1.0, "b": 1.0}
    for bad in (NAN, INF):
        got = P.worst_ratios(masks, torch.tensor([0.5, bad, 0.25], dtype=torch.float64), e32)
        assert got == {"a": (INF, 1), "b": (0.25, 2)}


def test_masks_over_leading_and_trailing_axes():
    mask = torch.tensor([[True, False, False], [False, False, True]])  # [2,3]
    hwc = torch.arange(24, dtype=torch.float64).reshape(2, 3, 4)  # the mask covers the leading axes: pixels (0,0) and (1,2)
    chw = hwc.permute(2, 0, 1).contiguous()  # [4,2,3]: the trailing axes
    for d, where in ((hwc, (1, 2, 3)), (chw, (3, 1, 2))):
        assert P.yardstick({"m": mask}, d, 1.0) == {"m": 23.0}
        assert P.yardstick({"m": ~mask}, d, 1.0) == {"m": 19.0}  # pixel (1,1), last channel
        assert P.worst_ratios({"m": mask}, d, {"m": 2.0}) == {"m": (11.5, where)}
        assert P.worst_ratios({"m": mask.numpy()}, d.numpy(), {"m": 2.0}) == {"m": (11.5, where)}
    square = torch.arange(8, dtype=torch.float64).reshape(2, 2, 2)  # both would fit: the leading axes are taken
    assert P.worst_ratios({"m": torch.tensor([[False, True], [False, False]])}, square, {"m": 1.0}) == {"m": (3.0, (0, 1, 1))}


def test_three_quarter_cap():
    # the largest F at which ceil(3 n / 4) of the ratios are still >= 4 F: a quarter of the k-th largest
    assert P.three_quarter_cap(torch.tensor([])) == 0.0
    assert P.three_quarter_cap(torch.tensor([40.0])) == 10.0  # 1 of 1
    assert P.three_quarter_cap(torch.tensor([8.0, 40.0, 4.0])) == 1.0  # 3 of 3: the smallest
    assert P.three_quarter_cap(torch.tensor([8.0, 40.0, 4.0, 12.0])) == 2.0  # 3 of 4: the third largest, 8
    assert P.three_quarter_cap(np.array([8.0, 40.0, 4.0, 12.0, 16.0])) == 2.0  # 4 of 5: the fourth largest, 8
    assert P.three_quarter_cap(torch.tensor([INF, INF, INF, 4.0])) == INF


def test_bound():
    assert P.bound(8.0, 8.0) and not P.bound(8.5, 8.0) and not P.bound(NAN, 8.0) and not P.bound(INF, 8.0)
    assert P.bound(8.5, None) and P.bound(INF, None) and P.bound(NAN, None)  # the recording run


def test_check_records_both_keys_before_it_appends_a_failure(monkeypatch):
    events = []

    class Failures(list):
        def append(self, item):
            events.append(("failure", item))
            super().append(item)

    monkeypatch.setattr(helpers, "_record", lambda kind, value, depth=2: events.append((kind, value, depth)))
    masks = {"a": torch.tensor([True, True, False]), "b": torch.tensor([False, False, True])}
    d, e32 = torch.tensor([1.0, 6.0, 1.0], dtype=torch.float64), {"a": 2.0, "b": 4.0}
    failures = Failures()
    P.check("tag|what|{regime}|tail", masks, d, e32, 2.0, failures)
    assert [e[:2] for e in events[:2]] == [("ratio|tag|what|a|tail", 3.0), ("e32|tag|what|a|tail", 2.0)]
    assert events[2][0] == "failure" and "element 1" in events[2][1] and "3.0 x E32" in events[2][1]
    assert [e[:2] for e in events[3:]] == [("ratio|tag|what|b|tail", 0.25), ("e32|tag|what|b|tail", 4.0)] and len(failures) == 1
    events.clear()
    P.check("t|{regime}", masks, d, e32, None, failures)  # F unset: everything recorded, nothing fails
    assert len(events) == 4 and len(failures) == 1
    P.check_cell("t|value", 9.0, 1.0, 8.0, failures, "the value")
    assert [e[:2] for e in events[4:]] == [("ratio|t|value", 9.0), ("e32|t|value", 1.0), ("failure", failures[-1])]


def test_records_name_the_callers_line(monkeypatch):
    monkeypatch.setattr(helpers, "RECORDS", [])
    failures = []
    P.check("t|{regime}", {"a": torch.tensor([True])}, torch.tensor([1.0], dtype=torch.float64), {"a": 1.0}, 2.0, failures)
    P.check_cell("t|value", 1.0, 1.0, 2.0, failures)
    assert len(helpers.RECORDS) == 4 and all(where.startswith("test_parity_common_host.py:") for _, where, _, _ in helpers.RECORDS)


def test_read_records(tmp_path):
    path = tmp_path / "report.jsonl"
    lines = [dict(test="tests/test_x_gpu.py::test_a", at="f:1", kind="ratio|t|a", value=0.5),
             dict(test="tests/test_x_gpu.py::test_b", at="f:2", kind="ratio|t|a", value=1.5),
             dict(test="tests/test_x_gpu.py::test_a", at="f:1", kind="e32|t|a", value=1e-6),
             dict(test="tests/test_y_gpu.py::test_a", at="f:1", kind="ratio|t|a", value=9.0),
             dict(test="tests/test_x_gpu.py::test_a", at="f:3", kind="rel_err", value=1e-5)]  # fmt: skip
    path.write_text("".join(json.dumps(r) + "\n" for r in lines))
    assert P.read_records(str(path), "test_x_gpu") == ({("t", "a"): 1.5}, {("t", "a"): 1e-6})

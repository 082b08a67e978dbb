"""tests/util.py's gate pinned on hand-written arrays (no GPU, no library): every gradient of the project is judged by these numbers."""
import numpy as np

from tests import util

DENORMAL = 2.0 ** -149  # ulp32(0): the smallest fp32 denormal


def test_ulp32():
    assert util.ulp32(1.0) == 2.0 ** -23
    assert util.ulp32(-1.0) == 2.0 ** -23 and util.ulp32(1.5) == 2.0 ** -23 and util.ulp32(2.0) == 2.0 ** -22
    assert util.ulp32(0.0) == DENORMAL


def test_gate_value_is_the_formula():
    ref32 = np.array([[1.0, -2.0], [0.5, 4.0]], dtype=np.float32)
    ref64 = np.array([[1.0, -2.25], [0.5, 3.0]])  # max |a - b| = 1, max |b| = 3: one ulp of 3 is 2^-22
    assert util.gate_value(ref32, ref64) == 2.0 * 1.0 + 2.0 ** -22
    assert util.gate_value(ref64, ref64) == 2.0 ** -22  # the reference's own error exactly zero: the ulp term alone
    assert util.gate_value(np.float32(0.5), 0.75) == 0.5 + 2.0 ** -24  # scalars
    assert util.gate_value(np.zeros(3, dtype=np.float32), np.zeros(3)) == DENORMAL  # all-zero float64: one denormal
    assert util.gate_value(np.full(3, 0.25, dtype=np.float32), np.zeros(3)) == 0.5 + DENORMAL
    assert util.gate_value(np.zeros((0, 4), dtype=np.float32), np.zeros((0, 4))) == DENORMAL  # empty: both maxima start at 0


def test_gates_with_and_without_names():
    ref32 = {"a": np.array([1.0], dtype=np.float32), "b": np.array([2.0, 0.0], dtype=np.float32), "only32": np.zeros(1)}
    ref64 = {"a": np.array([1.5]), "b": np.array([2.0, 0.0]), "only64": np.zeros(1)}
    want = {"a": 1.0 + 2.0 ** -23, "b": 2.0 ** -22}
    got = util.gates(ref32, ref64)
    assert got == want and list(got) == ["a", "b"]  # the keys of ref64 that ref32 also has, in ref64's order
    assert util.gates(ref32, ref64, names=("b",)) == {"b": want["b"]}
    assert util.gates(ref32, ref64, names=["b", "a"]) == want


def test_shares():
    ref64 = {"w": np.array([[1.0, 2.0], [3.0, 4.0]]), "b": np.array([1.0, 1.0]), "nan": np.ones(3), "inf": np.ones(3), "none": np.ones(2),
             "empty": np.zeros((0, 5)), "scalar": np.float64(2.0)}
    gates = {"w": 0.5, "b": 0.25, "nan": 1.0, "inf": 1.0, "none": 1.0, "empty": DENORMAL, "scalar": 2.0}
    got = {"w": np.array([1.0, 2.0, 3.25, 4.0], dtype=np.float32),  # another shape, the same size: taken in ref64's shape
           "b": np.array([1.0, 0.75]), "nan": np.array([1.0, np.nan, 1.0]), "inf": np.array([np.inf, 1.0, 1.0]), "none": None,
           "empty": np.zeros((0, 5), dtype=np.float32), "scalar": np.array([3.0], dtype=np.float32)}
    sh = util.shares(got, ref64, gates)
    assert sh == {"w": 0.5, "b": 1.0, "nan": float("inf"), "inf": float("inf"), "empty": 0.0, "scalar": 0.5}  # None: skipped
    assert all(type(v) is float for v in sh.values())
    assert util.shares(got, ref64, gates, names=("b", "none", "w")) == {"b": 1.0, "w": 0.5}
    assert util.shares({"b": np.array([1.0, 0.75])}, ref64, gates, names=("b", "w")) == {"b": 1.0}  # a missing key is a None entry


def test_share_of_names_the_worst_element():
    assert util.share_of(np.array([[1.0, 2.0], [3.5, 4.0]]), np.array([[1.0, 2.0], [3.0, 4.0]]), 0.25) == (2.0, 2)
    assert util.share_of(np.array([1.0, np.inf, np.nan]), np.ones(3), 1.0) == (float("inf"), 1)  # the first non-finite element
    assert util.share_of(np.zeros(0), np.zeros(0), 1.0) == (0.0, -1)

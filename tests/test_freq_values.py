"""CPU: dsf::call_value (csrc/ds_freq.h), the routine freq_values_kernel runs, held to Python through ds_freq_values_reference: for the
act row of a call it must give the doubles float(str(np.float32(q))) gives for the two normalised probabilities -- the shortest
digits that round-trip float32, then the correctly rounded double of THAT decimal -- bit for bit, and take every finite q in
[1e-14, 1] itself."""
import numpy as np
import pytest

from deepsignal_amd import engine as eng

from callfreq_cases import (HOST, OK, act_for, assert_values, bits, digits_of, edge_q, normalised, outside_act, python_value,
                            random_q)


def test_the_double_of_the_shortest_decimal_is_not_the_widened_float():
    p0, p1, status = eng.freq_values_reference(act_for([np.float32(0.1)]))
    assert status.tolist() == [OK]
    assert bits(float(p0[0])) == bits(0.1) and float(p0[0]) != float(np.float32(0.1))
    assert bits(float(p1[0])) == bits(python_value(np.float32(1) - np.float32(0.1)))


@pytest.mark.parametrize("seed", [11, 12])
def test_random_bit_patterns(seed):
    act = act_for(random_q(100_000, seed))                        # 200 k patterns over the two seeds, and their 1 - q
    p0, p1, status = eng.freq_values_reference(act)
    assert (status == OK).all()
    assert_values(act, p0, p1, status, must_be_ok=True)


def test_edges_of_the_range_and_of_the_printed_forms():
    q = edge_q()
    assert q.size > 150 and q.min() < 2e-14 and q.max() == 1
    for x in (0.5, 1e-4, 1.0, 1e-14, 2.0 ** -46):
        assert np.float32(x) in q
    act = act_for(q)
    p0, p1, status = eng.freq_values_reference(act)
    assert (status == OK).all(), q[status != OK]
    assert_values(act, p0, p1, status, must_be_ok=True)
    # the value half way between two eight-digit decimals goes to the even one, as the printed form does
    tie = float(p0[list(q).index(np.float32(87.0 / 512.0))])
    assert str(np.float32(87.0 / 512.0)) == "0.16992188" and bits(tie) == bits(0.16992188)


def test_every_digit_count():
    q = np.concatenate([edge_q(), random_q(4000, 13)])
    counts = {d: 0 for d in range(1, 10)}
    for x in q:
        counts[digits_of(x)] += 1
    assert all(counts[d] > 0 for d in range(1, 10)), counts
    act = act_for(q)
    assert_values(act, *eng.freq_values_reference(act), must_be_ok=True)


def test_general_act_rows():
    """Pairs as the forward gives them (two sigmoid outputs): the sum is not 1 and both quotients round."""
    rng = np.random.default_rng(14)
    act = (1 / (1 + np.exp(-rng.normal(0, 4, (50_000, 2))))).astype(np.float32)
    q0, q1 = normalised(act)
    assert (q0 + q1 != 1).any()
    assert_values(act, *eng.freq_values_reference(act), must_be_ok=True)
    wide = np.concatenate([act, rng.random((50_000, 3)).astype(np.float32)], axis=1)      # class_num 5: columns 0 and 1 are read
    a, b = eng.freq_values_reference(wide)[:2], eng.freq_values_reference(act)[:2]
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_values_outside_the_range_are_never_wrong():
    act = outside_act()
    p0, p1, status = eng.freq_values_reference(act)
    assert_values(act, p0, p1, status)
    q0, _ = normalised(act)
    assert (status[~np.isfinite(q0)] == HOST).all()                 # NaN (0 / 0) and inf (1 / 0) are Python's
    assert (status[np.abs(q0) > 1] == HOST).all()
    zero = (q0 == 0)
    assert zero.sum() == 2 and (status[zero] == OK).all()           # +-0 print as 0.0 / -0.0
    assert sorted(bits(float(v)) for v in p0[zero]) == sorted([bits(0.0), bits(-0.0)])


def test_argument_checks():
    with pytest.raises(ValueError):
        eng.freq_values_reference(np.zeros((4, 1), np.float32))
    with pytest.raises(ValueError):
        eng.freq_values_reference(np.zeros(4, np.float32))
    p0, p1, status = eng.freq_values_reference(np.zeros((0, 2), np.float32))
    assert p0.size == p1.size == status.size == 0

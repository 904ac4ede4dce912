"""CPU: ds_train_mask_reference, the dropout mask function of the training step (csrc/ds_train.h) on the host. The GPU tests
check the kernels' masks against it bit for bit; here the function itself is held to what a dropout mask must be."""
import numpy as np
import pytest

import __graft_entry__ as g


@pytest.fixture(scope="module")
def ref():
    g.build()
    from deepsignal_amd import engine
    return engine.train_mask_reference


def test_deterministic_and_keyed(ref):
    a = ref(3, 0, "fw_l0", 8, 17, 0.5)
    assert a.shape == (8, 17, 256) and a.dtype == np.uint8 and set(np.unique(a)) == {0, 1}
    assert (ref(3, 0, "fw_l0", 8, 17, 0.5) == a).all()
    for other in (ref(4, 0, "fw_l0", 8, 17, 0.5), ref(3, 1, "fw_l0", 8, 17, 0.5), ref(3, 0, "bw_l0", 8, 17, 0.5),
                  ref(3, 0, "fw_l1", 8, 17, 0.5)):
        # independent fair bits agree on half the positions: 6 sigma of 34,816 draws is 0.016
        assert abs((other == a).mean() - 0.5) < 0.02
    assert ref(3, 0, "fc1", 8, 17, 0.5).shape == (8, 512) and ref(3, 0, "fc2", 8, 17, 0.5).shape == (8, 2)
    # rows and steps of one stream differ from each other too
    assert abs((a[0] == a[1]).mean() - 0.5) < 0.1 and abs((a[:, 0] == a[:, 1]).mean() - 0.5) < 0.1


def test_keep_prob_one_keeps_everything(ref):
    for s in ("fw_l2", "bw_l1", "fc1", "fc2"):
        assert ref(9, 5, s, 6, 5, 1.0).all()


def test_a_rows_mask_does_not_depend_on_n(ref):
    for s in ("fw_l0", "bw_l2", "fc1", "fc2"):
        big = ref(21, 2, s, 33, 5, 0.5)
        for n in (1, 5, 32):
            assert (ref(21, 2, s, n, 5, 0.5) == big[:n]).all()


def test_wide_reference_is_the_same_function(ref):
    """ds_train_mask_reference and ds_train_mask_reference_wide are one function: the joint-layer streams agree byte for byte at
    the BiLSTM widths, and a unit's mask does not depend on the width of its row."""
    from deepsignal_amd.engine import train_mask_reference_wide as wide
    seed, step, n, T, kp = 21, 2, 5, 5, 0.5
    assert ref(seed, step, "fc1", n, T, kp).tobytes() == wide(seed, step, "fc1", n, 512, kp).tobytes()
    assert ref(seed, step, "fc2", n, T, kp).tobytes() == wide(seed, step, "fc2", n, 2, kp).tobytes()
    assert np.ascontiguousarray(wide(seed, step, "fc1", n, 720, kp)[:, :240]).tobytes() == wide(seed, step, "fc1", n, 240, kp).tobytes()


@pytest.mark.parametrize("keep_prob", [0.5, 0.8, 0.1])
def test_kept_share_is_keep_prob(ref, keep_prob):
    m = ref(1234, 7, "bw_l1", 64, 17, keep_prob)
    N = m.size
    sigma = np.sqrt(keep_prob * (1 - keep_prob) / N)
    assert abs(m.mean() - keep_prob) <= 6 * sigma
    # per unit column and per time step as well (each over N / 256 resp. N / 17 draws)
    for axis, cnt in (((0, 1), N // 256), ((0, 2), N // 17)):
        assert np.abs(m.mean(axis=axis) - keep_prob).max() <= 6 * np.sqrt(keep_prob * (1 - keep_prob) / cnt)


def test_bad_arguments_are_refused(ref):
    for args in ((1, 0, "nope", 4, 5, 0.5), (1, 0, "fc1", 4, 5, 0.0), (1, 0, "fc1", 4, 5, 1.5)):
        with pytest.raises(ValueError):
            ref(*args)

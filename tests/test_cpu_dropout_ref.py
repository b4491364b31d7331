"""The CPU replica of the kernels' hash dropout (tests/dropout_ref.py) against a scalar restatement in plain Python ints, and its
shape / value properties.  The replica against the kernels themselves: tests/test_gpu_dropout.py."""
import numpy as np
import pytest

import dropout_ref as DR

GOLDEN = 0x9E3779B9


def _triples():
    """(rng0, counter, stream, idx): a few hundred, with the wrap-around cases the kernels meet"""
    rs = np.random.RandomState(7)
    out = []
    # idx near multiples of 2^32 / GOLDEN: idx * GOLDEN wraps right there
    for j in (1, 2, 3, 1000, 61803):
        base = (j << 32) // GOLDEN
        for d in (-1, 0, 1):
            out.append((0x5EED, 0, 1, base + d))
    # counters whose product with the golden-ratio constant wraps (every counter >= 2 does) and the edges of the counter itself
    for c in (0, 1, 2, 3, 77, 1 << 16, (1 << 31) - 1, 1 << 31, (1 << 32) - 1, ((1 << 32) // GOLDEN) + 1):
        for s in (1, 2, 6):
            out.append((0x5EED, c, s, 12345))
    # rng0 as the engine's int32 tensor holds it: negative values = top bit set
    for r0 in (-1, -0x5EED, -(1 << 31), np.int32(-123456789).item(), 0x7FFFFFFF):
        for c in (0, 5):
            out.append((r0, c, 3, 99))
    # the largest element indices of the suite's layers and of a 2048 x 5005 batch
    for idx in (0, 1, 31, 32 * 1024 - 1, 33 * 5005 - 1, 2048 * 5005 - 1, (1 << 32) - 1):
        out.append((0x5EED, 1, 1, idx))
    for _ in range(300):
        out.append((int(rs.randint(-(1 << 31), 1 << 31)), int(rs.randint(0, 1 << 32)), int(rs.randint(1, 8)), int(rs.randint(0, 1 << 32))))
    return out


def test_vectorised_hash_equals_int_restatement():
    xs = [0, 1, 0xFFFFFFFF, 0x80000000, 0x7FEB352D, 0x846CA68B, GOLDEN] + [int(v) for v in np.random.RandomState(1).randint(0, 1 << 32, 300)]
    got = DR.hash_u32(np.array(xs, dtype=np.uint32))
    assert got.dtype == np.uint32
    assert [int(g) for g in got] == [DR.hash_u32_int(x) for x in xs]


@pytest.mark.parametrize("p", [0.3, 0.2])
def test_replica_equals_scalar_restatement(p):
    T = _triples()
    assert len(T) >= 300
    for r0, c, s, idx in T:
        u = DR.uniform(DR.seed_of(r0, c), s, idx)
        want = DR.scale_int(r0, c, s, idx, p)
        got = np.float32(0.0) if u < np.float32(p) else np.float32(1.0) / (np.float32(1.0) - np.float32(p))
        assert got == want and got.dtype == np.float32, (r0, c, s, idx)
    # the [M, K] form indexes m * K + k
    for r0, c, s in ((0x5EED, 0, 1), (-5, 77, 6), (0x5EED, (1 << 32) - 1, 3)):
        m = DR.mask(r0, c, s, 7, 130, p)
        for (i, k) in ((0, 0), (0, 129), (3, 64), (6, 129), (5, 1)):
            assert m[i, k] == DR.scale_int(r0, c, s, i * 130 + k, p), (r0, c, s, i, k)


def test_negative_int32_seed_word_is_its_twos_complement():
    a = DR.mask(-0x5EED, 3, 2, 4, 64, 0.3)
    b = DR.mask((1 << 32) - 0x5EED, 3, 2, 4, 64, 0.3)
    assert np.array_equal(a, b)


def test_shape_and_values():
    for p in (0.3, 0.2):
        m = DR.mask(0x5EED, 0, 1, 32, 1024, p)
        assert m.shape == (32, 1024) and m.dtype == np.float32
        keep = np.float32(1.0) / (np.float32(1.0) - np.float32(p))
        assert set(np.unique(m).tolist()) == {0.0, float(keep)}
        rate = float((m != 0).mean())
        # binomial: sd of the rate over 32768 draws is sqrt(p (1 - p) / 32768) < 0.0026; five of them
        assert abs(rate - (1 - p)) < 0.013, rate
    assert np.array_equal(DR.mask(0x5EED, 4, 2, 5, 33, 0.0), np.ones((5, 33), dtype=np.float32))


def test_masks_of_other_counter_or_stream_differ():
    a = DR.mask(0x5EED, 5, 2, 32, 1024, 0.3)
    for other in (DR.mask(0x5EED, 6, 2, 32, 1024, 0.3), DR.mask(0x5EED, 5, 3, 32, 1024, 0.3)):
        agree = float(((a != 0) == (other != 0)).mean())
        # independent masks agree on 0.7^2 + 0.3^2 = 0.58 of the positions (sd 0.0027 over 32768)
        assert abs(agree - 0.58) < 0.014, agree


def test_wrapper_maps_dropouts_by_name():
    """ReplicaDropout on a stand-in pair (no package import): streams from the program's `lins`, names matched, eval = identity"""
    import torch
    import torch.nn as nn

    class L:
        def __init__(self, lin, drop):
            self.lin, self.pro_drop = lin, drop

    def net():
        return nn.Sequential(nn.Linear(6, 8), nn.ReLU(), nn.Dropout(0.3), nn.Linear(8, 4), nn.ReLU(), nn.Dropout(0.2), nn.Linear(4, 1))
    torch.manual_seed(0)
    hip, ora = net(), net()
    ora.load_state_dict(hip.state_dict())
    lins = [L(hip[0], None), L(hip[3], hip[2]), L(hip[6], hip[5])]
    w = DR.ReplicaDropout(ora, hip, lins)
    assert w.streams == {"2": (2, 8, 0.3), "5": (3, 4, 0.2)}
    x = torch.randn(5, 6)
    w.train().set(0x5EED, 1, 5)
    m2, m3 = torch.from_numpy(DR.mask(0x5EED, 1, 2, 5, 8, 0.3)), torch.from_numpy(DR.mask(0x5EED, 1, 3, 5, 4, 0.2))
    want = hip[6](torch.relu(hip[3](torch.relu(hip[0](x)) * m2)) * m3)
    assert torch.equal(w(x), want)
    w.eval()
    assert torch.equal(w(x), hip.eval()(x))
    # a Dropout the program forgot is an error, not a silent identity
    with pytest.raises(AssertionError):
        DR.ReplicaDropout(net(), hip, lins[:2])

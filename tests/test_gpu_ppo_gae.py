"""spl_ppo_gae (include/splendor_ppo.h) against the numpy oracle of tests/test_ppo_host.py: advantages
and returns bit for bit, the advantage statistics within the worst-case error of a float64 sum, and
the same bytes from run to run."""
import math

import numpy as np
import pytest

from test_ppo_host import gae_oracle

pytestmark = pytest.mark.gpu

# one lane; a partial wave; several workgroups plus a tail... the full depth; a step count no unroll divides
SHAPES = [(1, 1), (2, 65), (5, 200), (128, 64), (7, 4096)]
GAMMA_LAMBDA = [(0.999, 0.95), (1.0, 1.0), (0.5, 0.0)]
DONE = ["none", "all", "first", "last", "random"]


def planes(K, T, seed):
    """Seeded rewards, values and bootstrap values: both signs, magnitudes near 1e3, 1 and 1e-6, and the
    engine's own rewards (-0.01, -0.1, 0, +-1)."""
    rng = np.random.default_rng(seed)

    def mixed(shape):
        scale = rng.choice(np.array([1e3, 1.0, 1e-6], dtype=np.float32), size=shape)
        return (rng.normal(size=shape).astype(np.float32) * scale).astype(np.float32)

    engine = np.array([-0.01, -0.1, 0.0, 1.0, -1.0], dtype=np.float32)
    reward = np.where(rng.random((K, T)) < 0.5, rng.choice(engine, size=(K, T)), mixed((K, T))).astype(np.float32)
    reward.flat[0] = np.float32(-0.01)
    return reward, mixed((K, T)), mixed((T,)), rng


def done_plane(kind, K, T, rng):
    d = np.zeros((K, T), dtype=np.uint8)
    if kind == "all":
        d[:] = 1
    elif kind == "first":
        d[0] = 1
    elif kind == "last":
        d[K - 1] = 1
    elif kind == "random":
        d = (rng.random((K, T)) < 0.05).astype(np.uint8)
    return d


def check_stats(st, adv):
    x = adv.astype(np.float64).ravel()
    n = x.size
    assert st["count"] == n
    eps = 2.0 ** -53
    assert abs(st["sum"] - math.fsum(x)) <= n * eps * math.fsum(np.abs(x)), (st["sum"], math.fsum(x))
    sq = x * x  # exact: a float32 squared has 48 significant bits
    assert abs(st["sumsq"] - math.fsum(sq)) <= n * eps * math.fsum(sq), (st["sumsq"], math.fsum(sq))
    with np.errstate(all="ignore"):  # the header's formula, one float64 operation at a time
        s, ss, nn = np.float64(st["sum"]), np.float64(st["sumsq"]), np.float64(n)
        mean = s / nn
        var = (ss - s * mean) / (nn - np.float64(1.0))
        if var < 0:
            var = np.float64(0.0)
        std = np.sqrt(var)
    got = np.array([st["mean"], st["std"]], dtype=np.float64)
    assert np.array_equal(got, np.array([mean, std]), equal_nan=True), (got, mean, std)
    got32 = np.array([st["mean32"], st["std32"]], dtype=np.float32)
    assert np.array_equal(got32, np.array([mean, std]).astype(np.float32), equal_nan=True)
    if n > 1 and np.isfinite(x).all() and np.isfinite(std):  # and it is the n-1 deviation, to rounding
        assert math.isclose(float(std), float(np.std(x, ddof=1)), rel_tol=1e-6, abs_tol=1e-30)


@pytest.mark.parametrize("gamma,lam", GAMMA_LAMBDA)
@pytest.mark.parametrize("K,T", SHAPES)
def test_gae_bit_equal_and_statistics(K, T, gamma, lam):
    import torch
    from splendor_gym.ppo import PPORolloutStore
    reward, value, last_value, rng = planes(K, T, seed=1000 * K + T)
    store = PPORolloutStore(K, T, "cuda:0")
    store.reward.copy_(torch.from_numpy(reward))
    store.value.copy_(torch.from_numpy(value))
    lv = torch.from_numpy(last_value).to(store.device)
    for kind in DONE:
        done = done_plane(kind, K, T, rng)
        store.done.copy_(torch.from_numpy(done))
        store.adv.fill_(float("nan"))
        store.ret.fill_(float("nan"))
        store.compute_gae(lv, gamma=gamma, gae_lambda=lam)
        adv, ret = store.adv.cpu().numpy(), store.ret.cpu().numpy()
        raw = store._stats.cpu().numpy().tobytes()
        want_adv, want_ret = gae_oracle(reward, value, done, last_value, gamma, lam)
        assert np.array_equal(adv.view(np.uint32), want_adv.view(np.uint32)), (kind, np.argwhere(adv != want_adv)[:4])
        assert np.array_equal(ret.view(np.uint32), want_ret.view(np.uint32)), (kind, np.argwhere(ret != want_ret)[:4])
        check_stats(store.stats(), adv)
        # a second launch on the same data: the same bytes in every output
        store.compute_gae(lv.view(T, 1), gamma=gamma, gae_lambda=lam)
        assert store.adv.cpu().numpy().tobytes() == adv.tobytes() and store.ret.cpu().numpy().tobytes() == ret.tobytes()
        assert store._stats.cpu().numpy().tobytes() == raw


def test_gae_leaves_its_inputs_alone():
    import torch
    from splendor_gym.ppo import PPORolloutStore
    K, T = 5, 200
    reward, value, last_value, rng = planes(K, T, seed=3)
    store = PPORolloutStore(K, T, "cuda:0")
    store.reward.copy_(torch.from_numpy(reward))
    store.value.copy_(torch.from_numpy(value))
    store.done.copy_(torch.from_numpy(done_plane("random", K, T, rng)))
    lv = torch.from_numpy(last_value).to(store.device)
    store.compute_gae(lv)
    assert np.array_equal(store.reward.cpu().numpy(), reward) and np.array_equal(store.value.cpu().numpy(), value)
    assert np.array_equal(lv.cpu().numpy(), last_value)
    with pytest.raises(ValueError):
        store.compute_gae(lv[:-1])

"""The bf16 PPO network passes without a GPU (spl_ppo_net_forward_bf16 / spl_ppo_net_backward_bf16,
include/splendor_ppo.h): bf16_nets.to_bf16 against hand-picked bit patterns, the emulator against the float64
oracle where nothing is rounded, the header against the bindings, the host-side refusals, which are those of
the tiled pair, and DeviceNets' `operands` switch."""
import re

import numpy as np
import pytest

import bf16_nets
from test_ppo_adam_host import _lib
from test_ppo_net_host import make_rows, net_oracle
from test_ppo_net_tiled_host import cases, header


def f32(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def test_to_bf16_bit_patterns():
    cases_ = [
        (0x3F800000, 0x3F800000),  # 1.0: already a bf16
        (0x3F808000, 0x3F800000),  # a tie, the kept bit even: down
        (0x3F818000, 0x3F820000),  # a tie, the kept bit odd: up
        (0x3F808001, 0x3F810000),  # just above a tie: up
        (0x3F807FFF, 0x3F800000),  # just below a tie: down
        (0x3FFF8000, 0x40000000),  # a tie whose carry runs into the exponent: 1.99609375 -> 2.0
        (0x3FFFFFFF, 0x40000000),  # the largest float32 below 2
        (0x00000000, 0x00000000),  # +0
        (0x80000000, 0x80000000),  # -0 keeps its sign
        (0x7F7F0000, 0x7F7F0000),  # the largest finite bf16
        (0x7F7F7FFF, 0x7F7F0000),  # the largest float32 that still rounds to it
        (0xBF808000, 0xBF800000), (0xBF818000, 0xBF820000),  # ties are by magnitude
        (0x43808000, 0x43800000),  # 257 -> 256
        (0x43BF8000, 0x43C00000),  # 383 -> 384
    ]
    got = bf16_nets.to_bf16(f32([a for a, _ in cases_])).view(np.uint32)
    assert got.tolist() == [b for _, b in cases_]
    assert bf16_nets.to_bf16(np.float32(257.0)) == 256.0 and bf16_nets.to_bf16(np.float32(383.0)) == 384.0
    # every byte, and 256 * every byte, is a bf16; shape and dtype are kept
    ints = np.arange(256, dtype=np.float32).reshape(16, 16)
    r = bf16_nets.to_bf16(ints)
    assert r.dtype == np.float32 and r.shape == (16, 16) and np.array_equal(r, ints)
    assert np.array_equal(bf16_nets.to_bf16(256 * ints), 256 * ints)
    # against the definition on random values: the nearest of the two neighbouring bf16, ties to even
    x = np.random.default_rng(0).normal(size=4096).astype(np.float32) * np.float32(37.0)
    lo = (x.view(np.uint32) & 0xFFFF0000).view(np.float32).astype(np.float64)
    hi = ((x.view(np.uint32) & 0xFFFF0000) + 0x10000).view(np.float32).astype(np.float64)
    got = bf16_nets.to_bf16(x).astype(np.float64)
    nearest = np.where(np.abs(x - lo) <= np.abs(hi - x), lo, hi)
    ties = np.abs(x - lo) == np.abs(hi - x)
    assert np.array_equal(got[~ties], nearest[~ties]) and (np.abs(got - x) <= np.abs(x) * 2.0 ** -8).all()


def test_split_of_column_295():
    rng = np.random.default_rng(1)
    rows = make_rows(rng, 9, big_moves=(0, 4, 8))
    x = bf16_nets.split_inputs(rows)
    assert x.shape == (9, 298) and np.array_equal(bf16_nets.to_bf16(x.astype(np.float32)), x)  # nothing to round
    w = rng.normal(size=(256, 297))
    full = rows[:, :297].astype(np.float64)
    full[:, 295] += 256.0 * rows[:, 297]
    assert np.allclose(x @ bf16_nets.split_weights(w).T, full @ w.T, rtol=1e-13, atol=1e-9)
    d = rng.normal(size=(9, 256))
    assert np.allclose(bf16_nets.fold_columns(d.T @ x), d.T @ full, rtol=1e-13, atol=1e-9)


def test_emulator_is_the_oracle_where_nothing_rounds():
    """With weights, activations' inputs and gradients that are bf16 already the emulator differs from the float64
    oracle only by the float32 rounding of the four saved planes."""
    rng = np.random.default_rng(2)
    B = 7
    rows = make_rows(rng, B, big_moves=(1,))
    bf = lambda a: bf16_nets.to_bf16((a).astype(np.float32)).astype(np.float64)
    params = {net: [bf(rng.normal(size=s) * 0.05) for s in ((256, 297), (256,), (256, 256), (256,), (n3, 256), (n3,))]
              for net, n3 in (("actor", 45), ("critic", 1))}
    dlogits, dvalue = bf(rng.normal(size=(B, 45))), bf(rng.normal(size=B))
    bad = np.zeros(B, dtype=bool)
    bad[3] = True
    got, want = bf16_nets.emulate(params, rows, dlogits, dvalue, bad=bad), net_oracle(params, rows, dlogits, dvalue, bad=bad)
    assert not got["logits"][3].any() and got["value"][3] == 0
    # the planes are rounded to bf16 as operands: 2^-8 relative, through at most three layers
    for name in ("logits", "value"):
        assert bf16_nets.rel_l2(got[name], want[name]) < 0.05, name
    for net in bf16_nets.NETS:
        for g, w in zip(got["grads"][net], want["grads"][net]):
            assert g.shape == w.shape and bf16_nets.rel_l2(g, w) < 0.05
        # db3 and the critic's dW3-free parts take unrounded operands: equal
        assert np.allclose(got["grads"][net][5], want["grads"][net][5], rtol=1e-12, atol=0)


def test_product_bound():
    rng = np.random.default_rng(3)
    a, b = rng.normal(size=(5, 64)).astype(np.float32), rng.normal(size=(64, 3)).astype(np.float32)
    start = rng.normal(size=3).astype(np.float32)
    y, bound = bf16_nets.product(a, b, start=start, n_extra=2)
    assert np.allclose(y, a.astype(np.float64) @ b.astype(np.float64) + start)
    n = 64 + 2 + 1
    mag = np.abs(a).astype(np.float64) @ np.abs(b).astype(np.float64) + np.abs(start)
    assert np.allclose(bound, n * 2.0 ** -23 / (1 - n * 2.0 ** -23) * mag, rtol=1e-12)
    # a float32 chain of fused multiply-adds stays inside it
    chain = np.tile(start, (5, 1))
    for k in range(64):
        chain = (chain.astype(np.float64) + a[:, k:k + 1].astype(np.float64) * b[k].astype(np.float64)).astype(np.float32)
    assert (np.abs(chain - y) <= bound).all()


def test_header_advertises_the_bf16_calls():
    native, lib = _lib()
    src = header()
    assert re.search(r"#define SPL_PPO_NET_BF16 1\b", src) and native.PPO_NET_BF16 == 1
    assert re.search(r"#define SPL_PPO_ABI 1\b", src) and lib.spl_abi_version() == 9  # additive: neither moved
    for name, block in (("spl_ppo_net_forward_bf16", "spl_ppo_net_fwd_t"), ("spl_ppo_net_backward_bf16", "spl_ppo_net_bwd_t")):
        assert re.search(rf"int {name}\(int32_t B, const {block} \*args, void \*stream\);", src), name
    # nothing already in the header moved: the new block comes behind the last earlier declaration
    assert src.index("#define SPL_PPO_NET_BF16") > src.index("int spl_ppo_net_backward_tiled(")


def test_library_exports_both_symbols():
    native, lib = _lib()
    assert native.has_net_bf16(lib) and native.has_net_tiled(lib)
    for name in native.OPTIONAL_BF16:
        assert hasattr(lib, name) and name in native.SIGNATURES
    assert native.SIGNATURES["spl_ppo_net_forward_bf16"] == native.SIGNATURES["spl_ppo_net_forward_tiled"]
    assert native.SIGNATURES["spl_ppo_net_backward_bf16"] == native.SIGNATURES["spl_ppo_net_backward_tiled"]
    assert getattr(lib, "spl_ppo_net_forward_bf16").argtypes == native.SIGNATURES["spl_ppo_net_forward_bf16"][0]


@pytest.mark.parametrize("which", ["forward", "backward"])
def test_the_same_refusals_as_the_tiled_calls(which):
    """The one shared check: every argument error is returned on the host before any launch, with the tiled call's
    code and message."""
    native, lib = _lib()
    old, new = ((lib.spl_ppo_net_forward_tiled, lib.spl_ppo_net_forward_bf16) if which == "forward" else
                (lib.spl_ppo_net_backward_tiled, lib.spl_ppo_net_backward_bf16))
    n = 0
    for label, B, args in cases(native, which):
        want = old(B, args, None)
        want_text = lib.spl_last_error()
        got = new(B, args, None)
        assert want < 0 and got == want and lib.spl_last_error() == want_text and want_text, label
        n += 1
    assert n >= 6 + 12 + 24


def test_device_nets_takes_two_values_of_operands():
    import inspect
    from splendor_gym.policy import ActorCritic
    from splendor_gym.ppo import DeviceNets
    sig = inspect.signature(DeviceNets.__init__).parameters
    assert sig["operands"].default == "f32" and sig["tiled"].default is False
    assert list(sig)[:4] == ["self", "agent", "tiled", "operands"]
    for bad in (None, 16, "fp32", "BF16", "bfloat16", "", True):
        with pytest.raises(ValueError, match="'f32' or 'bf16'"):
            DeviceNets(ActorCritic(), operands=bad)
    for good in ("f32", "bf16"):  # accepted; what then fails is the missing GPU or the CPU parameters
        with pytest.raises((RuntimeError, ValueError)) as e:
            DeviceNets(ActorCritic(), operands=good)
        assert "operands must be" not in str(e.value)


def test_cli_has_the_switch():
    from splendor_gym.scripts import ppo_device
    with pytest.raises(SystemExit):
        ppo_device.main(["--net-operands", "fp16"])

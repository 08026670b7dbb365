"""The device permutation without a GPU (spl_ppo_permute / spl_ppo_loss_dev, include/splendor_ppo.h,
splendor_gym.ppo.permutation_reference): the numpy reference is a permutation, keyed by both of (seed, draw) and
uniform as far as a chi-square sees; a known answer pins the definition; the header against the bindings; the
host-side refusals; and what ppo_update(graph=True) refuses before it touches a device."""
import ctypes
import re
import types

import numpy as np
import pytest

from test_ppo_adam_host import _lib, _refused, header_fields
from test_ppo_net_tiled_host import header


def reference():
    from splendor_gym import ppo
    return ppo.permutation_reference, ppo.permutation_positions


@pytest.mark.parametrize("n", list(range(1, 301)) + [1023, 1024, 1025, 2048, 100003])
def test_reference_is_a_permutation(n):
    perm, _ = reference()
    p = perm(n, 7, 3)
    assert p.dtype == np.int64 and p.shape == (n,) and np.array_equal(np.sort(p), np.arange(n))


def test_one_position_is_the_identity():
    perm, _ = reference()
    assert perm(1, 5, 9).tolist() == [0]


def test_seed_and_draw_both_key_it():
    perm, _ = reference()
    n = 2048
    pairs = [(0, 0), (0, 1), (1, 0), (1, 1), (2 ** 32, 0), (0, 2 ** 32), (2 ** 32 + 1, 1), (1, 2 ** 32 + 1), (2 ** 63, 2 ** 63)]
    perms = [perm(n, s, d) for s, d in pairs]
    for i in range(len(pairs)):
        assert np.array_equal(perms[i], perm(n, *pairs[i]))  # a function of its arguments
        for j in range(i):
            assert (perms[i] != perms[j]).mean() > 0.9, (pairs[i], pairs[j])  # and another one for another pair


def test_positions_are_the_references_elements():
    perm, positions = reference()
    n = 1025
    for draw in (0, 5, 2 ** 32 + 5):
        full = perm(n, 1234, draw)
        assert np.array_equal(positions(np.array([0, 1, 77, n - 1]), n, 1234, draw), full[[0, 1, 77, n - 1]])
    both = positions(np.array([[0], [n - 1]]), n, 1234, np.arange(3))
    assert both.shape == (2, 3) and both[:, 2].tolist() == perm(n, 1234, 2)[[0, n - 1]].tolist()


@pytest.mark.parametrize("n", [64, 1024])
def test_destinations_are_uniform(n):
    """Seed 1234, draws 0..4095: where position 0 and position n - 1 go, in 64 bins.  chi-square with 63 degrees
    of freedom below 110 (about the 1e-4 tail).  Measured: 70.8 and 59.0 (n = 64), 63.6 and 52.1 (n = 1024)."""
    _, positions = reference()
    dest = positions(np.array([[0], [n - 1]]), n, 1234, np.arange(4096))
    for which, row in zip(("0", "n - 1"), dest):
        hist = np.bincount(row * 64 // n, minlength=64)
        expect = 4096 / 64
        chi2 = float(((hist - expect) ** 2 / expect).sum())
        print(f"n {n} position {which}: chi-square {chi2:.2f}")
        assert hist.sum() == 4096 and chi2 < 110, (n, which, chi2)


def test_neighbours_are_ordered_either_way():
    """n = 64, seed 99, 4096 draws: perm[0] < perm[1] in half of them, +- 0.04 (five standard deviations of a fair
    coin over 4096 draws are 0.039).  Measured: 0.4963."""
    _, positions = reference()
    d = positions(np.array([[0], [1]]), 64, 99, np.arange(4096))
    share = float((d[0] < d[1]).mean())
    print(f"share of perm[0] < perm[1]: {share:.4f}")
    assert abs(share - 0.5) <= 0.04


def test_known_answer():
    """(n, seed, draw) = (1025, 42, 7): pins the definition (rounds, widths, Philox's counter and key words)."""
    perm, _ = reference()
    assert perm(1025, 42, 7)[:16].tolist() == [766, 521, 308, 407, 365, 231, 953, 712, 423, 888, 672, 718, 313, 884, 118, 958]


def test_reference_refuses():
    perm, positions = reference()
    for n in (0, -1, 2 ** 31):
        with pytest.raises(ValueError):
            perm(n, 0, 0)
    for draw in (-1, 2 ** 64):
        with pytest.raises(ValueError):
            perm(8, 0, draw)
    with pytest.raises(ValueError):
        positions(np.array([8]), 8, 0, 0)


def test_header_advertises_the_calls():
    native, lib = _lib()
    src = header()
    assert re.search(r"#define SPL_PPO_PERMUTE 1\b", src) and native.PPO_PERMUTE == 1
    assert re.search(r"#define SPL_PPO_ABI 1\b", src) and lib.spl_abi_version() == 9  # additive: neither moved
    assert re.search(r"int spl_ppo_permute\(const spl_ppo_permute_t \*args, void \*stream\);", src)
    assert re.search(r"int spl_ppo_loss_dev\(int32_t B, const spl_ppo_loss_t \*args, const float \*coef, void \*stream\);", src)
    # nothing already in the header moved: the new block comes behind the last earlier declaration
    assert src.index("#define SPL_PPO_PERMUTE") > src.index("int spl_ppo_net_backward_bf16(")
    assert native.has_permute(lib)
    for name in native.OPTIONAL_PERMUTE:
        assert hasattr(lib, name) and name in native.SIGNATURES
    assert not native.has_permute(types.SimpleNamespace(spl_ppo_permute=1))  # both, as has_net_bf16


def test_struct_layouts_against_the_header():
    native, _ = _lib()
    src = header()
    S, A = native.PpoPermState, native.PpoPermute
    assert re.search(r"typedef struct \{ uint64_t seed, draw; \} spl_ppo_perm_state_t;", src)
    assert [f[0] for f in S._fields_] == ["seed", "draw"]
    assert ctypes.sizeof(S) == 16 and (S.seed.offset, S.draw.offset) == (0, 8)
    assert header_fields(src, "spl_ppo_permute_t") == [f[0] for f in A._fields_]
    assert ctypes.sizeof(A) == 32
    assert (A.n.offset, A.B.offset, A.reserved.offset, A.state.offset, A.out.offset) == (0, 8, 12, 16, 24)
    assert ctypes.sizeof(native.PpoLoss) == 4 * 4 + 10 * 8 + 4 * 4 + 5 * 8  # spl_ppo_loss_dev takes it unchanged


def test_permute_refusals_on_the_host():
    """Every argument error is returned before anything is launched (the pointers are never dereferenced)."""
    native, lib = _lib()
    E_ARG, E_RANGE = -1, -3
    good = dict(n=100, B=7, reserved=0, state=0x1000, out=0x2000)
    cases = [("n = 0", dict(n=0), E_RANGE, "n must"), ("n < 0", dict(n=-5), E_RANGE, "n must"),
             ("n = 2^31", dict(n=2 ** 31), E_RANGE, "n must"), ("B = 0", dict(B=0), E_RANGE, "B must"),
             ("B < 0", dict(B=-1), E_RANGE, "B must"), ("B > n", dict(B=101), E_RANGE, "B must"),
             ("reserved", dict(reserved=1), E_ARG, "reserved"), ("null state", dict(state=None), E_ARG, "null"),
             ("null out", dict(out=None), E_ARG, "null"), ("state misaligned", dict(state=0x1004), E_ARG, "8-byte"),
             ("out misaligned", dict(out=0x2008), E_ARG, "16-byte")]
    for label, change, code, word in cases:
        got = lib.spl_ppo_permute(ctypes.byref(native.PpoPermute(**{**good, **change})), None)
        assert got == code, (label, got)
        _refused(lib, got, word)
    _refused(lib, lib.spl_ppo_permute(None, None), "null")


def test_loss_dev_refusals_on_the_host():
    """spl_ppo_loss's refusals, and the coefficient block's own; the struct's four fields are not looked at."""
    native, lib = _lib()
    fields = ("idx", "mask_bits", "action", "logprob", "value", "adv", "ret", "stats", "logits", "new_value", "dlogits",
              "dvalue", "out", "errors", "scratch")
    good = dict(K=2, T=3, normalize=1, reserved=0, **{k: 0x1000 * (i + 1) for i, k in enumerate(fields)},
                clip_coef=-1.0, vclip=float("nan"), vf_coef=-2.0, ent_coef=float("nan"))
    call = lambda B, coef, **change: lib.spl_ppo_loss_dev(B, ctypes.byref(native.PpoLoss(**{**good, **change})), coef, None)
    _refused(lib, call(0, 0x100), "B must")
    _refused(lib, call(4, None), "null")
    _refused(lib, call(4, 0x108), "16-byte")
    _refused(lib, call(4, 0x100, K=0), "K and T")
    _refused(lib, call(4, 0x100, logits=None), "null")
    _refused(lib, call(4, 0x100, out=0x1004), "8-byte")
    _refused(lib, lib.spl_ppo_loss_dev(4, None, 0x100, None), "null")
    # the argument-block entry still refuses what it refused
    _refused(lib, lib.spl_ppo_loss(4, ctypes.byref(native.PpoLoss(**good)), None), "NaN")


def test_graph_update_names_what_is_missing():
    """ppo_update(graph=True) without a DeviceAdam, without a DeviceNets or without a DevicePermutation: a
    ValueError that names it, raised before the store or a device is touched."""
    import torch
    from splendor_gym import ppo
    from splendor_gym.policy import ActorCritic
    agent = ActorCritic()
    store = types.SimpleNamespace(torch=torch, num_steps=4, num_envs=8, device=torch.device("cpu"))
    adam, nets = object.__new__(ppo.DeviceAdam), object.__new__(ppo.DeviceNets)
    perm = object.__new__(ppo.DevicePermutation)
    perm.total, perm.batch_size, perm.rows, perm.device = 32, 1, 32, store.device
    with pytest.raises(ValueError, match="DeviceAdam"):
        ppo.ppo_update(agent, torch.optim.Adam(agent.parameters()), store, device_nets=nets, permutation=perm, graph=True)
    for missing in (False, True, None):
        with pytest.raises(ValueError, match="DeviceNets"):
            ppo.ppo_update(agent, adam, store, device_nets=missing, permutation=perm, graph=True)
    with pytest.raises(ValueError, match="DevicePermutation"):
        ppo.ppo_update(agent, adam, store, device_nets=nets, graph=True)
    # a permutation for another shape, with or without the graph
    with pytest.raises(ValueError, match="32 positions in minibatches of 1"):
        ppo.ppo_update(agent, adam, store, device_nets=nets, permutation=perm, minibatch_size=2, graph=True)
    with pytest.raises(ValueError, match="DevicePermutation or None"):
        ppo.ppo_update(agent, torch.optim.Adam(agent.parameters()), store, permutation=torch.arange(32))
    # 4 epochs x 32 minibatches fit; 33 epochs x 32 do not
    assert ppo.GRAPH_MAX_MINIBATCHES == 1024
    with pytest.raises(ValueError, match="GRAPH_MAX_MINIBATCHES"):
        ppo.ppo_update(agent, adam, store, device_nets=nets, permutation=perm, minibatch_size=1, update_epochs=33, graph=True)


def test_cli_has_the_switches():
    from splendor_gym.scripts import ppo_device
    with pytest.raises(SystemExit):
        ppo_device.main(["--graph-update", "--device-permutation", "--help"])

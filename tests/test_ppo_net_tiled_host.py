"""The tiled PPO network passes without a GPU (spl_ppo_net_forward_tiled / spl_ppo_net_backward_tiled,
include/splendor_ppo.h): the header's macros, the exported symbols, the host-side refusals, which are those of
spl_ppo_net_forward / spl_ppo_net_backward with the same error codes, and DeviceNets' `tiled` switch."""
import os
import re

import pytest

from test_ppo_adam_host import P, _lib
from test_ppo_net_host import FIELDS, bwd_args, fwd_args


def header():
    return open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "splendor_ppo.h")).read()


def test_header_advertises_the_tiled_calls():
    native, lib = _lib()
    src = header()
    assert re.search(r"#define SPL_PPO_NET_TILED 1\b", src) and native.PPO_NET_TILED == 1
    assert re.search(rf"#define SPL_PPO_NET_TILE_ROWS {native.PPO_NET_TILE_ROWS}\b", src)
    assert native.PPO_NET_TILE_ROWS >= 32 and native.PPO_NET_BWD_ROWS % 32 == 0
    assert re.search(r"#define SPL_PPO_ABI 1\b", src) and lib.spl_abi_version() == 9  # additive: neither moved
    for name, block in (("spl_ppo_net_forward_tiled", "spl_ppo_net_fwd_t"), ("spl_ppo_net_backward_tiled", "spl_ppo_net_bwd_t")):
        assert re.search(rf"int {name}\(int32_t B, const {block} \*args, void \*stream\);", src), name
    # nothing already in the header moved: the new block comes behind the last earlier declaration
    assert src.index("SPL_PPO_NET_TILED") > src.index("int spl_ppo_net_backward(")


def test_library_exports_both_symbols():
    native, lib = _lib()
    assert native.has_net_tiled(lib)
    for name in native.OPTIONAL:
        assert hasattr(lib, name) and name in native.SIGNATURES
    assert native.SIGNATURES["spl_ppo_net_forward_tiled"] == native.SIGNATURES["spl_ppo_net_forward"]
    assert native.SIGNATURES["spl_ppo_net_backward_tiled"] == native.SIGNATURES["spl_ppo_net_backward"]


def cases(native, which):
    """(label, B, args) of every refusal the issue lists: B = 0, B = MAX_ROWS + 1, each null pointer, a misaligned
    pointer of each kind, reserved = 1, K = 0 (and T = 0)."""
    args = fwd_args if which == "forward" else bwd_args
    yield "B = 0", 0, args(native)
    yield "B = MAX_ROWS + 1", native.PPO_NET_MAX_ROWS + 1, args(native)
    yield "null block", 8, None
    yield "reserved", 8, args(native, reserved=1)
    yield "K = 0", 8, args(native, K=0)
    yield "T = 0", 8, args(native, T=0)
    plain = ("idx", "obs_u8", "act") + (("logits", "new_value", "errors") if which == "forward" else ("dlogits", "dvalue", "scratch"))
    for name in plain:
        yield f"{name} null", 8, args(native, **{name: None})
        yield f"{name} misaligned", 8, args(native, **{name: P + 4})
    for block in ("actor", "critic") + (() if which == "forward" else ("actor_grad", "critic_grad")):
        for f in FIELDS:
            yield f"{block}.{f} null", 8, args(native, **{block: {f: None}})
            yield f"{block}.{f} misaligned", 8, args(native, **{block: {f: P + 8}})


@pytest.mark.parametrize("which", ["forward", "backward"])
def test_the_same_refusals_as_the_existing_calls(which):
    """Every argument error is returned on the host, with the existing call's code and message: nothing here is
    a device address, so a launch would fault."""
    native, lib = _lib()
    old, new = ((lib.spl_ppo_net_forward, lib.spl_ppo_net_forward_tiled) if which == "forward" else
                (lib.spl_ppo_net_backward, lib.spl_ppo_net_backward_tiled))
    n = 0
    for label, B, args in cases(native, which):
        want = old(B, args, None)
        want_text = lib.spl_last_error()
        got = new(B, args, None)
        assert want < 0 and got == want and lib.spl_last_error() == want_text and want_text, label
        n += 1
    assert n >= 6 + 12 + 24
    assert new(native.PPO_NET_MAX_ROWS + 1, (fwd_args if which == "forward" else bwd_args)(native), None) == -3  # SPL_E_RANGE


def test_device_nets_takes_three_values_of_tiled():
    import inspect
    from splendor_gym.policy import ActorCritic
    from splendor_gym.ppo import DeviceNets
    assert inspect.signature(DeviceNets.__init__).parameters["tiled"].default is False
    assert DeviceNets.TILE_ROWS == _lib()[0].PPO_NET_TILE_ROWS
    for bad in (None, 1, 0, "on", "AUTO", 4096):
        with pytest.raises(ValueError, match="tiled"):
            DeviceNets(ActorCritic(), tiled=bad)
    for good in (False, True, "auto"):  # accepted; what then fails is the missing GPU or the CPU parameters
        with pytest.raises((RuntimeError, ValueError)) as e:
            DeviceNets(ActorCritic(), tiled=good)
        assert "tiled must be" not in str(e.value)


def test_cli_has_the_switch():
    from splendor_gym.scripts import ppo_device
    with pytest.raises(SystemExit):
        ppo_device.main(["--tiled-nets", "sometimes"])

"""The PPO network passes without a GPU (spl_ppo_net_forward / spl_ppo_net_backward, include/splendor_ppo.h):
the numpy float64 oracle the GPU tests compare against, pinned to torch.autograd on a float64 ActorCritic on
the CPU; the struct layouts and constants against the header; every host-side refusal of the entry points;
and DeviceNets' refusals that need no device."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_ppo_adam_host import P, _lib, _refused, header_fields

NA, IN, H, ROW = 45, 297, 256, 300
NETS = ("actor", "critic")
FIELDS = ("w1", "b1", "w2", "b2", "w3", "b3")


def expand(rows):
    """uint8 [B, 300] compact rows -> float64 [B, 297]: column 295 = byte 295 + 256 * byte 297, else the byte
    (spl_ppo_gather's expansion)."""
    x = rows[:, :IN].astype(np.float64)
    x[:, 295] += 256.0 * rows[:, 297]
    return x


def net_oracle(params, obs_u8_rows, dlogits, dvalue, bad=None):
    """Forward and backward of both networks in float64.  params: {"actor": [w1, b1, w2, b2, w3, b3], "critic":
    [...]} in torch's nn.Linear layout; obs_u8_rows uint8 [B, 300]; dlogits [B, 45]; dvalue [B]; bad: bool [B],
    rows whose outputs are zeros and which add nothing to any gradient.  Returns logits [B, 45], value [B]
    and grads in params' layout."""
    B = len(obs_u8_rows)
    bad = np.zeros(B, dtype=bool) if bad is None else np.asarray(bad, dtype=bool)
    x = expand(obs_u8_rows)
    x[bad] = 0.0
    out = {"grads": {}}
    for net, d_out in (("actor", np.asarray(dlogits, dtype=np.float64).reshape(B, NA)),
                       ("critic", np.asarray(dvalue, dtype=np.float64).reshape(B, 1))):
        w1, b1, w2, b2, w3, b3 = (np.asarray(p, dtype=np.float64) for p in params[net])
        h1 = np.tanh(x @ w1.T + b1)
        h2 = np.tanh(h1 @ w2.T + b2)
        y = h2 @ w3.T + b3
        y[bad] = 0.0
        d = d_out.copy()
        d[bad] = 0.0
        dz2 = (d @ w3) * (1.0 - h2 * h2)
        dz1 = (dz2 @ w2) * (1.0 - h1 * h1)
        out["grads"][net] = [dz1.T @ x, dz1.sum(0), dz2.T @ h1, dz2.sum(0), d.T @ h2, d.sum(0)]
        out["logits" if net == "actor" else "value"] = y if net == "actor" else y[:, 0]
    return out


def params_of(agent):
    """{"actor": [...], "critic": [...]} float64 numpy copies of an ActorCritic's parameters."""
    return {net: [p.detach().double().cpu().numpy() for i in (0, 2, 4) for p in (getattr(agent, net)[i].weight,
                                                                                   getattr(agent, net)[i].bias)]
            for net in NETS}


def tensors_of(agent):
    """The twelve parameters in DeviceNets' order: the actor's six, then the critic's."""
    return [p for net in NETS for i in (0, 2, 4) for p in (getattr(agent, net)[i].weight, getattr(agent, net)[i].bias)]


def torch_passes(agent, x, dlogits, dvalue):
    """The same through torch.autograd on `agent` (any dtype, any device) from zeroed gradients: x [B, 297],
    dlogits [B, 45], dvalue [B].  float64 numpy results in net_oracle's layout."""
    import torch
    for p in agent.parameters():
        p.grad = None
    logits, value = agent.actor(x), agent.critic(x)
    torch.autograd.backward([logits, value], [dlogits, dvalue.view(-1, 1)])
    grads = {net: [p.grad.double().cpu().numpy() for i in (0, 2, 4) for p in (getattr(agent, net)[i].weight,
                                                                               getattr(agent, net)[i].bias)]
             for net in NETS}
    return {"logits": logits.detach().double().cpu().numpy(), "value": value.detach().double().cpu().numpy()[:, 0],
            "grads": grads}


def quantities(res, B):
    """(name, array) of everything a comparison looks at: the outputs and B * each gradient."""
    yield "logits", res["logits"]
    yield "value", res["value"]
    for net in NETS:
        for field, g in zip(FIELDS, res["grads"][net]):
            yield f"{net}.{field}", B * g


def make_rows(rng, B, big_moves=(0,)):
    """Observation-like compact rows: small counts, bytes 298-299 zero, byte 297 nonzero on rows big_moves."""
    rows = rng.integers(0, 8, size=(B, ROW)).astype(np.uint8)
    rows[:, 295] = rng.integers(0, 256, size=B)
    rows[:, 297:] = 0
    for r in big_moves:
        if r < B:
            rows[r, 297] = 1 + r % 3
    return rows


@pytest.mark.parametrize("B", [1, 3, 65])
def test_oracle_equals_torch_autograd_in_float64(B):
    """1e-11 x the largest magnitude of each quantity: both sides are float64 sums of at most 297 + 256 + 45
    terms."""
    import torch
    from splendor_gym.policy import ActorCritic
    torch.manual_seed(B)
    agent = ActorCritic().double()
    rng = np.random.default_rng(B)
    rows = make_rows(rng, B, big_moves=(0, 2))
    assert rows[0, 297] != 0
    dlogits, dvalue = rng.normal(size=(B, NA)) / B, rng.normal(size=B) / B
    want = torch_passes(agent, torch.from_numpy(expand(rows)), torch.from_numpy(dlogits), torch.from_numpy(dvalue))
    got = net_oracle(params_of(agent), rows, dlogits, dvalue)
    for (name, a), (_, b) in zip(quantities(got, B), quantities(want, B)):
        err, scale = float(np.abs(a - b).max()), float(np.abs(b).max())
        print(f"oracle against torch float64 B={B} {name}: {err:.3e} of {scale:.3e}")
        assert a.shape == b.shape and err <= 1e-11 * scale, name
    # column 295 is rebuilt from two bytes
    cleared = rows.copy()
    cleared[:, 297] = 0
    assert not np.array_equal(net_oracle(params_of(agent), cleared, dlogits, dvalue)["logits"][0], got["logits"][0])


def test_oracle_bad_rows_are_left_out():
    import torch
    from splendor_gym.policy import ActorCritic
    torch.manual_seed(7)
    agent = ActorCritic().double()
    rng = np.random.default_rng(7)
    B = 9
    rows = make_rows(rng, B)
    dlogits, dvalue = rng.normal(size=(B, NA)), rng.normal(size=B)
    bad = np.zeros(B, dtype=bool)
    bad[[2, 8]] = True
    got = net_oracle(params_of(agent), rows, dlogits, dvalue, bad=bad)
    kept = net_oracle(params_of(agent), rows[~bad], dlogits[~bad], dvalue[~bad])
    assert not got["logits"][bad].any() and not got["value"][bad].any()
    # the same rows in a smaller batch: the matrix products may sum in another order
    assert np.abs(got["logits"][~bad] - kept["logits"]).max() <= 1e-12 and np.abs(got["value"][~bad] - kept["value"]).max() <= 1e-12
    for net in NETS:
        for a, b in zip(got["grads"][net], kept["grads"][net]):
            assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max())


# --------------------------------------------------------------------------------------------
def test_struct_layouts_and_constants_against_the_header():
    native, lib = _lib()
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "splendor_ppo.h")).read()
    assert re.search(r"#define SPL_PPO_ABI 1\b", src) and lib.spl_abi_version() == 9  # additive: neither moved
    for macro, value in (("SPL_PPO_NET", 1), ("SPL_PPO_NET_MAX_ROWS", native.PPO_NET_MAX_ROWS),
                         ("SPL_PPO_NET_HIDDEN", native.PPO_NET_HIDDEN), ("SPL_PPO_NET_FWD_ROWS", native.PPO_NET_FWD_ROWS),
                         ("SPL_PPO_NET_BWD_ROWS", native.PPO_NET_BWD_ROWS), ("SPL_PPO_NET_BWD_PARTS", native.PPO_NET_BWD_PARTS)):
        assert re.search(rf"#define {macro} {value}\b", src), macro
    assert native.PPO_NET_MAX_ROWS == 65536
    M, F, Bw = native.PpoMlp, native.PpoNetFwd, native.PpoNetBwd
    assert header_fields(src, "spl_ppo_mlp_t") == header_fields(src, "spl_ppo_mlp_grad_t") == [f[0] for f in M._fields_]
    assert header_fields(src, "spl_ppo_net_fwd_t") == [f[0] for f in F._fields_]
    assert header_fields(src, "spl_ppo_net_bwd_t") == [f[0] for f in Bw._fields_]
    assert ctypes.sizeof(M) == 48 and ctypes.sizeof(F) == 160 and ctypes.sizeof(Bw) == 256
    assert {k: getattr(F, k).offset for k in ("K", "T", "reserved", "idx", "obs_u8", "actor", "critic", "logits", "new_value",
                                              "act", "errors")} == \
        {"K": 0, "T": 4, "reserved": 8, "idx": 16, "obs_u8": 24, "actor": 32, "critic": 80, "logits": 128, "new_value": 136,
         "act": 144, "errors": 152}
    assert {k: getattr(Bw, k).offset for k in ("idx", "obs_u8", "actor", "critic", "dlogits", "dvalue", "act", "actor_grad",
                                               "critic_grad", "scratch")} == \
        {"idx": 16, "obs_u8": 24, "actor": 32, "critic": 80, "dlogits": 128, "dvalue": 136, "act": 144, "actor_grad": 152,
         "critic_grad": 200, "scratch": 248}


def test_buffer_sizes():
    native, lib = _lib()
    S, parts = native.PPO_NET_BWD_ROWS, native.PPO_NET_BWD_PARTS
    grads = 2 * (H * IN + H + H * H + H) + (NA + 1) * (H + 1)  # every parameter once: 295 982
    assert grads == 295982
    for B in (1, S, S + 1, 256, parts * S, parts * S + 1, native.PPO_NET_MAX_ROWS):
        assert lib.spl_ppo_net_act_bytes(B) == 2 * 2 * B * H * 4, B
        n_parts = min((B + S - 1) // S, parts)
        assert lib.spl_ppo_net_scratch_bytes(B) == (2 * 2 * B * H + n_parts * ((grads + 3) // 4 * 4)) * 4, B
    for fn in (lib.spl_ppo_net_act_bytes, lib.spl_ppo_net_scratch_bytes):
        for B in (0, -1):
            assert fn(B) == -1 and b"positive" in lib.spl_last_error()
        assert fn(native.PPO_NET_MAX_ROWS + 1) == -3 and b"65536" in lib.spl_last_error()  # SPL_E_RANGE


def fwd_args(native, **kw):
    mlp = lambda **m: native.PpoMlp(**{**{f: P for f in FIELDS}, **m})
    a = native.PpoNetFwd(K=3, T=70, reserved=0, idx=P, obs_u8=P, actor=mlp(**kw.pop("actor", {})),
                         critic=mlp(**kw.pop("critic", {})), logits=P, new_value=P, act=P, errors=P)
    for k, v in kw.items():
        setattr(a, k, v)
    return ctypes.byref(a)


def bwd_args(native, **kw):
    mlp = lambda **m: native.PpoMlp(**{**{f: P for f in FIELDS}, **m})
    a = native.PpoNetBwd(K=3, T=70, reserved=0, idx=P, obs_u8=P, actor=mlp(**kw.pop("actor", {})),
                         critic=mlp(**kw.pop("critic", {})), dlogits=P, dvalue=P, act=P,
                         actor_grad=mlp(**kw.pop("actor_grad", {})), critic_grad=mlp(**kw.pop("critic_grad", {})), scratch=P)
    for k, v in kw.items():
        setattr(a, k, v)
    return ctypes.byref(a)


@pytest.mark.parametrize("which", ["forward", "backward"])
def test_refusals(which):
    """Every argument error is returned on the host: nothing here is a device address, so a launch would
    fault."""
    native, lib = _lib()
    fn, args = (lib.spl_ppo_net_forward, fwd_args) if which == "forward" else (lib.spl_ppo_net_backward, bwd_args)
    for B in (0, -5):
        _refused(lib, fn(B, args(native), None), "positive")
    code = fn(native.PPO_NET_MAX_ROWS + 1, args(native), None)
    assert code == -3  # SPL_E_RANGE
    _refused(lib, code, "SPL_PPO_NET_MAX_ROWS")
    _refused(lib, fn(8, None, None), "null")
    _refused(lib, fn(8, args(native, reserved=1), None), "reserved")
    for k in ("K", "T"):
        _refused(lib, fn(8, args(native, **{k: 0}), None), "K and T")
    plain = ("idx", "obs_u8", "act") + (("logits", "new_value", "errors") if which == "forward" else ("dlogits", "dvalue", "scratch"))
    for name in plain:
        _refused(lib, fn(8, args(native, **{name: None}), None), "null")
        for off in (1, 4, 8):
            _refused(lib, fn(8, args(native, **{name: P + off}), None), "16-byte aligned")
    blocks = ("actor", "critic") + (() if which == "forward" else ("actor_grad", "critic_grad"))
    for block in blocks:
        for f in FIELDS:
            _refused(lib, fn(8, args(native, **{block: {f: None}}), None), "null")
            _refused(lib, fn(8, args(native, **{block: {f: P + 4}}), None), "16-byte aligned")


# --------------------------------------------------------------------------------------------
def test_device_nets_refusals_that_need_no_device():
    import torch
    from splendor_gym.policy import ActorCritic
    from splendor_gym.ppo import DeviceNets
    with pytest.raises(ValueError, match="float32"):
        DeviceNets(ActorCritic().double())
    skewed = ActorCritic()
    skewed.critic[2].weight = torch.nn.Parameter(torch.randn(H, H).t())
    assert not skewed.critic[2].weight.is_contiguous()
    with pytest.raises(ValueError, match="not contiguous"):
        DeviceNets(skewed)
    with pytest.raises(ValueError, match=r"actor\.w1"):
        DeviceNets(ActorCritic(obs_dim=296))
    with pytest.raises(ValueError, match=r"actor\.w3"):
        DeviceNets(ActorCritic(act_dim=44))
    with pytest.raises(ValueError, match="Sequential"):
        DeviceNets(torch.nn.Linear(3, 3))


def test_device_nets_needs_a_gpu_or_refuses():
    """No CPU fallback: without a GPU the constructor raises; with one it refuses CPU parameters."""
    from splendor_gym.policy import ActorCritic
    from splendor_gym.ppo import DeviceNets
    with pytest.raises((RuntimeError, ValueError)):
        DeviceNets(ActorCritic())


def test_ppo_update_has_the_switch():
    import inspect
    from splendor_gym.ppo import ppo_update
    assert inspect.signature(ppo_update).parameters["device_nets"].default is False
